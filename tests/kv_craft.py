"""Hand-made KV rows for the attention tests (tests/test_attention_crafted_cpu.py, tests/test_gpu_attention_crafted.py).

lnb_ctx_load_prefix writes arbitrary rows [0, n_pos) of every layer into a device context and the oracle's Context.cache(layer, which) is a
writable view of its own cache, so the same crafted K / V rows go into both; one call at position n_pos then meets data no synthetic-weight
model produces: scores spread over a hundred nats, f32-denormal probabilities that reach the output, e = exp(score) near 1e300, one
overflowing score, ties, signed zeros, and (device only) NaN rows beyond T that no kernel may read.

Everything here is numpy: the blob layout is include/lnb.h's ("LNBKV1"), K as [kv head][hd/8][n_pos][8], V as [n_pos][kv_dim].

How a case reaches a score: K_j = a_j * q / (q . q) for the FIRST query head of each KV head (q = the oracle's xq_rope of the call, which in a
one-layer model does not depend on the cache), so that head's raw score is ~a_j and its divided score ~a_j / sqrt(head_dim).  bf16 truncation
of K shrinks |score| by up to ~0.5 %; the targets below keep that much room.  The other query heads of the KV head get whatever q_other . K_j
gives: generic scores.  A case's CONDITION is therefore counted on the aligned heads only (aligned_heads())."""
import struct

import numpy as np

from oracle import oracle as orc

TOKEN = 5                                   # the token of the one-row call at position n_pos = T - 1
TAIL = 64                                   # poison_beyond: rows [T, T + TAIL) of 0x7FC0 on the device side
QNAN = 0x7FC0
CAPACITY = 640                              # >= 513 + TAIL
TS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513)

_L1 = dict(orc.TINY, n_layers=1)
GEOMETRIES = {
    "hd64": dict(_L1),                                               # 4 query heads on 2 KV heads
    "hd128": dict(_L1, n_heads=2, n_kv_heads=1),
    "h8kv2_hd128": dict(_L1, dim=1024, n_heads=8, n_kv_heads=2),
    "hd32": dict(_L1, n_heads=8, n_kv_heads=2),                      # never takes the matrix cores
    "hd64_two_layers": dict(orc.TINY),                               # layer 1 gets generic gaussian rows: the blob's per-layer plumbing
}
SEED_MODEL = 1234


def bf(a):
    return orc.f32_to_bf16(np.asarray(a, dtype=np.float32))


def wide(a):
    return orc.bf16_to_f32(a).reshape(np.shape(a))


def head_dim(cfg):
    return cfg["dim"] // cfg["n_heads"]


def aligned_heads(cfg):
    """the query heads whose scores the crafted K rows control: the first of each KV head's group"""
    rep = cfg["n_heads"] // cfg["n_kv_heads"]
    return [k * rep for k in range(cfg["n_kv_heads"])]


# ---- the blob -------------------------------------------------------------------------------------------------------------------------------
def blob(K, V):
    """LNBKV1 blob of a whole model (every layer cached): K, V = per-layer lists of uint16 [n_pos, n_kv_heads, head_dim]"""
    n_layers = len(K)
    n_pos, kvh, hd = K[0].shape
    head = b"LNBKV1\0\0" + struct.pack("<7I", 1, n_pos, 0, 3 * n_layers, kvh, hd, n_layers) + bytes(28)
    parts = [np.frombuffer(head, dtype=np.uint8)]
    for k, v in zip(K, V):
        k = np.ascontiguousarray(k, dtype=np.uint16); v = np.ascontiguousarray(v, dtype=np.uint16)
        assert k.shape == v.shape == (n_pos, kvh, hd)
        parts.append(np.ascontiguousarray(k.reshape(n_pos, kvh, hd // 8, 8).transpose(1, 2, 0, 3)).view(np.uint8).ravel())
        parts.append(v.view(np.uint8).ravel())
    return np.concatenate(parts)


def inject(oracle_ctx, gpu_ctx, K, V, poison_beyond=False):
    """the rows [0, n_pos) of every layer into both contexts (either may be None); poison_beyond: the device context also gets rows
    [n_pos, n_pos + 1 + TAIL) of 0x7FC0 -- the call at n_pos overwrites row n_pos, [T, T + TAIL) stay NaN.  The oracle never reads past T."""
    n_pos = K[0].shape[0]
    if oracle_ctx is not None:
        for l, (k, v) in enumerate(zip(K, V)):
            oracle_ctx.cache(l, 0)[:n_pos] = k
            oracle_ctx.cache(l, 1)[:n_pos] = v
    if gpu_ctx is not None:
        if poison_beyond:
            tail = np.full((1 + TAIL,) + K[0].shape[1:], QNAN, dtype=np.uint16)
            K = [np.concatenate([k, tail]) for k in K]; V = [np.concatenate([v, tail]) for v in V]
        if K[0].shape[0]:
            assert gpu_ctx.LoadPrefix(blob(K, V)) == K[0].shape[0]
    return n_pos


# ---- queries and aligned K rows -----------------------------------------------------------------------------------------------------------------
def query(om, token, pos, layer=0):
    """(xq_rope [n_heads, head_dim] f32, the divided score [n_heads] of the call's own row) of `token` at `pos` in `layer`, from a dry oracle
    run on an empty context"""
    oc = orc.Context(om, pos + 1)
    dumps = oc.capture()
    oc.forward([token], pos, want_logits=False)
    q = wide(dumps[("xq_rope", layer)][0])
    own = wide(dumps[("scores", layer)][:, 0, pos])
    oc.close()
    return q, own


def aligned_k(cfg, q, a):
    """K rows uint16 [len(a), n_kv_heads, head_dim]: row j of KV head k is a[j] * q_h / (q_h . q_h), h the first query head of k; `a` is in units
    of the DIVIDED score (it is multiplied by sqrt(head_dim) here); a [n] for every KV head alike, or [n, n_kv_heads]"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = np.repeat(a[:, None], cfg["n_kv_heads"], axis=1)
    hd = head_dim(cfg)
    out = np.empty((a.shape[0], cfg["n_kv_heads"], hd), dtype=np.uint16)
    for k, h in enumerate(aligned_heads(cfg)):
        qh = q[h].astype(np.float64)
        out[:, k, :] = bf((a[:, k, None] * np.sqrt(hd)) * (qh / (qh @ qh))[None, :])
    return out


def gaussian_v(rng, cfg, n, scale=0.3):
    return bf(rng.standard_normal((n, cfg["n_kv_heads"], head_dim(cfg))) * scale)


def gaussian_rows(rng, cfg, n):
    """generic K and V rows (scores of a few units)"""
    return bf(rng.standard_normal((n, cfg["n_kv_heads"], head_dim(cfg))) * 0.5), gaussian_v(rng, cfg, n)


# ---- the case table: (rng, cfg, q, own, T) -> (K, V) of layer 0, uint16 [T - 1, n_kv_heads, head_dim] ---------------------------------------------------
# p = e / Z is an f32 denormal for ln p in (-103.3, -87.3); its bf16 truncation keeps a non-zero bit down to 2^-133, ln p > -91.2.
def case_spread(rng, cfg, q, own, T):
    n = T - 1
    a = np.linspace(-150.0, 25.0, n)
    if n < 64:                              # too few rows for the linspace to hit the 3.8-nat window below the top score: place three there
        a[1:4] = (25.0 - 88.2, 25.0 - 89.4, 25.0 - 90.6)
    return aligned_k(cfg, q, rng.permutation(a)), gaussian_v(rng, cfg, n)


def case_denormal_visible(rng, cfg, q, own, T):
    """one dominant row (K = 0: score exactly 0, V = 0) beside the call's own row; up to eight rows whose p is a bf16-visible f32 denormal carry
    V = +-2^118 .. 2^120; the rest (p -> 0) generic V"""
    n = T - 1
    own = np.asarray(own, dtype=np.float64)[aligned_heads(cfg)]
    ln_z = np.log(np.exp(own) + (1.0 if n >= 2 else 0.0))                # per aligned head: the call's own row (+ the dominant row, e = 1)
    a = np.full((n, cfg["n_kv_heads"]), -100.0) + ln_z
    V = gaussian_v(rng, cfg, n)
    order = rng.permutation(n)
    den = order[:min(8, max(1, n - 1))]
    a[den] = ln_z - 89.75 + 0.5 * rng.integers(0, 3, (den.size, 1))      # ln p in (-89.75, -88.3) with the 0.5 % the truncation of K takes
    V[den] = bf(rng.choice([-1.0, 1.0], (den.size,) + V.shape[1:]) * 2.0 ** rng.integers(118, 121, (den.size,) + V.shape[1:]))
    if n >= 2:
        dom = order[-1]
        a[dom] = 0.0
        V[dom] = 0
    return aligned_k(cfg, q, a), V


def case_huge_finite(rng, cfg, q, own, T):
    n = T - 1
    a = rng.uniform(600.0, 690.0, n)        # bf16 steps of 4 up there: 708 is the last score below exp's overflow at 709.78
    a[rng.integers(0, n)] = 690.0
    return aligned_k(cfg, q, a), gaussian_v(rng, cfg, n)


def case_one_inf(rng, cfg, q, own, T):
    n = T - 1
    a = rng.uniform(-3.0, 3.0, n)
    a[rng.integers(0, n)] = 760.0
    return aligned_k(cfg, q, a), gaussian_v(rng, cfg, n)


def case_ties(rng, cfg, q, own, T):
    """blocks of eight identical K rows with different V rows; in every second block the V rows are identical too"""
    n = T - 1
    a = np.repeat(rng.uniform(-3.0, 3.0, n // 8 + 1), 8)[:n]
    V = gaussian_v(rng, cfg, n)
    for b in range(1, (n + 7) // 8, 2):
        V[8 * b:8 * b + 8] = V[8 * b]
    return aligned_k(cfg, q, a), V


def case_signed_zero_v(rng, cfg, q, own, T):
    """first half: V of +-0 only; second half: -0 mixed with tiny values (bf16 denormals and 1e-30 .. 1e-36)"""
    n = T - 1
    K, _ = gaussian_rows(rng, cfg, n)
    shape = K.shape
    V = rng.choice(np.array([0x0000, 0x8000], dtype=np.uint16), shape)
    half = n // 2
    tiny = np.where(rng.random(shape) < 0.5, rng.integers(1, 0x80, shape).astype(np.uint16) | rng.choice(np.array([0, 0x8000], dtype=np.uint16), shape),
                    bf(rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-36, -30, shape)))
    V[half:] = np.where(rng.random(shape) < 0.5, np.uint16(0x8000), tiny)[half:]
    return K, V


def case_minus_masked_tail(rng, cfg, q, own, T):
    return gaussian_rows(rng, cfg, T - 1)


# ---- the PV chain on columns that reveal a wrong order of its adds (tests/order_craft.py) ------------------------------------------------------------------
PV_E_TOP, PV_WINDOWS = 118, 40              # a ladder's first opener 2^118, its last (window 39) 2^40 with v = 1.5 * 2^14: beside p ~ 2^-10 still far above the call's own term
PV_ZS = (20, 60)                            # the zero-sum columns' binades


def pv_windows(n, hd):
    """windows per ladder: PV_WINDOWS, more when the columns of a head would not hold the ladders of n positions (three offsets each) beside a head column and eight zero-sum ones"""
    per = max((hd - 9) // 3, 1)
    return max(PV_WINDOWS, -(-(n // 3) // per))


def pv_kinds(n, hd):
    """the construction of every V column of a KV head over n cached positions: ("ladder", offset, ladder), ("head",), then zero-sum columns"""
    w = pv_windows(n, hd)
    kinds = [("ladder", o, l) for l in range(-(-(n // 3) // w)) for o in range(3)] if n >= 3 else []
    kinds += [("head",)] if n >= 8 else []
    assert len(kinds) <= hd - 8
    return kinds + ["zero_sum"] * (hd - len(kinds))


def case_v_order(rng, cfg, q, own, T):
    """K rows of +0: every cached position has the score 0, e = 1 and the same p, whatever the head; the V columns are ladders, a head column and zero-sum columns
    over the cached positions (tests/order_craft.py), so p * V -- a product of two bf16 values, exact -- keeps each construction: a ladder column sums to exactly
    +0 and the output is the call's own term alone, any other order of the adds leaves residue far above it.  QK^T itself is not covered: the query cannot be
    injected and its dot runs over 64 or 128 terms."""
    import order_craft as od
    n, kvh, hd = T - 1, cfg["n_kv_heads"], head_dim(cfg)
    K = np.zeros((n, kvh, hd), dtype=np.uint16)
    V = np.zeros((n, kvh, hd), dtype=np.float32)
    kinds, w = pv_kinds(n, hd), pv_windows(n, hd)
    for k in range(kvh):
        for d in rng.permutation(hd):
            kd = kinds[d]
            V[:, k, d] = (od.zero_sum_products(rng, n, *PV_ZS) if kd == "zero_sum" else od.head_products(rng, n, PV_E_TOP) if kd == ("head",)
                          else od.ladder_products(rng, n, kd[1], kd[2], PV_E_TOP, w))
    Vb = bf(V)
    assert np.array_equal(wide(Vb), V)
    return K, Vb


CASES = {
    "spread": case_spread,
    "denormal_visible": case_denormal_visible,
    "huge_finite": case_huge_finite,
    "one_inf": case_one_inf,
    "ties": case_ties,
    "signed_zero_v": case_signed_zero_v,
    "minus_masked_tail": case_minus_masked_tail,
    "v_order": case_v_order,                # (sorts last: the other cases keep their seeds)
}
POISON_BEYOND = {"minus_masked_tail"}

# (case, T) left out because the case's condition cannot hold there.  T = 1: no crafted row at all (the two cases without a condition still
# run: the call's own row alone, with and without the NaN tail).  T = 2: one crafted row cannot give both a denormal and a zero p, nor 8 ties.
LEFT_OUT = {
    ("spread", 1), ("denormal_visible", 1), ("huge_finite", 1), ("one_inf", 1), ("ties", 1),
    ("spread", 2), ("ties", 2),
    ("v_order", 1), ("v_order", 2),           # no window of three fits
}
MAX_LEFT_OUT_FRACTION = 1.0 / 8.0


def grid():
    """every (case, T) the tests run"""
    return [(c, T) for c in CASES for T in TS if (c, T) not in LEFT_OUT]


def rows(case, geometry, T, om, q=None):
    """per-layer lists (K, V) of `case` at context length T for a model of GEOMETRIES[geometry]; deterministic per (case, geometry, T)"""
    cfg = GEOMETRIES[geometry]
    rng = np.random.default_rng([sorted(CASES).index(case), sorted(GEOMETRIES).index(geometry), T])
    if q is None:
        q = query(om, TOKEN, T - 1)
    k0, v0 = CASES[case](rng, cfg, q[0], q[1], T)
    K, V = [k0], [v0]
    for _ in range(1, cfg["n_layers"]):
        k, v = gaussian_rows(rng, cfg, T - 1)
        K.append(k); V.append(v)
    return K, V


# ---- the oracle's side of the grid, computed once per process and left unchanged ---------------------------------------------------------------------
_MODELS, _RUNS, _STEPS = {}, {}, {}


def oracle_model(geometry):
    if geometry not in _MODELS:
        _MODELS[geometry] = orc.Model(**GEOMETRIES[geometry]).fill_synthetic(SEED_MODEL).finalize()
    return _MODELS[geometry]


def oracle_run(case, geometry, T):
    """the oracle's one-row call (TOKEN at T - 1) after the crafted rows: dict of dumps, logits [1, V], am, kv (per layer (K, V), rows [0, T))"""
    key = (case, geometry, T)
    if key not in _RUNS:
        om = oracle_model(geometry)
        K, V = rows(case, geometry, T, om)
        oc = orc.Context(om, T)
        inject(oc, None, K, V)
        dumps = oc.capture()
        logits, am = oc.forward([TOKEN], T - 1)
        kv = [(oc.cache(l, 0).copy(), oc.cache(l, 1).copy()) for l in range(len(K))]
        oc.close()
        _RUNS[key] = dict(dumps=dumps, logits=logits, am=am, kv=kv, K=K, V=V)
    return _RUNS[key]


def step_tokens(geometry, n):
    """the tokens of an n-row continuation at n_pos: TOKEN (the row the crafted K rows are aligned with), then synthetic ones"""
    V = GEOMETRIES[geometry]["vocab_size"]
    return np.concatenate([[TOKEN], orc.synth_tokens(4242, n - 1, V)]).astype(np.int32)


def oracle_steps(case, geometry, n_pos, n):
    """n one-token oracle steps from n_pos after the crafted rows of (case, geometry, T = n_pos + 1): (logits [n, V], am [n], kv rows [0, n_pos + n))"""
    key = (case, geometry, n_pos, n)
    if key not in _STEPS:
        om = oracle_model(geometry)
        K, V = rows(case, geometry, n_pos + 1, om)
        oc = orc.Context(om, n_pos + n)
        inject(oc, None, K, V)
        toks = step_tokens(geometry, n)
        lg = np.empty((n, GEOMETRIES[geometry]["vocab_size"]), dtype=np.float32); am = np.empty(n, dtype=np.int64)
        for i in range(n):
            l1, a1 = oc.forward(toks[i:i + 1], n_pos + i)
            lg[i] = l1[0]; am[i] = a1
        kv = [(oc.cache(l, 0).copy(), oc.cache(l, 1).copy()) for l in range(len(K))]
        oc.close()
        _STEPS[key] = dict(logits=lg, am=am, kv=kv, K=K, V=V, toks=toks)
    return _STEPS[key]


def eq_or_both_nan_f32(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def eq_or_both_nan_bf16(a, b):
    a = np.ascontiguousarray(a, dtype=np.uint16); b = np.ascontiguousarray(b, dtype=np.uint16)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(wide(a)) & np.isnan(wide(b)))).all())
