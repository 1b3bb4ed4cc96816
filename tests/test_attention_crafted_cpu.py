"""The crafted-KV attention grid on the CPU oracle alone (no GPU): what tests/test_gpu_attention_crafted.py compares the device with.

1. every (case, geometry, T) of kv_craft's grid meets its case's condition on the oracle's own dumps (scores, softmax, attn_pre_wo), counted
   on the heads the crafted K rows are aligned with;
2. a short numpy restatement of attention_forward's per-row loop (oracle/lnb_oracle.c: same order, f64 serial sum) reproduces the oracle's
   softmax and attn_pre_wo dumps bit for bit (NaN for NaN), for the one-row grid and for the multi-row poison-token calls;
3. the restatement with ONE defect injected -- the mistakes a hand-scheduled kernel can make on such data -- changes the bits of a named case:
   the proof that the GPU comparison can fail.  One defect is the exception: a pairwise softmax denominator moves Z's last f64 bits and, over
   the whole grid, not one bf16 bit behind the two roundings (counted below); it is pinned on Z's own bits."""
import ctypes as C

import numpy as np
import pytest

import kv_craft as kc
from oracle import oracle as orc

F32_MIN_NORMAL = np.float32(2.0 ** -126)


def _eq_or_both_nan_bf16(a, b):
    a = np.ascontiguousarray(a, dtype=np.uint16); b = np.ascontiguousarray(b, dtype=np.uint16)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(kc.wide(a)) & np.isnan(kc.wide(b)))).all())


_EXP = []


def exp_table():
    """orc_exp(float64(bf16 s)) for all 65536 scores: the oracle's own exp, so the restatement does not depend on numpy's"""
    if not _EXP:
        L = orc.lib()
        x = kc.wide(np.arange(65536, dtype=np.uint32).astype(np.uint16)).astype(np.float64)
        _EXP.append(np.array([L.orc_exp_f64(C.c_double(v)) for v in x], dtype=np.float64))
    return _EXP[0]


def pairwise_sum(e):
    """sum over the last axis as a balanced tree (what a wave reduction computes) instead of the reference's serial chain"""
    while e.shape[-1] > 1:
        if e.shape[-1] & 1:
            e = np.concatenate([e, np.zeros(e.shape[:-1] + (1,), dtype=e.dtype)], axis=-1)
        e = e[..., 0::2] + e[..., 1::2]
    return e[..., 0]


DEFECTS = ("flush_denormal_p", "masked_e0_skip_beyond_diagonal", "padded_position", "pairwise_z")


def restate(cfg, q16, K16, V16, start_pos, defect=None, pad_v16=None, want_z=False):
    """attention_forward's loop over (head, row) of oracle/lnb_oracle.c in numpy, heads and rows vectorised, every chain in the oracle's order.
    q16 [S, H, hd], K16 / V16 [T, KVH, hd] (uint16, T = start_pos + S) -> (softmax uint16 [H, S, T], attn_pre_wo uint16 [S, H * hd])"""
    S, H, hd = q16.shape
    T = start_pos + S
    rep = H // cfg["n_kv_heads"]
    kvh = np.arange(H) // rep
    q = kc.wide(q16)
    K = kc.wide(K16)[:T, kvh, :]                             # [T, H, hd]
    V = kc.wide(V16)[:T, kvh, :]
    with np.errstate(all="ignore"):
        acc = np.zeros((S, H, T), dtype=np.float32)
        for d in range(hd):
            acc += q[:, :, None, d] * K[None, :, :, d].transpose(0, 2, 1)
        divisor = kc.wide(kc.bf(np.float32(np.sqrt(float(hd)))))
        s16 = kc.bf(kc.wide(kc.bf(acc)) / divisor)
        i = np.arange(S)[:, None, None]; j = np.arange(T)[None, None, :]
        dead = np.broadcast_to((S > 1) & ((j % S) - i >= 1), s16.shape)
        if S > 1:
            s16 = kc.bf(kc.wide(s16) + np.where(dead, np.float32(-np.inf), np.float32(0.0)))
        e = exp_table()[s16]
        if defect == "masked_e0_skip_beyond_diagonal":
            e = np.where(dead, 0.0, e)
        if defect == "pairwise_z":
            z = pairwise_sum(e)
        else:
            z = np.zeros((S, H), dtype=np.float64)
            for t in range(T):
                z = z + e[:, :, t]
        if want_z:
            return z
        p32 = (e / z[:, :, None]).astype(np.float32)
        if defect == "flush_denormal_p":
            p32 = np.where(np.abs(p32) < F32_MIN_NORMAL, np.float32(0.0), p32)
        p16 = kc.bf(p32)
        p = kc.wide(p16)
        out = np.zeros((S, H, hd), dtype=np.float32)
        for t in range(T):
            term = p[:, :, t, None] * V[None, t, :, :]
            if defect == "masked_e0_skip_beyond_diagonal":
                live = (t <= start_pos + np.arange(S))[:, None, None]
                out = np.where(live, out + term, out)
            else:
                out = out + term
        if defect == "padded_position":                         # one position past T multiplied in with p = +0: the clamped row T - 1, or what lies there
            pad = kc.wide(pad_v16)[kvh, :] if pad_v16 is not None else V[T - 1]
            out = out + np.float32(0.0) * pad[None, :, :]
    return p16.transpose(1, 0, 2), kc.bf(out).reshape(S, H * hd)


# ---- the one-row grid ---------------------------------------------------------------------------------------------------------------------------
run = kc.oracle_run


def restated(case, geometry, T, defect=None, want_z=False):
    r = run(case, geometry, T)
    cfg = kc.GEOMETRIES[geometry]
    pad = np.full((cfg["n_kv_heads"], kc.head_dim(cfg)), kc.QNAN, dtype=np.uint16) if case in kc.POISON_BEYOND else None
    return restate(cfg, r["dumps"][("xq_rope", 0)], r["kv"][0][0], r["kv"][0][1], T - 1, defect, pad, want_z)


def is_denormal_bf16(p16):
    return ((p16 & 0x7F80) == 0) & ((p16 & 0x007F) != 0)


def check_condition(case, geometry, T):
    r = run(case, geometry, T)
    cfg = kc.GEOMETRIES[geometry]
    heads = kc.aligned_heads(cfg)
    d = r["dumps"]
    scores = kc.wide(d[("scores", 0)])[heads, 0, :]          # [aligned heads, T]
    p16 = d[("softmax", 0)][heads, 0, :]
    tag = (case, geometry, T)
    if case == "spread":
        assert (scores.max(axis=1) - scores.min(axis=1) >= 110.0).all(), tag
        assert (is_denormal_bf16(p16).sum(axis=1) >= 1).all() and ((p16 & 0x7FFF) == 0).sum(axis=1).min() >= 1, tag
        assert not np.isnan(r["logits"]).any(), tag
    elif case == "denormal_visible":
        assert (is_denormal_bf16(p16).sum(axis=1) >= 1).all(), tag
        _, flushed = restated(case, geometry, T, "flush_denormal_p")
        assert not np.array_equal(flushed, d[("attn_pre_wo", 0)]), tag
        assert not np.isnan(r["logits"]).any(), tag
    elif case == "huge_finite":
        e = exp_table()[d[("scores", 0)][heads, 0, :]]
        assert (scores[:, :T - 1] >= 590.0).all() and e.max() >= 1e280, tag
        assert not np.isnan(kc.wide(d[("softmax", 0)])).any() and not np.isnan(r["logits"]).any(), tag
    elif case == "one_inf":
        hot = scores > 709.78
        assert (hot.sum(axis=1) == 1).all() and np.array_equal(np.isnan(kc.wide(p16)), hot), tag
        assert np.isnan(r["logits"]).all() and r["am"] == -1, tag
    elif case == "ties":
        for row in p16:
            assert np.unique(row, return_counts=True)[1].max() >= 8, tag
        assert not np.isnan(r["logits"]).any(), tag
    elif case == "v_order":                                    # (what the columns show: tests/test_order_crafted_cpu.py)
        assert not d[("scores", 0)][:, 0, :T - 1].any() and not np.isnan(r["logits"]).any(), tag
        ladder = [c for c, kd in enumerate(kc.pv_kinds(T - 1, kc.head_dim(cfg))) if kd != "zero_sum"]
        own = kc.bf(kc.wide(d[("softmax", 0)])[:, 0, T - 1, None] * kc.wide(r["kv"][0][1])[T - 1][np.arange(cfg["n_heads"]) // (cfg["n_heads"] // cfg["n_kv_heads"])])
        assert np.array_equal(d[("attn_pre_wo", 0)].reshape(cfg["n_heads"], -1)[:, ladder], own[:, ladder]), tag      # exactly +0 from the cached rows
    else:                                                      # signed_zero_v, minus_masked_tail: equality with the device is the whole test
        assert not np.isnan(r["logits"]).any(), tag


def test_the_grid_leaves_out_at_most_one_case_in_eight():
    full = len(kc.CASES) * len(kc.TS)
    assert all(c in kc.CASES and T in kc.TS for c, T in kc.LEFT_OUT)
    assert len(kc.LEFT_OUT) <= full * kc.MAX_LEFT_OUT_FRACTION and kc.MAX_LEFT_OUT_FRACTION == 1.0 / 8.0
    assert len(kc.grid()) == full - len(kc.LEFT_OUT)
    assert set(kc.TS) >= {1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513} and kc.CAPACITY >= max(kc.TS) + kc.TAIL
    assert set(kc.CASES) == {"spread", "denormal_visible", "huge_finite", "one_inf", "ties", "signed_zero_v", "minus_masked_tail", "v_order"}


def test_the_blob_is_the_documented_layout():
    rng = np.random.default_rng(3)
    K = [rng.integers(0, 65536, (5, 2, 16)).astype(np.uint16) for _ in range(2)]
    V = [rng.integers(0, 65536, (5, 2, 16)).astype(np.uint16) for _ in range(2)]
    b = kc.blob(K, V)
    assert bytes(b[:8]) == b"LNBKV1\0\0" and not b[36:64].any()
    assert list(b[8:36].view("<u4")) == [1, 5, 0, 6, 2, 16, 2]
    assert b.size == 64 + 2 * 2 * 5 * 32 * 2
    body = b[64:].view(np.uint16).reshape(2, 2, 5 * 32)
    for l in range(2):
        assert np.array_equal(body[l, 1].reshape(5, 2, 16), V[l])
        k = body[l, 0].reshape(2, 2, 5, 8)                                  # [kv head][hd/8][n_pos][8]
        for kh in range(2):
            for d in range(16):
                assert np.array_equal(k[kh, d >> 3, :, d & 7], K[l][:, kh, d])


@pytest.mark.parametrize("geometry", sorted(kc.GEOMETRIES))
@pytest.mark.parametrize("case", sorted(kc.CASES))
def test_the_oracle_meets_the_condition_and_the_restatement_meets_the_oracle(case, geometry):
    for c, T in kc.grid():
        if c != case:
            continue
        check_condition(case, geometry, T)
        d = run(case, geometry, T)["dumps"]
        p16, att = restated(case, geometry, T)
        assert _eq_or_both_nan_bf16(p16, d[("softmax", 0)]), (case, geometry, T, "softmax")
        assert _eq_or_both_nan_bf16(att, d[("attn_pre_wo", 0)]), (case, geometry, T, "attn_pre_wo")


def test_two_layer_rows_reach_their_own_layer():
    """the second layer's gaussian rows are what its attention reads: the restatement on layer 1's own q and cache gives layer 1's dumps"""
    r = run("ties", "hd64_two_layers", 65)
    cfg = kc.GEOMETRIES["hd64_two_layers"]
    assert not np.array_equal(r["kv"][0][0][:64], r["kv"][1][0][:64])
    p16, att = restate(cfg, r["dumps"][("xq_rope", 1)], r["kv"][1][0], r["kv"][1][1], 64)
    assert _eq_or_both_nan_bf16(p16, r["dumps"][("softmax", 1)]) and _eq_or_both_nan_bf16(att, r["dumps"][("attn_pre_wo", 1)])


# ---- the multi-row calls with a NaN embedding row (two-layer TINY: the NaN row's K / V exist in layer 1) ---------------------------------------------
POISON_ID = 77
POISON_CALLS = {"poison_S20_row17": (20, 17), "poison_S20_row5": (20, 5), "poison_S12_row5": (12, 5)}
_POISON = {}


def poison_run(name):
    if name not in _POISON:
        S, at = POISON_CALLS[name]
        cfg = dict(orc.TINY)
        om = orc.Model(**cfg).fill_synthetic(kc.SEED_MODEL)
        emb = om.get_tensor("tok_embeddings.weight").copy().reshape(cfg["vocab_size"], cfg["dim"])
        emb[POISON_ID] = kc.QNAN
        om.set_tensor("tok_embeddings.weight", emb)
        om.finalize()
        toks = orc.synth_tokens(4242, S, cfg["vocab_size"]).copy()
        toks[toks == POISON_ID] = POISON_ID + 1
        toks[at] = POISON_ID
        oc = orc.Context(om, S)
        dumps = oc.capture()
        logits, am = oc.forward(toks, 0)
        kv = [(oc.cache(l, 0).copy(), oc.cache(l, 1).copy()) for l in range(2)]
        oc.close(); om.close()
        _POISON[name] = dict(cfg=cfg, dumps=dumps, logits=logits, am=am, kv=kv, S=S, at=at)
    return _POISON[name]


@pytest.mark.parametrize("name", sorted(POISON_CALLS))
def test_a_nan_row_of_the_call_poisons_every_row_in_the_reference(name):
    """the reference adds the mask to the score (NaN + -inf = NaN: Z and the whole row NaN) and multiplies p = +0 by every V row of the call, so
    a NaN row ANYWHERE in a modulo-mask call makes every row of layer 1's attention -- and every logits row -- NaN.  The restatement agrees."""
    r = poison_run(name)
    assert np.isnan(r["logits"]).all() and r["am"] == -1
    for l in range(2):
        p16, att = restate(r["cfg"], r["dumps"][("xq_rope", l)], r["kv"][l][0], r["kv"][l][1], 0)
        assert _eq_or_both_nan_bf16(p16, r["dumps"][("softmax", l)]), (name, l)
        assert _eq_or_both_nan_bf16(att, r["dumps"][("attn_pre_wo", l)]), (name, l)
        assert np.isnan(kc.wide(r["dumps"][("attn_pre_wo", l)])).all(), (name, l)      # the NaN embedding row is a NaN K / V row of both layers


# ---- every defect changes a named case ------------------------------------------------------------------------------------------------------------
NAMED = {
    "flush_denormal_p": ("denormal_visible", "hd64", 65),
    "masked_e0_skip_beyond_diagonal": "poison_S20_row17",
    "padded_position": ("minus_masked_tail", "hd128", 17),
    "pairwise_z": ("ties", "h8kv2_hd128", 257),
}


def test_a_pairwise_denominator_changes_z_but_hides_behind_the_two_roundings():
    """Z summed as a balanced tree differs from the serial chain in the last bits of the f64 (the named case: every aligned head).  The quotient
    e / Z is then rounded to f32 and truncated to bf16, so a relative 1e-15 of Z moves a bf16 p only when e / Z lies within that distance of an
    f32 rounding boundary that is also a bf16 boundary: one chance in ~1e12 per entry, which no crafted row of bf16 scores can aim at.  Counted
    over the whole grid here: the number of (case, geometry, T) whose softmax or attn_pre_wo bits move is printed, and Z's own bits are what
    this defect is pinned on.  On the device the serial walk is proven to run by lnb_ctx_zseq_count (tests/test_gpu_attention_crafted.py)."""
    named = NAMED["pairwise_z"]
    assert named[:1] + named[2:] in kc.grid()
    heads = kc.aligned_heads(kc.GEOMETRIES[named[1]])
    serial = restated(*named, want_z=True)[0, heads]
    tree = restated(*named, defect="pairwise_z", want_z=True)[0, heads]
    assert (serial.view(np.uint64) != tree.view(np.uint64)).all(), named
    assert (np.abs(tree / serial - 1.0) < 1e-13).all()
    moved = 0
    for geometry in sorted(kc.GEOMETRIES):
        for case, T in kc.grid():
            d = run(case, geometry, T)["dumps"]
            p16, att = restated(case, geometry, T, defect="pairwise_z")
            moved += not (_eq_or_both_nan_bf16(p16, d[("softmax", 0)]) and _eq_or_both_nan_bf16(att, d[("attn_pre_wo", 0)]))
    print("pairwise Z: %d of %d grid runs change a bf16 bit" % (moved, len(kc.grid()) * len(kc.GEOMETRIES)))


@pytest.mark.parametrize("defect", [d for d in DEFECTS if d != "pairwise_z"])
def test_each_defect_changes_the_bits_of_its_named_case(defect):
    named = NAMED[defect]
    if isinstance(named, str):
        r = poison_run(named)
        ref = r["dumps"][("attn_pre_wo", 0)]                   # layer 0: every q row but the poison row's is finite there
        args = (r["cfg"], r["dumps"][("xq_rope", 0)], r["kv"][0][0], r["kv"][0][1], 0)
        _, clean = restate(*args)
        _, bad = restate(*args, defect=defect)
        rows_before = np.arange(r["S"]) < r["at"]
        assert np.isnan(kc.wide(ref)[rows_before]).all() and not np.isnan(kc.wide(bad)[rows_before]).any(), named
    else:
        assert named[:1] + named[2:] in kc.grid()
        ref = run(*named)["dumps"][("attn_pre_wo", 0)]
        _, clean = restated(*named)
        _, bad = restated(*named, defect=defect)
    assert _eq_or_both_nan_bf16(clean, ref), (defect, named)
    assert not _eq_or_both_nan_bf16(bad, ref), (defect, named)


def test_the_defects_leave_ordinary_rows_alone():
    """on generic rows (no NaN tail) three of the four defects are invisible: that is why the crafted cases are needed"""
    named = ("ties", "hd64", 17)
    ref = run(*named)["dumps"][("attn_pre_wo", 0)]
    for defect in ("flush_denormal_p", "masked_e0_skip_beyond_diagonal", "padded_position"):
        assert _eq_or_both_nan_bf16(restated(*named, defect=defect)[1], ref), defect
