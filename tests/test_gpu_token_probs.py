"""Token probabilities on the MI355X (include/lnb.h "token probabilities"): every reported probability must be the bits of the oracle's
orc_softmax_f32 on the same logits row (the reference's ml.Softmax with the host libm exp), the top-k must follow ml.Argmax's order, and
the feature must not change a single generated token."""
import json
import math
import os

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FMAX = np.float32(3.4028234663852886e38)


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


# ---- host references -------------------------------------------------------------------------------------------------------------
def orc_softmax(rows_f32):
    rows_f32 = np.ascontiguousarray(rows_f32, dtype=np.float32)
    out = np.empty_like(rows_f32)
    orc.lib().orc_softmax_f32(orc._p(rows_f32), orc._p(out), rows_f32.shape[0], rows_f32.shape[1])
    return out


_ETAB = None


def _exp(x):
    if math.isnan(x):
        return math.nan
    try:
        return math.exp(x)
    except OverflowError:                                    # (libm returns +inf there; Python raises)
        return math.inf


def exp_table():
    """exp(double(bf16)) with math.exp (the host libm) for every pattern"""
    global _ETAB
    if _ETAB is None:
        v = orc.bf16_to_f32(np.arange(65536, dtype=np.uint16)).astype(np.float64)
        _ETAB = np.array([_exp(x) for x in v], dtype=np.float64)
    return _ETAB


def serial_ln_z(rows_u16):
    """ln of the reference's serial sum (cumsum adds in index order)"""
    e = exp_table()[rows_u16.astype(np.int64)]
    z = np.cumsum(e, axis=1)[:, -1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(z)


def ref_topk(row_f32, k):
    """ml.Argmax's candidates (not NaN, > -MaxFloat32), value descending, lowest index first; -1 padded"""
    idx = np.nonzero(row_f32 > -FMAX)[0]
    order = idx[np.lexsort((idx, -row_f32[idx].astype(np.float64)))][:k]
    return np.concatenate([order, -np.ones(k - order.size, dtype=np.int64)]).astype(np.int32)


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float32); b = np.asarray(b, dtype=np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def check_records(row_f32, ids, logits, probs, k, ref_p=None):
    """one record (ids / logits / probs [k]) against the oracle on its logits row"""
    if ref_p is None:
        ref_p = orc_softmax(row_f32[None, :])[0]
    want = ref_topk(row_f32, k)
    assert (ids == want).all(), (ids, want)
    ok = want >= 0
    assert same_bits(logits[ok], row_f32[want[ok]]) and same_bits(probs[ok], ref_p[want[ok]])
    assert np.isnan(logits[~ok]).all() and np.isnan(probs[~ok]).all()


def llama_like_rows(rng, rows, V):
    """gaussian body plus a few peaks, truncated to bf16 like the head's output"""
    x = rng.normal(0.0, 2.2, size=(rows, V)).astype(np.float32)
    for r in range(rows):
        n = rng.integers(1, 6)
        x[r, rng.integers(0, V, size=n)] += rng.uniform(6.0, 16.0, size=n).astype(np.float32)
    return orc.f32_to_bf16(x)


# ---- 1. operator level -----------------------------------------------------------------------------------------------------------
def test_op_rows_match_the_oracle_bit_for_bit_and_the_walk_really_runs(lnb):
    V, K, R = 128256, 16, 2048
    rng = np.random.default_rng(20261015)
    walks_total, walked = 0, []
    for part in range(0, R, 512):
        u = llama_like_rows(rng, 512, V)
        tg = rng.integers(0, V, size=512).astype(np.int32)
        tg[::97] = -1
        r = lnb.op_token_probs(u, K, targets=tg)
        f = orc.bf16_to_f32(u)
        ref = orc_softmax(f)
        for i in range(512):
            check_records(f[i], r["ids"][i], r["logits"][i], r["probs"][i], K, ref[i])
        ok = tg >= 0
        assert same_bits(r["target_prob"][ok], ref[np.nonzero(ok)[0], tg[ok]]) and np.isnan(r["target_prob"][~ok]).all()
        lz = serial_ln_z(u)
        assert (np.abs(r["log_z"] - lz) <= (V + 8) * 2.0 ** -52).all()
        walks_total += r["serial_walks"]
        # the serial fallback for every row gives the same bits
        s = lnb.op_token_probs(u, K, targets=tg, force_serial=True)
        assert s["serial_walks"] == 512
        for key in ("ids", "logits", "probs", "target_prob"):
            assert same_bits(s[key], r[key]) if key != "ids" else (s[key] == r[key]).all(), key
        walked.append(r["serial_walks"])
    print("token probabilities: %d of %d rows walked the serial sum (top-16 + target), per part %s" % (walks_total, R, walked))
    assert walks_total > 0


def _special_rows(V):
    rng = np.random.default_rng(7)
    base = orc.bf16_to_f32(llama_like_rows(rng, 1, V))[0]
    rows = []
    r = base.copy(); r[[5, 77, V - 1]] = 40.0; rows.append(r)                      # ties at the maximum
    r = base.copy(); r[123] = np.nan; rows.append(r)                               # one NaN
    rows.append(np.full(V, np.nan, dtype=np.float32))                               # all NaN
    r = base.copy(); r[10] = np.inf; r[11] = -np.inf; r[V // 2] = np.inf; rows.append(r)   # +-inf
    r = np.full(V, -np.inf, dtype=np.float32); r[3] = -3.3895314e38; r[9] = -3.3895314e38; r[V - 2] = 1.0; rows.append(r)   # largest negative bf16, fewer than k candidates
    r = base.copy(); r[42] = 712.0; rows.append(r)                                  # exp overflows: Z = +inf
    r = np.zeros(V, dtype=np.float32); r[-1] = -0.0; r[1] = 0.0; r[0] = -0.0; rows.append(r)   # signed zeros tie
    r = np.full(V, -200.0, dtype=np.float32); r[V // 3] = 100.0; rows.append(r)    # one dominant value: prob 1.0f
    r = np.full(V, -800.0, dtype=np.float32); rows.append(r)                       # every exp underflows: Z = 0
    return orc.f32_to_bf16(np.stack(rows))


@pytest.mark.parametrize("V", [128256, 1024, 1001])
def test_op_special_rows(lnb, V):
    u = _special_rows(V)
    f = orc.bf16_to_f32(u)
    ref = orc_softmax(f)
    tg = np.array([5, 123, 0, 10, 3, 42, 1, V // 3, 7], dtype=np.int32)
    for fs in (False, True):
        r = lnb.op_token_probs(u, 16, targets=tg, force_serial=fs)
        for i in range(u.shape[0]):
            check_records(f[i], r["ids"][i], r["logits"][i], r["probs"][i], 16, ref[i])
            assert r["ids"][i, 0] == lnb.op_argmax(u[i])                            # entry 0 = ml.Argmax
        assert same_bits(r["target_prob"], ref[np.arange(u.shape[0]), tg])
        lz = serial_ln_z(u)
        fin = np.isfinite(lz)
        assert (np.abs(r["log_z"][fin] - lz[fin]) <= (V + 8) * 2.0 ** -52).all()
        assert same_bits(r["log_z"][~fin].astype(np.float32), lz[~fin].astype(np.float32))
    assert r["probs"][7, 0] == np.float32(1.0)
    # a generic V that is not a multiple of 8, rows at odd offsets: gaussian rows as well
    if V == 1001:
        g = llama_like_rows(np.random.default_rng(3), 64, V)
        r = lnb.op_token_probs(g, 5)
        gf = orc.bf16_to_f32(g); gr = orc_softmax(gf)
        for i in range(64):
            check_records(gf[i], r["ids"][i], r["logits"][i], r["probs"][i], 5, gr[i])


# ---- 2. tiny model: greedy loop ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(lnb):
    cfg = dict(orc.TINY)
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize()
    om = orc.Model(**cfg).fill_synthetic(1234).finalize()
    prompt = lnb.synth_tokens(99, 8, cfg["vocab_size"])
    # the oracle's logits row of every step
    oc = orc.Context(om, 64)
    _, tok = oc.forward(prompt, 0, want_logits=False)
    first, rows, toks = tok, [], []
    for i in range(24):
        lg, tok = oc.forward([tok], 8 + i, want_logits=True)
        rows.append(lg[0]); toks.append(tok)
    oc.close()
    yield gm, prompt, first, np.array(toks, dtype=np.int32), np.stack(rows)
    gm.close(); om.close()


def _tiny_run(lnb, gm, prompt, k, steps=24, stop=None):
    c = lnb.InferenceContext(gm, 64)
    _, f = c.Forward(prompt, 0, want_logits=False)
    c.set_token_probs(k)
    if stop is not None:
        c.set_stop_ids([stop])
    got, fin, _ = c.decode_greedy_until(f, 8, steps)
    return c, f, got


@pytest.mark.parametrize("graph", ["graph", "nograph"])
def test_tiny_greedy_records_match_the_oracle(lnb, tiny, graph, monkeypatch):
    if graph == "nograph":
        monkeypatch.setenv("LNB_NO_GRAPH", "1")
    gm, prompt, first, ref_toks, ref_rows = tiny
    c0, f0, plain = _tiny_run(lnb, gm, prompt, 0)
    c, f, got = _tiny_run(lnb, gm, prompt, 8)
    assert f == f0 == first
    assert (got == plain).all() and (got == ref_toks).all()
    ids, lg, pr, lz = c.token_probs(24)
    assert ids.shape == (24, 8) and (ids[:, 0] == got).all()
    ref = orc_softmax(ref_rows)
    for i in range(24):
        check_records(ref_rows[i], ids[i], lg[i], pr[i], 8, ref[i])
    lzr = serial_ln_z(orc.f32_to_bf16(ref_rows))
    assert (np.abs(lz - lzr) <= (1024 + 8) * 2.0 ** -52).all()
    # a window of the log
    i2, _, p2, _ = c.token_probs(5, first=10)
    assert (i2 == ids[10:15]).all() and same_bits(p2, pr[10:15])
    c.close(); c0.close()


def test_tiny_stop_id_bounds_the_records(lnb, tiny):
    gm, prompt, first, ref_toks, ref_rows = tiny
    j = next(i for i in range(5, 24) if ref_toks[i] not in ref_toks[:i])
    c, f, got = _tiny_run(lnb, gm, prompt, 4, stop=int(ref_toks[j]))
    assert got.size == j + 1 and (got == ref_toks[:j + 1]).all()
    ids, _, pr, _ = c.token_probs(j + 1)
    assert (ids[:, 0] == got).all()
    with pytest.raises(lnb.LnbError, match="generated"):
        c.token_probs(j + 2)
    with pytest.raises(lnb.LnbError):
        c.token_probs(1, first=j + 1)
    c.close()


def test_toggling_and_refusals(lnb, tiny):
    gm, prompt, first, ref_toks, ref_rows = tiny
    c = lnb.InferenceContext(gm, 64)
    _, f = c.Forward(prompt, 0, want_logits=False)
    c.set_token_probs(16)
    a, _ = c.decode_greedy(f, 8, 12)
    assert (c.token_probs(12)[0][:, 0] == a).all()
    c.set_token_probs(0)
    b, _ = c.decode_greedy(f, 8, 12)
    assert (a == b).all() and (a == ref_toks[:12]).all()
    with pytest.raises(lnb.LnbError, match="no token probabilities"):
        c.token_probs(1)
    for bad in (-1, 17):
        with pytest.raises(lnb.LnbError, match="top_k"):
            c.set_token_probs(bad)
    # batches: one top-k for all members, fixed while the batch lives
    gm.enable_batch()
    d = lnb.InferenceContext(gm, 64)
    d.set_token_probs(4)
    with pytest.raises(lnb.LnbError, match="one setting"):
        lnb.Batch([c, d])
    c.set_token_probs(4)
    bat = lnb.Batch([c, d])
    with pytest.raises(lnb.LnbError, match="live batch"):
        c.set_token_probs(8)
    _, f2 = d.Forward(prompt, 0, want_logits=False)
    out, _ = bat.decode([f, f2], [8, 8], 6)
    assert (out[0] == ref_toks[:6]).all() and (out[1] == ref_toks[:6]).all()
    for x in (c, d):
        ids, _, pr, _ = x.token_probs(6)
        assert (ids[:, 0] == ref_toks[:6]).all()
        check_records(ref_rows[3], ids[3], x.token_probs(6)[1][3], pr[3], 4)
    bat.close()
    c.close(); d.close()


# ---- 3..6. the 8B shape (configs[1]) -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def m8b(lnb):
    g = json.load(open(os.path.join(GOLD, "configs1_tokens.json")))
    gm = lnb.LlamaTransformer(**lnb.LLAMA_8B).fill_synthetic(g["weights_seed"]).finalize()
    prompt = lnb.synth_tokens(g["prompt_seed"], 128, 128256)
    yield gm, prompt, g
    gm.close()


def _row_hash(row):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(row, dtype=np.float32).view(np.uint32).astype("<u4").tobytes()).hexdigest()


def test_8b_greedy_top16_records_match_the_oracle_on_the_devices_logits(lnb, m8b):
    gm, prompt, g = m8b
    N = 64
    c = lnb.InferenceContext(gm, 256)
    _, first = c.Forward(prompt, 0, want_logits=False)
    c.set_token_probs(16)
    got, _ = c.decode_greedy(first, 128, N)
    assert [first] + [int(t) for t in got] == g["tokens"][:N + 1]
    ids, lg, pr, lz = c.token_probs(N)
    assert (ids[:, 0] == got).all()
    walks = c.token_prob_walks()
    # the logits rows of the same steps, from lnb_forward on a second context over prompt + generated tokens
    d = lnb.InferenceContext(gm, 256)
    seq = np.concatenate([prompt, [first], got[:N - 1]]).astype(np.int32)
    rows, am = d.Forward(seq, 0, want_logits=True)
    assert am == got[N - 1]
    hashes = json.load(open(os.path.join(GOLD, "configs1_logits.json")))
    steps = rows[128:128 + N]
    for i, st in enumerate(hashes["steps"][:N]):
        assert _row_hash(steps[i]) == st["logits_sha256"], i
    ref = orc_softmax(steps)
    for i in range(N):
        check_records(steps[i], ids[i], lg[i], pr[i], 16, ref[i])
    lzr = serial_ln_z(orc.f32_to_bf16(steps))
    assert (np.abs(lz - lzr) <= (128256 + 8) * 2.0 ** -52).all()
    print("8B top-16: %d of %d steps walked the serial sum" % (walks, N))
    c.close(); d.close()


@pytest.mark.parametrize("n", [16, 128])
def test_8b_batch_records_equal_single_context_runs(lnb, m8b, n):
    gm, _, _ = m8b
    g = json.load(open(os.path.join(GOLD, "configs1_multi_P128_tokens.json")))
    steps = 6
    prompts = [lnb.synth_tokens(g["prompt_seed_base"] + s, 128, 128256) for s in range(n)]
    ctxs = [lnb.InferenceContext(gm, 136) for _ in range(n)]
    firsts = [c.Forward(p, 0, want_logits=False)[1] for c, p in zip(ctxs, prompts)]
    for c in ctxs:
        c.set_token_probs(4)
    bat = lnb.Batch(ctxs)
    out, _ = bat.decode(firsts, [128] * n, steps)
    bat.close()
    recs = [c.token_probs(steps) for c in ctxs]
    for s in range(n):
        gs = g["tokens"].get(str(s))
        if gs is not None:
            m_ = min(len(gs), steps + 1)
            assert ([firsts[s]] + [int(t) for t in out[s]])[:m_] == gs[:m_], s
    single = lnb.InferenceContext(gm, 136).set_token_probs(4)
    for s in range(n):
        _, f = single.Forward(prompts[s], 0, want_logits=False)
        t, _ = single.decode_greedy(f, 128, steps)
        assert (t == out[s]).all(), s
        r1 = single.token_probs(steps)
        assert (r1[0] == recs[s][0]).all() and same_bits(r1[1], recs[s][1]) and same_bits(r1[2], recs[s][2]), s
        assert (r1[3].view(np.uint64) == recs[s][3].view(np.uint64)).all(), s
    single.close()
    for c in ctxs:
        c.close()


def test_8b_score_matches_forward(lnb, m8b):
    gm, prompt, g = m8b
    c = lnb.InferenceContext(gm, 256); d = lnb.InferenceContext(gm, 256)
    tg = np.concatenate([prompt[1:], [-1]]).astype(np.int32)
    tl, tp, lz, am = c.score(prompt, 0, tg)
    rows, am2 = d.Forward(prompt, 0, want_logits=True)
    assert am == am2 == g["tokens"][0]
    ref = orc_softmax(rows)
    ok = tg >= 0
    assert same_bits(tp[ok], ref[np.nonzero(ok)[0], tg[ok]]) and same_bits(tl[ok], rows[np.nonzero(ok)[0], tg[ok]])
    assert np.isnan(tp[~ok]).all() and np.isnan(tl[~ok]).all()
    assert (np.abs(lz - serial_ln_z(orc.f32_to_bf16(rows))) <= (128256 + 8) * 2.0 ** -52).all()
    for layer in (0, 31):
        assert (c.CacheK(layer)[:128] == d.CacheK(layer)[:128]).all() and (c.CacheV(layer)[:128] == d.CacheV(layer)[:128]).all()
    c.close(); d.close()
    # a 4096-row prompt: a sample of rows against lnb_forward's logits rows
    P = 4096
    long_prompt = lnb.synth_tokens(5, P, 128256)
    tg = np.concatenate([long_prompt[1:], [-1]]).astype(np.int32)
    c = lnb.InferenceContext(gm, P)
    tl, tp, lz, am = c.score(long_prompt, 0, tg)
    c.close()
    d = lnb.InferenceContext(gm, P)
    rows, am2 = d.Forward(long_prompt, 0, want_logits=True)
    d.close()
    assert am == am2
    sample = np.array([0, 1, 777, 2048, 3333, P - 2], dtype=np.int64)
    ref = orc_softmax(rows[sample])
    assert same_bits(tp[sample], ref[np.arange(sample.size), tg[sample]])
    assert np.isnan(tp[P - 1])
