"""Causal multi-row append on the MI355X (include/lnb.h, lnb_forward_append / lnb_forward_score_append).

The contract: the logits rows, the KV rows [start_pos, start_pos + seq) of every layer and the argmax of an append are BIT-IDENTICAL to seq
consecutive one-token Forward calls at start_pos, start_pos + 1, ...; rows below start_pos are never written; any seq >= 1 is accepted.
Every comparison here is on bit patterns (np.array_equal of uint16 / uint32 / uint64 views): no tolerance anywhere."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def one(t):
    return np.array([int(t)], dtype=np.int32)


# ---- 1, 2. the oracle, one token at a time, at three head geometries --------------------------------------------------------------------
STARTS = (0, 1, 5, 16, 37, 64, 200)
SEQS = (1, 2, 7, 15, 16, 17, 33, 64, 100)
N_TOK, SEQ_LEN = 300, 320
CFGS = {
    "hd64": dict(orc.TINY),                                              # 4 query heads on 2 KV heads: attn_mfma3_kernel<64> from 16 rows on
    "hd128_gqa": dict(orc.TINY, dim=1024, n_heads=8, n_kv_heads=2),      # attn_mfma3_kernel<128>, four query heads per KV head
    "hd32": dict(orc.TINY, n_heads=8, n_kv_heads=2),                     # no matrix-core attention: the row-per-workgroup kernel at every row count
}


def test_the_grid_has_both_kinds_of_cases():
    grid = [(p, s) for p in STARTS for s in SEQS]
    assert any((p + s) % s != 0 for p, s in grid)                        # refused by lnb_forward
    assert any((p + s) % s == 0 and p > 0 and s > 1 for p, s in grid)    # accepted by lnb_forward, with the tiled mask
    assert max(p + s for p, s in grid) <= N_TOK <= SEQ_LEN and SEQ_LEN >= 320


@pytest.fixture(scope="module", params=sorted(CFGS))
def geo(lnb, request):
    """the model on both sides and the oracle's one-token run over the whole text: every row an append can be asked for"""
    cfg = CFGS[request.param]
    om = orc.Model(**cfg).fill_synthetic(1234).finalize()
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize()
    toks = orc.synth_tokens(4242, N_TOK, cfg["vocab_size"])
    oc = orc.Context(om, SEQ_LEN)
    rows = np.empty((N_TOK, cfg["vocab_size"]), dtype=np.float32)
    am = np.empty(N_TOK, dtype=np.int64)
    for p in range(N_TOK):
        lo, a = oc.forward(one(toks[p]), p)
        rows[p] = lo[0]; am[p] = a
    kv = [(oc.cache(l, 0).copy(), oc.cache(l, 1).copy()) for l in range(cfg["n_layers"])]
    oc.close()
    yield request.param, cfg, om, gm, toks, rows, am, kv
    gm.close(); om.close()


def _fill_one_token(gc, toks, upto, rows):
    """the prefix, one oracle-checked token at a time"""
    for p in range(upto):
        lg, _ = gc.Forward(one(toks[p]), p)
        assert same(lg[0], rows[p]), "one-token step at %d differs from the oracle" % p


def _kv_equal(gc, kv, upto):
    for l, (k, v) in enumerate(kv):
        if not (np.array_equal(gc.CacheK(l)[:upto], k[:upto]) and np.array_equal(gc.CacheV(l)[:upto], v[:upto])):
            return False
    return True


@pytest.mark.parametrize("start_pos", STARTS)
def test_append_equals_the_oracle_one_token_at_a_time(lnb, geo, start_pos):
    name, cfg, om, gm, toks, rows, am, kv = geo
    gc = lnb.InferenceContext(gm, SEQ_LEN)
    _fill_one_token(gc, toks, start_pos, rows)
    # rows below start_pos are never written, so one context serves every row count (each append is checked on all rows [0, T) of the caches)
    for seq in SEQS:
        T = start_pos + seq
        lg, a = gc.ForwardAppend(toks[start_pos:T], start_pos)
        assert same(lg, rows[start_pos:T]), (name, start_pos, seq, "logits")
        assert a == am[T - 1], (name, start_pos, seq, "argmax")
        assert _kv_equal(gc, kv, T), (name, start_pos, seq, "KV")
        want_form = 3 if (seq >= 16 and name != "hd32") else 0
        if seq > 1:
            assert gc.prefill_attention_form() == want_form, (name, seq)
        _, a2 = gc.ForwardAppend(toks[start_pos:T], start_pos, want_logits=False)          # only the last row's head
        assert a2 == a
    gc.close()


@pytest.mark.parametrize("start_pos,seq", [(p, s) for p in STARTS for s in SEQS if p > 0 and s > 1 and (p + s) % s == 0])
def test_forward_keeps_the_reference_mask_where_it_is_accepted(lnb, geo, start_pos, seq):
    """T % seq == 0 at start_pos > 0: lnb_forward still computes the reference's tiled mask (the oracle's multi-row forward), which is NOT the append"""
    name, cfg, om, gm, toks, rows, am, kv = geo
    T = start_pos + seq
    oc = orc.Context(om, SEQ_LEN)
    for p in range(start_pos):
        oc.forward(one(toks[p]), p, want_logits=False)
    lo, ao = oc.forward(toks[start_pos:T], start_pos)
    gc = lnb.InferenceContext(gm, SEQ_LEN)
    _fill_one_token(gc, toks, start_pos, rows)
    lg, ag = gc.Forward(toks[start_pos:T], start_pos)
    assert same(lg, lo) and ag == ao, (name, start_pos, seq)
    for l in range(cfg["n_layers"]):
        assert np.array_equal(gc.CacheK(l)[:T], oc.cache(l, 0)[:T]) and np.array_equal(gc.CacheV(l)[:T], oc.cache(l, 1)[:T])
    la, _ = gc.ForwardAppend(toks[start_pos:T], start_pos)
    assert same(la, rows[start_pos:T])
    assert not same(la, lg), "the tiled mask and the causal mask gave the same logits"
    gc.close(); oc.close()


def test_forward_still_refuses_what_the_reference_refuses(lnb, geo):
    name, cfg, om, gm, toks, rows, am, kv = geo
    gc = lnb.InferenceContext(gm, SEQ_LEN)
    _fill_one_token(gc, toks, 5, rows)
    with pytest.raises(lnb.LnbError, match="cannot be broadcasted"):
        gc.Forward(toks[5:12], 5)
    lg, _ = gc.ForwardAppend(toks[5:12], 5)
    assert same(lg, rows[5:12])
    gc.close()


# ---- 3. chunk invariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sidx_mb,form", [(None, 3), ("0", 1)])
def test_chunking_a_prompt_changes_nothing(lnb, geo, sidx_mb, form, monkeypatch):
    name, cfg, om, gm, toks, rows, am, kv = geo
    if sidx_mb is not None:
        monkeypatch.setenv("LNB_ATTN_SIDX_MB", sidx_mb)                  # the score-index scratch is refused: attn_mfma_kernel (scores twice)
    if name == "hd32":
        form = 0
    P = 300
    results = []
    for chunks in ((P,), (64, 64, 100, 72), (16,) * 18 + (12,)):
        assert sum(chunks) == P
        gc = lnb.InferenceContext(gm, SEQ_LEN)
        p = 0
        for i, n in enumerate(chunks):
            if len(chunks) == 1:
                lg, a = gc.Forward(toks[:P], 0)
            else:
                lg, a = gc.ForwardAppend(toks[p:p + n], p)
            if n >= 16:
                assert gc.prefill_attention_form() == form, (name, chunks, i)
            p += n
        results.append((lg[-1].copy(), a, [(gc.CacheK(l)[:P].copy(), gc.CacheV(l)[:P].copy()) for l in range(cfg["n_layers"])]))
        gc.close()
    for last, a, caches in results:
        assert same(last, rows[P - 1]) and a == am[P - 1]
        for l, (k, v) in enumerate(caches):
            assert np.array_equal(k, kv[l][0][:P]) and np.array_equal(v, kv[l][1][:P])


# ---- 4. long context: the GPU's own one-token steps (which the existing suite pins to the oracle) ------------------------------------------
def test_long_context_appends_equal_one_token_steps(lnb):
    """8B head geometry (32 query heads on 8 KV heads, head_dim 128), two layers, 8400 positions.  Prefixes above the long-context crossover
    (one-token steps run attn_long_*) and above what the row-per-workgroup kernel stages in the LDS (8 rows there: the one-token fallback
    inside the entry point; 64 rows: the matrix-core kernel, which has no such limit)."""
    cfg = dict(orc.TINY, dim=4096, n_heads=32, n_kv_heads=8, multiple_of=1024, max_seq_len=4224)
    SL, P = 8400, 8000
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(77).finalize()
    toks = lnb.synth_tokens(31, SL, cfg["vocab_size"])
    a_ctx, b_ctx = lnb.InferenceContext(gm, SL), lnb.InferenceContext(gm, SL)
    for c in (a_ctx, b_ctx):                                             # the prefix, filled once: one exact prefill of 8000 rows at position 0
        c.Forward(toks[:P], 0, want_logits=False)
    L = cfg["n_layers"]
    base = [(a_ctx.CacheK(l).copy(), a_ctx.CacheV(l).copy()) for l in range(L)]
    for l in range(L):
        assert np.array_equal(base[l][0][:P], b_ctx.CacheK(l)[:P]) and np.array_equal(base[l][1][:P], b_ctx.CacheV(l)[:P])
    for start, counts in ((1000, (1, 8, 64)), (P, (8, 64))):
        n = max(counts)
        ref = np.empty((n, cfg["vocab_size"]), dtype=np.float32)
        ram = []
        for i in range(n):                                               # one-token steps on the second context
            lg, a = b_ctx.Forward(one(toks[start + i]), start + i)
            ref[i] = lg[0]; ram.append(a)
        for seq in counts:
            lg, a = a_ctx.ForwardAppend(toks[start:start + seq], start)
            assert same(lg, ref[:seq]) and a == ram[seq - 1], (start, seq)
            for l in range(L):
                k, v = a_ctx.CacheK(l), a_ctx.CacheV(l)
                assert np.array_equal(k[:start], base[l][0][:start]) and np.array_equal(v[:start], base[l][1][:start]), (start, seq, "rows below start_pos were written")
                assert np.array_equal(k[start:start + seq], b_ctx.CacheK(l)[start:start + seq]), (start, seq)
                assert np.array_equal(v[start:start + seq], b_ctx.CacheV(l)[start:start + seq]), (start, seq)
    # lnb_forward's refusal beyond the row kernel's reach is unchanged
    with pytest.raises(lnb.LnbError, match="2..15"):
        a_ctx.Forward(toks[P + 64:P + 72], P + 64)                       # T = 8072 = 8 * 1009
    a_ctx.close(); b_ctx.close(); gm.close()


# ---- 5. continuation --------------------------------------------------------------------------------------------------------------------
def test_the_device_loops_continue_an_appended_context(lnb):
    cfg = dict(orc.TINY)
    om = orc.Model(**cfg).fill_synthetic(1234).finalize()
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize()
    toks = orc.synth_tokens(4242, N_TOK, cfg["vocab_size"])
    P, steps = 41, 12

    def ingest(chunks):
        gc = lnb.InferenceContext(gm, 96)
        p = 0
        for n in chunks:
            _, a = (gc.Forward(toks[p:p + 1], p, want_logits=False) if chunks == (1,) * P else gc.ForwardAppend(toks[p:p + n], p, want_logits=False))
            p += n
        return gc, a

    def runs(chunks):
        out = {}
        gc, first = ingest(chunks)
        t, fin, _ = gc.decode_greedy_until(first, P, steps)
        out["greedy"] = ([int(x) for x in t], fin); gc.close()
        gc, first = ingest(chunks)
        gc.set_draft(4, 1, 4, toks[:P])
        t, fin, st, _ = gc.decode_speculative_until(toks[:P], first, P, steps)
        out["spec"] = ([int(x) for x in t], fin); gc.close()
        (g0, f0), (g1, f1) = ingest(chunks), ingest(chunks)
        bat = lnb.Batch([g0, g1])
        bt, _ = bat.decode([f0, f1], [P, P], steps)
        out["batch"] = [[int(x) for x in r] for r in bt]
        bat.close(); g0.close(); g1.close()
        return first, out

    f_one, r_one = runs((1,) * P)
    f_app, r_app = runs((17, 3, 21))
    assert f_one == f_app
    assert r_one == r_app
    assert r_app["greedy"][0] == r_app["spec"][0] == r_app["batch"][0] == r_app["batch"][1]
    oc = orc.Context(om, 96)                                             # ... and they are the oracle's tokens
    for p in range(P):
        oc.forward(one(toks[p]), p, want_logits=False)
    ref, t = [], f_app
    for i in range(steps):
        _, t = oc.forward(one(t), P + i, want_logits=False)
        ref.append(t)
    oc.close()
    assert r_app["greedy"][0] == ref
    # a further append continues a decoded context
    gc, first = ingest((17, 3, 21))
    t, _, _ = gc.decode_greedy_until(first, P, 3)
    more = np.array([first] + [int(x) for x in t], dtype=np.int32)
    gd = lnb.InferenceContext(gm, 96)
    full = np.concatenate([toks[:P], more, toks[100:123]]).astype(np.int32)
    want = [gd.Forward(full[p:p + 1], p)[0][0] for p in range(full.size)]
    lg, _ = gc.ForwardAppend(full[P + 3:], P + 3)                         # (rewrites the last decoded row's successor onwards: the same text)
    assert same(lg, np.stack(want[P + 3:]))
    gc.close(); gd.close(); gm.close(); om.close()


# ---- 6. scoring -------------------------------------------------------------------------------------------------------------------------
def test_score_append_gives_the_bits_of_one_row_score_calls(lnb, geo):
    name, cfg, om, gm, toks, rows, am, kv = geo
    P = 90
    tg = np.concatenate([toks[1:P], [-1]]).astype(np.int32)
    tg[7] = -1; tg[40] = -1
    ref = lnb.InferenceContext(gm, SEQ_LEN)
    r_tl, r_tp, r_lz, r_am = [], [], [], None
    for p in range(P):
        tl, tp, lz, r_am = ref.score(toks[p:p + 1], p, tg[p:p + 1])
        r_tl.append(tl[0]); r_tp.append(tp[0]); r_lz.append(lz[0])
    r_tl, r_tp, r_lz = np.array(r_tl, dtype=np.float32), np.array(r_tp, dtype=np.float32), np.array(r_lz, dtype=np.float64)
    ok = tg >= 0
    assert same(r_tl[ok], rows[np.nonzero(ok)[0], tg[ok]])               # (the one-row calls themselves: the target's logit is the oracle's)
    gc = lnb.InferenceContext(gm, SEQ_LEN)
    g_tl, g_tp, g_lz = [], [], []
    p = 0
    for n in (5, 16, 1, 33, 35):
        tl, tp, lz, a = gc.score_append(toks[p:p + n], p, tg[p:p + n])
        g_tl.append(tl.copy()); g_tp.append(tp.copy()); g_lz.append(lz.copy())
        p += n
    assert p == P and a == r_am == am[P - 1]
    g_tl, g_tp, g_lz = np.concatenate(g_tl), np.concatenate(g_tp), np.concatenate(g_lz)
    assert same(g_tl[ok], r_tl[ok]) and same(g_tp[ok], r_tp[ok]) and same(g_lz, r_lz)
    assert np.isnan(g_tl[~ok]).all() and np.isnan(g_tp[~ok]).all() and np.isfinite(g_lz).all()
    assert _kv_equal(gc, kv, P)
    with pytest.raises(lnb.LnbError, match="outside the vocabulary"):
        gc.score_append(toks[:4], P, np.array([1, 2, cfg["vocab_size"], 3], dtype=np.int32))
    gc.close(); ref.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(lnb, geo):
    name, cfg, om, gm, toks, rows, am, kv = geo
    gc = lnb.InferenceContext(gm, 64)
    gc.ForwardAppend(toks[:20], 0, want_logits=False)
    gc.set_mode("fast")
    with pytest.raises(lnb.LnbError, match="exact-mode only"):
        gc.ForwardAppend(toks[20:40], 20)
    with pytest.raises(lnb.LnbError, match="exact-mode only"):
        gc.score_append(toks[20:40], 20, toks[21:41])
    gc.set_mode("exact")
    with pytest.raises(lnb.LnbError, match="beyond the KV cache"):
        gc.ForwardAppend(toks[20:70], 20)                               # T = 70 > 64
    with pytest.raises(lnb.LnbError, match="outside the vocabulary"):
        gc.ForwardAppend(np.array([1, cfg["vocab_size"], 2], dtype=np.int32), 20)
    lg, a = gc.ForwardAppend(toks[20:57], 20)                           # the context still works
    assert same(lg, rows[20:57]) and a == am[56] and _kv_equal(gc, kv, 57)
    gc.close()
    rope_rows = gm.PrecomputedFreqsCis.shape[0]
    big = lnb.InferenceContext(gm, rope_rows + 32)
    with pytest.raises(lnb.LnbError, match="RoPE table"):
        big.ForwardAppend(np.zeros(32, dtype=np.int32), rope_rows - 16)
    big.close()
    stage = lnb.LlamaTransformer(device=0, layer_begin=0, layer_end=1, **cfg).fill_synthetic(1234).finalize()
    sc = lnb.InferenceContext(stage, 64)
    with pytest.raises(lnb.LnbError, match="whole-model"):
        sc.ForwardAppend(toks[:20], 0)
    sc.close(); stage.close()


def test_engine_prefill_chunk_gives_the_same_tokens(lnb, geo):
    name, cfg, om, gm, toks, rows, am, kv = geo
    prompt = [int(t) for t in toks[:70]]
    want = lnb.InferenceEngine(gm, 96).GenerateTokens(prompt, max_new=10)
    for chunk in (1, 7, 16, 33, 64, 200):
        assert lnb.InferenceEngine(gm, 96, prefill_chunk=chunk).GenerateTokens(prompt, max_new=10) == want, chunk
    assert want[0] == am[69]


# ---- 8. the full 8B shape ---------------------------------------------------------------------------------------------------------------
def test_llama8b_configs1_prompt_appended_in_two_chunks_continues_token_identical(lnb):
    """BASELINE.json configs[1]: the 128-token prompt ingested as appends of 48 + 80 rows (128 % 80 != 0: lnb_forward refuses that second call),
    then the greedy loop: the tokens of the committed oracle continuation."""
    g = json.load(open(os.path.join(GOLD, "configs1_tokens.json")))
    n_new = 32
    gm = lnb.LlamaTransformer(**lnb.LLAMA_8B).fill_synthetic(g["weights_seed"]).finalize()
    prompt = lnb.synth_tokens(g["prompt_seed"], 128, 128256)
    assert g["prompt_len"] == 128
    gc = lnb.InferenceContext(gm, 128 + n_new)
    gc.ForwardAppend(prompt[:48], 0, want_logits=False)
    with pytest.raises(lnb.LnbError, match="cannot be broadcasted"):
        gc.Forward(prompt[48:], 48, want_logits=False)
    lg, first = gc.ForwardAppend(prompt[48:], 48)
    assert gc.prefill_attention_form() == 3
    rest, _ = gc.decode_greedy(first, 128, n_new - 1)
    got = [first] + [int(t) for t in rest]
    assert got == g["tokens"][:n_new]
    # the same rows from one exact prefill at position 0: logits of the appended rows and the caches, bit for bit
    gd = lnb.InferenceContext(gm, 128 + n_new)
    lf, f2 = gd.Forward(prompt, 0)
    assert f2 == first and same(lg, lf[48:])
    for layer in (0, 15, 31):
        assert np.array_equal(gc.CacheK(layer)[:128], gd.CacheK(layer)[:128]) and np.array_equal(gc.CacheV(layer)[:128], gd.CacheV(layer)[:128])
    gc.close(); gd.close(); gm.close()
