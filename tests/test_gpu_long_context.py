"""Contexts of up to 131072 positions (-m gpu): lnb_ctx_create_long, the long-context PV kernel with an LDS layout that does not grow with the context,
activation buffers sized by max_rows.  Every comparison is bit-exact.  References: the CPU oracle's golden file across position 23552 (where
lnb_ctx_create stops; tests/golden/make_long_context_tokens.py), the contexts of lnb_ctx_create (pinned to the oracle by the rest of the suite), and at the
far end two independent kernels against each other (the matrix-core append and the one-token scores + PV pair)."""
import ctypes as C
import hashlib
import json
import os
import time

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = json.load(open(os.path.join(ROOT, "tests", "golden", "long_context_tiny_tokens.json")))
CFG = dict(orc.TINY, n_heads=2, n_kv_heads=1, n_layers=1, max_seq_len=12288)     # the golden's model
P, CHUNK, FAR = G["prompt_len"], 4096, 131072
GOLD = [G["first_token"]] + G["tokens"]                      # GOLD[k]: the input of the step at position P + k
BIG = dict(orc.TINY, n_heads=2, n_kv_heads=1, max_seq_len=4224)                  # tests/test_gpu_batch_long.py's shape beyond the one-workgroup cap


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


@pytest.fixture(scope="module")
def gm(lnb):
    """the golden's model with a RoPE table of 131072 rows (the same formula further: the first 24576 rows are the golden's)"""
    m = lnb.LlamaTransformer(**CFG).fill_synthetic(G["weights_seed"]).finalize(FAR)
    yield m
    m.close()


@pytest.fixture(scope="module")
def prompt(lnb):
    return lnb.synth_tokens(G["prompt_seed"], P, CFG["vocab_size"])


def _row_hash(row):
    return hashlib.sha256(np.ascontiguousarray(row, dtype=np.float32).view(np.uint32).astype("<u4").tobytes()).hexdigest()


def _rows_hash(rows):
    return hashlib.sha256(np.ascontiguousarray(rows, dtype=np.uint16).astype("<u2").tobytes()).hexdigest()


def _ingest(ctx, tokens, chunk=CHUNK, start=0):
    first = None
    for p0 in range(0, len(tokens), chunk):
        _, first = ctx.ForwardAppend(tokens[p0:p0 + chunk], start + p0, want_logits=False)
    return first


def _golden_run(ctx):
    """four eager one-token steps (logits hashes), then the captured graph for the other 20: the golden's tokens and K / V rows"""
    for k, s in enumerate(G["steps"]):
        lg, nxt = ctx.Forward([GOLD[k]], P + k)
        assert _row_hash(lg[0]) == s["logits_sha256"] and nxt == GOLD[k + 1], k
    more, _ = ctx.decode_greedy(GOLD[4], P + 4, 20)
    assert [int(t) for t in more] == GOLD[5:]
    assert _rows_hash(ctx.CacheK(0)[P:P + 24]) == G["k_rows_sha256"]
    assert _rows_hash(ctx.CacheV(0)[P:P + 24]) == G["v_rows_sha256"]


def test_golden_across_the_old_cap(lnb, gm, prompt):
    """23540 oracle-checked positions, then 24 steps across 23552 -- the capacity lnb_ctx_create stops at and a batch edge of the PV kernel"""
    with pytest.raises(lnb.LnbError, match="too long"):
        lnb.InferenceContext(gm, 23600)
    c = lnb.InferenceContext(gm, 23600, max_rows=CHUNK)
    assert c.max_rows() == CHUNK
    assert _ingest(c, prompt) == GOLD[0]
    z0 = c.zseq_count()
    _golden_run(c)
    print("long-context golden: %d serial walks in 24 steps" % (c.zseq_count() - z0))
    # the serial walk of every head and step: the same bits
    c.set_attention(512, 1)
    z0 = c.zseq_count()
    _golden_run(c)
    assert c.zseq_count() >= z0 + CFG["n_heads"] * CFG["n_layers"] * 24
    c.close()


def test_capacity_does_not_change_bits(lnb):
    """one prompt on lnb_ctx_create(8400) and on lnb_ctx_create_long(131072, 8192): the constant LDS layout at small T, the lazy body (8000 positions)
    and the eager body (600 positions, T <= 1024)"""
    m = lnb.LlamaTransformer(**BIG).fill_synthetic(777).finalize(FAR)
    for seed, L in ((4000, 8000), (4002, 600)):
        pr = lnb.synth_tokens(seed, L, BIG["vocab_size"])
        res = []
        for long_ in (False, True):
            c = lnb.InferenceContext(m, FAR, max_rows=8192) if long_ else lnb.InferenceContext(m, 8400)
            assert c.max_rows() == (8192 if long_ else 8400)
            _, first = c.Forward(pr, 0, want_logits=False)
            toks, _ = c.decode_greedy(first, L, 24)
            kv = [(c.CacheK(l)[L:L + 24].copy(), c.CacheV(l)[L:L + 24].copy()) for l in range(BIG["n_layers"])]
            res.append((first, [int(t) for t in toks], kv))
            c.close()
        assert res[0][0] == res[1][0] and res[0][1] == res[1][1], L
        assert len(set(res[0][1])) > 4, L
        for l in range(BIG["n_layers"]):
            assert np.array_equal(res[0][2][l][0], res[1][2][l][0]) and np.array_equal(res[0][2][l][1], res[1][2][l][1]), (L, l)
    m.close()


def test_far_end_two_kernels_agree_up_to_position_131071(lnb, gm):
    """131040 positions of prefix, then 16 rows: one causal 16-row append on the matrix cores against 16 one-token steps on the scores + lazy-PV pair;
    both continue identically to the last position of the cache, and the step behind it is refused"""
    n_pre, rows = FAR - 32, 16
    toks = lnb.synth_tokens(4100, n_pre + rows, CFG["vocab_size"])
    a = lnb.InferenceContext(gm, FAR, max_rows=CHUNK)
    b = lnb.InferenceContext(gm, FAR, max_rows=CHUNK)
    t0 = time.time()
    _ingest(a, toks[:n_pre]); _ingest(b, toks[:n_pre])
    print("far end: two prefills of %d positions in %.1f s" % (n_pre, time.time() - t0))
    la, na = a.ForwardAppend(toks[n_pre:], n_pre)
    assert a.prefill_attention_form() in (1, 3)
    z0 = b.zseq_count()
    lb = np.empty_like(la)
    for i in range(rows):
        lg, nb = b.Forward([int(toks[n_pre + i])], n_pre + i)
        lb[i] = lg[0]
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)) and na == nb
    assert np.unique(la.view(np.uint32)).size > 100
    walks = b.zseq_count() - z0
    print("far end: %d serial walks in %d one-token steps" % (walks, rows))
    ka, va, kb, vb = a.CacheK(0), a.CacheV(0), b.CacheK(0), b.CacheV(0)
    assert np.array_equal(ka[:n_pre + rows], kb[:n_pre + rows]) and np.array_equal(va[:n_pre + rows], vb[:n_pre + rows])
    assert not ka[n_pre + rows:].any() and not va[n_pre + rows:].any()
    # the same 16 steps with every head walking the reference's serial sum: the same bits (the fallback is expected now and then out here)
    b.set_attention(-1, 1)
    z0 = b.zseq_count()
    for i in range(rows):
        lg, _ = b.Forward([int(toks[n_pre + i])], n_pre + i)
        assert np.array_equal(lg[0].view(np.uint32), lb[i].view(np.uint32)), i
    assert b.zseq_count() >= z0 + CFG["n_heads"] * CFG["n_layers"] * rows
    b.set_attention(-1, 0)
    assert np.array_equal(b.CacheK(0), kb) and np.array_equal(b.CacheV(0), vb)
    # up to the last position of the cache
    left = FAR - (n_pre + rows)
    ta, _ = a.decode_greedy(na, n_pre + rows, left)
    tb, _ = b.decode_greedy(nb, n_pre + rows, left)
    assert [int(t) for t in ta] == [int(t) for t in tb]
    assert np.array_equal(a.CacheK(0), b.CacheK(0)) and np.array_equal(a.CacheV(0), b.CacheV(0))
    with pytest.raises(lnb.LnbError, match=r"beyond the (KV cache of 131072|131072-row RoPE table)"):
        a.decode_greedy(int(ta[-1]), FAR, 1)
    with pytest.raises(lnb.LnbError, match=r"beyond the (KV cache of 131072|131072-row RoPE table)"):
        a.Forward([int(ta[-1])], FAR)
    with pytest.raises(lnb.LnbError, match=r"beyond the (KV cache of 131072|131072-row RoPE table)"):
        a.ForwardAppend([int(ta[-1])] * 16, FAR - 15)
    again, _ = a.decode_greedy(int(ta[-2]), FAR - 1, 1)       # still usable: the last step once more
    assert int(again[0]) == int(ta[-1])
    a.close(); b.close()


def test_batch_and_speculative_decode_on_long_contexts(lnb, gm, prompt):
    """three members of capacity 23600 / 131072 / 64 at positions 23540 / 17000 / 20 in one batch; the speculative loop across position 23552"""
    prompts = [prompt, lnb.synth_tokens(4200, 17000, CFG["vocab_size"]), lnb.synth_tokens(4201, 20, CFG["vocab_size"])]
    make = [lambda: lnb.InferenceContext(gm, 23600, max_rows=CHUNK), lambda: lnb.InferenceContext(gm, FAR, max_rows=CHUNK),
            lambda: lnb.InferenceContext(gm, 64, long_context=True)]
    refs, ctxs, firsts = [], [], []
    for s in range(3):
        r, c = make[s](), make[s]()
        fr, fc = _ingest(r, prompts[s]), _ingest(c, prompts[s])
        assert fr == fc
        toks, _ = r.decode_greedy(fr, len(prompts[s]), 8)
        refs.append(([int(t) for t in toks], r.CacheK(0)[len(prompts[s]):len(prompts[s]) + 8].copy(), r.CacheV(0)[len(prompts[s]):len(prompts[s]) + 8].copy()))
        r.close()
        ctxs.append(c); firsts.append(fc)
    assert firsts[0] == GOLD[0] and refs[0][0] == GOLD[1:9]
    bat = lnb.Batch(ctxs)
    got, _ = bat.decode(firsts, [len(p) for p in prompts], 8)
    assert bat.attention_form() == 1
    for s in range(3):
        L = len(prompts[s])
        assert [int(t) for t in got[s]] == refs[s][0], s
        assert np.array_equal(ctxs[s].CacheK(0)[L:L + 8], refs[s][1]) and np.array_equal(ctxs[s].CacheV(0)[L:L + 8], refs[s][2]), s
    bat.close()
    # speculative decode on the golden's context, the golden's tokens as the corpus
    c = ctxs[0]
    c.set_draft(7, 1, 4, np.array(GOLD, dtype=np.int32))
    spec, fin, st, _ = c.decode_speculative_until(prompt, GOLD[0], P, 24)
    assert [int(t) for t in spec] == GOLD[1:] and not fin
    assert st["verify_passes"] > 0 and st["accepted"] > 0 and c.verify_attention_form() == 1
    assert _rows_hash(c.CacheK(0)[P:P + 24]) == G["k_rows_sha256"] and _rows_hash(c.CacheV(0)[P:P + 24]) == G["v_rows_sha256"]
    for c in ctxs:
        c.close()


def test_arguments_and_refusals(lnb, gm):
    L = lnb.lib()
    err = lambda: L.lnb_last_error().decode()
    out, n = C.c_void_p(), C.c_int(0)
    assert L.lnb_ctx_create_long(gm.h, FAR + 1, 0, C.byref(out)) != 0 and "too long" in err() and not out.value
    assert L.lnb_ctx_create_long(gm.h, 10 ** 9, 16, C.byref(out)) != 0 and "too long" in err()
    assert L.lnb_ctx_create_long(None, 64, 0, C.byref(out)) != 0 and "null" in err()
    assert L.lnb_ctx_create_long(gm.h, 64, 0, None) != 0 and "null" in err()
    assert L.lnb_ctx_max_rows(None, C.byref(n)) != 0 and "null" in err()
    # the model's RoPE table must reach seq_len
    small = lnb.LlamaTransformer(**CFG).fill_synthetic(G["weights_seed"]).finalize()          # 2 * max_seq_len = 24576 rows
    assert L.lnb_ctx_create_long(small.h, 24577, 0, C.byref(out)) != 0 and "rope_rows" in err() and "lnb_model_finalize" in err()
    assert L.lnb_ctx_create_long(small.h, 24576, 16, C.byref(out)) == 0 and out.value
    assert L.lnb_ctx_max_rows(out, None) != 0 and "null" in err()
    assert L.lnb_ctx_max_rows(out, C.byref(n)) == 0 and n.value == 16
    assert L.lnb_ctx_destroy(out) == 0
    small.close()
    # lnb_ctx_create keeps its cap and its message; max_rows <= 0 or beyond seq_len means seq_len
    assert L.lnb_ctx_create(gm.h, 23553, C.byref(out)) != 0 and "too long" in err()
    assert L.lnb_ctx_create(gm.h, 23552, C.byref(out)) == 0 and L.lnb_ctx_max_rows(out, C.byref(n)) == 0 and n.value == 23552
    assert L.lnb_ctx_destroy(out) == 0
    for mr, want in ((0, 300), (-5, 300), (301, 300), (300, 300), (1, 1)):
        assert L.lnb_ctx_create_long(gm.h, 300, mr, C.byref(out)) == 0 and L.lnb_ctx_max_rows(out, C.byref(n)) == 0 and n.value == want, mr
        assert L.lnb_ctx_destroy(out) == 0
    # a call of more rows than the buffers hold is refused up front, by every entry point that takes rows; the context stays usable
    V = CFG["vocab_size"]
    c = lnb.InferenceContext(gm, 400, max_rows=32)
    ref = lnb.InferenceContext(gm, 400)
    toks = lnb.synth_tokens(4300, 66, V)
    for call in (lambda: c.Forward(toks[:33], 0), lambda: c.ForwardAppend(toks[:33], 0), lambda: c.score(toks[:33], 0, toks[1:34]),
                 lambda: c.score_append(toks[:33], 0, toks[1:34]), lambda: c.ForwardAppend(toks[:66], 0)):
        with pytest.raises(lnb.LnbError, match=r"(33|66) rows.*hold 32 rows"):
            call()
    assert L.lnb_forward_stage_begin(c.h, lnb._p(np.ascontiguousarray(toks[:33], dtype=np.int32)), 33, 0, 1) != 0 and "33 rows" in err() and "32 rows" in err()
    lg, first = c.Forward(toks[:32], 0)
    lr, first_ref = ref.Forward(toks[:32], 0)
    assert np.array_equal(lg.view(np.uint32), lr.view(np.uint32)) and first == first_ref
    lg2, nxt = c.ForwardAppend(toks[32:64], 32)
    lr2, nxt_ref = ref.ForwardAppend(toks[32:64], 32)
    assert np.array_equal(lg2.view(np.uint32), lr2.view(np.uint32)) and nxt == nxt_ref
    assert [int(t) for t in c.decode_greedy(nxt, 64, 8)[0]] == [int(t) for t in ref.decode_greedy(nxt_ref, 64, 8)[0]]
    c.close(); ref.close()


@pytest.mark.parametrize("form", ["one_launch", "eager_everywhere"])
def test_forms_that_cannot_stage_the_context_run_the_default_pair(lnb, gm, prompt, monkeypatch, form):
    """beyond lnb_ctx_create's capacity the one-launch form (flag 8) and LNB_ATTN_LAZY=0 cannot stage the context in the LDS: the default pair runs"""
    if form == "eager_everywhere":
        monkeypatch.setenv("LNB_ATTN_LAZY", "0")
    c = lnb.InferenceContext(gm, 24000, max_rows=CHUNK)
    if form == "one_launch":
        c.set_attention(-1, 8)
    assert _ingest(c, prompt) == GOLD[0]
    for k, s in enumerate(G["steps"]):
        lg, nxt = c.Forward([GOLD[k]], P + k)
        assert _row_hash(lg[0]) == s["logits_sha256"] and nxt == GOLD[k + 1], (form, k)
    c.close()
    c = lnb.InferenceContext(gm, 24000, max_rows=CHUNK)      # ... and through the captured graph
    if form == "one_launch":
        c.set_attention(-1, 8)
    assert _ingest(c, prompt) == GOLD[0]
    toks, _ = c.decode_greedy(GOLD[0], P, 4)
    assert [int(t) for t in toks] == GOLD[1:5]
    c.close()
