"""Long-context attention in batched and speculative decode (-m gpu): the chip-wide scores / PV pair with the sequences as a grid dimension
(lnb_batch_set_attention, lnb_ctx_set_batched_attention).  Every comparison is bit-exact.  References: the CPU oracle at small T, and the
single-sequence path (Forward + decode_greedy, pinned to the oracle by the rest of the suite) where the oracle would be slow.
Shapes cross the kernels' boundaries: 256 positions per scores block, 512 per PV batch (and the eager / lazy PV switch at 1024 beyond the cap),
the column / groups / rows output layouts, members of unequal capacity, the LDS cap of the one-workgroup kernels."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

CFGS = {                                                     # the shapes of tests/test_gpu_batch.py
    "tiny_hd64": dict(orc.TINY),
    "tiny_hd128": dict(orc.TINY, n_heads=2, n_kv_heads=1),
    "h8kv2_hd128": dict(orc.TINY, dim=1024, n_heads=8, n_kv_heads=2),
}
STEPS = 11
# (prompt length, capacity of the member): 250 -> 261 crosses 255 -> 257, 505 -> 516 crosses 511 -> 513, 20 stays below 256 (its later blocks
# return at once); three different capacities = three different K strides in one batch
POOL = [(250, 300), (505, 530), (20, 640)]
N_REF = STEPS + 4
N_SPEC = 40                                                  # the speculative test continues pool prompt 0 further (across position 256)


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


_ORACLE = {}


def oracle_pool(name):
    """per config, once: tokens and K / V rows of the oracle's own run of every pool prompt"""
    if name not in _ORACLE:
        cfg = CFGS[name]
        om = orc.Model(**cfg).fill_synthetic(606).finalize()
        rows = []
        for i, (plen, _) in enumerate(POOL):
            prompt = orc.synth_tokens(7000 + i, plen, cfg["vocab_size"])
            n_out = N_SPEC + 1 if i == 0 else N_REF
            oc = orc.Context(om, plen + n_out + 2)
            r, _ = oc.generate(prompt, n_out)
            kv = [(oc.cache(l, 0).copy(), oc.cache(l, 1).copy()) for l in range(cfg["n_layers"])]
            oc.close()
            rows.append((prompt, [int(t) for t in r], kv))
        om.close()
        _ORACLE[name] = rows
    return _ORACLE[name]


def _assert_kv(ctx, kv, T, tag):
    for layer, (k, v) in enumerate(kv):
        assert np.array_equal(ctx.CacheK(layer)[:T], k[:T]), tag + (layer, "K")
        assert np.array_equal(ctx.CacheV(layer)[:T], v[:T]), tag + (layer, "V")


@pytest.mark.parametrize("copy", [True, False], ids=["columns", "rows"])
@pytest.mark.parametrize("name", sorted(CFGS))
def test_forced_long_form_equals_the_oracle_per_sequence(lnb, name, copy):
    cfg = CFGS[name]
    pool = oracle_pool(name)
    gm = lnb.LlamaTransformer(**cfg).fill_synthetic(606).finalize()
    if copy:
        gm.enable_batch()
    for n in (1, 2, 5, 16, 17, 40):
        idx = [s % len(POOL) for s in range(n)]
        plens = [POOL[i][0] for i in idx]
        ctxs = [lnb.InferenceContext(gm, POOL[i][1]) for i in idx]
        firsts = [ctxs[s].Forward(pool[idx[s]][0], 0, want_logits=False)[1] for s in range(n)]
        assert firsts == [pool[i][1][0] for i in idx]
        b = lnb.Batch(ctxs)
        assert b.attention_form() == 0
        b.set_attention(0, 0)
        got, _ = b.decode(firsts, plens, STEPS)
        assert b.attention_form() == 1
        for s in range(n):
            ref = pool[idx[s]][1]
            assert [int(t) for t in got[s]] == ref[1:1 + STEPS], (name, n, s)
            _assert_kv(ctxs[s], pool[idx[s]][2], plens[s] + STEPS, (name, n, s))
        # a second call on the same batch continues where the first stopped
        more, _ = b.decode([pool[idx[s]][1][STEPS] for s in range(n)], [plens[s] + STEPS for s in range(n)], 1)
        assert b.attention_form() == 1
        for s in range(n):
            assert int(more[s][0]) == pool[idx[s]][1][STEPS + 1], (name, n, s)
        # back to the one-workgroup kernels: the next 2 steps still match
        b.set_attention(10 ** 9, 0)
        last, _ = b.decode([pool[idx[s]][1][STEPS + 1] for s in range(n)], [plens[s] + STEPS + 1 for s in range(n)], 2)
        assert b.attention_form() == 0
        for s in range(n):
            assert [int(t) for t in last[s]] == pool[idx[s]][1][STEPS + 2:STEPS + 4], (name, n, s)
            _assert_kv(ctxs[s], pool[idx[s]][2], plens[s] + STEPS + 3, (name, n, s, "after the switch back"))
        b.close()
        for c in ctxs:
            c.close()
    gm.close()


def test_forced_serial_sum_in_the_batched_long_form(lnb):
    """force_zseq: every (sequence, head) walks the reference's serial sum (counted), same tokens and rows"""
    name = "tiny_hd128"
    cfg, pool = CFGS[name], oracle_pool(name)
    gm = lnb.LlamaTransformer(**cfg).fill_synthetic(606).finalize().enable_batch()
    n = 5
    idx = [s % len(POOL) for s in range(n)]
    ctxs = [lnb.InferenceContext(gm, POOL[i][1]) for i in idx]
    firsts = [ctxs[s].Forward(pool[idx[s]][0], 0, want_logits=False)[1] for s in range(n)]
    b = lnb.Batch(ctxs).set_attention(0, 1)
    before = ctxs[0].zseq_count()
    got, _ = b.decode(firsts, [POOL[i][0] for i in idx], STEPS)
    assert b.attention_form() == 1
    assert ctxs[0].zseq_count() >= before + n * cfg["n_heads"] * cfg["n_layers"] * STEPS
    for s in range(n):
        assert [int(t) for t in got[s]] == pool[idx[s]][1][1:1 + STEPS], s
        _assert_kv(ctxs[s], pool[idx[s]][2], POOL[idx[s]][0] + STEPS, (s,))
    b.close()
    for c in ctxs:
        c.close()
    gm.close()


# ---- beyond what the one-workgroup kernels stage in the LDS --------------------------------------------------------------------------
SL, P = 8400, 8000
BIG = dict(orc.TINY, n_heads=2, n_kv_heads=1, max_seq_len=4224)      # tiny_hd128 with a RoPE table of 8448 rows


@pytest.fixture(scope="module")
def big(lnb):
    """the single-sequence reference beyond the cap, once: prompts of 8000 / 7990 / 300 / 9 / 23 tokens, their greedy continuation and rows"""
    gm = lnb.LlamaTransformer(**BIG).fill_synthetic(777).finalize()
    lens = [P, P - 10, 300, 9, 23]
    prompts = [lnb.synth_tokens(4000 + i, L, BIG["vocab_size"]) for i, L in enumerate(lens)]
    refs = []
    for pr, L in zip(prompts, lens):
        c = lnb.InferenceContext(gm, SL if L >= 300 else 64)
        _, first = c.Forward(pr, 0, want_logits=False)
        toks, _ = c.decode_greedy(first, L, 24)
        kv = [(c.CacheK(l)[L:L + 24].copy(), c.CacheV(l)[L:L + 24].copy()) for l in range(BIG["n_layers"])]
        c.close()
        refs.append((first, [int(t) for t in toks], kv))
    yield gm, prompts, lens, refs
    gm.close()


def _new_rows_equal(ctx, L, kv, rows, tag):
    for layer, (k, v) in enumerate(kv):
        assert np.array_equal(ctx.CacheK(layer)[L:L + rows], k[:rows]), tag + (layer, "K")
        assert np.array_equal(ctx.CacheV(layer)[L:L + rows], v[:rows]), tag + (layer, "V")


def test_batch_beyond_the_cap_equals_single_sequence_runs(lnb, big):
    gm, prompts, lens, refs = big
    ctxs = [lnb.InferenceContext(gm, SL) for _ in range(3)]
    for s in range(3):
        assert ctxs[s].Forward(prompts[s], 0, want_logits=False)[1] == refs[s][0]
    b = lnb.Batch(ctxs)                                      # (refused before the long form existed)
    got, _ = b.decode([refs[s][0] for s in range(3)], lens[:3], 8)
    assert b.attention_form() == 1
    for s in range(3):
        assert [int(t) for t in got[s]] == refs[s][1][:8], s
        _new_rows_equal(ctxs[s], lens[s], refs[s][2], 8, (s,))
    b.close()
    for c in ctxs:
        c.close()


def test_groups_batch_of_17_beyond_the_cap(lnb, big):
    """17 sequences on a model with the matrix-core copy: two column groups, the attention writes the B-operand layout per group"""
    _, prompts, lens, refs = big
    gm = lnb.LlamaTransformer(**BIG).fill_synthetic(777).finalize().enable_batch()
    which = [0, 1, 2] + [3 + (s % 2) for s in range(14)]
    ctxs = [lnb.InferenceContext(gm, SL if lens[w] >= 300 else 64) for w in which]
    for c, w in zip(ctxs, which):
        assert c.Forward(prompts[w], 0, want_logits=False)[1] == refs[w][0]
    b = lnb.Batch(ctxs)
    got, _ = b.decode([refs[w][0] for w in which], [lens[w] for w in which], 8)
    assert b.attention_form() == 1
    for s, w in enumerate(which):
        assert [int(t) for t in got[s]] == refs[w][1][:8], s
        _new_rows_equal(ctxs[s], lens[w], refs[w][2], 8, (s,))
    b.close()
    for c in ctxs:
        c.close()
    gm.close()


@pytest.mark.parametrize("corpus_kind", ["exact", "wrong_after_3"])
def test_speculative_decode_beyond_the_cap_equals_greedy(lnb, big, corpus_kind):
    gm, prompts, lens, refs = big
    first, toks, kv = refs[0]
    corpus = np.array(toks, dtype=np.int32)
    if corpus_kind == "wrong_after_3":                       # rejected columns write stale rows that must be overwritten
        corpus[3:] = (corpus[3:] + 1) % BIG["vocab_size"]
    c = lnb.InferenceContext(gm, SL)
    assert c.Forward(prompts[0], 0, want_logits=False)[1] == first
    c.set_draft(7, 1, 4, corpus)
    got, fin, st, _ = c.decode_speculative_until(prompts[0], first, P, 24)     # (refused before the long form existed)
    assert [int(t) for t in got] == toks and not fin
    assert st["verify_passes"] > 0 and c.verify_attention_form() == 1
    if corpus_kind == "exact":
        assert st["accepted"] > 0
    _new_rows_equal(c, P, kv, 24, (corpus_kind,))
    c.close()


@pytest.mark.parametrize("copy", [True, False], ids=["columns", "rows"])
def test_speculative_forced_long_form_equals_the_oracle(lnb, copy):
    cfg = CFGS["tiny_hd128"]
    prompt, ref, okv = oracle_pool("tiny_hd128")[0]          # 250 tokens, then N_SPEC + 1 of the oracle's
    assert len(prompt) == 250 and len(ref) == N_SPEC + 1
    gm = lnb.LlamaTransformer(**cfg).fill_synthetic(606).finalize()
    if copy:
        gm.enable_batch()
    c = lnb.InferenceContext(gm, 300).set_batched_attention(0, 0)
    assert c.Forward(prompt, 0, want_logits=False)[1] == ref[0]
    c.set_draft(7, 1, 4, ref)
    got, fin, st, _ = c.decode_speculative_until(prompt, ref[0], 250, 40)      # crosses position 256
    assert [int(t) for t in got] == ref[1:] and not fin
    assert st["verify_passes"] > 0 and st["accepted"] > 0 and c.verify_attention_form() == 1
    _assert_kv(c, okv, 250 + 40, ("spec",))
    # the serial sum in a verify pass, then the short form again on the same context: the same tokens
    for thr, fz, form in ((0, 1, 1), (10 ** 9, 0, 0)):
        c.set_batched_attention(thr, fz)
        z0 = c.zseq_count()
        got, _, st, _ = c.decode_speculative_until(prompt, ref[0], 250, 40)
        assert [int(t) for t in got] == ref[1:] and c.verify_attention_form() == form
        assert (c.zseq_count() > z0) == bool(fz)
    c.close(); gm.close()


def test_stop_ids_and_frozen_sequences_under_the_long_form(lnb):
    """a member hits a stop id mid-run; the next chunk passes it with start_pos < 0: counts, flags, tokens and caches as in the short form"""
    name = "tiny_hd128"
    cfg, pool = CFGS[name], oracle_pool(name)
    gm = lnb.LlamaTransformer(**cfg).fill_synthetic(606).finalize().enable_batch()
    idx = [0, 1, 2]
    out1 = pool[1][1][1:]                                    # sequence 1 stops at the first token of its run that did not occur earlier in it
    j = next(i for i in range(2, 8) if out1[i] not in out1[:i])
    res = {}
    for form in (0, 1):
        ctxs = [lnb.InferenceContext(gm, POOL[i][1]) for i in idx]
        firsts = [ctxs[s].Forward(pool[i][0], 0, want_logits=False)[1] for s, i in enumerate(idx)]
        ctxs[1].set_stop_ids([out1[j]])
        b = lnb.Batch(ctxs)
        if form:
            b.set_attention(0, 0)
        toks, _ = b.decode_until(firsts, [POOL[i][0] for i in idx], 8)
        fin = list(b.finished)
        assert b.attention_form() == form
        assert [len(t) for t in toks] == [8, j + 1, 8] and fin == [False, True, False]
        frozen_kv = [(ctxs[1].CacheK(l).copy(), ctxs[1].CacheV(l).copy()) for l in range(cfg["n_layers"])]
        pos = [POOL[0][0] + 8, -1, POOL[2][0] + 8]
        toks2, _ = b.decode_until([int(toks[0][-1]), 0, int(toks[2][-1])], pos, 3)
        assert b.attention_form() == form
        assert [len(t) for t in toks2] == [3, 0, 3] and list(b.finished) == [False, True, False]
        for l, (k, v) in enumerate(frozen_kv):
            assert np.array_equal(ctxs[1].CacheK(l), k) and np.array_equal(ctxs[1].CacheV(l), v), (form, l)
        for s in (0, 2):
            want = pool[idx[s]][1]
            assert [int(t) for t in toks[s]] + [int(t) for t in toks2[s]] == want[1:12], (form, s)
        assert [int(t) for t in toks[1]] == out1[:j + 1]
        res[form] = ([list(map(int, t)) for t in toks + toks2], fin)
        b.close()
        for c in ctxs:
            c.close()
    assert res[0] == res[1]
    gm.close()


def test_attention_setters_check_arguments_and_lifetime(lnb):
    import ctypes as C
    L = lnb.lib()
    n = C.c_int(0)
    err = lambda: L.lnb_last_error().decode()
    assert L.lnb_batch_set_attention(None, 0, 0) != 0 and "null" in err()
    assert L.lnb_ctx_set_batched_attention(None, 0, 0) != 0 and "null" in err()
    assert L.lnb_batch_set_attention(None, 0, 2) != 0 and "force_zseq" in err()      # arguments before the handle
    assert L.lnb_ctx_set_batched_attention(None, 0, -1) != 0 and "force_zseq" in err()
    assert L.lnb_batch_attention_form(None, C.byref(n)) != 0 and L.lnb_ctx_verify_attention_form(None, C.byref(n)) != 0
    cfg = CFGS["tiny_hd64"]
    gm = lnb.LlamaTransformer(**cfg).fill_synthetic(606).finalize()
    ctxs = [lnb.InferenceContext(gm, 64) for _ in range(2)]
    b = lnb.Batch(ctxs)
    assert L.lnb_batch_attention_form(b.h, None) != 0 and L.lnb_ctx_verify_attention_form(ctxs[0].h, None) != 0
    with pytest.raises(lnb.LnbError):
        b.set_attention(0, 4)
    assert b.set_attention(-1, 0).attention_form() == 0 and ctxs[0].verify_attention_form() == 0
    with pytest.raises(lnb.LnbError):                        # a member cannot go while the batch lives
        ctxs[0].close()
    b.close()
    with pytest.raises(lnb.LnbError):                        # a destroyed batch: its handle is gone
        b.set_attention(0, 0)
    with pytest.raises(lnb.LnbError):
        b.attention_form()
    for c in ctxs:
        c.close()
    with pytest.raises(lnb.LnbError):
        ctxs[0].set_batched_attention(0, 0)
    gm.close()


def test_setters_are_refused_while_a_member_is_inside_a_stage_call(lnb):
    """a lnb_forward_stage_begin that has not been ended on a member: both setters refuse; after the end they succeed"""
    import ctypes as C
    L = lnb.lib()
    cfg = CFGS["tiny_hd64"]
    gm = lnb.LlamaTransformer(**cfg).fill_synthetic(606).finalize()
    ctxs = [lnb.InferenceContext(gm, 64) for _ in range(2)]
    b = lnb.Batch(ctxs)
    toks = np.ascontiguousarray(orc.synth_tokens(11, 20, cfg["vocab_size"]), dtype=np.int32)
    lnb._chk(L.lnb_forward_stage_begin(ctxs[1].h, lnb._p(toks), 20, 0, 1))
    with pytest.raises(lnb.LnbError, match="has not been ended"):
        b.set_attention(0, 0)
    with pytest.raises(lnb.LnbError, match="has not been ended"):
        ctxs[1].set_batched_attention(0, 0)
    got = C.c_int32(-2)
    lnb._chk(L.lnb_forward_stage_end(ctxs[1].h, C.byref(got)))
    b.set_attention(0, 0)
    ctxs[1].set_batched_attention(0, 0)
    assert b.attention_form() == 0 and ctxs[1].verify_attention_form() == 0      # nothing has run yet
    b.close()
    for c in ctxs:
        c.close()
    gm.close()


def test_long_form_through_batched_ticks_and_the_profile_call(lnb):
    """lnb_batch_set_state applies the rule for the ticks that follow (a graph of its own per form); lnb_batch_profile_kernel applies it to pos.
    The ticks' tokens and K / V rows equal the oracle's, in the long form, after a switch back to the short form, and in the long form again."""
    name = "tiny_hd128"
    cfg, pool = CFGS[name], oracle_pool(name)
    gm = lnb.LlamaTransformer(**cfg).fill_synthetic(606).finalize().enable_batch()
    n = 3
    ctxs = [lnb.InferenceContext(gm, POOL[s][1]) for s in range(n)]
    firsts = [ctxs[s].Forward(pool[s][0], 0, want_logits=False)[1] for s in range(n)]
    plens = [POOL[s][0] for s in range(n)]
    b = lnb.Batch(ctxs)
    pipe = lnb.Pipeline(gm, 0, 1, None)
    done = 0
    for thr, form, steps in ((0, 1, 8), (10 ** 9, 0, 2), (0, 1, 2)):
        b.set_attention(thr, 0)
        b.set_state([pool[s][1][done] for s in range(n)], [plens[s] + done for s in range(n)])
        slots = [pipe.tick_batch(run=b) for _ in range(steps)]
        pipe.sync(); b.check_error()
        assert b.attention_form() == form
        for i, q in enumerate(slots):
            assert [int(t) for t in pipe.read_tokens(q, n)] == [pool[s][1][done + i + 1] for s in range(n)], (thr, i)
        done += steps
    for s in range(n):
        _assert_kv(ctxs[s], pool[s][2], plens[s] + done, (s,))
    # the measurement call: long above the threshold, short below it (it overwrites row `pos`: the contexts are not used afterwards)
    b.set_attention(100, 0)
    assert b.profile_kernel(1, 200, 2) > 0 and b.attention_form() == 1
    assert b.profile_kernel(1, 50, 2) > 0 and b.attention_form() == 0
    pipe.close(); b.close()
    for c in ctxs:
        c.close()
    gm.close()
