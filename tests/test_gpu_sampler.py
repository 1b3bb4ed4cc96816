"""Seeded temperature / top-k / top-p sampling on the MI355X (include/lnb.h): the sampled token is a pure function of the logits row, the sampler and the
position, on integers behind the exp table -- so the kernel is compared bit for bit with tests/sampler_ref.py (tokens and every info field), and a whole
sampled generation with the chain "oracle one-token step, sampler_ref, feed the token"."""
import ctypes

import numpy as np
import pytest

from form_tally import ran
from oracle import oracle as orc
import sampler_ref as sr

pytestmark = pytest.mark.gpu

SAMPLERS = ((1.0, 0, 1.0), (0.7, 40, 0.9), (1.5, 0, 0.5), (1.0, 1, 1.0))     # the table of the issue; (temperature, top_k, top_p)
SEED, P0, STEPS, SEQ = 777, 8, 24, 64


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


def op_check(lnb, rows, cases):
    """cases: (row, (t, k, p), seed, pos, u or None): lnb.op_sample on them against the restatement -- tokens and every info field"""
    preps = {}
    for at in range(0, len(cases), 256):
        part = cases[at:at + 256]
        x = np.stack([rows[c[0]] for c in part])
        smp = [c[1] + (c[2],) for c in part]
        pos = [c[3] for c in part]
        if any(c[4] is not None for c in part):
            tok, info = lnb.op_sample(x, smp, pos, draws=[sr.draw(c[2], c[3]) if c[4] is None else c[4] for c in part])
        else:
            tok, info = lnb.op_sample(x, smp, pos)
        for i, (r, tkp, seed, p, u) in enumerate(part):
            if (r, tkp) not in preps:
                preps[(r, tkp)] = sr.prepare(rows[r], *tkp)
            prep = preps[(r, tkp)]
            assert info[i] == prep[3], (r, tkp, info[i], prep[3])
            want = sr.pick(prep, sr.draw(seed, p) if u is None else u)
            assert tok[i] == want, (r, tkp, seed, p, u, int(tok[i]), want)
    return preps


# ---- 1. the operator, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1001, 1024, 128256])
def test_op_sample_equals_the_restatement_over_the_grid(lnb, V):
    rows = sr.llama_like_rows(np.random.default_rng(20261019 + V), 64, V)
    cases = []
    for n, (r, tkp) in enumerate(sr.grid_cases(V)):
        for j in range(3):                                                   # every position and every seed on every grid point
            cases.append((r, tkp, sr.SEEDS[(n + j) % 3], sr.POSITIONS[j], None))
    with ran(lnb, "sample.row"):
        preps = op_check(lnb, rows, cases)
    kept = [p[3]["n_kept"] for p in preps.values()]
    assert min(kept) == 1 and max(kept) > V // 2                            # from one entry to most of the row


# ---- 2. crafted rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1001, 128256])
def test_op_sample_on_the_crafted_rows(lnb, V):
    crafted = sr.crafted(V)
    rows = np.stack([c[1] for c in crafted])
    cases, checks = [], []
    for r, (name, row, tkp, check, boundaries) in enumerate(crafted):
        for seed, pos in ((0, 0), (777, 8), (12345, 131071)):
            cases.append((r, tkp, seed, pos, None)); checks.append((name, check))
        for u in (sr.boundary_draws(sr.prepare(row, *tkp)) if boundaries else []):
            cases.append((r, tkp, 0, 0, u)); checks.append((name, check))
    op_check(lnb, rows, cases)
    x = np.stack([rows[c[0]] for c in cases])
    tok, info = lnb.op_sample(x, [c[1] + (c[2],) for c in cases], [c[3] for c in cases], draws=[sr.draw(c[2], c[3]) if c[4] is None else c[4] for c in cases])
    for (name, check), t, i, c in zip(checks, tok, info, cases):
        if check:
            check(int(t), i, rows[c[0]])


def test_op_sample_on_the_all_equal_row_of_131072_entries(lnb):
    """the 63-bit bound: every weight just under 2^46, their sum just under 2^63"""
    V = 131072
    rows = np.full((1, V), sr.bf(0.6875), dtype=np.uint16)
    cases = [(0, (1.0, 0, 1.0), 1, 5, None), (0, (1.0, 0, 0.9), 2, 6, None), (0, (1.0, 0, 1.0), 0, 0, sr.MASK), (0, (1.0, 0, 1.0), 0, 0, 0), (0, (1.0, 70000, 0.5), 3, 7, None)]
    preps = op_check(lnb, rows, cases)
    w = int(np.floor(np.ldexp(sr.exp_table()[sr.bf(0.6875)], 45)))
    assert preps[(0, (1.0, 0, 1.0))][3]["w_all"] == V * w and 2 ** 62 < V * w < 2 ** 63


# ---- 3. the tiny model against the oracle ------------------------------------------------------------------------------------------------
def oracle_chain(om, prompt, smp, seed, steps, seq_len=SEQ):
    """oracle one-token step, sampler_ref, feed the token: what lnb_decode_sample_until(first, len(prompt), steps) must emit
    -> (the prompt's argmax, the sampled tokens, how many of them are their row's argmax, the oracle context)"""
    c = orc.Context(om, seq_len)
    row, first = c.forward(prompt, 0)
    row, tok, toks, greedy = row[-1], first, [], 0
    for i in range(steps):
        row, _ = c.forward(np.array([tok], dtype=np.int32), len(prompt) + i)
        r16 = orc.f32_to_bf16(np.ascontiguousarray(row[-1], dtype=np.float32))
        tok, _ = sr.sample(r16, smp + (seed,), pos=len(prompt) + i)
        greedy += tok == sr.argmax(r16)
        toks.append(tok)
    return first, np.array(toks, dtype=np.int32), greedy, c


@pytest.fixture(scope="module")
def tiny(lnb):
    cfg = dict(orc.TINY)
    om = orc.Model(**cfg).fill_synthetic(1234).finalize()
    prompt = lnb.synth_tokens(99, 8, cfg["vocab_size"])
    chains = {}
    for smp in SAMPLERS:
        first, toks, greedy, oc = oracle_chain(om, prompt, smp, SEED, STEPS)
        kv = [(oc.cache(l, 0)[:P0 + STEPS].copy(), oc.cache(l, 1)[:P0 + STEPS].copy()) for l in range(cfg["n_layers"])]
        chains[smp] = (first, toks, greedy, kv)
        oc.close()
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize()
    yield gm, om, prompt, chains, cfg
    gm.close(); om.close()


def fresh(lnb, gm, prompt, seq_len=SEQ):
    c = lnb.InferenceContext(gm, seq_len)
    _, first = c.Forward(prompt, 0, want_logits=False)
    return c, first


@pytest.mark.parametrize("no_graph", [False, True])
def test_tiny_sampled_generation_equals_the_oracle_chain(lnb, tiny, monkeypatch, no_graph):
    gm, _, prompt, chains, cfg = tiny
    if no_graph:
        monkeypatch.setenv("LNB_NO_GRAPH", "1")
    for smp in SAMPLERS[:3]:
        first, want, greedy, kv = chains[smp]
        assert greedy <= 8                                                   # a kernel that silently stayed greedy cannot pass
        c, f = fresh(lnb, gm, prompt)
        assert f == first
        with ran(lnb, "sample.row"):
            got, fin, _ = c.decode_sample_until(smp + (SEED,), f, P0, STEPS)
        assert (got == want).all() and not fin, (smp, got, want)
        for l in range(cfg["n_layers"]):                                     # rows 0 .. P0 + STEPS - 1: the last sampled token is not fed
            assert (c.CacheK(l)[:P0 + STEPS] == kv[l][0]).all() and (c.CacheV(l)[:P0 + STEPS] == kv[l][1]).all(), (smp, l)
        c.close()


def test_tiny_chunking_greedy_equivalents_and_graph_reuse(lnb, tiny):
    gm, _, prompt, chains, _ = tiny
    # one call of 24 steps equals three calls of 8
    smp = SAMPLERS[1]
    first, want, _, _ = chains[smp]
    c, f = fresh(lnb, gm, prompt)
    parts, tok = [], f
    for k in range(3):
        got, fin, _ = c.decode_sample_until(smp + (SEED,), tok, P0 + 8 * k, 8)
        parts.append(got); tok = int(got[-1])
    assert (np.concatenate(parts) == want).all()
    c.close()
    # temperature 0 and top_k 1 both equal decode_greedy_until
    g, f = fresh(lnb, gm, prompt)
    greedy, _, _ = g.decode_greedy_until(f, P0, STEPS)
    g.close()
    for s in ((0.0, 40, 0.5, 1), (1.0, 1, 1.0, 2), (0.7, 1, 0.3, 3)):
        c, f = fresh(lnb, gm, prompt)
        got, fin, _ = c.decode_sample_until(s, f, P0, STEPS)
        assert (got == greedy).all() and not fin, s
        c.close()
    assert (chains[SAMPLERS[3]][1] == greedy).all()
    # a greedy call after a sampling call on the same context gives the greedy tokens; another sampler needs no recapture and gives its own chain
    c, f = fresh(lnb, gm, prompt)
    got, _, _ = c.decode_sample_until(SAMPLERS[0] + (SEED,), f, P0, STEPS)
    assert (got == chains[SAMPLERS[0]][1]).all()
    again, _, _ = c.decode_greedy_until(f, P0, STEPS)
    assert (again == greedy).all()
    lnb.form_count_reset()
    got, _, _ = c.decode_sample_until(SAMPLERS[2] + (SEED,), f, P0, STEPS)
    assert (got == chains[SAMPLERS[2]][1]).all()
    assert lnb.form_count("sample.row") == 0 and not lnb.form_count("rowcast_lds") and not lnb.form_count("gemv_chain.rw56")      # replays only: nothing was launched eagerly or captured
    again, _, _ = c.decode_greedy_until(f, P0, STEPS)
    assert (again == greedy).all()
    c.close()


def test_tiny_a_stop_id_the_chain_produces_ends_the_run(lnb, tiny):
    gm, _, prompt, chains, _ = tiny
    smp = SAMPLERS[0]
    _, want, _, _ = chains[smp]
    stop = int(want[5])
    n = int(np.nonzero(want == stop)[0][0]) + 1
    c, f = fresh(lnb, gm, prompt)
    c.set_stop_ids([stop])
    got, fin, _ = c.decode_sample_until(smp + (SEED,), f, P0, STEPS)
    assert fin and (got == want[:n]).all() and got[-1] == stop
    c.close()


# ---- 4. the batch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 17])
@pytest.mark.parametrize("copy", [False, True])
def test_batch_members_equal_their_own_single_context_runs(lnb, n, copy):
    cfg = dict(orc.TINY)
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize()
    if copy:
        gm.enable_batch()
    steps, V = 12, cfg["vocab_size"]
    plen = [(5, 8, 11)[s % 3] for s in range(n)]
    prompts = [lnb.synth_tokens(300 + s, plen[s], V) for s in range(n)]
    smps = [((1.0, 0, 1.0), (0.7, 40, 0.9), (1.5, 0, 0.5), (0.25, 2, 1.0))[s % 4] + (1000 + 7 * s,) for s in range(n)]
    smps[1] = (0.0, 5, 0.5, 9)                                               # a greedy member
    # every member alone, first without stop ids (to learn a token its chain produces), member 2 then again with one
    want, fins, stop = [], [], None
    for s in range(n):
        c, f = fresh(lnb, gm, prompts[s])
        got, fin, _ = c.decode_sample_until(smps[s], f, plen[s], steps)
        c.close()
        if s == 2:
            stop = int(got[4])
            c, f = fresh(lnb, gm, prompts[s])
            c.set_stop_ids([stop])
            got, fin, _ = c.decode_sample_until(smps[s], f, plen[s], steps)
            c.close()
            assert fin and len(got) <= 5 and got[-1] == stop
        want.append(got); fins.append(fin)
    g, f = fresh(lnb, gm, prompts[1])
    greedy, _, _ = g.decode_greedy_until(f, plen[1], steps)
    g.close()
    assert (want[1] == greedy).all() and any((want[s] != want[0][:len(want[s])]).any() for s in range(1, n))
    ctxs, firsts = [], []
    for s in range(n):
        c, f = fresh(lnb, gm, prompts[s])
        ctxs.append(c); firsts.append(f)
    ctxs[2].set_stop_ids([stop])
    bat = lnb.Batch(ctxs)
    with ran(lnb, "sample.batch"):
        got, _ = bat.decode_sample_until(smps, firsts, plen, steps)
    for s in range(n):
        assert len(got[s]) == len(want[s]) and (got[s] == want[s]).all() and bat.finished[s] == fins[s], (s, got[s], want[s])
    # a second chunk: the finished member frozen (start_pos < 0), the others continue their own chains
    pos2 = [-1 if s == 2 else plen[s] + steps for s in range(n)]
    tok2 = [int(got[s][-1]) for s in range(n)]
    more, _ = bat.decode_sample_until(smps, tok2, pos2, 4)
    assert len(more[2]) == 0 and bat.finished[2]
    c, f = fresh(lnb, gm, prompts[0])
    full, _, _ = c.decode_sample_until(smps[0], f, plen[0], steps + 4)
    c.close()
    assert (np.concatenate([got[0], more[0]]) == full).all()
    bat.close()
    for c in ctxs:
        c.close()
    gm.close()


# ---- 5. the full vocabulary through the loop ---------------------------------------------------------------------------------------------
def test_full_vocabulary_head_through_the_loop(lnb):
    """the 8B vocabulary and head shape, one layer: every emitted token is the restatement's on the device's own logits row of that step"""
    cfg = dict(lnb.LLAMA_8B, n_layers=1)
    gm = lnb.LlamaTransformer(**cfg).fill_synthetic(4321).finalize()
    V, P, N = cfg["vocab_size"], 8, 8
    prompt = lnb.synth_tokens(41, P, V)
    for smp in ((1.0, 0, 1.0, 5), (0.7, 40, 0.9, 6)):
        c, f = fresh(lnb, gm, prompt, 32)
        with ran(lnb, "sample.row"):
            got, fin, _ = c.decode_sample_until(smp, f, P, N)
        assert len(got) == N and not fin
        c.close()
        d = lnb.InferenceContext(gm, 32)
        rows, _ = d.Forward(np.concatenate([prompt, [f], got[:N - 1]]).astype(np.int32), 0, want_logits=True)
        d.close()
        greedy = 0
        for i in range(N):
            r16 = orc.f32_to_bf16(np.ascontiguousarray(rows[P + i], dtype=np.float32))
            tok, info = sr.sample(r16, smp, pos=P + i)
            assert tok == got[i], (smp, i, tok, int(got[i]), info)
            greedy += tok == sr.argmax(r16)
        assert greedy < N
    gm.close()


def test_the_generation_engine_samples_every_token_the_prompts_next_one_included(lnb, tiny):
    gm, om, prompt, _, _ = tiny
    smp = (0.7, 40, 0.9, 4242)
    oc = orc.Context(om, SEQ)
    row, greedy_first = oc.forward(prompt, 0)
    want = []
    for i in range(10):                                                      # token i is sampled from the row whose input token sits at position 7 + i
        tok, _ = sr.sample(orc.f32_to_bf16(np.ascontiguousarray(row[-1], dtype=np.float32)), smp, pos=len(prompt) - 1 + i)
        want.append(tok)
        row, _ = oc.forward(np.array([tok], dtype=np.int32), len(prompt) + i)
    oc.close()
    for chunk in (0, 3):
        got = lnb.InferenceEngine(gm, SEQ, sampler=lnb.Sampler(*smp), prefill_chunk=chunk).GenerateTokens(prompt, max_new=10)
        assert got == want, (chunk, got, want)
    assert want[0] != greedy_first                                           # (with this seed the prompt's next token is not the argmax: it was sampled)
    assert lnb.InferenceEngine(gm, SEQ, sampler=smp, stop_token_ids=[want[4]]).GenerateTokens(prompt, max_new=10) == want[:want.index(want[4]) + 1]
    assert lnb.InferenceEngine(gm, SEQ).GenerateTokens(prompt, max_new=3)[0] == greedy_first


def test_profile_sample_times_the_token_launch_alone(lnb, tiny):
    gm, _, prompt, _, _ = tiny
    c, f = fresh(lnb, gm, prompt)
    c.decode_greedy_until(f, P0, 2)                                          # leaves a logits row behind
    with ran(lnb, "sample.row"):
        ms = c.profile_sample((0.7, 40, 0.9, 1), P0, 8)
    assert 0 < ms < 100
    lnb.form_count_reset()
    assert 0 < c.profile_sample(None, P0, 8) < 100 and lnb.form_count("sample.row") == 0      # the argmax launch: no sampler kernel
    for bad, word in (((-1.0, 0, 1.0, 0), "temperature"), ((1.0, 0, 2.0, 0), "top_p")):
        with pytest.raises(lnb.LnbError, match=word):
            c.profile_sample(bad, P0, 8)
    with pytest.raises(lnb.LnbError, match="bad arguments"):
        c.profile_sample(None, P0, 0)
    got, _, _ = c.decode_greedy_until(f, P0, 4)                              # the context is usable afterwards
    g, _ = fresh(lnb, gm, prompt)
    assert (got == g.decode_greedy_until(f, P0, 4)[0]).all()
    c.close(); g.close()


# ---- 6. refusals that need a device -----------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_device(lnb, tiny):
    gm, _, prompt, _, cfg = tiny
    smp = (0.7, 40, 0.9, 1)
    c, f = fresh(lnb, gm, prompt)
    c.set_token_probs(4)
    with pytest.raises(lnb.LnbError, match=r"token probabilities.*lnb_ctx_set_token_probs\(ctx, 0\)"):
        c.decode_sample_until(smp, f, P0, 4)
    d, _ = fresh(lnb, gm, prompt)
    c.set_token_probs(0)
    got, _, _ = c.decode_sample_until(smp, f, P0, 4)                         # switched off: the call goes through
    assert len(got) == 4
    for bad, word in (((-1.0, 0, 1.0, 0), "temperature"), ((1.0, -2, 1.0, 0), "top_k"), ((1.0, 0, 0.0, 0), "top_p")):
        with pytest.raises(lnb.LnbError, match=word):
            c.decode_sample_until(bad, f, P0, 4)
    with pytest.raises(lnb.LnbError, match="exceeds the context length"):
        c.decode_sample_until(smp, f, P0, SEQ + 1)
    with pytest.raises(lnb.LnbError, match="beyond the KV cache"):
        c.decode_sample_until(smp, f, SEQ - 2, 8)
    # a pending lnb_forward_stage_begin
    one = np.array([f], dtype=np.int32)
    lnb._chk(c.L.lnb_forward_stage_begin(c.h, lnb._p(one), 1, P0, 1))
    with pytest.raises(lnb.LnbError, match="lnb_forward_stage_begin has not been ended"):
        c.decode_sample_until(smp, f, P0, 4)
    with pytest.raises(lnb.LnbError, match="lnb_forward_stage_begin has not been ended"):
        c.profile_sample(smp, P0, 4)
    am = ctypes.c_int32(0)
    lnb._chk(c.L.lnb_forward_stage_end(c.h, ctypes.byref(am)))
    assert len(c.decode_sample_until(smp, f, P0, 4)[0]) == 4
    # max_steps beyond the RoPE table (a model finalized with 16 rows of it, contexts of 64 positions)
    short = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize(rope_rows=16)
    rc, rf = fresh(lnb, short, prompt)
    with pytest.raises(lnb.LnbError, match="beyond the 16-row RoPE table"):
        rc.decode_sample_until(smp, rf, P0, 9)
    assert len(rc.decode_sample_until(smp, rf, P0, 8)[0]) == 8
    rc.close(); short.close()
    c.set_token_probs(4); d.set_token_probs(4)
    bat = lnb.Batch([c, d])
    with pytest.raises(lnb.LnbError, match=r"sequence 0.*token probabilities"):
        bat.decode_sample_until([smp, smp], [f, f], [P0, P0], 4)
    bat.close()
    c.close(); d.close()
    # a stage handle that is not the whole model
    st = lnb.LlamaTransformer(device=0, layer_begin=0, layer_end=1, **cfg).fill_synthetic(1234).finalize()
    sc = lnb.InferenceContext(st, SEQ)
    with pytest.raises(lnb.LnbError, match="whole-model"):
        sc.decode_sample_until(smp, 1, 0, 4)
    sc.close(); st.close()
    # V too large through the operator
    with pytest.raises(lnb.LnbError, match="131072"):
        lnb.op_sample(np.zeros((1, 131073), dtype=np.uint16), [smp], [0])
