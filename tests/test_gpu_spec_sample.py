"""Sampling in the speculative loops on the MI355X (include/lnb.h "sampling in the speculative loops"): lnb_decode_speculative_sample_until and
lnb_decode_speculative_sample_many against lnb_decode_sample_until, bit for bit -- tokens, n_generated, finished and the KV rows -- and against the CPU
chains "oracle one-token step, sampler_ref.sample, feed the token" (tests/spec_sim.py, whose conditions tests/test_spec_sample_cpu.py asserts: the chains are
not greedy, a true corpus gets drafts accepted, a half-wrong one gets some rejected).  The stats follow from the tokens alone (spec_sim.simulate /
simulate_many).  The accept-and-emit kernel is first checked on bare logits rows against the restatement, one column at a time."""
import ctypes

import numpy as np
import pytest

from form_tally import ran, snapshot
from oracle import oracle as orc
import sampler_ref as sr
import spec_sim as ss

pytestmark = pytest.mark.gpu

P0, STEPS, SEQ, NMIN, NMAX = ss.P0, ss.STEPS, ss.SEQ, ss.NMIN, ss.NMAX


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


# ---- 1. the accept-and-emit kernel on bare rows ----------------------------------------------------------------------------------------------
_PREP = {}


def wanted(rows, key, smp, seed, pos0):
    """the restatement's token of every row at its own position pos0 + i (steps 1-7 once per (rows, sampler, row))"""
    out = []
    for i, row in enumerate(rows):
        k = (key, smp, i)
        if k not in _PREP:
            _PREP[k] = sr.prepare(row, *smp)
        out.append(sr.pick(_PREP[k], sr.draw(seed, pos0 + i)))
    return out


def columns(g, a, V, cur=3):
    """column inputs whose accepted prefix is a: right up to column a, wrong at a + 1, right again behind it (acceptance stops at the first miss)"""
    col = [cur] + [int(t) for t in g[:-1]]
    if a + 1 < len(col):
        col[a + 1] = (col[a + 1] + 1) % V
    return col


def emitted(g, a, stops=()):
    out = []
    for t in g[:a + 1]:
        out.append(int(t))
        if int(t) in stops:
            return out, True
    return out, False


@pytest.mark.parametrize("V", [1001, 1024, 128256])
def test_op_spec_sample_accept_on_bare_rows(lnb, V):
    W = 16
    rows = sr.llama_like_rows(np.random.default_rng(20261021 + V), W, V)
    ties = sr.crafted(V)[0]
    assert ties[0] == "ties_straddle_the_top_k_cut"
    rows[9] = ties[1]
    pos0, seed = (8, 777) if V < 100000 else (100000, 0xFEDCBA9876543210)
    for smp in ss.SAMPLERS + (ties[2], (0.0, 0, 1.0)):
        g = wanted(rows, V, smp, seed, pos0)
        if smp[0] > 0 and smp[1] == 0:
            assert any(t != sr.argmax(r) for t, r in zip(g, rows)), smp      # (a kernel that stayed greedy cannot pass)
        for a in (0, 1, 7, 15):
            with ran(lnb, "sample.spec", not_ran=("sample.row", "sample.batch")):
                got, fin = lnb.op_spec_sample_accept(rows, smp + (seed,), pos0, columns(g, a, V))
            assert ([int(t) for t in got], fin) == emitted(g, a), (V, smp, a, list(got), g)
        # a stop id at an accepted draft (column 3's token, accepted as column 4's input) and as the bonus token (column 7's, which no draft predicted)
        for at in (3, 7):
            stop = int(g[at])
            got, fin = lnb.op_spec_sample_accept(rows, smp + (seed,), pos0, columns(g, 7, V), stop_ids=[V + 5, stop])
            want, wfin = emitted(g, 7, (stop,))
            assert wfin and len(want) <= at + 1
            assert ([int(t) for t in got], fin) == (want, True), (V, smp, at, list(got), want)


@pytest.mark.parametrize("V", [1001, 128256])
def test_op_identical_rows_draw_at_their_own_positions(lnb, V):
    """sixteen copies of ONE row from position 5: the tokens differ only through the draw u(seed, 5 + i).  A kernel that drew at column 0's position would emit
    sixteen times the same token."""
    row = orc.f32_to_bf16(np.random.default_rng(5 + V).normal(0.0, 1.5, size=(1, V)).astype(np.float32))      # (a body without peaks: no token dominates)
    rows = np.repeat(row, 16, axis=0)
    smp, seed, pos0 = (1.0, 0, 1.0), 777, 5
    prep = sr.prepare(row[0], *smp)
    g = [sr.pick(prep, sr.draw(seed, pos0 + i)) for i in range(16)]
    assert len(set(g)) >= 3                                                  # (when the test was written: 14 distinct tokens at V = 1001, 16 at 128256)
    got, fin = lnb.op_spec_sample_accept(rows, smp + (seed,), pos0, columns(g, 15, V))
    assert [int(t) for t in got] == g and not fin
    got, _ = lnb.op_spec_sample_accept(rows, smp + (seed,), pos0, columns(g, 7, V))
    assert [int(t) for t in got] == g[:8]


# ---- 2. the tiny model, one context --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(lnb):
    cfg, prompt, chains = ss.tiny_chains()
    assert (lnb.synth_tokens(ss.PROMPT_SEED, P0, cfg["vocab_size"]) == prompt).all()
    models = {}
    for form in ("rows", "columns"):
        gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(ss.MODEL_SEED).finalize()
        if form == "columns":
            gm.enable_batch()
        models[form] = gm
    yield models, prompt, chains, cfg
    for gm in models.values():
        gm.close()


def fresh(lnb, gm, prompt, seq_len=SEQ, stop=()):
    c = lnb.InferenceContext(gm, seq_len)
    if stop:
        c.set_stop_ids(list(stop))
    _, first = c.Forward(prompt, 0, want_logits=False)
    return c, int(first)


def kv_rows(ctx, n_layers, rows):
    return [(ctx.CacheK(l)[:rows].copy(), ctx.CacheV(l)[:rows].copy()) for l in range(n_layers)]


def same_kv(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


_REF = {}


def reference(lnb, tiny, form, smp):
    """decode_sample_until of a fresh context (once per form and sampler): tokens and the KV rows [0, P0 + STEPS)"""
    models, prompt, chains, cfg = tiny
    if (form, smp) not in _REF:
        c, f = fresh(lnb, models[form], prompt)
        got, fin, _ = c.decode_sample_until(smp + (ss.SEEDS[smp],), f, P0, STEPS)
        assert not fin
        _REF[(form, smp)] = (f, got, kv_rows(c, cfg["n_layers"], P0 + STEPS))
        c.close()
    return _REF[(form, smp)]


@pytest.mark.parametrize("smp", ss.SAMPLERS, ids=["t1", "t07_k40_p09", "t15_p05"])
@pytest.mark.parametrize("form", ["rows", "columns"])
def test_tiny_equals_the_sampling_loop_and_the_cpu_chain(lnb, tiny, form, smp):
    models, prompt, chains, cfg = tiny
    gm, V, seed = models[form], cfg["vocab_size"], ss.SEEDS[smp]
    first, want, kv_want = reference(lnb, tiny, form, smp)
    cfirst, chain, greedy = chains[smp]
    assert first == cfirst and (want == chain).all() and 3 * greedy <= STEPS
    for kind in ("none", "exact", "every2", "every5"):
        C = ss.corpus(kind, [first] + [int(t) for t in want], V)
        for md in (1, 7, 15):
            widths = set()
            sim = ss.simulate(prompt, first, want, C, NMIN, NMAX, md, STEPS, SEQ, P0, widths=widths)
            c, f = fresh(lnb, gm, prompt)
            c.set_draft(md, NMIN, NMAX, C)
            if kind == "exact":
                with ran(lnb, "sample.spec"):
                    got, fin, st, _ = c.decode_speculative_sample_until(smp + (seed,), prompt, f, P0, STEPS)
            else:
                lnb.form_count_reset()
                got, fin, st, _ = c.decode_speculative_sample_until(smp + (seed,), prompt, f, P0, STEPS)
            # one capture per width of a pass with a draft, at most the one-token sampling graph's capture beside them: every token of the call came out of a
            # sampling launch (the greedy verify pass has no row of the tally: its graphs are looked at in test_tiny_greedy_and_sampling_graphs_live_side_by_side)
            assert lnb.form_count("sample.spec") == len(widths) and lnb.form_count("sample.row") <= 1 and lnb.form_count("sample.batch") == 0, (kind, md, snapshot(lnb))
            assert (got == want).all() and not fin, (kind, md, list(got), list(want))
            assert st == sim, (kind, md, st, sim)
            if kind == "exact" and md == 7:
                assert st["accepted"] >= 10
            assert same_kv(kv_rows(c, cfg["n_layers"], P0 + STEPS), kv_want), (kind, md, "KV rows")
            c.close()


def test_tiny_temperature_0_and_top_k_1_are_the_greedy_speculative_loop(lnb, tiny):
    models, prompt, chains, cfg = tiny
    gm = models["columns"]
    g, f = fresh(lnb, gm, prompt)
    greedy, _, _ = g.decode_greedy_until(f, P0, STEPS)
    g.close()
    C = ss.corpus("every5", [f] + [int(t) for t in greedy], cfg["vocab_size"])
    g, f = fresh(lnb, gm, prompt)
    g.set_draft(7, NMIN, NMAX, C)
    want, wfin, wst, _ = g.decode_speculative_until(prompt, f, P0, STEPS)
    g.close()
    assert (want == greedy).all() and wst["accepted"] > 0
    for s in ((0.0, 40, 0.5, 1), (1.0, 1, 1.0, 2), (0.7, 1, 0.3, 3)):
        c, f = fresh(lnb, gm, prompt)
        c.set_draft(7, NMIN, NMAX, C)
        got, fin, st, _ = c.decode_speculative_sample_until(s, prompt, f, P0, STEPS)
        assert (got == want).all() and fin == wfin and st == wst, (s, st, wst)
        c.close()


def test_tiny_chunks_a_stop_id_and_no_draft(lnb, tiny):
    models, prompt, chains, cfg = tiny
    gm, smp = models["rows"], ss.SAMPLERS[1]
    seed = ss.SEEDS[smp]
    first, want, _ = reference(lnb, tiny, "rows", smp)
    C = ss.corpus("every5", [first] + [int(t) for t in want], cfg["vocab_size"])
    # three calls of 8 steps equal one of 24
    c, f = fresh(lnb, gm, prompt)
    c.set_draft(7, NMIN, NMAX, C)
    parts, tok, hist = [], f, [int(t) for t in prompt]
    for k in range(3):
        got, fin, _, _ = c.decode_speculative_sample_until(smp + (seed,), hist, tok, P0 + 8 * k, 8)
        parts.append(got)
        hist = hist + [tok] + [int(t) for t in got[:-1]]
        tok = int(got[-1])
    c.close()
    c, f = fresh(lnb, gm, prompt)
    c.set_draft(7, NMIN, NMAX, C)
    one, _, _, _ = c.decode_speculative_sample_until(smp + (seed,), prompt, f, P0, 24)
    c.close()
    assert (np.concatenate(parts) == one).all() and (one == want[:24]).all()
    # a stop id the chain produces ends the run at the same token
    stop = int(want[9])
    n = int(np.nonzero(want == stop)[0][0]) + 1
    r, f = fresh(lnb, gm, prompt, stop=[stop])
    rwant, rfin, _ = r.decode_sample_until(smp + (seed,), f, P0, STEPS)
    r.close()
    assert rfin and len(rwant) == n
    for kind in ("exact", "every5"):
        Ck = ss.corpus(kind, [first] + [int(t) for t in want], cfg["vocab_size"])
        c, f = fresh(lnb, gm, prompt, stop=[stop])
        c.set_draft(7, NMIN, NMAX, Ck)
        got, fin, st, _ = c.decode_speculative_sample_until(smp + (seed,), prompt, f, P0, STEPS)
        assert fin and (got == want[:n]).all() and got[-1] == stop, (kind, list(got))
        assert st == ss.simulate(prompt, f, want[:n], Ck, NMIN, NMAX, 7, STEPS, SEQ, P0), kind
        c.close()
    # max_draft 0: the sampling loop itself, one pass per token
    c, f = fresh(lnb, gm, prompt)
    with ran(lnb, "sample.row", not_ran=("sample.spec",)):
        got, fin, st, _ = c.decode_speculative_sample_until(smp + (seed,), prompt, f, P0, STEPS)
    assert (got == want).all() and st == dict(passes=STEPS, verify_passes=0, drafted=0, accepted=0)
    c.close()


def test_tiny_greedy_and_sampling_graphs_live_side_by_side(lnb, tiny):
    models, prompt, chains, cfg = tiny
    gm = models["columns"]
    a, b = ss.SAMPLERS[0], ss.SAMPLERS[2]
    first, want_a, _ = reference(lnb, tiny, "columns", a)
    _, want_b, _ = reference(lnb, tiny, "columns", b)
    g, f = fresh(lnb, gm, prompt)
    greedy, _, _ = g.decode_greedy_until(f, P0, STEPS)
    g.close()
    # one corpus that drafts for all three runs: every chain's tokens in turn
    C = np.concatenate([[first], want_a, [first], want_b, [first], greedy]).astype(np.int32)
    c, f = fresh(lnb, gm, prompt)
    c.set_draft(1, NMIN, NMAX, C)                            # (one draft token: every pass with a draft is two columns wide, so all three runs use one width)
    with ran(lnb, "sample.spec"):
        got, _, st_a, _ = c.decode_speculative_sample_until(a + (ss.SEEDS[a],), prompt, f, P0, STEPS)
    assert (got == want_a).all() and st_a["verify_passes"] > 0
    # the greedy loop on the same context: its own tokens, and its verify graphs are captured NOW -- the sampling call had captured none of them
    lnb.form_count_reset()
    got, _, st_g, _ = c.decode_speculative_until(prompt, f, P0, STEPS)
    assert (got == greedy).all() and st_g["verify_passes"] > 0
    seen = snapshot(lnb)
    assert lnb.form_count("batch_rmsnorm") > 0 and not any(name.startswith("sample.") for name, _ in seen), seen      # (the batched step's norm: a verify pass was captured)
    # another sampler replays the sampling graphs: no launch is recorded at all, and the greedy graphs were not dropped either
    lnb.form_count_reset()
    got, _, st_b, _ = c.decode_speculative_sample_until(b + (ss.SEEDS[b],), prompt, f, P0, STEPS)
    assert (got == want_b).all() and st_b["verify_passes"] > 0
    assert snapshot(lnb) == {}, snapshot(lnb)
    got, _, _, _ = c.decode_speculative_until(prompt, f, P0, STEPS)
    assert (got == greedy).all() and snapshot(lnb) == {}, snapshot(lnb)
    c.close()


def test_the_engine_with_a_draft_gives_the_engines_own_tokens(lnb, tiny):
    models, prompt, chains, cfg = tiny
    gm, smp = models["columns"], (0.7, 40, 0.9, 4242)
    for sampler in (None, smp):
        want = lnb.InferenceEngine(gm, SEQ, sampler=sampler).GenerateTokens(prompt, max_new=20)
        got = lnb.InferenceEngine(gm, SEQ, sampler=sampler, draft=(7, 1, 4)).GenerateTokens(prompt, max_new=20)
        assert got == want, (sampler, got, want)


# ---- 3. the long-context forms of a verify pass --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["long", "rows"])
def test_tiny_long_context_verify_passes(lnb, tiny, which):
    models, prompt, chains, cfg = tiny
    gm, smp = models["columns"], ss.SAMPLERS[1]
    first, want, kv_want = reference(lnb, tiny, "columns", smp)
    C = ss.corpus("exact", [first] + [int(t) for t in want], cfg["vocab_size"])
    c, f = fresh(lnb, gm, prompt)
    c.set_batched_attention(0, 0)
    if which == "rows":
        c.set_rows_attention(0, 2)
    c.set_draft(7, NMIN, NMAX, C)
    with ran(lnb, "sample.spec"):
        got, fin, st, _ = c.decode_speculative_sample_until(smp + (ss.SEEDS[smp],), prompt, f, P0, STEPS)
    assert (got == want).all() and not fin
    assert c.verify_attention_form() == (1 if which == "long" else 2)
    assert st == ss.simulate(prompt, f, want, C, NMIN, NMAX, 7, STEPS, SEQ, P0) and st["accepted"] >= 10
    assert same_kv(kv_rows(c, cfg["n_layers"], P0 + STEPS), kv_want)
    c.close()


# ---- 4. many contexts ----------------------------------------------------------------------------------------------------------------------------
MANY_STEPS, CHUNK = 24, 16
MANY_SAMPLERS = ((1.0, 0, 1.0), (0.7, 40, 0.9), (1.5, 0, 0.5), (0.25, 2, 1.0))


@pytest.mark.parametrize("form", ["rows", "columns"])
@pytest.mark.parametrize("n", [3, 17])
def test_many_members_equal_their_own_sampling_loops(lnb, tiny, n, form):
    """Two calls per run: CHUNK steps with every member, then the rest with member 2 -- which a stop id of its own chain finished in the first call --
    skipped (start_pos < 0).  Every member's reference is its own decode_sample_until of MANY_STEPS steps on a fresh context."""
    models, _, _, cfg = tiny
    gm, V, L = models[form], cfg["vocab_size"], cfg["n_layers"]
    plen = [(5, 8, 11)[s % 3] for s in range(n)]
    prompts = [lnb.synth_tokens(300 + s, plen[s], V) for s in range(n)]
    smps = [MANY_SAMPLERS[s % 4] + (1000 + 7 * s,) for s in range(n)]
    smps[1] = (0.0, 5, 0.5, 9)                                               # a greedy member
    mds = [(7, 15, 3, 0, 1)[s % 5] for s in range(n)]                       # member 3 never drafts ...
    if n == 3:
        mds[1] = 0                                                           # ... and with three members the greedy one
    kinds = [("exact", "every5", "exact", "exact", "every2", "none")[s % 6] for s in range(n)]
    # every member alone: first without stop ids (to learn a token its chain produces), member 2 then again with one
    refs, stop = [], None
    for s in range(n):
        c, f = fresh(lnb, gm, prompts[s])
        out, fin, _ = c.decode_sample_until(smps[s], f, plen[s], MANY_STEPS)
        full = out
        if s == 2:
            stop = int(out[6])
            c.close()
            c, f = fresh(lnb, gm, prompts[s], stop=[stop])
            out, fin, _ = c.decode_sample_until(smps[s], f, plen[s], MANY_STEPS)
            assert fin and len(out) <= 7 and out[-1] == stop
        refs.append(dict(first=f, out=out, fin=fin, kv=kv_rows(c, L, plen[s] + len(out)), corpus=ss.corpus(kinds[s], [f] + [int(t) for t in full], V)))
        c.close()
    g, f = fresh(lnb, gm, prompts[1])
    greedy, _, _ = g.decode_greedy_until(f, plen[1], MANY_STEPS)
    g.close()
    assert (refs[1]["out"] == greedy).all() and (refs[0]["out"] != greedy[:len(refs[0]["out"])]).any()
    for budget in (0, 32):
        ctxs = []
        for s in range(n):
            c, f = fresh(lnb, gm, prompts[s], stop=[stop] if s == 2 else ())
            assert f == refs[s]["first"]
            c.set_draft(mds[s], NMIN, NMAX, refs[s]["corpus"])
            ctxs.append(c)

        def member(s, g0, steps, skip=False):
            """what member s emits in a call of `steps` steps that starts behind its first g0 tokens"""
            R = refs[s]
            if skip:                                         # (its token is ignored and nothing of it is read)
                return dict(history=[int(t) for t in prompts[s]], token=0, out=R["out"][:0], corpus=R["corpus"], md=mds[s], seq_len=SEQ, start=None)
            return dict(history=[int(t) for t in prompts[s]] + ([R["first"]] + [int(t) for t in R["out"][:g0 - 1]] if g0 else []),
                        token=int(R["out"][g0 - 1]) if g0 else R["first"], out=R["out"][g0:g0 + steps], corpus=R["corpus"], md=mds[s], seq_len=SEQ,
                        start=None if skip else plen[s] + g0)

        # the first call: everybody
        mem = [member(s, 0, CHUNK) for s in range(n)]
        with ran(lnb, "sample.spec_many", not_ran=("sample.spec", "sample.row", "sample.batch")):
            toks, fins, stats, info, _ = lnb.DecodeSpeculativeSampleMany(ctxs, smps, [m["history"] for m in mem], [m["token"] for m in mem], [m["start"] for m in mem],
                                                                         CHUNK, budget)
        want_stats, want_info = ss.simulate_many(mem, budget, CHUNK, NMIN, NMAX)
        for s in range(n):
            assert np.array_equal(toks[s], mem[s]["out"]) and fins[s] == (s == 2), (budget, s, list(toks[s]), list(mem[s]["out"]))
        assert stats == want_stats, (budget, stats, want_stats)
        assert {k: info[k] for k in want_info} == want_info and info["long_passes"] == 0, (budget, info, want_info)
        assert sum(st["accepted"] for st in stats) > 0 and info["max_columns"] <= (budget or 16 * -(-n // 16))
        # the second call: member 2 is skipped, the others go on to MANY_STEPS
        frozen = kv_rows(ctxs[2], L, SEQ)
        mem = [member(s, CHUNK, MANY_STEPS - CHUNK, skip=s == 2) for s in range(n)]
        toks2, fins2, stats2, info2, _ = lnb.DecodeSpeculativeSampleMany(ctxs, smps, [m["history"] for m in mem], [m["token"] for m in mem],
                                                                           [-1 if m["start"] is None else m["start"] for m in mem], MANY_STEPS - CHUNK, budget)
        want_stats, want_info = ss.simulate_many(mem, budget, MANY_STEPS - CHUNK, NMIN, NMAX)
        assert stats2 == want_stats and {k: info2[k] for k in want_info} == want_info, (budget, stats2, want_stats, info2, want_info)
        for s in range(n):
            R = refs[s]
            if s == 2:
                assert len(toks2[s]) == 0 and fins2[s] and same_kv(kv_rows(ctxs[s], L, SEQ), frozen), budget
            else:
                assert np.array_equal(np.concatenate([toks[s], toks2[s]]), R["out"]) and not fins2[s], (budget, s)
            assert same_kv(kv_rows(ctxs[s], L, plen[s] + len(R["out"])), R["kv"]), (budget, s, "KV rows")
        for c in ctxs:
            c.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------
BAD_SAMPLERS = (((-1.0, 0, 1.0, 0), "temperature"), ((float("nan"), 0, 1.0, 0), "temperature"), ((float("inf"), 0, 1.0, 0), "temperature"), ((1.0, -2, 1.0, 0), "top_k"),
                ((1.0, 0, float("nan"), 0), "top_p"), ((1.0, 0, 0.0, 0), "top_p"), ((1.0, 0, 1.25, 0), "top_p"))


def bad_samplers(lnb):
    r = lnb.Sampler(1.0, 0, 1.0, 1); r.reserved = 7
    return [(lnb.Sampler(*s), w) for s, w in BAD_SAMPLERS] + [(r, "reserved")]


def test_refusals_leave_the_caches_alone_and_a_valid_call_follows(lnb, tiny):
    models, prompt, chains, cfg = tiny
    gm, smp, L = models["columns"], ss.SAMPLERS[1], cfg["n_layers"]
    seed = ss.SEEDS[smp]
    first, want, _ = reference(lnb, tiny, "columns", smp)
    C = ss.corpus("exact", [first] + [int(t) for t in want], cfg["vocab_size"])
    c, f = fresh(lnb, gm, prompt)
    d, _ = fresh(lnb, gm, prompt)
    for x in (c, d):
        x.set_draft(7, NMIN, NMAX, C)
    kv0 = [kv_rows(x, L, SEQ) for x in (c, d)]
    S = smp + (seed,)

    def one(match, sampler=S, history=prompt, token=f, pos=P0, steps=8):
        with pytest.raises(lnb.LnbError, match=match):
            c.decode_speculative_sample_until(sampler, history, token, pos, steps)
        assert same_kv(kv_rows(c, L, SEQ), kv0[0]), match

    def many(match, samplers=(S, S), tokens=(f, f), pos=(P0, P0), steps=8, budget=0, ctxs=None):
        with pytest.raises(lnb.LnbError, match=match):
            lnb.DecodeSpeculativeSampleMany(ctxs or [c, d], samplers, [prompt, prompt], list(tokens), list(pos), steps, budget)
        assert same_kv(kv_rows(c, L, SEQ), kv0[0]) and same_kv(kv_rows(d, L, SEQ), kv0[1]), match

    # what lnb_decode_sample_until refuses
    one("sampler", sampler=None)
    many("samplers", samplers=None)
    for bad, word in bad_samplers(lnb):
        one(word, sampler=bad)
        many("member 1.*" + word, samplers=(S, bad))
    for x in (c, d):
        x.set_token_probs(4)
    one("token probabilities")
    many("context 0 records token probabilities")
    for x in (c, d):
        x.set_token_probs(0)
    # what the greedy speculative forms refuse
    one("max_steps must be positive", steps=0)
    many("max_steps must be positive", steps=0)
    one("exceeds the context length", steps=SEQ + 1)
    many("exceeds its token log", steps=SEQ + 1)
    one("beyond the KV cache", pos=SEQ - 2)
    many("beyond the KV cache", pos=(P0, SEQ - 2))
    one("outside the vocabulary", token=cfg["vocab_size"])
    many("outside the vocabulary", tokens=(f, -1))
    many("col_budget", budget=1)
    many("appears twice", ctxs=[c, c])
    c.set_mode("fast")
    one("exact")
    many("tolerance mode")
    c.set_mode("exact")
    e, _ = fresh(lnb, gm, prompt)
    bat = lnb.Batch([c, e])
    one("live batch")
    many("live batch")
    bat.close(); e.close()
    one_tok = np.array([f], dtype=np.int32)
    lnb._chk(c.L.lnb_forward_stage_begin(c.h, lnb._p(one_tok), 1, P0, 1))
    kv0[0] = kv_rows(c, L, SEQ)                              # (the stage step wrote row P0 of c, as the one-token step at P0 does: the same bits the valid call below writes again)
    one("lnb_forward_stage_begin has not been ended")
    many("lnb_forward_stage_begin has not been ended")
    am = ctypes.c_int32(0)
    lnb._chk(c.L.lnb_forward_stage_end(c.h, ctypes.byref(am)))
    other = lnb.InferenceContext(models["rows"], SEQ)
    many("another lnb_model handle", ctxs=[d, other])
    other.close()
    # a stage handle that is not the whole model
    st = lnb.LlamaTransformer(device=0, layer_begin=0, layer_end=1, **cfg).fill_synthetic(ss.MODEL_SEED).finalize()
    sc = lnb.InferenceContext(st, SEQ)
    with pytest.raises(lnb.LnbError, match="whole-model"):
        sc.decode_speculative_sample_until(S, prompt, 1, 0, 4)
    with pytest.raises(lnb.LnbError, match="whole-model"):
        lnb.DecodeSpeculativeSampleMany([sc], [S], [prompt], [1], [8], 4)
    sc.close(); st.close()
    # a vocabulary beyond what the sampler's integer sums hold
    with pytest.raises(lnb.LnbError, match="131072"):
        lnb.op_spec_sample_accept(np.zeros((2, 131073), dtype=np.uint16), S, 0, [0, 0])
    big = lnb.LlamaTransformer(device=0, **dict(cfg, vocab_size=131200, n_layers=1)).fill_synthetic(1).finalize()
    bc = lnb.InferenceContext(big, 16)
    with pytest.raises(lnb.LnbError, match="131072"):
        bc.decode_speculative_sample_until(S, [1, 2], 3, 2, 4)
    with pytest.raises(lnb.LnbError, match="131072"):
        lnb.DecodeSpeculativeSampleMany([bc], [S], [[1, 2]], [3], [2], 4)
    bc.close(); big.close()
    # and after all of it both entry points give the sampling loop's tokens
    got, fin, _, _ = c.decode_speculative_sample_until(S, prompt, f, P0, STEPS)
    assert (got == want).all() and not fin
    toks, _, _, _, _ = lnb.DecodeSpeculativeSampleMany([c, d], [S, S], [prompt, prompt], [f, f], [P0, P0], STEPS)
    assert (toks[0] == want).all() and (toks[1] == want).all()
    c.close(); d.close()
