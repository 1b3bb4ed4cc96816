"""Speculative decoding of many contexts under token automata (include/lnb.h: lnb_decode_speculative_automaton_many), on the MI355X.  Everything is compared
bit for bit: the verify launch with tests/spec_automaton_ref.py run per member on that member's own rows, whole generations with every member's own sampling
loop under the same automaton and start state.  The automata are those of tests/test_gpu_spec_automaton.py."""
import numpy as np
import pytest

from form_tally import ran
from oracle import oracle as orc
import automaton_ref as ar
import logit_rules_ref as lr
import sampler_ref as sr
import spec_automaton_ref as sa
from test_gpu_spec_automaton import ACCEPT_ROWS, ACCEPTS, P0, RUN, SEED, SEQ, STEPS, T, V, csr, engine_dfa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


# member = (start state or -1, the draft columns, stop ids): an accepted forced run into a free state, a draft rejected at column 0, a stop id inside a run, a
# final state inside a run, one column, and a member without an automaton
MIXED = [(1, [T(1), T(10), T(12), T(26), T(2)], ()), (17, [0], ()), (0, RUN[:5], (T(24),)), (4, [T(4)], ()), (17, [], ()), (-1, [7, 9], ())]
FULL = [ACCEPTS[k] for k in ("w16_accepted", "w16_rejected", "w16_stop_id", "w16_five_accepted")] * 2      # 8 members x 16 columns = the widest pass
PASSES = [(v, r, s, MIXED) for v in (1057, 128256) for r in (lr.OFF, ar.PENALTIES) for s in range(3)] + [(1057, ar.PENALTIES, 2, FULL)]


@pytest.mark.parametrize("vocab,rules,smp,members", PASSES, ids=lambda p: {id(MIXED): "mixed", id(FULL): "full", id(lr.OFF): "off", id(ar.PENALTIES): "penalties"}.get(id(p)))
def test_op_spec_automaton_many_accept_equals_the_restatement_per_member(lnb, vocab, rules, smp, members):
    dfa, free, rng = csr(ACCEPT_ROWS(vocab), 55), ar.build([np.arange(vocab)], 1), np.random.default_rng(vocab)
    cols = [[vocab // 2 + s] + d for s, (_, d, _) in enumerate(members)]
    first = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    rows = sr.llama_like_rows(rng, int(first[-1]), vocab)
    counts, pos0 = lr.counted_rows(rng, rows)[first[:-1]], [40 + 7 * s for s in range(len(members))]
    smps = [ar.SAMPLERS[(smp + s) % 3] + (sr.SEEDS[(smp + s) % 3],) for s in range(len(members))]
    want = [sa.verify_pass(rows[f:f + len(c)], dfa if s0 >= 0 else free, max(s0, 0), sm, rules, cn, p, c, stop)
            for f, c, (s0, _, stop), sm, cn, p in zip(first, cols, members, smps, counts, pos0)]
    if members is MIXED:                                     # (the members are what the comment above says)
        assert [w[4] for w in want[:5]] == [5, 0, 5, 1, 0] and [len(w[0]) for w in want[:5]] == [6, 1, 3, 1, 1] and want[2][1] and want[3][1]
    with ran(lnb, "sample.spec_many_dfa"):
        got = lnb.op_spec_automaton_many_accept(rows, [(f, len(c)) for f, c in zip(first, cols)], smps, None if rules is lr.OFF else [rules] * len(members), counts, pos0,
                                                np.concatenate(cols), dfa, [m[0] for m in members], stop_ids=[m[2] for m in members])
    for (tok, fin, state, after), (wtok, wfin, wstate, wafter, _), (s0, _, _) in zip(got, want, members):
        assert ([int(t) for t in tok], fin, state) == (wtok, bool(wfin), wstate if s0 >= 0 else -1) and (after == wafter).all()


@pytest.fixture(scope="module")
def tiny(lnb):
    gm = lnb.LlamaTransformer(device=0, **dict(orc.TINY)).fill_synthetic(1234).finalize()
    autos = [lnb.TokenAutomaton(gm, *engine_dfa(e)) for e in (False, True)]
    yield gm, lnb.synth_tokens(99, P0, V), autos, {}
    [a.close() for a in autos]
    gm.close()


# member = (start state or None: no automaton, sampler, max_draft): two in front of the six forced tokens, one in a free state whose corpus -- every id once,
# so every pass finds a 1-gram match -- drafts what the state mostly forbids, one without an automaton that never drafts; the fifth is skipped
MEMBERS = [(1, 0, 15), (1, 2, 15), (0, 1, 15), (None, 2, 0)]
CORPUS = np.random.default_rng(5).permutation(V).astype(np.int32)


def member(lnb, tiny, s, ends):
    """a fresh context behind the prompt under member s's automaton and start state (ends: member 1 runs the automaton whose forced run ends in a final state)"""
    gm, prompt, autos, _ = tiny
    c = lnb.InferenceContext(gm, SEQ)
    _, first = c.Forward(prompt, 0, want_logits=False)
    if MEMBERS[s][0] is not None:
        c.set_automaton(autos[ends and s == 1], MEMBERS[s][0])
    return c, int(first)


def state_and_kv(c, n):
    return c.automaton_state(), [(c.CacheK(l)[:P0 + n].copy(), c.CacheV(l)[:P0 + n].copy()) for l in range(orc.TINY["n_layers"])]


@pytest.mark.parametrize("rules,budget,chunks,ends", [(r, b, ch, False) for r in (None, ar.PENALTIES) for b in (16, 5) for ch in (1, 2)] + [(ar.PENALTIES, 16, 2, True)])
def test_every_member_equals_its_own_sampling_loop_under_its_automaton(lnb, tiny, rules, budget, chunks, ends):
    prompt, refs, n = list(tiny[1]), tiny[3], len(MEMBERS)
    smps = [ar.SAMPLERS[m[1]] + (SEED,) for m in MEMBERS]
    if (rules, ends) not in refs:
        refs[rules, ends] = []
        for s in range(n):
            c, first = member(lnb, tiny, s, ends)
            got, fin, _ = c.decode_sample_until(smps[s], first, P0, STEPS, rules=rules, counted=None if rules is None else prompt)
            refs[rules, ends].append((got, bool(fin)) + state_and_kv(c, len(got)))
            c.close()
    want = refs[rules, ends]
    assert [(len(w[0]), w[1]) for w in want] == [((3, True) if ends and s == 1 else (STEPS, False)) for s in range(n)]
    made = [member(lnb, tiny, s, ends) for s in range(n)] + [member(lnb, tiny, 3, False)]          # (the fifth: skipped, never touched)
    ctxs, tok = [c for c, _ in made], [f for _, f in made]
    for c, m in zip(ctxs, MEMBERS):
        c.set_draft(m[2], 1, 3, corpus=CORPUS)
    texts, parts, pos, stats = [list(prompt) for _ in ctxs], [[] for _ in ctxs], [P0] * n + [-1], []
    with ran(lnb, ("sample.spec_many_dfa", "draft.dfa_many")):
        for steps in ((STEPS,) if chunks == 1 else (9, STEPS - 9)):
            got, fin, st, _, _ = lnb.DecodeSpeculativeAutomatonMany(ctxs, smps + [smps[0]], texts, tok, pos, steps, rules=None if rules is None else [rules] * (n + 1),
                                                                    counted=None if rules is None else texts, col_budget=budget)
            stats.append(st)
            for s in range(n):
                if pos[s] >= 0:
                    parts[s].append(got[s])
                    texts[s], tok[s] = texts[s] + [tok[s]] + [int(t) for t in got[s][:-1]], int(got[s][-1])
                    pos[s] = -1 if fin[s] else pos[s] + len(got[s])
            assert len(got[n]) == 0
    for s, (wtok, wfin, wstate, wkv) in enumerate(want):
        out = np.concatenate(parts[s])
        state, kv = state_and_kv(ctxs[s], len(out))
        assert (len(out), pos[s] < 0) == (len(wtok), wfin) and (out == wtok).all() and state == wstate, "member %d" % s
        assert all((k == wk).all() and (v == wv).all() for (k, v), (wk, wv) in zip(kv, wkv)), "member %d" % s
    if budget == 16:                                         # six forced tokens from state 1 are certain drafts, whatever the logits; the final state cuts the run of three
        st = stats[0]
        assert st[0]["accepted"] >= 6 and st[0]["drafted"] >= 6 and (not ends or (st[1]["passes"], st[1]["drafted"]) == (1, 3))
    [c.close() for c in ctxs]


@pytest.mark.parametrize("case", ["final_state", "the_rules_many_call"])
def test_a_final_member_and_the_other_many_calls_are_refused(lnb, tiny, case):
    gm, prompt, autos, _ = tiny
    c = lnb.InferenceContext(gm, SEQ)
    c.Forward(prompt, 0, want_logits=False)
    c.set_automaton(autos[1], 26 if case == "final_state" else 1)        # (26: the state that engine_dfa(ends=True) leaves without a row)
    sm = [ar.SAMPLERS[2] + (SEED,)]
    if case == "final_state":
        with pytest.raises(lnb.LnbError, match="lnb_decode_speculative_automaton_many: member 0: .*final state 26"):
            lnb.DecodeSpeculativeAutomatonMany([c], sm, [prompt], [5], [P0], 4)
    else:
        with pytest.raises(lnb.LnbError, match="lnb_decode_speculative_sample_rules_many: the context holds a token automaton"):
            lnb.DecodeSpeculativeSampleMany([c], sm, [prompt], [5], [P0], 4, rules=[ar.PENALTIES])
    c.close()
