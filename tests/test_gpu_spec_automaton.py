"""Speculative decoding under a token automaton (include/lnb.h: lnb_decode_speculative_automaton_until), on the MI355X.  Everything is compared bit for bit: the
draft filter with the numpy walk of tests/spec_automaton_ref.py, the verify launch with tests/logit_rules_ref.py on the rows masked by the column states, and
whole generations with the sampling loop under the same automaton and start state."""
import numpy as np
import pytest

from form_tally import ran
from oracle import oracle as orc
import automaton_ref as ar
import logit_rules_ref as lr
import sampler_ref as sr
import spec_automaton_ref as sa

pytestmark = pytest.mark.gpu
SEED, P0, STEPS, SEQ, V = 777, 8, 24, 64, 1024
VOCABS = (1057, 128256)
T = lambda s: (37 * s + 5) % 1000                            # the token of a one-token state of the verify automaton
RUN = [T(s) for s in (0, 3, 24, 49, 41, 46, 20, 21, 28, 16, 54, 15, 47, 27, 9)]      # automaton_ref.build: a one-token state s leads to (7 s + 3) mod 61


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


def csr(rows, n):
    return ar.build([rows.get(s, []) for s in range(n)])     # (a state without a row is final)


# state 0 = the multiples of 3 (rank r leads to (3 + r) mod 61), state 2 = the odd ids (to (17 + r) mod 61); 1 -> 10 -> 12 -> 26 -> 2 hold one token each
DRAFT_ROWS = lambda v: {0: np.arange(0, v, 3), 2: np.arange(1, v, 2), 1: [0], 10: [31], 12: [32], 26: [v - 1]}
DRAFTS = {"forbidden_first": (0, [1, 906], 15), "forbidden_middle": (0, [906, 912, 4, 89], 15), "forbidden_nowhere": (0, [906, 174, 912, 943, 180], 15),
          "final_in_the_middle": (0, [906, 6, 174], 15), "forced_from_k0": (1, [], 15), "forced_behind_a_kept_draft": (0, [912, 91], 15),
          "forced_longer_than_max_draft": (1, [], 3), "rank_36902_at_the_large_vocabulary": (0, [110706, 909], 15)}


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("name", sorted(DRAFTS))
def test_op_automaton_draft_equals_the_numpy_walk(lnb, vocab, name):
    dfa, (s0, draft, md) = csr(DRAFT_ROWS(vocab), 27), DRAFTS[name]
    with ran(lnb, "draft.dfa"):
        tok, states = lnb.op_automaton_draft(dfa, s0, draft, md, V=vocab)
    assert ([int(t) for t in tok], [int(s) for s in states]) == sa.filter_draft(dfa, s0, draft, md)


# states 1 -> 10 -> 12 -> 26 -> 2 -> 17 and 0 -> 3 -> ... -> 9 -> 5 hold one token each; 17 (the multiples of 3, rank r to r mod 61) and 5 (the odd ids) are free;
# 4 holds one token that leads to the final state 31.  case = (start state, the draft columns, stop ids)
ACCEPT_ROWS = lambda v: {**{s: [T(s)] for s in (1, 10, 12, 26, 2, 4, 0, 3, 24, 49, 41, 46, 20, 21, 28, 16, 54, 15, 47, 27, 9)}, 17: np.arange(0, v, 3), 5: np.arange(1, v, 2)}
ACCEPTS = {"one_column": (17, [], ()), "w2_rejected": (17, [0], ()), "w2_accepted": (1, [T(1)], ()), "w16_accepted": (0, RUN, ()), "w16_stop_id": (0, RUN, (T(41),)),
           "w16_five_accepted": (1, [T(1), T(10), T(12), T(26), T(2), 0] + RUN[:9], ()), "w16_rejected": (17, [0] + RUN[:14], ()), "w2_final_inside": (4, [T(4)], ())}


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("rules", [lr.OFF, ar.PENALTIES], ids=["off", "penalties"])
@pytest.mark.parametrize("smp", range(3), ids=["greedy", "plain", "topk_topp"])
@pytest.mark.parametrize("name", sorted(ACCEPTS))
def test_op_spec_automaton_accept_equals_the_restatement_on_the_masked_rows(lnb, vocab, rules, smp, name):
    dfa, (s0, draft, stop), rng = csr(ACCEPT_ROWS(vocab), 55), ACCEPTS[name], np.random.default_rng(vocab)
    rows = sr.llama_like_rows(rng, 16, vocab)
    counts = lr.counted_rows(rng, rows)[0]
    col, sm = [vocab // 2] + draft, ar.SAMPLERS[smp] + (sr.SEEDS[smp],)
    want, fin, state, after, a = sa.verify_pass(rows[:len(col)], dfa, s0, sm, rules, counts, 40, col, stop)
    assert a == {"w2_accepted": 1, "w16_accepted": 15, "w16_stop_id": 15, "w16_five_accepted": 5, "w2_final_inside": 1}.get(name, 0)      # (the case is what its name says)
    assert fin >= (name in ("w16_stop_id", "w2_final_inside")) and len(want) == {"w16_stop_id": 5, "w2_final_inside": 1}.get(name, a + 1)
    with ran(lnb, "sample.spec_dfa"):
        got = lnb.op_spec_automaton_accept(rows[:len(col)], sm, rules, counts, 40, col, dfa, s0, stop_ids=stop)
    assert ([int(t) for t in got[0]], got[1], got[2]) == (want, fin, state) and (got[3] == after).all()


def engine_dfa(ends):
    """random rows; 1 -> 10 -> 12 -> 26 -> 2 -> 17 force one token each, a run of six from state 1 into the free state 0; ends: the run's fourth state is final"""
    rows = ar.random_rows(np.random.default_rng(4242), ar.N_STATES, V)
    for s, t in zip((1, 10, 12, 26, 2, 17), (0, 31, 32, V - 1, V // 3, 33)):
        rows[s] = [] if ends and s == 26 else [t]
    return ar.build(rows)


@pytest.fixture(scope="module")
def tiny(lnb):
    gm = lnb.LlamaTransformer(device=0, **dict(orc.TINY)).fill_synthetic(1234).finalize()
    autos = [lnb.TokenAutomaton(gm, *engine_dfa(e)) for e in (False, True)]
    yield gm, lnb.synth_tokens(99, P0, V), autos, {}
    [a.close() for a in autos]
    gm.close()


def run(lnb, tiny, ends, call):
    """a fresh context behind the prompt, in state 1 of the automaton -> what `call` returns, the end state and the KV rows behind the generated tokens"""
    gm, prompt, autos, _ = tiny
    c = lnb.InferenceContext(gm, SEQ)
    _, first = c.Forward(prompt, 0, want_logits=False)
    c.set_automaton(autos[ends], 1)
    got = call(c, int(first))
    out = got, c.automaton_state(), [(c.CacheK(l)[:P0 + len(got[0])].copy(), c.CacheV(l)[:P0 + len(got[0])].copy()) for l in range(orc.TINY["n_layers"])]
    c.close()
    return out


GENERATIONS = [(s, r, md, ch, False) for s in (0, 2) for r in (None, ar.PENALTIES) for md in (4, 15) for ch in (1, 2)] + [(2, ar.PENALTIES, 15, 1, True)]


@pytest.mark.parametrize("smp,rules,max_draft,chunks,ends", GENERATIONS)
def test_a_generation_equals_the_sampling_loop_under_the_same_automaton(lnb, tiny, smp, rules, max_draft, chunks, ends):
    """ends: the forced run reaches a final state in the middle of the first pass -- three tokens, one pass, finished"""
    prompt, refs, sm = tiny[1], tiny[3], ar.SAMPLERS[smp] + (SEED,)
    if (smp, rules, ends) not in refs:
        refs[smp, rules, ends] = run(lnb, tiny, ends, lambda c, f: c.decode_sample_until(sm, f, P0, STEPS, rules=rules, counted=None if rules is None else prompt))
    (want, wfin, _), wstate, wkv = refs[smp, rules, ends]
    assert (len(want), bool(wfin)) == ((3, True) if ends else (STEPS, False))

    def call(c, tok):
        c.set_draft(max_draft, 1, 3)
        parts, text, stats = [], list(prompt), []
        for p0, n in ((0, STEPS),) if chunks == 1 else ((0, 9), (9, STEPS - 9)):
            got, fin, st, _ = c.decode_speculative_automaton_until(sm, text, tok, P0 + p0, n, rules=rules, counted=None if rules is None else text)
            parts.append(got); stats.append(st)
            text, tok = text + [tok] + [int(t) for t in got[:-1]], int(got[-1])
        if ends:
            with pytest.raises(lnb.LnbError, match="final state"):
                c.decode_speculative_automaton_until(sm, prompt, tok, P0, 4)
        return np.concatenate(parts), fin, stats[0]

    with ran(lnb, ("sample.spec_dfa", "draft.dfa")):
        (got, fin, st), state, kv = run(lnb, tiny, ends, call)
    assert (got == want).all() and bool(fin) == bool(wfin) and state == wstate and all((k == wk).all() and (v == wv).all() for (k, v), (wk, wv) in zip(kv, wkv))
    # the forced run from the start state: certain drafts, whatever the logits
    assert st["verify_passes"] > 0 and ((st["passes"], st["drafted"]) == (1, 3) if ends else st["accepted"] >= 3)


def test_the_engine_routes_an_automaton_with_a_draft_to_the_new_call_and_a_context_without_one_is_refused(lnb, tiny):
    gm, prompt, _, _ = tiny
    c = lnb.InferenceContext(gm, SEQ)
    with pytest.raises(lnb.LnbError, match="holds no token automaton"):
        c.set_draft(4, 1, 3).decode_speculative_automaton_until(ar.SAMPLERS[2] + (SEED,), prompt, 5, P0, 4)
    c.close()
    kw = dict(sampler=ar.SAMPLERS[2] + (SEED,), rules=ar.PENALTIES, automaton=engine_dfa(False), automaton_state=1)
    want = lnb.InferenceEngine(gm, SEQ, **kw).GenerateTokens(prompt, 16)
    with ran(lnb, ("sample.spec_dfa", "draft.dfa")):
        assert lnb.InferenceEngine(gm, SEQ, draft=(15, 1, 3), **kw).GenerateTokens(prompt, 16) == want and len(want) == 16
