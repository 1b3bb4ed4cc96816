"""A token automaton in the device sampling loops (include/lnb.h: lnb_ctx_set_automaton), on the MI355X.  Step 0d is "every entry outside the state's row
is -inf" in front of an integer rule, so everything is compared bit for bit: the kernel on host rows and whole generations with tests/logit_rules_ref.py on
the pre-masked row and the numpy walk of tests/automaton_ref.py, and the loop a second time with the -inf bias list of the logit rules."""
import math

import numpy as np
import pytest

from form_tally import ran
from oracle import oracle as orc
import automaton_ref as ar
import logit_rules_ref as lr

pytestmark = pytest.mark.gpu
SEED, P0, STEPS, SEQ, V = 777, 8, 48, 64, 1024


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


@pytest.mark.parametrize("vocab", [1000, 1024, 1057, 131072])
def test_op_sample_automaton_equals_the_restatement_on_the_masked_row(lnb, vocab):
    """1000: lanes without entries and a ragged last mask word; 1024: one entry per lane; 1057: a ragged word behind full ones; the largest vocabulary"""
    dfa, cases = ar.op_cases(vocab)
    rows, counts = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    smps, rules, pos, states = [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases], [c[5] for c in cases]
    with ran(lnb, "sample.dfa_row"):
        tok, nxt, _ = lnb.op_sample_automaton(rows, smps, dfa, states, pos, rules=rules, counts=counts)
    assert [int(t) for t in tok] == [c[6] for c in cases] and [int(s) for s in nxt] == [c[7] for c in cases]
    free = [i for i, s in enumerate(states) if s == 1]       # everything allowed: lnb_op_sample_rules without an automaton, token for token
    assert (lnb.op_sample_rules(rows[free], [smps[i] for i in free], [rules[i] for i in free], counts[free], [pos[i] for i in free])[0] == tok[free]).all()


@pytest.fixture(scope="module")
def tiny(lnb):
    gm = lnb.LlamaTransformer(device=0, **dict(orc.TINY)).fill_synthetic(1234).finalize()
    rng = np.random.default_rng(4242)
    csr = [ar.build(ar.random_rows(rng, ar.N_STATES, V)) for _ in range(2)]
    autos = [lnb.TokenAutomaton(gm, *d) for d in csr]
    yield gm, lnb.synth_tokens(99, P0, V), csr, autos
    for a in autos:
        a.close()
    gm.close()


def fresh(lnb, gm, prompt):
    c = lnb.InferenceContext(gm, SEQ)
    _, first = c.Forward(prompt, 0, want_logits=False)
    return c, first


@pytest.mark.parametrize("smp", ar.SAMPLERS, ids=["greedy", "plain", "topk_topp"])
def test_a_constrained_generation_in_any_chunking_equals_the_restatement_and_the_bias_path(lnb, tiny, smp):
    gm, prompt, csr, autos = tiny
    dfa, s0, sm = csr[0], 5, smp + (SEED,)
    c, f = fresh(lnb, gm, prompt)
    c.set_automaton(autos[0], s0)
    one, fin, _ = c.decode_sample_until(sm, f, P0, STEPS)
    end = c.automaton_state()
    assert len(one) == STEPS and not fin
    for chunk in (1, 7, STEPS):                              # the state carries over from call to call
        c.set_automaton(autos[0], s0)
        parts, tok = [], f
        for p in range(0, STEPS, chunk):
            part, fin, _ = c.decode_sample_until(sm, tok, P0 + p, min(chunk, STEPS - p))
            parts.append(part); tok = int(part[-1])
        assert (np.concatenate(parts) == one).all() and not fin and c.automaton_state() == end, chunk
    # every step's own logits row from a second context; a third runs the rules loop one step at a time with -inf bias on the forbidden ids
    c2, _ = fresh(lnb, gm, prompt)
    c3, _ = fresh(lnb, gm, prompt)
    state, tok, moved = s0, f, 0
    for i in range(STEPS):
        row = orc.f32_to_bf16(np.ascontiguousarray(c2.ForwardAppend([tok], P0 + i, want_logits=True)[0][0], dtype=np.float32))
        want = lr.sample(ar.mask_row(row, dfa, state), sm, pos=P0 + i)[0]
        moved += want != lr.sample(row, sm, pos=P0 + i)[0]
        ban = tuple((int(j), -math.inf) for j in np.setdiff1d(np.arange(V), ar.allowed(dfa, state)))      # (at most 1023 at this V and density)
        assert int(one[i]) == want == int(c3.decode_sample_until(sm, tok, P0 + i, 1, rules=(1.0, 0.0, 0.0, 0.0, ban))[0][0]), i
        state, tok = ar.walk(dfa, state, want), want
    assert state == end and moved * 4 >= STEPS               # (a condition on the reference: the automaton changed at least a quarter of the tokens)
    c.close(); c2.close(); c3.close()


def test_a_final_state_finishes_the_generation_and_a_stop_id_freezes_the_state(lnb, tiny):
    gm, prompt, _, _ = tiny
    rows = ar.random_rows(np.random.default_rng(7), 3, V)
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows]), [sum(r.size for r in rows)]]).astype(np.int64)      # states 0 -> 1 -> 2 -> 3, 3 final
    chain = lnb.TokenAutomaton(gm, rp, np.concatenate(rows), np.concatenate([np.full(r.size, s + 1) for s, r in enumerate(rows)]))
    sm = (0.7, 40, 0.9, SEED)
    c, f = fresh(lnb, gm, prompt)
    c.set_automaton(chain, 0)
    got, fin, _ = c.decode_sample_until(sm, f, P0, 8)
    assert len(got) == 3 and fin and c.automaton_state() == 3 and all(int(t) in rows[s] for s, t in enumerate(got))
    with pytest.raises(lnb.LnbError, match="final state 3"):
        c.decode_sample_until(sm, int(got[-1]), P0 + 3, 4)
    c.set_automaton(chain, 0)                                # the same automaton: the state starts again
    c.set_stop_ids([int(got[1])])
    again, fin, _ = c.decode_sample_until(sm, f, P0, 8)
    n = 1 if got[0] == got[1] else 2
    assert (again == got[:n]).all() and fin and c.automaton_state() == n      # the stop token moved the state, the frozen steps behind it did not
    c.set_automaton(None)
    c.close(); chain.close()


def test_batch_members_under_their_own_automata_equal_their_single_runs(lnb, tiny):
    gm, _, csr, autos = tiny
    prompts = [lnb.synth_tokens(300 + s, (5, 8, 11, 6, 9)[s], V) for s in range(5)]
    smps = [(0.7, 40, 0.9, 11), (0.0, 0, 1.0, 12), (1.0, 0, 1.0, 13), (0.7, 40, 0.9, 14), (1.0, 0, 1.0, 15)]
    attach = [(autos[0], 0), (autos[0], 9), (autos[1], 3), None, (autos[1], 4)]
    pos = [len(p) for p in prompts[:4]] + [-1]               # member 4 sits the call out
    single = []
    for s in range(3):
        c, f = fresh(lnb, gm, prompts[s])
        c.set_automaton(*attach[s])
        single.append((c.decode_sample_until(smps[s], f, pos[s], 10)[0], c.automaton_state()))
        c.close()

    def batch(with_automata):
        ctxs, firsts = zip(*(fresh(lnb, gm, p) for p in prompts))
        for c, a in zip(ctxs, attach):
            if with_automata and a:
                c.set_automaton(*a)
        return lnb.Batch(list(ctxs)), ctxs, [int(f) for f in firsts]

    bat, ctxs, firsts = batch(True)
    with pytest.raises(lnb.LnbError, match="live batch"):
        ctxs[3].set_automaton(autos[0], 0)
    with ran(lnb, "sample.dfa_batch"):
        got, _ = bat.decode_sample_until(smps, firsts, pos, 10)
    for s in range(3):
        assert (got[s] == single[s][0]).all() and ctxs[s].automaton_state() == single[s][1], s
    assert len(got[4]) == 0 and ctxs[4].automaton_state() == 4
    plain, pctxs, pfirsts = batch(False)
    assert firsts == pfirsts and (plain.decode_sample_until(smps, pfirsts, pos, 10)[0][3] == got[3]).all()
    bat.close(); plain.close()
    [c.close() for c in ctxs + pctxs]


def test_detaching_restores_the_plain_loop_and_the_other_loops_refuse(lnb, tiny):
    gm, prompt, _, autos = tiny
    sm = (0.7, 40, 0.9, SEED)
    c, f = fresh(lnb, gm, prompt)
    before = c.decode_sample_until(sm, f, P0, 12)[0]
    c.set_automaton(autos[1], 2)
    assert (c.decode_sample_until(sm, f, P0, 12)[0] != before).any()
    c.set_draft(4, 1, 2)
    for call in (lambda: c.decode_greedy_until(f, P0, 4), lambda: c.decode_greedy(f, P0, 4), lambda: c.decode_speculative_until(prompt, f, P0, 4),
                 lambda: c.decode_speculative_sample_until(sm, prompt, f, P0, 4), lambda: c.set_emitted_probs(2).decode_sample_until(sm, f, P0, 4)):
        with pytest.raises(lnb.LnbError, match="lnb_ctx_set_automaton"):
            call()
    c.set_emitted_probs(-1)
    with pytest.raises(lnb.LnbError, match="hold the automaton"):
        autos[1].close()
    c.set_automaton(None)
    assert c.automaton_state() == -1 and (c.decode_sample_until(sm, f, P0, 12)[0] == before).all()
    c.close()
