"""Speculative decoding under a token automaton (include/lnb.h: lnb_decode_speculative_automaton_until) without a GPU: the three names, the refusals that come
before any handle or device is touched, and the numpy statement of the draft filter (tests/spec_automaton_ref.py) on hand-written automata."""
import ctypes as C
import re

import numpy as np
import pytest

import spec_automaton_ref as sa

NAMES = ["lnb_decode_speculative_automaton_until", "lnb_op_automaton_draft", "lnb_op_spec_automaton_accept"]


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


def test_the_three_functions_are_bound_and_exported(lnb):
    assert all(n in lnb.EXPORTS and hasattr(lnb.lib(), n) for n in NAMES)
    assert all(hasattr(lnb, n) for n in ("op_automaton_draft", "op_spec_automaton_accept")) and hasattr(lnb.InferenceContext, "decode_speculative_automaton_until")


RP, ET, EN = np.array([0, 2, 2], dtype=np.int64), np.array([1, 5], dtype=np.int32), np.array([1, 0], dtype=np.int32)


def test_the_calls_refuse_their_arguments_before_any_handle_or_device(lnb):
    L = lnb.lib()
    out, n = np.zeros(4, dtype=np.int32), C.c_int(0)
    smp = lnb._samplers([(-1.0, 0, 1.0, 0)], 1)
    for s, word in ((None, "null argument (sampler)"), (smp, "temperature")):
        assert L.lnb_decode_speculative_automaton_until(None, s, None, None, 0, None, 0, 1, 0, 4, lnb._p(out), C.byref(n), None, None, None) < 0
        assert word in L.lnb_last_error().decode()
    dfa = (RP, ET, EN)
    for kw, word in ((dict(state0=2), "state0 2 is outside [0, 2)"), (dict(draft=[1, 5], max_draft=1), "n_draft must be 0..max_draft"), (dict(max_draft=16), "max_draft must be 0..15"),
                     (dict(automaton=(np.array([0, 2, 1]), ET, EN)), "row_ptr must not decrease")):
        a = dict(automaton=dfa, state0=0, draft=[1], max_draft=4, V=8)
        a.update(kw)
        with pytest.raises(lnb.LnbError, match=re.escape(word)):
            lnb.op_automaton_draft(**a)
    row = np.zeros((2, 8), dtype=np.uint16)
    for kw, word in ((dict(state0=-1), "state0 -1 is outside [0, 2)"), (dict(col_tokens=[0, 2]), "cannot be walked from state 0"), (dict(col_tokens=[0, 8]), "outside the vocabulary"),
                     (dict(sampler=(1.0, -1, 1.0, 0)), "top_k"), (dict(rules=(0.0, 0.0, 0.0, 0.0)), "repetition_penalty")):
        a = dict(sampler=(1.0, 0, 1.0, 0), rules=None, counts=None, pos0=0, col_tokens=[0, 1], automaton=dfa, state0=0)
        a.update(kw)
        with pytest.raises(lnb.LnbError, match=re.escape(word)):
            lnb.op_spec_automaton_accept(row, **a)
    with pytest.raises(lnb.LnbError, match="emitted_probs"):
        lnb.InferenceEngine(None, 16, automaton=dfa, emitted_probs=2, draft=(4, 1, 2))


def test_the_filter_rule_on_hand_written_automata():
    # states: 0 = {2, 4, 9} -> 1, 2, 3; 1 = {7} -> 2; 2 = {3} -> 4; 3 final; 4 = {0, 1} -> 0, 0
    dfa = (np.array([0, 3, 4, 5, 5, 7], dtype=np.int64), np.array([2, 4, 9, 7, 3, 0, 1], dtype=np.int32), np.array([1, 2, 3, 2, 4, 0, 0], dtype=np.int32))
    f = sa.filter_draft
    assert f(dfa, 0, [2, 7, 3, 1, 5], 15) == ([2, 7, 3, 1], [0, 1, 2, 4, 0])             # walked, then cut at the forbidden 5; state 0 forces nothing
    assert f(dfa, 0, [5, 2], 15) == ([], [0])                                             # forbidden at once, nothing to extend
    assert f(dfa, 0, [9, 2], 15) == ([9], [0, 3])                                         # a final state cuts behind its token
    assert f(dfa, 1, [], 15) == ([7, 3], [1, 2, 4])                                       # forced from nothing, until a state with two tokens
    assert f(dfa, 0, [2], 15) == ([2, 7, 3], [0, 1, 2, 4]) and f(dfa, 0, [2], 2) == ([2, 7], [0, 1, 2]) and f(dfa, 1, [], 0) == ([], [1])
    assert f(dfa, 1, [3], 15) == ([7, 3], [1, 2, 4])                                      # a forbidden guess is replaced by the forced token
