"""Speculative decoding of many contexts under token automata (include/lnb.h: lnb_decode_speculative_automaton_many) without a GPU: the two names and the
refusals that come before any handle or device is touched."""
import ctypes as C
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


def test_the_two_functions_are_bound_and_exported(lnb):
    assert all(n in lnb.EXPORTS and hasattr(lnb.lib(), n) for n in ("lnb_decode_speculative_automaton_many", "lnb_op_spec_automaton_many_accept"))
    assert hasattr(lnb, "DecodeSpeculativeAutomatonMany") and hasattr(lnb, "op_spec_automaton_many_accept")


DFA = (np.array([0, 2, 2], dtype=np.int64), np.array([1, 5], dtype=np.int32), np.array([1, 0], dtype=np.int32))      # state 0 = {1, 5} -> 1, 0; state 1 final
OP_REFUSALS = [(dict(segs=[(0, 1), (2, 1)]), "must follow the member before it"), (dict(segs=[(0, 1), (1, 1)]), "the members' columns end at 2, the pass at 3"),
               (dict(state0=[0, 2]), "member 1: state0 2 is outside [0, 2)"), (dict(col_tokens=[0, 2, 0]), "member 0: column token 2 at index 1 cannot be walked from state 0"),
               (dict(col_tokens=[0, 5, 8]), "outside the vocabulary"), (dict(samplers=[(1.0, 0, 1.0, 0), (1.0, -1, 1.0, 0)]), "member 1: sampler: top_k"),
               (dict(rules=[None, (0.0, 0.0, 0.0, 0.0)]), "member 1: rules: repetition_penalty")]


@pytest.mark.parametrize("kw,word", OP_REFUSALS, ids=[w.split(":")[-1].strip().replace(" ", "_")[:24] for _, w in OP_REFUSALS])
def test_the_op_refuses_its_arguments_before_any_device(lnb, kw, word):
    a = dict(segs=[(0, 2), (2, 1)], samplers=[(1.0, 0, 1.0, 0)] * 2, rules=None, counts=None, pos0=[0, 4], col_tokens=[0, 5, 3], automaton=DFA, state0=[0, -1])
    a.update(kw)
    with pytest.raises(lnb.LnbError, match=re.escape(word)):
        lnb.op_spec_automaton_many_accept(np.zeros((3, 8), dtype=np.uint16), **a)


def test_the_call_refuses_its_arguments_before_any_handle(lnb):
    L, i32 = lnb.lib(), C.c_int32
    one = lambda v: (C.c_void_p * 1)(v)
    for smp, n, word in ((None, 1, "lnb_decode_speculative_automaton_many: null argument (samplers)"), (lnb._samplers([(-1.0, 0, 1.0, 0)], 1), 1, "member 0: sampler: temperature"),
                         (lnb._samplers([(1.0, 0, 1.0, 0)], 1), 0, "a call takes 1..128 contexts")):
        assert L.lnb_decode_speculative_automaton_many(one(0x10), n, smp, None, None, None, one(None), (i32 * 1)(0), (i32 * 1)(1), (i32 * 1)(8), 8, 0, (i32 * 8)(),
                                                       (i32 * 1)(), None, None, None, None) < 0
        assert word in L.lnb_last_error().decode()
