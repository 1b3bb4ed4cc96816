"""The token automaton of the sampling loops (include/lnb.h: lnb_ctx_set_automaton) without a GPU: the six names, the refusals that come before any handle or
device is touched, and the inputs of tests/test_gpu_automaton.py's operator test -- which must be such that a kernel ignoring the mask cannot pass."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import automaton_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lnb_automaton_create", "lnb_automaton_destroy", "lnb_automaton_info", "lnb_ctx_set_automaton", "lnb_ctx_automaton_state", "lnb_op_sample_automaton"]


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


def test_the_six_functions_are_declared_bound_and_exported(lnb):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lnb.h")).read(), flags=re.S)
    L = C.CDLL(os.path.join(ROOT, "llama-nuts-and-bolts_amd", "liblnb_hip.so"))
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in lnb.EXPORTS and hasattr(L, n), n


RP, ET, EN = np.array([0, 2, 2], dtype=np.int64), np.array([1, 5], dtype=np.int32), np.array([1, 0], dtype=np.int32)
CREATE = [(dict(row_ptr=None), "(row_ptr)"), (dict(edge_token=None), "(edge_token)"), (dict(edge_next=None), "(edge_next)"), (dict(out=None), "(out)"),
          (dict(n_states=0), "n_states must be >= 1"), (dict(row_ptr=np.array([1, 2, 2], dtype=np.int64)), "row_ptr[0] must be 0"),
          (dict(row_ptr=np.array([0, 2, 1], dtype=np.int64)), "row_ptr must not decrease"), (dict(), "(m)")]


@pytest.mark.parametrize("bad,word", CREATE, ids=[w for _, w in CREATE])
def test_create_checks_its_arguments_before_the_model_handle(lnb, bad, word):
    L = lnb.lib()
    a = dict(row_ptr=RP, edge_token=ET, edge_next=EN, n_states=2, out=C.c_void_p())
    a.update(bad)
    ptr = lambda v: None if v is None else lnb._p(v)
    rc = L.lnb_automaton_create(None, a["n_states"], ptr(a["row_ptr"]), ptr(a["edge_token"]), ptr(a["edge_next"]), None if a["out"] is None else C.byref(a["out"]))
    assert rc < 0 and word in L.lnb_last_error().decode(), L.lnb_last_error().decode()


def test_the_context_calls_and_the_op_refuse_before_any_device(lnb):
    L = lnb.lib()
    v = C.c_int(0)
    for call, word in ((lambda: L.lnb_ctx_set_automaton(None, None, 0), "lnb_ctx_set_automaton: null argument (c)"),
                       (lambda: L.lnb_ctx_automaton_state(None, C.byref(v)), "lnb_ctx_automaton_state"), (lambda: L.lnb_automaton_info(None, None, None, None), "lnb_automaton_info")):
        assert call() < 0 and word in L.lnb_last_error().decode()
    assert L.lnb_automaton_destroy(None) == 0
    row = np.zeros((1, 8), dtype=np.uint16)
    dfa = (RP, ET, EN)
    for kw, word in ((dict(states=[2]), "state 2 is outside [0, 2)"), (dict(states=[-1]), "outside [0, 2)"), (dict(samplers=[(-1.0, 0, 1.0, 0)]), "temperature"),
                     (dict(automaton=(np.array([0, 2, 1]), ET, EN)), "row_ptr must not decrease"), (dict(rules=[(0.0, 0.0, 0.0, 0.0)]), "repetition_penalty")):
        a = dict(samplers=[(1.0, 0, 1.0, 0)], automaton=dfa, states=[0], pos=[0])
        a.update(kw)
        with pytest.raises(lnb.LnbError, match=re.escape(word)):
            lnb.op_sample_automaton(row, **a)


@pytest.mark.parametrize("V", [1000, 1024, 1057, 131072])
def test_the_operator_inputs_defeat_a_kernel_that_ignores_the_mask(V):
    dfa, cases = ar.op_cases(V)
    assert sum(tok != plain for *_, tok, _, plain in cases) * 2 >= len(cases)
    assert sum(plain not in ar.allowed(dfa, state) for *_, state, _, _, plain in cases) * 2 >= len(cases)
    for row, counts, smp, rules, pos, state, tok, nxt, plain in cases:
        assert tok == {0: V // 3, 1: plain}.get(state, tok)      # the one allowed token whatever the draw; everything allowed: the rules' own token
        assert tok in ar.allowed(dfa, state) and 0 <= nxt < ar.N_STATES
