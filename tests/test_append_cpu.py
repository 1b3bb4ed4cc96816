"""Causal multi-row append (include/lnb.h, lnb_forward_append / lnb_forward_score_append): what can be checked without a GPU -- the symbols
are declared, exported and bound, the ABI version did not move, and bad arguments are refused with a message before any handle or device
is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lnb_forward_append", "lnb_forward_score_append")


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


def test_new_symbols_are_declared_bound_and_exported(lnb):
    L = lnb.lib()
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    for n in NEW:
        assert n in lnb.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
        assert hasattr(L, n)
        assert getattr(L, n).argtypes, n
    assert len(L.lnb_forward_append.argtypes) == 6 and len(L.lnb_forward_score_append.argtypes) == 9


def test_abi_version_stays_6(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    assert re.search(r"#define\s+LNB_ABI_VERSION\s+6\b", hdr)
    assert lnb.lib().lnb_abi_version() == 6


def test_python_layer_has_the_append_methods(lnb):
    import inspect
    assert callable(lnb.InferenceContext.ForwardAppend) and callable(lnb.InferenceContext.score_append)
    sig = inspect.signature(lnb.InferenceEngine.__init__)
    assert sig.parameters["prefill_chunk"].default == 0
    with pytest.raises(lnb.LnbError, match="prefill_chunk"):
        lnb.InferenceEngine(None, 16, prefill_chunk=-1)


def _fails(rc, L, *words):
    assert rc < 0
    msg = L.lnb_last_error().decode()
    assert msg, "no error message"
    for w in words:
        assert w in msg, (w, msg)


def test_forward_append_checks_its_arguments_before_the_handle(lnb):
    L = lnb.lib()
    t = np.arange(8, dtype=np.int32)
    lg = np.zeros(8, dtype=np.float32)
    am = C.c_int32(0)
    call = lambda ctx, tok, seq, pos: L.lnb_forward_append(ctx, tok, seq, pos, lnb._p(lg), C.byref(am))
    _fails(call(None, None, 8, 0), L, "lnb_forward_append", "null")
    _fails(call(None, lnb._p(t), 0, 0), L, "lnb_forward_append", "seq must be positive")
    _fails(call(None, lnb._p(t), -3, 0), L, "seq must be positive")
    _fails(call(None, lnb._p(t), 8, -1), L, "negative start position")
    _fails(call(None, lnb._p(t), 8, 0), L, "null")                   # the handle is looked at last


def test_forward_score_append_checks_its_arguments_before_the_handle(lnb):
    L = lnb.lib()
    t = np.arange(8, dtype=np.int32)
    tl, tp, lz = np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.float64)
    am = C.c_int32(0)
    call = lambda ctx, tok, seq, pos, tg=lnb._p(t), a=lnb._p(tl), b=lnb._p(tp), z=lnb._p(lz): L.lnb_forward_score_append(
        ctx, tok, seq, pos, tg, a, b, z, C.byref(am))
    _fails(call(None, None, 8, 0), L, "lnb_forward_score_append", "null")
    _fails(call(None, lnb._p(t), 8, 0, tg=None), L, "null")
    _fails(call(None, lnb._p(t), 8, 0, a=None), L, "null")
    _fails(call(None, lnb._p(t), 8, 0, b=None), L, "null")
    _fails(call(None, lnb._p(t), 8, 0, z=None), L, "null")
    _fails(call(None, lnb._p(t), 0, 0), L, "seq must be positive")
    _fails(call(None, lnb._p(t), 8, -2), L, "negative start position")
    _fails(call(None, lnb._p(t), 8, 0), L, "null")
