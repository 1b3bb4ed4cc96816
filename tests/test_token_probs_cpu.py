"""Token probabilities (include/lnb.h, lnb_ctx_set_token_probs / lnb_forward_score / lnb_op_token_probs): what can be checked without a GPU --
the constant the bindings share with the header, and that every new entry point refuses null and out-of-range arguments with a message
instead of touching memory or reaching for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


def test_max_top_k_is_the_same_in_the_header_and_the_binding(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    m = re.search(r"#define\s+LNB_MAX_TOP_K\s+(\d+)", hdr)
    assert m, "LNB_MAX_TOP_K missing from include/lnb.h"
    assert int(m.group(1)) == lnb.MAX_TOP_K == 16


def test_new_symbols_are_declared_and_exported(lnb):
    L = lnb.lib()
    for n in ("lnb_ctx_set_token_probs", "lnb_ctx_read_token_probs", "lnb_ctx_token_prob_walks", "lnb_forward_score", "lnb_op_token_probs"):
        assert n in lnb.EXPORTS
        assert hasattr(L, n)


def _fails(rc, L, *words):
    assert rc < 0
    msg = L.lnb_last_error().decode()
    assert msg, "no error message"
    for w in words:
        assert w in msg, (w, msg)


def test_context_entry_points_refuse_null_handles(lnb):
    L = lnb.lib()
    buf = np.zeros(64, dtype=np.float64)
    _fails(L.lnb_ctx_set_token_probs(None, 4), L, "null")
    _fails(L.lnb_ctx_read_token_probs(None, 0, 1, lnb._p(buf), lnb._p(buf), lnb._p(buf), lnb._p(buf)), L, "null")
    n = C.c_int(0)
    _fails(L.lnb_ctx_token_prob_walks(None, C.byref(n)), L, "null")
    tok = np.zeros(4, dtype=np.int32)
    am = C.c_int32(0)
    _fails(L.lnb_forward_score(None, lnb._p(tok), 4, 0, lnb._p(tok), lnb._p(buf), lnb._p(buf), lnb._p(buf), C.byref(am)), L, "null")


def test_op_token_probs_checks_its_arguments_before_any_device(lnb):
    L = lnb.lib()
    x = np.zeros((2, 10), dtype=np.uint16)
    ids = np.zeros(64, dtype=np.int32); f = np.zeros(64, dtype=np.float32); lz = np.zeros(8, dtype=np.float64)
    w = C.c_int(0)
    # null logits, null log_z, null top-k outputs with k > 0, targets without target_prob
    _fails(L.lnb_op_token_probs(0, None, 2, 10, 4, None, 0, lnb._p(ids), lnb._p(f), lnb._p(f), None, lnb._p(lz), C.byref(w)), L, "null")
    _fails(L.lnb_op_token_probs(0, lnb._p(x), 2, 10, 4, None, 0, lnb._p(ids), lnb._p(f), lnb._p(f), None, None, C.byref(w)), L, "null")
    _fails(L.lnb_op_token_probs(0, lnb._p(x), 2, 10, 4, None, 0, None, lnb._p(f), lnb._p(f), None, lnb._p(lz), C.byref(w)), L, "null")
    tg = np.zeros(2, dtype=np.int32)
    _fails(L.lnb_op_token_probs(0, lnb._p(x), 2, 10, 0, lnb._p(tg), 0, None, None, None, None, lnb._p(lz), C.byref(w)), L, "null")
    # sizes and ranges
    _fails(L.lnb_op_token_probs(0, lnb._p(x), 0, 10, 4, None, 0, lnb._p(ids), lnb._p(f), lnb._p(f), None, lnb._p(lz), C.byref(w)), L, "empty")
    _fails(L.lnb_op_token_probs(0, lnb._p(x), 2, 0, 4, None, 0, lnb._p(ids), lnb._p(f), lnb._p(f), None, lnb._p(lz), C.byref(w)), L, "empty")
    for k in (-1, 17):
        _fails(L.lnb_op_token_probs(0, lnb._p(x), 2, 10, k, None, 0, lnb._p(ids), lnb._p(f), lnb._p(f), None, lnb._p(lz), C.byref(w)), L, "top_k", "0..16")
    tg = np.array([3, 10], dtype=np.int32)
    _fails(L.lnb_op_token_probs(0, lnb._p(x), 2, 10, 0, lnb._p(tg), 0, None, None, None, lnb._p(f), lnb._p(lz), C.byref(w)), L, "outside")


def test_op_token_probs_without_a_device_is_an_error_not_a_fallback(lnb):
    if os.path.exists("/dev/kfd"):                           # (a GPU box: the same call runs the kernel; tests/test_gpu_token_probs.py checks it)
        return
    with pytest.raises(lnb.LnbError, match="device"):
        lnb.op_token_probs(np.zeros((1, 16), dtype=np.uint16), 4)
