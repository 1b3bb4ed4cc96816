"""Speculative greedy decoding (include/lnb.h, lnb_ctx_set_draft / lnb_decode_speculative_until / lnb_op_ngram_draft): what can be checked
without a GPU -- the symbols, the constant the binding shares with the header, and that bad arguments are refused with a message before
any handle or device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lnb_ctx_set_draft", "lnb_decode_speculative_until", "lnb_op_ngram_draft")


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
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(L, n)
        assert getattr(L, n).argtypes, n


def test_max_draft_is_the_same_in_the_header_and_the_binding(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    m = re.search(r"#define\s+LNB_MAX_DRAFT\s+(\d+)", hdr)
    assert m, "LNB_MAX_DRAFT missing from include/lnb.h"
    assert int(m.group(1)) == lnb.MAX_DRAFT == 15


def test_stats_struct_matches_the_header(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    m = re.search(r"typedef struct (?:lnb_spec_stats )?\{\s*int64_t ([^;]+);\s*\}\s*lnb_spec_stats;", hdr)
    assert m
    assert [f.strip() for f in m.group(1).split(",")] == [n for n, _ in lnb.SpecStats._fields_]
    assert C.sizeof(lnb.SpecStats) == 32


def _fails(rc, L, *words):
    assert rc < 0
    msg = L.lnb_last_error().decode()
    assert msg, "no error message"
    for w in words:
        assert w in msg, (w, msg)


def test_set_draft_checks_its_arguments_before_the_handle(lnb):
    L = lnb.lib()
    corpus = np.arange(8, dtype=np.int32)
    _fails(L.lnb_ctx_set_draft(None, 16, 1, 4, lnb._p(corpus), 8), L, "max_draft", "0..15")
    _fails(L.lnb_ctx_set_draft(None, -1, 1, 4, lnb._p(corpus), 8), L, "max_draft")
    _fails(L.lnb_ctx_set_draft(None, 4, 0, 4, lnb._p(corpus), 8), L, "ngram_min")
    _fails(L.lnb_ctx_set_draft(None, 4, 5, 4, lnb._p(corpus), 8), L, "ngram_min <= ngram_max")
    _fails(L.lnb_ctx_set_draft(None, 4, 1, 17, lnb._p(corpus), 8), L, "ngram_max <= 16")
    _fails(L.lnb_ctx_set_draft(None, 4, 1, 4, lnb._p(corpus), -1), L, "negative")
    _fails(L.lnb_ctx_set_draft(None, 4, 1, 4, None, 8), L, "null")
    _fails(L.lnb_ctx_set_draft(None, 4, 1, 4, lnb._p(corpus), 8), L, "null")
    _fails(L.lnb_ctx_set_draft(None, 0, 1, 4, None, 0), L, "null")


def test_decode_speculative_checks_its_arguments_before_the_handle(lnb):
    L = lnb.lib()
    h = np.arange(8, dtype=np.int32)
    out = np.zeros(16, dtype=np.int32)
    n, fin, ms, st = C.c_int(0), C.c_int(0), C.c_float(0), lnb.SpecStats()
    call = lambda ctx, hist, nh, steps, o=lnb._p(out), ng=C.byref(n): L.lnb_decode_speculative_until(
        ctx, hist, nh, 1, 8, steps, o, ng, C.byref(fin), C.byref(st), C.byref(ms))
    _fails(call(None, lnb._p(h), -1, 8), L, "negative")
    _fails(call(None, lnb._p(h), 8, 0), L, "max_steps")
    _fails(call(None, lnb._p(h), 8, 8), L, "null")
    _fails(call(None, None, 8, 8), L, "null")
    _fails(call(None, lnb._p(h), 8, 8, o=None), L, "null")
    _fails(call(None, lnb._p(h), 8, 8, ng=None), L, "null")


def test_op_ngram_draft_checks_its_arguments_before_any_device(lnb):
    L = lnb.lib()
    t = np.arange(8, dtype=np.int32)
    out = np.zeros(16, dtype=np.int32)
    n = C.c_int(0)
    op = lambda text, nt, corpus, nc, nmin, nmax, md, o=lnb._p(out): L.lnb_op_ngram_draft(0, text, nt, corpus, nc, nmin, nmax, md, o, C.byref(n))
    _fails(op(lnb._p(t), -1, None, 0, 1, 4, 4), L, "negative")
    _fails(op(lnb._p(t), 8, None, -2, 1, 4, 4), L, "negative")
    _fails(op(lnb._p(t), 8, None, 0, 1, 4, 16), L, "max_draft")
    _fails(op(lnb._p(t), 8, None, 0, 0, 4, 4), L, "ngram_min")
    _fails(op(lnb._p(t), 8, None, 0, 3, 2, 4), L, "ngram_min")
    _fails(op(None, 8, None, 0, 1, 4, 4), L, "null")
    _fails(op(lnb._p(t), 8, None, 5, 1, 4, 4), L, "null")
    _fails(op(lnb._p(t), 8, None, 0, 1, 4, 4, o=None), L, "null")


def test_op_ngram_draft_without_a_device_is_an_error_not_a_fallback(lnb):
    if os.path.exists("/dev/kfd"):                           # (a GPU box: the same call runs the kernel; tests/test_gpu_speculative.py checks it)
        return
    with pytest.raises(lnb.LnbError, match="device"):
        lnb.op_ngram_draft([1, 2, 1], [], 1, 2, 4)
