"""Ragged append to many contexts (include/lnb.h, lnb_forward_append_many / lnb_model_append_many_info): what can be checked without a GPU -- the
symbols are declared, exported and bound in every layer, the ABI version did not move, the pass-width knob is in the table and the document with one
default, bad arguments are refused with a message before any handle is dereferenced, and the host-only row packing (csrc/lnb_rowpack.h) walks every
row exactly once (tests/native/rowpack_test.cpp, a stand-alone program under the address and undefined-behaviour sanitizers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")
NEW = ("lnb_forward_append_many", "lnb_model_append_many_info")


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
    assert len(L.lnb_forward_append_many.argtypes) == 7 and len(L.lnb_model_append_many_info.argtypes) == 4
    assert callable(lnb.ForwardAppendMany) and callable(lnb.LlamaTransformer.append_many_info)


def test_abi_version_stays_6(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    assert re.search(r"#define\s+LNB_ABI_VERSION\s+6\b", hdr)
    assert lnb.lib().lnb_abi_version() == 6 == lnb.ABI_VERSION


@pytest.mark.parametrize("rel", ["llama-nuts-and-bolts_amd/host/lnb_host.hpp", "llama-nuts-and-bolts_amd/go/inferencecontext_hip.go", "README.md", "DESIGN.md",
                                 "INTEGRATION.md"])
def test_every_layer_and_document_names_the_call(rel):
    assert "lnb_forward_append_many" in open(os.path.join(ROOT, rel)).read(), rel


def test_the_header_says_that_max_rows_does_not_limit_the_call():
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    sec = hdr.split("ragged append to many contexts", 1)[1].split("int lnb_forward_append_many", 1)[0]
    assert re.search(r"max_rows does NOT limit n_rows", sec)


def test_the_knob_is_in_the_table_and_the_document_with_one_default():
    tab = open(os.path.join(PKG, "csrc", "lnb_knobs.h")).read()
    m = re.search(r"^\s*X\(APPEND_MANY_COLS,\s*(\d+),\s*(ONCE|LIVE),", tab, re.M)
    assert m and m.group(1) == "128" and m.group(2) == "LIVE"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read().split("## Environment knobs", 1)[1]
    d = re.search(r"^\| `LNB_APPEND_MANY_COLS` \| (\d+) \| (\w+) \|", doc, re.M)
    assert d and d.group(1) == m.group(1) and d.group(2) == m.group(2)


def _fails(rc, L, *words):
    assert rc < 0
    msg = L.lnb_last_error().decode()
    assert msg, "no error message"
    for w in words:
        assert w in msg, (w, msg)


def test_arguments_are_refused_before_any_handle_is_dereferenced(lnb, monkeypatch):
    """The handles below are NULL or point at 64 bytes of 0xFF (a model pointer of all ones: dereferencing it would end the process)."""
    L = lnb.lib()
    monkeypatch.delenv("LNB_APPEND_MANY_COLS", raising=False)
    junk = [np.full(64, 0xFF, dtype=np.uint8) for _ in range(3)]
    fake = lambda *idx: (C.c_void_p * len(idx))(*[None if i is None else junk[i].ctypes.data for i in idx])
    tok = np.arange(16, dtype=np.int32)
    am = np.zeros(128, dtype=np.int32)
    i32 = lambda *v: np.array(v, dtype=np.int32)

    def call(ctxs, n, tokens=tok, rows=i32(1, 5, 7), pos=i32(0, 37, 20)):
        p = lambda a: None if a is None else lnb._p(a)
        return L.lnb_forward_append_many(ctxs, n, p(tokens), p(rows), p(pos), None, lnb._p(am))

    _fails(call(None, 3), L, "lnb_forward_append_many", "null", "ctxs")
    _fails(call(fake(0, 1, 2), 3, tokens=None), L, "null", "tokens")
    _fails(call(fake(0, 1, 2), 3, rows=None), L, "null", "n_rows")
    _fails(call(fake(0, 1, 2), 3, pos=None), L, "null", "start_pos")
    _fails(call(fake(0, 1, 2), 0), L, "1..128")
    _fails(call(fake(0, 1, 2), -1), L, "1..128")
    _fails(call(fake(0, 1, 2), 129), L, "1..128")
    _fails(call(fake(0, None, 2), 3), L, "null context at index 1")
    _fails(call(fake(0, 1, 2), 3, rows=i32(1, 0, 7)), L, "member 1", "n_rows must be positive")
    _fails(call(fake(0, 1, 2), 3, rows=i32(1, 5, -7)), L, "member 2", "n_rows must be positive")
    _fails(call(fake(0, 1, 2), 3, pos=i32(0, -1, 20)), L, "member 1", "negative start position")
    _fails(call(fake(0, 1, 0), 3), L, "context 2 appears twice")
    for bad in ("0", "129", "-5"):                            # the pass width is read per call (LIVE) and checked before the handles as well
        monkeypatch.setenv("LNB_APPEND_MANY_COLS", bad)
        _fails(call(fake(0, 1, 2), 3), L, "LNB_APPEND_MANY_COLS", "1..128")
    monkeypatch.delenv("LNB_APPEND_MANY_COLS")
    _fails(L.lnb_model_append_many_info(None, None, None, None), L, "lnb_model_append_many_info", "null")
    with pytest.raises(lnb.LnbError, match="2 contexts, 1 token lists"):
        lnb.ForwardAppendMany([object(), object()], [[1, 2]], [0, 0])


def test_row_packing_under_the_sanitizers(tmp_path):
    """csrc/lnb_rowpack.h is plain C++ without HIP: the stand-alone program walks it over W in {1, 5, 16, 17, 128} against a brute-force enumeration"""
    src = os.path.join(ROOT, "tests", "native", "rowpack_test.cpp")
    hdr = open(os.path.join(PKG, "csrc", "lnb_rowpack.h")).read()
    assert "hip" not in re.sub(r"//.*", "", hdr).lower()
    exe = str(tmp_path / "rowpack_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rowpack_test: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
