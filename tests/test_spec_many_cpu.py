"""Speculative decoding of many contexts (include/lnb.h, lnb_decode_speculative_many): what can be checked without a GPU -- the symbol is declared,
exported and bound in every layer, the info struct has the header's layout, the ABI version did not move, bad arguments are refused with a message
before any handle is dereferenced, and the grant rule (csrc/lnb_specpack.h) equals its brute-force restatement (tests/native/specpack_test.cpp, a
stand-alone program under the address and undefined-behaviour sanitizers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")
NAME = "lnb_decode_speculative_many"


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


def test_the_symbol_is_declared_bound_and_exported(lnb):
    L = lnb.lib()
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    assert NAME in lnb.EXPORTS
    assert re.search(r"\bint\s+%s\s*\(" % NAME, hdr)
    assert hasattr(L, NAME) and len(getattr(L, NAME).argtypes) == 14
    assert callable(lnb.DecodeSpeculativeMany)
    assert re.search(r"#define\s+LNB_ABI_VERSION\s+6\b", hdr) and L.lnb_abi_version() == 6 == lnb.ABI_VERSION


def test_the_info_struct_has_the_headers_layout(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    m = re.search(r"typedef struct lnb_spec_many_info \{ int64_t ([^;]*); \} lnb_spec_many_info;", hdr)
    assert m
    names = [n.strip() for n in m.group(1).split(",")]
    assert names == ["passes", "verify_passes", "columns", "max_columns", "long_passes"]
    assert [f[0] for f in lnb.SpecManyInfo._fields_] == names and all(f[1] is C.c_int64 for f in lnb.SpecManyInfo._fields_)
    assert C.sizeof(lnb.SpecManyInfo) == 8 * len(names) and C.sizeof(lnb.SpecStats) == 32


@pytest.mark.parametrize("rel", ["llama-nuts-and-bolts_amd/host/lnb_host.hpp", "llama-nuts-and-bolts_amd/go/inferencecontext_hip.go", "README.md", "DESIGN.md",
                                 "INTEGRATION.md", "NOTES.md"])
def test_every_layer_and_document_names_the_call(rel):
    assert NAME in open(os.path.join(ROOT, rel)).read(), rel


def _fails(rc, L, *words):
    assert rc < 0
    msg = L.lnb_last_error().decode()
    assert msg, "no error message"
    for w in words:
        assert w in msg, (w, msg)


def test_arguments_are_refused_before_any_handle_is_dereferenced(lnb):
    """The handles below are NULL or point at 64 bytes of 0xFF (a model pointer of all ones: dereferencing it would end the process)."""
    L = lnb.lib()
    junk = [np.full(64, 0xFF, dtype=np.uint8) for _ in range(3)]
    fake = lambda *idx: (C.c_void_p * len(idx))(*[None if i is None else junk[i].ctypes.data for i in idx])
    i32 = lambda *v: np.array(v, dtype=np.int32)
    h = [i32(1, 2, 3), i32(4, 5), i32(6)]
    hist = lambda *idx: (C.c_void_p * len(idx))(*[None if i is None else h[i].ctypes.data for i in idx])
    out = np.zeros((128, 8), dtype=np.int32); ng = np.zeros(128, dtype=np.int32)
    K = dict(history=hist(0, 1, 2), n_history=i32(3, 2, 1), tokens=i32(1, 2, 3), start_pos=i32(4, 3, 2), max_steps=8, col_budget=0, out=out, ng=ng)

    def call(ctxs, n, **kw):
        a = dict(K, **kw)
        p = lambda x: None if x is None else lnb._p(x)
        return L.lnb_decode_speculative_many(ctxs, n, a["history"], p(a["n_history"]), p(a["tokens"]), p(a["start_pos"]), a["max_steps"], a["col_budget"],
                                             p(a["out"]), p(a["ng"]), None, None, None, None)

    _fails(call(None, 3), L, NAME, "null", "ctxs")
    for k, word in (("history", "history"), ("n_history", "n_history"), ("tokens", "tokens"), ("start_pos", "start_pos"), ("out", "out_tokens"), ("ng", "n_generated")):
        _fails(call(fake(0, 1, 2), 3, **{k: None}), L, "null", word)
    for n in (0, -1, 129):
        _fails(call(fake(0, 1, 2), n), L, "1..128")
        _fails(call(None, n), L, NAME)
    _fails(call(fake(0, None, 2), 3), L, "null context at index 1")
    _fails(call(fake(0, 1, 0), 3), L, "context 2 appears twice")
    _fails(call(fake(0, 1, 2), 3, n_history=i32(3, -2, 1)), L, "member 1", "negative history length")
    _fails(call(fake(0, 1, 2), 3, history=hist(0, None, 2)), L, "member 1", "null history")
    for ms in (0, -3):
        _fails(call(fake(0, 1, 2), 3, max_steps=ms), L, "max_steps must be positive")
    for b in (-1, 1, 2, 129, 1000):
        _fails(call(fake(0, 1, 2), 3, col_budget=b), L, "col_budget", "3..128")
    with pytest.raises(lnb.LnbError, match="2 contexts, 1 histories"):
        lnb.DecodeSpeculativeMany([object(), object()], [[1, 2]], [0, 0], [0, 0], 4)


def test_the_grant_rule_under_the_sanitizers(tmp_path):
    """csrc/lnb_specpack.h is plain C++ that includes nothing: n = 1..128, wants 0..15, budgets n..128 against the rule handed out one column at a time"""
    src = os.path.join(ROOT, "tests", "native", "specpack_test.cpp")
    hdr = open(os.path.join(PKG, "csrc", "lnb_specpack.h")).read()
    code = re.sub(r"//.*", "", hdr)
    assert "hip" not in code.lower() and "#include" not in code
    exe = str(tmp_path / "specpack_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "specpack_test: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_makefile_names_the_headers():
    hdrs = re.search(r"^HDRS = (.*)$", open(os.path.join(PKG, "csrc", "Makefile")).read(), re.M).group(1)
    assert "lnb_specpack.h" in hdrs and "lnb_spec_many.h" in hdrs
