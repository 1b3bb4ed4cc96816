"""The LM head's 13-bit packed stream (csrc/lnb_wpack.h, the wpack_head_* functions) on the host: a matrix packed through the head addressing from the
resident 64-row layout comes back bit for bit the way the kernel consumes it, padding is zeros, and the stage and byte counts are what the kernel and the
allocation assume (tests/native/wpack_head_test.cpp, a stand-alone program under the address and undefined-behaviour sanitizers).  Plus what binds the
packed head to the library without a GPU: the symbols, the knob, the form row."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")


def test_head_addressing_on_the_host_under_the_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "wpack_head_test.cpp")
    exe = str(tmp_path / "wpack_head_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wpack_head_test: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_test_program_includes_only_the_format_header():
    src = open(os.path.join(ROOT, "tests", "native", "wpack_head_test.cpp")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["../../llama-nuts-and-bolts_amd/csrc/lnb_wpack.h"]


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    return _lnb


def test_queries_knob_and_form_are_declared_exported_and_bound(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    L = lnb.lib()
    for name in ("lnb_model_wpack_head_bytes", "lnb_model_wpack_head_status", "lnb_op_rmsnorm_head"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in lnb.EXPORTS and hasattr(L, name)
    assert L.lnb_model_wpack_head_bytes(None) == 0
    assert L.lnb_model_wpack_head_status(None) == -1 and b"null" in L.lnb_last_error()
    assert re.search(r"X\(HEAD_PACKED,\s*1,\s*LIVE,", open(os.path.join(PKG, "csrc", "lnb_knobs.h")).read())
    # the head's form is a top-level name of its own: "gemv_chain_pk" (gate|up) must not stand for it
    names = lnb.form_names()
    assert "gemv_head_pk" in names and not any(n != "gemv_head_pk" and (n.startswith("gemv_head_pk.") or "gemv_head_pk".startswith(n + ".")) for n in names)
    assert re.search(r"#define\s+LNB_ABI_VERSION\s+6\b", hdr) and L.lnb_abi_version() == 6        # additions only


def test_op_refuses_bad_arguments_before_touching_a_device(lnb):
    L = lnb.lib()
    assert L.lnb_op_rmsnorm_head(0, None, None, 1e-5, None, None, 128, 256, 1, 0, None) != 0
    assert b"null" in L.lnb_last_error()
