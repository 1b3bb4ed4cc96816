"""The lossless 13-bit planar weight copy (csrc/lnb_wpack.h) on the host: every bf16 pattern survives pack -> unpack in a window that admits it, the
matrices the format cannot hold are refused with their reason, and the four-at-a-time decode the gate|up kernel runs gives the scalar definition's bits
(tests/native/wpack_test.cpp, a stand-alone program under the address and undefined-behaviour sanitizers).  Plus what binds the format to the library
without a GPU: the symbols, the knob and the Makefile."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")


def test_format_on_the_host_under_the_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "wpack_test.cpp")
    exe = str(tmp_path / "wpack_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wpack_test: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_header_is_plain_cxx_and_the_makefile_names_it():
    hdr = open(os.path.join(PKG, "csrc", "lnb_wpack.h")).read()
    assert "hip_runtime" not in hdr and set(re.findall(r"#include <(\S+)>", hdr)) == {"stdint.h", "stddef.h"}
    hdrs = re.search(r"^HDRS = (.*)$", open(os.path.join(PKG, "csrc", "Makefile")).read(), re.M).group(1)
    assert "lnb_wpack.h" in hdrs.split()


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    return _lnb


def test_queries_and_knob_are_declared_exported_and_bound(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    L = lnb.lib()
    for name in ("lnb_model_wpack_bytes", "lnb_model_wpack_info", "lnb_op_rmsnorm_gate_up"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in lnb.EXPORTS and hasattr(L, name)
    assert L.lnb_model_wpack_bytes(None) == 0
    assert L.lnb_model_wpack_info(None, None) != 0 and b"null" in L.lnb_last_error()
    knobs = open(os.path.join(PKG, "csrc", "lnb_knobs.h")).read()
    assert re.search(r"X\(W13_PACKED,\s*1,\s*LIVE,", knobs)


def test_op_refuses_bad_arguments_before_touching_a_device(lnb):
    L = lnb.lib()
    assert L.lnb_op_rmsnorm_gate_up(0, None, None, 1e-5, None, None, None, 56, 256, 1, None) != 0
    assert b"null" in L.lnb_last_error()
