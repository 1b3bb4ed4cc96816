"""The one-token GEMV geometry table (csrc/lnb_gemv_geom.h): the one statement of which chain / quad kernel instantiation serves a block height, what it
needs of the LDS and the staging registers, and which tally row and report form it has.  The header is plain C++ without HIP: tests/native/gemv_geom_test.cpp,
a stand-alone program under the address and undefined-behaviour sanitizers, checks the table against expectations recorded from the launch functions that
spelled these geometries out by hand (profiles/gemv_geometry.md)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")
HDR = "lnb_gemv_geom.h"


def _includes(name):
    return re.findall(r"#include\s*(\S+)", re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", name)).read()))


def test_the_table_keeps_what_the_hand_written_launches_decided(tmp_path):
    """unique rows; one reachable row per fused report form; chunks or refusal at K = 4096, 8192, 14336, 28672; the packed kernels' longest rows; rw 4 / rw 24"""
    src = os.path.join(ROOT, "tests", "native", "gemv_geom_test.cpp")
    exe = str(tmp_path / "gemv_geom_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gemv_geom_test: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_header_has_no_hip_and_the_makefile_and_the_design_document_name_it():
    own = {'"lnb_seqsum.h"', '"lnb_forms.h"'}
    assert all(inc in own or re.fullmatch(r"<[a-z_.]+>", inc) for inc in _includes(HDR)), _includes(HDR)
    for name in (HDR, "lnb_seqsum.h", "lnb_forms.h"):
        assert not any("hip" in inc.lower() for inc in _includes(name)), name
    assert HDR in re.search(r"^HDRS = (.*)$", open(os.path.join(PKG, "csrc", "Makefile")).read(), re.M).group(1)
    assert HDR in open(os.path.join(ROOT, "DESIGN.md")).read()
    for user in ("lnb_kernels.hip", "lnb_api.cpp"):
        assert '"%s"' % HDR in _includes(user), user
