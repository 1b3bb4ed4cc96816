"""Who releases a device resource of the host layer (csrc/lnb_own.h): the owner of one handle, the buffer grown on demand, the arena of one scope and
the table of captured graphs.  The header is plain C++ without HIP: tests/native/own_test.cpp, a stand-alone program under the address and
undefined-behaviour sanitizers, instantiates every type with counting acquire and release functions whose i-th acquire can be told to fail."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")


def test_owning_types_release_exactly_once_under_the_sanitizers(tmp_path):
    """single owner: scope exit, reset, move-assignment over a full owner, a moved-from owner; growable buffer: fits / release-then-acquire / empty after a
    failed growth; arena: a failure at each of eight allocations; graph table: distinct slots, drop(form), drop_all, refill, destruction"""
    src = os.path.join(ROOT, "tests", "native", "own_test.cpp")
    hdr = open(os.path.join(PKG, "csrc", "lnb_own.h")).read()
    code = re.sub(r"//.*", "", hdr)
    assert "hip" not in hdr.lower() and "getenv" not in hdr
    assert all(re.fullmatch(r"<[a-z_]+>", inc) for inc in re.findall(r"#include\s*(\S+)", code))      # standard headers at most
    exe = str(tmp_path / "own_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "own_test: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_makefile_and_the_design_document_name_the_header():
    assert "lnb_own.h" in re.search(r"^HDRS = (.*)$", open(os.path.join(PKG, "csrc", "Makefile")).read(), re.M).group(1)
    assert "lnb_own.h" in open(os.path.join(ROOT, "DESIGN.md")).read()
