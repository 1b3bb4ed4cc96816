"""The feed plan of a batched step (csrc/lnb_batchplan.h): which of the five products of a block and the head run on the column feed and which as
rows, and in how many column groups, as a function of the width, the matrix-core copy and LNB_BATCH_GROUPS.  The header is plain C++ without HIP:
tests/native/batchplan_test.cpp, a stand-alone program under the address and undefined-behaviour sanitizers, walks it against the written-out table."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")


def test_feed_plan_under_the_sanitizers(tmp_path):
    """n = 1..128 x copy {0, 1} x knob {0, 1, 7}: feeds, group count and the derived layout code 0 / 1 / 2 against the table"""
    src = os.path.join(ROOT, "tests", "native", "batchplan_test.cpp")
    hdr = open(os.path.join(PKG, "csrc", "lnb_batchplan.h")).read()
    assert "hip" not in hdr.lower()
    assert "#include" not in re.sub(r"//.*", "", hdr)             # the knob is an argument: the header reads no environment and includes nothing
    exe = str(tmp_path / "batchplan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "batchplan_test: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_makefile_and_the_design_document_name_the_header():
    assert "lnb_batchplan.h" in re.search(r"^HDRS = (.*)$", open(os.path.join(PKG, "csrc", "Makefile")).read(), re.M).group(1)
    assert "lnb_batchplan.h" in open(os.path.join(ROOT, "DESIGN.md")).read()
