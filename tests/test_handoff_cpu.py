"""What crosses a pipeline stage boundary, and the mailbox of the in-process transport (csrc/lnb_handoff.h): per hand-off the peer rank, the token
hop and the segments (buffer, bytes), and which send fits which receive.  The header is plain C++ without HIP: tests/native/handoff_test.cpp, a
stand-alone program under the address and undefined-behaviour sanitizers, walks it against the written-out tables."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")


def test_handoff_plans_and_mailbox_under_the_sanitizers(tmp_path):
    """worlds 1, 2, 3, 8 x cuts between blocks / behind an attention part / behind a gate/up part x every rank x send, receive x sequence, batch;
    the mailbox: both posting orders, two queued sequences in order, the four refusals with their texts and what the queues hold afterwards"""
    src = os.path.join(ROOT, "tests", "native", "handoff_test.cpp")
    hdr = open(os.path.join(PKG, "csrc", "lnb_handoff.h")).read()
    code = re.sub(r"//.*", "", hdr)
    assert "hip" not in hdr.lower() and "getenv" not in hdr
    assert all(re.fullmatch(r"<[a-z_]+>", inc) for inc in re.findall(r"#include\s*(\S+)", code))      # standard headers at most
    exe = str(tmp_path / "handoff_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "handoff_test: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_makefile_and_the_design_document_name_the_header():
    assert "lnb_handoff.h" in re.search(r"^HDRS = (.*)$", open(os.path.join(PKG, "csrc", "Makefile")).read(), re.M).group(1)
    assert "lnb_handoff.h" in open(os.path.join(ROOT, "DESIGN.md")).read()
