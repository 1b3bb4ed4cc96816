"""The LNB_* environment knobs of the shared library live in one table (csrc/lnb_knobs.h): its parse rule and lifetimes on the host, the table
against INTEGRATION.md's "Environment knobs" section, and every LNB_* name a test or tool sets against the names something can read."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llama-nuts-and-bolts_amd", "csrc")

# LNB_* variables read outside the shared library: by lnb.py / pipeline.py / bench.py, by the tests themselves and by tests/native/host_mirror_test.cpp
PYTHON_SIDE = {"LNB_SO", "LNB_MODEL_DIR", "LNB_FORCE_PIPELINE", "LNB_FORCE_PREFLIGHT", "LNB_PREFLIGHT_TIMEOUT", "LNB_PIPELINE_BACKEND",
               "LNB_PIPELINE_BATCH", "LNB_PIPELINE_OVERLAP", "LNB_PIPELINE_PROBE", "LNB_DRY_RUN_FAIL_RANK", "LNB_GOLDEN_TINY",
               "LNB_STOP_IDS", "LNB_CHUNK"}
PYTHON_SIDE_PREFIXES = ("LNB_TEST_",)
# names that nothing reads any more, and the one place that still sets each: the round-5 visit script's A/B of an Infinity-Cache prefetch whose
# knobs left the library with the experiment.  Kept as the record of that visit; a new entry here needs the same kind of reason.
KNOWN_STALE = {"tools/gpu_r05.sh": {"LNB_MALL_EVERY", "LNB_MALL_ATTN_UNITS", "LNB_MALL_WO_UNITS"}}


def table_names():
    hdr = open(os.path.join(CSRC, "lnb_knobs.h")).read()
    names = re.findall(r"^\s*X\((\w+),\s*[^,]+,\s*(?:ONCE|LIVE),\s*\"", hdr, re.M)
    assert len(names) >= 40 and len(names) == len(set(names))
    return {"LNB_" + n for n in names}


def test_knob_table_on_the_host(tmp_path):
    exe = str(tmp_path / "knobs_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "native", "knobs_test.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("LNB_")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "knobs_test: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_table_and_document_list_the_same_knobs_and_nothing_else_reads_the_environment():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc.split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    documented = re.findall(r"^\| `(LNB_\w+)` \|", sec, re.M)
    assert len(documented) == len(set(documented))
    assert set(documented) == table_names()
    for path in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(path) != "lnb_knobs.h" and os.path.isfile(path):
            assert 'getenv("LNB_' not in open(path, errors="replace").read(), path


def names_set_by(path):
    txt = open(path, errors="replace").read()
    if path.endswith(".sh"):
        return set(re.findall(r"(?<![\w$])(LNB_\w+)=", txt))
    found = set(re.findall(r"""(?:setenv\(|environ\[|environ\.setdefault\()\s*["'](LNB_\w+)["']""", txt))
    for call in re.findall(r"dict\(\s*(?:os\.environ|env)\s*,([^()]*(?:\([^()]*\)[^()]*)*)\)", txt):
        found |= set(re.findall(r"\b(LNB_\w+)\s*=", call))
    return found | set(re.findall(r"""["'](LNB_\w+)["']\s*:""", txt))         # a dict literal handed to env= / environ.update


def test_every_knob_a_test_or_tool_sets_is_one_something_reads():
    known = table_names() | PYTHON_SIDE
    n_files = n_names = 0
    for sub in ("tests", "tools"):
        for path in sorted(glob.glob(os.path.join(ROOT, sub, "**", "*"), recursive=True)):
            if not path.endswith((".py", ".sh")) or os.path.abspath(path) == os.path.abspath(__file__):
                continue
            rel = os.path.relpath(path, ROOT).replace(os.sep, "/")
            names = names_set_by(path)
            stale = KNOWN_STALE.get(rel, set())
            assert stale <= names, "%s no longer sets %s: take it out of KNOWN_STALE" % (rel, sorted(stale - names))
            unknown = {n for n in names - stale if n not in known and not n.startswith(PYTHON_SIDE_PREFIXES)}
            assert not unknown, "%s sets %s: neither in csrc/lnb_knobs.h nor a Python-side name" % (rel, sorted(unknown))
            n_files += bool(names); n_names += len(names)
    assert n_files >= 10 and n_names >= 40          # the scan found the files it is about
