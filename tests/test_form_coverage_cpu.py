"""The ledger that keeps the gap closed (CPU): every kernel form of csrc/lnb_forms.h is named by a `ran(...)` of some GPU test -- so that test fails unless the form
really ran -- or stands in FORM_EXEMPT with a reason; every knob of csrc/lnb_knobs.h is set by a GPU test or stands in KNOB_EXEMPT with a reason.  A new arm in a
launch function means a new row in the form table, and this test then asks for its GPU test.

What counts as "named by a ran(...)": a form name written out in full
  * as a string in the arguments of a ran(...) call (not under not_ran=), or
  * in a module-level table whose name ends in _FORMS AND is written inside the arguments of a ran(...) call of the same source (not under not_ran=) -- the
    convention of the GPU tests for what they hand to ran(): such a table lists forms that some case of its file REQUIRES to have run, never forms that must not;
in tests/test_gpu_*.py or in the source of a child process kept there as a string (a ONCE knob needs a fresh process).  A prefix ("gemm_stream") covers nothing.

What counts as "set by a GPU test" for a knob: a real setting in those sources -- setenv("K", ...), environ["K"] = ..., environ.setdefault("K", ...), K=... in a dict(os.environ, ...), "K": in a dict handed to a child's
environment or walked with setenv -- never a mention in a comment or a docstring."""
import ast
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llama-nuts-and-bolts_amd", "csrc")

FORM_EXEMPT = {}
KNOB_EXEMPT = {
    # measurement only: they change what is timed or printed, never a result
    "LNB_GEMV_TIMING": "timing only, produces no result", "LNB_PROFILE_SAME_LAYER": "timing only, produces no result",
    "LNB_MEASURE_SKIP_TOKEN_KERNELS": "timing only: the tokens are garbage by design", "LNB_W2_PRIO": "a wave priority: timing only, produces no result",
    "LNB_W2_LDS_PAD": "LDS padding of the profiled pair: timing only, produces no result", "LNB_ATTN_GQA_DBG": "prints phase stamps, produces no result",
    # covered elsewhere, or an aid that picks nothing of its own
    "LNB_PIPELINE_LOG_CAP": "set by the wrap-around test of tests/test_pipeline_cabi.py (GPU-marked, outside the test_gpu_* files): a log size, no kernel form",
    "LNB_ATTN_LONG_T": "only the initial value of a per-context threshold: the tests set that threshold itself, through lnb_ctx_set_attention / lnb_batch_set_attention "
                       "(tests/test_gpu_long_context.py, test_gpu_batch_long.py, test_gpu_attention_crafted.py force the long kernels at every length and leave them off)",
    "LNB_GS_NTW_CHAIN": "experiment aid: LNB_GS_NTW restricted to the chain layouts; tests/test_gpu_forms.py forces every tile count on every source through LNB_GS_NTW",
}


def test_form_table_on_the_host(tmp_path):
    """tests/native/forms_test.cpp, stand-alone: unique names, none a path prefix of another, lookup, per-epilogue counters, reset, no lost count under threads"""
    exe = str(tmp_path / "forms_test")
    src = os.path.join(ROOT, "tests", "native", "forms_test.cpp")
    # under the address and undefined-behaviour sanitizers, and -- the program counts from eight threads -- once more under the thread sanitizer
    for flags in (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], ["-fsanitize=thread"]):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"] + flags + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "forms_test: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(re.search(r"\((\d+) forms\)", r.stdout).group(1)) == len(form_names())


def form_names():
    hdr = open(os.path.join(CSRC, "lnb_forms.h")).read()
    names = re.findall(r'^\s*X\(\w+,\s*"([a-z0-9_.]+)",\s*"', hdr, re.M)
    assert len(names) >= 30 and len(names) == len(set(names))
    return names


def knob_names():
    hdr = open(os.path.join(CSRC, "lnb_knobs.h")).read()
    names = re.findall(r"^\s*X\((\w+),\s*[^,]+,\s*(?:ONCE|LIVE),\s*\"", hdr, re.M)
    assert len(names) >= 40
    return ["LNB_" + n for n in names]


def _strings(node):
    return {n.value for n in ast.walk(node) if isinstance(n, ast.Constant) and isinstance(n.value, str)}


def named_in(source, found, depth=0):
    """form names a piece of test source hands to ran(); child-process sources (strings that call ran themselves) are read the same way"""
    tree = ast.parse(source)
    tables, handed = {}, set()                                # _FORMS tables of this source; names written inside a ran(...)'s arguments
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and (getattr(node.func, "id", None) == "ran" or getattr(node.func, "attr", None) == "ran"):
            for arg in node.args[1:] + [kw.value for kw in node.keywords if kw.arg == "form"]:
                found |= _strings(arg)
                handed |= {n.id for n in ast.walk(arg) if isinstance(n, ast.Name)}
        if isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Name) and t.id.endswith("_FORMS"):
                    tables[t.id] = _strings(node.value)
    forms = set(form_names())
    unused = sorted(t for t in set(tables) - handed if tables[t] & forms)      # (a *_FORMS table about something else -- attention variants by name -- is not meant)
    assert not unused, "tables named *_FORMS that no ran(...) of their source is handed: %s" % unused
    for t in handed & set(tables):
        found |= tables[t]
    if depth == 0:
        for s in _strings(tree):
            if "ran(" in s and "\n" in s:
                named_in(re.sub(r"%\(\w+\)[rsd]", "None", s).replace("%%", "%"), found, 1)
    return found


def gpu_test_sources():
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))
    assert len(paths) >= 15
    return {os.path.basename(p): open(p).read() for p in paths}


def test_every_kernel_form_is_named_by_a_gpu_test_that_asserts_it_ran():
    forms = form_names()
    found = set()
    for name, src in gpu_test_sources().items():
        named_in(src, found)
    unknown = {f for f in found if re.fullmatch(r"[a-z0-9_]+(\.[a-z0-9_]+)+", f) and f.split(".")[0] in {n.split(".")[0] for n in forms} and f not in forms
               and not any(n.startswith(f + ".") for n in forms)}
    assert not unknown, "ran(...) names forms that csrc/lnb_forms.h does not have: %s" % sorted(unknown)
    stale = sorted(set(FORM_EXEMPT) - set(forms))
    assert not stale, "FORM_EXEMPT lists forms the table no longer has: %s" % stale
    both = sorted(f for f in FORM_EXEMPT if f in found)
    assert not both, "exempt AND named by a ran(...): take them out of FORM_EXEMPT: %s" % both
    missing = [f for f in forms if f not in found and f not in FORM_EXEMPT]
    assert not missing, "kernel forms no GPU test asserts to have run (add a ran(...) to a test that runs them, or an exemption with its reason): %s" % missing
    assert all(len(r) > 20 for r in FORM_EXEMPT.values())


def test_every_knob_is_set_by_a_gpu_test_or_exempt_with_a_reason():
    knobs = knob_names()
    text = "\n".join(gpu_test_sources().values())
    used = {k for k in knobs if re.search(r"""(?:setenv|environ\.setdefault)\(\s*["']%s["']|environ\[\s*["']%s["']\s*\]\s*=[^=]|["']%s["']\s*:|\b%s\s*=\s*["'\w]""" % (k, k, k, k), text)}
    stale = sorted(set(KNOB_EXEMPT) - set(knobs))
    assert not stale, "KNOB_EXEMPT lists knobs the table no longer has: %s" % stale
    both = sorted(k for k in KNOB_EXEMPT if k in used)
    assert not both, "exempt AND set by a GPU test: take them out of KNOB_EXEMPT: %s" % both
    missing = [k for k in knobs if k not in used and k not in KNOB_EXEMPT]
    assert not missing, "knobs no GPU test sets (set them in a test that asserts the form they pick, or exempt them with a reason): %s" % missing
    assert all(len(r) > 20 for r in KNOB_EXEMPT.values())


PRODUCT_FAMILIES = ("gemm_mfma", "gemm_stream", "gemm_stream_order", "gemm_blgp", "mfma_pair", "mfma_stream", "rowcast", "rowcast_lds", "gemv_quad", "gemv_chain",
                    "gemv_chain_pk", "gemv_head_pk")


def test_every_product_form_runs_on_the_order_revealing_rows_or_is_exempt_there():
    """every form that evaluates a dot product is named by a ran(...) of tests/test_gpu_order_crafted.py -- the rows on which a wrong order of the adds changes a
    bf16 output -- or stands in that file's docstring under "Exempt, one line each:" as `  name: reason`"""
    forms = form_names()
    product = [f for f in forms if f.split(".")[0] in PRODUCT_FAMILIES]
    assert len(product) >= 30 and {f.split(".")[0] for f in product} == set(PRODUCT_FAMILIES)
    src = gpu_test_sources()["test_gpu_order_crafted.py"]
    found = named_in(src, set())
    doc = ast.get_docstring(ast.parse(src))
    assert "Exempt, one line each:" in doc
    exempt = dict(re.findall(r"^\s*([a-z0-9_.]+): (.+)$", doc.split("Exempt, one line each:")[1], re.M))
    stale = sorted(set(exempt) - set(forms))
    assert not stale, "exempt forms the table does not have: %s" % stale
    both = sorted(f for f in exempt if f in found)
    assert not both, "exempt AND named by a ran(...): %s" % both
    missing = [f for f in product if f not in found and f not in exempt]
    assert not missing, "product forms that never meet the order-revealing rows: %s" % missing
    assert all(len(r) > 20 for r in exempt.values())
