"""CPU-side checks of the multi-row long-context attention (lnb_ctx_set_rows_attention): the exports, the PV kernel's LDS (which must not depend on
the context length), the LNB_ATTN_ROWS_RPW knob, and every binding layer naming the two entry points."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")
ENTRY = ("lnb_ctx_set_rows_attention", "lnb_ctx_append_attention_form")


@pytest.fixture(scope="module")
def so():
    import lnb as _lnb
    _lnb.build()
    return C.CDLL(os.path.join(PKG, "liblnb_hip.so"))


def test_library_exports_the_entry_points(so):
    import lnb
    for n in ENTRY:
        assert hasattr(so, n), n
        assert n in lnb.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    assert re.search(r"int lnb_ctx_set_rows_attention\(lnb_ctx\* c, int long_threshold, int flags\);", hdr)
    assert re.search(r"int lnb_ctx_append_attention_form\(const lnb_ctx\* c, int\* out\);", hdr)
    assert int(re.search(r"#define\s+LNB_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6          # additions only


def test_pv_kernel_lds_fits_a_cu_and_takes_no_context_length(so):
    f = so.lnbk_attn_rows_lds
    f.restype = C.c_size_t
    f.argtypes = [C.c_int, C.c_int]                           # (head_dim, rows per workgroup): no seq_len
    for hd in (32, 64, 128):
        for rpw in (1, 2, 4):
            n = f(hd, rpw)
            assert 0 < n <= 160 * 1024, (hd, rpw, n)
    src = open(os.path.join(PKG, "csrc", "lnb_kernels.hip")).read()
    assert re.search(r'extern "C" size_t lnbk_attn_rows_lds\(int hd, int rpw\)', src)
    # the existing long pair's layout for the longest context, for comparison: the rows kernel must be launchable there for every RPW
    g = so.lnbk_attn_long_layout_lds
    g.restype = C.c_size_t
    g.argtypes = [C.c_int]
    assert g(131072) <= 160 * 1024


def test_knob_is_in_the_table_and_in_the_document():
    hdr = open(os.path.join(PKG, "csrc", "lnb_knobs.h")).read()
    m = re.search(r"^\s*X\(ATTN_ROWS_RPW,\s*(\d+),\s*ONCE,", hdr, re.M)
    assert m and int(m.group(1)) in (1, 2, 4)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc.split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    row = re.search(r"^\| `LNB_ATTN_ROWS_RPW` \| (\d+) \| ONCE \|", sec, re.M)
    assert row and row.group(1) == m.group(1)


def test_every_layer_names_both_entry_points():
    for rel in ("include/lnb.h", "llama-nuts-and-bolts_amd/lnb.py", "llama-nuts-and-bolts_amd/host/lnb_host.hpp",
                "llama-nuts-and-bolts_amd/go/inferencecontext_hip.go", "INTEGRATION.md"):
        txt = open(os.path.join(ROOT, rel)).read()
        for n in ENTRY:
            assert n in txt, (rel, n)
    import lnb
    assert inspect.signature(lnb.InferenceContext.set_rows_attention).parameters.keys() >= {"long_threshold", "flags"}
    assert callable(lnb.InferenceContext.append_attention_form)
