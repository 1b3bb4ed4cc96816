"""Prefix sharing (lnb_ctx_fork, lnb_ctx_save_prefix / lnb_ctx_load_prefix) without a device: the exports, the header's signatures, every binding
layer and the documents, the LNB_FORK_COPY knob, the argument checks that come before any handle is touched, and the index arithmetic of
csrc/lnb_kvcopy.h on the host under AddressSanitizer and UBSan (tests/native/kvcopy_test.cpp: a stand-alone program, no LD_PRELOAD).

About the offsets-only case of kvcopy_test.cpp: 64 KV heads of head_dim 128 at 131072 positions make K exactly 2^31 bytes, so the last vector of
that geometry starts at 2^31 - 16, not above 2^31.  The program checks that value against independent 64-bit arithmetic, and checks 128 and 256
heads as well, whose last vectors (2^32 - 16, 2^33 - 16) are above 2^31 and above 2^32."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")
NAMES = ("lnb_ctx_fork", "lnb_ctx_prefix_bytes", "lnb_ctx_save_prefix", "lnb_ctx_load_prefix")


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    return _lnb


def test_library_header_and_binding_agree(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    assert int(re.search(r"#define\s+LNB_ABI_VERSION\s+(\d+)", hdr).group(1)) == lnb.ABI_VERSION == 6
    assert int(re.search(r"#define\s+LNB_MAX_FORK\s+(\d+)", hdr).group(1)) == lnb.MAX_FORK == 128
    for sig in ("int lnb_ctx_fork(lnb_ctx* src, int n_pos, lnb_ctx* const* dsts, int n_dst);",
                "int64_t lnb_ctx_prefix_bytes(const lnb_ctx* c, int n_pos);",
                "int lnb_ctx_save_prefix(lnb_ctx* c, int n_pos, void* host, int64_t cap);",
                "int lnb_ctx_load_prefix(lnb_ctx* c, const void* host, int64_t nbytes, int* n_pos_out);"):
        assert hdr.count("\n" + sig + "\n") == 1, sig
    assert "no model identity" in hdr.lower()
    L = C.CDLL(os.path.join(PKG, "liblnb_hip.so"))
    assert L.lnb_abi_version() == 6
    for n in NAMES:
        assert hasattr(L, n) and n in lnb.EXPORTS, n
    B = lnb.lib()
    assert B.lnb_ctx_fork.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int]
    assert B.lnb_ctx_prefix_bytes.argtypes == [C.c_void_p, C.c_int] and B.lnb_ctx_prefix_bytes.restype is C.c_int64
    assert B.lnb_ctx_save_prefix.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    assert B.lnb_ctx_load_prefix.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int)]
    for m in ("ForkPrefix", "SavePrefix", "LoadPrefix"):
        assert callable(getattr(lnb.InferenceContext, m))


def test_every_binding_layer_and_the_documents_name_them():
    files = {"host/lnb_host.hpp": os.path.join(PKG, "host", "lnb_host.hpp"), "go": os.path.join(PKG, "go", "inferencecontext_hip.go"),
             "lnb.py": os.path.join(PKG, "lnb.py"), "INTEGRATION.md": os.path.join(ROOT, "INTEGRATION.md")}
    for tag, path in files.items():
        txt = open(path).read()
        for n in NAMES:
            assert n in txt, (tag, n)
        if not path.endswith(".md"):
            for m in ("ForkPrefix", "SavePrefix", "LoadPrefix"):
                assert m in txt, (tag, m)
    integ = open(files["INTEGRATION.md"]).read()
    assert "bytes per position" in integ.lower() and "kv_dim" in integ
    assert "lnb_ctx_fork" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "lnb_ctx_fork" in open(os.path.join(ROOT, "README.md")).read()
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^HDRS\s*=.*\blnb_kvcopy\.h\b", mk, re.M)
    assert '#include "lnb_kvcopy.h"' in open(os.path.join(PKG, "csrc", "lnb_kernels.hip")).read()


def test_fork_copy_knob_in_the_table_and_the_document_with_one_default():
    hdr = open(os.path.join(PKG, "csrc", "lnb_knobs.h")).read()
    m = re.search(r"^\s*X\(FORK_COPY,\s*([^,]+),\s*(ONCE|LIVE),", hdr, re.M)
    assert m and m.group(2) == "LIVE"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read().split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    row = re.search(r"^\| `LNB_FORK_COPY` \|\s*([^|]+?)\s*\|\s*([^|]+?)\s*\|", doc, re.M)
    assert row, "INTEGRATION.md has no LNB_FORK_COPY row"
    assert row.group(1).strip("` ") == m.group(1).strip() == "0"


def test_argument_checks_come_before_any_handle(lnb):
    L = lnb.lib()
    err = lambda: L.lnb_last_error().decode()
    bogus = C.c_void_p(0x10)                                  # never dereferenced: every check below fails on the arguments alone
    arr = (C.c_void_p * 2)(0x20, 0x30)
    assert L.lnb_ctx_fork(None, 1, arr, 2) < 0 and "null" in err()
    assert L.lnb_ctx_fork(bogus, 1, None, 2) < 0 and "null" in err()
    for n in (0, -1, lnb.MAX_FORK + 1):
        assert L.lnb_ctx_fork(bogus, 1, arr, n) < 0 and "n_dst" in err(), n
    assert L.lnb_ctx_fork(bogus, -1, arr, 2) < 0 and "n_pos" in err()
    assert L.lnb_ctx_fork(bogus, 1, (C.c_void_p * 2)(0x20, None), 2) < 0 and "destination 1 is NULL" in err()
    assert L.lnb_ctx_fork(bogus, 1, (C.c_void_p * 2)(0x20, 0x10), 2) < 0 and "destination 1 is the source" in err()
    assert L.lnb_ctx_fork(bogus, 1, (C.c_void_p * 3)(0x20, 0x30, 0x20), 3) < 0 and "0 and 2" in err()
    buf = (C.c_uint8 * 64)()
    n = C.c_int(0)
    assert L.lnb_ctx_prefix_bytes(None, 1) < 0 and "null" in err()
    assert L.lnb_ctx_save_prefix(None, 1, buf, 64) < 0 and "null" in err()
    assert L.lnb_ctx_save_prefix(bogus, 1, None, 64) < 0 and "null" in err()
    assert L.lnb_ctx_load_prefix(None, buf, 64, C.byref(n)) < 0 and "null" in err()
    assert L.lnb_ctx_load_prefix(bogus, None, 64, C.byref(n)) < 0 and "null" in err()
    assert L.lnb_ctx_load_prefix(bogus, buf, 63, C.byref(n)) < 0 and "header" in err()
    assert L.lnb_ctx_load_prefix(bogus, buf, 64, C.byref(n)) < 0 and "magic" in err()


def test_index_arithmetic_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "kvcopy_test")
    # (the sanitizer runtimes are linked INTO the program: it needs nothing preloaded and does not care what else the process loads first)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "kvcopy_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "kvcopy_test: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
