"""Long contexts (lnb_ctx_create_long) without a device: the golden file of tests/test_gpu_long_context.py, the header, the binding's constants and
the LDS sizes the library answers from the host."""
import ctypes as C
import json
import os
import re

import pytest

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "long_context_tiny_tokens.json")


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    return _lnb


def test_golden_file_schema_and_prompt():
    g = json.load(open(GOLDEN))
    assert g["prompt_len"] == 23540 and g["weights_seed"] == 777 and g["prompt_seed"] == 4000
    assert g["model"] == dict(dim=256, n_layers=1, n_heads=2, n_kv_heads=1, vocab_size=1024, multiple_of=64, max_seq_len=12288)
    V = g["model"]["vocab_size"]
    toks = [g["first_token"]] + g["tokens"]
    assert len(g["tokens"]) == 24 and all(isinstance(t, int) and 0 <= t < V for t in toks)
    assert len(set(toks)) > 12                                # a varied continuation, not a repeated id
    assert len(g["steps"]) == 4
    for k, s in enumerate(g["steps"]):
        assert s["position"] == g["prompt_len"] + k and s["input_token"] == toks[k] and s["argmax"] == toks[k + 1]
        assert re.fullmatch(r"[0-9a-f]{64}", s["logits_sha256"])
    assert re.fullmatch(r"[0-9a-f]{64}", g["k_rows_sha256"]) and re.fullmatch(r"[0-9a-f]{64}", g["v_rows_sha256"])
    # the run crosses lnb_ctx_create's capacity, which is also a 512-position batch edge of the PV kernel
    assert g["prompt_len"] < 23552 < g["prompt_len"] + 24 and 23552 % 512 == 0
    # the prompt is not stored: it is re-derived from its seed
    prompt = orc.synth_tokens(g["prompt_seed"], g["prompt_len"], V)
    assert [int(t) for t in prompt[:8]] == g["prompt_head"] and [int(t) for t in prompt[-8:]] == g["prompt_tail"]
    assert len(set(int(t) for t in prompt[:512])) > 100


def test_header_binding_and_exports_agree(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    assert int(re.search(r"#define\s+LNB_MAX_SEQ_LEN\s+(\d+)", hdr).group(1)) == lnb.MAX_SEQ_LEN == 131072
    assert re.search(r"int\s+lnb_ctx_create_long\(lnb_model\*\s*m,\s*int\s+seq_len,\s*int\s+max_rows,\s*lnb_ctx\*\*\s*out\);", hdr)
    assert re.search(r"int\s+lnb_ctx_max_rows\(const\s+lnb_ctx\*\s*c,\s*int\*\s*out\);", hdr)
    assert "lnb_ctx_create_long" in lnb.EXPORTS and "lnb_ctx_max_rows" in lnb.EXPORTS
    L = C.CDLL(os.path.join(ROOT, "llama-nuts-and-bolts_amd", "liblnb_hip.so"))
    assert hasattr(L, "lnb_ctx_create_long") and hasattr(L, "lnb_ctx_max_rows")
    # without a device: the argument checks that come before anything touches one
    out, n = C.c_void_p(), C.c_int(0)
    L.lnb_last_error.restype = C.c_char_p
    assert L.lnb_ctx_create_long(None, 16, 0, C.byref(out)) != 0 and b"null" in L.lnb_last_error()
    assert L.lnb_ctx_max_rows(None, C.byref(n)) != 0 and b"null" in L.lnb_last_error()


def test_pv_lds_is_constant_beyond_the_per_position_layout(lnb):
    """lnbk_attn_long_lds: the per-position layout's size (what lnb_ctx_create checks against 160 KB); lnbk_attn_long_layout_lds: what the PV launch of
    a context requests -- the same up to 23552 positions, 3 batches of 512 floats + the product ring + 64 bytes beyond"""
    L = C.CDLL(os.path.join(ROOT, "llama-nuts-and-bolts_amd", "liblnb_hip.so"))
    for f in (L.lnbk_attn_long_lds, L.lnbk_attn_long_layout_lds):
        f.restype, f.argtypes = C.c_size_t, [C.c_int]
    per_position = lambda s: ((s + 511) // 512 + 1) * 2048 + 65536 + 64
    for s in (1, 32, 512, 513, 4096, 8400, 22000, 23551, 23552):
        assert L.lnbk_attn_long_lds(s) == L.lnbk_attn_long_layout_lds(s) == per_position(s) <= 160 * 1024, s
    const = 3 * 512 * 4 + 65536 + 64
    for s in (23553, 23600, 24000, 32768, 65536, 131071, 131072):
        assert L.lnbk_attn_long_lds(s) == per_position(s) > 160 * 1024, s
        assert L.lnbk_attn_long_layout_lds(s) == const, s
    assert 2 * const <= 160 * 1024                            # two such workgroups fit a CU's LDS
