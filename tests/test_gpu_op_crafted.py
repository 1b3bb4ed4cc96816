"""The RoPE, SiLU * up and residual epilogues on crafted values, through single-part stages (-m gpu).  lnb_model_create_parts builds a stage that holds one third
of a block; lnb_ctx_hidden_ptr exposes its input (0), its output (1) and the [S, ffn_hidden] activations (2), so tests/op_craft.py's bf16 patterns are written in
front of a part and its output (or the K and V rows it appended) is read back and compared with the composition of the oracle's operators: all 16 bits, NaN-ness
where the reference is NaN.  What the values are, and that a wrong epilogue would change them, is tests/test_op_crafted_cpu.py's business.  Every comparison sits
inside a `ran` block (tests/form_tally.py): the launch tally proves which kernel computed the bits.

  down part       w2 + residual: act in ptr 2, h in ptr 0 (= ptr 1: a part stage adds in place), 1 / 2 / 7 / 15 / 16 / 17 / 83 rows and the full 256 x 256 grid
  gate/up part    ffn_norm, w1|w3, SiLU * up: h in ptr 0, the activations in ptr 2; h must come through unchanged
  attention part  attention_norm, wq|wk|wv + RoPE + KV append: the K and V rows of the call and every row around them (lnb_ctx_read_kv); at position 0 with one row
                  the attention output IS the V row (p = 1.0), so a wo of selector rows puts a crafted y against h in wo's residual epilogue
Q rows are not observable from a stage: they go through the same instructions as the K rows (one branch on the output row picks q_out or the cache) -- no entry
point is invented for them.

(form, epilogue) pairs asserted here: gemv_chain.rw16 x (qkv_rope, resid, silu_mul), gemv_chain.rw32 / rw64 x resid, gemv_chain.rw56 / rw56_tp / rw28 / gemv_chain_pk
x silu_mul, gemv_quad x (qkv_rope, resid), rowcast / rowcast_lds x resid, gemm_mfma.t16 / t64 / t128 x (qkv_rope, resid, silu_mul), gemm_blgp x (qkv_rope, silu_mul),
gemm_stream.chain x (qkv_rope, silu_mul), gemm_stream.rowcast.ntw1 / 2 / 4 / 4_tt x resid, gemm_stream.copy x qkv_rope, mfma_pair x (qkv_rope, resid),
mfma_stream.c1 x (qkv_rope, resid), mfma_stream.c2 x silu_mul.
Exempt, one line each:
  gemm_stream.copy x (resid, silu_mul): the copy exists on whole-block models only (lnb_model_enable_batch refuses a stage cut inside a block); same gemm_epilogue4 as the resident sources.
  gemm_stream.copy.ntw4_tt x resid: the copy again (whole-block models only); the row-broadcast source's two-weight-tile form is asserted here.
  gemv_chain.rw56 under the throughput schedule with LNB_TP_W13=0 (ONCE): the instantiation the latency schedule runs here.
  multi-row wo on crafted y: its forms (gemm_stream.rowcast, gemm_mfma.t16) are the down part's, asserted there; here it runs behind the attention on what the crafted rows give.
  attention output h' of calls of 16 rows and more: the matrix-core attention multiplies subnormal K and V elements fused (the documented limit); compared for 1 .. 15 rows."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import op_craft as oc
from form_tally import count, ran
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")
SCHEDULES = ("latency", "throughput")


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


_HIP = []


def hip():
    if not _HIP:
        h = C.CDLL("libamdhip64.so")
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.append(h)
    return _HIP[0]


def poke(lnb, ctx, which, a):
    a = np.ascontiguousarray(a, dtype=np.uint16)
    assert hip().hipMemcpy(lnb.lib().lnb_ctx_hidden_ptr(ctx.h, which), a.ctypes.data, a.nbytes, 1) == 0 and hip().hipDeviceSynchronize() == 0


def peek(lnb, ctx, which, shape):
    out = np.empty(shape, dtype=np.uint16)
    assert hip().hipDeviceSynchronize() == 0 and hip().hipMemcpy(out.ctypes.data, lnb.lib().lnb_ctx_hidden_ptr(ctx.h, which), out.nbytes, 2) == 0
    return out


def call(lnb, ctx, rows, pos=0):
    try:
        lnb._chk(lnb.lib().lnb_forward_stage(ctx.h, None, rows, pos, None, None))
    except lnb.LnbError as e:                                # a device fault ends the session: nothing more is started on that GPU
        if "illegal memory access" in str(e) or "launch failure" in str(e):
            pytest.exit("the device faulted: %s" % e, returncode=3)
        raise


def part_model(lnb, geo, part, tensors):
    """the stage that holds part `part` (0 attention, 1 gate/up, 2 down) of block LAYER, the given tensors ({suffix: array}) in place of the synthetic ones"""
    pb = 3 * oc.LAYER + part
    cfg = dict(oc.GEOS[geo], max_seq_len=128) if part else oc.GEOS[geo]      # (a call's rows are checked against the cis table even where no RoPE runs: 256 rows for the grid)
    gm = lnb.LlamaTransformer(device=0, part_begin=pb, part_end=pb + 1, **cfg).fill_synthetic(3)
    for suffix, a in tensors.items():
        gm.set_tensor("layers.%d.%s.weight" % (oc.LAYER, suffix), a)
    return gm.finalize()


def check(got, ref, tag):
    ok = oc.same_or_both_nan(got, ref)
    bad = np.argwhere(~ok)
    assert bad.size == 0, "%s: %d of %d differ; first (row, col): %s got %s oracle %s" % (
        tag, len(bad), ok.size, bad[:6].tolist(), [hex(int(got[tuple(i)])) for i in bad[:6]], [hex(int(ref[tuple(i)])) for i in bad[:6]])


_REF = {}


def ref_of(kind, key):
    """the oracle's side of a case set, computed once per process and left unchanged"""
    if (kind, key) not in _REF:
        if kind == "down":
            c = oc.down_case(*key); r = oc.down_ref(c)
        elif kind == "gate_up":
            c = oc.gate_up_case(*key); r = oc.gate_up_ref(c)
        else:
            c = oc.attn_case(*key); r = oc.kv_ref(c)
            if key[4] == "finite" and key[3] < 16:
                r["h_out"] = oc.attn_oracle(c)[0][("h", 0)]
        _REF[(kind, key)] = (c, r)
    return _REF[(kind, key)]


# ---- down part ---------------------------------------------------------------------------------------------------------------------------------------------------
def down_form(geo, rows, sched):
    """what the default dispatch picks for w2 (lnb_api.cpp: auto_rw, gemm_dispatch; lnb_kernels.hip: launch_rowcast)"""
    if rows >= 16:
        return "gemm_mfma.t16" if geo == "odd192" else "gemm_stream.rowcast"
    return {"tiny": "rowcast", "odd192": "gemv_chain.rw16", "wide1024": "rowcast_lds" if sched == "latency" else "rowcast"}[geo]


def run_down(lnb, gm, key, sched="latency"):
    c, r = ref_of("down", key)
    rows = key[1]
    ctx = lnb.InferenceContext(gm, max(rows, 16)).set_schedule(sched)
    poke(lnb, ctx, 0, c["h"]); poke(lnb, ctx, 2, c["act"])
    call(lnb, ctx, rows)
    out = peek(lnb, ctx, 1, c["h"].shape)
    ctx.close()
    check(out, r["out"], ("down",) + key + (sched,))


_GM = {}                                      # the part stages shared by several tests, made on first use with no knob of this file set (guarded below), closed by `models`
CREATE_KNOBS = ("LNB_RW_W2", "LNB_RW_W13", "LNB_RW_QKV", "LNB_RW_WO", "LNB_W13_PACKED")


def shared_model(key, make):
    if key not in _GM:
        assert not [k for k in CREATE_KNOBS if k in os.environ], "a shared model must be made under the default layouts"
        _GM[key] = make()
    return _GM[key]


@pytest.fixture(scope="module", autouse=True)
def models():
    yield
    for gm in _GM.values():
        gm.close()
    _GM.clear()


def down_model(lnb, geo, grid=False):
    return shared_model(("down", geo, grid), lambda: part_model(lnb, geo, 2, {"feed_forward.w2": oc.down_case(geo, 256 if grid else 1)["w2"]}))


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("geo,rows", oc.RESID_SETS)
def test_residual_epilogue_of_the_down_part_on_the_default_dispatch(lnb, geo, rows, sched):
    gm = down_model(lnb, geo, rows == 256)
    with ran(lnb, down_form(geo, rows, sched), epi="resid"):
        run_down(lnb, gm, (geo, rows), sched)


W2_KNOB_FORMS = {("tiny", "16", "0"): "gemv_chain.rw16", ("tiny", "32", "0"): "gemv_chain.rw32", ("tiny", "64", "0"): "gemv_chain.rw64", ("tiny", "16", "1"): "gemv_quad",
                 ("wide1024", "16", "1"): "gemv_quad", ("wide1024", "16", "2"): "gemv_quad"}


@pytest.mark.parametrize("geo,rw,quad", sorted(W2_KNOB_FORMS))
def test_residual_epilogue_on_the_chain_layouts_and_the_quad_kernel(lnb, monkeypatch, geo, rw, quad):
    """LNB_RW_W2 (LIVE, read when the model is created) puts w2 on 16 / 32 / 64-row chain blocks; LNB_W2_QUAD (LIVE) runs the 16-row layout on gemv_quad_kernel with
    128-step (1) or 256-step (2) stages -- the latter wants K a multiple of 256: wide1024's 3584, not tiny's 896"""
    monkeypatch.setenv("LNB_RW_W2", rw); monkeypatch.setenv("LNB_W2_QUAD", quad)
    gm = part_model(lnb, geo, 2, {"feed_forward.w2": oc.down_case(geo, 1)["w2"]})
    for rows in (1, 7, 15) if geo == "tiny" else (1, 7):
        with ran(lnb, W2_KNOB_FORMS[(geo, rw, quad)], epi="resid", not_ran=("rowcast", "rowcast_lds")):
            run_down(lnb, gm, (geo, rows))
    gm.close()


NTW_FORMS = {("1", "0"): "gemm_stream.rowcast.ntw1", ("2", "0"): "gemm_stream.rowcast.ntw2", ("4", "0"): "gemm_stream.rowcast.ntw4", ("4", "1"): "gemm_stream.rowcast.ntw4_tt"}


@pytest.mark.parametrize("ntw,tt", sorted(NTW_FORMS))
def test_residual_epilogue_of_the_streaming_product_with_one_two_and_four_batch_tiles_per_wave(lnb, monkeypatch, ntw, tt):
    """LNB_GS_NTW and LNB_GS_TT (LIVE): one, two and four batch tiles per wave, and four with two weight tiles per wave -- an instantiation with an epilogue call
    and tile arithmetic of its own -- at 17 and 83 rows and on the full grid, from the resident row-broadcast layout"""
    monkeypatch.setenv("LNB_GS_NTW", ntw); monkeypatch.setenv("LNB_GS_TT", tt)
    others = tuple(f for f in NTW_FORMS.values() if f != NTW_FORMS[(ntw, tt)])
    for rows in (17, 83, 256):
        with ran(lnb, NTW_FORMS[(ntw, tt)], epi="resid", not_ran=others + ("gemm_mfma",)):
            run_down(lnb, down_model(lnb, "tiny", rows == 256), ("tiny", rows))


# ---- gate/up part ------------------------------------------------------------------------------------------------------------------------------------------------
def gate_up_form(geo, rows):
    if rows >= 16:
        return "gemm_mfma.t16" if geo == "odd192" else "gemm_stream.chain"
    return "gemv_chain.rw16"


def run_gate_up(lnb, gm, key, sched="latency"):
    c, r = ref_of("gate_up", key)
    rows, F = key[1], gm.ffn_hidden
    ctx = lnb.InferenceContext(gm, max(rows, 16)).set_schedule(sched)
    poke(lnb, ctx, 0, c["h"]); poke(lnb, ctx, 2, np.full((rows, F), oc.QNAN, dtype=np.uint16))
    call(lnb, ctx, rows)
    out, h = peek(lnb, ctx, 2, (rows, F)), peek(lnb, ctx, 1, c["h"].shape)
    ctx.close()
    check(out, r["out"], ("gate_up",) + key + (sched,))
    assert (h == c["h"]).all(), ("h must come through the gate/up part unchanged",) + key


def gate_up_model(lnb, geo, variant):
    def make():
        c = oc.gate_up_case(geo, 1, variant)
        return part_model(lnb, geo, 1, {"ffn_norm": c["nw"], "feed_forward.w1": c["w1"], "feed_forward.w3": c["w3"]})
    return shared_model(("gate_up", geo, variant), make)


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("geo,rows,variant", oc.GATE_UP_SETS)
def test_silu_mul_epilogue_of_the_gate_up_part_on_the_default_dispatch(lnb, geo, rows, variant, sched):
    gm = gate_up_model(lnb, geo, variant)
    with ran(lnb, gate_up_form(geo, rows), epi="silu_mul", not_ran=("gemv_chain_pk",)):
        run_gate_up(lnb, gm, (geo, rows, variant), sched)


RW56_FORMS = {("latency", True): "gemv_chain_pk", ("latency", False): "gemv_chain.rw56", ("throughput", True): "gemv_chain.rw56_tp", ("throughput", False): "gemv_chain.rw56_tp"}
WPACK_STATUS = ("packed", "subnormal", "infnan", "window")


@pytest.mark.parametrize("packed", ["1", "0"])
@pytest.mark.parametrize("variant", ["exact", "split", "window"])
def test_silu_mul_epilogue_on_the_56_row_blocks_raw_and_from_the_13_bit_copy(lnb, monkeypatch, variant, packed):
    """LNB_RW_W13=56 (LIVE, read when the model is created; FFN hidden 896 = 16 blocks) with LNB_W13_PACKED 1 and 0: the window set packs and its one-token step runs
    gemv_chain_pk_kernel; the crafted sets with subnormal weights are refused, SAY SO, and keep the raw kernel; several rows and the throughput schedule never
    read the copy"""
    monkeypatch.setenv("LNB_RW_W13", "56"); monkeypatch.setenv("LNB_W13_PACKED", packed)
    c = oc.gate_up_case("tiny", 1, variant)
    gm = part_model(lnb, "tiny", 1, {"ffn_norm": c["nw"], "feed_forward.w1": c["w1"], "feed_forward.w3": c["w3"]})
    info = gm.wpack_info()
    want = oc.wpack_expect(c["w1"], c["w3"])
    if packed == "1":
        assert info[WPACK_STATUS[want]] == 1 and sum(info.values()) == 1, (variant, info)
    else:
        assert info["not_tried"] == 1 and info["packed"] == 0, info
    is_packed = packed == "1" and want == 0
    for sched in SCHEDULES:
        with ran(lnb, RW56_FORMS[(sched, is_packed)], epi="silu_mul", not_ran=() if is_packed and sched == "latency" else ("gemv_chain_pk",)):
            run_gate_up(lnb, gm, ("tiny", 1, variant), sched)
    rows = 7 if variant != "split" else 1
    if rows > 1:
        with ran(lnb, "gemv_chain.rw56", epi="silu_mul", not_ran=("gemv_chain_pk",)):
            run_gate_up(lnb, gm, ("tiny", rows, variant))
    gm.close()


def test_silu_mul_epilogue_on_the_half_height_blocks(lnb, monkeypatch):
    """LNB_RW_W13=28: gemv_chain_kernel<28, 2, ...>, 32 blocks in the band order"""
    monkeypatch.setenv("LNB_RW_W13", "28")
    c = oc.gate_up_case("tiny", 1, "exact")
    gm = part_model(lnb, "tiny", 1, {"ffn_norm": c["nw"], "feed_forward.w1": c["w1"], "feed_forward.w3": c["w3"]})
    for rows in (1, 7, 15):
        with ran(lnb, "gemv_chain.rw28", epi="silu_mul", not_ran=("gemv_chain.rw56", "gemv_chain_pk")):
            run_gate_up(lnb, gm, ("tiny", rows, "exact"))
    gm.close()


# ---- attention part: RoPE and the KV append -------------------------------------------------------------------------------------------------------------------
def attn_forms(geo, rows, sched):
    if rows >= 16:
        return {"gemm_mfma.t16": ("qkv_rope", "resid")} if geo == "odd192" else {"gemm_stream.chain": "qkv_rope", "gemm_stream.rowcast": "resid"}
    wo = {"tiny": "rowcast", "hd32": "rowcast", "odd192": "gemv_chain.rw16", "wide1024": "rowcast_lds" if sched == "latency" else "rowcast"}[geo]
    return {"gemv_chain.rw16": ("qkv_rope", "resid")} if wo == "gemv_chain.rw16" else {"gemv_chain.rw16": "qkv_rope", wo: "resid"}


SENTINEL = 0x4D4D


def kv_blob(c, s, sentinel_from):
    """LNBKV1 blob (include/lnb.h) of the stage's one cached layer over the whole capacity: the case's prefix rows, then SENTINEL from `sentinel_from` on (a FINITE pattern: a NaN would
    raise the context's sticky word and every finite set would run the attention of the non-finite ones)"""
    import struct
    n_pos, kvh, hd = c["capacity"], s["KVH"], s["hd"]
    K = np.full((n_pos, kvh, hd), SENTINEL, dtype=np.uint16); V = K.copy()
    K[:sentinel_from], V[:sentinel_from] = c["prefix_k"], c["prefix_v"]
    pb = 3 * oc.LAYER
    head = b"LNBKV1\0\0" + struct.pack("<7I", 1, n_pos, pb, pb + 1, kvh, hd, 1) + bytes(28)
    body = [np.ascontiguousarray(K.reshape(n_pos, kvh, hd // 8, 8).transpose(1, 2, 0, 3)).view(np.uint8).ravel(), V.view(np.uint8).ravel()]
    return np.concatenate([np.frombuffer(head, dtype=np.uint8)] + body), K, V


def run_attn(lnb, gm, key, sched="latency"):
    """the call of a RoPE set on a context that holds the set's prefix rows and a sentinel pattern everywhere else: the rows written are the reference's, every other
    row is untouched; the finite sets of 1 .. 15 rows also compare the part's output h' with the oracle's forward"""
    c, r = ref_of("attn", key)
    s = oc.shape_of(key[0])
    cap, start, rows = key[1], key[2], key[3]
    ctx = lnb.InferenceContext(gm, cap).set_schedule(sched)
    blob, K0, V0 = kv_blob(c, s, start)
    assert ctx.LoadPrefix(blob) == cap
    poke(lnb, ctx, 0, c["h"])
    call(lnb, ctx, rows, start)
    K, V = ctx.CacheK(oc.LAYER), ctx.CacheV(oc.LAYER)
    out = peek(lnb, ctx, 1, c["h"].shape)
    ctx.close()
    tag = ("attention",) + key + (sched,)
    check(K[start:start + rows].reshape(rows, -1), r["xk_rope"], tag + ("K",)); check(V[start:start + rows].reshape(rows, -1), r["xv"], tag + ("V",))
    for got, was, what in ((K, K0, "K"), (V, V0, "V")):
        assert (got[:start] == was[:start]).all() and (got[start + rows:] == was[start + rows:]).all(), tag + (what, "a row outside the call was written")
    if "h_out" in r:
        check(out, r["h_out"], tag + ("h'",))


def attn_model(lnb, key):
    c, _ = ref_of("attn", key)
    return part_model(lnb, key[0], 0, {"attention_norm": c["nw"], "attention.wq": c["wq"], "attention.wk": c["wk"], "attention.wv": c["wv"], "attention.wo": c["wo"]})


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("key", oc.ROPE_SETS, ids=lambda k: "-".join(str(x) for x in k))
def test_rope_epilogue_and_kv_append_of_the_attention_part_on_the_default_dispatch(lnb, key, sched):
    gm = attn_model(lnb, key)
    with ran(lnb, attn_forms(key[0], key[3], sched)):
        run_attn(lnb, gm, key, sched)
    gm.close()


@pytest.mark.parametrize("key", [k for k in oc.ROPE_SETS if k[0] in ("tiny", "wide1024") and k[3] < 16], ids=lambda k: "-".join(str(x) for x in k))
def test_rope_epilogue_on_the_quad_kernel_whose_partner_sits_four_lanes_away(lnb, monkeypatch, key):
    """LNB_RW_QKV=24 (LIVE, read when the model is created): gemv_quad_kernel, four lanes per row, the RoPE partner fetched from lane ^ 4; 256- and (throughput
    schedule) 128-step stages; a ragged last block (512 and 1536 rows are no multiples of 24)"""
    monkeypatch.setenv("LNB_RW_QKV", "24")
    gm = attn_model(lnb, key)
    for sched in SCHEDULES:
        with ran(lnb, "gemv_quad", epi="qkv_rope", not_ran=("gemv_chain.rw16",) if key[0] == "wide1024" else ()):
            run_attn(lnb, gm, key, sched)
    gm.close()


BLGP_FORMS = {"qkv_rope": "gemm_blgp", "silu_mul": "gemm_blgp"}


def test_rope_and_silu_mul_epilogues_of_the_blgp_product(lnb, monkeypatch):
    """LNB_GEMM_BLGP=2 (LIVE): the chain layouts' prefill products on gemm_blgp_kernel -- wq|wk|wv and gate|up at 16, 17 and 83 rows"""
    monkeypatch.setenv("LNB_GEMM_BLGP", "2")
    for key in (("tiny", 128, 16, 16, "finite"), ("tiny", 128, 17, 17, "finite"), ("tiny", 128, 0, 83, "finite"), ("tiny", 128, 0, 17, "nonfinite")):
        gm = attn_model(lnb, key)
        with ran(lnb, BLGP_FORMS["qkv_rope"], epi="qkv_rope", not_ran=("gemm_stream.chain",)):
            run_attn(lnb, gm, key)
        gm.close()
    for rows in (16, 17, 83):
        with ran(lnb, BLGP_FORMS["silu_mul"], epi="silu_mul", not_ran=("gemm_stream.chain",)):
            run_gate_up(lnb, gate_up_model(lnb, "tiny", "split"), ("tiny", rows, "split"))


# ---- ONCE knobs: a child process each, one after another -------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
import lnb
import op_craft as oc
import test_gpu_op_crafted as t
from form_tally import ran
case = os.environ["LNB_TEST_OP_CRAFTED_CASE"]
TILE_FORMS = {"tile64": "gemm_mfma.t64", "tile128": "gemm_mfma.t128"}
if case in TILE_FORMS:                                           # LNB_GEMM_TILE with LNB_PREFILL_STREAM=0: every product of 16+ rows on the LDS-tiled kernel
    others = tuple(f for f in ("gemm_mfma.t16", "gemm_mfma.t64", "gemm_mfma.t128") if f != TILE_FORMS[case]) + ("gemm_stream", "gemm_blgp")
    for rows in (17, 83, 256):
        with ran(lnb, TILE_FORMS[case], epi="resid", not_ran=others):
            t.run_down(lnb, t.down_model(lnb, "tiny", rows == 256), ("tiny", rows))
    for rows in (17, 83):
        with ran(lnb, TILE_FORMS[case], epi="silu_mul", not_ran=others):
            t.run_gate_up(lnb, t.gate_up_model(lnb, "tiny", "split"), ("tiny", rows, "split"))
    for key in (("tiny", 128, 17, 17, "finite"), ("tiny", 128, 0, 83, "finite"), ("tiny", 128, 0, 17, "nonfinite"), ("wide1024", 128, 16, 16, "finite")):
        with ran(lnb, TILE_FORMS[case], epi=("qkv_rope", "resid"), not_ran=others):
            t.run_attn(lnb, t.attn_model(lnb, key), key)
ROWCAST_FORMS = {"rowcast_self": "rowcast"}
if case in ROWCAST_FORMS:                                        # LNB_ROWCAST_LDS=0: the self-feeding kernel at a K the LDS-fed one takes by default
    for rows in (1, 7):
        with ran(lnb, ROWCAST_FORMS[case], epi="resid", not_ran=("rowcast_lds",)):
            t.run_down(lnb, t.down_model(lnb, "wide1024"), ("wide1024", rows))
print("op crafted child ok", case)
"""
CHILD_ENV = {"tile64": {"LNB_GEMM_TILE": "64", "LNB_PREFILL_STREAM": "0"}, "tile128": {"LNB_GEMM_TILE": "128", "LNB_PREFILL_STREAM": "0"}, "rowcast_self": {"LNB_ROWCAST_LDS": "0"}}


@pytest.mark.parametrize("case", sorted(CHILD_ENV))
def test_once_knob_forms_in_a_child_process(lnb, case):
    code = CHILD % dict(root=ROOT, pkg=PKG, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, LNB_TEST_OP_CRAFTED_CASE=case, **CHILD_ENV[case]))
    assert r.returncode == 0 and "op crafted child ok " + case in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- a whole one-block model: the matrix-core copy and the batched step ----------------------------------------------------------------------------------------------
VOCAB = 64
COPY_FORMS = {"prefill": "gemm_stream.copy"}
STEP_FORMS = {(3, "1"): {"mfma_pair": ("qkv_rope", "resid"), "mfma_stream.c2": "silu_mul"}, (17, "1"): {"mfma_pair": ("qkv_rope", "resid")},
              (3, "0"): {"mfma_stream.c1": ("qkv_rope", "resid"), "mfma_stream.c2": "silu_mul"}}
STEP_NOT = {"1": ("mfma_stream.c1",), "0": ("mfma_pair",)}


def whole_model(lnb):
    """(device model with the copy, oracle model, the attention case whose weights and rows they carry): tok_embeddings = the finite crafted rows of h, attention
    weights = a finite RoPE set's (positions 0 .. 31), gate|up = the window set's (finite everywhere, so that every token is defined), the rest synthetic"""
    a = oc.attn_case("tiny", 128, 0, 32, "finite")
    big = (np.abs(oc.wide(a["wk"])) > 2.0).any(axis=1)           # the cancelling pairs' large halves (b = a cr / ci at a small angle) would overflow a score's
    a["wk"][big] = 0                                             # exponential and leave no token defined: those rows give +0 here
    g = oc.gate_up_case("tiny", 1, "window")
    cfg = dict(oc.GEOS["tiny"], n_layers=1, vocab_size=VOCAB)
    rng = np.random.default_rng(64)
    emb, _, _ = oc.norm_rows(rng, VOCAB, cfg["dim"], nan_row=False)
    tensors = {"tok_embeddings": emb, "layers.0.attention_norm": a["nw"], "layers.0.attention.wq": a["wq"], "layers.0.attention.wk": a["wk"], "layers.0.attention.wv": a["wv"],
               "layers.0.ffn_norm": g["nw"], "layers.0.feed_forward.w1": g["w1"], "layers.0.feed_forward.w3": g["w3"]}
    om, gm = orc.Model(**cfg).fill_synthetic(9), lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(9)
    for name, t in tensors.items():
        om.set_tensor(name + ".weight", t); gm.set_tensor(name + ".weight", t)
    return gm.finalize().enable_batch(), om.finalize(), a, emb


def test_whole_block_model_with_the_copy_and_the_batched_step(lnb, monkeypatch):
    """... and LNB_STREAM_PAIR=0 (LIVE): the thin products of the three-member step on mfma_stream_kernel<1, ...> instead of mfma_pair_kernel"""
    gm, om, a, emb = whole_model(lnb)
    s = oc.shape_of("tiny")
    # 17 rows at position 0 from the matrix-core copy: the K and V rows are the composition's
    toks = np.arange(17, dtype=np.int32)
    r = oc.kv_ref(dict(geo="tiny", start_pos=0, h=emb[:17], nw=a["nw"], wk=a["wk"], wv=a["wv"]))
    gc = lnb.InferenceContext(gm, 32)
    with ran(lnb, COPY_FORMS["prefill"], epi="qkv_rope", not_ran=("gemm_stream.chain", "gemm_mfma")):
        gc.Forward(toks, 0, want_logits=False)
    check(gc.CacheK(0)[:17].reshape(17, -1), r["xk_rope"], ("copy", "K")); check(gc.CacheV(0)[:17].reshape(17, -1), r["xv"], ("copy", "V"))
    gc.close()
    steps = 3
    for n, pair in ((3, "1"), (17, "1"), (3, "0")):              # members at different positions, each against the oracle's own one-token steps
        monkeypatch.setenv("LNB_STREAM_PAIR", pair)
        plens = [2 + (5 * m) % 12 for m in range(n)]         # (prompts of 2 .. 13 rows, below 16: the row-per-workgroup attention, which multiplies and then adds)
        prompts = [((7 * m + np.arange(plens[m])) % VOCAB).astype(np.int32) for m in range(n)]
        ocs = [orc.Context(om, plens[m] + steps + 2) for m in range(n)]
        refs = [[int(t) for t in ocs[m].generate(prompts[m], steps + 1)[0]] for m in range(n)]
        ctxs = [lnb.InferenceContext(gm, plens[m] + steps + 2) for m in range(n)]
        firsts = [ctxs[m].Forward(prompts[m], 0, want_logits=False)[1] for m in range(n)]
        assert firsts == [x[0] for x in refs]
        b = lnb.Batch(ctxs)
        with ran(lnb, STEP_FORMS[(n, pair)], not_ran=STEP_NOT[pair]):
            got, _ = b.decode(firsts, plens, steps)
        for m in range(n):
            assert [int(t) for t in got[m]] == refs[m][1:], (n, pair, m)
            T = plens[m] + steps
            check(ctxs[m].CacheK(0)[:T], ocs[m].cache(0, 0)[:T], ("batch", n, pair, m, "K")); check(ctxs[m].CacheV(0)[:T], ocs[m].cache(0, 1)[:T], ("batch", n, pair, m, "V"))
        b.close()
        for c_ in ctxs:
            c_.close()
        for o_ in ocs:
            o_.close()
    gm.close(); om.close()
