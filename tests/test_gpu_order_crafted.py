"""Every product form on rows that reveal a wrong order of the adds (-m gpu).  tests/order_craft.py builds zero-sum rows, ladder rows and a head row whose f32
sum is nothing but rounding residue -- or exactly +0 -- so that a chain split in two, two swapped stages, a rotated unit or ONE transposed pair of neighbours
changes the leading bits of a bf16 output; tests/test_order_crafted_cpu.py proves that of every wrong order on its list, for every set run here.  The reference
is the oracle's orc_linear_bf16 (and the oracle's SiLU * up behind the gate|up kernel), never the device.  Every comparison sits inside a `ran` block
(tests/form_tally.py): the launch tally proves which kernel made the bits.

  lnb_op_linear            gemv_chain.rw16 / rw32 / rw64; rowcast (K no multiple of 512, and K = 512: rowcast_lds_kernel wants two stages); rowcast_lds (two, three
                           and eight stages); gemv_quad (one, two, three and sixteen stages of 256); from 16 rows on gemm_stream.chain / rowcast / copy at one, two
                           and four batch tiles per wave, the two-weight-tile forms, both dispatch orders, gemm_blgp, gemm_mfma.t16; in child processes (ONCE knobs)
                           gemm_mfma.t64 / t128 and rowcast where rowcast_lds is the default
  lnb_op_rmsnorm_gate_up   gemv_chain.rw56 from the raw bf16 behind the fused norm, the crafted chain once on the gate side and once on the up side
  lnb_op_rmsnorm_head      gemv_chain.rw64 with the fused norm (the raw head)
  a gate|up part stage     (tests/test_gpu_op_crafted.py's harness) gemv_chain.rw56 and, under the throughput schedule, rw56_tp; gemv_chain.rw28 (LNB_RW_W13=28)
  a whole one-block model  with the matrix-core copy: the set's rows are tok_embeddings behind the attention norm, wv carries the set and the V rows of the cache are the
                           product's truncated output -- gemm_stream.copy (a 17-row Forward), mfma_pair and mfma_stream.c1 (a batched step of 3 and of 17 members)

  the 13-bit packed copies  gemv_chain_pk (lnb_op_rmsnorm_gate_up, packed) and gemv_head_pk (lnb_op_rmsnorm_head, packed) on order_craft's packed groups: a packable
                           matrix spans 30 binades, so the exponents ride on the norm weight, one column profile per matrix; the packed status is asserted

Exempt, one line each:
  mfma_stream.c2: the fat gate|up product of a batched step is observable through the step's tokens only, and a token does not carry a residue of 2^-80."""
import os
import subprocess
import sys

import numpy as np
import pytest

import op_craft as oc
import order_craft as od
from form_tally import count, ran
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


def check(lnb, key, rw, tag=()):
    """lnb_op_linear on the set: every bit the oracle's; the message names the kinds of the first rows that differ"""
    s = od.get_set(*key)
    y = lnb.op_linear(s["x"], s["w"], rw=rw)
    bad = np.argwhere(y != s["ref"])
    assert bad.size == 0, "%s set %s rw %d: %d of %d outputs differ; first (x row, w row, kind, got, oracle): %s" % (
        tag, key, rw, len(bad), y.size, [(int(r), int(i), s["kinds"][i], hex(int(y[r, i])), hex(int(s["ref"][r, i]))) for r, i in bad[:6]])


# ---- one to fifteen rows: the GEMVs ----------------------------------------------------------------------------------------------------------------------------
CHAIN_FORMS = {16: "gemv_chain.rw16", 32: "gemv_chain.rw32", 64: "gemv_chain.rw64"}
GEMV_OTHERS = ("rowcast", "rowcast_lds", "gemv_quad", "gemm_mfma", "gemm_stream", "gemm_blgp")


@pytest.mark.parametrize("rw", sorted(CHAIN_FORMS))
def test_chain_gemv(lnb, rw):
    with ran(lnb, CHAIN_FORMS[rw], epi="store", not_ran=GEMV_OTHERS + tuple(f for r, f in CHAIN_FORMS.items() if r != rw)):
        for key in od.GEMV_SETS:
            check(lnb, key, rw)
    assert count(lnb, CHAIN_FORMS[rw], "store") == len(od.GEMV_SETS)


def test_row_broadcast_gemv_self_feeding(lnb):
    with ran(lnb, "rowcast", epi="store", not_ran=("rowcast_lds", "gemv_chain", "gemv_quad")):
        for key in od.ROWCAST_SETS:
            check(lnb, key, 4)


def test_row_broadcast_gemv_fed_through_the_lds(lnb):
    with ran(lnb, "rowcast_lds", epi="store", not_ran=("rowcast", "gemv_chain", "gemv_quad")):
        for key in od.ROWCAST_LDS_SETS:
            check(lnb, key, 4)
    assert count(lnb, "rowcast_lds", "store") == len(od.ROWCAST_LDS_SETS)


def test_quad_gemv(lnb):
    with ran(lnb, "gemv_quad", epi="store", not_ran=("rowcast", "rowcast_lds", "gemv_chain")):
        for key in od.QUAD_SETS:
            check(lnb, key, 24)
    assert count(lnb, "gemv_quad", "store") == len(od.QUAD_SETS)


# ---- sixteen rows and more: the matrix cores ---------------------------------------------------------------------------------------------------------------------
STREAM_FORMS = {("chain", 1): "gemm_stream.chain.ntw1", ("chain", 2): "gemm_stream.chain.ntw2", ("chain", 4): "gemm_stream.chain.ntw4",
                ("rowcast", 1): "gemm_stream.rowcast.ntw1", ("rowcast", 2): "gemm_stream.rowcast.ntw2", ("rowcast", 4): "gemm_stream.rowcast.ntw4",
                ("copy", 1): "gemm_stream.copy.ntw1", ("copy", 2): "gemm_stream.copy.ntw2", ("copy", 4): "gemm_stream.copy.ntw4"}
STREAM_RW = {"chain": (16, 32, 64), "rowcast": (4,), "copy": (16,)}


@pytest.mark.parametrize("ntw", [1, 2, 4])
@pytest.mark.parametrize("source", sorted(STREAM_RW))
def test_streaming_product(lnb, monkeypatch, source, ntw):
    """gemm_stream_kernel from the chain layouts (transposed inside the quad), the row-broadcast layout and the matrix-core copy (LNB_OP_STREAM=1), with one, two and
    four batch tiles of 16 rows per wave: 17 rows = two tiles, the second with one row; 83 = six, the last with three"""
    monkeypatch.setenv("LNB_GS_NTW", str(ntw)); monkeypatch.setenv("LNB_GEMM_BLGP", "0"); monkeypatch.setenv("LNB_GS_TT", "0")
    monkeypatch.setenv("LNB_OP_STREAM", "1" if source == "copy" else "0")
    others = tuple(f for f in lnb.form_names() if f.startswith("gemm_stream.") and f != STREAM_FORMS[(source, ntw)])
    with ran(lnb, STREAM_FORMS[(source, ntw)], epi="store", not_ran=others + ("gemm_mfma", "gemm_blgp")):
        for key in od.STREAM_SETS:
            for rw in STREAM_RW[source]:
                check(lnb, key, rw, (source, ntw))


TT_FORMS = {"rowcast": "gemm_stream.rowcast.ntw4_tt", "copy": "gemm_stream.copy.ntw4_tt"}


@pytest.mark.parametrize("source", sorted(TT_FORMS))
def test_streaming_product_with_two_weight_tiles_per_wave(lnb, monkeypatch, source):
    """LNB_GS_TT=1: 40 weight rows = three tiles (a pair and a single one), 100 = seven"""
    monkeypatch.setenv("LNB_GS_NTW", "4"); monkeypatch.setenv("LNB_GS_TT", "1"); monkeypatch.setenv("LNB_OP_STREAM", "1" if source == "copy" else "0")
    with ran(lnb, TT_FORMS[source], epi="store", not_ran=("gemm_mfma", "gemm_blgp", "gemm_stream.chain")):
        for key in od.STREAM_SETS:
            check(lnb, key, 4 if source == "rowcast" else 16, (source, "tt"))


def test_blgp_product(lnb, monkeypatch):
    monkeypatch.setenv("LNB_GEMM_BLGP", "2"); monkeypatch.setenv("LNB_OP_STREAM", "0")
    with ran(lnb, "gemm_blgp", epi="store", not_ran=("gemm_mfma", "gemm_stream")):
        for key in od.STREAM_SETS:
            for rw in (16, 32, 64):
                check(lnb, key, rw, ("blgp",))


def test_lds_tiled_product_on_the_16_row_tile(lnb):
    """K = 320 and 192 are no multiples of 128: gemm_mfma_kernel, the 16-row tile (few tiles), from every resident layout"""
    with ran(lnb, "gemm_mfma.t16", epi="store", not_ran=("gemm_stream", "gemm_blgp", "gemm_mfma.t64", "gemm_mfma.t128")):
        for key in od.MFMA_SETS[:2]:
            for rw in (16, 32, 64):
                check(lnb, key, rw, ("t16",))


# ---- the forms a ONCE knob picks: a fresh process each ---------------------------------------------------------------------------------------------------------
def run_child(code, env, marker):
    r = subprocess.run([sys.executable, "-c", code % dict(root=ROOT, pkg=PKG, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


CHILD_HEAD = r"""
import os, sys
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
import lnb
import order_craft as od
import test_gpu_order_crafted as t
from form_tally import count, ran
"""

TILE_CHILD = CHILD_HEAD + r"""
TILE_FORMS = {"64": "gemm_mfma.t64", "128": "gemm_mfma.t128"}
FORM = TILE_FORMS[os.environ["LNB_GEMM_TILE"]]
with ran(lnb, TILE_FORMS[os.environ["LNB_GEMM_TILE"]], epi="store", not_ran=tuple(f for f in ("gemm_mfma.t16", "gemm_mfma.t64", "gemm_mfma.t128") if f != FORM) + ("gemm_stream", "gemm_blgp")):
    for key in od.MFMA_SETS + od.STREAM_SETS[:1]:
        for rw in (16, 64, 4) if key[2] %% 128 == 0 else (16, 64):
            t.check(lnb, key, rw, (FORM,))
print("tile child ok", FORM)
"""


@pytest.mark.parametrize("tile", ["64", "128"])
def test_lds_tiled_product_on_the_64_row_tiles(lnb, tile):
    """LNB_GEMM_TILE = 64 / 128 with LNB_PREFILL_STREAM=0 (both ONCE): ragged batch tiles (17, 83 rows), ragged weight tiles (40, 100, 130 rows), K = 192, 320, 256, 896"""
    run_child(TILE_CHILD, {"LNB_GEMM_TILE": tile, "LNB_PREFILL_STREAM": "0"}, "tile child ok gemm_mfma.t" + tile)


ROWCAST_CHILD = CHILD_HEAD + r"""
with ran(lnb, "rowcast", epi="store", not_ran=("rowcast_lds",)):
    for key in od.ROWCAST_LDS_SETS:
        t.check(lnb, key, 4, ("rowcast",))
print("rowcast child ok")
"""


def test_row_broadcast_gemv_self_feeding_where_the_lds_form_is_the_default(lnb):
    run_child(ROWCAST_CHILD, {"LNB_ROWCAST_LDS": "0"}, "rowcast child ok")


ORDER_CHILD = CHILD_HEAD + r"""
ORDER_FORMS = {"1": "gemm_stream_order.rows", "0": "gemm_stream_order.tiles"}
ORDER = os.environ["LNB_GS_ORDER"]
for ntw in ("1", "2"):
    os.environ["LNB_GS_NTW"] = ntw                           # LIVE
    for op_stream, rw in (("0", 16), ("0", 4), ("1", 16)):
        os.environ["LNB_OP_STREAM"] = op_stream              # LIVE
        with ran(lnb, ORDER_FORMS[ORDER], epi="store", not_ran=(ORDER_FORMS[str(1 - int(ORDER))], "gemm_mfma")):
            for key in od.STREAM_SETS:
                t.check(lnb, key, rw, (ORDER, ntw, op_stream))
print("order child ok", ORDER)
"""


@pytest.mark.parametrize("order", ["0", "1"])
def test_streaming_product_in_both_dispatch_orders(lnb, order):
    """LNB_GS_ORDER (ONCE): the same workgroups on other (tile group, row group) pairs, from every source -- two and six row groups at one tile per wave"""
    run_child(ORDER_CHILD, {"LNB_GS_ORDER": order}, "order child ok " + order)


# ---- behind a fused norm -------------------------------------------------------------------------------------------------------------------------------------------
def test_raw_gate_up_with_the_crafted_chain_on_either_side(lnb):
    """gemv_chain_kernel<56, 2, ...> (packed = 0): h = +-1.0 and the norm weight 0x3F81 * 2^j hand the product the set's x row; the ladder rows' exact +0 gives
    SiLU(0) * up = 0 and 1.0-gate times 0 = 0, any residue shows (tests/test_order_crafted_cpu.py, routes gate and up)"""
    key = od.NORM_SETS[0]
    s = od.get_set(*key)
    h, nw = od.norm_front(s["pat"][0])
    const_u, const_g = od.gate_up_constant(s, od.U_CONST), od.gate_up_constant(s, od.G_CONST)
    n = s["n"]
    with ran(lnb, "gemv_chain.rw56", epi="silu_mul", not_ran=("gemv_chain_pk", "gemv_chain.rw56_tp")):
        y, _ = lnb.op_rmsnorm_gate_up(h, nw, oc.EPS, s["w"], const_u, packed=0)
        ref = oc.silu_mul_ref(s["ref"][0], np.full(n, od.U_CONST, dtype=np.uint16))[1]
        assert np.array_equal(y, ref), ("gate", np.argwhere(y != ref)[:6].tolist())
        y, _ = lnb.op_rmsnorm_gate_up(h, nw, oc.EPS, const_g, s["w"], packed=0)
        ref = oc.silu_mul_ref(np.full(n, od.G_CONST, dtype=np.uint16), s["ref"][0])[1]
        assert np.array_equal(y, ref), ("up", np.argwhere(y != ref)[:6].tolist())
    assert count(lnb, "gemv_chain.rw56", "silu_mul") == 2


def test_raw_head_behind_the_fused_norm(lnb):
    with ran(lnb, "gemv_chain.rw64", epi="store", not_ran=("gemv_head_pk",)):
        for key in od.NORM_SETS:
            s = od.get_set(*key)
            h, nw = od.norm_front(s["pat"][0])
            y, _ = lnb.op_rmsnorm_head(h, nw, oc.EPS, s["w"], packed=0)
            assert np.array_equal(y, s["ref"][0]), (key, np.argwhere(y != s["ref"][0])[:6].tolist())


# ---- the 13-bit packed copies -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", od.PACKED_KS)
def test_packed_gate_up_with_the_crafted_chain_on_either_side(lnb, K):
    """gemv_chain_pk_kernel: two and eight 128-step stages (five in flight); status 0 = the matrix was packed and the packed kernel ran -- the tally says so too"""
    for m in od.get_packed(K):
        n = m["n"]
        with ran(lnb, "gemv_chain_pk", epi="silu_mul", not_ran=("gemv_chain.rw56", "gemv_chain.rw56_tp")):
            y, st = lnb.op_rmsnorm_gate_up(m["h"], m["nw"], oc.EPS, m["w"], od.packed_constant(m, od.U_CONST), packed=1)
            ref = oc.silu_mul_ref(m["ref"], np.full(n, od.U_CONST, dtype=np.uint16))[1]
            assert st == 0 and np.array_equal(y, ref), (K, m["name"], "gate", st, np.argwhere(y != ref)[:6].tolist())
            y, st = lnb.op_rmsnorm_gate_up(m["h"], m["nw"], oc.EPS, od.packed_constant(m, od.G_CONST), m["w"], packed=1)
            ref = oc.silu_mul_ref(np.full(n, od.G_CONST, dtype=np.uint16), m["ref"])[1]
            assert st == 0 and np.array_equal(y, ref), (K, m["name"], "up", st, np.argwhere(y != ref)[:6].tolist())
        assert count(lnb, "gemv_chain_pk", "silu_mul") == 2


@pytest.mark.parametrize("K", od.PACKED_KS)
def test_packed_head(lnb, K):
    """gemv_chain_pk_kernel in 128-row blocks as two chains of 64 (112 rows: a ragged block)"""
    for m in od.get_packed(K):
        with ran(lnb, "gemv_head_pk", epi="store", not_ran=("gemv_chain.rw64",)):
            y, st = lnb.op_rmsnorm_head(m["h"], m["nw"], oc.EPS, m["w"], packed=1)
        assert st == 0 and np.array_equal(y, m["ref"]), (K, m["name"], st, np.argwhere(y != m["ref"])[:6].tolist())


# ---- a gate|up part stage: the block forms no operator entry point launches ------------------------------------------------------------------------------------------
W13_FORMS = {("56", "latency"): "gemv_chain.rw56", ("56", "throughput"): "gemv_chain.rw56_tp", ("28", "latency"): "gemv_chain.rw28"}


@pytest.mark.parametrize("rw13", ["56", "28"])
def test_gate_up_part_stage_on_the_56_and_28_row_blocks(lnb, monkeypatch, rw13):
    """LNB_RW_W13 (LIVE, read when the model is created) with LNB_W13_PACKED=0: FFN hidden 896 = 16 blocks of 56 (eight ring stages, six under the throughput
    schedule) or 32 of 28; the crafted chain on the gate side, then on the up side"""
    import test_gpu_op_crafted as t
    monkeypatch.setenv("LNB_RW_W13", rw13); monkeypatch.setenv("LNB_W13_PACKED", "0")
    s = od.get_set(*od.PART_SETS[0])
    F = s["n"]
    h, nw = od.norm_front(s["pat"][0])
    for side in ("gate", "up"):
        if side == "gate":
            w1, w3 = s["w"], od.gate_up_constant(s, od.U_CONST)
            ref = oc.silu_mul_ref(s["ref"][0], np.full(F, od.U_CONST, dtype=np.uint16))[1]
        else:
            w1, w3 = od.gate_up_constant(s, od.G_CONST), s["w"]
            ref = oc.silu_mul_ref(np.full(F, od.G_CONST, dtype=np.uint16), s["ref"][0])[1]
        gm = t.part_model(lnb, "tiny", 1, {"ffn_norm": nw, "feed_forward.w1": w1, "feed_forward.w3": w3})
        assert gm.ffn_hidden == F
        for sched in ("latency", "throughput") if rw13 == "56" else ("latency",):
            ctx = lnb.InferenceContext(gm, 16).set_schedule(sched)
            t.poke(lnb, ctx, 0, h[None, :]); t.poke(lnb, ctx, 2, np.full((1, F), oc.QNAN, dtype=np.uint16))
            with ran(lnb, W13_FORMS[(rw13, sched)], epi="silu_mul", not_ran=("gemv_chain_pk",) + tuple(f for f in W13_FORMS.values() if f != W13_FORMS[(rw13, sched)])):
                t.call(lnb, ctx, 1)
            out = t.peek(lnb, ctx, 2, (1, F))[0]
            ctx.close()
            assert np.array_equal(out, ref), (rw13, side, sched, np.argwhere(out != ref)[:6].tolist())
        gm.close()


# ---- a whole one-block model with the matrix-core copy ------------------------------------------------------------------------------------------------------------------
VOCAB = 64
COPY_FORMS = {"prefill": "gemm_stream.copy.ntw1"}
STEP_FORMS = {(3, "1"): "mfma_pair", (17, "1"): "mfma_pair", (3, "0"): "mfma_stream.c1"}
STEP_NOT = {"1": ("mfma_stream.c1",), "0": ("mfma_pair",)}


def test_whole_block_model_with_the_copy_and_the_batched_step(lnb, monkeypatch):
    """token m is row m of the set (behind the attention norm), wv the set's matrix: the V row a call appends for token m is the product's row m, bit for bit the
    oracle's cache row and the set's reference -- from the copy in a 17-row Forward, and in a batched step whose member m feeds token m behind a two-token prompt
    (mfma_pair_kernel; LNB_STREAM_PAIR=0, LIVE: mfma_stream_kernel<1, ...>)"""
    s = od.get_set(*od.WHOLE_SETS[0])
    rows = s["rows"]
    hrows, nw = od.norm_front_rows(s)
    cfg = dict(oc.GEOS["tiny"], n_layers=1, vocab_size=VOCAB)
    om, gm = orc.Model(**cfg).fill_synthetic(9), lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(9)
    emb = om.get_tensor("tok_embeddings.weight").reshape(VOCAB, cfg["dim"]).copy()
    emb[:rows] = hrows
    for name, a in (("tok_embeddings", emb), ("layers.0.attention_norm", nw), ("layers.0.attention.wv", s["w"])):
        om.set_tensor(name + ".weight", a); gm.set_tensor(name + ".weight", a)
    om.finalize(); gm.finalize().enable_batch()
    toks = np.arange(rows, dtype=np.int32)
    oc_, gc = orc.Context(om, 32), lnb.InferenceContext(gm, 32)
    oc_.forward(toks, 0, want_logits=False)
    assert np.array_equal(oc_.cache(0, 1)[:rows].reshape(rows, -1), s["ref"])          # the oracle's whole forward gives the set's reference
    with ran(lnb, COPY_FORMS["prefill"], epi="qkv_rope", not_ran=("gemm_stream.chain", "gemm_stream.rowcast", "gemm_mfma")):
        gc.Forward(toks, 0, want_logits=False)
    assert np.array_equal(gc.CacheV(0)[:rows].reshape(rows, -1), s["ref"]) and np.array_equal(gc.CacheK(0)[:rows], oc_.cache(0, 0)[:rows])
    gc.close(); oc_.close()
    for n, pair in sorted(STEP_FORMS):
        monkeypatch.setenv("LNB_STREAM_PAIR", pair)
        prompts = [np.array([20 + m, 40 + m], dtype=np.int32) for m in range(n)]          # (generic rows of the synthetic table)
        ocs = [orc.Context(om, 8) for _ in range(n)]
        ctxs = [lnb.InferenceContext(gm, 8) for _ in range(n)]
        for m in range(n):
            ocs[m].forward(prompts[m], 0, want_logits=False); ocs[m].forward(np.array([m], dtype=np.int32), 2, want_logits=False)
            ctxs[m].Forward(prompts[m], 0, want_logits=False)
        b = lnb.Batch(ctxs)
        with ran(lnb, STEP_FORMS[(n, pair)], epi="qkv_rope", not_ran=STEP_NOT[pair]):
            b.decode(list(range(n)), [2] * n, 1)
        for m in range(n):
            assert np.array_equal(ctxs[m].CacheV(0)[2].ravel(), s["ref"][m]), (n, pair, m, "V")
            assert np.array_equal(ctxs[m].CacheV(0)[:3], ocs[m].cache(0, 1)[:3]) and np.array_equal(ctxs[m].CacheK(0)[:3], ocs[m].cache(0, 0)[:3]), (n, pair, m)
        b.close()
        for c_ in ctxs:
            c_.close()
        for o_ in ocs:
            o_.close()
    gm.close(); om.close()
