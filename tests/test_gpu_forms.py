"""Every kernel form the launch layer can pick, run once and PROVEN to have run (-m gpu).  The launch layer chooses a kernel by shape and by LNB_* knob; the
launch tally (csrc/lnb_forms.h, tests/form_tally.py) says which one a call took, so every case here names the form it is about and fails when that form did not
run -- a ONCE knob set too late, a shape that falls on the other side of a threshold.  Oracle: tests/form_cases.py (one CPU run per geometry), bit for bit.

* models whose sizes are no multiples of 128 on the DEFAULT dispatch: gemm_mfma_kernel with all four epilogues, the one-wave row norm, chain GEMVs for wo / w2;
* the 64-row tiles of gemm_mfma_kernel (LNB_GEMM_TILE = 64 / 128, ONCE: a child process each);
* gemm_stream_kernel with 1 / 2 / 4 batch tiles per wave from each source, both dispatch orders, LNB_PREFILL_NATIVE=0, LNB_NORM_ROWS_WIDE=0;
* batched decode as rows (LNB_BATCH_GROUPS=0), the row-broadcast GEMV pair (LNB_ROWCAST_LDS), the throughput gate|up kernels (LNB_TP_W13),
  the resident layouts LNB_RW_WO / LNB_RW_OUT pick, pipeline stage steps replayed and eager (LNB_PIPELINE_GRAPH)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import form_cases as fc
from form_tally import count, ran
from linear_cases import bf, orc_linear
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")
ALL_EPIS = ("qkv_rope", "resid", "silu_mul", "store")


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


def run_child(code, env, marker):
    r = subprocess.run([sys.executable, "-c", code % dict(root=ROOT, pkg=PKG, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


CHILD_HEAD = r"""
import os, sys
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
import numpy as np
import lnb
import form_cases as fc
import linear_cases as lc
from form_tally import count, ran
ALL_EPIS = ("qkv_rope", "resid", "silu_mul", "store")
"""


# ---- 1. sizes that are no multiples of 128, no knob set ---------------------------------------------------------------------------------------------
# Which form each product takes, from the dispatch code: gemm_dispatch (lnb_api.cpp) sends a product of 16+ rows to gemm_stream_kernel only when its K is a
# multiple of 128; lnbk_rmsnorm_rows takes the wide kernel only then; auto_rw gives wo / w2 the row-broadcast layout only then, else 16-row chain blocks.
#   odd192      K = 192 (wq|wk|wv, wo, gate|up, head) and 704 (w2): everything on gemm_mfma_kernel's 16-row tile, the one-wave norm; decode: gemv_chain_kernel<16>
#               for all five products, wo and w2 with the residual epilogue
#   odd_hidden  K = 256 everywhere but w2 (888): wq|wk|wv, gate|up, head stream from their chain layouts, wo from its row-broadcast layout, w2 alone on
#               gemm_mfma_kernel; the wide norm; decode: wo on rowcast_kernel (256 is no multiple of rowcast_lds_kernel's 512-step stage), w2 on gemv_chain_kernel<16>
PREFILL_FORMS = {
    "odd192": {"gemm_mfma.t16": ALL_EPIS, "rmsnorm_rows.wave": None},
    "odd_hidden": {"gemm_mfma.t16": "resid", "gemm_stream.chain.ntw1": ("qkv_rope", "silu_mul", "store"), "gemm_stream.rowcast.ntw1": "resid", "rmsnorm_rows.wide": None},
}
PREFILL_NOT = {"odd192": ("gemm_stream", "gemm_blgp", "gemm_mfma.t64", "gemm_mfma.t128", "rmsnorm_rows.wide"),
               "odd_hidden": ("gemm_stream.copy", "gemm_blgp", "gemm_mfma.t64", "gemm_mfma.t128", "rmsnorm_rows.wave")}
DECODE_FORMS = {
    "odd192": {"gemv_chain.rw16": ALL_EPIS},
    "odd_hidden": {"gemv_chain.rw16": ALL_EPIS, "rowcast": "resid"},
}
DECODE_NOT = ("rowcast_lds", "gemv_quad", "gemv_chain_pk", "gemv_chain.rw32", "gemv_chain.rw64", "gemm_mfma", "gemm_stream", "rmsnorm_rows")


@pytest.mark.parametrize("geo", ["odd192", "odd_hidden"])
def test_models_off_the_128_grid_on_the_default_dispatch(lnb, geo):
    R, gm, nl = fc.reference(geo), fc.gpu_model(lnb, geo), fc.GEOS[geo]["n_layers"]
    for rows in (17, 83):
        with ran(lnb, PREFILL_FORMS[geo], not_ran=PREFILL_NOT[geo]):
            gc = fc.check_prefill(lnb, gm, R, rows, (geo,))
        # per layer: wq|wk|wv, wo, gate|up, w2; once: the head.  odd192: all nine on gemm_mfma_kernel; odd_hidden: w2 only -- no product with K = 888 streams
        assert count(lnb, "gemm_mfma", "resid") == (2 * nl if geo == "odd192" else nl)
        assert count(lnb, "gemm_mfma") == (4 * nl + 1 if geo == "odd192" else nl)
        assert count(lnb, "gemm_stream") == (0 if geo == "odd192" else 3 * nl + 1) and count(lnb, "gemm_stream", "resid") == (0 if geo == "odd192" else nl)
        assert count(lnb, "rmsnorm_rows") == 2 * nl + 1
        if rows == 17:
            gc.close()
    with ran(lnb, DECODE_FORMS[geo], not_ran=DECODE_NOT + (("rowcast",) if geo == "odd192" else ())):
        fc.check_steps(gc, R, fc.N_STEPS, (geo,))
    # decode: wo and w2 -- both chain GEMVs (odd192), or the self-feeding row-broadcast kernel for wo and the chain GEMV for w2 (odd_hidden)
    assert count(lnb, "gemv_chain.rw16", "resid") == fc.N_STEPS * nl * (2 if geo == "odd192" else 1)
    assert count(lnb, "rowcast", "resid") == (0 if geo == "odd192" else fc.N_STEPS * nl)
    with ran(lnb, {"gemv_chain.rw16": ALL_EPIS, "gemm_mfma.t16": "resid"}):     # 3 rows: the GEMVs with three launch rows; 20 rows: the prefill forms again
        fc.check_appends(gc, R, (geo,))
    with ran(lnb, {"gemv_chain.rw16": ALL_EPIS}, not_ran=("gemm_mfma", "gemm_stream")):      # (counted once, when the loop is captured)
        fc.check_greedy(gc, R, (geo,))
    gc.close()


# ---- 2. the 64-row tiles of gemm_mfma_kernel ---------------------------------------------------------------------------------------------------------
TILE_CHILD = CHILD_HEAD + r"""
from linear_cases import check_linear_bit_exact, check_linear_special_values
TILE_FORMS = {"64": "gemm_mfma.t64", "128": "gemm_mfma.t128"}
TILE = os.environ["LNB_GEMM_TILE"]
FORM = TILE_FORMS[TILE]
OTHERS = tuple(f for f in ("gemm_mfma.t16", "gemm_mfma.t64", "gemm_mfma.t128") if f != FORM) + ("gemm_stream", "gemm_blgp")
# ragged M (83, 130: the last 64-row batch tile holds 19 / 2 rows), ragged N (100, 520: the last 64-row weight tile holds 36 / 8), K not a multiple of the slab (896 is,
# 768 and 256 are; the models below bring 888), two row tiles for the 64 x 64 form, every resident layout (the f32-x B tile of the one-chain 64-row forms included)
with ran(lnb, TILE_FORMS[TILE], epi="store", not_ran=OTHERS):
    for rows, n, k in ((83, 100, 896), (130, 520, 256)):
        for rw in (16, 32, 64, 4):
            check_linear_bit_exact(lnb, rows, n, k, rw, seed=rows * 7 + n + k + rw)
    check_linear_bit_exact(lnb, 83, 100, 768, 24, seed=5)
    n_plain = count(lnb, FORM, "store")
    for rows, rw in ((20, 16), (20, 4), (130, 64)):
        check_linear_special_values(lnb, rows, rw)
assert n_plain == 9 and count(lnb, FORM, "store") == 12
for geo in ("tiny520", "odd_hidden"):
    R, gm = fc.reference(geo), fc.gpu_model(lnb, geo)
    for rows in (17, 83):
        with ran(lnb, TILE_FORMS[TILE], epi=ALL_EPIS, not_ran=OTHERS):
            gc = fc.check_prefill(lnb, gm, R, rows, (FORM, geo))
        assert count(lnb, FORM) == 4 * fc.GEOS[geo]["n_layers"] + 1
        if rows == 83:
            fc.check_steps(gc, R, 2, (FORM, geo))
        gc.close()
print("tile child ok", FORM)
"""


@pytest.mark.parametrize("tile", ["64", "128"])
def test_the_64_row_tiles_of_the_lds_tiled_prefill_product(lnb, tile):
    """gemm_mfma_kernel<*, *, 4, 64> and <*, *, 4, 128> (LNB_GEMM_TILE, with LNB_PREFILL_STREAM=0 so that every product of 16+ rows takes the LDS-tiled kernel):
    lnb_op_linear bit for bit and on the special values, then whole models -- all four epilogues -- against the oracle"""
    run_child(TILE_CHILD, {"LNB_GEMM_TILE": tile, "LNB_PREFILL_STREAM": "0"}, "tile child ok gemm_mfma.t" + tile)


# ---- 3. gemm_stream_kernel: batch tiles per wave x source, dispatch order -------------------------------------------------------------------------------
# 17 / 40 / 83 rows = 2 / 3 / 6 batch tiles of 16: a ragged last wave for two and for four tiles per wave, a ragged last tile everywhere
NTW_FORMS = {
    ("copy", 1): {"gemm_stream.copy.ntw1": ALL_EPIS}, ("copy", 2): {"gemm_stream.copy.ntw2": ALL_EPIS}, ("copy", 4): {"gemm_stream.copy.ntw4": ALL_EPIS},
    ("resident", 1): {"gemm_stream.chain.ntw1": ("qkv_rope", "silu_mul", "store"), "gemm_stream.rowcast.ntw1": "resid"},
    ("resident", 2): {"gemm_stream.chain.ntw2": ("qkv_rope", "silu_mul", "store"), "gemm_stream.rowcast.ntw2": "resid"},
    ("resident", 4): {"gemm_stream.chain.ntw4": ("qkv_rope", "silu_mul", "store"), "gemm_stream.rowcast.ntw4": "resid"},
}


@pytest.mark.parametrize("ntw", [1, 2, 4])
@pytest.mark.parametrize("source", ["copy", "resident"])
def test_streaming_prefill_product_with_one_two_and_four_batch_tiles_per_wave(lnb, monkeypatch, source, ntw):
    """LNB_GS_NTW (LIVE) forces what lnb_gemm_stream_ntw picks by shape -- two tiles per wave is the default for a ~300-row prompt at the 8B shape, one for every
    tiny shape -- from the matrix-core copy and from the resident chain and row-broadcast layouts; LNB_GEMM_BLGP held at 0 (gemm_blgp_kernel would take the chain
    layouts' one- and two-tile launches) and LNB_GS_TT at 0 (the two-weight-tile form has its own test): logits and KV bits against the oracle"""
    monkeypatch.setenv("LNB_GS_NTW", str(ntw)); monkeypatch.setenv("LNB_GEMM_BLGP", "0"); monkeypatch.setenv("LNB_GS_TT", "0")
    R, gm = fc.reference("tiny520"), fc.gpu_model(lnb, "tiny520", copy=source == "copy")
    others = tuple(f for f in lnb.form_names() if f.startswith("gemm_stream.") and f not in NTW_FORMS[(source, ntw)])
    for rows in fc.ROWS:
        with ran(lnb, NTW_FORMS[(source, ntw)], not_ran=others + ("gemm_mfma", "gemm_blgp")):
            fc.check_prefill(lnb, gm, R, rows, (source, ntw)).close()


ORDER_CHILD = CHILD_HEAD + r"""
ORDER_FORMS = {"1": "gemm_stream_order.rows", "0": "gemm_stream_order.tiles"}
ORDER = os.environ["LNB_GS_ORDER"]
FORM, OTHER = ORDER_FORMS[ORDER], ORDER_FORMS[str(1 - int(ORDER))]
R = fc.reference("tiny520")
for copy in (False, True):
    gm = fc.gpu_model(lnb, "tiny520", copy=copy)
    for ntw in ("1", "2"):                                   # (two tiles per wave: more than one row group only from 33 rows on)
        os.environ["LNB_GS_NTW"] = ntw                       # LIVE
        for rows in fc.ROWS:
            with ran(lnb, {ORDER_FORMS[ORDER]: ALL_EPIS, "gemm_stream": ALL_EPIS}, not_ran=(OTHER, "gemm_mfma")):
                fc.check_prefill(lnb, gm, R, rows, (FORM, copy, ntw)).close()
print("order child ok", FORM)
"""


@pytest.mark.parametrize("order", ["0", "1"])
def test_streaming_prefill_product_in_both_dispatch_orders(lnb, order):
    """LNB_GS_ORDER (ONCE): weight-tile groups fastest (what every short prompt gets) and row groups fastest (by default only beyond eight row groups) map the
    same workgroups to other (tile group, row group) pairs -- 1, 2, 3 and 6 row groups here, from the copy and from the resident layouts"""
    run_child(ORDER_CHILD, {"LNB_GS_ORDER": order}, "order child ok gemm_stream_order." + ("rows" if order == "1" else "tiles"))


MODEL_CHILD = CHILD_HEAD + r"""
# case -> forms that must run / prefixes that must not
CHILD_FORMS = {
    "native_off": {"gemm_mfma.t16": ALL_EPIS, "rmsnorm_rows.wide": None},
    "norm_wave": {"rmsnorm_rows.wave": None, "gemm_stream.chain.ntw1": ("qkv_rope", "silu_mul", "store")},
}
CHILD_NOT = {"native_off": ("gemm_stream", "gemm_blgp"), "norm_wave": ("rmsnorm_rows.wide",)}
case = os.environ["LNB_TEST_FORMS_CASE"]
geo, copy = "tiny520", False
R, gm = fc.reference(geo), fc.gpu_model(lnb, geo, copy=copy)
for rows in (17, 83):
    with ran(lnb, CHILD_FORMS[case], not_ran=CHILD_NOT[case]):
        gc = fc.check_prefill(lnb, gm, R, rows, (case,))
    if rows == 83:
        fc.check_steps(gc, R, 2, (case,))
    gc.close()
if case == "norm_wave":                                      # the k = 4096, 24-row adversarial families on the one-wave kernel
    with ran(lnb, "rmsnorm_rows.wave", not_ran=("rmsnorm_rows.wide",)):
        lc.check_rmsnorm_adversarial(lnb, 4096, 16, reps=2)
print("model child ok", case)
"""


def test_prefill_without_the_copy_and_without_the_resident_feed_takes_the_lds_tiled_product(lnb):
    """LNB_PREFILL_NATIVE=0 (ONCE) on a model without the matrix-core copy: nothing for gemm_stream_kernel to read, so every product is gemm_mfma_kernel's"""
    run_child(MODEL_CHILD, {"LNB_PREFILL_NATIVE": "0", "LNB_TEST_FORMS_CASE": "native_off"}, "model child ok native_off")


def test_one_wave_row_norm_where_the_wide_one_is_the_default(lnb):
    """LNB_NORM_ROWS_WIDE=0 (ONCE): rmsnorm_rows_kernel at K = 256 inside a model and at K = 4096 on the twelve adversarial families twice over"""
    run_child(MODEL_CHILD, {"LNB_NORM_ROWS_WIDE": "0", "LNB_TEST_FORMS_CASE": "norm_wave"}, "model child ok norm_wave")


# ---- 4. batched decode as rows ----------------------------------------------------------------------------------------------------------------------
GROUPS_CHILD = CHILD_HEAD + r"""
from oracle import oracle as orc
cfg = fc.GEOS["tiny520"]
gm = fc.gpu_model(lnb, "tiny520", copy=True)
om = orc.Model(**cfg).fill_synthetic(fc.SEED).finalize()
steps = 6
for n in (17, 25):
    plens = [4 + (5 * s) %% 23 for s in range(n)]
    prompts = [orc.synth_tokens(300 * n + s, plens[s], cfg["vocab_size"]) for s in range(n)]
    ocs = [orc.Context(om, plens[s] + steps + 2) for s in range(n)]
    refs = [[int(t) for t in ocs[s].generate(prompts[s], steps + 1)[0]] for s in range(n)]
    ctxs = [lnb.InferenceContext(gm, plens[s] + steps + 2) for s in range(n)]
    firsts = [ctxs[s].Forward(prompts[s], 0, want_logits=False)[1] for s in range(n)]
    assert firsts == [r[0] for r in refs]
    b = lnb.Batch(ctxs)
    # 17..32 members with the knob off: every product a row product of gemm_stream_kernel on the copy, the row norm in front -- no column kernel, no column norm
    with ran(lnb, {"gemm_stream.copy": ALL_EPIS, "rmsnorm_rows.wide": None}, not_ran=("mfma_pair", "mfma_stream", "batch_rmsnorm", "gemm_mfma")):
        got, _ = b.decode(firsts, plens, steps)
    for s in range(n):
        assert [int(t) for t in got[s]] == refs[s][1:], (n, s)
        T = plens[s] + steps
        for l in range(cfg["n_layers"]):
            assert (ocs[s].cache(l, 0)[:T] == ctxs[s].CacheK(l)[:T]).all() and (ocs[s].cache(l, 1)[:T] == ctxs[s].CacheV(l)[:T]).all(), (n, s, l)
    b.close()
    for c in ctxs: c.close()
    for oc in ocs: oc.close()
print("groups child ok")
"""


def test_seventeen_to_thirty_two_sequences_decode_as_rows_with_the_groups_knob_off(lnb):
    """LNB_BATCH_GROUPS=0 (ONCE): 17 and 25 members of a model WITH the copy, each against its own oracle run -- the plan the CPU test checks, run"""
    run_child(GROUPS_CHILD, {"LNB_BATCH_GROUPS": "0"}, "groups child ok")


# ---- 5. the row-broadcast GEMV pair -------------------------------------------------------------------------------------------------------------------
ROWCAST_FORMS = {"lds": "rowcast_lds", "self": "rowcast"}       # the form a case requires; the other one must not run


def rowcast_cases(lnb, which):
    """lnb_op_linear at two K that are whole numbers of rowcast_lds_kernel's 512-step stages (store), then a model whose wo (K = 1024) and w2 (K = 3584) are:
    17-row prefill and four one-token steps -- the residual epilogue"""
    form, other = ROWCAST_FORMS[which], ROWCAST_FORMS["self" if which == "lds" else "lds"]
    with ran(lnb, ROWCAST_FORMS[which], epi="store", not_ran=(other,)):
        for rows, n, k in ((1, 64, 1024), (3, 100, 1536)):
            rng = np.random.default_rng(rows * 1000003 + n * 101 + k + 4)
            x, w = bf(rng.standard_normal((rows, k))), bf(rng.standard_normal((n, k)) * 0.05)
            assert (lnb.op_linear(x, w, rw=4) == orc_linear(x, w)).all(), (form, rows, n, k)
    cfg = fc.GEOS["wide1024"]
    om, gm = orc.Model(**cfg).fill_synthetic(fc.SEED).finalize(), fc.gpu_model(lnb, "wide1024")
    toks = orc.synth_tokens(21, 17, cfg["vocab_size"])
    oc, gc = orc.Context(om, 32), lnb.InferenceContext(gm, 32)
    lo, tok = oc.forward(toks, 0)
    lg, tg = gc.Forward(toks, 0)
    assert fc.same(lg, lo) and tg == tok
    with ran(lnb, ROWCAST_FORMS[which], epi="resid", not_ran=(other,)):
        for i in range(4):
            lo, to = oc.forward(fc.one(tok), 17 + i)
            lg, tg = gc.Forward(fc.one(tok), 17 + i)
            assert fc.same(lg, lo) and tg == to, (form, i)
            tok = to
    assert count(lnb, form, "resid") == 4 * 2 * cfg["n_layers"]          # wo and w2 of every layer and step
    fc.kv_equal(gc, [(oc.cache(l, 0), oc.cache(l, 1)) for l in range(cfg["n_layers"])], 21, (form,))
    gc.close(); oc.close(); om.close()


def test_row_broadcast_gemv_fed_through_the_lds_by_default(lnb):
    rowcast_cases(lnb, "lds")


ROWCAST_CHILD = CHILD_HEAD + r"""
import test_gpu_forms as t
t.rowcast_cases(lnb, "self")
print("rowcast child ok")
"""


def test_row_broadcast_gemv_self_feeding_where_the_lds_form_is_the_default(lnb):
    """LNB_ROWCAST_LDS=0 (ONCE): the same cases on rowcast_kernel, which otherwise runs only at K that are no multiples of 512"""
    run_child(ROWCAST_CHILD, {"LNB_ROWCAST_LDS": "0"}, "rowcast child ok")


# ---- 6. the throughput schedule's gate|up kernels ---------------------------------------------------------------------------------------------------------
TP_CHILD = CHILD_HEAD + r"""
from oracle import oracle as orc
TP_FORMS = {"1": "gemv_chain.rw56_tp", "0": "gemv_chain.rw56"}
TP = os.environ["LNB_TP_W13"]
FORM, OTHER = TP_FORMS[TP], TP_FORMS[str(1 - int(TP))]
cfg, P, N = fc.GEOS["tiny520"], 12, 12                       # FFN hidden 896 = 16 blocks of 56 rows (LNB_RW_W13=56, read when the model is created)
om, gm = orc.Model(**cfg).fill_synthetic(fc.SEED).finalize(), fc.gpu_model(lnb, "tiny520")
prompt = orc.synth_tokens(5, P, cfg["vocab_size"])
ref, _ = orc.Context(om, P + N + 4).generate(prompt, N + 1)
gc = lnb.InferenceContext(gm, P + N + 4).set_schedule("throughput")
with ran(lnb, TP_FORMS[TP], epi="silu_mul", not_ran=(OTHER, "gemv_chain_pk")):
    _, first = gc.Forward(prompt, 0, want_logits=False)
    got, _ = gc.decode_greedy(first, P, N)
assert [first] + [int(t) for t in got] == [int(t) for t in ref]
oc = orc.Context(om, P + N + 4)
oc.forward(prompt, 0, want_logits=False)
tok = int(ref[0])
for i in range(N):                                           # the oracle's cache behind the same tokens, then one eager step: its logits bits
    _, tok = oc.forward(fc.one(tok), P + i, want_logits=False)
lo, _ = oc.forward(fc.one(int(got[-1])), P + N)
with ran(lnb, TP_FORMS[TP], epi="silu_mul", not_ran=(OTHER, "gemv_chain_pk")):
    lg, _ = gc.Forward(fc.one(int(got[-1])), P + N)
assert fc.same(lg, lo)
fc.kv_equal(gc, [(oc.cache(l, 0), oc.cache(l, 1)) for l in range(cfg["n_layers"])], P + N + 1, (FORM,))
print("tp child ok", FORM)
"""


@pytest.mark.parametrize("tp", ["1", "0"])
def test_throughput_schedule_gate_up_kernel_with_six_and_with_eight_ring_stages(lnb, tp):
    """the throughput schedule runs the 56-row gate|up blocks on a six-stage ring (two of its waves beside two of another context's wq|wk|wv waves on a SIMD);
    LNB_TP_W13=0 (ONCE) keeps the eight-stage kernel of the latency schedule: tokens, logits and KV bits against the oracle either way"""
    run_child(TP_CHILD, {"LNB_TP_W13": tp, "LNB_RW_W13": "56"}, "tp child ok gemv_chain.rw56" + ("_tp" if tp == "1" else ""))


# ---- 7. the layouts LNB_RW_WO / LNB_RW_OUT pick -------------------------------------------------------------------------------------------------------------
RW_KNOBS = {"LNB_RW_WO": ("16", "64"), "LNB_RW_OUT": ("16", "32")}
RW_FORMS = {("LNB_RW_WO", "16"): {"gemv_chain.rw16": "resid"}, ("LNB_RW_WO", "64"): {"gemv_chain.rw64": "resid"},
            ("LNB_RW_OUT", "16"): {"gemv_chain.rw16": "store"}, ("LNB_RW_OUT", "32"): {"gemv_chain.rw32": "store"}}


@pytest.mark.parametrize("knob,rw", [(k, v) for k in sorted(RW_KNOBS) for v in RW_KNOBS[k]])
def test_resident_layouts_of_wo_and_the_head_picked_by_knob(lnb, monkeypatch, knob, rw):
    """LNB_RW_WO / LNB_RW_OUT (LIVE, read when the model is created): wo on 16- / 64-row chain blocks instead of the row-broadcast layout, the head on 16- / 32-row
    blocks -- 17-row prefill (gemm_stream_kernel reads that layout) and four one-token steps against the oracle"""
    monkeypatch.setenv(knob, rw)
    gm = lnb.LlamaTransformer(device=0, **fc.GEOS["tiny520"]).fill_synthetic(fc.SEED).finalize()
    monkeypatch.delenv(knob)
    R = fc.reference("tiny520")
    wo = knob == "LNB_RW_WO"
    with ran(lnb, {"gemm_stream.chain.ntw1": ("resid", "store") if wo else "store"}, not_ran=("gemm_mfma",)):
        gc = fc.check_prefill(lnb, gm, R, 17, (knob, rw))
    # wo on a chain layout: only w2 is left on the row-broadcast one; the head's layout changes nothing there
    assert count(lnb, "gemm_stream.rowcast", "resid") == (1 if wo else 2) * fc.GEOS["tiny520"]["n_layers"]
    tok, pos = R["prefill"][17][1], 17
    om = orc.Model(**fc.GEOS["tiny520"]).fill_synthetic(fc.SEED).finalize()
    oc = orc.Context(om, 32)
    oc.forward(R["toks"][:17], 0, want_logits=False)
    with ran(lnb, RW_FORMS[(knob, rw)]):
        for i in range(4):
            lo, to = oc.forward(fc.one(tok), pos + i)
            lg, tg = gc.Forward(fc.one(tok), pos + i)
            assert fc.same(lg, lo) and tg == to, (knob, rw, i)
            tok = to
    (form, epi), = RW_FORMS[(knob, rw)].items()
    # wo: one launch per layer and step; the head: one per step (at 16 rows per block the gate|up and wq|wk|wv blocks are gemv_chain_kernel<16> too, other epilogues)
    assert count(lnb, form, epi) == 4 * (fc.GEOS["tiny520"]["n_layers"] if wo else 1)
    fc.kv_equal(gc, [(oc.cache(l, 0), oc.cache(l, 1)) for l in range(fc.GEOS["tiny520"]["n_layers"])], 21, (knob, rw))
    gc.close(); gm.close(); oc.close(); om.close()


OP_FORMS = {"16": "gemv_chain.rw16", "32": "gemv_chain.rw32", "64": "gemv_chain.rw64", "4": "rowcast"}


@pytest.mark.parametrize("rw", sorted(OP_FORMS))
def test_layout_of_a_stand_alone_operand_picked_by_knob(lnb, monkeypatch, rw):
    """LNB_RW_OP (LIVE): the layout lnb_op_linear gives an operand whose caller leaves it open (rw = 0) -- three rows, ragged N, K = 896 (no multiple of 512: the
    row-broadcast layout runs the self-feeding kernel)"""
    monkeypatch.setenv("LNB_RW_OP", rw)
    with ran(lnb, OP_FORMS[rw], epi="store", not_ran=tuple(f for f in OP_FORMS.values() if f != OP_FORMS[rw]) + ("rowcast_lds", "gemv_quad")):
        rng = np.random.default_rng(int(rw))
        x, w = bf(rng.standard_normal((3, 896))), bf(rng.standard_normal((100, 896)) * 0.05)
        assert (lnb.op_linear(x, w, rw=0) == orc_linear(x, w)).all()


def test_gate_up_on_the_half_height_blocks(lnb, monkeypatch):
    """LNB_RW_W13=28 (LIVE, read when the model is created): gemv_chain_kernel<28, 2, ...>, the band order in which rows [0, F/2) are complete after the first
    block of every workgroup -- FFN hidden 896 = 32 blocks of 28; a 7-row Forward (seven launch rows), four one-token steps and the captured greedy loop"""
    monkeypatch.setenv("LNB_RW_W13", "28")
    cfg = fc.GEOS["tiny520"]
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(fc.SEED).finalize()
    monkeypatch.delenv("LNB_RW_W13")
    om = orc.Model(**cfg).fill_synthetic(fc.SEED).finalize()
    toks = orc.synth_tokens(5, 7, cfg["vocab_size"])
    oc, gc = orc.Context(om, 32), lnb.InferenceContext(gm, 32)
    lo, tok = oc.forward(toks, 0)
    with ran(lnb, "gemv_chain.rw28", epi="silu_mul", not_ran=("gemv_chain.rw56", "gemv_chain.rw56_tp", "gemv_chain_pk")):
        lg, tg = gc.Forward(toks, 0)
        assert fc.same(lg, lo) and tg == tok
        for i in range(4):
            lo, to = oc.forward(fc.one(tok), 7 + i)
            lg, tg = gc.Forward(fc.one(tok), 7 + i)
            assert fc.same(lg, lo) and tg == to, i
            tok = to
    assert count(lnb, "gemv_chain.rw28", "silu_mul") == 5 * cfg["n_layers"]
    with ran(lnb, "gemv_chain.rw28", epi="silu_mul"):
        got, _ = gc.decode_greedy(tok, 11, 6)
    for i in range(6):
        _, tok = oc.forward(fc.one(tok), 11 + i, want_logits=False)
        assert int(got[i]) == tok, i
    fc.kv_equal(gc, [(oc.cache(l, 0), oc.cache(l, 1)) for l in range(cfg["n_layers"])], 17, ("rw28",))
    gc.close(); gm.close(); oc.close(); om.close()


# ---- the dense dispatch of the batched short-context attention ----------------------------------------------------------------------------------------------
DENSE_FORMS = {"tile_major": "attn_batch.dense", "head_major": "attn_batch.dense_headmajor", "off": "attn_batch.plain"}
DENSE_KNOBS = {"tile_major": {"LNB_ATTN_BATCH_DENSE": "1", "LNB_ATTN_BATCH_HEADMAJOR": "0"}, "head_major": {"LNB_ATTN_BATCH_DENSE": "1", "LNB_ATTN_BATCH_HEADMAJOR": "1"},
               "off": {"LNB_ATTN_BATCH_DENSE": "0", "LNB_ATTN_BATCH_HEADMAJOR": "0"}}


def test_dense_batch_attention_tile_major_head_major_and_off(lnb, monkeypatch):
    """attn_exact_kernel<128, DENSE> runs only at head_dim 128 with more than 256 (head, sequence) workgroups: 70 sequences x 4 heads of 128 on 2 KV heads (two query
    heads per KV head: attn_gqa_kernel does not apply), prompts of 5 .. 499 positions, six steps, all below the 512 positions from which a batch decodes with the
    long-context kernels.  Tile-major (the default), head-major (LNB_ATTN_BATCH_HEADMAJOR=1: another (head, sequence) per workgroup id) and the one-token kernel
    (LNB_ATTN_BATCH_DENSE=0), all LIVE: every sequence's tokens and KV bits against its own oracle run"""
    cfg = dict(orc.TINY, dim=512, n_heads=4, n_kv_heads=2, vocab_size=520, n_layers=2)
    n, steps = 70, 6
    plens = [5 + (s * 7) % 44 for s in range(n)]
    plens[0], plens[1], plens[2] = 499, 127, 64                # near the longest the short form takes; crossing / at a 64-position PV chunk edge
    cap = max(plens) + steps + 2
    om = orc.Model(**cfg).fill_synthetic(fc.SEED).finalize()
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(fc.SEED).finalize().enable_batch()
    prompts = [orc.synth_tokens(8000 + s, plens[s], cfg["vocab_size"]) for s in range(n)]
    refs, kvs = [], {}
    for s in range(n):
        oc = orc.Context(om, plens[s] + steps + 2)
        refs.append([int(t) for t in oc.generate(prompts[s], steps + 1)[0]])
        if s in (0, 1, 2, 35, 69):                              # (the long ones, one from the middle, the last)
            kvs[s] = [(oc.cache(l, 0)[:plens[s] + steps].copy(), oc.cache(l, 1)[:plens[s] + steps].copy()) for l in range(cfg["n_layers"])]
        oc.close()
    for which in ("tile_major", "head_major", "off"):
        for k, v in DENSE_KNOBS[which].items():
            monkeypatch.setenv(k, v)
        ctxs = [lnb.InferenceContext(gm, cap) for _ in range(n)]
        firsts = [ctxs[s].Forward(prompts[s], 0, want_logits=False)[1] for s in range(n)]
        b = lnb.Batch(ctxs)
        with ran(lnb, DENSE_FORMS[which], not_ran=tuple(f for f in DENSE_FORMS.values() if f != DENSE_FORMS[which]) + ("attn_batch.gqa",)):
            got, _ = b.decode(firsts, plens, steps)
        for s in range(n):
            assert [firsts[s]] + [int(t) for t in got[s]] == refs[s], (which, s)
        for s, kv in kvs.items():
            fc.kv_equal(ctxs[s], kv, plens[s] + steps, (which, s))
        b.close()
        for c in ctxs:
            c.close()
    gm.close(); om.close()


# ---- 8. pipeline stage steps: replayed from the captured graph, or eager ---------------------------------------------------------------------------------------
PIPE_FORMS = {"1": "pipeline.replay", "0": "pipeline.eager"}


@pytest.mark.parametrize("graph", ["1", "0"])
def test_pipeline_stage_steps_replayed_and_eager(lnb, monkeypatch, graph):
    """LNB_PIPELINE_GRAPH (LIVE, read when the pipe is created): two stages on one GPU through the in-process transport, ticked as two processes would, four
    sequences in flight -- every token the oracle's whether a one-token stage step replays its captured graph or launches its kernels one by one"""
    import pipeline
    monkeypatch.setenv("LNB_PIPELINE_GRAPH", graph)
    cfg, cuts = fc.GEOS["tiny520"], (0, 3, 6)
    om = orc.Model(**cfg).fill_synthetic(fc.SEED).finalize()
    world = len(cuts) - 1
    P, n_seq, n_decode = 5, 2 * world, 5
    stages = [lnb.LlamaTransformer(part_begin=a, part_end=b, **cfg).fill_synthetic(fc.SEED).finalize() for a, b in zip(cuts[:-1], cuts[1:])]
    ctxs = [[lnb.InferenceContext(st, P + n_decode + 2) for _ in range(n_seq)] for st in stages]
    pipes = [lnb.Pipeline(stages[r], r, world, loopback_group="forms" + graph) for r in range(world)]
    prompts = [orc.synth_tokens(70 + s, P, cfg["vocab_size"]) for s in range(n_seq)]
    state = [None] * world
    with ran(lnb, PIPE_FORMS[graph], not_ran=(PIPE_FORMS[str(1 - int(graph))],)):
        for t in range((1 + n_decode) * n_seq + 2 * (world - 1)):
            for r in range(world):
                state[r] = pipeline.run_ticks_native(r, world, pipes[r], ctxs[r], prompts, n_decode, t, t + 1, state[r])
        for p_ in pipes:
            p_.sync()
    assert count(lnb, PIPE_FORMS[graph]) == world * n_seq * n_decode          # every one-token step of every stage and sequence
    for s in range(n_seq):
        got = [int(pipes[-1].read_tokens(q, 1)[0]) for q in state[-1]["slots"][s]]
        ref, _ = orc.Context(om, P + n_decode + 2).generate(prompts[s], n_decode + 1)
        assert got == [int(t) for t in ref], (graph, s)
    for p_ in pipes:
        p_.close()
    for cs in ctxs:
        for c in cs:
            c.close()
    for st in stages:
        st.close()
    om.close()
