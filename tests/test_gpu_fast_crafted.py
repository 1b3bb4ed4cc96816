"""Every kernel form of the tolerance mode (LNB_MODE_FAST, csrc/lnb_fast.hip) on the sets of tests/fast_craft.py (-m gpu).  The mode only changes the order of
f32 adds, so on operands for which every order gives the same f32 its products owe the oracle's 16 bits -- tests/test_fast_crafted_cpu.py proves that the sets are
such operands and that a wrong address, a dropped unit, swapped chains or a wrong RoPE partner would change them.  The flash attention differs from the reference
at documented rounding points and is held to the bound derived from them (fast_craft.bound).  Every comparison sits inside a `ran` block (tests/form_tally.py).

  products     lnb.op_linear_mode(..., MODE_FAST): address probes and exact sums (2^24 and 2^16 grid units) through fast_gemv_a.rg8 / rg16 / rg32 / rg64, fast_gemv_b and
               fast_gemm.a / fast_gemm.b; the grid-cap loop, the forced rows per unit and LNB_FAST_GEMM_2WG=0 (ONCE knobs) in child processes, one after another
  fused norm   the norm-front sets through fast_gemv_a's stage_x
  epilogues    the single-part stages of tests/test_gpu_op_crafted.py on a context in fast mode
  attention    lnb_ctx_attention: anchored in exact mode on tests/test_attention_crafted_cpu.py's restate(), then fast_attn.hd64 / hd128 on every set, geometry and call

The anchor's contexts hold a FINITE pattern beyond T: a NaN row loaded into a context raises its sticky word and an exact multi-row call then recomputes every row
the reference's way -- the matrix-core kernel would not be what the comparison sees.  The fast calls run over NaN rows beyond T."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_craft as fc
import kv_craft as kc
import op_craft as oc
from form_tally import count, ran
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
os.environ.setdefault("LNB_FAST_GEMM_MIN_ROWS", "16")     # (the library keeps the exact GEMM below 192 rows by default: exercise the bf16 one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")
EXACT_PRODUCTS = ("gemm_mfma", "gemm_stream", "gemm_blgp", "rowcast", "rowcast_lds", "gemv_quad", "gemv_chain", "gemv_chain_pk")
GEMV_FORMS = ("fast_gemv_a.rg8", "fast_gemv_a.rg16", "fast_gemv_a.rg32", "fast_gemv_a.rg64", "fast_gemv_b")
GEMM_FORMS = {False: "fast_gemm.a.mt4_wb2", True: "fast_gemm.b.mt4_wb2"}
GEMM_ONE_WG = {(False, False): "fast_gemm.a.mt4_wb3", (False, True): "fast_gemm.a.mt8_wb3", (True, False): "fast_gemm.b.mt4_wb3", (True, True): "fast_gemm.b.mt8_wb3"}
ATTN_FORMS = {64: "fast_attn.hd64", 128: "fast_attn.hd128"}


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


def guarded(lnb, fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except lnb.LnbError as e:                                # a device fault ends the session: nothing more is started on that GPU
        if "illegal memory access" in str(e) or "launch failure" in str(e):
            pytest.exit("the device faulted: %s" % e, returncode=3)
        raise


TALLY = {}                                                   # what the run saw, printed per test: {label: [elements, differing]}


def compare(got, ref, label, tag):
    ok = oc.same_or_both_nan(got, ref)
    t = TALLY.setdefault(label, [0, 0])
    t[0] += ok.size; t[1] += int((~ok).sum())
    bad = np.argwhere(~ok)
    assert bad.size == 0, "%s %s: %d of %d differ; first (row, col): %s got %s oracle %s" % (
        label, tag, len(bad), ok.size, bad[:6].tolist(), [hex(int(got[tuple(i)])) for i in bad[:6]], [hex(int(ref[tuple(i)])) for i in bad[:6]])


def report(label):
    t = TALLY.get(label, [0, 0])
    print("FASTCRAFT %s: %d of %d elements differ" % (label, t[1], t[0]))


def product_sets(lnb, N, K, rows, rw, label, full):
    """address probes (both variants) and exact sums (both bounds) of one shape through op_linear_mode in fast mode against the oracle's bits"""
    w = fc.hash_w(N, K)
    for call in fc.probe_calls(K, rows, None if full else 3):
        for variant in (0, 1):
            x = fc.probe_x(K, call, variant)
            compare(guarded(lnb, lnb.op_linear_mode, x, w, lnb.MODE_FAST, rw=rw), oc.linear(x, w), label, ("probe", variant, N, K, rows, rw, call[0]))
    for bits in (24, 16):
        s = fc.exact_sum_set(rows, N, K, bits)
        compare(guarded(lnb, lnb.op_linear_mode, s["x"], s["w"], lnb.MODE_FAST, rw=rw), oc.linear(s["x"], s["w"]), label + (" (2^%d)" % bits if label.startswith("fast_gemm") else ""),
                ("sum", bits, N, K, rows, rw))


# ---- the split-K GEMV ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,N,rw,K", fc.GEMV_SHAPES)
def test_split_k_gemv_gives_the_oracles_bits(lnb, form, N, rw, K):
    assert form in GEMV_FORMS
    for rows in fc.GEMV_ROWS:
        with ran(lnb, GEMV_FORMS[GEMV_FORMS.index(form)], epi="store", not_ran=tuple(f for f in GEMV_FORMS if f != form) + ("fast_gemm",) + EXACT_PRODUCTS):
            product_sets(lnb, N, K, rows, rw, form, rows == 15 and N * K <= 1 << 22)
    report(form)


# ---- the bf16 GEMM ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rw,K", [(rw, K) for rw in fc.GEMM_RWS for K in fc.GEMM_KS[rw]])
def test_bf16_gemm_gives_the_oracles_bits(lnb, rw, K):
    form = GEMM_FORMS[rw == 4]
    for _, _, N, S in [s for s in fc.gemm_shapes() if s[0] == rw and s[1] == K]:
        with ran(lnb, GEMM_FORMS[rw == 4], epi="store", not_ran=tuple(f for f in list(GEMM_FORMS.values()) + list(GEMM_ONE_WG.values()) if f != form) + ("fast_gemv_a", "fast_gemv_b") + EXACT_PRODUCTS):
            product_sets(lnb, N, K, S, rw, form, S >= 128)
    report(form); report(form + " (2^24)"); report(form + " (2^16)")


def test_bf16_gemm_leaves_k_40_to_the_exact_kernel(lnb):
    s = fc.exact_sum_set(20, 17, 40, 24)
    with ran(lnb, (), not_ran=("fast_gemm", "fast_gemv_a", "fast_gemv_b")):
        y = guarded(lnb, lnb.op_linear_mode, s["x"], s["w"], lnb.MODE_FAST, rw=64)
        assert sum(count(lnb, f) for f in ("gemm_mfma", "gemm_stream")) == 1
    compare(y, oc.linear(s["x"], s["w"]), "exact fall-back", (20, 17, 40))


# ---- the fused norm -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["equal", "pow2"])
@pytest.mark.parametrize("rw,K", fc.NORM_SHAPES)
def test_fused_norm_of_the_split_k_gemv_gives_the_oracles_bits(lnb, rw, K, kind):
    for rows in (1, 15):
        s = fc.norm_front_set(rows, fc.NORM_N, K, kind)
        with ran(lnb, "fast_gemv_a", epi="store", not_ran=("fast_gemv_b", "fast_gemm") + EXACT_PRODUCTS):
            y = guarded(lnb, lnb.op_linear_mode, s["h"], s["w"], lnb.MODE_FAST, norm_w_u16=s["nw"], eps=float(oc.EPS), rw=rw)
            compare(y, oc.linear(s["xn"], s["w"]), "fused norm", (rw, K, kind, rows))
    report("fused norm")


# ---- ONCE knobs: a child process each, one after another ----------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
import lnb
import test_gpu_fast_crafted as t
from form_tally import ran
case = os.environ["LNB_TEST_FAST_CRAFTED_CASE"]
CAP_FORMS = {"cap3_rg8": "fast_gemv_a.rg8", "cap3_rg64": "fast_gemv_a.rg64"}
if case in CAP_FORMS:                                            # LNB_FAST_GRID_CAP=3 with LNB_FAST_RG=8 / 64: 32 and 4 work units of 64-row blocks on three workgroups
    for K in (64, 2056):
        for rows in (1, 2, 15):
            with ran(lnb, CAP_FORMS[case], epi="store", not_ran=tuple(f for f in t.GEMV_FORMS if f != CAP_FORMS[case])):
                t.product_sets(lnb, 200, K, rows, 64, CAP_FORMS[case] + " grid cap", rows == 15)
    t.report(CAP_FORMS[case] + " grid cap")
TWO_WG_FORMS = {(False, False): "fast_gemm.a.mt4_wb3", (False, True): "fast_gemm.a.mt8_wb3", (True, False): "fast_gemm.b.mt4_wb3", (True, True): "fast_gemm.b.mt8_wb3"}
if case == "2wg0":                                         # LNB_FAST_GEMM_2WG=0: one workgroup per CU, 128 batch rows up to 128 rows and 256 above
    for rw, Ks in ((32, (128, 448)), (4, (128, 384))):
        for K in Ks:
            for N, S in zip((100, 260, 100), t.fc.GEMM_2WG0_ROWS):
                form = TWO_WG_FORMS[(rw == 4, S > 128)]
                assert TWO_WG_FORMS == t.GEMM_ONE_WG
                with ran(lnb, TWO_WG_FORMS[(rw == 4, S > 128)], epi="store", not_ran=tuple(f for f in list(t.GEMM_FORMS.values()) + list(t.GEMM_ONE_WG.values()) if f != form)):
                    t.product_sets(lnb, N, K, S, rw, form, True)
    for form in sorted(set(TWO_WG_FORMS.values())):
        t.report(form); t.report(form + " (2^24)"); t.report(form + " (2^16)")
print("fast crafted child ok", case)
"""
CHILD_ENV = {"cap3_rg8": {"LNB_FAST_GRID_CAP": "3", "LNB_FAST_RG": "8"}, "cap3_rg64": {"LNB_FAST_GRID_CAP": "3", "LNB_FAST_RG": "64"}, "2wg0": {"LNB_FAST_GEMM_2WG": "0"}}


@pytest.mark.parametrize("case", sorted(CHILD_ENV))
def test_once_knob_forms_in_a_child_process(lnb, case):
    code = CHILD % dict(root=ROOT, pkg=PKG, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, LNB_TEST_FAST_CRAFTED_CASE=case, **CHILD_ENV[case]))
    print("".join(line + "\n" for line in r.stdout.splitlines() if line.startswith("FASTCRAFT")))
    assert r.returncode == 0 and "fast crafted child ok " + case in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the epilogues, through single-part stages in fast mode ----------------------------------------------------------------------------------------------------------
def part():
    import test_gpu_op_crafted as t                          # part_model, poke, peek, call, kv_blob: unchanged, shared
    return t


_GM = {}


@pytest.fixture(scope="module", autouse=True)
def models():
    yield
    for gm in _GM.values():
        gm.close()
    _GM.clear()


def shared(key, make):
    if key not in _GM:
        _GM[key] = make()
    return _GM[key]


def fast_ctx(lnb, gm, cap):
    return lnb.InferenceContext(gm, cap).set_mode("fast")


@pytest.mark.parametrize("geo,rows", fc.DOWN_SETS)
def test_residual_epilogue_of_the_down_part_in_fast_mode(lnb, geo, rows):
    t = part()
    c = fc.down_case(geo, rows); r = oc.down_ref(c)
    gm = shared(("down", geo), lambda: t.part_model(lnb, geo, 2, {"feed_forward.w2": fc.down_case(geo, 1)["w2"]}))
    with ran(lnb, "fast_gemm.b.mt4_wb2" if rows >= 16 else "fast_gemv_b", epi="resid", not_ran=EXACT_PRODUCTS):
        ctx = fast_ctx(lnb, gm, max(rows, 16))
        t.poke(lnb, ctx, 0, c["h"]); t.poke(lnb, ctx, 2, c["act"])
        t.call(lnb, ctx, rows)
        out = t.peek(lnb, ctx, 1, c["h"].shape)               # the part adds in place: out aliases res
        ctx.close()
        compare(out, r["out"], "down part (resid)", (geo, rows))
    report("down part (resid)")


@pytest.mark.parametrize("geo,rows,variant", fc.GATE_UP_SETS)
def test_silu_mul_epilogue_of_the_gate_up_part_in_fast_mode(lnb, geo, rows, variant):
    t = part()
    c = fc.gate_up_case(geo, rows, variant); r = oc.gate_up_ref(c)
    gm = shared(("gate_up", geo, variant), lambda: t.part_model(lnb, geo, 1, {"ffn_norm": c["nw"], "feed_forward.w1": c["w1"], "feed_forward.w3": c["w3"]}))
    F = gm.ffn_hidden
    with ran(lnb, "fast_gemm.a.mt4_wb2" if rows >= 16 else "fast_gemv_a", epi="silu_mul", not_ran=EXACT_PRODUCTS):
        ctx = fast_ctx(lnb, gm, max(rows, 16))
        t.poke(lnb, ctx, 0, c["h"]); t.poke(lnb, ctx, 2, np.full((rows, F), oc.QNAN, dtype=np.uint16))
        t.call(lnb, ctx, rows)
        out, h = t.peek(lnb, ctx, 2, (rows, F)), t.peek(lnb, ctx, 1, c["h"].shape)
        ctx.close()
        compare(out, r["out"], "gate/up part (silu_mul)", (geo, rows, variant))
        assert (h == c["h"]).all(), ("h must come through the gate/up part unchanged", geo, rows, variant)
    report("gate/up part (silu_mul)")


@pytest.mark.parametrize("key", fc.ATTN_PART_SETS, ids=lambda k: "-".join(str(x) for x in k))
def test_rope_epilogue_and_kv_append_of_the_attention_part_in_fast_mode(lnb, key):
    t = part()
    c = fc.attn_case(*key); r = oc.kv_ref(c)
    s = oc.shape_of(key[0])
    cap, start, rows = key[1], key[2], key[3]
    gm = t.part_model(lnb, key[0], 0, {"attention_norm": c["nw"], "attention.wq": c["wq"], "attention.wk": c["wk"], "attention.wv": c["wv"], "attention.wo": c["wo"]})
    forms = {"fast_gemm.a.mt4_wb2": "qkv_rope", "fast_gemm.b.mt4_wb2": "resid"} if rows >= 16 else {"fast_gemv_a": "qkv_rope", "fast_gemv_b": "resid"}
    with ran(lnb, forms, not_ran=EXACT_PRODUCTS):
        ctx = fast_ctx(lnb, gm, cap)
        blob, K0, V0 = t.kv_blob(c, s, start)
        assert ctx.LoadPrefix(blob) == cap
        t.poke(lnb, ctx, 0, c["h"])
        t.call(lnb, ctx, rows, start)
        K, V = ctx.CacheK(oc.LAYER), ctx.CacheV(oc.LAYER)
        out = t.peek(lnb, ctx, 1, c["h"].shape)
        ctx.close()
        compare(K[start:start + rows].reshape(rows, -1), r["xk_rope"], "attention part (qkv_rope)", key + ("K",))
        compare(V[start:start + rows].reshape(rows, -1), r["xv"], "attention part (qkv_rope)", key + ("V",))
        for got, was, what in ((K, K0, "K"), (V, V0, "V")):
            assert (got[:start] == was[:start]).all() and (got[start + rows:] == was[start + rows:]).all(), key + (what, "a row outside the call was written")
        if oc.wo_selects(start, rows, key[4]):              # one row at position 0: p = 1.0, the attention output is the V row, wo's selector rows put it against h
            compare(out, oc.attn_oracle(c)[0][("h", 0)], "attention part (wo resid)", key)
    gm.close()
    report("attention part (qkv_rope)")


# ---- attention through lnb_ctx_attention ----------------------------------------------------------------------------------------------------------------------------
FINITE_TAIL = 0x4D4D
TAIL = 64


def attn_model(lnb, geometry):
    hd, H, KVH = fc.GEOMETRIES[geometry]
    cfg = dict(orc.TINY, n_layers=1, dim=H * hd, n_heads=H, n_kv_heads=KVH)
    return shared(("attn", geometry), lambda: lnb.LlamaTransformer(**cfg).fill_synthetic(5).finalize()), cfg


def run_attention(lnb, ctx, c, capacity, tail):
    K, V = fc.cache_rows(c, capacity, tail)
    assert ctx.LoadPrefix(kc.blob([K], [V])) == capacity
    return guarded(lnb, ctx.attention, 0, c["q"], c["start_pos"])


@pytest.mark.parametrize("geometry", sorted(fc.GEOMETRIES))
def test_lnb_ctx_attention_in_exact_mode_is_the_restated_reference_bit_for_bit(lnb, geometry):
    """1 and 15 rows: the one-row and the row-per-workgroup kernel; 16 and 40: the matrix-core kernel (scores once) -- on queries no synthetic model produces"""
    import test_attention_crafted_cpu as ac
    gm, cfg = attn_model(lnb, geometry)
    for name in fc.SETS:
        for S, pos in fc.ANCHOR_CALLS:
            c = fc.attention_set(name, geometry, S, pos)
            ctx = lnb.InferenceContext(gm, c["T"] + 8)
            with ran(lnb, (), not_ran=("fast_attn",)):
                out = run_attention(lnb, ctx, c, c["T"] + 8, FINITE_TAIL)
            assert S < 16 or ctx.prefill_attention_form() == 3
            ctx.close()
            _, want = ac.restate(cfg, c["q"], c["k"], c["v"], pos)
            compare(out.reshape(S, -1), want, "lnb_ctx_attention exact", (name, geometry, S, pos))
    report("lnb_ctx_attention exact")


@pytest.mark.parametrize("geometry", sorted(fc.GEOMETRIES))
@pytest.mark.parametrize("name", fc.SETS)
def test_flash_attention_stays_inside_the_derived_bound(lnb, name, geometry):
    gm, _ = attn_model(lnb, geometry)
    hd = fc.GEOMETRIES[geometry][0]
    cap = max(p + S for S, p in fc.CALLS) + TAIL
    ctx = fast_ctx(lnb, gm, cap)
    worst = 0.0
    for S, pos in fc.CALLS:
        c = fc.attention_set(name, geometry, S, pos)
        with ran(lnb, ATTN_FORMS[hd], not_ran=tuple(f for f in ATTN_FORMS.values() if f != ATTN_FORMS[hd])):
            out = run_attention(lnb, ctx, c, cap, fc.QNAN)
        ref, A = fc.softmax_f64(c)
        got = oc.wide(out).astype(np.float64)
        with np.errstate(all="ignore"):
            r = np.abs(got - ref) / fc.bound(ref, A)
        r = np.where(np.isnan(r), np.inf, r)
        worst = max(worst, float(r.max()))
        assert r.max() <= 1.0, "%s %s S=%d start_pos=%d: |got - ref| / bound = %g at (row, head, dim) %s: got %g, reference %g" % (
            name, geometry, S, pos, r.max(), np.unravel_index(r.argmax(), r.shape), got.ravel()[r.argmax()], ref.ravel()[r.argmax()])
        if (S, pos) in ((33, 33), (129, 0)):                # the NaN rows beyond T change nothing
            with ran(lnb, ATTN_FORMS[hd]):
                again = run_attention(lnb, ctx, c, cap, FINITE_TAIL)
            assert np.array_equal(again, out), (name, geometry, S, pos, "the rows beyond T reached the output")
    ctx.close()
    print("FASTCRAFT attention %s %s: largest |got - ref| / bound = %.3f" % (name, geometry, worst))


@pytest.mark.parametrize("geometry", sorted(fc.GEOMETRIES))
def test_fifteen_rows_in_fast_mode_take_the_exact_kernel(lnb, geometry):
    import test_attention_crafted_cpu as ac
    gm, cfg = attn_model(lnb, geometry)
    for name in fc.SETS:
        for pos in (0, 15):
            c = fc.attention_set(name, geometry, 15, pos)
            ctx = fast_ctx(lnb, gm, c["T"] + TAIL)
            with ran(lnb, (), not_ran=("fast_attn",)):
                out = run_attention(lnb, ctx, c, c["T"] + TAIL, fc.QNAN)
            ctx.close()
            compare(out.reshape(15, -1), ac.restate(cfg, c["q"], c["k"], c["v"], pos)[1], "15 rows in fast mode", (name, geometry, pos))
    report("15 rows in fast mode")


def test_a_forward_refuses_what_the_reference_cannot_broadcast_and_the_flash_kernel_takes_it(lnb):
    """40 rows at start_pos 24: T = 64 is no multiple of 40.  In exact mode lnb_ctx_attention refuses it as a Forward does; the flash kernel's mask is defined there"""
    gm, _ = attn_model(lnb, "hd64_4_2")
    c = fc.attention_set("rising", "hd64_4_2", 40, 24)
    ctx = lnb.InferenceContext(gm, 64)
    with pytest.raises(lnb.LnbError, match="cannot be broadcasted"):
        ctx.attention(0, c["q"], 24)
    ctx.close()
