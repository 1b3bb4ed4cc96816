"""The sets of tests/fast_craft.py on the CPU (no GPU): what tests/test_gpu_fast_crafted.py hands the tolerance-mode kernels, and why a wrong kernel fails there.

(a) every product, norm-front and epilogue set is order-independent: the sufficient condition holds for every output (fast_craft.order_independent), five orders
    of the f32 adds give the same bits as the oracle's chain on a sample of every set, and the steered outputs are the integers they were steered to;
(b) each named defect of a product kernel changes a compared output of the set named for it;
(c) the f32 model of the flash attention stays inside the derived bound on every attention set, geometry and call, and each named defect moves an output of the
    set named for it by at least four times the bound;
(d) no grid leaves out more than one case in eight."""
import numpy as np
import pytest

import fast_craft as fc
import op_craft as oc


def sample(n, count=48):
    return np.unique(np.linspace(0, n - 1, min(n, count)).astype(np.int64))


def check_orders(x, w, tag):
    sub = sample(w.shape[0])
    ev = fc.evaluate_orders(x[:3], w[sub])
    ref = oc.linear_acc(x[:3], w[sub])
    for name, acc in ev.items():
        assert fc.same_f32(acc, ref), tag + (name,)


# ---- (a) products ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [24, 16])
@pytest.mark.parametrize("form,N,rw,K", fc.GEMV_SHAPES)
def test_exact_sum_sets_of_the_gemv_shapes_are_order_independent_and_steered(form, N, rw, K, bits):
    s = fc.exact_sum_set(15, N, K, bits)
    sub = sample(N, 600)
    assert fc.order_independent(s["x"], s["w"][sub]).all()
    check_orders(s["x"], s["w"], (form, N, K, bits))
    y = oc.wide(oc.linear(s["x"], s["w"][sub])).astype(np.float64)
    want = s["t"][None, sub] * s["scale"][:, None] * s["wscale"][None, sub]
    made_for = np.arange(15)[:, None] % fc.N_PAT == sub[None, :] % fc.N_PAT
    assert np.array_equal(y[made_for], want[made_for]) and (np.abs(s["t"]) <= 255).all() and (np.abs(s["t"]) >= 1).all()
    # one product more or less is visible in every steered output: the smallest product is a grid unit, the total at most 255 of them
    assert fc.sum_bound(K, bits) < 2 ** bits


def test_exact_sum_sets_of_the_gemm_shapes_are_order_independent():
    seen = set()
    for rw, K, N, S in fc.gemm_shapes():
        if (K, N, S) in seen:
            continue
        seen.add((K, N, S))
        for bits in (24, 16):
            s = fc.exact_sum_set(S, N, K, bits)
            assert fc.order_independent(s["x"], s["w"]).all(), (K, N, S, bits)
            if S <= 33:
                check_orders(s["x"], s["w"], (K, N, S, bits))


@pytest.mark.parametrize("K", [8, 64, 896, 4224])
def test_address_probes_select_the_hashed_pattern(K):
    w = fc.hash_w(100, K)
    assert (((w >> 7) & 0xFF) >= 64).all() and (((w >> 7) & 0xFF) <= 190).all()
    cols = fc.probe_columns(K)
    want = set(range(min(130, K))) | set(range(max(0, K - 17), K)) | {b - 1 for b in range(64, K, 64)} | set(range(64, K, 64))
    assert want <= set(cols) and len(set(cols)) >= min(K, 130)
    covered = set()
    for call in fc.probe_calls(K, 15):
        covered |= set(call)
        for variant in (0, 1):
            x = fc.probe_x(K, call, variant)
            assert fc.order_independent(x, w).all()
            assert np.array_equal(oc.linear(x, w), fc.probe_expected(w, call, variant)), (K, variant)
    assert covered == set(cols)
    # neighbouring columns and rows carry other patterns: a wrong address reads another value
    assert (w[:, 1:] != w[:, :-1]).mean() > 0.999 and (w[1:] != w[:-1]).mean() > 0.999


@pytest.mark.parametrize("kind", ["equal", "pow2"])
@pytest.mark.parametrize("rw,K", fc.NORM_SHAPES)
def test_norm_front_sets_have_an_exact_sum_of_squares_and_an_exact_sum_behind_it(rw, K, kind):
    s = fc.norm_front_set(15, fc.NORM_N, K, kind)
    sq = oc.wide(s["h"]) ** 2
    chain = np.zeros(15, dtype=np.float32)
    for k in range(K):
        chain = chain + sq[:, k]
    back = np.zeros(15, dtype=np.float32)
    for k in range(K - 1, -1, -1):
        back = back + sq[:, k]
    tree = sq.copy()
    while tree.shape[1] > 1:
        tree = tree[:, 0::2] + tree[:, 1::2]
    exact = (oc.wide(s["h"]).astype(np.float64) ** 2).sum(axis=1)
    assert np.array_equal(chain.astype(np.float64), exact) and np.array_equal(back, chain) and np.array_equal(tree[:, 0], chain)
    xn = oc.wide(s["xn"]).astype(np.float64)
    mant, _ = np.frexp(np.abs(xn))
    assert (mant == mant[:, :1]).all() and (kind != "equal" or (mant == 0.5).all())                # one significand per row; +-2^j behind the equal-magnitude rows
    assert fc.order_independent(s["xn"], s["w"]).all()
    check_orders(s["xn"], s["w"], (K, kind))


# ---- (a) epilogue sets -------------------------------------------------------------------------------------------------------------------------------------------------
def rows_have_one_magnitude(h):
    a = oc.wide(h)
    ok = ~np.isnan(a).any(axis=1)
    return (np.abs(a[ok]) == np.abs(a[ok][:, :1])).all()


@pytest.mark.parametrize("geo,rows,variant", fc.GATE_UP_SETS)
def test_gate_up_sets_are_order_independent(geo, rows, variant):
    c = fc.gate_up_case(geo, rows, variant)
    r = oc.gate_up_ref(c)
    assert rows_have_one_magnitude(c["h"])
    for w in (c["w1"], c["w3"]):
        assert fc.order_independent(r["xn"], w).all()
    assert oc.nan_fraction(r["out"]) <= oc.MAX_NAN_FRACTION
    n_sel = c["w1"].shape[0] - oc.N_GAUSS_ROWS
    check_orders(r["xn"], c["w1"][n_sel:], (geo, rows, variant))
    fin = ~oc.is_nan(r["out"])
    assert len(np.unique(r["out"][fin])) > 200


@pytest.mark.parametrize("geo,rows", fc.DOWN_SETS)
def test_down_sets_are_order_independent(geo, rows):
    c = fc.down_case(geo, rows)
    r = oc.down_ref(c)
    assert fc.order_independent(c["act"], c["w2"]).all()
    assert oc.nan_fraction(r["out"]) <= oc.MAX_NAN_FRACTION
    ok = ~oc.is_nan(c["act"]).any(axis=1)
    check_orders(c["act"][ok], c["w2"][-32:], (geo, rows))


@pytest.mark.parametrize("key", fc.ATTN_PART_SETS, ids=lambda k: "-".join(str(x) for x in k))
def test_attention_part_sets_are_order_independent(key):
    c = fc.attn_case(*key)
    r = oc.kv_ref(c)
    assert rows_have_one_magnitude(c["h"])
    for w in (c["wk"], c["wv"]):
        assert fc.order_independent(r["xn"], w).all()
    assert oc.nan_fraction(r["xk_rope"]) <= oc.MAX_NAN_FRACTION and oc.nan_fraction(r["xv"]) <= oc.MAX_NAN_FRACTION
    if oc.wo_selects(key[2], key[3], key[4]):
        s = oc.shape_of(key[0])
        att = np.repeat(r["xv"].reshape(1, s["KVH"], s["hd"]), s["H"] // s["KVH"], axis=1).reshape(1, -1)          # p = 1.0: the V row of each head's KV head
        assert fc.order_independent(att, c["wo"]).all()


# ---- (b) the product defects ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_dropped_or_duplicated_unit_in_the_tail_changes_every_steered_output_it_touches():
    for bits in (24, 16):
        s = fc.exact_sum_set(15, 100, 2056, bits)
        ref = oc.linear(s["x"], s["w"])
        xf, wf = oc.wide(s["x"]).astype(np.float64), oc.wide(s["w"]).astype(np.float64)
        full = xf @ wf.T
        tail = xf[:, -8:] @ wf[:, -8:].T
        assert np.array_equal(oc.bf(full.astype(np.float32)), ref)
        made_for = np.arange(15)[:, None] % fc.N_PAT == np.arange(100)[None, :] % fc.N_PAT
        for sign in (-1.0, 1.0):
            bad = oc.bf((full + sign * tail).astype(np.float32))
            touched = made_for & (tail != 0)
            assert touched.sum() > 100 and (bad[touched] != ref[touched]).all(), (bits, sign)


def layout_b_permutation(K):
    """position of k in the row-broadcast layout's order inside each chunk of 128: k = 128 c + 16 e + j is unit j, slot e"""
    k = np.arange(K)
    return (k // 128) * 128 + (k % 16) * 8 + (k % 128) // 16


def test_the_layout_b_permutation_on_x_alone_changes_the_outputs():
    K = 1024
    perm = layout_b_permutation(K)
    assert sorted(perm) == list(range(K))
    w = fc.hash_w(18, K)
    call = fc.probe_calls(K, 15)[2]
    x = fc.probe_x(K, call, 0)
    moved = [m for m, k in enumerate(call) if perm[k] != k]
    assert len(moved) >= 10
    assert (oc.linear(x[:, perm], w)[moved] != oc.linear(x, w)[moved]).mean() > 0.99
    s = fc.exact_sum_set(15, 18, K, 24)
    assert (oc.linear(s["x"][:, perm], s["w"]) != oc.linear(s["x"], s["w"])).mean() > 0.9


def test_swapped_gate_and_up_chains_change_the_gate_up_set():
    for key in (("tiny", 1, "exact"), ("tiny", 17, "split")):
        c = fc.gate_up_case(*key)
        r = oc.gate_up_ref(c)
        g, u = oc.linear_acc(r["xn"], c["w1"]), oc.linear_acc(r["xn"], c["w3"])
        assert np.array_equal(oc.same_or_both_nan(oc.silu_mul_np(g, u), r["out"]).all(), True)
        bad = oc.silu_mul_np(g, u, "swapped")
        assert (~oc.same_or_both_nan(bad, r["out"])).mean() > 0.5, key


def test_a_stored_clamped_row_lands_in_the_next_row():
    """rows of w past n_rows are clamped to the last one, computed and dropped; stored, element (m, n >= N) is element (m + 1, n - N) of the output"""
    N, K = 100, 64
    s = fc.exact_sum_set(15, N, K, 24)
    ref = oc.linear(s["x"], s["w"])
    flat = ref.copy().ravel()
    for m in range(14):
        for n in range(N, 112):                              # (the 16-row block of fast_gemv_a; the 32-row tile of the GEMM reaches 128)
            flat[m * N + n] = ref[m, N - 1]
    assert (flat.reshape(15, N) != ref).sum() >= 14 * 10


def test_a_rope_partner_from_the_wrong_lane_changes_the_rope_set():
    for key in (("tiny", 128, 15, 15, "finite"), ("tiny", 128, 17, 17, "finite")):
        c = fc.attn_case(*key)
        r = oc.kv_ref(c)
        s = oc.shape_of(key[0])
        cis = oc.cis_table(key[0])[key[2]:key[2] + key[3]]
        assert np.array_equal(oc.rope_np(r["xk"], s["KVH"], s["hd"], cis), r["xk_rope"])
        bad = oc.rope_np(r["xk"], s["KVH"], s["hd"], cis, "partner_xor2")
        assert (bad != r["xk_rope"]).mean() > 0.5


# ---- (c) attention ---------------------------------------------------------------------------------------------------------------------------------------------------------
def ratio(c, defect=None):
    ref, A = fc.softmax_f64(c)
    got = oc.wide(fc.flash_model(c, defect)).astype(np.float64)
    with np.errstate(all="ignore"):
        r = np.abs(got - ref) / fc.bound(ref, A)
    return float(np.where(np.isnan(r), np.inf, r).max())


@pytest.mark.parametrize("geometry", sorted(fc.GEOMETRIES))
@pytest.mark.parametrize("name", fc.SETS)
def test_the_kernel_model_stays_inside_the_bound(name, geometry):
    worst = 0.0
    for S, pos in fc.CALLS:
        c = fc.attention_set(name, geometry, S, pos)
        assert not oc.is_nan(c["q"]).any() and c["k"].shape == c["v"].shape == (pos + S, fc.GEOMETRIES[geometry][2], fc.GEOMETRIES[geometry][0])
        worst = max(worst, ratio(c))
    print("%s %s: the model's largest |got - ref| / bound = %.3f" % (name, geometry, worst))
    assert worst <= 1.0


NAMED = {"mask_plus_one": "rising", "mask_minus_one": "rising", "tile_dropped": "rising", "alpha_one": "rising", "v_positions_exchanged": "spike", "kvh_modulo": "per_head"}
DEFECT_CALLS = [(16, 0), (33, 33), (129, 0), (160, 160), (300, 0), (40, 24)]


@pytest.mark.parametrize("defect", fc.DEFECTS)
def test_each_attention_defect_moves_its_set_by_four_times_the_bound(defect):
    assert set(NAMED) == set(fc.DEFECTS)
    for geometry in sorted(fc.GEOMETRIES):
        seen = []
        for S, pos in DEFECT_CALLS:
            c = fc.attention_set(NAMED[defect], geometry, S, pos)
            if fc.defect_applies(defect, c):
                seen.append(ratio(c, defect))
        if defect == "kvh_modulo" and not seen:
            continue                                         # (one KV head, or one query head per KV head: h % KVH is h / rep there)
        assert seen and max(seen) >= 4.0, (defect, geometry, seen)
    assert defect != "kvh_modulo" or any(fc.defect_applies(defect, fc.attention_set("per_head", g, 16, 0)) for g in fc.GEOMETRIES)


def test_the_attention_sets_are_what_they_are_called():
    for geometry in sorted(fc.GEOMETRIES):
        hd = fc.GEOMETRIES[geometry][0]
        for S, pos in ((33, 33), (129, 0)):
            c = fc.attention_set("rising", geometry, S, pos)
            s, visible, _ = fc.scores(c)
            i, j = np.arange(S)[:, None], np.arange(pos + S)[None, :]
            assert np.array_equal(s[0], fc.C0[hd] * (j - i)) and 0.9 < fc.C0[hd] / fc.divisor(hd) <= 1.0
            first_masked = np.where(~visible, s[0], -np.inf).max(axis=1)[:-1]
            assert (first_masked > np.where(visible, s[0], -np.inf).max(axis=1)[:-1]).all()          # the first masked position outweighs every visible one
            c = fc.attention_set("falling", geometry, S, pos)
            assert (np.diff(fc.scores(c)[0], axis=2) < 0).all()
            c = fc.attention_set("spike", geometry, S, pos)
            s = fc.scores(c)[0]
            assert ((s > 0).sum(axis=2) <= 1).all() and (s.max() / fc.divisor(hd) > 19.9) and len({int(a) % 16 for a in s[0].argmax(axis=1)[(s[0] > 0).any(axis=1)]}) == 16
            c = fc.attention_set("uniform", geometry, S, pos)
            assert not c["k"].any() and (oc.wide(c["v"]).sum(axis=2) == 1).all()
            c = fc.attention_set("per_head", geometry, S, pos)
            s = fc.scores(c)[0]
            assert len({float(s[h, 0, 1]) for h in range(c["H"])}) == min(c["H"], 4)
            assert c["KVH"] == 1 or not np.array_equal(c["k"][:, 0], c["k"][:, 1])
        v = fc.attention_set("rising", geometry, 129, 0)["v"]
        assert (v[1:] != v[:-1]).mean() > 0.99 and (v[:, :, 1:] != v[:, :, :-1]).mean() > 0.99


# ---- (d) the grids ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_no_grid_leaves_out_more_than_one_case_in_eight():
    full = sum(len(fc.GEMM_KS[rw]) for rw in fc.GEMM_RWS) * len(fc.GEMM_NS)
    assert len(fc.gemm_shapes()) * 8 >= full * 7
    assert {S for _, _, _, S in fc.gemm_shapes()} >= {16, 33, 128, 129, 300} and {N for _, _, N, _ in fc.gemm_shapes()} >= {32, 100, 256, 260}
    assert {K for rw, K, _, _ in fc.gemm_shapes() if rw != 4} == {64, 128, 192, 448, 4096}
    assert set(fc.ROWS) == {16, 17, 31, 32, 33, 127, 128, 129, 160, 300} and len(fc.CALLS) == 21 and (40, 24) in fc.CALLS
    assert {S for S, _ in fc.ANCHOR_CALLS} == {1, 15, 16, 40} and all((p + S) % S == 0 for S, p in fc.ANCHOR_CALLS)
    assert set(fc.GEOMETRIES.values()) == {(64, 4, 2), (128, 2, 1), (128, 8, 2), (64, 4, 4)}
    assert {f for f, _, _, _ in fc.GEMV_SHAPES} == {"fast_gemv_a.rg8", "fast_gemv_a.rg16", "fast_gemv_a.rg32", "fast_gemv_a.rg64", "fast_gemv_b"}
