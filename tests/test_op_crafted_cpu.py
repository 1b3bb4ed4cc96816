"""The crafted-value cases of the RoPE, SiLU * up and residual epilogues on the CPU oracle alone (no GPU): what tests/test_gpu_op_crafted.py compares the device
with, and the proof that the comparison can fail.

(a) the references of tests/op_craft.py -- plain compositions of the oracle's operator functions -- reproduce orc_forward's own dumps (xk, xv, xk_rope, h, ffn_h,
    block_out) bit for bit, on a synthetic model and on one that carries the crafted weights (crafted tok_embeddings rows stand in for the crafted h);
(b) every case set meets its conditions ON THE REFERENCE'S VALUES -- what reaches the epilogue, not what the recipe intends -- and keeps its NaN outputs under 1 / 8;
(c) each plausible wrong epilogue, restated in numpy, changes the bits of a finite output of every case set it can touch.

What no recipe can reach, and why: a product never gives -0 except by the underflow of the truncation (a chain starts at +0 and +0 + (-0) = +0), so y = -0 of the
residual pair is left out ((-0) + (+0) has the -0 on the residual's side) while the gate, the up value and xk get their -0 from -2^-140; a NaN accumulator in a
call of 16 rows or more needs a NaN product, so there the NaNs come in rows of their own and NaN in ONE half of a RoPE pair exists in the 1 .. 15 row sets only;
at position 0 the cis row is (1, 0): RoPE in f32 and a flipped sign of ci compute the same bits there, so the sets that hold position 0 alone do not show those two."""
import numpy as np
import pytest

import op_craft as oc

F32_MIN = np.float64(2.0 ** -126)


def finite(p):
    return (np.asarray(p) & 0x7F80) != 0x7F80


def changed(ref, got):
    """finite outputs of the reference whose bits the wrong epilogue changes"""
    return int((finite(ref) & (ref != got)).sum())


def pin(a, b, what):
    ok = oc.same_or_both_nan(a, np.asarray(b).reshape(np.shape(a)))
    assert ok.all(), "%s: %d of %d differ from the oracle's dump" % (what, int((~ok).sum()), ok.size)


# ---- (a) the compositions are the oracle's forward ---------------------------------------------------------------------------------------------------------------
def _pin_block(geo, h_rows, start_pos, capacity, tensors, prefix, tag):
    s = oc.shape_of(geo)
    d, kv, w = oc.oracle_block(geo, h_rows, start_pos, capacity, tensors, prefix)
    rows = h_rows.shape[0]
    pin(d[("embedding", -1)], h_rows, tag + " embedding")
    c = dict(geo=geo, start_pos=start_pos, h=h_rows, nw=w["attention_norm"], wk=w["attention.wk"].reshape(s["kv_dim"], s["dim"]),
             wv=w["attention.wv"].reshape(s["kv_dim"], s["dim"]))
    r = oc.kv_ref(c)
    pin(r["xk"], d[("xk", 0)], tag + " xk"); pin(r["xv"], d[("xv", 0)], tag + " xv"); pin(r["xk_rope"], d[("xk_rope", 0)], tag + " xk_rope")
    pin(r["xk_rope"], kv[0][start_pos:start_pos + rows].reshape(rows, -1), tag + " K cache rows"); pin(r["xv"], kv[1][start_pos:start_pos + rows].reshape(rows, -1), tag + " V cache rows")
    wo = oc.down_ref(dict(act=d[("attn_pre_wo", 0)], h=h_rows, w2=w["attention.wo"].reshape(s["dim"], s["q_dim"])))
    pin(wo["out"], d[("h", 0)], tag + " h")
    gu = oc.gate_up_ref(dict(h=d[("h", 0)], nw=w["ffn_norm"], w1=w["feed_forward.w1"].reshape(s["F"], s["dim"]), w3=w["feed_forward.w3"].reshape(s["F"], s["dim"])))
    pin(gu["out"], d[("ffn_h", 0)], tag + " ffn_h")
    dn = oc.down_ref(dict(act=d[("ffn_h", 0)], h=d[("h", 0)], w2=w["feed_forward.w2"].reshape(s["dim"], s["F"])))
    pin(dn["out"], d[("block_out", 0)], tag + " block_out")


@pytest.mark.parametrize("geo", ["tiny", "wide1024", "hd32"])
def test_compositions_are_the_forward_on_a_synthetic_model(geo):
    rng = np.random.default_rng(5)
    s = oc.shape_of(geo)
    _pin_block(geo, oc.bf(rng.standard_normal((7, s["dim"]))), 0, 16, None, None, geo + " 7 rows at 0")
    pk, pv = oc.bf(rng.standard_normal((36, s["KVH"], s["hd"])) * 0.5), oc.bf(rng.standard_normal((36, s["KVH"], s["hd"])) * 0.3)
    _pin_block(geo, oc.bf(rng.standard_normal((1, s["dim"]))), 36, 37, None, (pk, pv), geo + " 1 row at 36")


@pytest.mark.parametrize("st", [("tiny", 128, 0, 2, "finite"), ("tiny", 128, 0, 2, "nonfinite"), ("tiny", 128, 16, 16, "finite"), ("tiny", 128, 0, 17, "nonfinite"),
                                ("tiny", 37, 36, 1, "nonfinite"), ("wide1024", 128, 127, 1, "nonfinite"), ("hd32", 128, 17, 17, "finite")], ids=str)
def test_compositions_are_the_forward_on_a_model_with_the_crafted_weights(st):
    geo, rows = st[0], st[3]
    a = oc.attn_case(*st)
    g = oc.gate_up_case(geo, rows, "exact" if rows < 16 else "split")
    dn = oc.down_case("tiny", rows) if geo == "tiny" else None
    tensors = {"attention_norm": a["nw"], "attention.wq": a["wq"], "attention.wk": a["wk"], "attention.wv": a["wv"], "attention.wo": a["wo"],
               "ffn_norm": g["nw"], "feed_forward.w1": g["w1"], "feed_forward.w3": g["w3"]}
    if dn is not None:
        tensors["feed_forward.w2"] = dn["w2"]
    _pin_block(geo, a["h"], a["start_pos"], a["capacity"], tensors, (a["prefix_k"], a["prefix_v"]), str(st))


def test_numpy_restatements_without_a_defect_are_the_references():
    for st in oc.ROPE_SETS:
        c = oc.attn_case(*st); r = oc.kv_ref(c); s = oc.shape_of(st[0])
        cis = oc.cis_table(st[0])[st[2]:st[2] + st[3]]
        pin(oc.rope_np(r["xk"], s["KVH"], s["hd"], cis), r["xk_rope"], "rope_np %s" % (st,))
    for geo, rows in oc.RESID_SETS:
        c = oc.down_case(geo, rows); r = oc.down_ref(c)
        acc = oc.linear_acc(c["act"], c["w2"])
        pin(oc.bf(acc), r["y"], "linear_acc %s %d" % (geo, rows)); pin(oc.add_np(c["h"], acc), r["out"], "add_np %s %d" % (geo, rows))
    for geo, rows, v in oc.GATE_UP_SETS:
        c = oc.gate_up_case(geo, rows, v); r = oc.gate_up_ref(c)
        pin(oc.silu_mul_np(oc.linear_acc(r["xn"], c["w1"]), oc.linear_acc(r["xn"], c["w3"])), r["out"], "silu_mul_np %s %d %s" % (geo, rows, v))


# ---- (b) the conditions, on the reference's values ------------------------------------------------------------------------------------------------------------------
def test_value_set():
    V = oc.V
    assert V.size == 256 and len(set(V.tolist())) == 256
    nan = V[oc.is_nan(V)]
    assert 2 <= nan.size <= 8 and (nan & 0x8000).any() and (~nan & 0x8000).any() and ((nan & 0x40) == 0).any(), "NaNs of both signs, one signalling, at most 8"
    for p in (0x0000, 0x8000, 0x7F80, 0xFF80, 0x0080, 0x8080, 0x7F7F, 0xFF7F, 0x3F80, 0xBF80, 0x3F7F, 0x3F81):
        assert p in V, hex(p)
    assert oc.is_sub(V).sum() >= 4
    pw = V[((V & 0x7F) == 0) & finite(V) & ((V & 0x7F80) != 0)]
    ef = (pw >> 7) & 0xFF
    assert ef.min() <= 8 and ef.max() >= 246 and np.diff(np.unique(ef)).max() <= 8, "powers of two over the whole exponent range"


def resid_conditions(res, y):
    """counts over the pairs (residual, y = trunc(acc)) of a case set"""
    out = oc.add_ref(res, y)
    with np.errstate(all="ignore"):
        r, v = oc.wide(res).astype(np.float64), oc.wide(y).astype(np.float64)
        exact = r + v                                        # exact in f64 while the exponents lie less than ~45 apart; beyond, the side of the large value decides
        s32 = (oc.wide(res) + oc.wide(y))
    fin = np.isfinite(r) & np.isfinite(v)
    er, ey = (res >> 7) & 0xFF, (y >> 7) & 0xFF
    far = fin & (r != 0) & (v != 0) & (np.abs(er.astype(int) - ey.astype(int)) > 16)
    big = np.where(np.abs(r) >= np.abs(v), r, v); small = np.where(np.abs(r) >= np.abs(v), v, r)
    # RN then truncation differs from truncating the exact sum: RN returned the large (bf16) value although the exact sum lies just inside it
    rn_differs = far & (s32.astype(np.float64) == big) & (np.sign(small) != np.sign(big)) & ((big.astype(np.float32).view(np.uint32) & 0xFFFF) == 0)
    return {
        "an exact cancellation to +0": int((fin & (r != 0) & (r == -v) & (out == 0x0000)).sum()),
        "(-0) + (+0)": int(((res == 0x8000) & (y == 0x0000) & (out == 0x0000)).sum()),
        "a finite sum that overflows to inf": int((fin & ((out & 0x7FFF) == 0x7F80)).sum()),
        "inf + (-inf)": int((np.isinf(r) & np.isinf(v) & (r != v) & oc.is_nan(out)).sum()),
        "a subnormal result": int((fin & oc.is_sub(out)).sum()),
        "a negative result whose truncation drops set bits": int((fin & (s32 < 0) & ((s32.view(np.uint32) & 0xFFFF) != 0) & finite(out)).sum()),
        "exponents more than 16 apart where RN + truncation differs from truncating the exact sum": int(rn_differs.sum()),
    }


@pytest.mark.parametrize("geo,rows", oc.RESID_SETS)
def test_residual_sets_meet_their_conditions(geo, rows):
    c = oc.down_case(geo, rows); r = oc.down_ref(c)
    assert oc.nan_fraction(r["out"]) <= oc.MAX_NAN_FRACTION, "NaN outputs %.3f of the set" % oc.nan_fraction(r["out"])
    n_sel = c["h"].shape[1] if rows == 256 else c["h"].shape[1] - 32
    counts = resid_conditions(c["h"][:, :n_sel], r["y"][:, :n_sel])
    print(geo, rows, counts)
    for name, n in counts.items():
        assert n >= (32 if name.startswith("exponents") else 1), "%s %d rows: no pair with %s (%s)" % (geo, rows, name, counts)
    if rows == 256:                                          # the full grid: row m carries y = V[m] (a product cannot give -0: that row carries +0), column n the residual V[n]
        want = np.where(oc.V == 0x8000, 0, oc.V)
        assert oc.same_or_both_nan(r["y"], np.broadcast_to(want[:, None], r["y"].shape)).all() and (c["h"] == oc.V[None, :]).all()
        assert oc.nan_fraction(r["out"]) < 0.063


SILU_ALL = ("+0 gate", "-0 gate", "a subnormal gate", "+inf gate", "-inf gate", "the most negative gate whose SiLU is a normal f32", "a table entry that loses set bits in the truncation",
            "up +0", "up -0", "a subnormal up", "an infinite up", "gs * u subnormal", "gs * u overflows", "0 * inf")
# what a variant cannot hold: "split" sets have finite normal weights only, so a NaN gate or up exists only in a NaN row of h (16 rows and more; one sign);
# "window" sets are what the 13-bit copy admits: 30 binades, no subnormal, no inf, no NaN
SILU_CONDITIONS = {
    "exact": SILU_ALL + ("a NaN gate of each sign", "a NaN up"),
    "split": SILU_ALL,
    "window": ("+0 gate", "a table entry that loses set bits in the truncation", "up +0", "gs * u subnormal"),
}


def silu_conditions(r):
    t = oc.silu_table()
    g, u, gs, out = r["g"], r["u"], r["gs"], r["out"]
    gsf, uf = oc.wide(gs).astype(np.float64), oc.wide(u).astype(np.float64)
    with np.errstate(all="ignore"):
        prod = gsf * uf
    edge = oc.most_negative_normal_gate()
    nan_g = g[oc.is_nan(g)]
    return {
        "+0 gate": int((g == 0).sum()), "-0 gate": int((g == 0x8000).sum()), "a subnormal gate": int(oc.is_sub(g).sum()),
        "+inf gate": int((g == 0x7F80).sum()), "-inf gate": int((g == 0xFF80).sum()),
        "a NaN gate of each sign": int(min((nan_g & 0x8000 != 0).sum(), (nan_g & 0x8000 == 0).sum())),
        "the most negative gate whose SiLU is a normal f32": int((g == edge).sum()),
        "a table entry that loses set bits in the truncation": int(((t[g].view(np.uint32) & 0xFFFF != 0) & np.isfinite(t[g])).sum()),
        "up +0": int((u == 0).sum()), "up -0": int((u == 0x8000).sum()), "a subnormal up": int(oc.is_sub(u).sum()), "an infinite up": int(((u & 0x7FFF) == 0x7F80).sum()),
        "a NaN up": int(oc.is_nan(u).sum()),
        "gs * u subnormal": int((np.isfinite(prod) & (prod != 0) & (np.abs(prod) < F32_MIN) & oc.is_sub(out)).sum()),
        "gs * u overflows": int((np.isfinite(gsf) & np.isfinite(uf) & ((out & 0x7FFF) == 0x7F80)).sum()),
        "0 * inf": int((((gsf == 0) & np.isinf(uf)) | (np.isinf(gsf) & (uf == 0))).sum()),
    }


@pytest.mark.parametrize("geo,rows,variant", oc.GATE_UP_SETS)
def test_gate_up_sets_meet_their_conditions(geo, rows, variant):
    c = oc.gate_up_case(geo, rows, variant); r = oc.gate_up_ref(c)
    assert oc.nan_fraction(r["out"]) <= oc.MAX_NAN_FRACTION
    for m, kd in enumerate(c["kinds"]):                      # the fused norm gives what the recipe rests on
        if kd in "+-":
            want = 0x3F80 if kd == "+" else 0xBF80
            assert (r["xn"][m, :120] == want).all() and (r["xn"][m, 120:128] == want + 1).all(), (m, kd)
        elif kd == "g":                                      # mixed signs, the same magnitudes
            assert ((r["xn"][m, :120] & 0x7FFF) == 0x3F80).all() and ((r["xn"][m, 120:128] & 0x7FFF) == 0x3F81).all() and len(set(r["xn"][m, :120].tolist())) == 2, m
    counts = silu_conditions(r)
    combos = set((r["g"][~oc.is_nan(r["g"])] >> 7).tolist())
    missing = sorted(set(range(512)) - combos)
    print(geo, rows, variant, counts, "sign and exponent combinations:", len(combos), "missing:", missing)
    for name in SILU_CONDITIONS[variant]:
        assert counts[name] >= 1, "%s %d %s: no element with %s" % (geo, rows, variant, name)
    if variant != "window":
        assert len(combos) >= 400, "only %d of the 512 sign and exponent-field combinations reach the table; missing %s" % (len(combos), missing)
    if rows >= 16:
        assert oc.is_nan(r["g"]).any() and oc.is_nan(r["u"]).any(), "the NaN row"
    assert oc.wpack_expect(c["w1"], c["w3"]) == (0 if variant == "window" else 1)


ROPE_ALL = ("a * cr and b * ci agree in 20 leading bits", "a result in the f32-subnormal range", "(+0, +0)", "(-0, +0)", "(+0, -0)", "(-0, -0)")
ROPE_NONFINITE = ("a finite pair whose result overflows", "b = inf at position 0: inf * 0", "NaN in one half only")


def rope_conditions(c, r):
    s = oc.shape_of(c["geo"])
    S = r["xk"].shape[0]
    x = r["xk"].reshape(S, s["KVH"], s["hd"] // 2, 2); o = r["xk_rope"].reshape(S, s["KVH"], s["hd"] // 2, 2)
    a16, b16 = x[..., 0], x[..., 1]
    a, b = oc.wide(a16).astype(np.float64), oc.wide(b16).astype(np.float64)
    cis = oc.cis_table(c["geo"])[c["start_pos"]:c["start_pos"] + S].astype(np.float64)[:, None, :, :]
    cr, ci = np.broadcast_to(cis[..., 0], a.shape), np.broadcast_to(cis[..., 1], a.shape)
    pos = np.broadcast_to((c["start_pos"] + np.arange(S))[:, None, None], a.shape)
    with np.errstate(all="ignore"):
        p1, p2 = a * cr, b * ci
        re, im = p1 - p2, a * ci + b * cr
        agree = np.abs(p1 - p2) <= np.abs(p1) * 2.0 ** -20
    fin = np.isfinite(a) & np.isfinite(b)
    return {
        "a * cr and b * ci agree in 20 leading bits": int((fin & (p1 != 0) & agree).sum()),
        "a result in the f32-subnormal range": int((fin & (((re != 0) & (np.abs(re) < F32_MIN) & oc.is_sub(o[..., 0])) | ((im != 0) & (np.abs(im) < F32_MIN) & oc.is_sub(o[..., 1])))).sum()),
        "a finite pair whose result overflows": int((fin & (((o[..., 0] & 0x7FFF) == 0x7F80) | ((o[..., 1] & 0x7FFF) == 0x7F80))).sum()),
        "(+0, +0)": int(((a16 == 0) & (b16 == 0)).sum()), "(-0, +0)": int(((a16 == 0x8000) & (b16 == 0)).sum()),
        "(+0, -0)": int(((a16 == 0) & (b16 == 0x8000)).sum()), "(-0, -0)": int(((a16 == 0x8000) & (b16 == 0x8000)).sum()),
        "b = inf at position 0: inf * 0": int(((pos == 0) & np.isfinite(a) & np.isinf(b) & oc.is_nan(o[..., 0])).sum()),
        "NaN in one half only": int((oc.is_nan(a16) ^ oc.is_nan(b16)).sum()),
    }


@pytest.mark.parametrize("geo", ["tiny", "wide1024", "hd32", "odd192"])
def test_rope_sets_meet_their_conditions(geo):
    """the pairs of a geometry over all its sets (a condition tied to a position needs the set that holds the position); the NaN cap per set"""
    total, positions = {}, set()
    for st in [t for t in oc.ROPE_SETS if t[0] == geo]:
        c = oc.attn_case(*st); r = oc.kv_ref(c)
        for what in ("xk_rope", "xv"):
            assert oc.nan_fraction(r[what]) <= oc.MAX_NAN_FRACTION, (st, what, oc.nan_fraction(r[what]))
        if st[4] == "finite":
            assert finite(r["xk_rope"]).all() and finite(r["xv"]).all(), "%s: a finite set with a non-finite K or V row" % (st,)
        else:
            assert not finite(r["xk_rope"]).all()
        for k, n in rope_conditions(c, r).items():
            total[k] = total.get(k, 0) + n
        positions |= set(range(st[2], st[2] + st[3]))
        assert st[2] + st[3] <= st[1]
    print(geo, total)
    for name in ROPE_ALL + ROPE_NONFINITE:
        assert total[name] >= 1, "%s: no pair with %s (%s)" % (geo, name, total)
    last_cis = oc.shape_of(geo)["cis_rows"] - 1
    assert {0, 1, last_cis} <= positions and (geo == "odd192" or 36 in positions)
    if geo != "odd192":
        assert any(t[1] == 37 and t[2] + t[3] == 37 for t in oc.ROPE_SETS if t[0] == geo), "the last position of a 37-position context"


@pytest.mark.parametrize("st", [t for t in oc.ROPE_SETS if oc.wo_selects(t[2], t[3], t[4])], ids=str)
def test_one_row_at_position_0_puts_the_v_row_into_the_residual_epilogue_of_wo(st):
    c = oc.attn_case(*st); r = oc.kv_ref(c); s = oc.shape_of(st[0])
    d = oc.attn_oracle(c)[0]
    att = r["xv"].reshape(1, s["KVH"], 1, s["hd"]).repeat(s["H"] // s["KVH"], axis=2).reshape(1, s["q_dim"])
    pin(att, d[("attn_pre_wo", 0)], "%s: p = 1.0, the attention output is the V row" % (st,))
    y = d[("attn_out", 0)]
    pin(att[:, np.arange(s["dim"]) % s["q_dim"]], y, "%s: wo selects" % (st,))
    counts = resid_conditions(c["h"], y)
    print(st, counts)
    for name in ("an exact cancellation to +0", "exponents more than 16 apart where RN + truncation differs from truncating the exact sum", "a negative result whose truncation drops set bits"):
        assert counts[name] >= 1, (st, name, counts)
    assert oc.is_sub(y).any() and finite(d[("h", 0)]).all()


# ---- (c) every wrong epilogue changes a finite output of every case set ------------------------------------------------------------------------------------------------
ROPE_DEFECTS = ("f32", "ci_sign", "next_row", "partner_xor2", "ftz")
INVISIBLE_AT_POSITION_0 = ("f32", "ci_sign")                 # cis row 0 is (1, 0): a * 1 - b * 0 is exact in either width, and +-0 * a adds nothing


@pytest.mark.parametrize("st", oc.ROPE_SETS, ids=str)
def test_wrong_rope_changes_a_finite_output_of_every_set(st):
    geo, _, start, rows, _ = st
    c = oc.attn_case(*st); r = oc.kv_ref(c); s = oc.shape_of(geo)
    import ctypes as C
    from oracle import oracle as orc
    ext = np.zeros((s["cis_rows"] + 1, s["hd"] // 2, 2), dtype=np.float32)           # (one row more: position + 1 of the last cis row)
    orc.lib().orc_rope_table(s["hd"], s["cis_rows"] + 1, C.c_double(oc.GEOS[geo]["rope_theta"]), oc.GEOS[geo]["use_scaled_rope"], orc._p(ext), None)
    assert (ext[:-1] == oc.cis_table(geo)).all()
    counts = {}
    for d in ROPE_DEFECTS:
        got = oc.rope_np(r["xk"], s["KVH"], s["hd"], ext[start:start + rows], d, next_rows=ext[start + 1:start + rows + 1])
        counts[d] = changed(r["xk_rope"], got)
        if not (start + rows == 1 and d in INVISIBLE_AT_POSITION_0):
            assert counts[d] >= 1, "%s: RoPE with the defect %r gives the reference's bits everywhere" % (st, d)
    print(st, counts)


RESID_DEFECTS = ("no_trunc", "exact_sum", "ftz")


@pytest.mark.parametrize("geo,rows", oc.RESID_SETS)
def test_wrong_residual_changes_a_finite_output_of_every_set(geo, rows):
    c = oc.down_case(geo, rows); r = oc.down_ref(c)
    acc = oc.linear_acc(c["act"], c["w2"])
    counts = {d: changed(r["out"], oc.add_np(c["h"], acc, d)) for d in RESID_DEFECTS}
    print(geo, rows, counts)
    for d, n in counts.items():
        assert n >= 1, "%s %d rows: the residual with the defect %r gives the reference's bits everywhere" % (geo, rows, d)


SILU_DEFECTS = ("f32_formula", "gs_not_truncated", "ftz", "swapped")


@pytest.mark.parametrize("geo,rows,variant", oc.GATE_UP_SETS)
def test_wrong_silu_mul_changes_a_finite_output_of_every_set(geo, rows, variant):
    c = oc.gate_up_case(geo, rows, variant); r = oc.gate_up_ref(c)
    ga, ua = oc.linear_acc(r["xn"], c["w1"]), oc.linear_acc(r["xn"], c["w3"])
    counts = {d: changed(r["out"], oc.silu_mul_np(ga, ua, d)) for d in SILU_DEFECTS}
    print(geo, rows, variant, counts)
    for d, n in counts.items():
        assert n >= 1, "%s %d %s: SiLU * up with the defect %r gives the reference's bits everywhere" % (geo, rows, variant, d)
