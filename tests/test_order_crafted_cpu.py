"""The conditions the order-revealing sets of tests/order_craft.py rest on (CPU; the device side is tests/test_gpu_order_crafted.py):

  * the numpy sequential f32 evaluator is orc_linear_bf16 bit for bit on every set, so its mutations are mutations of the reference;
  * on the reference's values every product is exact and a normal f32 or zero, every partial sum finite and a normal f32 or zero, every output finite: a fused
    multiply-add gives what multiply-then-add gives, and the sets serve the matrix-core forms;
  * EVERY wrong order of order_craft.mutations, the pairwise block of four and every single transposition (k, k + 1), k >= 1, changes at least one bf16 output of
    EVERY set, behind the epilogue the GPU test reads it through (plain truncation; SiLU(gate) * up with the chain under test on the gate side and on the up side).
    A condition, not a measurement: a set that cannot meet it is changed, no mutation is left out;
  * the old inputs -- the gaussian sets of the bit-exactness tests and the vector of test_linear_order_sensitivity_guard -- reveal none of them.

QK^T is not covered: the query cannot be injected and the dot runs over 64 or 128 terms only.  The RMSNorm sum of squares is not either: its terms are
non-negative, nothing cancels (NOTES.md).  `python tests/test_order_crafted_cpu.py` prints the table of profiles/order_crafted.md."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":                    # (as a script: what tests/conftest.py does for pytest)
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import kv_craft as kc  # noqa: E402
import op_craft as oc  # noqa: E402
import order_craft as od  # noqa: E402
from linear_cases import bf, orc_linear  # noqa: E402


def routes_of(key):
    return ("store", "gate", "up") if key in od.NORM_SETS + od.PART_SETS else ("store",)


U_CONST, G_CONST = od.U_CONST, od.G_CONST


def through(route, acc):
    """what the GPU test reads of a chain whose f32 result is acc: its truncation, or SiLU(gate) * up with the other side a constant"""
    y = bf(acc)
    if route == "store":
        return y
    if route == "gate":
        return oc.silu_mul_ref(y, np.full(y.shape, U_CONST, dtype=np.uint16))[1]
    return oc.silu_mul_ref(np.full(y.shape, G_CONST, dtype=np.uint16), y)[1]


def counts(key):
    """{(family, route): the smallest number of changed bf16 outputs over the family's mutations} and the (family, name, route) that change none"""
    s = od.get_set(*key)
    K, xf, wf = s["K"], od.wide(s["x"]), od.wide(s["w"])
    muts = od.mutations(K)
    orders, chains = np.stack([m[2] for m in muts]), np.stack([m[3] for m in muts])
    routes = routes_of(key)
    changed = {r: np.zeros(len(muts) + 1, dtype=np.int64) for r in routes}          # (the last one: the pairwise block of four)
    for p in range(len(s["pat"])):
        r0 = int(np.flatnonzero(s["x_pat"] == p)[0]); sel = np.flatnonzero(s["w_pat"] == p)
        P = od.products(xf[r0], wf[sel])
        ref = od.seq_sum(P)
        assert np.array_equal(bf(ref), s["ref"][r0, sel])
        got = np.concatenate([od.evaluate(P, orders, chains), od.pairwise4(P)[None]])
        for r in routes:
            changed[r] += (through(r, got) != through(r, ref)[None]).sum(axis=1)
    fam = [m[0] for m in muts] + ["block of four summed pairwise"]
    names = [m[1] for m in muts] + [""]
    # every single transposition, on the ladder row that holds it as a (v, closer) pair
    trans = {r: np.zeros(K - 1, dtype=np.int64) for r in routes}
    for i, kd in enumerate(s["kinds"]):
        if kd == "zero_sum" or kd == ("head",):
            continue
        r0 = int(np.flatnonzero(s["x_pat"] == s["w_pat"][i])[0])
        p = od.products(xf[r0], wf[i:i + 1])[0]
        res = od.transposition_results(p)
        assert od.seq_sum(p[None])[0] == 0 and s["ref"][r0, i] == 0
        ks = [k for k in range(1, K - 1) if od.closer_row(s["kinds"], k) == i]
        for r in routes:
            zero = through(r, np.zeros(1, dtype=np.float32))[0]
            trans[r][ks] += (through(r, res[ks]) != zero)
    table, silent = {}, []
    for r in routes:
        for f, nm, c in zip(fam, names, changed[r]):
            table[(f, r)] = min(table.get((f, r), 1 << 30), int(c))
            if c == 0:
                silent.append((f, nm, r))
        table[("a single transposition (k, k + 1)", r)] = int(trans[r][1:].min())
        silent += [("transposition", str(k), r) for k in range(1, K - 1) if trans[r][k] == 0]
    return table, silent, len(muts) + 1 + K - 2


@pytest.mark.parametrize("key", od.ALL_SETS)
def test_numpy_evaluator_is_the_oracle_and_the_values_stay_exact_and_normal(key):
    s = od.get_set(*key)
    xf, wf = od.wide(s["x"]), od.wide(s["w"])
    assert np.array_equal(od.linear_np(s["x"], s["w"]), s["ref"])
    tiny = 2.0 ** -126
    for r in range(s["rows"]):
        P = od.products(xf[r], wf)
        P64 = xf[r].astype(np.float64)[None, :] * wf.astype(np.float64)
        assert np.array_equal(P.astype(np.float64), P64), "a product is not exact"
        assert np.all((P == 0) | (np.abs(P) >= tiny)) and np.all(np.isfinite(P))
        acc, ok = od.seq_sum(P, track=True)
        assert ok, "a partial sum is not finite, or subnormal"
        assert np.all(np.isfinite(acc))
    assert np.all(np.isfinite(od.wide(s["ref"])))
    # the ladder rows give exactly +0 under their own pattern, whatever the scale of the x row
    for i, kd in enumerate(s["kinds"]):
        if kd != "zero_sum":
            assert np.all(s["ref"][s["x_pat"] == s["w_pat"][i], i] == 0)


@pytest.mark.parametrize("key", od.ALL_SETS)
def test_every_wrong_order_changes_a_bf16_output_of_every_set(key):
    table, silent, n = counts(key)
    assert not silent, "%d of %d wrong orders change no bf16 output of the set %s: %s" % (len(silent), n, key, silent[:10])


@pytest.mark.parametrize("key", od.WHOLE_SETS)
def test_the_norm_of_a_whole_model_hands_the_product_the_rows(key):
    s = od.get_set(*key)
    h, nw = od.norm_front_rows(s)
    assert np.array_equal(oc.rmsnorm(h, nw), s["x"]) and len({tuple(r) for r in h.tolist()}) == s["rows"]


@pytest.mark.parametrize("key", od.NORM_SETS + od.PART_SETS)
def test_the_fused_norm_hands_the_product_the_pattern(key):
    s = od.get_set(*key)
    h, nw = od.norm_front(s["pat"][0])
    xn = oc.rmsnorm(h[None, :], nw)
    assert s["rows"] == 1 and np.array_equal(xn, s["x"])
    # gate and up as the GPU test composes them: a constant on the other side
    w3 = od.gate_up_constant(s, U_CONST)
    assert np.all(orc_linear(s["x"], w3) == U_CONST)


# ---- the sets of the 13-bit packed kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", od.PACKED_KS)
def test_the_packed_sets_pack_and_every_wrong_order_changes_a_bf16_output_of_the_group(K):
    """every matrix of the group: the fused norm gives its x row, the matrix -- alone (the head) and beside the constant of the other side (gate|up) -- lies inside
    lnb_wpack.h's window, the values are exact and normal, the numpy evaluator is the oracle; over the GROUP every wrong order changes a bf16 output behind each
    epilogue, and every transposition (k, k + 1), 1 <= k <= K - 2, changes the ladder row of some ramp matrix that holds it as a (v, closer) pair"""
    group = od.get_packed(K)
    muts = od.mutations(K)
    orders, chains = np.stack([m[2] for m in muts]), np.stack([m[3] for m in muts])
    routes = ("store", "gate", "up")
    changed = {r: np.zeros(len(muts) + 1, dtype=np.int64) for r in routes}
    trans = {r: np.zeros(K, dtype=np.int64) for r in routes}
    for m in group:
        assert np.array_equal(oc.rmsnorm(m["h"][None, :], m["nw"]), m["x"]), m["name"]
        for value in (U_CONST, G_CONST):
            c = od.packed_constant(m, value)
            assert oc.wpack_expect(m["w"], c) == 0 and oc.wpack_expect(c, m["w"]) == 0 and np.all(orc_linear(m["x"], c) == value), m["name"]
        assert oc.wpack_expect(m["w"], m["w"]) == 0
        xf, wf = od.wide(m["x"])[0], od.wide(m["w"])
        P = od.products(xf, wf)
        assert np.array_equal(P.astype(np.float64), xf.astype(np.float64)[None, :] * wf.astype(np.float64))
        assert np.all((P == 0) | (np.abs(P) >= 2.0 ** -126)) and np.all(np.isfinite(P))
        ref, ok = od.seq_sum(P, track=True)
        assert ok and np.array_equal(bf(ref), m["ref"]), m["name"]
        assert all(m["ref"][i] == 0 for i, kd in enumerate(m["kinds"]) if kd != "zero_sum")
        got = np.concatenate([od.evaluate(P, orders, chains), od.pairwise4(P)[None]])
        for r in routes:
            changed[r] += (through(r, got) != through(r, ref)[None]).sum(axis=1)
        for row in sorted(set(m["pairs"].values())):
            res = od.transposition_results(P[row])
            ks = [k for k, i in m["pairs"].items() if i == row]
            for r in routes:
                trans[r][ks] += (through(r, res[ks]) != through(r, np.zeros(1, dtype=np.float32))[0])
    for r in routes:
        silent = [m[:2] for m, c in zip(muts + [("block of four summed pairwise", "")], changed[r]) if c == 0]
        silent += [("transposition", k) for k in range(1, K - 1) if trans[r][k] == 0]
        assert not silent, (K, r, len(silent), silent[:10])


# ---- the PV chain of the attention (tests/kv_craft.py, case v_order) ----------------------------------------------------------------------------------------------
PV_STAGES = (64, 256, 512)          # positions per PV chunk, per scores block, per PV batch; the second K register set begins at 512: one of the splits in two


@pytest.mark.parametrize("geometry", sorted(kc.GEOMETRIES))
def test_every_wrong_order_of_the_pv_chain_changes_a_bf16_output(geometry):
    """for every T of the grid and every query head: the chain out = out + p[t] * V[t] over the T positions (the call's own row last) on the oracle's own softmax and
    cache -- exact products, normal partial sums, the oracle's attn_pre_wo bits -- and every wrong order changes a bf16 output of that head"""
    cfg = kc.GEOMETRIES[geometry]
    H, hd, rep = cfg["n_heads"], kc.head_dim(cfg), cfg["n_heads"] // cfg["n_kv_heads"]
    Ts = [T for c, T in kc.grid() if c == "v_order"]
    assert Ts == [T for T in kc.TS if T >= 15]
    for T in Ts:
        r = kc.oracle_run("v_order", geometry, T)
        d = r["dumps"]
        assert not np.isnan(r["logits"]).any() and not d[("scores", 0)][:, 0, :T - 1].any()          # every cached score is +0
        p = kc.wide(d[("softmax", 0)])[:, 0, :]
        V = kc.wide(r["kv"][0][1])
        att = d[("attn_pre_wo", 0)].reshape(H, hd)
        kinds, w = kc.pv_kinds(T - 1, hd), kc.pv_windows(T - 1, hd)
        muts = od.mutations(T, PV_STAGES)
        orders, chains = np.stack([m[2] for m in muts]), np.stack([m[3] for m in muts])
        for h in range(H):
            assert (p[h, :T - 1] == p[h, 0]).all() and p[h, 0] > 0
            P = od.products(p[h], V[:, h // rep, :].T)
            assert np.array_equal(P.astype(np.float64), p[h].astype(np.float64)[None, :] * V[:, h // rep, :].T.astype(np.float64))
            assert np.all((P == 0) | (np.abs(P) >= 2.0 ** -126))
            ref, ok = od.seq_sum(P, track=True)
            assert ok and np.array_equal(bf(ref), att[h]), (geometry, T, h)
            got = np.concatenate([od.evaluate(P, orders, chains), od.pairwise4(P)[None]])
            changed = (bf(got) != bf(ref)[None]).sum(axis=1)
            silent = [m[:2] for m, c in zip(muts + [("block of four summed pairwise", "")], changed) if c == 0]
            for col, kd in enumerate(kinds):
                if isinstance(kd, tuple) and kd[0] == "ladder":
                    res = od.transposition_results(P[col])
                    ks = [k for k in range(1, T - 2) if od.closer_row(kinds, k, w) == col]
                    silent += [("transposition", k) for k in ks if bf(res[k:k + 1])[0] == bf(ref[col:col + 1])[0]]
            assert not silent, (geometry, T, h, len(silent), silent[:8])


# ---- what the old inputs show ------------------------------------------------------------------------------------------------------------------------------------
def _gaussian(rows, n, k, rw=16):
    """tests/linear_cases.py's check_linear_bit_exact inputs, with test_gpu_parity.py's seed"""
    rng = np.random.default_rng(rows * 7 + n + k + rw)
    return bf(rng.standard_normal((rows, k)) * 10 ** rng.uniform(-2, 2)), bf(rng.standard_normal((n, k)) * 0.05)


def _three_wrong_orders(K):
    ident, zero = np.arange(K), np.zeros(K, dtype=np.int64)
    last = np.concatenate([ident[:K - 128], ident[K - 64:], ident[K - 128:K - 64]])
    return np.stack([ident, ident, last]), np.stack([(ident >= K // 2).astype(np.int64), ident % 2, zero])


def test_the_old_inputs_reveal_almost_nothing():
    """the three small gaussian sets: split in halves, even / odd chains and the last two 64-blocks swapped change many f32 sums and NO bf16 output; the vector of
    test_linear_order_sensitivity_guard (1.0 and 4095 terms of 2^-12: 13 significant bits) has the same f32 sum in every order"""
    for rows, n, k in ((1, 24, 256), (1, 16, 512), (3, 100, 896)):
        x, w = _gaussian(rows, n, k)
        orders, chains = _three_wrong_orders(k)
        f32_changed = 0
        for r in range(rows):
            P = od.products(od.wide(x)[r], od.wide(w))
            ref, got = od.seq_sum(P), od.evaluate(P, orders, chains)
            f32_changed += int((got != ref[None]).sum())
            assert np.array_equal(bf(got), np.broadcast_to(bf(ref), got.shape)), (rows, n, k)
        assert f32_changed > 0
    k = 4096
    wrow = np.full(k, 2.0 ** -12, dtype=np.float32); wrow[0] = 1.0
    P = wrow[None, :]
    orders, chains = _three_wrong_orders(k)
    got = od.evaluate(P, np.concatenate([orders, np.arange(k)[None, ::-1]]), np.concatenate([chains, np.zeros((1, k), dtype=np.int64)]))
    assert np.all(got == od.seq_sum(P)[0]) and od.pairwise4(P)[0] == od.seq_sum(P)[0]


def table_text():
    lines = []
    fams = None
    rows = {}
    for key in od.ALL_SETS:
        t, silent, n = counts(key)
        assert not silent
        for (f, r), c in t.items():
            rows.setdefault((f, r), {})[key] = c
    keys = od.ALL_SETS
    lines.append("| wrong order (smallest count over the family) | read through | " + " | ".join(", ".join(str(v) for v in k) for k in keys) + " |")
    lines.append("|---|---|" + "---|" * len(keys))
    for (f, r), d in rows.items():
        lines.append("| %s | %s | " % (f, r) + " | ".join(str(d[k]) if k in d else "-" for k in keys) + " |")
    return "\n".join(lines)


if __name__ == "__main__":
    print(table_text())
