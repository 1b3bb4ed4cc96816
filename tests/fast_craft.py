"""Inputs on which the tolerance mode (LNB_MODE_FAST, csrc/lnb_fast.hip) has no tolerance (tests/test_fast_crafted_cpu.py, tests/test_gpu_fast_crafted.py).
numpy and the oracle only, no GPU code.

The mode changes the ORDER of every product's f32 adds (split-K over lanes, waves and matrix-core k-steps) and nothing else.  On operands for which every order
of the adds gives the same f32 the fast kernels owe the oracle's 16 bits, and a wrong address, a dropped unit or a swapped chain shows in them:

  address probes  row m of x is one-hot at k_m (1.0, or -2^e), w[n][k] a hash of (n, k) into normal bf16 patterns: the output IS w[n][k_m] (or its scaled,
                  negated pattern).  probe_columns(K): every k of the first 130, both sides of every 64-boundary, the last 17, and a spread.
  exact sums      x elements +-2^j, w elements small integers times a power of two per row: every product is an integer of a grid and the sum of the
                  magnitudes of a row's products stays below 2^24 (variant 24) or 2^16 (variant 16) grid units, so every partial sum of every order is exact.
                  A call has up to three x patterns (row m: pattern m % 3 times +-2^e); weight row n is made for pattern n % 3: a few closing terms steer its
                  total there to an integer t, 0 < |t| <= 255 -- all 16 output bits significant, one product more or less visible.  Under the other patterns'
                  rows the sums are generic and as exact.
  norm front      rows of h whose sum of squares is exact in any order: equal magnitudes (op_craft's recipe: trunc(x r) = +-0x3F7F, norm weight 0x3F81 * 2^j ->
                  +-2^j) or elements +-2^e (one significand c behind the norm: xn = c * +-2^e); the weights are steered for the normalised rows.
  epilogue sets   op_craft's residual, SiLU * up and RoPE cases with their gaussian rows and columns replaced by exact-sum ones.

order_independent() is the sufficient condition (at most two non-zero products, or integers of a grid whose magnitudes sum below 2^24 units); evaluate_orders()
sums a set in five orders in f32.

Attention sets (Q [S, H, hd], K, V [T, KVH, hd] as bf16 bits): every score is an integer or a half, exact in f32 in any order.  flash_model() restates
fast_attn_prefill_kernel in f32 numpy with its rounding points and takes the defects a flash kernel can have; softmax_f64() is the reference and bound() the
derived bound of the GPU test."""
import numpy as np

import op_craft as oc
from oracle import oracle as orc

bf, wide = oc.bf, oc.wide
ONE = 0x3F80


def exact_bf(a):
    """bf16 bits of values that must be bf16-exact"""
    a = np.asarray(a, dtype=np.float64)
    b = bf(a.astype(np.float32))
    assert np.array_equal(wide(b).astype(np.float64), a), "not exact in bf16"
    return b


# ---- address probes ---------------------------------------------------------------------------------------------------------------------------------------------
def hash_w(N, K, seed=0):
    """w[n][k]: a 32-bit mix of (n, k) folded into sign | exponent field 64 .. 190 | mantissa: normal, finite, non-zero"""
    n = np.arange(N, dtype=np.uint32)[:, None]; k = np.arange(K, dtype=np.uint32)[None, :]
    h = n * np.uint32(0x9E3779B1) + k * np.uint32(0x85EBCA77) + np.uint32((seed * 0xC2B2AE3D + 0x27D4EB2F) & 0xFFFFFFFF)
    h ^= h >> np.uint32(15); h *= np.uint32(0x2C1B3C6D); h ^= h >> np.uint32(12); h *= np.uint32(0x297A2D39); h ^= h >> np.uint32(15)
    return (((h & np.uint32(1)) << np.uint32(15)) | ((np.uint32(64) + (h >> np.uint32(1)) % np.uint32(127)) << np.uint32(7)) | ((h >> np.uint32(9)) & np.uint32(0x7F))).astype(np.uint16)


def probe_columns(K):
    ks = set(range(min(130, K))) | set(range(max(0, K - 17), K))
    for b in range(64, K, 64):
        ks |= {b - 1, b}
    ks |= {(i * K) // 29 + (i * 5) % 8 for i in range(29) if (i * K) // 29 + (i * 5) % 8 < K}
    return sorted(ks)


def probe_x(K, cols, variant):
    """x [len(cols), K]: row m one-hot at cols[m]; variant 0: 1.0, variant 1: -2^e, e = -8 .. 8 by row and column"""
    x = np.zeros((len(cols), K), dtype=np.uint16)
    for m, k in enumerate(cols):
        x[m, k] = ONE if variant == 0 else int(bf(np.float32(-2.0 ** ((3 * m + k) % 17 - 8))))
    return x


def probe_calls(K, rows, limit=None):
    """the column lists of calls of `rows` rows that cover probe_columns(K) (the last one wraps around); limit: that many calls, spread over the list"""
    cols = probe_columns(K)
    calls = [[cols[(i + r) % len(cols)] for r in range(rows)] for i in range(0, len(cols), rows)]
    if limit is not None and len(calls) > limit:
        calls = [calls[(i * len(calls)) // limit] for i in range(limit)]
    return calls


def probe_expected(w, cols, variant):
    """what the one-hot rows select: the pattern itself, or its sign flipped and its exponent field moved"""
    sel = w[:, cols].T.astype(np.int32)
    if variant == 0:
        return sel.astype(np.uint16)
    e = np.array([(3 * m + k) % 17 - 8 for m, k in enumerate(cols)], dtype=np.int32)[:, None]
    return ((sel ^ 0x8000) + (e << 7)).astype(np.uint16)


# ---- exact sums ---------------------------------------------------------------------------------------------------------------------------------------------------
N_PAT = 3
AW_MAX = {24: 15, 16: 3}
XJ_MAX = {24: 2, 16: 1}                        # x elements +-2^j, j = 0 .. XJ_MAX


def sum_bound(K, bits):
    """the largest sum of magnitudes of a steered row's products, in grid units: the free terms, the closing terms (which cancel them down to t), t itself"""
    return 2 * K * AW_MAX[bits] * 2 ** XJ_MAX[bits] + 255


def steered_w(rng, U, N, bits, cols=None):
    """w f64 [N, K] of small integers such that row n against pattern U[n % len(U)] (elements +-2^j, f64) sums to t[n], 0 < |t| <= 255; -> (w, t).
    The closing terms sit at spread places (another base place in every row) and carry the part of t - partial their 8 bits hold.  cols: the columns in use
    (the others stay zero)."""
    P, K = U.shape
    cols = np.arange(K) if cols is None else np.asarray(cols)
    Kc = cols.size
    aw = AW_MAX[bits]
    assert np.all(np.abs(U[:, cols]) >= 1) and 2 * Kc * aw * np.abs(U).max() + 255 < 2 ** bits
    w = np.zeros((N, K), dtype=np.float64)
    w[:, cols] = rng.choice([-1.0, 1.0], (N, Kc)) * rng.integers(1, aw + 1, (N, Kc))
    t = rng.choice([-1.0, 1.0], N) * rng.integers(1, 256, N)
    bound = Kc * aw * np.abs(U).max() + 255
    n_close = 0 if bound <= 255 else int(np.ceil(np.log2(bound + 1) / 8.0))
    if n_close == 0:
        return w, (U[np.arange(N) % P] * w).sum(axis=1)
    assert n_close < Kc
    rows = np.arange(N)
    pos = cols[(rng.integers(0, Kc, N)[:, None] + np.arange(n_close)[None, :] * (Kc // n_close)) % Kc]        # [N, n_close], distinct in a row
    w[rows[:, None], pos] = 0.0
    Un = U[rows % P]
    R = t - (Un * w).sum(axis=1)
    a = np.abs(R).astype(np.int64)
    for i in range(n_close):
        piece = np.sign(R) * ((a >> (8 * i)) & 255) * 2.0 ** (8 * i)
        w[rows, pos[:, i]] = piece / Un[rows, pos[:, i]]
    assert np.array_equal((Un * w).sum(axis=1), t)
    return w, t


def x_patterns(rng, K, bits, n_pat=N_PAT):
    return rng.choice([-1.0, 1.0], (n_pat, K)) * 2.0 ** rng.integers(0, XJ_MAX[bits] + 1, (n_pat, K))


def row_scales(rows, n_pat=N_PAT):
    """row m = pattern m % n_pat times +-2^e: the first group unscaled"""
    g = np.arange(rows) // n_pat
    return np.where(g % 2 == 1, -1.0, 1.0) * 2.0 ** ((g + 2) % 5 - 2)


_SETS = {}


def exact_sum_set(rows, N, K, bits=24, seed=0):
    """dict(x [rows, K], w [N, K] uint16, t [N], scale [rows], wscale [N]): y[m][n] = t[n] * scale[m] * wscale[n] wherever m % 3 == n % 3"""
    key = ("sum", N, K, bits, seed)
    if key not in _SETS:                                                     # (the weights do not depend on the row count; only the last ones made are kept)
        for old in [k_ for k_ in _SETS if k_[0] == "sum"][:-3]:
            del _SETS[old]
        rng = np.random.default_rng([21, N, K, bits, seed])
        U = x_patterns(rng, K, bits)
        w, t = steered_w(rng, U, N, bits)
        wscale = 2.0 ** (np.arange(N) % 7 - 3)
        _SETS[key] = dict(U=U, w=exact_bf(w * wscale[:, None]), t=t, wscale=wscale, bits=bits)
    scale = row_scales(rows)
    return dict(_SETS[key], x=exact_bf(_SETS[key]["U"][np.arange(rows) % N_PAT] * scale[:, None]), scale=scale)


# ---- through the fused norm -----------------------------------------------------------------------------------------------------------------------------------------
def norm_front_set(rows, N, K, kind, seed=0):
    """dict(h [rows, K], nw [K], w [N, K] uint16, xn: the oracle's normalised rows).  kind "equal": h = +-c per row (c a power of two), nw = 0x3F81 * 2^j: xn is
    +-2^j exactly.  kind "pow2": h = +-2^e (e in {0, 1}) times the row's scale, nw = 1.0: xn = c * +-2^e with ONE 8-bit significand c per row.  The weights are
    steered (variant 16: 2^16 grid units times c's 8 bits stay below 2^24) for the three patterns as the oracle normalises them."""
    key = ("norm", rows, N, K, kind, seed)
    if key not in _SETS:
        rng = np.random.default_rng([22, N, K, kind == "equal", seed])
        sg = rng.choice([-1.0, 1.0], (N_PAT, K))
        if kind == "equal":
            hp = sg.copy()
            nw = (0x3F81 + (rng.integers(0, 2, K) << 7)).astype(np.uint16)
        else:
            hp = sg * 2.0 ** rng.integers(0, 2, (N_PAT, K))
            nw = np.full(K, ONE, dtype=np.uint16)
        xp = wide(oc.rmsnorm(exact_bf(hp), nw)).astype(np.float64)                    # the three patterns behind the oracle's norm
        mant, ex = np.frexp(np.abs(xp))
        assert (mant == mant[:, :1]).all(), "one significand per normalised row"
        U = np.sign(xp) * 2.0 ** (ex - ex.min())
        assert kind != "equal" or (mant == 0.5).all()
        w, t = steered_w(rng, U, N, 16)
        wscale = 2.0 ** (np.arange(N) % 7 - 3)
        scale = row_scales(rows)
        h = exact_bf(hp[np.arange(rows) % N_PAT] * scale[:, None])
        _SETS[key] = dict(h=h, nw=nw, w=exact_bf(w * wscale[:, None]), xn=oc.rmsnorm(h, nw), t=t)
    return _SETS[key]


# ---- the sufficient condition, and five orders ---------------------------------------------------------------------------------------------------------------------
def _lsb_exp(v):
    """exponent of the lowest set bit of every non-zero finite bf16 value (f64 array); zeros: +inf"""
    mant, ex = np.frexp(np.abs(v))
    m = np.round(mant * 256).astype(np.int64)
    tz = np.zeros(v.shape, dtype=np.int64)
    for b in range(8):
        tz += ((m & ((1 << (b + 1)) - 1)) == 0) & (m != 0)
    return np.where(v != 0, (ex - 8 + tz).astype(np.float64), np.inf)


def order_independent(x16, w16):
    """bool [rows, N]: the f32 sum of output (m, n) is the same in every order -- at most two non-zero products (one add, commutative), or every product an integer
    of the grid 2^(lowest bit of the row of x + lowest bit of the row of w) and the sum of their magnitudes below 2^24 units (every partial sum exact).  A NaN in
    either row makes one product NaN and with it the sum, in any order; rows that hold an infinity count through the first rule only."""
    with np.errstate(all="ignore"):
        xf, wf = wide(x16).astype(np.float64), wide(w16).astype(np.float64)
    nan = np.isnan(xf).any(axis=1)[:, None] | np.isnan(wf).any(axis=1)[None, :]
    fx, fw = np.isfinite(xf).all(axis=1), np.isfinite(wf).all(axis=1)
    x0, w0 = np.where(np.isfinite(xf), xf, 1.0), np.where(np.isfinite(wf), wf, 1.0)
    nnz = (x0 != 0).astype(np.float64) @ (w0 != 0).astype(np.float64).T
    with np.errstate(all="ignore"):
        grid = _lsb_exp(x0).min(axis=1)[:, None] + _lsb_exp(w0).min(axis=1)[None, :]
        units = (np.abs(x0) @ np.abs(w0).T) / 2.0 ** grid
    lo = (np.abs(x0) @ np.abs(w0).T) < 2.0 ** 127                                     # (no overflow on the way)
    tiny = grid >= -149                                                              # (the grid itself is an f32 value)
    ok = nan | (nnz <= 2) | ((units < 2.0 ** 24) & lo & tiny & fx[:, None] & fw[None, :])
    # the grid above is that of the whole rows; where it fails, the grid of the places where BOTH operands are non-zero (a column of zero weights does not count)
    lx, lw = _lsb_exp(x0), _lsb_exp(w0)
    for n in np.unique(np.argwhere(~ok)[:, 1]):
        if not fw[n]:
            continue
        both = (x0 != 0) & (w0[n] != 0)[None, :]
        g = np.where(both, lx + lw[n][None, :], np.inf).min(axis=1)
        with np.errstate(all="ignore"):
            u = (np.abs(x0) * np.abs(w0[n])[None, :]).sum(axis=1) / 2.0 ** g
        ok[:, n] |= fx & ((u < 2.0 ** 24) | ~both.any(axis=1)) & (g >= -149)
    return ok


def evaluate_orders(x16, w16):
    """the f32 accumulators [rows, N] of five orders: the reference's chain (k ascending), reversed, 4-way and 64-way split-K (k mod ways, the partials added in
    ascending order), and a pairwise tree"""
    xf, wf = wide(x16), wide(w16)
    P = xf[:, None, :] * wf[None, :, :]                      # exact: 8 x 8 bits
    K = P.shape[2]

    def chain(Q):
        acc = np.zeros(Q.shape[:-1], dtype=np.float32)
        for k in range(Q.shape[-1]):
            acc = acc + Q[..., k]
        return acc

    def split(ways):
        parts = []
        for r in range(min(ways, K)):
            parts.append(chain(P[..., r::ways]))
        return chain(np.stack(parts, axis=-1))

    def tree(Q):
        while Q.shape[-1] > 1:
            if Q.shape[-1] & 1:
                Q = np.concatenate([Q, np.zeros(Q.shape[:-1] + (1,), dtype=np.float32)], axis=-1)
            Q = Q[..., 0::2] + Q[..., 1::2]
        return Q[..., 0]

    with np.errstate(all="ignore"):
        return dict(chain=chain(P), reversed=chain(P[..., ::-1]), split4=split(4), split64=split(64), tree=tree(P))


def same_f32(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


# ---- the shapes the GPU test runs (tests/test_gpu_fast_crafted.py), shared with the CPU proof ----------------------------------------------------------------------
# (form, N, rw, K): the split-K GEMV at 1 / 2 / 15 rows.  A round of loads of fast_gemv_a is 4 * (64 / RG) * 8 chunks of 8: K = 2056 / 1032 / 520 / 264 leave the
# first round exceeded by one chunk, the smaller K leave it partial.  fast_gemv_b: 32 chunks of 128 per round; 4224 = 33 chunks.
GEMV_SHAPES = ([("fast_gemv_a.rg8", 100, 16, K) for K in (8, 64, 896, 2056)] + [("fast_gemv_a.rg16", 4096, 16, K) for K in (256, 1032)] +
               [("fast_gemv_a.rg32", 32768, 32, K) for K in (64, 520)] + [("fast_gemv_a.rg64", 65536, 64, K) for K in (64, 264)] +
               [("fast_gemv_b", N, 4, K) for K in (128, 1024, 4224) for N in (16, 18, 5000)])
GEMV_ROWS = (1, 2, 15)
# the bf16 GEMM: layout (rw) x K x (N, S); every N and S meets every layout, and every K but 4096 (four of the seven pairs there: the oracle's time)
GEMM_RWS = (16, 32, 64, 4)
GEMM_KS = {16: (64, 128, 192, 448, 4096), 32: (64, 128, 192, 448, 4096), 64: (64, 128, 192, 448, 4096), 4: (128, 384, 4096)}      # layout B: K a multiple of 128
GEMM_NS = ((32, 16), (100, 33), (256, 128), (260, 129), (100, 300), (260, 16), (32, 129))
GEMM_2WG0_ROWS = (100, 130, 300)                # LNB_FAST_GEMM_2WG=0: MT 4 / WB 3 up to 128 rows, MT 8 / WB 3 above


def gemm_shapes():
    out = []
    for rw in GEMM_RWS:
        for K in GEMM_KS[rw]:
            for i, (N, S) in enumerate(GEMM_NS):
                if K == 4096 and i not in (2, 3, 4, 5):
                    continue
                out.append((rw, K, N, S))
    return out


NORM_SHAPES = [(rw, K) for rw in (16, 32, 64) for K in (8, 256, 4096)]
NORM_N = 100


# ---- the epilogue sets: op_craft's cases, their gaussian parts replaced ------------------------------------------------------------------------------------------------
def _sign_row(geo, dim):
    return np.random.default_rng([23, sorted(oc.GEOS).index(geo)]).choice([-1.0, 1.0], dim)


def _exact_h(c, geo):
    """the half-gaussian "g" rows of op_craft.norm_rows become rows of mixed signs and one magnitude; the norm weight 0x3F81 (0x3F82 on columns 120 .. 127, the
    -0 recipe's) on EVERY column: xn = +-1.0 (+-0x3F81 there) in every row, and the sum of squares K c^2 in any order"""
    dim = c["h"].shape[1]
    sg = _sign_row(geo, dim)
    for m, kd in enumerate(c["kinds"]):
        if kd == "g":
            c["h"][m] = bf((sg * (1.0, 2.0, 0.5, 4.0)[(m // 4) % 4]).astype(np.float32))
    c["nw"] = np.full(dim, 0x3F81, dtype=np.uint16)
    c["nw"][120:128] = 0x3F82
    return sg


def _norm_patterns(geo, dim):
    """the three rows xn can be on the columns outside 120 .. 127: all +1.0, the sign row, all -1.0 (steered through the first: its negative)"""
    return np.stack([np.ones(dim), _sign_row(geo, dim), -np.ones(dim)])


def gate_up_case(geo, rows, variant):
    assert variant in ("exact", "split")
    c = oc.gate_up_case(geo, rows, variant)
    dim = c["h"].shape[1]
    _exact_h(c, geo)
    F = c["w1"].shape[0]
    n_sel = F - oc.N_GAUSS_ROWS
    cols = np.concatenate([np.arange(120), np.arange(128, dim)])
    for name, s in (("w1", 31), ("w3", 33)):
        rng = np.random.default_rng([s, sorted(oc.GEOS).index(geo)])
        w, _ = steered_w(rng, _norm_patterns(geo, dim), oc.N_GAUSS_ROWS, 24, cols)
        c[name][n_sel:] = exact_bf(w * 2.0 ** (np.arange(oc.N_GAUSS_ROWS) % 5 - 9)[:, None])            # (gates and ups of a few units and below)
    return c


def down_case(geo, rows):
    """op_craft.down_case with the gaussian block under the last 32 output rows (activations b0 .. c0 against w2[n_sel:, b0:c0]) made of exact sums; the gaussian
    activations under zero weights and the gaussian weights over zero activations stay: their products are zeros"""
    assert rows != 256
    c = oc.down_case(geo, rows)
    dim, F = c["w2"].shape
    b0, c0 = 2 * oc.SLOTS, 2 * oc.SLOTS + (F - 2 * oc.SLOTS) // 2
    n_sel = dim - 32
    rng = np.random.default_rng([24, sorted(oc.GEOS).index(geo)])
    U = x_patterns(rng, c0 - b0, 24)
    w, _ = steered_w(rng, U, 32, 24)
    c["w2"][n_sel:, b0:c0] = exact_bf(w * 2.0 ** (np.arange(32) % 5 - 6)[:, None])
    nan_rows = oc.is_nan(c["act"]).any(axis=1)
    x = U[np.arange(rows) % N_PAT] * row_scales(rows)[:, None]
    c["act"][:, b0:c0] = exact_bf(x)
    assert np.array_equal(oc.is_nan(c["act"]).any(axis=1), nan_rows)
    return c


def attn_case(geo, capacity, start_pos, rows, variant):
    """op_craft.attn_case with exact rows of h: wk and wv are selector and two-hot rows throughout; wq stays gaussian (Q is not observable from a stage, and at
    position 0 with one row the attention output is the V row whatever Q is)"""
    c = oc.attn_case(geo, capacity, start_pos, rows, variant)
    _exact_h(c, geo)
    return c


GATE_UP_SETS = [(g, r, "exact") for g in ("tiny", "wide1024") for r in (1, 2, 15)] + [(g, r, "split") for g in ("tiny", "wide1024") for r in (16, 17, 83)]
DOWN_SETS = [(g, r) for g in ("tiny", "wide1024") for r in (1, 2, 15, 16, 17, 83)]
ATTN_PART_SETS = [("tiny", 37, 0, 1, "finite"), ("tiny", 128, 0, 2, "finite"), ("tiny", 128, 15, 15, "finite"), ("tiny", 128, 16, 16, "finite"), ("tiny", 128, 17, 17, "finite"),
                  ("tiny", 128, 0, 83, "finite"), ("tiny", 128, 0, 2, "nonfinite"), ("tiny", 128, 0, 17, "nonfinite"), ("wide1024", 37, 0, 1, "finite"),
                  ("wide1024", 128, 0, 2, "finite"), ("wide1024", 128, 15, 15, "finite"), ("wide1024", 128, 16, 16, "finite"), ("wide1024", 128, 17, 17, "finite"),
                  ("wide1024", 128, 0, 83, "finite")]


# ---- attention sets ---------------------------------------------------------------------------------------------------------------------------------------------------
GEOMETRIES = {"hd64_4_2": (64, 4, 2), "hd128_2_1": (128, 2, 1), "hd128_8_2": (128, 8, 2), "hd64_4_4": (64, 4, 4)}      # head_dim, heads, KV heads; 8 heads: the XCD remap
ROWS = (16, 17, 31, 32, 33, 127, 128, 129, 160, 300)
CALLS = [(S, 0) for S in ROWS] + [(S, S) for S in ROWS] + [(40, 24)]
ANCHOR_CALLS = [(1, 0), (1, 39), (15, 0), (15, 15), (16, 0), (16, 16), (40, 0), (40, 40)]      # exact mode: the reference's broadcast rule holds in all of them
SETS = ("rising", "falling", "spike", "uniform", "per_head")
QNAN = 0x7FC0
C0 = {64: 8.0, 128: 11.0}                      # raw score per nat: the divisor is trunc_bf16(sqrt(head_dim)) = 8 and 11.3125 (0.972 nats per step at head_dim 128)
SPIKE = {64: (16.0, 10.0), 128: (2.0, 113.0)}  # q * k = 160 and 226: 20 and 19.98 nats above the rest


def divisor(hd):
    return float(wide(bf(np.float32(np.sqrt(float(hd))))))


def _hash_v(T, KVH, hd, seed):
    """V[j][kvh][d] = +-(1 + m / 128) * 2^(-1 .. 0), another pattern at every position, KV head and dim"""
    h = hash_w(T * KVH, hd, seed).reshape(T, KVH, hd)
    return ((h & 0x807F) | ((126 + ((h >> 7) & 1)) << 7)).astype(np.uint16)


def _dims(hd, kvh, n):
    """n dims of a head, other ones for every KV head, none in the same 8-unit twice"""
    return [(5 + 8 * (3 * i + kvh) + (i + kvh) % 8) % hd for i in range(n)]


def attention_set(name, geometry, S, start_pos):
    """dict(q [S, H, hd], k, v [T, KVH, hd] uint16, S, start_pos, T, hd, H, KVH).  Positions and rows enter the scores split as 32 a + b, so every operand is an
    integer of at most 8 bits; the dims that carry a score differ per KV head, and where one operand of a dim is non-zero the other is zero in every other dim
    that is used: a product read from a wrong dim or a wrong head changes a score by whole nats."""
    hd, H, KVH = GEOMETRIES[geometry]
    T = start_pos + S
    rep = H // KVH
    c0 = C0[hd]
    q = np.zeros((S, H, hd)); k = np.zeros((T, KVH, hd))
    i = np.arange(S); j = np.arange(T)
    seed = SETS.index(name) * 16 + sorted(GEOMETRIES).index(geometry)
    v = _hash_v(T, KVH, hd, seed)
    for h in range(H):
        g = h // rep
        d = _dims(hd, g, 6)
        if name in ("rising", "falling", "per_head"):
            slope = c0 if name != "per_head" else c0 * (1 + h % 4) / 2.0
            sgn = 1.0 if name == "rising" else -1.0
            q[:, h, d[0]] = sgn * 32 * slope; q[:, h, d[1]] = sgn * slope                     # . (a_j, b_j) = +-slope j
            if name == "rising":
                q[:, h, d[2]] = -(i // 32); q[:, h, d[3]] = -(i % 32)                         # . (32 c0, c0) = -c0 i
            q[:, h, d[4]] = 1 + (i + h) % 7                                                   # against zeros of K: a wrong dim shows
        elif name == "spike":
            o = (7 * i + 3 + h) % 16                                                         # the offset inside the 16-group, another for every row and head
            for r in range(S):
                q[r, h, (d[5] // 16) * 16 + o[r]] = SPIKE[hd][0]
        else:                                                                                 # uniform: K = 0, any Q
            q[:, h, :] = wide(hash_w(S, hd, seed + 7 + h)).astype(np.float64)
    for g in range(KVH):
        d = _dims(hd, g, 6)
        if name in ("rising", "falling", "per_head"):
            k[:, g, d[0]] = j // 32; k[:, g, d[1]] = j % 32
            if name == "rising":
                k[:, g, d[2]] = 32 * c0; k[:, g, d[3]] = c0
            k[:, g, d[5]] = 1 + (j + g) % 5                                                   # against zeros of Q
        elif name == "spike":
            grp = (T // 2) // 16                                                              # a middle 16-group
            base = (d[5] // 16) * 16
            for jj in range(16 * grp, min(16 * grp + 16, T)):
                k[jj, g, base + jj % 16] = SPIKE[hd][1]
    if name == "uniform":
        v = np.zeros((T, KVH, hd), dtype=np.uint16)
        v[j, :, j % hd] = ONE
    return dict(q=exact_bf(q) if name != "uniform" else bf(q.astype(np.float32)), k=exact_bf(k), v=v, S=S, start_pos=start_pos, T=T, hd=hd, H=H, KVH=KVH, name=name, geometry=geometry)


def scores(c, kvh_of=None):
    """raw scores f64 [H, S, T] (integers: exact in f32 in any order -- asserted), and the visible mask of the reference: (j mod S) <= i for S > 1"""
    H, KVH, S, T = c["H"], c["KVH"], c["S"], c["T"]
    kv = (np.arange(H) // (H // KVH)) if kvh_of is None else kvh_of
    q, k = wide(c["q"]).astype(np.float64), wide(c["k"]).astype(np.float64)
    s = np.einsum("ihd,jhd->hij", q, k[:, kv, :])
    mag = np.einsum("ihd,jhd->hij", np.abs(q), np.abs(k[:, kv, :]))
    assert (2 * mag < 2.0 ** 24).all() and (c["name"] == "uniform" or (2 * s == np.round(2 * s)).all())       # (halves: the slopes 5.5 and 16.5 of per_head at head_dim 128)
    i = np.arange(S)[:, None]; j = np.arange(T)[None, :]
    visible = (j % S <= i) if S > 1 else np.ones((S, T), dtype=bool)
    return s, visible, kv


def softmax_f64(c):
    """(out f64 [S, H, hd], A = sum_j p_j |v_jd|): the f64 softmax of the same bf16 inputs under the reference's mask"""
    s, visible, kv = scores(c)
    z = np.where(visible[None], s / divisor(c["hd"]), -np.inf)
    p = np.exp(z - z.max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    v = wide(c["v"]).astype(np.float64)[:, kv, :]             # [T, H, hd]
    out = np.einsum("hij,jhd->ihd", p, v)
    A = np.einsum("hij,jhd->ihd", p, np.abs(v))
    return out, A


def bound(ref, A):
    """|got - ref| <= 2^-7 |ref| + (2^-7 + 2^-10) A + 2^-126: the truncation of the output, the one-sided truncation of p, and 2^-10 for everything f32 (the scale
    multiply, exp2 within an ulp, ~600 accumulations, 1 / l and the multiply)"""
    return 2.0 ** -7 * np.abs(ref) + (2.0 ** -7 + 2.0 ** -10) * A + 2.0 ** -126


DEFECTS = ("mask_plus_one", "mask_minus_one", "tile_dropped", "v_positions_exchanged", "alpha_one", "kvh_modulo")


def flash_model(c, defect=None):
    """fast_attn_prefill_kernel in f32 numpy: tiles of 32 positions, scores * (log2 e / divisor) in f32, running maximum and sum, p = exp2(s - m), l from the
    untruncated p, p truncated to bf16 for PV, O and l rescaled by alpha, out = trunc(O * (1 / l)) -> uint16 [S, H, hd].
    defect: the mask one position wider / narrower, the second-to-last tile skipped, two positions of a 16-group exchanged in V only, alpha = 1, kvh = h % KVH"""
    H, KVH, S, T, hd = c["H"], c["KVH"], c["S"], c["T"], c["hd"]
    kvh_of = (np.arange(H) % KVH) if defect == "kvh_modulo" else None
    s, visible, kv = scores(c, kvh_of)
    i = np.arange(S)[:, None]; j = np.arange(T)[None, :]
    if defect == "mask_plus_one":
        visible = (j % S <= i + 1) if c["start_pos"] else (j <= i + 1)
    if defect == "mask_minus_one":
        visible = (j % S < i) | (j == 0) if c["start_pos"] == 0 else (j % S < i) | (j % S == 0)
    scale = np.float32(np.float32(1.4426950408889634) / np.float32(divisor(hd)))
    t = np.where(visible[None], s.astype(np.float32) * scale, np.float32(-np.inf)).astype(np.float32)
    v = wide(c["v"])[:, kv, :].copy()                        # [T, H, hd] f32
    if defect == "v_positions_exchanged":
        a = (T // 2) // 16 * 16 + 5
        if a + 1 < T:
            v[[a, a + 1]] = v[[a + 1, a]]
    m = np.full((H, S), -np.inf, dtype=np.float32); l = np.zeros((H, S), dtype=np.float32)
    o = np.zeros((H, S, hd), dtype=np.float32)
    ntiles = (T + 31) // 32
    with np.errstate(all="ignore"):
        for jt in range(ntiles):
            if defect == "tile_dropped" and ntiles > 1 and jt == max(ntiles - 2, 0):
                continue
            tt = t[:, :, 32 * jt:32 * jt + 32]
            mn = np.maximum(m, tt.max(axis=2))
            msafe = np.where(np.isneginf(mn), np.float32(0), mn)
            alpha = np.exp2(m - msafe).astype(np.float32) if defect != "alpha_one" else np.ones_like(m)
            p = np.exp2(tt - msafe[:, :, None]).astype(np.float32)
            l = (l * alpha + p.sum(axis=2, dtype=np.float32)).astype(np.float32)
            pb = wide(bf(p))
            o = (o * alpha[:, :, None] + np.einsum("hij,jhd->hid", pb, v[32 * jt:32 * jt + 32]).astype(np.float32)).astype(np.float32)
            m = mn
        out = o * (np.float32(1) / l)[:, :, None]
    return bf(out.astype(np.float32)).transpose(1, 0, 2)


def defect_applies(defect, c):
    """the calls on which a defect is something else than the correct kernel"""
    ntiles = (c["T"] + 31) // 32
    return {"tile_dropped": ntiles > 1, "alpha_one": ntiles > 1, "kvh_modulo": c["H"] // c["KVH"] > 1 and c["KVH"] > 1}.get(defect, True)


def cache_rows(c, capacity, tail=QNAN):
    """K, V [capacity, KVH, hd] for kv_craft.blob: the set's rows, then `tail` in every row from T on"""
    K = np.full((capacity, c["KVH"], c["hd"]), tail, dtype=np.uint16); V = K.copy()
    K[:c["T"]], V[:c["T"]] = c["k"], c["v"]
    return K, V
