"""Hand-made inputs for the three epilogues that follow a product (tests/test_op_crafted_cpu.py, tests/test_gpu_op_crafted.py): EPI_RESID (wo and w2: the
reference's ml.Add), EPI_SILU_MUL (w1|w3: SiLU table lookup times up) and EPI_QKV_ROPE (wq|wk|wv: RoPE and the KV append).  numpy and the oracle's operator
functions only, no GPU code: the value sets, the weight recipes, the references, and the wrong epilogues the CPU test proves visible.

A stage made by lnb_model_create_parts holds a single third of a block, lnb_ctx_hidden_ptr exposes its input and output, so any bf16 pattern can be put in
front of a part and read behind it.  The stage is block LAYER of a three-block model: neither the first stage (which wants tokens) nor the last.

How a value reaches an epilogue
  selector row   w[n] is one-hot at column k1(n): the product reproduces x[k1] times that weight exactly;
  two-hot row    w[n] has a second weight at k2(n): acc = p1 + p2 in f32 -- a subnormal as the difference of two normal products, +-inf as a sum that overflows,
                 an accumulator with bits below bf16;  split() makes the pair for a target;
  -0             a chain starts at +0 and +0 + (-0) = +0, so a product can only give -0 by underflow of the truncation: p1 + p2 = -2^-140 (two normal products
                 with 16-bit significands) is 0x80000200 in f32 and 0x8000 in bf16 (neg_zero_rows);
  beside them, gaussian rows and gaussian columns (weights where the activations are zero, activations where the weights are zero): no launch is degenerate.
The fused norm: a row of h whose elements all have the magnitude c gives trunc(x * r) = +-0x3F7F (r a little below 1 / c, c in 0.5 .. 4), and a norm weight of
0x3F81 then gives exactly +-1.0 (0x3F82: +-0x3F81, one of the two factors of the -0 recipe).  So every product of a selector row is the weight itself, in every row.

The matrix-core products (16 rows and more) FUSE the multiply: their bits are the reference's while every single product is a normal f32, a zero or a NaN
(tests/linear_cases.py, NOTES.md section 2).  The `exact` recipes (1 to 15 rows) put subnormals, infinities and NaNs straight into the weights; the others reach
them through two-hot rows and give a NaN a row of h of its own."""
import ctypes as C

import numpy as np

import form_cases as fc
from oracle import oracle as orc

EPS = np.float32(1e-5)
LAYER = 1                                     # the block the part stages hold
ONE, MAXF, MINN = 0x3F80, 0x7F7F, 0x0080      # 1.0, the largest finite bf16, the smallest normal one
QNAN = 0x7FC0
_SMALL = dict(n_layers=3, vocab_size=64, max_seq_len=64)        # 128 cis rows
GEOS = {
    "tiny": dict(orc.TINY, **_SMALL),                                        # dim 256, 4 heads of 64 on 2 KV heads, FFN hidden 896
    "odd192": dict(fc.GEOS["odd192"], **_SMALL),                             # dim 192, FFN hidden 704: no K a multiple of 128
    "wide1024": dict(fc.GEOS["wide1024"], **_SMALL),                         # dim 1024, heads of 128, FFN hidden 3584: K = whole rowcast_lds_kernel stages
    "hd32": dict(orc.TINY, n_heads=8, n_kv_heads=2, **_SMALL),               # heads of 32 (RoPE only)
}


def bf(a):
    return orc.f32_to_bf16(np.asarray(a, dtype=np.float32)).reshape(np.shape(a))


def wide(a):
    return orc.bf16_to_f32(a).reshape(np.shape(a))


def shape_of(geo):
    cfg = GEOS[geo]
    hd = cfg["dim"] // cfg["n_heads"]
    F = orc.lib().orc_ffn_hidden_dim(C.byref(orc.make_args(**cfg)))
    return dict(dim=cfg["dim"], F=F, H=cfg["n_heads"], KVH=cfg["n_kv_heads"], hd=hd, q_dim=cfg["n_heads"] * hd, kv_dim=cfg["n_kv_heads"] * hd,
                cis_rows=2 * cfg["max_seq_len"])


def is_nan(p):
    p = np.asarray(p)
    return ((p & 0x7F80) == 0x7F80) & ((p & 0x7F) != 0)


def is_sub(p):
    p = np.asarray(p)
    return ((p & 0x7F80) == 0) & ((p & 0x7F) != 0)


def same_or_both_nan(a, b):
    """the comparison of every test here: all 16 bits, except where the reference (b) is NaN -- there NaN-ness"""
    a = np.ascontiguousarray(a, dtype=np.uint16); b = np.ascontiguousarray(b, dtype=np.uint16)
    return (a == b) | (is_nan(a) & is_nan(b))


def nan_fraction(ref):
    return float(is_nan(ref).mean())


MAX_NAN_FRACTION = 1.0 / 8.0


# ---- the oracle's operators -------------------------------------------------------------------------------------------------------------------------
def linear(x, w):
    x = np.ascontiguousarray(x, dtype=np.uint16); w = np.ascontiguousarray(w, dtype=np.uint16)
    y = np.zeros((x.shape[0], w.shape[0]), dtype=np.uint16)
    orc.lib().orc_linear_bf16(orc._p(x), orc._p(w), orc._p(y), x.shape[0], w.shape[0], x.shape[1], 8)
    return y


def linear_acc(x, w):
    """the f32 accumulators in front of the truncation (orc_linear_f32: the same chain, k ascending) -- for the wrong epilogues only"""
    xf = np.ascontiguousarray(wide(x)); wf = np.ascontiguousarray(wide(w))
    acc = np.zeros((xf.shape[0], wf.shape[0]), dtype=np.float32)
    orc.lib().orc_linear_f32(orc._p(xf), orc._p(wf), orc._p(acc), None, xf.shape[0], wf.shape[0], xf.shape[1])
    return acc


def rmsnorm(h, nw):
    h = np.ascontiguousarray(h, dtype=np.uint16); nw = np.ascontiguousarray(nw, dtype=np.uint16)
    y = np.zeros_like(h)
    orc.lib().orc_rmsnorm_bf16(orc._p(h), orc._p(nw), orc._p(y), h.shape[0], h.shape[1], EPS, None)
    return y


def silu_table():
    return np.ctypeslib.as_array(orc.lib().orc_silu_table(), shape=(1 << 16,))


_CIS = {}


def cis_table(geo):
    """the oracle's cis rows [2 * max_seq_len, head_dim / 2, 2] f32"""
    if geo not in _CIS:
        cfg, s = GEOS[geo], shape_of(geo)
        cis = np.zeros((s["cis_rows"], s["hd"] // 2, 2), dtype=np.float32)
        orc.lib().orc_rope_table(s["hd"], s["cis_rows"], C.c_double(cfg["rope_theta"]), cfg["use_scaled_rope"], orc._p(cis), None)
        _CIS[geo] = cis
    return _CIS[geo]


def rope(x, n_heads, hd, cis_rows):
    """orc_rope_apply on a copy: x [S, n_heads * hd], cis_rows [S, hd / 2, 2] -- the rows of the call's positions"""
    y = np.ascontiguousarray(x, dtype=np.uint16).copy()
    c = np.ascontiguousarray(cis_rows, dtype=np.float32)
    assert c.shape == (y.shape[0], hd // 2, 2)
    orc.lib().orc_rope_apply(orc._p(y), y.shape[0], n_heads, hd, orc._p(c))
    return y


# ---- the references: plain compositions of the oracle's operators ---------------------------------------------------------------------------------------
def add_ref(res, y):
    """ml.Add: trunc(f32(res) + f32(y))"""
    with np.errstate(all="ignore"):
        return bf(wide(res) + wide(y))


def down_ref(c):
    """w2 + residual -> dict(y, out)"""
    y = linear(c["act"], c["w2"])
    return dict(y=y, out=add_ref(c["h"], y))


def silu_mul_ref(g, u):
    gs = bf(silu_table()[g])
    with np.errstate(all="ignore"):
        return gs, bf(wide(gs) * wide(u))


def gate_up_ref(c):
    """ffn_norm, w1 and w3, SiLU * up -> dict(xn, g, u, gs, out)"""
    xn = rmsnorm(c["h"], c["nw"])
    g, u = linear(xn, c["w1"]), linear(xn, c["w3"])
    gs, out = silu_mul_ref(g, u)
    return dict(xn=xn, g=g, u=u, gs=gs, out=out)


def kv_ref(c):
    """attention_norm, wk and wv, RoPE at the call's positions -> dict(xn, xk, xv, xk_rope)"""
    s = shape_of(c["geo"])
    xn = rmsnorm(c["h"], c["nw"])
    xk, xv = linear(xn, c["wk"]), linear(xn, c["wv"])
    cis = cis_table(c["geo"])[c["start_pos"]:c["start_pos"] + xk.shape[0]]
    return dict(xn=xn, xk=xk, xv=xv, xk_rope=rope(xk, s["KVH"], s["hd"], cis))


# ---- the value set of the residual grid -------------------------------------------------------------------------------------------------------------------
NANS = (0x7FC0, 0xFFC0, 0x7F81, 0xFFA5, 0x7FFF, 0xFFFF, 0x7FC1, 0xFFE0)     # both signs; 0x7F81 and 0xFFA5 are signalling (bit 6 clear)


def value_set():
    """256 bf16 patterns: +-0, +-inf, eight NaNs, subnormals, the smallest and largest normals, +-1 and its neighbours, powers of two over the whole exponent
    range, seeded random finite patterns for the rest"""
    v = [0x0000, 0x8000, 0x7F80, 0xFF80] + list(NANS)
    v += [0x0001, 0x8001, 0x007F, 0x807F, 0x0040, 0x8040, 0x0013, 0x8055]
    v += [MINN, 0x8000 | MINN, MAXF, 0x8000 | MAXF, ONE, 0xBF80, 0x3F7F, 0xBF7F, 0x3F81, 0xBF81]
    for ef in range(2, 254, 6):
        v += [ef << 7, 0x8000 | (ef << 7)]
    rng = np.random.default_rng(256)
    while len(v) < 256:
        p = int(rng.integers(0, 1 << 16))
        if (p & 0x7F80) != 0x7F80 and p not in v:
            v.append(p)
    assert len(set(v)) == 256
    return np.array(v, dtype=np.uint16)


V = value_set()


def split(y):
    """(a1, a2), two bf16 patterns whose f32 sum truncates to y -- neither of them subnormal or infinite.  A normal y or a zero: (y, +0) (-0 comes out as +0:
    see the module docstring); a subnormal j * 2^-133: 2^-126 * (1 + j / 128) - 2^-126; +-inf: the largest finite value twice; a NaN: (y, +0)."""
    y = np.asarray(y, dtype=np.uint16)
    sign, man = y & 0x8000, y & 0x7F
    a1, a2 = y.copy(), np.zeros_like(y)
    sub, inf = is_sub(y), (y & 0x7FFF) == 0x7F80
    a1 = np.where(sub, sign | MINN | man, a1); a2 = np.where(sub, (sign ^ 0x8000) | MINN, a2)
    a1 = np.where(inf, sign | MAXF, a1); a2 = np.where(inf, sign | MAXF, a2)
    return a1.astype(np.uint16), a2.astype(np.uint16)


def _finite_random(rng, shape, ef_lo=1, ef_hi=254):
    return ((rng.integers(0, 2, shape) << 15) | (rng.integers(ef_lo, ef_hi + 1, shape) << 7) | rng.integers(0, 128, shape)).astype(np.uint16)


def _gauss(rng, shape, scale):
    return bf(rng.standard_normal(shape) * scale)


# ---- down part: w2 + residual -------------------------------------------------------------------------------------------------------------------------------
# columns of act: [0, 128) first addends, [128, 256) second addends (w2[n] = 1.0 at n % 128 and at 128 + n % 128: y[m, n] = act[m, n % 128] + act[m, 128 + n % 128]),
# then B: gaussian activations under zero weights, then C: zero activations under gaussian weights.  In the mixed sets the last 32 output rows are gaussian over B and C.
SLOTS = 128
FAR_PAIRS = 40
RESID_SETS = [("tiny", r) for r in (1, 2, 7, 15, 16, 17, 83, 256)] + [(g, r) for g in ("odd192", "wide1024") for r in (1, 7, 17, 83)]


def _special_slots(rng):
    """(a1, a2, res of column j, res of column j + 128): what every row of a mixed set carries, whatever the row count"""
    s = [
        (0x0000, 0, 0x8000, 0x0000),                        # (-0) + (+0); (+0) + (+0)
        (ONE, 0, 0xBF80, int(bf(-2.0 ** -30))),             # exact cancellation to +0; 1.0 + (-2^-30) = 0x3F80, not 0x3F7F
        (MAXF, 0, MAXF, 0x8000 | MAXF),                     # a finite sum that overflows; cancellation of the largest value
        (MAXF, MAXF, 0xFF80, ONE),                          # y = +inf (a sum): inf + (-inf); inf + 1
        (0x0081, 0x8080, 0x0000, MINN),                     # y = 0x0001 (a difference of normals): a subnormal result; subnormal + smallest normal
        (0xBF80, 0, int(bf(2.0 ** -20)), 0x3F7F),           # a negative result whose truncation drops set bits
        (ONE, int(bf(2.0 ** -10)), 0xBF80, 0xBF80),         # an accumulator with bits below bf16: trunc(acc) = 1.0 cancels, acc does not
        (MINN, 0, 0x0001, 0x8001),                          # a subnormal residual
        (0x8000 | MAXF, 0x8000 | MAXF, 0x7F80, 0xFF80),     # y = -inf: -inf + inf; -inf + -inf
        (0x0000, 0, 0x0053, 0x8000 | MAXF),                 # +0 + subnormal; +0 + the most negative value
    ]
    for _ in range(FAR_PAIRS):                              # exponents 25 .. 60 apart, opposite signs: RN gives the large value back, the exact sum lies below it
        gap, sg = int(rng.integers(25, 61)), int(rng.integers(0, 2)) << 15
        ef = int(rng.integers(gap + 2, 254))
        big = sg | (ef << 7) | int(rng.integers(0, 128))
        small = (sg ^ 0x8000) | ((ef - gap) << 7) | int(rng.integers(0, 128))
        s.append((big, 0, small, small ^ 0x8000))
    return s


def down_case(geo, rows):
    """dict(geo, rows, act [rows, F], h [rows, dim], w2 [dim, F]); (tiny, 256) is the full grid: row m carries y = V[m] in every slot, column n the residual V[n]"""
    s = shape_of(geo)
    dim, F = s["dim"], s["F"]
    rng = np.random.default_rng([1, sorted(GEOS).index(geo), rows])
    grid = rows == 256
    assert not grid or dim == 256
    rng_w = np.random.default_rng([11, sorted(GEOS).index(geo), grid])       # w2 depends on the geometry and on grid / mixed only: one device model serves every row count
    b0, c0 = 2 * SLOTS, 2 * SLOTS + (F - 2 * SLOTS) // 2
    act = np.zeros((rows, F), dtype=np.uint16)
    act[:, b0:c0] = _gauss(rng, (rows, c0 - b0), 1.0)
    w2 = np.zeros((dim, F), dtype=np.uint16)
    w2[:, c0:] = _gauss(rng_w, (dim, F - c0), 0.05)
    n_sel = dim if grid else dim - 32
    for n in range(n_sel):
        w2[n, n % SLOTS] = ONE; w2[n, SLOTS + n % SLOTS] = ONE
    w2[n_sel:, b0:c0] = _gauss(rng_w, (dim - n_sel, c0 - b0), 0.05)
    if grid:
        a1, a2 = split(V)
        ef = (V >> 7) & 0xFF                                 # every second normal row: a second addend of the same sign nine binades down -- trunc(acc) is still V[m],
        low = (ef >= 12) & (ef < 255) & (np.arange(256) % 2 == 1)            # acc itself has bits below bf16's last one
        a2 = np.where(low, (V & 0x8000) | ((ef - 9) << 7), a2).astype(np.uint16)
        act[:, :SLOTS] = a1[:, None]; act[:, SLOTS:b0] = a2[:, None]
        h = np.broadcast_to(V[None, :], (rows, dim)).copy()
        return dict(geo=geo, rows=rows, act=act, h=h, w2=w2)
    finite = V[~is_nan(V)]
    h = V[rng.integers(0, 256, (rows, dim))]                 # any pattern of V, NaNs among them (8 of 256)
    h[:, n_sel:] = _gauss(rng, (rows, dim - n_sel), 1.0)
    special = _special_slots(rng)
    for m in range(rows):
        a1, a2 = split(finite[rng.integers(0, finite.size, SLOTS)])
        for i, (p1, p2, r0, r1) in enumerate(special):
            j = (i + 11 * m) % SLOTS                         # (another lane and column in every row)
            a1[j], a2[j] = p1, p2
            for n, r in ((j, r0), (j + SLOTS, r1)):
                if n < n_sel:
                    h[m, n] = r
        if rows >= 16 and m % 16 == 5:                       # a NaN y poisons its row through 0 * NaN: a row of its own
            a1[:] = np.array(NANS, dtype=np.uint16)[np.arange(SLOTS) % len(NANS)]; a2[:] = 0
        act[m, :SLOTS], act[m, SLOTS:b0] = a1, a2
    return dict(geo=geo, rows=rows, act=act, h=h, w2=w2)


# ---- the rows of h in front of a fused norm -------------------------------------------------------------------------------------------------------------------
SEL_K = 60                                    # selector columns k1 = n % 60, k2 = 60 + n % 60; columns 120 .. 127 carry xn = 0x3F81 for the -0 recipe
ROW_KINDS = ("+", "-", "g", "+")


def norm_rows(rng, rows, dim, nan_row=True):
    """(h [rows, dim], norm weight [dim], kinds): row m is all +c ("+": xn = +1.0 on the selector columns), all -c ("-"), or half gaussian ("g": random +-1.0 on
    columns [0, 128), gaussians behind them scaled so that the mean square is 1.004 -- r = 0.998, so trunc(+-1.0 * r) is +-0x3F7F there too and xn = +-1.0 on the
    selector columns: a row of mixed signs whose products stay the weights themselves, which the matrix-core limit needs); with 16 rows or more every row
    m = 5 mod 16 has one NaN: a NaN row of its own"""
    kinds = [ROW_KINDS[m % 4] for m in range(rows)]
    h = np.zeros((rows, dim), dtype=np.uint16)
    for m, kd in enumerate(kinds):
        if kd != "g":
            c = (1.0, 2.0, 0.5, 4.0)[(m // 4) % 4]
            h[m, :] = bf(np.float32(c if kd == "+" else -c))
        else:
            g = rng.standard_normal(dim - 128)
            for _ in range(4):                               # (bf16 truncation shrinks every element: scale until the TRUNCATED values have the sum of squares)
                gt = wide(bf(g)).astype(np.float64)
                g *= np.sqrt((1.004012 * dim - 128.0) / (gt @ gt))
            h[m, :128] = bf(rng.choice([-1.0, 1.0], 128)); h[m, 128:] = bf(g)
    if nan_row and rows >= 16:
        for m in range(5, rows, 16):
            h[m, 3] = QNAN
            kinds[m] = "nan"
    nw = bf(1 + 0.1 * rng.standard_normal(dim))
    nw[:120] = 0x3F81
    nw[120:128] = 0x3F82
    return h, nw, kinds


def put(w, n, pattern, exact):
    """make row n of w give `pattern` on a "+" row of h: the pattern itself as the one weight (exact: 1 to 15 rows), or split() over two weights"""
    k1, k2 = n % SEL_K, SEL_K + n % SEL_K
    w[n, :] = 0
    if exact:
        w[n, k1] = pattern
    else:
        assert not is_nan(pattern)
        a1, a2 = split(np.array([pattern], dtype=np.uint16))
        w[n, k1], w[n, k2] = a1[0], a2[0]


def put_neg_zero(w, n):
    """row n gives -0 on a "+" row: xn[0] * 0x0082 = +(1 + 2^-6) 2^-126 first, then xn[120] * 0x8081 = -(1 + 2^-7)^2 2^-126: the sum is -2^-140"""
    w[n, :] = 0
    w[n, 0] = 0x0082; w[n, 120] = 0x8081


# ---- gate/up part: ffn_norm, w1|w3, SiLU * up ------------------------------------------------------------------------------------------------------------------
# variant "exact": 1 to 15 rows, any pattern as a weight; "split": any row count, finite normal weights only; "window": weights within the 30 binades the 13-bit
# planar copy admits (exponent fields 112 .. 141): what gemv_chain_pk_kernel can be given
GATE_UP_SETS = ([("tiny", r, "exact") for r in (1, 2, 7, 15)] + [("tiny", r, "split") for r in (1, 16, 17, 83)] + [("tiny", r, "window") for r in (1, 7)] +
                [(g, r, v) for g in ("odd192", "wide1024") for r, v in ((1, "exact"), (7, "exact"), (17, "split"))])
N_GAUSS_ROWS = 128


def most_negative_normal_gate():
    """the most negative bf16 gate whose table entry is still a normal f32"""
    t = silu_table()
    neg = np.arange(0x8080, 0xFF80, dtype=np.uint32).astype(np.uint16)       # negative normals, ascending magnitude
    ok = np.abs(t[neg]) >= np.float32(2.0 ** -126)
    return int(neg[ok][-1])


def gate_up_targets(rng, n_sel, variant):
    """(G, U, rows of the -0 recipe): the gate and up patterns of output rows [0, n_sel) on a "+" row"""
    lo, hi = (112, 141) if variant == "window" else (1, 254)
    G, U = _finite_random(rng, n_sel, lo, hi), _finite_random(rng, n_sel, max(lo, 100), min(hi, 150))
    neg0 = []
    if variant != "window":
        n = np.arange(min(512, n_sel))
        ef = n >> 1                                          # every (sign, exponent field): +-0, subnormals, ..., +-inf
        man = np.where((ef == 255) | (n < 2), 0, np.maximum(G[:n.size] & 0x7F, 1))
        G[:n.size] = ((n & 1) << 15) | (ef << 7) | man
    edge = most_negative_normal_gate()
    pairs = [(0x0000, 0x7F80), (ONE, 0x0000), (0x4000, 0x0005), (0x4040, 0x7F80), (0xC040, 0xFF80), (0x7F80, 0x0000), (0xFF80, ONE), (0x7F80, 0x7F80),
             (int(bf(1.3 * 2.0 ** -60)), int(bf(1.7 * 2.0 ** -70))), (int(bf(2.0 ** 100)), int(bf(2.0 ** 100))), (int(bf(2.0 ** 100)), int(bf(-2.0 ** 100))),
             (edge, ONE), (edge, int(bf(2.0 ** 100))), (edge + 1, ONE), (edge + 1, int(bf(2.0 ** 100))), (edge - 1, ONE), (0x0001, ONE), (0x8001, 0x4000),
             (ONE, 0x8003), (0x0000, 0x0000), (0x3FC0, 0x0001)]
    if variant == "exact":
        pairs += [(0x7FC0, ONE), (0xFFC0, ONE), (0x7F81, ONE), (ONE, 0x7FC0), (0x4000, 0xFFC1), (0x0000, 0xFF80)]
    if variant == "window":
        pairs = [(int(bf(-90.0)), ONE), (int(bf(-90.0)), int(bf(0.125))), (int(bf(-13.5)), ONE), (int(bf(-16384.0)), int(bf(16384.0))), (int(bf(2.0 ** -15)), int(bf(2.0 ** -15))), (int(bf(16384.0)), int(bf(-16384.0))),
                 (0x0000, ONE), (ONE, 0x0000)]
    base = n_sel - len(pairs) - 4
    assert base >= (512 if variant != "window" else 0)
    for i, (g, u) in enumerate(pairs):
        G[base + i], U[base + i] = g, u
    if variant != "window":
        neg0 = [n_sel - 4, n_sel - 3]                        # gate -0 against up +1.0 and -1.0
        U[n_sel - 4], U[n_sel - 3] = ONE, 0xBF80
        G[n_sel - 2], U[n_sel - 2] = ONE, 0x8000             # (gate 1.0 against up -0: the rows of neg0_up)
    return G, U, neg0


def gate_up_case(geo, rows, variant):
    """dict(geo, rows, variant, h, nw, w1, w3, kinds)"""
    s = shape_of(geo)
    dim, F = s["dim"], s["F"]
    rng_h = np.random.default_rng([2, sorted(GEOS).index(geo), rows, ("exact", "split", "window").index(variant)])
    rng = np.random.default_rng([12, sorted(GEOS).index(geo), ("exact", "split", "window").index(variant)])          # the weights (and the norm weight): per (geometry, variant)
    h, _, kinds = norm_rows(rng_h, rows, dim)
    _, nw, _ = norm_rows(rng, 1, dim)
    n_sel = F - N_GAUSS_ROWS
    if variant == "window":
        w1, w3 = _finite_random(rng, (F, dim), 112, 141), _finite_random(rng, (F, dim), 112, 141)
        w1[n_sel:] = (w1[n_sel:] & 0x807F) | (rng.integers(112, 122, (N_GAUSS_ROWS, dim)) << 7).astype(np.uint16)     # (2^-15 .. 2^-6: no sum overflows)
        w3[n_sel:] = (w3[n_sel:] & 0x807F) | (rng.integers(112, 122, (N_GAUSS_ROWS, dim)) << 7).astype(np.uint16)
    else:
        w1, w3 = _gauss(rng, (F, dim), 0.05), _gauss(rng, (F, dim), 0.05)
    G, U, neg0 = gate_up_targets(rng, n_sel, variant)
    for n in range(n_sel):
        put(w1, n, G[n], variant != "split"); put(w3, n, U[n], variant != "split")
    for n in neg0:
        put_neg_zero(w1, n)
    if variant != "window":
        put_neg_zero(w3, n_sel - 2)
    return dict(geo=geo, rows=rows, variant=variant, h=h, nw=nw, w1=w1, w3=w3, kinds=kinds)


def wpack_expect(w1, w3):
    """what lnb_wpack.h's window rule says of the gate|up pair, restated: 0 packable, 1 a subnormal or an exponent of 1, 2 inf / NaN, 3 too many binades"""
    w = np.concatenate([w1.ravel(), w3.ravel()])
    ef = (w >> 7) & 0xFF
    if ((ef < 2) & ((w & 0x7FFF) != 0)).any():
        return 1
    if (ef == 255).any():
        return 2
    e2 = (ef >> 1)[(ef >= 2)]
    return 0 if e2.size == 0 or int(e2.max()) - (int(e2.min()) - 1) <= 15 else 3


# ---- attention part: attention_norm, wq|wk|wv, RoPE, KV append -----------------------------------------------------------------------------------------------------
# (geometry, capacity of the context, start position, rows, variant): positions 0 and 1, the last position of a 37-position context (the K layout
# [kv head][hd / 8][position][8] has no padding to land in), the last cis row 2 * max_seq_len - 1 = 127 in a context that long; a multi-row call needs
# (start + rows) % rows == 0.  "finite" sets keep every K and V row finite (the attention behind them is compared too); "nonfinite" sets hold the overflow, inf
# and NaN pairs and live in contexts of their own: a non-finite row sets the context's sticky word.
ROPE_SETS = [
    ("tiny", 37, 0, 1, "finite"), ("tiny", 37, 0, 1, "nonfinite"), ("tiny", 37, 36, 1, "finite"), ("tiny", 37, 36, 1, "nonfinite"), ("tiny", 128, 0, 2, "finite"),
    ("tiny", 128, 0, 2, "nonfinite"), ("tiny", 128, 127, 1, "finite"), ("tiny", 128, 127, 1, "nonfinite"), ("tiny", 37, 28, 7, "finite"), ("tiny", 128, 15, 15, "finite"),
    ("tiny", 128, 16, 16, "finite"), ("tiny", 128, 112, 16, "finite"), ("tiny", 128, 17, 17, "finite"), ("tiny", 128, 0, 83, "finite"), ("tiny", 128, 0, 17, "nonfinite"),
    ("wide1024", 37, 36, 1, "finite"), ("wide1024", 128, 0, 2, "finite"), ("wide1024", 128, 127, 1, "nonfinite"), ("wide1024", 128, 16, 16, "finite"),
    ("wide1024", 37, 0, 1, "nonfinite"), ("wide1024", 37, 0, 1, "finite"), ("odd192", 37, 0, 1, "finite"),
    ("hd32", 37, 36, 1, "finite"), ("hd32", 128, 0, 2, "nonfinite"), ("hd32", 128, 127, 1, "finite"), ("hd32", 128, 17, 17, "finite"),
    ("odd192", 128, 0, 2, "nonfinite"), ("odd192", 128, 16, 16, "finite"), ("odd192", 128, 127, 1, "finite"),
]
N_CANCEL = 8


def cancel_pair(cr, ci):
    """(relative difference, a, b): the bf16 patterns a = m_i / 128, b = m_j / 128 * 2^k for which a * cr and b * ci come closest (the real part a * cr - b * ci
    cancels); None at cr = 0 or ci = 0"""
    cr, ci = float(cr), float(ci)
    if cr == 0.0 or ci == 0.0:
        return None
    t = abs(cr / ci)                                         # b / a
    m = np.arange(128, 256, dtype=np.float64)
    R = m[None, :] / m[:, None]                              # R[i, j] = m_j / m_i
    e = int(np.floor(np.log2(t)))
    best = None
    for k in (e - 1, e, e + 1):
        if not -100 < k < 100:
            continue
        err = np.abs(R * 2.0 ** k - t) / t
        i, j = np.unravel_index(np.argmin(err), err.shape)
        if best is None or err[i, j] < best[0]:
            a = int(bf(np.float32(m[i] / 128.0))); b = int(bf(np.float32(m[j] / 128.0 * 2.0 ** k)))
            best = (float(err[i, j]), a, b ^ 0x8000 if (cr > 0) != (ci > 0) else b)
    return best


def rope_targets(rng, geo, positions, kinds, variant, exact):
    """(Kt [kv_dim], Vt [kv_dim], rows of the -0 recipe in wk): the xk and xv patterns on a "+" row.  Pair i of head k is (Kt[k * hd + 2i], Kt[k * hd + 2i + 1])."""
    s = shape_of(geo)
    kvd, hd = s["kv_dim"], s["hd"]
    cis = cis_table(geo)
    Kt, Vt = _finite_random(rng, kvd, 100, 126), _finite_random(rng, kvd, 100, 140)          # (|K| < 1: scores of a few units behind them)
    Vt[:16] = [0x0000, 0x0001, 0x8001, 0x007F, MINN, 0x8000 | MINN, ONE, 0xBF80, 0x3F7F, 0x3F81, 0x0040, 0x8040, 0x0013, 0x0000, 0x0002, 0x8003]
    pairs = [(0x0000, 0x0000), (0x0000, int(bf(1.5 * 2.0 ** -120))), (MINN | 0x33, 0x0000), (MINN, MINN), (0x0003, 0x8005), (int(bf(2.0 ** -124)), int(bf(-2.0 ** -124))),
             ("-0", 0x0000), (0x0000, "-0"), ("-0", "-0"), (0x0001, ONE), (ONE, 0x8001)]
    if variant == "nonfinite":                              # in front: the low pair indices turn by about the position itself (cr + ci > 1 somewhere)
        pairs = [(MAXF, 0x8000 | MAXF), (MAXF, MAXF), (0x3F80, 0x7F80), (0xFF80, 0x4000), (int(bf(2.0 ** 126)), int(bf(2.0 ** 126)))] + pairs
        if exact:
            pairs += [(0x7FC0, ONE), (0x4000, 0xFFC1), (0x7F81, 0x0000)]
        Vt[16:22] = [0x7F80, 0xFF80, MAXF, 0x8000 | MAXF, 0x7F00, 0xFF00]
        if exact:
            Vt[22:24] = [0x7FC0, 0xFFA5]
    # the cancelling pairs: made for the cis row of one position each, a "+" or "-" row's (both halves keep their relative sign there)
    cand = []
    for p, kd in zip(positions, kinds):
        if kd in "+-":
            for i in range(hd // 2):
                ab = cancel_pair(cis[p, i, 0], cis[p, i, 1])
                if ab is not None:
                    cand.append((ab[0], i, ab[1:]))
    # one per pair index: the N_CANCEL - 2 closest that do not cancel EXACTLY (at a small angle cr = 1.0 and ci has eight significant bits: a * cr == b * ci, and every
    # arithmetic gives +0 there), then two that do
    found = []
    for want_exact, n in ((False, N_CANCEL - 2), (True, N_CANCEL)):
        for err, i, ab in sorted(cand):
            if len(found) < n and (err == 0.0) == want_exact and all(i != f[0] for f in found):
                found.append((i, ab))
    neg0 = []
    for i, ab in found:                                       # head 0, pair i
        Kt[2 * i], Kt[2 * i + 1] = ab
    free = [i for i in range(hd // 2) if all(i != f[0] for f in found)]
    # the other specials: the last head's pairs, and the first head's free ones
    slots = [(s["KVH"] - 1) * hd + 2 * i for i in range(hd // 2)] + [2 * i for i in free]
    for (a, b), n in zip(pairs, slots):
        for q, v in ((n, a), (n + 1, b)):
            if v == "-0":
                neg0.append(q); Kt[q] = 0x8000
            else:
                Kt[q] = v
    assert len(pairs) <= len(slots)
    return Kt, Vt, neg0


def wo_selects(start_pos, rows, variant):
    return rows == 1 and start_pos == 0 and variant == "finite"


def attn_case(geo, capacity, start_pos, rows, variant):
    """dict(geo, capacity, start_pos, rows, variant, h, nw, wq, wk, wv, wo, kinds, prefix_k, prefix_v): prefix_* are the finite gaussian rows [0, start_pos) the
    context holds before the call"""
    s = shape_of(geo)
    dim, kvd = s["dim"], s["kv_dim"]
    assert (start_pos + rows) % rows == 0 and start_pos + rows <= min(capacity, s["cis_rows"])
    rng = np.random.default_rng([3, sorted(GEOS).index(geo), capacity, start_pos, rows, variant == "finite"])
    exact = rows < 16
    h, nw, kinds = norm_rows(rng, rows, dim, nan_row=variant == "nonfinite")
    wq, wo = _gauss(rng, (s["q_dim"], dim), 0.05), _gauss(rng, (dim, s["q_dim"]), 0.05)
    wk, wv = _gauss(rng, (kvd, dim), 0.05), _gauss(rng, (kvd, dim), 0.05)
    Kt, Vt, neg0 = rope_targets(rng, geo, list(range(start_pos, start_pos + rows)), kinds, variant, exact)
    if wo_selects(start_pos, rows, variant):
        # one row at position 0: p = 1.0 and the attention output is the V row itself, so a wo of selector rows (y[n] = att[n % q_dim]) puts the V patterns -- -1.0
        # against h = +1.0, values 30 binades below it, subnormals, the largest finite ones -- into wo's residual epilogue
        fin = V[(V & 0x7F80) != 0x7F80]
        Vt = fin[(np.arange(kvd) * 5) % fin.size]
        Vt[:8] = [0xBF80, int(bf(-2.0 ** -30)), MAXF, 0x8000 | MAXF, 0x0001, 0x8001, MINN, int(bf(2.0 ** -40))]
        wo[:] = 0
        wo[np.arange(dim), np.arange(dim) % s["q_dim"]] = ONE
    for n in range(kvd):
        put(wk, n, Kt[n], exact); put(wv, n, Vt[n], exact)
    for n in neg0:
        put_neg_zero(wk, n)
    pk = _gauss(rng, (start_pos, s["KVH"], s["hd"]), 0.5); pv = _gauss(rng, (start_pos, s["KVH"], s["hd"]), 0.3)
    return dict(geo=geo, capacity=capacity, start_pos=start_pos, rows=rows, variant=variant, h=h, nw=nw, wq=wq, wk=wk, wv=wv, wo=wo, kinds=kinds,
                prefix_k=pk, prefix_v=pv)


# ---- the oracle's whole forward on a model that carries crafted weights ----------------------------------------------------------------------------------------
def oracle_block(geo, rows_h, start_pos=0, capacity=None, tensors=None, prefix=None, seed=77):
    """orc_forward on a ONE-block model of the geometry whose tok_embeddings rows are `rows_h` (token m = row m) and whose block tensors are `tensors` ({suffix:
    array}, the rest synthetic) -> (dumps, (K rows, V rows) of the whole context)"""
    rows = rows_h.shape[0]
    cfg = dict(GEOS[geo], n_layers=1, vocab_size=max(rows, 16))
    om = orc.Model(**cfg).fill_synthetic(seed)
    emb = om.get_tensor("tok_embeddings.weight").reshape(cfg["vocab_size"], cfg["dim"]).copy()
    emb[:rows] = rows_h
    om.set_tensor("tok_embeddings.weight", emb)
    for suffix, a in (tensors or {}).items():
        om.set_tensor("layers.0.%s.weight" % suffix, a)
    om.finalize()
    oc = orc.Context(om, capacity or (start_pos + rows))
    if prefix is not None and start_pos:
        oc.cache(0, 0)[:start_pos] = prefix[0]; oc.cache(0, 1)[:start_pos] = prefix[1]
    dumps = oc.capture()
    oc.forward(np.arange(rows, dtype=np.int32), start_pos, want_logits=False)
    kv = (oc.cache(0, 0).copy(), oc.cache(0, 1).copy())
    weights = {n.split(".", 2)[2][:-7]: om.get_tensor(n).copy() for n in om.tensor_names() if n.startswith("layers.0.")}
    oc.close(); om.close()
    return dumps, kv, weights


def attn_oracle(c):
    return oracle_block(c["geo"], c["h"], c["start_pos"], c["capacity"], {"attention_norm": c["nw"], "attention.wq": c["wq"], "attention.wk": c["wk"],
                                                                          "attention.wv": c["wv"], "attention.wo": c["wo"]}, (c["prefix_k"], c["prefix_v"]))


# ---- the wrong epilogues (tests/test_op_crafted_cpu.py shows that each changes a finite output of every case set) --------------------------------------------------
def _ftz32(x):
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.abs(x) < np.float32(2.0 ** -126), np.copysign(np.float32(0), x), x).astype(np.float32)


def rope_np(xk, n_heads, hd, cis_rows, defect=None, next_rows=None):
    """orc_rope_apply restated in numpy: x [S, n_heads * hd] uint16.  defect: None, "f32", "ci_sign", "next_row" (next_rows = the cis rows of position + 1),
    "partner_xor2", "ftz" """
    S = xk.shape[0]
    x = np.ascontiguousarray(xk, dtype=np.uint16).reshape(S, n_heads, hd // 2, 2)
    c = np.asarray(next_rows if defect == "next_row" else cis_rows, dtype=np.float32)[:, None, :, :]
    a16, b16 = x[..., 0], x[..., 1]
    if defect == "partner_xor2":                             # the partner of element n taken from n ^ 2: the other pair's element of the same parity
        flat = x.reshape(S, n_heads, hd)
        part = flat[..., np.arange(hd) ^ 2].reshape(S, n_heads, hd // 2, 2)
        with np.errstate(all="ignore"):
            cr, ci = c[..., 0].astype(np.float64), c[..., 1].astype(np.float64)
            re = (wide(a16).astype(np.float64) * cr - wide(part[..., 0]).astype(np.float64) * ci).astype(np.float32)
            im = (wide(part[..., 1]).astype(np.float64) * ci + wide(b16).astype(np.float64) * cr).astype(np.float32)
        return np.stack([bf(re), bf(im)], axis=-1).reshape(S, n_heads * hd)
    a, b = wide(a16), wide(b16)
    cr, ci = c[..., 0], c[..., 1]
    if defect == "ftz":
        a, b = _ftz32(a), _ftz32(b)
    ty = np.float32 if defect == "f32" else np.float64
    a, b, cr, ci = a.astype(ty), b.astype(ty), cr.astype(ty), ci.astype(ty)
    with np.errstate(all="ignore"):
        re = (a * cr - b * ci).astype(np.float32)
        im = (a * (-ci if defect == "ci_sign" else ci) + b * cr).astype(np.float32)
    if defect == "ftz":
        re, im = _ftz32(re), _ftz32(im)
    return np.stack([bf(re), bf(im)], axis=-1).reshape(S, n_heads * hd)


def add_np(res, acc, defect=None):
    """the residual epilogue on the f32 accumulator: None (the reference), "no_trunc" trunc(res + acc), "exact_sum" truncation of the exact sum, "ftz" """
    r = wide(res)
    with np.errstate(all="ignore"):
        if defect == "no_trunc":
            return bf(r + acc)
        y = wide(bf(acc))
        if defect == "exact_sum":
            # the exact sum of two bf16 values, truncated toward zero to bf16's 8 significant bits: in f64 the sum of two values whose exponents lie less than
            # ~45 apart is exact; beyond that the small one only decides on which side of the large one the sum lies
            s = r.astype(np.float64) + y.astype(np.float64)
            big = np.where(np.abs(r) >= np.abs(y), r, y).astype(np.float64); small = np.where(np.abs(r) >= np.abs(y), y, r).astype(np.float64)
            below = np.isfinite(s) & (s == big) & (small != 0) & (np.sign(small) != np.sign(big))
            t = s.astype(np.float32)
            up = np.abs(t.astype(np.float64)) > np.abs(s)                   # RN went away from zero: step back before truncating
            t = np.where(up & np.isfinite(t), np.nextafter(t, np.float32(0)), t)
            out = bf(t)
            ok = below & np.isfinite(wide(out)) & ((out & 0x7FFF) != 0)
            return np.where(ok, out - 1, out).astype(np.uint16)             # (one bf16 step toward zero)
        if defect == "ftz":
            return bf(_ftz32(_ftz32(r) + _ftz32(y)))
        return bf(r + y)


def silu_f32_formula(g):
    """x / (1 + exp(-x)) evaluated in f32 for every gate pattern, instead of the f64 table"""
    x = wide(g)
    with np.errstate(all="ignore"):
        return (x / (np.float32(1) + np.exp(-x, dtype=np.float32))).astype(np.float32)


def silu_mul_np(g_acc, u_acc, defect=None):
    """the SiLU * up epilogue on the two f32 accumulators: None, "f32_formula", "gs_not_truncated", "ftz", "swapped" """
    if defect == "swapped":
        g_acc, u_acc = u_acc, g_acc
    g, u = bf(g_acc), wide(bf(u_acc))
    with np.errstate(all="ignore"):
        s = silu_f32_formula(g) if defect == "f32_formula" else silu_table()[g]
        if defect == "gs_not_truncated":
            return bf(s * u)
        gs = wide(bf(s))
        if defect == "ftz":
            return bf(_ftz32(_ftz32(wide(bf(_ftz32(s)))) * _ftz32(u)))
        return bf(gs * u)
