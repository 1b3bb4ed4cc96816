"""Operator-level cases shared by tests/test_gpu_parity.py and the child processes of tests/test_gpu_forms.py (a ONCE knob such as LNB_GEMM_TILE needs a fresh
process; the case must be the same one): the oracle's linear operator and the special-values product."""
import numpy as np

from oracle import oracle as orc


def bf(a):
    return orc.f32_to_bf16(np.asarray(a, dtype=np.float32))


def orc_linear(x, w, nthreads=8):
    y = np.zeros((x.shape[0], w.shape[0]), dtype=np.uint16)
    orc.lib().orc_linear_bf16(orc._p(x), orc._p(w), orc._p(y), x.shape[0], w.shape[0], x.shape[1], nthreads)
    return y


def check_linear_bit_exact(lnb, rows, n, k, rw, seed):
    """gaussian activations of varied scale against small gaussian weights: every output bit the oracle's"""
    rng = np.random.default_rng(seed)
    x = bf(rng.standard_normal((rows, k)) * 10 ** rng.uniform(-2, 2))
    w = bf(rng.standard_normal((n, k)) * 0.05)
    assert (lnb.op_linear(x, w, rw=rw) == orc_linear(x, w)).all(), (rows, n, k, rw)


def check_linear_special_values(lnb, rows, rw):
    """Values outside the comfortable range, through every exact kernel family (chain GEMV, row-broadcast GEMV, f32 matrix-core GEMM):
    signed zeros (the chain starts at +0, so a sum of -0 products is +0), +-inf and NaN in weights and activations (inf - inf, 0 * inf),
    products that overflow f32, products and partial sums in the f32-subnormal range (bf16 shares f32's exponent range: two tiny
    operands give a subnormal, inexactly rounded product -- operations_lineartransform.go:60 multiplies in float32), and sums that
    cancel to exactly zero.  Bits must match the oracle; for NaN results only the NaN-ness.
    The GEMVs multiply, then add, like the reference, and match everywhere.  The f32 matrix-core instruction of the prefill GEMM
    (16 or more rows) FUSES the multiply: same bits whenever every single product is a normal f32 (NOTES.md section 2) -- its rows
    here keep sums that overflow and subnormal partial sums, but no single product outside [2^-126, 2^128)."""
    k, n = 512, 96
    rng = np.random.default_rng(rows * 131 + rw)
    x = bf(rng.standard_normal((rows, k)))
    w = bf(rng.standard_normal((n, k)) * 0.05)
    xf, wf = orc.bf16_to_f32(x).copy(), orc.bf16_to_f32(w).copy()
    wf[0, :] = -0.0                                              # all products -0 (or +0): result +0
    wf[1, :] = 0.0; wf[1, 7] = np.inf                            # one inf product
    wf[2, 3] = np.inf; wf[2, 200] = -np.inf                      # inf - inf -> NaN
    wf[3, 11] = np.nan
    gemm = rows >= 16
    wf[4, :] = 3.0e38                                            # single products overflow (GEMV rows) ...
    if gemm:
        wf[4, :] = 0.0; wf[4, :64] = 1.0e37                      # ... or only the running SUM does (x[:, :64] = 2 below: 64 x 2e37)
    wf[5, :] = 1e-30 * rng.standard_normal(k)                    # products ~1e-30 x 1: tiny but normal
    wf[6, :] = 1e-38 * rng.standard_normal(k)                    # bf16 values at the edge of / inside the subnormal range
    wf[7, :] = np.float32(2.0 ** -100) * rng.integers(1, 128, k)      # with the tiny activations below: subnormal products
    wf[8, 0::2] = 1.0; wf[8, 1::2] = -1.0                        # exact cancellation on duplicated activations
    wf[9, :] = 0.0; wf[9, 100] = np.inf                          # inf * 0 -> NaN (activation 100 is zeroed below)
    wf[10, :] = -wf[5, :]
    xf[:, 100] = 0.0
    xf[:, 1::2] = xf[:, 0::2]
    if gemm:
        xf[:, :64] = 2.0
    if rows > 1:
        # tiny activations: with weight row 7 (2^-100 x small integers) the products are 2^-140 x integers -- exact subnormals in both
        # arithmetics, partial sums subnormal; with weight row 6 (1e-38) single products underflow inexactly: GEMV rows only
        xf[1, :] = np.float32(2.0 ** -40) * rng.integers(-127, 128, k)
        if gemm:
            wf[6, :] = 1e-20 * rng.standard_normal(k)
    if rows > 2:
        xf[2, 17] = np.nan; xf[2, 18] = -np.inf
    x, w = bf(xf), bf(wf)
    y = lnb.op_linear(x, w, rw=rw)
    ref = orc_linear(x, w)
    bad = np.argwhere(~((y == ref) | (np.isnan(orc.bf16_to_f32(y)) & np.isnan(orc.bf16_to_f32(ref)))))
    assert bad.size == 0, "first differences (row, col): %s  got %s  oracle %s" % (bad[:6].tolist(), [hex(int(y[i, j])) for i, j in bad[:6]], [hex(int(ref[i, j])) for i, j in bad[:6]])
    assert y[0, 0] == 0x0000                                     # +0, not -0


def check_rmsnorm_adversarial(lnb, k, rw, reps=1):
    """The RMSNorm sum of squares is evaluated by the exact parity-map tree (rms_scale_wide); inputs chosen to stress it:
    huge dynamic range, ties everywhere (powers of two), sparse rows, subnormal squares, outliers, leading zeros.
    reps = 2: the twelve families twice over, 24 rows: the prefill form (a row norm kernel in front of a matrix-core product)."""
    rng = np.random.default_rng(k + rw)
    rows = []
    for kind in range(12):
        if kind == 0: x = rng.standard_normal(k)
        elif kind == 1: x = rng.standard_normal(k) * 1e-15
        elif kind == 2: x = 2.0 ** rng.integers(-12, 4, k)
        elif kind == 3: x = rng.standard_normal(k) * (rng.random(k) < 0.05)
        elif kind == 4: x = np.exp(rng.uniform(-40, 5, k))
        elif kind == 5: x = np.full(k, 2.0 ** rng.integers(-8, 8))
        elif kind == 6: x = np.abs(rng.standard_normal(k)) * np.where(rng.random(k) < 0.01, 1e4, 1.0)
        elif kind == 7: x = np.where(np.arange(k) < k // 3, 0.0, rng.standard_normal(k))
        elif kind == 8: x = np.zeros(k)
        elif kind == 9: x = rng.standard_normal(k) * 1e12
        elif kind == 10: x = np.where(np.arange(k) == k - 1, 3e4, 1e-3 * rng.standard_normal(k))
        else: x = rng.standard_normal(k) * np.exp(rng.uniform(-20, 8, k))
        rows.append(x)
    x = bf(np.stack(rows * reps))
    nw = bf(1 + 0.1 * rng.standard_normal(k))
    w = bf(rng.standard_normal((64, k)) * 0.05)
    y = lnb.op_rmsnorm_linear(x, nw, 1e-5, w, rw=rw)
    xn = np.zeros_like(x)
    orc.lib().orc_rmsnorm_bf16(orc._p(x), orc._p(nw), orc._p(xn), x.shape[0], k, np.float32(1e-5), None)
    assert (y == orc_linear(xn, w)).all()
