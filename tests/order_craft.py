"""Rows that make the ORDER of a dot product's adds visible in its bf16 output (tests/test_order_crafted_cpu.py, tests/test_gpu_order_crafted.py), the wrong
orders a kernel could fall into, and their evaluation.  numpy and the oracle only, no GPU code.

Every kernel form must evaluate the reference's chain acc = acc + x[k] * w[k], k ascending, in f32.  Gaussian data cannot tell a wrong order from the right one
once the sum is truncated to bf16 (test_the_old_inputs_reveal_almost_nothing).  Here the f32 result is nothing but what the roundings left behind:

  zero-sum rows   half of the products are m * 2^e (m 128 .. 255, a random sign, e uniform over 40 binades), the other half their negatives, permuted per
                  output row.  The exact sum is 0, the sequential f32 sum is rounding residue: split chains, interleaved chains and moved blocks change its
                  leading bits.
  ladder rows     windows of three products +B_j, v_j, -B_j with B_j = 2^(E_TOP - 2j) and |v_j| = 1.5 * 2^-26 * B_j, zeros elsewhere.  In order, the opener absorbs
                  v_j (0.19 ulp) and the closer cancels: exactly +0.  If v_j changes places with its closer it survives, and no later, smaller B absorbs it
                  (B_(j+1) = B_j / 4): the result is not zero.  A row holds ONE ladder of up to WINDOWS windows (a second one would absorb the first one's
                  residue); the three window offsets 0, 1, 2 (mod 3) and as many ladders as K needs, one row each, put every neighbouring pair (k, k + 1),
                  k >= 1, at a (v, closer) place of some row.  The pair (0, 1) is no mutation: the chain starts at +0, and fl(p0 + p1) = fl(p1 + p0).
  head row        v, B, five zeros, -B at the front: the first unit of eight reversed adds v last (the windows' first two adds commute, so they cannot show it).

x rows are +-2^j patterns, so every product is exact, and everything stays a normal f32 or zero: the matrix-core instruction's fused multiply cannot differ
from the reference's multiply-then-add, and the same rows serve the GEMV and the matrix-core forms.  A call of several x rows has up to three different
patterns (row r has pattern r % 3, scaled by another +-2^e in every group of three); weight row i is made for ONE pattern (w = product / x), so every x row meets
its own crafted rows and, under the other patterns' rows, generic sums.

Through a fused RMSNorm (norm_front): a row of +-1.0 normalises to +-0x3F7F and a norm weight of 0x3F81 * 2^j makes it exactly +-2^j: pattern 0, from h and the
norm weight."""
import numpy as np

from linear_cases import bf, orc_linear
from oracle import oracle as orc

E_TOP = 100          # the first opener of a ladder is 2^E_TOP; the last of WINDOWS windows 2^(E_TOP - 2 * (WINDOWS - 1)) = 2^-58, its v 1.5 * 2^-84
WINDOWS = 80         # windows per ladder = 240 positions
JITTER = 3           # x elements are +-2^j, |j| <= JITTER
ZS_BINADES = 40      # spread of the zero-sum rows' exponents (with 12 every sum is exactly 0 and nothing shows)
MIN_ZERO_SUM = 16
STAGES = (64, 128, 256, 512)        # the k-steps per stage of the kernels: gemv_chain (64 .. 192), the packed gate|up and head (128 = 16 units of 8), gemv_quad
                                    # (128 / 256), rowcast_lds (512), the matrix-core slabs (128)
STRIDES = (2, 4, 8, 16, 64)


def wide(a):
    return orc.bf16_to_f32(a).reshape(np.shape(a))


def n_ladders(K):
    return -(-(K // 3) // WINDOWS)


def min_rows(K):
    return 3 * n_ladders(K) + 1 + MIN_ZERO_SUM


# ---- the x rows ------------------------------------------------------------------------------------------------------------------------------------------
def x_patterns(K, n_pat, seed):
    rng = np.random.default_rng([7, K, seed])
    return (rng.choice([-1.0, 1.0], (n_pat, K)) * 2.0 ** rng.integers(-JITTER, JITTER + 1, (n_pat, K))).astype(np.float32)


def x_rows(K, rows, seed, front="plain"):
    """(x uint16 [rows, K], pattern of every row, the patterns f32 [n_pat, K]): row r = pattern r % n_pat times +-2^e, e = (r // n_pat + 2) % 5 - 2 (the first group
    unscaled).  front = "norm": rows that come out of ONE fused RMSNorm (norm_front_rows) -- the patterns share pattern 0's exponents and differ in their signs, and
    no row is scaled (the norm takes the scale of a row of h away)"""
    n_pat = min(rows, 3)
    pat = x_patterns(K, n_pat, seed)
    which = np.arange(rows) % n_pat
    g = np.arange(rows) // n_pat
    scale = (np.where(g % 2 == 1, -1.0, 1.0) * 2.0 ** ((g + 2) % 5 - 2)).astype(np.float32)
    if front == "norm":
        pat = (np.sign(pat) * np.abs(pat[0])[None, :]).astype(np.float32)
        scale = np.where(g % 2 == 1, -1.0, 1.0).astype(np.float32)
    x = pat[which] * scale[:, None]
    xb = bf(x)
    assert np.array_equal(wide(xb), x)
    return xb, which, pat


# ---- the products of one output row ----------------------------------------------------------------------------------------------------------------------
def zero_sum_products(rng, K, e_lo=-ZS_BINADES // 2, e_hi=ZS_BINADES // 2):
    """K // 2 terms m * 2^e (e in [e_lo, e_hi)) and their negatives, permuted (an odd K: one zero among them)"""
    half = K // 2
    v = rng.choice([-1.0, 1.0], half) * rng.integers(128, 256, half) * 2.0 ** rng.integers(e_lo, e_hi, half)
    return rng.permutation(np.concatenate([v, -v, np.zeros(K - 2 * half)])).astype(np.float32)


def ladder_products(rng, K, offset, ladder, e_top=E_TOP, windows=WINDOWS):
    """windows at offset + 3 i for i in [ladder * windows, (ladder + 1) * windows), as far as K reaches"""
    p = np.zeros(K, dtype=np.float32)
    n_win = (K - offset) // 3
    for j, i in enumerate(range(ladder * windows, min((ladder + 1) * windows, n_win))):
        s = offset + 3 * i
        B = rng.choice([-1.0, 1.0]) * 2.0 ** (e_top - 2 * j)
        p[s], p[s + 1], p[s + 2] = B, rng.choice([-1.0, 1.0]) * 1.5 * abs(B) * 2.0 ** -26, -B
    return p


def head_products(rng, K, e_top=E_TOP):
    """v, B, five zeros, -B: +0 in order like a window, but the very first unit reversed adds v last, where nothing absorbs it (a window's own first two adds
    commute: the chain starts at +0)"""
    p = np.zeros(K, dtype=np.float32)
    B = rng.choice([-1.0, 1.0]) * 2.0 ** e_top
    p[0], p[1], p[7] = rng.choice([-1.0, 1.0]) * 1.5 * abs(B) * 2.0 ** -26, B, -B
    return p


def closer_row(kinds, k, windows=WINDOWS):
    """the ladder row in which (k, k + 1) is a (v, closer) pair, k in [1, K - 2]"""
    offset, i = (k - 1) % 3, (k - 1) // 3
    return kinds.index(("ladder", offset, i // windows))


def make_set(rows, n, K, front="plain", seed=0):
    """dict(rows, n, K, x [rows, K], w [n, K] (uint16), x_pat [rows], w_pat [n], pat f32 [n_pat, K], kinds [n]: "zero_sum", ("ladder", offset, ladder) or ("head",))"""
    assert K % 8 == 0 and n >= min_rows(K), (n, K, min_rows(K))
    x, x_pat, pat = x_rows(K, rows, seed, front)
    rng = np.random.default_rng([8, rows, n, K, seed])
    kinds = [("ladder", o, l) for l in range(n_ladders(K)) for o in range(3)] + [("head",)]
    kinds += ["zero_sum"] * (n - len(kinds))
    kinds = [kinds[i] for i in rng.permutation(n)]                # (ladder rows in every block of rows, at every lane)
    w = np.zeros((n, K), dtype=np.float32)
    w_pat = np.zeros(n, dtype=np.int64)
    seen = {}
    for i, kd in enumerate(kinds):
        key = kd if isinstance(kd, str) else "ladder"
        w_pat[i] = seen.get(key, 0) % len(pat); seen[key] = seen.get(key, 0) + 1
        p = zero_sum_products(rng, K) if kd == "zero_sum" else head_products(rng, K) if kd == ("head",) else ladder_products(rng, K, kd[1], kd[2])
        w[i] = p / pat[w_pat[i]]
    wb = bf(w)
    assert np.array_equal(wide(wb), w)
    return dict(rows=rows, n=n, K=K, x=x, w=wb, x_pat=x_pat, w_pat=w_pat, pat=pat, kinds=kinds)


_SETS = {}


def get_set(rows, n, K, front="plain"):
    if (rows, n, K, front) not in _SETS:
        s = make_set(rows, n, K, front)
        s["ref"] = orc_linear(s["x"], s["w"])
        _SETS[(rows, n, K, front)] = s
    return _SETS[(rows, n, K, front)]


# the sets the GPU tests run: (x rows, weight rows, K)
GEMV_SETS = [(1, 24, 256), (3, 40, 640), (3, 40, 1536)]                     # the chain GEMVs of 16 / 32 / 64 rows per block
ROWCAST_SETS = [(1, 24, 128), (3, 40, 640), (1, 40, 512)]                   # K = 512 is ONE stage of rowcast_lds_kernel, which wants two: the self-feeding kernel
ROWCAST_LDS_SETS = [(1, 40, 1024), (3, 50, 1536), (3, 72, 4096)]            # two, three and eight stages of 512
QUAD_SETS = [(1, 24, 256), (3, 40, 512), (3, 50, 768), (1, 72, 4096)]       # rw 24: one, two, three and sixteen stages of 256
STREAM_SETS = [(17, 40, 256), (83, 100, 896)]                               # 16 rows and more, K a multiple of 128: gemm_stream_kernel / gemm_blgp_kernel
MFMA_SETS = [(17, 40, 320), (83, 130, 192), (83, 100, 896)]                 # gemm_mfma_kernel: K no multiple of 128 (and one that is, for the forced tiles)
NORM_SETS = [(1, 112, 256), (1, 130, 1024)]                                 # through a fused RMSNorm: the raw gate|up kernel (56-row blocks) and the raw head
PART_SETS = [(1, 896, 256)]                                                 # the gate|up part of a stage (dim 256, FFN hidden 896 = 16 blocks of 56, 32 of 28)
WHOLE_SETS = [(17, 128, 256, "norm")]                                       # wv of a whole one-block model (two KV heads of 64): the rows are tok_embeddings behind the norm
ALL_SETS = sorted(set(GEMV_SETS + ROWCAST_SETS + ROWCAST_LDS_SETS + QUAD_SETS + STREAM_SETS + MFMA_SETS + NORM_SETS + PART_SETS)) + WHOLE_SETS


# ---- the sequential evaluator and its mutations ----------------------------------------------------------------------------------------------------------------
def products(xrow, w):
    """f32 [n, K]: x[k] * w[i, k], rounded to f32 as the reference's multiply does (exact on the crafted sets)"""
    with np.errstate(all="ignore"):
        return (np.asarray(xrow, dtype=np.float32)[None, :] * np.asarray(w, dtype=np.float32)).astype(np.float32)


def seq_sum(P, track=False):
    """acc = acc + P[:, k] for k ascending, in f32 -> acc [n] (track: also whether every partial sum was finite and normal or zero)"""
    acc = np.zeros(P.shape[0], dtype=np.float32)
    ok = True
    tiny = np.float32(2.0 ** -126)
    with np.errstate(all="ignore"):
        for k in range(P.shape[1]):
            acc = acc + P[:, k]
            if track:
                ok = ok and bool(np.all(np.isfinite(acc) & ((acc == 0) | (np.abs(acc) >= tiny))))
    return (acc, ok) if track else acc


def linear_np(x, w):
    """the numpy evaluator as an operator: uint16 [rows, K] x uint16 [n, K] -> uint16 [rows, n]"""
    xf, wf = wide(x), wide(w)
    return np.stack([bf(seq_sum(products(xf[r], wf))) for r in range(xf.shape[0])])


def evaluate(P, orders, chains):
    """a batch of wrong orders: mutation m adds the products in the sequence orders[m], step t onto partial chain chains[m, t]; the partial chains are then summed
    onto chain 0 in their order.  P f32 [n, K]; orders, chains int [M, K] -> f32 [M, n]"""
    orders = np.asarray(orders); chains = np.asarray(chains)
    M, K = orders.shape
    C = int(chains.max()) + 1
    acc = np.zeros((M, C, P.shape[0]), dtype=np.float32)
    ar = np.arange(M)
    PT = np.ascontiguousarray(P.T)
    with np.errstate(all="ignore"):
        for t in range(K):
            c = chains[:, t]
            acc[ar, c] = acc[ar, c] + PT[orders[:, t]]
        out = acc[:, 0].copy()
        for c in range(1, C):
            out = out + acc[:, c]
    return out


def pairwise4(P):
    """the matrix-core block of four k-steps summed pairwise: acc + ((p0 + p1) + (p2 + p3))"""
    acc = np.zeros(P.shape[0], dtype=np.float32)
    K4 = P.shape[1] // 4 * 4
    with np.errstate(all="ignore"):
        for k in range(0, K4, 4):
            acc = acc + ((P[:, k] + P[:, k + 1]) + (P[:, k + 2] + P[:, k + 3]))
        for k in range(K4, P.shape[1]):                           # (a ragged tail: one by one)
            acc = acc + P[:, k]
    return acc


def _stage_order(K, S, f):
    """the order in which f(list of the stages' index arrays) puts the stages of S steps (the last one ragged when S does not divide K)"""
    return np.concatenate(f([np.arange(a, min(a + S, K)) for a in range(0, K, S)]))


def _in_units(K, f, only=None):
    """the order with f applied to every whole unit of 8 (only: to that unit alone)"""
    o = np.arange(K)
    body = o[:K // 8 * 8].reshape(K // 8, 8)
    for u in (range(K // 8) if only is None else [only]):
        body[u] = f(body[u].copy())
    return o


def mutations(K, stages=STAGES):
    """[(family, name, order [K], chain [K])]: every wrong order of the issue's list that applies at K, but the single transpositions (transposition_result)
    and the pairwise block of four (pairwise4)"""
    ident, zero = np.arange(K), np.zeros(K, dtype=np.int64)
    out = []
    for s in range(8, K - 1, 8):                                 # (a second chain of ONE term is no other arithmetic: 0 + p = p)
        out.append(("split in two", "at %d" % s, ident, (ident >= s).astype(np.int64)))
    for parts in (4, 8):
        out.append(("split in %d" % parts, "equal parts", ident, ident * parts // K))
    for S in stages:
        if S < K:
            nst = -(-K // S)
            if nst > 2:
                out.append(("a chain per stage", "stages of %d" % S, ident, ident // S))
            for i in range(nst - 1):
                out.append(("two stages swapped", "stages of %d, %d and %d" % (S, i, i + 1), _stage_order(K, S, lambda st: st[:i] + [st[i + 1], st[i]] + st[i + 2:]), zero))
            out.append(("the last stage first", "stages of %d" % S, _stage_order(K, S, lambda st: st[-1:] + st[:-1]), zero))
        if S <= K and S >= 16:
            out.append(("units rotated in a stage", "stages of %d" % S,
                        _stage_order(K, S, lambda st: [np.concatenate([a[8:], a[:8]]) for a in st]), zero))
            out.append(("two units of a stage swapped", "stages of %d, the first two" % S,
                        _stage_order(K, S, lambda st: [np.concatenate([a[8:16], a[:8], a[16:]]) for a in st]), zero))
            out.append(("two units of a stage swapped", "stages of %d, the last two" % S,
                        _stage_order(K, S, lambda st: [np.concatenate([a[:-16], a[-8:], a[-16:-8]]) if len(a) >= 16 else a for a in st]), zero))
    for t in STRIDES:
        if t < K:
            out.append(("interleaved chains", "stride %d" % t, ident, ident % t))
    rev, quads, pairs = (lambda u: u[::-1]), (lambda u: np.concatenate([u[4:], u[:4]])), (lambda u: u.reshape(4, 2)[:, ::-1].ravel())
    out.append(("a unit reversed", "every unit", _in_units(K, rev), zero))
    out.append(("the quads of a unit swapped", "every unit", _in_units(K, quads), zero))
    out.append(("elements 2i and 2i+1 swapped", "every pair", _in_units(K, pairs), zero))
    for u in range(K // 8):
        out.append(("a unit reversed", "unit %d" % u, _in_units(K, rev, u), zero))
        out.append(("the quads of a unit swapped", "unit %d" % u, _in_units(K, quads, u), zero))
    return out


def transposition_results(p):
    """one ladder row's products p [K] -> f32 [K]: entry k is the chain's result with k and k + 1 swapped (entry K - 1 unused: the unchanged chain)"""
    K = p.size
    nz = np.flatnonzero(p)                                        # (zeros change nothing: the chain starts at +0 and x + (+-0) = x, +0 + -0 = +0)
    out = np.zeros(K, dtype=np.float32)
    if nz.size:
        a, b = max(int(nz[0]) - 1, 0), min(int(nz[-1]) + 2, K)     # the swaps (k, k + 1) with a <= k < b - 1 touch a non-zero product
        L = b - a
        orders = np.tile(np.arange(L), (L - 1, 1))
        for k in range(L - 1):
            orders[k, k], orders[k, k + 1] = k + 1, k
        out[a:b - 1] = evaluate(p[None, a:b], orders, np.zeros((L - 1, L), dtype=np.int64))[:, 0]
    return out


# ---- through a fused RMSNorm -----------------------------------------------------------------------------------------------------------------------------------
def norm_front(pat0):
    """(h uint16 [K], norm weight uint16 [K]) whose normalised row is exactly the +-2^j pattern pat0: h = +-1.0 normalises to +-0x3F7F (the scale lies a little
    below 1), and 0x3F7F * (0x3F81 * 2^j) = (1 + 2^-8 - 2^-15) * 2^j truncates to 2^j"""
    h = bf(np.sign(pat0).astype(np.float32))
    nw = bf((np.abs(pat0) * np.float32(1.0078125)).astype(np.float32))
    return h, nw


def norm_front_rows(s):
    """(h uint16 [rows, K], norm weight [K]) for a set made with front = "norm": row r of h is the sign of x row r times c, c = 1, 2, 0.5, 4 for six rows each -- every
    element of a row has the same magnitude, so the row normalises to +-0x3F7F whatever c is"""
    x = wide(s["x"])
    c = np.array([1.0, 2.0, 0.5, 4.0], dtype=np.float32)[(np.arange(s["rows"]) // 6) % 4]
    return bf(np.sign(x) * c[:, None]), norm_front(s["pat"][0])[1]


U_CONST, G_CONST = bf(np.float32(1.5)), bf(np.float32(1.0))          # the other side of SiLU(gate) * up while the crafted chain is the gate / the up


def gate_up_constant(s, value):
    """a matrix of one-hot rows (column 0) whose product with the set's x row is `value` in every output"""
    w = np.zeros((s["n"], s["K"]), dtype=np.float32)
    w[:, 0] = wide(np.array([value], dtype=np.uint16))[0] / s["pat"][0][0]
    return bf(w)


# ---- sets for the 13-bit packed kernels: every weight inside one window of 28 binades ----------------------------------------------------------------------------
# A packable matrix spans at most 30 binades (lnb_wpack.h: exponent field / 2 within 15 values), so the exponents of the products ride on the x row -- that is, on
# the norm weight -- and ALL rows of a matrix share one column profile a[k]: product[i, k] = (+-2^a[k]) * w[i, k], w's exponent in [-13, 14].  One x row per
# matrix (the packed kernels are one-token kernels), so a set is a GROUP of matrices, each with its own norm weight and its own launch:
#   "flat"    a[k] random in [-13, 13): zero-sum rows (a pair of columns shares a product exponent that both windows reach; the products spread over ~50 binades)
#             and the head row;
#   "ramp"    a[k] = PK_E_TOP - 13 - j(k), j = (k // 3 + phase) % PK_WINDOWS: ladders that fall by 2 per window with |v| = 1.5 * 2^-25 B (0.375 ulp: absorbed by its
#             opener, 0.75 ulp of the next, smaller opener: it survives) -- B needs w = 2^13 or 2^14, v needs 1.5 * 2^-12 or 2^-11.  The ramp restarts every
#             PK_WINDOWS windows; a window across a restart is left out and lies inside a ramp of the second phase, so K > 3 * PK_WINDOWS takes two ramp matrices.
PK_E_TOP, PK_WINDOWS, PK_ROWS = 100, 171, 112
PACKED_KS = (256, 1024)             # two and eight of the packed kernels' 128-step stages (five are in flight: the ring wraps)


def _pk_j(K, phase):
    return (np.arange(K) // 3 + phase) % PK_WINDOWS


def pk_ladder(rng, K, offset, seg, phase):
    """(products [K], [k of every (v, closer) pair]) of the ladder of window offset `offset` in ramp `seg` of the phase"""
    p, pairs = np.zeros(K, dtype=np.float32), []
    for i in range((K - offset) // 3):
        j = (i + phase) % PK_WINDOWS
        if (i + phase) // PK_WINDOWS != seg or (offset and j == PK_WINDOWS - 1):
            continue
        s = offset + 3 * i
        B = rng.choice([-1.0, 1.0]) * 2.0 ** (PK_E_TOP - j)
        p[s], p[s + 1], p[s + 2] = B, 1.5 * B * 2.0 ** -25, -B       # (v with B's sign: towards zero the ulp halves and 0.375 ulp would be 0.75)
        pairs.append(s + 1)
    return p, pairs


def packed_group(K, seed=0):
    """[dict(name, K, n, h [K], nw [K], x [1, K] (what the norm must give), w [n, K], kinds, pairs {k: row}, col, ref [n])]: the matrices of the packed set of K"""
    out = []
    phases = (0,) if K // 3 + 1 <= PK_WINDOWS else (0, PK_WINDOWS // 2)
    for name, phase in [("flat", None)] + [("ramp%d" % ph, ph) for ph in phases]:
        rng = np.random.default_rng([9, K, seed, 999 if phase is None else phase])
        sign = rng.choice([-1.0, 1.0], K)
        kinds, pairs, P = [], {}, np.zeros((PK_ROWS, K), dtype=np.float32)
        if phase is None:
            a = rng.integers(-13, 13, K)
            a[[0, 1, 7]] = 0
            P[0, 0], P[0, 1], P[0, 7] = 1.5 * 2.0 ** -12, 2.0 ** 13, -2.0 ** 13                # the head row: v, B, five zeros, -B
            kinds.append(("head",))
            for i in range(1, PK_ROWS):
                perm = rng.permutation(K)
                for k, k2 in zip(perm[0::2], perm[1::2]):
                    e = rng.integers(max(a[k], a[k2]) - 13, min(a[k], a[k2]) + 14)
                    P[i, k] = rng.choice([-1.0, 1.0]) * rng.integers(128, 256) / 128.0 * 2.0 ** e
                    P[i, k2] = -P[i, k]
                kinds.append("zero_sum")
        else:
            a = PK_E_TOP - 13 - _pk_j(K, phase)
            rows = [(o, seg) for seg in range((K // 3 + phase) // PK_WINDOWS + 1) for o in range(3)]
            for i in range(PK_ROWS):                                 # (the ladders again with other signs until two blocks of 56 rows are full)
                o, seg = rows[i % len(rows)]
                P[i], pr = pk_ladder(rng, K, o, seg, phase)
                kinds.append(("ladder", o, seg))
                if i < len(rows):
                    pairs.update({k: i for k in pr})
        x = (sign * 2.0 ** a).astype(np.float32)
        w = (P / x[None, :]).astype(np.float32)
        wb, xb = bf(w), bf(x[None, :])
        assert np.array_equal(wide(wb), w) and np.array_equal(wide(xb)[0], x)
        h, nw = norm_front(x)
        out.append(dict(name=name, K=K, n=PK_ROWS, rows=1, h=h, nw=nw, x=xb, w=wb, kinds=kinds, pairs=pairs, col=int(np.argmin(np.abs(a))), ref=orc_linear(xb, wb)[0]))
    return out


_PACKED = {}


def get_packed(K):
    if K not in _PACKED:
        _PACKED[K] = packed_group(K)
    return _PACKED[K]


def packed_constant(m, value):
    """gate_up_constant for a matrix of a packed group: the one-hot weight sits in the column whose x is nearest 1, so that it lies inside the window too"""
    w = np.zeros((m["n"], m["K"]), dtype=np.float32)
    w[:, m["col"]] = wide(np.array([value], dtype=np.uint16))[0] / wide(m["x"])[0, m["col"]]
    return bf(w)
