"""The sampling rule of include/lnb.h ("seeded temperature / top-k / top-p sampling") restated in numpy and Python integers -- a helper module (as kv_craft.py),
shared by tests/test_sampler_cpu.py (against the serial C++ walk of csrc/lnb_sample.h) and tests/test_gpu_sampler.py (against the kernel).

A sampler is (temperature, top_k, top_p, seed).  One bf16 logits row x[0..V) at position pos gives one token:
  1. y = trunc_bf16(f32(x) / temperature)
  2. candidates: y not NaN and > -MaxFloat32; none -> token -1
  3. e = exp(f64(y)) (math.exp: the host libm); a = first maximum of y; e[a] = +inf or below 2^-1022 -> degenerate, token a
  4. w = floor(e * 2^(45 - E)), E = floor(log2(e[a])); S = {w >= 1}
  5. S ordered by y descending, lowest index first among equals
  6. top_k > 0 keeps the first min(top_k, |S|); W1 = their weight
  7. top_p < 1 keeps the shortest prefix with weight >= P = floor(f64(f32(top_p)) * f64(W1)), at least one entry
  8. u = splitmix64(splitmix64(seed) ^ (pos * 0x9E3779B97F4A7C15)), r = (u * W_K) >> 64; the token = the first kept index, in index order, whose running weight exceeds r
temperature 0 = ml.Argmax(x)."""
import math

import numpy as np

from oracle import oracle as orc

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
FMAX = np.float32(3.4028234663852886e38)
INFO_FIELDS = ("w_all", "w_topk", "w_kept", "n_candidates", "n_kept", "degenerate")
_ETAB = None


def splitmix64(z):
    z = (z + GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, pos):
    return splitmix64(splitmix64(seed & MASK) ^ (((pos & MASK) * GOLDEN) & MASK))


def u_for(r, w_kept):
    """a u whose (u * w_kept) >> 64 is exactly r (0 <= r < w_kept)"""
    u = ((r << 64) + w_kept - 1) // w_kept
    assert u <= MASK and (u * w_kept) >> 64 == r
    return u


def _exp(x):
    if math.isnan(x):
        return math.nan
    try:
        return math.exp(x)
    except OverflowError:                                    # (libm returns +inf there; Python raises)
        return math.inf


def exp_table():
    global _ETAB
    if _ETAB is None:
        with np.errstate(invalid="ignore"):                  # (the signalling NaN patterns)
            v = orc.bf16_to_f32(np.arange(65536, dtype=np.uint16)).astype(np.float64)
        _ETAB = np.array([_exp(x) for x in v], dtype=np.float64)
    return _ETAB


def argmax(row_u16):
    """ml.Argmax: first maximum among the entries that are not NaN and > -MaxFloat32; -1 if there is none"""
    f = orc.bf16_to_f32(np.ascontiguousarray(row_u16, dtype=np.uint16))
    idx = np.nonzero(f > -FMAX)[0]
    return int(idx[np.argmax(f[idx])]) if idx.size else -1


def scale(row_u16, temperature):
    row_u16 = np.ascontiguousarray(row_u16, dtype=np.uint16)
    if np.float32(temperature) == np.float32(1.0):
        return row_u16
    with np.errstate(all="ignore"):
        q = (orc.bf16_to_f32(row_u16) / np.float32(temperature)).astype(np.float32)
    return orc.f32_to_bf16(q)


def zero_info():
    return dict.fromkeys(INFO_FIELDS, 0)


def prepare(row_u16, temperature, top_k, top_p):
    """steps 1-7: -> (token or None, kept indices in index order, their running weight sums (uint64), info)"""
    info = zero_info()
    if temperature == 0:
        return argmax(row_u16), None, None, info
    y16 = scale(row_u16, temperature)
    y = orc.bf16_to_f32(y16)
    cand = y > -FMAX
    if not cand.any():
        return -1, None, None, info
    ci = np.nonzero(cand)[0]
    a = int(ci[np.argmax(y[ci])])
    e = exp_table()[y16.astype(np.int64)]
    if math.isinf(e[a]) or e[a] < 2.0 ** -1022:
        info["degenerate"] = 1
        return a, None, None, info
    E = math.frexp(e[a])[1] - 1
    w = np.zeros(y.size, dtype=np.uint64)
    w[ci] = np.floor(np.ldexp(e[ci], 45 - E)).astype(np.uint64)
    S = np.nonzero(w >= 1)[0]
    order = S[np.lexsort((S, -y[S].astype(np.float64)))]
    info["n_candidates"] = int(S.size); info["w_all"] = int(w[S].sum(dtype=np.uint64))
    kept = order[:top_k] if top_k > 0 else order
    info["w_topk"] = int(w[kept].sum(dtype=np.uint64))
    if np.float32(top_p) < np.float32(1.0):
        P = int(np.floor(np.float64(np.float32(top_p)) * np.float64(np.uint64(info["w_topk"]))))
        cs = np.cumsum(w[kept], dtype=np.uint64)
        n = int(np.searchsorted(cs, np.uint64(P), side="left")) + 1
        kept = kept[:max(1, min(n, kept.size))]
    ks = np.sort(kept)
    cs = np.cumsum(w[ks], dtype=np.uint64)
    info["n_kept"] = int(ks.size); info["w_kept"] = int(cs[-1])
    return None, ks, cs, info


def pick(prep, u):
    tok, ks, cs, info = prep
    if tok is not None:
        return tok
    r = (u * info["w_kept"]) >> 64
    return int(ks[int(np.searchsorted(cs, np.uint64(r), side="right"))])


def sample(row_u16, sampler, pos=0, u=None):
    """-> (token, info)"""
    t, k, p, seed = sampler
    prep = prepare(row_u16, t, k, p)
    return pick(prep, draw(seed, pos) if u is None else u), prep[3]


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------------
def llama_like_rows(rng, rows, V):
    """gaussian body plus a few peaks, truncated to bf16 like the head's output (the rows of the token-probability tests)"""
    x = rng.normal(0.0, 2.2, size=(rows, V)).astype(np.float32)
    for r in range(rows):
        n = rng.integers(1, 6)
        x[r, rng.integers(0, V, size=n)] += rng.uniform(6.0, 16.0, size=n).astype(np.float32)
    return orc.f32_to_bf16(x)


TEMPERATURES = (1.0, 0.7, 1.5, 0.25)
TOP_PS = (1.0, 0.9, 0.5, 1e-6)
POSITIONS = (0, 8, 131071)
SEEDS = (0, 777, 0xFEDCBA9876543210)


def grid(V):
    """every (temperature, top_k, top_p) of the issue's grid"""
    return [(t, k, p) for t in TEMPERATURES for k in (0, 1, 2, 40, V) for p in TOP_PS]


def grid_cases(V, rows=64):
    """(row index, (t, k, p)): every grid point on two of the rows"""
    g = grid(V)
    return [((c * 7 + rep * 29) % rows, g[c]) for c in range(len(g)) for rep in range(2)]


def bf(v):
    return int(orc.f32_to_bf16(np.array([v], dtype=np.float32))[0])


def crafted(V):
    """[(name, row u16 [V], (temperature, top_k, top_p), check(token, info, row) or None, boundary_draws)] -- each row named for the defect it catches.
    boundary_draws: also run with explicit u that put r at 0, W_K - 1 and at c - 1 / c for every running weight sum c of the kept set."""
    NINF, NAN = 0xFF80, 0x7FC0
    out = []

    def row(fill):
        return np.full(V, fill, dtype=np.uint16)

    def expect(**kw):
        tokens = kw.pop("tokens", None)

        def check(tok, info, _row):
            for k, v in kw.items():
                assert info[k] == v, (k, info[k], v)
            if tokens is not None:
                assert tok in tokens, (tok, tokens)
        return check

    r = row(bf(-30.0)); r[[7, 300, V - 1, 50, 500]] = bf(2.0); r[600] = bf(3.0)
    out.append(("ties_straddle_the_top_k_cut", r, (1.0, 3, 1.0), expect(n_kept=3, tokens={7, 50, 600}), True))
    r = row(bf(-40.0)); r[[900, 20, 450, 21, 700, 3]] = bf(2.0); r[640] = bf(3.0)
    out.append(("ties_straddle_the_nucleus_cut", r, (1.0, 0, 0.5), expect(n_kept=3, tokens={3, 20, 640}), True))
    r = row(NINF); r[[5, 17, 100, 101, 555, 800, 999, 1000]] = 0
    out.append(("prefix_sum_equals_p_exactly", r, (1.0, 0, 0.5), expect(n_candidates=8, w_all=8 << 45, w_kept=4 << 45, n_kept=4, tokens={5, 17, 100, 101}), True))
    r = row(bf(17.0)); r[V // 2] = bf(50.0)
    out.append(("one_dominant_value", r, (1.0, 0, 1.0), expect(n_candidates=1, n_kept=1, tokens={V // 2}), False))
    r = row(bf(-1.0)); r[::3] = NAN; r[1::7] = NINF; r[11] = bf(1.0); r[12] = 0xFFC0
    out.append(("nan_and_minus_inf_entries", r, (1.0, 0, 1.0), expect(degenerate=0), True))
    r = row(bf(1.0)); r[::5] = NAN; r[[33, 66]] = 0x7F80; r[3] = NINF
    out.append(("plus_inf_entry", r, (1.0, 0, 0.9), expect(degenerate=1, tokens={33}), False))
    r = row(NAN); r[1::2] = 0xFFC1
    out.append(("all_nan_row", r, (0.7, 40, 0.9), expect(degenerate=0, n_candidates=0, tokens={-1}), False))
    r = row(bf(3.0)); r[[44, 45]] = bf(800.0)
    out.append(("exp_overflows", r, (1.0, 0, 1.0), expect(degenerate=1, tokens={44}), False))
    r = row(bf(300.0)); r[[9, 70]] = bf(400.0)
    out.append(("exp_overflows_after_scaling", r, (0.25, 0, 1.0), expect(degenerate=1, tokens={9}), False))
    out.append(("minus_800_everywhere", row(bf(-800.0)), (1.0, 0, 1.0), expect(degenerate=1, tokens={0}), False))
    r = row(NINF); r[[4, 8, 15, 16, 23, 42]] = [0x8000, 0, 0x8000, 0, 0, 0x8000]
    out.append(("signed_zeros_tie", r, (1.0, 3, 1.0), expect(n_candidates=6, n_kept=3, w_kept=3 << 45, tokens={4, 8, 15}), True))
    r = row(NINF); r[[2, 5]] = 0; r[10] = bf(2.0 ** -100)          # 2^-100 / (1.5 * 2^27) is an f32 subnormal: larger than the zeros, not equal to them
    out.append(("subnormal_quotient", r, (201326592.0, 1, 1.0), expect(n_kept=1, tokens={10}), False))
    r = row(NINF); r[[1, 30, 31, 990]] = [bf(1.0), bf(0.5), bf(0.0), bf(2.0)]
    out.append(("top_k_larger_than_s", r, (1.0, 1000, 1.0), expect(n_candidates=4, n_kept=4), True))
    r = row(bf(-2.0)); r[[0, 499, V - 1]] = [bf(1.5), bf(2.5), bf(2.0)]
    out.append(("draws_on_every_boundary", r, (0.7, 0, 1.0), None, True))
    return out


def boundary_draws(prep):
    """u values that put r at 0, W_K - 1 and both sides of up to 6 running sums spread over the kept set"""
    _, ks, cs, info = prep
    if ks is None:
        return []
    W = info["w_kept"]
    rs = {0, W - 1}
    for i in sorted({0, 1, ks.size // 2, ks.size - 2, ks.size - 1} & set(range(ks.size))):
        c = int(cs[i])
        rs |= {c - 1, c} if c < W else {c - 1}
    return [u_for(r, W) for r in sorted(rs)]
