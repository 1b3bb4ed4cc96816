"""Rows for the RMSNorm sum of squares (rms_fold / rms_scale_wide of csrc/lnb_kernels.hip), built for the folding-wave count and the leaf size the device
uses at a given K: the families the suite already had, and one builder per way out of the branch-free item walk.  Everything is bf16 (uint16 bit patterns);
the squares the kernels add are exact in f32 unless they leave its range.  No GPU: tests/test_norm_sum_cpu.py runs every builder through the emulation of
tests/native/seqsum_host.cpp and asserts the path class it was built for; tests/test_gpu_norm_sum.py sends the same rows to every kernel form."""
import numpy as np

RMS_HEAD = 256                       # lnb_kernels.hip
K_SET = (8, 64, 200, 256, 512, 1000, 1024, 3072, 4096, 5120, 8192)
# the path word (RMS_PATH_* of csrc/lnb_seqsum.h)
LEFT, FLAGGED, OVER64, CHECK = 7 << 28, 1 << 28, 2 << 28, 4 << 28
NOFIT, UNCOVERED, SCANFAIL = 1 << 19, 1 << 18, 1 << 17
CLASSES = ("runs", "split", "single", "count", "check", "nonfinite", "replay")


def classes_of(word):
    """the path classes (a)..(g) one path word proves"""
    w = int(word) & 0xFFFFFFFF
    if w == 0xFFFFFFFF:
        return set()                                             # the plain serial loop: no item list
    if not w & LEFT:
        items, split, single = (w >> 16) & 0xFFF, (w >> 8) & 0xFF, w & 0xFF
        out = set()
        if items and not split and not single: out.add("runs")
        if split: out.add("split")
        if single: out.add("single")
        return out
    out = set()
    if w & OVER64 or w & NOFIT: out.add("count")
    if w & CHECK: out.add("check")
    if w & UNCOVERED: out.add("nonfinite")
    if w & 0xFF: out.add("replay")
    return out


def bf16_bits(a):
    """truncation to bf16, as the oracle's f32_to_bf16"""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def squares(x_u16):
    """the f32 terms the kernels add: x * x rounded to f32 once (exact unless it leaves the f32 range)"""
    x = (x_u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray((x * x).astype(np.float32))


def leaf_size(K, nh):
    """seq_leaf_size(K, nh * 64) of csrc/lnb_seqsum.h"""
    lanes = nh * 64
    leaf = ((K + lanes - 1) // lanes + 3) & ~3
    return max(leaf, 8)


def head_leaves(K, nh):
    return min(K, RMS_HEAD) // leaf_size(K, nh)


# ---- the families the suite already has -----------------------------------------------------------------------------------------------------
def adversarial(rng, K):
    """the twelve of tests/linear_cases.check_rmsnorm_adversarial"""
    rows = []
    for kind in range(12):
        if kind == 0: x = rng.standard_normal(K)
        elif kind == 1: x = rng.standard_normal(K) * 1e-15
        elif kind == 2: x = 2.0 ** rng.integers(-12, 4, K)
        elif kind == 3: x = rng.standard_normal(K) * (rng.random(K) < 0.05)
        elif kind == 4: x = np.exp(rng.uniform(-40, 5, K))
        elif kind == 5: x = np.full(K, 2.0 ** rng.integers(-8, 8))
        elif kind == 6: x = np.abs(rng.standard_normal(K)) * np.where(rng.random(K) < 0.01, 1e4, 1.0)
        elif kind == 7: x = np.where(np.arange(K) < K // 3, 0.0, rng.standard_normal(K))
        elif kind == 8: x = np.zeros(K)
        elif kind == 9: x = rng.standard_normal(K) * 1e12
        elif kind == 10: x = np.where(np.arange(K) == K - 1, 3e4, 1e-3 * rng.standard_normal(K))
        else: x = rng.standard_normal(K) * np.exp(rng.uniform(-20, 8, K))
        rows.append(x)
    return rows


def fuzz_cases(rng, K, reps=2):
    """the eight of tests/test_seqsum._cases, as activations"""
    rows = []
    for trial in range(8 * reps):
        kind = trial % 8
        if kind == 0: x = rng.standard_normal(K)
        elif kind == 1: x = rng.standard_normal(K) * 10 ** rng.uniform(-18, 6)
        elif kind == 2: x = 2.0 ** rng.integers(-12, 4, K)
        elif kind == 3: x = rng.standard_normal(K) * (rng.random(K) < 0.05)
        elif kind == 4: x = np.exp(rng.uniform(-40, 5, K))
        elif kind == 5: x = np.full(K, 2.0 ** rng.integers(-8, 8))
        elif kind == 6: x = np.abs(rng.standard_normal(K)) * np.where(rng.random(K) < 0.01, 1e4, 1.0)
        else: x = np.where(np.arange(K) < rng.integers(0, K), 0.0, rng.standard_normal(K))
        rows.append(x)
    return rows


def non_finite(rng, K):
    """the ten of test_rmsnorm_rows_with_non_finite_and_overflowing_squares"""
    base = rng.standard_normal(K).astype(np.float32)
    rows = []
    for kind in range(10):
        x = base.copy()
        if kind == 0: x[K // 2] = np.inf
        elif kind == 1: x[K // 3] = np.nan
        elif kind == 2: x[5] = -np.inf
        elif kind == 3: x[K // 2: K // 2 + 9] = 1e20
        elif kind == 4: x[K - 1] = -3e38
        elif kind == 5: x[:] = 3e38 * np.sign(base)
        elif kind == 6: x[:] = 1e19
        elif kind == 7: x[0] = np.nan
        elif kind == 8: x[:] = 0.0; x[0] = np.inf
        else: x[:] = 1e-30 * base
        rows.append(x)
    return rows


def outliers(rng, K, n=9):
    """the outlier-channel rows of the item-list tests: one to three terms lift the sum several binades"""
    rows = []
    for trial in range(n):
        x = rng.standard_normal(K) * 0.05 * np.exp(rng.uniform(-6, 6))
        lo = min(300, K - 1)
        for pos in rng.integers(lo, K, size=1 + trial % 3):
            x[pos] = rng.uniform(20, 400) * (1.0 if trial % 2 else 50.0)
        rows.append(x)
    return rows


# ---- one builder per way out of the fast path -----------------------------------------------------------------------------------------------
def climb(rng, K, nh, leaves_per_binade):
    """squares that grow smoothly so that the running sum enters the next binade every `leaves_per_binade` leaves behind the head: few crossings are
    split leaves between runs (class split); many make more than 64 items (class count)"""
    leaf = leaf_size(K, nh)
    k = np.arange(K, dtype=np.float64)
    period = leaves_per_binade * leaf
    span = min((K - RMS_HEAD) / period, 230.0) if K > RMS_HEAD else 1.0
    p = 2.0 ** ((k - RMS_HEAD) / period)
    p[:RMS_HEAD] = p[RMS_HEAD] if K > RMS_HEAD else 1.0
    x = np.sqrt(p) * 2.0 ** (-span / 4 - 8) * (1 + 0.2 * rng.random(K))
    return x


def powers_of_two(rng, K, nh):
    """one power of two in every position: the running sum is n * p exactly, so it meets every binade edge exactly, at a leaf end wherever the leaf size
    divides a power of two: no guess, no split -- single-term items"""
    return np.full(K, 2.0 ** rng.integers(-20, 20))


def list_overflow(rng, K, nh):
    """behind the head, inside the first folding wave: a stretch where every second term doubles the running sum, so that every leaf crosses several
    binades and is neither a run member nor split -- LEAF single-term items each, more than the wave's 128-entry segment holds"""
    leaf, hl = leaf_size(K, nh), head_leaves(K, nh)
    n_leaves = 128 // leaf + 2
    start, n = hl * leaf, n_leaves * leaf
    x = np.zeros(K)
    if start + n > K or hl + n_leaves > 64:
        return None
    x[:start] = 2.0 ** -62 * rng.random(start)
    x[start:start + n] = 2.0 ** (-60 + np.arange(n) // 2 / 2.0)            # squares 2^-120 * 2^(j // 2)
    x[start + n:] = rng.standard_normal(K - start - n) * 1e-3
    return x


def bad_guess(rng, K, nh, scale_exp=0):
    """a head that sums to 2 - 2^-22 exactly, then terms just below half an ulp of it: the serial sum absorbs every one and stays where it is, the tree
    sums of the guess do not -- some 600 terms on they put the leaves in the next binade.  The guess is consistent, so the leaves form runs; the item
    check against the true running sum fails"""
    head = [1.0] + [2.0 ** -i for i in range(1, 12) for _ in range(3)]      # squares 1 + 3 * sum 4^-i
    if K < len(head) + 900:
        return None
    x = np.full(K, 2.0 ** -13 * (1 + (120 + rng.integers(0, 8)) / 128.0))
    x[:len(head)] = head
    return x * 2.0 ** scale_exp


def skipped_leaves(rng, K, nh):
    """rows that are zero up to, and from, each leaf boundary around the end of the head"""
    leaf, hl = leaf_size(K, nh), head_leaves(K, nh)
    rows = []
    for b in range(max(hl - 1, 0), hl + 3):
        if b * leaf >= K: continue
        g = rng.standard_normal(K) * 10 ** rng.uniform(-3, 3)
        a = g.copy(); a[:b * leaf] = 0.0
        c = g.copy(); c[b * leaf:] = 0.0
        rows += [a, c]
    return rows


def mid_run_non_finite(rng, K, nh):
    """a single non-finite square in the middle of a run: an infinity, a NaN, a square that overflows"""
    rows = []
    for v in (np.inf, np.nan, 1e20, -np.inf):
        x = rng.standard_normal(K)
        x[int(K * rng.uniform(0.55, 0.9))] = v
        rows.append(x)
    return rows


def mid_leaf_overflow(rng, K, nh):
    """finite squares whose running sum overflows to inf in the middle of a leaf behind the head"""
    leaf = leaf_size(K, nh)
    rows = []
    for _ in range(3):
        x = rng.standard_normal(K) * 1e15
        at = (int(K * rng.uniform(0.5, 0.9)) // leaf) * leaf + leaf // 2 - 2
        x[at:] = 1e19
        rows.append(x)
    return rows


def crafted(rng, K, nh):
    """-> list of (builder name, the path class it is built for or None, row)"""
    out = []
    for m in (40, 24, 12):
        out += [("climb%d" % m, "split", climb(rng, K, nh, m)) for _ in range(2)]
    for m in (3, 2):
        out += [("climb%d" % m, "count", climb(rng, K, nh, m)) for _ in range(2)]
    out += [("powers_of_two", "single", powers_of_two(rng, K, nh)) for _ in range(4)]
    out += [("list_overflow", "count", list_overflow(rng, K, nh)) for _ in range(2)]
    out += [("bad_guess", "check", bad_guess(rng, K, nh, e)) for e in (0, -30, 24)]
    out += [("skipped_leaves", None, r) for r in skipped_leaves(rng, K, nh)]
    out += [("mid_run_non_finite", "nonfinite", r) for r in mid_run_non_finite(rng, K, nh)]
    out += [("mid_leaf_overflow", "nonfinite", r) for r in mid_leaf_overflow(rng, K, nh)]
    return [(n, c, r) for n, c, r in out if r is not None]


def old_families(rng, K):
    return ([("adversarial", None, r) for r in adversarial(rng, K)] + [("fuzz_cases", None, r) for r in fuzz_cases(rng, K)] +
            [("non_finite", None, r) for r in non_finite(rng, K)] + [("outliers", None, r) for r in outliers(rng, K)])


def variants(x_u16):
    """the row, its terms reversed, and shifted (rotated) by one to three positions: leaf boundaries fall elsewhere"""
    return [x_u16, x_u16[::-1].copy(), np.roll(x_u16, 1), np.roll(x_u16, 2), np.roll(x_u16, 3)]


def row_set(K, nh):
    """-> (names, intended classes, x uint16 [rows][K]) for the kernels that fold K terms on nh waves (nh None: the plain serial loop; leaves as for 6 waves).
    Deterministic in (K, nh).  A variant keeps its row's name with a suffix and claims no class of its own."""
    w = nh if nh else 6
    rng = np.random.default_rng(1000 * K + w)
    names, want, rows = [], [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for name, cls, r in old_families(rng, K) + crafted(rng, K, w):
            for i, v in enumerate(variants(bf16_bits(r))):
                names.append(name + ("", ":rev", ":shift1", ":shift2", ":shift3")[i]); want.append(cls if i == 0 else None); rows.append(v)
    return names, want, np.ascontiguousarray(np.stack(rows))
