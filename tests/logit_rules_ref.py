"""The logit rules of include/lnb.h ("logit rules in the sampling loops") restated in numpy on top of tests/sampler_ref.py -- a helper module, shared by
tests/test_logit_rules_cpu.py (against the serial C++ walk of csrc/lnb_sample.h) and tests/test_gpu_logit_rules.py (against the kernel).

Rules are (repetition_penalty, presence_penalty, frequency_penalty, min_p, ((id, bias value), ...)); counts[j] = occurrences of token j in the counted text.
  0a. c > 0 and rp != 1:                      f = trunc(f > 0 ? f / rp : f * rp)         every operation one numpy float32 operation,
  0b. c > 0 and (presence or frequency != 0):  t = frequency * f32(c); t = presence + t;  every truncation `>> 16`
                                               f = trunc(f - t)
  0c. a bias list:                             f = trunc(f + f32(trunc(bias)))            for every entry, +0 where no id is listed
  4b. M = uint64(f64(min_p) * f64(w_a)); S = {w >= max(M, 1)}: the entries below that are no candidates of anything behind step 4
temperature 0 = ml.Argmax of the adjusted row."""
import math

import numpy as np

import sampler_ref as sr

OFF = (1.0, 0.0, 0.0, 0.0, ())
NINF = 0xFF80


def trunc(f32):
    return (np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def wide(u16):
    return (np.ascontiguousarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def adjust(row_u16, rules, counts=None):
    """step 0 -> the adjusted bf16 row"""
    rp, pres, freq, _, bias = rules
    rp, pres, freq = np.float32(rp), np.float32(pres), np.float32(freq)
    x = np.ascontiguousarray(row_u16, dtype=np.uint16).copy()
    c = np.zeros(x.size, dtype=np.uint32) if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    hit = c > 0
    with np.errstate(all="ignore"):
        if rp != 1 and hit.any():
            f = wide(x[hit])
            x[hit] = trunc(np.where(f > 0, f / rp, f * rp))
        if (pres != 0 or freq != 0) and hit.any():
            t = freq * c[hit].astype(np.float32)
            t = pres + t
            x[hit] = trunc(wide(x[hit]) - t)
        if len(bias):
            b = np.zeros(x.size, dtype=np.uint16)
            for j, v in bias:
                b[j] = trunc(np.array([v], dtype=np.float32))[0]
            x = trunc(wide(x) + wide(b))
    return x


def prepare(row_u16, temperature, top_k, top_p, rules=OFF, counts=None):
    """sampler_ref.prepare on the adjusted row with step 4b's S"""
    x = adjust(row_u16, rules, counts)
    if temperature == 0 or np.float32(rules[3]) == 0:
        return sr.prepare(x, temperature, top_k, top_p)
    y16 = sr.scale(x, temperature)
    y = wide(y16)
    cand = y > -sr.FMAX
    if not cand.any():
        return sr.prepare(x, temperature, top_k, top_p)
    ci = np.nonzero(cand)[0]
    a = int(ci[np.argmax(y[ci])])
    e = sr.exp_table()[y16.astype(np.int64)]
    if math.isinf(e[a]) or e[a] < 2.0 ** -1022:
        return sr.prepare(x, temperature, top_k, top_p)
    E = math.frexp(e[a])[1] - 1
    w = np.zeros(y.size, dtype=np.uint64)
    w[ci] = np.floor(np.ldexp(e[ci], 45 - E)).astype(np.uint64)
    wmin = max(int(np.float64(np.float32(rules[3])) * np.float64(w[a])), 1)
    x = x.copy()
    x[cand & (w < np.uint64(wmin))] = NINF                   # below step 4b's bar: out of S, as an entry of weight 0 is
    return sr.prepare(x, temperature, top_k, top_p)


def sample(row_u16, sampler, rules=OFF, counts=None, pos=0, u=None):
    """-> (token, info)"""
    t, k, p, seed = sampler
    prep = prepare(row_u16, t, k, p, rules, counts)
    return sr.pick(prep, sr.draw(seed, pos) if u is None else u), prep[3]


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------------
def rule_sets(V):
    """each rule alone, and all together"""
    bias = ((3, 2.5), (V // 2, -math.inf), (V - 1, -1.25), (V - 2, 1e-3))
    return {"repetition": (1.3, 0.0, 0.0, 0.0, ()), "presence": (1.0, 0.5, 0.0, 0.0, ()), "frequency": (1.0, 0.0, 0.25, 0.0, ()), "bias": (1.0, 0.0, 0.0, 0.0, bias),
            "min_p": (1.0, 0.0, 0.0, 0.05, ()), "all": (1.3, 0.5, 0.25, 0.05, bias)}


def counted_rows(rng, rows_u16):
    """sparse occurrence counts for llama-like rows: a few hundred ids, each row's argmax and its last two entries among them"""
    R, V = rows_u16.shape
    c = np.zeros((R, V), dtype=np.uint32)
    for r in range(R):
        ids = rng.integers(0, V, size=min(300, V // 3))
        c[r, ids] = rng.integers(1, 6, size=ids.size)
        c[r, [sr.argmax(rows_u16[r]), V - 1, V - 2]] = (3, 1, 2)
    return c


SAMPLERS = ((1.0, 0, 1.0), (0.7, 40, 0.9), (0.0, 0, 1.0), (1.5, 0, 0.5))


def crafted(V):
    """[(name, row u16 [V], counts u32 [V], (temperature, top_k, top_p), rules, token that must come out or None, boundary_draws)].  A = 5 sits in an aligned
    group of a lane, B = V - 3 in the row's last (at an odd V: element-wise) group.  In the flip rows A beats B by ONE bf16 step until the rule acts on A."""
    A, B = 5, V - 3
    out = []

    def make(fill, a, b, ca):
        row = np.full(V, fill, dtype=np.uint16); row[A] = a; row[B] = b
        c = np.zeros(V, dtype=np.uint32); c[A] = ca
        return row, c

    greedy, plain = (0.0, 0, 1.0), (1.0, 0, 1.0)
    for smp in (greedy, (0.7, 0, 1.0)):                      # temperature 0 and != 1
        row, c = make(sr.bf(-4.0), 0x4001, 0x4000, 1)        # 2.0078 / 1.5 < 2.0
        out.append(("repetition_flips_a_positive_maximum", row, c, smp, (1.5, 0.0, 0.0, 0.0, ()), B if smp is greedy else None, False))
        row, c = make(sr.bf(-8.0), 0xBFFF, 0xC000, 2)        # -1.992 * 1.5 < -2.0
        out.append(("repetition_flips_a_negative_maximum", row, c, smp, (1.5, 0.0, 0.0, 0.0, ()), B if smp is greedy else None, False))
        row, c = make(sr.bf(-1.0), 0x0000, 0x8000, 1); c[B] = 4          # +0 * rp and -0 * rp stay zeros, equal: the lower index
        out.append(("repetition_leaves_the_zeros_tied", row, c, smp, (1.5, 0.0, 0.0, 0.0, ()), A if smp is greedy else None, False))
        row, c = make(sr.bf(-4.0), 0x4041, 0x4040, 70000)    # 3.0156 - 1e-5 * 70000 < 3.0; f32(70000) is exact
        out.append(("frequency_with_a_count_of_70000", row, c, smp, (1.0, 0.0, 1e-5, 0.0, ()), B if smp is greedy else None, False))
        row, c = make(sr.bf(-4.0), 0x4041, 0x4040, 1)
        out.append(("presence_flips_the_maximum", row, c, smp, (1.0, 0.5, 0.0, 0.0, ()), B if smp is greedy else None, False))
        row, c = make(sr.bf(-4.0), 0x4041, 0x4040, 0); row[77] = sr.bf(1.0)       # the maximum banned, B pushed below 77 + 2.5
        out.append(("minus_inf_bias_on_the_maximum", row, c, smp, (1.0, 0.0, 0.0, 0.0, ((A, -math.inf), (77, 2.5), (B, -0.5))), 77 if smp is greedy else None, False))
    # min-p: the maximum is 0 (e = 1, w_a = 2^45); B = -20.75 weighs about 2^15; min_p * 2^45 steps by 2^-9 there, so an M of exactly w_B and one of w_B + 1 exist
    row = np.full(V, NINF, dtype=np.uint16); row[[A, 40, 41, V // 2]] = [0, sr.bf(-5.0), sr.bf(-5.0), sr.bf(-2.0)]; row[B] = sr.bf(-20.75)
    wb = int(np.floor(np.ldexp(sr.exp_table()[sr.bf(-20.75)], 45)))
    zero = np.zeros(V, dtype=np.uint32)
    for name, m in (("min_p_bar_equals_a_weight_kept", wb), ("min_p_bar_one_above_a_weight_dropped", wb + 1)):
        p = float(np.float32((m + 0.5) / 2.0 ** 45))
        assert int(np.float64(np.float32(p)) * 2.0 ** 45) == m
        out.append((name, row, zero, plain, (1.0, 0.0, 0.0, p, ()), None, True))
    row = np.full(V, sr.bf(-2.0), dtype=np.uint16); row[[0, 499, V - 1]] = [sr.bf(1.5), sr.bf(2.5), sr.bf(2.0)]
    c = np.zeros(V, dtype=np.uint32); c[[499, V - 1, 7]] = (2, 1, 9)
    out.append(("draws_on_every_boundary_under_all_rules", row, c, (0.7, 0, 0.95), (1.2, 0.25, 0.125, 0.01, ((0, 0.75), (8, -math.inf))), None, True))
    return out
