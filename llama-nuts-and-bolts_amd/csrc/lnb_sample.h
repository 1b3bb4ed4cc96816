// lnb_sample.h -- the definition of "the sampled token" (include/lnb.h: lnb_sampler): plain C++ that includes nothing.  sample_kernel of
// lnb_kernels.hip uses the scalar pieces on the device; tests/native/sample_test.cpp runs lnb_sample_row_serial on the host under the sanitizers.
//
// One bf16 logits row x[0..V), a sampler {temperature, top_k, top_p, seed} and the position pos of the step's input token give one token:
//   1. y_j = trunc_bf16(f32(x_j) / temperature)              (ml.DivToScalar; temperature 1 leaves the row as it is)
//   2. candidates = ml.Argmax's: y_j not NaN and > -MaxFloat32; none: token -1
//   3. e_j = etab[y_j] (exp(double(bf16)) of the host C library, all 65536 patterns); a = first maximum of y, e_max = e_a;
//      e_max = +inf or below 2^-1022: the row is DEGENERATE and the token is a
//   4. E = the exponent of e_max, w_j = floor(e_j * 2^(45 - E)) as an unsigned 64-bit integer (a shift of e_j's significand: exact); S = {j: w_j >= 1}
//   5. S is ordered by y descending, the lowest index first among equal values (+0 and -0 are equal)
//   6. top_k > 0 keeps the first min(top_k, |S|) entries (0: all of S); W1 = their weight sum
//   7. top_p < 1 keeps the shortest prefix of those whose weight sum is >= P = floor(f64(top_p) * f64(W1)), at least one entry
//   8. W_K = the kept weight; u = splitmix64(splitmix64(seed) ^ (uint64(pos) * 0x9E3779B97F4A7C15)); r = (u * W_K) >> 64; the token is the first
//      kept index, in INDEX order, at which the running kept weight exceeds r
// Everything behind the table lookup is integer arithmetic, so a parallel kernel, this serial walk and a Python restatement give the same token.
// Steps 6 and 7 each come down to a pair (threshold key t, number m of entries kept among those whose key equals t, the lowest indices first).
#pragma once

#ifndef LNB_SAMPLE_FN
#define LNB_SAMPLE_FN static inline      // (the device build defines it with the device attributes before including this file)
#endif
#ifndef LNB_SAMPLE_FDIV
#define LNB_SAMPLE_FDIV(a, b) ((a) / (b))   // one IEEE f32 division (the device build names its correctly rounded one)
#endif

#define LNB_SAMPLE_MAX_V 131072          // every weight sum stays below 2^63: 131072 weights below 2^46

typedef unsigned long long lnbs_u64;
typedef unsigned int lnbs_u32;
typedef unsigned short lnbs_u16;

struct LnbSampler { float temperature, top_p; int top_k, reserved; lnbs_u64 seed; };                           // = lnb_sampler of lnb.h
struct LnbSampleInfo { lnbs_u64 w_all, w_topk, w_kept; int n_candidates, n_kept, degenerate, pad; };           // = lnb_sample_info of lnb.h

LNB_SAMPLE_FN lnbs_u64 lnb_sample_splitmix64(lnbs_u64 z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// u of step 8: a function of the seed and the position alone
LNB_SAMPLE_FN lnbs_u64 lnb_sample_draw(lnbs_u64 seed, int pos) {
    return lnb_sample_splitmix64(lnb_sample_splitmix64(seed) ^ ((lnbs_u64)(long long)pos * 0x9E3779B97F4A7C15ULL));
}
// (a * b) >> 64
LNB_SAMPLE_FN lnbs_u64 lnb_sample_mulhi(lnbs_u64 a, lnbs_u64 b) {
    const lnbs_u64 al = a & 0xFFFFFFFFULL, ah = a >> 32, bl = b & 0xFFFFFFFFULL, bh = b >> 32;
    const lnbs_u64 ll = al * bl, lh = al * bh, hl = ah * bl, hh = ah * bh;
    const lnbs_u64 mid = (ll >> 32) + (lh & 0xFFFFFFFFULL) + (hl & 0xFFFFFFFFULL);
    return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}
// step 1 on one entry
LNB_SAMPLE_FN lnbs_u16 lnb_sample_scale(lnbs_u16 x16, float temperature) {
    lnbs_u32 b = (lnbs_u32)x16 << 16;
    float f, q;
    __builtin_memcpy(&f, &b, 4);
    q = LNB_SAMPLE_FDIV(f, temperature);
    __builtin_memcpy(&b, &q, 4);
    return (lnbs_u16)(b >> 16);
}
// y -> a key that orders as step 5 does: larger y = larger key, +0 and -0 share one, 0 = no candidate (NaN, -inf).  Candidates have keys >= 0x81.
LNB_SAMPLE_FN lnbs_u32 lnb_sample_key(lnbs_u16 y16) {
    const lnbs_u32 mag = y16 & 0x7FFFu;
    if (mag > 0x7F80u) return 0;                             // NaN
    if (y16 & 0x8000u) return mag == 0x7F80u ? 0 : 0x8000u - mag;   // -inf is no candidate (not > -MaxFloat32)
    return 0x8000u | mag;
}
// the bf16 pattern of a candidate's key (the +0 of the two zeros: their exp is the same)
LNB_SAMPLE_FN lnbs_u16 lnb_sample_key_bits(lnbs_u32 key) {
    return key >= 0x8000u ? (lnbs_u16)(key & 0x7FFFu) : (lnbs_u16)(0x8000u | (0x8000u - key));
}
LNB_SAMPLE_FN lnbs_u64 lnb_sample_f64_bits(double d) { lnbs_u64 b; __builtin_memcpy(&b, &d, 8); return b; }
// step 3: e_max = +inf (or NaN) or below 2^-1022 (zero, subnormal)
LNB_SAMPLE_FN int lnb_sample_degenerate(lnbs_u64 emax_bits) {
    const int ef = (int)((emax_bits >> 52) & 0x7FF);
    return ef == 0x7FF || ef == 0;
}
LNB_SAMPLE_FN int lnb_sample_exponent(lnbs_u64 emax_bits) { return (int)((emax_bits >> 52) & 0x7FF) - 1023; }
// step 4: floor(e * 2^(45 - E)) for 0 <= e < 2^(E + 1), from e's bits
LNB_SAMPLE_FN lnbs_u64 lnb_sample_weight(lnbs_u64 e_bits, int E) {
    // branch-free (the kernel runs eight of these side by side): e = m * 2^(ej - 52) with the implicit bit for a normal e, ej = max(ef, 1) - 1023
    const lnbs_u32 ef = (lnbs_u32)(e_bits >> 52) & 0x7FFu;
    const lnbs_u32 ef1 = ef ? ef : 1u;
    const lnbs_u64 m = (e_bits & 0xFFFFFFFFFFFFFULL) | ((lnbs_u64)(ef ? 1u : 0u) << 52);
    int sh = 7 + E + 1023 - (int)ef1;                        // 52 - 45 + E - ej; >= 7 because e < 2^(E + 1) for every entry of the row
    sh = sh < 0 ? 0 : sh;
    sh = sh > 63 ? 63 : sh;                                  // m < 2^53: a shift by 63 gives 0, as every larger one would
    return m >> sh;
}
// step 7: P from (top_p, W1) -- one u64 -> f64 conversion, one f64 product, one floor
LNB_SAMPLE_FN lnbs_u64 lnb_sample_p(float top_p, lnbs_u64 w1) {
    const double p = (double)top_p * (double)w1;
    return (lnbs_u64)p;
}

#ifndef LNB_SAMPLE_NO_SERIAL
// The whole rule on one row, serially, as written above.  has_u: pos_or_u is u itself (a test puts r on a boundary), otherwise the position.
// etab = the 65536 exp values.  -> the token (-1: no candidate); info (optional) as lnb_sample_info.  temperature 0 = ml.Argmax(x), info all zero.
LNB_SAMPLE_FN int lnb_sample_row_serial(const lnbs_u16* x16, int V, const double* etab, const LnbSampler* s, int has_u, lnbs_u64 pos_or_u,
                                        LnbSampleInfo* info) {
    LnbSampleInfo z = {0, 0, 0, 0, 0, 0, 0};
    if (info) *info = z;
    const int greedy = s->temperature == 0.0f;
    const float T = greedy ? 1.0f : s->temperature;
    // steps 1-3: the first maximum among the candidates
    int a = -1; lnbs_u32 kmax = 0;
    for (int j = 0; j < V; j++) {
        const lnbs_u32 k = lnb_sample_key(lnb_sample_scale(x16[j], T));
        if (k > kmax) { kmax = k; a = j; }
    }
    if (a < 0 || greedy) return a;
    const lnbs_u64 emax = lnb_sample_f64_bits(etab[lnb_sample_key_bits(kmax)]);
    if (lnb_sample_degenerate(emax)) { z.degenerate = 1; if (info) *info = z; return a; }
    const int E = lnb_sample_exponent(emax);
    // step 4: S as entries per key (equal keys = equal weights)
    static_assert(sizeof(lnbs_u32) == 4 && sizeof(lnbs_u64) == 8, "integer widths");
    lnbs_u32 cnt[65536];
    for (int k = 0; k < 65536; k++) cnt[k] = 0;
    for (int j = 0; j < V; j++) {
        const lnbs_u32 k = lnb_sample_key(lnb_sample_scale(x16[j], T));
        if (!k) continue;
        const lnbs_u64 w = lnb_sample_weight(lnb_sample_f64_bits(etab[lnb_sample_key_bits(k)]), E);
        if (w >= 1) { cnt[k]++; z.n_candidates++; z.w_all += w; }
    }
    // steps 5-6: walk the keys downwards = the order, group by group
    const lnbs_u64 kk = s->top_k > 0 && s->top_k < z.n_candidates ? (lnbs_u64)s->top_k : (lnbs_u64)z.n_candidates;
    lnbs_u32 t1 = kmax, m1 = 0; lnbs_u64 seen = 0, w1 = 0;
    for (lnbs_u32 k = kmax; k >= 1; k--) {
        if (!cnt[k]) continue;
        const lnbs_u64 w = lnb_sample_weight(lnb_sample_f64_bits(etab[lnb_sample_key_bits(k)]), E);
        const lnbs_u64 take = seen + cnt[k] <= kk ? cnt[k] : kk - seen;
        t1 = k; m1 = (lnbs_u32)take; seen += take; w1 += take * w;
        if (seen == kk) break;
    }
    z.w_topk = w1;
    // step 7
    lnbs_u32 t2 = t1, m2 = m1; lnbs_u64 wk = w1, nk = kk;
    if (s->top_p < 1.0f) {
        const lnbs_u64 P = lnb_sample_p(s->top_p, w1);
        lnbs_u64 above = 0, n_above = 0;
        for (lnbs_u32 k = kmax; k >= t1; k--) {
            const lnbs_u64 c = k == t1 ? m1 : cnt[k];
            if (!c) continue;
            const lnbs_u64 w = lnb_sample_weight(lnb_sample_f64_bits(etab[lnb_sample_key_bits(k)]), E);
            if (above + c * w >= P || k == t1) {
                lnbs_u64 need = P > above ? (P - above + w - 1) / w : 0;
                if (need < 1) need = 1;
                if (need > c) need = c;
                t2 = k; m2 = (lnbs_u32)need; nk = n_above + need; wk = above + need * w;
                break;
            }
            above += c * w; n_above += c;
        }
    }
    z.w_kept = wk; z.n_kept = (int)nk;
    if (info) *info = z;
    // step 8
    const lnbs_u64 u = has_u ? pos_or_u : lnb_sample_draw(s->seed, (int)pos_or_u);
    const lnbs_u64 r = lnb_sample_mulhi(u, wk);
    lnbs_u64 run = 0; lnbs_u32 ties = 0;
    for (int j = 0; j < V; j++) {
        const lnbs_u32 k = lnb_sample_key(lnb_sample_scale(x16[j], T));
        if (k < t2) continue;
        if (k == t2 && ties++ >= m2) continue;
        run += lnb_sample_weight(lnb_sample_f64_bits(etab[lnb_sample_key_bits(k)]), E);
        if (run > r) return j;
    }
    return -1;                                               // (not reached: run ends at W_K > r)
}
#endif
