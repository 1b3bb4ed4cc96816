// lnb_ragged_prefix.h -- shared-prefix attention of a RAGGED pass (lnb_model_set_many_shared_prefix): the passes of lnb_forward_append_many and of the
// lnb_decode_speculative*_many calls, whose columns are one-token steps of SEVERAL rows per member.  Included in lnb_kernels.hip behind lnb_shared_prefix.h
// (same translation unit: sp_row, sp_idx_elem, ASP_NT and everything that header borrows).
//
// Rows, tiles, dead rows and the scratch are the shared form's (lnb_shared_prefix.h): row r = column * G + (h mod G) of a KV head, tiles of 16, a dead row of
// the last tile aliases the last live row, one 8-byte index word per lane and 16-position tile, one z_part sum per 256 positions.  What a ragged pass adds is
// that consecutive columns belong to ONE member: they share the source's rows [0, n_pos) with everybody and that member's own rows [n_pos, T) with each other.
// Every row's positions are walked in ascending j in four segments, in the PV launch on the same accumulator registers:
//   A  [0, P16), P16 = n_pos & ~15                    the source's K / V on v_mfma_f32_16x16x4_f32, as the shared form
//   B  [P16, Q16), Q16 = min(T_row, (n_pos+15) & ~15) the mixed tile: source below n_pos, the member's own cache from n_pos on; vector pipe, multiply then add,
//                                                     a masked position is skipped
//   C  [Q16, R16), R16 = (min T of the tile) & ~15    only a UNIFORM tile: all 16 rows (live rows and their aliases) point at one member cache -- a wave-uniform
//                                                     comparison of the rows' ck pointers, made on the device because spec_many_pack_kernel picks the columns
//                                                     there.  The member's OWN K (its own stride) and V on the matrix cores, four positions per instruction;
//                                                     every row of the tile is unmasked below R16, so there is no mask.  (T_row < (n_pos+15) & ~15 for some
//                                                     row makes R16 <= Q16: the segment is empty.)
//   D  [max(Q16, R16), T_row)                         vector pipe as B.  A tile that is not uniform runs all of [P16, T_row) this way: the shared form's loop.
// Segment C is exact for the reason A is: the matrix instruction is the k-ordered chain, and p and v are bf16, so its fused product differs from multiply-then-
// add only where a single product is no normal f32 (lnb_shared_prefix.h, NOTES.md section 2).
//
//   attn_ragged_scores_kernel<HD>   grid (blocks of 256 positions, row tiles, KV heads), block 256.  A wave owns four 16-position tiles of its block; each is
//       a matrix-core tile against the source (A), against the member (C), or left to the per-position chains (B, D: one position per thread, mac8).
//   attn_ragged_pv_kernel<HD>       grid (row tiles, HD / 32, KV heads), one wave each, two 16 x 16 accumulators (32 output dims).  The matrix segments run a
//       register pipeline two tiles deep: while tile jt multiplies, the exp-table entries and V words of jt + 1 and the index word of jt + 2 are in flight
//       (the two dependent loads in front of every tile are what the shared form's loop waits for: profiles/shared_prefix_attention.md).  No arithmetic
//       changes.  Uncertified elements or force_zseq: lanes 0..15 walk the serial f64 sums and the pass is redone, as in the shared form.  The wave with
//       blockIdx.y == 0 counts a tile that took segment C in own_tiles, once per launch.
#pragma once

// where segment C of a tile ends (C0 = (n_pos + 15) & ~15 is where it begins; the result is C0 for "no segment C").  me: row fi of the tile in every lane.
DEVINL int rg_own_end(const AttnRaggedParams& rp, const SpRow& me, int C0) {
    int Tmin = me.T;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) { const int o = __shfl_xor(Tmin, m); Tmin = o < Tmin ? o : Tmin; }
    const uint64_t k = (uint64_t)(uintptr_t)me.ck;
    const uint32_t k0h = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(k >> 32)), k0l = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)k);
    const uint64_t k0 = ((uint64_t)k0h << 32) | (uint64_t)k0l;      // (the builtin returns a signed int: widened as it is, a low word with its top bit set would smear over the high one)
    const bool uniform = __builtin_amdgcn_ballot_w64(k != k0) == 0;
    const int R16 = Tmin & ~15;
    return uniform && !rp.no_own && R16 > C0 ? R16 : C0;
}

template <int HD> __global__ __launch_bounds__(ASP_NT) void attn_ragged_scores_kernel(AttnRaggedParams rp) {
    constexpr int NK = HD / 8;
    __shared__ __attribute__((aligned(16))) float qs[16 * HD];
    __shared__ double zs[ASP_NT / 64][16];
    __shared__ int rT[16], rLen[16];
    __shared__ const uint16_t* rK[16];
    const AttnSharedParams& sp = rp.s;
    const AttnParams& p = sp.a;
    const int tid = threadIdx.x, lane = tid & 63, fi = lane & 15, fk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.y, kvh = blockIdx.z;
    const int j0 = (int)blockIdx.x * ASP_NT, P16 = sp.n_pos & ~15, C0 = (sp.n_pos + 15) & ~15;
    const SpRow me = sp_row(sp, kvh, tile * 16 + fi);        // column i = fi of the S^T tile
    int Tmax = me.T;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) { const int o = __shfl_xor(Tmax, m); Tmax = o > Tmax ? o : Tmax; }
    if (j0 >= Tmax) return;                                  // (uniform over the workgroup: the grid is sized for the largest capacity)
    const int C1 = rg_own_end(rp, me, C0);                   // (every wave holds all 16 rows: the same value in all four)
    uint64_t* const strip = sp.idx + ((size_t)kvh * sp.n_tiles + tile) * (size_t)sp.njt * 64;
    {   // the tile's query rows as f32 (the per-row chains), and what those chains need of each row
        const SpRow rq = sp_row(sp, kvh, tile * 16 + (tid >> 4));
        const uint16_t* q = p.q + ((size_t)rq.s * p.H + rq.h) * HD + (tid & 15) * (HD / 16);
#pragma unroll
        for (int d = 0; d < HD / 16; d++) qs[(tid >> 4) * HD + (tid & 15) * (HD / 16) + d] = bf_wide(q[d]);
        if ((tid & 15) == 0) { rT[tid >> 4] = rq.T; rLen[tid >> 4] = rq.seq_len; rK[tid >> 4] = rq.ck; }
    }
    // ---- segments A and C: this wave's four 16-position tiles, each wholly inside [0, P16) (the source's K), inside [C0, C1) (the member's own) or neither
    double zacc = 0.0;
    const int jw = j0 + wave * 64;
    if (jw < P16 || (jw < C1 && jw + 64 > C0)) {
        const uint32_t sel = 0x0c0cu | ((uint32_t)(2 * fk) << 16) | ((uint32_t)(2 * fk + 1) << 24);      // element kk of a 4-element word pair (attn_mfma_kernel)
        float qf[2 * NK];                                    // Q[row fi][8 c + kk], Q[row fi][8 c + 4 + kk]
        const uint4* q = (const uint4*)(p.q + ((size_t)me.s * p.H + me.h) * HD);
#pragma unroll
        for (int c = 0; c < NK; c++) {
            const uint4 u = q[c];
            qf[2 * c] = __uint_as_float(__builtin_amdgcn_perm(u.y, u.x, sel));
            qf[2 * c + 1] = __uint_as_float(__builtin_amdgcn_perm(u.w, u.z, sel));
        }
        const uint4* const ksrc = (const uint4*)sp.src_k + (size_t)kvh * NK * sp.src_len;
        const uint4* const kown = (const uint4*)me.ck + (size_t)kvh * NK * me.seq_len;       // (read only on a uniform tile: every lane's member is the same)
        for (int t = 0; t < 4; t++) {
            const int jb = jw + t * 16;
            const bool own = jb >= C0 && jb < C1;            // (uniform; P16, C0 and C1 are multiples of 16: a tile lies wholly on one side)
            if (jb >= P16 && !own) continue;
            uint4 k[NK];
            attn_load_k<NK>(k, own ? kown : ksrc, own ? me.seq_len : sp.src_len, jb + 4 * (fi & 3) + (fi >> 2));      // operand row m = fi is position 4 (m & 3) + (m >> 2)
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NK; c++) {                   // MatMul q.k, d ascending (operations_matmul.go:37-55)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(__builtin_amdgcn_perm(k[c].y, k[c].x, sel)), qf[2 * c], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(__builtin_amdgcn_perm(k[c].w, k[c].z, sel)), qf[2 * c + 1], acc, 0, 0, 0);
            }
            // D row 4 fk + r = position jb + 4 r + fk: slot r of the word is k-group r of the PV launch's lane (fi, fk)
            const uint16_t s0 = bf_trunc(acc[0]), s1 = bf_trunc(acc[1]), s2 = bf_trunc(acc[2]), s3 = bf_trunc(acc[3]);       // llamatransformer.go:459
            strip[(size_t)(jb >> 4) * 64 + lane] = (uint64_t)s0 | ((uint64_t)s1 << 16) | ((uint64_t)s2 << 32) | ((uint64_t)s3 << 48);
            zacc += (p.exp_tab[s0] + p.exp_tab[s1]) + (p.exp_tab[s2] + p.exp_tab[s3]);     // / sqrt(hd) :464, exp impl:498: tabulated (exp_table_kernel)
        }
    }
    zacc += __shfl_xor(zacc, 16); zacc += __shfl_xor(zacc, 32);      // the four k-group lanes of row fi
    if (lane < 16) zs[wave][lane] = zacc;
    __syncthreads();
    // ---- segments B and D: one position per thread, the per-row chain of the long scores form, wherever the block is not wholly matrix-core ground
    const int j = j0 + tid;
    if (j0 + ASP_NT > P16 && !(j0 >= C0 && j0 + ASP_NT <= C1)) {
        uint16_t* const strip16 = (uint16_t*)strip;
        const bool mine = j >= P16 && !(j >= C0 && j < C1);
        for (int i = 0; i < 16; i++) {
            const int Ti = rT[i];
            if (Ti <= j0 || Ti <= P16) continue;             // (uniform)
            double ev = 0.0;
            if (mine && j < Ti) {
                const bool own = j >= sp.n_pos;
                const int len = own ? rLen[i] : sp.src_len;
                const uint4* kb = (const uint4*)(own ? rK[i] : sp.src_k) + (size_t)kvh * NK * len;
                uint4 k[NK];
                attn_load_k<NK>(k, kb, len, j);
                float acc = 0.0f;
#pragma unroll
                for (int c = 0; c < NK; c++) acc = mac8(acc, *(const float4*)(qs + i * HD + c * 8), *(const float4*)(qs + i * HD + c * 8 + 4), k[c]);
                const uint16_t s16 = bf_trunc(acc);
                strip16[sp_idx_elem(i, j)] = s16;
                ev = p.exp_tab[s16];
            }
            ev = wave_sum_f64(ev);
            if (lane == 0) zs[wave][i] += ev;
        }
        __syncthreads();
    }
    if (tid < 16) p.z_part[(((size_t)kvh * sp.n_tiles + tile) * 16 + tid) * ((p.seq_len + ASP_NT - 1) / ASP_NT) + blockIdx.x] = (zs[0][tid] + zs[1][tid]) + (zs[2][tid] + zs[3][tid]);
}

template <int HD> __global__ __launch_bounds__(64) void attn_ragged_pv_kernel(AttnRaggedParams rp) {
    const AttnSharedParams& sp = rp.s;
    const AttnParams& p = sp.a;
    const int lane = threadIdx.x, fi = lane & 15, fk = lane >> 4;
    const int tile = blockIdx.x, kvh = blockIdx.z;
    const int G = p.H / p.KVH, nrows = p.S * G;
    const int P16 = sp.n_pos & ~15, C0 = (sp.n_pos + 15) & ~15, nblk_max = (p.seq_len + ASP_NT - 1) / ASP_NT;
    const size_t vrow = (size_t)p.KVH * HD, voff = (size_t)kvh * HD + (size_t)blockIdx.y * 32 + 2 * fi;      // B operand column n = fi: output dims voff, voff + 1
    const uint64_t* const strip = sp.idx + ((size_t)kvh * sp.n_tiles + tile) * (size_t)sp.njt * 64;
    const uint16_t* const strip16 = (const uint16_t*)strip;
    // ---- Z estimate of row fi (the A operand's row): the per-block tree sums in block order; rows 4 fk + r (the accumulators') take theirs from lane 4 fk + r
    const SpRow ra = sp_row(sp, kvh, tile * 16 + fi);
    const int C1 = rg_own_end(rp, ra, C0);
    double zt = 0.0;
    {
        const double* zp = p.z_part + (((size_t)kvh * sp.n_tiles + tile) * 16 + fi) * nblk_max;
        const int nblk = (ra.T + ASP_NT - 1) / ASP_NT;
        for (int b = 0; b < nblk; b++) zt += zp[b];
    }
    const CertZ cza = cert_z(zt, ra.T);
    SpRow rd[4]; CertZ czd[4]; int tmax = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        rd[r] = sp_row(sp, kvh, tile * 16 + 4 * fk + r);
        czd[r] = cert_z(__shfl(zt, 4 * fk + r), rd[r].T);
        tmax = rd[r].T > tmax ? rd[r].T : tmax;
    }
    if (lane == 0 && blockIdx.y == 0 && C1 > C0 && rp.own_tiles) atomicAdd(rp.own_tiles, 1ull);
    f32x4 acc0, acc1;
    int bad = 0;
    // one pass over all positions; exact: p = trunc(f32(e / Z)) with the walked serial sums (za: row fi's, zd: rows 4 fk + r), else cert_p (sets bad)
    auto run_pv = [&](bool exact, double za, const double (&zd)[4]) {
        acc0 = f32x4{0.f, 0.f, 0.f, 0.f}; acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
        // tiles [jt0, jt1) of vb's rows on the matrix cores: MatMul p.v, j ascending (llamatransformer.go:504-514), positions 16 jt + 4 g + kk;
        // A = p[i][j] = cert_p(exp_tab[idx]), B = V[j][d].  Look-ahead indices are clamped to the segment's last tile: in bounds, never used.
        auto mfma_seg = [&](const uint16_t* vb, int jt0, int jt1) {
            if (jt0 >= jt1) return;
            const int last = jt1 - 1;
            auto ld_w = [&](int jt) { return strip[(size_t)(jt < last ? jt : last) * 64 + lane]; };
            auto ld_e = [&](double (&e)[4], uint64_t w) {
#pragma unroll
                for (int g = 0; g < 4; g++) e[g] = p.exp_tab[(unsigned)(w >> (16 * g)) & 0xFFFFu];
            };
            auto ld_v = [&](uint32_t (&v)[4], int jt) {
#pragma unroll
                for (int g = 0; g < 4; g++) v[g] = *(const uint32_t*)(vb + (size_t)((jt < last ? jt : last) * 16 + 4 * g + fk) * vrow);
            };
            double e[4], en[4]; uint32_t vv[4], vn[4];
            uint64_t wn = ld_w(jt0 + 1);
            ld_e(e, ld_w(jt0)); ld_v(vv, jt0);
            for (int jt = jt0; jt < jt1; jt++) {
                ld_e(en, wn); ld_v(vn, jt + 1);              // tile jt + 1: its table entries and V words
                wn = ld_w(jt + 2);                           // tile jt + 2: its index word
                float pa[4];
#pragma unroll
                for (int g = 0; g < 4; g++) pa[g] = exact ? alp_p(e[g], za) : cert_p(e[g], cza, bad);        // impl:506 + ToBFloat16 :493
                __builtin_amdgcn_sched_barrier(0);           // the quotients in one batch AHEAD of the run of matrix instructions (lnb_batch_kernels.h)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[g], bf_lo(vv[g]), acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[g], bf_hi(vv[g]), acc1, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < 4; g++) { e[g] = en[g]; vv[g] = vn[g]; }
            }
        };
        // positions [ja, jb) of each row up to its own T: multiply, then add, on the same accumulators (D layout: rows 4 fk + r, column fi)
        auto vec_seg = [&](int ja, int jb) {
            jb = jb < tmax ? jb : tmax;
            for (int j = ja; j < jb; j++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (j >= rd[r].T) continue;
                    const double e = p.exp_tab[strip16[sp_idx_elem(4 * fk + r, j)]];
                    const float pj = exact ? alp_p(e, zd[r]) : cert_p(e, czd[r], bad);
                    const uint32_t v = *(const uint32_t*)((j < sp.n_pos ? sp.src_v : rd[r].cv) + (size_t)j * vrow + voff);
                    acc0[r] = __fadd_rn(acc0[r], __fmul_rn(pj, bf_lo(v)));
                    acc1[r] = __fadd_rn(acc1[r], __fmul_rn(pj, bf_hi(v)));
                }
            }
        };
        mfma_seg(sp.src_v + voff, 0, P16 >> 4);              // A
        vec_seg(P16, C0);                                    // B
        mfma_seg(ra.cv + voff, C0 >> 4, C1 >> 4);            // C (a uniform tile: ra.cv is every row's)
        vec_seg(C1, tmax);                                   // D (C1 == C0: B's loop goes on)
    };
    const double none[4] = {0.0, 0.0, 0.0, 0.0};
    if (!p.force_zseq) run_pv(false, 0.0, none);
    if (p.force_zseq || __builtin_amdgcn_ballot_w64(bad != 0) != 0) {
        // the reference's serial sum, j ascending, f64 (operations_impl.go:492-499): lane i < 16 walks row i, a 16-position tile's look-ups in flight ahead of its adds
        double z = 0.0;
        if (lane < 16) {
            for (int jb = 0; jb < ra.T; jb += 16) {
                uint64_t w[4]; double e[16];
#pragma unroll
                for (int kk = 0; kk < 4; kk++) w[kk] = strip[(size_t)(jb >> 4) * 64 + kk * 16 + lane];
#pragma unroll
                for (int u = 0; u < 16; u++) e[u] = p.exp_tab[(unsigned)(w[u & 3] >> (16 * (u >> 2))) & 0xFFFFu];
#pragma unroll
                for (int u = 0; u < 16; u++) z += (jb + u < ra.T) ? e[u] : 0.0;
            }
        }
        if (lane == 0 && blockIdx.y == 0 && p.zseq_count) atomicAdd(p.zseq_count, nrows - tile * 16 < 16 ? nrows - tile * 16 : 16);
        double zd[4];
#pragma unroll
        for (int r = 0; r < 4; r++) zd[r] = __shfl(z, 4 * fk + r);
        run_pv(true, __shfl(z, fi), zd);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (tile * 16 + 4 * fk + r >= nrows) continue;
        const int s = rd[r].s, k0 = rd[r].h * HD + (int)blockIdx.y * 32 + 2 * fi;
        if (p.out_xt) {                                      // the B-operand layout of the wo product (columns, column groups) or rows: al_store's two destinations
            uint16_t* o = p.out_xt + xt_group(s, p.H * HD);
            o[xt_index(s & 15, k0)] = bf_trunc(acc0[r]); o[xt_index(s & 15, k0 + 1)] = bf_trunc(acc1[r]);
        } else *(uint32_t*)(p.out + (size_t)s * p.H * HD + k0) = (uint32_t)bf_trunc(acc0[r]) | ((uint32_t)bf_trunc(acc1[r]) << 16);
    }
}
