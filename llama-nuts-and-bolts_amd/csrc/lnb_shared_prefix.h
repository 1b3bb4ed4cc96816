// lnb_shared_prefix.h -- shared-prefix attention of a batched decode step (lnb_batch_set_shared_prefix): the K and V rows [0, n_pos) of ONE source
// context serve every member of the batch.  Included near the end of lnb_kernels.hip (one translation unit: the exp table index, cert_z / cert_p, alp_p,
// attn_load_k, mac8, wave_sum_f64 and xt_index / xt_group are the decode kernels' own).
//
// Below the shared length every (member, query head) row of one KV head multiplies the same K rows and adds the same V rows in the same j order: the shape of
// the exact prefill attention.  Rows of KV head g are numbered r = s * G + (h mod G) (member-major, G = H / KVH) and cut into tiles of 16; a tile is one
// operand of v_mfma_f32_16x16x4_f32, which is the reference's k-ordered chain bit for bit (NOTES.md 5.6).  Rows past n * G in the last tile alias the last
// live row (they compute its duplicate and store nothing), so no operand is ever a made-up zero: V may hold inf, and +0 * inf is a NaN.
//
//   attn_shared_scores_kernel<HD>   grid (blocks of 256 positions, row tiles, KV heads), block 256.  Positions below P16 = n_pos & ~15: a wave holds its
//       tile's 16 query rows as one MFMA operand and walks four 16-position tiles of the source's K (HD / 4 dependent MFMAs each, d ascending), then per
//       element truncates and stores the SIXTEEN-BIT exp-table index (2 bytes per score instead of the 8 of the f64 exponential).  Row m of the K operand
//       is position 4 (m & 3) + (m >> 2) of the tile, so the lane that ends up with the four scores of (row i, k-group slot kk) is exactly the lane whose
//       A operand they are in the PV launch: an 8-byte word per lane and tile, written and read back coalesced, no transpose.  Positions from P16 up to each
//       row's own T = pos + 1: one position per thread, the per-row f32 chain of the long scores form (mac8), from the source below n_pos and from the
//       member's own cache (its own K stride) from n_pos on; same scratch.  Per block and row one tree sum of e -> z_part (an ESTIMATE of Z: cert_z).
//   attn_shared_pv_kernel<HD>       grid (row tiles, HD / 32, KV heads), one wave each: the accumulators are two 16 x 16 MFMA tiles out[i][d] (32 output
//       dims, so each p is evaluated HD / 32 times -- 4 at head_dim 128 -- instead of the HD / 16 of a 16-dim slice; the waves stay independent, no
//       barrier).  Z per row from z_part; prefix chain j = 0 .. P16 - 1 on the matrix cores, four positions per instruction, j ascending inside and across
//       instructions, A = p[i][j] = cert_p(exp_tab[idx]), B = V[j][d] of the source: one V read serves 16 rows.  Then, on the same accumulator registers,
//       multiply-then-add on the vector pipe for j = P16 .. T_i - 1 of each row (source V below n_pos, the member's own from n_pos on; lanes masked per
//       row, a masked position is skipped, never added as +0 * v).  If an element of the tile cannot be certified, or force_zseq is set, lanes 0..15 walk the
//       16 rows' serial f64 sums in j order and the whole pass is redone with p = trunc(f32(e / Z)); counted per live row in zseq_count.
//
// Fused product: the MFMA fuses p * v where the vector kernels multiply, round, then add.  p and v are bf16 values, so the product is exact in f32 and
// both give the same bits unless a single product is not a normal f32 (it underflows below 2^-126 or overflows): the deviation NOTES.md section 2
// documents for the prefill attention.  The q.k chains are fused in every decode kernel (mac8), so the scores have no such case.
//
// A member whose state word lies below n_pos (only a frozen member can: the entry points refuse a live one) is computed at T = n_pos: defined, in
// bounds, and read by nobody.
#pragma once

constexpr int ASP_NT = 256;                                  // positions per scores workgroup = the granularity of z_part (ALS_NT)
static_assert(ASP_NT == ALS_NT, "z_part holds one partial sum per 256 positions in every form");

struct SpRow { int s, h, T, seq_len; const uint16_t* ck; const uint16_t* cv; };
DEVINL SpRow sp_row(const AttnSharedParams& sp, int kvh, int r) {
    const AttnParams& p = sp.a;
    const int G = p.H / p.KVH, nrows = p.S * G;
    r = r < nrows ? r : nrows - 1;                           // a dead row of the ragged last tile: the last live row's duplicate
    SpRow a; a.s = r / G; a.h = kvh * G + r % G;
    a.seq_len = p.btab->seq_len[a.s]; a.ck = p.bkv->ck[a.s]; a.cv = p.bkv->cv[a.s];
    int T = p.btab->st[a.s]->pos + 1;
    T = T < sp.n_pos ? sp.n_pos : T;
    a.T = T > a.seq_len ? a.seq_len : T;                     // (n_pos < every member's capacity: the entry point checked it)
    return a;
}
// the 16-bit index of (row i of the tile, position j) inside the tile's strip: word (j >> 4, lane (j & 3) * 16 + i), slot (j & 15) >> 2
DEVINL size_t sp_idx_elem(int i, int j) { return ((size_t)(j >> 4) * 64 + (size_t)((j & 3) * 16 + i)) * 4 + (size_t)((j & 15) >> 2); }

template <int HD> __global__ __launch_bounds__(ASP_NT) void attn_shared_scores_kernel(AttnSharedParams sp) {
    constexpr int NK = HD / 8;
    __shared__ __attribute__((aligned(16))) float qs[16 * HD];
    __shared__ double zs[ASP_NT / 64][16];
    __shared__ int rT[16], rLen[16];
    __shared__ const uint16_t* rK[16];
    const AttnParams& p = sp.a;
    const int tid = threadIdx.x, lane = tid & 63, fi = lane & 15, fk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.y, kvh = blockIdx.z;
    const int j0 = (int)blockIdx.x * ASP_NT, P16 = sp.n_pos & ~15;
    const SpRow me = sp_row(sp, kvh, tile * 16 + fi);        // column i = fi of the S^T tile
    int Tmax = me.T;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) { const int o = __shfl_xor(Tmax, m); Tmax = o > Tmax ? o : Tmax; }
    if (j0 >= Tmax) return;                                  // (uniform over the workgroup: the grid is sized for the largest capacity)
    uint64_t* const strip = sp.idx + ((size_t)kvh * sp.n_tiles + tile) * (size_t)sp.njt * 64;
    {   // the tile's query rows as f32 (the per-row chains), and what those chains need of each row
        const SpRow rq = sp_row(sp, kvh, tile * 16 + (tid >> 4));
        const uint16_t* q = p.q + ((size_t)rq.s * p.H + rq.h) * HD + (tid & 15) * (HD / 16);
#pragma unroll
        for (int d = 0; d < HD / 16; d++) qs[(tid >> 4) * HD + (tid & 15) * (HD / 16) + d] = bf_wide(q[d]);
        if ((tid & 15) == 0) { rT[tid >> 4] = rq.T; rLen[tid >> 4] = rq.seq_len; rK[tid >> 4] = rq.ck; }
    }
    // ---- positions below P16: the source's K on the matrix cores, four 16-position tiles per wave
    double zacc = 0.0;
    if (j0 + wave * 64 < P16) {
        const uint32_t sel = 0x0c0cu | ((uint32_t)(2 * fk) << 16) | ((uint32_t)(2 * fk + 1) << 24);      // element kk of a 4-element word pair (attn_mfma_kernel)
        float qf[2 * NK];                                    // Q[row fi][8 c + kk], Q[row fi][8 c + 4 + kk]
        const uint4* q = (const uint4*)(p.q + ((size_t)me.s * p.H + me.h) * HD);
#pragma unroll
        for (int c = 0; c < NK; c++) {
            const uint4 u = q[c];
            qf[2 * c] = __uint_as_float(__builtin_amdgcn_perm(u.y, u.x, sel));
            qf[2 * c + 1] = __uint_as_float(__builtin_amdgcn_perm(u.w, u.z, sel));
        }
        const uint4* kbase = (const uint4*)sp.src_k + (size_t)kvh * NK * sp.src_len;
        for (int t = 0; t < 4; t++) {
            const int jb = j0 + wave * 64 + t * 16;
            if (jb >= P16) break;                            // (uniform; P16 is a multiple of 16: a tile lies wholly on one side)
            uint4 k[NK];
            attn_load_k<NK>(k, kbase, sp.src_len, jb + 4 * (fi & 3) + (fi >> 2));      // operand row m = fi is position 4 (m & 3) + (m >> 2)
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
    // ---- positions from P16 on: one position per thread, the per-row chain of the long scores form
    const int j = j0 + tid;
    if (j0 + ASP_NT > P16) {
        uint16_t* const strip16 = (uint16_t*)strip;
        for (int i = 0; i < 16; i++) {
            const int Ti = rT[i];
            if (Ti <= j0 || Ti <= P16) continue;             // (uniform)
            double ev = 0.0;
            if (j >= P16 && j < Ti) {
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

template <int HD> __global__ __launch_bounds__(64) void attn_shared_pv_kernel(AttnSharedParams sp) {
    const AttnParams& p = sp.a;
    const int lane = threadIdx.x, fi = lane & 15, fk = lane >> 4;
    const int tile = blockIdx.x, kvh = blockIdx.z;
    const int G = p.H / p.KVH, nrows = p.S * G;
    const int P16 = sp.n_pos & ~15, nblk_max = (p.seq_len + ASP_NT - 1) / ASP_NT;
    const size_t vrow = (size_t)p.KVH * HD, voff = (size_t)kvh * HD + (size_t)blockIdx.y * 32 + 2 * fi;      // B operand column n = fi: output dims voff, voff + 1
    const uint64_t* const strip = sp.idx + ((size_t)kvh * sp.n_tiles + tile) * (size_t)sp.njt * 64;
    const uint16_t* const strip16 = (const uint16_t*)strip;
    // ---- Z estimate of row fi (the A operand's row): the per-block tree sums in block order; rows 4 fk + r (the accumulators') take theirs from lane 4 fk + r
    const SpRow ra = sp_row(sp, kvh, tile * 16 + fi);
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
    f32x4 acc0, acc1;
    int bad = 0;
    // one pass over all positions; exact: p = trunc(f32(e / Z)) with the walked serial sums (za: row fi's, zd: rows 4 fk + r), else cert_p (sets bad)
    auto run_pv = [&](bool exact, double za, const double (&zd)[4]) {
        acc0 = f32x4{0.f, 0.f, 0.f, 0.f}; acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
        const uint16_t* vsrc = sp.src_v + voff;
        for (int jt = 0; jt < (P16 >> 4); jt++) {            // MatMul p.v, j ascending (llamatransformer.go:504-514): positions 16 jt + 4 g + kk
            const uint64_t w = strip[(size_t)jt * 64 + lane];
            uint32_t vv[4]; float pa[4];
#pragma unroll
            for (int g = 0; g < 4; g++) vv[g] = *(const uint32_t*)(vsrc + (size_t)(jt * 16 + 4 * g + fk) * vrow);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const double e = p.exp_tab[(unsigned)(w >> (16 * g)) & 0xFFFFu];
                pa[g] = exact ? alp_p(e, za) : cert_p(e, cza, bad);                 // impl:506 + ToBFloat16 :493
            }
            __builtin_amdgcn_sched_barrier(0);               // the look-ups and quotients in one batch AHEAD of the run of matrix instructions (lnb_batch_kernels.h)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[g], bf_lo(vv[g]), acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[g], bf_hi(vv[g]), acc1, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        for (int j = P16; j < tmax; j++) {                   // the rows' own ends: multiply, then add, on the same accumulators (D layout: rows 4 fk + r, column fi)
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
