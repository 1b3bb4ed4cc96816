// lnb_tree_verify.h -- a verify pass over a TREE of n-gram drafts (lnb_ctx_set_draft_branches; TreeCols and tree_draft_kernel: lnb_device.h, lnb_kernels.hip).
// Included in lnb_kernels.hip behind lnb_ragged_prefix.h (one translation unit: sp_idx_elem, ASP_NT, the exp table index, cert_z / cert_p, alp_p, attn_load_k,
// mac8, wave_sum_f64, xt_index / xt_group, argmax_block and sample_block are the decode kernels' own -- nothing of their arithmetic is restated here).
//
// The w <= 16 columns of the pass are nodes of a trie and all belong to ONE context.  Column i is the one-token step at position pos + depth[i]; the wq|wk|wv
// epilogue (EPI_QKV_ROPE_SLOT) has rotated its K row by that position and parked its K / V rows in cache slot pos + i.  Column i attends over
//   [0, pos)          the context's rows, shared by every column, and
//   [pos, pos + w)    the pass's own slots, slot pos + j only if bit j of mask[i] is set (j an ancestor of i, or i): every other own slot contributes e = 0
//                     and its score is never computed, read or stored.
// Slots ascend with depth along a root path, so the unmasked positions of a row, in ascending j, are the one-token step's positions 0 .. pos + depth[i] in
// order.  The reference's softmax subtracts no maximum: a masked entry adds +0 to the f64 sum and nothing to the PV chain, so the row is that step's row bit for
// bit (include/lnb.h, lnb_forward_append) for finite V rows.
//
// Rows of KV head g are r = column * G + (h mod G), G = H / KVH, in tiles of 16 -- at the 8B geometry 16 columns x 4 heads = four tiles -- and a dead row of the
// last tile aliases the last live row (lnb_shared_prefix.h).  K and V of [0, pos) are read ONCE per KV head for all columns; the short verify form reads them once
// per (head, column).
//   attn_tree_scores_kernel<HD>   grid (blocks of 256 positions, row tiles, KV heads), block 256.  Positions below P16 = pos & ~15: the tile's 16 query rows as
//       one operand of v_mfma_f32_16x16x4_f32 against four 16-position tiles of K per wave, d ascending, the sixteen-bit exp-table indices out in the PV launch's
//       operand order (the shared form's chain and scratch layout).  Positions [P16, pos + w): one position per thread, the per-row f32 chain (mac8), under the
//       row's mask from pos on.  Per block and row one tree sum of e -> z_part (an ESTIMATE of Z: cert_z).
//   attn_tree_pv_kernel<HD>       grid (row tiles, HD / 32, KV heads), one wave each, two 16 x 16 accumulators.  [0, P16) on the matrix cores, four positions per
//       instruction, j ascending; then multiply-then-add on the same accumulators for [P16, pos + w), a masked slot skipped.  The denominator is certified per
//       row (cert_z with the row's own length pos + depth + 1, cert_p); an uncertified element or force_zseq: lanes 0..15 walk the rows' serial f64 sums in j
//       order (a masked slot adds +0) and the pass is redone with p = trunc(f32(e / Z)).
//   tree_commit_kernel / tree_sample_commit_kernel   the walk from node 0: at node i with token g_i go to the child whose input token is g_i (a trie has at most
//       one), else stop; g is emitted along the path exactly as spec_accept_emit emits; the path goes to TreeCols::path.
//   tree_kv_compact_kernel        grid (16-byte pieces of a row / 256, K | V, layers): the accepted node at depth d sits in slot pos + path[d] and moves to
//       pos + d, depth ascending.  path[d] >= d, so a move never overwrites a later source; a thread owns one 16-byte piece of every row, so the moves of
//       different pieces never meet.  Workgroups return at once when no node moves (a chain-shaped path).
//
// Fused product, as in the shared form (lnb_shared_prefix.h, NOTES.md section 2): over [0, P16) the matrix instruction fuses p * v where the one-token kernels
// multiply, round, then add.  p and v are bf16 values, so the product is exact in f32 and both give the same bits unless a single product is no normal f32
// (it underflows below 2^-126 or overflows); the own slots and the last shared positions run multiply-then-add and have no such case.
// The two attention kernels are the shared form's bodies with another row descriptor and the mask predicate; they are kept as kernels of their own so that
// the shared and ragged kernels compile to the code they had.
//
// Reach: head_dim 128 / 64 and contexts the one-workgroup kernels serve (seq_len <= attn_short_cap); beyond, the host drafts the chain and runs what it ran.
#pragma once

struct TrRow { int col, h, T; uint32_t mask; };
DEVINL TrRow tr_row(const AttnTreeParams& tp, int kvh, int r, int pos) {
    const AttnParams& p = tp.a;
    const int G = p.H / p.KVH, nrows = p.S * G;
    r = r < nrows ? r : nrows - 1;                           // a dead row of the ragged last tile: the last live row's duplicate
    TrRow a; a.col = r / G; a.h = kvh * G + r % G;
    a.mask = tp.tree->mask[a.col]; a.T = pos + tp.tree->depth[a.col] + 1;
    return a;
}
DEVINL bool tr_sees(uint32_t mask, int j, int pos) { return j < pos || ((mask >> (j - pos)) & 1u); }      // (j < pos + 16)
// the end of the pass's own slots; the draft kernel keeps pos + w <= seq_len, the clamp keeps every index in bounds whatever the tables hold
DEVINL int tr_end(const AttnParams& p, int pos) { const int e = pos + p.S; return e < p.seq_len ? e : p.seq_len; }

template <int HD> __global__ __launch_bounds__(ASP_NT) void attn_tree_scores_kernel(AttnTreeParams tp) {
    constexpr int NK = HD / 8;
    __shared__ __attribute__((aligned(16))) float qs[16 * HD];
    __shared__ double zs[ASP_NT / 64][16];
    __shared__ uint32_t rMask[16];
    const AttnParams& p = tp.a;
    const int tid = threadIdx.x, lane = tid & 63, fi = lane & 15, fk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.y, kvh = blockIdx.z;
    int pos = p.btab->st[0]->pos;
    pos = pos < 0 ? 0 : pos < p.seq_len ? pos : p.seq_len - 1;
    const int j0 = (int)blockIdx.x * ASP_NT, P16 = pos & ~15, Tend = tr_end(p, pos);
    if (j0 >= Tend) return;                                  // (uniform over the workgroup: the grid is sized for the capacity)
    const TrRow me = tr_row(tp, kvh, tile * 16 + fi, pos);   // column i = fi of the S^T tile
    uint64_t* const strip = tp.idx + ((size_t)kvh * tp.n_tiles + tile) * (size_t)tp.njt * 64;
    const uint4* const kbase = (const uint4*)p.bkv->ck[0] + (size_t)kvh * NK * p.seq_len;
    {   // the tile's query rows as f32 (the per-row chains) and their masks
        const TrRow rq = tr_row(tp, kvh, tile * 16 + (tid >> 4), pos);
        const uint16_t* q = p.q + ((size_t)rq.col * p.H + rq.h) * HD + (tid & 15) * (HD / 16);
#pragma unroll
        for (int d = 0; d < HD / 16; d++) qs[(tid >> 4) * HD + (tid & 15) * (HD / 16) + d] = bf_wide(q[d]);
        if ((tid & 15) == 0) rMask[tid >> 4] = rq.mask;
    }
    // ---- positions below P16: the context's K on the matrix cores, four 16-position tiles per wave
    double zacc = 0.0;
    if (j0 + wave * 64 < P16) {
        const uint32_t sel = 0x0c0cu | ((uint32_t)(2 * fk) << 16) | ((uint32_t)(2 * fk + 1) << 24);      // element kk of a 4-element word pair (attn_mfma_kernel)
        float qf[2 * NK];                                    // Q[row fi][8 c + kk], Q[row fi][8 c + 4 + kk]
        const uint4* q = (const uint4*)(p.q + ((size_t)me.col * p.H + me.h) * HD);
#pragma unroll
        for (int c = 0; c < NK; c++) {
            const uint4 u = q[c];
            qf[2 * c] = __uint_as_float(__builtin_amdgcn_perm(u.y, u.x, sel));
            qf[2 * c + 1] = __uint_as_float(__builtin_amdgcn_perm(u.w, u.z, sel));
        }
        for (int t = 0; t < 4; t++) {
            const int jb = j0 + wave * 64 + t * 16;
            if (jb >= P16) break;                            // (uniform; P16 is a multiple of 16: a tile lies wholly on one side)
            uint4 k[NK];
            attn_load_k<NK>(k, kbase, p.seq_len, jb + 4 * (fi & 3) + (fi >> 2));       // operand row m = fi is position 4 (m & 3) + (m >> 2)
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
    // ---- positions from P16 on: one position per thread, the per-row chain; from pos on only what the row's mask lets through
    const int j = j0 + tid;
    if (j0 + ASP_NT > P16) {
        uint16_t* const strip16 = (uint16_t*)strip;
        for (int i = 0; i < 16; i++) {
            double ev = 0.0;
            if (j >= P16 && j < Tend && tr_sees(rMask[i], j, pos)) {
                uint4 k[NK];
                attn_load_k<NK>(k, kbase, p.seq_len, j);
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
    if (tid < 16) p.z_part[(((size_t)kvh * tp.n_tiles + tile) * 16 + tid) * ((p.seq_len + ASP_NT - 1) / ASP_NT) + blockIdx.x] = (zs[0][tid] + zs[1][tid]) + (zs[2][tid] + zs[3][tid]);
}

template <int HD> __global__ __launch_bounds__(64) void attn_tree_pv_kernel(AttnTreeParams tp) {
    const AttnParams& p = tp.a;
    const int lane = threadIdx.x, fi = lane & 15, fk = lane >> 4;
    const int tile = blockIdx.x, kvh = blockIdx.z;
    const int G = p.H / p.KVH, nrows = p.S * G;
    int pos = p.btab->st[0]->pos;
    pos = pos < 0 ? 0 : pos < p.seq_len ? pos : p.seq_len - 1;
    const int P16 = pos & ~15, Tend = tr_end(p, pos), nblk_max = (p.seq_len + ASP_NT - 1) / ASP_NT;
    const size_t vrow = (size_t)p.KVH * HD, voff = (size_t)kvh * HD + (size_t)blockIdx.y * 32 + 2 * fi;      // B operand column n = fi: output dims voff, voff + 1
    const uint16_t* const vsrc = p.bkv->cv[0] + voff;
    const uint64_t* const strip = tp.idx + ((size_t)kvh * tp.n_tiles + tile) * (size_t)tp.njt * 64;
    const uint16_t* const strip16 = (const uint16_t*)strip;
    // ---- Z estimate of row fi (the A operand's row): the per-block tree sums in block order; rows 4 fk + r (the accumulators') take theirs from lane 4 fk + r
    const TrRow ra = tr_row(tp, kvh, tile * 16 + fi, pos);
    double zt = 0.0;
    {
        const double* zp = p.z_part + (((size_t)kvh * tp.n_tiles + tile) * 16 + fi) * nblk_max;
        const int nblk = (Tend + ASP_NT - 1) / ASP_NT;
        for (int b = 0; b < nblk; b++) zt += zp[b];
    }
    const CertZ cza = cert_z(zt, ra.T);
    TrRow rd[4]; CertZ czd[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        rd[r] = tr_row(tp, kvh, tile * 16 + 4 * fk + r, pos);
        czd[r] = cert_z(__shfl(zt, 4 * fk + r), rd[r].T);
    }
    f32x4 acc0, acc1;
    int bad = 0;
    // one pass over all positions; exact: p = trunc(f32(e / Z)) with the walked serial sums (za: row fi's, zd: rows 4 fk + r), else cert_p (sets bad)
    auto run_pv = [&](bool exact, double za, const double (&zd)[4]) {
        acc0 = f32x4{0.f, 0.f, 0.f, 0.f}; acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
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
        for (int j = P16; j < Tend; j++) {                   // the last shared positions and the own slots: multiply, then add (D layout: rows 4 fk + r, column fi)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                if (!tr_sees(rd[r].mask, j, pos)) continue;  // a masked slot is skipped, never added as +0 * v
                const double e = p.exp_tab[strip16[sp_idx_elem(4 * fk + r, j)]];
                const float pj = exact ? alp_p(e, zd[r]) : cert_p(e, czd[r], bad);
                const uint32_t v = *(const uint32_t*)(vsrc + (size_t)j * vrow);
                acc0[r] = __fadd_rn(acc0[r], __fmul_rn(pj, bf_lo(v)));
                acc1[r] = __fadd_rn(acc1[r], __fmul_rn(pj, bf_hi(v)));
            }
        }
    };
    const double none[4] = {0.0, 0.0, 0.0, 0.0};
    if (!p.force_zseq) run_pv(false, 0.0, none);
    if (p.force_zseq || __builtin_amdgcn_ballot_w64(bad != 0) != 0) {
        // the reference's serial sum, j ascending, f64 (operations_impl.go:492-499): lane i < 16 walks row i; a masked slot adds +0 (its scratch word is never read as a score)
        double z = 0.0;
        if (lane < 16) {
            for (int jb = 0; jb < Tend; jb += 16) {
                uint64_t w[4]; double e[16];
#pragma unroll
                for (int kk = 0; kk < 4; kk++) w[kk] = strip[(size_t)(jb >> 4) * 64 + kk * 16 + lane];
#pragma unroll
                for (int u = 0; u < 16; u++) e[u] = p.exp_tab[(unsigned)(w[u & 3] >> (16 * (u >> 2))) & 0xFFFFu];
#pragma unroll
                for (int u = 0; u < 16; u++) z += (jb + u < Tend && tr_sees(ra.mask, jb + u, pos)) ? e[u] : 0.0;
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
        const int s = rd[r].col, k0 = rd[r].h * HD + (int)blockIdx.y * 32 + 2 * fi;
        if (p.out_xt) {                                      // the B-operand layout of the wo product (columns) or rows: al_store's two destinations
            uint16_t* o = p.out_xt + xt_group(s, p.H * HD);
            o[xt_index(s & 15, k0)] = bf_trunc(acc0[r]); o[xt_index(s & 15, k0 + 1)] = bf_trunc(acc1[r]);
        } else *(uint32_t*)(p.out + (size_t)s * p.H * HD + k0) = (uint32_t)bf_trunc(acc0[r]) | ((uint32_t)bf_trunc(acc1[r]) << 16);
    }
}

// ---- accept, emit, compact --------------------------------------------------------------------------------------------------------------------------
// g[i] = column i's token at ITS position (spec_argmax_kernel, or the sampler's draw u(seed, pos + depth[i])).  One thread; the emission of one token is
// spec_accept_emit's: token log, position, the context's token word, the stop ids freezing the run.
DEVINL void tree_accept_emit(const int32_t* g, int w, const BatchTab* tab, TreeCols* tree) {
    StepState* st = tab->st[0];
    tree->n_path = 0;
    if (st->finished) return;
    int i = 0, d = 0;
    for (;;) {
        tree->path[d++] = i;
        const int tok = g[i];
        const int n = st->n_out;
        if (n < tab->dout_cap[0]) tab->dout[0][n] = tok;
        st->n_out = n + 1;
        st->pos = st->pos + 1;
        *tab->dtok[0] = tok;
        bool stop = false;
        if (st->honour_stop) for (int k = 0; k < st->n_stop; k++) if (tok == st->stop[k]) stop = true;
        if (stop) { st->finished = 1; break; }
        int child = -1;
        for (int c = i + 1; c < w; c++) if (tree->parent[c] == i && *tab->dtok[c] == tok) child = c;
        if (child < 0) break;
        i = child;
    }
    tree->n_path = d;
}
__global__ void tree_commit_kernel(const int32_t* g, int w, const BatchTab* tab, TreeCols* tree) {
    if (threadIdx.x != 0) return;
    tree_accept_emit(g, w, tab, tree);
}
// spec_sample_commit_kernel with the tree walk behind the ticket: workgroup i samples column i's row at tab->st[i]->pos = pos + depth[i]
struct TreeSampleEnd { SpecSampleEnd e; TreeCols* tree; };
__global__ __launch_bounds__(1024) void tree_sample_commit_kernel(const uint16_t* logits, int V, const double* etab, const LnbSampler* smp, int32_t* g,
                                                                  const BatchTab* tab, unsigned* cnt, TreeCols* tree) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    __shared__ SampleSh sh;
    __shared__ TreeSampleEnd end;
    const int i = blockIdx.x;
    const LnbSampler s = smp[0];
    const uint16_t* x = logits + (size_t)i * V;
    const unsigned long long pos = (unsigned long long)(long long)tab->st[i]->pos;
    if (threadIdx.x == 0) { end.e.g = g; end.e.cnt = cnt; end.e.tab = tab; end.e.w = (int)gridDim.x; end.e.last = 0; end.tree = tree; }
    const int tok = s.temperature == 0.0f ? argmax_block(x, V, sv, si) : sample_block(x, V, etab, s, false, pos, sh);
    if (threadIdx.x != 0) return;
    end.e.g[i] = tok;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const unsigned t = __hip_atomic_fetch_add(end.e.cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (t != (unsigned)end.e.w - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    *end.e.cnt = 0;                                          // (ready for the next launch: stream order)
    tree_accept_emit(end.e.g, end.e.w, end.e.tab, end.tree);
}
// K rows live as [kv head][head_dim / 8][position][8], V rows as [position][kv_dim]: both are kv_dim / 8 pieces of 16 bytes per position
__global__ __launch_bounds__(256) void tree_kv_compact_kernel(TreeCompactParams cp) {
    const TreeCols* t = cp.tree;
    int np = t->n_path;
    np = np < 0 ? 0 : np > 16 ? 16 : np;
    bool moves = false;
    for (int d = 1; d < np; d++) moves |= t->path[d] != d;
    if (!moves) return;                                      // (uniform: the launch geometry is fixed, the path is the device's)
    const int piece = (int)blockIdx.x * 256 + (int)threadIdx.x, npieces = cp.kv_dim >> 3;
    if (piece >= npieces) return;
    const int pos = t->pos;
    const BatchKV& kv = cp.kv[blockIdx.z];
    uint4* base; size_t step;
    if (blockIdx.y == 0) { base = (uint4*)kv.ck[0] + (size_t)piece * cp.seq_len; step = 1; }
    else { base = (uint4*)kv.cv[0] + piece; step = (size_t)npieces; }
    for (int d = 1; d < np; d++) {
        const int i = t->path[d];
        if (i == d || i < d || pos + i >= cp.seq_len || pos < 0) continue;        // (i > d for a moved node; the rest keeps every index in bounds)
        base[(size_t)(pos + d) * step] = base[(size_t)(pos + i) * step];
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------------
extern "C" hipError_t lnbk_tree_draft(const TreeDraftParams* tp, hipStream_t st) {
    if (!tp) return hipErrorInvalidValue;
    const DraftParams* p = &tp->d;
    if (p->ngram_min < 1 || p->ngram_max < p->ngram_min || p->ngram_max > LNB_SPEC_MAX_NGRAM || p->max_draft < 0 || p->max_draft > LNB_SPEC_MAX_DRAFT) return hipErrorInvalidValue;
    if (tp->n_branches < 1 || tp->n_branches > LNB_TREE_MAX_BRANCHES || tp->max_nodes < 1 || tp->max_nodes > 16 || !tp->tbest || !p->out || !p->word || !p->cnt) return hipErrorInvalidValue;
    if ((tp->op_depth == nullptr) != (tp->op_parent == nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tree_draft_kernel, dim3((unsigned)(p->ngram_max - p->ngram_min + 1)), dim3(256), 0, st, *tp);
    return hipGetLastError();
}
// scores, then PV.  The grids cover the context's capacity and every row tile: a captured graph serves every position and every tree of its width.
extern "C" hipError_t lnbk_attn_tree(const AttnTreeParams* tp, hipStream_t st) {
    if (!tp) return hipErrorInvalidValue;
    const AttnParams* p = &tp->a;
    if (!p->btab || !p->bkv || !p->q || !p->exp_tab || !p->z_part || !tp->idx || !tp->tree || (!p->out && !p->out_xt)) return hipErrorInvalidValue;
    if (p->S < 1 || p->S > 16 || p->KVH < 1 || p->H % p->KVH || p->seq_len < 1 || p->seq_len > LNB_SEQ_MAX) return hipErrorInvalidValue;
    if (tp->n_tiles != lnb_shared_tiles(p->S, p->H / p->KVH) || tp->njt != (p->seq_len + 15) / 16) return hipErrorInvalidValue;
    return with_hd<64>(p, [&](auto HD) {
        form_ran(Form::ATTN_TREE_SCORES);
        hipLaunchKernelGGL(attn_tree_scores_kernel<HD>, dim3((p->seq_len + ASP_NT - 1) / ASP_NT, tp->n_tiles, p->KVH), dim3(ASP_NT), 0, st, *tp);
        form_ran(Form::ATTN_TREE_PV);
        hipLaunchKernelGGL(attn_tree_pv_kernel<HD>, dim3(tp->n_tiles, HD / 32, p->KVH), dim3(64), 0, st, *tp);
        return hipGetLastError();
    });
}
extern "C" hipError_t lnbk_tree_commit(const int32_t* g, int w, const BatchTab* tab, TreeCols* tree, hipStream_t st) {
    if (!g || !tab || !tree || w < 1 || w > 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tree_commit_kernel, dim3(1), dim3(64), 0, st, g, w, tab, tree);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_tree_sample_commit(const uint16_t* logits, int V, int w, const double* etab, const LnbSampler* smp, int32_t* g, const BatchTab* tab,
                                              unsigned* cnt, TreeCols* tree, hipStream_t st) {
    if (V < 1 || V > LNB_SAMPLE_MAX_V || w < 1 || w > 16 || !logits || !etab || !smp || !g || !tab || !cnt || !tree) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tree_sample_commit_kernel, dim3((unsigned)w), dim3(1024), 0, st, logits, V, etab, smp, g, tab, cnt, tree);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_tree_kv_compact(const TreeCompactParams* cp, hipStream_t st) {
    if (!cp || !cp->tree || !cp->kv || cp->n_layers < 1 || cp->n_layers > 65535 || cp->kv_dim < 8 || (cp->kv_dim & 7) || cp->seq_len < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tree_kv_compact_kernel, dim3((unsigned)(((cp->kv_dim >> 3) + 255) / 256), 2, (unsigned)cp->n_layers), dim3(256), 0, st, *cp);
    return hipGetLastError();
}
