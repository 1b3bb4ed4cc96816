// lnb_fast.hip -- the TOLERANCE ("fast") mode of the MI355X LlamaTransformer.Forward path: same operators, same bf16 truncation
// points as the reference (src/model/llamatransformer.go:215-254, :289-527, :593-660), but every matmul output is a SPLIT-K f32
// sum instead of the reference's single k-ordered chain (src/ml/operations_lineartransform.go:46-65), so these kernels are
// HBM-bound instead of add-latency-bound.  Results are NOT bit-identical to the reference (f32 addition is not associative and
// every bf16 truncation amplifies a last-bit difference to 2^-8 relative); the mode is opt-in (lnb_ctx_set_mode) and its
// distance from the oracle is MEASURED (tools/fast_mode_stats.py, NOTES.md section 6.2) -- the default stays the exact-order path.
//
// The weights are read IN PLACE from the layouts the exact-order kernels stream (lnb_device.h: tiled_index), one resident copy:
//   layout A  [N/RW][K/8][NCH][RW][8]   (wq|wk|wv, w1|w3, output; every matrix of the 70B-like shape)
//   layout B  [N/4][K/128][row%4][k%16][(k%128)/16]   (wo, w2 of the 8B shape: the row-broadcast layout)
// Decode (S < 16 rows): fast_gemv_a / fast_gemv_b, f32 FMAs on exact bf16 x bf16 products; RMSNorm, RoPE + KV append, SiLU*up and
// the residual add fused as in the exact kernels.  Prefill (S >= 16): fast_gemm_kernel on the bf16 matrix cores
// (v_mfma_f32_32x32x16_bf16, the 2.5 PFLOP/s pipe the exact path cannot use: it sums products before rounding).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "lnb_device.h"
#include "lnb_knobs.h"
#include "lnb_forms.h"

#define DEVINL __device__ __forceinline__

namespace {

DEVINL float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
DEVINL float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
DEVINL float bf_wide(uint16_t b) { return __uint_as_float(((uint32_t)b) << 16); }
DEVINL uint16_t bf_trunc(float f) { return (uint16_t)(__float_as_uint(f) >> 16); }   // bfloat16.go:31-33

DEVINL uint4 ld_stream(const void* p) {                     // weights are read once per token: keep them out of the way of x / KV in L2
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    u4v v = __builtin_nontemporal_load((const u4v*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
DEVINL float dot8(const uint4& w, const float4& xa, const float4& xb, float acc) {
    acc = fmaf(bf_lo(w.x), xa.x, acc); acc = fmaf(bf_hi(w.x), xa.y, acc);
    acc = fmaf(bf_lo(w.y), xa.z, acc); acc = fmaf(bf_hi(w.y), xa.w, acc);
    acc = fmaf(bf_lo(w.z), xb.x, acc); acc = fmaf(bf_hi(w.z), xb.y, acc);
    acc = fmaf(bf_lo(w.w), xb.z, acc); acc = fmaf(bf_hi(w.w), xb.w, acc);
    return acc;
}
DEVINL float dot8_bf(const uint4& w, const uint4& x, float acc) {
    acc = fmaf(bf_lo(w.x), bf_lo(x.x), acc); acc = fmaf(bf_hi(w.x), bf_hi(x.x), acc);
    acc = fmaf(bf_lo(w.y), bf_lo(x.y), acc); acc = fmaf(bf_hi(w.y), bf_hi(x.y), acc);
    acc = fmaf(bf_lo(w.z), bf_lo(x.z), acc); acc = fmaf(bf_hi(w.z), bf_hi(x.z), acc);
    acc = fmaf(bf_lo(w.w), bf_lo(x.w), acc); acc = fmaf(bf_hi(w.w), bf_hi(x.w), acc);
    return acc;
}
DEVINL float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- x staging: the activation row as f32 in the LDS, through the fused RMSNorm when NORM (llamatransformer.go:641-660 with a
// tree-ordered sum of squares instead of the serial one; the two truncations of :656 / :638 are kept) ---------------------------
template <bool NORM>
DEVINL void stage_x(const GemvParams& p, const uint16_t* xrow, float* xs, float* scratch, int tid) {
    const int nunits = p.K >> 3;
    float r = 1.0f;
    if (NORM) {
        float ss = 0.0f;
        for (int u = tid; u < nunits; u += 256) {
            const uint4 v = ((const uint4*)xrow)[u];
            const float a0 = bf_lo(v.x), a1 = bf_hi(v.x), a2 = bf_lo(v.y), a3 = bf_hi(v.y), a4 = bf_lo(v.z), a5 = bf_hi(v.z), a6 = bf_lo(v.w), a7 = bf_hi(v.w);
            ss += ((a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3)) + ((a4 * a4 + a5 * a5) + (a6 * a6 + a7 * a7));
        }
        ss = wave_sum(ss);
        if ((tid & 63) == 0) scratch[tid >> 6] = ss;
        __syncthreads();
        const float tot = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
        float mean = tot / (float)p.K;
        mean = mean + p.eps;
        r = (float)(1.0 / sqrt((double)mean));
    }
    for (int u = tid; u < nunits; u += 256) {
        const uint4 v = ((const uint4*)xrow)[u];
        float4 a = make_float4(bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y)), c = make_float4(bf_lo(v.z), bf_hi(v.z), bf_lo(v.w), bf_hi(v.w));
        if (NORM) {
            const uint4 g = ((const uint4*)p.norm_w)[u];
            a.x = bf_wide(bf_trunc(bf_wide(bf_trunc(a.x * r)) * bf_lo(g.x))); a.y = bf_wide(bf_trunc(bf_wide(bf_trunc(a.y * r)) * bf_hi(g.x)));
            a.z = bf_wide(bf_trunc(bf_wide(bf_trunc(a.z * r)) * bf_lo(g.y))); a.w = bf_wide(bf_trunc(bf_wide(bf_trunc(a.w * r)) * bf_hi(g.y)));
            c.x = bf_wide(bf_trunc(bf_wide(bf_trunc(c.x * r)) * bf_lo(g.z))); c.y = bf_wide(bf_trunc(bf_wide(bf_trunc(c.y * r)) * bf_hi(g.z)));
            c.z = bf_wide(bf_trunc(bf_wide(bf_trunc(c.z * r)) * bf_lo(g.w))); c.w = bf_wide(bf_trunc(bf_wide(bf_trunc(c.w * r)) * bf_hi(g.w)));
        }
        *(float4*)(xs + 8 * u) = a; *(float4*)(xs + 8 * u + 4) = c;
    }
    __syncthreads();
}

// ---- epilogues: the reference's rounding points (same code shape as gemv_epilogue in lnb_kernels.hip) --------------------------
template <int NCH, int EPI>
DEVINL void fast_epilogue(const GemvParams& p, const float (&acc)[NCH], int m, int n, bool valid) {
    if (EPI == EPI_STORE) {
        if (valid) p.out[(size_t)m * p.n_rows + n] = bf_trunc(acc[0]);
    } else if (EPI == EPI_RESID) {                          // ml.Add, operations_impl.go:320-332
        if (valid) { const size_t o = (size_t)m * p.n_rows + n; p.out[o] = bf_trunc(bf_wide(p.res[o]) + bf_wide(bf_trunc(acc[0]))); }
    } else if (EPI == EPI_SILU_MUL) {                       // activations.go:36-39, llamatransformer.go:614
        if (valid) {
            const uint16_t g = bf_trunc(acc[0]), u = bf_trunc(acc[NCH - 1]);
            const uint16_t gs = bf_trunc(p.silu[g]);
            p.out[(size_t)m * p.n_rows + n] = bf_trunc(bf_wide(gs) * bf_wide(u));
        }
    } else if (EPI == EPI_QKV_ROPE) {                       // llamatransformer.go:297-403, :753-790
        const int pos = p.st->pos + m;
        const uint16_t mine = bf_trunc(acc[0]);
        const uint16_t other = (uint16_t)__shfl_xor((int)mine, 1);
        if (valid) {
            if (n < p.q_dim + p.kv_dim) {
                const int d = n % p.head_dim, i = d >> 1;
                const float2 cs = *(const float2*)(p.cis + ((size_t)pos * (p.head_dim >> 1) + i) * 2);
                const double cr = (double)cs.x, ci = (double)cs.y;
                uint16_t r16;
                if ((n & 1) == 0) { const double a = (double)bf_wide(mine), bb = (double)bf_wide(other); r16 = bf_trunc((float)(a * cr - bb * ci)); }
                else              { const double a = (double)bf_wide(other), bb = (double)bf_wide(mine); r16 = bf_trunc((float)(a * ci + bb * cr)); }
                if (n < p.q_dim) p.q_out[(size_t)m * p.q_dim + n] = r16;
                else {
                    const int kc = n - p.q_dim, kh = kc / p.head_dim;
                    p.cache_k[(((size_t)kh * (p.head_dim >> 3) + (d >> 3)) * p.seq_len + pos) * 8 + (d & 7)] = r16;
                }
            } else p.cache_v[(size_t)pos * p.kv_dim + (n - p.q_dim - p.kv_dim)] = mine;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// fast_gemv_a: split-K GEMV over layout A.  A work unit is RG rows of one RW-row block; lane = (row r = lane % RG, k phase
// ph = lane / RG): one 16 B load per lane = 8 weights of its row, the wave covers 64 / RG consecutive 8-wide k chunks per
// instruction, the four waves of the workgroup consecutive runs of chunks (split-K four ways in the workgroup, 64 / RG ways in
// the wave).  UNR loads per lane are in flight before the first is consumed; several workgroups are resident per CU.
// Partial sums: xor-shuffles over the phases, LDS over the waves, fixed order (deterministic run to run).
// grid (min(units, cap), S), block 256, dynamic LDS = K * 4 + 256 bytes.
// ------------------------------------------------------------------------------------------------
constexpr int FA_UNR = 8;
template <int NCH, int EPI, bool NORM, int RG>
__global__ __launch_bounds__(256) void fast_gemv_a(GemvParams p, int RW) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xs = (float*)smem;
    float* red = xs + p.K;                                   // [4 waves][NCH][RG] (<= 4 * 2 * 64 floats)
    constexpr int PH = 64 / RG, CPI = 4 * PH;                // chunks per workgroup per load round
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = blockIdx.y, K = p.K, nunits = K >> 3;
    const int groups = RW / RG, n_units = p.n_blocks * groups;
    const size_t chunk_stride = (size_t)NCH * RW * 16, block_bytes = (size_t)nunits * chunk_stride;
    const int r = lane & (RG - 1), ph = lane / RG;
    // the first round of weight loads of the first unit does not depend on x: in flight while x is staged (and normalised)
    uint4 wv[FA_UNR][NCH];
    auto issue = [&](const char* base, int kb) {
        const int kc0 = kb + wave * PH + ph;
#pragma unroll
        for (int j = 0; j < FA_UNR; j++) {
            const int kc = kc0 + j * CPI;
            const char* a = base + (size_t)(kc < nunits ? kc : nunits - 1) * chunk_stride;
#pragma unroll
            for (int c = 0; c < NCH; c++) wv[j][c] = ld_stream(a + (size_t)c * RW * 16);
        }
    };
    auto base_of = [&](int u) { const int b = u / groups, g = u - b * groups; return (const char*)p.w + (size_t)b * block_bytes + (size_t)(g * RG + r) * 16; };
    if ((int)blockIdx.x < n_units) issue(base_of(blockIdx.x), 0);
    stage_x<NORM>(p, p.x + (size_t)m * K, xs, red, tid);
    for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
        const int b = u / groups, g = u - b * groups;
        const char* base = base_of(u);
        float acc[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) acc[c] = 0.0f;
        for (int kb = 0; kb < nunits; kb += CPI * FA_UNR) {     // (uniform trip count)
            const int kc0 = kb + wave * PH + ph;
            if (kb != 0 || u != (int)blockIdx.x) issue(base, kb);
#pragma unroll
            for (int j = 0; j < FA_UNR; j++) {
                const int kc = kc0 + j * CPI;
                if (kc < nunits) {
                    const float4 xa = *(const float4*)(xs + 8 * kc), xb = *(const float4*)(xs + 8 * kc + 4);
#pragma unroll
                    for (int c = 0; c < NCH; c++) acc[c] = dot8(wv[j][c], xa, xb, acc[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NCH; c++) {
#pragma unroll
            for (int o = RG; o < 64; o <<= 1) acc[c] += __shfl_xor(acc[c], o);
            if (lane < RG) red[(wave * NCH + c) * RG + lane] = acc[c];
        }
        __syncthreads();
        if (wave == 0) {
            float tot[NCH];
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int li = lane & (RG - 1);
                tot[c] = (red[(0 * NCH + c) * RG + li] + red[(1 * NCH + c) * RG + li]) + (red[(2 * NCH + c) * RG + li] + red[(3 * NCH + c) * RG + li]);
            }
            const int n = b * RW + g * RG + lane;
            fast_epilogue<NCH, EPI>(p, tot, m, n, lane < RG && n < p.n_rows);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// fast_gemv_b: split-K GEMV over layout B (the row-broadcast layout of wo / w2).  A wave tile is 4 rows; one 1 KiB chunk = 128
// k-steps of the 4 rows: lane (q = lane / 16, j = lane % 16) holds the eight weights of row q with k = 128c + 16e + j.  x sits in
// the LDS as bf16 TRANSPOSED per chunk ([c][j][e]) so the lane's eight operands are one 16 B read.  The workgroup's four waves
// split the chunks of one tile four ways.  grid (tiles, S), block 256, dynamic LDS = K * 2 + 64 bytes.
// ------------------------------------------------------------------------------------------------
constexpr int FB_UNR = 8;
template <int EPI>
__global__ __launch_bounds__(256) void fast_gemv_b(GemvParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t* xT = (uint16_t*)smem;                          // x[128c + 16e + j] at xT[(c*16 + j)*8 + e]
    float* red = (float*)(smem + (size_t)p.K * 2);           // [4 waves][4 rows]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = blockIdx.y, K = p.K, nchunks = K >> 7;
    const int tile = blockIdx.x;
    const char* base = (const char*)p.w + (size_t)tile * nchunks * 1024 + (size_t)lane * 16;
    // the first round of weight loads does not depend on x: in flight while x is staged
    uint4 wv[FB_UNR];
#pragma unroll
    for (int j = 0; j < FB_UNR; j++) { const int c = wave + 4 * j; wv[j] = ld_stream(base + (size_t)(c < nchunks ? c : nchunks - 1) * 1024); }
    const uint16_t* xrow = p.x + (size_t)m * K;
    for (int u = tid; u < (K >> 3); u += 256) {
        const uint4 v = ((const uint4*)xrow)[u];
        const int k = u * 8, c = k >> 7, e = (k & 127) >> 4, j0 = k & 15;
        uint16_t* d = xT + ((size_t)(c * 16 + j0) * 8 + e);
        d[0] = (uint16_t)v.x; d[8] = (uint16_t)(v.x >> 16); d[16] = (uint16_t)v.y; d[24] = (uint16_t)(v.y >> 16);
        d[32] = (uint16_t)v.z; d[40] = (uint16_t)(v.z >> 16); d[48] = (uint16_t)v.w; d[56] = (uint16_t)(v.w >> 16);
    }
    __syncthreads();
    const uint16_t* xl = xT + (size_t)(lane & 15) * 8;
    float acc = 0.0f;
    for (int c0 = wave; c0 < nchunks; c0 += 4 * FB_UNR) {
        if (c0 != wave) {
#pragma unroll
            for (int j = 0; j < FB_UNR; j++) { const int c = c0 + 4 * j; wv[j] = ld_stream(base + (size_t)(c < nchunks ? c : nchunks - 1) * 1024); }
        }
#pragma unroll
        for (int j = 0; j < FB_UNR; j++) {
            const int c = c0 + 4 * j;
            if (c < nchunks) acc = dot8_bf(wv[j], *(const uint4*)(xl + (size_t)c * 128), acc);
        }
    }
    acc += __shfl_xor(acc, 1); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 4); acc += __shfl_xor(acc, 8);
    if ((lane & 15) == 0) red[wave * 4 + (lane >> 4)] = acc;
    __syncthreads();
    if (tid < 4) {
        const float tot = (red[tid] + red[4 + tid]) + (red[8 + tid] + red[12 + tid]);
        const int n = tile * 4 + tid;
        if (n < p.n_rows) {
            const size_t o = (size_t)m * p.n_rows + n;
            if (EPI == EPI_RESID) p.out[o] = bf_trunc(bf_wide(p.res[o]) + bf_wide(bf_trunc(tot)));      // ml.Add, operations_impl.go:320-332
            else p.out[o] = bf_trunc(tot);
        }
    }
}


// ------------------------------------------------------------------------------------------------
// fast_gemm_kernel: the prefill GEMM of the tolerance mode on the bf16 matrix cores, Y[m][n] = sum_k X[m][k] W[n][k], f32 accumulate.
//
// v_mfma_f32_32x32x16_bf16: A lane (row = lane & 31, kg = lane >> 5) supplies 8 bf16 of its row, k = 8 kg .. 8 kg + 7 of the
// 16-step; B likewise per column; D[row][col]: lane holds col = lane & 31, rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
// A = the WEIGHTS, straight from HBM/L2 into the operand registers: a 16 B unit of either resident layout IS 8 k-values of one
// weight row (layout A: consecutive k; layout B: k = 128c + 16e + j, e = 0..7 -- the k order inside an instruction does not matter
// for a sum, the X tile is staged in the matching order), a 32-row tile of layout A is one 512 B run per k-group, and every weight
// unit is consumed by exactly one wave, so an LDS stage would buy nothing.  B = X, staged through the LDS (shared by the four
// waves): 128 batch rows x 64 k per slab, row pitch 144 B (conflict-free ds_read_b128), double-buffered, one barrier per slab.
// Wave w owns 64 output rows (two 32-row tiles; one 32-row tile of BOTH chains for the gate|up matrix) x 128 batch rows:
// 8 MFMAs per 16-step on 2 weight loads + 4 LDS reads.  The next slab's weights and X rows are in flight during a slab's 32 MFMAs.
// Epilogues = the reference's rounding points, four consecutive output rows per lane (RoPE partner in the same lane).
// grid (ceil(N / 256 or 128), ceil(S / 128)), block 256, static LDS 36 KB: two workgroups per CU.
// ------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int FG_BK = 64, FG_PITCH = 144;

template <int EPI> DEVINL void fast_gemm_epilogue4(const GemmParams& p, const f32x4& g, const f32x4& u, int m, int n0) {
    if (m >= p.S) return;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int n = n0 + r;
        if (n >= p.n_rows) continue;
        const size_t o = (size_t)m * p.n_rows + n;
        if (EPI == EPI_STORE) p.out[o] = bf_trunc(g[r]);
        else if (EPI == EPI_RESID) p.out[o] = bf_trunc(bf_wide(p.res[o]) + bf_wide(bf_trunc(g[r])));
        else if (EPI == EPI_SILU_MUL) {
            const uint16_t gs = bf_trunc(p.silu[bf_trunc(g[r])]);
            p.out[o] = bf_trunc(bf_wide(gs) * bf_wide(bf_trunc(u[r])));
        } else if (EPI == EPI_QKV_ROPE) {
            const int pos = p.st->pos + m;
            const uint16_t mine = bf_trunc(g[r]), other = bf_trunc(g[r ^ 1]);
            if (n < p.q_dim + p.kv_dim) {
                const int d = n % p.head_dim, i = d >> 1;
                const float2 cs = *(const float2*)(p.cis + ((size_t)pos * (p.head_dim >> 1) + i) * 2);
                const double cr = (double)cs.x, ci = (double)cs.y;
                uint16_t r16;
                if ((n & 1) == 0) { const double a = (double)bf_wide(mine), bb = (double)bf_wide(other); r16 = bf_trunc((float)(a * cr - bb * ci)); }
                else              { const double a = (double)bf_wide(other), bb = (double)bf_wide(mine); r16 = bf_trunc((float)(a * ci + bb * cr)); }
                if (n < p.q_dim) p.q_out[(size_t)m * p.q_dim + n] = r16;
                else {
                    const int kc = n - p.q_dim, kh = kc / p.head_dim;
                    p.cache_k[(((size_t)kh * (p.head_dim >> 3) + (d >> 3)) * p.seq_len + pos) * 8 + (d & 7)] = r16;
                }
            } else p.cache_v[(size_t)pos * p.kv_dim + (n - p.q_dim - p.kv_dim)] = mine;
        }
    }
}

// (The RoPE epilogue is long -- f64 complex product -- and hipcc refuses to unroll the 64-iteration epilogue loop around it: the
// accumulator tiles of that instantiation are indexed through 576 B of scratch, once per output tile.  An out-of-line epilogue call
// keeps them in registers but saves and restores them around each of the 64 calls: measured 609 against 469 us for the 4096-row
// wq|wk|wv GEMM.  The refused unroll is therefore accepted, and its -Wpass-failed remark silenced.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
// WB = weight register sets: 3 (two slabs of prefetch distance, one workgroup per CU, accumulators for 256 batch rows) or 2 (one slab, two
// workgroups per CU within 256 registers per wave: a second wave per SIMD issues MFMAs while the first is parked on a wait)
template <int EPI, int NCH, bool LAYB, int MT, int WB>
__global__ __launch_bounds__(256, WB == 2 ? 2 : 1) void fast_gemm_kernel(GemmParams p) {
    constexpr int AT = NCH == 2 ? 1 : 2;                     // 32-row weight tiles per wave and chain
    constexpr int NWG = 4 * 32 * AT;                         // output rows per workgroup
    constexpr int MB = 32 * MT, XQ = MB / 32;                // batch rows per workgroup; X units per thread and slab
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    char* const lds0 = lds_raw; char* const lds1 = lds_raw + (size_t)MB * FG_PITCH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane & 31, kg = lane >> 5;
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so the workgroups that stream the SAME
    // weight rows (one per batch tile) are given linear ids 8 apart: they run at the same time on ONE XCD and share the rows in its L2
    // (measured neutral at S = 4096 on the 8B shape -- 93.7 against 95.5 ms per Forward: the weight stream is not the limiter there)
    const int gx = (p.S + MB - 1) / MB, ny = (p.n_rows + NWG - 1) / NWG;
    const int lin = blockIdx.x, chunk = lin / (8 * gx), within = lin - chunk * (8 * gx);
    const int by = chunk * 8 + (within & 7), bx = within >> 3;
    if (by >= ny) return;                                    // (uniform: padding of the last group of 8 weight tiles)
    const int n0 = by * NWG + wave * 32 * AT, m0 = bx * MB;
    const int K = p.K, nslabs = K / FG_BK;
    // ---- weight stream: per-lane byte offset of k-step 0 of slab 0 from the wave-uniform base; uniform strides per k-step and slab
    // (32-bit offsets: a matrix is < 4 GB, and offsets cost half the registers of pointers)
    uint32_t wp[NCH][AT];
    const char* const wbase = (const char*)p.w;
    uint32_t w_step, w_slab0, w_slab1;                       // slab s -> s+1 advances by w_slab0 (s even) / w_slab1 (s odd)
    if (LAYB) { w_step = 32; w_slab0 = 128; w_slab1 = 1024 - 128; }
    else { w_step = (uint32_t)(2 * p.nch * p.rw * 16); w_slab0 = w_slab1 = (uint32_t)(8 * p.nch * p.rw * 16); }
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int a = 0; a < AT; a++) {
            int n = n0 + 32 * a + ln; n = n < p.n_rows ? n : p.n_rows - 1;         // clamped rows are computed and dropped
            if (LAYB) wp[c][a] = (uint32_t)((((size_t)(n >> 2) * (size_t)(K >> 7) * 64 + (size_t)((n & 3) * 16 + kg)) * 16));
            else wp[c][a] = (uint32_t)((((((size_t)(n / p.rw) * (size_t)(K >> 3) + (size_t)kg) * p.nch + c) * p.rw + (size_t)(n % p.rw)) * 16));
        }
    // ---- X staging: thread = (row = tid / 8 + 32 q, unit = tid % 8) of the MB x 64 slab
    const int xr_row = tid >> 3, xr_u = tid & 7;
    uint32_t xp[XQ];                                         // element offsets of this thread's rows (S * K < 2^31)
#pragma unroll
    for (int q = 0; q < XQ; q++) { int m = m0 + xr_row + 32 * q; m = m < p.S ? m : p.S - 1; xp[q] = (uint32_t)m * (uint32_t)K; }
    uint4 xr[XQ];
    auto x_issue = [&](int s) {                              // layout A: 8 consecutive k; layout B: the unit whose k % 16 lies in this slab's half
        const int off = LAYB ? ((s >> 1) * 128 + (2 * xr_u + (s & 1)) * 8) : (s * FG_BK + xr_u * 8);
#pragma unroll
        for (int q = 0; q < XQ; q++) xr[q] = *(const uint4*)(p.x + (size_t)(xp[q] + (uint32_t)off));
    };
    auto x_commit = [&](char* buf) {
#pragma unroll
        for (int q = 0; q < XQ; q++) {
            char* row = buf + (size_t)(xr_row + 32 * q) * FG_PITCH;
            if (LAYB) {                                      // element i of the loaded unit = k % 16 = 8 h + i -> LDS unit i, slot e = xr_u
                const uint32_t wd[4] = {xr[q].x, xr[q].y, xr[q].z, xr[q].w};
#pragma unroll
                for (int i = 0; i < 8; i++) *(uint16_t*)(row + i * 16 + xr_u * 2) = (uint16_t)(wd[i >> 1] >> ((i & 1) * 16));
            } else *(uint4*)(row + xr_u * 16) = make_uint4(xr[q].x, xr[q].y, xr[q].z, xr[q].w);   // (component reads: a whole-struct copy keeps xr on the stack)
        }
    };
    typedef uint4 wbuf_t[4][NCH][AT];
    wbuf_t w0, w1, w2;                                       // weights of WB consecutive slabs (w2 unused when WB == 2)
    int s_w = 0;                                             // slab the pointers stand on
    auto w_issue = [&](wbuf_t& w) {                          // loads the slab the pointers stand on, then steps them to the next
#pragma unroll
        for (int ks = 0; ks < 4; ks++)
#pragma unroll
            for (int c = 0; c < NCH; c++)
#pragma unroll
                for (int a = 0; a < AT; a++) w[ks][c][a] = *(const uint4*)(wbase + (size_t)(wp[c][a] + (uint32_t)ks * w_step));
        const uint32_t d = (s_w & 1) ? w_slab1 : w_slab0;
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int a = 0; a < AT; a++) wp[c][a] += d;
        s_w++;
    };
    f32x16 acc[NCH][AT][MT];
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int a = 0; a < AT; a++)
#pragma unroll
            for (int t = 0; t < MT; t++)
#pragma unroll
                for (int i = 0; i < 16; i++) acc[c][a][t][i] = 0.0f;
    // slab s: X of slab s+1 and the weights of slab s+2 go in flight (X first: its wait must not drain the younger weight loads),
    // 32 MT MFMAs on slab s, then X(s+1) is written to the other LDS buffer; one barrier
    auto slab = [&](int s, const wbuf_t& wa, wbuf_t& wc) {
        const bool more = s + 1 < nslabs;                    // (uniform)
        if (more) x_issue(s + 1);
        if (s + WB - 1 < nslabs) w_issue(wc);
        const char* bl = ((s & 1) ? lds1 : lds0) + (size_t)ln * FG_PITCH + kg * 16;
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            bf16x8 bfr[MT];
#pragma unroll
            for (int t = 0; t < MT; t++) bfr[t] = *(const bf16x8*)(bl + (size_t)t * 32 * FG_PITCH + ks * 32);
#pragma unroll
            for (int c = 0; c < NCH; c++)
#pragma unroll
                for (int a = 0; a < AT; a++) {
                    const bf16x8 af = __builtin_bit_cast(bf16x8, wa[ks][c][a]);
#pragma unroll
                    for (int t = 0; t < MT; t++) acc[c][a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[t], acc[c][a][t], 0, 0, 0);
                }
        }
        if (more) x_commit((s & 1) ? lds0 : lds1);
        __syncthreads();
    };
    x_issue(0); w_issue(w0); if (WB == 3 && nslabs > 1) w_issue(w1);
    x_commit(lds0);
    __syncthreads();
    if constexpr (WB == 3) {
        for (int s = 0; s < nslabs; s += 3) {
            slab(s, w0, w2);
            if (s + 1 < nslabs) slab(s + 1, w1, w0);
            if (s + 2 < nslabs) slab(s + 2, w2, w1);
        }
    } else {
        for (int s = 0; s < nslabs; s += 2) {
            slab(s, w0, w1);
            if (s + 1 < nslabs) slab(s + 1, w1, w0);
        }
    }
    // D: lane holds batch column m0 + 32 t + ln, output rows 8 g + 4 kg + r (g = 0..3, r = 0..3) of each 32-row tile
#pragma unroll
    for (int a = 0; a < AT; a++)
#pragma unroll
        for (int t = 0; t < MT; t++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f32x16& A0 = acc[0][a][t]; const f32x16& A1 = acc[NCH - 1][a][t];
                const f32x4 gv = {A0[4 * g], A0[4 * g + 1], A0[4 * g + 2], A0[4 * g + 3]};
                const f32x4 uv = {A1[4 * g], A1[4 * g + 1], A1[4 * g + 2], A1[4 * g + 3]};
                fast_gemm_epilogue4<EPI>(p, gv, uv, m0 + 32 * t + ln, n0 + 32 * a + 8 * g + 4 * kg);
            }
}
#pragma clang diagnostic pop

template <int EPI, int NCH, bool LAYB, int MT, int WB = 3> hipError_t launch_gemm_fast_t(const GemmParams* p, hipStream_t st) {
    auto kfn = fast_gemm_kernel<EPI, NCH, LAYB, MT, WB>;
    const size_t lds = 2 * (size_t)32 * MT * FG_PITCH;
    if (!p) return hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const int nwg = NCH == 2 ? 128 : 256;
    const unsigned gx = (unsigned)((p->S + 32 * MT - 1) / (32 * MT)), ny = (unsigned)((p->n_rows + nwg - 1) / nwg);
    const dim3 grid(((ny + 7) / 8) * 8 * gx);                // (padded to whole groups of 8 weight tiles: see the tile order in the kernel)
    form_ran(MT == 8 ? (LAYB ? Form::FAST_GEMM_B_MT8_WB3 : Form::FAST_GEMM_A_MT8_WB3) : WB == 3 ? (LAYB ? Form::FAST_GEMM_B_MT4_WB3 : Form::FAST_GEMM_A_MT4_WB3)
                     : (LAYB ? Form::FAST_GEMM_B_MT4_WB2 : Form::FAST_GEMM_A_MT4_WB2), EPI);
    hipLaunchKernelGGL(kfn, grid, dim3(256), lds, st, *p);
    return hipGetLastError();
}
template <int EPI, int NCH> hipError_t launch_gemm_fast(const GemmParams* p, int layb, hipStream_t st) {
    if (!p) {                                                // raise the dynamic-LDS limits (72 KB for the 256-row batch tile)
        hipError_t e = launch_gemm_fast_t<EPI, NCH, false, 4>(nullptr, nullptr);
        if (e == hipSuccess) e = launch_gemm_fast_t<EPI, NCH, false, 8>(nullptr, nullptr);
        if (NCH == 1 && e == hipSuccess) e = launch_gemm_fast_t<EPI, NCH, true, 4>(nullptr, nullptr);
        if (NCH == 1 && e == hipSuccess) e = launch_gemm_fast_t<EPI, NCH, true, 8>(nullptr, nullptr);
        if (e == hipSuccess) e = launch_gemm_fast_t<EPI, NCH, false, 4, 2>(nullptr, nullptr);
        if (NCH == 1 && e == hipSuccess) e = launch_gemm_fast_t<EPI, NCH, true, 4, 2>(nullptr, nullptr);
        return e;
    }
    // 128-row batch tiles with two workgroups per CU win while there are few tiles (512 rows: 35.6 against 42.5 ms per Forward of the 8B
    // shape), 256-row tiles with one workgroup per CU from ~1000 rows up (2048: 61.8 against 67.5 ms; 4096: 94.8 against 128.7)
    const int two = knob(Knob::FAST_GEMM_2WG);                // -1: by row count
    if (two == 1 || (two < 0 && p->S < 1024)) {              // 128 batch rows, two workgroups per CU
        if constexpr (NCH == 1) if (layb) return launch_gemm_fast_t<EPI, NCH, true, 4, 2>(p, st);
        return launch_gemm_fast_t<EPI, NCH, false, 4, 2>(p, st);
    }
    const bool big = p->S > 128;                             // 256 batch rows per workgroup: twice the MFMAs per weight byte and per slab
    if constexpr (NCH == 1) if (layb) return big ? launch_gemm_fast_t<EPI, NCH, true, 8>(p, st) : launch_gemm_fast_t<EPI, NCH, true, 4>(p, st);
    return big ? launch_gemm_fast_t<EPI, NCH, false, 8>(p, st) : launch_gemm_fast_t<EPI, NCH, false, 4>(p, st);
}

// ------------------------------------------------------------------------------------------------
// fast_attn_prefill_kernel: the prefill attention of the tolerance mode (S >= 16 query rows) on the bf16 matrix cores, flash form:
// one pass over the cached positions in tiles of 32 with an online softmax (running maximum and sum per query row, f32), instead of
// the reference's f64 softmax without maximum subtraction over materialised scores (llamatransformer.go:456-514).
//   S^T tile [32 j][32 q] = K Q^T: A = K rows straight from the position-contiguous cache (a 16 B unit = 8 dims of one position: the MFMA
//       operand as it lies in HBM), B = Q rows held in registers; D: lane = query row q (lane & 31), 16 positions per lane
//       (j = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) -- everything per query row (mask, maximum, sum, rescale) is lane-local plus ONE
//       exchange with lane ^ 32;
//   O^T [d][q] += V^T P^T: B = the lane's own 16 probabilities packed to bf16 (its k-slots are its own positions: no transpose), A = V^T from
//       the LDS, where the workgroup stages the tile TRANSPOSED ([d][j], the positions of a 16-group permuted into the order the lanes
//       hold them, pitch 80 B: conflict-free 16 B reads); D: lane = query row again, so the softmax rescale of O is lane-local too.
// A wave owns 32 query rows of one head, a workgroup 128 (the V tile is shared); causal tiles only; heavy workgroups first.
// The mask is the reference's modulo-broadcast triu (tensoriterators.go:47-55): (j mod S) > i is masked.
// grid (H, ceil(S / 128)), block 256, static LDS 20 KB (hd 128).
// ------------------------------------------------------------------------------------------------
constexpr int FA_VP = 80;                                    // bytes per d row of the staged V tile (32 positions x 2 B + pad)
template <int HD> __global__ __launch_bounds__(256, 2) void fast_attn_prefill_kernel(AttnParams p) {
    constexpr int NKS = HD / 16, DT = HD / 32, VU = 32 * (HD / 8) / 256;     // QK k-steps, 32-dim output tiles, V units per thread
    static_assert(VU >= 1, "head_dim >= 64");
    __shared__ __attribute__((aligned(16))) char vl[2][HD * FA_VP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane & 31, kg = lane >> 5;
    // XCD-aware (like xcd_head_block of lnb_kernels.hip): XCD x runs heads x*H/8 .. -- the heads of a GQA group read their K / V tiles
    // through one L2 --, and inside the XCD the longest query blocks of all its heads come first
    const unsigned H_ = gridDim.x, nb_ = gridDim.y, lin_ = blockIdx.y * H_ + blockIdx.x;
    int h = (int)blockIdx.x, qb = (int)nb_ - 1 - (int)blockIdx.y;
    if ((H_ & 7u) == 0) { const unsigned hg_ = H_ >> 3, w_ = lin_ >> 3; h = (int)((lin_ & 7u) * hg_ + w_ % hg_); qb = (int)nb_ - 1 - (int)(w_ / hg_); }
    const int S = p.S, H = p.H, KVH = p.KVH;
    const int pos0 = p.st->pos, T = pos0 + S;
    const int kvh = h / (H / KVH);
    const int q0 = qb * 128 + wave * 32, i = q0 + ln;         // this lane's query row
    const float scale = 1.4426950408889634f / p.divisor;      // scores in log2 units: exp(x) = exp2(x * log2 e)
    // ---- Q operand: 8 consecutive dims of row i per k-step
    bf16x8 qf[NKS];
    {
        const uint16_t* qr = p.q + ((size_t)(i < S ? i : S - 1) * H + h) * HD + 8 * kg;
#pragma unroll
        for (int s2 = 0; s2 < NKS; s2++) qf[s2] = __builtin_bit_cast(bf16x8, *(const uint4*)(qr + 16 * s2));
    }
    const int qmax = (qb * 128 + 127 < S ? qb * 128 + 127 : S - 1);
    const int jlast = (pos0 == 0) ? qmax : T - 1;            // last position any row of this workgroup can see
    const int ntiles = jlast / 32 + 1;
    const uint4* kbase = (const uint4*)p.cache_k + (size_t)kvh * (HD / 8) * p.seq_len;
    const uint16_t* vbase = p.cache_v + (size_t)kvh * HD;
    const size_t vrow = (size_t)KVH * HD;
    auto load_k = [&](uint4 (&k)[NKS], int jt) {
        int j = jt * 32 + ln; j = j < T ? j : T - 1;
#pragma unroll
        for (int s2 = 0; s2 < NKS; s2++) k[s2] = kbase[(size_t)(2 * s2 + kg) * p.seq_len + j];
    };
    uint4 vr[VU];
    auto load_v = [&](int jt) {
#pragma unroll
        for (int u = 0; u < VU; u++) {
            const int un = tid + 256 * u, jr = un / (HD / 8), dc = un % (HD / 8);
            int j = jt * 32 + jr; j = j < T ? j : T - 1;
            vr[u] = *(const uint4*)(vbase + (size_t)j * vrow + 8 * dc);
        }
    };
    auto store_v = [&](int buf) {                            // transposed, positions permuted into the lanes' order
#pragma unroll
        for (int u = 0; u < VU; u++) {
            const int un = tid + 256 * u, jr = un / (HD / 8), dc = un % (HD / 8);
            const int w = jr & 15, pj = (jr & 16) + 8 * ((w >> 2) & 1) + (w & 3) + 4 * (w >> 3);
            char* d = vl[buf] + (size_t)(8 * dc) * FA_VP + pj * 2;
            const uint32_t wd[4] = {vr[u].x, vr[u].y, vr[u].z, vr[u].w};
#pragma unroll
            for (int e = 0; e < 8; e++) *(uint16_t*)(d + e * FA_VP) = (uint16_t)(wd[e >> 1] >> ((e & 1) * 16));
        }
    };
    f32x16 o[DT];
#pragma unroll
    for (int t = 0; t < DT; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[t][r] = 0.0f;
    float m = -INFINITY, l = 0.0f;
    uint4 kt[NKS];
    load_v(0); store_v(0); load_k(kt, 0);
    for (int jt = 0; jt < ntiles; jt++) {
        __syncthreads();                                     // V(jt) is staged; everybody is done with the buffer V(jt+1) goes to
        const bool more = jt + 1 < ntiles;
        if (more) load_v(jt + 1);
        f32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; r++) sc[r] = 0.0f;
#pragma unroll
        for (int s2 = 0; s2 < NKS; s2++) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kt[s2]), qf[s2], sc, 0, 0, 0);
        if (more) load_k(kt, jt + 1);
        // ---- online softmax of this lane's 16 positions of row i
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int j = jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
            const bool dead = j >= T || i >= S || ((pos0 == 0 ? j : j % S) > i);
            sc[r] = dead ? -INFINITY : sc[r] * scale;
            mx = fmaxf(mx, sc[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);
        const float msafe = mn == -INFINITY ? 0.0f : mn;      // a row with nothing visible yet: every p is exp2(-inf) = 0
        const float alpha = __builtin_amdgcn_exp2f(m - msafe);   // m == -inf -> 0
        float rs = 0.0f;
        uint32_t pk[8];
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const float p0 = __builtin_amdgcn_exp2f(sc[r] - msafe), p1 = __builtin_amdgcn_exp2f(sc[r + 1] - msafe);
            rs += p0 + p1;
            pk[r >> 1] = __builtin_amdgcn_perm(__float_as_uint(p1), __float_as_uint(p0), 0x07060302u);   // two truncated bf16
        }
        rs += __shfl_xor(rs, 32);
        l = l * alpha + rs; m = mn;
#pragma unroll
        for (int t = 0; t < DT; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[t][r] *= alpha;
        // ---- O^T += V^T P^T: two 16-position k-steps
        const char* vb = vl[jt & 1] + (size_t)ln * FA_VP + kg * 16;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            const uint4 pu = make_uint4(pk[4 * ks], pk[4 * ks + 1], pk[4 * ks + 2], pk[4 * ks + 3]);
            const bf16x8 pf = __builtin_bit_cast(bf16x8, pu);
#pragma unroll
            for (int t = 0; t < DT; t++) {
                const bf16x8 vf = *(const bf16x8*)(vb + (size_t)t * 32 * FA_VP + ks * 32);
                o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[t], 0, 0, 0);
            }
        }
        if (more) store_v((jt + 1) & 1);
    }
    // ---- out[i][h][d] = trunc(O^T[d][i] / l): lane = row i, dims 32 t + 8 g + 4 kg + (0..3)
    if (i < S) {
        const float inv = 1.0f / l;
        uint16_t* dst = p.out + ((size_t)i * H + h) * HD + 4 * kg;
#pragma unroll
        for (int t = 0; t < DT; t++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const uint32_t lo = (uint32_t)bf_trunc(o[t][4 * g] * inv) | ((uint32_t)bf_trunc(o[t][4 * g + 1] * inv) << 16);
                const uint32_t hi = (uint32_t)bf_trunc(o[t][4 * g + 2] * inv) | ((uint32_t)bf_trunc(o[t][4 * g + 3] * inv) << 16);
                *(uint2*)(dst + 32 * t + 8 * g) = make_uint2(lo, hi);
            }
    }
}

int fast_rg(int rw, int nch, int n_blocks) {
    const int force = knob(Knob::FAST_RG);
    if (force && rw % force == 0 && (force == 8 || force == 16 || force == 32 || force == 64)) return force;
    // measured on MI355X (8B shape, gpurun call A of round 2): LM head (2004 blocks of 64) 181 / 170 / 154 us with 8 / 16 / 32 rows per unit,
    // wq|wk|wv (192 blocks of 32) 14.1 / 13.0 / 17.0 us: the longer the contiguous run per wave load the better, as long as the
    // matrix still splits into a few units per CU
    if (rw % 64 == 0 && n_blocks >= 1024) return 64;
    if (rw % 32 == 0 && (long)n_blocks * (rw / 32) >= 1024) return 32;
    if (rw % 16 == 0 && (long)n_blocks * (rw / 16) >= 256) return 16;
    return 8;
}

template <int NCH, int EPI, bool NORM, int RG>
hipError_t launch_a_rg(const GemvParams* p, int rw, hipStream_t st) {
    auto kfn = fast_gemv_a<NCH, EPI, NORM, RG>;
    if (!p) return hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const size_t lds = (size_t)p->K * 4 + 4 * NCH * 64 * 4 + 64;
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const int units = p->n_blocks * (rw / RG);
    const int cap = knob(Knob::FAST_GRID_CAP);
    form_ran(RG == 64 ? Form::FAST_GEMV_A_RG64 : RG == 32 ? Form::FAST_GEMV_A_RG32 : RG == 16 ? Form::FAST_GEMV_A_RG16 : Form::FAST_GEMV_A_RG8, EPI);
    hipLaunchKernelGGL(kfn, dim3((unsigned)(units < cap ? units : cap), (unsigned)p->S), dim3(256), lds, st, *p, rw);
    return hipGetLastError();
}
template <int NCH, int EPI, bool NORM>
hipError_t launch_a(const GemvParams* p, int rw, hipStream_t st) {
    if (!p) {
        hipError_t e = launch_a_rg<NCH, EPI, NORM, 8>(nullptr, 0, nullptr);
        if (e == hipSuccess) e = launch_a_rg<NCH, EPI, NORM, 16>(nullptr, 0, nullptr);
        if (e == hipSuccess) e = launch_a_rg<NCH, EPI, NORM, 32>(nullptr, 0, nullptr);
        if (e == hipSuccess) e = launch_a_rg<NCH, EPI, NORM, 64>(nullptr, 0, nullptr);
        return e;
    }
    if (rw % 8 || p->K % 8) return hipErrorInvalidValue;
    switch (fast_rg(rw, NCH, p->n_blocks)) {
        case 64: return launch_a_rg<NCH, EPI, NORM, 64>(p, rw, st);
        case 32: return launch_a_rg<NCH, EPI, NORM, 32>(p, rw, st);
        case 16: return launch_a_rg<NCH, EPI, NORM, 16>(p, rw, st);
        default: return launch_a_rg<NCH, EPI, NORM, 8>(p, rw, st);
    }
}
template <int EPI> hipError_t launch_b(const GemvParams* p, hipStream_t st) {
    auto kfn = fast_gemv_b<EPI>;
    if (!p) return hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (p->K & 127) return hipErrorInvalidValue;
    const size_t lds = (size_t)p->K * 2 + 64;
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    form_ran(Form::FAST_GEMV_B, EPI);
    hipLaunchKernelGGL(kfn, dim3((unsigned)(p->n_blocks * 4), (unsigned)p->S), dim3(256), lds, st, *p);
    return hipGetLastError();
}

}  // namespace

// p == nullptr: raise the dynamic-LDS limits once (outside any stream capture)
extern "C" hipError_t lnbk_fast_gemv(const GemvParams* p, int rw, int nch, int epi, int norm, hipStream_t st) {
    if (rw == 4) {
        if (nch != 1 || norm) return hipErrorInvalidValue;
        if (epi == EPI_STORE) return launch_b<EPI_STORE>(p, st);
        if (epi == EPI_RESID) return launch_b<EPI_RESID>(p, st);
        return hipErrorInvalidValue;
    }
    if (nch == 2) return (epi == EPI_SILU_MUL && norm) ? launch_a<2, EPI_SILU_MUL, true>(p, rw, st) : hipErrorInvalidValue;
    switch (epi) {
        case EPI_STORE: return norm ? launch_a<1, EPI_STORE, true>(p, rw, st) : launch_a<1, EPI_STORE, false>(p, rw, st);
        case EPI_QKV_ROPE: return norm ? launch_a<1, EPI_QKV_ROPE, true>(p, rw, st) : hipErrorInvalidValue;
        case EPI_RESID: return norm ? hipErrorInvalidValue : launch_a<1, EPI_RESID, false>(p, rw, st);
        default: return hipErrorInvalidValue;
    }
}
// S >= 16 rows on the bf16 matrix cores.  K must be a multiple of 64 (128 for the row-broadcast layout): the caller falls back to the
// exact GEMM otherwise (hipErrorNotSupported).
extern "C" hipError_t lnbk_fast_gemm(const GemmParams* p, int epi, hipStream_t st) {
    if (!p) return hipErrorInvalidValue;
    if (p->K % FG_BK || (p->rw == 4 && (p->K & 127 || p->nch != 1)) || (p->rw != 4 && p->rw % 8)) return hipErrorNotSupported;
    const int layb = p->rw == 4;
    switch (epi) {
        case EPI_STORE: return p->nch == 1 ? launch_gemm_fast<EPI_STORE, 1>(p, layb, st) : hipErrorInvalidValue;
        case EPI_RESID: return p->nch == 1 ? launch_gemm_fast<EPI_RESID, 1>(p, layb, st) : hipErrorInvalidValue;
        case EPI_QKV_ROPE: return p->nch == 1 ? launch_gemm_fast<EPI_QKV_ROPE, 1>(p, layb, st) : hipErrorInvalidValue;
        case EPI_SILU_MUL: return p->nch == 2 ? launch_gemm_fast<EPI_SILU_MUL, 2>(p, layb, st) : hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
}
// prefill attention of the tolerance mode; head_dim 64 / 128 (others: hipErrorNotSupported -> the caller keeps the exact kernel)
extern "C" hipError_t lnbk_fast_attn(const AttnParams* p, hipStream_t st) {
    if (!p || p->S < 16) return hipErrorInvalidValue;
    const dim3 grid((unsigned)p->H, (unsigned)((p->S + 127) / 128));
    if (p->hd == 128) { form_ran(Form::FAST_ATTN_HD128); hipLaunchKernelGGL(fast_attn_prefill_kernel<128>, grid, dim3(256), 0, st, *p); }
    else if (p->hd == 64) { form_ran(Form::FAST_ATTN_HD64); hipLaunchKernelGGL(fast_attn_prefill_kernel<64>, grid, dim3(256), 0, st, *p); }
    else return hipErrorNotSupported;
    return hipGetLastError();
}
extern "C" hipError_t lnbk_fast_init(void) {
    static bool done = false;
    if (done) return hipSuccess;
    hipError_t e;
    if ((e = lnbk_fast_gemv(nullptr, 4, 1, EPI_STORE, 0, nullptr)) != hipSuccess) return e;
    if ((e = lnbk_fast_gemv(nullptr, 4, 1, EPI_RESID, 0, nullptr)) != hipSuccess) return e;
    if ((e = lnbk_fast_gemv(nullptr, 64, 2, EPI_SILU_MUL, 1, nullptr)) != hipSuccess) return e;
    if ((e = lnbk_fast_gemv(nullptr, 64, 1, EPI_STORE, 1, nullptr)) != hipSuccess) return e;
    if ((e = lnbk_fast_gemv(nullptr, 64, 1, EPI_STORE, 0, nullptr)) != hipSuccess) return e;
    if ((e = lnbk_fast_gemv(nullptr, 64, 1, EPI_QKV_ROPE, 1, nullptr)) != hipSuccess) return e;
    if ((e = lnbk_fast_gemv(nullptr, 64, 1, EPI_RESID, 0, nullptr)) != hipSuccess) return e;
    if ((e = launch_gemm_fast<EPI_STORE, 1>(nullptr, 0, nullptr)) != hipSuccess) return e;
    if ((e = launch_gemm_fast<EPI_RESID, 1>(nullptr, 0, nullptr)) != hipSuccess) return e;
    if ((e = launch_gemm_fast<EPI_QKV_ROPE, 1>(nullptr, 0, nullptr)) != hipSuccess) return e;
    if ((e = launch_gemm_fast<EPI_SILU_MUL, 2>(nullptr, 0, nullptr)) != hipSuccess) return e;
    done = true;
    return hipSuccess;
}
