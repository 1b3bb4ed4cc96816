// lnb_kernels.hip -- hand-written gfx950 (MI355X / CDNA4) kernels for LlamaTransformer.Forward.
//
// Reference behaviour restated (never copied): adalkiran/llama-nuts-and-bolts
//   src/model/llamatransformer.go:145-180 (Forward), :215-254 (block), :289-527 (attention),
//   :593-624 (SwiGLU), :633-660 (RMSNorm), :753-790 (RoPE); src/ml/operations_lineartransform.go:37-70.
//
// Design: "exact-order" kernels.  The reference defines every output as ONE sequential f32 chain over k followed by a
// bf16 truncation, so a kernel never splits k; it only decides which lane walks a chain and how that lane is fed.
// bf16 x bf16 products are exact in f32, so everything except the dependent add can be done by other lanes / waves:
//   * gemv_chain_kernel (norm-fused and fat matrices): weights re-tiled ONCE at load time into [N/RW][K/8][NCH][RW][8]
//     (one linear byte stream per row block); helper waves stream them HBM -> VGPR ring (hand-counted vmcnt), multiply by x
//     and leave f32 products in an LDS ring; ONE chain wave per CU only adds (v_pk_add_f32 for the two-chain w1|w3);
//   * rowcast_kernel (thin wo / w2): products stay in registers; 16 lanes of a DPP row hold the products of 16 consecutive
//     k and every lane adds them in order with v_add_f32_dpp row_newbcast -- no LDS round trip in the chain;
//   * RMSNorm is fused into the consuming GEMV; its sequential f32 sum of squares is evaluated EXACTLY in parallel with
//     composable parity maps (lnb_seqsum.h); RoPE + KV-cache append are fused into the QKV epilogue, SiLU*up and the
//     residual adds are epilogues too: 5 launches per transformer block;
//   * attn_exact_kernel: one position per lane for the scores, f64 softmax in the reference's order, exact-product PV.
// Every register prefetch ring is inline asm with hand-counted waits; tools/isa_audit.py checks the compiled code.
// Compile with -ffp-contract=off: every a*b+c below is either an explicit fmaf (product exact) or
// must stay two roundings.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <type_traits>
#include "lnb_device.h"
#include "lnb_seqsum.h"
#include "lnb_gemv_geom.h"                                       // (XCh, rms_scratch_bytes, gq_ncw, GQ_SLOTS: what the launch checks share with the kernels)
#include "lnb_wpack.h"
#include "../../include/lnb.h"                                // (LNB_NORM_*: the forms of lnbk_gemv_norm_report)

#define DEVINL __device__ __forceinline__
#define LNB_SAMPLE_FN DEVINL
#define LNB_SAMPLE_FDIV(a, b) __fdiv_rn(a, b)
#define LNB_SAMPLE_NO_SERIAL                 // (the serial whole-row walk is the host's: tests/native/sample_test.cpp)
#include "lnb_sample.h"

DEVINL float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
DEVINL float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
DEVINL float bf_wide(uint16_t b) { return __uint_as_float(((uint32_t)b) << 16); }
DEVINL uint16_t bf_trunc(float f) { return (uint16_t)(__float_as_uint(f) >> 16); }   // bfloat16.go:31-33

DEVINL uint4 ld_nt_u4(const void* p) {
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    u4v v = __builtin_nontemporal_load((const u4v*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// one 8-wide k chunk of one chain: acc <- acc + x_k*w_k, k ascending (operations_lineartransform.go:46-65).
// bf16*bf16 is exact in f32, so fmaf == mul-then-add unless the product underflows 2^-126.
DEVINL float mac8(float acc, const float4& xa, const float4& xb, const uint4& w) {
    acc = fmaf(xa.x, bf_lo(w.x), acc); acc = fmaf(xa.y, bf_hi(w.x), acc);
    acc = fmaf(xa.z, bf_lo(w.y), acc); acc = fmaf(xa.w, bf_hi(w.y), acc);
    acc = fmaf(xb.x, bf_lo(w.z), acc); acc = fmaf(xb.y, bf_hi(w.z), acc);
    acc = fmaf(xb.z, bf_lo(w.w), acc); acc = fmaf(xb.w, bf_hi(w.w), acc);
    return acc;
}

// ------------------------------------------------------------------------------------------------
// The serial chains.  Measured on gfx950 (tools/microbench.hip, profiles/): ONE wave issues one
// instruction per ~4.4 cycles whatever it is, and a dependent v_add_f32 / v_fmac_f32 costs 4.33
// cycles, so a k-ordered chain runs at its latency floor only if the wave that owns it executes ~1
// instruction per k step.  bf16*bf16 products are EXACT in f32, so the chain is split by role:
//   helper waves (other SIMDs of the CU) unpack the bf16 weights, multiply by x and leave the exact f32
//   products in LDS;  the chain wave only does  acc = acc + p_k  (one v_add_f32 per step, operands
//   fetched 4 steps per ds_read_b128), with all 64 lanes active (a partially masked wave issues slower).
// mul-then-add is also literally what the reference does (operations_lineartransform.go:60-64).
// ------------------------------------------------------------------------------------------------
DEVINL float add4(float acc, const float4& p) { acc += p.x; acc += p.y; acc += p.z; acc += p.w; return acc; }
// zero-instruction "use" of 16 loaded registers: makes hipcc place ONE counted s_waitcnt lgkmcnt(N) for the whole
// group (LDS returns in order) instead of one wait per ds_read_b128 result in front of the adds
DEVINL void touch16(const float4& a, const float4& b, const float4& c, const float4& d) {
    asm volatile("" ::"v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w),
                 "v"(c.x), "v"(c.y), "v"(c.z), "v"(c.w), "v"(d.x), "v"(d.y), "v"(d.z), "v"(d.w));
}
typedef float f32x2 __attribute__((ext_vector_type(2)));
DEVINL float4 mul4(const float4& x, float w0, float w1, float w2, float w3) {   // packed f32 multiplies (exact products)
    f32x2 a = {x.x, x.y}, b = {x.z, x.w}, u = {w0, w1}, v = {w2, w3};
    a = a * u; b = b * v;
    return make_float4(a.x, a.y, b.x, b.y);
}


// ---- x staging (cooperative: the chain wave and the helper waves are the NS "stagers") -----------------
// x row -> LDS as f32, zero padded up to kpad (a whole number of stages + 64 floats of slack, so the
// software-pipelined readers may run one group ahead), optionally through the fused RMSNorm.
// The global loads of x are ISSUED BEFORE the loaders start their LDS-DMA burst (barrier B0) -- otherwise the
// 8 KB of x queue behind ~56 KiB of weight prefetch per CU (measured: +4 us per launch).
// 512-element chunks per stager wave held in registers: 12 for the plain kernels (K up to 18k with 3 stagers), 6 for the
// RMSNorm kernels (K = dim <= 8192; they also hold the norm weights and must stay clear of the 256-VGPR budget): XCh<NORM> of lnb_gemv_geom.h
// X_CH (deduced from the register arrays) is a compile-time property of the kernel instance: the launchers pick the smallest count that covers the
// row (2 for K = 4096 -- round 5: the norm-fused kernels used to carry 6 chunks' worth of clamped loads, lane-varying compares and registers
// through x_issue / x_store / x_normalize; of the 2 k cycles x_normalize took, ~1.7 k were control flow around five empty rounds)
template <bool NORM, int NS, int X_CH>
DEVINL void x_issue(const GemvParams& p, const uint16_t* xrow, int sidx, int lane, uint4 (&xv)[X_CH], uint4 (&nv)[X_CH]) {
#pragma unroll
    for (int i = 0; i < X_CH; i++) {
        // UNCONDITIONAL loads (address clamped, value zeroed afterwards): a predicated load would make hipcc
        // wait for each one before issuing the next (measured: 12 serialized round trips)
        const int k = ((i * NS + sidx) * 64 + lane) * 8;
        const int kc = k < p.K ? k : p.K - 8;
        uint4 a = *(const uint4*)(xrow + kc);
        uint4 b = make_uint4(0, 0, 0, 0);
        if (NORM) b = *(const uint4*)(p.norm_w + kc);
        const bool in = k < p.K;
        xv[i] = make_uint4(in ? a.x : 0u, in ? a.y : 0u, in ? a.z : 0u, in ? a.w : 0u);
        nv[i] = b;
    }
}
// squares (NORM: Pow(x,2), exact in f32, operations_impl.go:197-217) or plain values; zeros in [K, kpad)
template <bool NORM, int NS, int X_CH>
DEVINL void x_store(const GemvParams& p, float* xs, int kpad, int sidx, int lane, const uint4 (&xv)[X_CH]) {
#pragma unroll
    for (int i = 0; i < X_CH; i++) {
        const int k = ((i * NS + sidx) * 64 + lane) * 8;
        if (k < kpad) {
            float4 a = make_float4(bf_lo(xv[i].x), bf_hi(xv[i].x), bf_lo(xv[i].y), bf_hi(xv[i].y));
            float4 c = make_float4(bf_lo(xv[i].z), bf_hi(xv[i].z), bf_lo(xv[i].w), bf_hi(xv[i].w));
            if (NORM) {
                a.x = a.x * a.x; a.y = a.y * a.y; a.z = a.z * a.z; a.w = a.w * a.w;
                c.x = c.x * c.x; c.y = c.y * c.y; c.z = c.z * c.z; c.w = c.w * c.w;
            }
            *(float4*)(xs + k) = a; *(float4*)(xs + k + 4) = c;
        }
    }
}
// RMSNorm.doNormalization (llamatransformer.go:641-660): Mean = serial f32 sum of the squares in xs, k ascending
// (operations_impl.go:236-251), /K, +eps (f32), f32(1/sqrt(f64)).
//
// 4096 dependent roundings cost >= 7.4 us as a plain chain (measured ~15 us with its LDS reads) in front of EVERY
// workgroup of the RMSNorm-fused GEMVs.  The sum is evaluated EXACTLY in parallel instead (lnb_seqsum.h): inside one
// binade an f32 add of a non-negative term is the integer map M -> M + c_{M&1}, and such maps compose.
//   helpers (NH waves): lane = one leaf of 8 consecutive squares; approximate prefix sums (wave scan + wave totals) guess
//                       the leaf's binade; the leaf map is folded; a segmented inclusive wave scan composes every run of
//                       valid equal-binade leaves; run ends and invalid leaves are flagged in a 64-bit item mask;
//   chain wave (walker): adds the first RMS_HEAD squares one by one (the sum changes binade every few terms there) while
//                       the helpers fold, then visits only the items: a run's composed map is applied when it starts
//                       exactly at the walker's position, its binade matches the running sum and the sum stays inside it
//                       (a wrong guess can never be used); anything else is replayed term by term.
// Bit-identical to the sequential loop for every input (fuzzed on the CPU: tests/test_seqsum.py emulates this lane by
// lane; on the GPU: tests/test_gpu_parity.py through lnb_op_rmsnorm_linear); ~17 items + ~5 replayed leaves for gaussian x.
// A leaf is seq_leaf_size(K, NH*64) terms (one leaf per folding lane; the last one may run into the zero padding).
constexpr int RMS_HEAD = 256;
// LDS scratch (the idle product ring; rms_scratch_bytes of lnb_gemv_geom.h): SeqNode rec[NH][64] | uint64 items[NH] | float wtot[NH] | uint32 scan_failed[NH] |
//                                      SeqItem list[NH][128] (each wave's items of the branch-free walk, in leaf order) | uint32 {count, uncovered}[NH] |
//                                      64 spare bytes, of which the REPORT instantiations use the first 8: the walker's report address (rms_report_park)
// Folding waves: every helper (-DLNB_RMS_NF_MAX=4 restricts the fold to four waves on four different SIMDs -- waves w and w+4 of a workgroup
// share one: HW_ID read per wave, round 4 -- with leaves of 16 terms instead of 12: measured SLOWER, wq|wk|wv 21.2 vs 20.1 us; the fold's time
// follows its instruction count per wave, not the number of waves on a SIMD).  Helpers past the limit only pass the fold's two barriers.
// ring stages a norm-fused kernel's helper issues IN FRONT of the fold (the rest behind it): wq|wk|wv, w1|w3 (two chains), output.
// All R in front stalls the folding waves ~3 k cycles in the issue queue (round 4, first half: everything behind the fold); FOUR of w1|w3's
// eight do not, and the HBM pipe is already streaming when the prologue ends: w1|w3 44.1 -> 43.0 us, block 127.4 -> 126.1 (0 / 2 / 4 / 6 stages:
// 44.1 / 43.6 / 43.0 / 43.8); wq|wk|wv (20.2 -> 20.6 at four) and the output product (159.0 -> 159.9) want none.
#ifndef LNB_EARLY_QUAD
#define LNB_EARLY_QUAD 0
#endif
#ifndef LNB_EARLY_W13
#define LNB_EARLY_W13 4
#endif
#ifndef LNB_EARLY_HEAD
#define LNB_EARLY_HEAD 0
#endif
// the packed-source forms have macros of their own (a packed stage is 52 bytes per lane, not 32 per load: what suits the raw form need not suit them)
#ifndef LNB_EARLY_W13P
#define LNB_EARLY_W13P 2                                    // gate|up from the 13-bit copy: 2 / 3 / 4 -> block 119.4 / 119.8 / 120.5 us, headline +1.0 % at 2 (profiles/head_packed.md, section 5)
#endif
#ifndef LNB_EARLY_HEADP
#define LNB_EARLY_HEADP 2                                   // the LM head from the 13-bit copy: 0 / 2 -> launch 151.6 / 150.1 us and 149.9 / 148.3 us on two boxes (same section)
#endif
// (LNB_RMS_NF_MAX, rms_nf: lnb_seqsum.h -- the host emulation folds on the same wave counts)
__host__ __device__ inline size_t rms_list_off(int NH) { return (size_t)NH * 528; }
__host__ __device__ inline size_t rms_meta_off(int NH) { return (size_t)NH * (528 + 2048); }

// wave scans on DPP data movement (VALU, no LDS round trip like ds_bpermute): in-row shifts by 1, 2, 4, 8, then lane 15 of a row
// into the next row (rows 1, 3) and lane 31 into rows 2, 3 -- the classic gfx9 inclusive-scan order.  `old` is what lanes
// without a source keep.
template <int CTRL, int ROWMASK> DEVINL int dpp_mov(int v, int old) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROWMASK, 0xf, false); }
template <int D> DEVINL int dpp_row_shr(int v, int old) { return dpp_mov<0x110 + D, 0xf>(v, old); }       // lane i <- lane i-D inside its row of 16
DEVINL int dpp_bcast15(int v, int old) { return dpp_mov<0x142, 0xa>(v, old); }                             // rows 1,3 <- lane 15 of the row before
DEVINL int dpp_bcast31(int v, int old) { return dpp_mov<0x143, 0xc>(v, old); }                             // rows 2,3 <- lane 31
DEVINL int dpp_wave_shr1(int v, int old) { return dpp_mov<0x138, 0xf>(v, old); }                           // lane i <- lane i-1 (whole wave)
DEVINL int dpp_wave_shl1(int v, int old) { return dpp_mov<0x130, 0xf>(v, old); }                           // lane i <- lane i+1
DEVINL float wave_inclusive_sum(float v) {
#define LNB_SUM_STEP(EXPR) { const float o_ = __int_as_float(EXPR); v += o_; }
    LNB_SUM_STEP(dpp_row_shr<1>(__float_as_int(v), 0)) LNB_SUM_STEP(dpp_row_shr<2>(__float_as_int(v), 0))
    LNB_SUM_STEP(dpp_row_shr<4>(__float_as_int(v), 0)) LNB_SUM_STEP(dpp_row_shr<8>(__float_as_int(v), 0))
    LNB_SUM_STEP(dpp_bcast15(__float_as_int(v), 0)) LNB_SUM_STEP(dpp_bcast31(__float_as_int(v), 0))
#undef LNB_SUM_STEP
    return v;
}

// sum of a double over the wave, every lane gets it: six DPP steps on the two 32-bit halves (VALU data movement) + two v_readlane, instead of the twelve
// ds_bpermute round trips a __shfl_xor butterfly of doubles costs (~1.2 k cycles in front of attn_exact_kernel's certified p_j).  Only ever used for
// ESTIMATES with a rigorous error bound (the softmax denominator's tree sum): the order of the additions is free.
DEVINL double wave_sum_f64(double v) {
#define LNB_DSUM_STEP(MOV) { const int lo_ = MOV(__double2loint(v), 0), hi_ = MOV(__double2hiint(v), 0); v += __hiloint2double(hi_, lo_); }
    LNB_DSUM_STEP(dpp_row_shr<1>) LNB_DSUM_STEP(dpp_row_shr<2>) LNB_DSUM_STEP(dpp_row_shr<4>) LNB_DSUM_STEP(dpp_row_shr<8>)
    LNB_DSUM_STEP(dpp_bcast15) LNB_DSUM_STEP(dpp_bcast31)
#undef LNB_DSUM_STEP
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

DEVINL void rms_load16(float (&tv)[16], const float* q, int c, int LEAF) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c + 4 * i < LEAF) v = *(const float4*)(q + c + 4 * i);       // (wave-uniform)
        tv[4 * i] = v.x; tv[4 * i + 1] = v.y; tv[4 * i + 2] = v.z; tv[4 * i + 3] = v.w;
    }
}
DEVINL float rms_tree16(const float (&tv)[16]) {
    return (((tv[0] + tv[1]) + (tv[2] + tv[3])) + ((tv[4] + tv[5]) + (tv[6] + tv[7]))) + (((tv[8] + tv[9]) + (tv[10] + tv[11])) + ((tv[12] + tv[13]) + (tv[14] + tv[15])));
}
// REPORT (the instantiations lnb_op_rmsnorm_sum launches, never production's): the wave's flag word says WHY the row takes the record walk
// TIMING (the instantiations launched with GemvParams.dbg set, never production's): the fold / walk time goes to t_dbg; false: no clock read, no dbg branch
template <int NH, bool REPORT = false, bool TIMING = false> DEVINL void rms_fold(const GemvParams& p, const float* xs, char* scratch, int hw, int lane, long long& t_dbg) {
    if (hw < 0) { __builtin_amdgcn_s_barrier(); __builtin_amdgcn_s_barrier(); return; }      // a helper that does not fold: X1, X2
    const long long tf0_ = (TIMING && p.dbg) ? clock64() : 0;
    const int LEAF = seq_leaf_size(p.K, NH * 64), nleaf = (p.K + LEAF - 1) / LEAF;
    SeqNode* rec = (SeqNode*)scratch;
    unsigned long long* items = (unsigned long long*)(scratch + (size_t)NH * 512);
    float* wtot = (float*)(scratch + (size_t)NH * 520);
    const int headleaf = (p.K < RMS_HEAD ? p.K : RMS_HEAD) / LEAF;
    const int b = hw * 64 + lane;
    const float* q = xs + (size_t)(b < nleaf ? b : nleaf - 1) * LEAF;    // (xs is zero padded past K: the last leaf may over-read)
    // the leaf's terms are read from LDS ONCE, into registers (16 per pass; what lies past the leaf is replaced by +0, which changes no sum):
    // the three passes below were bound by their LDS reads (a loop of dependent ds_read_b128 -> wait -> add; lanes 48 or 64 bytes apart
    // conflict 3- or 4-way), not by their arithmetic.  Leaves of more than 16 terms (K > 4096) re-read chunk by chunk.
    float tv[16];
    rms_load16(tv, q, 0, LEAF);
    float bsum = rms_tree16(tv);                                         // only feeds the guess
    for (int c = 16; c < LEAF; c += 16) { rms_load16(tv, q, c, LEAF); bsum += rms_tree16(tv); }
    bsum = b < nleaf ? bsum : 0.0f;
    const float incl = wave_inclusive_sum(bsum);             // (x + 0.0f for lanes without a source: only feeds the guess)
    if (lane == 63) wtot[hw] = incl;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();                                        // X1: wave totals published
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    float base = 0.0f;
#pragma unroll
    for (int w = 0; w < NH; w++) { const float v = wtot[w]; base += w < hw ? v : 0.0f; }
    SeqNode n; n.a = 0u; n.b = 0u;
    const float lo = base + (incl - bsum), hi = base + incl;           // approximate running sum in front of / behind this leaf
    {   // the leaf's parity map from two simulated f32 running sums (lnb_seqsum.h: seq_leaf): 2 adds per term
        const int32_t e = b < nleaf ? seq_guess_tight(lo, hi) : 0;
        float s0, s1; seq_sim_init(e, s0, s1);
        for (int c = 0; c < LEAF; c += 16) {
            if (LEAF > 16) rms_load16(tv, q, c, LEAF);
#pragma unroll
            for (int i = 0; i < 8; i++) { s0 = s0 + tv[i]; s1 = s1 + tv[i]; }
            if (LEAF > 8) {                                              // (wave-uniform: the terms past the leaf are zeros, skipped instead of added)
#pragma unroll
                for (int i = 8; i < 12; i++) { s0 = s0 + tv[i]; s1 = s1 + tv[i]; }
            }
            if (LEAF > 12) {
#pragma unroll
                for (int i = 12; i < 16; i++) { s0 = s0 + tv[i]; s1 = s1 + tv[i]; }
            }
        }
        if (b < nleaf) n = seq_sim_node(e, s0, s1);
    }
    if (b < nleaf && bsum == 0.0f && (n.a >> 24) == 0u) n.a = SEQ_ZERO_LEAF;      // nothing to add, whatever the running sum is
    // A leaf that enters the next binade: split at the crossing term (lnb_seqsum.h: seq_split_leaf, here branch-free for the whole wave --
    // only waves that hold such a leaf run it): map of the terms before x*, x*, map of the terms after it.
    SeqItem sa, sb2; sa.x = sa.c0 = 0u; sa.d = 0; sa.e = 0u; sb2 = sa;
    bool split_ok = false;
    {
        const bool cand = b < nleaf && (n.a >> 24) == 0u && n.a != SEQ_ZERO_LEAF && seq_split_candidate(lo, hi);
        if (__ballot(cand)) {
            const SeqSplit sp = LEAF <= 12 ? seq_split_leaf(tv, 12, lo, hi) : LEAF <= 16 ? seq_split_leaf(tv, 16, lo, hi) : seq_split_leaf(q, LEAF, lo, hi);
            split_ok = cand && sp.ok; sa = sp.a; sb2 = sp.b;
        }
    }
    SeqNode left; left.a = (uint32_t)dpp_wave_shr1((int)n.a, 0); left.b = 0u;
    int f = seq_is_start(lane, n, left, b == headleaf);
    const int fnext = dpp_wave_shl1(f, 1);
    const unsigned long long mask = __ballot((n.a >> 24) == 0u || lane == 63 || fnext);
    if (lane == 0) items[hw] = mask;
    int start = lane;
    // segmented inclusive scan of the leaf maps (associative: a run absorbs the run that ends right in front of it), six DPP steps
    int failed = 0;                                                      // a composition that did not go through (cannot happen inside a verified binade)
#define LNB_SEG_STEP(MOV, VALID) { SeqNode o_; o_.a = (uint32_t)MOV((int)n.a, 0); o_.b = (uint32_t)MOV((int)n.b, 0); const int ofs_ = MOV((f << 8) | start, 0); \
                                   if ((VALID) && !f) failed |= seq_scan_step(n, f, start, o_, ofs_ >> 8, ofs_ & 0xFF) ^ 1; }
    LNB_SEG_STEP(dpp_row_shr<1>, (lane & 15) >= 1) LNB_SEG_STEP(dpp_row_shr<2>, (lane & 15) >= 2)
    LNB_SEG_STEP(dpp_row_shr<4>, (lane & 15) >= 4) LNB_SEG_STEP(dpp_row_shr<8>, (lane & 15) >= 8)
    LNB_SEG_STEP(dpp_bcast15, (lane & 16) != 0) LNB_SEG_STEP(dpp_bcast31, lane >= 32)
#undef LNB_SEG_STEP
    {   // the wave's items of the branch-free walk, in leaf order: the end of every run (its composed map), the two items of every split leaf;
        // leaves of exact zeros emit nothing; a leaf that nothing covers marks the row for the old walk
        const bool pick = ((mask >> lane) & 1ull) && b >= headleaf && b < nleaf && n.a != SEQ_ZERO_LEAF;
        const bool valid = (n.a >> 24) != 0u;
        // round 6: a leaf that no guess covers -- too close to a binade edge to call (SEQ_MARGIN), neither a run member nor cleanly split -- is replayed INSIDE the
        // branch-free walk as LEAF single-term items (exact adds, no binade assumed) instead of sending the whole row to the record walk (2.7 % of gaussian rows at
        // K = 4096, 6.8 % at 8192 -> ~0 / < 1 %: tests/test_seqsum.py emulates it).  Non-finite squares stay the record walk's business.
        const bool single = pick && !valid && !split_ok && bsum <= 3.4028234e38f;
        const unsigned long long m1 = __ballot(pick && (valid || split_ok)), m2 = __ballot(pick && !valid && split_ok), m3 = __ballot(single);
        const unsigned cntw = (unsigned)(__builtin_popcountll(m1) + __builtin_popcountll(m2)) + (unsigned)LEAF * (unsigned)__builtin_popcountll(m3);
        const bool fits = cntw <= 128u;                                  // (the wave's list segment; the walker takes at most 64 items per row anyway)
        const unsigned long long mu = __ballot(pick && !valid && !split_ok && !single) | ((REPORT || fits) ? 0ull : 1ull);
        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m1, 0u)) +
                              __builtin_amdgcn_mbcnt_hi((unsigned)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m2, 0u)) +
                              (unsigned)LEAF * __builtin_amdgcn_mbcnt_hi((unsigned)(m3 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m3, 0u));
        uint4* list = (uint4*)(scratch + rms_list_off(NH)) + hw * 128;
        if (fits) {
            if (pick && valid) { const SeqItem it = seq_item_of_node(n); list[rank] = make_uint4(it.x, it.c0, (uint32_t)it.d, it.e); }
            if (pick && !valid && split_ok) {
                list[rank] = make_uint4(sa.x, sa.c0, (uint32_t)sa.d, sa.e);
                list[rank + 1] = make_uint4(sb2.x, sb2.c0, (uint32_t)sb2.d, sb2.e);
            }
            if (single) for (int i = 0; i < LEAF; i++) list[rank + i] = make_uint4(__float_as_uint(q[i]), 0u, 0u, SEQ_ANY_BINADE);      // (terms from the LDS: rare path)
        }
        if (lane == 0) {
            uint32_t* meta = (uint32_t*)(scratch + rms_meta_off(NH)) + hw * 2;
            meta[0] = fits ? cntw : 0u;
            meta[1] = (mu ? 1u : 0u) | ((REPORT && !fits) ? 2u : 0u);    // != 0: the row takes the record walk (REPORT: 1 a leaf nothing covers, 2 the segment is too short)
        }
    }
    n.b |= (uint32_t)start << 24;                                        // c1 < 2^24: the run's first leaf rides in the top byte
    rec[hw * 64 + lane] = n;
    { const unsigned long long fm = __ballot(failed != 0); if (lane == 0) ((uint32_t*)(scratch + (size_t)NH * 524))[hw] = fm ? 1u : 0u; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (TIMING && p.dbg) t_dbg = clock64() - tf0_;                       // fold time incl. the X1 wait
    __builtin_amdgcn_s_barrier();                                        // X2: records published
}

// the items of one wave's 64 leaves: rc = this lane's record, from leaf `pos` up to `nloc`; sq = the wave's first square.
// Scalar code (SGPRs + v_readlane); the accept test is evaluated branch-free, the only branch is the rare replay.
DEVINL uint32_t rms_walk_heap(uint32_t sb, const SeqNode& rc, unsigned long long mask, int pos, int nloc, const float* sq, int LEAF) {
    mask &= ~0ull << pos;                                                // items in front of the head are done
    if (nloc < 64) mask &= ~(~0ull << nloc);                             // leaves past the end of the row
    // leaves of exact zeros that no binade could be guessed for (a row that starts with zeros, or is all zeros): not visited, stepped
    // over -- x + 0 == x.  (Visiting them one by one made an all-zero row 1.8x, replaying them 2.7x the kernel time.)
    const unsigned long long zm = __ballot(rc.a == SEQ_ZERO_LEAF);
    mask &= ~zm;
    while (mask) {
        const int i = __builtin_ctzll(mask);
        mask &= mask - 1;
        const uint32_t na = (uint32_t)__builtin_amdgcn_readlane((int)rc.a, i), nb = (uint32_t)__builtin_amdgcn_readlane((int)rc.b, i);
        const int st = (int)(nb >> 24);
        if (st > pos && ((((1ull << st) - 1ull) & (~0ull << pos)) & ~zm) == 0ull) pos = st;       // only zeros between the walker and this run
        const uint32_t e = na >> 24, es = sb >> 23;
        const uint32_t M = (sb & 0x7FFFFFu) | 0x800000u;
        const uint32_t Mn = M + (((M & 1u) ? nb : na) & 0xFFFFFFu);
        const uint32_t ok = (uint32_t)((nb >> 24) == (uint32_t)pos) & (uint32_t)(e == es) & (uint32_t)(e != 0u) & (uint32_t)(Mn < 0x1000000u);
        const uint32_t snew = (es << 23) | (Mn & 0x7FFFFFu);
        if (__builtin_expect(!ok, 0)) {                                  // replay leaves pos..i term by term
            float f = __uint_as_float(sb);
            const float* qe = sq + (size_t)(i + 1) * LEAF;
            for (const float* q = sq + (size_t)pos * LEAF; q < qe; q += 4) f = add4(f, *(const float4*)q);
            sb = (uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(f));
        } else sb = snew;
        pos = i + 1;
    }
    return sb;
}

// The same walk without the per-item bookkeeping (round 4: 280 -> ~90 cycles per item, 6.8 k -> ~2.5 k cycles per norm).  The items of a wave
// TILE its leaves by construction -- every non-zero leaf is either invalid (an item of its own) or belongs to exactly one run, and a run's
// record covers [its first leaf, the item's lane] -- unless a composition inside the segmented scan failed, which the folding wave reports
// (scan_failed: then rms_walk_heap above, which checks every record's start, is used).  So an item only has to match the running sum's
// binade and keep the sum inside it; anything else is replayed from the leaf behind the previous item (leaves of exact zeros in between
// add nothing).  A replay fetches up to 16 terms at once (one LDS round trip per 16 terms instead of one per 4).
// tq: this wave-set's x^2 terms, lane l holding leaf l's (up to 12) terms -- loaded by the walker while it waits for the fold; `regs` says
// whether they are there (LEAF <= 12).  A replayed leaf then costs a v_readlane + v_add per term (~120 cycles) instead of an LDS round trip
// behind a cold branch (~750 measured).
DEVINL uint32_t rms_walk_fast(uint32_t sb, const SeqNode& rc, unsigned long long mask, int pos, int nloc, const float* sq, int LEAF, int& cnt) {
    mask &= ~0ull << pos;
    if (nloc < 64) mask &= ~(~0ull << nloc);
    mask &= ~__ballot(rc.a == SEQ_ZERO_LEAF);
    // (tools/chainbench4.hip: what this loop pays for is the hand-offs between the vector and the scalar unit -- a dynamic v_readlane
    //  between scalar ops ~50 cycles, a branch on a vector result ~40 even when not taken, a taken branch ~22 -- not the arithmetic:
    //  the same recurrence on the vector unit measured no faster)
    while (mask) {
        const int i = __builtin_ctzll(mask);
        mask &= mask - 1;
        const uint32_t na = (uint32_t)__builtin_amdgcn_readlane((int)rc.a, i), nb = (uint32_t)__builtin_amdgcn_readlane((int)rc.b, i);
        // M + c on the f32 BITS of the running sum: no carry into the exponent field <=> the sum stays inside the binade
        const uint32_t e = na >> 24;
        const uint32_t t = sb + (((sb & 1u) ? nb : na) & 0xFFFFFFu);
        const uint32_t bad = ((t ^ sb) >> 23) | (e ^ (sb >> 23)) | ((e - 1u) >> 31);      // (e == 0 as integer arithmetic: hipcc sent the comparison through the vector unit and back)
        cnt += 0x10000;                                                  // (diagnostics: items << 16 | replays)
        if (__builtin_expect(bad == 0u, 1)) sb = t;
        else {                                                           // replay leaves pos..i term by term
            cnt += 1;
            float f = __uint_as_float(sb);
            {
                const float* qe = sq + (size_t)(i + 1) * LEAF;
                for (const float* q = sq + (size_t)pos * LEAF; q < qe; q += 16) {
                    // (reads past qe stay inside the zero-padded x buffer; what lies past the range is replaced by +0, and f + 0 == f)
                    float4 v0 = *(const float4*)q, v1 = *(const float4*)(q + 4), v2 = *(const float4*)(q + 8), v3 = *(const float4*)(q + 12);
                    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (q + 4 >= qe) v1 = z;
                    if (q + 8 >= qe) v2 = z;
                    if (q + 12 >= qe) v3 = z;
                    f = add4(f, v0); f = add4(f, v1); f = add4(f, v2); f = add4(f, v3);
                }
            }
            sb = (uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(f));
        }
        pos = i + 1;
    }
    return sb;
}

// REPORT: the instantiations that lnb_op_rmsnorm_sum launches (production launches the REPORT = 0 ones, whose code is what it was): this row's three words
// -- sum bits, r bits, path word (RMS_PATH_*, lnb_seqsum.h) -- go to `o` (1: the stand-alone norm kernels) or to the address rms_report_park left in the
// spare bytes behind the LDS scratch (2: the norm-fused kernels, which have no scalar registers to carry it across the x staging and the walk)
template <int NH> DEVINL void rms_report_park(const GemvParams& p, char* scratch, int row, int lane) {
    if (lane == 0) *(uint32_t* volatile*)(scratch + rms_scratch_bytes(NH) - 64) = (p.norm_out && row >= 0) ? p.norm_out + (size_t)row * 3 : nullptr;
}
template <int NH, int REPORT = 0, bool TIMING = false> DEVINL float rms_scale_wide(const GemvParams& p, const float* xs, const char* scratch, int lane, long long& t_dbg, uint32_t* o = nullptr) {
    const int K = p.K, LEAF = seq_leaf_size(K, NH * 64), nleaf = (K + LEAF - 1) / LEAF;
    const SeqNode* rec = (const SeqNode*)scratch;
    const unsigned long long* items = (const unsigned long long*)(scratch + (size_t)NH * 512);
    __builtin_amdgcn_s_barrier();                                        // X1 (the helpers' wave totals)
    // head of the sum, term by term, while the helpers fold
    const int headleaf = (K < RMS_HEAD ? K : RMS_HEAD) / LEAF, head = headleaf * LEAF;
    float sum = 0.0f;
    for (int k0 = 0; k0 < head; k0 += 4) sum = add4(sum, *(const float4*)(xs + k0));
    __builtin_amdgcn_s_barrier();                                        // X2 (the records)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    uint32_t sb = (uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(sum));
    const long long tw0_ = (TIMING && p.dbg) ? clock64() : 0;
    int cnt = 0;
    // ---- the row's item list (rms_fold), walked WITHOUT a branch per item -------------------------------------------------------
    // lane w < NH: wave w's item count and "something uncovered" flag; lane g: global item g, fetched from its wave's list segment
    bool done = false;
    int why = 0;
    {
        const uint2 meta = ((const uint2*)(scratch + rms_meta_off(NH)))[lane < NH ? lane : 0];
        const uint32_t failv = ((const uint32_t*)(scratch + (size_t)NH * 524))[lane < NH ? lane : 0];
        const unsigned long long badm = __ballot(lane < NH && (meta.y != 0u || failv != 0u));
        int tot = 0, wsel = 0, below = 0;                                // items in front of lane g's wave
#pragma unroll
        for (int w = 0; w < NH; w++) {
            const int cw = __builtin_amdgcn_readlane((int)meta.x, w);
            tot += cw;
            if (w + 1 < NH) { const bool past = lane >= tot; wsel += past ? 1 : 0; below = past ? tot : below; }
        }
        why = (badm ? 1 << 28 : 0) | (tot > 64 ? 2 << 28 : 0) | ((tot & 0xFF) << 8) | (int)((badm & 0xFF) << 20);
        if (badm == 0ull && tot <= 64) {
            const uint4 it = ((const uint4*)(scratch + rms_list_off(NH)))[wsel * 128 + (lane < tot ? lane - below : 0)];
            const float ix = __uint_as_float(lane < tot ? it.x : 0u);    // lanes past the list: identity items (never reached anyway)
            const uint32_t ic0 = lane < tot ? it.y : 0u;
            const int id = lane < tot ? (int)it.z : 0;
            // systolic recurrence: the running sum hops one lane per step (DPP wave_shr:1); lane g holds its true input at step g, computes
            // u = bits(f32(s) + x), t = u + c0 + (u & 1) d, latches t and hands it on.  Seven vector instructions per item, no scalar work.
            // (inline asm: the compiler turns (u & 1) * d into v_cmp + v_cndmask and the latch into v_cmp + v_cndmask -- two SGPR round trips
            // with their wait states per item; here: add (DPP), bfe, and, add3, latch through a constant lane mask in SGPRs, and the two
            // wait states a DPP read of a just-written VGPR needs -- s_nop 1: whatever the compiler put in front of the first step)
            uint32_t tv, lat = 0u, tmp;
            {   // item 0: every lane from the head's sum
                const uint32_t u0 = __float_as_uint(__uint_as_float(sb) + ix);
                tv = u0 + ic0 + (uint32_t)(-(int)(u0 & 1u) & id);
                lat = lane == 0 ? tv : 0u;
            }
#define LNB_ITEM_STEP(G) asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %3 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
                                      "v_bfe_i32 %2, %0, 0, 1\n\tv_and_b32 %2, %2, %4\n\tv_add3_u32 %0, %0, %5, %2\n\t" \
                                      "v_cndmask_b32_e64 %1, %1, %0, %6" \
                                      : "+v"(tv), "+v"(lat), "=&v"(tmp) : "v"(ix), "v"(id), "v"(ic0), "s"(1ull << (G)));
#define LNB_ITEM_STEP4(G) LNB_ITEM_STEP(G) LNB_ITEM_STEP((G) + 1) LNB_ITEM_STEP((G) + 2) LNB_ITEM_STEP((G) + 3)
            if (tot > 1) { LNB_ITEM_STEP(1) LNB_ITEM_STEP(2) LNB_ITEM_STEP(3) }
#pragma unroll
            for (int G = 4; G < 64; G += 4) if (G < tot) { LNB_ITEM_STEP4(G) }
#undef LNB_ITEM_STEP4
#undef LNB_ITEM_STEP
            // every item's check at once: lane g redoes its step from the latched output of lane g-1 (lane 0: the head's sum).  (The DPP move
            // is NOT inside a conditional: a lane masked off by the condition would be read as "no source lane".)
            const uint32_t lprev = (uint32_t)dpp_wave_shr1((int)lat, 0);
            const uint32_t sin = lane == 0 ? sb : lprev;
            const uint32_t u = __float_as_uint(__uint_as_float(sin) + ix);
            const uint32_t t = u + ic0 + (uint32_t)(-(int)(u & 1u) & id);
            const uint32_t bad = lane < tot ? (((t ^ u) >> 23) | (it.w != SEQ_ANY_BINADE ? (it.w ^ (u >> 23)) : 0u) | (t ^ lat)) : 0u;      // (single-term items assume no binade)
            if (__ballot(bad != 0u) == 0ull) {
                if (tot > 0) sb = (uint32_t)__builtin_amdgcn_readlane((int)lat, tot - 1);
                done = true;
                cnt = tot << 16;
            } else why |= 4 << 28;
        }
    }
    if (!done && p.norm_fb && blockIdx.x == 0 && lane == 0) atomicAdd(p.norm_fb, 1);       // (diagnostics: every workgroup walks the same row, one counts)
    if (!done) {
        // ---- the old walk (every record's binade verified item by item, crossing leaves replayed term by term): rows with a leaf that is
        // neither a run member nor cleanly split (non-finite terms, jumps of several binades, a crossing too close to call), with a guess
        // that did not hold, or with more than 64 items
        SeqNode rc[NH];
        unsigned long long mk[NH];
#pragma unroll
        for (int w = 0; w < NH; w++) { rc[w] = rec[w * 64 + lane]; mk[w] = items[w]; }
        const uint32_t badv = ((const uint32_t*)(scratch + (size_t)NH * 524))[lane < NH ? lane : 0];      // scan_failed[w] in lane w
        const unsigned long long badm = __ballot(badv != 0u);
        cnt = 1;
#pragma unroll
        for (int w = 0; w < NH; w++) {
            int nloc = nleaf - w * 64; nloc = nloc < 0 ? 0 : (nloc > 64 ? 64 : nloc);
            int pos = headleaf - w * 64; pos = pos < 0 ? 0 : pos;
            const unsigned lo32 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)mk[w]);
            const unsigned hi32 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(mk[w] >> 32));
            if (__builtin_expect((badm >> w) & 1ull, 0)) sb = rms_walk_heap(sb, rc[w], ((unsigned long long)hi32 << 32) | lo32, pos, nloc, xs + (size_t)w * 64 * LEAF, LEAF);
            else sb = rms_walk_fast(sb, rc[w], ((unsigned long long)hi32 << 32) | lo32, pos, nloc, xs + (size_t)w * 64 * LEAF, LEAF, cnt);
        }
    }
    if (TIMING && p.dbg) t_dbg = clock64() - tw0_;                       // walk time
    if constexpr (REPORT == 2) o = *(uint32_t* volatile*)(scratch + rms_scratch_bytes(NH) - 64);
    // (one scalar branch and selects behind it: every lane mask held across this block is a pair of scalar registers)
    if (REPORT && (__builtin_amdgcn_readfirstlane((int)(uintptr_t)o) | __builtin_amdgcn_readfirstlane((int)((uintptr_t)o >> 32))) != 0) {
        // the path word (RMS_PATH_*, lnb_seqsum.h; the host zeroes it): what the folding waves left in the LDS, read again here; lane g adds what it counts
        uint32_t val = 0u, fl = 0u;
#pragma unroll 1
        for (int w = 0; w < NH; w++) {
            const uint2 mw = ((const uint2*)(scratch + rms_meta_off(NH)))[w];                  // (every lane reads the same words)
            const uint32_t fv = ((const uint32_t*)(scratch + (size_t)NH * 524))[w];
            fl |= ((mw.y & 2u) ? RMS_PATH_NOFIT : 0u) | ((mw.y & 1u) ? RMS_PATH_UNCOVERED : 0u) | (fv ? RMS_PATH_SCANFAIL : 0u);
            const bool mine = (uint32_t)lane < mw.x;                     // done: at most 64 items, so a wave's segment holds at most 64
            const uint4 it = ((const uint4*)(scratch + rms_list_off(NH)))[w * 128 + (mine ? lane : 0)];
            val += !mine ? 0u : it.w == SEQ_ANY_BINADE ? 1u : it.x != 0u ? 256u : 0u;          // single-term items | split leaves << 8
        }
        const int rp = (cnt & 0xFFFF) - 1;                               // leaves replayed by rms_walk_fast
        const uint32_t own = done ? (uint32_t)cnt : ((uint32_t)why | fl | (uint32_t)(rp > 255 ? 255 : rp));
        val = (done ? val : 0u) + (lane == 0 ? own : 0u);
        atomicAdd(o + 2, val);
    }
    if (!done) cnt = why;
    if (TIMING && p.dbg && lane == 0) p.dbg[(size_t)4096 * 8 * 4 + ((size_t)blockIdx.x * 8 + 0) * 8 + 7] = cnt;   // stamp slot 7 of the walker: items << 16 | (old walk: 1 + ...)
    float mean = __fdiv_rn(__uint_as_float(sb), (float)K);
    mean = mean + p.eps;
    const float r = (float)(1.0 / sqrt((double)mean));
    if (REPORT && o && lane == 0) { o[0] = sb; o[1] = __float_as_uint(r); }
    return r;
}
// trunc(x*r) then trunc(.*w): two truncations (llamatransformer.go:656,638), from the registers loaded by x_issue
template <int NS, int X_CH>
DEVINL void x_normalize(const GemvParams& p, float* xs, int kpad, float r, int sidx, int lane, const uint4 (&xv)[X_CH], const uint4 (&nv)[X_CH]) {
#pragma unroll
    for (int i = 0; i < X_CH; i++) {
        const int k = ((i * NS + sidx) * 64 + lane) * 8;
        if (k >= p.K && k < kpad) {   // the (padded) squares may have spilled past K: the stage walkers need zeros there
            *(float4*)(xs + k) = make_float4(0.f, 0.f, 0.f, 0.f); *(float4*)(xs + k + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (k < p.K) {
            const uint4 v = xv[i], wv = nv[i];
            float4 a, c;
            a.x = bf_wide(bf_trunc(bf_wide(bf_trunc(bf_lo(v.x) * r)) * bf_lo(wv.x)));
            a.y = bf_wide(bf_trunc(bf_wide(bf_trunc(bf_hi(v.x) * r)) * bf_hi(wv.x)));
            a.z = bf_wide(bf_trunc(bf_wide(bf_trunc(bf_lo(v.y) * r)) * bf_lo(wv.y)));
            a.w = bf_wide(bf_trunc(bf_wide(bf_trunc(bf_hi(v.y) * r)) * bf_hi(wv.y)));
            c.x = bf_wide(bf_trunc(bf_wide(bf_trunc(bf_lo(v.z) * r)) * bf_lo(wv.z)));
            c.y = bf_wide(bf_trunc(bf_wide(bf_trunc(bf_hi(v.z) * r)) * bf_hi(wv.z)));
            c.z = bf_wide(bf_trunc(bf_wide(bf_trunc(bf_lo(v.w) * r)) * bf_lo(wv.w)));
            c.w = bf_wide(bf_trunc(bf_wide(bf_trunc(bf_hi(v.w) * r)) * bf_hi(wv.w)));
            *(float4*)(xs + k) = a; *(float4*)(xs + k + 4) = c;
        }
    }
}

// PX: lane distance of the RoPE partner row (2i <-> 2i+1): 1 when a lane is a row, 4 in gemv_quad_kernel (four lanes per row)
template <int NCH, int EPI, int PX = 1>
DEVINL void gemv_epilogue(const GemvParams& p, const float (&acc)[NCH], int m, int n, bool valid) {
    if (EPI == EPI_STORE) {
        if (valid) p.out[(size_t)m * p.n_rows + n] = bf_trunc(acc[0]);
    } else if (EPI == EPI_RESID) {
        // ml.Add (operations_impl.go:320-332): trunc(wide(x) + wide(y)), y = trunc(acc)
        if (valid) {
            size_t o = (size_t)m * p.n_rows + n;
            p.out[o] = bf_trunc(bf_wide(p.res[o]) + bf_wide(bf_trunc(acc[0])));
        }
    } else if (EPI == EPI_SILU_MUL) {
        // Silu table lookup on the raw bf16 bits (activations.go:36-39) then MultiplyElementwise (:614)
        if (valid) {
            uint16_t g = bf_trunc(acc[0]), u = bf_trunc(acc[NCH - 1]);
            uint16_t gs = bf_trunc(p.silu[g]);
            p.out[(size_t)m * p.n_rows + n] = bf_trunc(bf_wide(gs) * bf_wide(u));
        }
    } else if (EPI == EPI_QKV_ROPE) {
        // rows [0,q_dim) = xq, [q_dim,q_dim+kv_dim) = xk, rest = xv (llamatransformer.go:297-384)
        const int pos = p.st->pos + m;
        const uint16_t mine = bf_trunc(acc[0]);
        const uint16_t other = (uint16_t)__shfl_xor((int)mine, PX);      // RoPE partner (2i <-> 2i+1)
        if (valid) {
            if (n < p.q_dim + p.kv_dim) {
                // applyRotaryEmbeddings (:753-790): complex64 product evaluated in f64, narrowed, truncated
                const int d = n % p.head_dim, i = d >> 1;
                const float2 cs = *(const float2*)(p.cis + ((size_t)pos * (p.head_dim >> 1) + i) * 2);
                const double cr = (double)cs.x, ci = (double)cs.y;
                uint16_t r16;
                if ((n & 1) == 0) { double a = (double)bf_wide(mine), bb = (double)bf_wide(other); r16 = bf_trunc((float)(a * cr - bb * ci)); }
                else              { double a = (double)bf_wide(other), bb = (double)bf_wide(mine); r16 = bf_trunc((float)(a * ci + bb * cr)); }
                if (n < p.q_dim) p.q_out[(size_t)m * p.q_dim + n] = r16;
                else {                                                                // :402, K cache layout [kv head][d/8][position][8]
                    const int kc = n - p.q_dim, kh = kc / p.head_dim;
                    p.cache_k[(((size_t)kh * (p.head_dim >> 3) + (d >> 3)) * p.seq_len + pos) * 8 + (d & 7)] = r16;
                }
            } else {
                p.cache_v[(size_t)pos * p.kv_dim + (n - p.q_dim - p.kv_dim)] = mine;  // :403
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Exact-order streaming GEMV / skinny GEMM:   y[m, n] = trunc( sum_{k ascending} x[m,k] * W[n,k] )
//
// workgroup = 1 + NH waves, ONE workgroup per CU (every wave on its own SIMD: two issue-hungry waves on
// one SIMD halve each other's rate), ONE raw s_barrier per stage:
//   waves 1..NH  helpers: stream the block's bf16 weights HBM -> VGPR (16 B/lane non-temporal loads, a
//                         register ring of R stages in flight, COUNTED s_waitcnt vmcnt(N) -- never 0 in
//                         steady state), multiply by x (exact products) and leave f32 products
//                         [k4][chain][row][4] in a double-buffered LDS ring;
//   wave 0       chain  : RW rows (lane & (RW-1)), NCH chains per lane: per 16 k-steps 4 ds_read_b128 +
//                         16 v_add_f32 per chain.
// iteration t: helpers produce stage t | chain walks stage t-1.
// (An LDS-DMA loader wave + separate multiplier waves was measured first: the extra LDS round trip of the
//  bf16 bytes and the DMA's arbitration against ds traffic capped a CU at ~12 GB/s; see DESIGN.md.)
// A workgroup is PERSISTENT over its row blocks (b = wg, wg + n_wg, ...): x is staged (and RMS-normalised)
// once, the load pipeline runs across block boundaries, the epilogue runs at every block end.
// "thin" matrices (wq|wk|wv, wo, w2: latency bound) use RW=16/32 with one block per workgroup on all CUs;
// "fat" ones (w1|w3, output: HBM bound) use RW=64.
// grid.x = S * n_wg (m fastest so that the S workgroups sharing a weight block run together)
// dynamic LDS: [2 * 2*SA product ring][kpad f32 x + 16 B]
// ------------------------------------------------------------------------------------------------
// optional per-wave timing (GemvParams.dbg != nullptr): [wg][wave][4] = {total, barrier wait, x staging / vm wait, -} in s_memtime ticks
// TIMING (a compile-time constant in scope wherever these macros are used): true in the instantiations the launch functions pick when GemvParams.dbg is set
// (lnb_profile_kernel_stamps, LNB_GEMV_TIMING), false in production's -- there no clock is read, no stamp is stored, nothing branches on dbg / dbg_full and a
// barrier is one s_barrier: the measurement code is neither executed nor fetched (profiles/prologue_fetch.md)
#define LNB_DBG (TIMING && p.dbg)
#define LNB_DBG_FULL (TIMING && p.dbg_full)
#define TIMED_BARRIER() do { if (LNB_DBG_FULL) { long long tb_ = clock64(); __builtin_amdgcn_s_barrier(); t_wait += clock64() - tb_; } else __builtin_amdgcn_s_barrier(); } while (0)
// phase stamp i (0..7) of this wave, cycles since the kernel started: a second region behind the [4096][8][4] totals (lnb_api.cpp prints the averages)
// (the buffer has eight wave slots per workgroup: a ninth wave -- the packed LM head's -- records nothing instead of writing into the next workgroup's slots)
#define LNB_STAMP(i) do { if (LNB_DBG && lane == 0 && wave < 8) p.dbg[(size_t)4096 * 8 * 4 + ((size_t)blockIdx.x * 8 + wave) * 8 + (i)] = clock64() - t_begin; } while (0)
// ... and stamp 7 = the same interval on the constant-rate wall clock (s_memrealtime; hipDeviceAttributeWallClockRate): the shader clock of THIS launch
// under ITS load = total / wall, which is what turns the cycle counts into microseconds (bench.py: roofline.measured_model)
#define LNB_WALL_EXIT() do { if (LNB_DBG && lane == 0 && wave < 8) p.dbg[(size_t)4096 * 8 * 4 + ((size_t)blockIdx.x * 8 + wave) * 8 + 7] = (long long)wall_clock64() - t_wall0; } while (0)
#define DBG_EXIT() do { if (LNB_DBG && lane == 0 && wave < 8) { long long* d_ = p.dbg + ((size_t)blockIdx.x * 8 + wave) * 4; d_[0] = clock64() - t_begin; d_[1] = t_wait; d_[2] = t_x; d_[3] = t_aux; } LNB_WALL_EXIT(); } while (0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// asm loads are invisible to hipcc's s_waitcnt bookkeeping: the ring below is waited for by hand (wait_ring)
// saddr form: wave-uniform 64-bit base in SGPRs + per-lane 32-bit byte offset -> no per-load VALU address arithmetic
DEVINL void ld_nt_asm(u32x4& dst, unsigned voff, const char* sbase) { asm volatile("global_load_dwordx4 %0, %1, %2 nt ; RING_LOAD" : "=&v"(dst) : "v"(voff), "s"(sbase) : "memory"); }
// the "; RING_RETIRE ..." comment names the registers this wait retires: tools/isa_audit.py checks on the compiled
// code that hipcc touches no ring register between its asm load and the wait that retires it
DEVINL void ld_nt_asm4(unsigned& dst, unsigned voff, const char* sbase) { asm volatile("global_load_dword %0, %1, %2 nt ; RING_LOAD" : "=&v"(dst) : "v"(voff), "s"(sbase) : "memory"); }
// packed source (PK): a stage is three 16-byte loads and one dword per lane
template <int N> DEVINL void wait_ring_pk(u32x4 (&b)[4], unsigned& s) {
    asm volatile("s_waitcnt vmcnt(%4) ; RING_RETIRE %0 %1 %2 %3" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(s) : "n"(N) : "memory");
}
template <int N, int NP> DEVINL void wait_ring(u32x4 (&b)[NP]) {
    static_assert(NP == 1 || NP == 2 || NP == 4 || NP == 8, "loads per stage per helper");
    if constexpr (NP == 1) asm volatile("s_waitcnt vmcnt(%1) ; RING_RETIRE %0" : "+v"(b[0]) : "n"(N) : "memory");
    if constexpr (NP == 2) asm volatile("s_waitcnt vmcnt(%2) ; RING_RETIRE %0 %1" : "+v"(b[0]), "+v"(b[1]) : "n"(N) : "memory");
    if constexpr (NP == 4) asm volatile("s_waitcnt vmcnt(%4) ; RING_RETIRE %0 %1 %2 %3" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) : "n"(N) : "memory");
    if constexpr (NP == 8) asm volatile("s_waitcnt vmcnt(%8) ; RING_RETIRE %0 %1 %2 %3 %4 %5 %6 %7" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]) : "n"(N) : "memory");
}

// PK (two chains only): the helpers stream the 13-bit planar copy of the block (lnb_wpack.h) instead of the raw bf16 -- per lane and stage two 16-byte
// loads of low bytes, one of exponent codes and one dword of signs for 32 weights -- and rebuild the same f32 weights; everything behind the unpack is the raw form's.
// Two instances: gate|up (RW 56, seven helpers, EPI_SILU_MUL: the chains are gate and up of one row) and the LM head (RW 64, eight helpers, EPI_STORE2: the
// chains are rows r and 64 + r of a 128-row block)
template <int RW, int NCH, int SA, int NH, int R, int EPI, bool NORM, int XC, bool PK, bool REPORT = false, bool TIMING = false>
DEVINL void gemv_chain_body(const GemvParams& p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    long long t_begin = LNB_DBG ? clock64() : 0, t_wait = 0, t_x = 0, t_aux = 0;
    const long long t_wall0 = LNB_DBG ? (long long)wall_clock64() : 0;
    constexpr int KC = SA / (NCH * RW * 16);              // 8-wide k chunks per stage
    constexpr int GS = KC / 2;                            // 16-step groups per stage
    constexpr int SB = 2 * SA;                            // f32 product stage
    constexpr int UNITS = SA / 16;                        // 16-byte (8 x bf16) units per stage
    constexpr int NP = UNITS / (64 * NH);                 // 16 B loads per lane per stage per helper
    static_assert(KC >= 2 && (KC & 1) == 0, "bad stage geometry");
    static_assert(UNITS % (64 * NH) == 0 && R * NP <= 60, "vmcnt is a 6-bit counter");
    static_assert(NH >= 2, "x staging is sized for >= 3 stager waves");
    static_assert(!PK || (NCH == 2 && NP == 4 && 2 * NH * 64 == KC * RW), "packed source: one 32-weight group (two (chunk, row) pairs x two chains) per helper lane and stage");
    char* ringB = smem;
    float* xs = (float*)(smem + 2 * SB);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int K = p.K, S = p.S;
    const int m = (S == 1) ? 0 : (int)(blockIdx.x % (unsigned)S);
    const int wg = (S == 1) ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)S);
    const size_t stream_bytes = (size_t)K * NCH * RW * 2;
    const int nstages = (int)((stream_bytes + SA - 1) / SA);
    const int nb_mine = (p.n_blocks - wg + p.n_wg - 1) / p.n_wg;       // row blocks wg, wg+n_wg, ...
    const int T = nb_mine * nstages;                                   // global stage count of this workgroup
    constexpr int NS = 1 + NH;                                         // x stagers: chain wave + helpers
    const int kpad = nstages * KC * 8 + 320;                           // launcher guarantees kpad <= X_CH*NS*512
    const uint16_t* xrow = p.x + (size_t)m * K;

    // wave roles: with more than 3 helpers the chain wave is wave 3 -- waves w and w+4 share a SIMD, so waves 0..2
    // and 4..6 (six helpers) pair up on three SIMDs and the chain wave keeps the fourth one to itself
    constexpr int CW = (NH > 3) ? 3 : 0;
    if (wave != CW) {
        // ================================ helper waves ============================================
        const int hw = wave < CW ? wave : wave - 1;
        u32x4 buf[R][NP];
        unsigned sgn[PK ? R : 1];                                      // PK: buf[j][0..1] low plane, buf[j][2] codes, sgn[j] signs
        {
            uint4 xv[XC], nv[XC];
            x_issue<NORM, NS>(p, xrow, 1 + hw, lane, xv, nv);
            __builtin_amdgcn_s_waitcnt(0x0F70);                        // vmcnt(0): x (and the norm weights) have landed; hipcc needs no
                                                                       // wait of its own in x_store, which would drain the ring below too
        // the weight stream starts only now, BEHIND the x loads in this CU's memory queue (in front of them, or right behind them
        // with a counted wait, it delays x: measured), and the LDS writes of x_store run in its shadow
        // issue cursor: next global stage to load = (block ib, stage is); past the end it re-reads the last stage
        const size_t last16 = stream_bytes - 16;
        // unit of load i:  q = (kc*NCH + c)*RW + r.  One chain: q = (i*NH + hw)*64 + lane.  Two chains (w1|w3): the lane takes BOTH
        // chains of (kc, r) = ((hw*64 + lane) / RW, (hw*64 + lane) % RW) -- load i is chain i -- so that it can leave the
        // products pair-interleaved (gate_k, up_k) for the chain wave's v_pk_add_f32
        static_assert(NCH == 1 || (NCH == 2 && NP % 2 == 0), "two chains: an even number of loads per lane (pairs)");
        unsigned loff[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int pq = ((i >> 1) * NH + hw) * 64 + lane;               // pair index of load i (two chains)
            loff[i] = NCH == 2 ? (unsigned)((((pq / RW) * 2 + (i & 1)) * RW + (pq % RW)) * 16) : (unsigned)(((i * NH + hw) * 64 + lane) * 16);
        }
        int ib = wg, is = 0, issued = 0;
        const unsigned pk_l16 = (unsigned)wpack_plane_off(NH * 64, 0, hw * 64 + lane), pk_l4 = (unsigned)wpack_plane_off(NH * 64, 3, hw * 64 + lane);
        auto issue_next = [&](u32x4 (&dst)[NP], unsigned& sg) {
            if constexpr (PK) {
                // whole stages only (the copy pads a block's last stage with zeros): no clamp
                const char* sb = (const char*)p.wp + ((size_t)ib * nstages + is) * wpack_stage_bytes(NH * 64);     // wave-uniform
                ld_nt_asm(dst[0], pk_l16, sb); ld_nt_asm(dst[1], pk_l16 + NH * 64 * 16, sb); ld_nt_asm(dst[2], pk_l16 + NH * 64 * 32, sb);
                ld_nt_asm4(sg, pk_l4, sb);
                if (issued + 1 < T) { issued++; if (++is == nstages) { is = 0; ib += p.n_wg; } }
                return;
            }
            const size_t soff = (size_t)is * SA;
            const char* sb = (const char*)p.w + (size_t)ib * stream_bytes + soff;     // wave-uniform
            // branch-free clamp (only the last, partial stage of a block ever clamps): one v_min_u32 per load
            const unsigned lim = (soff + SA <= stream_bytes) ? 0xFFFFFFFFu : (unsigned)(last16 - soff);
#pragma unroll
            for (int i = 0; i < NP; i++) ld_nt_asm(dst[i], loff[i] < lim ? loff[i] : lim, sb);
            if (issued + 1 < T) { issued++; if (++is == nstages) { is = 0; ib += p.n_wg; } }
        };
            // norm-fused kernels start the weight stream BEHIND the norm's fold (round 4): issuing R stages per helper into a cold memory
            // pipeline stalls the issuing waves ~3 k cycles -- the waves that fold; behind the fold they only wait for the walker anyway
            // (measured: wq|wk|wv -1.0 us, w1|w3 -2.3 us, output -1 us)
            constexpr bool late = NORM;
            constexpr int EARLY_ = PK ? (EPI == EPI_STORE2 ? LNB_EARLY_HEADP : LNB_EARLY_W13P) : NCH == 2 ? LNB_EARLY_W13 : LNB_EARLY_HEAD;
            constexpr int EARLY = late ? (EARLY_ < R ? EARLY_ : R) : R;      // stages issued in front of the fold
#pragma unroll
            for (int j = 0; j < EARLY; j++) issue_next(buf[j], sgn[PK ? j : 0]);
            x_store<NORM, NS>(p, xs, kpad, 1 + hw, lane, xv);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            TIMED_BARRIER();                                           // B1: xs (or the squares) are in LDS
            if (NORM) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                rms_fold<rms_nf(NH), REPORT, TIMING>(p, xs, ringB, hw - (NH - rms_nf(NH)), lane, t_aux);      // X1, X2 inside; the LAST four helpers fold (waves 4..7 of 8: four SIMDs)
                {                                                      // the walker walks now: the issue stall costs nothing here
#pragma unroll
                    for (int j = EARLY; j < R; j++) issue_next(buf[j], sgn[PK ? j : 0]);
                }
                TIMED_BARRIER();                                       // B2: r published
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if constexpr (NORM) x_normalize<NS>(p, xs, kpad, xs[kpad], 1 + hw, lane, xv, nv);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                TIMED_BARRIER();                                       // B3: xs normalised
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        int st = 0;                                        // stage-in-block of the stage being converted
        for (int it0 = 0; it0 <= T; it0 += R) {
#pragma unroll
            for (int j = 0; j < R; j++) {
                const int t = it0 + j;
                if (t <= T) {
                    if (t < T) {
                        const long long tb_ = LNB_DBG_FULL ? clock64() : 0;
                        if constexpr (PK) wait_ring_pk<(R - 1) * 4>(buf[j], sgn[j]);
                        else wait_ring<(R - 1) * NP, NP>(buf[j]);           // stage t landed; R-1 younger stages stay in flight
                        if (LNB_DBG_FULL) t_x += clock64() - tb_;
                        char* dst = ringB + (t & 1) * SB;
                        const float* xst = xs + (size_t)st * (KC * 8);
                        if constexpr (PK) {
                            // the raw form's two (chunk, row) pairs, their weights rebuilt from the planes: quads 4 pi .. 4 pi + 3 = gate 0-3, gate 4-7, up 0-3, up 4-7
                            const unsigned base4 = p.wp_base4, sg = sgn[j];
#pragma unroll
                            for (int pi = 0; pi < 2; pi++) {
                                const int pq = (pi * NH + hw) * 64 + lane, kc = pq / RW, r = pq % RW;
                                const float4 xa = *(const float4*)(xst + kc * 8), xb = *(const float4*)(xst + kc * 8 + 4);
                                const u32x4 lo = buf[j][pi];
                                const unsigned cg = pi ? buf[j][2].z : buf[j][2].x, cu = pi ? buf[j][2].w : buf[j][2].y;
                                const unsigned hg0 = wpack_hi4(wpack_spread(cg, 0), sg, 4 * pi + 0, base4), hg1 = wpack_hi4(wpack_spread(cg, 1), sg, 4 * pi + 1, base4);
                                const unsigned hu0 = wpack_hi4(wpack_spread(cu, 0), sg, 4 * pi + 2, base4), hu1 = wpack_hi4(wpack_spread(cu, 1), sg, 4 * pi + 3, base4);
#define LNB_WIDE4(h, l) __uint_as_float(wpack_wide<0>(h, l)), __uint_as_float(wpack_wide<1>(h, l)), __uint_as_float(wpack_wide<2>(h, l)), __uint_as_float(wpack_wide<3>(h, l))
                                const float4 ga = mul4(xa, LNB_WIDE4(hg0, lo.x)), gb = mul4(xb, LNB_WIDE4(hg1, lo.y));
                                const float4 ua = mul4(xa, LNB_WIDE4(hu0, lo.z)), ub = mul4(xb, LNB_WIDE4(hu1, lo.w));
#undef LNB_WIDE4
                                char* d = dst + r * 16;
                                *(float4*)(d + ((4 * kc + 0) * RW) * 16) = make_float4(ga.x, ua.x, ga.y, ua.y);
                                *(float4*)(d + ((4 * kc + 1) * RW) * 16) = make_float4(ga.z, ua.z, ga.w, ua.w);
                                *(float4*)(d + ((4 * kc + 2) * RW) * 16) = make_float4(gb.x, ub.x, gb.y, ub.y);
                                *(float4*)(d + ((4 * kc + 3) * RW) * 16) = make_float4(gb.z, ub.z, gb.w, ub.w);
                            }
                        } else if constexpr (NCH == 2) {
                            // both chains of (kc, r): products written pair-interleaved, [k4][half][r] x (gate_s, up_s, gate_s+1, up_s+1)
#pragma unroll
                            for (int pi = 0; pi < NP / 2; pi++) {
                                const int pq = (pi * NH + hw) * 64 + lane, kc = pq / RW, r = pq % RW;
                                const float4 xa = *(const float4*)(xst + kc * 8), xb = *(const float4*)(xst + kc * 8 + 4);
                                const u32x4 vg = buf[j][2 * pi], vu = buf[j][(2 * pi + 1) % NP];
                                const float4 ga = mul4(xa, bf_lo(vg.x), bf_hi(vg.x), bf_lo(vg.y), bf_hi(vg.y)), gb = mul4(xb, bf_lo(vg.z), bf_hi(vg.z), bf_lo(vg.w), bf_hi(vg.w));
                                const float4 ua = mul4(xa, bf_lo(vu.x), bf_hi(vu.x), bf_lo(vu.y), bf_hi(vu.y)), ub = mul4(xb, bf_lo(vu.z), bf_hi(vu.z), bf_lo(vu.w), bf_hi(vu.w));
                                char* d = dst + r * 16;
                                *(float4*)(d + ((4 * kc + 0) * RW) * 16) = make_float4(ga.x, ua.x, ga.y, ua.y);
                                *(float4*)(d + ((4 * kc + 1) * RW) * 16) = make_float4(ga.z, ua.z, ga.w, ua.w);
                                *(float4*)(d + ((4 * kc + 2) * RW) * 16) = make_float4(gb.x, ub.x, gb.y, ub.y);
                                *(float4*)(d + ((4 * kc + 3) * RW) * 16) = make_float4(gb.z, ub.z, gb.w, ub.w);
                            }
                        } else {
                        float4 xa[NP], xb[NP];
#pragma unroll
                        for (int i = 0; i < NP; i++) {
                            const int q = (i * NH + hw) * 64 + lane;       // q = (kc*NCH + c)*RW + r
                            const int kc = q / (NCH * RW);
                            xa[i] = *(const float4*)(xst + kc * 8); xb[i] = *(const float4*)(xst + kc * 8 + 4);
                        }
#pragma unroll
                        for (int i = 0; i < NP; i++) {
                            const int q = (i * NH + hw) * 64 + lane;
                            const int kc = q / (NCH * RW), u = q % (NCH * RW);
                            const u32x4 v = buf[j][i];
                            // exact products (8-bit x 8-bit significands): val1F32 * val2F32, operations_lineartransform.go:60
                            *(float4*)(dst + ((2 * kc) * (NCH * RW) + u) * 16) = mul4(xa[i], bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y));
                            *(float4*)(dst + ((2 * kc + 1) * (NCH * RW) + u) * 16) = mul4(xb[i], bf_lo(v.z), bf_hi(v.z), bf_lo(v.w), bf_hi(v.w));
                        }
                        }
                        if (++st == nstages) st = 0;
                        __builtin_amdgcn_sched_barrier(0);             // refill AFTER the slot has been consumed (no register copies)
                        issue_next(buf[j], sgn[PK ? j : 0]);           // refill this register slot with stage t+R
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // ds_writes complete before the barrier
                    TIMED_BARRIER();
                }
            }
        }
        }
        asm volatile("s_waitcnt vmcnt(0) ; RING_RETIRE_ALL" ::: "memory");
        DBG_EXIT();
        return;
    }
    // ==================================== chain wave ==================================================
    {
        if constexpr (NORM && REPORT) rms_report_park<rms_nf(NH)>(p, ringB, wg == 0 ? m : -1, lane);
        uint4 xv[XC], nv[XC];
        x_issue<NORM, NS>(p, xrow, 0, lane, xv, nv);
        x_store<NORM, NS>(p, xs, kpad, 0, lane, xv);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        TIMED_BARRIER();                                               // B1
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (NORM) {
            const float r = rms_scale_wide<rms_nf(NH), REPORT ? 2 : 0, TIMING>(p, xs, ringB, lane, t_aux);     // X1, X2 inside
            if (lane == 0) xs[kpad] = r;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            TIMED_BARRIER();                                           // B2
            if constexpr (NORM) x_normalize<NS>(p, xs, kpad, r, 0, lane, xv, nv);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            TIMED_BARRIER();                                           // B3
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
    if (LNB_DBG) t_x = clock64() - t_begin;
    LNB_STAMP(6);                                                      // (stamp 6 marks a chain wave: the cycle its main loop starts)
    float acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) acc[c] = 0.0f;
    const int row = (RW & (RW - 1)) == 0 ? (lane & (RW - 1)) : (lane % RW);   // RW 56 / 28: the lanes past RW shadow rows 0.. (every lane stays active: a partially masked wave issues slower)
    int st = 0, blk = wg;
    // every stage is walked in full: beyond K the x values (hence the products) are +0, and acc + 0 == acc
    // because acc is never -0
    for (int it = 0; it <= T; it++) {
        const int t = it - 1;
        if (t >= 0) {
            const char* src = ringB + (t & 1) * SB + row * 16;
            // software pipeline: group g+1's 16 products per chain are in flight while group g is added
            float4 pb[2][NCH][4];
#pragma unroll
            for (int c = 0; c < NCH; c++)
#pragma unroll
                for (int j = 0; j < 4; j++) pb[0][c][j] = *(const float4*)(src + ((j * NCH + c) * RW) * 16);
#pragma unroll
            for (int g = 0; g < GS; g++) {
                const int cur = g & 1, nxt = cur ^ 1;
                if (g + 1 < GS) {
#pragma unroll
                    for (int c = 0; c < NCH; c++)
#pragma unroll
                        for (int j = 0; j < 4; j++) pb[nxt][c][j] = *(const float4*)(src + (((4 * (g + 1) + j) * NCH + c) * RW) * 16);
                }
                __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ABOVE the adds (hipcc otherwise sinks it next to its use)
#pragma unroll
                for (int c = 0; c < NCH; c++) touch16(pb[cur][c][0], pb[cur][c][1], pb[cur][c][2], pb[cur][c][3]);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (NCH == 2) {
                    // pb[cur][half][j] = (gate_s, up_s, gate_s+1, up_s+1): both chains advance with one v_pk_add_f32 per k-step
                    // (6.0 cycles per dependent op against 2 x 4.33; written as separate adds hipcc paired them anyway, behind two
                    // v_mov per step to build the register pairs)
                    f32x2 a2 = {acc[0], acc[1]};
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            const float4 q4 = pb[cur][h][j];
                            a2 = a2 + f32x2{q4.x, q4.y};
                            a2 = a2 + f32x2{q4.z, q4.w};
                        }
                    acc[0] = a2.x; acc[1] = a2.y;
                } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int c = 0; c < NCH; c++) acc[c] = add4(acc[c], pb[cur][c][j]);   // valDstF32 += p, k ascending (:63)
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (++st == nstages) {                                     // end of a row block: write it out, start the next
                if constexpr (EPI == EPI_STORE2) {
                    // the packed LM head: a block is 2 RW rows, chain c of lane r is row blk * 2 RW + c * RW + r
                    static_assert(EPI != EPI_STORE2 || NCH == 2, "the two-row store epilogue needs two chains");
#pragma unroll
                    for (int c = 0; c < NCH; c++) {
                        const int n = blk * (2 * RW) + c * RW + lane;
                        if (lane < RW && n < p.n_rows) p.out[(size_t)m * p.n_rows + n] = bf_trunc(acc[c]);
                    }
                } else
                gemv_epilogue<NCH, EPI>(p, acc, m, blk * RW + lane, (lane < RW) && (blk * RW + lane < p.n_rows));
#pragma unroll
                for (int c = 0; c < NCH; c++) acc[c] = 0.0f;
                st = 0; blk += p.n_wg;
            }
        }
        TIMED_BARRIER();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    DBG_EXIT();
}
// TIMING: the instantiation with the measurement code (stamps, timed barriers and ring waits), launched exactly when GemvParams.dbg is set
template <int RW, int NCH, int SA, int NH, int R, int EPI, bool NORM, int XC = XCh<NORM>::value, bool TIMING = false>
__global__ __launch_bounds__((1 + NH) * 64) void gemv_chain_kernel(GemvParams p) { gemv_chain_body<RW, NCH, SA, NH, R, EPI, NORM, XC, false, false, TIMING>(p); }
template <int RW, int NCH, int SA, int NH, int R, int EPI, bool NORM, int XC = XCh<NORM>::value, bool TIMING = false>
__global__ __launch_bounds__((1 + NH) * 64) void gemv_chain_pk_kernel(GemvParams p) { gemv_chain_body<RW, NCH, SA, NH, R, EPI, NORM, XC, true, false, TIMING>(p); }
// the same two kernels with the norm's report compiled in (GemvParams.norm_out): launched by lnb_op_rmsnorm_sum only
template <int RW, int NCH, int SA, int NH, int R, int EPI, bool NORM, int XC = XCh<NORM>::value>
__global__ __launch_bounds__((1 + NH) * 64) void gemv_chain_report_kernel(GemvParams p) { gemv_chain_body<RW, NCH, SA, NH, R, EPI, NORM, XC, false, true>(p); }
template <int RW, int NCH, int SA, int NH, int R, int EPI, bool NORM, int XC = XCh<NORM>::value>
__global__ __launch_bounds__((1 + NH) * 64) void gemv_chain_pk_report_kernel(GemvParams p) { gemv_chain_body<RW, NCH, SA, NH, R, EPI, NORM, XC, true, true>(p); }

// ------------------------------------------------------------------------------------------------
// gemv_quad_kernel (round 4): the norm-fused thin product wq|wk|wv on ALL CUs, its chains fed through the LDS AND by DPP.
//
// gemv_chain_kernel gives a chain lane its own products (one ds_read_b128 per 4 steps: 8.7-9.0 cycles per step, the returning data
// occupies the SIMD's register write port) and 6144 rows in 32-row blocks fill 192 of the 256 CUs.  A DPP operand serves several
// lanes at once: with quad_perm a row lives in FOUR lanes, lane j of the quad receives the products k = 16g + 4j .. 4j + 3 of a
// 16-step group in one ds_read_b128 and every lane of the quad adds all sixteen in k order,
//     v_add_f32_dpp acc, p_e, acc quad_perm:[j,j,j,j]     e = 0..3 inside j = 0..3,
// i.e. one LDS read per 16 steps and 16 rows per chain wave: 6.8 cycles per step (tools/chainbench3.hip; 7.5 with helpers hammering
// the LDS).  A block is RW = n_rows / 256 rows (24 for the 8B shape): ceil(RW / 16) chain waves, each on its own SIMD.
//   waves 0 .. NCW-1    chain  : rows 16w .. 16w+15 of the block (lanes past the last row shadow earlier ones: every lane stays active);
//   waves NCW .. NCW+NH-1 helper: stream the block's bf16 weights (layout [N/RW][K/8][RW][8], the register ring of gemv_chain_kernel),
//                                  multiply by x and leave the exact f32 products in the LDS as [16-step group][row][4 x 16 B], the
//                                  16-byte slots of a row XOR-swizzled with (row >> 1) & 3 so that both the helpers' ds_write_b128
//                                  (eight consecutive rows of one k-chunk) and the chain waves' ds_read_b128 are conflict-free;
// stages of KS steps in a three-slot ring, one s_barrier per stage, the chain waves two stages behind the helpers so that their
// prefetch (three groups ahead) runs across stage boundaries (as in rowcast_lds_kernel).  The fused RMSNorm prologue is
// gemv_chain_kernel's: the helpers fold, chain wave 0 walks.
// grid.x = S * n_wg, block = (NCW + NH) * 64, dynamic LDS = 3 * RW * KS * 4 + x.
// ------------------------------------------------------------------------------------------------
#define LNB_QP(j) " quad_perm:[" #j "," #j "," #j "," #j "] row_mask:0xf bank_mask:0xf\n\t"
#define LNB_QADD4(j) "v_add_f32_dpp %0, %1, %0" LNB_QP(j) "v_add_f32_dpp %0, %2, %0" LNB_QP(j) "v_add_f32_dpp %0, %3, %0" LNB_QP(j) "v_add_f32_dpp %0, %4, %0" LNB_QP(j)
// the 16 dependent adds of one group in ONE asm statement (separate statements get an s_nop each from hipcc's hazard recognizer);
// the leading s_nop covers the VGPR-write -> DPP-read wait states for whatever was scheduled last
DEVINL void chain16q(float& acc, const float4& q) {
    asm volatile("s_nop 1\n\t" LNB_QADD4(0) LNB_QADD4(1) LNB_QADD4(2) LNB_QADD4(3) : "+v"(acc) : "v"(q.x), "v"(q.y), "v"(q.z), "v"(q.w));
}
template <int RW, int KS, int NH, int R, int EPI, bool NORM, int XC = XCh<NORM>::value, bool TIMING = false>
__global__ __launch_bounds__((gq_ncw(RW) + NH) * 64) void gemv_quad_kernel(GemvParams p) {
#define LNB_QUAD_REPORT false
#include "lnb_gemv_quad_body.h"
#undef LNB_QUAD_REPORT
}
// the same kernel with the norm's report compiled in (GemvParams.norm_out): launched by lnb_op_rmsnorm_sum only
template <int RW, int KS, int NH, int R, int EPI, bool NORM, int XC = XCh<NORM>::value>
__global__ __launch_bounds__((gq_ncw(RW) + NH) * 64) void gemv_quad_report_kernel(GemvParams p) {
    constexpr bool TIMING = false;
#define LNB_QUAD_REPORT true
#include "lnb_gemv_quad_body.h"
#undef LNB_QUAD_REPORT
}

// ------------------------------------------------------------------------------------------------
// Row-broadcast exact GEMV for THIN matrices (wo, w2: 16 output rows per CU are all there is to do).
//
// In gemv_chain_kernel a chain lane receives its products through the LDS: measured on gfx950 a ds_read_b128 occupies the
// wave for ~12.5 cycles, i.e. ~3.1 cycles per k-step on top of the 4.33-cycle dependent add, and the thin kernels are pure
// chain latency (K x ~7.6 cycles).  Here the products never leave the register file:
//   a wave owns 4 output rows, one per DPP row of 16 lanes; lane (q, j) streams the weights of row q with k = j (mod 16)
//   (16 B = eight of them, k ascending, per 128-step chunk), multiplies them by x (exact products) and every lane of the
//   row adds the 16 lanes' products in k order with  v_add_f32_dpp row_newbcast:j  -- a DPP operand costs nothing measurable
//   (8.75 vs 8.63 ticks per dependent add in tools/chainbench2.hip), so a k-step is ~4.33 cycles + ~0.8 of producer work.
// All 16 lanes of a row compute the same sum (same operands, same order); lane j == 0 stores it.
// Four waves (16 rows) per workgroup share x (f32, transposed per chunk in LDS); weights come through the same hand-counted
// register ring as gemv_chain_kernel (RING_LOAD / RING_RETIRE, tools/isa_audit.py).
// grid.x = S * n_wg, block = 256; dynamic LDS = K * 4 bytes.
// ------------------------------------------------------------------------------------------------
constexpr int RC_R = 14;                                    // 1 KiB chunks in flight per wave (56 KiB per CU)
// 16 dependent adds in ONE asm statement: acc += pr(lane 0) ... += pr(lane 15) of this lane's DPP row.  (One statement per add
// made hipcc's hazard recognizer put an s_nop behind every one of them -- it cannot see which operand is the DPP one -- and
// doubled the step time.  Inside the block no further wait states are needed: acc is the plain operand.)
// the 128 dependent adds of one chunk in ONE asm statement: acc += pr[i](lane 0) ... += pr[i](lane 15), i = 0..7.  (Separate
// statements make hipcc's hazard recognizer put an s_nop behind each -- it cannot see which operand is the DPP one.)
// VALU write of pr -> DPP read needs 2 wait states: the leading s_nop covers whatever hipcc scheduled last.
DEVINL void chain128(float& acc, const float (&pr)[8]) {
    asm volatile("s_nop 1\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %1, %0 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %2, %0 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %3, %0 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %4, %0 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %5, %0 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %6, %0 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %7, %0 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %8, %0 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 : "+v"(acc) : "v"(pr[0]), "v"(pr[1]), "v"(pr[2]), "v"(pr[3]), "v"(pr[4]), "v"(pr[5]), "v"(pr[6]), "v"(pr[7]));
}
template <int EPI, bool TIMING = false>
__global__ __launch_bounds__(256) void rowcast_kernel(GemvParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xT = (float*)smem;                                // x[128c + 16i + j] at xT[(c*16 + j)*8 + i]
    const long long t_begin = LNB_DBG ? clock64() : 0;       // LNB_GEMV_TIMING: [wg][wave] = {total, -, prologue, -}
    const long long t_wall0 = LNB_DBG ? (long long)wall_clock64() : 0;
    long long t_x = 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = p.K, S = p.S, nchunks = K >> 7;
    const int m = (S == 1) ? 0 : (int)(blockIdx.x % (unsigned)S);
    const int wg = (S == 1) ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)S);
    const int nb_mine = (p.n_blocks - wg + p.n_wg - 1) / p.n_wg;       // 16-row blocks wg, wg+n_wg, ...
    const int T = nb_mine * nchunks;                                   // chunks this wave walks
    const size_t tile_bytes = (size_t)nchunks * 1024;                  // one wave tile (4 rows)
    const unsigned voff = (unsigned)lane * 16u;
    // x first, all of its loads in flight at once, and the weight stream only once x has landed: queued in front of x -- or
    // even right behind it -- the 14 MB burst of first weight loads delays the x rows that every CU reads (measured both ways)
    constexpr int RC_XU = 8;                                 // 16 B units of x per thread: K <= 16384
    const uint16_t* xrow = p.x + (size_t)m * K;
    uint4 xv[RC_XU];
#pragma unroll
    for (int i = 0; i < RC_XU; i++) {
        const int u = tid + i * 256;
        xv[i] = *(const uint4*)(xrow + (size_t)(u < (K >> 3) ? u : 0) * 8);      // unconditional (clamped) loads
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0): x has landed (hipcc then needs no wait of its own below, which
                                                             // would also drain the weight loads that are issued next)
    u32x4 buf[RC_R];
    // issue cursor: a running wave-uniform pointer (1 KiB per chunk; at the end of a tile jump to this wave's tile of the
    // next block); past the last chunk it stays put and re-reads
    const char* sb = (const char*)p.w + ((size_t)wg * 4 + wave) * tile_bytes;
    const size_t blk_jump = (size_t)p.n_wg * 4 * tile_bytes - tile_bytes;                                  // from the end of a tile
    int ic = 0, issued = 0;
    auto issue_next = [&](u32x4& dst) {
        ld_nt_asm(dst, voff, sb);
        if (issued + 1 < T) { issued++; sb += 1024; if (++ic == nchunks) { ic = 0; sb += blk_jump; } }
    };
#pragma unroll
    for (int j = 0; j < RC_R; j++) issue_next(buf[j]);
#pragma unroll
    for (int i = 0; i < RC_XU; i++) {
        const int u = tid + i * 256;
        if (u < (K >> 3)) {
            const uint4 v = xv[i];
            const int k = u * 8, c = k >> 7, ii = (k & 127) >> 4, j0 = k & 15;
            float* d = xT + ((size_t)(c * 16 + j0) * 8 + ii);
            d[0] = bf_lo(v.x); d[8] = bf_hi(v.x); d[16] = bf_lo(v.y); d[24] = bf_hi(v.y);
            d[32] = bf_lo(v.z); d[40] = bf_hi(v.z); d[48] = bf_lo(v.w); d[56] = bf_hi(v.w);
        }
    }
    __syncthreads();
    if (LNB_DBG) t_x = clock64() - t_begin;
    LNB_STAMP(6);
    if (p.prio) __builtin_amdgcn_s_setprio(3);               // (rung (a) of the FFN ladder: what a prioritised w2 chain keeps beside a co-resident gate|up workgroup)
    const float* xl = xT + (size_t)(lane & 15) * 8;
    float acc = 0.0f;
    float pr[8];
    auto products = [&](float (&d)[8], const u32x4& v, const float4& xa, const float4& xb) {   // exact: 8-bit x 8-bit significands
        const float4 pa = mul4(xa, bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y)), pb = mul4(xb, bf_lo(v.z), bf_hi(v.z), bf_lo(v.w), bf_hi(v.w));
        d[0] = pa.x; d[1] = pa.y; d[2] = pa.z; d[3] = pa.w; d[4] = pb.x; d[5] = pb.y; d[6] = pb.z; d[7] = pb.w;
    };
    int c = 0, blk = wg;
    // the x values of a chunk are read from the LDS one chunk ahead, in the shadow of the previous chunk's 128 adds
    float4 xa = *(const float4*)(xl), xb = *(const float4*)(xl + 4);
    for (int t0 = 0; t0 < T; t0 += RC_R) {
#pragma unroll
        for (int j = 0; j < RC_R; j++) {
            if (t0 + j < T) {
                // chunk t0+j landed; RC_R-1 younger ones stay in flight.  (The wait names buf[j] itself: handing wait_ring a cast
                // reference made hipcc copy the register BEFORE the wait -- caught by tools/isa_audit.py.)
                asm volatile("s_waitcnt vmcnt(%1) ; RING_RETIRE %0" : "+v"(buf[j]) : "n"(RC_R - 1) : "memory");
                products(pr, buf[j], xa, xb);
                // pin the products in front of the refill: otherwise hipcc sinks the unpack/multiply into the chain below, behind
                // the asm that reloads buf[j], and keeps the old value alive through a register copy made BEFORE the wait
                asm volatile("" : "+v"(pr[0]), "+v"(pr[1]), "+v"(pr[2]), "+v"(pr[3]), "+v"(pr[4]), "+v"(pr[5]), "+v"(pr[6]), "+v"(pr[7]));
                issue_next(buf[j]);
                {
                    const int cn = (c + 1 == nchunks) ? 0 : c + 1;     // next chunk of this row (or chunk 0 of the next block's)
                    xa = *(const float4*)(xl + (size_t)cn * 128); xb = *(const float4*)(xl + (size_t)cn * 128 + 4);
                }
                __builtin_amdgcn_sched_barrier(0);                     // the reads are issued HERE, waited for after the chain
                chain128(acc, pr);                                     // valDstF32 += p, k ascending (operations_lineartransform.go:63)
                if (++c == nchunks) {                                  // end of this wave's 4 rows
                    const int n = blk * 16 + wave * 4 + (lane >> 4);
                    if ((lane & 15) == 0 && n < p.n_rows) {
                        const size_t o = (size_t)m * p.n_rows + n;
                        if (EPI == EPI_RESID) p.out[o] = bf_trunc(bf_wide(p.res[o]) + bf_wide(bf_trunc(acc)));   // ml.Add, operations_impl.go:320-332
                        else p.out[o] = bf_trunc(acc);
                    }
                    acc = 0.0f; c = 0; blk += p.n_wg;
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0) ; RING_RETIRE_ALL" ::: "memory");
    if (LNB_DBG && lane == 0) { long long* d_ = p.dbg + ((size_t)blockIdx.x * 8 + wave) * 4; d_[0] = clock64() - t_begin; d_[1] = 0; d_[2] = t_x; d_[3] = t_x; }
    LNB_WALL_EXIT();
}

// ------------------------------------------------------------------------------------------------
// rowcast_lds_kernel (round 4): the row-broadcast chain with its PRODUCER work moved to a second wave.
//
// tools/chainbench3.hip: a dependent v_add_f32_dpp row_newbcast costs 5.3 cycles when nothing else is issued between the adds,
// and whatever the chain wave issues besides them is paid in full (a wave issues one instruction per ~4.4 cycles): rowcast_kernel's
// chain wave also unpacks and multiplies its weights, reads x and refills its register ring -- 6.2-6.6 cycles per step.  Every
// way of handing a lane its OWN operand per step is worse (ds_read_b128 per 4 steps: 9.0 cycles per step with 64, 32 or 16 lanes
// active -- the returning data occupies the SIMD's register write port like four VALU ops; products made by the matrix pipe with a
// one-hot selector operand: 7.5), but a DPP operand serves 16 lanes, so here one ds_read_b128 feeds 64 steps: 5.56 measured.
//   waves 0..3  chain : 4 rows each, one per DPP row; per 128-step chunk two ds_read_b128 (the next chunk's products) + 128 adds;
//   waves 4..7  helper: wave 4+c streams the weights of chain wave c (same lane mapping as rowcast_kernel: lane (q, j) holds the
//                       eight weights of row q with k = j mod 16), multiplies them by x (exact products) and leaves them in a
//                       lane-private LDS ring -- wave w and w+4 share a SIMD, the helper is the younger wave there and only takes
//                       the issue slots the chain's DPP latency leaves free (NOTES.md 5.8: 5.3 cycles per step beside a younger
//                       vector-heavy wave);
// stages of RL_SC chunks in a three-slot ring, one s_barrier per stage: at iteration t the helpers write stage t while the chain
// waves add stage t-2 and prefetch the first chunk of stage t-1 (complete since the previous barrier), so no LDS round trip is
// exposed at a stage boundary.  x lives in the LDS as raw bf16 (K * 2 bytes), transposed per chunk like the weights.
// Same weight layout as rowcast_kernel (tag RW 4); requires K % (128 * RL_SC) == 0 and at least two stages (the launcher falls back otherwise).
// grid.x = S * n_wg, block = 512, dynamic LDS = rl_lds_bytes(K).
// ------------------------------------------------------------------------------------------------
constexpr int RL_SC = 4;                                    // 128-step chunks per stage
constexpr int RL_SLOTS = 3;
constexpr int RL_R = 12;                                    // 1 KiB weight chunks in flight per helper wave (a multiple of RL_SC * RL_SLOTS' unroll)
constexpr int RL_STAGE = 4 * RL_SC * 2048;                  // bytes of products per stage: 4 pairs x RL_SC chunks x 2 KiB
__host__ __device__ constexpr size_t rl_lds_bytes(int K) { return (size_t)RL_SLOTS * RL_STAGE + (size_t)K * 2; }
template <int EPI, bool TIMING = false>
__global__ __launch_bounds__(512) void rowcast_lds_kernel(GemvParams p) {
    static_assert(RL_R == RL_SC * RL_SLOTS, "the helper's ring index and the product slot are static inside a three-stage unroll");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;
    uint16_t* xb = (uint16_t*)(smem + RL_SLOTS * RL_STAGE);  // x[128c + 16i + j] at xb[(c*16 + j)*8 + i]
    const long long t_begin = LNB_DBG ? clock64() : 0;       // LNB_GEMV_TIMING: [wg][wave] = {total, barrier wait, x staged, chain start (chain waves)}
    const long long t_wall0 = LNB_DBG ? (long long)wall_clock64() : 0;
    long long t_x = 0, t_wait = 0, t_chain = 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), pair = wave & 3;
    const int K = p.K, S = p.S, nchunks = K >> 7, nst = nchunks / RL_SC;
    const int m = (S == 1) ? 0 : (int)(blockIdx.x % (unsigned)S);
    const int wg = (S == 1) ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)S);
    const int nb_mine = (p.n_blocks - wg + p.n_wg - 1) / p.n_wg;       // 16-row blocks wg, wg+n_wg, ...
    const int NS = nb_mine * nst;                                      // stages this workgroup walks
    // x first, all of its loads in flight at once; the weight stream starts once x has landed (NOTES.md 5.1)
    constexpr int RL_XU = 4;                                 // 16 B units of x per thread: K <= 16384
    const uint16_t* xrow = p.x + (size_t)m * K;
    uint4 xv[RL_XU];
#pragma unroll
    for (int i = 0; i < RL_XU; i++) {
        const int u = tid + i * 512;
        xv[i] = *(const uint4*)(xrow + (size_t)(u < (K >> 3) ? u : 0) * 8);      // unconditional (clamped) loads
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0): hipcc then needs no wait of its own below (it would drain the weight ring too)
    u32x4 buf[RL_R];
    const size_t tile_bytes = (size_t)nchunks * 1024;        // one wave tile (4 rows)
    const char* sb = (const char*)p.w + ((size_t)wg * 4 + pair) * tile_bytes;
    const size_t blk_jump = (size_t)p.n_wg * 4 * tile_bytes - tile_bytes;
    const unsigned voff = (unsigned)lane * 16u;
    const int T = NS * RL_SC;
    int ic = 0, issued = 0;
    auto stage_x = [&]() {
#pragma unroll
        for (int i = 0; i < RL_XU; i++) {
            const int u = tid + i * 512;
            if (u < (K >> 3)) {
                const uint4 v = xv[i];
                const int k = u * 8, c = k >> 7, ii = (k & 127) >> 4, j0 = k & 15;
                uint16_t* d = xb + ((size_t)(c * 16 + j0) * 8 + ii);
                d[0] = (uint16_t)v.x; d[8] = (uint16_t)(v.x >> 16); d[16] = (uint16_t)v.y; d[24] = (uint16_t)(v.y >> 16);
                d[32] = (uint16_t)v.z; d[40] = (uint16_t)(v.z >> 16); d[48] = (uint16_t)v.w; d[56] = (uint16_t)(v.w >> 16);
            }
        }
        __syncthreads();
        if (LNB_DBG) t_x = clock64() - t_begin;
    };
#define RL_BARRIER() do { if (LNB_DBG_FULL) { const long long tb_ = clock64(); __builtin_amdgcn_s_barrier(); t_wait += clock64() - tb_; } else __builtin_amdgcn_s_barrier(); } while (0)
    // Schedule (iterations it = 0 .. NS, one s_barrier each).  Iteration 0 fills the ring from BOTH sides: the helper makes stage 0, the
    // chain wave -- idle until there is something to add -- makes stage 1 from four weight loads of its own (otherwise it sits through
    // two helper stages, ~4 k cycles per launch measured).  From then on: iteration it, the helper writes stage it+1 (slot (it+1) % 3),
    // the chain wave adds stage it-1 (slot (it-1) % 3) and prefetches the first chunk of stage it (complete since the previous barrier),
    // so no LDS round trip is exposed at a stage boundary.
    auto products = [&](float4& pa, float4& pb, const u32x4& b, const uint4& xq) {      // exact: 8-bit x 8-bit significands (operations_lineartransform.go:60)
        pa = mul4(make_float4(bf_lo(xq.x), bf_hi(xq.x), bf_lo(xq.y), bf_hi(xq.y)), bf_lo(b.x), bf_hi(b.x), bf_lo(b.y), bf_hi(b.y));
        pb = mul4(make_float4(bf_lo(xq.z), bf_hi(xq.z), bf_lo(xq.w), bf_hi(xq.w)), bf_lo(b.z), bf_hi(b.z), bf_lo(b.w), bf_hi(b.w));
    };
    const char* xl = (const char*)xb + (size_t)(lane & 15) * 16;
    if (wave >= 4) {
        // ================================ helper: stage 0, then stages 2, 3, ... of chain wave `pair` ===================
        // (the two roles are separate straight-line paths from here on: tools/isa_audit.py follows each role's ring registers on its own path)
        const int Th = T - RL_SC;                            // loads of this wave: every chunk but the four of stage 1
        auto advance = [&]() { sb += 1024; if (++ic == nchunks) { ic = 0; sb += blk_jump; } };
        auto issue_h = [&](u32x4& dst) {
            ld_nt_asm(dst, voff, sb);
            if (issued + 1 < Th) { issued++; advance(); if (issued == RL_SC) { for (int j = 0; j < RL_SC; j++) advance(); } }   // past the last chunk: stays put, re-reads
        };
        // the first stage's loads in front of the x scatter, the rest of the ring behind it: twelve loads per wave issued into the cold
        // memory pipeline stall the issuing wave, and with it the scatter every wave waits for (prologue 2.9 k -> 4.4 k cycles measured)
#pragma unroll
        for (int j = 0; j < RL_SC; j++) issue_h(buf[j]);
        stage_x();
#pragma unroll
        for (int j = RL_SC; j < RL_R; j++) issue_h(buf[j]);
        char* const dst0 = ring + (size_t)pair * (RL_SC * 2048) + (size_t)lane * 16;
        int c = 0;
        for (int it0 = 0; it0 <= NS; it0 += RL_SLOTS) {
#pragma unroll
            for (int u = 0; u < RL_SLOTS; u++) {
                const int it = it0 + u;
                if (it <= NS) {
                    if (it == 0 || it + 1 < NS) {
                        char* dst = dst0 + (size_t)(it == 0 ? 0 : (u + 1) % RL_SLOTS) * RL_STAGE;
#pragma unroll
                        for (int cc = 0; cc < RL_SC; cc++) {
                            u32x4& b = buf[u * RL_SC + cc];
                            asm volatile("s_waitcnt vmcnt(%1) ; RING_RETIRE %0" : "+v"(b) : "n"(RL_R - 1) : "memory");
                            const uint4 xq = *(const uint4*)(xl + (size_t)c * 256);
                            float4 pa, pb;
                            products(pa, pb, b, xq);
                            // pin the products in front of the refill (else hipcc sinks the unpack behind the asm that reloads b)
                            asm volatile("" : "+v"(pa.x), "+v"(pa.y), "+v"(pa.z), "+v"(pa.w), "+v"(pb.x), "+v"(pb.y), "+v"(pb.z), "+v"(pb.w));
                            issue_h(b);
                            *(float4*)(dst + cc * 2048) = pa; *(float4*)(dst + cc * 2048 + 1024) = pb;
                            if (++c == nchunks) c = 0;
                        }
                        if (it == 0) c = (2 * RL_SC) % nchunks;            // stage 1 is the chain wave's
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // ds_writes complete before the barrier
                    RL_BARRIER();
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0) ; RING_RETIRE_ALL" ::: "memory");
    } else {
        // ================================ chain wave: 4 rows, one per DPP row =========================================
        u32x4 cb[RL_SC];
#pragma unroll
        for (int j = 0; j < RL_SC; j++) ld_nt_asm(cb[j], voff, sb + (size_t)(RL_SC + j) * 1024);      // stage 1: chunks 4 .. 7 of this wave's first tile (K >= 1024)
        stage_x();
        const char* const src0 = ring + (size_t)pair * (RL_SC * 2048) + (size_t)lane * 16;
        {   // iteration 0: stage 1 into slot 1
            char* dst = ring + (size_t)pair * (RL_SC * 2048) + (size_t)lane * 16 + (size_t)1 * RL_STAGE;
#pragma unroll
            for (int cc = 0; cc < RL_SC; cc++) {
                if (cc == 0) asm volatile("s_waitcnt vmcnt(3) ; RING_RETIRE %0" : "+v"(cb[0]) :: "memory");
                if (cc == 1) asm volatile("s_waitcnt vmcnt(2) ; RING_RETIRE %0" : "+v"(cb[1]) :: "memory");
                if (cc == 2) asm volatile("s_waitcnt vmcnt(1) ; RING_RETIRE %0" : "+v"(cb[2]) :: "memory");
                if (cc == 3) asm volatile("s_waitcnt vmcnt(0) ; RING_RETIRE %0" : "+v"(cb[3]) :: "memory");
                const uint4 xq = *(const uint4*)(xl + (size_t)(RL_SC + cc) * 256);
                float4 pa, pb;
                products(pa, pb, cb[cc], xq);
                *(float4*)(dst + cc * 2048) = pa; *(float4*)(dst + cc * 2048 + 1024) = pb;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            RL_BARRIER();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        __builtin_amdgcn_s_setprio(3);
        if (LNB_DBG) { t_chain = clock64() - t_begin; t_wait = 0; }         // (chain waves report the barrier wait of the main loop only)
        LNB_STAMP(6);
        float acc = 0.0f;
        float4 ba[2], bb[2];                                 // products of the chunk being added / of the next one
        ba[0] = *(const float4*)src0; bb[0] = *(const float4*)(src0 + 1024);     // stage 0, chunk 0
        int sdone = 0, blk = wg;
        for (int it0 = 0; it0 <= NS; it0 += RL_SLOTS) {
#pragma unroll
            for (int u = 0; u < RL_SLOTS; u++) {
                const int it = it0 + u;
                if (it >= 1 && it <= NS) {
                    // stage it-1 lives in slot (u+2) % 3, stage it (complete since the last barrier) in slot u
                    const char* cur = src0 + (size_t)((u + 2) % RL_SLOTS) * RL_STAGE;
                    const char* nxt = src0 + (size_t)u * RL_STAGE;
#pragma unroll
                    for (int cc = 0; cc < RL_SC; cc++) {
                        const char* q = cc + 1 < RL_SC ? cur + (cc + 1) * 2048 : nxt;      // past the last stage: stale bytes, never added
                        ba[(cc + 1) & 1] = *(const float4*)q; bb[(cc + 1) & 1] = *(const float4*)(q + 1024);
                        __builtin_amdgcn_sched_barrier(0);         // the reads are issued HERE, in front of the chunk's 128 adds
                        const float4 a = ba[cc & 1], b = bb[cc & 1];
                        const float pr[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                        chain128(acc, pr);                         // valDstF32 += p, k ascending (operations_lineartransform.go:63)
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (++sdone == nst) {                          // end of this wave's 4 rows
                        const int n = blk * 16 + pair * 4 + (lane >> 4);
                        if ((lane & 15) == 0 && n < p.n_rows) {
                            const size_t o = (size_t)m * p.n_rows + n;
                            if (EPI == EPI_RESID) p.out[o] = bf_trunc(bf_wide(p.res[o]) + bf_wide(bf_trunc(acc)));   // ml.Add, operations_impl.go:320-332
                            else p.out[o] = bf_trunc(acc);
                        }
                        acc = 0.0f; sdone = 0; blk += p.n_wg;
                    }
                    RL_BARRIER();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                }
            }
        }
    }
#undef RL_BARRIER
    if (LNB_DBG && lane == 0) { long long* d_ = p.dbg + ((size_t)blockIdx.x * 8 + wave) * 4; d_[0] = clock64() - t_begin; d_[1] = t_wait; d_[2] = t_x; d_[3] = t_chain; }
    LNB_WALL_EXIT();
}

// ------------------------------------------------------------------------------------------------
// Prefill (S >= 16 rows per call): the same exact chains on the f32 MATRIX cores.
//
// v_mfma_f32_16x16x4_f32 is, bit for bit, the k-ordered chain  D = fma(a_k3,b_k3, fma(a_k2,b_k2, fma(a_k1,b_k1, fma(a_k0,b_k0, C))))
// (one rounding per product, no wider internal accumulation; verified against the reference's loop on MI355X by
// tools/mfma_exact.hip), and bf16 x bf16 products are exact, so fma == the reference's multiply-then-add.  One instruction
// advances 16 output rows x 16 batch rows by four k-steps in 32 cycles: ~20x the chain throughput of the S = 1 kernels,
// with identical bits.  (It does not help decode: one batch column uses 1/16 of the instruction, 10 cycles per k-step.)
//
// rmsnorm_rows_kernel: RMSNorm of S rows, one wave per row (the rows are the parallelism here; each wave walks its row's
// sequential sum of squares out of the LDS), output bf16 [S][K] with the reference's two truncations.
// gemm_mfma_kernel: workgroup = 4 waves = 64 output rows x 128 batch rows; K is walked in 128-step slabs staged through the
// LDS as f32, k-major and padded so that both operand fragments are bank-conflict free:
//   A (weights): lane (i = l&15, kk = l>>4) reads As[4g+kk][16w+i];  B (x): Bs[4g+kk][16t+j]   (row strides 80 / 144 floats)
// wave w owns n-tile w and all 8 m-tiles: 8 (16 for the two-chain w1|w3) MFMAs per 1-2 A reads + 8 B reads.
// Weights are gathered 16 B at a time from whichever tiled layout the matrix was stored in (tiled_index).
// grid = (ceil(n_rows/64), ceil(S/128)); dynamic LDS = (NCH*128*80 + 128*144) * 4 bytes.
// ------------------------------------------------------------------------------------------------
template <bool REPORT>                                    // REPORT: lnb_op_rmsnorm_sum's instantiation (norm_out: [S][3] words); production launches <false> with null
__global__ __launch_bounds__(64) void rmsnorm_rows_kernel(const uint16_t* x, const uint16_t* w, uint16_t* out, int S, int K, float eps, uint32_t* norm_out) {
    // one wave per row: the row's squares go to the LDS with coalesced loads, every lane then walks the SAME sequential sum
    // (broadcast float4 reads, the next 16 values in flight behind 16 adds), and the lanes share the normalisation
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sq = (float*)smem;                                // K (+32 zero pad) f32
    const int m = blockIdx.x, lane = threadIdx.x;
    const uint16_t* xr = x + (size_t)m * K;
    for (int k = lane * 8; k < K + 32; k += 512) {           // Pow(x,2): exact in f32 (impl:197-217)
        uint4 v = make_uint4(0, 0, 0, 0);
        if (k < K) v = *(const uint4*)(xr + k);
        const float a0 = bf_lo(v.x), a1 = bf_hi(v.x), a2 = bf_lo(v.y), a3 = bf_hi(v.y), a4 = bf_lo(v.z), a5 = bf_hi(v.z), a6 = bf_lo(v.w), a7 = bf_hi(v.w);
        if (k < K + 32) { *(float4*)(sq + k) = make_float4(a0 * a0, a1 * a1, a2 * a2, a3 * a3); *(float4*)(sq + k + 4) = make_float4(a4 * a4, a5 * a5, a6 * a6, a7 * a7); }
    }
    __syncthreads();
    float sum = 0.0f;                                        // Mean's serial f32 sum, k ascending (impl:236-251); + 0.0 past K changes nothing
    float4 a0 = *(const float4*)(sq), a1 = *(const float4*)(sq + 4), a2 = *(const float4*)(sq + 8), a3 = *(const float4*)(sq + 12);
    for (int k0 = 0; k0 < K; k0 += 32) {
        const float4 b0 = *(const float4*)(sq + k0 + 16), b1 = *(const float4*)(sq + k0 + 20), b2 = *(const float4*)(sq + k0 + 24), b3 = *(const float4*)(sq + k0 + 28);
        __builtin_amdgcn_sched_barrier(0);
        touch16(a0, a1, a2, a3);
        __builtin_amdgcn_sched_barrier(0);
        sum = add4(sum, a0); sum = add4(sum, a1); sum = add4(sum, a2); sum = add4(sum, a3);
        __builtin_amdgcn_sched_barrier(0);
        if (k0 + 32 < K) { a0 = *(const float4*)(sq + k0 + 32); a1 = *(const float4*)(sq + k0 + 36); a2 = *(const float4*)(sq + k0 + 40); a3 = *(const float4*)(sq + k0 + 44); }
        __builtin_amdgcn_sched_barrier(0);
        touch16(b0, b1, b2, b3);
        __builtin_amdgcn_sched_barrier(0);
        if (k0 + 16 < K) { sum = add4(sum, b0); sum = add4(sum, b1); sum = add4(sum, b2); sum = add4(sum, b3); }
        __builtin_amdgcn_sched_barrier(0);
    }
    float mean = __fdiv_rn(sum, (float)K);
    mean = mean + eps;
    const float r = (float)(1.0 / sqrt((double)mean));
    if (REPORT && norm_out && lane == 0) { uint32_t* no = norm_out + (size_t)m * 3; no[0] = __float_as_uint(sum); no[1] = __float_as_uint(r); no[2] = RMS_PATH_SERIAL; }   // (lnb_op_rmsnorm_sum; nullptr in production)
    uint16_t* o = out + (size_t)m * K;
    for (int k = lane * 8; k < K; k += 512) {                // trunc(trunc(x*r)*w) (llamatransformer.go:656,638)
        const uint4 v = *(const uint4*)(xr + k), g = *(const uint4*)(w + k);
        const uint32_t xs_[4] = {v.x, v.y, v.z, v.w}, ws_[4] = {g.x, g.y, g.z, g.w};
        uint32_t r4[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint16_t lo = bf_trunc(bf_wide(bf_trunc(bf_lo(xs_[e]) * r)) * bf_lo(ws_[e]));
            const uint16_t hi = bf_trunc(bf_wide(bf_trunc(bf_hi(xs_[e]) * r)) * bf_hi(ws_[e]));
            r4[e] = (uint32_t)lo | ((uint32_t)hi << 16);
        }
        *(uint4*)(o + k) = make_uint4(r4[0], r4[1], r4[2], r4[3]);
    }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int GM_NB = 64, GM_KS = 128;
constexpr unsigned GM_MB64_UPTO = 0xFFFFFFFFu;              // 64-row batch tiles up to this many 64x128 tiles: always -- tools/gemmbench.hip, S = 256..2048:
                                                            // 64 x 64 tiles are 2-28 % faster than 64 x 128 everywhere (more workgroups per CU to overlap staging)
template <int EPI> DEVINL void gemm_epilogue4(const GemmParams& p, const f32x4& g, const f32x4& u, int m, int n0) {
    // one lane: batch row m, four consecutive output rows n0..n0+3 (n0 % 4 == 0)
    if (m >= p.S) return;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int n = n0 + r;
        if (n >= p.n_rows) continue;
        const size_t o = (size_t)m * p.n_rows + n;
        if (EPI == EPI_STORE) p.out[o] = bf_trunc(g[r]);
        else if (EPI == EPI_RESID) p.out[o] = bf_trunc(bf_wide(p.res[o]) + bf_wide(bf_trunc(g[r])));            // ml.Add, impl:320-332
        else if (EPI == EPI_SILU_MUL) {                                                                           // activations.go:36-39, :614
            const uint16_t gs = bf_trunc(p.silu[bf_trunc(g[r])]);
            const uint16_t y = bf_trunc(bf_wide(gs) * bf_wide(bf_trunc(u[r])));
            if (p.out_xt) p.out_xt[xt_group(m, p.n_rows) + xt_index(m & 15, n)] = y;       // the next product reads column groups (mfma_pair_kernel)
            else p.out[o] = y;
        } else if (EPI == EPI_QKV_ROPE) {                                                                         // llamatransformer.go:297-403
            // rows of one sequence: consecutive positions of its cache; rows of a batch (btab): row m is sequence m's one new token
            const int pos = p.btab ? p.btab->st[m]->pos : p.st->pos + m;
            const int seq_len = p.btab ? p.btab->seq_len[m] : p.seq_len;
            uint16_t* const cache_k = p.btab ? p.bkv->ck[m] : p.cache_k;
            uint16_t* const cache_v = p.btab ? p.bkv->cv[m] : p.cache_v;
            const uint16_t mine = bf_trunc(g[r]), other = bf_trunc(g[r ^ 1]);                                      // RoPE partner 2i <-> 2i+1: same lane
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
                    cache_k[(((size_t)kh * (p.head_dim >> 3) + (d >> 3)) * seq_len + pos) * 8 + (d & 7)] = r16;
                }
            } else cache_v[(size_t)pos * p.kv_dim + (n - p.q_dim - p.kv_dim)] = mine;
        }
    }
}

// WN = waves along n: 4 -> the workgroup owns 64 output rows, every wave all 8 m-tiles; 1 -> the workgroup owns 16 output rows and
// its four waves split the 8 m-tiles (4x the workgroups for thin matrices at small S, where 64-row tiles fill a quarter of the CUs)
// LDS operand tiles of gemm_mfma_kernel, as raw bf16 in per-lane STREAMS: the MFMA lane (i = l&15, kk = l>>4) of k-group g consumes
// k = 4g + kk, so everything that lane will read during a 128-step slab is laid out contiguously for it:
//   A (weights): stream (chain c, n-tile w, kk, i) = its 32 values, g ascending (64 B + 16 B pad): 4 ds_read_b128 per slab;
//   B (x):       stream (kk, i) = [g/2][m-tile t][g&1] (512 B + 16 B pad): one ds_read_b128 = four m-tiles of two k-groups.
// (An f32 k-major tile cost nine ds_reads per eight MFMAs and an LDS round trip in front of every pair; raw bf16 halves the LDS,
// two workgroups fit a CU, and a staged 16 B unit -- 8 consecutive k = two k-groups -- lands as four packed words.)
constexpr int GM_APAD = 80;                                 // stream strides in bytes: conflict-free 16 B reads across 16 lanes
// The one-chain 64-row tiles (WN 4, NCH 1) keep x in the LDS as f32 (bf16 << 16, converted once per element while staging): the B
// operand -- each value feeds ONE MFMA there -- then needs no widening op between matrix instructions (+6 % at S = 512).  The
// two-chain w1|w3 kernel uses every B value twice and is faster with the compact tile (two workgroups per CU at 64 x 128); the
// 16-row tiles (WN 1) keep raw bf16 pairs too.
__host__ __device__ constexpr bool gemm_bf32(int NCH, int WN) { return WN == 4 && NCH == 1; }
__host__ __device__ constexpr int gemm_bpad(int MB, bool f32 = false) { return (f32 ? 32 : 16) * (MB / 16) * 4 + 16; }   // stream bytes (+ pad)
__host__ __device__ constexpr size_t gemm_lds_a(int NCH, int WN) { return (size_t)NCH * WN * 64 * GM_APAD; }
__host__ __device__ constexpr size_t gemm_lds_bytes(int NCH, int WN, int MB = 128) { return gemm_lds_a(NCH, WN) + (size_t)64 * gemm_bpad(MB, gemm_bf32(NCH, WN)); }

#ifndef GM_DBG
#define GM_DBG 0                                            // tools/gemmbench.hip: 1 = stage only the first slab, 2 = no barriers, 4 = no LDS reads
#endif
// MB = batch rows per workgroup: 128, or 64 (WN = 4 only) when 128-row tiles would put at most one workgroup on a CU
template <int EPI, int NCH, int WN, int MB = 128>
__global__ __launch_bounds__(256) void gemm_mfma_kernel(GemmParams p) {
    static_assert(MB == 128 || (MB == 64 && WN == 4), "batch tile");
    constexpr bool BF32 = gemm_bf32(NCH, WN);                // x tile as f32: stream (kk, i) = [g][m-tile t]
    constexpr int GM_MB = MB, GM_BPAD = gemm_bpad(MB, BF32), TB = MB / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;                                         // streams [(c*WN + w)*4 + kk][i] of GM_APAD bytes
    char* Bs = smem + gemm_lds_a(NCH, WN);                   // streams [kk][i] of GM_BPAD bytes
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NB = 16 * WN, MT = WN == 4 ? TB : 2;      // output rows per workgroup, m-tiles per wave
    const int n0 = blockIdx.x * NB, m0 = blockIdx.y * GM_MB;
    const int nt_off = WN == 4 ? wave * 16 : 0, mt0 = WN == 4 ? 0 : wave * 2;
    const int K = p.K;
    f32x4 acc[NCH][MT];
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int t = 0; t < MT; t++) acc[c][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fi = lane & 15, fk = lane >> 4;
    // staging registers: the NEXT slab's 16 B units are loaded before the current slab's MFMAs and written to the LDS after them
    // (a load-use loop paid one memory round trip per unit).  Unit q of a thread: weights = row tid % NB, unit kc = tid / NB + q*256/NB
    // of the slab; x = batch row tid % 128, unit tid / 128 + 2q.  Their addresses are a per-thread base + uniform strides (both tiled
    // layouts are affine in the slab, unit and chain index), so a full slab is staged without a compare, a select or a divergent
    // branch; only the last slab of a K that is not a multiple of 128 takes the checked path.
    constexpr int WU = NB * (GM_KS / 8) / 256, XU = GM_MB * (GM_KS / 8) / 256, WQ = 256 / NB, XQ = 256 / GM_MB;   // 4 (or 1) and 8 (4) units per thread
    uint4 wreg[NCH][WU], xreg[XU];
    const bool rw4 = p.rw == 4;                              // row-broadcast layout: a 16 B unit holds k0 + 16e + kc, e = 0..7
    const int kst = rw4 ? 16 : 1;                            // k stride inside a 16 B weight unit
    const int wrow = tid & (NB - 1), wkc = tid / NB, xrow = tid & (GM_MB - 1), xkc = tid / GM_MB;
    int wn = n0 + wrow; wn = wn < p.n_rows ? wn : p.n_rows - 1;                             // clamped rows are computed and dropped
    int xm = m0 + xrow; xm = xm < p.S ? xm : p.S - 1;
    const uint16_t* wp = p.w + tiled_index(wn, rw4 ? wkc : 8 * wkc, 0, K, p.rw, p.nch);     // slab 0, unit q = 0, chain 0
    const uint16_t* xp = p.x + (size_t)xm * K + 8 * xkc;
    const size_t w_slab = rw4 ? (size_t)512 : (size_t)16 * p.nch * p.rw * 8;                // elements per 128 k
    const size_t w_unit = rw4 ? (size_t)WQ * 8 : (size_t)WQ * p.nch * p.rw * 8;             // ... per unit step q
    const size_t w_chain = (size_t)p.rw * 8;                                                // ... per chain (chain layouts only)
    auto issue = [&](int k0) {
        if (k0 + GM_KS <= K) {                               // full slab (uniform branch)
#pragma unroll
            for (int c = 0; c < NCH; c++)
#pragma unroll
                for (int q = 0; q < WU; q++) wreg[c][q] = *(const uint4*)(wp + c * w_chain + q * w_unit);
#pragma unroll
            for (int q = 0; q < XU; q++) xreg[q] = *(const uint4*)(xp + 8 * XQ * q);
            wp += w_slab; xp += GM_KS;
            return;
        }
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int q = 0; q < WU; q++) {
                const int kc = wkc + q * WQ;
                int kf = rw4 ? k0 + kc : k0 + 8 * kc;
                kf = kf + 7 * kst < K ? kf : 0;              // (zeroed past K in commit: no use here, or the load would be waited for at once)
                wreg[c][q] = *(const uint4*)(p.w + tiled_index(wn, kf, c, K, p.rw, p.nch));
            }
#pragma unroll
        for (int q = 0; q < XU; q++) {
            int kf = k0 + 8 * (xkc + XQ * q);
            kf = kf < K ? kf : 0;
            xreg[q] = *(const uint4*)(p.x + (size_t)xm * K + kf);
        }
    };
    // a unit of 8 consecutive k = k-groups 2kc (elements 0..3) and 2kc+1 (4..7): lane-stream kk gets the word (e[kk] | e[4+kk] << 16)
    auto pack4 = [](const uint4& v, uint32_t (&w)[4]) {
        w[0] = (v.x & 0xFFFFu) | (v.z << 16); w[1] = (v.x >> 16) | (v.z & 0xFFFF0000u);
        w[2] = (v.y & 0xFFFFu) | (v.w << 16); w[3] = (v.y >> 16) | (v.w & 0xFFFF0000u);
    };
    char* const wblk = As + (size_t)((wrow >> 4) * 4) * 16 * GM_APAD + (size_t)(wrow & 15) * GM_APAD;   // (+ c*WN*64*GM_APAD per chain)
    char* const xblk = Bs + (size_t)(xrow & 15) * GM_BPAD + ((BF32 ? 2 : 1) * xkc * TB + (xrow >> 4)) * 4;
    auto commit = [&](int k0) {                              // raw bf16, no conversion (beyond K: zeros)
        const bool full = k0 + GM_KS <= K;
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int q = 0; q < WU; q++) {
                const int kc = wkc + q * WQ;
                uint4 v = wreg[c][q];
                if (!full && !((rw4 ? k0 + kc : k0 + 8 * kc) + 7 * kst < K)) v = make_uint4(0, 0, 0, 0);
                char* blk = wblk + (size_t)c * WN * 64 * GM_APAD;
                if (rw4) {                                   // element e -> k = 16e + kc: k-group 4e + kc/4, stream kc&3
                    char* d = blk + (size_t)(kc & 3) * 16 * GM_APAD + (kc >> 2) * 2;
                    const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 8; e++) *(uint16_t*)(d + e * 8) = (uint16_t)(wd[e >> 1] >> ((e & 1) * 16));
                } else {
                    uint32_t w4[4]; pack4(v, w4);
#pragma unroll
                    for (int kk = 0; kk < 4; kk++) *(uint32_t*)(blk + (size_t)kk * 16 * GM_APAD + kc * 4) = w4[kk];
                }
            }
#pragma unroll
        for (int q = 0; q < XU; q++) {
            uint4 v = xreg[q];
            if (!full && !(k0 + 8 * (xkc + XQ * q) < K)) v = make_uint4(0, 0, 0, 0);
            if (BF32) {                                      // element kk -> k-group 2kc, element 4+kk -> k-group 2kc+1, widened here
                const uint32_t e0[4] = {v.x << 16, v.x & 0xFFFF0000u, v.y << 16, v.y & 0xFFFF0000u};
                const uint32_t e1[4] = {v.z << 16, v.z & 0xFFFF0000u, v.w << 16, v.w & 0xFFFF0000u};
#pragma unroll
                for (int kk = 0; kk < 4; kk++) {
                    char* d = xblk + (size_t)kk * 16 * GM_BPAD + q * 2 * XQ * TB * 4;
                    *(uint32_t*)d = e0[kk]; *(uint32_t*)(d + TB * 4) = e1[kk];
                }
            } else {
                uint32_t w4[4]; pack4(v, w4);
#pragma unroll
                for (int kk = 0; kk < 4; kk++) *(uint32_t*)(xblk + (size_t)kk * 16 * GM_BPAD + q * XQ * TB * 4) = w4[kk];
            }
        }
    };
    const char* ap = As + (size_t)(((WN == 4 ? wave : 0) * 4 + fk) * 16 + fi) * GM_APAD;       // (+ c*WN*64*GM_APAD for chain c)
    const char* bp = Bs + (size_t)(fk * 16 + fi) * GM_BPAD + mt0 * 4;
    issue(0);
    for (int k0 = 0; k0 < K; k0 += GM_KS) {
        if (!(GM_DBG & 1) || k0 == 0) commit(k0);
        if (!(GM_DBG & 2)) __syncthreads();
        if (!(GM_DBG & 1) && k0 + GM_KS < K) issue(k0 + GM_KS);   // in flight during this slab's MFMAs
        // ---- 32 k-groups of 4 as 16 pairs: acc[n-tile][m-tile t] = mfma(A, B, acc), k ascending (beyond K both operands are 0).
        // Fully unrolled and software-pipelined by hand, three stages (the sched_barriers pin them):
        //   read    pair j+2's B words (and every fourth pair the next eight groups' A words): ds_read_b128, raw bf16 pairs;
        //   widen   pair j+1's operands into their own registers (lo half: shift, hi half: mask -- 2*(MT+NCH) VALU ops);
        //   MFMA    pair j: 2 k-groups x MT x NCH matrix instructions back to back, nothing in between.
        // Measured (tools/gemmbench.hip, tools/mfma_lds_bench.hip): a widening op right in front of its MFMA -- hipcc's choice, into
        // ONE reused register -- serialises on that register (write-after-read against the MFMA in flight + the VALU->MFMA hazard
        // nops): 52 instead of 32 cycles per MFMA; ds_reads among MFMAs are free; an LDS round trip in front of each MFMA pair
        // (hipcc's other choice) costs 40 %.
        constexpr int NP = GM_KS / 8;
        uint32_t fb[2][BF32 ? 2 : 1][MT], fa[2][NCH][4];    // raw ring: pair j+1 (being widened / waiting), pair j+2 being read
        float wa[2][2][NCH], wb[2][2][BF32 ? 1 : MT];        // [pair parity][k-group parity]
        auto read_b = [&](int j) {
            const int sl = j & 1;
            if (GM_DBG & 4) { for (int h = 0; h < (BF32 ? 2 : 1); h++) for (int t = 0; t < MT; t++) fb[sl][h][t] = (uint32_t)(k0 + j + t) * 0x10001u; return; }
            if (BF32) {                                      // two k-groups x MT f32 values
#pragma unroll
                for (int h = 0; h < 2; h++)
#pragma unroll
                    for (int t4 = 0; t4 < MT; t4 += 4) {
                        const uint4 v = *(const uint4*)(bp + ((2 * j + h) * TB + t4) * 4);
                        fb[sl][h % (BF32 ? 2 : 1)][t4] = v.x; fb[sl][h % (BF32 ? 2 : 1)][(t4 + 1) % MT] = v.y;
                        fb[sl][h % (BF32 ? 2 : 1)][(t4 + 2) % MT] = v.z; fb[sl][h % (BF32 ? 2 : 1)][(t4 + 3) % MT] = v.w;
                    }
            } else if (MT == 8) {                            // raw bf16 pairs: one word = (k-group 2j | k-group 2j+1 << 16) of one m-tile
                const uint4 lo = *(const uint4*)(bp + j * 32), hi = *(const uint4*)(bp + j * 32 + 16);
                fb[sl][0][0] = lo.x; fb[sl][0][1] = lo.y; fb[sl][0][2 % MT] = lo.z; fb[sl][0][3 % MT] = lo.w;
                fb[sl][0][4 % MT] = hi.x; fb[sl][0][5 % MT] = hi.y; fb[sl][0][6 % MT] = hi.z; fb[sl][0][7 % MT] = hi.w;
            } else if (MT == 4) {
                const uint4 lo = *(const uint4*)(bp + j * 16);
                fb[sl][0][0] = lo.x; fb[sl][0][1] = lo.y; fb[sl][0][2 % MT] = lo.z; fb[sl][0][3 % MT] = lo.w;
            } else {
                const uint2 v = *(const uint2*)(bp + j * (TB * 4));
                fb[sl][0][0] = v.x; fb[sl][0][1 % MT] = v.y;
            }
        };
        auto read_a = [&](int o) {                           // octet o: k-groups 8o .. 8o+7
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                if (GM_DBG & 4) { for (int e = 0; e < 4; e++) fa[o & 1][c][e] = (uint32_t)(k0 + o + e) * 0x10001u; continue; }
                const uint4 v = *(const uint4*)(ap + (size_t)c * WN * 64 * GM_APAD + o * 16);
                fa[o & 1][c][0] = v.x; fa[o & 1][c][1] = v.y; fa[o & 1][c][2] = v.z; fa[o & 1][c][3] = v.w;
            }
        };
        auto widen = [&](int j) {
            const int sl = j & 1, q = j & 1;
#pragma unroll
            for (int c = 0; c < NCH; c++) { const uint32_t w = fa[(j >> 2) & 1][c][j & 3]; wa[q][0][c] = bf_lo(w); wa[q][1][c] = bf_hi(w); }
            if (!BF32) {
#pragma unroll
                for (int t = 0; t < MT; t++) { wb[q][0][t % (BF32 ? 1 : MT)] = bf_lo(fb[sl][0][t]); wb[q][1][t % (BF32 ? 1 : MT)] = bf_hi(fb[sl][0][t]); }
            }
        };
        read_a(0); read_b(0);
        widen(0);
        if (!BF32) read_b(1);
#pragma unroll
        for (int j = 0; j < NP; j++) {
            if (j + 1 < NP) widen(j + 1);                    // (frees raw slot j+1 & 1 ... which pair j+2 then refills)
            if (BF32) { if (j + 1 < NP) read_b(j + 1); }     // f32 tile: pair j+1's values are read while pair j's MFMAs run, used as they are
            else if (j + 2 < NP) read_b(j + 2);
            if ((j & 3) == 1 && j + 3 < NP) read_a(j / 4 + 1);   // octet o+1 is first widened at pair 4o+3, last use of octet o-1 was pair 4o-1
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int par = 0; par < 2; par++)
#pragma unroll
                for (int t = 0; t < MT; t++) {
                    const float bval = BF32 ? __uint_as_float(fb[j & 1][par % (BF32 ? 2 : 1)][t]) : wb[j & 1][par][t % (BF32 ? 1 : MT)];
#pragma unroll
                    for (int c = 0; c < NCH; c++) acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j & 1][par][c], bval, acc[c][t], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!(GM_DBG & 2)) __syncthreads();
    }
    // D layout: lane holds rows (lane>>4)*4 + r of the n-tile, column lane&15 of the m-tile
#pragma unroll
    for (int t = 0; t < MT; t++)
        gemm_epilogue4<EPI>(p, acc[0][t], acc[NCH - 1][t], m0 + (mt0 + t) * 16 + (lane & 15), n0 + nt_off + (lane >> 4) * 4);
}

// The softmax numerator of every possible raw score, in f64: a q.k chain is truncated to bf16 before anything else happens to it
// (llamatransformer.go:459), so  s -> trunc(s / sqrt(hd)) -> (+ 0 where unmasked) -> exp  is a function of 16 bits.  The table is
// filled by the DEVICE code path attn_exact_kernel evaluates inline (same __fdiv_rn, same exp), so a lookup is bit-identical to
// computing it (adding the mask's +0 can only turn -0 into +0, and exp(-0) == exp(+0)); the prefill attention replaces ~130
// instructions per element by one 8-byte load from 512 KB (the reference does the same for SiLU, activations.go:15-25).
__global__ void exp_table_kernel(double* tab, float divisor) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1 << 16)) return;
    const uint16_t s16 = bf_trunc(__fdiv_rn(bf_wide((uint16_t)i), divisor));        // DivToScalar :464
    tab[i] = exp((double)bf_wide(s16));                                              // Softmax impl:498
}
extern "C" hipError_t lnbk_exp_table(double* tab, float divisor, hipStream_t st) {
    hipLaunchKernelGGL(exp_table_kernel, dim3(256), dim3(256), 0, st, tab, divisor);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// attn_mfma_kernel: the prefill form of the attention (S >= 16 query rows), the same arithmetic as attn_exact_kernel below with
// both matrix products on the exact f32 matrix cores (v_mfma_f32_16x16x4_f32 == the reference's k-ordered chain, see gemm_mfma_kernel).
// One WAVE owns 16 query rows of one head and walks the cached positions in tiles of 16, twice:
//   pass 1  S^T tile [16 j][16 i] = sum_d K[j][d] Q[i][d] (d ascending: 32 dependent MFMAs), then per element trunc, /sqrt(hd), mask,
//           exp in f64; the row sums Z_i must be added in j order in f64: the tile goes through a 2.3 KB LDS patch and lane i < 16
//           walks row i's sixteen values (the reference's serial sum, impl:492-499);
//   pass 2  the scores again (cheaper than keeping S x T doubles), p = trunc(f32(e / Z_i)), transposed through the LDS into the A
//           operand layout, and out[i][d] += p[i][j] v[j][d] with j ascending inside and across the MFMAs (lane n owns the HD/16
//           consecutive output dims n*HD/16.., so one 16 B load of a V row feeds its eight MFMAs).
// Masked positions (j % S > i, the modulo-broadcast [S,S] mask) contribute e = 0 -> p = +0.  With FINITE K and V rows the masked score adds
// to -inf and the product p * v is +-0, acc + (+-0) == acc and acc is never -0, so with the standard causal layout (pos0 == 0) the tiles above
// the diagonal are skipped like attn_exact_kernel does.  With a NaN or inf in a row this is NOT the reference (NaN + -inf = NaN, +0 x NaN = NaN,
// and a tile's 16 positions are the B operand of all 16 query rows): the entry point scans the rows a multi-row call writes
// (kv_nonfinite_scan_kernel) and attn_plain_kernel, launched behind this kernel, recomputes the call's rows when the context holds such a row.
// CAUSAL (lnb_forward_append, AttnParams::causal; a template parameter, so the modulo form's instantiation is the code it was): the mask is
// j > pos0 + irow at ANY pos0.  The softmax subtracts no maximum and a masked entry adds +0 to the f64 sum and to the PV chain, so row i of the
// call is the shorter row of the one-token step at pos0 + i, bit for bit; tiles wholly above the SHIFTED diagonal are skipped
// (Tmax = min(pos0 + i0 + 16, T)), the longest rows are still handed out first.  attn_mfma3_kernel has the same parameter.
// K cache layout [kv head][d/8][position][8]: a lane (j, kk) loads its position's 16 B units and picks elements kk and 4+kk
// (k-groups 2c, 2c+1) with one v_perm_b32 each; the four kk-lanes of a position load the same unit (L1 traffic, not HBM).
// grid (H, ceil(S/64)), block 256 = 4 independent waves (no workgroup barrier anywhere).
// ------------------------------------------------------------------------------------------------
// workgroup -> (head, sub-block) for the attention grids (gridDim = (heads, sub-blocks)).  The hardware hands workgroup w to XCD w % 8,
// each XCD has its own L2, and the query heads of one GQA group read the SAME K / V rows: with the plain (blockIdx.x, blockIdx.y)
// mapping the four heads of a group sit on four XCDs and the rows are fetched from HBM four times (rocprofv3 FETCH_SIZE of the
// long-context kernels at T = 4101: 33.3 MB per launch against 8.4 MB of V).  Here consecutive VIRTUAL ids stay on one XCD and virtual
// ids are head-major, so a group's heads share an L2 (8B shape: XCD x runs heads 4x .. 4x+3 = KV head x).
// xcd_head_block: inside an XCD head-major (a head's sub-blocks follow each other: the decode kernels, equal-cost sub-blocks; measured
// 191.0 against 189.5 tokens/s at configs[2] for the other order).  xcd_head_block_bmajor: sub-block-major (all of the XCD's heads for
// sub-block 0, then sub-block 1, ...), so a caller whose sub-blocks differ in cost can hand out the longest ones first (prefill).
DEVINL void xcd_head_block(int& h, int& b) {
    const unsigned H = gridDim.x, nb = gridDim.y, lin = blockIdx.y * H + blockIdx.x;
    if ((H & 7u) == 0) {
        const unsigned v = (lin & 7u) * ((H >> 3) * nb) + (lin >> 3);     // consecutive virtual ids stay on one XCD
        h = (int)(v / nb); b = (int)(v % nb);
    } else { h = (int)blockIdx.x; b = (int)blockIdx.y; }
}
DEVINL void xcd_head_block_bmajor(int& h, int& b) {
    const unsigned H = gridDim.x, lin = blockIdx.y * H + blockIdx.x;
    if ((H & 7u) == 0) {
        const unsigned hg = H >> 3, w = lin >> 3;            // heads per XCD; index inside the XCD's share
        h = (int)((lin & 7u) * hg + w % hg); b = (int)(w / hg);
    } else { h = (int)blockIdx.x; b = (int)blockIdx.y; }
}
constexpr int ATM_ET = 144, ATM_PT = 80, ATM_WLDS = 16 * ATM_ET + 16 * ATM_PT + 128;     // per-wave LDS patch: e tile | p tile | Z row
template <int HD, bool CAUSAL = false> __global__ __launch_bounds__(256, 2) void attn_mfma_kernel(AttnParams p) {
    __shared__ __attribute__((aligned(16))) char sm[4 * ATM_WLDS];
    constexpr int NK = HD / 8, DPL = HD / 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int h, by_; xcd_head_block_bmajor(h, by_);
    by_ = (int)gridDim.y - 1 - by_;                          // the last query rows see the longest context: handed out first
    const int i0 = (by_ * 4 + wave) * 16;
    const int S = p.S, H = p.H, KVH = p.KVH;
    if (i0 >= S) return;                                     // (waves are independent)
    const int pos0 = p.st->pos, T = pos0 + S;
    const int kvh = h / (H / KVH);
    const int fi = lane & 15, fk = lane >> 4;
    char* et = sm + wave * ATM_WLDS;
    char* pt = et + 16 * ATM_ET;
    double* zrow = (double*)(pt + 16 * ATM_PT);
    const uint4* kbase = (const uint4*)p.cache_k + (size_t)kvh * NK * p.seq_len;
    const uint16_t* vbase = p.cache_v + (size_t)kvh * HD + fi * DPL;
    const size_t vrow = (size_t)KVH * HD;
    const uint32_t sel = 0x0c0cu | ((uint32_t)(2 * fk) << 16) | ((uint32_t)(2 * fk + 1) << 24);   // element kk of a 4-element word pair
    const int Tmax = CAUSAL ? (pos0 + i0 + 16 < T ? pos0 + i0 + 16 : T)      // the shifted diagonal: tiles wholly above it are skipped at every start position
                            : (S > 1 && pos0 == 0) ? (i0 + 16 < T ? i0 + 16 : T) : T;
    const int NJ = (Tmax + 15) >> 4;
    const int irow = i0 + fi;                                // this lane's query row in the S^T tile (column i)

    float qf[2 * NK];                                        // Q[irow][4g + kk], g = 0 .. HD/4-1
    {
        const uint4* q = (const uint4*)(p.q + ((size_t)(irow < S ? irow : S - 1) * H + h) * HD);
#pragma unroll
        for (int c = 0; c < NK; c++) {
            const uint4 u = q[c];
            qf[2 * c] = __uint_as_float(__builtin_amdgcn_perm(u.y, u.x, sel));
            qf[2 * c + 1] = __uint_as_float(__builtin_amdgcn_perm(u.w, u.z, sel));
        }
    }
    auto load_k = [&](uint4 (&k)[NK], int j0) {
        int j = j0 + fi; j = j < T ? j : T - 1;
#pragma unroll
        for (int c = 0; c < NK; c++) k[c] = kbase[(size_t)c * p.seq_len + j];
    };
    // raw scores of the tile: lane holds positions j0 + 4*kk + r (r = 0..3) against query row irow
    auto qk = [&](const uint4 (&k)[NK]) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NK; c++) {                       // MatMul q.k, d ascending (operations_matmul.go:37-55)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(__builtin_amdgcn_perm(k[c].y, k[c].x, sel)), qf[2 * c], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(__builtin_amdgcn_perm(k[c].w, k[c].z, sel)), qf[2 * c + 1], acc, 0, 0, 0);
        }
        return acc;
    };
    // e[r] = exp(score) (0 where masked or past T)
    auto expo = [&](const f32x4& acc, int j0, double (&e)[4]) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = j0 + 4 * fk + r;
            const bool dead = CAUSAL ? j > pos0 + irow || j >= T                       // row irow is the one-token step at pos0 + irow: positions 0 .. pos0 + irow
                                     : j >= T || ((S > 1) && ((pos0 == 0 ? j : j % S) > irow));   // triu(-inf,1) broadcast by modulo (tensoriterators.go:47-55);
                                                                                         // pos0 == 0: T == S, no wrap (uniform branch, saves the division)
            const double ev = p.exp_tab[bf_trunc(acc[r])];                       // / sqrt(hd) :464, (+ mask 0 :469-473), exp impl:498: tabulated
            e[r] = dead ? 0.0 : ev;                                              // exp(-inf) == 0
        }
    };
#define ATM_LDS_TURN() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

    // ---- pass 1: Z_i = sum_j exp(s_ij), f64, j ascending (lane i < 16 carries row i)
    double z = 0.0;
    uint4 kt[NK];                                            // the tile's K rows; the next tile's are loaded into the same registers as
                                                             // soon as the 32 MFMAs have read them, and land during the exps
    auto zsum = [&](int j0, bool more) {
        const f32x4 sc = qk(kt);
        if (more) load_k(kt, j0 + 16);
        double e[4];
        expo(sc, j0, e);
        typedef double d2 __attribute__((ext_vector_type(2)));
        d2* w = (d2*)(et + fi * ATM_ET + fk * 32);
        w[0] = d2{e[0], e[1]}; w[1] = d2{e[2], e[3]};
        ATM_LDS_TURN();
        if (lane < 16) {
            const d2* row = (const d2*)(et + lane * ATM_ET);
            d2 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = row[u];
#pragma unroll
            for (int u = 0; u < 8; u++) { z += v[u].x; z += v[u].y; }
        }
        ATM_LDS_TURN();
    };
    load_k(kt, 0);
    for (int jt = 0; jt < NJ; jt++) zsum(jt * 16, jt + 1 < NJ);      // (wave-uniform trip count)
    if (lane < 16) zrow[lane] = z;
    ATM_LDS_TURN();
    const double zi = zrow[fi];

    // ---- pass 2: p = trunc(f32(e / Z_i)), out = sum_j p_j v_j (j ascending)
    f32x4 o[DPL];
#pragma unroll
    for (int t = 0; t < DPL; t++) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto pv = [&](int j0, bool more) {
        const f32x4 sc = qk(kt);
        if (more) load_k(kt, j0 + 16);
        uint4 vv[4];                                         // V[j0 + 4g + kk][dims fi*DPL ..]: in flight during the exps
#pragma unroll
        for (int g = 0; g < 4; g++) {
            int j = j0 + 4 * g + fk; j = j < T ? j : T - 1;
            const uint16_t* a = vbase + (size_t)j * vrow;
            if (DPL == 8) vv[g] = *(const uint4*)a;
            else { const uint2 t2 = *(const uint2*)a; vv[g] = make_uint4(t2.x, t2.y, 0, 0); }
        }
        double e[4];
        expo(sc, j0, e);
        float4 pf;                                           // impl:506 + ToBFloat16 :493
        pf.x = bf_wide(bf_trunc((float)(e[0] / zi))); pf.y = bf_wide(bf_trunc((float)(e[1] / zi)));
        pf.z = bf_wide(bf_trunc((float)(e[2] / zi))); pf.w = bf_wide(bf_trunc((float)(e[3] / zi)));
        *(float4*)(pt + fi * ATM_PT + fk * 16) = pf;         // p[i = fi][j = 4kk .. 4kk+3]
        ATM_LDS_TURN();
        float pa[4];
#pragma unroll
        for (int g = 0; g < 4; g++) pa[g] = *(const float*)(pt + fi * ATM_PT + (4 * g + fk) * 4);     // A operand: p[i = fi][j = 4g + kk]
        ATM_LDS_TURN();
#pragma unroll
        for (int g = 0; g < 4; g++) {                        // MatMul p.v, j ascending (llamatransformer.go:504-514)
            const uint32_t wd[4] = {vv[g].x, vv[g].y, vv[g].z, vv[g].w};
#pragma unroll
            for (int t = 0; t < DPL; t++)
                o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[g], (t & 1) ? bf_hi(wd[t >> 1]) : bf_lo(wd[t >> 1]), o[t], 0, 0, 0);
        }
    };
    load_k(kt, 0);
    for (int jt = 0; jt < NJ; jt++) pv(jt * 16, jt + 1 < NJ);
#undef ATM_LDS_TURN
    // D layout: lane holds query rows 4*kk + r, output dims fi*DPL + t
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = i0 + 4 * fk + r;
        if (row >= S) continue;
        uint32_t w[DPL / 2];
#pragma unroll
        for (int t = 0; t < DPL; t += 2) w[t / 2] = (uint32_t)bf_trunc(o[t][r]) | ((uint32_t)bf_trunc(o[t + 1][r]) << 16);
        uint16_t* dst = p.out + ((size_t)row * H + h) * HD + fi * DPL;
        if (DPL == 8) *(uint4*)dst = make_uint4(w[0], w[1], w[2 % (DPL / 2)], w[3 % (DPL / 2)]);
        else *(uint2*)dst = make_uint2(w[0], w[1]);
    }
}

// ------------------------------------------------------------------------------------------------
// attn_mfma3_kernel (round 6): attn_mfma_kernel with the scores computed ONCE and the exp-table look-ups issued a tile ahead.
//
// profiles/r06_prefill_stalls.md: of the 11.3 k cycles a wave of attn_mfma_kernel spends per (query tile, position tile) pair, 7.0 k are issue stalls on the matrix pipe
// (a wave's program is chains of dependent matrix instructions, 32 for q.k -- and pass 2 runs that chain a second time only to get the same sixteen-bit values back) and
// 2.0 k are spent parked on the four table look-ups of each pass.  Here
//   pass 1  keeps what the table is indexed with: the truncated raw score (0xFF80 = -inf -> exp == 0 for masked / past-the-end elements), four 16-bit values per lane and
//           tile = one 8-byte store into score_idx[head][query tile][position tile][lane] (512 B per tile, coalesced; written and read by the same lane);
//   pass 2  reads them back: no K rows, no q.k chain -- a third of the matrix instructions gone;
//   both    issue a tile's look-ups and let the NEXT tile's matrix work run before the values are used (pass 1: tile t's exponentials are added to Z after tile t + 1's
//           chain; pass 2: tile t + 1's indices, look-ups and V rows go in flight before tile t's 4 x HD/16 matrix instructions).
// Every vector-memory load of the loops is an asm load with a hand-counted wait (hipcc drains vmcnt(0) around loop-carried loads, NOTES 5.1); tools/isa_audit.py follows the
// registers.  Counts assume what LLVM assumes for gfx9: loads and stores retire in issue order on the one counter.  Loads are unconditional (clamped tile / position), the
// tile loops of pass 2 are unrolled by two for static buffer indices; a padded tile is loaded and not consumed.
// Same arithmetic per element in the same order as attn_mfma_kernel: same bits (tests/test_gpu_round6.py runs both).
// ------------------------------------------------------------------------------------------------
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
DEVINL void atm_ld16(u32x4& d, unsigned voff, const char* sb) { asm volatile("global_load_dwordx4 %0, %1, %2 ; RING_LOAD" : "=&v"(d) : "v"(voff), "s"(sb) : "memory"); }
DEVINL void atm_ld8(u32x2& d, unsigned voff, const char* sb) { asm volatile("global_load_dwordx2 %0, %1, %2 ; RING_LOAD" : "=&v"(d) : "v"(voff), "s"(sb) : "memory"); }
DEVINL const char* atm_uniform(const char* a) {             // a pointer that IS wave-uniform, told to the compiler (an "s" operand must not be handed a VGPR pair)
    const size_t v = (size_t)a;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (const char*)(((size_t)hi << 32) | lo);
}
template <int HD, bool CAUSAL = false> __global__ __launch_bounds__(256, 2) void attn_mfma3_kernel(AttnParams p) {
    __shared__ __attribute__((aligned(16))) char sm[4 * ATM_WLDS];
    constexpr int NK = HD / 8, DPL = HD / 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int h, by_; xcd_head_block_bmajor(h, by_);
    by_ = (int)gridDim.y - 1 - by_;                          // the last query rows see the longest context: handed out first
    const int itile = by_ * 4 + wave, i0 = itile * 16;
    const int S = p.S, H = p.H, KVH = p.KVH;
    if (i0 >= S) return;                                     // (waves are independent)
    const int pos0 = p.st->pos, T = pos0 + S;
    const int kvh = h / (H / KVH);
    const int fi = lane & 15, fk = lane >> 4;
    char* et = sm + wave * ATM_WLDS;
    char* pt = et + 16 * ATM_ET;
    double* zrow = (double*)(pt + 16 * ATM_PT);
    const uint32_t sel = 0x0c0cu | ((uint32_t)(2 * fk) << 16) | ((uint32_t)(2 * fk + 1) << 24);   // element kk of a 4-element word pair
    const int Tmax = CAUSAL ? (pos0 + i0 + 16 < T ? pos0 + i0 + 16 : T)      // the shifted diagonal: tiles wholly above it are skipped at every start position
                            : (S > 1 && pos0 == 0) ? (i0 + 16 < T ? i0 + 16 : T) : T;
    const int NJ = (Tmax + 15) >> 4;
    const int irow = i0 + fi;                                // this lane's query row in the S^T tile (column i)
    const char* const kb = atm_uniform((const char*)p.cache_k + (size_t)kvh * NK * p.seq_len * 16);            // K runs of the KV head: [d / 8][position][8]
    const size_t krun = (size_t)p.seq_len * 16;
    const char* const vb = atm_uniform((const char*)p.cache_v + (size_t)kvh * HD * 2);
    const unsigned vrow2 = (unsigned)(KVH * HD * 2), vlane = (unsigned)(fi * DPL * 2);
    const char* const xb = atm_uniform((const char*)(p.score_idx + ((size_t)(h * ((S + 15) >> 4) + itile) * p.sidx_jt) * 64));
    const char* const tab = atm_uniform((const char*)p.exp_tab);

    float qf[2 * NK];                                        // Q[irow][4g + kk], g = 0 .. HD/4-1
    {
        const uint4* q = (const uint4*)(p.q + ((size_t)(irow < S ? irow : S - 1) * H + h) * HD);
#pragma unroll
        for (int c = 0; c < NK; c++) {
            const uint4 u = q[c];
            qf[2 * c] = __uint_as_float(__builtin_amdgcn_perm(u.y, u.x, sel));
            qf[2 * c + 1] = __uint_as_float(__builtin_amdgcn_perm(u.w, u.z, sel));
        }
    }
    __builtin_amdgcn_sched_barrier(0);                       // (the compiler's own loads are consumed in front of the first asm load)
#define ATM_LDS_TURN() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#define ATM_RETIRE(r) asm volatile("; RING_RETIRE %0" : "+v"(r))
    typedef double d2 __attribute__((ext_vector_type(2)));
    auto as_double = [](const u32x2& v) { return __hiloint2double((int)v.y, (int)v.x); };

    // ---- pass 1: raw scores -> table indices (kept) -> Z_i = sum_j exp(s_ij), f64, j ascending (lane i < 16 carries row i)
    u32x4 kr[NK];
    u32x2 er[4];
    auto k_issue = [&](int jt) {
        int j = jt * 16 + fi; j = j < T ? j : T - 1;
        const unsigned voff = (unsigned)j * 16u;
#pragma unroll
        for (int c = 0; c < NK; c++) atm_ld16(kr[c], voff, kb + (size_t)c * krun);
    };
    double z = 0.0;
    auto zadd = [&]() {                                      // the look-ups in er have landed: the tile goes through the LDS patch, lane i walks row i's sixteen values
        d2* w = (d2*)(et + fi * ATM_ET + fk * 32);
        w[0] = d2{as_double(er[0]), as_double(er[1])}; w[1] = d2{as_double(er[2]), as_double(er[3])};
        ATM_LDS_TURN();
        if (lane < 16) {
            const d2* row = (const d2*)(et + lane * ATM_ET);
            d2 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = row[u];
#pragma unroll
            for (int u = 0; u < 8; u++) { z += v[u].x; z += v[u].y; }
        }
        ATM_LDS_TURN();
    };
    k_issue(0);
#pragma unroll
    for (int r = 0; r < 4; r++) atm_ld8(er[r], 0xFF80u * 8u, tab);     // "tile -1": four zeros (exp(-inf)), so that the loop has one shape; z + 0.0 == z
    u32x2 pk = {0u, 0u};                                     // the previous tile's packed indices: stored one tile late, right behind the next K rows -- by the time a
                                                             // counted wait has the store in front of it, the store is a whole chain old (the counts below count LOADS only)
    for (int jt = 0; jt < NJ; jt++) {                        // (wave-uniform trip count)   in flight here: K(jt) [NK], (store), look-ups(jt - 1) [4]
        const int j0 = jt * 16;
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");     // K(jt) has landed; the four look-ups behind it may not have
#pragma unroll
        for (int c = 0; c < NK; c++) ATM_RETIRE(kr[c]);
        float ko[2 * NK];
#pragma unroll
        for (int c = 0; c < NK; c++) {
            ko[2 * c] = __uint_as_float(__builtin_amdgcn_perm(kr[c].y, kr[c].x, sel));
            ko[2 * c + 1] = __uint_as_float(__builtin_amdgcn_perm(kr[c].w, kr[c].z, sel));
        }
#pragma unroll
        for (int g = 0; g < 2 * NK; g++) asm volatile("" : "+v"(ko[g]));      // widened in front of the refill
        __builtin_amdgcn_sched_barrier(0);
        k_issue(jt + 1 < NJ ? jt + 1 : jt);                  // in flight: look-ups(jt - 1) [4], K(jt + 1) [NK], store
        if (jt > 0) asm volatile("global_store_dwordx2 %0, %1, %2" :: "v"((unsigned)(lane * 8 + (jt - 1) * 512)), "v"(pk), "s"(xb) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < 2 * NK; g++) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(ko[g], qf[g], sc, 0, 0, 0);      // MatMul q.k, d ascending (operations_matmul.go:37-55)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NK) : "memory");             // the PREVIOUS tile's exponentials: their latency ran under this tile's chain
#pragma unroll
        for (int r = 0; r < 4; r++) ATM_RETIRE(er[r]);
        zadd();
        unsigned ix[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = j0 + 4 * fk + r;
            const bool dead = CAUSAL ? j > pos0 + irow || j >= T                       // row irow is the one-token step at pos0 + irow: positions 0 .. pos0 + irow
                                     : j >= T || ((S > 1) && ((pos0 == 0 ? j : j % S) > irow));   // triu(-inf,1) broadcast by modulo (tensoriterators.go:47-55)
            ix[r] = dead ? 0xFF80u : (unsigned)bf_trunc(sc[r]);                          // -inf: exp == 0 (the mask's -inf added to the score, :469-473)
        }
        asm volatile("" : "+v"(ix[0]), "+v"(ix[1]), "+v"(ix[2]), "+v"(ix[3]));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 4; r++) atm_ld8(er[r], ix[r] * 8u, tab);           // / sqrt(hd) :464, exp impl:498: tabulated over the raw score (exp_table_kernel)
        pk = u32x2{ix[0] | (ix[1] << 16), ix[2] | (ix[3] << 16)};
        __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("global_store_dwordx2 %0, %1, %2" :: "v"((unsigned)(lane * 8 + (NJ - 1) * 512)), "v"(pk), "s"(xb) : "memory");
    asm volatile("s_waitcnt vmcnt(0) ; RING_RETIRE_ALL" ::: "memory");
#pragma unroll
    for (int c = 0; c < NK; c++) ATM_RETIRE(kr[c]);
#pragma unroll
    for (int r = 0; r < 4; r++) ATM_RETIRE(er[r]);
    zadd();                                                  // the last tile's
    if (lane < 16) zrow[lane] = z;
    ATM_LDS_TURN();
    const double zi = zrow[fi];
    __builtin_amdgcn_sched_barrier(0);

    // ---- pass 2: p = trunc(f32(e / Z_i)), out = sum_j p_j v_j (j ascending); e from the kept indices
    f32x4 o[DPL];
#pragma unroll
    for (int t = 0; t < DPL; t++) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x2 ixn;                                               // the NEXT tile's packed indices
    u32x2 e2[2][4];
    using VT = std::conditional_t<DPL == 8, u32x4, u32x2>;   // HD / 16 dims of a V row per lane: 16 or 8 bytes
    VT vv[2][4];
    auto idx_issue = [&](int t) { t = t < NJ ? t : NJ - 1; atm_ld8(ixn, (unsigned)(lane * 8 + t * 512), xb); };
    auto look_issue = [&](u32x2 (&e)[4], const unsigned (&o8)[4]) {
#pragma unroll
        for (int r = 0; r < 4; r++) atm_ld8(e[r], o8[r], tab);
    };
    auto v_issue = [&](VT (&v)[4], int t) {                  // V[16 t + 4g + kk][dims fi*DPL ..]
#pragma unroll
        for (int g = 0; g < 4; g++) {
            int j = t * 16 + 4 * g + fk; j = j < T ? j : T - 1;
            const unsigned voff = (unsigned)j * vrow2 + vlane;
            if constexpr (DPL == 8) atm_ld16(v[g], voff, vb); else atm_ld8(v[g], voff, vb);
        }
    };
    auto offs_of = [&](unsigned (&o8)[4]) {                  // byte offsets into the table from the packed indices in ixn
        o8[0] = (ixn.x & 0xFFFFu) * 8u; o8[1] = (ixn.x >> 16) * 8u; o8[2] = (ixn.y & 0xFFFFu) * 8u; o8[3] = (ixn.y >> 16) * 8u;
        asm volatile("" : "+v"(o8[0]), "+v"(o8[1]), "+v"(o8[2]), "+v"(o8[3]));
    };
    {
        idx_issue(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); ATM_RETIRE(ixn);
        unsigned o8[4]; offs_of(o8);
        __builtin_amdgcn_sched_barrier(0);
        idx_issue(1); look_issue(e2[0], o8); v_issue(vv[0], 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    auto tile = [&](auto curc, int t) __attribute__((always_inline)) {
        constexpr int cur = decltype(curc)::value, nxt = cur ^ 1;
        // in flight: look-ups(t) [4], V(t) [4], indices(t + 1) [1] -- all issued a whole tile ago
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int r = 0; r < 4; r++) { ATM_RETIRE(e2[cur][r]); ATM_RETIRE(vv[cur][r]); }
        ATM_RETIRE(ixn);
        unsigned o8[4]; offs_of(o8);
        __builtin_amdgcn_sched_barrier(0);
        idx_issue(t + 2); look_issue(e2[nxt], o8); v_issue(vv[nxt], t + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (t < NJ) {                                        // (wave-uniform; a padded tile is loaded and not consumed)
            float4 pf;                                       // impl:506 + ToBFloat16 :493
            pf.x = bf_wide(bf_trunc((float)(as_double(e2[cur][0]) / zi))); pf.y = bf_wide(bf_trunc((float)(as_double(e2[cur][1]) / zi)));
            pf.z = bf_wide(bf_trunc((float)(as_double(e2[cur][2]) / zi))); pf.w = bf_wide(bf_trunc((float)(as_double(e2[cur][3]) / zi)));
            *(float4*)(pt + fi * ATM_PT + fk * 16) = pf;     // p[i = fi][j = 4kk .. 4kk+3]
            ATM_LDS_TURN();
            float pa[4];
#pragma unroll
            for (int g = 0; g < 4; g++) pa[g] = *(const float*)(pt + fi * ATM_PT + (4 * g + fk) * 4);     // A operand: p[i = fi][j = 4g + kk]
            ATM_LDS_TURN();
#pragma unroll
            for (int g = 0; g < 4; g++) {                    // MatMul p.v, j ascending (llamatransformer.go:504-514)
                uint32_t wd[DPL / 2];
#pragma unroll
                for (int q = 0; q < DPL / 2; q++) wd[q] = vv[cur][g][q];
#pragma unroll
                for (int t2 = 0; t2 < DPL; t2++)
                    o[t2] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[g], (t2 & 1) ? bf_hi(wd[t2 >> 1]) : bf_lo(wd[t2 >> 1]), o[t2], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    for (int t = 0; t < NJ; t += 2) {
        tile(std::integral_constant<int, 0>{}, t);
        tile(std::integral_constant<int, 1>{}, t + 1);
    }
    asm volatile("s_waitcnt vmcnt(0) ; RING_RETIRE_ALL" ::: "memory");
#undef ATM_RETIRE
#undef ATM_LDS_TURN
    // D layout: lane holds query rows 4*kk + r, output dims fi*DPL + t
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = i0 + 4 * fk + r;
        if (row >= S) continue;
        uint32_t w[DPL / 2];
#pragma unroll
        for (int t = 0; t < DPL; t += 2) w[t / 2] = (uint32_t)bf_trunc(o[t][r]) | ((uint32_t)bf_trunc(o[t + 1][r]) << 16);
        uint16_t* dst = p.out + ((size_t)row * H + h) * HD + fi * DPL;
        if (DPL == 8) *(uint4*)dst = make_uint4(w[0], w[1], w[2 % (DPL / 2)], w[3 % (DPL / 2)]);
        else *(uint2*)dst = make_uint2(w[0], w[1]);
    }
}

// ------------------------------------------------------------------------------------------------
// attn_mfma2_kernel (round 6): attn_mfma_kernel with TWO query tiles (32 rows) per wave against each tile of cached positions.
//
// attn_mfma_kernel was 0.517 MFMA-busy for three rounds (profiles/r05_prefill_mfma_counters.md): per tile a wave runs 32 DEPENDENT matrix
// instructions (40 cycles of latency at a 32-cycle issue rate), waits for four table look-ups, turns the LDS patch twice, walks sixteen f64 adds on
// a quarter of its lanes -- and then does it all again in pass 2.  With two query tiles A and B per wave the SAME K operand (one v_perm per k-group instead
// of one per matrix instruction) feeds two independent accumulator chains, S_A^T and S_B^T, alternately: no dependent-issue stall; the V rows of a tile
// are loaded and unpacked once for both; the serial Z adds of the 32 rows run on lanes 0..31 in the same sixteen instructions; the LDS turns, the look-up
// latency and the loop overhead are paid once per 2 x 96 matrix instructions.  Same arithmetic per element, same order (j ascending inside and across the
// matrix instructions), same bits.  Tile A's rows see the diagonal one tile earlier than B's: its masked elements are e = 0, p = +0 (wasted work, not wrong).
// grid (H, ceil(S / 128)), block 256 = 4 independent waves x 32 query rows.  NOT the default (ATM2_MIN_S below): measured slower than the 16-row form.
// (Found on the way: widening an operand with an `asm volatile` VALU instruction right in front of the matrix instruction that reads it gave WRONG scores -- the
// compiler's hazard recognizer does not cover an asm-defined register feeding v_mfma; the packed words are made opaque with an EMPTY asm instead.)
// ------------------------------------------------------------------------------------------------
constexpr int ATM2_WLDS = 32 * ATM_ET + 32 * ATM_PT + 256;   // per-wave LDS patch: e tiles A|B | p tiles A|B | Z rows
constexpr int ATM2_MIN_S = 0;                                // 0: off.  Measured (profiles/r06_prefill_attn.log, 8B shape, whole Forward): 4096 rows 536.1 -> 537.8 ms, 2048: 249.9 -> 256.8, 512: 62.2 -> 64.8 -- SLOWER:
                                                             // the dependent-issue stall it removes is not what bounds the kernel (table look-up latency, eight f64 divisions and the LDS turns per tile are), and 32-row
                                                             // waves halve the number of jobs on a triangular workload.  Kept bit-exact and selectable (LNB_ATTN_MFMA2=<min rows>) for the next attempt.
template <int HD> __global__ __launch_bounds__(256, 2) void attn_mfma2_kernel(AttnParams p) {
    __shared__ __attribute__((aligned(16))) char sm[4 * ATM2_WLDS];
    constexpr int NK = HD / 8, DPL = HD / 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int h, by_; xcd_head_block_bmajor(h, by_);
    by_ = (int)gridDim.y - 1 - by_;                          // the last query rows see the longest context: handed out first
    const int i0 = (by_ * 4 + wave) * 32;
    const int S = p.S, H = p.H, KVH = p.KVH;
    if (i0 >= S) return;                                     // (waves are independent)
    const int pos0 = p.st->pos, T = pos0 + S;
    const int kvh = h / (H / KVH);
    const int fi = lane & 15, fk = lane >> 4;
    char* et = sm + wave * ATM2_WLDS;
    char* pt = et + 32 * ATM_ET;
    double* zrow = (double*)(pt + 32 * ATM_PT);
    const uint4* kbase = (const uint4*)p.cache_k + (size_t)kvh * NK * p.seq_len;
    const uint16_t* vbase = p.cache_v + (size_t)kvh * HD + fi * DPL;
    const size_t vrow = (size_t)KVH * HD;
    const uint32_t sel = 0x0c0cu | ((uint32_t)(2 * fk) << 16) | ((uint32_t)(2 * fk + 1) << 24);
    const int Tmax = (S > 1 && pos0 == 0) ? (i0 + 32 < T ? i0 + 32 : T) : T;       // tile B's diagonal
    const int NJ = (Tmax + 15) >> 4;
    const int irow[2] = {i0 + fi, i0 + 16 + fi};

    // Q[irow][4g + kk] of both query tiles, PACKED: the values are bf16, so the two k-groups of an 8-chunk share a register (low half: k-group 2c, high
    // half: 2c + 1) and are widened by one shift / mask in front of their matrix instruction -- 32 instead of 64 registers, which is what lets the kernel
    // keep two workgroups per CU without spilling
    uint32_t qp[2][NK];
    const uint32_t selp = ((uint32_t)(2 * (fk & 1)) | ((uint32_t)(2 * (fk & 1) + 1) << 8)) | (((uint32_t)(4 + 2 * (fk & 1)) | ((uint32_t)(5 + 2 * (fk & 1)) << 8)) << 16);
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const uint4* q = (const uint4*)(p.q + ((size_t)(irow[t] < S ? irow[t] : S - 1) * H + h) * HD);
#pragma unroll
        for (int c = 0; c < NK; c++) {
            const uint4 u = q[c];
            const uint32_t lo = fk < 2 ? u.x : u.y, hi = fk < 2 ? u.z : u.w;      // element kk of the first / second four of the chunk
            qp[t][c] = __builtin_amdgcn_perm(hi, lo, selp);                       // bytes: [elem kk of (x|y)] | [elem kk of (z|w)] << 16
        }
    }
    auto load_k = [&](uint4 (&k)[NK], int j0) {
        int j = j0 + fi; j = j < T ? j : T - 1;
#pragma unroll
        for (int c = 0; c < NK; c++) k[c] = kbase[(size_t)c * p.seq_len + j];
    };
    // raw scores of the tile for both query tiles: two independent chains fed by ONE K operand per k-group, d ascending (operations_matmul.go:37-55)
    auto qk2 = [&](const uint4 (&k)[NK], f32x4& sa, f32x4& sb) {
        sa = f32x4{0.f, 0.f, 0.f, 0.f}; sb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NK; c++) {
            const float k0 = __uint_as_float(__builtin_amdgcn_perm(k[c].y, k[c].x, sel)), k1 = __uint_as_float(__builtin_amdgcn_perm(k[c].w, k[c].z, sel));
            // (the empty volatile asm makes the packed word opaque in every iteration: left to itself hipcc hoists the loop-invariant widening out of the
            // tile loop and is back at 64 registers + spills)
            uint32_t qa = qp[0][c], qb = qp[1][c];
            asm volatile("" : "+v"(qa), "+v"(qb));
            const float a0 = bf_lo(qa), a1 = bf_hi(qa), b0 = bf_lo(qb), b1 = bf_hi(qb);
            sa = __builtin_amdgcn_mfma_f32_16x16x4f32(k0, a0, sa, 0, 0, 0);
            sb = __builtin_amdgcn_mfma_f32_16x16x4f32(k0, b0, sb, 0, 0, 0);
            sa = __builtin_amdgcn_mfma_f32_16x16x4f32(k1, a1, sa, 0, 0, 0);
            sb = __builtin_amdgcn_mfma_f32_16x16x4f32(k1, b1, sb, 0, 0, 0);
        }
    };
    auto expo = [&](const f32x4& acc, int j0, int ir, double (&e)[4]) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = j0 + 4 * fk + r;
            const bool dead = j >= T || ((S > 1) && ((pos0 == 0 ? j : j % S) > ir));   // triu(-inf,1) broadcast by modulo (tensoriterators.go:47-55)
            const double ev = p.exp_tab[bf_trunc(acc[r])];                       // / sqrt(hd) :464, (+ mask 0 :469-473), exp impl:498: tabulated
            e[r] = dead ? 0.0 : ev;
        }
    };
#define ATM_LDS_TURN() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
    typedef double d2 __attribute__((ext_vector_type(2)));

    // ---- pass 1: Z_i = sum_j exp(s_ij), f64, j ascending (lane i < 32 carries row i of the 32)
    double z = 0.0;
    uint4 kt[NK];
    load_k(kt, 0);
    for (int jt = 0; jt < NJ; jt++) {                        // (wave-uniform trip count)
        const int j0 = jt * 16;
        f32x4 sa, sb;
        qk2(kt, sa, sb);
        if (jt + 1 < NJ) load_k(kt, j0 + 16);
        double ea[4], eb[4];
        expo(sa, j0, irow[0], ea); expo(sb, j0, irow[1], eb);
        d2* wa = (d2*)(et + fi * ATM_ET + fk * 32);
        d2* wb = (d2*)(et + (16 + fi) * ATM_ET + fk * 32);
        wa[0] = d2{ea[0], ea[1]}; wa[1] = d2{ea[2], ea[3]};
        wb[0] = d2{eb[0], eb[1]}; wb[1] = d2{eb[2], eb[3]};
        ATM_LDS_TURN();
        if (lane < 32) {
            const d2* row = (const d2*)(et + lane * ATM_ET);
            d2 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = row[u];
#pragma unroll
            for (int u = 0; u < 8; u++) { z += v[u].x; z += v[u].y; }
        }
        ATM_LDS_TURN();
    }
    if (lane < 32) zrow[lane] = z;
    ATM_LDS_TURN();
    const double zia = zrow[fi], zib = zrow[16 + fi];

    // ---- pass 2: p = trunc(f32(e / Z_i)), out = sum_j p_j v_j (j ascending)
    f32x4 oa[DPL], ob[DPL];
#pragma unroll
    for (int t = 0; t < DPL; t++) { oa[t] = f32x4{0.f, 0.f, 0.f, 0.f}; ob[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    load_k(kt, 0);
    for (int jt = 0; jt < NJ; jt++) {
        const int j0 = jt * 16;
        f32x4 sa, sb;
        qk2(kt, sa, sb);
        if (jt + 1 < NJ) load_k(kt, j0 + 16);
        uint4 vv[4];                                         // V[j0 + 4g + kk][dims fi*DPL ..]: once for both query tiles
#pragma unroll
        for (int g = 0; g < 4; g++) {
            int j = j0 + 4 * g + fk; j = j < T ? j : T - 1;
            const uint16_t* a = vbase + (size_t)j * vrow;
            if (DPL == 8) vv[g] = *(const uint4*)a;
            else { const uint2 t2 = *(const uint2*)a; vv[g] = make_uint4(t2.x, t2.y, 0, 0); }
        }
        double ea[4], eb[4];
        expo(sa, j0, irow[0], ea); expo(sb, j0, irow[1], eb);
        float4 pfa, pfb;                                     // impl:506 + ToBFloat16 :493
        pfa.x = bf_wide(bf_trunc((float)(ea[0] / zia))); pfa.y = bf_wide(bf_trunc((float)(ea[1] / zia)));
        pfa.z = bf_wide(bf_trunc((float)(ea[2] / zia))); pfa.w = bf_wide(bf_trunc((float)(ea[3] / zia)));
        pfb.x = bf_wide(bf_trunc((float)(eb[0] / zib))); pfb.y = bf_wide(bf_trunc((float)(eb[1] / zib)));
        pfb.z = bf_wide(bf_trunc((float)(eb[2] / zib))); pfb.w = bf_wide(bf_trunc((float)(eb[3] / zib)));
        *(float4*)(pt + fi * ATM_PT + fk * 16) = pfa;        // p[i = fi][j = 4kk .. 4kk+3] of tile A, B
        *(float4*)(pt + (16 + fi) * ATM_PT + fk * 16) = pfb;
        ATM_LDS_TURN();
        float pa[4], pb[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {                        // A operands: p[i = fi][j = 4g + kk]
            pa[g] = *(const float*)(pt + fi * ATM_PT + (4 * g + fk) * 4);
            pb[g] = *(const float*)(pt + (16 + fi) * ATM_PT + (4 * g + fk) * 4);
        }
        ATM_LDS_TURN();
#pragma unroll
        for (int g = 0; g < 4; g++) {                        // MatMul p.v, j ascending (llamatransformer.go:504-514)
            const uint32_t wd[4] = {vv[g].x, vv[g].y, vv[g].z, vv[g].w};
#pragma unroll
            for (int t = 0; t < DPL; t++) {
                const float vf = (t & 1) ? bf_hi(wd[t >> 1]) : bf_lo(wd[t >> 1]);
                oa[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[g], vf, oa[t], 0, 0, 0);
                ob[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(pb[g], vf, ob[t], 0, 0, 0);
            }
        }
    }
#undef ATM_LDS_TURN
    // D layout: lane holds query rows 4*kk + r, output dims fi*DPL + t
#pragma unroll
    for (int tile = 0; tile < 2; tile++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = i0 + 16 * tile + 4 * fk + r;
            if (row >= S) continue;
            uint32_t w[DPL / 2];
#pragma unroll
            for (int t = 0; t < DPL; t += 2) w[t / 2] = tile ? ((uint32_t)bf_trunc(ob[t][r]) | ((uint32_t)bf_trunc(ob[t + 1][r]) << 16))
                                                             : ((uint32_t)bf_trunc(oa[t][r]) | ((uint32_t)bf_trunc(oa[t + 1][r]) << 16));
            uint16_t* dst = p.out + ((size_t)row * H + h) * HD + fi * DPL;
            if (DPL == 8) *(uint4*)dst = make_uint4(w[0], w[1], w[2 % (DPL / 2)], w[3 % (DPL / 2)]);
            else *(uint2*)dst = make_uint2(w[0], w[1]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Exact attention for one (head, query row): scores -> /sqrt(hd) -> mask -> f64 softmax -> PV.
// llamatransformer.go:409-514.  GQA head h reads KV head h/n_rep straight from the un-repeated cache
// (attentionRepeatKV :529-559 and the four Transposes :435-449 become index arithmetic).
// grid (H, S), block 512 = 8 waves (two per SIMD: a single wave issues at most one instruction per ~4.4 cycles):
//   scores : every thread owns one cached position j (512 per pass): the 128-long q.k chain (d ascending) over its K row, read
//            with 16 B loads that are contiguous across the wave (K cache layout [kv head][d/8][position][8]); the next pass's
//            rows are in flight during this pass's chains (register ping-pong); then exp in f64;
//   Z      : wave 0 walks sum_j exp(s_j) in f64, j ascending, 16 values per half-iteration with the other half's LDS reads in
//            flight and one counted wait per half (~9 cycles per dependent v_add_f64);
//   PV     : the role split of the GEMV -- waves 2,3,6,7 produce the EXACT products p_j*v[j,d] (bf16 x bf16) into a double-
//            buffered LDS ring [position][dim] (V rows come through a hand-counted asm prefetch ring three chunks deep);
//            waves 0,1 own one output dim per lane and only add, a whole 64-position chunk in flight per step.
// dynamic LDS: [T f64 e (+ zero pad)][T f32 p (+ zero pad)][hd f32 q][16 B][2 x 64 x hd f32 product ring]
// ------------------------------------------------------------------------------------------------
constexpr int ATT_JC = 64;                                  // cached positions per PV chunk
constexpr int ATT_RP = ATT_JC + 4;                          // product ring: [dim][position] f32, rows padded to 68 floats -- the adders read FOUR positions of their dim per
                                                            // ds_read_b128 (16 reads + 64 adds per chunk instead of 64 + 64: they were issue-bound), lanes 272 B apart: no conflict
__host__ __device__ inline size_t attn_off_pw(int seq_len) { return (((size_t)seq_len + 32) * 8 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t attn_off_q(int seq_len) { return attn_off_pw(seq_len) + ((((size_t)seq_len + ATT_JC) * 4 + 15) & ~(size_t)15); }
__host__ __device__ inline size_t attn_off_z(int seq_len, int hd) { return attn_off_q(seq_len) + (((size_t)hd * 4 + 15) & ~(size_t)15); }
__host__ __device__ inline size_t attn_off_ring(int seq_len, int hd) { return attn_off_z(seq_len, hd) + 128; }   // zb: Z | - | flag | - | 8 wave partials

constexpr int ATT_NT = 512;                                 // 8 waves: two per SIMD (one wave alone issues ~1 instruction / 4.4 cycles)
constexpr int ATT_NPROD = 4;                                // PV: waves 0,1 add; waves 2,3,6,7 produce; waves 4,5 share the adders' SIMDs and
                                                            // stay idle there (two issue-hungry waves on one SIMD halve each other)
constexpr int ATT_VU = ATT_JC / 4 / ATT_NPROD;              // 4-row units per producer per chunk

// V rows of PV chunk c for producer pwv.  One 16 B load covers 8 dims of one position: 16 lanes per row, 4 rows per instruction;
// a lane's four units are FOUR CONSECUTIVE positions c*64 + 4 (4 pwv + lane/16) + u of the same 8 dims (so that it can write its
// products as float4 runs along the position axis of the ring).  A PV step (~64 dependent adds) is several times shorter
// than a load round trip, so three chunks are kept in flight; hipcc drains vmcnt(0) around loop-carried register prefetch,
// hence the same hand-counted asm ring as the GEMV (RING_LOAD / RING_RETIRE, checked by tools/isa_audit.py).
// Always issued (rows clamped to T-1, whose p is +0 beyond the row) so that the count is the same on every path.
template <int HD> DEVINL void attn_load_v(u32x4 (&v)[ATT_VU], const uint16_t* vbase, uint32_t row_bytes, int c, int pwv, int lane, int T) {
    // byte offset of this lane's 8 dims.  With heads of 64 or 32 dims the lanes past the head (their loads are never used) stay INSIDE it: 16 bytes per lane
    // over sixteen lanes are 256 bytes, and from the last KV head of row seq_len - 1 that ran up to 192 bytes past the end of the V cache -- a fault when the
    // cache ends on a page boundary (tests/test_gpu_op_crafted.py: one row at position 127 of a 128-position context, two KV heads of 64)
    const uint32_t dq = (HD >= 128 || (lane & 15) * 8 < HD) ? (uint32_t)(lane & 15) * 16u : 0u;
#pragma unroll
    for (int u = 0; u < ATT_VU; u++) {
        int j = c * ATT_JC + (pwv * 4 + (lane >> 4)) * 4 + u;
        j = j < T ? j : T - 1;
        const char* a = (const char*)vbase + ((size_t)(uint32_t)j * row_bytes + dq);
        asm volatile("global_load_dwordx4 %0, %1, off ; RING_LOAD" : "=&v"(v[u]) : "v"(a) : "memory");
    }
}
template <int N> DEVINL void attn_retire_v(u32x4 (&v)[ATT_VU]) {      // v's loads are done once at most N younger ones are outstanding
    static_assert(ATT_VU == 4, "operand list below");
    asm volatile("s_waitcnt vmcnt(%4) ; RING_RETIRE %0 %1 %2 %3" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : "n"(N) : "memory");
}

// K rows of one scores pass: lane owns position j; chunk c of its row sits at kbase[c*seq_len + j] (position-contiguous)
template <int NK> DEVINL void attn_load_k(uint4 (&k)[NK], const uint4* kbase, int seq_len, int j) {
    const uint4* kr = kbase + j;
#pragma unroll
    for (int c = 0; c < NK; c++) { k[c] = *kr; kr += seq_len; }
}

// score + exp of one cached position (llamatransformer.go:456-473, Softmax impl:498)
template <int NK> DEVINL void attn_score(const uint4 (&k)[NK], const float* qf, int j, int T, int S, int i, float divisor, double* e, const double* exp_tab = nullptr) {
    if (j >= T) return;
    const bool masked = (S > 1) && ((j % S) > i);            // triu(-inf,1) broadcast by modulo (tensoriterators.go:47-55)
    double ev = 0.0;                                         // exp(-inf) == 0
    if (!masked) {
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < NK; c++) {                       // MatMul q.k, d ascending (operations_matmul.go:37-55)
            const float4 xa = *(const float4*)(qf + c * 8), xb = *(const float4*)(qf + c * 8 + 4);
            acc = mac8(acc, xa, xb, k[c]);
        }
        uint16_t s = bf_trunc(acc);
        if (exp_tab) ev = exp_tab[s];                        // the model's table of the three lines below over all 65536 raw scores (exp_table_kernel): the batched grids, where
                                                             // the vector unit is the bound (one stream alone: the ~130 inline instructions are faster than the load's round trip, measured)
        else {
            s = bf_trunc(__fdiv_rn(bf_wide(s), divisor));   // DivToScalar :464
            if (S > 1) s = bf_trunc(bf_wide(s) + 0.0f);      // Add(scores, mask) with mask==0 :469-473
            ev = exp((double)bf_wide(s));
        }
    }
    e[j] = ev;
}

// PV pipeline, one barrier per step on every wave: at step c the producers turn chunk c (rows already in vc) into exact products
// in ring slot c&1 ([position][dim] f32) after putting chunk c+3's rows in flight (vn); the adders add chunk c-1.
// The roles are split ONCE (three loops with the same barrier count) so that the ring's load/retire pairing is a property of
// straight-line code that tools/isa_audit.py can check.
template <int HD> DEVINL int attn_row_dim(int r) { return (r % (HD / 8)) * 8 + r / (HD / 8); }      // ring row r holds dim (r % (hd/8)) * 8 + r / (hd/8)
template <int HD, int D = 3> DEVINL void attn_pv_produce(int c, int nchunks, int pwv, int lane, int T, const uint16_t* vbase, uint32_t row_bytes,
                                              const float* pw, char* ring, u32x4 (&vc)[ATT_VU], u32x4 (&vn)[ATT_VU]) {
    constexpr int SLOT = ATT_RP * HD * 4;
    attn_load_v<HD>(vn, vbase, row_bytes, c + D, pwv, lane, T);
    attn_retire_v<D * ATT_VU>(vc);                           // chunks c+1 .. c+D stay in flight
    if (c < nchunks && (lane & 15) * 8 < HD) {
        const int pg = pwv * 4 + (lane >> 4);                // positions 4 pg .. 4 pg + 3 of the chunk
        // ring row of dim d: (d % 8) * (HD / 8) + d / 8 -- the 16 lanes of a write (same k, dim groups 0..15) hit 16 consecutive rows, 272 B
        // apart: 16 different 16-byte bank groups (row-major by dim: 8 rows apart, all in two bank groups -- measured 3x the whole kernel)
        float* dst = (float*)(ring + (c & 1) * SLOT) + (lane & 15) * ATT_RP + 4 * pg;
        const float4 pj = *(const float4*)(pw + c * ATT_JC + 4 * pg);
        const u32x4 a = vc[0], b4 = vc[1], c4 = vc[2], d4 = vc[3];    // exact products: 8-bit x 8-bit significands
        constexpr int KR = (HD / 8) * ATT_RP;                // row distance between k and k + 1
        *(float4*)(dst + 0 * KR) = make_float4(pj.x * bf_lo(a.x), pj.y * bf_lo(b4.x), pj.z * bf_lo(c4.x), pj.w * bf_lo(d4.x));
        *(float4*)(dst + 1 * KR) = make_float4(pj.x * bf_hi(a.x), pj.y * bf_hi(b4.x), pj.z * bf_hi(c4.x), pj.w * bf_hi(d4.x));
        *(float4*)(dst + 2 * KR) = make_float4(pj.x * bf_lo(a.y), pj.y * bf_lo(b4.y), pj.z * bf_lo(c4.y), pj.w * bf_lo(d4.y));
        *(float4*)(dst + 3 * KR) = make_float4(pj.x * bf_hi(a.y), pj.y * bf_hi(b4.y), pj.z * bf_hi(c4.y), pj.w * bf_hi(d4.y));
        *(float4*)(dst + 4 * KR) = make_float4(pj.x * bf_lo(a.z), pj.y * bf_lo(b4.z), pj.z * bf_lo(c4.z), pj.w * bf_lo(d4.z));
        *(float4*)(dst + 5 * KR) = make_float4(pj.x * bf_hi(a.z), pj.y * bf_hi(b4.z), pj.z * bf_hi(c4.z), pj.w * bf_hi(d4.z));
        *(float4*)(dst + 6 * KR) = make_float4(pj.x * bf_lo(a.w), pj.y * bf_lo(b4.w), pj.z * bf_lo(c4.w), pj.w * bf_lo(d4.w));
        *(float4*)(dst + 7 * KR) = make_float4(pj.x * bf_hi(a.w), pj.y * bf_hi(b4.w), pj.z * bf_hi(c4.w), pj.w * bf_hi(d4.w));
    }
    __syncthreads();
}
template <int HD> DEVINL void attn_pv_add(int c, int nchunks, int r, const char* ring, float& acc) {      // r: the lane's ring ROW (its dim: attn_row_dim)
    constexpr int SLOT = ATT_RP * HD * 4;
    if (c > 0 && c <= nchunks && r < HD) {
        // positions past the end of the row carry p == +0 and a V row clamped to T - 1, the call's own last row: for finite V their products are
        // +-0 and acc is never -0, so whole chunks are added (a multi-row call whose rows hold an inf or a NaN is recomputed by attn_plain_kernel)
        const float* src = (const float*)(ring + ((c - 1) & 1) * SLOT) + r * ATT_RP;
        float4 a[ATT_JC / 4];
#pragma unroll
        for (int j = 0; j < ATT_JC / 4; j++) a[j] = *(const float4*)(src + 4 * j);     // whole chunk in flight at once
#pragma unroll
        for (int j = 0; j < ATT_JC / 4; j++) acc = add4(acc, a[j]);
    }
    __syncthreads();
}

// p_j = trunc_bf16(f32(e / Z)) evaluated with an ESTIMATE Zt of the reference's serial f64 sum Z, and certified: any order of adding T
// non-negative doubles is within (T-1) 2^-53 of the exact sum, so Z lies in Zt (1 +- eps), eps = (4T + 8) 2^-53 -- and p is a step
// function of Z.  The quotient is formed as e * (1 / Zt) (within 2 ulps of e / Zt); it must not lie within delta32 = 4T + 12 ulps of the
// one point per bf16 cell where the result changes (low 45 mantissa bits = 2^45 - 2^28); f32-denormal quotients are certified by
// evaluating both ends of the interval.  Returns p; sets bad when the element cannot be certified (the caller then walks the serial sum).
// (Header of attn_long_pv_kernel / NOTES.md 5.9.)
struct CertZ { double rzt, zlo, zhi; unsigned delta32; };
DEVINL CertZ cert_z(double zt, int T) {
    const double epsr = (double)(4 * T + 8) * 1.1102230246251565e-16;
    static_assert(LNB_SEQ_MAX < (1 << 20), "delta32 = 4T + 12 must stay far below the 2^28 between a cell's step point and its end");
    CertZ c; c.rzt = 1.0 / zt; c.zlo = zt * (1.0 - epsr); c.zhi = zt * (1.0 + epsr); c.delta32 = 4u * (unsigned)T + 12u;
    return c;
}
DEVINL float cert_p(double e, const CertZ& c, int& bad) {
    const double q = e * c.rzt;
    const float pj = bf_wide(bf_trunc((float)q));
    const unsigned qh = (unsigned)__double2hiint(q), ql = (unsigned)__double2loint(q);
    const unsigned eq = (qh >> 20) & 0x7FFu;
    if (eq - 897u <= 126u) {                                 // f32-normal quotient (2^-126 <= q < 2): distance from the step point of its bf16 cell
        if ((qh & 0x1FFFu) == 0x1FFFu && ql - (0xF0000000u - c.delta32) <= 2u * c.delta32) bad = 1;
    } else if (q != 0.0) {                                   // f32 denormals, and anything that is not a finite in-range quotient (inf, NaN)
        const float plo = bf_wide(bf_trunc((float)(e / c.zlo))), phi = bf_wide(bf_trunc((float)(e / c.zhi)));
        if (__float_as_uint(plo) != __float_as_uint(phi) || __float_as_uint(pj) != __float_as_uint(plo)) bad = 1;
    }
    return pj;
}
// the reference's serial softmax denominator, walked by ONE wave: rowExpSum += exp(...), j ascending, f64 (impl:492-499).  16 values per half,
// the other half's LDS reads in flight, one wait per half; branch-free (e is zero-padded to a multiple of 32, and readable 16 values further)
DEVINL double attn_zseq_wave(const double* e, int T) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const d2* e2 = (const d2*)e;
    double z = 0.0;
    d2 a[8], b[8];
#define ATT_TOUCH8(r) asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]))
#pragma unroll
    for (int u = 0; u < 8; u++) a[u] = e2[u];
    ATT_TOUCH8(a);
    for (int j = 0; j < T; j += 32) {
#pragma unroll
        for (int u = 0; u < 8; u++) b[u] = e2[((j + 16) >> 1) + u];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; u++) { z += a[u].x; z += a[u].y; }
        __builtin_amdgcn_sched_barrier(0);
        ATT_TOUCH8(b);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; u++) a[u] = e2[((j + 32) >> 1) + u];      // may run past the row's padding: unused then
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; u++) { z += b[u].x; z += b[u].y; }
        __builtin_amdgcn_sched_barrier(0);
        ATT_TOUCH8(a);
        __builtin_amdgcn_sched_barrier(0);
    }
#undef ATT_TOUCH8
    return z;
}
// DENSE = the batched decode's heads x sequences grids (thousands of workgroups): registers for TWO workgroups per CU (4 waves per SIMD, 128
// VGPRs) instead of one -- the K rows of the next 512 positions are then NOT kept in flight during a pass's score chains (the ping-pong
// buffer is 64 of the 178 VGPRs of the single stream's form, which launches 32 workgroups on 256 CUs and wants every register)
// TIMING: the instantiation with the phase stamps (AttnParams.dbg, LNB_GEMV_TIMING): launched exactly when dbg is set; production reads no clock
template <int HD, bool DENSE = false, bool CAUSAL = false, bool TIMING = false> __global__ __launch_bounds__(ATT_NT, DENSE ? 4 : 2) void attn_exact_kernel(AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NK = HD / 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int h, i;
    // batched decode (DENSE): sequence-major inside an XCD -- the (H / 8) heads an XCD owns are the query heads of ONE KV head (H = 32, KVH = 8),
    // so the workgroups of one sequence's four heads are dispatched back to back on the same XCD and the K / V rows the first one pulls are
    // L2 hits for the other three (head-major order: 128 sequences x 92 KB between two readers of the same rows -- every read went to HBM)
    if (DENSE && !p.head_major) xcd_head_block_bmajor(h, i); else xcd_head_block(h, i);
    // batched decode: query row i is the one new token of SEQUENCE i of the batch -- its own position, caches and cache length
    const BatchTab* const bt = p.btab;
    // CAUSAL (lnb_forward_append): query row i IS the one-token step at position st->pos + i -- the same program as a call of one row there
    const int S = (bt || CAUSAL) ? 1 : p.S, KVH = p.KVH;
    const int seq_len = bt ? bt->seq_len[i] : p.seq_len;
    const int pos0 = bt ? bt->st[i]->pos : CAUSAL ? p.st->pos + i : p.st->pos, T = pos0 + S;
    const int kvh = h / (p.H / KVH);
    double* e = (double*)smem;
    float* pw = (float*)(smem + attn_off_pw(p.lds_T));
    float* qf = (float*)(smem + attn_off_q(p.lds_T));
    double* zb = (double*)(smem + attn_off_z(p.lds_T, HD));
    char* ring = smem + attn_off_ring(p.lds_T, HD);
    const uint32_t row_bytes = (uint32_t)KVH * HD * 2;
    // K cache is stored [kv head][d/8][position][8] so that "one position per lane" reads are contiguous across the wave
    const uint4* kbase = (const uint4*)(bt ? p.bkv->ck[i] : p.cache_k) + (size_t)kvh * NK * seq_len;
    const uint16_t* vbase = (bt ? p.bkv->cv[i] : p.cache_v) + (size_t)kvh * HD;
    const int Tend = (S > 1 && pos0 == 0) ? (i + 1) : T;    // see PV below
    const int nchunks = (Tend + ATT_JC - 1) / ATT_JC;
#define ATT_STAMP(n) do { if (LNB_DBG && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0) p.dbg[wave * 16 + (n)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
    ATT_STAMP(0);

    // q first (everything waits on it), then what does not depend on q: this thread's K row and chunk 0 of V (producers)
    const uint16_t* q = p.q + ((size_t)i * p.H + h) * HD;
    const uint16_t q16 = q[tid < HD ? tid : 0];             // unconditional: a predicated load would be waited on at once
    uint4 ka[NK], kb[NK];
    attn_load_k<NK>(ka, kbase, seq_len, tid < seq_len ? tid : seq_len - 1);      // (clamped to the ARRAY end: the first pass's K rows do not wait for the position word; a row past T is never scored)
    if (tid < HD) qf[tid] = bf_wide(q16);
    __syncthreads();
    ATT_STAMP(1);

    // scores: ATT_NT positions per pass, the next pass's rows in flight during this pass's chains (registers ping-pong)
    if constexpr (DENSE) {
        for (int j0 = 0; j0 < T; j0 += ATT_NT) {
            const int j = j0 + tid;
            if (j0 > 0) attn_load_k<NK>(ka, kbase, seq_len, j < T ? j : T - 1);
            attn_score<NK>(ka, qf, j, T, S, i, p.divisor, e, DENSE ? p.exp_tab : nullptr);
        }
    } else
    for (int j0 = 0; j0 < T; j0 += 2 * ATT_NT) {
        const int j = j0 + tid;
        const bool more = j0 + ATT_NT < T, more2 = j0 + 2 * ATT_NT < T;       // block-uniform
        if (more) attn_load_k<NK>(kb, kbase, seq_len, j + ATT_NT < T ? j + ATT_NT : T - 1);
        attn_score<NK>(ka, qf, j, T, S, i, p.divisor, e, DENSE ? p.exp_tab : nullptr);
        if (more) {
            if (more2) attn_load_k<NK>(ka, kbase, seq_len, j + 2 * ATT_NT < T ? j + 2 * ATT_NT : T - 1);
            attn_score<NK>(kb, qf, j + ATT_NT, T, S, i, p.divisor, e);
        }
    }
    // zero padding so that the Z chain can run whole groups (x + 0.0 == x for x >= +0)
    for (int j = T + tid; j < ((T + 31) & ~31); j += ATT_NT) e[j] = 0.0;
    // hipcc's waitcnt pass is path-insensitive: on a (statically possible, dynamically impossible) path a K prefetch of the scores
    // loop is still pending, and it then drains vmcnt(0) in front of every PV step when a V register is reused.  An explicit
    // vmcnt(0) here (all K loads are consumed anyway) clears its scoreboard.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    // producers: the first three PV chunks of V go in flight now and land during the Z chain
    const bool producer = (wave & 3) >= 2;
    const int pwv = (wave & 3) - 2 + ((wave >> 2) << 1);                   // waves 2,3,6,7 -> producers 0..3
    // (single stream: SEVEN chunks -- 448 positions, the whole row at the bench's contexts -- go in flight here, behind the scores: their K
    //  registers are free now, and with three chunks the producers waited for memory in every PV step: 7.4 k cycles of PV at T = 272,
    //  of which the adders' chains are 2.4 k.  The batched DENSE form has 128 registers: three chunks.)
    constexpr int VD = DENSE ? 3 : 7;
    u32x4 v0[ATT_VU], v1[ATT_VU], v2[ATT_VU], v3[ATT_VU], v4[ATT_VU], v5[ATT_VU], v6[ATT_VU], v7[ATT_VU];
    if (producer) {
        attn_load_v<HD>(v0, vbase, row_bytes, 0, pwv, lane, T);
        attn_load_v<HD>(v1, vbase, row_bytes, 1, pwv, lane, T);
        attn_load_v<HD>(v2, vbase, row_bytes, 2, pwv, lane, T);
        if constexpr (VD == 7) {
            attn_load_v<HD>(v3, vbase, row_bytes, 3, pwv, lane, T); attn_load_v<HD>(v4, vbase, row_bytes, 4, pwv, lane, T);
            attn_load_v<HD>(v5, vbase, row_bytes, 5, pwv, lane, T); attn_load_v<HD>(v6, vbase, row_bytes, 6, pwv, lane, T);
        }
    }
    ATT_STAMP(2);
    __syncthreads();
    ATT_STAMP(3);
    // ---- softmax denominator.  The reference adds the T exponentials one by one in f64 (impl:492-499): ~9 cycles per position on one
    // wave (1.1 us at T = 272, 2 us at 512).  As in the long-context kernels it is replaced by a tree estimate + CERTIFIED p_j
    // (cert_p); only a row that cannot be certified (or force_zseq) walks the serial sum.
    int* const zflag = (int*)(zb + 2);
    {
        double part = 0.0;
        for (int j = tid; j < T; j += ATT_NT) part += e[j];
        part = wave_sum_f64(part);
        if (lane == 0) zb[4 + wave] = part;
        if (tid == 0) *zflag = 0;
    }
    __syncthreads();
    const int Tp = (T + ATT_JC - 1) / ATT_JC * ATT_JC;
    {
        const double zt = ((zb[4] + zb[5]) + (zb[6] + zb[7])) + ((zb[8] + zb[9]) + (zb[10] + zb[11]));
        const CertZ cz = cert_z(zt, T);
        int bad = p.force_zseq;
        for (int j = tid; j < Tp; j += ATT_NT)               // impl:506 + ToBFloat16 :493 ; +0 padding up to the chunk
            pw[j] = j < T ? cert_p(e[j], cz, bad) : 0.0f;
        if (bad) *zflag = 1;
    }
    ATT_STAMP(4);
    __syncthreads();
    if (*zflag) {
        if (wave == 0) {                                     // rowExpSum += exp(...), j ascending, f64 (impl:492-499)
            const double z = attn_zseq_wave(e, T);
            if (lane == 0) { zb[0] = z; if (p.zseq_count && tid == 0) atomicAdd(p.zseq_count, 1); }
        }
        __syncthreads();
        const double z = zb[0];
        for (int j = tid; j < T; j += ATT_NT) pw[j] = bf_wide(bf_trunc((float)(e[j] / z)));
    }
    __syncthreads();
    ATT_STAMP(5);

    // PV: out[d] = trunc(sum_{j ascending} p_j * v[j,d]).  Masked columns have p == +0 and acc is never -0, so with the
    // standard causal layout (pos0 == 0) the chain can stop at the chunk that holds the diagonal (Tend).
    float acc = 0.0f;
    if (producer) {
        if constexpr (VD == 7) {
            for (int c = 0; c <= nchunks; c += 8) {          // eight steps per trip: the V register sets rotate without copies
                attn_pv_produce<HD, 7>(c, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v0, v7);
                attn_pv_produce<HD, 7>(c + 1, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v1, v0);
                attn_pv_produce<HD, 7>(c + 2, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v2, v1);
                attn_pv_produce<HD, 7>(c + 3, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v3, v2);
                attn_pv_produce<HD, 7>(c + 4, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v4, v3);
                attn_pv_produce<HD, 7>(c + 5, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v5, v4);
                attn_pv_produce<HD, 7>(c + 6, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v6, v5);
                attn_pv_produce<HD, 7>(c + 7, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v7, v6);
            }
        } else
        for (int c = 0; c <= nchunks; c += 4) {              // four steps per trip: the V register sets rotate without copies
            attn_pv_produce<HD>(c, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v0, v3);
            attn_pv_produce<HD>(c + 1, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v1, v0);
            attn_pv_produce<HD>(c + 2, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v2, v1);
            attn_pv_produce<HD>(c + 3, nchunks, pwv, lane, T, vbase, row_bytes, pw, ring, v3, v2);
        }
    } else if (wave < 2) {
        const int d = wave * 64 + lane;
        for (int c = 0; c <= nchunks; c += (VD + 1)) {       // (the same number of barriers as the producers' trips)
            attn_pv_add<HD>(c, nchunks, d, ring, acc); attn_pv_add<HD>(c + 1, nchunks, d, ring, acc);
            attn_pv_add<HD>(c + 2, nchunks, d, ring, acc); attn_pv_add<HD>(c + 3, nchunks, d, ring, acc);
            if constexpr (VD == 7) {
                attn_pv_add<HD>(c + 4, nchunks, d, ring, acc); attn_pv_add<HD>(c + 5, nchunks, d, ring, acc);
                attn_pv_add<HD>(c + 6, nchunks, d, ring, acc); attn_pv_add<HD>(c + 7, nchunks, d, ring, acc);
            }
        }
    } else {
        for (int c = 0; c <= nchunks; c += (VD + 1)) {
            __syncthreads(); __syncthreads(); __syncthreads(); __syncthreads();
            if constexpr (VD == 7) { __syncthreads(); __syncthreads(); __syncthreads(); __syncthreads(); }
        }
    }
    asm volatile("s_waitcnt vmcnt(0) ; RING_RETIRE_ALL" ::: "memory");   // prefetches past the last chunk
    ATT_STAMP(6);
    if (wave < 2) {
        const int r = wave * 64 + lane;
        if (r < HD) {
            const int d = attn_row_dim<HD>(r);
            if (bt && p.out_xt) p.out_xt[xt_group(i, p.H * HD) + xt_index(i & 15, h * HD + d)] = bf_trunc(acc);   // column batches: straight into the B-operand layout of the wo product
            else p.out[((size_t)i * p.H + h) * HD + d] = bf_trunc(acc);        // [S, H*hd] (:508-514)
        }
    }
}

// ------------------------------------------------------------------------------------------------
// attn_gqa_kernel<HD, G>: the batched decode's attention, one workgroup per (KV head, sequence) serving the G = H / KVH = 4 query heads
// that share the KV head (round 4).  attn_exact_kernel's grid is (H, sequences): at 128 sequences 4096 workgroups of three dependent
// memory round trips each (q -> K rows -> V rows), two resident per CU -- 63 us per layer -- and the vector unit does everything one
// lane-operation at a time (a wave64 instruction occupies its SIMD for four cycles: with two workgroups per CU the kernel is bound by
// the NUMBER of vector instructions, not by memory: profiles/r04_gqa_stamps.log).  Here:
//   scores : a thread owns (cached position, head PAIR): its K row feeds both heads' chains through ONE v_pk_fma_f32 per dimension
//            (q staged in the LDS as (head 2a, head 2a+1) pairs; the same fused multiply-add per lane as mac8); 256 positions per pass;
//   exp    : one 8-byte load from the model's table of exp(trunc(s / sqrt(hd))) over all 65536 bf16 scores (exp_table_kernel: filled by
//            the very instruction sequence attn_exact_kernel evaluates inline -- ~130 f64 instructions per score);
//   Z      : tree estimate + certified p_j per head (cert_p); a head that cannot be certified walks the reference's serial sum on its wave;
//   PV     : V rows are staged ONCE per workgroup (waves 4..7: raw bf16, 32 positions per chunk, four chunks in flight in registers and a
//            ring of four LDS buffers, one barrier per chunk); wave g < 4 adds head g, a lane owns two neighbouring dims: one ds_read_b32,
//            two unpack operations, v_pk_mul_f32 and v_pk_add_f32 per position (multiply, then add: bf16 x bf16 is exact in f32 and the
//            reference rounds only the sum; j ascending) -- the adders do nothing else, the stagers nothing but copy.
// Same bits as attn_exact_kernel per head.  dynamic LDS: [G][Tp] f64 e | [G][Tp] f32 p | q pairs | zb | [4][32][HD] bf16 V.
// grid (KVH, sequences), block 512, two workgroups per CU.
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline int gqa_tp(int lds_T) { return ((lds_T + 63) / 64) * 64 + 64; }
__host__ __device__ inline size_t gqa_lds_bytes(int lds_T, int hd, int G) { return (size_t)G * gqa_tp(lds_T) * 12 + (size_t)G * hd * 4 + 512 + 4 * 32 * (size_t)hd * 2; }
typedef float f32x2_t __attribute__((ext_vector_type(2)));
// adder side of attn_gqa_kernel: a quarter of a V chunk (8 positions of the lane's bf16 pair, ring buffer (q / 4) & 3) and its 8 p values
template <int HD> DEVINL void gqa_read_piece(uint32_t (&w)[8], float4 (&pq)[2], const char* vl, const float* pg, int q) {
    const char* vb = vl + ((q >> 2) & 3) * (32 * HD * 2) + (q & 3) * (8 * HD * 2);
    pq[0] = *(const float4*)(pg + q * 8); pq[1] = *(const float4*)(pg + q * 8 + 4);           // (wave-uniform addresses: broadcast reads)
#pragma unroll
    for (int u = 0; u < 8; u++) w[u] = *(const uint32_t*)(vb + u * (HD * 2));
}
DEVINL void gqa_add_piece(f32x2_t& a, const uint32_t (&w)[8], const float4 (&pq)[2]) {      // acc += p_j * v[j][d], j ascending: multiply, then add (:508-514)
#pragma unroll
    for (int k = 0; k < 2; k++) {
        a += f32x2_t{pq[k].x, pq[k].x} * f32x2_t{bf_lo(w[4 * k]), bf_hi(w[4 * k])};
        a += f32x2_t{pq[k].y, pq[k].y} * f32x2_t{bf_lo(w[4 * k + 1]), bf_hi(w[4 * k + 1])};
        a += f32x2_t{pq[k].z, pq[k].z} * f32x2_t{bf_lo(w[4 * k + 2]), bf_hi(w[4 * k + 2])};
        a += f32x2_t{pq[k].w, pq[k].w} * f32x2_t{bf_lo(w[4 * k + 3]), bf_hi(w[4 * k + 3])};
    }
}
template <int HD, int G> __global__ __launch_bounds__(512, 4) void attn_gqa_kernel(AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NK = HD / 8, NT = 512, NPOS = 256, VC = 32;      // a scores pass: 256 positions x 2 head pairs; V chunks of 32 positions
    static_assert(G == 4 && HD == 128, "two head pairs; one V unit per thread and chunk; two adder waves");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kvh = (int)blockIdx.x, i = (int)blockIdx.y;      // (dispatch order: the eight KV heads of a sequence go to the eight XCDs)
    const BatchTab* const bt = p.btab;
    const int seq_len = bt->seq_len[i], T = bt->st[i]->pos + 1, Tp = gqa_tp(p.lds_T);
    double* e = (double*)smem;                                  // [G][Tp]
    float* pw = (float*)(smem + (size_t)G * Tp * 8);            // [G][Tp]
    float* qi = (float*)(smem + (size_t)G * Tp * 12);           // [G / 2][HD][2]: (head 2a, head 2a+1) pairs
    double* zb = (double*)(smem + (size_t)G * Tp * 12 + (size_t)G * HD * 4);     // per head: 4 wave partials | - | Z | flag
    uint16_t* vs = (uint16_t*)(smem + (size_t)G * Tp * 12 + (size_t)G * HD * 4 + 512);   // ring [4][VC][HD] bf16
    const uint32_t row_bytes = (uint32_t)p.KVH * HD * 2;
    const uint4* kbase = (const uint4*)p.bkv->ck[i] + (size_t)kvh * NK * seq_len;
    const uint16_t* vbase = p.bkv->cv[i] + (size_t)kvh * HD;
    const int jl = tid & (NPOS - 1), hp = wave >> 2, pwv = wave & 3;       // position inside a pass, head pair, wave inside the pair
    const int nch = (T + VC - 1) / VC, Tc = nch * VC;
#define GQA_STAMP(n) do { if (p.dbg && blockIdx.x == 3 && blockIdx.y == gridDim.y / 2 && lane == 0) p.dbg[wave * 16 + (n)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
    GQA_STAMP(0);

    // q of the G heads (contiguous in the row) as head pairs, and this thread's K row of the first pass
    const uint16_t q16 = p.q[((size_t)i * p.H + (size_t)kvh * G) * HD + tid];
    uint4 ka[NK];
    if (pwv * 64 < T) attn_load_k<NK>(ka, kbase, seq_len, jl < T ? jl : T - 1);
    { const int g = tid >> 7, d = tid & (HD - 1); qi[((g >> 1) * HD + d) * 2 + (g & 1)] = bf_wide(q16); }
    __syncthreads();
    GQA_STAMP(1);
    // ---- scores: one cached position per thread and pass, both heads of the pair over the same K row (llamatransformer.go:456-473)
    const float* qh = qi + hp * HD * 2;
    for (int j0 = 0; j0 < T; j0 += NPOS) {
        const int j = j0 + jl;
        if (j0 + pwv * 64 >= T) continue;                       // (wave-uniform: a wave past the end of the row leaves the issue slots to the others)
        if (j0 > 0) attn_load_k<NK>(ka, kbase, seq_len, j < T ? j : T - 1);
        f32x2_t acc = {0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < NK; c++) {                          // MatMul q.k, d ascending (operations_matmul.go:37-55): acc = fma(q_d, k_d, acc) per head
            const float4 qa = *(const float4*)(qh + c * 16), qb = *(const float4*)(qh + c * 16 + 4), qc = *(const float4*)(qh + c * 16 + 8), qd = *(const float4*)(qh + c * 16 + 12);
            const uint4 k = ka[c];
            float kk;
            kk = bf_lo(k.x); acc = __builtin_elementwise_fma(f32x2_t{qa.x, qa.y}, f32x2_t{kk, kk}, acc);
            kk = bf_hi(k.x); acc = __builtin_elementwise_fma(f32x2_t{qa.z, qa.w}, f32x2_t{kk, kk}, acc);
            kk = bf_lo(k.y); acc = __builtin_elementwise_fma(f32x2_t{qb.x, qb.y}, f32x2_t{kk, kk}, acc);
            kk = bf_hi(k.y); acc = __builtin_elementwise_fma(f32x2_t{qb.z, qb.w}, f32x2_t{kk, kk}, acc);
            kk = bf_lo(k.z); acc = __builtin_elementwise_fma(f32x2_t{qc.x, qc.y}, f32x2_t{kk, kk}, acc);
            kk = bf_hi(k.z); acc = __builtin_elementwise_fma(f32x2_t{qc.z, qc.w}, f32x2_t{kk, kk}, acc);
            kk = bf_lo(k.w); acc = __builtin_elementwise_fma(f32x2_t{qd.x, qd.y}, f32x2_t{kk, kk}, acc);
            kk = bf_hi(k.w); acc = __builtin_elementwise_fma(f32x2_t{qd.z, qd.w}, f32x2_t{kk, kk}, acc);
        }
        if (j < T) {                                            // / sqrt(hd) :464, exp impl:498: tabulated over the raw bf16 score
            const double e0 = p.exp_tab[bf_trunc(acc.x)], e1 = p.exp_tab[bf_trunc(acc.y)];
            e[(hp * 2) * Tp + j] = e0; e[(hp * 2 + 1) * Tp + j] = e1;
        }
    }
    GQA_STAMP(2);
    // V chunks (32 positions x 256 B, raw bf16): staged by waves 4..7, two 16-byte units per thread and chunk, rows clamped to T-1 (p == +0
    // there).  Four chunks in flight in registers + a ring of four LDS buffers: the adders (waves 0..3) never wait for memory.  Hand-counted
    // asm ring (hipcc drains vmcnt(0) around loop-carried register prefetch): RING_LOAD / RING_RETIRE, checked by tools/isa_audit.py.
    const bool stager = wave >= 4;
    const int st_t = tid - 256;
    u32x4 s0[2], s1[2], s2[2], s3[2];
#define GQA_VLOAD(c, R_) do { int ja_ = (c) * VC + (st_t >> 4), jb_ = ja_ + 16; ja_ = ja_ < T ? ja_ : T - 1; jb_ = jb_ < T ? jb_ : T - 1; \
        const char* aa_ = (const char*)vbase + ((size_t)(uint32_t)ja_ * row_bytes + (uint32_t)(st_t & 15) * 16u); \
        const char* ab_ = (const char*)vbase + ((size_t)(uint32_t)jb_ * row_bytes + (uint32_t)(st_t & 15) * 16u); \
        asm volatile("global_load_dwordx4 %0, %1, off ; RING_LOAD" : "=&v"(R_[0]) : "v"(aa_) : "memory"); \
        asm volatile("global_load_dwordx4 %0, %1, off ; RING_LOAD" : "=&v"(R_[1]) : "v"(ab_) : "memory"); } while (0)
#define GQA_VSTORE(c, R_, N_) do { asm volatile("s_waitcnt vmcnt(%2) ; RING_RETIRE %0 %1" : "+v"(R_[0]), "+v"(R_[1]) : "n"(N_) : "memory"); \
        char* dst_ = (char*)vs + ((c) & 3) * (VC * HD * 2) + (st_t >> 4) * (HD * 2) + (st_t & 15) * 16; \
        *(u32x4*)dst_ = R_[0]; *(u32x4*)(dst_ + 16 * HD * 2) = R_[1]; } while (0)
    if (stager) { GQA_VLOAD(0, s0); GQA_VLOAD(1, s1); GQA_VLOAD(2, s2); GQA_VLOAD(3, s3); }     // they land during the denominators
    for (int j = T + tid; j < ((T + 31) & ~31); j += NT) {      // zero padding: the serial walk runs whole groups of 32
#pragma unroll
        for (int g = 0; g < G; g++) e[g * Tp + j] = 0.0;
    }
    __syncthreads();
    GQA_STAMP(3);
    // ---- softmax denominators: tree estimate + certified p_j per head (header of attn_long_pv_kernel)
    {
        double part[2] = {0.0, 0.0};
        for (int j = jl; j < T; j += NPOS) { part[0] += e[(hp * 2) * Tp + j]; part[1] += e[(hp * 2 + 1) * Tp + j]; }
#pragma unroll
        for (int g = 0; g < 2; g++) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part[g] += __shfl_xor(part[g], o);
            if (lane == 0) zb[(hp * 2 + g) * 10 + pwv] = part[g];
        }
        if (tid < G) *(int*)(zb + tid * 10 + 9) = 0;
    }
    __syncthreads();
    {
#pragma unroll 1
        for (int g = hp * 2; g < hp * 2 + 2; g++) {             // (not unrolled: inlined copies of cert_p cost registers)
            const double* z4 = zb + g * 10;
            const double zt = (z4[0] + z4[1]) + (z4[2] + z4[3]);
            const CertZ cz = cert_z(zt, T);
            int bad = p.force_zseq;
            for (int j = jl; j < Tc; j += NPOS) pw[g * Tp + j] = j < T ? cert_p(e[g * Tp + j], cz, bad) : 0.0f;   // impl:506 + ToBFloat16 :493; +0 up to the chunk
            if (bad) *(int*)(zb + g * 10 + 9) = 1;
        }
    }
    GQA_STAMP(4);
    if (stager) {                                               // chunks 0..2 into the ring, chunks 4..6 in flight
        GQA_VSTORE(0, s0, 6); GQA_VLOAD(4, s0);
        GQA_VSTORE(1, s1, 6); GQA_VLOAD(5, s1);
        GQA_VSTORE(2, s2, 6); GQA_VLOAD(6, s2);
    }
    __syncthreads();
    GQA_STAMP(5);
    {
        int flags = 0;
#pragma unroll
        for (int g = 0; g < G; g++) flags |= *(const int*)(zb + g * 10 + 9) << g;
        if (flags) {                                            // (block-uniform) a head that could not be certified: the reference's serial sum, on wave g
            // (the serial walk wants 64 registers: the stagers' V rows must have LANDED before anything may be spilled around it)
            if (stager) asm volatile("s_waitcnt vmcnt(0) ; RING_RETIRE %0 %1 %2 %3 %4 %5 %6 %7" : "+v"(s0[0]), "+v"(s0[1]), "+v"(s1[0]), "+v"(s1[1]), "+v"(s2[0]), "+v"(s2[1]), "+v"(s3[0]), "+v"(s3[1]) :: "memory");
            if (wave < G && ((flags >> wave) & 1)) {
                const double z = attn_zseq_wave(e + wave * Tp, T);
                if (lane == 0) { zb[wave * 10 + 8] = z; if (p.zseq_count) atomicAdd(p.zseq_count, 1); }
            }
            __syncthreads();
#pragma unroll 1
            for (int g = 0; g < G; g++) {
                if (!((flags >> g) & 1)) continue;
                const double z = zb[g * 10 + 8];
                for (int j = tid; j < T; j += NT) pw[g * Tp + j] = bf_wide(bf_trunc((float)(e[g * Tp + j] / z)));
            }
            __syncthreads();
        }
    }
    // ---- PV: out[g][d] = trunc(sum_{j ascending} p[g][j] * v[j][d]) (:508-514).  Wave g < 4 adds head g, lane l the dims 2l, 2l+1: one
    // ds_read_b32 (a bf16 pair), two unpack operations, v_pk_mul_f32, v_pk_add_f32 per position.  One barrier per chunk: at step c the adders
    // read ring buffer c & 3 while the stagers write chunk c+3 (into the buffer read at step c-1) and put chunk c+7 in flight.
    f32x2_t a0 = {0.0f, 0.0f};
    if (stager) {
#define GQA_SSTEP(c, R_) do { if ((c) < nch) { GQA_VSTORE((c) + 3, R_, 6); GQA_VLOAD((c) + 7, R_); __syncthreads(); } } while (0)
        for (int c = 0; c < nch; c += 4) { GQA_SSTEP(c, s3); GQA_SSTEP(c + 1, s0); GQA_SSTEP(c + 2, s1); GQA_SSTEP(c + 3, s2); }
#undef GQA_SSTEP
        asm volatile("s_waitcnt vmcnt(0) ; RING_RETIRE_ALL" ::: "memory");    // prefetches past the last chunk
        GQA_STAMP(6);
        return;                                                 // (the roles never join again: the ring registers are dead on the adders' path)
    }
    {
        // (a quarter chunk -- 8 positions: 8 V words + 2 x 4 p -- is read from the LDS while the quarter before it is added: left to hipcc, every
        //  ds_read sat right in front of its use, ~100 cycles of LDS latency per two positions.  The first quarter of chunk c+1 is read during
        //  step c: chunks up to c+2 are complete then.)
        const float* pg = pw + wave * Tp;
        const char* vl = (const char*)vs + lane * 4;
        uint32_t wA[8], wB[8]; float4 pA[2], pB[2];
        gqa_read_piece<HD>(wA, pA, vl, pg, 0);
        for (int q = 0; q < 4 * nch; q += 4) {
            gqa_read_piece<HD>(wB, pB, vl, pg, q + 1);
            __builtin_amdgcn_sched_barrier(0);
            gqa_add_piece(a0, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            gqa_read_piece<HD>(wA, pA, vl, pg, q + 2);
            __builtin_amdgcn_sched_barrier(0);
            gqa_add_piece(a0, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            gqa_read_piece<HD>(wB, pB, vl, pg, q + 3);
            __builtin_amdgcn_sched_barrier(0);
            gqa_add_piece(a0, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            if (q + 4 < 4 * nch) gqa_read_piece<HD>(wA, pA, vl, pg, q + 4);
            __builtin_amdgcn_sched_barrier(0);
            gqa_add_piece(a0, wB, pB);
            __syncthreads();
        }
    }
    GQA_STAMP(6);
#undef GQA_STAMP
#undef GQA_VLOAD
#undef GQA_VSTORE
    {
        const int h = kvh * G + wave, d = 2 * lane;
        if (p.out_xt) { uint16_t* o = p.out_xt + xt_group(i, p.H * HD); o[xt_index(i & 15, h * HD + d)] = bf_trunc(a0.x); o[xt_index(i & 15, h * HD + d + 1)] = bf_trunc(a0.y); }     // column batches: the B-operand layout of the wo product
        else *(uint32_t*)(p.out + ((size_t)i * p.H + h) * HD + d) = (uint32_t)bf_trunc(a0.x) | ((uint32_t)bf_trunc(a0.y) << 16);       // [S, H*hd]
    }
}

// ------------------------------------------------------------------------------------------------
// Long-context decode attention (S == 1, thousands of cached positions): the same arithmetic as attn_exact_kernel, spread over the
// chip.  attn_exact_kernel is one workgroup per head: at T = 4100 its scores take 12 us, the serial f64 Z chain 16 us and PV 31 us
// (one CU pulls a whole head's V rows).  Here:
//   attn_long_scores_kernel  grid (H, ceil(seq_len / 256)): one cached position per thread, the 128-long q.k chain, /sqrt(hd), exp
//       in f64 -> e_buf[h][j]; plus a tree sum of the block's 256 values -> z_part (an ESTIMATE of the row sum, see below);
//   attn_long_pv_kernel      grid (H, hd / 16): p_j for the whole row, then out[d] = sum_j p_j v[j][d] for 16 output dims with the
//       role split of the short kernel (four producer waves: V rows -> exact products in an LDS ring, one adder wave: one chain per
//       lane, j ascending).  256 workgroups instead of 32, each pulls 32 B per position instead of 256 B.
// Z WITHOUT the serial chain, still bit-exact:  the reference adds the T exponentials one by one in f64 (operations_impl.go:492-499).
// Every way of summing T non-negative doubles is within (T-1) u of the exact sum (u = 2^-53), so the tree estimate Zt and the
// reference's Zs differ by less than eps = 4 T u relatively -- and p_j = trunc_bf16(f32(e_j / Z)) is a MONOTONE step function of Z
// whose steps are 2^-8 wide relative to p.  So p_j is evaluated with Zt and CERTIFIED: the f64 quotient q must not lie within
// 4 T + 4 f64 ulps of the one point per bf16 cell where the result changes (the f32 rounding boundary just below a bf16 grid
// point: low 45 mantissa bits == 2^45 - 2^28); quotients in the f32 denormal range are certified by evaluating the step function at
// both ends of [Zt (1 - eps), Zt (1 + eps)].  If every p_j of the row is certified, they equal the reference's bits whatever Zs is
// (monotonicity); otherwise -- about once in 10^9 elements -- the workgroup walks the reference's serial sum itself (16 us, exact)
// and re-evaluates.  force_zseq runs that path always (tests/test_gpu_configs.py compares both with the oracle).
// ------------------------------------------------------------------------------------------------
constexpr int ALS_NT = 256;                                  // positions per scores workgroup
template <int NK> DEVINL double attn_score_value(const uint4 (&k)[NK], const float* qf, float divisor) {   // attn_score for S == 1 (no mask)
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < NK; c++) {                           // MatMul q.k, d ascending (operations_matmul.go:37-55)
        const float4 xa = *(const float4*)(qf + c * 8), xb = *(const float4*)(qf + c * 8 + 4);
        acc = mac8(acc, xa, xb, k[c]);
    }
    uint16_t s = bf_trunc(acc);
    s = bf_trunc(__fdiv_rn(bf_wide(s), divisor));           // DivToScalar :464
    return exp((double)bf_wide(s));                          // Softmax impl:498
}
// BATCH (batched decode and the verify passes of the speculative loop, grid.z = the sequences): one more grid dimension over the same program.
// Sequence s takes its position from its own StepState (btab), its caches from bkv and its OWN cache length (the K layout's stride, the
// arrays' ends) from btab->seq_len[s] -- the members of a batch may differ in capacity; p.seq_len is then the LARGEST member's (maxT): the
// stride of the e_buf [n][H][maxT] / z_part [n][H][ceil(maxT/256)] rows, the size of the scores grid and of the PV kernels' LDS arrays.
// A sequence at a short position leaves most of its blocks at once (uniform return); a frozen one (stop id) recomputes its last step.
// The position is clamped into the sequence's cache (a state word the batch never set cannot take a read past an array's end).
// The XCD remap acts inside a z-slice and the V touch carries over unchanged (each sequence's group touches its own rows).
struct AlSeq { int seq_len, T; const uint16_t* ck; const uint16_t* cv; size_t row; };       // row: (sequence, head) row of q / e_buf / z_part / out
DEVINL AlSeq al_seq(const AttnParams& p, int h) {
    AlSeq a;
    const int s = blockIdx.z;
    a.seq_len = p.btab->seq_len[s]; a.ck = p.bkv->ck[s]; a.cv = p.bkv->cv[s]; a.row = (size_t)s * p.H + h;
    const int T = p.btab->st[s]->pos + 1;
    a.T = T < 1 ? 1 : (T > a.seq_len ? a.seq_len : T);
    return a;
}
// (accessors: the S == 1 instantiations read the launch parameters where they always did -- their code is unchanged by the BATCH forms)
template <bool BATCH> DEVINL int al_len(const AttnParams& p, const AlSeq& a) { if constexpr (BATCH) return a.seq_len; else return p.seq_len; }
template <bool BATCH> DEVINL int al_T(const AttnParams& p, const AlSeq& a) { if constexpr (BATCH) return a.T; else return p.st->pos + 1; }
template <bool BATCH> DEVINL const uint16_t* al_ck(const AttnParams& p, const AlSeq& a) { if constexpr (BATCH) return a.ck; else return p.cache_k; }
template <bool BATCH> DEVINL const uint16_t* al_cv(const AttnParams& p, const AlSeq& a) { if constexpr (BATCH) return a.cv; else return p.cache_v; }
template <bool BATCH> DEVINL size_t al_row(const AlSeq& a, int h) { if constexpr (BATCH) return a.row; else return (size_t)h; }
// the batched step's two destinations (the end of attn_exact_kernel): the B-operand layout of the wo product (column forms, 17..32 "groups") or rows
DEVINL void al_store(const AttnParams& p, int h, int hd_, int d, float acc) {
    const int s = blockIdx.z;
    if (p.out_xt) p.out_xt[xt_group(s, p.H * hd_) + xt_index(s & 15, h * hd_ + d)] = bf_trunc(acc);
    else p.out[((size_t)s * p.H + h) * hd_ + d] = bf_trunc(acc);
}
template <int HD, bool BATCH = false> __global__ __launch_bounds__(ALS_NT) void attn_long_scores_kernel(AttnParams p) {
    constexpr int NK = HD / 8;
    __shared__ __attribute__((aligned(16))) float qf[HD];
    __shared__ double wsum[ALS_NT / 64];
    const int tid = threadIdx.x;
    int h, blk; xcd_head_block(h, blk);
    [[maybe_unused]] AlSeq sq{}; if constexpr (BATCH) sq = al_seq(p, h);      // (BATCH: p.seq_len = the largest member's -- row strides, LDS layout; al_len = this sequence's array ends)
    const int T = al_T<BATCH>(p, sq), j0 = blk * ALS_NT;
    if (j0 >= T) return;                                     // (uniform: the grid is sized for seq_len, the captured graph serves every T)
    const int kvh = h / (p.H / p.KVH);
    const uint4* kbase = (const uint4*)al_ck<BATCH>(p, sq) + (size_t)kvh * NK * al_len<BATCH>(p, sq);
    const uint16_t* q = p.q + al_row<BATCH>(sq, h) * HD;
    const uint16_t q16 = q[tid < HD ? tid : 0];
    const int j = j0 + tid;
    uint4 k[NK];
    attn_load_k<NK>(k, kbase, al_len<BATCH>(p, sq), j < T ? j : T - 1);
    // round 6 (AttnParams.touch): the query heads of a GQA group touch the V rows of their block for the PV launch that follows -- these workgroups sit on the
    // XCD whose L2 the PV workgroups of the group will read (xcd_head_block), so the lines land where they are needed (a touch from another XCD lands in the wrong L2, and the
    // memory-side cache is barely faster than HBM: profiles/r06_kv_touch_ab.log).  Issued BEHIND the K rows.
    // configs[2] step: attention 25.5 -> 23.7 us per layer (profiles/r06_attn_touch_ab.log)
    // One plain load per thread, straight-line (a `volatile` access compiles to a system-scope load with a full vmcnt(0) wait behind it, a conditional one makes the
    // destination a phi the compiler may copy in flight): the G heads of the group share the block's 256 * HD / 64 lines, the surplus heads repeat the first ones' (L2 hits);
    // the destination register is held until the end of the kernel by the empty asm below, the data is never looked at.
    unsigned vt;
    {
        constexpr int LPR = HD / 64 > 0 ? HD / 64 : 1;       // 128-byte lines per (row, kv head)
        const int l = ((h % (p.H / p.KVH)) % LPR) * ALS_NT + tid;
        int jl = j0 + l / LPR; jl = jl < T ? jl : T - 1;
        const char* va = (const char*)al_cv<BATCH>(p, sq) + ((size_t)jl * p.KVH + kvh) * HD * 2 + (l % LPR) * 128;
        va = p.touch ? va : (const char*)kbase;              // (off: a line this workgroup reads anyway)
        asm volatile("global_load_dword %0, %1, off ; RING_LOAD (never retired: tools/isa_audit.py flags any later use of the register)" : "=v"(vt) : "v"(va));
    }
    if (tid < HD) qf[tid] = bf_wide(q16);
    __syncthreads();
    double ev = 0.0;
    if (j < T) { ev = attn_score_value<NK>(k, qf, p.divisor); p.e_buf[al_row<BATCH>(sq, h) * p.seq_len + j] = ev; }
    // tree sum of the block (fixed shape: deterministic); only ever used as an estimate with a rigorous error bound
    ev = wave_sum_f64(ev);
    if ((tid & 63) == 0) wsum[tid >> 6] = ev;
    __syncthreads();
    if (tid == 0) p.z_part[al_row<BATCH>(sq, h) * ((p.seq_len + ALS_NT - 1) / ALS_NT) + blk] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    asm volatile("" :: "v"(vt));                              // the touch's destination stays allocated up to here
}

constexpr int ALP_DS = 16;                                   // output dims per workgroup
constexpr int ALP_BATCH = 512;                               // cached positions per PV batch (one barrier per batch) = four 128-position chunks
constexpr int ALP_NT = 512;                                  // waves 0..3: adders (4 dims each, one per DPP row); waves 4..7: producers
constexpr int ALP_SLOT = ALP_DS * ALP_BATCH;                 // floats per ring slot: [dim][chunk][half][position % 16][4]
constexpr int ALP_EU = 12;                                   // e_j per thread and round
__host__ __device__ inline size_t alp_lds_bytes(int seq_len) { return (size_t)((seq_len + ALP_BATCH - 1) / ALP_BATCH + 1) * ALP_BATCH * 4 + 2 * (size_t)ALP_SLOT * 4 + 64; }
// The p_j array in front of the ring: one float per cached position (+ a batch of zeros) while that fits the 160 KB of a CU's LDS -- contexts of up to 23552
// positions, every context lnb_ctx_create accepts: the layout and the size they always had.  Beyond (lnb_ctx_create_long) the array is a CONSTANT three
// batches: only the eager body reads it, attn_long_pv2_kernel runs that body for T <= 2 * ALP_BATCH (Tpad = 3 batches), and the lazy body evaluates p_j
// where it multiplies the V row.  The launcher never pairs the constant layout with attn_long_pv_kernel (the eager body at every T).
constexpr int ALP_PW_LONG = 3 * ALP_BATCH;
__host__ __device__ inline bool alp_per_position(int seq_len) { return alp_lds_bytes(seq_len) <= (size_t)160 * 1024; }
__host__ __device__ inline int alp_pw_floats(int seq_len) { return alp_per_position(seq_len) ? ((seq_len + ALP_BATCH - 1) / ALP_BATCH + 1) * ALP_BATCH : ALP_PW_LONG; }
__host__ __device__ inline size_t alp_layout_bytes(int seq_len) { return (size_t)alp_pw_floats(seq_len) * 4 + 2 * (size_t)ALP_SLOT * 4 + 64; }
DEVINL float alp_p(double e, double z) { return bf_wide(bf_trunc((float)(e / z))); }     // impl:506 + ToBFloat16 :493
template <int HD, bool BATCH = false, bool TIMING = false> DEVINL void alp_eager_body(const AttnParams& p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int h, ds; xcd_head_block(h, ds);
    [[maybe_unused]] AlSeq sq{}; if constexpr (BATCH) sq = al_seq(p, h);      // (BATCH: p.seq_len = the largest member's -- row strides, LDS layout; al_len = this sequence's array ends)
    const int T = al_T<BATCH>(p, sq), nblk = (T + ALS_NT - 1) / ALS_NT, nbatch = (T + ALP_BATCH - 1) / ALP_BATCH;
    const int Tpad = (nbatch + 1) * ALP_BATCH;               // (+ one batch of zeros: the producers run ahead)
    float* pw = (float*)smem;                                // [Tpad] p_j (+0 beyond T)
    float* ring = (float*)(smem + (size_t)p.pw_floats * 4);   // [2][ALP_SLOT] products, behind the p_j array (alp_pw_floats: the launcher's choice)
    double* zsh = (double*)(ring + 2 * ALP_SLOT);
    const double* E = p.e_buf + al_row<BATCH>(sq, h) * p.seq_len;
    const int kvh = h / (p.H / p.KVH);
#define ALP_STAMP(n) do { if (LNB_DBG && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0 && (wave & 3) == 0) p.dbg[(wave >> 2) * 16 + (n)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
    ALP_STAMP(0);
    // ---- everything that depends only on addresses goes in flight first, oldest-needed first (waits retire in issue order): the first
    // round of e_j, the per-block partial sums, then the producers' first three batches of V rows (HBM: the slowest, needed last)
    // (clamped to the ARRAY ends, not to T: the addresses must not wait for the position word to arrive; what lies past T is not used)
    double ev[ALP_EU];
#pragma unroll
    for (int u = 0; u < ALP_EU; u++) { const int j = u * ALP_NT + tid; ev[u] = E[j < al_len<BATCH>(p, sq) ? j : al_len<BATCH>(p, sq) - 1]; }
    const int nblk_max = (p.seq_len + ALS_NT - 1) / ALS_NT;
    const double* zp = p.z_part + al_row<BATCH>(sq, h) * nblk_max;
    double zmine = zp[lane < nblk_max ? lane : nblk_max - 1];
    const uint16_t* vbase = al_cv<BATCH>(p, sq) + (size_t)kvh * HD + (size_t)ds * ALP_DS;
    const size_t vrow = (size_t)p.KVH * HD;
    const int pl = tid & 255, half8 = pl & 1, prow = pl >> 1;                // producers: 128 positions x two 8-dim halves per round, 4 rounds per batch
    auto load = [&](uint4 (&v)[4], int b) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            int j = b * ALP_BATCH + r * 128 + prow; j = j < T ? j : T - 1;
            v[r] = *(const uint4*)(vbase + (size_t)j * vrow + half8 * 8);
        }
    };
    uint4 v0[4], v1[4], v2[4], v3[4];
    if (wave >= 4) { load(v0, 0); load(v1, 1); load(v2, 2); }
    // ---- Z estimate: the per-block tree sums, added in block order (same value in every thread): one partial per lane, a register walk
    double zt = 0.0;
    for (int b0 = 0; b0 < nblk; b0 += 64) {
        if (b0) zmine = zp[b0 + lane < nblk ? b0 + lane : nblk - 1];
        const int nb = nblk - b0 < 64 ? nblk - b0 : 64;
        const long long zbits = __double_as_longlong(zmine);
        for (int b = 0; b < nb; b++) {                       // v_readlane (a shuffle is an LDS round trip per step: 4 k cycles for 17 blocks)
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)zbits, b), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(zbits >> 32), b);
            zt += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        }
    }
    // ---- p_j with the estimate, certified (header comment).  The quotient is formed as e * (1 / Zt): within 2 ulps of the correctly
    // rounded e / Zt, which the certification band absorbs (its half-width 4 T + 12 ulps instead of 4 T + 4)
    static_assert(LNB_SEQ_MAX < (1 << 20), "the certification band 4T + 12 is sized for T < 2^20");
    const unsigned delta32 = 4u * (unsigned)T + 12u;         // (T < 2^20: far below the 2^28 between a cell's step point and its end)
    const double epsr = (double)(4 * T + 8) * 1.1102230246251565e-16;          // relative half-width of the interval that holds the reference's Z
    const double zlo = zt * (1.0 - epsr), zhi = zt * (1.0 + epsr), rzt = 1.0 / zt;
    int bad = p.force_zseq;
    int* const flag = (int*)(zsh + 1);                       // (own flag instead of __syncthreads_or: its library reduction takes static LDS)
    if (tid == 0) *flag = 0;
    __syncthreads();
    for (int j0 = 0; j0 < Tpad; j0 += ALP_EU * ALP_NT) {
        if (j0 != 0) {
#pragma unroll
            for (int u = 0; u < ALP_EU; u++) { const int j = j0 + u * ALP_NT + tid; ev[u] = E[j < T ? j : T - 1]; }
        }
#pragma unroll
        for (int u = 0; u < ALP_EU; u++) {
            const int j = j0 + u * ALP_NT + tid;
            if (j >= Tpad) continue;
            float pj = 0.0f;
            if (j < T) {
                const double e = ev[u];
                const double q = e * rzt;
                pj = bf_wide(bf_trunc((float)q));
                // the band test on the two 32-bit halves of q (64-bit integer code made this loop the longest phase of the kernel): the low 45
                // mantissa bits lie within delta of 2^45 - 2^28  <=>  bits 32..44 are all ones and the low word is within delta of 0xF0000000
                const unsigned qh = (unsigned)__double2hiint(q), ql = (unsigned)__double2loint(q);
                const unsigned eq = (qh >> 20) & 0x7FFu;
                if (eq - 897u <= 126u) {                     // f32-normal quotient (2^-126 <= q < 2): distance from the step point of its bf16 cell
                    if ((qh & 0x1FFFu) == 0x1FFFu && ql - (0xF0000000u - delta32) <= 2u * delta32) bad = 1;
                } else if (q != 0.0 && (alp_p(e, zlo) != alp_p(e, zhi) || pj != alp_p(e, zlo))) bad = 1;   // f32 denormals: both ends of the interval
            }
            pw[j] = pj;
        }
    }
    ALP_STAMP(1);
    if (bad) *flag = 1;
    __syncthreads();
    ALP_STAMP(2);
    if (*flag) {
        // the reference's serial sum, j ascending, f64 (operations_impl.go:492-499): one wave, 16 values in flight ahead of the adds
        if (wave == 0) {
            double z = 0.0;
            for (int j0 = 0; j0 < T; j0 += 16) {
                double v[16];
#pragma unroll
                for (int u = 0; u < 16; u++) v[u] = E[j0 + u < T ? j0 + u : T - 1];
#pragma unroll
                for (int u = 0; u < 16; u++) z += (j0 + u < T) ? v[u] : 0.0;
            }
            if (lane == 0) { zsh[0] = z; if (p.zseq_count && ds == 0) atomicAdd(p.zseq_count, 1); }
        }
        __syncthreads();
        const double z = zsh[0];
        for (int j0 = 0; j0 < T; j0 += ALP_EU * ALP_NT) {
#pragma unroll
            for (int u = 0; u < ALP_EU; u++) { const int j = j0 + u * ALP_NT + tid; ev[u] = E[j < T ? j : T - 1]; }
#pragma unroll
            for (int u = 0; u < ALP_EU; u++) { const int j = j0 + u * ALP_NT + tid; if (j < T) pw[j] = alp_p(ev[u], z); }
        }
        __syncthreads();
    }
    // ---- PV: out[d] = trunc(sum_{j ascending} p_j * v[j][d]) for d = ds*16 .. +15 (llamatransformer.go:504-514), the row-broadcast chain
    // of rowcast_kernel: an adder wave owns 4 output dims, one per DPP row of 16 lanes; lane (q, jj) receives the exact products of dim q at
    // the positions j = jj (mod 16) -- eight per 128-position chunk, two 16 B LDS reads -- and every lane of the row adds the 16 lanes'
    // products in position order with v_add_f32_dpp row_newbcast (chain128): 6 cycles per position instead of 8.7 for an LDS-fed chain.
    // Iteration it: the producers turn batch it (rows in registers, loaded three batches ahead) into products in ring[it & 1]
    // ([dim][chunk][half][position % 16][4]: both the scattered 4 B writes and the 16 B reads are conflict-free); the adders walk batch
    // it - 1.  Positions past T carry p == +0 (products +-0, acc is never -0).
    float acc = 0.0f;
    if (wave < 4) {
        const int d = 4 * wave + (lane >> 4), jj = lane & 15;
        ALP_STAMP(3);
        for (int it = 0; it <= nbatch; it++) {
            if (it == 2) ALP_STAMP(4);
            if (it > 0) {
                const float* src = ring + (size_t)((it - 1) & 1) * ALP_SLOT + (size_t)d * ALP_BATCH + jj * 4;
                float4 a0 = *(const float4*)(src), a1 = *(const float4*)(src + 64);
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    float pr[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                    if (c < 3) { a0 = *(const float4*)(src + (c + 1) * 128); a1 = *(const float4*)(src + (c + 1) * 128 + 64); }   // in flight behind the 128 adds
                    asm volatile("" : "+v"(pr[0]), "+v"(pr[1]), "+v"(pr[2]), "+v"(pr[3]), "+v"(pr[4]), "+v"(pr[5]), "+v"(pr[6]), "+v"(pr[7]));
                    __builtin_amdgcn_sched_barrier(0);
                    chain128(acc, pr);
                }
            }
            __syncthreads();
        }
        ALP_STAMP(5);
        if (jj == 0) { if constexpr (BATCH) al_store(p, h, HD, ds * ALP_DS + d, acc); else p.out[(size_t)h * HD + ds * ALP_DS + d] = bf_trunc(acc); }
        ALP_STAMP(6);
    } else {
        auto produce = [&](const uint4 (&v)[4], int b) {
            float* dst = ring + (size_t)(b & 1) * ALP_SLOT + (size_t)(half8 * 8) * ALP_BATCH + ((prow >> 6) & 1) * 64 + (prow & 15) * 4 + ((prow >> 4) & 3);
#pragma unroll
            for (int r = 0; r < 4; r++) {                    // round r = chunk r of the batch; position prow of it: e = prow >> 4, jj = prow & 15
                const float pj = pw[b * ALP_BATCH + r * 128 + prow];
                const uint4 w = v[r];                        // exact products: 8-bit x 8-bit significands
                float* q = dst + r * 128;
                q[0 * ALP_BATCH] = pj * bf_lo(w.x); q[1 * ALP_BATCH] = pj * bf_hi(w.x); q[2 * ALP_BATCH] = pj * bf_lo(w.y); q[3 * ALP_BATCH] = pj * bf_hi(w.y);
                q[4 * ALP_BATCH] = pj * bf_lo(w.z); q[5 * ALP_BATCH] = pj * bf_hi(w.z); q[6 * ALP_BATCH] = pj * bf_lo(w.w); q[7 * ALP_BATCH] = pj * bf_hi(w.w);
            }
        };
        auto step = [&](int it, const uint4 (&cur)[4], uint4 (&nxt)[4]) {
            if (it <= nbatch) {                              // (uniform; one barrier per iteration, like the adders)
                if (it < nbatch) { load(nxt, it + 3); produce(cur, it); }
                __syncthreads();
            }
        };
        ALP_STAMP(3);
        for (int it = 0; it <= nbatch; it += 4) { step(it, v0, v3); if (it == 0) ALP_STAMP(4); step(it + 1, v1, v0); step(it + 2, v2, v1); step(it + 3, v3, v2); }
        ALP_STAMP(5); ALP_STAMP(6);
    }
}

// TIMING: the instantiations with the phase stamps (AttnParams.dbg), launched exactly when dbg is set
template <int HD, bool BATCH = false, bool TIMING = false> __global__ __launch_bounds__(ALP_NT) void attn_long_pv_kernel(AttnParams p) { alp_eager_body<HD, BATCH, TIMING>(p); }

// ------------------------------------------------------------------------------------------------
// attn_long_pv2_kernel (round 6): attn_long_pv_kernel with the p_j evaluated LAZILY, off the critical path.
//
// Stamps of attn_long_pv_kernel at T = 4101 (profiles/r06_att_timing.log): 10.1 k cycles pass before the first product is made -- every
// thread fetches eight e_j, forms eight certified p_j -- then 25.8 k of PV.  Only the first batch's p_j are needed to start the chain: here a
// PRODUCER thread evaluates the p_j of a position right where it multiplies that position's V row (its e_j travels with the V rows, three batches
// ahead), so what stands in front of the chain is the Z estimate and one batch.  The certification is the same (cert_p); an element that
// cannot be certified is found while the chain already runs, so the kernel finishes the optimistic pass, and if ANY element failed (about
// once in 1e9) or force_zseq is set it walks the reference's serial sum and runs the whole PV again with the exact Z: a certified pass
// equals the reference's bits whatever the serial sum is (monotone step function, attn_long_pv_kernel's header); an uncertified one is discarded.
// Same grid, block and LDS as attn_long_pv_kernel (the p array is unused).  The kernel symbol attn_long_pv2_kernel picks between the two bodies (below).
// ------------------------------------------------------------------------------------------------
template <int HD, bool BATCH = false, bool TIMING = false> DEVINL void alp_lazy_body(const AttnParams& p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int h, ds; xcd_head_block(h, ds);
    [[maybe_unused]] AlSeq sq{}; if constexpr (BATCH) sq = al_seq(p, h);      // (BATCH: p.seq_len = the largest member's -- row strides, LDS layout; al_len = this sequence's array ends)
    const int T = al_T<BATCH>(p, sq), nblk = (T + ALS_NT - 1) / ALS_NT, nbatch = (T + ALP_BATCH - 1) / ALP_BATCH;
    float* ring = (float*)(smem + (size_t)p.pw_floats * 4);   // [2][ALP_SLOT] products, behind the p_j array (alp_pw_floats: the launcher's choice)
    double* zsh = (double*)(ring + 2 * ALP_SLOT);
    int* const flag = (int*)(zsh + 1);
    const double* E = p.e_buf + al_row<BATCH>(sq, h) * p.seq_len;
    const int kvh = h / (p.H / p.KVH);
#define ALQ_STAMP(n) do { if (LNB_DBG && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0 && (wave & 3) == 0) p.dbg[(wave >> 2) * 16 + (n)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
    ALQ_STAMP(0);
    // address-only loads first, oldest-needed first: the per-block partial sums, then the producers' first three batches of e_j and V rows
    const int nblk_max = (p.seq_len + ALS_NT - 1) / ALS_NT;
    const double* zp = p.z_part + al_row<BATCH>(sq, h) * nblk_max;
    double zmine = zp[lane < nblk_max ? lane : nblk_max - 1];
    const uint16_t* vbase = al_cv<BATCH>(p, sq) + (size_t)kvh * HD + (size_t)ds * ALP_DS;
    const size_t vrow = (size_t)p.KVH * HD;
    const int pl = tid & 255, half8 = pl & 1, prow = pl >> 1;                // producers: 128 positions x two 8-dim halves per round, 4 rounds per batch
    struct Rows { uint4 v[4]; double e[4]; };
    auto load = [&](Rows& r_, int b) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            int j = b * ALP_BATCH + r * 128 + prow; j = j < al_len<BATCH>(p, sq) ? j : al_len<BATCH>(p, sq) - 1;       // (clamped to the ARRAY end: no wait for the position word)
            r_.e[r] = E[j];
            r_.v[r] = *(const uint4*)(vbase + (size_t)j * vrow + half8 * 8);
        }
    };
    Rows v0, v1, v2, v3;
    if (wave >= 4) { load(v0, 0); load(v1, 1); load(v2, 2); }
    if (tid == 0) *flag = 0;
    // ---- Z estimate: the per-block tree sums in block order (same value in every thread)
    double zt = 0.0;
    for (int b0 = 0; b0 < nblk; b0 += 64) {
        if (b0) zmine = zp[b0 + lane < nblk ? b0 + lane : nblk - 1];
        const int nb = nblk - b0 < 64 ? nblk - b0 : 64;
        const long long zbits = __double_as_longlong(zmine);
        for (int b = 0; b < nb; b++) {
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)zbits, b), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(zbits >> 32), b);
            zt += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        }
    }
    const CertZ cz = cert_z(zt, T);
    __syncthreads();
    ALQ_STAMP(1);
    float acc = 0.0f;
    int bad = 0;
    // one pass of PV over all batches; exact_z == 0: p_j = cert_p(e_j) (sets bad), else p_j = trunc(f32(e_j / z)) with the walked serial sum z
    auto run_pv = [&](bool exact, double z) {
        acc = 0.0f;
        if (wave < 4) {
            const int d = 4 * wave + (lane >> 4), jj = lane & 15;
            for (int it = 0; it <= nbatch; it++) {
                if (it > 0) {
                    const float* src = ring + (size_t)((it - 1) & 1) * ALP_SLOT + (size_t)d * ALP_BATCH + jj * 4;
                    float4 a0 = *(const float4*)(src), a1 = *(const float4*)(src + 64);
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        float pr[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                        if (c < 3) { a0 = *(const float4*)(src + (c + 1) * 128); a1 = *(const float4*)(src + (c + 1) * 128 + 64); }   // in flight behind the 128 adds
                        asm volatile("" : "+v"(pr[0]), "+v"(pr[1]), "+v"(pr[2]), "+v"(pr[3]), "+v"(pr[4]), "+v"(pr[5]), "+v"(pr[6]), "+v"(pr[7]));
                        __builtin_amdgcn_sched_barrier(0);
                        chain128(acc, pr);
                    }
                }
                __syncthreads();
            }
        } else {
            auto produce = [&](const Rows& r_, int b) {
                float* dst = ring + (size_t)(b & 1) * ALP_SLOT + (size_t)(half8 * 8) * ALP_BATCH + ((prow >> 6) & 1) * 64 + (prow & 15) * 4 + ((prow >> 4) & 3);
#pragma unroll
                for (int r = 0; r < 4; r++) {                    // round r = chunk r of the batch; position prow of it
                    const int j = b * ALP_BATCH + r * 128 + prow;
                    float pj = 0.0f;                             // +0 past the row: products +-0, acc is never -0
                    if (j < T) pj = exact ? alp_p(r_.e[r], z) : cert_p(r_.e[r], cz, bad);       // impl:506 + ToBFloat16 :493
                    const uint4 w = r_.v[r];                     // exact products: 8-bit x 8-bit significands
                    float* q = dst + r * 128;
                    q[0 * ALP_BATCH] = pj * bf_lo(w.x); q[1 * ALP_BATCH] = pj * bf_hi(w.x); q[2 * ALP_BATCH] = pj * bf_lo(w.y); q[3 * ALP_BATCH] = pj * bf_hi(w.y);
                    q[4 * ALP_BATCH] = pj * bf_lo(w.z); q[5 * ALP_BATCH] = pj * bf_hi(w.z); q[6 * ALP_BATCH] = pj * bf_lo(w.w); q[7 * ALP_BATCH] = pj * bf_hi(w.w);
                }
            };
            auto step = [&](int it, const Rows& cur, Rows& nxt) {
                if (it <= nbatch) {                              // (uniform; one barrier per iteration, like the adders)
                    if (it < nbatch) { load(nxt, it + 3); produce(cur, it); }
                    __syncthreads();
                }
            };
            for (int it = 0; it <= nbatch; it += 4) { step(it, v0, v3); step(it + 1, v1, v0); step(it + 2, v2, v1); step(it + 3, v3, v2); }
        }
    };
    if (!p.force_zseq) {
        run_pv(false, 0.0);
        ALQ_STAMP(2);
        if (bad) *flag = 1;
        __syncthreads();
    }
    if (p.force_zseq || *flag) {
        // the reference's serial sum, j ascending, f64 (operations_impl.go:492-499): one wave, 16 values in flight ahead of the adds
        if (wave == 0) {
            double z = 0.0;
            for (int j0 = 0; j0 < T; j0 += 16) {
                double v[16];
#pragma unroll
                for (int u = 0; u < 16; u++) v[u] = E[j0 + u < T ? j0 + u : T - 1];
#pragma unroll
                for (int u = 0; u < 16; u++) z += (j0 + u < T) ? v[u] : 0.0;
            }
            if (lane == 0) { zsh[0] = z; if (p.zseq_count && ds == 0) atomicAdd(p.zseq_count, 1); }
        }
        if (wave >= 4) { load(v0, 0); load(v1, 1); load(v2, 2); }       // the producers' pipeline starts over
        __syncthreads();
        run_pv(true, zsh[0]);
    }
    ALQ_STAMP(5);
    if (wave < 4 && (lane & 15) == 0) {
        if constexpr (BATCH) al_store(p, h, HD, ds * ALP_DS + 4 * wave + (lane >> 4), acc);
        else p.out[(size_t)h * HD + ds * ALP_DS + 4 * wave + (lane >> 4)] = bf_trunc(acc);
    }
    ALQ_STAMP(6);
#undef ALQ_STAMP
}

// up to two batches (T <= 1024) the eager form is the faster one (all 512 threads share the first batch's p_j: 11.2 against 11.5 us at T = 768,
// 9.6 against 10.1 at 272); from three batches on the lazy one (T = 2048: 15.1 -> 14.5 us, 4101: 23.0 -> 21.8).  T lives on the device (one captured
// graph serves every position), so the choice is made here, per launch, uniformly over the grid.
template <int HD, bool BATCH = false, bool TIMING = false> __global__ __launch_bounds__(ALP_NT) void attn_long_pv2_kernel(AttnParams p) {
    if constexpr (BATCH) { if (p.btab->st[blockIdx.z]->pos + 1 <= 2 * ALP_BATCH) alp_eager_body<HD, true, TIMING>(p); else alp_lazy_body<HD, true, TIMING>(p); }     // (per sequence: uniform over its workgroups)
    else if (p.st->pos + 1 <= 2 * ALP_BATCH) alp_eager_body<HD, false, TIMING>(p); else alp_lazy_body<HD, false, TIMING>(p);
}

// ------------------------------------------------------------------------------------------------
// Long-context attention for W <= 16 CONSECUTIVE query rows of one context (lnb_forward_append of 2..15 rows beyond the row-per-workgroup
// kernel's reach; opt-in: the verify passes of the speculative loop).  Row i sits at position pos + i and attends to j <= pos + i: it is
// the one-token step at that position, and its arithmetic is attn_long_scores_kernel + the lazily certified PV pass for T_i = pos + i + 1,
// operation for operation.  What changes is who reads K and V: the batched long pair takes the rows as grid.z and reads every K and V row
// once per query row; here
//   attn_rows_scores_kernel  grid (H, blocks of 256 positions): a thread loads its K row ONCE and runs W chains against the W query
//       vectors in the LDS (f32, W * HD * 4 bytes); e_buf[i][h][j] for j < T_i, one tree sum per (row, block) in attn_long_scores_kernel's
//       fixed shape (positions >= T_i contribute +0); a block past the last row's T returns at once; the V touch once per block.
//   attn_rows_pv_kernel<HD, RPW>  grid (H, hd / 16, ceil(W / RPW)): a workgroup serves RPW rows of one (head, 16-dim slice); a producer
//       thread loads a V row once and turns it into RPW products (p_j of each row evaluated right there: alp_lazy_body's scheme, so the
//       LDS holds product rings only and does not depend on the context length), the adder waves walk the RPW chains one after the
//       other.  RPW 1: two ring slots of 512 positions (64 KB); RPW 2 / 4: slots of 256 positions (32 KB per row) -- the producers keep four
//       batches of V rows and RPW e_j per row in registers, and at 512 positions two rows of them no longer fit the 256 VGPRs of a wave.
// Certification per row with the band for ITS T_i (cert_z); if any element of any of the workgroup's rows fails (or force_zseq), the
// workgroup walks every row's serial sum (wave r walks row r) and runs the pass again with the exact sums.  A certified p_j has the
// reference's bits whether the one-token step formed it in its eager (T <= 1024) or its lazy body, so one body serves every T here.
// Scratch row = the row's index in the launch (AttnRowsParams).
// ------------------------------------------------------------------------------------------------
DEVINL int ar_pos(const AttnRowsParams& rp) { return (rp.pos0 >= 0 ? rp.pos0 : rp.a.btab ? rp.a.btab->st[0]->pos : rp.a.st->pos) + rp.pos_off; }
DEVINL int ar_T(const AttnRowsParams& rp, int pos, int i) { const int T = pos + i + 1; return T < 1 ? 1 : (T > rp.a.seq_len ? rp.a.seq_len : T); }      // (clamped into the cache, as al_seq does)
// (a verify pass carries the context's caches of the layer in its batch table: every column has the same)
DEVINL const uint16_t* ar_ck(const AttnParams& p) { return p.btab ? p.bkv->ck[0] : p.cache_k; }
DEVINL const uint16_t* ar_cv(const AttnParams& p) { return p.btab ? p.bkv->cv[0] : p.cache_v; }
DEVINL void ar_store(const AttnRowsParams& rp, int row, int h, int hd_, int d, float acc) {
    const AttnParams& p = rp.a;
    if (p.out_xt) p.out_xt[xt_group(row, p.H * hd_) + xt_index(row & 15, h * hd_ + d)] = bf_trunc(acc);
    else p.out[((size_t)row * p.H + h) * hd_ + d] = bf_trunc(acc);
}
template <int HD> __global__ __launch_bounds__(ALS_NT) void attn_rows_scores_kernel(AttnRowsParams rp) {
    constexpr int NK = HD / 8;
    __shared__ __attribute__((aligned(16))) float qf[LNB_ATTN_ROWS_MAX * HD];
    __shared__ double wsum[LNB_ATTN_ROWS_MAX][ALS_NT / 64];
    const AttnParams& p = rp.a;
    const int tid = threadIdx.x;
    int h, blk; xcd_head_block(h, blk);
    const int W = rp.W, pos = ar_pos(rp), j0 = blk * ALS_NT;
    const int Tl = ar_T(rp, pos, W - 1);                     // the last row's T: the rows' lengths ascend
    if (j0 >= Tl) return;                                    // (uniform)
    const int kvh = h / (p.H / p.KVH);
    const uint4* kbase = (const uint4*)ar_ck(p) + (size_t)kvh * NK * p.seq_len;
    const int j = j0 + tid;
    uint4 k[NK];
    attn_load_k<NK>(k, kbase, p.seq_len, j < Tl ? j : Tl - 1);
    unsigned vt;                                             // the V touch of attn_long_scores_kernel, once per block (for the longest row)
    {
        constexpr int LPR = HD / 64 > 0 ? HD / 64 : 1;
        const int l = ((h % (p.H / p.KVH)) % LPR) * ALS_NT + tid;
        int jl = j0 + l / LPR; jl = jl < Tl ? jl : Tl - 1;
        const char* va = (const char*)ar_cv(p) + ((size_t)jl * p.KVH + kvh) * HD * 2 + (l % LPR) * 128;
        va = p.touch ? va : (const char*)kbase;
        asm volatile("global_load_dword %0, %1, off ; RING_LOAD (never retired: tools/isa_audit.py flags any later use of the register)" : "=v"(vt) : "v"(va));
    }
    for (int x = tid; x < W * HD; x += ALS_NT) qf[x] = bf_wide(p.q[((size_t)(rp.row0 + x / HD) * p.H + h) * HD + x % HD]);
    __syncthreads();
    const size_t nblk_max = (size_t)((p.seq_len + ALS_NT - 1) / ALS_NT);
    for (int i = 0; i < W; i++) {
        const int Ti = ar_T(rp, pos, i);
        if (j0 >= Ti) continue;                              // (uniform: this row has no position in the block, the PV pass reads no partial sum of it)
        double ev = 0.0;
        if (j < Ti) { ev = attn_score_value<NK>(k, qf + i * HD, p.divisor); p.e_buf[((size_t)i * p.H + h) * p.seq_len + j] = ev; }
        ev = wave_sum_f64(ev);                               // attn_long_scores_kernel's tree
        if ((tid & 63) == 0) wsum[i][tid >> 6] = ev;
    }
    __syncthreads();
    if (tid < W && j0 < ar_T(rp, pos, tid)) p.z_part[((size_t)tid * p.H + h) * nblk_max + blk] = (wsum[tid][0] + wsum[tid][1]) + (wsum[tid][2] + wsum[tid][3]);
    asm volatile("" :: "v"(vt));
}

template <int RPW> struct ArCfg { static constexpr int B = RPW >= 2 ? 256 : 512, NR = B / 128, SLOT = ALP_DS * B; };      // positions per ring slot, 128-position rounds, floats per slot
__host__ __device__ inline size_t ar_lds_bytes(int rpw) { return (size_t)rpw * 2 * ALP_DS * (rpw >= 2 ? 256 : 512) * 4 + 64; }
template <int HD, int RPW> __global__ __launch_bounds__(ALP_NT) void attn_rows_pv_kernel(AttnRowsParams rp) {
    constexpr int B = ArCfg<RPW>::B, NR = ArCfg<RPW>::NR, SLOT = ArCfg<RPW>::SLOT;
    static_assert(RPW <= 4, "zsh holds four walked sums and the flag in 64 bytes; the serial walk is one wave per row of the adder waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const AttnParams& p = rp.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int h, ds; xcd_head_block(h, ds);
    const int g0 = blockIdx.z * RPW;                         // first row of the launch this workgroup serves (g0 < W: the grid is ceil(W / RPW))
    const int pos = ar_pos(rp);
    float* ring = (float*)smem;                              // [RPW][2][SLOT] products: [dim][chunk][half][position % 16][4] per slot (alp_lazy_body's)
    double* zsh = (double*)(ring + (size_t)RPW * 2 * SLOT);  // [RPW] walked serial sums
    int* const flag = (int*)(zsh + RPW);
    int T[RPW]; bool on[RPW]; const double* E[RPW];
    int Tmax = 1;
#pragma unroll
    for (int r = 0; r < RPW; r++) {
        on[r] = g0 + r < rp.W;
        const int i = on[r] ? g0 + r : rp.W - 1;             // (a row past the launch's last: nothing of it is used; its addresses stay inside the scratch)
        T[r] = on[r] ? ar_T(rp, pos, i) : 0;
        if (on[r]) Tmax = T[r];
        E[r] = p.e_buf + ((size_t)i * p.H + h) * p.seq_len;
    }
    const int nbatch = (Tmax + B - 1) / B;
    const int kvh = h / (p.H / p.KVH);
    // address-only loads first: the producers' first three batches of e_j and V rows
    const uint16_t* vbase = ar_cv(p) + (size_t)kvh * HD + (size_t)ds * ALP_DS;
    const size_t vrow = (size_t)p.KVH * HD;
    const int pl = tid & 255, half8 = pl & 1, prow = pl >> 1; // producers: 128 positions x two 8-dim halves per round, NR rounds per batch
    struct Rows { uint4 v[NR]; double e[RPW][NR]; };
    auto load = [&](Rows& r_, int b) {
#pragma unroll
        for (int rr = 0; rr < NR; rr++) {
            int j = b * B + rr * 128 + prow; j = j < p.seq_len ? j : p.seq_len - 1;        // (clamped to the ARRAY end)
#pragma unroll
            for (int r = 0; r < RPW; r++) r_.e[r][rr] = on[r] ? E[r][j] : 0.0;     // (uniform: a row past the launch's last costs no traffic)
            r_.v[rr] = *(const uint4*)(vbase + (size_t)j * vrow + half8 * 8);
        }
    };
    Rows v0, v1, v2, v3;
    if (wave >= 4) { load(v0, 0); load(v1, 1); load(v2, 2); }
    if (tid == 0) *flag = 0;
    // ---- Z estimates: each row's per-block tree sums in block order (same value in every thread)
    const size_t nblk_max = (size_t)((p.seq_len + ALS_NT - 1) / ALS_NT);
    CertZ cz[RPW];
#pragma unroll
    for (int r = 0; r < RPW; r++) {
        double zt = 1.0;
        if (on[r]) {
            const int nblk = (T[r] + ALS_NT - 1) / ALS_NT;
            const double* zp = p.z_part + ((size_t)(g0 + r) * p.H + h) * nblk_max;
            zt = 0.0;
            for (int b0 = 0; b0 < nblk; b0 += 64) {
                const double zmine = zp[b0 + lane < nblk ? b0 + lane : nblk - 1];
                const int nb = nblk - b0 < 64 ? nblk - b0 : 64;
                const long long zbits = __double_as_longlong(zmine);
                for (int b = 0; b < nb; b++) {
                    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)zbits, b), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(zbits >> 32), b);
                    zt += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
                }
            }
        }
        cz[r] = cert_z(zt, T[r]);
    }
    __syncthreads();
    float acc[RPW];
    int bad = 0;
    // one pass of PV over all batches for the workgroup's rows; exact == false: p_j = cert_p(e_j) (sets bad), else p_j = trunc(f32(e_j / z_r)) with the walked sums
    auto run_pv = [&](bool exact) {
#pragma unroll
        for (int r = 0; r < RPW; r++) acc[r] = 0.0f;
        if (wave < 4) {
            const int d = 4 * wave + (lane >> 4), jj = lane & 15;
            for (int it = 0; it <= nbatch; it++) {
                if (it > 0) {
#pragma unroll
                    for (int r = 0; r < RPW; r++) {
                        if (!on[r]) continue;                // (uniform)
                        const float* src = ring + (size_t)(2 * r + ((it - 1) & 1)) * SLOT + (size_t)d * B + jj * 4;
                        float4 a0 = *(const float4*)(src), a1 = *(const float4*)(src + 64);
#pragma unroll
                        for (int c = 0; c < NR; c++) {
                            float pr[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                            if (c < NR - 1) { a0 = *(const float4*)(src + (c + 1) * 128); a1 = *(const float4*)(src + (c + 1) * 128 + 64); }   // in flight behind the 128 adds
                            asm volatile("" : "+v"(pr[0]), "+v"(pr[1]), "+v"(pr[2]), "+v"(pr[3]), "+v"(pr[4]), "+v"(pr[5]), "+v"(pr[6]), "+v"(pr[7]));
                            __builtin_amdgcn_sched_barrier(0);
                            chain128(acc[r], pr);            // j ascending: batches, chunks, then the chunk's 128 positions
                        }
                    }
                }
                __syncthreads();
            }
        } else {
            auto produce = [&](const Rows& r_, int b) {
                float* dst = ring + (size_t)(b & 1) * SLOT + (size_t)(half8 * 8) * B + ((prow >> 6) & 1) * 64 + (prow & 15) * 4 + ((prow >> 4) & 3);
#pragma unroll
                for (int rr = 0; rr < NR; rr++) {            // round rr = chunk rr of the batch; position prow of it
                    const int j = b * B + rr * 128 + prow;
                    const uint4 wv = r_.v[rr];               // ONE V row, products for every row of the workgroup (exact: 8-bit x 8-bit significands)
#pragma unroll
                    for (int r = 0; r < RPW; r++) {
                        if (!on[r]) continue;
                        // past the row's end: p = +0 AND V = +0, products +0 (acc is never -0).  The V row there is a later row of the call, a stale row of
                        // an earlier generation or the array's end: it may hold anything, a NaN or an inf included, and +0 x NaN would reach the chain
                        const bool live = j < T[r];
                        const uint4 w = live ? wv : make_uint4(0u, 0u, 0u, 0u);
                        float pj = 0.0f;
                        if (live) pj = exact ? alp_p(r_.e[r][rr], zsh[r]) : cert_p(r_.e[r][rr], cz[r], bad);       // impl:506 + ToBFloat16 :493
                        float* q = dst + (size_t)(2 * r) * SLOT + rr * 128;
                        q[0 * B] = pj * bf_lo(w.x); q[1 * B] = pj * bf_hi(w.x); q[2 * B] = pj * bf_lo(w.y); q[3 * B] = pj * bf_hi(w.y);
                        q[4 * B] = pj * bf_lo(w.z); q[5 * B] = pj * bf_hi(w.z); q[6 * B] = pj * bf_lo(w.w); q[7 * B] = pj * bf_hi(w.w);
                    }
                }
            };
            auto step = [&](int it, const Rows& cur, Rows& nxt) {
                if (it <= nbatch) {                          // (uniform; one barrier per iteration, like the adders)
                    if (it < nbatch) { load(nxt, it + 3); produce(cur, it); }
                    __syncthreads();
                }
            };
            for (int it = 0; it <= nbatch; it += 4) { step(it, v0, v3); step(it + 1, v1, v0); step(it + 2, v2, v1); step(it + 3, v3, v2); }
        }
    };
    if (!p.force_zseq) {
        run_pv(false);
        if (bad) *flag = 1;
        __syncthreads();
    }
    if (p.force_zseq || *flag) {
        // the reference's serial sums, j ascending, f64 (operations_impl.go:492-499): wave r walks row r, 16 values in flight ahead of the adds
#pragma unroll
        for (int r = 0; r < RPW; r++) {
            if (wave != r || !on[r]) continue;
            double z = 0.0;
            for (int j0 = 0; j0 < T[r]; j0 += 16) {
                double v[16];
#pragma unroll
                for (int u = 0; u < 16; u++) v[u] = E[r][j0 + u < T[r] ? j0 + u : T[r] - 1];
#pragma unroll
                for (int u = 0; u < 16; u++) z += (j0 + u < T[r]) ? v[u] : 0.0;
            }
            if (lane == 0) { zsh[r] = z; if (p.zseq_count && ds == 0) atomicAdd(p.zseq_count, 1); }      // once per (row, head)
        }
        if (wave >= 4) { load(v0, 0); load(v1, 1); load(v2, 2); }       // the producers' pipeline starts over
        __syncthreads();
        run_pv(true);
    }
    if (wave < 4 && (lane & 15) == 0) {
#pragma unroll
        for (int r = 0; r < RPW; r++) if (on[r]) ar_store(rp, rp.row0 + g0 + r, h, HD, ds * ALP_DS + 4 * wave + (lane >> 4), acc[r]);
    }
}

// ------------------------------------------------------------------------------------------------
// Non-finite K / V rows in a multi-row call (lnb_forward, lnb_forward_append): the matrix-core kernels and the multi-row forms of
// attn_exact_kernel rest on FINITE rows -- a masked entry is e = 0 without its score, tiles and chunks beyond the diagonal are skipped, and
// the 16 positions of a tile are the B operand of all 16 query rows.  The reference adds the mask to the score (NaN + -inf = NaN: the whole
// row NaN) and multiplies p = +0 by every V row of the call (+0 x NaN = NaN); the one-token step at an earlier position never sees a later row.
//   kv_nonfinite_scan_kernel  raises the context's sticky word when one of the rows [pos, pos + rows) of a layer's K or V holds an inf or a NaN;
//   attn_plain_kernel<HD>     launched behind the attention of such a call: returns at once while the word is clear; otherwise workgroup
//       (head, row) computes the row again as the reference's attention does (llamatransformer.go:409-514) -- every position's score, the mask ADDED (modulo form)
//       or the row's own T (causal form), the serial f64 sum, PV over every position, j ascending -- and overwrites the row's output.
// Slow and obvious on purpose: 256 positions scored per round, one thread adds them in order, head_dim threads own one output dim each.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_nonfinite_scan_kernel(const uint16_t* ck, const uint16_t* cv, int seq_len, int kv_dim, int hd, const StepState* st, int pos0,
                                                                int rows, int* word) {
    const int pos = st ? st->pos : pos0;
    const size_t n = (size_t)rows * kv_dim;
    bool hit = false;
    for (size_t x = (size_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (size_t)gridDim.x * 256) {
        const int j = pos + (int)(x / kv_dim), c = (int)(x % kv_dim), kh = c / hd, d = c % hd;
        if (j >= seq_len) break;
        const uint16_t k = ck[(((size_t)kh * (hd >> 3) + (d >> 3)) * seq_len + j) * 8 + (d & 7)], v = cv[(size_t)j * kv_dim + c];
        hit |= (k & 0x7F80) == 0x7F80 || (v & 0x7F80) == 0x7F80;
    }
    if (hit) atomicOr(word, 1);
}
__global__ void nonfinite_or_kernel(int* dst, const int* src) { if (*src) atomicOr(dst, 1); }
template <int HD> __global__ __launch_bounds__(256) void attn_plain_kernel(AttnParams p, const int* nonfinite) {
    if (*nonfinite == 0) return;                             // (uniform) every row the call can see is finite: the fast kernel's result stands
    constexpr int NK = HD / 8, NT = 256;
    __shared__ __attribute__((aligned(16))) float qf[HD];
    __shared__ double eb[NT];
    __shared__ float pb[NT];
    __shared__ double zs;
    const int tid = threadIdx.x, h = blockIdx.x, i = blockIdx.y;
    const int S = p.S, pos0 = p.st->pos;
    int T = p.causal ? pos0 + i + 1 : pos0 + S;              // causal: row i IS the one-token step at pos0 + i
    T = T > p.seq_len ? p.seq_len : T;
    const bool add_mask = !p.causal && S > 1;                // Add(scores, mask), the [S,S] mask broadcast by modulo (llamatransformer.go:469-473)
    const int kvh = h / (p.H / p.KVH);
    const uint4* kbase = (const uint4*)p.cache_k + (size_t)kvh * NK * p.seq_len;
    const uint16_t* vbase = p.cache_v + (size_t)kvh * HD;
    const size_t vrow = (size_t)p.KVH * HD;
    if (tid < HD) qf[tid] = bf_wide(p.q[((size_t)i * p.H + h) * HD + tid]);
    __syncthreads();
    auto e_of = [&](int j) -> double {
        uint4 k[NK];
        attn_load_k<NK>(k, kbase, p.seq_len, j);
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < NK; c++) {                       // MatMul q.k, d ascending (operations_matmul.go:37-55)
            const float4 xa = *(const float4*)(qf + c * 8), xb = *(const float4*)(qf + c * 8 + 4);
            acc = mac8(acc, xa, xb, k[c]);
        }
        uint16_t s = bf_trunc(acc);
        s = bf_trunc(__fdiv_rn(bf_wide(s), p.divisor));     // DivToScalar :464
        if (add_mask) s = bf_trunc(bf_wide(s) + ((j % S) > i ? -INFINITY : 0.0f));
        return exp((double)bf_wide(s));
    };
    double z = 0.0;                                          // rowExpSum += exp(...), j ascending, f64 (impl:492-499): thread 0
    for (int j0 = 0; j0 < T; j0 += NT) {
        const int j = j0 + tid;
        eb[tid] = j < T ? e_of(j) : 0.0;
        __syncthreads();
        if (tid == 0) { const int n = T - j0 < NT ? T - j0 : NT; for (int u = 0; u < n; u++) z += eb[u]; }
        __syncthreads();
    }
    if (tid == 0) zs = z;
    __syncthreads();
    z = zs;
    float acc = 0.0f;
    for (int j0 = 0; j0 < T; j0 += NT) {
        const int j = j0 + tid;
        if (j < T) pb[tid] = bf_wide(bf_trunc((float)(e_of(j) / z)));       // impl:506 + ToBFloat16 :493
        __syncthreads();
        if (tid < HD) {
            const int n = T - j0 < NT ? T - j0 : NT;
            for (int u = 0; u < n; u++) acc += pb[u] * bf_wide(vbase[(size_t)(j0 + u) * vrow + tid]);      // MatMul(scores, values) :504, every position
        }
        __syncthreads();
    }
    if (tid < HD) p.out[((size_t)i * p.H + h) * HD + tid] = bf_trunc(acc);
}

// ------------------------------------------------------------------------------------------------
// attn_one_kernel (round 6): the long-context decode attention in ONE launch.
//
// The two-launch form above pays, per layer at T = 4100: the scores launch (6.3 us), a kernel boundary, and ~8 k cycles at the head of
// the PV launch in which every workgroup waits for e_buf / z_part to come back through the fabric (stamps: profiles/r06_att_timing.log) --
// 23.1 us against a PV chain of 10.4 us.  Here the (head, 16-dim slice) workgroups of attn_long_pv_kernel compute the scores themselves:
//   T <= 512  every slice workgroup of a head scores all positions (one per thread; the K rows are L2 hits for seven of the eight) and keeps
//             the exponentials in its LDS: no exchange at all;
//   T >  512  position block b (512 positions) belongs to slice b % slices: the workgroup scores its blocks, publishes e_j (f64) and the block's
//             tree sum with WRITE-THROUGH stores (global_store ... sc1), drains them (s_waitcnt vmcnt(0)), arrives on the head's counter
//             (one device-scope atomic; the generation of the launch is old / slices, so the counter never has to be reset and a replayed
//             graph needs no per-launch argument), polls it with sc1 loads, and then reads the head's row with sc1 loads (L2 / fabric, never a
//             stale L1 line) -- the flag form MI355X_MICROARCH.md lists as valid for any placement of the workgroups (no agent fence:
//             round 3's single-launch attempt paid an L2 write-back + invalidate per fence, 34.5 us against 26.8).
// A workgroup NEVER depends on another one being resident: the poll is bounded (ATT1_TIMEOUT ticks of the 100 MHz wall clock); when it
// runs out -- another context's launch holds the CUs its peers need -- the workgroup scores the missing blocks itself (the values it stores
// are the ones the owner would store: same instructions, same bits) and goes on.  Two such launches of two contexts can therefore never
// wait for each other; the price of contention is time, not a hang (longctx == 3 forces that path for the tests).
// Everything after the scores is attn_long_pv_kernel: tree estimate of Z + certified p_j (or the serial walk), the row-broadcast PV chain.
// grid (H, hd / 16) through xcd_head_block (a head's slices and its GQA group share an XCD), block 512, dynamic LDS att1_lds_bytes().
// ------------------------------------------------------------------------------------------------
constexpr long long ATT1_TIMEOUT = 4000;                     // 40 us of wall clock: ~2x the whole kernel at 4 K positions
__host__ __device__ inline size_t att1_lds_bytes(int seq_len, int hd) { return alp_lds_bytes(seq_len) + 64 + (size_t)hd * 4 + 64 + (size_t)ALP_BATCH * 8; }
DEVINL void st_sc1_f64(double* p, double v) { __hip_atomic_store((unsigned long long*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DEVINL double ld_sc1_f64(const double* p) { return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
template <int HD> __global__ __launch_bounds__(ALP_NT) void attn_one_kernel(AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NK = HD / 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int h, ds; xcd_head_block(h, ds);
    const int NSL = (int)gridDim.y;
    const int T = p.st->pos + 1, nbatch = (T + ALP_BATCH - 1) / ALP_BATCH;      // 512-position blocks: the unit of the scores AND of the PV batches
    const int Tpad = (nbatch + 1) * ALP_BATCH;
    float* pw = (float*)smem;
    float* ring = (float*)(smem + (size_t)((p.seq_len + ALP_BATCH - 1) / ALP_BATCH + 1) * ALP_BATCH * 4);
    double* zsh = (double*)(ring + 2 * ALP_SLOT);            // [0] serial Z | [1] flags (two ints) | [2..3] -
    int* const flag = (int*)(zsh + 1);
    double* wsum = zsh + 8;                                  // [8] wave partials of a block's tree sum
    float* qf = (float*)(wsum + 8);                          // [HD]
    double* e_s = (double*)(qf + HD);                        // [512] (T <= 512: the row's exponentials never leave the workgroup)
    double* E = p.e_buf + (size_t)h * p.seq_len;
    double* zp = p.z_part + (size_t)h * (((size_t)p.seq_len + 63) / 64 + 8);      // one partial per 64 positions (a wave of a block)
    const int kvh = h / (p.H / p.KVH);
    const bool local = nbatch <= 1;                          // (uniform over the grid: T comes from the device-side position)
#define AT1_STAMP(n) do { if (p.dbg && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0 && (wave & 3) == 0) p.dbg[(wave >> 2) * 16 + (n)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
    AT1_STAMP(0);
    // ---- q and this workgroup's first TWO blocks of K rows go in flight first (a block = 512 positions, one per thread; block b belongs to slice
    // b % NSL; at T = 4101 slice 0 owns two: scored one after the other with the second one's rows fetched behind the first one's chain they cost
    // 11.7 k cycles, prefetched 6 k), then the producers' first three batches of V rows
    const uint4* kbase = (const uint4*)p.cache_k + (size_t)kvh * NK * p.seq_len;
    const uint16_t q16 = p.q[(size_t)h * HD + (tid < HD ? tid : 0)];
    const int b_first = local ? 0 : ds;
    uint4 ka[NK], kb[NK];
    auto load_k = [&](uint4 (&k)[NK], int b) { const int j = b * ALP_BATCH + tid; attn_load_k<NK>(k, kbase, p.seq_len, j < T ? j : T - 1); };
    load_k(ka, b_first);
    if (!local && b_first + NSL < nbatch) load_k(kb, b_first + NSL);
    const uint16_t* vbase = p.cache_v + (size_t)kvh * HD + (size_t)ds * ALP_DS;
    const size_t vrow = (size_t)p.KVH * HD;
    const int pl = tid & 255, half8 = pl & 1, prow = pl >> 1;
    auto load = [&](uint4 (&v)[4], int b) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            int j = b * ALP_BATCH + r * 128 + prow; j = j < T ? j : T - 1;
            v[r] = *(const uint4*)(vbase + (size_t)j * vrow + half8 * 8);
        }
    };
    uint4 v0[4], v1[4], v2[4], v3[4];
    if (wave >= 4) { load(v0, 0); load(v1, 1); load(v2, 2); }
    if (tid < HD) qf[tid] = bf_wide(q16);
    if (tid == 0) { flag[0] = 0; flag[1] = 0; }
    __syncthreads();
    AT1_STAMP(1);
    // ---- scores of one 512-position block (llamatransformer.go:456-473, Softmax impl:498) + every WAVE's tree sum of its 64 exponentials (only ever
    // an ESTIMATE of Z): no workgroup barrier in here
    auto score_block = [&](const uint4 (&k)[NK], int b) {
        const int j = b * ALP_BATCH + tid;
        double ev = 0.0;
        if (j < T) ev = attn_score_value<NK>(k, qf, p.divisor);
        if (local) e_s[tid] = ev; else if (j < T) st_sc1_f64(E + j, ev);
        double sm = ev;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
        if (lane == 0) { if (local) wsum[wave] = sm; else st_sc1_f64(zp + b * 8 + wave, sm); }
    };
    auto score_mine = [&](int ofs) {                         // blocks ofs, ofs + NSL, ... of this workgroup, the next one's K rows always in flight
        for (int b = ofs; b < nbatch; b += 2 * NSL) {
            if (b != ofs) { if (b + NSL < nbatch) load_k(kb, b + NSL); }
            score_block(ka, b);
            if (b + NSL < nbatch) {
                if (b + 2 * NSL < nbatch) load_k(ka, b + 2 * NSL);
                score_block(kb, b + NSL);
            }
        }
    };
    if (b_first < nbatch) score_mine(b_first);
    if (!local) {
        AT1_STAMP(2);
        // ---- publish: the write-through stores have left this CU (vmcnt counts stores on gfx9), one lane arrives and polls
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            unsigned* cnt = (unsigned*)p.cnt + h;
            const unsigned old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned target = (old / (unsigned)NSL + 1u) * (unsigned)NSL;
            int ok = 0;
            if (p.longctx != 3) {
                const long long t0 = (long long)wall_clock64();
                for (;;) {
                    if ((int)(__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) >= 0) { ok = 1; break; }
                    if ((long long)wall_clock64() - t0 > ATT1_TIMEOUT) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                if (!ok) atomicAdd((unsigned*)p.cnt + p.H, 1u);      // (diagnostics: polls that ran out)
            }
            flag[1] = ok;
        }
        __syncthreads();
        if (!flag[1]) {                                      // peers not resident (or the forced test path): score their blocks here -- same bits
            for (int o = 1; o < NSL; o++) {
                const int ofs = (ds + o) % NSL;
                if (ofs < nbatch) { load_k(ka, ofs); if (ofs + NSL < nbatch) load_k(kb, ofs + NSL); score_mine(ofs); }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    } else __syncthreads();                                  // (e_s and wsum are complete)
    AT1_STAMP(3);
    // ---- Z estimate: the waves' tree sums (64 positions each), 64 of them per round, reduced by a fixed-shape butterfly: every thread of every
    // workgroup of the head gets the same value (any order of adding T non-negative doubles is inside the certified band)
    double zt = 0.0;
    if (local) zt = ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])) + ((wsum[4] + wsum[5]) + (wsum[6] + wsum[7]));
    else {
        const int nw = (T + 63) >> 6;                        // waves that stored a partial
        for (int w0 = 0; w0 < nw; w0 += 64) {
            double z = w0 + lane < nw ? ld_sc1_f64(zp + w0 + lane) : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
            zt += z;
        }
    }
    // ---- p_j with the estimate, certified (attn_long_pv_kernel's header); e_j from the LDS (local) or with sc1 loads
    const unsigned delta32 = 4u * (unsigned)T + 12u;
    const double epsr = (double)(4 * T + 8) * 1.1102230246251565e-16;
    const double zlo = zt * (1.0 - epsr), zhi = zt * (1.0 + epsr), rzt = 1.0 / zt;
    int bad = p.force_zseq;
    double ev[ALP_EU];
    for (int j0 = 0; j0 < Tpad; j0 += ALP_EU * ALP_NT) {
#pragma unroll
        for (int u = 0; u < ALP_EU; u++) {
            const int j = j0 + u * ALP_NT + tid;
            ev[u] = local ? (j < ALP_BATCH ? e_s[j] : 0.0) : ld_sc1_f64(E + (j < T ? j : T - 1));
        }
#pragma unroll
        for (int u = 0; u < ALP_EU; u++) {
            const int j = j0 + u * ALP_NT + tid;
            if (j >= Tpad) continue;
            float pj = 0.0f;
            if (j < T) {
                const double e = ev[u];
                const double q = e * rzt;
                pj = bf_wide(bf_trunc((float)q));
                const unsigned qh = (unsigned)__double2hiint(q), ql = (unsigned)__double2loint(q);
                const unsigned eq = (qh >> 20) & 0x7FFu;
                if (eq - 897u <= 126u) {
                    if ((qh & 0x1FFFu) == 0x1FFFu && ql - (0xF0000000u - delta32) <= 2u * delta32) bad = 1;
                } else if (q != 0.0 && (alp_p(e, zlo) != alp_p(e, zhi) || pj != alp_p(e, zlo))) bad = 1;
            }
            pw[j] = pj;
        }
        if (local) break;                                    // (Tpad = 1024: one round covers it)
    }
    AT1_STAMP(4);
    if (bad) flag[0] = 1;
    __syncthreads();
    if (flag[0]) {
        // the reference's serial sum, j ascending, f64 (operations_impl.go:492-499)
        if (wave == 0) {
            double z = 0.0;
            for (int j0 = 0; j0 < T; j0 += 16) {
                double v[16];
#pragma unroll
                for (int u = 0; u < 16; u++) { const int j = j0 + u < T ? j0 + u : T - 1; v[u] = local ? e_s[j] : ld_sc1_f64(E + j); }
#pragma unroll
                for (int u = 0; u < 16; u++) z += (j0 + u < T) ? v[u] : 0.0;
            }
            if (lane == 0) { zsh[0] = z; if (p.zseq_count && ds == 0) atomicAdd(p.zseq_count, 1); }
        }
        __syncthreads();
        const double z = zsh[0];
        for (int j = tid; j < T; j += ALP_NT) pw[j] = alp_p(local ? e_s[j] : ld_sc1_f64(E + j), z);
        __syncthreads();
    }
    // ---- PV: attn_long_pv_kernel's row-broadcast chain (llamatransformer.go:504-514)
    float acc = 0.0f;
    if (wave < 4) {
        const int d = 4 * wave + (lane >> 4), jj = lane & 15;
        AT1_STAMP(5);
        for (int it = 0; it <= nbatch; it++) {
            if (it > 0) {
                const float* src = ring + (size_t)((it - 1) & 1) * ALP_SLOT + (size_t)d * ALP_BATCH + jj * 4;
                float4 a0 = *(const float4*)(src), a1 = *(const float4*)(src + 64);
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    float pr[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                    if (c < 3) { a0 = *(const float4*)(src + (c + 1) * 128); a1 = *(const float4*)(src + (c + 1) * 128 + 64); }
                    asm volatile("" : "+v"(pr[0]), "+v"(pr[1]), "+v"(pr[2]), "+v"(pr[3]), "+v"(pr[4]), "+v"(pr[5]), "+v"(pr[6]), "+v"(pr[7]));
                    __builtin_amdgcn_sched_barrier(0);
                    chain128(acc, pr);
                }
            }
            __syncthreads();
        }
        AT1_STAMP(6);
        if (jj == 0) p.out[(size_t)h * HD + ds * ALP_DS + d] = bf_trunc(acc);
    } else {
        auto produce = [&](const uint4 (&v)[4], int b) {
            float* dst = ring + (size_t)(b & 1) * ALP_SLOT + (size_t)(half8 * 8) * ALP_BATCH + ((prow >> 6) & 1) * 64 + (prow & 15) * 4 + ((prow >> 4) & 3);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float pj = pw[b * ALP_BATCH + r * 128 + prow];
                const uint4 w = v[r];
                float* q = dst + r * 128;
                q[0 * ALP_BATCH] = pj * bf_lo(w.x); q[1 * ALP_BATCH] = pj * bf_hi(w.x); q[2 * ALP_BATCH] = pj * bf_lo(w.y); q[3 * ALP_BATCH] = pj * bf_hi(w.y);
                q[4 * ALP_BATCH] = pj * bf_lo(w.z); q[5 * ALP_BATCH] = pj * bf_hi(w.z); q[6 * ALP_BATCH] = pj * bf_lo(w.w); q[7 * ALP_BATCH] = pj * bf_hi(w.w);
            }
        };
        auto step = [&](int it, const uint4 (&cur)[4], uint4 (&nxt)[4]) {
            if (it <= nbatch) {
                if (it < nbatch) { load(nxt, it + 3); produce(cur, it); }
                __syncthreads();
            }
        };
        AT1_STAMP(5);
        for (int it = 0; it <= nbatch; it += 4) { step(it, v0, v3); step(it + 1, v1, v0); step(it + 2, v2, v1); step(it + 3, v3, v2); }
        AT1_STAMP(6);
    }
#undef AT1_STAMP
}

// ------------------------------------------------------------------------------------------------
// small kernels
// ------------------------------------------------------------------------------------------------
// Fwd_Get_Rows (operations_impl.go:142-173): byte copy of embedding rows
__global__ void embed_kernel(const uint16_t* emb, const int32_t* tokens, uint16_t* x, int dim, int vocab, int* err) {
    const int m = blockIdx.x;
    const int t = tokens[m];
    if (t < 0 || t >= vocab) { if (threadIdx.x == 0) atomicExch(err, 1 + m); return; }
    const uint4* src = (const uint4*)(emb + (size_t)t * dim);
    uint4* dst = (uint4*)(x + (size_t)m * dim);
    for (int i = threadIdx.x; i < dim / 8; i += blockDim.x) dst[i] = src[i];
}

// ml.Argmax (operations_impl.go:513-548): strict '<' scan from -MaxFloat32 => first maximum wins, NaN and
// -inf are never selected (index -1 if nothing qualifies).  Parallel form: max value, lowest index.
// Also advances the device-resident greedy loop (inference.go:211-226): next token -> tokens[0], pos += 1.
DEVINL int argmax_block(const uint16_t* logits, int V, float* sv, int* si) {      // result valid in thread 0
    const int tid = threadIdx.x;
    float best = -3.40282346638528859811704183484516925440e+38f; int bi = -1;
    // 16 B loads, four in flight per thread (the scalar one-load-per-iteration form was pure latency: 42 us for V=128256);
    // each thread still visits its own elements in ascending index order, so '<' keeps the first maximum
    const int nv = ((((uintptr_t)logits) & 15) == 0) ? V >> 3 : 0;
    const uint4* l4 = (const uint4*)logits;
    for (int c0 = tid; c0 < nv; c0 += 4096) {
        uint4 w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int c = c0 + u * 1024; w[u] = l4[c < nv ? c : c0]; }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int c = c0 + u * 1024;
            if (c < nv) {
                const uint32_t q[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const float a = bf_lo(q[t]), b = bf_hi(q[t]);
                    if (best < a) { best = a; bi = c * 8 + 2 * t; }
                    if (best < b) { best = b; bi = c * 8 + 2 * t + 1; }
                }
            }
        }
    }
    for (int j = nv * 8 + tid; j < V; j += 1024) { float v = bf_wide(logits[j]); if (best < v) { best = v; bi = j; } }
    sv[tid] = best; si[tid] = bi;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) {
            float v2 = sv[tid + s]; int i2 = si[tid + s];
            float v1 = sv[tid]; int i1 = si[tid];
            bool take = (i2 >= 0) && (i1 < 0 || v1 < v2 || (v1 == v2 && i2 < i1));
            if (take) { sv[tid] = v2; si[tid] = i2; }
        }
        __syncthreads();
    }
    return si[0];
}
// What a step's token does to its generation (inference.go:211-226): the token word the next step embeds, the token log, the position, the stop ids --
// and nothing at all for a finished generation (see StepState).  The stop token itself is emitted (GSFinishedByReachingEOS).
DEVINL void step_advance(StepState* st, int tok, int32_t* token_word, int32_t* ring_word, int32_t* out_tokens, int out_cap) {
    if (st->finished) return;
    *token_word = tok;
    if (ring_word) *ring_word = tok;
    const int n = st->n_out;
    if (n < out_cap) out_tokens[n] = tok;
    st->n_out = n + 1;
    st->pos = st->pos + 1;
    if (st->honour_stop) for (int k = 0; k < st->n_stop; k++) if (tok == st->stop[k]) st->finished = 1;
}
__global__ __launch_bounds__(1024) void argmax_kernel(const uint16_t* logits, int V, int32_t* next_token, StepState* st,
                                                      int32_t* out_tokens, int out_cap, int advance) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    const int tok = argmax_block(logits, V, sv, si);
    if (threadIdx.x == 0) {
        if (!advance) next_token[0] = tok;
        else step_advance(st, tok, next_token, nullptr, out_tokens, out_cap);
    }
}
// the same for the batch: block s = sequence s's logits row; its context's token word, token log and position advance (inference.go:211-226)
__global__ __launch_bounds__(1024) void batch_argmax_kernel(const uint16_t* logits, int V, const BatchTab* tab, int32_t* ring) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    const int s = blockIdx.x;
    const int tok = argmax_block(logits + (size_t)s * V, V, sv, si);
    if (threadIdx.x == 0) {
        // a finished sequence keeps its token word, log and position (its column goes on computing the same step); ring (pipeline): the contiguous
        // words the last stage sends to the first
        step_advance(tab->st[s], tok, tab->dtok[s], ring ? ring + s : nullptr, tab->dout[s], tab->dout_cap[s]);
    }
}

// ---- seeded temperature / top-k / top-p sampling (lnb_decode_sample_until, include/lnb.h; the rule: lnb_sample.h) -------------------------
// One workgroup of 1024 lanes per logits row.  The row is read ONCE: lane l keeps the keys (lnb_sample_key of the scaled entry, 16 bits, 0 = no
// candidate) of the `per` consecutive entries [l * per, (l + 1) * per), per = ceil(V / 1024) rounded up to 8, packed two to a register -- at most
// 64 registers for V <= 131072.  So the layout is index order: lane-major, then the element inside the lane, and the two index-order prefix sums
// (ties at the threshold, kept weights) are a per-lane sum, one workgroup scan and a walk inside one lane.  Everything else is a register pass
// plus a workgroup reduction of integers (any order gives the same bits): the thresholds come from bisection on the key -- counts for top-k,
// weights for the nucleus -- and a weight is one lookup of the model's exp table by the key's bf16 pattern.
struct SampleSh {
    unsigned long long w[2][16];
    unsigned c[2][16];
    uint32_t keys[64];                                       // the lane that holds the draw hands its keys to the workgroup
    unsigned long long ex;
    unsigned tie0;
    int owner, tok;
    LnbSampleInfo z;                                         // filled as the sums become known (thread 0), copied out at the end
};
// (a reduction's result is the same in every lane: saying so keeps everything the thresholds are computed from in scalar registers)
DEVINL unsigned sample_uniform(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
DEVINL unsigned long long sample_uniform(unsigned long long v) {
    return ((unsigned long long)sample_uniform((unsigned)(v >> 32)) << 32) | sample_uniform((unsigned)v);
}
DEVINL void sample_wg_sum(SampleSh& sh, int& par, unsigned& c, unsigned long long& w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { c += __shfl_xor(c, o); w += __shfl_xor(w, o); }
    if ((threadIdx.x & 63) == 0) { sh.c[par][threadIdx.x >> 6] = c; sh.w[par][threadIdx.x >> 6] = w; }
    __syncthreads();                                         // (two slots: the next reduction writes the other one, the one after comes behind its barrier)
    c = 0; w = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) { c += sh.c[par][i]; w += sh.w[par][i]; }
    c = sample_uniform(c); w = sample_uniform(w);
    par ^= 1;
}
DEVINL unsigned sample_wg_min(SampleSh& sh, int& par, unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(v, o); v = t < v ? t : v; }
    if ((threadIdx.x & 63) == 0) sh.c[par][threadIdx.x >> 6] = v;
    __syncthreads();
    v = sh.c[par][0];
#pragma unroll
    for (int i = 1; i < 16; i++) v = sh.c[par][i] < v ? sh.c[par][i] : v;
    par ^= 1;
    return sample_uniform(v);
}
// exclusive prefix of v in lane order; total = the workgroup's sum
DEVINL unsigned long long sample_wg_scan(SampleSh& sh, int& par, unsigned long long v, unsigned long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) sh.w[par][wave] = inc;
    __syncthreads();
    unsigned long long base = 0; total = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) { const unsigned long long t = sh.w[par][i]; if (i < wave) base += t; total += t; }
    total = sample_uniform(total);
    par ^= 1;
    return base + inc - v;
}
// f(key) for the lane's keys in index order (per is a multiple of 8: the groups in use are the first per / 8)
template <class F> DEVINL void sample_each(const uint32_t (&kr)[64], int per, F f) {
#pragma unroll
    for (int q = 0; q < 16; q++) {
        if (q * 8 < per) {
#pragma unroll
            for (int t = 0; t < 4; t++) { f(kr[q * 4 + t] & 0xffffu); f(kr[q * 4 + t] >> 16); }
        }
    }
}
// g(eight keys) group by group; the fence keeps one group's table lookups in flight at a time (their registers are the keys').  The empty asm
// statements make `per` and the packed keys opaque per pass: otherwise the sixteen group conditions, the 128 unpacked keys and their table offsets are
// hoisted out of the bisection loop -- into spilled scalar registers and into scratch.  They emit no instruction; like the fences they steer THIS compiler's
// schedule and register allocation, so "no scratch" is a property of the build, not of the source: tools/isa_audit.py (tests/test_isa_audit.py) checks the
// compiled kernels' scratch size and VGPR spill count on every build, and a compiler that spills here anyway fails that test instead of running slowly.
template <class G> DEVINL void sample_groups(uint32_t (&kr)[64], int per, G g) {
    asm volatile("" : "+s"(per));
#pragma unroll
    for (int q = 0; q < 16; q++) {
        if (q * 8 < per) {
#pragma unroll
            for (int t = 0; t < 4; t++) asm volatile("" : "+v"(kr[q * 4 + t]));
            const unsigned k8[8] = {kr[q * 4] & 0xffffu, kr[q * 4] >> 16, kr[q * 4 + 1] & 0xffffu, kr[q * 4 + 1] >> 16,
                                    kr[q * 4 + 2] & 0xffffu, kr[q * 4 + 2] >> 16, kr[q * 4 + 3] & 0xffffu, kr[q * 4 + 3] >> 16};
            g(k8);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}
DEVINL unsigned long long sample_key_weight(const double* etab, unsigned key, int E) {
    return lnb_sample_weight((unsigned long long)__double_as_longlong(etab[lnb_sample_key_bits(key)]), E);
}
// -> the token, valid in thread 0, and sh.z = the row's info.  has_u: pos_or_u is u of step 8 itself.
DEVINL int sample_block(const uint16_t* x, int V, const double* etab, const LnbSampler& s, bool has_u, unsigned long long pos_or_u, SampleSh& sh) {
    const int tid = threadIdx.x;
    int par = 0;
    if (tid == 0) { const LnbSampleInfo z0 = {0, 0, 0, 0, 0, 0, 0}; sh.z = z0; }      // (read back by thread 0 only)
    const float T = s.temperature;
    const int per = (((V + 1023) >> 10) + 7) & ~7;
    // the row, once: scaled (step 1), keyed (steps 2 and 5), packed
    uint32_t kr[64];
    const bool al = (((uintptr_t)x) & 15) == 0;
    auto key_of = [&](uint16_t b) -> uint32_t { return lnb_sample_key(T == 1.0f ? b : lnb_sample_scale(b, T)); };
#pragma unroll
    for (int q = 0; q < 16; q++) {
        if (q * 8 < per) {
            const int j0 = tid * per + q * 8;
            if (al && j0 + 8 <= V) {
                const uint4 v = *(const uint4*)(x + j0);
                const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int t = 0; t < 4; t++) kr[q * 4 + t] = key_of((uint16_t)(wd[t] & 0xffffu)) | (key_of((uint16_t)(wd[t] >> 16)) << 16);
            } else {
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int j = j0 + 2 * t;
                    const uint32_t lo = j < V ? key_of(x[j]) : 0u, hi = j + 1 < V ? key_of(x[j + 1]) : 0u;
                    kr[q * 4 + t] = lo | (hi << 16);
                }
            }
            if (q & 1) __builtin_amdgcn_sched_barrier(0);    // (two 16 B loads in flight: with all sixteen hoisted, the raw words and the keys would not fit)
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++) kr[q * 4 + t] = 0;
        }
    }
    // step 3: the largest key and its first index
    unsigned kmax_l = 0;
    sample_each(kr, per, [&](unsigned k) { kmax_l = k > kmax_l ? k : kmax_l; });
    const unsigned kmax = ~sample_wg_min(sh, par, ~kmax_l);
    if (kmax == 0) return -1;                                            // no candidate
    unsigned a_l = 0xffffffffu, e_l = 0;
    sample_each(kr, per, [&](unsigned k) { if (k == kmax && a_l == 0xffffffffu) a_l = (unsigned)(tid * per) + e_l; e_l++; });
    const int a = (int)sample_wg_min(sh, par, a_l);
    const unsigned long long emax = (unsigned long long)__double_as_longlong(etab[lnb_sample_key_bits(kmax)]);
    if (lnb_sample_degenerate(emax)) { if (tid == 0) sh.z.degenerate = 1; return a; }
    const int E = lnb_sample_exponent(emax);
    // step 4: S = the keys >= kmin, kmin = the smallest key of weight >= 1 (the weight grows with the key).  Two rounds of 1024 probes.
    unsigned kmin;
    {
        const unsigned lo0 = 0x80u, step = (kmax - lo0 + 1023u) >> 10;           // probes lo0 + (i + 1) * step, the last ones clamped to kmax (weight >= 2^45)
        unsigned k = lo0 + ((unsigned)tid + 1u) * step; k = k > kmax ? kmax : k;
        const unsigned k1 = sample_wg_min(sh, par, sample_key_weight(etab, k, E) >= 1 ? k : 0xffffffffu);
        const unsigned lo1 = k1 > lo0 + step ? k1 - step : lo0;                  // weight(lo1) == 0 (a probe that failed) or lo1 is no candidate's key
        unsigned k2 = lo1 + 1u + (unsigned)tid; k2 = k2 > k1 ? k1 : k2;          // step <= 64: the probes lo1 + 1 .. k1
        kmin = sample_wg_min(sh, par, sample_key_weight(etab, k2, E) >= 1 ? k2 : 0xffffffffu);
    }
    // Steps 6 and 7 as ONE loop around one tally -- (count, weight) of the entries whose key is >= t, t >= kmin: the weight of all of S, then the
    // bisection for top-k on counts, the weight above its threshold, the bisection for the nucleus on weights, and last the weight above the final
    // threshold t2, whose per-lane part feeds the index-order prefix sum.  (t, m) = a threshold key and the ties kept at it, lowest indices first;
    // t = kmin - 1, m = 0 keeps all of S.
    enum { PH_ALL, PH_TOPK, PH_TOPK_W, PH_TOPP, PH_LAST, PH_DONE };
    const bool do_p = s.top_p < 1.0f;
    unsigned t1 = kmin - 1, m1 = 0, n1 = 0, t2 = 0, m2 = 0, nk = 0, kk = 0;
    unsigned long long w1 = 0, P = 0;
    unsigned lo = 0, hi = 0, c_hi = 0; unsigned long long w_hi = 0;
    unsigned t = kmin, lane_t = 0; bool want_w = true; int ph = PH_ALL;
    unsigned long long lane_w = 0;                                               // this lane's part of the last weight tally, which was for t = lane_t
    auto begin_last = [&]() {
        if (lane_t == t2 + 1) ph = PH_DONE; else { t = t2 + 1; want_w = true; ph = PH_LAST; }
    };
    auto next_topp = [&]() {
        if (hi - lo > 1) { t = lo + ((hi - lo) >> 1); want_w = true; ph = PH_TOPP; return; }
        const unsigned long long wt = sample_key_weight(etab, lo, E);           // kept weight(>= lo) >= P > weight(>= hi), hi = lo + 1
        unsigned long long need = P > w_hi ? (P - w_hi + wt - 1) / wt : 0;
        if (need < 1) need = 1;                                                  // at least one entry
        if (lo == t1 && need > m1) need = m1;
        t2 = lo; m2 = (unsigned)need; nk = c_hi + m2;
        begin_last();
    };
    auto start_topp = [&]() {
        if (!do_p) { if (tid == 0) sh.z.w_topk = w1; t2 = t1; m2 = m1; nk = n1; begin_last(); return; }
        if (tid == 0) sh.z.w_topk = w1;
        P = lnb_sample_p(s.top_p, w1);
        lo = P == 0 ? kmax : t1; hi = kmax + 1; c_hi = 0; w_hi = 0;              // above t1 the kept weight is the plain one; P == 0 keeps the first entry
        next_topp();
    };
    auto next_topk = [&]() {
        if (hi - lo > 1) { t = lo + ((hi - lo) >> 1); want_w = false; ph = PH_TOPK; }
        else { t = lo + 1; want_w = true; ph = PH_TOPK_W; }                      // count(>= lo) >= kk > count(>= hi) = c_hi
    };
    while (ph != PH_DONE) {
        unsigned c = 0; unsigned long long w = 0;
        if (!want_w) sample_each(kr, per, [&](unsigned k) { c += 1u + (unsigned)((int)(k - t) >> 31); });      // (keys are 16 bits: the sign of k - t)
        else {
            // Branch-free and select-free (eight entries side by side would otherwise hold eight compare masks in scalar registers): every lane looks
            // up max(key, t) -- a valid pattern, t >= kmin -- eight lookups in flight; an entry below t then adds weight(t), taken off again at the end
            unsigned seen = 0;
            sample_groups(kr, per, [&](const unsigned (&k8)[8]) {
                unsigned gm = k8[0];
#pragma unroll
                for (int i = 1; i < 8; i++) gm = k8[i] > gm ? k8[i] : gm;
                if (!__any(gm >= t)) return;                                     // (wave-uniform: near the top of the row most groups hold nothing)
                unsigned long long e8[8];
#pragma unroll
                for (int i = 0; i < 8; i++) e8[i] = (unsigned long long)__double_as_longlong(etab[lnb_sample_key_bits(k8[i] > t ? k8[i] : t)]);
#pragma unroll
                for (int i = 0; i < 8; i++) { c += 1u + (unsigned)((int)(k8[i] - t) >> 31); w += lnb_sample_weight(e8[i], E); }
                seen += 8;
            });
            w -= (unsigned long long)(seen - c) * sample_key_weight(etab, t, E);
        }
        if (want_w) { lane_w = w; lane_t = t; }
        sample_wg_sum(sh, par, c, w);
        if (ph == PH_ALL) {
            n1 = c; w1 = w;
            if (tid == 0) { sh.z.n_candidates = (int)c; sh.z.w_all = w; }
            if (s.top_k > 0 && (unsigned)s.top_k < c) { kk = (unsigned)s.top_k; lo = kmin; hi = kmax + 1; c_hi = 0; next_topk(); }
            else start_topp();
        } else if (ph == PH_TOPK) {
            if (c >= kk) lo = t; else { hi = t; c_hi = c; }
            next_topk();
        } else if (ph == PH_TOPK_W) {
            t1 = lo; m1 = kk - c_hi; n1 = kk;
            w1 = w + (unsigned long long)m1 * sample_key_weight(etab, t1, E);
            start_topp();
        } else if (ph == PH_TOPP) {
            if (w >= P) lo = t; else { hi = t; c_hi = c; w_hi = w; }
            next_topp();
        } else ph = PH_DONE;                                                     // PH_LAST
    }
    // the ties at t2 in index order: this lane's first tie has rank tie0; the lane's kept weight = what it holds above t2 + its kept ties
    unsigned long long ties_l = 0, ties_all;
    sample_each(kr, per, [&](unsigned k) { if (k == t2) ties_l++; });
    const unsigned long long tie0 = sample_wg_scan(sh, par, ties_l, ties_all);
    if (m2 > ties_all) m2 = (unsigned)ties_all;                                  // (t2 = kmin - 1: no tie is kept, none is wanted)
    const unsigned long long ties_in = tie0 >= m2 ? 0 : (m2 - tie0 < ties_l ? m2 - tie0 : ties_l);
    const unsigned long long wl = lane_w + (ties_in ? ties_in * sample_key_weight(etab, t2, E) : 0);
    // step 8: the kept weights in index order -- the lane whose span holds r, then the entry inside it
    unsigned long long wk;
    const unsigned long long ex = sample_wg_scan(sh, par, wl, wk);
    const unsigned long long u = has_u ? pos_or_u : lnb_sample_draw(s.seed, (int)pos_or_u);
    const unsigned long long r = lnb_sample_mulhi(u, wk);
    if (tid == 0) { sh.tok = -1; sh.z.w_kept = wk; sh.z.n_kept = (int)nk; }
    if (wl > 0 && ex <= r && r < ex + wl) {                                      // exactly one lane
#pragma unroll
        for (int i = 0; i < 64; i++) sh.keys[i] = kr[i];
        sh.owner = tid; sh.ex = ex; sh.tie0 = (unsigned)tie0;
    }
    __syncthreads();
    {
        const unsigned k = tid < per ? (sh.keys[tid >> 1] >> ((tid & 1) * 16)) & 0xffffu : 0u;
        unsigned long long tt;
        const unsigned long long rank = sh.tie0 + sample_wg_scan(sh, par, k == t2 && tid < per ? 1ull : 0ull, tt);
        const bool member = tid < per && (k > t2 || (k == t2 && rank < m2));
        const unsigned long long wv = member ? sample_key_weight(etab, k, E) : 0;
        const unsigned long long exv = sh.ex + sample_wg_scan(sh, par, wv, tt);
        if (member && exv <= r && r < exv + wv) sh.tok = sh.owner * per + tid;
    }
    __syncthreads();
    return sh.tok;
}
// What thread 0 needs AFTER the row is sampled -- where the token goes -- waits in the LDS meanwhile instead of in scalar registers across the bisection
// loop, which uses nearly all of them (a dozen scalars are still parked in the lanes of one vector register around it: no memory, tools/isa_audit.py).
struct SampleEnd { StepState* st; int32_t* token_word; int32_t* out_tokens; LnbSampleInfo* info; int out_cap, advance; };
// sample_kernel: argmax_kernel with the sampler's token (advance: the decode loop's step; its position is the state's).  advance == 0: block i = row i
// of lnb_op_sample -- its own sampler, position, optional u and info.  temperature 0 = argmax_block on the raw row.
__global__ __launch_bounds__(1024) void sample_kernel(const uint16_t* logits, int V, const double* etab, const LnbSampler* smp, int32_t* next_token,
                                                      StepState* st, int32_t* out_tokens, int out_cap, int advance, const int32_t* op_pos,
                                                      const unsigned long long* op_draws, LnbSampleInfo* op_info) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    __shared__ SampleSh sh;
    __shared__ SampleEnd end;
    const int row = advance ? 0 : blockIdx.x;
    const LnbSampler s = smp[row];
    const uint16_t* x = logits + (size_t)row * V;
    const bool has_u = !advance && op_draws != nullptr;
    const unsigned long long pos_or_u = advance ? (unsigned long long)(long long)st->pos : has_u ? op_draws[row] : (unsigned long long)(long long)op_pos[row];
    if (threadIdx.x == 0) {
        end.st = st; end.token_word = next_token + row; end.out_tokens = out_tokens; end.out_cap = out_cap; end.advance = advance;
        end.info = !advance && op_info ? op_info + row : nullptr;
        const LnbSampleInfo z0 = {0, 0, 0, 0, 0, 0, 0}; sh.z = z0;             // (what a greedy row reports)
    }
    int tok;
    if (s.temperature == 0.0f) tok = argmax_block(x, V, sv, si);
    else tok = sample_block(x, V, etab, s, has_u, pos_or_u, sh);
    if (threadIdx.x == 0) {
        if (end.info) *end.info = sh.z;
        if (!end.advance) *end.token_word = tok;
        else step_advance(end.st, tok, end.token_word, nullptr, end.out_tokens, end.out_cap);
    }
}
// the same for the batch: block s = sequence s's logits row, sampler s, its context's position
__global__ __launch_bounds__(1024) void batch_sample_kernel(const uint16_t* logits, int V, const double* etab, const LnbSampler* smp, const BatchTab* tab) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    __shared__ SampleSh sh;
    __shared__ SampleEnd end;
    const int q = blockIdx.x;
    const LnbSampler s = smp[q];
    const uint16_t* x = logits + (size_t)q * V;
    const unsigned long long pos = (unsigned long long)(long long)tab->st[q]->pos;
    if (threadIdx.x == 0) { end.st = tab->st[q]; end.token_word = tab->dtok[q]; end.out_tokens = tab->dout[q]; end.out_cap = tab->dout_cap[q]; }
    const int tok = s.temperature == 0.0f ? argmax_block(x, V, sv, si) : sample_block(x, V, etab, s, false, pos, sh);
    if (threadIdx.x == 0) step_advance(end.st, tok, end.token_word, nullptr, end.out_tokens, end.out_cap);
}

// ---- speculative greedy decoding (lnb_decode_speculative_until, include/lnb.h) ----------------------------------------------------------
// A verify pass is a batched step whose w columns alias one context (DraftParams, lnb_device.h): column i's logits row is the one-token step
// at pos + i, bit for bit.  spec_argmax_kernel: block i = ml.Argmax of column i's row (argmax_block, the greedy loop's rule).
__global__ __launch_bounds__(1024) void spec_argmax_kernel(const uint16_t* logits, int V, int32_t* g) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    const int i = blockIdx.x;
    const int tok = argmax_block(logits + (size_t)i * V, V, sv, si);
    if (threadIdx.x == 0) g[i] = tok;
}
// After the verify pass: a = the longest prefix of columns whose argmax equals the next column's input (the draft d_{i+1}); the argmax of
// columns 0 .. a is emitted in order, exactly as a greedy step emits its token -- token log, position, the context's token word, and the stop
// ids (the stop token is emitted and freezes the generation: nothing behind it).  Column 0 is the context's own state (tab->st[0]).
// (spec_accept_emit: one thread; shared with spec_sample_commit_kernel, whose g holds the sampler's tokens -- the same loop for both)
DEVINL void spec_accept_emit(const int32_t* g, int w, const BatchTab* tab) {
    StepState* st = tab->st[0];
    if (st->finished) return;
    int a = 0;
    while (a < w - 1 && g[a] == *tab->dtok[a + 1]) a++;
    for (int i = 0; i <= a; i++) {
        const int tok = g[i];
        const int n = st->n_out;
        if (n < tab->dout_cap[0]) tab->dout[0][n] = tok;
        st->n_out = n + 1;
        st->pos = st->pos + 1;
        *tab->dtok[0] = tok;
        bool stop = false;
        if (st->honour_stop) for (int k = 0; k < st->n_stop; k++) if (tok == st->stop[k]) stop = true;
        if (stop) { st->finished = 1; break; }
    }
}
__global__ void spec_commit_kernel(const int32_t* g, int w, const BatchTab* tab) {
    if (threadIdx.x != 0) return;
    spec_accept_emit(g, w, tab);
}
// ---- sampling in the speculative loop (lnb_decode_speculative_sample_until) --------------------------------------------------------------
// The sampler's draw is u(seed, pos) and nothing else, so the token the sampling loop emits at position p is sample(row_p, sampler, p): column i of a
// verify pass has row_{pos + i} exactly, and the greedy acceptance rule holds with "the sampler's token of column i AT POSITION pos + i" in place of
// the argmax.  spec_sample_commit_kernel: workgroup i samples column i's row at tab->st[i]->pos (column 0: the context's own state; columns 1..: what
// ngram_draft_kernel wrote, pos + i) -> g[i]; the last workgroup to arrive (agent-scope ticket, as ngram_draft_kernel's) runs spec_accept_emit.  One
// launch in place of spec_argmax_kernel + spec_commit_kernel.  What the epilogue needs waits in the LDS across sample_block (see SampleEnd).
struct SpecSampleEnd { int32_t* g; unsigned* cnt; const BatchTab* tab; int w, last; };
__global__ __launch_bounds__(1024) void spec_sample_commit_kernel(const uint16_t* logits, int V, const double* etab, const LnbSampler* smp, int32_t* g,
                                                                  const BatchTab* tab, unsigned* cnt) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    __shared__ SampleSh sh;
    __shared__ SpecSampleEnd end;
    const int i = blockIdx.x;
    const LnbSampler s = smp[0];
    const uint16_t* x = logits + (size_t)i * V;
    const unsigned long long pos = (unsigned long long)(long long)tab->st[i]->pos;
    if (threadIdx.x == 0) { end.g = g; end.cnt = cnt; end.tab = tab; end.w = (int)gridDim.x; end.last = 0; }
    const int tok = s.temperature == 0.0f ? argmax_block(x, V, sv, si) : sample_block(x, V, etab, s, false, pos, sh);
    if (threadIdx.x != 0) return;
    end.g[i] = tok;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const unsigned t = __hip_atomic_fetch_add(end.cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (t != (unsigned)end.w - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    *end.cnt = 0;                                            // (ready for the next launch: stream order)
    spec_accept_emit(end.g, end.w, end.tab);
}
DEVINL int32_t spec_text_at(const DraftParams& p, int j) { return j < p.n_text ? p.text[j] : p.gen[j - p.n_text]; }
// N-gram (prompt lookup) draft of the next pass.  Workgroup b tries n = ngram_max - b: the latest start j in R = text ++ gen of an earlier
// occurrence of R's last n tokens with at least one token after it (j <= L - n - 1: R's own final suffix is no match), and the same in the
// corpus (j <= n_corpus - n - 1).  The last workgroup to arrive (agent-scope ticket) picks the longest n that matched, R before C, and takes
// up to max_draft tokens after the match, cut at the end of its array and -- decoding -- at max_steps - n_out - 1 and seq_len - pos - 1.
// It writes the draft into the column token words out[1 ..], the columns' positions pos + i, and {draft_len, n_out, finished}.
// ngram_search_block: the search of ONE n by one workgroup (all its threads call it; suf [LNB_SPEC_MAX_NGRAM] and sbest [2] are its LDS) -> after
// the call sbest = {latest match start in R, in C} (-1: none).  ngram_pick: what the last workgroup makes of the `count` results in p.best
// (result q belongs to n = ngram_max - q) -> the draft length after every cut, *src = 0 R / 1 C, *start = the draft's first token in that array.
// Shared by ngram_draft_kernel and spec_many_draft_kernel (lnb_spec_many.h): one rule, one body.
DEVINL void ngram_search_block(const DraftParams& p, int n, int L, int32_t* suf, int* sbest) {
    const int tid = threadIdx.x;
    if (tid < 2) sbest[tid] = -1;
    if (tid < n && n <= L) suf[tid] = spec_text_at(p, L - n + tid);
    __syncthreads();
    if (n < L) {                                             // descending per thread: its first hit is its latest
        int mine = -1;
        for (int j = L - n - 1 - tid; j >= 0; j -= (int)blockDim.x) {
            bool ok = true;
            for (int t = 0; t < n && ok; t++) ok = spec_text_at(p, j + t) == suf[t];
            if (ok) { mine = j; break; }
        }
        if (mine >= 0) atomicMax(&sbest[0], mine);
    }
    if (n <= L && p.n_corpus > n) {
        int mine = -1;
        for (int j = p.n_corpus - n - 1 - tid; j >= 0; j -= (int)blockDim.x) {
            bool ok = true;
            for (int t = 0; t < n && ok; t++) ok = p.corpus[j + t] == suf[t];
            if (ok) { mine = j; break; }
        }
        if (mine >= 0) atomicMax(&sbest[1], mine);
    }
    __syncthreads();
}
DEVINL int ngram_pick(const DraftParams& p, int count, int L, int n_gen, int* src_out, int* start_out) {
    int src = -1, start = 0, avail = 0;
    for (int q = 0; q < count && src < 0; q++) {
        const int r = p.best[2 * q], c = p.best[2 * q + 1], nq = p.ngram_max - q;
        if (r >= 0) { src = 0; start = r + nq; avail = L - start; }
        else if (c >= 0) { src = 1; start = c + nq; avail = p.n_corpus - start; }
    }
    int k = src < 0 ? 0 : min(avail, p.max_draft);
    if (p.st) {
        k = min(k, min(p.max_steps - n_gen - 1, p.seq_len - p.st->pos - 1));
        if (p.st->finished || k < 0) k = 0;
    }
    *src_out = src; *start_out = start;
    return k;
}
__global__ __launch_bounds__(256) void ngram_draft_kernel(DraftParams p) {
    __shared__ int32_t suf[LNB_SPEC_MAX_NGRAM];
    __shared__ int sbest[2];
    __shared__ int s_last;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = p.ngram_max - b;
    const int n_gen = p.st ? p.st->n_out : 0;
    const int L = p.n_text + n_gen;
    ngram_search_block(p, n, L, suf, sbest);
    if (tid == 0) {
        p.best[2 * b] = sbest[0];
        p.best[2 * b + 1] = sbest[1];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned t = __hip_atomic_fetch_add(p.cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last || tid != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    *p.cnt = 0;                                              // (ready for the next launch: stream order)
    int src = -1, start = 0;
    const int k = ngram_pick(p, (int)gridDim.x, L, n_gen, &src, &start);
    const int finished = p.st ? p.st->finished : 0, pos = p.st ? p.st->pos : 0;
    for (int i = 0; i < k; i++) p.out[1 + i] = src == 0 ? spec_text_at(p, start + i) : p.corpus[start + i];
    if (p.col_st) for (int i = 1; i <= k; i++) p.col_st[i].pos = pos + i;
    p.word[0] = k; p.word[1] = n_gen; p.word[2] = finished;
}

// ---- token probabilities: what the reference's Softmax (operations_impl.go:478-511) gives for one logits row, and ml.Argmax's top k ----
// prob(j) = f32(e_j / Z) with e_j = exp(f64(x_j)) and Z = sum_{j ascending} e_j in f64 -- the reference's serial order.  e comes from
// a table of the host C library's exp for all 65536 bf16 patterns (p.etab), so the device evaluates no transcendental here.
// Per workgroup (slice of a row): a partial f64 sum in any order + a top-k per lane in registers; the LAST workgroup of the row to arrive
// (agent-scope ticket) merges them into the estimate Zt and the row's top k, and certifies each reported probability against the serial
// Z: |Z - Zt| <= (4V + 8) 2^-53 Zt (cert_z, T = V), so a quotient that lies further than that from the one point of its f32 cell where
// round-to-nearest changes (the midpoint: low 29 bits of the f64 mantissa = 2^28) is the reference's bits.  Anything else -- a quotient
// in the band, an f32-denormal quotient whose ends disagree, a row with Zt zero, inf or NaN, or force_serial -- walks the serial sum on
// one wave and recomputes every reported probability from the exact Z.
// Top-k order = ml.Argmax's (operations_impl.go:529-541, strict '<' from -MaxFloat32): candidates are > -MaxFloat32 (never NaN), value
// descending, lowest index first on ties.  As one 64-bit key: (order-preserving bits of the value, -0 folded into +0) << 32 | ~index;
// 0 = no entry.
DEVINL uint64_t tp_key(float v, int j) {
    if (!(v > -3.40282346638528859811704183484516925440e+38f)) return 0;
    const uint32_t u = __float_as_uint(v + 0.0f);            // (-0 + 0 = +0: ml.Argmax sees the two zeros as equal)
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)o << 32) | (uint32_t)~(uint32_t)j;
}
DEVINL int tp_key_index(uint64_t key) { return (int)~(uint32_t)key; }
template <int KT> DEVINL void tp_insert(uint64_t (&lk)[KT], uint64_t key) {     // lk sorted descending; key > lk[KT - 1]
#pragma unroll
    for (int r = KT - 1; r > 0; r--) lk[r] = key > lk[r - 1] ? lk[r - 1] : (key > lk[r] ? key : lk[r]);
    lk[0] = key > lk[0] ? key : lk[0];
}
DEVINL uint64_t tp_wave_max(uint64_t v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { const uint64_t o = __shfl_xor(v, s, 64); v = o > v ? o : v; }
    return v;
}
DEVINL double tp_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}
// the wave's k largest keys (one sorted list per lane) in descending order: k rounds of a wave maximum, the winning lane pops its head
template <int KT> DEVINL void tp_wave_topk(uint64_t (&lk)[KT], int k, uint64_t* dst) {
    for (int r = 0; r < k; r++) {
        const uint64_t m = tp_wave_max(lk[0]);
        if ((threadIdx.x & 63) == 0) dst[r] = m;
        if (m != 0 && lk[0] == m) {
#pragma unroll
            for (int q = 0; q < KT - 1; q++) lk[q] = lk[q + 1];
            lk[KT - 1] = 0;
        }
    }
}
// f32-cell form of cert_p: p = f32(e / Z) (round to nearest) from the estimate; sets bad when Z's band may move it to another f32
DEVINL float cert_p32(double e, const CertZ& c, int& bad) {
    const double q = e * c.rzt;
    const float pj = (float)q;
    const unsigned qh = (unsigned)__double2hiint(q), ql = (unsigned)__double2loint(q);
    const unsigned eq = (qh >> 20) & 0x7FFu;
    if (eq - 897u <= 126u) {                                 // f32-normal quotient (2^-126 <= q < 2): distance from its cell's rounding midpoint
        if ((ql & 0x1FFFFFFFu) - (0x10000000u - c.delta32) <= 2u * c.delta32) bad = 1;
    } else if (q != 0.0) {                                   // f32 denormals (and anything out of range): both ends of the band
        const float plo = (float)(e / c.zlo), phi = (float)(e / c.zhi);
        if (__float_as_uint(plo) != __float_as_uint(phi) || __float_as_uint(pj) != __float_as_uint(plo)) bad = 1;
    }
    return pj;
}
DEVINL double tp_readlane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// the reference's serial sum over the row (impl:492-499: rowExpSum += exp, j ascending), walked by ONE wave: 256 table values per
// round gathered by the lanes (the next round's in flight), then added in index order by every lane
DEVINL double tp_zseq_wave(const uint16_t* x, int V, const double* etab) {
    const int lane = threadIdx.x & 63;
    auto gather = [&](int base, double (&e)[4]) {
#pragma unroll
        for (int u = 0; u < 4; u++) { const int j = base + u * 64 + lane; e[u] = j < V ? etab[x[j]] : 0.0; }     // (+0 added past the end: exact)
    };
    double z = 0.0, a[4], b[4];
    gather(0, a);
    for (int base = 0; base < V; base += 256) {
        gather(base + 256, b);
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll 16
            for (int l = 0; l < 64; l++) z += tp_readlane(a[u], l);
#pragma unroll
        for (int u = 0; u < 4; u++) a[u] = b[u];
    }
    return z;
}
template <int KT> __global__ __launch_bounds__(256) void token_probs_kernel(TokProbParams p) {
    constexpr int KA = KT > 0 ? KT : 1;                      // (KT = 0: scoring only, no top-k)
    __shared__ uint64_t sk[4 * KA];
    __shared__ double sz[4 * LNB_TOKPROB_MAX_G];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.y, g = blockIdx.x, G = p.G, V = p.V, k = p.k;
    const uint16_t* x = p.logits + (size_t)row * V;
    const TokProbOut& o = p.out[p.per_row_out ? row : 0];
    int slot = row;
    if (o.st) {                                              // (the argmax that advances the state runs after this launch)
        if (o.st->finished || o.st->n_out >= o.cap) return;  // a finished generation records nothing (every workgroup of the row agrees)
        slot = o.st->n_out;
    }
    // this workgroup's slice: the unaligned head (workgroup 0), 16-byte chunks, the tail (workgroup G - 1)
    int h = (int)((16 - (((uintptr_t)x) & 15)) & 15) >> 1;
    if (h > V) h = V;
    const int nb = (V - h) >> 3, tail0 = h + nb * 8;
    const uint4* l4 = (const uint4*)(x + h);
    uint64_t lk[KA];
#pragma unroll
    for (int r = 0; r < KA; r++) lk[r] = 0;
    auto visit = [&](uint16_t b, int j) {
        if constexpr (KT > 0) { const uint64_t key = tp_key(bf_wide(b), j); if (key > lk[KA - 1]) tp_insert<KA>(lk, key); }
    };
    // Zt is summed over LNB_TOKPROB_MAX_G fixed sub-slices of the row in a fixed order whatever G is (G divides it): a row's estimate, hence
    // its ln Z and whether it walks, is the same in every launch shape (one sequence, a batch, scoring)
    const int S = LNB_TOKPROB_MAX_G / G;
    double mine = 0.0;                                       // lane l: the wave's sum of sub-slice l
    for (int v = 0; v < S; v++) {
        const int vs = g * S + v;
        const int c0 = (int)((long)nb * vs / LNB_TOKPROB_MAX_G), c1 = (int)((long)nb * (vs + 1) / LNB_TOKPROB_MAX_G);
        double zs = 0.0;
        if (vs == 0 && tid < h) { zs += p.etab[x[tid]]; visit(x[tid], tid); }
        if (vs == LNB_TOKPROB_MAX_G - 1 && tail0 + tid < V) { zs += p.etab[x[tail0 + tid]]; visit(x[tail0 + tid], tail0 + tid); }
        for (int c = c0 + tid; c < c1; c += 512) {               // two chunks in flight: 16 table gathers before the first add
            const bool two = c + 256 < c1;
            const uint4 wa = l4[c], wb = l4[two ? c + 256 : c];
            const uint32_t q[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
            double e[16];
#pragma unroll
            for (int t = 0; t < 16; t++) e[t] = p.etab[(t & 1) ? (q[t >> 1] >> 16) : (q[t >> 1] & 0xFFFFu)];
#pragma unroll
            for (int t = 0; t < 8; t++) zs += e[t];
            if (two) {
#pragma unroll
                for (int t = 8; t < 16; t++) zs += e[t];
            }
            if constexpr (KT > 0) {
#pragma unroll
                for (int t = 0; t < 16; t++) {
                    if (t >= 8 && !two) break;
                    const int cc = t < 8 ? c : c + 256;
                    visit((uint16_t)((t & 1) ? (q[t >> 1] >> 16) : (q[t >> 1] & 0xFFFFu)), h + cc * 8 + (t & 7));
                }
            }
        }
        zs = tp_wave_sum(zs);
        if (lane == vs) mine = zs;
    }
    // the workgroup's sub-slice sums and top k -> this slice's partials
    sz[wave * LNB_TOKPROB_MAX_G + lane] = mine;
    if constexpr (KT > 0) tp_wave_topk<KA>(lk, k, sk + wave * KA);
    __syncthreads();
    if (wave == 0) {
        uint64_t key = (KT > 0 && lane < 4 * KA && lane % KA < k) ? sk[lane] : 0;
        for (int r = 0; r < k; r++) {                        // the four waves' lists: one key per lane, k rounds
            const uint64_t m = tp_wave_max(key);
            if (m != 0 && key == m) key = 0;
            if (lane == 0) p.kpart[((size_t)row * G + g) * k + r] = m;
        }
        if (lane >= g * S && lane < (g + 1) * S) {
            constexpr int M = LNB_TOKPROB_MAX_G;
            p.zpart[(size_t)row * M + lane] = (sz[lane] + sz[M + lane]) + (sz[2 * M + lane] + sz[3 * M + lane]);
        }
        if (lane == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            const unsigned t = __hip_atomic_fetch_add(p.cnt + row, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            s_last = t == (unsigned)G - 1;
        }
    }
    __syncthreads();
    if (!s_last || wave != 0) return;
    // ---- the last workgroup of the row, one wave: merge the G slices, certify, walk if needed, report ----
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (lane == 0) p.cnt[row] = 0;                           // (ready for the next launch: stream order)
    const double zt = tp_wave_sum(p.zpart[(size_t)row * LNB_TOKPROB_MAX_G + lane]);
    uint64_t top = 0;                                        // lane r < k: the row's r-th entry
    if constexpr (KT > 0) {
        uint64_t mk[KA];
#pragma unroll
        for (int r = 0; r < KA; r++) mk[r] = (lane < G && r < k) ? p.kpart[((size_t)row * G + lane) * k + r] : 0;
        for (int r = 0; r < k; r++) {
            const uint64_t m = tp_wave_max(mk[0]);
            if (lane == r) top = m;
            if (m != 0 && mk[0] == m) {
#pragma unroll
                for (int q = 0; q < KA - 1; q++) mk[q] = mk[q + 1];
                mk[KA - 1] = 0;
            }
        }
    }
    // lanes 0..k-1: the top entries; lane 32: the scoring target
    int id = -1;
    if (lane < k && top != 0) id = tp_key_index(top);
    if (lane == 32 && p.targets) { const int t = p.targets[row]; if (t >= 0 && t < V) id = t; }
    const uint16_t b = id >= 0 ? x[id] : (uint16_t)0;
    const double e = id >= 0 ? p.etab[b] : 0.0;
    const CertZ cz = cert_z(zt, V);
    int bad = p.force_serial || !(zt > 0.0) || !(cz.zhi <= 1.7976931348623157e308);
    float pr = 0.0f;
    if (id >= 0) pr = cert_p32(e, cz, bad);
    double z = zt;
    if (__any(bad)) {
        z = tp_zseq_wave(x, V, p.etab);
        if (id >= 0) pr = (float)(e / z);
        if (lane == 0 && o.walks) atomicAdd(o.walks, 1);
    }
    const float qnan = __uint_as_float(0x7FC00000u);
    if (lane < k) {
        const size_t at = (size_t)slot * k + lane;
        o.ids[at] = id;
        o.logit[at] = id >= 0 ? bf_wide(b) : qnan;
        o.prob[at] = id >= 0 ? pr : qnan;
    }
    if (lane == 0 && o.log_z) o.log_z[slot] = log(z);
    if (lane == 32 && p.targets) { p.tlogit[row] = id >= 0 ? bf_wide(b) : qnan; p.tprob[row] = id >= 0 ? pr : qnan; }
}

__global__ void set_state_kernel(StepState* st, int pos, int n_out, int honour_stop) { st->pos = pos; st->n_out = n_out; st->finished = 0; st->honour_stop = honour_stop; }
struct StopIds { int32_t n; int32_t id[LNB_MAX_STOP_IDS]; };
__global__ void set_stop_kernel(StepState* st, StopIds s) { st->n_stop = s.n; for (int k = 0; k < LNB_MAX_STOP_IDS; k++) st->stop[k] = k < s.n ? s.id[k] : -1; st->finished = 0; }
__global__ void advance_state_kernel(StepState* st, int rows) { st->pos = st->pos + rows; }   // end of a captured pipeline-stage step

// ---- weight re-tiling (load time, once) ------------------------------------------------------------
__global__ void tile_scatter_kernel(const uint16_t* src, uint16_t* dst, int rows, int K, int row_off, int chain, int RW, int NCH) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;          // one thread per 8-element chunk
    size_t total = (size_t)rows * (K >> 3);
    if (idx >= total) return;
    int r = (int)(idx / (K >> 3)), kc = (int)(idx % (K >> 3));
    uint4 v = *(const uint4*)(src + (size_t)r * K + (size_t)kc * 8);
    if (RW == 4) {                                           // row-broadcast layout: the 8 k's are not adjacent
        const uint16_t* e = (const uint16_t*)&v;
        for (int i = 0; i < 8; i++) dst[tiled_index(row_off + r, kc * 8 + i, chain, K, RW, NCH)] = e[i];
        return;
    }
    *(uint4*)(dst + tiled_index(row_off + r, kc * 8, chain, K, RW, NCH)) = v;
}
__global__ void tile_gather_kernel(const uint16_t* src, uint16_t* dst, int rows, int K, int row_off, int chain, int RW, int NCH) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)rows * (K >> 3);
    if (idx >= total) return;
    int r = (int)(idx / (K >> 3)), kc = (int)(idx % (K >> 3));
    if (RW == 4) {
        for (int i = 0; i < 8; i++) dst[(size_t)r * K + (size_t)kc * 8 + i] = src[tiled_index(row_off + r, kc * 8 + i, chain, K, RW, NCH)];
        return;
    }
    uint4 v = *(const uint4*)(src + tiled_index(row_off + r, kc * 8, chain, K, RW, NCH));
    *(uint4*)(dst + (size_t)r * K + (size_t)kc * 8) = v;
}
// synthetic weights straight into their final layout (RW == 0: linear row-major)
__global__ void synth_fill_kernel(uint16_t* dst, int rows, int K, int row_off, int chain, int RW, int NCH,
                                  uint64_t base, int kind, float sigma) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)rows * K;
    if (idx >= total) return;
    int r = (int)(idx / K), k = (int)(idx % K);
    float g = (float)lnb_synth_isum(base, idx) * (1.0f / 53510.0f);
    float v = kind == 1 ? fmaf(0.1f, g, 1.0f) : sigma * g;
    size_t o = RW ? tiled_index(row_off + r, k, chain, K, RW, NCH) : idx;
    dst[o] = bf_trunc(v);
}

// ---- the 13-bit planar copy of a gate|up matrix (lnb_wpack.h), built once on the device from the resident chain layout ----------------
// stats[4] = {min_e2, max_e2, subnormal, infnan} (WpackStats), preset to {0xFF, 0, 0, 0} by the caller
__global__ void wpack_stats_kernel(const uint16_t* w, size_t n_units, unsigned* stats) {
    __shared__ unsigned sh[4];
    if (threadIdx.x == 0) { sh[0] = 0xFFu; sh[1] = sh[2] = sh[3] = 0; }
    __syncthreads();
    WpackStats s; wpack_stats_init(&s);
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (size_t)gridDim.x * blockDim.x) {
        const uint4 v = *(const uint4*)(w + u * 8);
        const uint16_t* e = (const uint16_t*)&v;
#pragma unroll
        for (int i = 0; i < 8; i++) wpack_stats_add(&s, e[i]);
    }
    atomicMin(&sh[0], s.min_e2); atomicMax(&sh[1], s.max_e2); if (s.subnormal) atomicOr(&sh[2], 1u); if (s.infnan) atomicOr(&sh[3], 1u);
    __syncthreads();
    if (threadIdx.x == 0) { atomicMin(&stats[0], sh[0]); atomicMax(&stats[1], sh[1]); if (sh[2]) atomicOr(&stats[2], 1u); if (sh[3]) atomicOr(&stats[3], 1u); }
}
// one thread per (block, stage, helper lane): the lane's four units out of the chain layout [N/RW][K/8][2][RW][8], its group into the stage's planes
__global__ void wpack_pack_kernel(const uint16_t* w, char* out, int K, int rw, int lanes, int n_blocks, unsigned base) {
    const int nst = wpack_stages(K, lanes, rw), kcs = 2 * lanes / rw;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n_blocks * nst * lanes) return;
    const int L = (int)(idx % lanes), st = (int)((idx / lanes) % nst), b = (int)(idx / ((size_t)lanes * nst));
    uint4 g[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int pq = (u >> 1) * lanes + L, kcg = st * kcs + pq / rw, r = pq % rw;
        g[u] = kcg < (K >> 3) ? *(const uint4*)(w + ((((size_t)b * (K >> 3) + kcg) * 2 + (u & 1)) * rw + r) * 8) : make_uint4(0, 0, 0, 0);
    }
    uint32_t low8[8], code4[4], sg;
    wpack_pack_group((const uint16_t*)g, base, low8, code4, &sg);
    char* o = out + ((size_t)b * nst + st) * wpack_stage_bytes(lanes);
    *(uint4*)(o + (size_t)L * 16) = make_uint4(low8[0], low8[1], low8[2], low8[3]);
    *(uint4*)(o + (size_t)lanes * 16 + (size_t)L * 16) = make_uint4(low8[4], low8[5], low8[6], low8[7]);
    *(uint4*)(o + (size_t)lanes * 32 + (size_t)L * 16) = make_uint4(code4[0], code4[1], code4[2], code4[3]);
    *(uint32_t*)(o + (size_t)lanes * 48 + (size_t)L * 4) = sg;
}
// the LM head's copy: one thread per (128-row block, stage, helper lane); the lane's four units out of the resident [N/64][K/8][1][64][8] layout
// (wpack_head_src_unit: chain 0 from resident block 2 b, chain 1 from 2 b + 1, zeros past N and past K)
__global__ void wpack_pack_head_kernel(const uint16_t* w, char* out, int N, int K, unsigned base) {
    const int nst = wpack_head_stages(K), lanes = WPACK_HEAD_LANES;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)wpack_head_blocks(N) * nst * lanes) return;
    const int L = (int)(idx % lanes), st = (int)((idx / lanes) % nst), b = (int)(idx / ((size_t)lanes * nst));
    uint4 g[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const long long su = wpack_head_src_unit(N, K, b, st, L, u);
        g[u] = su >= 0 ? *(const uint4*)(w + (size_t)su * 8) : make_uint4(0, 0, 0, 0);
    }
    uint32_t low8[8], code4[4], sg;
    wpack_pack_group((const uint16_t*)g, base, low8, code4, &sg);
    char* o = out + wpack_head_stage_off(K, b, st);
    *(uint4*)(o + wpack_plane_off(lanes, 0, L)) = make_uint4(low8[0], low8[1], low8[2], low8[3]);
    *(uint4*)(o + wpack_plane_off(lanes, 1, L)) = make_uint4(low8[4], low8[5], low8[6], low8[7]);
    *(uint4*)(o + wpack_plane_off(lanes, 2, L)) = make_uint4(code4[0], code4[1], code4[2], code4[3]);
    *(uint32_t*)(o + wpack_plane_off(lanes, 3, L)) = sg;
}

#include "lnb_batch_kernels.h"
#include "lnb_knobs.h"
#include "lnb_forms.h"

// ------------------------------------------------------------------------------------------------
// host-side launchers (called from lnb_api.cpp)
// ------------------------------------------------------------------------------------------------
// Dynamic-LDS limits: a launcher called with NULL params ("prepare") raises the limit of every kernel it can pick and launches nothing: what is launched
// and what is raised is one list.  Never inside a stream capture: prepare is reached from lnbk_init / lnbk_batch_prepare only.  Stops at the first error.
template <class... K> static hipError_t raise_lds_to(int bytes, K... kernels) {
    hipError_t e = hipSuccess;
    ((e = e != hipSuccess ? e : hipFuncSetAttribute((const void*)kernels, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)), ...);
    return e;
}
template <class... K> static hipError_t raise_lds(K... kernels) { return raise_lds_to(160 * 1024, kernels...); }
// f(std::integral_constant<int, HD>) for p's head dimension (MIN_HD 64: the matrix-core forms have none for 32), hipErrorInvalidValue for one without
// instantiations; NULL p (prepare): every head dimension in turn, up to the first error
template <int MIN_HD = 32, class F> static hipError_t with_hd(const AttnParams* p, F&& f) {
    hipError_t e = hipErrorInvalidValue;
    if (!p || p->hd == 128) e = f(std::integral_constant<int, 128>{});
    if (p ? p->hd == 64 : e == hipSuccess) e = f(std::integral_constant<int, 64>{});
    if constexpr (MIN_HD <= 32) if (p ? p->hd == 32 : e == hipSuccess) e = f(std::integral_constant<int, 32>{});
    return e;
}

// The launch functions of the one-token chain and quad kernels take a row of lnb_gemv_geom.h: the template arguments, the LDS, the checks and the tally row
// are all the row's.
#define X(name) static_assert((int)GEMV_REPORT_##name == LNB_NORM_##name, "lnb_gemv_geom.h and include/lnb.h number the report forms differently");
LNB_GEMV_REPORTS(X)
#undef X
static_assert(gemv_geom(Geom::HEAD_PACKED).rw == WPACK_HEAD_RW && gemv_geom(Geom::HEAD_PACKED).nh * 64 == WPACK_HEAD_LANES, "lnb_wpack.h cuts the LM head for another geometry");
// kfn: production's instantiation; ktm: the one with the measurement code compiled in, launched exactly when p->dbg is set (the report kernels have none)
static hipError_t launch_row(const GemvGeom& g, void (*kfn)(GemvParams), void (*ktm)(GemvParams), const GemvParams* p, int epi, bool norm, int xc, hipStream_t st) {
    if (!p) return raise_lds(kfn, ktm);
    if (!gemv_geom_fits(g, p->K, norm, xc)) return hipErrorInvalidValue;
    form_ran(g.form, epi == EPI_STORE2 ? EPI_STORE : epi);
    hipLaunchKernelGGL(p->dbg ? ktm : kfn, dim3((unsigned)(p->S * p->n_wg)), dim3(g.waves() * 64), g.ring_bytes() + xs_bytes(p->K, g.steps()), st, *p);
    return hipGetLastError();
}
template <Geom ID, int EPI, bool NORM, int XC, bool REPORT = false>
static hipError_t launch_chain_x(const GemvParams* p, hipStream_t st) {
    constexpr GemvGeom G = gemv_geom(ID);
    constexpr int RW = G.rw, NCH = G.nch, SA = G.stage, NH = G.nh, R = G.r;
    static_assert(!NORM || rms_norm_helpers_has(NH), "a norm on this many helper waves: add it to LNB_RMS_NORM_HELPERS (lnb_seqsum.h)");
    void (*kfn)(GemvParams), (*ktm)(GemvParams);
    if constexpr (REPORT) { if constexpr (G.packed) kfn = gemv_chain_pk_report_kernel<RW, NCH, SA, NH, R, EPI, NORM, XC>; else kfn = gemv_chain_report_kernel<RW, NCH, SA, NH, R, EPI, NORM, XC>; ktm = kfn; }
    else if constexpr (G.packed) { kfn = gemv_chain_pk_kernel<RW, NCH, SA, NH, R, EPI, NORM, XC>; ktm = gemv_chain_pk_kernel<RW, NCH, SA, NH, R, EPI, NORM, XC, true>; }
    else { kfn = gemv_chain_kernel<RW, NCH, SA, NH, R, EPI, NORM, XC>; ktm = gemv_chain_kernel<RW, NCH, SA, NH, R, EPI, NORM, XC, true>; }
    return launch_row(gemv_geom(ID), kfn, ktm, p, EPI, NORM, XC, st);
}
// the smallest x staging chunk count that holds the padded row (gemv_geom_chunks); prepare: every one the kernels are instantiated for
template <Geom ID, int EPI, bool NORM, bool REPORT = false>
static hipError_t launch_chain_t(const GemvParams* p, hipStream_t st) {
    if constexpr (NORM) {
        const int xc = p ? gemv_geom_chunks(gemv_geom(ID), p->K, NORM) : 0;
        hipError_t e = hipSuccess;
        if (!p || xc == 2) e = launch_chain_x<ID, EPI, NORM, 2, REPORT>(p, st);
        if (p ? xc == 3 : e == hipSuccess) e = launch_chain_x<ID, EPI, NORM, 3, REPORT>(p, st);
        if (p ? xc == 2 || xc == 3 : e != hipSuccess) return e;
    }
    return launch_chain_x<ID, EPI, NORM, XCh<NORM>::value, REPORT>(p, st);
}

template <Geom ID, int EPI, bool NORM, int XC, bool REPORT = false>
static hipError_t launch_quad_x(const GemvParams* p, hipStream_t st) {
    constexpr GemvGeom G = gemv_geom(ID);
    constexpr int RW = G.rw, KS = G.stage, NH = G.nh, R = G.r;
    static_assert(!NORM || rms_norm_helpers_has(NH), "a norm on this many helper waves: add it to LNB_RMS_NORM_HELPERS (lnb_seqsum.h)");
    void (*kfn)(GemvParams), (*ktm)(GemvParams);
    if constexpr (REPORT) { kfn = gemv_quad_report_kernel<RW, KS, NH, R, EPI, NORM, XC>; ktm = kfn; }
    else { kfn = gemv_quad_kernel<RW, KS, NH, R, EPI, NORM, XC>; ktm = gemv_quad_kernel<RW, KS, NH, R, EPI, NORM, XC, true>; }
    return launch_row(gemv_geom(ID), kfn, ktm, p, EPI, NORM, XC, st);
}
template <Geom ID, int EPI, bool NORM, bool REPORT = false>
static hipError_t launch_quad_t(const GemvParams* p, hipStream_t st) {
    if constexpr (NORM) {
        const bool two = p && gemv_geom_chunks(gemv_geom(ID), p->K, NORM) == 2;
        if (!p || two) { const hipError_t e = launch_quad_x<ID, EPI, NORM, 2, REPORT>(p, st); if (two || e != hipSuccess) return e; }
    }
    return launch_quad_x<ID, EPI, NORM, XCh<NORM>::value, REPORT>(p, st);
}

template <int EPI, bool NORM, int NCH>
static hipError_t launch_gemv_rw(const GemvParams* p, int rw, hipStream_t st) {
    // a choice between two forms that depends on the call: a launch takes one of them, prepare raises both
    auto either = [&](bool first, auto a, auto b) { const hipError_t e = (p && !first) ? hipSuccess : a(p, st); return (p ? first : e != hipSuccess) ? e : b(p, st); };
    // RW 24 (one chain; the 8B wq|wk|wv: 6144 rows = 256 blocks of 24, one per CU): quad-DPP chain waves fed through the LDS, 256-step
    // stages, six helpers x 2 loads x 5 stages = 60 KiB in flight per CU
    // Throughput schedule (GemvParams.sched, lnb_ctx_set_schedule): the same kernel with 128-step stages -- 3 x 12 KiB of products + x = 55 KB of LDS
    // instead of 91 KB, so that a workgroup fits a CU beside the gate|up workgroup (75 KB) of another context's step; twice the stage barriers
    // (slower alone, which is why one stream keeps the 256-step form), ten stages of one load per helper in flight = the same 60 KiB per CU.
    if constexpr (NCH == 1) if (rw == 24) return either(p && p->sched, launch_quad_t<Geom::QUAD24_SCHED, EPI, NORM>, launch_quad_t<Geom::QUAD24, EPI, NORM>);
    // stage geometry (one workgroup per CU).  SA = bf16 bytes per stage, R = stages in flight per helper.
    //  RW 16/32 plain (thin; chain bound): 8 KiB stages, 2 helpers x 4 loads x 7 stages = 56 KiB in flight per CU.
    //  RW 32 with the fused RMSNorm (wq|wk|wv): six helpers so that the exact parallel norm sum has 384 folding lanes, and
    //  12 KiB = 192-step stages (a stage boundary costs one barrier + one exposed LDS round trip: 96-step stages ran the
    //  chain at 10.2 cycles per step, 192-step ones at 8.7); 6 x 2 loads x 5 stages = 60 KiB in flight per CU.
    //  RW 64 (fat; HBM bound): 12 KiB stages, six helpers paired on three SIMDs (the chain wave owns the fourth),
    //  6 x 2 loads x 8 stages = 96 KiB in flight per CU (5 stages: 5.8 TB/s on the LM head, 8: 6.2, 14: worse again).
    // very long rows (70B-like w2: K = 28672): x needs more staging registers than three stager waves hold -> four helpers (prepare: these, then on)
    if (!NORM && NCH == 1 && (rw == 16 || rw == 32) && (!p || !gemv_geom_fits(gemv_geom(rw == 16 ? Geom::CHAIN16 : Geom::CHAIN32), p->K, false, XCh<false>::value))) {
        const hipError_t e = rw == 16 ? launch_chain_t<Geom::CHAIN16_LONG, EPI, false>(p, st) : launch_chain_t<Geom::CHAIN32_LONG, EPI, false>(p, st);
        if (p || e != hipSuccess) return e;
    }
    // rung (a') of the FFN ladder (profiles/r06_ffn_stream.md; LNB_RW_W2=16 LNB_W2_QUAD=1, measurement only): the down projection's 16 rows per CU on ONE
    // quad_perm chain wave + four helpers -- the only w2 form that would leave a co-resident gate|up producer three SIMDs
    if constexpr (NCH == 1 && !NORM && (EPI == EPI_RESID || EPI == EPI_STORE)) {
        const int quad16 = p ? knob(Knob::W2_QUAD) : 0;
        if (rw == 16 && (!p || (quad16 && p->K % 128 == 0))) {
            const hipError_t e = either(quad16 == 2, launch_quad_t<Geom::QUAD16_256, EPI, false>, launch_quad_t<Geom::QUAD16_128, EPI, false>);
            if (p || e != hipSuccess) return e;
        }
    }
    if (rw == 16) return launch_chain_t<NCH == 2 ? Geom::CHAIN16_X2 : Geom::CHAIN16, EPI, NORM>(p, st);
    if (rw == 32) return (NORM && NCH == 1) ? launch_chain_t<Geom::CHAIN32_NORM, EPI, NORM>(p, st) : launch_chain_t<NCH == 2 ? Geom::CHAIN32_X2 : Geom::CHAIN32, EPI, NORM>(p, st);
    if (rw == 64) return launch_chain_t<NCH == 2 ? Geom::CHAIN64_X2 : Geom::CHAIN64, EPI, NORM>(p, st);
    // RW 56 (two chains only): 28672 gate/up rows = 256 blocks of 56 x 2 -- one block per CU on ALL 256 CUs instead of 224 of them;
    // seven helpers (448 lanes = one (k-chunk, row) pair each), 64-step stages
    // (throughput schedule: six ring stages instead of eight -- 133 instead of 149 VGPRs, so that two of its waves and two of the 128-step
    // wq|wk|wv kernel's fit one SIMD's 512 registers: a gate|up workgroup of one context beside a wq|wk|wv workgroup of another)
    if constexpr (NCH == 2) if (rw == 56) return either(p && p->sched && knob(Knob::TP_W13), launch_chain_t<Geom::CHAIN56_TP, EPI, NORM>, launch_chain_t<Geom::CHAIN56, EPI, NORM>);
    // RW 28 (two chains, LNB_RW_W13=28): the same stream cut into 512 half-height blocks, two per workgroup -- rows [0, F/2) are complete
    // after the first block of every workgroup: the row-band order a w1|w3 -> w2 pipeline needs (measurement, NOTES.md 6.1)
    if constexpr (NCH == 2) if (rw == 28) return launch_chain_t<Geom::CHAIN28, EPI, NORM>(p, st);
    return hipErrorInvalidValue;
}

// The one-token gate|up product of 56-row blocks from the 13-bit planar copy (GemvParams.wp, lnb_wpack.h): 128-step stages -- one 32-weight group per helper
// lane -- so 2 x 56 KB of products + x = 132 KB of LDS; LNB_W13P_R stages of 52 bytes per lane in flight (5: the raw form's 114 KB per CU)
#define WPACK_LANES_W13 (gemv_geom(Geom::W13_PACKED).nh * 64)
// a packed row's launch (always norm-fused): gate|up, or the LM head's blocks of two chains stored side by side
template <Geom ID, bool REPORT = false> static hipError_t launch_packed(const GemvParams* p, hipStream_t st) {
    constexpr bool HEAD = gemv_geom(ID).form == Form::GEMV_HEAD_PK;
    if (p && (!p->wp || !gemv_packed_takes(gemv_geom(ID), p->K) || (HEAD && (p->S != 1 || p->n_blocks != wpack_head_blocks(p->n_rows))))) return hipErrorInvalidValue;
    return launch_chain_t<ID, HEAD ? EPI_STORE2 : EPI_SILU_MUL, true, REPORT>(p, st);
}
extern "C" int lnbk_w13p_supported(int rw, int K) { return rw == gemv_geom(Geom::W13_PACKED).rw && gemv_packed_takes(gemv_geom(Geom::W13_PACKED), K); }
extern "C" hipError_t lnbk_gemv_w13p(const GemvParams* p, hipStream_t st) { return launch_packed<Geom::W13_PACKED>(p, st); }
extern "C" size_t lnbk_wpack_w13_bytes(int n_blocks, int K) { return wpack_bytes(n_blocks, K, WPACK_LANES_W13, 56); }
// d_stats: four words on the device; on return (after the stream has run) the matrix's WpackStats
extern "C" hipError_t lnbk_wpack_stats(const uint16_t* w, size_t elems, unsigned* d_stats, hipStream_t st) {
    static const unsigned init[4] = {0xFFu, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(d_stats, init, sizeof init, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wpack_stats_kernel, dim3(1024), dim3(256), 0, st, w, elems / 8, d_stats);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_wpack_w13(const uint16_t* w, void* out, int K, int n_blocks, unsigned base, hipStream_t st) {
    const size_t n = (size_t)n_blocks * wpack_stages(K, WPACK_LANES_W13, 56) * WPACK_LANES_W13;
    hipLaunchKernelGGL(wpack_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, (char*)out, K, 56, WPACK_LANES_W13, n_blocks, base);
    return hipGetLastError();
}

// The one-token LM head from ITS 13-bit copy (blocks of 128 rows as two chains per lane; lnb_wpack.h): the one-chain 64-row form walks 8.7 - 9.0 cycles per step,
// which at 13/16 of the bytes would be the bound (7.83 blocks x 4096 steps = 123 us); two chains through one v_pk_add_f32 walk half the blocks at 6.0.
// Eight helpers (512 lanes, one 32-weight group each), 128-step stages: 2 x 64 KB of products + x = 149 KB of LDS; nine waves = three on one SIMD, so the
// instance has 168 VGPRs at most; LNB_HEADP_R stages of 52 bytes per lane in flight (5: 133 KB per CU).
extern "C" int lnbk_headp_supported(int K) { return gemv_packed_takes(gemv_geom(Geom::HEAD_PACKED), K); }
// p->w: unused; p->n_blocks / p->n_wg count 128-row blocks
extern "C" hipError_t lnbk_gemv_headp(const GemvParams* p, hipStream_t st) { return launch_packed<Geom::HEAD_PACKED>(p, st); }
extern "C" size_t lnbk_wpack_head_bytes(int N, int K) { return wpack_head_bytes(N, K); }
// lnb_op_rmsnorm_sum: the norm-fused kernel of `form` (LNB_NORM_CHAIN16 .. LNB_NORM_HEAD_PACKED of include/lnb.h) in its REPORT instantiation -- the table row that
// serves the form, through the launch function, checks and tally row of the production launch, with the norm's report (p->norm_out) compiled in and the
// epilogue its matrix has in production.  Never inside a stream capture (it raises the instantiation's dynamic-LDS limit first).
template <Geom ID> static hipError_t report_launch(const GemvParams* p, hipStream_t st) {
    static_assert(ID != Geom::COUNT, "a fused kernel's report form without a row in lnb_gemv_geom.h");
    constexpr GemvGeom G = gemv_geom(ID);
    hipError_t (*f)(const GemvParams*, hipStream_t);
    if constexpr (G.packed) f = launch_packed<ID, true>;
    else if constexpr (G.quad) f = launch_quad_t<ID, EPI_STORE, true, true>;
    else f = launch_chain_t<ID, G.nch == 2 ? EPI_SILU_MUL : EPI_STORE, true, true>;
    const hipError_t e = f(nullptr, st);
    return e != hipSuccess ? e : f(p, st);
}
extern "C" hipError_t lnbk_gemv_norm_report(const GemvParams* p, int form, hipStream_t st) {
    if (!p || !p->norm_w || !p->norm_out) return hipErrorInvalidValue;
    switch (form) {
#define X(name) case LNB_NORM_##name: return report_launch<gemv_report_geom(LNB_NORM_##name)>(p, st);
        LNB_GEMV_REPORTS(X)
#undef X
        default: return hipErrorInvalidValue;
    }
}
// w: the resident 64-row one-chain layout of the [N][K] matrix
extern "C" hipError_t lnbk_wpack_head(const uint16_t* w, void* out, int N, int K, unsigned base, hipStream_t st) {
    const size_t n = (size_t)wpack_head_blocks(N) * wpack_head_stages(K) * WPACK_HEAD_LANES;
    hipLaunchKernelGGL(wpack_pack_head_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, (char*)out, N, K, base);
    return hipGetLastError();
}

template <int EPI> static hipError_t launch_rowcast(const GemvParams* p, hipStream_t st) {
    // (the <EPI, true> instantiations carry the measurement code: launched exactly when p->dbg is set)
    const auto kfn = (p && p->dbg) ? rowcast_kernel<EPI, true> : rowcast_kernel<EPI>;
    const auto kl = (p && p->dbg) ? rowcast_lds_kernel<EPI, true> : rowcast_lds_kernel<EPI>;
    if (!p) return raise_lds(kl, kfn, rowcast_lds_kernel<EPI, true>, rowcast_kernel<EPI, true>);
    if (!gemv_layout_takes(4, p->K)) return hipErrorInvalidValue;                // x staging: 8 x 16 B per thread, K*4 bytes of LDS
    // helper-fed chain waves (rowcast_lds_kernel) whenever K is a whole number of its 512-step stages; LNB_ROWCAST_LDS=0: the self-feeding kernel
    // (throughput schedule: the self-feeding kernel -- four waves and K * 4 bytes of LDS instead of eight waves and 96 KB + K * 2: co-resident with
    // another context's gate|up workgroup, NOTES R5)
    if (knob(Knob::ROWCAST_LDS) && !p->sched && p->K % (128 * RL_SC) == 0 && p->K >= 2 * 128 * RL_SC && rl_lds_bytes(p->K) + (size_t)(p->lds_pad > 0 ? p->lds_pad : 0) <= 160 * 1024) {
        form_ran(Form::ROWCAST_LDS, EPI);
        hipLaunchKernelGGL(kl, dim3((unsigned)(p->S * p->n_wg)), dim3(512), rl_lds_bytes(p->K) + (size_t)(p->lds_pad > 0 ? p->lds_pad : 0), st, *p);
        return hipGetLastError();
    }
    form_ran(Form::ROWCAST, EPI);
    hipLaunchKernelGGL(kfn, dim3((unsigned)(p->S * p->n_wg)), dim3(256), (size_t)p->K * 4 + (size_t)(p->lds_pad > 0 ? p->lds_pad : 0), st, *p);
    return hipGetLastError();
}

// the (chains, epilogue, norm) combinations lnbk_gemv has kernels for; the row-broadcast layout (thin matrices): one chain, no norm
constexpr bool gemv_dispatches(int rw, int nch, int epi, bool norm) {
    if (rw == 4 && (nch != 1 || norm)) return false;
    return nch == 2 ? epi == EPI_SILU_MUL && norm : epi == EPI_STORE || (epi == EPI_QKV_ROPE && norm) || (epi == EPI_RESID && !norm);
}
extern "C" hipError_t lnbk_gemv(const GemvParams* p, int rw, int nch, int epi, int norm, hipStream_t st) {
    if (!gemv_dispatches(rw, nch, epi, norm != 0)) return hipErrorInvalidValue;
    if (rw == 4) return epi == EPI_STORE ? launch_rowcast<EPI_STORE>(p, st) : launch_rowcast<EPI_RESID>(p, st);
    if (nch == 2) return launch_gemv_rw<EPI_SILU_MUL, true, 2>(p, rw, st);
    if (epi == EPI_QKV_ROPE) return launch_gemv_rw<EPI_QKV_ROPE, true, 1>(p, rw, st);
    if (epi == EPI_RESID) return launch_gemv_rw<EPI_RESID, false, 1>(p, rw, st);
    return norm ? launch_gemv_rw<EPI_STORE, true, 1>(p, rw, st) : launch_gemv_rw<EPI_STORE, false, 1>(p, rw, st);
}

template <int EPI, int NCH> static hipError_t launch_gemm(const GemmParams* p, hipStream_t st) {
    // the three tile forms, each with the LDS it asks for: 53 / 73 KB (37 / 57, 39 / 44): >= two workgroups per CU
    const struct { void (*k)(GemmParams); size_t lds; } t128{gemm_mfma_kernel<EPI, NCH, 4, 128>, gemm_lds_bytes(NCH, 4)},
        t64{gemm_mfma_kernel<EPI, NCH, 4, 64>, gemm_lds_bytes(NCH, 4, 64)}, t1{gemm_mfma_kernel<EPI, NCH, 1, 128>, gemm_lds_bytes(NCH, 1)};
    hipError_t e = hipSuccess;
    if (!p) { for (const auto& t : {t128, t64, t1}) if (e == hipSuccess) e = raise_lds_to((int)t.lds, t.k); return e; }
    const unsigned mb = (unsigned)((p->S + 127) / 128), nb4 = (unsigned)((p->n_rows + GM_NB - 1) / GM_NB);
    const int force = knob(Knob::GEMM_TILE);                 // 1 / 64 / 128: measurement aid
    // the two-chain w1|w3 kernel already runs 2x the MFMAs per staged byte: with more than four 64 x 128 tiles per CU it keeps them
    // (S = 2048: 3.90 ms against 4.11 ms with 64 x 64 tiles; the one-chain kernels gain 5 % from the smaller tile there;
    // S = 512, 896 tiles: the small tile still wins, 74 against 77 ms per Forward)
    const int tile = force ? force : (nb4 * mb <= 160 ? 1 : (NCH == 2 && nb4 * mb > 1024) ? 128 : nb4 * mb <= GM_MB64_UPTO ? 64 : 128);
    form_ran(tile == 1 ? Form::GEMM_MFMA_T16 : tile == 64 ? Form::GEMM_MFMA_T64 : Form::GEMM_MFMA_T128, EPI);
    if (tile == 1)             // 64 x 128 tiles would leave most CUs idle: 16-row tiles, the four waves split the batch rows
                               // (tools/gemmbench.hip: 64 / 96 / 128 tiles: 1.4-2x faster; 256 tiles and up: 64-row tiles win)
        hipLaunchKernelGGL(t1.k, dim3((unsigned)((p->n_rows + 15) / 16), mb), dim3(256), t1.lds, st, *p);
    else if (tile == 64)       // about one 64 x 128 tile per CU: 64 x 64 tiles, two to three workgroups per CU overlap staging and MFMAs
        hipLaunchKernelGGL(t64.k, dim3(nb4, (unsigned)((p->S + 63) / 64)), dim3(256), t64.lds, st, *p);
    else
        hipLaunchKernelGGL(t128.k, dim3(nb4, mb), dim3(256), t128.lds, st, *p);
    return hipGetLastError();
}

extern "C" hipError_t lnbk_gemm(const GemmParams* p, int epi, hipStream_t st) {
    switch (epi) {
        case EPI_STORE: return launch_gemm<EPI_STORE, 1>(p, st);
        case EPI_RESID: return launch_gemm<EPI_RESID, 1>(p, st);
        case EPI_QKV_ROPE: return launch_gemm<EPI_QKV_ROPE, 1>(p, st);
        case EPI_SILU_MUL: return (p && p->nch != 2) ? hipErrorInvalidValue : launch_gemm<EPI_SILU_MUL, 2>(p, st);
        default: return hipErrorInvalidValue;
    }
}
// form 0: by knob and shape (production); 1 / 2: the wide / the one-wave kernel or an error, whatever the knob says (lnb_op_rmsnorm_sum).  norm_out: the kernels' report argument, [S][3] words or null
extern "C" hipError_t lnbk_rmsnorm_rows_form(const uint16_t* x, const uint16_t* w, uint16_t* out, int S, int K, float eps, int form, uint32_t* norm_out, hipStream_t st) {
    const size_t lds_w = bn_scratch() + ((size_t)bn_kpad(K) + 8) * 4;                  // one workgroup of seven waves per row: the exact parallel evaluation of the serial sum
    if ((form ? form == 1 : knob(Knob::NORM_ROWS_WIDE) != 0) && !(K & 127) && lds_w <= 64 * 1024 && (size_t)bn_kpad(K) <= (size_t)XCh<true>::value * (1 + BN_NH) * 512 && seq_leaf_size(K, rms_nf(BN_NH) * 64) <= 256) {
        form_ran(Form::RMSNORM_ROWS_WIDE);
        if (norm_out) hipLaunchKernelGGL((batch_rmsnorm_xt_kernel<false, true>), dim3((unsigned)S), dim3((1 + BN_NH) * 64), lds_w, st, x, w, eps, out, K, norm_out);
        else hipLaunchKernelGGL((batch_rmsnorm_xt_kernel<false, false>), dim3((unsigned)S), dim3((1 + BN_NH) * 64), lds_w, st, x, w, eps, out, K, norm_out);
        return hipGetLastError();
    }
    if (form == 1 || ((size_t)K + 64) * 4 > 150 * 1024) return hipErrorInvalidValue;
    form_ran(Form::RMSNORM_ROWS_WAVE);
    if (norm_out) hipLaunchKernelGGL(rmsnorm_rows_kernel<true>, dim3((unsigned)S), dim3(64), ((size_t)K + 64) * 4, st, x, w, out, S, K, eps, norm_out);
    else hipLaunchKernelGGL(rmsnorm_rows_kernel<false>, dim3((unsigned)S), dim3(64), ((size_t)K + 64) * 4, st, x, w, out, S, K, eps, norm_out);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_rmsnorm_rows(const uint16_t* x, const uint16_t* w, uint16_t* out, int S, int K, float eps, hipStream_t st) {
    return lnbk_rmsnorm_rows_form(x, w, out, S, K, eps, 0, nullptr, st);
}

static size_t attn_lds_bytes(int seq_len, int hd) { return attn_off_ring(seq_len, hd) + 2 * (size_t)ATT_RP * hd * 4; }
extern "C" size_t lnbk_attn_short_lds(int seq_len, int hd) { return attn_lds_bytes(seq_len, hd); }
// the longest context the one-workgroup-per-head kernel can stage in 160 KB of LDS (e f64 + p f32 per position + q + the product ring)
extern "C" int lnbk_attn_short_max_T(int hd) {
    int lo = 64, hi = 1 << 20;
    while (lo < hi) { const int mid = (lo + hi + 1) / 2; if (attn_lds_bytes(mid, hd) <= 160 * 1024) lo = mid; else hi = mid - 1; }
    return lo;
}
static long long* g_gqa_dbg = nullptr;                       // LNB_ATTN_GQA_DBG: phase stamps of one attn_gqa_kernel workgroup
// long-context decode attention: scores, then PV -- the lazily certified form (attn_long_pv2_kernel, round 6) unless LNB_ATTN_LAZY=0.
// BATCH (p->btab): p->S sequences in grid.z, p->seq_len = the largest member's cache length (e_buf [S][H][seq_len], z_part [S][H][ceil(seq_len/256)])
template <bool BATCH> static hipError_t launch_attn_long(const AttnParams* p, hipStream_t st) {
    return with_hd(p, [&](auto HD) {
        const bool tm = p && p->dbg;                                 // the PV pair's instantiations with the phase stamps
        const auto scores = attn_long_scores_kernel<HD, BATCH>, lazy = tm ? attn_long_pv2_kernel<HD, BATCH, true> : attn_long_pv2_kernel<HD, BATCH>,
                   eager = tm ? attn_long_pv_kernel<HD, BATCH, true> : attn_long_pv_kernel<HD, BATCH>;
        if (!p) return raise_lds(lazy, eager, attn_long_pv2_kernel<HD, BATCH, true>, attn_long_pv_kernel<HD, BATCH, true>);
        // (a context beyond the per-position layout cannot stage p_j for the eager-everywhere form: LNB_ATTN_LAZY=0 runs the default pair there)
        const auto pv = knob(Knob::ATTN_LAZY) || !alp_per_position(p->seq_len) ? lazy : eager;
        const size_t lds = alp_layout_bytes(p->seq_len);
        if (lds > 160 * 1024 || p->seq_len > LNB_SEQ_MAX || p->hd % ALP_DS || !p->e_buf || !p->z_part) return hipErrorInvalidValue;
        if (BATCH && (!p->bkv || p->S < 1 || p->S > LNB_BATCH_MAX || (!p->out && !p->out_xt))) return hipErrorInvalidValue;
        const unsigned z = BATCH ? p->S : 1;
        AttnParams ps = *p;
        ps.touch = knob(Knob::ATTN_TOUCH) != 0;
        ps.pw_floats = alp_pw_floats(p->seq_len);
        hipLaunchKernelGGL(scores, dim3(p->H, (p->seq_len + ALS_NT - 1) / ALS_NT, z), dim3(ALS_NT), 0, st, ps);
        hipLaunchKernelGGL(pv, dim3(p->H, p->hd / ALP_DS, z), dim3(ALP_NT), lds, st, ps);
        return hipGetLastError();
    });
}
// the one-launch form (attn_one_kernel): scores, softmax and PV per (head, 16-dim slice) workgroup with a bounded in-launch exchange
static hipError_t launch_attn_one(const AttnParams* p, hipStream_t st) {
    return with_hd(p, [&](auto HD) {
        const auto one = attn_one_kernel<HD>;
        if (!p) return raise_lds(one);
        const size_t lds = att1_lds_bytes(p->seq_len, p->hd);
        if (lds > 160 * 1024 || p->hd % ALP_DS || !p->e_buf || !p->z_part || !p->cnt) return hipErrorInvalidValue;
        hipLaunchKernelGGL(one, dim3(p->H, p->hd / ALP_DS), dim3(ALP_NT), lds, st, *p);
        return hipGetLastError();
    });
}
extern "C" size_t lnbk_attn_one_lds(int seq_len, int hd) { return att1_lds_bytes(seq_len, hd); }
extern "C" size_t lnbk_attn_long_lds(int seq_len) { return alp_lds_bytes(seq_len); }
// what the PV launch of a context of seq_len positions really requests: lnbk_attn_long_lds up to 160 KB, a constant beyond (alp_pw_floats)
extern "C" size_t lnbk_attn_long_layout_lds(int seq_len) { return alp_layout_bytes(seq_len); }
// long-context attention for p->S consecutive rows of one context (attn_rows_*_kernel), any row count: groups of up to 16 rows, launched one
// after the other on the stream, so the 16-row scratch p->e_buf / p->z_part serves them all.  pos0: the first row's position when the host
// knows it (the scores grid then ends at the group's last position), < 0: read from the device state (a captured graph: p->btab's column 0, else p->st).
// Rows per PV workgroup: LNB_ATTN_ROWS_RPW (1 / 2 / 4).
static int attn_rows_rpw() { const int v = knob(Knob::ATTN_ROWS_RPW); return v == 1 || v == 2 || v == 4 ? v : 0; }      // 0: no such form -- the launch is refused
static hipError_t launch_attn_rows(const AttnParams* p, int pos0, hipStream_t st) {
    return with_hd(p, [&](auto HD) {
        const auto scores = attn_rows_scores_kernel<HD>;
        const auto pv1 = attn_rows_pv_kernel<HD, 1>, pv2 = attn_rows_pv_kernel<HD, 2>, pv4 = attn_rows_pv_kernel<HD, 4>;
        if (!p) return raise_lds(pv1, pv2, pv4);
        const int rpw = attn_rows_rpw();
        const size_t lds = ar_lds_bytes(rpw);
        if (rpw == 0 || lds > 160 * 1024 || p->seq_len < 1 || p->seq_len > LNB_SEQ_MAX || p->hd % ALP_DS || !p->e_buf || !p->z_part) return hipErrorInvalidValue;
        if (p->S < 1 || (!p->out && !p->out_xt) || (pos0 < 0 && !p->btab && !p->st) || pos0 > p->seq_len - p->S) return hipErrorInvalidValue;
        if (p->btab ? (!p->bkv || p->S > LNB_ATTN_ROWS_MAX) : (!p->cache_k || !p->cache_v)) return hipErrorInvalidValue;       // (a verify pass: one column group)
        if (!p->q || p->H < 1 || p->KVH < 1 || p->H % p->KVH) return hipErrorInvalidValue;
        AttnRowsParams rp{};
        rp.a = *p; rp.a.touch = knob(Knob::ATTN_TOUCH) != 0; rp.pos0 = pos0;
        for (int row0 = 0; row0 < p->S; row0 += LNB_ATTN_ROWS_MAX) {
            rp.W = p->S - row0 < LNB_ATTN_ROWS_MAX ? p->S - row0 : LNB_ATTN_ROWS_MAX; rp.row0 = row0; rp.pos_off = row0;
            const int reach = pos0 >= 0 ? pos0 + row0 + rp.W : p->seq_len;     // positions the group can see
            hipLaunchKernelGGL(scores, dim3(p->H, (reach + ALS_NT - 1) / ALS_NT), dim3(ALS_NT), 0, st, rp);
            hipLaunchKernelGGL(rpw == 1 ? pv1 : rpw == 2 ? pv2 : pv4, dim3(p->H, p->hd / ALP_DS, (rp.W + rpw - 1) / rpw), dim3(ALP_NT), lds, st, rp);
        }
        return hipGetLastError();
    });
}
extern "C" hipError_t lnbk_attn_rows(const AttnParams* p, int pos0, hipStream_t st) { return p ? launch_attn_rows(p, pos0, st) : hipErrorInvalidValue; }
extern "C" size_t lnbk_attn_rows_lds(int hd, int rpw) { return (hd == 32 || hd == 64 || hd == 128) && (rpw == 1 || rpw == 2 || rpw == 4) ? ar_lds_bytes(rpw) : 0; }

extern "C" void lnbk_attn_gqa_dbg_dump(void) {
    if (!g_gqa_dbg) return;
    (void)hipDeviceSynchronize();
    long long h[128];
    if (hipMemcpy(h, g_gqa_dbg, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int w = 0; w < 8; w++) {
        fprintf(stderr, "[gqa] wave %d: q+K %lld scores %lld pad+barrier %lld Z+cert %lld V0 store+barrier %lld PV %lld  (start %+lld)\n", w,
                h[w * 16 + 1] - h[w * 16], h[w * 16 + 2] - h[w * 16 + 1], h[w * 16 + 3] - h[w * 16 + 2], h[w * 16 + 4] - h[w * 16 + 3], h[w * 16 + 5] - h[w * 16 + 4], h[w * 16 + 6] - h[w * 16 + 5], h[w * 16] - h[0]);
    }
}
// prefill (head_dim 128 / 64): 16 (attn_mfma_kernel) or 32 (attn_mfma2_kernel, round 6) query rows per wave on the matrix cores; static LDS only.  The order of the conditions decides the form
static hipError_t launch_attn_prefill(const AttnParams* p, hipStream_t st) {
    const int min2 = knob(Knob::ATTN_MFMA2);                 // 0: never the two-tile form (the default: measured slower, see attn_mfma2_kernel); N > 0: from N rows on
    static_assert(ATM2_MIN_S == 0, "LNB_ATTN_MFMA2's default in lnb_knobs.h is the kernel's");
    const bool two = min2 > 0 && p->S >= min2 && !p->causal;                             // (the opt-in two-tile form has no causal instantiation: an append never selects it)
    const bool kept = !two && p->score_idx && p->host_T > 0 && p->sidx_jt * 16 >= p->host_T;   // round 6: scores once, indices kept (the caller sized the scratch for this call's context)
    return with_hd<64>(p, [&](auto HD) {
        // causal (lnb_forward_append): the true causal mask with an offset -- template instantiations of their own, the modulo forms' code is untouched
        void (*const k)(AttnParams) = two ? attn_mfma2_kernel<HD> : kept ? (p->causal ? attn_mfma3_kernel<HD, true> : attn_mfma3_kernel<HD>)
                                                                         : (p->causal ? attn_mfma_kernel<HD, true> : attn_mfma_kernel<HD>);
        hipLaunchKernelGGL(k, dim3(p->H, two ? (p->S + 127) / 128 : (p->S + 63) / 64), dim3(256), 0, st, *p);
        return hipGetLastError();
    });
}
// one workgroup per (head, row) and its batched forms
static hipError_t launch_attn_short(const AttnParams* p, hipStream_t st) {
    const auto gqa = attn_gqa_kernel<128, 4>;
    const auto dense = attn_exact_kernel<128, true>;
    const size_t lds = p ? attn_lds_bytes(p->lds_T, p->hd) : 0;
    if (!p) { const hipError_t e = raise_lds(gqa, dense); if (e != hipSuccess) return e; }
    else {
        // (host_T: e[] / pw[] are sized for lds_T positions: never launch past them -- lnb_api.cpp check_call refuses first)
        if (lds > 160 * 1024 || p->lds_T <= 0 || p->lds_T > p->seq_len || p->host_T > p->lds_T) return hipErrorInvalidValue;
        if (p->btab && p->hd == 128 && p->H == 4 * p->KVH) {        // batched decode: one workgroup per (KV head, sequence) when that fills the chip
            const int mode = knob(Knob::ATTN_GQA);                  // 0: never, 1: always, default: from LNB_ATTN_GQA_MIN_WG workgroups on
            const size_t gl = gqa_lds_bytes(p->lds_T, 128, 4);
            if (mode != 0 && p->exp_tab && gl <= 160 * 1024 && (mode == 1 || (long)p->KVH * p->S >= 256)) {
                AttnParams q = *p;
                if (knob(Knob::ATTN_GQA_FORCE_ZSEQ)) q.force_zseq = 1;      // (tests: every head walks the serial denominator)
                if (knob(Knob::ATTN_GQA_DBG)) q.dbg = g_gqa_dbg;            // phase stamps of one workgroup (allocated by lnbk_init: no allocation inside a stream capture)
                form_ran(Form::ATTN_BATCH_GQA);
                hipLaunchKernelGGL(gqa, dim3(p->KVH, p->S), dim3(512), gl, st, q);
                return hipGetLastError();
            }
        }
        if (p->btab && p->hd == 128 && (long)p->H * p->S > 256 && knob(Knob::ATTN_BATCH_DENSE)) {       // more workgroups than CUs (never an append: that has no btab)
            AttnParams q = *p;
            q.head_major = knob(Knob::ATTN_BATCH_HEADMAJOR) != 0;   // (A/B of the dispatch order)
            form_ran(q.head_major ? Form::ATTN_BATCH_DENSE_HM : Form::ATTN_BATCH_DENSE);
            hipLaunchKernelGGL(dense, dim3(p->H, p->S), dim3(ATT_NT), lds, st, q);
            return hipGetLastError();
        }
    }
    return with_hd(p, [&](auto HD) {
        const bool tm = p && p->dbg;                                 // the instantiations with the phase stamps
        const auto plain = tm ? attn_exact_kernel<HD, false, false, true> : attn_exact_kernel<HD>, append = tm ? attn_exact_kernel<HD, false, true, true> : attn_exact_kernel<HD, false, true>;
        if (!p) return raise_lds(plain, append, attn_exact_kernel<HD, false, false, true>, attn_exact_kernel<HD, false, true, true>);
        // lnb_forward_append, 2..15 rows (any row count at head_dim 32): workgroup (h, i) runs the one-token step at pos + i
        const auto k = p->causal && !p->btab && p->S > 1 ? append : plain;
        if (p->btab) form_ran(Form::ATTN_BATCH_PLAIN);
        hipLaunchKernelGGL(k, dim3(p->H, p->S), dim3(ATT_NT), lds, st, *p);
        return hipGetLastError();
    });
}
extern "C" hipError_t lnbk_attn(const AttnParams* p, hipStream_t st) {
    if (p->btab && p->longctx) return launch_attn_long<true>(p, st);      // batched decode / verify pass in the long-context form (the caller chose it: lnb_api.cpp batch_want_long / batch_select_form)
    if (p->longctx >= 2 && p->S == 1) return launch_attn_one(p, st);
    if (p->longctx && p->S == 1) return launch_attn_long<false>(p, st);
    if (p->mfma && p->S >= 16 && (p->hd == 128 || p->hd == 64)) return launch_attn_prefill(p, st);
    return launch_attn_short(p, st);
}
// rows [pos, pos + rows) of one layer's caches (st: the position is the device state's; nullptr: pos0): raises *word on an inf or a NaN
extern "C" hipError_t lnbk_kv_scan_nonfinite(const uint16_t* ck, const uint16_t* cv, int seq_len, int kv_dim, int hd, const StepState* st, int pos0, int rows, int* word, hipStream_t s) {
    if (!ck || !cv || !word || rows < 1 || kv_dim < 1 || hd < 8 || kv_dim % hd || (!st && (pos0 < 0 || pos0 > seq_len - rows))) return hipErrorInvalidValue;
    const size_t n = (size_t)rows * kv_dim;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(kv_nonfinite_scan_kernel, dim3(blocks), dim3(256), 0, s, ck, cv, seq_len, kv_dim, hd, st, pos0, rows, word);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_nonfinite_or(int* dst, const int* src, hipStream_t s) {
    hipLaunchKernelGGL(nonfinite_or_kernel, dim3(1), dim3(1), 0, s, dst, src);
    return hipGetLastError();
}
// behind the attention launch of a multi-row call of one context: the rows again, the reference's way, if the context's word is set
extern "C" hipError_t lnbk_attn_plain(const AttnParams* p, const int* word, hipStream_t st) {
    if (!p || !word || p->btab || !p->st || !p->q || !p->out || !p->cache_k || !p->cache_v || p->S < 1 || p->H < 1 || p->KVH < 1 || p->H % p->KVH) return hipErrorInvalidValue;
    return with_hd(p, [&](auto HD) {
        hipLaunchKernelGGL(attn_plain_kernel<HD>, dim3(p->H, p->S), dim3(256), 0, st, *p, word);
        return hipGetLastError();
    });
}
extern "C" hipError_t lnbk_init(void) {
    static bool done = false;
    if (done) return hipSuccess;
    hipError_t e = raise_lds(rmsnorm_rows_kernel<false>, rmsnorm_rows_kernel<true>);           // (lnbk_rmsnorm_rows' other form stays within the 64 KiB every kernel gets)
    for (int ep = EPI_STORE; ep <= EPI_SILU_MUL && e == hipSuccess; ep++) e = lnbk_gemm(nullptr, ep, nullptr);
    // the row-broadcast layout and every raw row of lnb_gemv_geom.h, each under every (epilogue, norm) lnbk_gemv dispatches its (rows per block, chains) to;
    // the two packed rows
    auto gemv = [&](int rw, int nch) {
        for (int epi = EPI_STORE; epi <= EPI_SILU_MUL; epi++)
            for (int norm = 0; norm <= 1; norm++) if (e == hipSuccess && gemv_dispatches(rw, nch, epi, norm != 0)) e = lnbk_gemv(nullptr, rw, nch, epi, norm, nullptr);
    };
    gemv(4, 1);
    for (const GemvGeom& g : LNB_GEMV_GEOM_TABLE) if (!g.packed) gemv(g.rw, g.nch);
    if (e == hipSuccess) e = lnbk_gemv_w13p(nullptr, nullptr);
    if (e == hipSuccess) e = lnbk_gemv_headp(nullptr, nullptr);
    for (auto prepare : {launch_attn_long<true>, launch_attn_long<false>, launch_attn_one, launch_attn_short}) if (e == hipSuccess) e = prepare(nullptr, nullptr);
    if (e == hipSuccess) e = launch_attn_rows(nullptr, -1, nullptr);
    if (e != hipSuccess) return e;
    if (knob(Knob::ATTN_GQA_DBG) && !g_gqa_dbg) { if (hipMalloc(&g_gqa_dbg, 8 * 16 * 8) != hipSuccess) return hipErrorOutOfMemory; (void)hipMemset(g_gqa_dbg, 0, 8 * 16 * 8); }
    done = true;
    return hipSuccess;
}

extern "C" hipError_t lnbk_embed(const uint16_t* emb, const int32_t* tokens, uint16_t* x, int S, int dim, int vocab, int* err, hipStream_t st) {
    hipLaunchKernelGGL(embed_kernel, dim3(S), dim3(256), 0, st, emb, tokens, x, dim, vocab, err);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_argmax(const uint16_t* logits, int V, int32_t* next_token, StepState* state, int32_t* out_tokens,
                                  int out_cap, int advance, hipStream_t st) {
    hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, st, logits, V, next_token, state, out_tokens, out_cap, advance);
    return hipGetLastError();
}
// the decode step's sampler launch (advance = 1, one row, smp[0]) or rows of lnb_op_sample (advance = 0: next_token[rows], pos[rows], draws / info optional)
extern "C" hipError_t lnbk_sample(const uint16_t* logits, int V, int rows, const double* etab, const LnbSampler* smp, int32_t* next_token, StepState* state,
                                  int32_t* out_tokens, int out_cap, int advance, const int32_t* pos, const unsigned long long* draws, LnbSampleInfo* info, hipStream_t st) {
    if (V < 1 || V > LNB_SAMPLE_MAX_V || rows < 1 || (advance && rows != 1)) return hipErrorInvalidValue;
    form_ran(Form::SAMPLE_ROW);
    hipLaunchKernelGGL(sample_kernel, dim3(rows), dim3(1024), 0, st, logits, V, etab, smp, next_token, state, out_tokens, out_cap, advance, pos, draws, info);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_batch_sample(const uint16_t* logits, int V, const double* etab, const LnbSampler* smp, const BatchTab* tab, int nseq, hipStream_t st) {
    if (V < 1 || V > LNB_SAMPLE_MAX_V) return hipErrorInvalidValue;
    form_ran(Form::SAMPLE_BATCH);
    hipLaunchKernelGGL(batch_sample_kernel, dim3(nseq), dim3(1024), 0, st, logits, V, etab, smp, tab);
    return hipGetLastError();
}
// the verify pass's token launch of the sampling speculative loop: w columns of one context, smp[0], cnt = the launch's arrival ticket (zero between launches)
extern "C" hipError_t lnbk_spec_sample_commit(const uint16_t* logits, int V, int w, const double* etab, const LnbSampler* smp, int32_t* g, const BatchTab* tab,
                                              unsigned* cnt, hipStream_t st) {
    if (V < 1 || V > LNB_SAMPLE_MAX_V || w < 1 || w > LNB_SPEC_MAX_DRAFT + 1 || !logits || !etab || !smp || !g || !tab || !cnt) return hipErrorInvalidValue;
    form_ran(Form::SAMPLE_SPEC);
    hipLaunchKernelGGL(spec_sample_commit_kernel, dim3((unsigned)w), dim3(1024), 0, st, logits, V, etab, smp, g, tab, cnt);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_set_state(StepState* state, int pos, int n_out, int honour_stop, hipStream_t st) {
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, state, pos, n_out, honour_stop);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_set_stop(StepState* state, const int32_t* ids, int n, hipStream_t st) {
    StopIds s{}; s.n = n; for (int k = 0; k < n && k < LNB_MAX_STOP_IDS; k++) s.id[k] = ids[k];
    hipLaunchKernelGGL(set_stop_kernel, dim3(1), dim3(1), 0, st, state, s);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_advance_state(StepState* state, int rows, hipStream_t st) {
    hipLaunchKernelGGL(advance_state_kernel, dim3(1), dim3(1), 0, st, state, rows);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_tile(const uint16_t* src, uint16_t* dst, int rows, int K, int row_off, int chain, int RW, int NCH, int gather, hipStream_t st) {
    size_t total = (size_t)rows * (K >> 3);
    unsigned blocks = (unsigned)((total + 255) / 256);
    if (gather) hipLaunchKernelGGL(tile_gather_kernel, dim3(blocks), dim3(256), 0, st, src, dst, rows, K, row_off, chain, RW, NCH);
    else hipLaunchKernelGGL(tile_scatter_kernel, dim3(blocks), dim3(256), 0, st, src, dst, rows, K, row_off, chain, RW, NCH);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_synth_fill(uint16_t* dst, int rows, int K, int row_off, int chain, int RW, int NCH,
                                      uint64_t seed, uint32_t tensor_id, int kind, float sigma, hipStream_t st) {
    uint64_t base = lnb_splitmix64(seed + 0x9E3779B97F4A7C15ULL * (uint64_t)(tensor_id + 1u));
    size_t total = (size_t)rows * K;
    unsigned blocks = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(synth_fill_kernel, dim3(blocks), dim3(256), 0, st, dst, rows, K, row_off, chain, RW, NCH, base, kind, sigma);
    return hipGetLastError();
}

// ---- batched decode launchers -----------------------------------------------------------------------
extern "C" hipError_t lnbk_m16_from_tiled(const uint16_t* src, uint16_t* dst, int rows, int K, int RW, int NCH, hipStream_t st) {
    const size_t total = (size_t)rows * NCH * K;
    hipLaunchKernelGGL(m16_from_tiled_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, dst, rows, K, RW, NCH);
    return hipGetLastError();
}
// the epilogues mfma_pair_kernel exists for (nullptr: none)
static auto pair_kernel(int epi) -> void (*)(StreamParams) {
    return epi == EPI_STORE ? mfma_pair_kernel<EPI_STORE> : epi == EPI_RESID ? mfma_pair_kernel<EPI_RESID> : epi == EPI_QKV_ROPE ? mfma_pair_kernel<EPI_QKV_ROPE> : nullptr;
}
// acc2: two tile-chains per wave (fat matrices and the gate|up pairs); else one (thin matrices: every tile on its own SIMD)
extern "C" hipError_t lnbk_stream(const StreamParams* p, int epi, int acc2, int num_cus, hipStream_t st) {
    const int G = p->n_groups > 1 ? p->n_groups : 1;
    if ((p->K & 127) || p->nseq < 1 || p->nseq > G * LNB_STREAM_COLS || p->n_chains < 1 || (G > 1 && acc2)) return hipErrorInvalidValue;
    StreamParams q = *p;
    const int ACC = acc2 ? 2 : 1;
    q.n_jobs = (p->n_chains + ACC - 1) / ACC;
    unsigned grid = (unsigned)((q.n_jobs + 3) / 4); if (grid > (unsigned)num_cus) grid = (unsigned)num_cus;
    // thin matrices: chain wave + helper wave per tile (mfma_pair_kernel); LNB_STREAM_PAIR=0: the one-wave form
    if (const auto pair = pair_kernel(epi); pair && !acc2 && (G > 1 || knob(Knob::STREAM_PAIR))) {
        const size_t lds = (size_t)2 * 2 * MP_BUF;
        unsigned gp = (unsigned)((q.n_jobs * G + 1) / 2); if (gp > (unsigned)num_cus) gp = (unsigned)num_cus;
        form_ran(Form::MFMA_PAIR, epi);
        hipLaunchKernelGGL(pair, dim3(gp), dim3(256), lds, st, q);
        return hipGetLastError();
    }
#define LNB_STREAM(E) (acc2 ? mfma_stream_kernel<2, E> : mfma_stream_kernel<1, E>)
    void (*const k)(StreamParams) = epi == EPI_STORE ? LNB_STREAM(EPI_STORE) : epi == EPI_RESID ? LNB_STREAM(EPI_RESID) : epi == EPI_QKV_ROPE ? LNB_STREAM(EPI_QKV_ROPE)
                                    : (epi == EPI_SILU_MUL && acc2 && p->nch == 2) ? mfma_stream_kernel<2, EPI_SILU_MUL> : nullptr;
#undef LNB_STREAM
    if (!k) return hipErrorInvalidValue;
    form_ran(acc2 ? Form::MFMA_STREAM_C2 : Form::MFMA_STREAM_C1, epi);
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, st, q);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_gemm_stream(const GemmParams* p, int epi, int num_cus, hipStream_t st);
// a one-wave kernel that occupies its stream for `us` microseconds of the constant-rate wall clock (measurement aid: lnb_runtime_info's count of
// streams that really run concurrently; the delayed second launch of tools/ffn_overlap.py)
__global__ void spin_kernel(long long ticks) { const long long t0 = (long long)wall_clock64(); while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8); }
extern "C" hipError_t lnbk_spin(int us, hipStream_t st) {
    int khz = 100000, dev = 0;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, st, (long long)us * khz / 1000);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_batch_prepare(void) {             // raise the dynamic-LDS limits once, outside any stream capture
    static bool done = false;
    if (done) return hipSuccess;
    hipError_t e = raise_lds(batch_rmsnorm_xt_kernel<true, false>, batch_rmsnorm_xt_kernel<true, true>);
    for (int ep = EPI_STORE; ep <= EPI_SILU_MUL && e == hipSuccess; ep++) {
        if (pair_kernel(ep)) e = raise_lds(pair_kernel(ep));
        if (e == hipSuccess) e = lnbk_gemm_stream(nullptr, ep, 0, nullptr);
    }
    done = e == hipSuccess;
    return e;
}
extern "C" hipError_t lnbk_batch_rmsnorm_out(const uint16_t* x, const uint16_t* norm_w, float eps, uint16_t* xt, int K, int nseq, uint32_t* norm_out, hipStream_t st) {
    const size_t lds = bn_scratch() + ((size_t)bn_kpad(K) + 8) * 4;
    if ((K & 127) || lds > 160 * 1024 || (size_t)bn_kpad(K) > (size_t)XCh<true>::value * (1 + BN_NH) * 512 || seq_leaf_size(K, rms_nf(BN_NH) * 64) > 256) return hipErrorInvalidValue;
    form_ran(Form::BATCH_RMSNORM);
    if (norm_out) hipLaunchKernelGGL((batch_rmsnorm_xt_kernel<true, true>), dim3((unsigned)nseq), dim3((1 + BN_NH) * 64), lds, st, x, norm_w, eps, xt, K, norm_out);
    else hipLaunchKernelGGL((batch_rmsnorm_xt_kernel<true, false>), dim3((unsigned)nseq), dim3((1 + BN_NH) * 64), lds, st, x, norm_w, eps, xt, K, norm_out);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_batch_rmsnorm(const uint16_t* x, const uint16_t* norm_w, float eps, uint16_t* xt, int K, int nseq, hipStream_t st) {
    return lnbk_batch_rmsnorm_out(x, norm_w, eps, xt, K, nseq, nullptr, st);
}
extern "C" hipError_t lnbk_batch_embed(const uint16_t* emb, const BatchTab* tab, uint16_t* x, int nseq, int dim, int vocab, int* err, hipStream_t st) {
    hipLaunchKernelGGL(batch_embed_kernel, dim3((unsigned)nseq), dim3(256), 0, st, emb, tab, x, dim, vocab, err);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_batch_argmax(const uint16_t* logits, int V, const BatchTab* tab, int nseq, int32_t* ring, hipStream_t st) {
    hipLaunchKernelGGL(batch_argmax_kernel, dim3((unsigned)nseq), dim3(1024), 0, st, logits, V, tab, ring);
    return hipGetLastError();
}
// one launch for `rows` rows of p->logits: grid G slices x rows, 256 threads (k picks the register top-k: 1 / 2 / 4 / 8 / 16, 0 = none)
extern "C" hipError_t lnbk_token_probs(const TokProbParams* p, hipStream_t st) {
    const dim3 grid((unsigned)p->G, (unsigned)p->rows), block(256);
    const auto k = p->k <= 0 ? token_probs_kernel<0> : p->k <= 1 ? token_probs_kernel<1> : p->k <= 2 ? token_probs_kernel<2> : p->k <= 4 ? token_probs_kernel<4>
                 : p->k <= 8 ? token_probs_kernel<8> : token_probs_kernel<16>;
    hipLaunchKernelGGL(k, grid, block, 0, st, *p);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_batch_set_state(const BatchTab* tab, const int32_t* tokens, const int32_t* pos, int32_t* ring, int honour_stop, hipStream_t st) {
    hipLaunchKernelGGL(batch_set_state_kernel, dim3(1), dim3(LNB_BATCH_MAX), 0, st, tab, tokens, pos, ring, honour_stop);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_batch_scatter_ring(const BatchTab* tab, const int32_t* ring, hipStream_t st) {
    hipLaunchKernelGGL(batch_scatter_ring_kernel, dim3(1), dim3(LNB_BATCH_MAX), 0, st, tab, ring);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_batch_advance(const BatchTab* tab, hipStream_t st) {
    hipLaunchKernelGGL(batch_advance_kernel, dim3(1), dim3(LNB_BATCH_MAX), 0, st, tab);
    return hipGetLastError();
}

// prefill product on the streaming matrix-core feed (gemm_stream_kernel): one weight tile per wave and NTW batch tiles of 16 rows.
// (batch tiles per wave and dispatch order: lnb_gemm_stream_ntw / lnb_gemm_stream_rows_fastest, lnb_device.h -- host logic, tests/test_layouts.py)
// gemm_stream_kernel<EPI, NCH> for ntw batch tiles per wave (1 / 2, else 4), A-operand source src and tt (two weight tiles per wave); nullptr: no such instantiation
// (source 1 and TT: one-chain EPI_STORE / EPI_RESID only).  Prepare walks this function: nothing it returns is launched unraised (up to 66,560 B of LDS)
template <int EPI, int NCH, int SRC> static auto gs_ntw(int ntw) -> void (*)(GemmParams) {
    return ntw == 1 ? gemm_stream_kernel<EPI, NCH, 1, SRC> : ntw == 2 ? gemm_stream_kernel<EPI, NCH, 2, SRC> : gemm_stream_kernel<EPI, NCH, 4, SRC>;
}
template <int EPI, int NCH> static auto gs_kernel(int ntw, int src, bool tt) -> void (*)(GemmParams) {
    if constexpr (NCH == 1 && (EPI == EPI_STORE || EPI == EPI_RESID)) {
        if (tt) return ntw != 4 ? nullptr : src == 0 ? gemm_stream_kernel<EPI, NCH, 4, 0, 1> : src == 1 ? gemm_stream_kernel<EPI, NCH, 4, 1, 1> : nullptr;
        if (src == 1) return gs_ntw<EPI, NCH, 1>(ntw);
    }
    return tt ? nullptr : src == 0 ? gs_ntw<EPI, NCH, 0>(ntw) : src == 2 ? gs_ntw<EPI, NCH, 2>(ntw) : nullptr;
}
template <int EPI, int NCH> static hipError_t launch_gemm_stream(const GemmParams* p, int num_cus, hipStream_t st) {
    if (!p) {
        hipError_t e = hipSuccess;
        for (int ntw : {1, 2, 4}) for (int src = 0; src < 3; src++) for (int tt = 0; tt < 2; tt++)
            if (const auto k = gs_kernel<EPI, NCH>(ntw, src, tt != 0); k && e == hipSuccess) e = raise_lds(k);
        return e;
    }
    // A operand: the M16 copy when the model carries one, else the RESIDENT layout (round 5: no second copy needed for a prompt) -- the row-broadcast
    // layout's units are M16 units in another order (src 1), the chain layouts' units hold eight consecutive k and are transposed inside the quad (src 2)
    const int src = p->w16 ? 0 : (p->w && p->rw == 4 && NCH == 1 && (EPI == EPI_STORE || EPI == EPI_RESID)) ? 1 : (p->w && p->rw >= 16 && p->nch == NCH) ? 2 : -1;
    if (src < 0 || (p->K & 127) || p->S < 1) return hipErrorInvalidValue;
    const int n_tiles = (p->n_rows + 15) / 16;
    const int ct = (p->S + 15) / 16;                         // batch tiles of 16 rows
    int ntw = lnb_gemm_stream_ntw(n_tiles, ct, NCH, num_cus);
    const int force = knob(Knob::GS_NTW);                    // (tools / experiments / tests)
    if (force == 1 || force == 2 || force == 4) ntw = force;
    const int force_ct = knob(Knob::GS_NTW_CHAIN);           // (experiments: the chain layouts only)
    if (src == 2 && (force_ct == 1 || force_ct == 2 || force_ct == 4)) ntw = force_ct;
    GemmParams q = *p;
    // round 6: few batch rows on the chain layouts -- the one-k matrix instruction with FOUR WEIGHT blocks and the B operand broadcast by BLGP (gemm_blgp_kernel):
    // no transpose, no second copy.  Bit-exact and NOT the default: measured slower than the row-swap transpose it was meant to replace (profiles/r06_blgp.log: wq|wk|wv
    // of a 128-token prompt 125-130 us against 91, gate|up 346 against 301; whole Forward 16 / 128 rows 13.2 / 20.7 ms against 9.2 / 19.4) -- a wave carries FOUR weight
    // tiles as ONE dependent chain of 4 K one-k instructions with an unpack op in front of each (67 cycles per instruction instead of 32), and a quarter as many waves
    // to spread over the SIMDs (96 for wq|wk|wv at 16 rows).  LNB_GEMM_BLGP=1: where gemm_stream_kernel would run one or two batch tiles per wave; =2: every chain-layout product
    if (const int blgp = knob(Knob::GEMM_BLGP); src == 2 && blgp && (ntw <= 2 || blgp == 2) && p->rw % 8 == 0) {
        const int tpg = 4 / NCH, n_tg = (n_tiles + tpg - 1) / tpg;
        const dim3 g((unsigned)((n_tg + 3) / 4), (unsigned)ct);
        const size_t l = (size_t)2 * 16 * GS_PITCH * 4;             // (16 KiB + padding: within what every kernel gets)
        form_ran(Form::GEMM_BLGP, EPI);
        hipLaunchKernelGGL((gemm_blgp_kernel<EPI, NCH>), g, dim3(256), l, st, q);
        return hipGetLastError();
    }
    const int rows_wg = 16 * ntw;
    // round 6: wo / w2 with many rows -- two neighbouring weight tiles per wave (gemm_stream_kernel's TT form: the gate|up product's shape), as long as the tile PAIRS still
    // give every CU its two workgroups.  LNB_GS_TT=0: never, 1: whenever the form exists
    bool tt = false;
    if constexpr (NCH == 1 && (EPI == EPI_STORE || EPI == EPI_RESID)) {
        const int ttm = knob(Knob::GS_TT);
        const long wgs = (long)(((n_tiles + 1) / 2 + 3) / 4) * ((p->S + rows_wg - 1) / rows_wg);
        tt = ntw == 4 && (src == 0 || src == 1) && ttm != 0 && (ttm == 1 || wgs >= 2L * num_cus);
    }
    unsigned gx = (unsigned)(((tt ? (n_tiles + 1) / 2 : n_tiles) + 3) / 4); if (gx > (unsigned)num_cus) gx = (unsigned)num_cus;
    const dim3 grid(gx, (unsigned)((p->S + rows_wg - 1) / rows_wg));
    // Dispatch order (workgroup id % 8 = XCD, each with its own L2).  Weight-tile groups fastest: an XCD owns 1/8 of the tile groups for every
    // row group -- right while all row groups are in flight together (<= 8 of them: short prompts, batches), each weight byte is then fetched
    // once; with many row groups the same tile group comes back once per row group (4096 rows: 15.6 GB of fabric reads per gate|up launch
    // for 235 MB of weights, rocprofv3 FETCH_SIZE).  Row groups fastest: the workgroups in flight cover ~8 tile groups x all row groups, a
    // weight tile is fetched once per XCD and shared through its L2 (4.8 GB; 1-4 % faster at 4096 rows, 2-3 % slower at 512).
    const int order = knob(Knob::GS_ORDER);
    q.rows_fastest = order >= 0 ? order : lnb_gemm_stream_rows_fastest((int)grid.y);
    const size_t lds = (size_t)2 * rows_wg * GS_PITCH * 4;
    const auto k = gs_kernel<EPI, NCH>(ntw, src, tt);
    if (!k) return hipErrorInvalidValue;
    // (the table's rows run source-major: copy 1 / 2 / 4 / 4.tt, row-broadcast the same four, chain 1 / 2 / 4)
    form_ran((Form)((int)Form::GS_COPY_1 + 4 * src + (ntw == 1 ? 0 : ntw == 2 ? 1 : tt ? 3 : 2)), EPI);
    form_ran(q.rows_fastest ? Form::GS_ORDER_ROWS : Form::GS_ORDER_TILES, EPI);
    hipLaunchKernelGGL(k, grid, dim3(256), lds, st, q);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_gemm_stream(const GemmParams* p, int epi, int num_cus, hipStream_t st) {
    switch (epi) {
        case EPI_STORE: return launch_gemm_stream<EPI_STORE, 1>(p, num_cus, st);
        case EPI_RESID: return launch_gemm_stream<EPI_RESID, 1>(p, num_cus, st);
        case EPI_QKV_ROPE: return launch_gemm_stream<EPI_QKV_ROPE, 1>(p, num_cus, st);
        case EPI_SILU_MUL: return (p && p->nch != 2) ? hipErrorInvalidValue : launch_gemm_stream<EPI_SILU_MUL, 2>(p, num_cus, st);
        default: return hipErrorInvalidValue;
    }
}

// speculative decoding: column argmax of a verify pass (w rows), the commit, the n-gram draft (one workgroup per n)
extern "C" hipError_t lnbk_spec_argmax(const uint16_t* logits, int V, int w, int32_t* g, hipStream_t st) {
    hipLaunchKernelGGL(spec_argmax_kernel, dim3((unsigned)w), dim3(1024), 0, st, logits, V, g);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_spec_commit(const int32_t* g, int w, const BatchTab* tab, hipStream_t st) {
    hipLaunchKernelGGL(spec_commit_kernel, dim3(1), dim3(64), 0, st, g, w, tab);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_ngram_draft(const DraftParams* p, hipStream_t st) {
    if (p->ngram_min < 1 || p->ngram_max < p->ngram_min || p->ngram_max > LNB_SPEC_MAX_NGRAM || p->max_draft < 0 || p->max_draft > LNB_SPEC_MAX_DRAFT)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ngram_draft_kernel, dim3((unsigned)(p->ngram_max - p->ngram_min + 1)), dim3(256), 0, st, *p);
    return hipGetLastError();
}

// lnb_ctx_fork: rows [0, n_pos) of every cached layer of one context into 1..KVC_MAX_DST others, one launch (lnb_kvcopy.h).  nt: non-temporal loads and
// stores; split > 1: that many destination groups over grid.z.  The caller has checked n_pos against every capacity.
#include "lnb_kvcopy.h"
extern "C" hipError_t lnbk_kv_fork(const KvForkTab* tab, int nt, int split, hipStream_t st) {
    if (!tab || tab->n_arrays < 1 || tab->n_arrays > 65535 || tab->n_dst < 1 || tab->n_dst > KVC_MAX_DST || tab->n_pos < 1 || (tab->kv_dim & 7)) return hipErrorInvalidValue;
    const size_t tk = kvc_tiles(0, tab->kv_dim, tab->n_pos), tv = kvc_tiles(1, tab->kv_dim, tab->n_pos), tmax = tk > tv ? tk : tv;
    size_t gx = KVC_GRID_CAP / (size_t)tab->n_arrays;
    if (gx < 1) gx = 1;
    if (gx > tmax) gx = tmax;
    const int gz = split > 1 ? (split < tab->n_dst ? split : tab->n_dst) : 1;
    const dim3 grid((unsigned)gx, (unsigned)tab->n_arrays, (unsigned)gz);
    form_ran(nt ? Form::KV_FORK_NT : Form::KV_FORK_PLAIN);
    if (gz > 1) form_ran(Form::KV_FORK_SPLIT);
    if (nt) hipLaunchKernelGGL(kv_fork_kernel<true>, grid, dim3(KVC_THREADS), 0, st, *tab);
    else hipLaunchKernelGGL(kv_fork_kernel<false>, grid, dim3(KVC_THREADS), 0, st, *tab);
    return hipGetLastError();
}

// lnb_forward_append_many: per pass, the columns' tables from the call's row and member tables, and the argmax of the members' last rows (lnb_append_many.h)
#include "lnb_append_many.h"
extern "C" hipError_t lnbk_append_many_setup(const AmPass* p, hipStream_t st) {
    if (!p || !p->rows || !p->members || !p->member_kv || !p->tab || !p->kv || !p->st || !p->tok || p->width < 1 || p->width > LNB_BATCH_MAX || p->n_layers < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(append_many_setup_kernel, dim3((unsigned)(1 + p->n_layers)), dim3(LNB_BATCH_MAX), 0, st, *p);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_append_many_finish(const uint16_t* logits, int V, const AmRow* rows, int width, int32_t* out, hipStream_t st) {
    if (!logits || !rows || !out || V < 1 || width < 1 || width > LNB_BATCH_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(append_many_finish_kernel, dim3((unsigned)width), dim3(1024), 0, st, logits, V, rows, out);
    return hipGetLastError();
}

// lnb_decode_speculative_many: per pass, every member's draft, the pass's row table from the grant rule, and the per-member commit (lnb_spec_many.h)
#include "lnb_spec_many.h"
static bool spec_many_tables_ok(const SmPass* p) {
    return p && p->members && p->want && p->running && p->draft && p->best && p->cnt && p->rows && p->seg && p->stats && p->word && p->g &&
           p->n >= 1 && p->n <= LNB_BATCH_MAX && p->budget >= p->n && p->budget <= LNB_BATCH_MAX && p->max_steps >= 1;
}
extern "C" hipError_t lnbk_spec_many_draft(const SmPass* p, hipStream_t st) {
    if (!spec_many_tables_ok(p) || p->n_levels < 1 || p->n_levels > LNB_SPEC_MAX_NGRAM) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_many_draft_kernel, dim3((unsigned)p->n_levels, (unsigned)p->n), dim3(256), 0, st, *p);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_spec_many_pack(const SmPass* p, hipStream_t st) {
    if (!spec_many_tables_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_many_pack_kernel, dim3(1), dim3(LNB_BATCH_MAX), 0, st, *p);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_spec_many_commit(const SmPass* p, hipStream_t st) {
    if (!spec_many_tables_ok(p) || !p->logits || p->V < 1 || p->width < 1 || p->width > LNB_BATCH_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_many_commit_kernel, dim3((unsigned)p->width), dim3(1024), 0, st, *p);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_spec_many_sample_commit(const SmPass* p, hipStream_t st) {
    if (!spec_many_tables_ok(p) || !p->logits || p->V < 1 || p->V > LNB_SAMPLE_MAX_V || p->width < 1 || p->width > LNB_BATCH_MAX || !p->smp || !p->etab) return hipErrorInvalidValue;
    form_ran(Form::SAMPLE_SPEC_MANY);
    hipLaunchKernelGGL(spec_many_sample_commit_kernel, dim3((unsigned)p->width), dim3(1024), 0, st, *p);
    return hipGetLastError();
}
