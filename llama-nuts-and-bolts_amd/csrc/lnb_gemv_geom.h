// Every one-token GEMV GEOMETRY the launch layer can pick, one row each: which gemv_chain_kernel / gemv_chain_pk_kernel / gemv_quad_kernel instantiation
// serves a block height and chain count, the LDS and staging registers it needs, and the tally row it counts under.  Plain C++17, no HIP
// (tests/native/gemv_geom_test.cpp).  The launch functions of lnb_kernels.hip take a row (launch_chain_t<Geom::CHAIN64, ...>) and read everything from
// it; lnbk_gemv_norm_report looks its REPORT instantiation up in the same table, so what tests/test_gpu_norm_sum.py proves is what production runs;
// lnbk_init prepares by walking it; lnb_api.cpp reads the layouts' row lengths and the report forms' matrices from it.
// WHY each geometry is what it is stands where it is picked (launch_gemv_rw, lnbk_gemv_w13p, lnbk_gemv_headp in lnb_kernels.hip).
#pragma once
#include <cstddef>
#include "lnb_seqsum.h"
#include "lnb_forms.h"

// ring stages in flight per helper, the three a -D build overrides (tools/kernel_ab.py)
#ifndef LNB_QUAD_R
#define LNB_QUAD_R 5                                        // gemv_quad_kernel<24, 256, ...> (A/B builds: 4, 6)
#endif
#ifndef LNB_W13P_R
#define LNB_W13P_R 5                                        // gate|up from the 13-bit copy: stages of 52 bytes per lane (5: the raw form's 114 KB per CU)
#endif
#ifndef LNB_HEADP_R
#define LNB_HEADP_R 5                                       // the LM head from its 13-bit copy (5: 133 KB per CU)
#endif

// the fused kernels' LNB_NORM_* report forms of include/lnb.h, in its order (lnb_kernels.hip asserts the values against that header)
#define LNB_GEMV_REPORTS(X) X(CHAIN16) X(CHAIN32) X(CHAIN64) X(QUAD24) X(QUAD24_SCHED) X(GATE_UP56) X(GATE_UP28) X(GATE_UP56_PACKED) X(HEAD_PACKED)
#define X(name) GEMV_REPORT_##name,
enum GemvReport { GEMV_REPORT_NONE = -1, LNB_GEMV_REPORTS(X) GEMV_REPORTS };
#undef X

// id | quad | rows per block and chain | chains | chain: bf16 bytes per stage, quad: k steps per stage | helper waves | ring stages | packed | tally row | report form
#define LNB_GEMV_GEOMS(X) \
    /* gemv_chain_kernel from the raw bf16 */ \
    X(CHAIN16,       false, 16, 1,  8192, 2, 7,           false, GEMV_CHAIN_16,    CHAIN16) \
    X(CHAIN16_X2,    false, 16, 2,  8192, 2, 7,           false, GEMV_CHAIN_16,    NONE) \
    X(CHAIN16_LONG,  false, 16, 1,  8192, 4, 7,           false, GEMV_CHAIN_16,    NONE)                 /* plain, rows past three stager waves' registers */ \
    X(CHAIN32,       false, 32, 1,  8192, 2, 7,           false, GEMV_CHAIN_32,    NONE) \
    X(CHAIN32_X2,    false, 32, 2,  8192, 2, 7,           false, GEMV_CHAIN_32,    NONE) \
    X(CHAIN32_LONG,  false, 32, 1,  8192, 4, 7,           false, GEMV_CHAIN_32,    NONE) \
    X(CHAIN32_NORM,  false, 32, 1, 12288, 6, 5,           false, GEMV_CHAIN_32,    CHAIN32)              /* one chain with the fused RMSNorm: wq|wk|wv */ \
    X(CHAIN64,       false, 64, 1, 12288, 6, 8,           false, GEMV_CHAIN_64,    CHAIN64) \
    X(CHAIN64_X2,    false, 64, 2, 12288, 6, 8,           false, GEMV_CHAIN_64,    NONE) \
    X(CHAIN56,       false, 56, 2, 14336, 7, 8,           false, GEMV_CHAIN_56,    GATE_UP56) \
    X(CHAIN56_TP,    false, 56, 2, 14336, 7, 6,           false, GEMV_CHAIN_56_TP, NONE)                 /* the throughput schedule's gate|up */ \
    X(CHAIN28,       false, 28, 2, 14336, 7, 8,           false, GEMV_CHAIN_28,    GATE_UP28) \
    /* gemv_chain_pk_kernel from the 13-bit planar copies (lnb_wpack.h: 7 * 64 lanes of gate|up; WPACK_HEAD_RW rows and WPACK_HEAD_LANES / 64 helpers) */ \
    X(W13_PACKED,    false, 56, 2, 28672, 7, LNB_W13P_R,  true,  GEMV_CHAIN_PK,    GATE_UP56_PACKED) \
    X(HEAD_PACKED,   false, 64, 2, 32768, 8, LNB_HEADP_R, true,  GEMV_HEAD_PK,     HEAD_PACKED) \
    /* gemv_quad_kernel */ \
    X(QUAD24,        true,  24, 1,   256, 6, LNB_QUAD_R,  false, GEMV_QUAD,        QUAD24) \
    X(QUAD24_SCHED,  true,  24, 1,   128, 6, 10,          false, GEMV_QUAD,        QUAD24_SCHED)         /* the throughput schedule's wq|wk|wv */ \
    X(QUAD16_256,    true,  16, 1,   256, 4, 7,           false, GEMV_QUAD,        NONE)                 /* LNB_W2_QUAD=2 */ \
    X(QUAD16_128,    true,  16, 1,   128, 4, 14,          false, GEMV_QUAD,        NONE)                 /* LNB_W2_QUAD=1 */

constexpr int GQ_SLOTS = 3;                                  // product stages of gemv_quad_kernel's LDS ring
SEQ_HD constexpr int gq_ncw(int RW) { return (RW + 15) / 16; }       // its chain waves
// the RMSNorm prologue's LDS scratch on NH folding waves (laid out in lnb_kernels.hip, "LDS scratch"): it lives in the idle product ring
SEQ_HD constexpr size_t rms_scratch_bytes(int NH) { return (size_t)NH * (512 + 8 + 4 + 4 + 2048 + 8) + 64; }
// 512-element x chunks a stager wave holds in registers at most: 12 in the plain kernels, 6 in the RMSNorm kernels (which also hold the norm weights)
template <bool NORM> struct XCh { static constexpr int value = NORM ? 6 : 12; };
constexpr size_t GEMV_LDS_MAX = 160 * 1024;

struct GemvGeom {
    bool quad;
    int rw, nch, stage, nh, r;
    bool packed;
    Form form;
    int report;                                              // GemvReport (= LNB_NORM_*), GEMV_REPORT_NONE without a report form
    constexpr int steps() const { return quad ? stage : stage / (nch * rw * 2); }                        // k steps per stage
    constexpr int waves() const { return (quad ? gq_ncw(rw) : 1) + nh; }                                 // all of them stage x
    constexpr size_t ring_bytes() const { return quad ? GQ_SLOTS * ((size_t)rw * stage * 4) : 4 * (size_t)stage; }      // the f32 products in the LDS
    // the resident layout the matrix is read from: the packed LM head walks blocks of 2 x 64 rows cut from the one-chain 64-row layout
    constexpr int resident_nch() const { return form == Form::GEMV_HEAD_PK ? 1 : nch; }
    constexpr int block_rows() const { return rw * nch / resident_nch(); }                               // rows (per resident chain) of one block
};
#define X(id, quad, rw, nch, stage, nh, r, packed, form, report) id,
enum class Geom { LNB_GEMV_GEOMS(X) COUNT };
#undef X
#define X(id, quad, rw, nch, stage, nh, r, packed, form, report) {quad, rw, nch, stage, nh, r, packed, Form::form, GEMV_REPORT_##report},
constexpr GemvGeom LNB_GEMV_GEOM_TABLE[] = {LNB_GEMV_GEOMS(X)};
#undef X
constexpr const GemvGeom& gemv_geom(Geom g) { return LNB_GEMV_GEOM_TABLE[(int)g]; }
// the row whose REPORT instantiation serves an LNB_NORM_* form (Geom::COUNT: a stand-alone norm kernel's form, or none)
constexpr Geom gemv_report_geom(int report) {
    for (int i = 0; i < (int)Geom::COUNT; i++) if (report >= 0 && LNB_GEMV_GEOM_TABLE[i].report == report) return (Geom)i;
    return Geom::COUNT;
}

// x staging: a whole number of stages + 64 floats of slack
constexpr size_t xs_bytes(int K, int steps_per_stage) { return ((size_t)((K + steps_per_stage - 1) / steps_per_stage) * steps_per_stage + 320) * 4 + 16; }
// x staging chunks per stager wave: the norm-fused kernels are instantiated for 2, 3 and 6 chunks of 512 elements per wave (K up to ~4 K, ~6 K / 12 K with
// the 70B-like shape's 8192 in the middle one, 24 K; quad: 2 and 6) and the smallest that holds the padded row is launched; the plain kernels keep their 12
constexpr int gemv_geom_chunks(const GemvGeom& g, int K, bool norm) {
    const size_t need = xs_bytes(K, g.steps()) / 4, per = (size_t)g.waves() * 512;
    if (norm && need <= 2 * per) return 2;
    if (norm && !g.quad && need <= 3 * per) return 3;
    return norm ? XCh<true>::value : XCh<false>::value;
}
// what a launch checks of its row length: whole stages (quad), LDS, x staging registers at xc chunks per wave, and with a fused norm its records inside the
// idle ring and a leaf whose over-read stays inside the x padding
SEQ_HD bool gemv_geom_fits(const GemvGeom& g, int K, bool norm, int xc) {
    const size_t xs = xs_bytes(K, g.steps());
    if (g.quad && K % g.stage) return false;                 // (auto_rw in lnb_api.cpp picks the layout accordingly)
    if (g.ring_bytes() + xs > GEMV_LDS_MAX || xs / 4 > (size_t)xc * g.waves() * 512) return false;
    return !norm || (rms_scratch_bytes(rms_nf(g.nh)) <= g.ring_bytes() && seq_leaf_size(K, rms_nf(g.nh) * 64) <= 256);
}
// a packed row (always norm-fused) takes in_features K
SEQ_HD bool gemv_packed_takes(const GemvGeom& g, int K) { return K > 0 && K % 8 == 0 && gemv_geom_fits(g, K, true, XCh<true>::value); }
// resident layout rw takes row length K: the row-broadcast layout stages x as 8 x 16 B per thread in K * 4 bytes of LDS, the 24-row quad layout whole stages
constexpr bool gemv_layout_takes(int rw, int K) { return rw == 4 ? K % 128 == 0 && K <= 16384 : rw == 24 ? K % gemv_geom(Geom::QUAD24).stage == 0 : true; }
