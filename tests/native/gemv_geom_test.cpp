// The one-token GEMV geometry table (csrc/lnb_gemv_geom.h) on the host, stand-alone under the address and undefined-behaviour sanitizers
// (tests/test_gemv_geom_cpu.py builds and runs it).  The expectations below were recorded from the launch functions as they stood before the table
// existed (profiles/gemv_geometry.md): what a row takes and with how many x staging chunks, and the longest row each packed kernel accepts.
#include <cstdio>
#include "../../include/lnb.h"
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_gemv_geom.h"

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_failed++; } } while (0)

#define X(name) static_assert((int)GEMV_REPORT_##name == LNB_NORM_##name, "report forms numbered as in include/lnb.h");
LNB_GEMV_REPORTS(X)
#undef X
static_assert((int)GEMV_REPORTS == (int)LNB_NORM_ROWS_WIDE, "the fused kernels' forms are the ones in front of the stand-alone norms'");

constexpr int N = (int)Geom::COUNT;
static const int KS[4] = {4096, 8192, 14336, 28672};                 // the 8B and 70B-like row lengths: dim, 70B dim, 8B ffn, 70B ffn
// x staging chunks per stager wave the launch picks for the row at KS[i], 0: refused; plain, then with a fused norm
static const struct { Geom id; int plain[4], norm[4]; } LADDER[] = {
    {Geom::CHAIN16,      {12, 12, 12,  0}, {3, 6, 0, 0}},
    {Geom::CHAIN16_X2,   {12, 12, 12,  0}, {3, 6, 0, 0}},
    {Geom::CHAIN16_LONG, {12, 12, 12, 12}, {2, 6, 6, 0}},
    {Geom::CHAIN32,      {12, 12, 12,  0}, {3, 6, 0, 0}},
    {Geom::CHAIN32_X2,   {12, 12, 12,  0}, {3, 6, 0, 0}},
    {Geom::CHAIN32_LONG, {12, 12, 12, 12}, {2, 6, 6, 0}},
    {Geom::CHAIN32_NORM, {12, 12, 12,  0}, {2, 3, 6, 0}},
    {Geom::CHAIN64,      {12, 12, 12,  0}, {2, 3, 6, 0}},
    {Geom::CHAIN64_X2,   {12, 12, 12,  0}, {2, 3, 6, 0}},
    {Geom::CHAIN56,      {12, 12, 12,  0}, {2, 3, 6, 0}},
    {Geom::CHAIN56_TP,   {12, 12, 12,  0}, {2, 3, 6, 0}},
    {Geom::CHAIN28,      {12, 12, 12,  0}, {2, 3, 6, 0}},
    {Geom::W13_PACKED,   {12, 12,  0,  0}, {2, 3, 0, 0}},
    {Geom::HEAD_PACKED,  {12,  0,  0,  0}, {2, 0, 0, 0}},
    {Geom::QUAD24,       {12, 12, 12,  0}, {2, 6, 6, 0}},
    {Geom::QUAD24_SCHED, {12, 12, 12, 12}, {2, 6, 6, 0}},
    {Geom::QUAD16_256,   {12, 12, 12,  0}, {2, 6, 6, 0}},
    {Geom::QUAD16_128,   {12, 12, 12, 12}, {2, 6, 6, 0}},
};
// what include/lnb.h says of each report form's kernel: quad, rows per block, chains, packed, folding waves
static const struct { int form; bool quad; int rw, nch; bool packed; int nf; } REPORTS[] = {
    {LNB_NORM_CHAIN16, false, 16, 1, false, 2}, {LNB_NORM_CHAIN32, false, 32, 1, false, 6}, {LNB_NORM_CHAIN64, false, 64, 1, false, 6},
    {LNB_NORM_QUAD24, true, 24, 1, false, 6}, {LNB_NORM_QUAD24_SCHED, true, 24, 1, false, 6},
    {LNB_NORM_GATE_UP56, false, 56, 2, false, 7}, {LNB_NORM_GATE_UP28, false, 28, 2, false, 7},
    {LNB_NORM_GATE_UP56_PACKED, false, 56, 2, true, 7}, {LNB_NORM_HEAD_PACKED, false, 64, 2, true, 8},
};

static int chunks_or_refusal(const GemvGeom& g, int K, bool norm) {
    const int xc = gemv_geom_chunks(g, K, norm);
    return gemv_geom_fits(g, K, norm, xc) ? xc : 0;
}
static int largest_k(const GemvGeom& g) {
    int best = 0;
    for (int K = 8; K <= 65536; K += 8) if (gemv_packed_takes(g, K)) best = K;
    return best;
}

int main() {
    // every row is unique, and the packed rows are the two chain rows with a planar copy
    for (int i = 0; i < N; i++) for (int j = 0; j < i; j++) {
        const GemvGeom &a = LNB_GEMV_GEOM_TABLE[i], &b = LNB_GEMV_GEOM_TABLE[j];
        CHECK(!(a.quad == b.quad && a.rw == b.rw && a.nch == b.nch && a.stage == b.stage && a.nh == b.nh && a.r == b.r && a.packed == b.packed));
    }
    for (const GemvGeom& g : LNB_GEMV_GEOM_TABLE) {
        CHECK(g.rw > 0 && g.rw <= 64 && (g.nch == 1 || g.nch == 2) && g.nh >= 1 && g.r >= 1 && g.steps() > 0 && !(g.quad && (g.packed || g.nch != 1)));
        CHECK(g.quad || g.steps() * g.nch * g.rw * 2 == g.stage);                // a chain stage is a whole number of k steps
        CHECK((g.form == Form::GEMV_QUAD) == g.quad && (g.form == Form::GEMV_CHAIN_PK || g.form == Form::GEMV_HEAD_PK) == g.packed);
    }
    // every report form of the fused kernels has exactly one row: the kernel include/lnb.h describes, on helper waves a norm is tested on
    CHECK((int)(sizeof REPORTS / sizeof *REPORTS) == (int)GEMV_REPORTS);
    for (const auto& r : REPORTS) {
        int n = 0;
        for (const GemvGeom& g : LNB_GEMV_GEOM_TABLE) n += g.report == r.form;
        CHECK(n == 1);
        const Geom id = gemv_report_geom(r.form);
        CHECK(id != Geom::COUNT);
        if (id == Geom::COUNT) continue;
        const GemvGeom& g = gemv_geom(id);
        CHECK(g.quad == r.quad && g.rw == r.rw && g.nch == r.nch && g.packed == r.packed && rms_nf(g.nh) == r.nf && rms_norm_helpers_has(g.nh));
        // ... and one a production selection reaches: the default arm of its block height (the schedule's quad form aside), never a by-K or knob-only row
        CHECK(id != Geom::CHAIN16_LONG && id != Geom::CHAIN32_LONG && id != Geom::QUAD16_256 && id != Geom::QUAD16_128 && id != Geom::CHAIN56_TP);
    }
    for (int f = (int)GEMV_REPORTS; f < LNB_NORM_FORMS + 2; f++) CHECK(gemv_report_geom(f) == Geom::COUNT);
    CHECK(gemv_report_geom(-1) == Geom::COUNT);
    CHECK(gemv_geom(Geom::HEAD_PACKED).resident_nch() == 1 && gemv_geom(Geom::HEAD_PACKED).block_rows() == 128);
    CHECK(gemv_geom(Geom::W13_PACKED).resident_nch() == 2 && gemv_geom(Geom::W13_PACKED).block_rows() == 56 && gemv_geom(Geom::CHAIN16).block_rows() == 16);

    // the staging ladder at the model row lengths
    CHECK((int)(sizeof LADDER / sizeof *LADDER) == N);
    for (const auto& l : LADDER) {
        const GemvGeom& g = gemv_geom(l.id);
        for (int i = 0; i < 4; i++) {
            const int plain = chunks_or_refusal(g, KS[i], false), norm = chunks_or_refusal(g, KS[i], true);
            if (plain != l.plain[i] || norm != l.norm[i]) { printf("FAILED row %d K %d: plain %d (expected %d), norm %d (expected %d)\n", (int)l.id, KS[i], plain, l.plain[i], norm, l.norm[i]); g_failed++; }
            CHECK(norm == 0 || norm == 2 || norm == 3 || norm == XCh<true>::value);
            CHECK(plain == 0 || plain == XCh<false>::value);
            CHECK(!(g.quad && norm == 3));
        }
    }
    // the longest rows the packed kernels accept (lnbk_w13p_supported / lnbk_headp_supported before the table: 11904 and 7808)
    CHECK(largest_k(gemv_geom(Geom::W13_PACKED)) == 11904);
    CHECK(largest_k(gemv_geom(Geom::HEAD_PACKED)) == 7808);
    CHECK(!gemv_packed_takes(gemv_geom(Geom::W13_PACKED), 0) && !gemv_packed_takes(gemv_geom(Geom::W13_PACKED), 4100) && gemv_packed_takes(gemv_geom(Geom::W13_PACKED), 4096));

    // which row lengths the row-broadcast (rw 4) and the 24-row quad layout take
    static const struct { int K; bool rw4, rw24; } LAYOUT[] = {{120, false, false}, {128, true, false}, {256, true, true}, {384, true, false}, {16384, true, true}, {16512, false, false}};
    for (const auto& l : LAYOUT) CHECK(gemv_layout_takes(4, l.K) == l.rw4 && gemv_layout_takes(24, l.K) == l.rw24 && gemv_layout_takes(16, l.K));

    if (g_failed) { printf("gemv_geom_test: %d FAILED\n", g_failed); return 1; }
    printf("gemv_geom_test: ok (%d rows)\n", N);
    return 0;
}
