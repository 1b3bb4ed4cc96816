// csrc/lnb_sample.h on the host: the serial whole-row walk of the sampling rule on rows, samplers and draws read from a file the test writes
// (tests/test_sampler_cpu.py compares the output with tests/sampler_ref.py).  Stand-alone, g++ -std=c++17 under the address and undefined-behaviour
// sanitizers, no HIP.
//   file: int32 n_rows, V, n_cases; uint16 rows[n_rows][V]; n_cases x { int32 row; float temperature, top_p; int32 top_k; uint64 seed; int32 has_u, pad; uint64 pos_or_u }
//   output, one line per case: token w_all w_topk w_kept n_candidates n_kept degenerate
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_sample.h"

struct Case { int32_t row; float temperature, top_p; int32_t top_k; uint64_t seed; int32_t has_u, pad; uint64_t pos_or_u; };
static_assert(sizeof(Case) == 40 && sizeof(LnbSampler) == 24 && sizeof(LnbSampleInfo) == 40, "layouts");

static int self_checks() {
    int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)
    CHECK(lnb_sample_splitmix64(0) == 0xE220A8397B1DCDAFULL);                     // the generator's published first output for state 0
    CHECK(lnb_sample_mulhi(~0ULL, ~0ULL) == 0xFFFFFFFFFFFFFFFEULL && lnb_sample_mulhi(1ULL << 63, 2) == 1 && lnb_sample_mulhi(12345, 67890) == 0);
    for (uint64_t a : {0x123456789ABCDEF0ULL, 0xFFFFFFFF00000001ULL, 0x8000000000000000ULL})
        for (uint64_t b : {0x0FEDCBA987654321ULL, 0x00003FFFFFFFFFFFULL, 0xFFFFFFFFFFFFFFFFULL})
            CHECK(lnb_sample_mulhi(a, b) == (uint64_t)(((unsigned __int128)a * b) >> 64));
    // keys: monotone in the value over every candidate pattern, the zeros equal, NaN and -inf no candidates, and the inverse gives the value back
    CHECK(lnb_sample_key(0x7FC0) == 0 && lnb_sample_key(0xFFC0) == 0 && lnb_sample_key(0xFF80) == 0 && lnb_sample_key(0x7F81) == 0);
    CHECK(lnb_sample_key(0x0000) == lnb_sample_key(0x8000) && lnb_sample_key(0x7F80) == 0xFF80 && lnb_sample_key(0xFF7F) == 0x81);
    for (uint32_t p = 0; p < 65536; p++) {
        const uint32_t k = lnb_sample_key((uint16_t)p);
        if (!k) continue;
        uint32_t b = p << 16, b2 = (uint32_t)lnb_sample_key_bits(k) << 16; float f, f2;
        memcpy(&f, &b, 4); memcpy(&f2, &b2, 4);
        CHECK(f == f2);
        if (p != 0x7F80 && p != 0xFF7F && p != 0x8000 && p != 0) {
            const uint16_t up = (p & 0x8000) ? (uint16_t)(p - 1) : (uint16_t)(p + 1);   // the next larger value
            CHECK(lnb_sample_key(up) == k + 1);
        }
    }
    // weights: floor(e * 2^(45 - E)) against ldexp, normal and subnormal e, E down to -1022
    for (double emax : {1.0, 1.9999, 3.7e300, 2.3e-308, 5e-300}) {
        uint64_t mb; memcpy(&mb, &emax, 8);
        const int E = lnb_sample_exponent(mb);
        CHECK(!lnb_sample_degenerate(mb) && E == std::ilogb(emax));
        for (double f : {1.0, 0.75, 0.5000001, 1e-5, 1e-13, 3e-14, 1e-16, 0.0}) {
            const double e = emax * f;
            uint64_t eb; memcpy(&eb, &e, 8);
            const int n = 45 - E;
            const double want = std::floor(std::ldexp(std::ldexp(e, n / 2), n - n / 2));         // (two exact steps: 2^(45 - E) itself can overflow)
            CHECK(lnb_sample_weight(eb, E) == (uint64_t)want);
        }
        CHECK(lnb_sample_weight(mb, E) >> 45 == 1);
    }
    const double inf = INFINITY, sub = 1e-310, zero = 0.0;
    uint64_t b; memcpy(&b, &inf, 8); CHECK(lnb_sample_degenerate(b));
    memcpy(&b, &sub, 8); CHECK(lnb_sample_degenerate(b));
    memcpy(&b, &zero, 8); CHECK(lnb_sample_degenerate(b));
    CHECK(lnb_sample_p(0.5f, 1ULL << 48) == 1ULL << 47 && lnb_sample_p(1e-6f, 1000) == 0);
    CHECK(lnb_sample_scale(0x4000, 1.0f) == 0x4000 && lnb_sample_scale(0x4000, 0.25f) == 0x4100 && lnb_sample_scale(0x0D80, 201326592.0f) == 0x002A);
#undef CHECK
    return fails;
}

int main(int argc, char** argv) {
    if (self_checks()) return 1;
    if (argc < 2) { printf("sample_test: ok (self checks)\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3 || hdr[0] < 1 || hdr[1] < 1 || hdr[2] < 0) { printf("bad header\n"); return 2; }
    const size_t R = (size_t)hdr[0], V = (size_t)hdr[1], N = (size_t)hdr[2];
    std::vector<uint16_t> rows(R * V);
    std::vector<Case> cases(N);
    if (fread(rows.data(), 2, R * V, f) != R * V || (N && fread(cases.data(), sizeof(Case), N, f) != N)) { printf("short file\n"); return 2; }
    fclose(f);
    std::vector<double> etab(65536);
    for (uint32_t i = 0; i < 65536; i++) { const uint32_t b = i << 16; float x; memcpy(&x, &b, 4); etab[i] = std::exp((double)x); }
    for (const Case& c : cases) {
        if (c.row < 0 || (size_t)c.row >= R) { printf("bad row\n"); return 2; }
        const LnbSampler s = {c.temperature, c.top_p, c.top_k, 0, c.seed};
        LnbSampleInfo info;
        const int tok = lnb_sample_row_serial(rows.data() + (size_t)c.row * V, (int)V, etab.data(), &s, c.has_u, c.pos_or_u, &info);
        printf("%d %llu %llu %llu %d %d %d\n", tok, info.w_all, info.w_topk, info.w_kept, info.n_candidates, info.n_kept, info.degenerate);
    }
    printf("sample_test: ok (%zu cases)\n", N);
    return 0;
}
