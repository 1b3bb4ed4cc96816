// csrc/lnb_sample.h on the host under logit rules: the serial whole-row walk with step 0 and step 4b on rows, count rows, bias rows and cases read from a
// file the test writes (tests/test_logit_rules_cpu.py compares the output with tests/logit_rules_ref.py).  Stand-alone, g++ -std=c++17 under the address
// and undefined-behaviour sanitizers, no HIP.
//   file: int32 n_rows, V, n_count_rows, n_bias_rows, n_cases; uint16 rows[n_rows][V]; uint32 counts[n_count_rows][V]; uint16 bias[n_bias_rows][V];
//         n_cases x Case (count_row / bias_row -1: none)
//   output, one line per case: token w_all w_topk w_kept n_candidates n_kept degenerate
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_sample.h"

struct Case { int32_t row, count_row, bias_row; float temperature, top_p; int32_t top_k; uint64_t seed; float rp, presence, frequency, min_p; int32_t has_u, pad; uint64_t pos_or_u; };
static_assert(sizeof(Case) == 64 && sizeof(LnbRulesDev) == 32, "layouts");

static int self_checks() {
    int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)
    // 0a: a positive entry is divided, anything else multiplied
    CHECK(lnb_sample_penalise(0x4040, 1, 1.5f, 0.0f, 0.0f) == 0x4000 && lnb_sample_penalise(0xC000, 1, 1.5f, 0.0f, 0.0f) == 0xC040);
    CHECK(lnb_sample_penalise(0x0000, 9, 1.5f, 0.0f, 0.0f) == 0x0000 && lnb_sample_penalise(0x8000, 9, 1.5f, 0.0f, 0.0f) == 0x8000);
    CHECK(lnb_sample_penalise(0x4040, 70000, 1.0f, 0.0f, 1e-5f) == 0x4013 && lnb_sample_penalise(0x4040, 1, 1.0f, 0.5f, 0.0f) == 0x4020);
    // 0b is two roundings: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11, which the subtraction then cancels; an fma would leave 2^-24
    const float a12 = 1.0f + 0.000244140625f;
    CHECK(lnb_sample_fmul_host(a12, a12) - (1.0f + 0.00048828125f) == 0.0f);
    CHECK(lnb_sample_add_bias(0x4040, 0xFF80) == 0xFF80 && lnb_sample_add_bias(0x4040, 0x0000) == 0x4040 && lnb_sample_add_bias(0x8000, 0x0000) == 0x0000);
    CHECK(lnb_sample_key(lnb_sample_add_bias(0x7F80, 0xFF80)) == 0);                  // +inf banned: NaN, no candidate
    CHECK(lnb_sample_min_weight(0.0f, 1ULL << 45) == 1 && lnb_sample_min_weight(1.0f, (1ULL << 46) - 1) == (1ULL << 46) - 1 && lnb_sample_min_weight(0.5f, 1ULL << 45) == 1ULL << 44);
#undef CHECK
    return fails;
}

int main(int argc, char** argv) {
    if (self_checks()) return 1;
    if (argc < 2) { printf("sample_rules_test: ok (self checks)\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[5];
    if (fread(hdr, 4, 5, f) != 5 || hdr[0] < 1 || hdr[1] < 1 || hdr[2] < 0 || hdr[3] < 0 || hdr[4] < 0) { printf("bad header\n"); return 2; }
    const size_t R = (size_t)hdr[0], V = (size_t)hdr[1], RC = (size_t)hdr[2], RB = (size_t)hdr[3], N = (size_t)hdr[4];
    std::vector<uint16_t> rows(R * V), bias(RB * V), adjusted(V);
    std::vector<uint32_t> counts(RC * V);
    std::vector<Case> cases(N);
    if (fread(rows.data(), 2, R * V, f) != R * V || (RC && fread(counts.data(), 4, RC * V, f) != RC * V) || (RB && fread(bias.data(), 2, RB * V, f) != RB * V) ||
        (N && fread(cases.data(), sizeof(Case), N, f) != N)) { printf("short file\n"); return 2; }
    fclose(f);
    std::vector<double> etab(65536);
    for (uint32_t i = 0; i < 65536; i++) { const uint32_t b = i << 16; float x; memcpy(&x, &b, 4); etab[i] = std::exp((double)x); }
    for (const Case& c : cases) {
        if (c.row < 0 || (size_t)c.row >= R || c.count_row < -1 || c.count_row >= (int)RC || c.bias_row < -1 || c.bias_row >= (int)RB) { printf("bad row\n"); return 2; }
        const LnbSampler s = {c.temperature, c.top_p, c.top_k, 0, c.seed};
        const LnbRulesDev ru = {c.rp, c.presence, c.frequency, c.min_p, c.count_row < 0 ? nullptr : counts.data() + (size_t)c.count_row * V,
                                c.bias_row < 0 ? nullptr : bias.data() + (size_t)c.bias_row * V};
        LnbSampleInfo info;
        const int tok = lnb_sample_row_serial(rows.data() + (size_t)c.row * V, (int)V, etab.data(), &s, c.has_u, c.pos_or_u, &info, &ru, adjusted.data());
        printf("%d %llu %llu %llu %d %d %d\n", tok, info.w_all, info.w_topk, info.w_kept, info.n_candidates, info.n_kept, info.degenerate);
    }
    printf("sample_rules_test: ok (%zu cases)\n", N);
    return 0;
}
