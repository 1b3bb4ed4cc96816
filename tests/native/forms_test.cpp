// csrc/lnb_forms.h on the host: the table's names, lookup, the per-epilogue counters and their reset.  g++ -std=c++17, no HIP.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <vector>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_forms.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main() {
    // ---- the table: one row per enumerator, unique names of [a-z0-9_.], no name a dotted prefix of another, every row with a purpose
    const int n = (int)Form::COUNT;
    CHECK(sizeof LNB_FORM_TABLE / sizeof LNB_FORM_TABLE[0] == (size_t)n && n >= 30);
    std::set<std::string> seen;
    for (const FormInfo& f : LNB_FORM_TABLE) {
        CHECK(f.name && *f.name && f.purpose && strlen(f.purpose) > 10);
        CHECK(strspn(f.name, "abcdefghijklmnopqrstuvwxyz0123456789_.") == strlen(f.name));
        CHECK(f.name[0] != '.' && f.name[strlen(f.name) - 1] != '.' && !strstr(f.name, ".."));
        CHECK(seen.insert(f.name).second);
    }
    for (const FormInfo& a : LNB_FORM_TABLE) for (const FormInfo& b : LNB_FORM_TABLE)      // "a" and "a.x" side by side: what would the prefix "a" mean
        CHECK(!(strlen(b.name) > strlen(a.name) && !strncmp(a.name, b.name, strlen(a.name)) && b.name[strlen(a.name)] == '.'));
    // ---- lookup: every name finds its own row, nothing else finds one
    for (int i = 0; i < n; i++) CHECK(form_index(LNB_FORM_TABLE[i].name) == i);
    CHECK(form_index("gemm_mfma") == -1 && form_index("") == -1 && form_index(nullptr) == -1 && form_index("gemm_mfma.t64 ") == -1);
    CHECK(form_index("gemm_mfma.t64") == (int)Form::GEMM_MFMA_T64 && form_index("pipeline.eager") == n - 1);
    // the streaming feed's rows run source-major, four per source (launch_gemm_stream computes the row from source and tiles per wave)
    CHECK((int)Form::GS_ROWCAST_1 == (int)Form::GS_COPY_1 + 4 && (int)Form::GS_CHAIN_1 == (int)Form::GS_COPY_1 + 8 && (int)Form::GS_CHAIN_4 == (int)Form::GS_COPY_1 + 10);
    CHECK((int)Form::GS_COPY_4_TT == (int)Form::GS_COPY_1 + 3 && (int)Form::GS_ROWCAST_4_TT == (int)Form::GS_ROWCAST_1 + 3);
    // ---- counters: zero at start, one cell per (form, epilogue), epi -1 the sum, out-of-range queries refused, reset clears everything
    for (int i = 0; i < n; i++) CHECK(form_count(i, -1) == 0);
    form_ran(Form::GEMM_MFMA_T64, 2); form_ran(Form::GEMM_MFMA_T64, 2); form_ran(Form::GEMM_MFMA_T64, 3); form_ran(Form::RMSNORM_ROWS_WAVE);
    CHECK(form_count((int)Form::GEMM_MFMA_T64, 2) == 2 && form_count((int)Form::GEMM_MFMA_T64, 3) == 1 && form_count((int)Form::GEMM_MFMA_T64, 0) == 0);
    CHECK(form_count((int)Form::GEMM_MFMA_T64, -1) == 3 && form_count((int)Form::RMSNORM_ROWS_WAVE, 0) == 1 && form_count((int)Form::RMSNORM_ROWS_WAVE, -1) == 1);
    CHECK(form_count((int)Form::GEMM_MFMA_T16, -1) == 0 && form_count((int)Form::GEMM_MFMA_T128, -1) == 0);        // the neighbours untouched
    CHECK(form_count(-1, 0) == -1 && form_count(n, 0) == -1 && form_count(0, LNB_FORM_EPIS) == -1 && form_count(0, -2) == -1);
    form_ran(Form::MFMA_PAIR, 99); CHECK(form_count((int)Form::MFMA_PAIR, 0) == 1);      // an epilogue out of range lands in cell 0, never outside the table
    form_count_reset();
    for (int i = 0; i < n; i++) for (int e = -1; e < LNB_FORM_EPIS; e++) CHECK(form_count(i, e) == 0);
    // ---- relaxed atomics: concurrent launches lose no count
    std::vector<std::thread> th;
    for (int t = 0; t < 8; t++) th.emplace_back([] { for (int i = 0; i < 10000; i++) form_ran(Form::GEMV_CHAIN_PK, 3); });
    for (auto& t : th) t.join();
    CHECK(form_count((int)Form::GEMV_CHAIN_PK, 3) == 80000);
    form_count_reset();
    if (!fails) printf("forms_test: ok (%d forms)\n", n);
    return fails ? 1 : 0;
}
