// specpack_test.cpp -- csrc/lnb_specpack.h (the grant rule of lnb_decode_speculative_many) against a brute-force restatement, as a stand-alone
// program under the address and undefined-behaviour sanitizers (tests/test_spec_many_cpu.py builds and runs it).
//
// The restatement hands out the columns ONE AT A TIME, exactly as the rule is written: every running member gets a column; then, while columns
// are left, level j = 1..15, members in order, "if want >= j and a column is left".  The header's early exits must not change a single count.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_specpack.h"

static uint64_t rng_state = 0x1234567ULL;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(rng_state >> 33); }

static int brute(int n, const std::vector<int>& run, const std::vector<int>& want, int budget, std::vector<int>& cols) {
    cols.assign(n, 0);
    int used = 0;
    for (int s = 0; s < n; s++) if (run[s]) { cols[s] = 1; used++; }
    for (int j = 1; j <= 15; j++)
        for (int s = 0; s < n; s++)
            if (run[s] && want[s] >= j && used < budget) { cols[s]++; used++; }
    return used;
}
static int fails = 0;
static void check(int n, const std::vector<int>& run, const std::vector<int>& want, int budget, const char* what) {
    std::vector<int> got(n, -7), ref;                        // exactly n entries: a write past cols[n - 1] is the sanitizer's to find
    const int w = specpack_grant(n, run.data(), want.data(), budget, got.data());
    const int wr = brute(n, run, want, budget, ref);
    bool ok = w == wr;
    int sum = 0, active = 0;
    for (int s = 0; s < n; s++) {
        ok = ok && got[s] == ref[s] && got[s] <= 1 + want[s] && (run[s] ? got[s] >= 1 : got[s] == 0);
        sum += got[s]; active += run[s] ? 1 : 0;
    }
    ok = ok && sum == w && w <= budget && w >= active;
    if (!ok) { fails++; if (fails < 10) printf("MISMATCH %s: n %d budget %d width %d (brute force %d)\n", what, n, budget, w, wr); }
}

int main() {
    // the named cases
    for (int n = 1; n <= 128; n++) {
        std::vector<int> run(n, 1), want(n, 15);
        check(n, run, want, n, "budget == |A|");                                       // no column left: every member exactly one
        std::vector<int> zero(n, 0);
        for (int b = n; b <= 128; b += 7) check(n, run, zero, b, "all wants 0");         // nothing asked for: width n whatever the budget
        if (n < 128) {
            for (int k = 0; k < n; k++) { std::vector<int> one(n, 0); one[k] = 15; check(n, run, one, n + 1, "one member wanting 15 with R = 1"); }
        }
        std::vector<int> small(n);
        int sum = n;
        for (int s = 0; s < n; s++) { small[s] = (int)(rnd() % 2); sum += small[s]; }
        if (sum < 128) check(n, run, small, 128, "R larger than the sum of wants");    // everybody gets all it wants, columns stay unused
    }
    { std::vector<int> run{1, 1, 1}, want{15, 0, 2}, cols(3);
      // budget 5: level 1 gives members 0 and 2 one column each -> {2, 1, 2}; a long draft does not starve the short one
      if (specpack_grant(3, run.data(), want.data(), 5, cols.data()) != 5 || cols[0] != 2 || cols[1] != 1 || cols[2] != 2) { fails++; printf("MISMATCH levels\n"); }
      if (specpack_grant(3, run.data(), want.data(), 8, cols.data()) != 8 || cols[0] != 4 || cols[1] != 1 || cols[2] != 3) { fails++; printf("MISMATCH levels (8)\n"); }
      run[0] = 0;
      if (specpack_grant(3, run.data(), want.data(), 3, cols.data()) != 3 || cols[0] != 0 || cols[1] != 1 || cols[2] != 2) { fails++; printf("MISMATCH not running\n"); } }
    // random inputs: n = 1..128, wants 0..15, budgets n..128, some members not running
    long cases = 0;
    for (int n = 1; n <= 128; n++)
        for (int it = 0; it < 60; it++) {
            std::vector<int> run(n), want(n);
            const int mode = it % 3;
            for (int s = 0; s < n; s++) { run[s] = mode == 0 ? 1 : (rnd() % 4 != 0); want[s] = mode == 2 ? (int)(rnd() % 3) : (int)(rnd() % 16); }
            const int budget = n + (int)(rnd() % (128 - n + 1));
            check(n, run, want, budget, "random"); cases++;
        }
    // refusals
    { std::vector<int> run(4, 1), want(4, 3), cols(4);
      const int bad_want[4] = {3, 16, 3, 3}, neg_want[4] = {3, -1, 3, 3};
      if (specpack_grant(0, run.data(), want.data(), 16, cols.data()) != -1 || specpack_grant(129, run.data(), want.data(), 128, cols.data()) != -1 ||
          specpack_grant(4, run.data(), want.data(), 3, cols.data()) != -1 || specpack_grant(4, run.data(), want.data(), 129, cols.data()) != -1 ||
          specpack_grant(4, run.data(), bad_want, 16, cols.data()) != -1 || specpack_grant(4, run.data(), neg_want, 16, cols.data()) != -1) { fails++; printf("MISMATCH refusals\n"); } }
    if (fails) { printf("specpack_test: %d FAILED\n", fails); return 1; }
    printf("specpack_test: ok (%ld random cases)\n", cases);
    return 0;
}
