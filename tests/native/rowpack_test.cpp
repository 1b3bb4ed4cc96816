// rowpack_test.cpp -- csrc/lnb_rowpack.h on the host (tests/test_append_many_cpu.py builds it with -fsanitize=address,undefined and runs it as a child
// process).  For every pass width W in {1, 5, 16, 17, 128} and every row list below it walks the passes exactly as lnb_forward_append_many does and
// compares them with a brute-force enumeration of the rows (member by member, row by row): every row appears exactly once and in order, no pass is
// wider than W, a member's segments are consecutive and ascending, and column + position arithmetic matches.  The segment array handed to the walk
// has exactly W entries: a segment too many is a heap overflow the sanitizer reports.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_rowpack.h"

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void run_case(const char* tag, const std::vector<int32_t>& n_rows, const std::vector<int32_t>& start, int W) {
    const int n = (int)n_rows.size();
    int64_t total = 0;
    for (int32_t r : n_rows) total += r;
    CHECK(rowpack_total(n, n_rows.data()) == total, "%s W=%d: total", tag, W);
    const int64_t passes = rowpack_passes(total, W);
    CHECK(passes == (total + W - 1) / W, "%s W=%d: passes", tag, W);
    RowPackWalk w;
    CHECK(rowpack_begin(&w, n, n_rows.data(), W) == 0, "%s W=%d: begin", tag, W);
    std::vector<RowSeg> segs((size_t)W);                    // exactly W: heap-allocated so that an overrun is caught
    // brute force: (bm, br) = the next row nobody has handed out yet
    int bm = 0; int32_t br = 0; int64_t seen = 0, p = 0;
    int width = 0; int64_t row0 = 0;
    std::vector<int32_t> next_first((size_t)n, 0);           // per member: where its next segment must start
    while (int ns = rowpack_next(&w, segs.data(), &width, &row0)) {
        CHECK(ns >= 1 && ns <= W, "%s W=%d pass %lld: %d segments", tag, W, (long long)p, ns);
        CHECK(width >= 1 && width <= W, "%s W=%d pass %lld: width %d", tag, W, (long long)p, width);
        CHECK(width == rowpack_width(total, W, p), "%s W=%d pass %lld: width %d against the closed form", tag, W, (long long)p, width);
        CHECK(row0 == seen && row0 == p * (int64_t)W, "%s W=%d pass %lld: row0 %lld", tag, W, (long long)p, (long long)row0);
        int col = 0;
        for (int g = 0; g < ns; g++) {
            const RowSeg& s = segs[(size_t)g];
            CHECK(s.member >= 0 && s.member < n && s.count >= 1 && s.col == col, "%s W=%d pass %lld seg %d: member %d count %d col %d", tag, W, (long long)p, g, s.member, s.count, s.col);
            if (s.member < 0 || s.member >= n || s.count < 1) return;
            CHECK(g == 0 || s.member > segs[(size_t)g - 1].member, "%s W=%d pass %lld seg %d: members not ascending", tag, W, (long long)p, g);
            CHECK(s.first == next_first[(size_t)s.member], "%s W=%d pass %lld seg %d: first %d, expected %d", tag, W, (long long)p, g, s.first, next_first[(size_t)s.member]);
            CHECK(s.first + s.count <= n_rows[(size_t)s.member], "%s W=%d pass %lld seg %d: beyond the member's rows", tag, W, (long long)p, g);
            next_first[(size_t)s.member] = s.first + s.count;
            for (int c = s.col; c < s.col + s.count; c++) {   // every column against the enumeration
                CHECK(bm < n && s.member == bm && s.first + (c - s.col) == br, "%s W=%d pass %lld col %d: row (%d, %d), enumeration says (%d, %d)", tag, W, (long long)p, c,
                      s.member, s.first + (c - s.col), bm, br);
                if (bm >= n) return;
                CHECK(rowpack_pos(&s, c, start[(size_t)bm]) == (int64_t)start[(size_t)bm] + br, "%s W=%d pass %lld col %d: position", tag, W, (long long)p, c);
                CHECK(row0 + c == seen, "%s W=%d pass %lld col %d: row index", tag, W, (long long)p, c);
                seen++;
                if (++br == n_rows[(size_t)bm]) { bm++; br = 0; }
            }
            col += s.count;
        }
        CHECK(col == width, "%s W=%d pass %lld: segments cover %d of %d columns", tag, W, (long long)p, col, width);
        p++;
        if (g_bad) return;
    }
    CHECK(seen == total && bm == n && br == 0, "%s W=%d: %lld of %lld rows", tag, W, (long long)seen, (long long)total);
    CHECK(p == passes && w.done == total, "%s W=%d: %lld passes, expected %lld", tag, W, (long long)p, (long long)passes);
    for (int s = 0; s < n; s++) CHECK(next_first[(size_t)s] == n_rows[(size_t)s], "%s W=%d: member %d got %d of %d rows", tag, W, s, next_first[(size_t)s], n_rows[(size_t)s]);
    CHECK(rowpack_next(&w, segs.data(), &width, &row0) == 0 && width == 0, "%s W=%d: the walk goes on after its end", tag, W);
}

int main() {
    const int Ws[] = {1, 5, 16, 17, 128};
    struct Case { const char* tag; std::vector<int32_t> rows, start; };
    std::vector<Case> cases;
    cases.push_back({"one row", {1}, {0}});
    cases.push_back({"single rows", {1, 1, 1, 1, 1, 1, 1}, {0, 5, 9, 0, 131071, 3, 3}});
    cases.push_back({"ragged", {1, 5, 7}, {0, 37, 20}});
    cases.push_back({"ragged 2", {3, 9, 1, 6, 8}, {4, 0, 11, 2, 40}});
    cases.push_back({"longer than 2 W", {2, 300, 1, 257}, {0, 100, 7, 1000}});                 // 300 > 2 * 128, 257 = 2 * 128 + 1
    cases.push_back({"exact multiples", {5440, 1, 5439}, {0, 1, 2}});                              // 10880 = lcm(5, 16, 17, 128): the last pass of every W is full
    cases.push_back({"4 passes of 128", {128, 256, 128}, {0, 1, 2}});                            // a member ends exactly where a pass of 16 / 128 ends
    cases.push_back({"exactly W", {128}, {9}});
    cases.push_back({"16 + 16", {16, 16}, {0, 0}});
    cases.push_back({"6 x 30", {30, 30, 30, 30, 30, 30}, {0, 0, 0, 0, 0, 0}});
    { Case big{"128 x 131072", {}, {}};                                                          // 2^24 rows
      for (int s = 0; s < 128; s++) { big.rows.push_back(131072); big.start.push_back(0); }
      cases.push_back(big); }
    for (int W : Ws)
        for (const Case& c : cases) run_case(c.tag, c.rows, c.start, W);
    // totals in 64 bits: 128 members of 2^31 - 1 rows (nothing to enumerate: the closed forms alone)
    { std::vector<int32_t> huge(128, 2147483647);
      const int64_t t = rowpack_total(128, huge.data());
      CHECK(t == 128LL * 2147483647LL, "64-bit total: %lld", (long long)t);
      CHECK(rowpack_passes(t, 128) == 2147483647LL, "64-bit passes");
      CHECK(rowpack_passes(t, 5) == (t + 4) / 5 && rowpack_passes(t, 1) == t, "64-bit passes at W = 5 / 1");
      CHECK(rowpack_width(t, 128, 2147483646LL) == 128 && rowpack_width(t, 5, (t + 4) / 5 - 1) == (int)(t - ((t + 4) / 5 - 1) * 5), "64-bit last widths"); }
    // refusals
    { RowPackWalk w; const int32_t ok[2] = {1, 2}, zero[2] = {1, 0}, neg[1] = {-4};
      CHECK(rowpack_begin(&w, 2, ok, 0) < 0 && rowpack_begin(&w, 2, ok, 129) < 0 && rowpack_begin(&w, 0, ok, 16) < 0, "bad W / n accepted");
      CHECK(rowpack_begin(&w, 2, zero, 16) < 0 && rowpack_begin(&w, 1, neg, 16) < 0 && rowpack_begin(&w, 2, nullptr, 16) < 0, "bad rows accepted");
      CHECK(rowpack_total(2, zero) < 0 && rowpack_passes(-1, 4) < 0 && rowpack_passes(4, 0) < 0, "closed forms accept bad input"); }
    if (g_bad) { printf("rowpack_test: %d failure(s)\n", g_bad); return 1; }
    printf("rowpack_test: ok\n");
    return 0;
}
