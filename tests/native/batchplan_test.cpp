// batchplan_test.cpp -- csrc/lnb_batchplan.h on the host (tests/test_batchplan_cpu.py builds it with -fsanitize=address,undefined and runs it as a
// child process).  For every width n = 1..128, with and without the matrix-core copy, with LNB_BATCH_GROUPS 0 and 1 (and 7: any non-zero
// value is "on"), the plan is compared with the table of the batched forms written out below row by row -- not computed by the header's logic --
// and the layout code derived from it with 0 (B-operand columns) / 1 (column groups) / 2 (rows).
#include <cstdio>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_batchplan.h"

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Row { const char* name; char qkv, wo, w13, w2, head; int layout; };     // 'C' / 'R'
static const Row ALL_COLUMNS = {"copy present, n <= 16", 'C', 'C', 'C', 'C', 'C', 0};
static const Row GROUPS = {"copy present, 17 <= n <= 32, knob != 0", 'C', 'C', 'R', 'C', 'R', 1};
static const Row ALL_ROWS = {"everything else", 'R', 'R', 'R', 'R', 'R', 2};
// ceil(n / 16) of the widths that run groups, one by one
static int groups_of(int n) { return n >= 17 && n <= 32 ? 2 : -1; }

int main() {
    const int knobs[] = {0, 1, 7};
    int checked = 0;
    for (int n = 1; n <= 128; n++)
        for (int copy = 0; copy <= 1; copy++)
            for (int knob : knobs) {
                const Row* want = &ALL_ROWS;
                int want_groups = 0;
                if (copy && n <= 16) want = &ALL_COLUMNS;
                else if (copy && n >= 17 && n <= 32 && knob != 0) { want = &GROUPS; want_groups = groups_of(n); }
                const BatchPlan p = batch_plan(n, copy != 0, knob);
                const char got[BP_COUNT] = {p.feed[BP_QKV] == FEED_COLUMN ? 'C' : 'R', p.feed[BP_WO] == FEED_COLUMN ? 'C' : 'R', p.feed[BP_W13] == FEED_COLUMN ? 'C' : 'R',
                                            p.feed[BP_W2] == FEED_COLUMN ? 'C' : 'R', p.feed[BP_HEAD] == FEED_COLUMN ? 'C' : 'R'};
                const char tab[BP_COUNT] = {want->qkv, want->wo, want->w13, want->w2, want->head};
                for (int i = 0; i < BP_COUNT; i++)
                    CHECK(got[i] == tab[i], "n=%d copy=%d knob=%d (%s): product %d takes %c, the table says %c", n, copy, knob, want->name, i, got[i], tab[i]);
                for (int i = 0; i < BP_COUNT; i++) CHECK(p.feed[i] == FEED_COLUMN || p.feed[i] == FEED_ROW, "n=%d copy=%d knob=%d: feed %d of product %d", n, copy, knob, (int)p.feed[i], i);
                CHECK(p.groups == want_groups, "n=%d copy=%d knob=%d (%s): %d groups, the table says %d", n, copy, knob, want->name, p.groups, want_groups);
                CHECK(batch_plan_layout(p) == want->layout, "n=%d copy=%d knob=%d (%s): layout %d, expected %d", n, copy, knob, want->name, batch_plan_layout(p), want->layout);
                checked++;
            }
    CHECK(checked == 128 * 2 * 3, "%d cases", checked);
    // the products are five, in the order the table lists them, and a column group holds 16 sequences
    CHECK(BP_QKV == 0 && BP_WO == 1 && BP_W13 == 2 && BP_W2 == 3 && BP_HEAD == 4 && BP_COUNT == 5 && BATCHPLAN_COLS == 16, "enumeration order");
    if (g_bad) { printf("batchplan_test: %d failure(s)\n", g_bad); return 1; }
    printf("batchplan_test: ok\n");
    return 0;
}
