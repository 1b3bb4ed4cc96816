// handoff_test.cpp -- csrc/lnb_handoff.h on the host (tests/test_handoff_cpu.py builds it with -fsanitize=address,undefined and runs it as a
// child process).  The plan of every hand-off -- worlds 1, 2, 3 and 8, cuts between blocks, behind an attention part and behind a gate/up
// part, every rank, both directions, both unit kinds -- is compared with the tables written out below (peers rank by rank, the kind of every
// boundary letter by letter, the byte counts as numbers), and the mailbox is walked through its matches and its four refusals.
#include <cstdio>
#include <cstring>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_handoff.h"

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// dim 64, ffn_hidden 176; a sequence hands over 5 rows, a batch has 3 members
enum { DIM = 64, FFN = 176, ROWS = 5, MEMBERS = 3 };
enum : size_t { SEQ_HIDDEN = 640, SEQ_ACTS = 1760, BATCH_HIDDEN = 384, BATCH_RING = 12, TOKEN_WORD = 4 };

// One pipeline: its cuts and, per boundary between rank r and r + 1, what lies in front of the cut: 'B' a whole block, 'A' an attention
// part, 'G' a gate/up part.  Only behind 'G' do a sequence's activations travel.
struct Pipe { int world; int cuts[9]; const char* boundary; };
static const Pipe PIPES[] = {
    {1, {0, 6}, ""},
    {2, {0, 3, 6}, "B"},
    {2, {0, 1, 6}, "A"},
    {2, {0, 2, 6}, "G"},
    {3, {0, 3, 6, 9}, "BB"},
    {3, {0, 1, 5, 9}, "AG"},
    {3, {0, 2, 4, 9}, "GA"},
    {8, {0, 3, 6, 9, 12, 15, 18, 21, 24}, "BBBBBBB"},
    {8, {0, 1, 2, 3, 4, 5, 7, 8, 9}, "AGBAGAG"},
};
// whom rank r sends to / receives from, per world
static const int SEND_PEER[9][8] = {{}, {-1}, {1, 0}, {1, 2, 0}, {}, {}, {}, {}, {1, 2, 3, 4, 5, 6, 7, 0}};
static const int RECV_PEER[9][8] = {{}, {-1}, {1, 0}, {2, 0, 1}, {}, {}, {}, {}, {7, 0, 1, 2, 3, 4, 5, 6}};

static int check_plans() {
    int checked = 0;
    for (const Pipe& pp : PIPES)
        for (int rank = 0; rank < pp.world; rank++)
            for (int sending = 0; sending <= 1; sending++)
                for (int batch = 0; batch <= 1; batch++) {
                    const int W = pp.world;
                    const HandoffPlan p = handoff_plan(rank, W, pp.cuts[rank], pp.cuts[rank + 1], sending != 0, batch ? HU_BATCH : HU_SEQUENCE, batch ? MEMBERS : ROWS, DIM, FFN);
                    char what[96];
                    snprintf(what, sizeof what, "world %d cuts \"%s\" rank %d %s %s", W, pp.boundary, rank, sending ? "send" : "recv", batch ? "batch" : "sequence");
                    checked++;
                    CHECK(p.sending == (sending != 0) && p.unit == (batch ? HU_BATCH : HU_SEQUENCE), "%s: direction / unit not carried", what);
                    CHECK(p.peer == (sending ? SEND_PEER : RECV_PEER)[W][rank], "%s: peer %d", what, p.peer);
                    if (W == 1) { CHECK(p.nseg == 0 && !p.token, "%s: a one-stage pipe hands nothing over (%d segments)", what, p.nseg); continue; }
                    const bool token = sending ? rank == W - 1 : rank == 0;
                    CHECK(p.token == token, "%s: token hop %d", what, (int)p.token);
                    if (token) {
                        CHECK(p.nseg == 1, "%s: %d segments", what, p.nseg);
                        if (batch) CHECK(p.seg[0].buf == HB_RING && p.seg[0].bytes == BATCH_RING && p.count == MEMBERS, "%s: ring segment (%d, %zu)", what, (int)p.seg[0].buf, p.seg[0].bytes);
                        else CHECK(p.seg[0].buf == (sending ? HB_TOKEN_OUT : HB_TOKEN_IN) && p.seg[0].bytes == TOKEN_WORD && p.count == 1, "%s: token segment (%d, %zu)", what, (int)p.seg[0].buf, p.seg[0].bytes);
                        continue;
                    }
                    const char kind = pp.boundary[sending ? rank : rank - 1];       // the boundary behind this stage / in front of it
                    const bool acts = kind == 'G' && !batch;
                    CHECK(p.edge == pp.cuts[sending ? rank + 1 : rank], "%s: edge %d", what, p.edge);
                    CHECK(p.count == (batch ? MEMBERS : ROWS), "%s: count %d", what, p.count);
                    CHECK(p.nseg == (acts ? 2 : 1), "%s (boundary %c): %d segments", what, kind, p.nseg);
                    CHECK(p.seg[0].buf == HB_HIDDEN && p.seg[0].bytes == (batch ? BATCH_HIDDEN : SEQ_HIDDEN), "%s: hidden segment (%d, %zu)", what, (int)p.seg[0].buf, p.seg[0].bytes);
                    if (acts && p.nseg == 2) CHECK(p.seg[1].buf == HB_ACTS && p.seg[1].bytes == SEQ_ACTS, "%s: activations segment (%d, %zu)", what, (int)p.seg[1].buf, p.seg[1].bytes);
                }
    CHECK(checked == (1 + 3 * 2 + 3 * 3 + 2 * 8) * 4, "%d plans", checked);
    return checked;
}

static size_t queued(const HandoffBox& b) {
    size_t n = 0;
    for (const auto& kv : b.sends) n += kv.second.size();
    for (const auto& kv : b.recvs) n += kv.second.size();
    return n;
}
// the two-stage pipe (0, 3, 6) of most mailbox checks: rank 0 sends what rank 1 receives
static HandoffMsg msg(int* owner, int rank, bool sending, HandoffUnit unit, int count, int part_begin = -1, int part_end = -1) {
    if (part_begin < 0) { part_begin = rank ? 3 : 0; part_end = rank ? 6 : 3; }
    return HandoffMsg{owner, handoff_plan(rank, 2, part_begin, part_end, sending, unit, count, DIM, FFN), {owner, owner + 1}};
}
static void expect_refusal(const char* name, const HandoffMsg& first, int first_rank, const HandoffMsg& late, int late_rank, const char* text) {
    HandoffBox box; HandoffMsg other{}; char why[320] = "";
    CHECK(box.post(first_rank, first, &other, why, sizeof why) == HandoffBox::QUEUED && queued(box) == 1, "%s: the first message is queued", name);
    const HandoffBox::Result r = box.post(late_rank, late, &other, why, sizeof why);
    CHECK(r == HandoffBox::REFUSED, "%s: result %d", name, (int)r);
    CHECK(strstr(why, text) != nullptr, "%s: refused with \"%s\", expected \"%s\"", name, why, text);
    CHECK(other.owner == first.owner, "%s: the counterpart handed back is the waiting message", name);
    CHECK(queued(box) == 0, "%s: after the refusal %zu message(s) queued (the waiting one is consumed, the late one is not queued)", name, queued(box));
}

static void check_mailbox() {
    int a[2], b[2], c[2], d[2];
    char why[320] = "";
    {   // send, then receive
        HandoffBox box; HandoffMsg other{};
        CHECK(box.post(0, msg(a, 0, true, HU_SEQUENCE, 4), &other, why, sizeof why) == HandoffBox::QUEUED, "send first: queued");
        CHECK(box.sends[std::make_pair(0, 1)].size() == 1 && queued(box) == 1, "send first: waits under (source 0, destination 1)");
        CHECK(box.post(1, msg(b, 1, false, HU_SEQUENCE, 4), &other, why, sizeof why) == HandoffBox::MATCHED && other.owner == a && other.plan.sending, "send first: the receive takes it");
        CHECK(other.ptr[0] == a && other.ptr[1] == a + 1 && queued(box) == 0, "send first: pointers carried, queues empty");
    }
    {   // receive, then send
        HandoffBox box; HandoffMsg other{};
        CHECK(box.post(1, msg(b, 1, false, HU_BATCH, 3), &other, why, sizeof why) == HandoffBox::QUEUED && box.recvs[std::make_pair(0, 1)].size() == 1, "receive first: queued under (0, 1)");
        CHECK(box.post(0, msg(a, 0, true, HU_BATCH, 3), &other, why, sizeof why) == HandoffBox::MATCHED && other.owner == b && !other.plan.sending && queued(box) == 0, "receive first: the send takes it");
    }
    {   // the token hop runs under its own key (1, 0); a send towards rank 1 does not meet rank 0's receive
        HandoffBox box; HandoffMsg other{};
        CHECK(box.post(0, msg(a, 0, true, HU_SEQUENCE, 1), &other, why, sizeof why) == HandoffBox::QUEUED, "keys: send 0 -> 1");
        CHECK(box.post(0, msg(c, 0, false, HU_SEQUENCE, 1), &other, why, sizeof why) == HandoffBox::QUEUED && queued(box) == 2, "keys: rank 0's receive waits for rank 1");
        CHECK(box.post(1, msg(d, 1, true, HU_SEQUENCE, 7), &other, why, sizeof why) == HandoffBox::MATCHED && other.owner == c, "keys: the token send meets it whatever its row count");
        CHECK(box.post(1, msg(b, 1, false, HU_SEQUENCE, 1), &other, why, sizeof why) == HandoffBox::MATCHED && other.owner == a && queued(box) == 0, "keys: 0 -> 1 matched");
    }
    {   // two sequences queued on one key come out in order
        HandoffBox box; HandoffMsg other{};
        box.post(0, msg(a, 0, true, HU_SEQUENCE, 1), &other, why, sizeof why);
        box.post(0, msg(c, 0, true, HU_SEQUENCE, 1), &other, why, sizeof why);
        CHECK(queued(box) == 2, "order: two sends wait");
        CHECK(box.post(1, msg(b, 1, false, HU_SEQUENCE, 1), &other, why, sizeof why) == HandoffBox::MATCHED && other.owner == a, "order: the first receive takes the first send");
        CHECK(box.post(1, msg(d, 1, false, HU_SEQUENCE, 1), &other, why, sizeof why) == HandoffBox::MATCHED && other.owner == c && queued(box) == 0, "order: the second takes the second");
    }
    expect_refusal("sequence meets batch", msg(b, 1, false, HU_BATCH, 3), 1, msg(a, 0, true, HU_SEQUENCE, 3), 0, "a single-sequence hand-off met a batch hand-off");
    expect_refusal("batch meets sequence", msg(a, 0, true, HU_SEQUENCE, 3), 0, msg(b, 1, false, HU_BATCH, 3), 1, "a batch hand-off met a single-sequence hand-off");
    expect_refusal("rows", msg(a, 0, true, HU_SEQUENCE, 2), 0, msg(b, 1, false, HU_SEQUENCE, 3), 1, "loopback exchange: 2 rows sent, 3 rows expected");
    expect_refusal("rows, receive first", msg(b, 1, false, HU_SEQUENCE, 3), 1, msg(a, 0, true, HU_SEQUENCE, 2), 0, "loopback exchange: 2 rows sent, 3 rows expected");
    expect_refusal("members", msg(a, 0, true, HU_BATCH, 2), 0, msg(b, 1, false, HU_BATCH, 3), 1, "loopback exchange: a batch of 2 sequences sent, 3 expected");
    expect_refusal("ring members", msg(b, 1, true, HU_BATCH, 2), 1, msg(a, 0, false, HU_BATCH, 3), 0, "loopback exchange: a batch of 2 sequences sent, 3 expected");
    // the sender is cut behind a gate/up part, (0, 2); the receiver was built as (3, 6): the rows agree, the segments do not
    expect_refusal("edges", msg(a, 0, true, HU_SEQUENCE, 4, 0, 2), 0, msg(b, 1, false, HU_SEQUENCE, 4, 3, 6), 1, "the sending stage ends at block part 2");
    expect_refusal("edges, receive first", msg(b, 1, false, HU_SEQUENCE, 4, 3, 6), 1, msg(a, 0, true, HU_SEQUENCE, 4, 0, 2), 0, "the receiving stage begins at part 3");
    {   // the same cut on both sides fits, activations included
        HandoffBox box; HandoffMsg other{};
        box.post(0, msg(a, 0, true, HU_SEQUENCE, 4, 0, 2), &other, why, sizeof why);
        CHECK(box.post(1, msg(b, 1, false, HU_SEQUENCE, 4, 2, 6), &other, why, sizeof why) == HandoffBox::MATCHED && other.plan.nseg == 2, "a cut behind a gate/up part matches with two segments");
    }
}

int main() {
    const int plans = check_plans();
    check_mailbox();
    if (g_bad) { printf("handoff_test: %d failure(s)\n", g_bad); return 1; }
    printf("handoff_test: ok (%d plans)\n", plans);
    return 0;
}
