// lnb_handoff.h -- what crosses a pipeline stage boundary, and the mailbox in which a send meets its receive: pure host logic, plain C++
// over standard headers only (tests/native/handoff_test.cpp compares it with a written-out table under the sanitizers).
//
// A pipeline tick (lnb_pipeline_tick: the unit is one sequence; lnb_pipeline_tick_batch: a batch) hands its unit over the boundary behind
// its stage (a SEND, towards rank + 1) and takes one over the boundary in front of it (a RECEIVE, from rank - 1).  The last rank's send
// and rank 0's receive are the TOKEN HOP that closes the ring.  What travels, stated once for both transports and both units:
//
//   unit      hop     segments (buffer, bytes)
//   sequence  stage   hidden state, rows * dim * 2;  plus the gate*up activations, rows * ffn_hidden * 2, when the edge being crossed has
//                     part % 3 == 2 (the cut lies between a block's gate/up and down parts).  The edge is the stage's part_end when
//                     sending and its part_begin when receiving.
//   sequence  token   4 bytes from the sender's token-out word into the receiver's token-in word, whatever the row count
//   batch     stage   hidden state, n * dim * 2 (a batch's stage holds whole blocks: no activations travel)
//   batch     token   the batch's token ring, n * 4
//
// A one-stage pipe (world 1) has no boundary: its plan has no peer and no segment.
#pragma once
#include <cstddef>
#include <cstdio>
#include <deque>
#include <map>
#include <utility>

enum HandoffBuf { HB_HIDDEN = 0, HB_ACTS, HB_TOKEN_OUT, HB_TOKEN_IN, HB_RING };
enum HandoffUnit { HU_SEQUENCE = 0, HU_BATCH = 1 };

struct HandoffSeg { HandoffBuf buf; size_t bytes; };
struct HandoffPlan {
    bool sending; HandoffUnit unit;
    int count;                           // what the two sides must agree on: rows (a token hop of a sequence: 1), or the batch's members
    int peer;                            // the rank on the other side; -1: a one-stage pipe
    bool token;                          // the token hop
    int edge;                            // the block part at the boundary being crossed
    int nseg; HandoffSeg seg[2];
};

static inline HandoffPlan handoff_plan(int rank, int world, int part_begin, int part_end, bool sending, HandoffUnit unit, int count, int dim, int ffn_hidden) {
    HandoffPlan p{sending, unit, count, -1, false, sending ? part_end : part_begin, 0, {{HB_HIDDEN, 0}, {HB_HIDDEN, 0}}};
    if (world < 2) return p;
    p.token = rank == (sending ? world - 1 : 0);
    p.peer = p.token ? (sending ? 0 : world - 1) : (sending ? rank + 1 : rank - 1);
    const size_t n = (size_t)count;
    if (p.token && unit == HU_BATCH) p.seg[p.nseg++] = {HB_RING, n * 4};
    else if (p.token) { p.count = 1; p.seg[p.nseg++] = {sending ? HB_TOKEN_OUT : HB_TOKEN_IN, 4}; }
    else {
        p.seg[p.nseg++] = {HB_HIDDEN, n * dim * 2};
        if (unit == HU_SEQUENCE && p.edge % 3 == 2) p.seg[p.nseg++] = {HB_ACTS, n * ffn_hidden * 2};
    }
    return p;
}

// One posted hand-off of the in-process transport: whose it is (opaque here), its plan, and where its segments live.
struct HandoffMsg { void* owner; HandoffPlan plan; void* ptr[2]; };

// The mailbox: sends and receives wait per (source rank, destination rank), in posting order.  post() queues a hand-off or, when its
// counterpart is already waiting, takes that one out; a pair that does not fit is refused -- the waiting message is consumed, the late
// one is not queued -- before the caller has enqueued anything.
struct HandoffBox {
    enum Result { QUEUED, MATCHED, REFUSED };
    std::map<std::pair<int, int>, std::deque<HandoffMsg>> sends, recvs;

    // rank: the posting stage's.  MATCHED / REFUSED: *other is the counterpart; REFUSED: why holds the reason.
    Result post(int rank, const HandoffMsg& mine, HandoffMsg* other, char* why, size_t why_cap) {
        const bool sending = mine.plan.sending;
        const std::pair<int, int> key = sending ? std::make_pair(rank, mine.plan.peer) : std::make_pair(mine.plan.peer, rank);
        std::deque<HandoffMsg>& theirs = sending ? recvs[key] : sends[key];
        if (theirs.empty()) { (sending ? sends[key] : recvs[key]).push_back(mine); return QUEUED; }
        *other = theirs.front(); theirs.pop_front();
        const HandoffPlan &s = sending ? mine.plan : other->plan, &r = sending ? other->plan : mine.plan;
        if (mine.plan.unit != other->plan.unit)
            snprintf(why, why_cap, "in-process pipeline: a %s hand-off met a %s hand-off (the stages must post the same ticks in the same order)",
                     mine.plan.unit == HU_BATCH ? "batch" : "single-sequence", other->plan.unit == HU_BATCH ? "batch" : "single-sequence");
        else if (s.count != r.count && s.unit == HU_BATCH) snprintf(why, why_cap, "loopback exchange: a batch of %d sequences sent, %d expected", s.count, r.count);
        else if (s.count != r.count) snprintf(why, why_cap, "loopback exchange: %d rows sent, %d rows expected", s.count, r.count);
        else if (!fits(s, r))
            snprintf(why, why_cap, "loopback exchange: the sending stage ends at block part %d and hands over %d buffer(s), the receiving stage begins at part %d and "
                     "expects %d: the receiver must begin where the sender ends", s.edge, s.nseg, r.edge, r.nseg);
        else return MATCHED;
        return REFUSED;
    }
    // the receiver expects, segment by segment, what the sender sends (a sequence's token leaves one word and arrives in another)
    static bool fits(const HandoffPlan& s, const HandoffPlan& r) {
        if (s.nseg != r.nseg) return false;
        for (int i = 0; i < s.nseg; i++)
            if (s.seg[i].bytes != r.seg[i].bytes || (s.seg[i].buf != r.seg[i].buf && !(s.seg[i].buf == HB_TOKEN_OUT && r.seg[i].buf == HB_TOKEN_IN))) return false;
        return true;
    }
};
