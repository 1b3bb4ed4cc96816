// lnb_batchplan.h -- which feed every product of a batched step takes: pure host arithmetic, plain C++ that includes nothing
// (tests/native/batchplan_test.cpp compares it with the table below under the sanitizers).
//
// A batched step of n sequences (lnb_batch_decode, a batched pipeline tick, a verify pass, a pass of lnb_forward_append_many) runs five
// products per block -- wq|wk|wv, wo, w1|w3, w2 -- and the output head.  Each takes its activations from one of two feeds:
//   COLUMN  mfma_stream_kernel / mfma_pair_kernel on the matrix-core copy of the weights (lnb_model_enable_batch); the activations in the
//           B-operand layout [K][16 sequences]; a normed product has the column norm in front of it;
//   ROW     gemm_stream_kernel on the copy or, without one, on the resident layouts; the activations as plain rows [n][K]; a normed
//           product has the row norm in front of it.
// The plan of a step follows from its width, from whether the model carries the copy and from the LNB_BATCH_GROUPS knob (passed in: this
// header reads no environment):
//
//   condition                                                        qkv  wo  w13  w2  head  groups
//   copy present, n <= 16                                             C    C   C    C   C     0
//   copy present, 17 <= n <= 32, knob != 0                            C    C   R    C   R     ceil(n / 16)
//   everything else (no copy at any n; n > 32; 17..32 with knob 0)    R    R   R    R   R     0
//
// groups != 0: the thin matrices run as that many column groups of 16 on disjoint CUs (every CU carries two chains) and the fat ones
// (w1|w3, the head) stay rows.  One rule covers the layouts between the products: a producer writes what its consumer's feed reads -- the
// attention writes B-operand columns when wo is COLUMN and rows otherwise, the SiLU*up epilogue of w1|w3 likewise for w2.
#pragma once

#define BATCHPLAN_COLS 16                // LNB_STREAM_COLS of lnb_device.h: the sequences of one column group

enum BatchFeed { FEED_COLUMN = 0, FEED_ROW = 1 };
enum BatchProduct { BP_QKV = 0, BP_WO, BP_W13, BP_W2, BP_HEAD, BP_COUNT };

struct BatchPlan {
    BatchFeed feed[BP_COUNT];
    int groups;                          // 0, or the column groups of the 17..32 form
};

static inline BatchPlan batch_plan(int n, bool copy, int groups_knob) {
    BatchPlan p{{FEED_ROW, FEED_ROW, FEED_ROW, FEED_ROW, FEED_ROW}, 0};
    if (!copy || n > 2 * BATCHPLAN_COLS || (n > BATCHPLAN_COLS && !groups_knob)) return p;
    p.feed[BP_QKV] = p.feed[BP_WO] = p.feed[BP_W2] = FEED_COLUMN;
    if (n <= BATCHPLAN_COLS) p.feed[BP_W13] = p.feed[BP_HEAD] = FEED_COLUMN;
    else p.groups = (n + BATCHPLAN_COLS - 1) / BATCHPLAN_COLS;
    return p;
}
// what the activation buffers of a step hold: 0 = B-operand columns, 1 = column groups, 2 = rows (lnb_forward_append_many re-zeroes
// them when this changes from one pass to the next)
static inline int batch_plan_layout(const BatchPlan& p) { return p.groups ? 1 : p.feed[BP_QKV] == FEED_COLUMN ? 0 : 2; }
