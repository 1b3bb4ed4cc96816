// lnb_rowpack.h -- how lnb_forward_append_many packs the rows of its members into passes: pure host arithmetic, plain C++ without HIP
// (tests/native/rowpack_test.cpp runs exactly these functions under the sanitizers).
//
// Member s brings n_rows[s] rows.  The rows of all members, in member order, are the ROWS of the call (row index R, 64 bits: 128 members of
// 131072 rows each are 2^24 rows, and nothing here stops a caller from asking for more).  A PASS is one batched step of at most W columns:
// pass p takes the rows [p W, min((p + 1) W, total)), column c of it is row p W + c.  Inside a pass the rows of one member are one SEGMENT
// (member, first row within the member, count, first column); a member whose rows straddle a pass boundary has a segment in each pass, the
// later one starting where the earlier one ended.  Nothing is allocated: the walk hands out one pass at a time into the caller's array of W segments.
#pragma once
#include <stdint.h>

#define ROWPACK_MAX_W 128                // LNB_BATCH_MAX of lnb_device.h: the columns of a batched step

struct RowSeg { int32_t member, first, count, col; };     // rows [first, first + count) of `member` are the columns [col, col + count) of the pass

// rows of the call; -1: a null array, n < 1 or a member without rows
static inline int64_t rowpack_total(int n, const int32_t* n_rows) {
    if (!n_rows || n < 1) return -1;
    int64_t t = 0;
    for (int s = 0; s < n; s++) { if (n_rows[s] < 1) return -1; t += (int64_t)n_rows[s]; }
    return t;
}
// passes of W columns that `total` rows take
static inline int64_t rowpack_passes(int64_t total, int W) { return W < 1 || total < 0 ? -1 : (total + W - 1) / W; }
// width of pass p
static inline int rowpack_width(int64_t total, int W, int64_t p) { const int64_t left = total - p * (int64_t)W; return (int)(left < W ? left : W); }

// the walk: member / row = where the next pass starts, done = rows handed out so far (= the call's index of the next pass's first row)
struct RowPackWalk { int n; const int32_t* n_rows; int W; int member; int32_t row; int64_t done; };
static inline int rowpack_begin(RowPackWalk* w, int n, const int32_t* n_rows, int W) {
    if (rowpack_total(n, n_rows) < 0 || W < 1 || W > ROWPACK_MAX_W) return -1;
    w->n = n; w->n_rows = n_rows; w->W = W; w->member = 0; w->row = 0; w->done = 0;
    return 0;
}
// the next pass: its segments into segs[0 .. W) -> number of segments (0: the walk is over), *width = its columns, *row0 = the call's index of its column 0
static inline int rowpack_next(RowPackWalk* w, RowSeg* segs, int* width, int64_t* row0) {
    int col = 0, ns = 0;
    *row0 = w->done;
    while (col < w->W && w->member < w->n) {
        const int32_t left = w->n_rows[w->member] - w->row, room = (int32_t)(w->W - col), take = left < room ? left : room;
        segs[ns].member = w->member; segs[ns].first = w->row; segs[ns].count = take; segs[ns].col = col; ns++;
        col += take; w->row += take;
        if (w->row == w->n_rows[w->member]) { w->member++; w->row = 0; }
    }
    w->done += col; *width = col;
    return ns;
}
// position of the row in column c of a segment: its member starts at start_pos
static inline int64_t rowpack_pos(const RowSeg* g, int c, int32_t start_pos) { return (int64_t)start_pos + g->first + (c - g->col); }
