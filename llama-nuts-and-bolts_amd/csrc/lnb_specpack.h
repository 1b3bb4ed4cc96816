// lnb_specpack.h -- how lnb_decode_speculative_many shares the columns of one pass between its members: plain C++ that includes nothing
// (spec_many_pack_kernel of lnb_spec_many.h calls it on the device; tests/native/specpack_test.cpp runs it on the host under the sanitizers).
//
// A = the members still running, in member order; want[s] = the draft length of member s (0 .. SPECPACK_MAX_WANT).  Every member of A gets one
// column (its current token).  The R = budget - |A| columns left are granted LEVEL BY LEVEL, so that a long draft never starves a short one:
//   for j = 1 .. SPECPACK_MAX_WANT, for s in A in member order: if want[s] >= j and R > 0, member s gets one more column.
// cols[s] = the columns of member s (0: not running); a member's columns are consecutive, members in member order, so its first column is the sum
// of the cols before it.  The caller guarantees budget >= |A| (the entry point refuses a budget below n).
#pragma once

#ifndef SPECPACK_FN
#define SPECPACK_FN static inline        // (the device build defines it with the host / device attributes before including this file)
#endif

#define SPECPACK_MAX_N 128               // LNB_BATCH_MAX of lnb_device.h: members of a call = columns of the widest pass
#define SPECPACK_MAX_WANT 15             // LNB_MAX_DRAFT of lnb.h

// -> the width of the pass (the sum of cols); -1: n outside 1..128, a want outside 0..15 or a budget that does not cover A or exceeds 128
SPECPACK_FN int specpack_grant(int n, const int* running, const int* want, int budget, int* cols) {
    if (n < 1 || n > SPECPACK_MAX_N || budget > SPECPACK_MAX_N) return -1;
    int width = 0;
    for (int s = 0; s < n; s++) {
        if (want[s] < 0 || want[s] > SPECPACK_MAX_WANT) return -1;
        cols[s] = running[s] ? 1 : 0;
        width += cols[s];
    }
    if (budget < width) return -1;
    int left = budget - width;
    for (int j = 1; j <= SPECPACK_MAX_WANT && left > 0; j++) {
        int granted = 0;
        for (int s = 0; s < n && left > 0; s++)
            if (running[s] && want[s] >= j) { cols[s]++; left--; granted++; }
        if (!granted) break;             // no member wants a level this deep: none wants a deeper one
    }
    return budget - left;
}
