// lnb_spec_many.h -- the three table kernels of lnb_decode_speculative_many (include/lnb.h).  Included at the end of lnb_kernels.hip, behind
// lnb_append_many.h (argmax_block, ngram_search_block and ngram_pick live in lnb_kernels.hip).
//
// The call decodes up to 128 contexts together, every member drafting for itself by n-gram lookup.  A pass is a pass of lnb_forward_append_many
// (append_many_setup_kernel + the batched step): its columns are consecutive rows of several members, column i of a member the one-token step at
// pos + i.  What these kernels add is the work around it, all of it on the device (SmMember / SmPass: lnb_device.h):
//   spec_many_draft_kernel    grid (n-gram lengths, members): workgroup (b, s) runs ngram_draft_kernel's search of n = ngram_max_s - b for member s
//                             (the same function body); the last workgroup of a member to arrive (agent-scope ticket, no poll) picks the match and
//                             writes want[s], the draft tokens and running[s].  A member that never drafts (max_draft 0) searches nothing.
//   spec_many_pack_kernel     one workgroup: the grant rule (specpack_grant, lnb_specpack.h), then thread s writes member s's rows of the pass's
//                             AmRow table (column 0 = its token word at its position, column i = draft token i - 1 at pos + i), its {first, cols},
//                             its counters, and thread 0 the pinned block {width, any_draft, running, largest seq_len} the host reads per pass.
//   spec_many_commit_kernel   one workgroup per column: ml.Argmax of the column (argmax_block); the last workgroup to arrive (ticket) lets thread s
//                             accept for member s -- a_s = the longest prefix of its columns whose argmax equals the next column's input -- and
//                             emit the argmax of its columns 0 .. a_s into the member's OWN state, token word and log, as spec_commit_kernel does.
//   spec_many_sample_commit_kernel   the same with every member's own sampler (lnb_decode_speculative_sample_many): column c's token is the sampler's of
//                             its member at the column's own position; acceptance and emission are the same function (spec_many_accept_emit).
// Plain C++ and vector stores; no waits; every index is bounded by the tables' own sizes (members < p.n <= LNB_BATCH_MAX, columns < LNB_BATCH_MAX,
// draft tokens < LNB_SPEC_MAX_DRAFT, n-gram results < LNB_SPEC_MAX_NGRAM).
#pragma once

#define SPECPACK_FN __host__ __device__ static inline
#include "lnb_specpack.h"

DEVINL DraftParams spec_many_draft_params(const SmPass& p, int s) {
    const SmMember& m = p.members[s];
    DraftParams d{};
    d.text = m.text; d.n_text = m.n_text; d.gen = m.log; d.st = m.st; d.corpus = m.corpus; d.n_corpus = m.n_corpus;
    d.ngram_min = m.ngram_min; d.ngram_max = m.ngram_max; d.max_draft = min(m.max_draft, LNB_SPEC_MAX_DRAFT);
    d.max_steps = p.max_steps; d.seq_len = m.seq_len;
    d.best = p.best + (size_t)s * 2 * LNB_SPEC_MAX_NGRAM; d.cnt = p.cnt + s;
    return d;
}
__global__ __launch_bounds__(256) void spec_many_draft_kernel(SmPass p) {
    __shared__ int32_t suf[LNB_SPEC_MAX_NGRAM];
    __shared__ int sbest[2];
    __shared__ int s_last;
    const int tid = threadIdx.x, b = blockIdx.x, s = blockIdx.y;
    if (s >= p.n || s >= LNB_BATCH_MAX) return;
    const SmMember& m = p.members[s];
    const DraftParams d = spec_many_draft_params(p, s);
    const bool running = m.active && !m.st->finished && m.st->n_out < p.max_steps;
    const int levels = min(m.ngram_max - m.ngram_min + 1, LNB_SPEC_MAX_NGRAM);
    const bool drafts = running && m.max_draft > 0;          // (uniform over the workgroup)
    const int n_gen = drafts ? m.st->n_out : 0, L = m.n_text + n_gen;
    const bool mine = drafts && b < levels;
    if (mine) ngram_search_block(d, m.ngram_max - b, L, suf, sbest);
    if (tid == 0) {
        if (mine) { d.best[2 * b] = sbest[0]; d.best[2 * b + 1] = sbest[1]; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned t = __hip_atomic_fetch_add(d.cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last || tid != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    *d.cnt = 0;                                              // (ready for the next launch: stream order)
    int src = -1, start = 0;
    const int k = drafts ? ngram_pick(d, min(levels, (int)gridDim.x), L, n_gen, &src, &start) : 0;
    for (int i = 0; i < k && i < LNB_SPEC_MAX_DRAFT; i++) p.draft[s * LNB_SPEC_MAX_DRAFT + i] = src == 0 ? spec_text_at(d, start + i) : d.corpus[start + i];
    p.want[s] = k;
    p.running[s] = running ? 1 : 0;
}

__global__ __launch_bounds__(LNB_BATCH_MAX) void spec_many_pack_kernel(SmPass p) {
    __shared__ int cols[LNB_BATCH_MAX];
    __shared__ int first[LNB_BATCH_MAX];
    __shared__ int s_width;
    const int s = (int)threadIdx.x, n = min(p.n, LNB_BATCH_MAX);
    if (s == 0) {
        int w = specpack_grant(n, p.running, p.want, p.budget, cols);
        if (w > LNB_BATCH_MAX) w = -1;
        int any = 0, run = 0, maxT = 0;
        for (int i = 0; i < n; i++) if (p.running[i]) { run++; maxT = max(maxT, p.members[i].seq_len); }     // (counted apart from the grant: a refused grant is reported as width -1 with members running)
        if (w >= 0) {
            int c = 0;
            for (int i = 0; i < n; i++) {
                first[i] = c; c += cols[i];
                if (cols[i] > 1) any = 1;
            }
        }
        s_width = w;
        p.word[0] = w; p.word[1] = any; p.word[2] = run; p.word[3] = maxT;
    }
    __syncthreads();
    if (s >= n) return;
    const int w = s_width;
    const int k = w < 0 ? 0 : cols[s], f = w < 0 ? 0 : first[s];
    p.seg[s] = SmSeg{f, k};
    if (k == 0 || f + k > LNB_BATCH_MAX) return;
    const SmMember& m = p.members[s];
    const int pos = m.st->pos;
    for (int i = 0; i < k; i++) {
        const int32_t tok = i == 0 ? *m.tok : p.draft[s * LNB_SPEC_MAX_DRAFT + min(i - 1, LNB_SPEC_MAX_DRAFT - 1)];
        p.rows[f + i] = AmRow{s, pos + i, tok, i == k - 1 ? 1 : 0};
    }
    SmStats& t = p.stats[s];
    t.passes += 1; t.verify_passes += k > 1 ? 1 : 0; t.drafted += k - 1;
}

// what the last workgroup's thread s does for member s (shared by spec_many_commit_kernel and spec_many_sample_commit_kernel: p.g holds the columns'
// argmax or the samplers' tokens, the loop is the same)
DEVINL void spec_many_accept_emit(const SmPass& p, int s) {
    if (s >= p.n || s >= LNB_BATCH_MAX) return;
    const SmSeg sg = p.seg[s];
    if (sg.cols <= 0 || sg.first < 0 || sg.first + sg.cols > p.width || p.width > LNB_BATCH_MAX) return;
    const SmMember& m = p.members[s];
    StepState* st = m.st;
    if (st->finished) return;
    int a = 0;
    while (a < sg.cols - 1 && p.g[sg.first + a] == p.rows[sg.first + a + 1].token) a++;
    for (int i = 0; i <= a; i++) {                           // exactly spec_commit_kernel's emission
        const int t = p.g[sg.first + i];
        const int no = st->n_out;
        if (no < m.log_cap) m.log[no] = t;
        st->n_out = no + 1;
        st->pos = st->pos + 1;
        *m.tok = t;
        bool stop = false;
        if (st->honour_stop) for (int q = 0; q < st->n_stop; q++) if (t == st->stop[q]) stop = true;
        if (stop) { st->finished = 1; break; }
    }
}

__global__ __launch_bounds__(1024) void spec_many_commit_kernel(SmPass p) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    __shared__ int s_last;
    const int c = (int)blockIdx.x;
    const int tok = argmax_block(p.logits + (size_t)c * p.V, p.V, sv, si);
    if (threadIdx.x == 0) {
        p.g[c] = tok;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned t = __hip_atomic_fetch_add(p.cnt + LNB_BATCH_MAX, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x == 0) p.cnt[LNB_BATCH_MAX] = 0;          // (ready for the next launch: stream order)
    spec_many_accept_emit(p, (int)threadIdx.x);
}

// spec_many_commit_kernel with every member's own sampler (lnb_decode_speculative_sample_many): column c is the one-token step of member rows[c].member at
// rows[c].pos, so its token is that member's sampler's at THAT position (a temperature-0 member: argmax_block).  The pass's tables wait in the LDS across
// sample_block, which leaves no scalar registers to hold them (SampleEnd, lnb_kernels.hip).
__global__ __launch_bounds__(1024) void spec_many_sample_commit_kernel(SmPass p) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    __shared__ SampleSh sh;
    __shared__ SmPass end;
    __shared__ int s_last;
    const int c = (int)blockIdx.x;
    const AmRow row = p.rows[c];
    const int mem = row.member >= 0 && row.member < LNB_BATCH_MAX ? row.member : 0;
    const LnbSampler s = p.smp[mem];
    const uint16_t* x = p.logits + (size_t)c * p.V;
    const double* etab = p.etab;
    const int V = p.V;
    const unsigned long long pos = (unsigned long long)(long long)row.pos;
    if (threadIdx.x == 0) { end = p; s_last = 0; }
    const int tok = s.temperature == 0.0f ? argmax_block(x, V, sv, si) : sample_block(x, V, etab, s, false, pos, sh);
    if (threadIdx.x == 0) {
        end.g[c] = tok;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned t = __hip_atomic_fetch_add(end.cnt + LNB_BATCH_MAX, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x == 0) end.cnt[LNB_BATCH_MAX] = 0;        // (ready for the next launch: stream order)
    spec_many_accept_emit(end, (int)threadIdx.x);
}
