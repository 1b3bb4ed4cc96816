// lnb_append_many.h -- the two table kernels of lnb_forward_append_many (include/lnb.h).  Included at the end of lnb_kernels.hip (argmax_block lives there).
//
// The call appends n_rows[s] rows to each of up to 128 contexts.  Its arithmetic is the batched step's (lnb_batch_kernels.h): a pass of `width`
// columns, each column the one-token step of ONE row -- its own position, token word and KV caches, taken from the device tables BatchTab / BatchKV.
// What changes from pass to pass is only which rows the columns are, so the host uploads the whole call ONCE (AmRow per row, AmMembers + a BatchKV
// per layer indexed by member: lnb_device.h) and these kernels do the per-pass work on the device:
//   append_many_setup_kernel    one launch per pass: column c <- row row0 + c.  Workgroup 0 writes the column states (position, nothing else set:
//                               no stop ids, not finished), the token words, the columns' cache lengths and the width; workgroup 1 + l copies the
//                               members' cache pointers of layer l into the columns of that layer's BatchKV.  A column past the width gets column
//                               0's member: the batched kernels never read it, and it is never null or stale from an earlier call.
//   append_many_finish_kernel   one launch per pass, one workgroup per column: ml.Argmax (argmax_block: first maximum wins) of the columns that are
//                               a member's LAST row, into out[member]; every other workgroup leaves at once.  Nothing of any context is written.
// Plain C++ and vector stores; every index is bounded by the tables' own sizes (c < LNB_BATCH_MAX threads, member < members->n <= LNB_BATCH_MAX).
#pragma once

__global__ __launch_bounds__(LNB_BATCH_MAX) void append_many_setup_kernel(AmPass p) {
    const int c = (int)threadIdx.x;
    const AmRow r = p.rows[c < p.width ? c : 0];
    const int mbr = r.member >= 0 && r.member < p.members->n ? r.member : 0;       // (the host built the table: cannot happen)
    if (blockIdx.x == 0) {
        p.tab->seq_len[c] = p.members->seq_len[mbr];
        if (c == 0) p.tab->n = p.width;
        if (c < p.width) {
            StepState* st = p.st + c;
            st->pos = r.pos; st->n_out = 0; st->finished = 0; st->n_stop = 0; st->honour_stop = 0;
            p.tok[c] = r.token;
        }
        return;
    }
    const int l = (int)blockIdx.x - 1;
    if (l >= p.n_layers) return;
    p.kv[l].ck[c] = p.member_kv[l].ck[mbr];
    p.kv[l].cv[c] = p.member_kv[l].cv[mbr];
}

__global__ __launch_bounds__(1024) void append_many_finish_kernel(const uint16_t* logits, int V, const AmRow* rows, int32_t* out) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    const AmRow r = rows[blockIdx.x];
    if (!r.last) return;                                     // (uniform over the workgroup)
    const int tok = argmax_block(logits + (size_t)blockIdx.x * V, V, sv, si);
    if (threadIdx.x == 0) out[r.member] = tok;
}
