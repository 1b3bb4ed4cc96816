// lnb_spec_automaton_many.h -- speculative decoding of many contexts under token automata (include/lnb.h: lnb_decode_speculative_automaton_many).  Included
// at the end of lnb_kernels.hip behind lnb_spec_many.h (SmPass's kernels, spec_many_accept_emit) and lnb_spec_automaton.h (dfa_filter_chain), whose pieces
// it joins: a pass is lnb_decode_speculative_many's pass, a member's columns are lnb_decode_speculative_automaton_until's columns.
//
// Member s holds the automaton view members[s].dfa (its state word s_0 governs the token behind its column 0) or none.  Two launches are new:
//   1. spec_many_dfa_draft_kernel: grid = members, behind spec_many_draft_kernel and in front of spec_many_pack_kernel on the pass's stream.  Workgroup s
//      runs dfa_filter_chain on member s's chain draft[s][0 .. want[s]): a forbidden token cuts in front of it, a final state behind it, forced tokens are
//      appended up to the smallest of max_draft, max_steps - n_out - 1 and seq_len - pos - 1 (want 0 extends as well) -> want[s], the draft tokens and
//      col_state[s][0 .. k].  A member without an automaton, not running or in a final state is left alone.  The grant rule then runs on the extended want;
//      a grant that cuts a forced run only leaves the row's tail unread, because col_state[s] is indexed by the member's own column.
//   2. spec_many_sample_dfa_commit_kernel: spec_many_sample_rules_commit_kernel with step 0d.  The workgroup of column c = column i of member mem stages the
//      mask row of col_state[mem][i] into the LDS and samples with the masked AND delta-patched row load (one read of the logits row); a member without an
//      automaton takes the unmasked instantiation and stages nothing (uniform over the workgroup).  n_c = next(state, g_c) comes from the workgroup's own
//      LDS copy of the row by dfa_rank; (g_c, n_c) are published in front of the release fence.  Thread s of the last workgroup through the ticket accepts,
//      emits and counts for member s (spec_many_accept_emit) and moves member s's state word to n_i for every emitted token; a stop id or a final n_i
//      finishes the member.  A rejected column leaves no trace in the state, the table or the log.
// LDS of the commit: the mask row 16384 bytes beside SampleSh (712), SpecDelta (64), the SmPass copy (160) and the end words (24): 17344 bytes per workgroup
// at every V.  The listing (tools/isa_audit.py): 121 VGPRs, scratch 0, no VGPR spill, 35 scalars parked in VGPR lanes -- two instantiations of sample_block
// share the kernel, and each parks its own loop-invariant scalars around its bisection loop (the one-instantiation kernels park 4 .. 18).  The draft kernel:
// 256 bytes of LDS, 37 VGPRs, nothing parked.
// Plain C++ and vector stores; no waits; members < p.n <= LNB_BATCH_MAX, columns < p.width <= LNB_BATCH_MAX, a member's column < LNB_SPEC_MAX_DRAFT + 1.
#pragma once

constexpr int LNB_SM_COLS = LNB_SPEC_MAX_DRAFT + 1;           // a member's row of SmPass::col_state

// ---- the draft filter of every member ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void spec_many_dfa_draft_kernel(SmPass p) {
    __shared__ DfaDraftSh sh;
    const int s = (int)blockIdx.x;
    if (s >= p.n || s >= LNB_BATCH_MAX) return;
    const SmMember& m = p.members[s];
    if (!m.active || !m.dfa || !p.running[s]) return;        // (uniform: the words are the same for every lane)
    const LnbDfaDev d = *m.dfa;
    int32_t* cs = p.col_state + s * LNB_SM_COLS;
    if (threadIdx.x == 0) cs[0] = d.state;
    if (dfa_final(d, d.state)) return;
    const int pos = m.st->pos, n_out = m.st->n_out;
    const int lim = min(min(m.max_draft, LNB_SPEC_MAX_DRAFT), min(p.max_steps - n_out - 1, m.seq_len - pos - 1));
    const int k = dfa_filter_chain(d, d.state, p.draft + s * LNB_SPEC_MAX_DRAFT, min(max(p.want[s], 0), LNB_SPEC_MAX_DRAFT), lim, cs, nullptr, pos, sh);
    if (threadIdx.x == 0) p.want[s] = k;
}

// ---- the verify pass's token launch -------------------------------------------------------------------------------------------------------------
// What the transition and the ticket need waits in the LDS across sample_block (SampleEnd, lnb_kernels.hip)
struct SmDfaEnd { LnbDfaDev* dfa; int state, tok, last, pad; };
LNB_NO_PK_F32 __global__ __launch_bounds__(1024) void spec_many_sample_dfa_commit_kernel(SmPass p) {
    __shared__ SampleSh sh;
    __shared__ SmPass end;
    __shared__ SmDfaEnd de;
    __shared__ SpecDelta dl;
    __shared__ uint32_t amask[LNB_DFA_MASK_WORDS];
    const int c = (int)blockIdx.x;
    const AmRow row = p.rows[c];
    const int mem = row.member >= 0 && row.member < LNB_BATCH_MAX ? row.member : 0;
    const LnbSampler s = p.smp[mem];
    const uint16_t* x = p.logits + (size_t)c * p.V;
    const double* etab = p.etab;
    const LnbRulesDev* rules = p.rules + mem;
    const int V = p.V;
    const unsigned long long pos = (unsigned long long)(long long)row.pos;
    const int first = p.seg[mem].first;
    const int nd = first < 0 || first > c ? 0 : min(c - first, LNB_SPEC_MAX_DRAFT);      // = the member's own column: its delta's length and its col_state index
    LnbDfaDev* const d = p.members[mem].dfa;
    const int state = d ? p.col_state[mem * LNB_SM_COLS + nd] : 0;
    if (threadIdx.x == 0) { end = p; dl.n = nd; de.dfa = d; de.state = state; de.last = 0; }
    if ((int)threadIdx.x < nd) dl.tok[threadIdx.x] = p.rows[first + 1 + (int)threadIdx.x].token;      // (first + nd <= c < the pass's width)
    int t0;
    if (d) {                                                 // (uniform: one path for the workgroup)
        dfa_stage_mask(amask, d, state);                     // (its closing barrier is the delta's as well)
        t0 = sample_block<true, true, false, true>(x, V, etab, s, false, pos, sh, rules, &dl, amask);
    } else {
        __syncthreads();
        t0 = sample_block<true, true>(x, V, etab, s, false, pos, sh, rules, &dl);
    }
    if (threadIdx.x == 0) de.tok = t0;
    __syncthreads();                                         // (the token for every lane; sample_block's reductions are all behind it)
    const int tok = de.tok;
    unsigned rank = 0;
    if (de.dfa && tok >= 0) rank = dfa_rank(amask, tok, sh);
    if (threadIdx.x == 0) {
        const SmDfaEnd e = de;
        int ns = e.state;
        // (an emitted token is a candidate, so its bit is set and rank < the row's length; the test keeps a stray token from indexing the edges at all)
        if (e.dfa && tok >= 0 && ((amask[tok >> 5] >> (tok & 31)) & 1u)) ns = e.dfa->edge_next[e.dfa->row_ptr[e.state] + (long long)rank];
        end.g[c] = tok; end.nst[c] = ns;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned t = __hip_atomic_fetch_add(end.cnt + LNB_BATCH_MAX, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        de.last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!de.last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x == 0) end.cnt[LNB_BATCH_MAX] = 0;        // (ready for the next launch: stream order)
    const int m = (int)threadIdx.x;
    spec_many_accept_emit(end, m, m < end.n && m < LNB_BATCH_MAX ? end.rules[m].counts : nullptr, end.nst);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
extern "C" hipError_t lnbk_spec_many_dfa_draft(const SmPass* p, hipStream_t st) {
    if (!spec_many_tables_ok(p) || !p->col_state) return hipErrorInvalidValue;
    form_ran(Form::DRAFT_DFA_MANY);
    hipLaunchKernelGGL(spec_many_dfa_draft_kernel, dim3((unsigned)p->n), dim3(1024), 0, st, *p);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_spec_many_sample_dfa_commit(const SmPass* p, hipStream_t st) {
    if (!spec_many_tables_ok(p) || !p->logits || p->V < 1 || p->V > LNB_SAMPLE_MAX_V || p->width < 1 || p->width > LNB_BATCH_MAX || !p->smp || !p->etab || !p->rules ||
        !p->col_state || !p->nst) return hipErrorInvalidValue;
    form_ran(Form::SAMPLE_SPEC_MANY_DFA);
    hipLaunchKernelGGL(spec_many_sample_dfa_commit_kernel, dim3((unsigned)p->width), dim3(1024), 0, st, *p);
    return hipGetLastError();
}
