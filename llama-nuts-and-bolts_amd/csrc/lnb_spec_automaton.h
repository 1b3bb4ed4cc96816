// lnb_spec_automaton.h -- speculative decoding under a token automaton (include/lnb.h: lnb_decode_speculative_automaton_until).  Included by lnb_kernels.hip
// behind lnb_automaton.h, whose mask row, dfa_stage_mask and dfa_rank it uses.
//
// A verify pass at position pos carries d_0 .. d_{w-1} (d_0 = the current token); the context's state word s_0 governs the token behind d_0.  Column i is the
// automaton step at pos + i in state s_i = next(s_{i-1}, d_i) with the rules counts c_j(i) of spec_sample_rules_commit_kernel.  Pieces:
//   1. dfa_draft_kernel: ONE workgroup on the context's stream behind ngram_draft_kernel and in front of the event the host waits on.
//      Walk: for i = 1 .. k, a d_i outside the row of s_{i-1} cuts the draft to i - 1 (a forbidden guess never takes a column); otherwise
//      s_i = edge_next[row_ptr[s_{i-1}] + rank(d_i)], the rank a workgroup popcount over the row's words below the token (dfa_rank's arithmetic on the row in
//      global memory: V / 8 bytes, at most four words per lane); a final s_i cuts to i.
//      Extend: while the row of s_k holds exactly ONE token t, s_k is not final and k is below max_draft, max_steps - n_out - 1 and seq_len - pos - 1:
//      d_{k+1} = t, s_{k+1} = edge_next[row_ptr[s_k]].  t comes from the mask row itself -- the one lane with a non-zero word, by ballot, and that word's
//      lowest bit -- because edge_token is not kept for the step kernels.  This runs for k = 0 as well: a forced run needs no n-gram match.
//      Write: the extended columns' token words and positions as ngram_draft_kernel writes them, col_state[0 .. k], and {k, n_out, finished} for the host.
//      A finished generation and a state that is already final are left alone (k as found, col_state[0] = the state).
//   2. spec_sample_dfa_commit_kernel: spec_sample_rules_commit_kernel with step 0d.  Workgroup i stages the mask row of col_state[i] into the LDS, samples with
//      the masked AND delta-patched row load (sample_block<RULES, DELTA, -, MASKED>: the logits row is still read once), computes n_i = next(s_i, g_i) from its
//      own LDS copy of the row (g_i == -1: n_i = s_i) and publishes (g_i, n_i) in front of its release fence.  The last workgroup through the ticket accepts and
//      emits (spec_accept_emit with the states): every emitted token is counted, moves the state word to its n_i, and a stop id or a final n_i finishes the
//      run.  It needs no mask row for that.  A rejected column leaves no trace in the state, the table or the log.  All-off rules are the plain sampler bit for
//      bit, so the one kernel serves both.
// LDS of spec_sample_dfa_commit_kernel: the mask row 16384 bytes beside SampleSh (712), SpecDelta (64) and the end struct (64): 17224 bytes per workgroup at
// every V.  The listing (tools/isa_audit.py): 128 VGPRs, scratch 0, no VGPR spill, 17 scalars parked in VGPR lanes around the bisection loop (the other
// sample_block kernels park 4 .. 18; the kernel is listed there for that).  dfa_draft_kernel: 256 bytes of LDS, 38 VGPRs, nothing parked.
#pragma once

// ---- the draft filter ------------------------------------------------------------------------------------------------------------------------
struct DfaDraftSh { unsigned c[2][16]; int t[2][16]; };
// the number of set bits of `row` below bit `lim` (uniform; lim = words * 32: the whole row) and, in *one, a set bit's index -- THE set bit where the count is 1
DEVINL unsigned dfa_row_count(const uint32_t* row, int words, int lim, DfaDraftSh& sh, int& par, int* one) {
    const int wl = lim >> 5;
    unsigned c = 0; int mine = -1;
    for (int i = threadIdx.x; i < words; i += 1024) {
        const uint32_t v = i < wl ? row[i] : i == wl ? row[i] & ((1u << (lim & 31)) - 1u) : 0u;
        c += (unsigned)__popc(v);
        if (v != 0u && mine < 0) mine = i * 32 + __ffs((int)v) - 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    const unsigned long long has = __ballot(mine >= 0);
    const int t = has ? __shfl(mine, __ffsll((long long)has) - 1) : -1;
    if ((threadIdx.x & 63) == 0) { sh.c[par][threadIdx.x >> 6] = c; sh.t[par][threadIdx.x >> 6] = t; }
    __syncthreads();                                         // (two slots, as sample_wg_sum's: the next count writes the other one)
    c = 0; int tt = -1;
#pragma unroll
    for (int i = 0; i < 16; i++) { c += sh.c[par][i]; tt = sh.t[par][i] > tt ? sh.t[par][i] : tt; }
    par ^= 1;
    *one = tt;
    return c;
}
DEVINL bool dfa_final(const LnbDfaDev& d, int q) { return d.row_ptr[q + 1] == d.row_ptr[q]; }
// Walk and extend, one rule for dfa_draft_kernel and spec_many_dfa_draft_kernel (lnb_spec_automaton_many.h): the chain d_1 .. d_k (d_i = tok1[i - 1]) from
// the non-final state s, extended up to lim tokens -> the k behind the filter; thread 0 writes the forced tokens, col_state[1 .. k] and, with col_st, the
// extended columns' positions pos + i.  Uniform: every lane reads the same words.
DEVINL int dfa_filter_chain(const LnbDfaDev& d, int s, int32_t* tok1, int k, int lim, int32_t* col_state, StepState* col_st, int pos, DfaDraftSh& sh) {
    const bool t0 = threadIdx.x == 0;
    int par = 0, one = -1, kept = 0;
    for (int i = 1; i <= k; i++) {
        const int t = tok1[i - 1];
        const uint32_t* row = d.mask + (size_t)s * d.words;
        if ((unsigned)t >= (unsigned)d.words * 32u || !((row[t >> 5] >> (t & 31)) & 1u)) break;      // (the bits behind V are zero: dfa_build_kernel)
        const unsigned rank = dfa_row_count(row, d.words, t, sh, par, &one);
        s = d.edge_next[d.row_ptr[s] + (long long)rank];
        kept = i;
        if (t0) col_state[i] = s;
        if (dfa_final(d, s)) break;
    }
    k = kept;
    while (k < lim && !dfa_final(d, s)) {
        if (dfa_row_count(d.mask + (size_t)s * d.words, d.words, d.words * 32, sh, par, &one) != 1u) break;
        s = d.edge_next[d.row_ptr[s]];
        k++;
        if (t0) {
            tok1[k - 1] = one; col_state[k] = s;
            if (col_st) col_st[k].pos = pos + k;
        }
    }
    return k;
}
__global__ __launch_bounds__(1024) void dfa_draft_kernel(DfaDraftParams p) {
    __shared__ DfaDraftSh sh;
    const LnbDfaDev d = *p.dfa;
    const bool t0 = threadIdx.x == 0;
    int k = p.word_in[0];
    const int n_out = p.word_in[1], fin = p.word_in[2];
    if (t0) p.col_state[0] = d.state;
    if (!fin && !dfa_final(d, d.state)) {
        const int pos = p.st ? p.st->pos : 0;
        int lim = p.max_draft < LNB_SPEC_MAX_DRAFT ? p.max_draft : LNB_SPEC_MAX_DRAFT;
        if (p.st) lim = min(lim, min(p.max_steps - n_out - 1, p.seq_len - pos - 1));
        k = dfa_filter_chain(d, d.state, p.tok + 1, k, lim, p.col_state, p.col_st, pos, sh);
    }
    if (t0) { p.word[0] = k; p.word[1] = n_out; p.word[2] = fin; }
}

// ---- the verify pass's token launch -------------------------------------------------------------------------------------------------------------
struct SpecDfaEnd { SpecSampleRulesEnd r; LnbDfaDev* dfa; int32_t* nst; int state, tok; };
LNB_NO_PK_F32 __global__ __launch_bounds__(1024) void spec_sample_dfa_commit_kernel(SpecDfaParams p) {
    __shared__ SampleSh sh;
    __shared__ SpecDfaEnd end;
    __shared__ SpecDelta dl;
    __shared__ uint32_t amask[LNB_DFA_MASK_WORDS];
    const int i = blockIdx.x;
    const LnbSampler s = p.smp[0];
    const uint16_t* x = p.logits + (size_t)i * p.V;
    const unsigned long long pos = (unsigned long long)(long long)p.tab->st[i]->pos;
    const int nd = i < LNB_SPEC_MAX_DRAFT ? i : LNB_SPEC_MAX_DRAFT;
    const int state = p.col_state[i];
    if (threadIdx.x == 0) {
        end.r.e.g = p.g; end.r.e.cnt = p.cnt; end.r.e.tab = p.tab; end.r.e.w = (int)gridDim.x; end.r.e.last = 0; end.r.counts = p.rules->counts; dl.n = nd;
        end.dfa = p.dfa; end.nst = p.nst; end.state = state;
    }
    if ((int)threadIdx.x < nd) dl.tok[threadIdx.x] = *p.tab->dtok[threadIdx.x + 1];    // d_1 .. d_i: the inputs of columns 1 .. i
    dfa_stage_mask(amask, p.dfa, state);                     // (its closing barrier is the delta's as well)
    const int t0 = sample_block<true, true, false, true>(x, p.V, p.etab, s, false, pos, sh, p.rules, &dl, amask);
    if (threadIdx.x == 0) end.tok = t0;
    __syncthreads();                                         // (the token for every lane; sample_block's reductions are all behind it)
    const int tok = end.tok;
    unsigned rank = 0;
    if (tok >= 0) rank = dfa_rank(amask, tok, sh);           // (uniform: one path for the workgroup)
    if (threadIdx.x != 0) return;
    const SpecDfaEnd e = end;
    int ns = e.state;
    if (tok >= 0 && ((amask[tok >> 5] >> (tok & 31)) & 1u)) ns = e.dfa->edge_next[e.dfa->row_ptr[e.state] + (long long)rank];
    e.r.e.g[i] = tok; e.nst[i] = ns;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const unsigned t = __hip_atomic_fetch_add(e.r.e.cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (t != (unsigned)e.r.e.w - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    *e.r.e.cnt = 0;                                          // (ready for the next launch: stream order)
    spec_accept_emit(e.r.e.g, e.r.e.w, e.r.e.tab, e.r.counts, e.nst, e.dfa);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
extern "C" hipError_t lnbk_automaton_draft(const DfaDraftParams* p, hipStream_t st) {
    if (!p->dfa || !p->tok || !p->word_in || !p->word || !p->col_state || p->max_draft < 0 || p->max_draft > LNB_SPEC_MAX_DRAFT) return hipErrorInvalidValue;
    form_ran(Form::DRAFT_DFA);
    hipLaunchKernelGGL(dfa_draft_kernel, dim3(1), dim3(1024), 0, st, *p);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_spec_sample_automaton_commit(const SpecDfaParams* p, int w, hipStream_t st) {
    if (p->V < 1 || p->V > LNB_SAMPLE_MAX_V || w < 1 || w > LNB_SPEC_MAX_DRAFT + 1 || !p->logits || !p->etab || !p->smp || !p->rules || !p->g || !p->nst || !p->tab ||
        !p->cnt || !p->dfa || !p->col_state) return hipErrorInvalidValue;
    form_ran(Form::SAMPLE_SPEC_DFA);
    hipLaunchKernelGGL(spec_sample_dfa_commit_kernel, dim3((unsigned)w), dim3(1024), 0, st, *p);
    return hipGetLastError();
}
