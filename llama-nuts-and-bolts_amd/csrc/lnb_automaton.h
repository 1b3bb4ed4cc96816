// lnb_automaton.h -- a token automaton in the sampling loops (include/lnb.h: lnb_ctx_set_automaton).  Included by lnb_kernels.hip behind the samplers
// and lnb_emit_probs.h.
//
// The caller's grammar engine compiles to a deterministic automaton over token ids: in state s the tokens of CSR row s are allowed, token t leads to
// next(s, t).  On the device it is a dense bitset mask[n_states][ceil(V / 32)], row_ptr and edge_next in token order (LnbDfaDev, lnb_device.h).  Pieces:
//   1. dfa_build_kernel: one workgroup per state zeroes its mask row and ORs one bit per edge into it, 32 bits at a time; on the way it checks what the
//      host cannot cheaply check (tokens strictly ascending inside a row, token < V, next < n_states) and reports the lowest offending edge.
//   2. sample_dfa_kernel<BATCH>: sample_rules_kernel / batch_sample_rules_kernel with step 0d.  The state's mask row (V / 8 bytes) is staged into the
//      LDS once, coalesced; sample_block's row load takes each group's byte from there (MASKED), so the logits row is still read once and a forbidden
//      entry is key 0 = -inf = no candidate.  The token then indexes the SAME LDS copy: every lane counts the set bits of its words below the token, one
//      workgroup reduction gives rank(t), and edge_next[row_ptr[state] + rank] is the next state -- no search over the edges.  A next state with an empty
//      row is final: the generation finishes as a stop id finishes it.  Token -1 and a finished generation leave the state word alone.
// A batch member without an automaton gets an all-ones mask in the same launch: its token is the rules kernel's, bit for bit.
// LDS: the mask row is a static array of LNB_SAMPLE_MAX_V / 8 = 16384 bytes BESIDE sample_block's own SampleSh (712 bytes, untouched) and the end struct
// (80 bytes): 17176 bytes per workgroup at V = 131072 and at every smaller V.  tools/isa_audit.py: 128 VGPRs, no scratch, no VGPR spill, 9 / 5 scalars
// parked in lanes (the other sample_block kernels park 4 .. 18).
// The speculative loop under an automaton (lnb_decode_speculative_automaton_until: the draft filter and the verify launch) is lnb_spec_automaton.h, its
// many-context form (lnb_decode_speculative_automaton_many) lnb_spec_automaton_many.h.
// Out of scope: the other speculative calls (the tree of drafts), the emitted-token records and pipeline ticks under an automaton, and any grammar compiler.
#pragma once

constexpr int LNB_DFA_MASK_WORDS = LNB_SAMPLE_MAX_V / 32;
static_assert(sizeof(SampleSh) <= 1024, "the LDS total stated above");

__global__ __launch_bounds__(256) void dfa_build_kernel(DfaBuildParams p) {
    const int s = blockIdx.x;
    uint32_t* row = p.mask + (size_t)s * p.words;
    for (int i = threadIdx.x; i < p.words; i += 256) row[i] = 0u;
    __syncthreads();                                         // (the row is this workgroup's alone: its zeroes are in front of its own ORs)
    const long long e0 = p.row_ptr[s], e1 = p.row_ptr[s + 1];
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
        const int t = p.edge_token[e], nx = p.edge_next[e];
        const bool bad = t < 0 || t >= p.V || nx < 0 || nx >= p.n_states || (e > e0 && p.edge_token[e - 1] >= t);
        if (bad) atomicMin(p.err, (unsigned long long)e);
        else atomicOr(row + (t >> 5), 1u << (t & 31));
    }
}

// What thread 0 needs after the row is sampled waits in the LDS meanwhile (see SampleEnd)
struct DfaEnd { SampleRulesEnd r; LnbDfaDev* dfa; int32_t* op_next; int state, tok; };

// the mask row of d's state into m (d nullptr: everything allowed); the words behind the row are zero, so that every group of the lane layout reads a defined byte
DEVINL void dfa_stage_mask(uint32_t* m, const LnbDfaDev* d, int state) {
    const int words = d ? d->words : 0;
    const uint32_t* row = d ? d->mask + (size_t)state * words : nullptr;
#pragma unroll
    for (int i = threadIdx.x; i < LNB_DFA_MASK_WORDS; i += 1024) m[i] = d ? (i < words ? row[i] : 0u) : 0xffffffffu;
    __syncthreads();
}
// the number of allowed tokens below tok (uniform, tok >= 0): every lane's four words of the LDS row, one reduction
DEVINL unsigned dfa_rank(const uint32_t* m, int tok, SampleSh& sh) {
    const int wt = tok >> 5;
    unsigned c = 0; unsigned long long w = 0;
#pragma unroll
    for (int i = threadIdx.x; i < LNB_DFA_MASK_WORDS; i += 1024) {
        const uint32_t v = i < wt ? m[i] : i == wt ? m[i] & ((1u << (tok & 31)) - 1u) : 0u;
        c += (unsigned)__popc(v);
    }
    int par = 0;
    sample_wg_sum(sh, par, c, w);
    return c;
}
template <bool BATCH>
LNB_NO_PK_F32 __global__ __launch_bounds__(1024) void sample_dfa_kernel(DfaTokParams p) {
    __shared__ SampleSh sh;
    __shared__ DfaEnd end;
    __shared__ uint32_t amask[LNB_DFA_MASK_WORDS];
    const bool adv = BATCH || p.advance != 0;
    const int row = BATCH || !p.advance ? (int)blockIdx.x : 0;
    const LnbSampler s = p.smp[row];
    const uint16_t* x = p.logits + (size_t)row * p.V;
    StepState* st = BATCH ? p.tab->st[row] : p.st;
    LnbDfaDev* d = BATCH ? p.member_dfa[row] : p.dfa;
    const int state = !d ? 0 : adv ? d->state : p.op_states[row];
    const bool has_u = !adv && p.op_draws != nullptr;
    const unsigned long long pos_or_u = adv ? (unsigned long long)(long long)st->pos : has_u ? p.op_draws[row] : (unsigned long long)(long long)p.op_pos[row];
    if (threadIdx.x == 0) {
        end.r.e.st = st; end.r.e.advance = adv;
        end.r.e.token_word = BATCH ? p.tab->dtok[row] : p.next_token + row;
        end.r.e.out_tokens = BATCH ? p.tab->dout[row] : p.out_tokens;
        end.r.e.out_cap = BATCH ? p.tab->dout_cap[row] : p.out_cap;
        end.r.e.info = !adv && p.op_info ? p.op_info + row : nullptr;
        end.r.counts = p.rules[row].counts;
        end.dfa = d; end.state = state; end.op_next = adv ? nullptr : p.op_next + row;
    }
    dfa_stage_mask(amask, d, state);
    const int t0 = sample_block<true, false, false, true>(x, p.V, p.etab, s, has_u, pos_or_u, sh, p.rules + row, nullptr, amask);
    if (threadIdx.x == 0) end.tok = t0;
    __syncthreads();                                         // (the token for every lane; sample_block's reductions are all behind it)
    const int tok = end.tok;
    unsigned rank = 0;
    if (end.dfa && tok >= 0) rank = dfa_rank(amask, tok, sh);       // (uniform: one path for the workgroup)
    if (threadIdx.x != 0) return;
    const DfaEnd e = end;
    if (e.r.e.info) *e.r.e.info = sh.z;
    const bool live = !e.r.e.advance || !e.r.e.st->finished;
    int ns = e.state;
    // (an emitted token is a candidate, so its bit is set and rank < the row's length; the test keeps a stray token from indexing the edges at all)
    const bool moved = e.dfa && live && tok >= 0 && ((amask[tok >> 5] >> (tok & 31)) & 1u);
    if (moved) ns = e.dfa->edge_next[e.dfa->row_ptr[e.state] + (long long)rank];
    if (!e.r.e.advance) { *e.r.e.token_word = tok; *e.op_next = ns; return; }
    sample_rules_advance(e.r, tok);
    if (moved) {
        e.dfa->state = ns;
        if (e.dfa->row_ptr[ns + 1] == e.dfa->row_ptr[ns]) e.r.e.st->finished = 1;     // a final state ends the generation as a stop id does: the token is out
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
extern "C" hipError_t lnbk_automaton_build(const DfaBuildParams* p, hipStream_t st) {
    if (p->n_states < 1 || p->V < 1 || p->V > LNB_SAMPLE_MAX_V || p->words != (p->V + 31) / 32 || !p->row_ptr || !p->edge_token || !p->edge_next || !p->mask || !p->err)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(dfa_build_kernel, dim3((unsigned)p->n_states), dim3(256), 0, st, *p);
    return hipGetLastError();
}
// rows of lnb_op_sample_automaton (p->advance 0) or the context's step (p->advance 1, rows 1)
extern "C" hipError_t lnbk_sample_automaton(const DfaTokParams* p, int rows, hipStream_t st) {
    if (p->V < 1 || p->V > LNB_SAMPLE_MAX_V || rows < 1 || (p->advance && rows != 1) || p->tab || !p->dfa || !p->smp || !p->rules ||
        (!p->advance && (!p->op_states || !p->op_next))) return hipErrorInvalidValue;
    form_ran(Form::SAMPLE_DFA_ROW);
    hipLaunchKernelGGL(sample_dfa_kernel<false>, dim3((unsigned)rows), dim3(1024), 0, st, *p);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_batch_sample_automaton(const DfaTokParams* p, int nseq, hipStream_t st) {
    if (p->V < 1 || p->V > LNB_SAMPLE_MAX_V || nseq < 1 || nseq > LNB_BATCH_MAX || !p->tab || !p->member_dfa || !p->smp || !p->rules) return hipErrorInvalidValue;
    form_ran(Form::SAMPLE_DFA_BATCH);
    hipLaunchKernelGGL(sample_dfa_kernel<true>, dim3((unsigned)nseq), dim3(1024), 0, st, *p);
    return hipGetLastError();
}
