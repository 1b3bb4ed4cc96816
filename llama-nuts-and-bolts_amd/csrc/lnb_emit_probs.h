// lnb_emit_probs.h -- the emitted token's record in the sampling and speculative loops (include/lnb.h: lnb_ctx_set_emitted_probs).  Included by
// lnb_kernels.hip behind the samplers, token_probs_kernel and the launch tally.
//
// A record = the raw logits row's top k (token_probs_kernel's, entry 0 = the row's argmax) + the token the step EMITTED: its logit, f32(e_t / Z) with the
// reference's serial Z, ln Z, and the sampler's own exact probability of it as the integer fraction w_tok / w_kept.  Three pieces:
//   1. the row summary launch = token_probs_kernel<KT, PARK>: the same 64 sub-slice sum order, per-lane lists and last-workgroup merge, so a row's estimate
//      and whether it walks are those of every other launch shape.  It runs BEFORE the token launch and cannot know the token: it writes the top k into the
//      record slot (a verify pass: blockIdx.y = column, into a pass scratch of w records) and PARKS the row's Z state (EmitPark) for the token launch.
//   2. emit_entry: called by ONE wave at the end of the token launch, after the token is known and before the state advances -- one table lookup for e_t,
//      cert_p32 against the parked estimate, and tp_zseq_wave only where this quotient is not settled and the row has not walked yet.
//   3. the verify pass's commit: the last workgroup through the ticket accepts and emits as spec_accept_emit does, then the same wave runs emit_entry per
//      EMITTED column against that column's parked Z and copies its top k from the pass scratch to the log slots in emission order; a rejected column
//      leaves no trace, a stop token ends the copy behind itself (n_out stops there).  Vector loads and stores only.
// The token launches are instantiations of their own (emit_sample_kernel, emit_spec_commit_kernel): sample_kernel and its kin are compiled as before.
#pragma once

// -> slot `slot` of L: tok_logit, tok_prob, ln Z (corrected when this entry walks) and the two weights.  All 64 lanes of one wave, uniform arguments.
DEVINL void emit_entry(const uint16_t* x, int V, const double* etab, const EmitPark* park, int tok, unsigned long long w_tok, unsigned long long w_kept,
                       const EmitLog& L, int slot) {
    const int lane = threadIdx.x & 63;
    const EmitPark k = *park;
    const float qnan = __uint_as_float(0x7FC00000u);
    float lg = qnan, pr = qnan;
    double z = k.z;                                          // (the estimate itself for a row that has not walked)
    if (tok >= 0) {                                          // (tok < V: an index of the row; -1: an all-NaN or candidate-less row)
        const uint16_t b = x[tok];
        const double e = etab[b];
        lg = bf_wide(b);
        if (k.walked) pr = (float)(e / k.z);
        else {                                               // (not walked: zt > 0 and its band is finite -- the summary launch has checked both)
            const CertZ cz = cert_z(k.zt, V);
            int bad = 0;
            pr = cert_p32(e, cz, bad);
            if (bad) {                                       // this one quotient sits in the band: the reference's serial sum, as the summary launch would walk it
                z = tp_zseq_wave(x, V, etab);
                pr = (float)(e / z);
                if (lane == 0 && L.walks) atomicAdd(L.walks, 1);
            }
        }
    } else { w_tok = 0; w_kept = 0; }
    if (lane == 0) {
        L.tok_logit[slot] = lg; L.tok_prob[slot] = pr; L.log_z[slot] = log(z);
        L.w[2 * (size_t)slot] = w_tok; L.w[2 * (size_t)slot + 1] = w_kept;
    }
}

// What wave 0 needs AFTER the row is sampled waits in the LDS meanwhile (see SampleEnd)
struct EmitEnd {
    StepState* st; int32_t* token_word; int32_t* out_tokens; uint32_t* counts;
    const uint16_t* x; const double* etab; const EmitPark* park; const EmitLog* log;
    int out_cap, adv, V, sampled;
};
// sample_kernel / sample_rules_kernel (RULES) and their batch forms (BATCH: block q = member q) with the emitted entry.  advance == 0: block i = row i of
// lnb_op_emitted_probs, record slot i.  Temperature 0 without rules = argmax_block on the raw row, both weights 0.
template <bool RULES, bool BATCH>
LNB_NO_PK_F32 __global__ __launch_bounds__(1024) void emit_sample_kernel(EmitTokParams p) {
    __shared__ float sv[RULES ? 1 : 1024];
    __shared__ int si[RULES ? 1 : 1024];
    __shared__ SampleSh sh;
    __shared__ EmitEnd end;
    const bool adv = BATCH || p.advance != 0;
    const int row = BATCH || !p.advance ? (int)blockIdx.x : 0;
    const LnbSampler s = p.smp[row];
    const uint16_t* x = p.logits + (size_t)row * p.V;
    StepState* st = BATCH ? p.tab->st[row] : p.st;
    const bool has_u = !adv && p.op_draws != nullptr;
    const unsigned long long pos_or_u = adv ? (unsigned long long)(long long)st->pos : has_u ? p.op_draws[row] : (unsigned long long)(long long)p.op_pos[row];
    if (threadIdx.x == 0) {
        end.st = st; end.adv = adv; end.V = p.V; end.x = x; end.etab = p.etab;
        end.token_word = BATCH ? p.tab->dtok[row] : p.next_token + row;
        end.out_tokens = BATCH ? p.tab->dout[row] : p.out_tokens;
        end.out_cap = BATCH ? p.tab->dout_cap[row] : p.out_cap;
        end.counts = RULES ? p.rules[row].counts : nullptr;
        end.park = p.park + row; end.log = p.log + (p.per_row_log ? row : 0);
        end.sampled = RULES || s.temperature != 0.0f;
    }
    int tok;
    if constexpr (RULES) tok = sample_block<true, false, true>(x, p.V, p.etab, s, has_u, pos_or_u, sh, p.rules + row);
    else tok = s.temperature == 0.0f ? argmax_block(x, p.V, sv, si) : sample_block<false, false, true>(x, p.V, p.etab, s, has_u, pos_or_u, sh);
    if (threadIdx.x >= 64) return;                           // (behind the last barrier of either path: tok, sh and end are the workgroup's)
    const EmitEnd e = end;
    const EmitLog L = *e.log;
    int slot = (int)blockIdx.x;
    bool rec = true;
    if (e.adv) { slot = e.st->n_out; rec = !e.st->finished && slot < L.cap; }       // (what the summary launch saw: the state moves below)
    if (rec) emit_entry(e.x, e.V, e.etab, e.park, tok, e.sampled ? sh.w_tok : 0ull, e.sampled ? sh.z.w_kept : 0ull, L, slot);
    if (threadIdx.x != 0) return;
    if (!e.adv) { *e.token_word = tok; return; }
    if (RULES && !e.st->finished && tok >= 0) e.counts[tok] += 1u;                  // (sample_rules_advance)
    step_advance(e.st, tok, e.token_word, nullptr, e.out_tokens, e.out_cap);
}

// spec_sample_commit_kernel / spec_sample_rules_commit_kernel (RULES) with records.  Every column workgroup leaves its token and the token's two weights;
// wave 0 of the last one through the ticket emits, then records column c < (tokens emitted) into slot n_out + c.
struct EmitSpecEnd { EmitSpecParams p; int w, sampled; };
template <bool RULES>
LNB_NO_PK_F32 __global__ __launch_bounds__(1024) void emit_spec_commit_kernel(EmitSpecParams p) {
    __shared__ float sv[RULES ? 1 : 1024];
    __shared__ int si[RULES ? 1 : 1024];
    __shared__ SampleSh sh;
    __shared__ EmitSpecEnd end;
    __shared__ SpecDelta dl;
    const int i = blockIdx.x;
    const LnbSampler s = p.smp[0];
    const uint16_t* x = p.logits + (size_t)i * p.V;
    const unsigned long long pos = (unsigned long long)(long long)p.tab->st[i]->pos;
    if (threadIdx.x == 0) { end.p = p; end.w = (int)gridDim.x; end.sampled = RULES || s.temperature != 0.0f; }
    int tok;
    if constexpr (RULES) {
        const int nd = i < LNB_SPEC_MAX_DRAFT ? i : LNB_SPEC_MAX_DRAFT;
        if (threadIdx.x == 0) dl.n = nd;
        if ((int)threadIdx.x < nd) dl.tok[threadIdx.x] = *p.tab->dtok[threadIdx.x + 1];      // d_1 .. d_i: the inputs of columns 1 .. i
        __syncthreads();
        tok = sample_block<true, true, true>(x, p.V, p.etab, s, false, pos, sh, p.rules, &dl);
    } else tok = s.temperature == 0.0f ? argmax_block(x, p.V, sv, si) : sample_block<false, false, true>(x, p.V, p.etab, s, false, pos, sh);
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const EmitSpecParams q = end.p;
    const int w = end.w;
    if (lane == 0) {
        q.g[i] = tok;
        q.gw[2 * i] = end.sampled ? sh.w_tok : 0ull; q.gw[2 * i + 1] = end.sampled ? sh.z.w_kept : 0ull;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    unsigned t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(q.cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    t = __shfl(t, 0);
    if (t != (unsigned)w - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    int n0 = 0, n1 = 0;
    if (lane == 0) {
        *q.cnt = 0;                                          // (ready for the next launch: stream order)
        StepState* st = q.tab->st[0];
        n0 = st->n_out;
        spec_accept_emit(q.g, w, q.tab, RULES ? q.rules->counts : nullptr);
        n1 = st->n_out;                                      // (a finished run: n0; a stop token: the count up to and with it)
    }
    n0 = __shfl(n0, 0); n1 = __shfl(n1, 0);
    const EmitLog L = *q.log;
    for (int c = 0; c < n1 - n0 && n0 + c < L.cap; c++) {
        const int slot = n0 + c;
        // (the pass's summary launch counts no walk -- it cannot tell an emitted column from a rejected one: an emitted column's is counted here, so that
        // lnb_ctx_token_prob_walks moves as it does in the sampling loop)
        if (lane == 0 && L.walks && q.park[c].walked) atomicAdd(L.walks, 1);
        emit_entry(q.logits + (size_t)c * q.V, q.V, q.etab, q.park + c, q.g[c], q.gw[2 * c], q.gw[2 * c + 1], L, slot);
        if (lane < L.k) {
            const size_t to = (size_t)slot * L.k + lane, from = (size_t)c * L.k + lane;
            L.ids[to] = q.s_ids[from]; L.logit[to] = q.s_logit[from]; L.prob[to] = q.s_prob[from];
        }
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
// the row summary launch: lnbk_token_probs's grid with the PARK instantiations (p->park: [rows])
extern "C" hipError_t lnbk_emit_summary(const TokProbParams* p, hipStream_t st) {
    if (!p->park || p->k < 0 || p->k > LNB_TOKPROB_MAX_K || p->G < 1 || LNB_TOKPROB_MAX_G % p->G || p->rows < 1) return hipErrorInvalidValue;
    const auto k = p->k <= 0 ? token_probs_kernel<0, true> : p->k <= 1 ? token_probs_kernel<1, true> : p->k <= 2 ? token_probs_kernel<2, true>
                 : p->k <= 4 ? token_probs_kernel<4, true> : p->k <= 8 ? token_probs_kernel<8, true> : token_probs_kernel<16, true>;
    form_ran(Form::EMIT_SUMMARY);
    hipLaunchKernelGGL(k, dim3((unsigned)p->G, (unsigned)p->rows), dim3(256), 0, st, *p);
    return hipGetLastError();
}
// the token launch: n = rows (p->advance: 1) or members (p->tab); p->rules picks the rules form
extern "C" hipError_t lnbk_emit_sample(const EmitTokParams* p, int n, hipStream_t st) {
    if (p->V < 1 || p->V > LNB_SAMPLE_MAX_V || n < 1 || (!p->tab && p->advance && n != 1) || !p->park || !p->log || !p->smp) return hipErrorInvalidValue;
    const auto k = p->tab ? (p->rules ? emit_sample_kernel<true, true> : emit_sample_kernel<false, true>)
                          : (p->rules ? emit_sample_kernel<true, false> : emit_sample_kernel<false, false>);
    form_ran(p->tab ? Form::EMIT_BATCH : Form::EMIT_ROW);
    hipLaunchKernelGGL(k, dim3((unsigned)n), dim3(1024), 0, st, *p);
    return hipGetLastError();
}
extern "C" hipError_t lnbk_emit_spec_commit(const EmitSpecParams* p, int w, hipStream_t st) {
    if (p->V < 1 || p->V > LNB_SAMPLE_MAX_V || w < 1 || w > LNB_SPEC_MAX_DRAFT + 1 || !p->logits || !p->etab || !p->smp || !p->g || !p->gw || !p->tab || !p->cnt ||
        !p->park || !p->log) return hipErrorInvalidValue;
    form_ran(Form::EMIT_SPEC);
    hipLaunchKernelGGL(p->rules ? emit_spec_commit_kernel<true> : emit_spec_commit_kernel<false>, dim3((unsigned)w), dim3(1024), 0, st, *p);
    return hipGetLastError();
}
