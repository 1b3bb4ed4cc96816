// lnb_api.cpp -- C ABI (include/lnb.h) over the gfx950 kernels of lnb_kernels.hip.
// Host-side orchestration of LlamaTransformer.Forward (reference: src/model/llamatransformer.go:145-180):
// device-resident weights (re-tiled once), device-resident KV cache, 5 launches per transformer block,
// and a hipGraph-replayed greedy decode loop whose position/token state lives on the device.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <dirent.h>
#include <unistd.h>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/lnb.h"
#include "lnb_device.h"
#include "lnb_knobs.h"
#include "lnb_forms.h"
#include "lnb_gemv_geom.h"
#include "lnb_kvcopy.h"
#include "lnb_rowpack.h"
#include "lnb_wpack.h"
#include "lnb_batchplan.h"
#include "lnb_handoff.h"
#include "lnb_own.h"
#include "lnb_rccl.h"
#include "lnb_sample.h"
static_assert(LNB_MAX_SEQ_LEN == LNB_SEQ_MAX, "lnb.h and lnb_device.h disagree on the longest context");
static_assert(ROWPACK_MAX_W == LNB_BATCH_MAX, "lnb_rowpack.h and lnb_device.h disagree on the columns of a pass");
static_assert(BATCHPLAN_COLS == LNB_STREAM_COLS, "lnb_batchplan.h and lnb_device.h disagree on the sequences of a column group");
static_assert(LNB_MAX_FORK == KVC_MAX_DST, "lnb.h and lnb_kvcopy.h disagree on the destinations of a fork");
static_assert(LNB_MAX_TOP_K == LNB_TOKPROB_MAX_K, "lnb.h and lnb_device.h disagree on the largest top-k");
static_assert(sizeof(lnb_sampler) == sizeof(LnbSampler) && sizeof(lnb_sampler) == 24 && sizeof(lnb_sample_info) == sizeof(LnbSampleInfo) && sizeof(lnb_sample_info) == 40 &&
              LNB_SAMPLE_MAX_VOCAB == LNB_SAMPLE_MAX_V, "lnb.h and lnb_sample.h disagree on the sampler");
static_assert(LNB_MAX_DRAFT == LNB_SPEC_MAX_DRAFT && LNB_MAX_DRAFT + 1 <= LNB_STREAM_COLS, "a verify pass is one column group of at most 16 columns");

extern "C" {
hipError_t lnbk_gemv(const GemvParams* p, int rw, int nch, int epi, int norm, hipStream_t st);
hipError_t lnbk_attn(const AttnParams* p, hipStream_t st);
hipError_t lnbk_attn_rows(const AttnParams* p, int pos0, hipStream_t st);
hipError_t lnbk_kv_scan_nonfinite(const uint16_t* ck, const uint16_t* cv, int seq_len, int kv_dim, int hd, const StepState* st, int pos0, int rows, int* word, hipStream_t s);
hipError_t lnbk_nonfinite_or(int* dst, const int* src, hipStream_t s);
hipError_t lnbk_attn_plain(const AttnParams* p, const int* word, hipStream_t st);
int lnbk_attn_short_max_T(int hd);
size_t lnbk_attn_long_lds(int seq_len);
size_t lnbk_attn_long_layout_lds(int seq_len);
size_t lnbk_attn_one_lds(int seq_len, int hd);
hipError_t lnbk_exp_table(double* tab, float divisor, hipStream_t st);
hipError_t lnbk_gemm(const GemmParams* p, int epi, hipStream_t st);
hipError_t lnbk_rmsnorm_rows(const uint16_t* x, const uint16_t* w, uint16_t* out, int S, int K, float eps, hipStream_t st);
hipError_t lnbk_rmsnorm_rows_form(const uint16_t* x, const uint16_t* w, uint16_t* out, int S, int K, float eps, int form, uint32_t* norm_out, hipStream_t st);
hipError_t lnbk_gemv_norm_report(const GemvParams* p, int form, hipStream_t st);
hipError_t lnbk_embed(const uint16_t* emb, const int32_t* tokens, uint16_t* x, int S, int dim, int vocab, int* err, hipStream_t st);
hipError_t lnbk_argmax(const uint16_t* logits, int V, int32_t* next_token, StepState* state, int32_t* out_tokens, int out_cap, int advance, hipStream_t st);
hipError_t lnbk_sample(const uint16_t* logits, int V, int rows, const double* etab, const LnbSampler* smp, int32_t* next_token, StepState* state, int32_t* out_tokens,
                       int out_cap, int advance, const int32_t* pos, const unsigned long long* draws, LnbSampleInfo* info, hipStream_t st);
hipError_t lnbk_batch_sample(const uint16_t* logits, int V, const double* etab, const LnbSampler* smp, const BatchTab* tab, int nseq, hipStream_t st);
hipError_t lnbk_set_state(StepState* state, int pos, int n_out, int honour_stop, hipStream_t st);
hipError_t lnbk_set_stop(StepState* state, const int32_t* ids, int n, hipStream_t st);
hipError_t lnbk_advance_state(StepState* state, int rows, hipStream_t st);
hipError_t lnbk_tile(const uint16_t* src, uint16_t* dst, int rows, int K, int row_off, int chain, int RW, int NCH, int gather, hipStream_t st);
hipError_t lnbk_synth_fill(uint16_t* dst, int rows, int K, int row_off, int chain, int RW, int NCH, uint64_t seed, uint32_t tensor_id, int kind, float sigma, hipStream_t st);
hipError_t lnbk_init(void);
int lnbk_w13p_supported(int rw, int K);
hipError_t lnbk_gemv_w13p(const GemvParams* p, hipStream_t st);
size_t lnbk_wpack_w13_bytes(int n_blocks, int K);
hipError_t lnbk_wpack_stats(const uint16_t* w, size_t elems, unsigned* d_stats, hipStream_t st);
hipError_t lnbk_wpack_w13(const uint16_t* w, void* out, int K, int n_blocks, unsigned base, hipStream_t st);
int lnbk_headp_supported(int K);
hipError_t lnbk_gemv_headp(const GemvParams* p, hipStream_t st);
size_t lnbk_wpack_head_bytes(int N, int K);
hipError_t lnbk_wpack_head(const uint16_t* w, void* out, int N, int K, unsigned base, hipStream_t st);
hipError_t lnbk_fast_gemv(const GemvParams* p, int rw, int nch, int epi, int norm, hipStream_t st);
hipError_t lnbk_fast_gemm(const GemmParams* p, int epi, hipStream_t st);
hipError_t lnbk_fast_attn(const AttnParams* p, hipStream_t st);
hipError_t lnbk_fast_init(void);
hipError_t lnbk_m16_from_tiled(const uint16_t* src, uint16_t* dst, int rows, int K, int RW, int NCH, hipStream_t st);
hipError_t lnbk_stream(const StreamParams* p, int epi, int acc2, int num_cus, hipStream_t st);
hipError_t lnbk_batch_rmsnorm(const uint16_t* x, const uint16_t* norm_w, float eps, uint16_t* xt, int K, int nseq, hipStream_t st);
hipError_t lnbk_batch_rmsnorm_out(const uint16_t* x, const uint16_t* norm_w, float eps, uint16_t* xt, int K, int nseq, uint32_t* norm_out, hipStream_t st);
hipError_t lnbk_batch_embed(const uint16_t* emb, const BatchTab* tab, uint16_t* x, int nseq, int dim, int vocab, int* err, hipStream_t st);
hipError_t lnbk_batch_argmax(const uint16_t* logits, int V, const BatchTab* tab, int nseq, int32_t* ring, hipStream_t st);
hipError_t lnbk_batch_set_state(const BatchTab* tab, const int32_t* tokens, const int32_t* pos, int32_t* ring, int honour_stop, hipStream_t st);
hipError_t lnbk_batch_scatter_ring(const BatchTab* tab, const int32_t* ring, hipStream_t st);
hipError_t lnbk_batch_advance(const BatchTab* tab, hipStream_t st);
hipError_t lnbk_batch_prepare(void);
hipError_t lnbk_gemm_stream(const GemmParams* p, int epi, int num_cus, hipStream_t st);
hipError_t lnbk_spin(int us, hipStream_t st);
hipError_t lnbk_token_probs(const TokProbParams* p, hipStream_t st);
hipError_t lnbk_spec_argmax(const uint16_t* logits, int V, int w, int32_t* g, hipStream_t st);
hipError_t lnbk_spec_commit(const int32_t* g, int w, const BatchTab* tab, hipStream_t st);
hipError_t lnbk_spec_sample_commit(const uint16_t* logits, int V, int w, const double* etab, const LnbSampler* smp, int32_t* g, const BatchTab* tab, unsigned* cnt, hipStream_t st);
hipError_t lnbk_ngram_draft(const DraftParams* p, hipStream_t st);
hipError_t lnbk_kv_fork(const KvForkTab* tab, int nt, int split, hipStream_t st);
hipError_t lnbk_append_many_setup(const AmPass* p, hipStream_t st);
hipError_t lnbk_append_many_finish(const uint16_t* logits, int V, const AmRow* rows, int width, int32_t* out, hipStream_t st);
hipError_t lnbk_spec_many_draft(const SmPass* p, hipStream_t st);
hipError_t lnbk_spec_many_pack(const SmPass* p, hipStream_t st);
hipError_t lnbk_spec_many_commit(const SmPass* p, hipStream_t st);
hipError_t lnbk_spec_many_sample_commit(const SmPass* p, hipStream_t st);
}

// The HIP runtime spreads a process's streams over a fixed number of hardware queues (its default: 4) and streams that share a queue run one
// after the other.  This library gives every context its own stream so that several generations can overlap on one GPU (one InferenceContext
// per generation, inference.go:174; 2N contexts per pipeline rank); how many really overlap is up to the process environment, which the library
// leaves alone.  lnb_runtime_info() reports what the environment asks for, whether the HIP runtime had ALREADY been initialised when this library
// was loaded and, on request, the number of streams that really run concurrently (measured, not read from the environment).
static int g_hwq_set_by_library = 0;      // always 0: the library no longer sets a default (the ABI field stays)
static int g_hip_live_at_load = 0;        // 1: /dev/kfd was already open when the library was loaded -> the runtime read the variable before us
static bool kfd_is_open() {
    // the ROCm runtime (HSA) opens /dev/kfd when it initialises, never before: an open descriptor on it = HIP has been used in this process
    DIR* d = opendir("/proc/self/fd");
    if (!d) return false;
    bool found = false;
    char path[64], target[256];
    while (struct dirent* e = readdir(d)) {
        if (e->d_name[0] == '.') continue;
        snprintf(path, sizeof path, "/proc/self/fd/%s", e->d_name);
        const ssize_t n = readlink(path, target, sizeof target - 1);
        if (n <= 0) continue;
        target[n] = 0;
        if (!strcmp(target, "/dev/kfd")) { found = true; break; }
    }
    closedir(d);
    return found;
}
__attribute__((constructor)) static void lnb_record_hip_state_at_load() {
    g_hip_live_at_load = kfd_is_open() ? 1 : 0;
}

static thread_local char g_err[1024] = "";
static int fail(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return -1;
}
extern "C" const char* lnb_last_error(void) { return g_err; }
// shared with lnb_checkpoint.cpp (same library, not part of the ABI)
extern "C" __attribute__((visibility("hidden"))) void lnb_set_error(const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); }
#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

// Who releases what (lnb_own.h): a device resource is an owning member or a local owner, released when its scope ends -- no free list to keep.
// Members are destroyed in reverse order of declaration: a handle struct declares its stream FIRST, so that it goes after everything enqueued on it.
template <class T> using Dev = Owned<T*, hipFree>;                    // device memory
template <class T> using Pinned = Owned<T*, hipHostFree>;             // pinned host memory
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;
template <class T> using DevGrown = Grown<T*, hipFree>;
using DevArena = Arena<hipError_t, hipMalloc, hipFree>;
template <class T> static hipError_t dev_alloc(Dev<T>& p, size_t bytes) { return p.fill([&](T** q) { return hipMalloc((void**)q, bytes); }); }
template <class T> static hipError_t dev_reserve(DevGrown<T>& p, size_t bytes) { return p.reserve(bytes, [](T** q, size_t n) { return hipMalloc((void**)q, n); }); }
template <class T> static hipError_t pinned_alloc(Pinned<T>& p, size_t bytes, unsigned flags) { return p.fill([&](T** q) { return hipHostMalloc((void**)q, bytes, flags); }); }
static hipError_t event_create(Event& e, unsigned flags = hipEventDefault) { return e.fill([&](hipEvent_t* q) { return hipEventCreateWithFlags(q, flags); }); }
static hipError_t stream_create(Stream& s, unsigned flags) { return s.fill([&](hipStream_t* q) { return hipStreamCreateWithFlags(q, flags); }); }
// which captured step: the token launch that ends it, and the attention form its launches bake in
enum GraphLaunch { GL_GREEDY = 0, GL_SAMPLE, GL_STAGE, GL_COUNT };
enum GraphForm { GF_SHORT = 0, GF_LONG, GF_ROWS, GF_COUNT };         // (0, 1, 2: also what lnb_ctx_verify_attention_form reports)
using Graphs = GraphTable<hipGraphExec_t, hipGraphExecDestroy, GL_COUNT, GF_COUNT>;

static inline float bf_wide_h(uint16_t b) { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }
static inline uint16_t bf_trunc_h(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)(u >> 16); }

// ---------------------------------------------------------------------------------------------------
struct TensorRef {
    int rows = 0, cols = 0;        // logical shape in the reference layout (1-D tensors: rows = 1)
    bool tiled = false;
    uint16_t* linear = nullptr;    // when !tiled (the model's `weights` arena owns it)
    TiledDesc* td = nullptr;       // when tiled
    int row_off = 0, chain = 0;
    uint32_t synth_id = 0; int synth_kind = 0;
    int rank = 2;
};
struct LayerW {
    // (raw pointers, these and TiledDesc::w / w16 -- the launch layer shares the descriptor: the model's `weights` arena owns them, its `m16` arena the M16 copies)
    uint16_t* attn_norm = nullptr; uint16_t* ffn_norm = nullptr;
    TiledDesc wqkv{}, wo{}, w13{}, w2{};
    // batched decode (lnb_model_enable_batch): the same matrices in the 16-row matrix-core layout (M16, lnb_device.h)
    uint16_t *m_wqkv = nullptr, *m_wo = nullptr, *m_w13 = nullptr, *m_w2 = nullptr;
    // one-token decode (lnb_model_finalize, LNB_W13_PACKED): the 13-bit planar copy of w13 (lnb_wpack.h) the latency form streams instead of the raw bf16
    Dev<void> p_w13; unsigned p_base = 0; bool p_ok = false;           // p_ok: the copy holds what w13 holds
    int p_status = -1;                                                  // WPACK_* of the last attempt (-1: none -- knob off or a layout the packed kernel has no form for)
};
struct lnb_model {
    lnb_model_args a{};
    int device = 0, layer_begin = 0, layer_end = 0;      // layers this handle touches
    int part_begin = 0, part_end = 0;                     // ... in thirds of a block: 3l = attention part of layer l, 3l+1 = gate/up, 3l+2 = down
    int head_dim = 0, n_rep = 0, ffn_hidden = 0, q_dim = 0, kv_dim = 0;
    Stream stream;
    DevArena weights, m16;                // what alloc_tiled / alloc_linear and m16_copy hand out: tok_embd, norm, output, m_output and the LayerW pointers
    uint16_t* tok_embd = nullptr; uint16_t* norm = nullptr; TiledDesc output{};
    std::vector<LayerW> layers;           // indexed by absolute layer id - layer_begin
    std::map<std::string, TensorRef> tensors;
    Dev<float> cis; int cis_rows = 0; Dev<float> silu; Dev<double> exp_tab;
    Dev<double> prob_etab;                // exp(double(bf16)) of the host C library for all 65536 patterns: the token probabilities (token_probs_kernel)
    std::vector<float> cis_host;
    bool finalized = false;
    int64_t weight_bytes = 0;
    bool batch_enabled = false; uint16_t* m_output = nullptr; int64_t batch_bytes = 0;
    int64_t wpack_bytes = 0;              // the 13-bit planar copies of the gate|up matrices (lnb_model_wpack_bytes)
    // the LM head's 13-bit copy (lnb_model_finalize, LNB_HEAD_PACKED; 128-row two-chain blocks: lnb_wpack.h), as LayerW's p_* fields are for gate|up
    Dev<void> p_out; unsigned p_out_base = 0; bool p_out_ok = false; int p_out_status = -1; int64_t wpack_head_bytes = 0;
    std::mutex am_mu; struct AppendMany* am = nullptr;     // lnb_forward_append_many: the call's buffers and tables, created on first use; the mutex is held for a whole call
    bool first() const { return part_begin == 0; }
    bool last() const { return part_end == 3 * a.n_layers; }
    bool has_part(int l, int q) const { return 3 * l + q >= part_begin && 3 * l + q < part_end; }
    bool has_attn(int l) const { return has_part(l, 0); }
    bool has_w13(int l) const { return has_part(l, 1); }
    bool has_w2(int l) const { return has_part(l, 2); }
    bool whole(int l) const { return has_attn(l) && has_w13(l) && has_w2(l); }
};
// What a unit that moves through the pipeline's stages -- a context (lnb_pipeline_tick) or a batch (lnb_pipeline_tick_batch) -- needs to be
// handed across a stage boundary: three events between its own stream and the pipe's exchange stream, and whether one is outstanding.
struct PipeLink {
    Event ev_done, ev_in, ev_sent;         // its stage step has run / its input has arrived / its output has left
    bool in_pending = false, sent_pending = false;
    bool recv_unmatched = false;           // in-process transport: a receive into this unit is posted and its sender has not arrived yet
    int ensure() {                         // (created on the unit's first tick)
        if (!ev_sent) for (Event* e : {&ev_done, &ev_in, &ev_sent}) HIPCHK(event_create(*e, hipEventDisableTiming));
        return 0;
    }
    // before the unit's stage step on its stream st: its input has arrived and its previous output has left
    int await(hipStream_t st, const char* unit) {
        if (recv_unmatched) return fail("in-process pipeline: this %s's input has been requested but the sending stage has not posted it yet "
                                        "(the mailbox transport needs the stages ticked in lock-step order from one thread)", unit);
        if (in_pending) { HIPCHK(hipStreamWaitEvent(st, ev_in, 0)); in_pending = false; }
        if (sent_pending) { HIPCHK(hipStreamWaitEvent(st, ev_sent, 0)); sent_pending = false; }
        return 0;
    }
};
struct lnb_ctx {
    lnb_model* m = nullptr; int seq_len = 0;
    int max_rows = 0;                      // rows per call the activation buffers (x, h, xn, q, att, ffn) hold: seq_len, or lnb_ctx_create_long's max_rows
    Stream stream;                         // (declared before everything enqueued on it: released last)
    std::vector<Dev<uint16_t>> ck, cv;     // per layer of the stage; empty where the stage holds no attention part of the block
    Dev<StepState> st; Dev<int32_t> dtok, dnext; Dev<int> derr;
    Dev<int32_t> dout; int dout_cap = 0;
    Dev<uint16_t> x, h, q, att, ffn, logits;
    Dev<uint16_t> xn;                      // [max_rows][dim] normalised rows for the matrix-core prefill path
    int logits_rows = 0;
    // the captured steps: greedy / sampling (lnb_decode_sample_until: they hold the POINTER d_smp, the call copies its sampler there before the replays) /
    // pipeline stage (lnb_pipeline_tick), each per attention form (short, long).  Every one bakes in the context's buffers, its arithmetic mode and its
    // attention form: whatever changes one of those drops them all (graphs.drop_all())
    Graphs graphs;
    Event ev0, ev1;
    lnb_layer_cb cb = nullptr; void* cb_user = nullptr;
    Pinned<int32_t> h_io;                  // pinned host words of lnb_forward_stage_begin/_end: [0] argmax, [1] token error, [2..] tokens
    bool pending = false, pending_tokens = false, pending_argmax = false;
    int mode = LNB_MODE_EXACT;             // LNB_MODE_FAST: split-K kernels of lnb_fast.hip (tolerance mode, opt-in)
    int sched = LNB_SCHED_LATENCY;         // LNB_SCHED_THROUGHPUT: the co-residency-friendly forms of the one-token kernels (lnb_ctx_set_schedule)
    int n_stop = 0;                        // host copy of StepState.n_stop (lnb_ctx_set_stop_ids): entry points that cannot honour stop ids refuse such a context
    int batch_users = 0;                   // live lnb_batch handles this context is a member of: their device tables and captured graphs hold its raw pointers
    // long-context decode attention (attn_long_*_kernel): used for one-token calls whose context exceeds attn_long_T
    Dev<double> e_buf, z_part; Dev<int> zseq_count;
    int last_prefill_form = 0;         // lnb_ctx_prefill_attention_form
    DevGrown<uint64_t> score_idx; int sidx_jt = 0;      // attn_mfma3_kernel's scratch (the exp-table indices of pass 1), grown on demand by check_call; sidx_jt = 0: this call runs attn_mfma_kernel
    Dev<unsigned> attn_cnt;                // attn_one_kernel: [n_heads] arrival counters of its in-launch exchange + [n_heads] = polls that ran out
    int attn_long_T = 0; int force_zseq = 0;   // force_zseq: bit 0 = walk the serial softmax denominator, bit 1 = keep the two-launch long-context form, bit 2 = one launch with every poll timing out (tests), bit 3 = one launch
    int attn_short_cap = 0;                // longest context the one-workgroup-per-head kernel can stage in the LDS
    bool attn_long = false;                // selection for the launches being enqueued (set per call / per captured graph)
    Dev<LnbSampler> d_smp;                 // the sampling step's sampler
    PipeLink link;                         // pipeline stage (lnb_pipeline_tick): events towards / from the exchange stream
    int dev_pos = -1;                      // position the device-side StepState will hold when the stream reaches this point (-1: unknown)
    bool attn_causal = false;              // set by lnb_forward_append around its multi-row call: the attention launches take the true causal mask (AttnParams::causal)
    int call_T = 0;                        // start_pos + rows of the call being enqueued (0: not known to the host, e.g. inside a replayed graph)
    Event ev_h2d; bool h2d_pending = false;   // the last copy out of the pinned staging words h_io[2..] (enqueue-only paths)
    // token probabilities of the greedy loop (lnb_ctx_set_token_probs): a record log of dout_cap x top_k beside the token log
    int top_k = 0;
    // (one struct, so that switching the feature off is `tp = {}`; the members of the TokProbOut on the device alias ids .. logz, st and zseq_count of this context)
    struct TokProbLog {
        Dev<TokProbOut> out;               // device: this context's log (st = c->st: the record slot is the token's)
        Dev<int32_t> ids; Dev<float> logit, prob; Dev<double> logz;
        Dev<double> zpart; Dev<uint64_t> kpart; Dev<unsigned> cnt;   // one row's partials, arrival ticket
    } tp;
    int tp_last_k = 0, tp_last_n = 0;      // what the last decode call that ran this context recorded (k 0: nothing)
    DevGrown<char> sc_buf;                 // lnb_forward_score's scratch, grown on demand
    // speculative decoding (lnb_ctx_set_draft, lnb_decode_speculative_until): drafting settings, the corpus, the running text's head (history +
    // token), the verify columns' states and token words (index 0 unused: column 0 is this context's own), their argmax, the draft kernel's
    // scratch and the pinned word it reports to the host; one verify batch per width 2..16, built and captured on first use
    int sp_max_draft = 0, sp_ngram_min = 1, sp_ngram_max = 1;
    Dev<int32_t> sp_corpus; int sp_n_corpus = 0;
    DevGrown<int32_t> sp_text;
    Dev<StepState> sp_st; Dev<int32_t> sp_tok, sp_g; Dev<int> sp_best; Dev<unsigned> sp_cnt;
    Pinned<int32_t> sp_word; Event sp_ev;
    int32_t* sp_word_dev = nullptr;        // the device address of sp_word (mapped pinned memory: sp_word owns it)
    struct lnb_batch* sp_b[LNB_MAX_DRAFT + 2] = {};      // (their scratch is this context's: destroyed before it, in lnb_ctx_destroy)
    // attention form of the verify passes (lnb_ctx_set_batched_attention): threshold (default: never), serial-sum switch, the ONE e_buf / z_part
    // scratch all widths share (sized for 16 columns, allocated when a pass first needs the long form), the form of the last verify pass
    int sp_attn_long_T = 0x7FFFFFFF, sp_force_zseq = 0, sp_last_form = 0;
    Dev<double> sp_e_buf, sp_z_part;
    // multi-row long-context attention (attn_rows_*_kernel, lnb_ctx_set_rows_attention): appends of 2..15 rows (any row count at head_dim 32) whose
    // start_pos + seq exceeds rows_T (default attn_short_cap: the calls the row-per-workgroup kernel cannot take) run it; rows_flags bit 0 = every row
    // walks the serial sum, bit 1 = the verify passes run it wherever they would run the long form.  Its scratch is sp_e_buf / sp_z_part.
    int rows_T = 0, rows_flags = 0, last_append_form = 0;
    bool attn_rows = false;                // set by lnb_forward_append around a multi-row call that runs the pair
    bool rows_no_scratch = false;          // an append could not allocate the pair's scratch: such calls run as one-token steps from then on
    DevGrown<char> fork_tab;               // lnb_ctx_fork with this context as the source: the device table of the call, grown on demand
};
// Every path that rewrites the device-side StepState goes through here, so that the pipeline tick's "the graph left pos+1 behind, skip
// the set_state launch" shortcut (dev_pos) can never act on a position some OTHER entry point has since overwritten (lnb_forward,
// lnb_decode_greedy and lnb_profile_kernel may be mixed with ticks on one context).  known = false: the caller is about to advance
// the state on the device by itself (greedy loop) and the host stops tracking it.
static hipError_t ctx_set_state(lnb_ctx* c, int pos, int n_out, bool known, bool honour_stop = false) {
    c->dev_pos = known ? pos : -1;
    return lnbk_set_state(c->st, pos, n_out, honour_stop ? 1 : 0, c->stream);
}
// the pinned staging words h_io[2..] are reused by every enqueue-only call that takes host tokens: wait for the copy that still reads them
static int staging_acquire(lnb_ctx* c) {
    if (c->h2d_pending) { HIPCHK(hipEventSynchronize(c->ev_h2d)); c->h2d_pending = false; }
    return 0;
}
static int staging_release(lnb_ctx* c) {
    if (!c->ev_h2d) HIPCHK(event_create(c->ev_h2d, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_h2d, c->stream)); c->h2d_pending = true;
    return 0;
}

static int auto_rw(int lane_rows, Knob env, int K = 0, bool plain = false, int unforced = 0) {      // unforced: the caller's choice while the knob is 0 (0: by shape)
    const int v = knob(env);
    if (v == 0 && unforced) return unforced;
    if (v == 16 || v == 32 || v == 64 || (v == 4 && plain && gemv_layout_takes(4, K)) || ((v == 56 || v == 28) && lane_rows % v == 0) || (v == 24 && K > 0 && gemv_layout_takes(24, K))) return v;
    // thin matrices without a fused norm / rope epilogue: the row-broadcast kernel (products stay in registers)
    if (plain && lane_rows <= 16 * 256 && K > 0 && gemv_layout_takes(4, K)) return 4;
    // thin matrices: one workgroup (16 or 32 rows) per CU, all resident at once on the 256 CUs -- a second round of
    // workgroups would double the serial chain time
    if (lane_rows <= 16 * 256) return 16;
    if (lane_rows <= 32 * 256) return 32;
    return 64;
}
static int g_num_cus = 256;
static thread_local long long* g_dbg = nullptr;   // (thread-local: arming the stamps on one thread must not reach another thread's launches -- ADVICE r5) LNB_GEMV_TIMING=1: per-wave timing dump of the profiled launch
static thread_local int g_dbg_full = 0;           // ... with every barrier and ring wait timed (perturbs the launch); 0: phase stamps and the exit record only
// one resident workgroup per CU: a matrix with more row blocks than CUs is walked persistently
static void set_grid(GemvParams& g, const TiledDesc& t) { g.dbg = g_dbg; g.dbg_full = g_dbg ? g_dbg_full : 0; g.n_blocks = t.n_blocks; g.n_wg = t.n_blocks < g_num_cus ? t.n_blocks : g_num_cus; }
// `bytes` of device memory out of an arena (the caller's scope owns them); a null pointer: the arena's latched error, in HIPCHK's words
template <class T> static int arena_alloc(DevArena& a, T** p, size_t bytes) {
    *p = (T*)a.alloc<char>(bytes);
    if (!*p) HIPCHK(a.error());
    return 0;
}
static int alloc_tiled(DevArena& a, TiledDesc& t, int n_rows, int K, int rw, int nch, int64_t& bytes) {
    t.n_rows = n_rows; t.k = K; t.rw = rw; t.nch = nch; t.n_blocks = rw == 4 ? (n_rows + 15) / 16 : (n_rows + rw - 1) / rw;   // rw 4: 16-row workgroups
    size_t n = tiled_elems(n_rows, K, rw, nch) * 2;
    if (arena_alloc(a, &t.w, n)) return -1;
    HIPCHK(hipMemset(t.w, 0, n));
    bytes += (int64_t)n;
    return 0;
}
static int alloc_linear(DevArena& a, uint16_t** p, size_t elems, int64_t& bytes) {
    if (arena_alloc(a, p, elems * 2)) return -1;
    HIPCHK(hipMemset(*p, 0, elems * 2)); bytes += (int64_t)elems * 2; return 0;
}

// what every entry point that takes a device index instead of a handle does first (the lnb_op_* test aids, lnb_pipeline_selftest)
static int op_device(int device) {
    int ndev = 0; HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev == 0) return fail("no HIP device: liblnb_hip.so has no CPU fallback");
    HIPCHK(hipSetDevice(device));
    return 0;
}
extern "C" int lnb_device_count(int* out) { int n = 0; HIPCHK(hipGetDeviceCount(&n)); *out = n; return 0; }
extern "C" int lnb_abi_version(void) { return LNB_ABI_VERSION; }
// the launch tally (lnb_forms.h): which kernel forms the launch functions of this process have picked since the last reset
extern "C" int lnb_form_count(const char* form, int epi, int64_t* out) {
    if (!form || !out) return fail("null argument");
    const int i = form_index(form);
    if (i < 0) return fail("unknown form '%s' (lnb_form_name enumerates the table of csrc/lnb_forms.h)", form);
    if (epi < -1 || epi >= LNB_FORM_EPIS) return fail("epilogue %d: -1 (the sum) or 0..%d", epi, LNB_FORM_EPIS - 1);
    *out = form_count(i, epi);
    return 0;
}
extern "C" int lnb_form_count_reset(void) { form_count_reset(); return 0; }
extern "C" int lnb_form_name(int index, const char** name) {
    if (!name) return fail("null argument");
    if (index < 0 || index >= (int)Form::COUNT) return fail("form index %d: the table has %d rows", index, (int)Form::COUNT);
    *name = LNB_FORM_TABLE[index].name;
    return 0;
}
// What the host should know before it trusts a multi-context run: the hardware queues the HIP runtime was told to use, who told it,
// whether that was in time, and -- probe_queues != 0 -- how many streams REALLY run concurrently: 32 one-wave kernels that each hold their stream for
// 2 ms of wall clock, one per stream; with Q queues they finish in ceil(32 / Q) rounds (4-20 ms including the stream set-up).
extern "C" int lnb_runtime_info(int device, int probe_queues, lnb_runtime_info_t* out) {
    if (!out) return fail("null argument");
    memset(out, 0, sizeof *out);
    out->abi_version = LNB_ABI_VERSION;
    int ndev = 0; HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev == 0) return fail("no HIP device: liblnb_hip.so has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, device));
    out->device = device; out->n_cus = prop.multiProcessorCount;
    snprintf(out->device_name, sizeof out->device_name, "%s", prop.name);
    snprintf(out->arch, sizeof out->arch, "%s", prop.gcnArchName);
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeClockRate, device) == hipSuccess) out->shader_clock_khz = v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMemoryClockRate, device) == hipSuccess) out->memory_clock_khz = v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, device) == hipSuccess) out->wall_clock_khz = v;
    const char* q = getenv("GPU_MAX_HW_QUEUES");
    out->hw_queues_env = q && *q ? atoi(q) : 0;
    out->hw_queues_set_by_library = g_hwq_set_by_library;
    out->hip_initialised_before_load = g_hip_live_at_load;
    // what the runtime will have honoured: the environment's value, else the runtime's default, 4
    out->hw_queues_expected = out->hw_queues_env > 0 ? out->hw_queues_env : 4;
    if (probe_queues) {
        constexpr int NSTREAM = 32, SPIN_US = 2000;      // (2 ms per spin: the ~0.3 ms it takes the host to launch on 32 streams must not count as a round)
        Stream sts[NSTREAM]; Event e0, e1, ej[NSTREAM];
        for (int i = 0; i < NSTREAM; i++) { HIPCHK(stream_create(sts[i], hipStreamNonBlocking)); HIPCHK(event_create(ej[i], hipEventDisableTiming)); }
        HIPCHK(event_create(e0)); HIPCHK(event_create(e1));
        float ms = 0;
        for (int rep = 0; rep < 2; rep++) {                          // (the first round warms the streams up)
            HIPCHK(hipEventRecord(e0, sts[0]));
            for (int i = 1; i < NSTREAM; i++) HIPCHK(hipStreamWaitEvent(sts[i], e0, 0));
            for (int i = 0; i < NSTREAM; i++) HIPCHK(lnbk_spin(SPIN_US, sts[i]));
            for (int i = 1; i < NSTREAM; i++) { HIPCHK(hipEventRecord(ej[i], sts[i])); HIPCHK(hipStreamWaitEvent(sts[0], ej[i], 0)); }
            HIPCHK(hipEventRecord(e1, sts[0]));
            HIPCHK(hipEventSynchronize(e1));
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        }
        const double rounds = (double)ms * 1000.0 / SPIN_US;     // 32 / Q, plus launch overhead
        int qm = rounds > 0.5 ? (int)((double)NSTREAM / rounds + 0.5) : NSTREAM;
        out->hw_queues_measured = qm < 1 ? 1 : (qm > NSTREAM ? NSTREAM : qm);
        out->probe_ms = ms;
    }
    return 0;
}
// what a multi-GPU host prints before it trusts a run (bench.py --gpus N: the per-rank preflight record): the device behind an index, and
// whether `device` can map `peer`'s memory (hipDeviceCanAccessPeer: xGMI / PCIe peer-to-peer, what RCCL's point-to-point path rides on)
extern "C" int lnb_device_info(int device, char* name, int name_cap, int64_t* hbm_bytes, int* n_cus, char* arch, int arch_cap) {
    int ndev = 0; HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
    hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, device));
    if (name && name_cap > 0) snprintf(name, (size_t)name_cap, "%s", prop.name);
    if (arch && arch_cap > 0) snprintf(arch, (size_t)arch_cap, "%s", prop.gcnArchName);
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    if (n_cus) *n_cus = prop.multiProcessorCount;
    return 0;
}
extern "C" int lnb_device_pci_bus_id(int device, char* out, int cap) {
    if (!out || cap < 16) return fail("null argument or a buffer under 16 bytes");
    int ndev = 0; HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipDeviceGetPCIBusId(out, cap, device));
    return 0;
}
extern "C" int lnb_device_can_access_peer(int device, int peer, int* out) {
    if (!out) return fail("null argument");
    int ndev = 0; HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev || peer < 0 || peer >= ndev) return fail("device pair (%d, %d) out of range (%d devices)", device, peer, ndev);
    if (device == peer) { *out = 1; return 0; }
    int can = 0; HIPCHK(hipDeviceCanAccessPeer(&can, device, peer));
    *out = can;
    return 0;
}

extern "C" int lnb_model_ffn_hidden_dim(const lnb_model_args* a) {   // llamatransformer.go:569-577
    int h = 4 * a->dim;
    h = (int)(2 * h / 3);
    if (a->ffn_dim_multiplier > -1) h = (int)(a->ffn_dim_multiplier * (double)h);
    h = a->multiple_of * ((h + a->multiple_of - 1) / a->multiple_of);
    return h;
}

static void reg_linear(lnb_model* m, const std::string& name, uint16_t* p, int cols, uint32_t sid, int kind, int rows = 1, int rank = 1) {
    TensorRef r; r.rows = rows; r.cols = cols; r.tiled = false; r.linear = p; r.synth_id = sid; r.synth_kind = kind; r.rank = rank;
    m->tensors[name] = r;
}
static void reg_tiled(lnb_model* m, const std::string& name, TiledDesc* td, int rows, int cols, int row_off, int chain, uint32_t sid) {
    TensorRef r; r.rows = rows; r.cols = cols; r.tiled = true; r.td = td; r.row_off = row_off; r.chain = chain; r.synth_id = sid; r.rank = 2;
    m->tensors[name] = r;
}

extern "C" int lnb_model_create(const lnb_model_args* args, int device, int layer_begin, int layer_end, lnb_model** out) {
    return lnb_model_create_parts(args, device, 3 * layer_begin, 3 * layer_end, out);
}
// Pipeline stages may be cut INSIDE a block, in thirds: 3l = attention part (attention_norm, wq|wk|wv, attention, wo + residual,
// llamatransformer.go:222-232), 3l+1 = gate/up part (ffn_norm, w1|w3, SiLU*up, :237, :601-617), 3l+2 = down part (w2 + residual,
// :619, :248).  After the attention part the live state is again one [S, dim] vector (h); after the gate/up part it is h plus the
// [S, ffn_hidden] activations.  The three parts cost about the same HBM time (48 / 47 / 45 us for the 8B shape), so the stages of a
// pipeline can be balanced to a third of a block (pipeline.stage_parts).
static int model_alloc(lnb_model* m);
extern "C" int lnb_model_create_parts(const lnb_model_args* args, int device, int part_begin, int part_end, lnb_model** out) {
    if (!args || !out) return fail("null argument");
    *out = nullptr;
    const int layer_begin = part_begin / 3, layer_end = (part_end + 2) / 3;
    lnb_model_args a = *args;
    if (a.n_kv_heads < 0) a.n_kv_heads = a.n_heads;                       // llamatransformer.go:73-75
    if (a.rope_theta <= 0) a.rope_theta = 500000.0;                       // :80-82
    if (a.n_layers <= 0) return fail("n_layers must be positive (got %d)", a.n_layers);
    if (a.vocab_size <= 0) return fail("vocab_size must be positive (got %d; params.json without the key gives -1: take it from tok_embeddings)", a.vocab_size);
    if (a.multiple_of <= 0) return fail("multiple_of must be positive (got %d)", a.multiple_of);
    if (a.dim <= 0 || a.n_heads <= 0 || a.n_kv_heads <= 0 || a.dim % a.n_heads || a.n_heads % a.n_kv_heads) return fail("invalid head configuration");
    if (part_begin < 0 || part_end > 3 * a.n_layers || part_begin >= part_end) return fail("invalid layer range [%d,%d)", part_begin / 3, (part_end + 2) / 3);
    int hd = a.dim / a.n_heads;
    if (a.dim % 8 || hd % 8) return fail("dim and head_dim must be multiples of 8");
    int ndev = 0; HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev == 0) return fail("no HIP device: liblnb_hip.so has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    HIPCHK(lnbk_init());
    HIPCHK(lnbk_fast_init());
    HIPCHK(lnbk_batch_prepare());                                         // dynamic-LDS limits of the prefill / batch kernels, once, outside any capture (a prompt on a model without enable_batch reaches gemm_stream_kernel too)
    { hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, device)); if (prop.multiProcessorCount > 0) g_num_cus = prop.multiProcessorCount; }
    lnb_model* m = new lnb_model();
    m->a = a; m->device = device; m->layer_begin = layer_begin; m->layer_end = layer_end; m->part_begin = part_begin; m->part_end = part_end;
    m->head_dim = hd; m->n_rep = a.n_heads / a.n_kv_heads; m->ffn_hidden = lnb_model_ffn_hidden_dim(&a);
    m->q_dim = a.n_heads * hd; m->kv_dim = a.n_kv_heads * hd;
    if (m->ffn_hidden <= 0 || m->ffn_hidden % 8) { delete m; return fail("ffn hidden dim must be a positive multiple of 8"); }
    if (model_alloc(m)) { lnb_model_destroy(m); return -1; }             // (the error text survives: destroy does not touch it)
    *out = m;
    return 0;
}
static int wpack_refresh(lnb_model* m, const TiledDesc* t);
static int model_alloc(lnb_model* m) {
    const lnb_model_args& a = m->a;
    const int layer_begin = m->layer_begin, layer_end = m->layer_end;
    HIPCHK(stream_create(m->stream, hipStreamDefault));
    int64_t& wb = m->weight_bytes; DevArena& A = m->weights;
    const int dim = a.dim, F = m->ffn_hidden;
    if (m->first()) {
        if (alloc_linear(A, &m->tok_embd, (size_t)a.vocab_size * dim, wb)) return -1;
        reg_linear(m, "tok_embeddings.weight", m->tok_embd, dim, 0, 0, a.vocab_size, 2);
    }
    m->layers.resize(layer_end - layer_begin);
    // block heights of the resident layouts, each knob read once per model: 24-row wq|wk|wv blocks (gemv_quad_kernel) / 56-row gate|up blocks when that puts one block on every CU (the 8B shape)
    const int qkv_rows = m->q_dim + 2 * m->kv_dim, rwo = auto_rw(dim, Knob::RW_WO, m->q_dim, true), rw2 = auto_rw(dim, Knob::RW_W2, F, true);
    const int rwq = auto_rw(qkv_rows, Knob::RW_QKV, dim, false, qkv_rows == 24 * g_num_cus && gemv_layout_takes(24, dim) ? 24 : 0);
    const int rw13 = auto_rw(F, Knob::RW_W13, 0, false, F == 56 * g_num_cus ? 56 : 0);
    for (int l = layer_begin; l < layer_end; l++) {
        LayerW& L = m->layers[l - layer_begin];
        char nm[128]; uint32_t base = 16u * (uint32_t)(l + 1);
        if (m->has_attn(l)) {
            if (alloc_linear(A, &L.attn_norm, dim, wb)) return -1;
            if (alloc_tiled(A, L.wqkv, m->q_dim + 2 * m->kv_dim, dim, rwq, 1, wb)) return -1;
            if (alloc_tiled(A, L.wo, dim, m->q_dim, rwo, 1, wb)) return -1;
            snprintf(nm, sizeof nm, "layers.%d.attention_norm.weight", l); reg_linear(m, nm, L.attn_norm, dim, base + 0, 1);
            snprintf(nm, sizeof nm, "layers.%d.attention.wq.weight", l); reg_tiled(m, nm, &L.wqkv, m->q_dim, dim, 0, 0, base + 1);
            snprintf(nm, sizeof nm, "layers.%d.attention.wk.weight", l); reg_tiled(m, nm, &L.wqkv, m->kv_dim, dim, m->q_dim, 0, base + 2);
            snprintf(nm, sizeof nm, "layers.%d.attention.wv.weight", l); reg_tiled(m, nm, &L.wqkv, m->kv_dim, dim, m->q_dim + m->kv_dim, 0, base + 3);
            snprintf(nm, sizeof nm, "layers.%d.attention.wo.weight", l); reg_tiled(m, nm, &L.wo, dim, m->q_dim, 0, 0, base + 4);
        }
        if (m->has_w13(l)) {
            if (alloc_linear(A, &L.ffn_norm, dim, wb)) return -1;
            if (alloc_tiled(A, L.w13, F, dim, rw13, 2, wb)) return -1;
            snprintf(nm, sizeof nm, "layers.%d.ffn_norm.weight", l); reg_linear(m, nm, L.ffn_norm, dim, base + 5, 1);
            snprintf(nm, sizeof nm, "layers.%d.feed_forward.w1.weight", l); reg_tiled(m, nm, &L.w13, F, dim, 0, 0, base + 6);
            snprintf(nm, sizeof nm, "layers.%d.feed_forward.w3.weight", l); reg_tiled(m, nm, &L.w13, F, dim, 0, 1, base + 8);
        }
        if (m->has_w2(l)) {
            if (alloc_tiled(A, L.w2, dim, F, rw2, 1, wb)) return -1;
            snprintf(nm, sizeof nm, "layers.%d.feed_forward.w2.weight", l); reg_tiled(m, nm, &L.w2, dim, F, 0, 0, base + 7);
        }
    }
    if (m->last()) {
        if (alloc_linear(A, &m->norm, dim, wb)) return -1;
        reg_linear(m, "norm.weight", m->norm, dim, 1, 1);
        if (alloc_tiled(A, m->output, a.vocab_size, dim, auto_rw(a.vocab_size, Knob::RW_OUT), 1, wb)) return -1;
        reg_tiled(m, "output.weight", &m->output, a.vocab_size, dim, 0, 0, 2);
    }
    return 0;
}

static void append_many_free(lnb_model* m);
extern "C" int lnb_model_destroy(lnb_model* m) {
    if (!m) return 0;
    hipSetDevice(m->device);
    append_many_free(m);
    delete m;
    return 0;
}

extern "C" int64_t lnb_model_weight_bytes(lnb_model* m) { return m ? m->weight_bytes : 0; }

// ---- the 13-bit planar copy of the gate|up matrices (lnb_wpack.h) ----------------------------------
// Window of a resident matrix, on the device (no pass over the weights on the host): WPACK_* and *base
static int wpack_matrix_window(lnb_model* m, const TiledDesc& t, unsigned* d_stats, unsigned* base) {
    HIPCHK(lnbk_wpack_stats(t.w, tiled_elems(t.n_rows, t.k, t.rw, t.nch), d_stats, m->stream));
    WpackStats s;
    HIPCHK(hipMemcpyAsync(&s, d_stats, sizeof s, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return wpack_window(&s, base);
}
// lnb_model_finalize: every gate|up matrix in the 56-row layout that has no valid copy yet gets one, if it is packable and the memory is there;
// a matrix that is refused keeps the raw kernel and says why (lnb_model_wpack_info)
static int wpack_build(lnb_model* m) {
    Dev<unsigned> d_stats;
    for (int l = m->layer_begin; l < m->layer_end; l++) {
        LayerW& L = m->layers[l - m->layer_begin];
        if (!m->has_w13(l) || L.p_ok || L.w13.nch != 2 || !lnbk_w13p_supported(L.w13.rw, L.w13.k)) continue;
        if (!d_stats) HIPCHK(dev_alloc(d_stats, sizeof(WpackStats)));
        unsigned base = 0;
        const int why = wpack_matrix_window(m, L.w13, d_stats, &base);
        if (why < 0) return -1;
        L.p_status = why;
        if (why != WPACK_OK) continue;
        const size_t n = lnbk_wpack_w13_bytes(L.w13.n_blocks, L.w13.k);
        if (!L.p_w13) {
            if (dev_alloc(L.p_w13, n) != hipSuccess) { (void)hipGetLastError(); L.p_status = WPACK_NOMEM; continue; }     // the model runs raw and reports it
            m->wpack_bytes += (int64_t)n;
        }
        hipError_t e = lnbk_wpack_w13(L.w13.w, L.p_w13, L.w13.k, L.w13.n_blocks, base, m->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
        if (e != hipSuccess) return fail("packing the gate|up matrix of layer %d failed: %s", l, hipGetErrorString(e));
        L.p_base = base; L.p_ok = true;
    }
    return 0;
}
// A gate|up matrix was rewritten after its copy was built (t: that matrix; nullptr: all of them).  A captured decode step may hold the copy's address and
// window, so the copy is rebuilt IN PLACE when the new weights still fit its window; otherwise the layer returns to the raw kernel and the call fails, saying so.
static int wpack_refresh(lnb_model* m, const TiledDesc* t) {
    Dev<unsigned> d_stats; int rc = 0;
    for (int l = m->layer_begin; l < m->layer_end && !rc; l++) {
        LayerW& L = m->layers[l - m->layer_begin];
        if (!L.p_ok || (t && t != &L.w13)) continue;
        if (!d_stats && dev_alloc(d_stats, sizeof(WpackStats)) != hipSuccess) { (void)hipGetLastError(); L.p_ok = false; rc = fail("out of memory"); break; }
        L.p_ok = false;
        HIPCHK(lnbk_wpack_stats(L.w13.w, tiled_elems(L.w13.n_rows, L.w13.k, L.w13.rw, L.w13.nch), d_stats, m->stream));
        WpackStats s;
        HIPCHK(hipMemcpyAsync(&s, d_stats, sizeof s, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        unsigned base = 0;
        const int why = wpack_window(&s, &base);
        const bool fits = why == WPACK_OK && (s.max_e2 == 0 || (s.min_e2 > L.p_base && s.max_e2 <= L.p_base + 15));
        if (!fits) {
            L.p_status = why != WPACK_OK ? why : WPACK_WINDOW;
            rc = fail("layer %d: the gate|up weights bound after lnb_model_finalize do not fit the window of the matrix's 13-bit copy; the layer decodes from the raw "
                      "weights from now on (a decode step captured before keeps the old copy: bind every tensor before lnb_model_finalize)", l);
            break;
        }
        HIPCHK(lnbk_wpack_w13(L.w13.w, L.p_w13, L.w13.k, L.w13.n_blocks, L.p_base, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        L.p_ok = true; L.p_status = WPACK_OK;
    }
    return rc;
}
// ---- the LM head's copy: the same format cut into 128-row two-chain blocks (lnb_wpack.h; lnbk_gemv_headp) ----
// The head has a packed form when its resident layout is the 64-row one, the row fits the 128-step stages (K = 8192 does not) and the vocabulary gives every
// CU at least one 128-row block: below that the launch is a few microseconds and the copy buys nothing.
static bool head_pack_applies(const lnb_model* m) {
    return m->last() && m->output.w && m->output.rw == 64 && m->output.nch == 1 && lnbk_headp_supported(m->output.k) && m->output.n_rows >= 128 * g_num_cus;
}
// lnb_model_finalize: build the copy if the head has none that is valid; a refusal keeps the raw kernel and records why (lnb_model_wpack_head_status)
static int wpack_head_build(lnb_model* m) {
    if (m->p_out_ok || !head_pack_applies(m)) return 0;
    const TiledDesc& t = m->output;
    Dev<unsigned> d_stats; unsigned base = 0;
    HIPCHK(dev_alloc(d_stats, sizeof(WpackStats)));
    const int why = wpack_matrix_window(m, t, d_stats, &base);
    d_stats.reset();
    if (why < 0) return -1;
    m->p_out_status = why;
    if (why != WPACK_OK) return 0;
    const size_t n = lnbk_wpack_head_bytes(t.n_rows, t.k);
    if (!m->p_out) {
        if (dev_alloc(m->p_out, n) != hipSuccess) { (void)hipGetLastError(); m->p_out_status = WPACK_NOMEM; return 0; }      // the head runs raw and reports it
        m->wpack_head_bytes = (int64_t)n;
    }
    hipError_t e = lnbk_wpack_head(t.w, m->p_out, t.n_rows, t.k, base, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) return fail("packing the LM head failed: %s", hipGetErrorString(e));
    m->p_out_base = base; m->p_out_ok = true;
    return 0;
}
// output.weight was rewritten after its copy was built: as wpack_refresh -- rebuilt in place inside the copy's window, or back to the raw kernel and an error
static int wpack_head_refresh(lnb_model* m) {
    if (!m->p_out_ok) return 0;
    m->p_out_ok = false;
    Dev<unsigned> d_stats;
    if (dev_alloc(d_stats, sizeof(WpackStats)) != hipSuccess) { (void)hipGetLastError(); return fail("out of memory"); }
    const TiledDesc& t = m->output;
    WpackStats s;
    HIPCHK(lnbk_wpack_stats(t.w, tiled_elems(t.n_rows, t.k, t.rw, t.nch), d_stats, m->stream));
    HIPCHK(hipMemcpyAsync(&s, d_stats, sizeof s, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    d_stats.reset();
    unsigned base = 0;
    const int why = wpack_window(&s, &base);
    const bool fits = why == WPACK_OK && (s.max_e2 == 0 || (s.min_e2 > m->p_out_base && s.max_e2 <= m->p_out_base + 15));
    if (!fits) {
        m->p_out_status = why != WPACK_OK ? why : WPACK_WINDOW;
        return fail("the output.weight bound after lnb_model_finalize does not fit the window of the LM head's 13-bit copy; the head decodes from the raw weights "
                    "from now on (a decode step captured before keeps the old copy: bind every tensor before lnb_model_finalize)");
    }
    HIPCHK(lnbk_wpack_head(t.w, m->p_out, t.n_rows, t.k, m->p_out_base, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->p_out_ok = true; m->p_out_status = WPACK_OK;
    return 0;
}
extern "C" int64_t lnb_model_wpack_head_bytes(lnb_model* m) { return m ? m->wpack_head_bytes : 0; }
// 0: the one-token head streams its 13-bit copy; WPACK_SUBNORMAL .. WPACK_NOMEM (1..4): refused for that reason; 5: never tried (LNB_HEAD_PACKED=0 at
// lnb_model_finalize, a stage without output.weight, or a shape the packed head has no form for); -1: null argument
extern "C" int lnb_model_wpack_head_status(lnb_model* m) {
    if (!m) return fail("null argument");
    return m->p_out_ok ? 0 : (m->p_out_status > 0 && m->p_out_status <= WPACK_NOMEM) ? m->p_out_status : 5;
}
extern "C" int64_t lnb_model_wpack_bytes(lnb_model* m) { return m ? m->wpack_bytes : 0; }
// counts[0] = gate|up matrices decoding from their 13-bit copy, counts[WPACK_SUBNORMAL / WPACK_INFNAN / WPACK_WINDOW / WPACK_NOMEM] = matrices refused for that
// reason, counts[5] = matrices never tried (LNB_W13_PACKED=0 at lnb_model_finalize, or a layout the packed kernel has no form for)
extern "C" int lnb_model_wpack_info(lnb_model* m, int32_t* counts6) {
    if (!m || !counts6) return fail("null argument");
    for (int i = 0; i < 6; i++) counts6[i] = 0;
    for (int l = m->layer_begin; l < m->layer_end; l++) {
        const LayerW& L = m->layers[l - m->layer_begin];
        if (!m->has_w13(l)) continue;
        counts6[L.p_ok ? 0 : (L.p_status > 0 && L.p_status <= WPACK_NOMEM) ? L.p_status : 5]++;
    }
    return 0;
}

extern "C" int lnb_model_set_tensor(lnb_model* m, const char* name, const uint16_t* host, const int64_t* shape, int rank) {
    if (!m || !name || !host || !shape) return fail("null argument");
    HIPCHK(hipSetDevice(m->device));
    auto it = m->tensors.find(name);
    if (it == m->tensors.end()) return fail("tensor \"%s\" does not belong to this model stage", name);
    if (m->batch_enabled) return fail("tensor \"%s\": the model's batched-decode copy has been built; bind tensors before lnb_model_enable_batch", name);
    TensorRef& r = it->second;
    // shape check as loader.go:183-192
    if (rank != r.rank || (rank == 1 && shape[0] != r.cols) || (rank == 2 && (shape[0] != r.rows || shape[1] != r.cols)))
        return fail("tensor \"%s\": shape mismatch, expected [%d%s%d]", name, r.rank == 1 ? r.cols : r.rows, r.rank == 1 ? "" : " ", r.rank == 1 ? 0 : r.cols);
    size_t n = (size_t)r.rows * r.cols;
    if (!r.tiled) { HIPCHK(hipMemcpy(r.linear, host, n * 2, hipMemcpyHostToDevice)); return 0; }
    Dev<uint16_t> stage;
    HIPCHK(dev_alloc(stage, n * 2));
    HIPCHK(hipMemcpy(stage, host, n * 2, hipMemcpyHostToDevice));
    HIPCHK(lnbk_tile(stage, r.td->w, r.rows, r.cols, r.row_off, r.chain, r.td->rw, r.td->nch, 0, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    stage.reset();
    if (wpack_refresh(m, r.td)) return -1;
    if (r.td == &m->output && wpack_head_refresh(m)) return -1;
    return 0;
}

// enumerate the tensors this model stage binds (names as in the checkpoint, shapes as getTensor expects them)
extern "C" int lnb_model_num_tensors(const lnb_model* m) { return m ? (int)m->tensors.size() : 0; }
extern "C" int lnb_model_tensor_info(const lnb_model* m, int k, const char** name, int64_t* shape, int* rank) {
    if (!m || k < 0 || k >= (int)m->tensors.size()) return fail("tensor index %d out of range", k);
    auto it = m->tensors.begin();
    std::advance(it, k);
    if (name) *name = it->first.c_str();
    if (rank) *rank = it->second.rank;
    if (shape) { if (it->second.rank == 1) shape[0] = it->second.cols; else { shape[0] = it->second.rows; shape[1] = it->second.cols; } }
    return 0;
}

extern "C" int lnb_model_get_tensor(lnb_model* m, const char* name, uint16_t* host, int64_t nelem) {
    if (!m || !name || !host) return fail("null argument");
    HIPCHK(hipSetDevice(m->device));
    auto it = m->tensors.find(name);
    if (it == m->tensors.end()) return fail("tensor \"%s\" does not belong to this model stage", name);
    TensorRef& r = it->second;
    size_t n = (size_t)r.rows * r.cols;
    if ((int64_t)n != nelem) return fail("tensor \"%s\": expected %zu elements", name, n);
    if (!r.tiled) { HIPCHK(hipMemcpy(host, r.linear, n * 2, hipMemcpyDeviceToHost)); return 0; }
    Dev<uint16_t> stage;
    HIPCHK(dev_alloc(stage, n * 2));
    HIPCHK(lnbk_tile(r.td->w, stage, r.rows, r.cols, r.row_off, r.chain, r.td->rw, r.td->nch, 1, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipMemcpy(host, stage, n * 2, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lnb_model_fill_synthetic(lnb_model* m, uint64_t seed) {
    if (!m) return fail("null argument");
    if (m->batch_enabled) return fail("the model's batched-decode copy has been built; fill the weights before lnb_model_enable_batch");
    HIPCHK(hipSetDevice(m->device));
    for (auto& kv : m->tensors) {
        TensorRef& r = kv.second;
        if (r.tiled) HIPCHK(lnbk_synth_fill(r.td->w, r.rows, r.cols, r.row_off, r.chain, r.td->rw, r.td->nch, seed, r.synth_id, 0, 0.02f, m->stream));
        else HIPCHK(lnbk_synth_fill(r.linear, r.rows, r.cols, 0, 0, 0, 1, seed, r.synth_id, r.synth_kind, 0.02f, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    if (wpack_refresh(m, nullptr)) return -1;
    if (wpack_head_refresh(m)) return -1;
    return 0;
}

// precomputeFreqsCis + applyScaling (llamatransformer.go:662-751): host-side, f32 arithmetic with bf16
// truncation of freqs, positions and angles; cos/sin in f64.  (Independent restatement: the oracle has its own.)
static void build_rope_table(int head_dim, int rows, double theta, bool scaled, std::vector<float>& cis) {
    const int n = head_dim / 2;
    std::vector<uint16_t> freqs(n);
    const float dimf = (float)head_dim;
    for (int i = 0; i < n; i++) {
        float val = bf_wide_h(bf_trunc_h((float)(2 * i)));
        freqs[i] = bf_trunc_h((float)(1.0 / std::pow(theta, (double)(val / dimf))));
    }
    if (scaled) {
        const float scale_factor = 8.0f, low_freq_factor = 1.0f, high_freq_factor = 4.0f, old_context_len = 8192.0f;
        const float low_freq_wavelen = old_context_len / low_freq_factor, high_freq_wavelen = old_context_len / high_freq_factor;
        for (int i = 0; i < n; i++) {
            volatile float freq = bf_wide_h(freqs[i]);
            volatile float wavelen = (float)(2 * M_PI) / freq;
            float nf;
            if (wavelen < high_freq_wavelen) nf = freq;
            else if (wavelen > low_freq_wavelen) nf = freq / scale_factor;
            else {
                volatile float smooth = (old_context_len / wavelen - low_freq_factor) / (high_freq_factor - low_freq_factor);
                volatile float t1 = (1 - smooth) * freq; t1 = t1 / scale_factor;
                volatile float t2 = smooth * freq;
                nf = t1 + t2;
            }
            freqs[i] = bf_trunc_h(nf);
        }
    }
    cis.resize((size_t)rows * n * 2);
    for (int p = 0; p < rows; p++) {
        const float t = bf_wide_h(bf_trunc_h((float)p));
        for (int i = 0; i < n; i++) {
            volatile float prod = t * bf_wide_h(freqs[i]);
            const double ang = (double)bf_wide_h(bf_trunc_h(prod));
            cis[((size_t)p * n + i) * 2 + 0] = (float)std::cos(ang);
            cis[((size_t)p * n + i) * 2 + 1] = (float)std::sin(ang);
        }
    }
}

static void prob_exp_table(std::vector<double>& et) {
    et.resize(1 << 16);
    for (int i = 0; i < (1 << 16); i++) et[i] = std::exp((double)bf_wide_h((uint16_t)i));
}
extern "C" int lnb_model_finalize(lnb_model* m, int rope_rows) {
    if (!m) return fail("null argument");
    HIPCHK(hipSetDevice(m->device));
    m->cis_rows = rope_rows > 0 ? rope_rows : m->a.max_seq_len * 2;           // llamatransformer.go:109
    build_rope_table(m->head_dim, m->cis_rows, m->a.rope_theta, m->a.use_scaled_rope != 0, m->cis_host);
    HIPCHK(dev_alloc(m->cis, m->cis_host.size() * 4));             // (a second call: the old table goes first)
    HIPCHK(hipMemcpy(m->cis, m->cis_host.data(), m->cis_host.size() * 4, hipMemcpyHostToDevice));
    // TABLE_SILU (activations.go:15-25): f32(x / (1 + exp(-x))) in f64 for every bf16 bit pattern
    std::vector<float> silu(1 << 16);
    for (int i = 0; i < (1 << 16); i++) { double x = (double)bf_wide_h((uint16_t)i); silu[i] = (float)(x / (1.0 + std::exp(-x))); }
    if (!m->silu) HIPCHK(dev_alloc(m->silu, silu.size() * 4));
    HIPCHK(hipMemcpy(m->silu, silu.data(), silu.size() * 4, hipMemcpyHostToDevice));
    // token probabilities: exp(double(bf16)) with the host C library's exp, the oracle's (orc_softmax_f32) by construction
    std::vector<double> et;
    prob_exp_table(et);
    if (!m->prob_etab) HIPCHK(dev_alloc(m->prob_etab, et.size() * 8));
    HIPCHK(hipMemcpy(m->prob_etab, et.data(), et.size() * 8, hipMemcpyHostToDevice));
    if (!m->exp_tab) HIPCHK(dev_alloc(m->exp_tab, (size_t)(1 << 16) * 8));
    HIPCHK(lnbk_exp_table(m->exp_tab, bf_wide_h(bf_trunc_h((float)std::sqrt((double)m->head_dim))), m->stream));   // (attn_mfma_kernel)
    HIPCHK(hipStreamSynchronize(m->stream));
    if (knob(Knob::W13_PACKED) && wpack_build(m)) return -1;
    if (knob(Knob::HEAD_PACKED) && wpack_head_build(m)) return -1;
    m->finalized = true;
    return 0;
}

extern "C" int lnb_model_rope_table(lnb_model* m, float* out, int64_t nfloats, int* rows_out) {
    if (!m || !m->finalized) return fail("model not finalized");
    if (rows_out) *rows_out = m->cis_rows;
    if (out) {
        if ((size_t)nfloats != m->cis_host.size()) return fail("rope table has %zu floats", m->cis_host.size());
        memcpy(out, m->cis_host.data(), m->cis_host.size() * 4);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
static int ctx_alloc(lnb_ctx* c);
// the common path of lnb_ctx_create / lnb_ctx_create_long (seq_len already resolved and checked against the caller's cap)
static int ctx_create_common(lnb_model* m, int seq_len, int max_rows, lnb_ctx** out) {
    if (m->head_dim != 128 && m->head_dim != 64 && m->head_dim != 32) return fail("head_dim %d not one of 32/64/128", m->head_dim);
    lnb_ctx* c = new lnb_ctx();
    c->m = m; c->seq_len = seq_len; c->max_rows = max_rows > 0 && max_rows < seq_len ? max_rows : seq_len;
    if (ctx_alloc(c)) { lnb_ctx_destroy(c); return -1; }
    *out = c;
    return 0;
}
extern "C" int lnb_ctx_create(lnb_model* m, int seq_len, lnb_ctx** out) {
    if (!m || !out) return fail("null argument");
    *out = nullptr;
    if (!m->finalized) return fail("model not finalized");
    HIPCHK(hipSetDevice(m->device));
    const int sl = seq_len > 0 ? seq_len : m->a.max_seq_len;                 // inferencecontext.go:22-26
    // Context length: one-token calls above the attention crossover and calls of 16 or more rows run kernels without a per-position LDS
    // array that would not fit (the long-context PV kernel keeps 4 bytes per position: ~23 K positions); the one-workgroup-per-head kernel
    // (12 bytes per position: ~7.8 K at head_dim 128) then only serves calls of 2..15 rows, which fail beyond its reach (lnb.h).
    // This entry point keeps that cap (and the per-position layout of the PV kernel below it); lnb_ctx_create_long goes beyond.
    if (m->head_dim != 128 && m->head_dim != 64 && m->head_dim != 32) return fail("head_dim %d not one of 32/64/128", m->head_dim);
    if (lnbk_attn_long_lds(sl) > 160 * 1024)
        return fail("seq_len %d too long for the LDS staging of the attention kernels (about 23000 positions)", sl);
    return ctx_create_common(m, sl, 0, out);
}
// Up to LNB_MAX_SEQ_LEN positions: beyond lnb_ctx_create's cap the long-context PV launch takes the layout whose LDS does not grow with the context
// (lnb_kernels.hip: alp_pw_floats), chosen per launch from the capacity -- a long context below the cap launches exactly what lnb_ctx_create's would.
// max_rows sizes the per-call activation buffers; the caches, the token words and log, e_buf and z_part stay sized by seq_len.
extern "C" int lnb_ctx_create_long(lnb_model* m, int seq_len, int max_rows, lnb_ctx** out) {
    if (!m || !out) return fail("null argument");
    *out = nullptr;
    if (!m->finalized) return fail("model not finalized");
    HIPCHK(hipSetDevice(m->device));
    const int sl = seq_len > 0 ? seq_len : m->a.max_seq_len;
    if (sl > LNB_MAX_SEQ_LEN) return fail("seq_len %d too long: a long context holds at most %d positions", sl, LNB_MAX_SEQ_LEN);
    if (sl > m->cis_rows)
        return fail("seq_len %d is beyond the model's %d-row RoPE table: pass rope_rows >= %d to lnb_model_finalize", sl, m->cis_rows, sl);
    return ctx_create_common(m, sl, max_rows, out);
}
extern "C" int lnb_ctx_max_rows(const lnb_ctx* c, int* out) {
    if (!c || !out) return fail("null argument");
    *out = c->max_rows;
    return 0;
}
static int ctx_alloc(lnb_ctx* c) {
    lnb_model* m = c->m;
    // a NON-blocking stream: it never synchronises with the legacy (null) stream.  Contexts are driven from several host threads at
    // once (one per generation); with a blocking stream, one thread's graph capture made any other thread's null-stream call
    // (hipMemcpy, hipMemset) fail with "would make the legacy stream depend on a capturing blocking stream".  Everything a context
    // does is therefore ordered on ITS stream: asynchronous copies and memsets + a stream synchronise, never the null stream.
    HIPCHK(stream_create(c->stream, hipStreamNonBlocking));
    HIPCHK(event_create(c->ev0)); HIPCHK(event_create(c->ev1));
    HIPCHK(pinned_alloc(c->h_io, ((size_t)c->seq_len + 2) * 4, hipHostMallocDefault));
    const size_t kvn = (size_t)c->seq_len * m->kv_dim;
    c->ck.resize(m->layers.size()); c->cv.resize(m->layers.size());
    for (size_t l = 0; l < m->layers.size(); l++) {
        if (!m->has_attn(m->layer_begin + (int)l)) continue;               // a stage that holds only FFN parts of a block keeps no cache for it
        HIPCHK(dev_alloc(c->ck[l], kvn * 2)); HIPCHK(dev_alloc(c->cv[l], kvn * 2));
        HIPCHK(hipMemsetAsync(c->ck[l], 0, kvn * 2, c->stream)); HIPCHK(hipMemsetAsync(c->cv[l], 0, kvn * 2, c->stream));     // ml.Zeros, inferencecontext.go:32-42
    }
    HIPCHK(dev_alloc(c->st, sizeof(StepState))); HIPCHK(hipMemsetAsync(c->st, 0, sizeof(StepState), c->stream));
    HIPCHK(dev_alloc(c->dtok, (size_t)c->seq_len * 4));
    HIPCHK(dev_alloc(c->dnext, 16)); HIPCHK(dev_alloc(c->derr, 16)); HIPCHK(hipMemsetAsync(c->derr, 0, 16, c->stream));
    c->dout_cap = c->seq_len; HIPCHK(dev_alloc(c->dout, (size_t)c->dout_cap * 4));
    const size_t S = c->max_rows;                            // rows per call (lnb_ctx_create: seq_len)
    HIPCHK(dev_alloc(c->x, S * m->a.dim * 2)); HIPCHK(dev_alloc(c->h, S * m->a.dim * 2));
    HIPCHK(dev_alloc(c->xn, S * m->a.dim * 2));
    HIPCHK(dev_alloc(c->q, S * m->q_dim * 2)); HIPCHK(dev_alloc(c->att, S * m->q_dim * 2));
    HIPCHK(dev_alloc(c->ffn, S * m->ffn_hidden * 2));
    if (m->last()) { HIPCHK(dev_alloc(c->logits, (size_t)m->a.vocab_size * 2)); c->logits_rows = 1; }
    const size_t SL = c->seq_len;
    HIPCHK(dev_alloc(c->e_buf, (size_t)m->a.n_heads * SL * 8));
    HIPCHK(dev_alloc(c->z_part, (size_t)m->a.n_heads * ((SL + 63) / 64 + 8) * 8));     // (two-launch form: one partial per 256 positions; attn_one_kernel: one per 64)
    HIPCHK(dev_alloc(c->zseq_count, 16)); HIPCHK(hipMemsetAsync(c->zseq_count, 0, 16, c->stream));      // [0] serial-sum walks, [1] norm fallbacks, [2] token-probability walks, [3] sticky: a cached row holds an inf or a NaN
    HIPCHK(dev_alloc(c->attn_cnt, ((size_t)m->a.n_heads + 4) * 4)); HIPCHK(hipMemsetAsync(c->attn_cnt, 0, ((size_t)m->a.n_heads + 4) * 4, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // crossover measured on MI355X (tools/att_timing.py): the one-workgroup-per-head kernel wins below a few hundred positions
    c->attn_long_T = knob(Knob::ATTN_LONG_T);
    c->attn_short_cap = lnbk_attn_short_max_T(m->head_dim);
    c->rows_T = c->attn_short_cap;
    return 0;
}

extern "C" int lnb_ctx_destroy(lnb_ctx* c) {
    if (!c) return 0;
    // a batch bakes its members' device pointers (state words, token words, caches) into its tables and captured graphs: freeing a member
    // under it would make the next lnb_batch_decode / lnb_pipeline_tick_batch read and write freed memory.  Destroy the batch first.
    if (c->batch_users > 0) return fail("context is a member of %d live batch(es): lnb_batch_destroy them first", c->batch_users);
    hipSetDevice(c->m->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (lnb_batch* b : c->sp_b) if (b) lnb_batch_destroy(b);      // the verify batches: their tables hold this context's pointers
    delete c;
    return 0;
}

extern "C" int lnb_ctx_reset(lnb_ctx* c) {
    if (!c) return fail("null argument");
    HIPCHK(hipSetDevice(c->m->device));
    const size_t kvn = (size_t)c->seq_len * c->m->kv_dim;
    for (size_t l = 0; l < c->ck.size(); l++) if (c->ck[l]) { HIPCHK(hipMemsetAsync(c->ck[l], 0, kvn * 2, c->stream)); HIPCHK(hipMemsetAsync(c->cv[l], 0, kvn * 2, c->stream)); }
    HIPCHK(hipMemsetAsync(c->zseq_count + 3, 0, 4, c->stream));      // no cached row holds an inf or a NaN any more
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int lnb_ctx_read_kv(lnb_ctx* c, int layer, int which, uint16_t* host) {
    if (!c || !host) return fail("null argument");
    HIPCHK(hipSetDevice(c->m->device));
    if (layer < c->m->layer_begin || layer >= c->m->layer_end || !c->m->has_attn(layer)) return fail("layer %d is not owned by this stage", layer);
    const size_t kvn = (size_t)c->seq_len * c->m->kv_dim;
    if (which) { HIPCHK(hipMemcpyAsync(host, c->cv[layer - c->m->layer_begin], kvn * 2, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); return 0; }
    // K lives as [kv head][d/8][position][8] on the device; hand it back in the reference's [position][kv head][d] order
    std::vector<uint16_t> raw(kvn);
    HIPCHK(hipMemcpyAsync(raw.data(), c->ck[layer - c->m->layer_begin], kvn * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int hd = c->m->head_dim, nk = hd >> 3, KVH = c->m->kv_dim / hd;
    for (int j = 0; j < c->seq_len; j++)
        for (int kh = 0; kh < KVH; kh++)
            for (int d = 0; d < hd; d++)
                host[(size_t)j * c->m->kv_dim + kh * hd + d] = raw[(((size_t)kh * nk + (d >> 3)) * c->seq_len + j) * 8 + (d & 7)];
    return 0;
}

// ---- a computed prefix shared between contexts: lnb_ctx_fork, lnb_ctx_save_prefix / lnb_ctx_load_prefix (include/lnb.h, lnb_kvcopy.h) ----------------
// A KV row depends on the tokens up to it and on nothing a context owns, so the rows [0, n_pos) of one context ARE the rows any
// other context of the same model would compute for that text: sharing them is a copy.  Nothing but cache rows moves -- every entry point
// re-establishes the device position itself -- and no captured graph bakes in cache CONTENTS, so none is dropped.
static int cached_layers(const lnb_ctx* c) { int n = 0; for (const auto& p : c->ck) n += p.get() != nullptr; return n; }
extern "C" int lnb_ctx_fork(lnb_ctx* src, int n_pos, lnb_ctx* const* dsts, int n_dst) {
    if (!src || !dsts) return fail("null argument");
    if (n_dst < 1 || n_dst > LNB_MAX_FORK) return fail("n_dst %d is outside 1..%d", n_dst, LNB_MAX_FORK);
    if (n_pos < 0) return fail("negative n_pos %d", n_pos);
    for (int d = 0; d < n_dst; d++) {
        if (!dsts[d]) return fail("destination %d is NULL", d);
        if (dsts[d] == src) return fail("destination %d is the source", d);
        for (int e = 0; e < d; e++) if (dsts[e] == dsts[d]) return fail("destinations %d and %d are the same context", e, d);
    }
    if (n_pos > src->seq_len) return fail("n_pos %d is beyond the source's %d positions", n_pos, src->seq_len);
    if (src->pending) return fail("source: a lnb_forward_stage_begin has not been ended");
    for (int d = 0; d < n_dst; d++) {
        if (dsts[d]->m != src->m) return fail("destination %d belongs to another lnb_model handle: a stage's contexts fork among themselves", d);
        if (n_pos > dsts[d]->seq_len) return fail("n_pos %d is beyond the %d positions of destination %d", n_pos, dsts[d]->seq_len, d);
        if (dsts[d]->pending) return fail("destination %d: a lnb_forward_stage_begin has not been ended", d);
    }
    const lnb_model* m = src->m;
    const int n_arrays = 2 * cached_layers(src);
    if (n_pos == 0 || n_arrays == 0) return 0;
    HIPCHK(hipSetDevice(m->device));
    const bool engine = knob(Knob::FORK_COPY) != 0;
    const size_t ptr_bytes = (size_t)n_arrays * (size_t)(1 + n_dst) * sizeof(void*), tab_bytes = ptr_bytes + (size_t)n_dst * sizeof(int);
    if (!engine && !src->fork_tab.fits(tab_bytes)) {               // before any copy is enqueued: a failure here leaves the caches as they were
        if (src->fork_tab) hipStreamSynchronize(src->stream);      // (the old table: nothing of a finished call reads it)
        if (dev_reserve(src->fork_tab, tab_bytes) != hipSuccess) { (void)hipGetLastError(); return fail("no device memory for the fork table (%zu bytes)", tab_bytes); }
    }
    HIPCHK(hipStreamSynchronize(src->stream));
    for (int d = 0; d < n_dst; d++) HIPCHK(hipStreamSynchronize(dsts[d]->stream));
    if (engine) {
        form_ran(Form::KV_FORK_COPY);
        const size_t runs = kvc_runs(0, m->kv_dim), width = kvc_byte_offset(kvc_run_len(0, m->kv_dim, n_pos)), v_bytes = kvc_byte_offset(kvc_run_len(1, m->kv_dim, n_pos));
        for (size_t l = 0; l < src->ck.size(); l++) {
            if (!src->ck[l]) continue;
            for (int d = 0; d < n_dst; d++) {
                HIPCHK(hipMemcpy2DAsync(dsts[d]->ck[l], kvc_byte_offset(kvc_stride(0, dsts[d]->seq_len)), src->ck[l], kvc_byte_offset(kvc_stride(0, src->seq_len)),
                                        width, runs, hipMemcpyDeviceToDevice, src->stream));
                HIPCHK(hipMemcpyAsync(dsts[d]->cv[l], src->cv[l], v_bytes, hipMemcpyDeviceToDevice, src->stream));
            }
        }
        for (int d = 0; d < n_dst; d++) HIPCHK(lnbk_nonfinite_or(dsts[d]->zseq_count + 3, src->zseq_count + 3, src->stream));
        HIPCHK(hipStreamSynchronize(src->stream));
        return 0;
    }
    std::vector<char> host(tab_bytes);
    const void** hp = (const void**)host.data();
    int* hc = (int*)(host.data() + ptr_bytes);
    size_t a = 0;
    for (size_t l = 0; l < src->ck.size(); l++) {
        if (!src->ck[l]) continue;
        for (int which = 0; which < 2; which++, a++) {
            const void** row = hp + a * (size_t)(1 + n_dst);
            row[0] = which ? src->cv[l] : src->ck[l];
            for (int d = 0; d < n_dst; d++) row[1 + d] = which ? dsts[d]->cv[l] : dsts[d]->ck[l];
        }
    }
    for (int d = 0; d < n_dst; d++) hc[d] = dsts[d]->seq_len;
    // (the upload reads `host`: every way out of this function from here on goes through a stream synchronise first)
    const hipError_t up = hipMemcpyAsync(src->fork_tab, host.data(), tab_bytes, hipMemcpyHostToDevice, src->stream);
    if (up != hipSuccess) { hipStreamSynchronize(src->stream); return fail("uploading the fork table failed: %s", hipGetErrorString(up)); }
    KvForkTab tab;
    tab.ptrs = (const void* const*)src->fork_tab.get(); tab.cap_dst = (const int*)(src->fork_tab.get() + ptr_bytes);
    tab.n_arrays = n_arrays; tab.n_dst = n_dst; tab.kv_dim = m->kv_dim; tab.n_pos = n_pos; tab.cap_src = src->seq_len;
    const hipError_t launched = lnbk_kv_fork(&tab, knob(Knob::FORK_NT), knob(Knob::FORK_SPLIT), src->stream);
    for (int d = 0; d < n_dst; d++) (void)lnbk_nonfinite_or(dsts[d]->zseq_count + 3, src->zseq_count + 3, src->stream);      // the word travels with the rows
    HIPCHK(hipStreamSynchronize(src->stream));
    if (launched != hipSuccess) return fail("kv_fork_kernel could not be launched: %s", hipGetErrorString(launched));
    return 0;
}

// The saved prefix: a 64-byte little-endian header, then per cached layer K as [kv head][head_dim/8][n_pos][8] (the device layout of a context of
// capacity n_pos) and V as [n_pos][kv_dim].  Header: bytes 0..7 "LNBKV1" + two zero bytes, then seven 32-bit words -- format version, n_pos, part_begin, part_end,
// n_kv_heads, head_dim, cached layers -- and 28 reserved zero bytes.
#define LNB_KV_BLOB_HEADER 64
#define LNB_KV_BLOB_VERSION 1
static const char LNB_KV_MAGIC[8] = {'L', 'N', 'B', 'K', 'V', '1', 0, 0};
static void put_le32(unsigned char* p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24); }
static uint32_t get_le32(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static int64_t prefix_bytes(const lnb_ctx* c, int n_pos) { return LNB_KV_BLOB_HEADER + (int64_t)cached_layers(c) * (int64_t)kvc_layer_bytes(c->m->kv_dim, n_pos); }
extern "C" int64_t lnb_ctx_prefix_bytes(const lnb_ctx* c, int n_pos) {
    if (!c) return fail("null argument");
    if (n_pos < 0 || n_pos > c->seq_len) return fail("n_pos %d is outside the context's 0..%d positions", n_pos, c->seq_len);
    return prefix_bytes(c, n_pos);
}
// the strided copies of one cached layer between the device caches and the blob's arrays at p (to_host: device -> blob)
static int prefix_copy_layer(lnb_ctx* c, size_t l, int n_pos, unsigned char* p, bool to_host) {
    const int kv_dim = c->m->kv_dim;
    const size_t runs = kvc_runs(0, kv_dim), width = kvc_byte_offset(kvc_run_len(0, kv_dim, n_pos)), pitch = kvc_byte_offset(kvc_stride(0, c->seq_len));
    const size_t v_bytes = kvc_byte_offset(kvc_run_len(1, kv_dim, n_pos));
    unsigned char* pv = p + runs * width;
    if (to_host) {
        HIPCHK(hipMemcpy2DAsync(p, width, c->ck[l], pitch, width, runs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(pv, c->cv[l], v_bytes, hipMemcpyDeviceToHost, c->stream));
    } else {
        HIPCHK(hipMemcpy2DAsync(c->ck[l], pitch, p, width, width, runs, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->cv[l], pv, v_bytes, hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}
extern "C" int lnb_ctx_save_prefix(lnb_ctx* c, int n_pos, void* host, int64_t cap) {
    if (!c || !host) return fail("null argument");
    if (n_pos < 0 || n_pos > c->seq_len) return fail("n_pos %d is outside the context's 0..%d positions", n_pos, c->seq_len);
    if (c->pending) return fail("a lnb_forward_stage_begin has not been ended");
    const int64_t need = prefix_bytes(c, n_pos);
    if (cap < need) return fail("the buffer holds %lld bytes, %d positions take %lld (lnb_ctx_prefix_bytes)", (long long)cap, n_pos, (long long)need);
    const lnb_model* m = c->m;
    unsigned char* p = (unsigned char*)host;
    memset(p, 0, LNB_KV_BLOB_HEADER);
    memcpy(p, LNB_KV_MAGIC, 8);
    const uint32_t words[7] = {LNB_KV_BLOB_VERSION, (uint32_t)n_pos, (uint32_t)m->part_begin, (uint32_t)m->part_end, (uint32_t)(m->kv_dim / m->head_dim), (uint32_t)m->head_dim, (uint32_t)cached_layers(c)};
    for (int i = 0; i < 7; i++) put_le32(p + 8 + 4 * i, words[i]);
    if (n_pos == 0) return 0;
    HIPCHK(hipSetDevice(m->device));
    p += LNB_KV_BLOB_HEADER;
    for (size_t l = 0; l < c->ck.size(); l++) {
        if (!c->ck[l]) continue;
        if (prefix_copy_layer(c, l, n_pos, p, true)) { hipStreamSynchronize(c->stream); return -1; }
        p += kvc_layer_bytes(m->kv_dim, n_pos);
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int lnb_ctx_load_prefix(lnb_ctx* c, const void* host, int64_t nbytes, int* n_pos_out) {
    if (!c || !host) return fail("null argument");
    if (nbytes < LNB_KV_BLOB_HEADER) return fail("a saved prefix has a %d-byte header, this blob has %lld bytes", LNB_KV_BLOB_HEADER, (long long)nbytes);
    const unsigned char* p = (const unsigned char*)host;
    if (memcmp(p, LNB_KV_MAGIC, 8)) return fail("not a saved prefix: the magic is not LNBKV1");
    uint32_t w[7];
    for (int i = 0; i < 7; i++) w[i] = get_le32(p + 8 + 4 * i);
    if (w[0] != LNB_KV_BLOB_VERSION) return fail("saved prefix of format version %u, this library reads version %d", w[0], LNB_KV_BLOB_VERSION);
    const lnb_model* m = c->m;
    if (w[2] != (uint32_t)m->part_begin || w[3] != (uint32_t)m->part_end)
        return fail("the saved prefix is of stage parts [%u, %u), the context's model of [%d, %d)", w[2], w[3], m->part_begin, m->part_end);
    if (w[4] != (uint32_t)(m->kv_dim / m->head_dim) || w[5] != (uint32_t)m->head_dim || w[6] != (uint32_t)cached_layers(c))
        return fail("the saved prefix has %u KV heads of head_dim %u in %u cached layers, the context's model %d of %d in %d", w[4], w[5], w[6],
                    m->kv_dim / m->head_dim, m->head_dim, cached_layers(c));
    if (w[1] > (uint32_t)LNB_MAX_SEQ_LEN) return fail("the saved prefix claims %u positions", w[1]);
    const int n_pos = (int)w[1];
    const int64_t need = prefix_bytes(c, n_pos);
    if (nbytes != need) return fail("a saved prefix of %d positions takes %lld bytes, this blob has %lld", n_pos, (long long)need, (long long)nbytes);
    if (n_pos > c->seq_len) return fail("the saved prefix holds %d positions, the context %d", n_pos, c->seq_len);
    if (c->pending) return fail("a lnb_forward_stage_begin has not been ended");
    if (n_pos > 0) {
        HIPCHK(hipSetDevice(m->device));
        HIPCHK(hipStreamSynchronize(c->stream));
        p += LNB_KV_BLOB_HEADER;
        for (size_t l = 0; l < c->ck.size(); l++) {
            if (!c->ck[l]) continue;
            if (prefix_copy_layer(c, l, n_pos, (unsigned char*)p, false)) { hipStreamSynchronize(c->stream); return -1; }
            p += kvc_layer_bytes(m->kv_dim, n_pos);
            // (the blob's rows are the caller's: an inf or a NaN among them raises the context's word, see enqueue_layer_kernel's K_ATTN)
            const hipError_t scanned = lnbk_kv_scan_nonfinite(c->ck[l], c->cv[l], c->seq_len, m->kv_dim, m->head_dim, nullptr, 0, n_pos, c->zseq_count + 3, c->stream);
            if (scanned != hipSuccess) { hipStreamSynchronize(c->stream); return fail("kv_nonfinite_scan_kernel could not be launched: %s", hipGetErrorString(scanned)); }
        }
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (n_pos_out) *n_pos_out = n_pos;
    return 0;
}

// exact-order (default) or tolerance mode for everything this context runs afterwards; the captured decode graph is per mode
extern "C" int lnb_ctx_set_mode(lnb_ctx* c, int mode) {
    if (!c) return fail("null argument");
    if (mode != LNB_MODE_EXACT && mode != LNB_MODE_FAST) return fail("unknown mode %d (LNB_MODE_EXACT = 0, LNB_MODE_FAST = 1)", mode);
    if (mode == c->mode) return 0;
    // (a long context, lnb_ctx_create_long, takes the tolerance mode too: none of lnb_fast.hip's kernels carries a per-position LDS array -- its GEMV / GEMM
    // stage x, its flash attention two static V tiles -- and its one-token attention is the exact kernels' own)
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->graphs.drop_all();
    c->mode = mode;
    return 0;
}
extern "C" int lnb_ctx_get_mode(const lnb_ctx* c) { return c ? c->mode : -1; }
// Which FORMS of the exact one-token kernels this context's steps launch (same arithmetic, same bits; tests/test_gpu_round5.py).  The latency
// forms (default) are built for ONE stream owning the chip: every launch takes all 256 CUs with eight or nine waves and 91 - 124 KB of LDS per
// workgroup, so nothing of another stream fits beside it.  A server or a pipeline rank keeps several generations in flight, one context and
// stream each (inference.go:174): there a chain-bound launch of one context should hide under the HBM-bound gate|up launch of another, which
// needs both workgroups on one CU -- the throughput forms keep every workgroup at or below 57 KB (wq|wk|wv: 128-step stages; wo, w2: the
// self-feeding row-broadcast kernel).  Round 4 had lost this (8 prompts in flight 308 -> 272 tokens/s) when it made the latency forms the only ones.
extern "C" int lnb_ctx_set_schedule(lnb_ctx* c, int sched) {
    if (!c) return fail("null argument");
    if (sched != LNB_SCHED_LATENCY && sched != LNB_SCHED_THROUGHPUT) return fail("unknown schedule %d (LNB_SCHED_LATENCY = 0, LNB_SCHED_THROUGHPUT = 1)", sched);
    if (sched == c->sched) return 0;
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->graphs.drop_all();
    c->sched = sched;
    return 0;
}
extern "C" int lnb_ctx_get_schedule(const lnb_ctx* c) { return c ? c->sched : -1; }
// Decode attention form: one-token calls at contexts above long_threshold run the chip-wide long-context kernels (bit-identical to the
// one-workgroup-per-head kernel, tests/test_gpu_configs.py).  long_threshold < 0 keeps the current value; force_zseq = 1 makes the
// long-context kernel always walk the reference's serial f64 sum instead of certifying the tree estimate (test hook).
// On a context beyond lnb_ctx_create's cap (lnb_ctx_create_long) the forms that stage the whole context in the LDS -- the one-launch form (bits 2 / 3,
// LNB_ATTN_ONE) and the eager-everywhere PV pass (LNB_ATTN_LAZY=0) -- cannot be launched: such a request runs the default scores + lazy-PV pair, same bits.
extern "C" int lnb_ctx_set_attention(lnb_ctx* c, int long_threshold, int force_zseq) {
    if (!c) return fail("null argument");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->graphs.drop_all();
    if (long_threshold >= 0) c->attn_long_T = long_threshold;
    c->force_zseq = force_zseq & 15;                         // bit 0: serial denominator; bit 1: two-launch long-context form; bit 2: one launch, every poll times out (tests); bit 3: one launch
    return 0;
}
// how many (head, token, layer) rows of the long-context attention had to walk the serial Z chain because the estimate could not be certified
extern "C" int lnb_ctx_zseq_count(lnb_ctx* c, int* out) {
    if (!c || !out) return fail("null argument");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipMemcpyAsync(c->h_io, c->zseq_count, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = c->h_io[0];
    return 0;
}
// how many fused-RMSNorm rows (one per norm-fused GEMV launch and row) could not be summed by the branch-free item walk and took the record walk
extern "C" int lnb_ctx_norm_fallbacks(lnb_ctx* c, int* out) {
    if (!c || !out) return fail("null argument");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipMemcpyAsync(c->h_io, c->zseq_count + 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = c->h_io[0];
    return 0;
}
// which matrix-core attention the last multi-row call of the context ran (check_call decides, per call): 3 scores once / 1 scores twice / 0 none
extern "C" int lnb_ctx_prefill_attention_form(const lnb_ctx* c, int* out) {
    if (!c || !out) return fail("null argument");
    *out = c->last_prefill_form;
    return 0;
}
extern "C" int lnb_ctx_set_layer_callback(lnb_ctx* c, lnb_layer_cb cb, void* user) { if (!c) return fail("null argument"); c->cb = cb; c->cb_user = user; return 0; }
extern "C" void* lnb_ctx_hidden_ptr(lnb_ctx* c, int which) { return !c ? nullptr : which == 2 ? (void*)c->ffn : (void*)c->x; }
extern "C" void* lnb_ctx_stream(lnb_ctx* c) { return c ? (void*)c->stream : nullptr; }
extern "C" int lnb_ctx_synchronize(lnb_ctx* c) { if (!c) return fail("null argument"); HIPCHK(hipSetDevice(c->m->device)); HIPCHK(hipStreamSynchronize(c->stream)); return 0; }

// ---- the five launches of one transformer block (position comes from c->st on the device) -----------
enum { K_QKV = 0, K_ATTN = 1, K_WO = 2, K_W13 = 3, K_W2 = 4, K_HEAD = 5, K_LAYER = 6 };
// Calls of 16 or more rows (prefill) run the same exact chains on the f32 matrix cores (gemm_mfma_kernel); LNB_PREFILL_MFMA=0
// keeps them on the S = 1 kernels (one launch row per token row), which is what the parity tests compare the two with.
static bool use_mfma(int S) { return knob(Knob::PREFILL_MFMA) && S >= 16; }
static GemmParams gemm_of(const TiledDesc& t, const uint16_t* x, int K, int n_rows, int S, const StepState* st) {
    GemmParams g{}; g.w = t.w; g.rw = t.rw; g.nch = t.nch; g.x = x; g.K = K; g.n_rows = n_rows; g.S = S; g.st = st; g.w16 = t.w16; return g;
}
// S < 16 rows: the exact-order chain kernels, or (LNB_MODE_FAST) the split-K kernels over the same resident weights
static hipError_t gemv_dispatch(const lnb_ctx* c, const GemvParams* g, int rw, int nch, int epi, int norm, hipStream_t st) {
    return c->mode == LNB_MODE_FAST ? lnbk_fast_gemv(g, rw, nch, epi, norm, st) : lnbk_gemv(g, rw, nch, epi, norm, st);
}
// S >= 16 rows: the exact chains on the f32 matrix cores, or (LNB_MODE_FAST) the bf16 matrix-core GEMM; shapes the fast kernel does not
// take (K not a multiple of 64) stay on the exact one
static hipError_t gemm_dispatch(int mode, const GemmParams* g, int epi, hipStream_t st) {
    // below ~200 rows the bf16 GEMM's 256-row weight tiles leave most CUs without work (wq|wk|wv: 24 workgroups) and the exact
    // kernel with its 16-row tiles is the faster one (128 rows: 29.6 ms against 36.6 ms per Forward): the tolerance mode may always
    // use an exact kernel
    if (mode == LNB_MODE_FAST && g->S >= knob(Knob::FAST_GEMM_MIN_ROWS)) { hipError_t e = lnbk_fast_gemm(g, epi, st); if (e != hipErrorNotSupported) return e; }
    // exact order with the matrix-core copy of the weights present (lnb_model_enable_batch): the streaming feed -- the same chains, the
    // same bits (tests/test_gpu_batch.py), the weights never staged through the LDS; LNB_PREFILL_STREAM=0 keeps the LDS-tiled kernel
    // Round 5: the same kernel also reads the RESIDENT layouts (no copy needed: the row-broadcast units are M16 units in another order, the chain
    // layouts' units are transposed inside the lane quads); LNB_PREFILL_NATIVE=0 keeps the LDS-tiled kernel for models without the copy
    if (knob(Knob::PREFILL_STREAM) && (g->K & 127) == 0 && (g->w16 || (knob(Knob::PREFILL_NATIVE) && g->w && (g->rw == 4 ? g->nch == 1 && (epi == EPI_STORE || epi == EPI_RESID) : g->rw >= 16))))
        return lnbk_gemm_stream(g, epi, g_num_cus, st);
    return lnbk_gemm(g, epi, st);
}
static int enqueue_layer_kernel(lnb_ctx* c, int l, int S, int which, hipStream_t st_other = nullptr, int lds_pad = 0) {
    lnb_model* m = c->m; const lnb_model_args& a = m->a; hipStream_t st = st_other ? st_other : c->stream;
    LayerW& L = m->layers[l - m->layer_begin];
    uint16_t* ck = c->ck[l - m->layer_begin]; uint16_t* cv = c->cv[l - m->layer_begin];
    // h = x + attention (llamatransformer.go:232) normally has its own buffer; in a block this stage holds only a part of, it lives
    // in x itself (the residual epilogues read and write element n from the same lane, so out may alias res): the hand-off inside a
    // block is then the same buffer as the hand-off between blocks (plus the ffn activations when the cut is in front of w2)
    uint16_t* const hbuf = m->whole(l) ? c->h : c->x;
    if (use_mfma(S) && which != K_ATTN) {
        switch (which) {
        case K_QKV: {
            HIPCHK(lnbk_rmsnorm_rows(c->x, L.attn_norm, c->xn, S, a.dim, a.norm_eps, st));
            GemmParams g = gemm_of(L.wqkv, c->xn, a.dim, L.wqkv.n_rows, S, c->st);
            g.cis = m->cis; g.q_out = c->q; g.cache_k = ck; g.cache_v = cv; g.seq_len = c->seq_len; g.q_dim = m->q_dim; g.kv_dim = m->kv_dim; g.head_dim = m->head_dim;
            HIPCHK(gemm_dispatch(c->mode, &g, EPI_QKV_ROPE, st)); return 0; }
        case K_WO: { GemmParams g = gemm_of(L.wo, c->att, m->q_dim, a.dim, S, c->st); g.out = hbuf; g.res = c->x; HIPCHK(gemm_dispatch(c->mode, &g, EPI_RESID, st)); return 0; }
        case K_W13: {
            HIPCHK(lnbk_rmsnorm_rows(hbuf, L.ffn_norm, c->xn, S, a.dim, a.norm_eps, st));
            GemmParams g = gemm_of(L.w13, c->xn, a.dim, m->ffn_hidden, S, c->st); g.out = c->ffn; g.silu = m->silu;
            HIPCHK(gemm_dispatch(c->mode, &g, EPI_SILU_MUL, st)); return 0; }
        case K_W2: { GemmParams g = gemm_of(L.w2, c->ffn, m->ffn_hidden, a.dim, S, c->st); g.out = c->x; g.res = hbuf; HIPCHK(gemm_dispatch(c->mode, &g, EPI_RESID, st)); return 0; }
        }
    }
    switch (which) {
    case K_QKV: {   // attn_norm + wq|wk|wv + RoPE + KV append  (llamatransformer.go:222, :297-403)
        GemvParams g{}; g.w = L.wqkv.w; g.x = c->x; g.norm_w = L.attn_norm; g.norm_fb = c->zseq_count + 1; g.eps = a.norm_eps; g.K = a.dim; g.n_rows = L.wqkv.n_rows; g.S = S; g.st = c->st;
        g.cis = m->cis; g.q_out = c->q; g.cache_k = ck; g.cache_v = cv; g.seq_len = c->seq_len; g.q_dim = m->q_dim; g.kv_dim = m->kv_dim; g.head_dim = m->head_dim;
        g.sched = c->sched;
        set_grid(g, L.wqkv); HIPCHK(gemv_dispatch(c, &g, L.wqkv.rw, 1, EPI_QKV_ROPE, 1, st)); return 0; }
    case K_ATTN: {  // scores / softmax / PV  (:409-514)
        AttnParams ap{}; ap.q = c->q; ap.cache_k = ck; ap.cache_v = cv; ap.out = c->att; ap.st = c->st; ap.dbg = g_dbg;
        ap.S = S; ap.H = a.n_heads; ap.KVH = a.n_kv_heads; ap.hd = m->head_dim; ap.seq_len = c->seq_len;
        ap.lds_T = c->seq_len < c->attn_short_cap ? c->seq_len : c->attn_short_cap;
        ap.host_T = c->call_T;
        ap.divisor = bf_wide_h(bf_trunc_h((float)std::sqrt((double)m->head_dim)));           // llamatransformer.go:464
        ap.mfma = use_mfma(S) ? 1 : 0; ap.exp_tab = m->exp_tab;
        ap.causal = (c->attn_causal && S > 1) ? 1 : 0;
        ap.longctx = 0; ap.force_zseq = c->force_zseq & 1; ap.e_buf = c->e_buf; ap.z_part = c->z_part; ap.zseq_count = c->zseq_count; ap.cnt = c->attn_cnt;
        if (ap.mfma && c->sidx_jt > 0 && c->call_T > 0 && c->sidx_jt * 16 >= c->call_T) { ap.score_idx = c->score_idx; ap.sidx_jt = c->sidx_jt; }     // (round 6: scores once, attn_mfma3_kernel)
        if (S == 1 && c->attn_long) {
            // ONE launch (attn_one_kernel, round 6): built, bit-exact in every form (tests/test_gpu_round6.py), and NOT the default -- measured on MI355X
            // (profiles/r06_att_timing.log, 8B head geometry): T = 4101: 26.3 us against 23.2 for the two launches; 1024: 14.1 / 11.5; 272: 8.2 against 7.7
            // for the one-workgroup-per-head kernel.  What the launch boundary costs (~1.2 us + the PV kernel's cold reads of e_buf) comes back as the
            // in-launch exchange (write-through stores drained + arrive + poll: 6.6 k cycles) plus a second dependent round trip for e_j (6.3 k).
            // Opt-in: LNB_ATTN_ONE=1, or bit 3 (8) of lnb_ctx_set_attention's flags; only for a context whose stream owns the chip (latency schedule)
            // and whose (head, slice) grid fits the CUs.  Bit 1 (2) of the flags keeps the two launches whatever the environment says.
            const bool one = (knob(Knob::ATTN_ONE) || (c->force_zseq & 12)) && !(c->force_zseq & 2) && c->sched == LNB_SCHED_LATENCY && m->head_dim % 16 == 0 &&
                             a.n_heads * (m->head_dim / 16) <= g_num_cus && lnbk_attn_one_lds(c->seq_len, m->head_dim) <= (size_t)160 * 1024;
            ap.longctx = one ? ((c->force_zseq & 4) ? 3 : 2) : 1;
        }
        // a multi-row call: the context's sticky word "a cached row holds an inf or a NaN" (zseq_count[3]) takes the rows this layer just wrote
        const bool multi = S > 1 && c->mode == LNB_MODE_EXACT;
        if (multi) HIPCHK(lnbk_kv_scan_nonfinite(ck, cv, c->seq_len, m->kv_dim, m->head_dim, c->st, 0, S, c->zseq_count + 3, st));
        if (c->attn_rows && ap.causal) {                     // lnb_forward_append beyond the row-per-workgroup kernel's reach: K and V read once for all rows
            ap.e_buf = c->sp_e_buf; ap.z_part = c->sp_z_part; ap.force_zseq = c->rows_flags & 1;
            HIPCHK(lnbk_attn_rows(&ap, c->call_T - S, st)); return 0;       // (every row of the pair ends at its own T: nothing to recompute)
        }
        if (c->mode == LNB_MODE_FAST && ap.mfma) {           // tolerance mode prefill: flash form on the bf16 matrix cores
            hipError_t e = lnbk_fast_attn(&ap, st);
            if (e != hipErrorNotSupported) { HIPCHK(e); return 0; }
        }
        HIPCHK(lnbk_attn(&ap, st));
        // the multi-row kernels rest on finite rows (lnb_kernels.hip, attn_mfma_kernel's header): with the word set the rows are computed again the
        // reference's way -- the launch returns at once otherwise, and a call of one row launches nothing new
        if (multi) HIPCHK(lnbk_attn_plain(&ap, c->zseq_count + 3, st));
        return 0; }
    case K_WO: {    // wo + residual  (:522, :232)
        GemvParams o{}; o.w = L.wo.w; o.x = c->att; o.K = m->q_dim; o.n_rows = a.dim; o.S = S; o.st = c->st; o.out = hbuf; o.res = c->x; o.sched = c->sched;
        set_grid(o, L.wo); HIPCHK(gemv_dispatch(c, &o, L.wo.rw, 1, EPI_RESID, 0, st)); return 0; }
    case K_W13: {   // ffn_norm + w1|w3 + SiLU*up  (:237, :601-617)
        GemvParams f{}; f.w = L.w13.w; f.x = hbuf; f.norm_w = L.ffn_norm; f.norm_fb = c->zseq_count + 1; f.eps = a.norm_eps; f.K = a.dim; f.n_rows = m->ffn_hidden; f.S = S; f.st = c->st;
        f.out = c->ffn; f.silu = m->silu; f.sched = c->sched;
        set_grid(f, L.w13);
        // one token, latency schedule, exact mode, and the layer has its 13-bit copy: the same chains fed from 13/16 of the bytes
        if (S == 1 && L.p_ok && c->mode == LNB_MODE_EXACT && c->sched == LNB_SCHED_LATENCY) { f.wp = L.p_w13; f.wp_base4 = L.p_base * 0x01010101u; HIPCHK(lnbk_gemv_w13p(&f, st)); return 0; }
        HIPCHK(gemv_dispatch(c, &f, L.w13.rw, 2, EPI_SILU_MUL, 1, st)); return 0; }
    case K_W2: {    // w2 + residual  (:619, :248)
        GemvParams d{}; d.w = L.w2.w; d.x = c->ffn; d.K = m->ffn_hidden; d.n_rows = a.dim; d.S = S; d.st = c->st; d.out = c->x; d.res = hbuf; d.lds_pad = lds_pad; d.sched = c->sched; d.prio = knob(Knob::W2_PRIO);
        set_grid(d, L.w2); HIPCHK(gemv_dispatch(c, &d, L.w2.rw, 1, EPI_RESID, 0, st)); return 0; }
    }
    return fail("bad kernel id");
}
static int enqueue_layers(lnb_ctx* c, int S, bool with_cb) {
    lnb_model* m = c->m;
    for (int l = m->layer_begin; l < m->layer_end; l++) {
        auto t0 = std::chrono::steady_clock::now();
        for (int k = K_QKV; k <= K_W2; k++) {
            if (!(k <= K_WO ? m->has_attn(l) : k == K_W13 ? m->has_w13(l) : m->has_w2(l))) continue;   // a stage may hold only parts of its first / last block
            if (enqueue_layer_kernel(c, l, S, k)) return -1;
        }
        if (with_cb && c->cb) {
            HIPCHK(hipStreamSynchronize(c->stream));
            double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            c->cb(l + 1, m->a.n_layers, secs, c->cb_user);                    // llamatransformer.go:163
        }
    }
    return 0;
}
// final RMSNorm + output projection of `rows` rows starting at row `first` (llamatransformer.go:166-170)
static int enqueue_head(lnb_ctx* c, int first, int rows) {
    lnb_model* m = c->m;
    if (use_mfma(rows)) {
        HIPCHK(lnbk_rmsnorm_rows(c->x + (size_t)first * m->a.dim, m->norm, c->xn, rows, m->a.dim, m->a.norm_eps, c->stream));
        GemmParams gm = gemm_of(m->output, c->xn, m->a.dim, m->a.vocab_size, rows, c->st); gm.out = c->logits;
        HIPCHK(gemm_dispatch(c->mode, &gm, EPI_STORE, c->stream));
        return 0;
    }
    GemvParams g{}; g.w = m->output.w; g.x = c->x + (size_t)first * m->a.dim; g.norm_w = m->norm; g.norm_fb = c->zseq_count + 1; g.eps = m->a.norm_eps; g.K = m->a.dim;
    g.n_rows = m->a.vocab_size; g.S = rows; g.st = c->st; g.out = c->logits;
    set_grid(g, m->output);
    // one token, latency schedule, exact mode, and the head has its 13-bit copy (head_pack_applies: 64-row resident layout, K fits, a 128-row block per CU):
    // the same chains, two per lane, fed from 13/16 of the bytes
    if (rows == 1 && m->p_out_ok && c->mode == LNB_MODE_EXACT && c->sched == LNB_SCHED_LATENCY) {
        g.wp = m->p_out; g.wp_base4 = m->p_out_base * 0x01010101u;
        g.n_blocks = (m->a.vocab_size + 127) / 128; g.n_wg = g.n_blocks < g_num_cus ? g.n_blocks : g_num_cus;
        HIPCHK(lnbk_gemv_headp(&g, c->stream));
        return 0;
    }
    HIPCHK(gemv_dispatch(c, &g, m->output.rw, 1, EPI_STORE, 1, c->stream));
    return 0;
}

// one-token call at context T: the long-context kernels above the crossover, and always beyond the short kernel's LDS reach
static bool want_long_attention(const lnb_ctx* c, int seq, int start_pos) {
    return seq == 1 && (start_pos + 1 > c->attn_long_T || start_pos + 1 > c->attn_short_cap);
}
static int check_call(lnb_ctx* c, int seq, int start_pos, bool causal = false) {
    if (seq == 0) return fail("empty token array");                                            // llamatransformer.go:146-148
    if (seq < 0 || start_pos < 0) return fail("negative sequence length or start position");
    const int T = start_pos + seq;
    if (T > c->m->cis_rows) return fail("incompatible locStart, locEnd values and tensor (position %d beyond the %d-row RoPE table)", T, c->m->cis_rows);
    if (T > c->seq_len) return fail("incompatible locStart, locEnd values and tensor (position %d beyond the KV cache of %d)", T, c->seq_len);
    if (seq > c->max_rows) return fail("a call of %d rows on a context whose activation buffers hold %d rows (lnb_ctx_create_long's max_rows)", seq, c->max_rows);
    if (seq > 1 && !causal && T % seq != 0) return fail("two tensor shapes cannot be broadcasted: [%d %d %d] and [%d %d]", c->m->a.n_heads, seq, T, seq, seq);
    // calls of 2.. rows that do NOT run on the matrix-core attention (fewer than 16 rows, or head_dim 32, which attn_mfma_kernel does not
    // take) go through the row-per-workgroup kernel, whose LDS arrays are sized for attn_short_cap positions
    const bool mfma_attn = use_mfma(seq) && (c->m->head_dim == 64 || c->m->head_dim == 128);
    c->call_T = T;
    // round 6: the matrix-core attention of an exact prefill keeps the table indices of its first pass (attn_mfma3_kernel): 512 bytes per (head, 16 query rows, 16
    // positions), one buffer per context, reused by every layer.  Grown here, on the host side of the call (never inside a capture); above LNB_ATTN_SIDX_MB
    // (default 4096; 0 = never) the call runs attn_mfma_kernel, which computes the scores twice instead.
    c->sidx_jt = 0;
    bool stage_has_attn = false;                             // (a pipeline stage cut inside a block may hold FFN parts only: no attention, no scratch)
    for (int l = c->m->layer_begin; l < c->m->layer_end && !stage_has_attn; l++) stage_has_attn = c->m->has_attn(l);
    // a one-token call on a context that still holds a LARGE scratch from its prompt (1.07 GB for 4096 rows of the 8B shape) gives it back: the decode steps never read it,
    // and a host that prefills many contexts would otherwise keep a gigabyte per context for their whole life.  Up to LNB_ATTN_SIDX_KEEP_MB (default 256) it stays for the next prompt.
    if (seq == 1 && c->score_idx && c->score_idx.capacity() > ((size_t)knob(Knob::ATTN_SIDX_KEEP_MB) << 20)) {
        HIPCHK(hipStreamSynchronize(c->stream));
        c->score_idx.reset();
    }
    if (mfma_attn && stage_has_attn && c->mode != LNB_MODE_FAST) {
        const int cap_mb = knob(Knob::ATTN_SIDX_MB);                 // (read per call: a test switches it inside one process)
        const size_t jt = (size_t)(T + 15) / 16, need = (size_t)c->m->a.n_heads * (size_t)((seq + 15) / 16) * jt * 512;
        if (cap_mb > 0 && need <= ((size_t)cap_mb << 20)) {
            if (!c->score_idx.fits(need)) {
                HIPCHK(hipStreamSynchronize(c->stream));
                if (dev_reserve(c->score_idx, need) != hipSuccess) (void)hipGetLastError();      // (no room: the two-pass kernel needs none)
            }
            if (c->score_idx) c->sidx_jt = (int)jt;
        }
    }
    if (seq > 1) c->last_prefill_form = (!mfma_attn || !stage_has_attn || c->mode == LNB_MODE_FAST) ? 0 : c->sidx_jt > 0 ? 3 : 1;
    if (seq > 1 && !mfma_attn && T > c->attn_short_cap && !(causal && c->attn_rows))
        return fail("a call of %d rows (2..15, or any multi-row call at head_dim 32) at context %d: the row-per-workgroup attention kernel stages "
                    "at most %d positions in the LDS; use one-token calls or 16 or more rows there", seq, T, c->attn_short_cap);
    return 0;
}

// lnb_forward_stage split in two so that a pipeline rank can put its exchange with the neighbouring ranks in flight while the stage
// computes: _begin enqueues the whole stage (embedding gather on the first stage, the blocks, norm + output + argmax on the last
// when want_argmax) on the ctx's stream and returns; _end waits for it and reports the token / the vocabulary check.
extern "C" int lnb_forward_stage_begin(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, int want_argmax) {
    if (!c) return fail("null argument");
    lnb_model* m = c->m; const int V = m->a.vocab_size;
    HIPCHK(hipSetDevice(m->device));
    if (c->pending) return fail("lnb_forward_stage_begin: the previous call has not been ended");
    if (check_call(c, seq, start_pos)) return -1;
    if (tokens && !m->first()) return fail("tokens given to a stage that does not own tok_embeddings");
    if (!tokens && m->first()) return fail("first stage needs tokens");
    if (want_argmax && !m->last()) return fail("logits requested from a stage that does not own output.weight");
    hipStream_t st = c->stream;
    c->attn_long = want_long_attention(c, seq, start_pos);
    HIPCHK(ctx_set_state(c, start_pos, 0, true));
    if (tokens) {
        if (staging_acquire(c)) return -1;
        memcpy(c->h_io + 2, tokens, (size_t)seq * 4);        // the caller's array need not outlive this call
        HIPCHK(hipMemcpyAsync(c->dtok, c->h_io + 2, (size_t)seq * 4, hipMemcpyHostToDevice, st));
        if (staging_release(c)) return -1;
        HIPCHK(hipMemsetAsync(c->derr, 0, 4, st));
        HIPCHK(lnbk_embed(m->tok_embd, c->dtok, c->x, seq, m->a.dim, V, c->derr, st));       // Fwd_Get_Rows :118
        HIPCHK(hipMemcpyAsync(c->h_io + 1, c->derr, 4, hipMemcpyDeviceToHost, st));
    }
    if (enqueue_layers(c, seq, false)) return -1;
    if (want_argmax) {
        if (c->logits_rows < 1) { HIPCHK(dev_alloc(c->logits, (size_t)V * 2)); c->logits_rows = 1; }
        if (enqueue_head(c, seq - 1, 1)) return -1;
        HIPCHK(lnbk_argmax(c->logits, V, c->dnext, c->st, c->dout, c->dout_cap, 0, st));        // inference.go:207-211
        HIPCHK(hipMemcpyAsync(c->h_io, c->dnext, 4, hipMemcpyDeviceToHost, st));
    }
    c->pending = true; c->pending_tokens = tokens != nullptr; c->pending_argmax = want_argmax != 0;
    return 0;
}
extern "C" int lnb_forward_stage_end(lnb_ctx* c, int32_t* argmax_last_out) {
    if (!c) return fail("null argument");
    if (!c->pending) return fail("lnb_forward_stage_end without a begin");
    HIPCHK(hipSetDevice(c->m->device));
    c->pending = false;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->pending_tokens && c->h_io[1]) return fail("token id at index %d is outside the vocabulary", c->h_io[1] - 1);
    if (argmax_last_out) {
        if (!c->pending_argmax) return fail("lnb_forward_stage_end: no argmax was requested at begin");
        *argmax_last_out = c->h_io[0];
    }
    return 0;
}

// token_probs_kernel over `rows` logits rows (lnb_device.h: TokProbParams)
static TokProbParams tp_params(const lnb_model* m, const uint16_t* logits, int rows, int k, double* zpart, uint64_t* kpart, unsigned* cnt,
                               const TokProbOut* out, int per_row_out) {
    TokProbParams p{};
    p.logits = logits; p.V = m->a.vocab_size; p.rows = rows; p.k = k; p.G = lnb_tokprob_slices(rows); p.etab = m->prob_etab;
    p.zpart = zpart; p.kpart = kpart; p.cnt = cnt; p.out = out; p.per_row_out = per_row_out;
    return p;
}

// lnb_forward_score: per row, the target's logit and probability and the row's ln Z, on the device instead of the logits copy
struct ScoreReq { const int32_t* targets; float* tlogit; float* tprob; double* log_z; };
static int forward_stage_impl(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, float* logits_out, int32_t* argmax_last_out, const ScoreReq* sc, bool causal = false);
extern "C" int lnb_forward_stage(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, float* logits_out, int32_t* argmax_last_out) {
    return forward_stage_impl(c, tokens, seq, start_pos, logits_out, argmax_last_out, nullptr);
}
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// causal (lnb_forward_append): the multi-row attention takes the true causal mask with an offset instead of the reference's modulo broadcast
static int forward_stage_impl(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, float* logits_out, int32_t* argmax_last_out, const ScoreReq* sc, bool causal) {
    if (!c) return fail("null argument");
    lnb_model* m = c->m; const int V = m->a.vocab_size;
    HIPCHK(hipSetDevice(m->device));
    if (check_call(c, seq, start_pos, causal)) return -1;
    struct CausalScope { lnb_ctx* c; ~CausalScope() { c->attn_causal = false; } } causal_scope{c};       // (every return below leaves the context on the reference's mask)
    c->attn_causal = causal;
    if (tokens && !m->first()) return fail("tokens given to a stage that does not own tok_embeddings");
    if (!tokens && m->first()) return fail("first stage needs tokens");
    if ((logits_out || argmax_last_out) && !m->last()) return fail("logits requested from a stage that does not own output.weight");
    hipStream_t st = c->stream;
    c->attn_long = want_long_attention(c, seq, start_pos);
    HIPCHK(ctx_set_state(c, start_pos, 0, true));
    if (tokens) {
        HIPCHK(hipMemcpyAsync(c->dtok, tokens, (size_t)seq * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(c->derr, 0, 4, st));
        HIPCHK(lnbk_embed(m->tok_embd, c->dtok, c->x, seq, m->a.dim, V, c->derr, st));       // Fwd_Get_Rows :118
    }
    if (enqueue_layers(c, seq, true)) return -1;
    TokProbOut so{};                                         // (lives until the synchronise below: its copy to the device is asynchronous)
    if (m->last() && (logits_out || argmax_last_out || sc)) {
        const int rows = (logits_out || sc) ? seq : 1;
        if (rows > c->logits_rows) {
            HIPCHK(hipStreamSynchronize(st));
            // the captured decode graph has the old buffer baked into its head GEMV / argmax nodes: drop it with the buffer
            c->graphs.drop_all();
            c->logits_rows = 0;
            HIPCHK(dev_alloc(c->logits, (size_t)rows * V * 2)); c->logits_rows = rows;
        }
        if (enqueue_head(c, rows == seq ? 0 : seq - 1, rows)) return -1;
        HIPCHK(lnbk_argmax(c->logits + (size_t)(rows - 1) * V, V, c->dnext, c->st, c->dout, c->dout_cap, 0, st));   // inference.go:207-211
        if (logits_out) {
            std::vector<uint16_t> hb((size_t)rows * V);
            HIPCHK(hipMemcpyAsync(hb.data(), c->logits, hb.size() * 2, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (size_t i = 0; i < hb.size(); i++) logits_out[i] = bf_wide_h(hb[i]);              // output.ToFloat32() :175
        }
        if (argmax_last_out) HIPCHK(hipMemcpyAsync(argmax_last_out, c->dnext, 4, hipMemcpyDeviceToHost, st));
        if (sc) {
            // scratch: [out record][partial sums rows x G][tickets][targets][target logits][target probs][ln Z]
            const size_t R = (size_t)rows;
            const size_t o_z = align256(sizeof(TokProbOut)), o_cnt = o_z + align256(R * LNB_TOKPROB_MAX_G * 8), o_tg = o_cnt + align256(R * 4), o_tl = o_tg + align256(R * 4),
                         o_tp = o_tl + align256(R * 4), o_lz = o_tp + align256(R * 4), need = o_lz + align256(R * 8);
            if (!c->sc_buf.fits(need)) {
                HIPCHK(hipStreamSynchronize(st));
                HIPCHK(dev_reserve(c->sc_buf, need));
            }
            char* b = c->sc_buf;
            so.log_z = (double*)(b + o_lz); so.walks = c->zseq_count + 2;
            HIPCHK(hipMemcpyAsync(b, &so, sizeof so, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemsetAsync(b + o_cnt, 0, R * 4, st));
            HIPCHK(hipMemcpyAsync(b + o_tg, sc->targets, R * 4, hipMemcpyHostToDevice, st));
            TokProbParams p = tp_params(m, c->logits, rows, 0, (double*)(b + o_z), nullptr, (unsigned*)(b + o_cnt), (const TokProbOut*)b, 0);
            p.targets = (const int32_t*)(b + o_tg); p.tlogit = (float*)(b + o_tl); p.tprob = (float*)(b + o_tp);
            HIPCHK(lnbk_token_probs(&p, st));
            HIPCHK(hipMemcpyAsync(sc->tlogit, b + o_tl, R * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(sc->tprob, b + o_tp, R * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(sc->log_z, b + o_lz, R * 8, hipMemcpyDeviceToHost, st));
        }
    }
    if (tokens) HIPCHK(hipMemcpyAsync(c->h_io + 1, c->derr, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (tokens && c->h_io[1]) return fail("token id at index %d is outside the vocabulary", c->h_io[1] - 1);
    return 0;
}

// lnb_forward with the head on every row and, instead of the logits, each row's target logit / probability and ln Z (include/lnb.h)
extern "C" int lnb_forward_score(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, const int32_t* targets,
                                 float* target_logit, float* target_prob, double* log_z, int32_t* argmax_last_out) {
    if (!c || !tokens || !targets || !target_logit || !target_prob || !log_z) return fail("null argument");
    if (!c->m->first() || !c->m->last()) return fail("lnb_forward_score needs a whole-model handle");
    for (int i = 0; i < seq; i++)
        if (targets[i] >= c->m->a.vocab_size) return fail("target id %d at index %d is outside the vocabulary (a negative id: no target)", targets[i], i);
    const ScoreReq sc{targets, target_logit, target_prob, log_z};
    return forward_stage_impl(c, tokens, seq, start_pos, nullptr, argmax_last_out, &sc);
}

extern "C" int lnb_forward(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, float* logits_out, int32_t* argmax_last_out) {
    if (!c || !tokens) return fail("null argument");
    if (!c->m->first() || !c->m->last()) return fail("lnb_forward needs a whole-model handle; use lnb_forward_stage for pipeline stages");
    return lnb_forward_stage(c, tokens, seq, start_pos, logits_out, argmax_last_out);
}

// lnb_ctx_attention (a test aid, include/lnb.h): the K_ATTN launch of `layer` as a Forward of `seq` rows at start_pos enqueues it, on a caller's query rows
extern "C" int lnb_ctx_attention(lnb_ctx* c, int layer, const uint16_t* q, int seq, int start_pos, uint16_t* out) {
    if (!c || !q || !out) return fail("null argument");
    lnb_model* m = c->m;
    HIPCHK(hipSetDevice(m->device));
    if (c->pending) return fail("a lnb_forward_stage_begin has not been ended");
    if (layer < m->layer_begin || layer >= m->layer_end || !m->has_attn(layer)) return fail("layer %d: this handle holds no attention of that block", layer);
    // the reference cannot broadcast its [seq, seq] mask over T positions unless seq divides T, and every exact kernel rests on that; the flash kernel of the
    // tolerance mode evaluates (j mod seq) > i at any T, and is reached with any T here (the same 16-row and head_dim conditions as enqueue_layer_kernel's)
    const bool flash = c->mode == LNB_MODE_FAST && use_mfma(seq) && (m->head_dim == 64 || m->head_dim == 128);
    if (check_call(c, seq, start_pos, flash)) return -1;
    hipStream_t st = c->stream;
    const size_t n = (size_t)seq * m->q_dim;
    c->attn_long = want_long_attention(c, seq, start_pos);
    HIPCHK(ctx_set_state(c, start_pos, 0, true));
    HIPCHK(hipMemcpyAsync(c->q, q, n * 2, hipMemcpyHostToDevice, st));
    if (enqueue_layer_kernel(c, layer, seq, K_ATTN)) return -1;
    HIPCHK(hipMemcpyAsync(out, c->att, n * 2, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// lnb_forward_append / lnb_forward_score_append: `seq` rows at ANY start position under the true causal mask -- row i is the one-token step at
// start_pos + i (include/lnb.h).  Always one multi-row call: 16 or more rows on the matrix-core kernel, fewer (or head_dim 32) on the row-per-workgroup
// kernel while the context fits its LDS, and beyond that -- or beyond lnb_ctx_set_rows_attention's threshold -- on the multi-row long-context pair
// (attn_rows_*_kernel: K and V read once for all rows).  Only when that pair's scratch cannot be allocated do the rows run as the one-token steps they are defined by.
static int attn_long_scratch(int n, int H, int maxT, Dev<double>& e_buf, Dev<double>& z_part, const char* whose, bool quiet = false);
static bool rows_rpw_invalid() { const int v = knob(Knob::ATTN_ROWS_RPW); return v != 1 && v != 2 && v != 4; }     // (attn_rows_pv_kernel's instantiations)
static int forward_append_impl(lnb_ctx* c, const char* name, const int32_t* tokens, int seq, int start_pos, float* logits_out, int32_t* argmax_last_out, const ScoreReq* sc) {
    if (!tokens) return fail("%s: null argument (tokens)", name);
    if (seq <= 0) return fail("%s: seq must be positive (got %d)", name, seq);
    if (start_pos < 0) return fail("%s: negative start position %d", name, start_pos);
    if (!c) return fail("%s: null argument (context)", name);
    lnb_model* m = c->m;
    if (!m->first() || !m->last()) return fail("%s needs a whole-model handle: pipeline stages have no append", name);
    if (c->mode != LNB_MODE_EXACT) return fail("%s is exact-mode only: the tolerance mode is frozen and its flash attention keeps the modulo mask", name);
    if (c->pending) return fail("a lnb_forward_stage_begin has not been ended");
    const int T = start_pos + seq, V = m->a.vocab_size;
    if (T > m->cis_rows) return fail("%s: position %d is beyond the %d-row RoPE table", name, T, m->cis_rows);
    if (T > c->seq_len) return fail("%s: position %d is beyond the KV cache of %d", name, T, c->seq_len);
    if (seq > c->max_rows) return fail("%s: a call of %d rows on a context whose activation buffers hold %d rows (lnb_ctx_create_long's max_rows)", name, seq, c->max_rows);
    const bool mfma_attn = use_mfma(seq) && (m->head_dim == 64 || m->head_dim == 128);
    // the multi-row long-context pair: its 16-row scratch is the verify passes', allocated here on first need (host side, outside any capture)
    // (no room for it: tried once per context, no error recorded -- the call succeeds on the one-token steps below)
    c->last_append_form = 0;
    bool rows = seq > 1 && !mfma_attn && T > std::min(c->rows_T, c->attn_short_cap) && !c->rows_no_scratch;
    if (rows && rows_rpw_invalid()) return fail("%s: LNB_ATTN_ROWS_RPW=%d is not a form of the multi-row long-context attention (1, 2 or 4)", name, knob(Knob::ATTN_ROWS_RPW));
    if (rows && attn_long_scratch(LNB_MAX_DRAFT + 1, m->a.n_heads, c->seq_len, c->sp_e_buf, c->sp_z_part, "a multi-row append", true)) { c->rows_no_scratch = true; rows = false; }
    if (seq == 1 || (!rows && !mfma_attn && T > c->attn_short_cap)) {
        for (int i = 0; i < seq; i++) {
            ScoreReq s1{}; if (sc) s1 = ScoreReq{sc->targets + i, sc->tlogit + i, sc->tprob + i, sc->log_z + i};
            if (forward_stage_impl(c, tokens + i, 1, start_pos + i, logits_out ? logits_out + (size_t)i * V : nullptr, i == seq - 1 ? argmax_last_out : nullptr, sc ? &s1 : nullptr)) return -1;
        }
        c->last_append_form = seq == 1 ? 0 : 3;
        return 0;
    }
    c->attn_rows = rows;
    const int rc = forward_stage_impl(c, tokens, seq, start_pos, logits_out, argmax_last_out, sc, true);
    c->attn_rows = false;
    if (rc == 0) c->last_append_form = rows ? 4 : mfma_attn ? 2 : 1;
    return rc;
}
extern "C" int lnb_forward_append(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, float* logits_out, int32_t* argmax_last_out) {
    return forward_append_impl(c, "lnb_forward_append", tokens, seq, start_pos, logits_out, argmax_last_out, nullptr);
}
extern "C" int lnb_forward_score_append(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, const int32_t* targets,
                                        float* target_logit, float* target_prob, double* log_z, int32_t* argmax_last_out) {
    if (!tokens || !targets || !target_logit || !target_prob || !log_z) return fail("lnb_forward_score_append: null argument");
    if (seq <= 0) return fail("lnb_forward_score_append: seq must be positive (got %d)", seq);
    if (start_pos < 0) return fail("lnb_forward_score_append: negative start position %d", start_pos);
    if (!c) return fail("lnb_forward_score_append: null argument (context)");
    for (int i = 0; i < seq; i++)
        if (targets[i] >= c->m->a.vocab_size) return fail("target id %d at index %d is outside the vocabulary (a negative id: no target)", targets[i], i);
    const ScoreReq sc{targets, target_logit, target_prob, log_z};
    return forward_append_impl(c, "lnb_forward_score_append", tokens, seq, start_pos, nullptr, argmax_last_out, &sc);
}

// one decode step = embed(token on device) -> layers -> head -> [token probabilities] -> argmax that feeds the next step; sample: the sampler's token
// (the context's device sampler, lnb_decode_sample_until) in place of the argmax
static int enqueue_decode_step(lnb_ctx* c, bool sample = false) {
    lnb_model* m = c->m;
    // LNB_MEASURE_SKIP_TOKEN_KERNELS=1 (timing only, the tokens are garbage): the step without its embedding gather and argmax launches =
    // the most that fusing them into the neighbouring products could return (NOTES 5.8)
    const bool skip = knob(Knob::MEASURE_SKIP_TOKEN_KERNELS) != 0;
    if (!skip) HIPCHK(lnbk_embed(m->tok_embd, c->dtok, c->x, 1, m->a.dim, m->a.vocab_size, c->derr, c->stream));
    if (enqueue_layers(c, 1, false)) return -1;
    if (enqueue_head(c, 0, 1)) return -1;
    if (c->top_k > 0 && !skip) {                             // the record of the token the argmax below appends (it reads the slot before the argmax advances it)
        TokProbParams p = tp_params(m, c->logits, 1, c->top_k, c->tp.zpart, c->tp.kpart, c->tp.cnt, c->tp.out, 0);
        HIPCHK(lnbk_token_probs(&p, c->stream));
    }
    if (sample) HIPCHK(lnbk_sample(c->logits, m->a.vocab_size, 1, m->prob_etab, c->d_smp, c->dtok, c->st, c->dout, c->dout_cap, 1, nullptr, nullptr, nullptr, c->stream));
    else if (!skip) HIPCHK(lnbk_argmax(c->logits, m->a.vocab_size, c->dtok, c->st, c->dout, c->dout_cap, 1, c->stream));
    return 0;
}

// Stop ids on the device (inference.go:233-252: generation ends with the first token that is one of model.StopTokenIds, and that token is
// emitted): the argmax kernel compares every generated token with the context's stop ids and freezes the generation -- position, token
// word, token log -- when one matches; whatever was enqueued behind it recomputes the same step and changes nothing.  0 ids = never stops.
extern "C" int lnb_ctx_set_stop_ids(lnb_ctx* c, const int32_t* ids, int n) {
    if (!c || (n > 0 && !ids)) return fail("null argument");
    if (n < 0 || n > LNB_MAX_STOP_IDS) return fail("a context takes 0..%d stop ids (got %d)", LNB_MAX_STOP_IDS, n);
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(lnbk_set_stop(c->st, ids, n, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->n_stop = n;
    return 0;
}
// Token probabilities of the greedy loop (include/lnb.h): top_k records per generated token, kept on the device beside the token log.
// 0 (default) enqueues nothing: the captured step is exactly the one without the feature.
extern "C" int lnb_ctx_set_token_probs(lnb_ctx* c, int top_k) {
    if (!c) return fail("null argument");
    if (top_k < 0 || top_k > LNB_MAX_TOP_K) return fail("top_k must be 0..%d (got %d)", LNB_MAX_TOP_K, top_k);
    if (!c->m->first() || !c->m->last()) return fail("token probabilities need a whole-model handle (pipeline stages are not supported)");
    if (c->batch_users > 0) return fail("context is a member of %d live batch(es): its top-k is fixed until they are destroyed", c->batch_users);
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->graphs.drop_all();
    c->tp = {};
    c->top_k = 0; c->tp_last_k = 0; c->tp_last_n = 0;
    if (top_k == 0) return 0;
    const size_t n = (size_t)c->dout_cap * top_k, G = LNB_TOKPROB_MAX_G;
    HIPCHK(dev_alloc(c->tp.ids, n * 4)); HIPCHK(dev_alloc(c->tp.logit, n * 4)); HIPCHK(dev_alloc(c->tp.prob, n * 4));
    HIPCHK(dev_alloc(c->tp.logz, (size_t)c->dout_cap * 8));
    HIPCHK(dev_alloc(c->tp.zpart, G * 8)); HIPCHK(dev_alloc(c->tp.kpart, G * LNB_TOKPROB_MAX_K * 8));
    HIPCHK(dev_alloc(c->tp.cnt, 16)); HIPCHK(hipMemsetAsync(c->tp.cnt, 0, 16, c->stream));
    TokProbOut o{}; o.st = c->st; o.ids = c->tp.ids; o.logit = c->tp.logit; o.prob = c->tp.prob; o.log_z = c->tp.logz; o.walks = c->zseq_count + 2; o.cap = c->dout_cap;
    HIPCHK(dev_alloc(c->tp.out, sizeof o));
    HIPCHK(hipMemcpyAsync(c->tp.out, &o, sizeof o, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                 // (o is stack memory)
    c->top_k = top_k;
    return 0;
}
extern "C" int lnb_ctx_read_token_probs(lnb_ctx* c, int first, int n, int32_t* ids, float* logits, float* probs, double* log_z) {
    if (!c || !ids || !logits || !probs || !log_z) return fail("null argument");
    if (c->tp_last_k <= 0) return fail("the last decode call of this context recorded no token probabilities (lnb_ctx_set_token_probs)");
    if (first < 0 || n < 0 || first + n > c->tp_last_n)
        return fail("records [%d, %d) requested: the last decode call generated %d tokens", first, first + n, c->tp_last_n);
    if (n == 0) return 0;
    const size_t k = c->tp_last_k, off = (size_t)first * k, cnt = (size_t)n * k;
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipMemcpyAsync(ids, c->tp.ids + off, cnt * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(logits, c->tp.logit + off, cnt * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(probs, c->tp.prob + off, cnt * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(log_z, c->tp.logz + first, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
// rows (decode steps, scored rows) of this context whose token probabilities walked the reference's serial sum
extern "C" int lnb_ctx_token_prob_walks(lnb_ctx* c, int* out) {
    if (!c || !out) return fail("null argument");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipMemcpyAsync(c->h_io, c->zseq_count + 2, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = c->h_io[0];
    return 0;
}
// What `body` enqueues on `st`, captured into the graph slot -- once: a slot that holds a graph is left alone and the body does not run.
// A body that fails has set the message; the capture is ended and its graph dropped.
template <class Body> static int capture_once(GraphExec& slot, hipStream_t st, Body body) {
    if (slot) return 0;
    Owned<hipGraph_t, hipGraphDestroy> g;                    // the transient graph: gone on every way out
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc = body();
    hipError_t e = g.fill([&](hipGraph_t* q) { return hipStreamEndCapture(st, q); });
    if (rc) return -1;
    HIPCHK(e);
    HIPCHK(slot.fill([&](hipGraphExec_t* q) { return hipGraphInstantiate(q, g, nullptr, nullptr, 0); }));
    return 0;
}
// one captured graph per attention form: the step at context T replays the long-context one when T exceeds the crossover.  Captures the
// forms that steps at positions start_pos .. start_pos + n_steps - 1 need and the context does not hold yet.
static int capture_decode_graphs(lnb_ctx* c, int start_pos, int n_steps, bool sample = false) {
    const GraphLaunch launch = sample ? GL_SAMPLE : GL_GREEDY;
    auto capture = [&](bool longctx) {
        return capture_once(c->graphs.slot(launch, longctx ? GF_LONG : GF_SHORT), c->stream, [&] { c->attn_long = longctx; return enqueue_decode_step(c, sample); });
    };
    const bool any_short = !want_long_attention(c, 1, start_pos), any_long = want_long_attention(c, 1, start_pos + n_steps - 1);
    if (any_short && capture(false)) return -1;
    if (any_long && capture(true)) return -1;
    return 0;
}
// what every sampling entry point asks of a sampler (who: "" or "sequence 3: "), before anything else is looked at
static int sampler_check(const lnb_sampler* s, const char* who) {
    if (!(s->temperature >= 0.0f) || std::isinf(s->temperature)) return fail("%ssampler: temperature must be finite and >= 0 (got %g; 0 = greedy)", who, (double)s->temperature);
    if (s->top_k < 0) return fail("%ssampler: top_k must be >= 0 (got %d; 0 = off)", who, s->top_k);
    if (!(s->top_p > 0.0f && s->top_p <= 1.0f)) return fail("%ssampler: top_p must be in (0, 1] (got %g; 1 = off)", who, (double)s->top_p);
    if (s->reserved != 0) return fail("%ssampler: reserved must be 0 (got %d)", who, s->reserved);
    return 0;
}
static int sample_vocab_check(int V) {
    if (V < 1 || V > LNB_SAMPLE_MAX_VOCAB) return fail("sampling takes rows of 1..%d entries (got %d): the integer weight sums of a longer row could pass 2^63", LNB_SAMPLE_MAX_VOCAB, V);
    return 0;
}
static const char* const k_sample_probs_advice = "records token probabilities, whose records promise ids[i * k] == out_tokens[i] -- a sampled token does not keep that: "
                                                 "switch them off (lnb_ctx_set_token_probs(ctx, 0)) for a sampling call";
static int decode_greedy_impl(lnb_ctx* c, int32_t token, int start_pos, int n_steps, int32_t* out_tokens, int* n_generated, int* finished, float* ms_out, const lnb_sampler* smp = nullptr);
extern "C" int lnb_decode_greedy(lnb_ctx* c, int32_t token, int start_pos, int n_steps, int32_t* out_tokens, float* ms_out) {
    return decode_greedy_impl(c, token, start_pos, n_steps, out_tokens, nullptr, nullptr, ms_out);
}
// the same loop, reporting how far it got: *n_generated tokens are valid in out_tokens (max_steps unless a stop id ended the generation;
// the stop token is the last of them), *finished = 1 if a stop id did
extern "C" int lnb_decode_greedy_until(lnb_ctx* c, int32_t token, int start_pos, int max_steps, int32_t* out_tokens, int* n_generated, int* finished, float* ms_out) {
    if (!n_generated) return fail("null argument");
    return decode_greedy_impl(c, token, start_pos, max_steps, out_tokens, n_generated, finished, ms_out);
}
// lnb_decode_greedy_until with the sampler's token in place of the argmax (include/lnb.h): the same loop over sampling steps, which have captured
// graphs of their own; the sampler is copied to the device struct those graphs point at
extern "C" int lnb_decode_sample_until(lnb_ctx* c, const lnb_sampler* sampler, int32_t token, int start_pos, int max_steps, int32_t* out_tokens, int* n_generated,
                                       int* finished, float* ms_out) {
    if (!c || !sampler || !out_tokens || !n_generated) return fail("null argument");
    if (sampler_check(sampler, "")) return -1;
    return decode_greedy_impl(c, token, start_pos, max_steps, out_tokens, n_generated, finished, ms_out, sampler);
}
// measurement aid (tools/sample_bench.py): average HIP-event time of the token launch of a decode step ALONE, on the logits row the context's last step
// left -- sample_kernel with this sampler, or argmax_kernel (sampler NULL).  Every launch advances the context's device state from `pos` as a step does.
extern "C" int lnb_profile_sample(lnb_ctx* c, const lnb_sampler* sampler, int pos, int iters, float* avg_ms_out) {
    if (!c || !avg_ms_out) return fail("null argument");
    if (sampler && sampler_check(sampler, "")) return -1;
    lnb_model* m = c->m;
    if (!m->first() || !m->last()) return fail("lnb_profile_sample needs a whole-model handle");
    if (sampler && sample_vocab_check(m->a.vocab_size)) return -1;
    if (iters <= 0 || pos < 0) return fail("bad arguments");
    if (c->pending) return fail("a lnb_forward_stage_begin has not been ended");
    HIPCHK(hipSetDevice(m->device));
    hipStream_t st = c->stream;
    if (sampler && !c->d_smp) HIPCHK(dev_alloc(c->d_smp, sizeof(LnbSampler)));
    if (sampler) HIPCHK(hipMemcpyAsync(c->d_smp, sampler, sizeof(LnbSampler), hipMemcpyHostToDevice, st));
    HIPCHK(ctx_set_state(c, pos, 0, false, false));
    auto launch = [&]() {
        return sampler ? lnbk_sample(c->logits, m->a.vocab_size, 1, m->prob_etab, c->d_smp, c->dtok, c->st, c->dout, c->dout_cap, 1, nullptr, nullptr, nullptr, st)
                       : lnbk_argmax(c->logits, m->a.vocab_size, c->dtok, c->st, c->dout, c->dout_cap, 1, st);
    };
    for (int i = 0; i < 3; i++) HIPCHK(launch());
    HIPCHK(hipEventRecord(c->ev0, st));
    for (int i = 0; i < iters; i++) HIPCHK(launch());
    HIPCHK(hipEventRecord(c->ev1, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *avg_ms_out = ms / (float)iters;
    return 0;
}
static int decode_greedy_impl(lnb_ctx* c, int32_t token, int start_pos, int n_steps, int32_t* out_tokens, int* n_generated, int* finished, float* ms_out, const lnb_sampler* smp) {
    if (!c || !out_tokens) return fail("null argument");
    lnb_model* m = c->m;
    if (!m->first() || !m->last()) return fail("%s needs a whole-model handle", smp ? "lnb_decode_sample_until" : "lnb_decode_greedy");
    if (smp) {
        if (sample_vocab_check(m->a.vocab_size)) return -1;
        if (c->top_k > 0) return fail("the context %s", k_sample_probs_advice);
        if (c->pending) return fail("a lnb_forward_stage_begin has not been ended");
    }
    HIPCHK(hipSetDevice(m->device));
    if (n_steps <= 0) return fail("n_steps must be positive");
    if (n_steps > c->dout_cap) return fail("n_steps %d exceeds the context length %d", n_steps, c->dout_cap);
    if (check_call(c, 1, start_pos) || check_call(c, 1, start_pos + n_steps - 1)) return -1;
    if (token < 0 || token >= m->a.vocab_size) return fail("token id at index 0 is outside the vocabulary");
    hipStream_t st = c->stream;
    const bool use_graph = knob(Knob::NO_GRAPH) == 0;
    if (smp && !c->d_smp) HIPCHK(dev_alloc(c->d_smp, sizeof(LnbSampler)));
    if (use_graph && capture_decode_graphs(c, start_pos, n_steps, smp != nullptr)) return -1;
    c->tp_last_k = 0; c->tp_last_n = 0;
    if (smp) HIPCHK(hipMemcpyAsync(c->d_smp, smp, sizeof(LnbSampler), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->dtok, &token, 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(c->derr, 0, 4, st));
    // (the argmax kernel advances the position on the device from here on.)  Stop ids are compared only on behalf of a caller that learns how far
    // the run got: lnb_decode_greedy promises n_steps tokens and ignores them -- it used to freeze silently at a stop id and hand back stale
    // log entries behind it
    HIPCHK(ctx_set_state(c, start_pos, 0, false, n_generated != nullptr));
    c->call_T = 0;                                           // (the captured graphs serve every position: nothing host-side to validate)
    HIPCHK(hipEventRecord(c->ev0, st));
    for (int i = 0; i < n_steps; i++) {
        const bool longctx = want_long_attention(c, 1, start_pos + i);
        if (use_graph) HIPCHK(hipGraphLaunch(c->graphs.slot(smp ? GL_SAMPLE : GL_GREEDY, longctx ? GF_LONG : GF_SHORT), st));
        else { c->attn_long = longctx; if (enqueue_decode_step(c, smp != nullptr)) return -1; }
    }
    HIPCHK(hipEventRecord(c->ev1, st));
    HIPCHK(hipMemcpyAsync(out_tokens, c->dout, (size_t)n_steps * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(c->h_io + 1, c->derr, 4, hipMemcpyDeviceToHost, st));
    StepState hs{};
    if (n_generated) HIPCHK(hipMemcpyAsync(&hs, c->st, sizeof(StepState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms_out) HIPCHK(hipEventElapsedTime(ms_out, c->ev0, c->ev1));
    if (c->h_io[1]) return fail("generated token id is outside the vocabulary");
    if (n_generated) { *n_generated = hs.n_out; if (finished) *finished = hs.finished; c->dev_pos = -1; }     // (a stopped run leaves the device position short of start_pos + n_steps)
    c->tp_last_k = c->top_k; c->tp_last_n = n_generated ? hs.n_out : n_steps;
    return 0;
}

// One launch of a GEMV class with the per-wave debug buffer armed (GemvParams.dbg): out[w * 16 + ..] for wave w = {workgroups that reported, avg
// total cycles, max total, avg barrier wait, avg [2] (x staged / prologue end), avg [3] (fold or walk; rowcast_lds chain waves: chain start),
// avg stamps 0..7 (stamp 7 = the launch on the constant-rate wall clock)}.  The device position must have been set by the caller.
static int gemv_stamps(lnb_ctx* c, int which, double* out, int full) {
    lnb_model* m = c->m; hipStream_t st = c->stream;
    const size_t n = (size_t)4096 * 8 * 4, n2 = (size_t)4096 * 8 * 8;       // + 8 phase stamps per wave behind the four totals (LNB_STAMP in lnb_kernels.hip)
    Dev<long long> dbuf;
    HIPCHK(dev_alloc(dbuf, (n + n2) * 8));
    HIPCHK(hipMemsetAsync(dbuf, 0, (n + n2) * 8, st));
    const int nl = m->layer_end - m->layer_begin;
    if (nl <= 0 && which != K_HEAD) return fail("this stage holds no transformer block: only kernel class %d (norm + output) can be stamped", K_HEAD);   // (i % nl below)
    // three plain launches of the class on other layers first, back to back with the stamped one: it then runs as a launch inside a decode step does
    // (instruction cache, clocks and memory pipeline warm) instead of as the first launch after an idle gap
    int rc = 0;
    for (int i = 4; i < 7 && !rc; i++) rc = which == K_HEAD ? enqueue_head(c, 0, 1) : enqueue_layer_kernel(c, m->layer_begin + i % nl, 1, which);
    g_dbg = dbuf; g_dbg_full = full;
    if (!rc) rc = which == K_HEAD ? enqueue_head(c, 0, 1) : enqueue_layer_kernel(c, m->layer_begin + 7 % nl, 1, which);
    g_dbg = nullptr; g_dbg_full = 0;
    if (rc) { hipStreamSynchronize(st); return -1; }          // (the launches that were accepted still write the buffer)
    std::vector<long long> h(n + n2);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(h.data(), dbuf, (n + n2) * 8, hipMemcpyDeviceToHost));
    for (int w = 0; w < 8; w++) {
        double* o = out + w * 16; for (int k = 0; k < 16; k++) o[k] = 0;
        int cnt = 0;
        for (int g = 0; g < 4096; g++) {
            const long long* d = &h[((size_t)g * 8 + w) * 4]; const long long* s8 = &h[n + ((size_t)g * 8 + w) * 8];
            if (d[0] <= 0) continue;
            cnt++; o[1] += (double)d[0]; if ((double)d[0] > o[2]) o[2] = (double)d[0]; o[3] += (double)d[1]; o[4] += (double)d[2]; o[5] += (double)d[3];
            for (int k = 0; k < 8; k++) o[6 + k] += (double)s8[k];
        }
        o[0] = cnt;
        if (cnt) { o[1] /= cnt; o[3] /= cnt; o[4] /= cnt; o[5] /= cnt; for (int k = 0; k < 8; k++) o[6 + k] /= cnt; }
    }
    return 0;
}
// measurement aid (bench.py: roofline.measured_model): the in-kernel cycle stamps of ONE launch of a GEMV class (which: 0, 2, 3, 4, 5 as in
// lnb_profile_kernel) at position pos; out = 8 waves x 16 doubles as gemv_stamps lays them out; *wall_clock_khz = the rate of stamp 7's clock
extern "C" int lnb_profile_kernel_stamps(lnb_ctx* c, int which, int pos, double* out, int* wall_clock_khz) {
    if (!c || !out) return fail("null argument");
    lnb_model* m = c->m;
    HIPCHK(hipSetDevice(m->device));
    if (which < 0 || which > K_HEAD || which == K_ATTN) return fail("bad arguments");
    if (check_call(c, 1, pos)) return -1;
    if (which == K_HEAD && !m->last()) return fail("this stage does not own output.weight");
    c->attn_long = want_long_attention(c, 1, pos);
    HIPCHK(ctx_set_state(c, pos, 0, true));
    if (wall_clock_khz) { int khz = 0; HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, m->device)); *wall_clock_khz = khz; }
    return gemv_stamps(c, which, out, 0);                    // light: the launch runs as it does in production
}

// measurement aid (tools/ffn_overlap.py, profiles/r06_ffn_stream.md): what a w1|w3 -> w2 streaming stage could reach, measured before it is built.  The gate|up
// kernel and the down kernel of a block are launched on two streams, the down kernel `w2_delay_us` microseconds behind the gate|up kernel (a one-wave
// spin kernel in front of it holds its stream): delay 0 = plain co-residency, delay ~ "the first row band is complete" = the timeline of a band
// pipeline, with no dependency stall at all (w2 reads STALE activations -- the results are meaningless, only the time is).  w2_lds_pad pads w2's
// LDS request (r3's way of forcing exactly one workgroup of each kernel per CU).  Both kernels take the forms of the context's schedule.
// the second stream of a two-stream measurement with its fork and join events; on every way out the device is idle before they are released
struct PairStreams {
    Stream st2; Event ef, ej;
    int create() {
        HIPCHK(stream_create(st2, hipStreamNonBlocking));
        HIPCHK(event_create(ef, hipEventDisableTiming)); HIPCHK(event_create(ej, hipEventDisableTiming));
        return 0;
    }
    ~PairStreams() { hipDeviceSynchronize(); }
};
extern "C" int lnb_profile_ffn_pair(lnb_ctx* c, int pos, int iters, int w2_delay_us, int w2_lds_pad, float* avg_ms_out) {
    if (!c || !avg_ms_out) return fail("null argument");
    lnb_model* m = c->m;
    HIPCHK(hipSetDevice(m->device));
    if (iters <= 0) return fail("bad arguments");
    if (check_call(c, 1, pos)) return -1;
    const int nl2 = m->layer_end - m->layer_begin;
    if (nl2 <= 0) return fail("this stage holds no transformer block");
    PairStreams ps;
    if (ps.create()) return -1;
    hipStream_t st = c->stream, st2 = ps.st2; hipEvent_t ef = ps.ef, ej = ps.ej;
    c->attn_long = false;
    HIPCHK(ctx_set_state(c, pos, 0, true));
    auto pair = [&](int i) -> int {
        const int l = m->layer_begin + i % nl2;
        HIPCHK(hipEventRecord(ef, st)); HIPCHK(hipStreamWaitEvent(st2, ef, 0));
        if (w2_delay_us >= 0) {
            if (enqueue_layer_kernel(c, l, 1, K_W13)) return -1;
            if (w2_delay_us > 0) HIPCHK(lnbk_spin(w2_delay_us, st2));
            if (enqueue_layer_kernel(c, l, 1, K_W2, st2, w2_lds_pad)) return -1;
        } else {                                             // w2 first (its waves are the older ones), gate|up -delay behind it
            if (enqueue_layer_kernel(c, l, 1, K_W2, st2, w2_lds_pad)) return -1;
            if (w2_delay_us < -1) HIPCHK(lnbk_spin(-w2_delay_us, st));
            if (enqueue_layer_kernel(c, l, 1, K_W13)) return -1;
        }
        HIPCHK(hipEventRecord(ej, st2)); HIPCHK(hipStreamWaitEvent(st, ej, 0));
        return 0;
    };
    int rc = 0;
    for (int i = 0; i < 3 && !rc; i++) rc = pair(i);
    if (!rc) { HIPCHK(hipEventRecord(c->ev0, st)); for (int i = 0; i < iters && !rc; i++) rc = pair(i + 3); HIPCHK(hipEventRecord(c->ev1, st)); }
    if (rc) return -1;
    HIPCHK(hipDeviceSynchronize());
    float ms2 = 0; HIPCHK(hipEventElapsedTime(&ms2, c->ev0, c->ev1));
    *avg_ms_out = ms2 / (float)iters;
    return 0;
}

extern "C" int lnb_profile_kernel(lnb_ctx* c, int which, int pos, int iters, float* avg_ms_out) {
    if (!c || !avg_ms_out) return fail("null argument");
    lnb_model* m = c->m;
    HIPCHK(hipSetDevice(m->device));
    // which 7 / 8 (measurement only): the gate|up kernel and the down kernel of a block launched CONCURRENTLY on two streams (7: w2 first, i.e.
    // its waves are the older ones on every SIMD; 8: w1|w3 first), w2's LDS request padded so that exactly one workgroup of each kernel sits on
    // every CU -- what co-residency would cost a w1|w3 -> w2 row-band pipeline (NOTES.md 6.1); results are NOT meaningful (w2 reads stale input)
    if (iters <= 0 || which < 0 || which > K_LAYER + 2) return fail("bad arguments");
    if (check_call(c, 1, pos)) return -1;
    if (which == K_HEAD && !m->last()) return fail("this stage does not own output.weight");
    hipStream_t st = c->stream;
    if (which > K_LAYER) {
        PairStreams ps;
        if (ps.create()) return -1;
        hipStream_t st2 = ps.st2; hipEvent_t ef = ps.ef, ej = ps.ej;
        c->attn_long = false;
        HIPCHK(ctx_set_state(c, pos, 0, true));
        const int nl2 = m->layer_end - m->layer_begin, pad = knob(Knob::W2_LDS_PAD);
        auto pair = [&](int i) -> int {
            const int l = m->layer_begin + i % nl2;
            HIPCHK(hipEventRecord(ef, st)); HIPCHK(hipStreamWaitEvent(st2, ef, 0));
            if (which == K_LAYER + 1) { if (enqueue_layer_kernel(c, l, 1, K_W2, st2, pad)) return -1; if (enqueue_layer_kernel(c, l, 1, K_W13)) return -1; }
            else { if (enqueue_layer_kernel(c, l, 1, K_W13)) return -1; if (enqueue_layer_kernel(c, l, 1, K_W2, st2, pad)) return -1; }
            HIPCHK(hipEventRecord(ej, st2)); HIPCHK(hipStreamWaitEvent(st, ej, 0));
            return 0;
        };
        int rc = 0;
        for (int i = 0; i < 3 && !rc; i++) rc = pair(i);
        if (!rc) { HIPCHK(hipEventRecord(c->ev0, st)); for (int i = 0; i < iters && !rc; i++) rc = pair(i + 3); HIPCHK(hipEventRecord(c->ev1, st)); }
        if (rc) return -1;
        HIPCHK(hipDeviceSynchronize());
        float ms2 = 0; HIPCHK(hipEventElapsedTime(&ms2, c->ev0, c->ev1));
        *avg_ms_out = ms2 / (float)iters;
        return 0;
    }
    c->attn_long = want_long_attention(c, 1, pos);
    HIPCHK(ctx_set_state(c, pos, 0, true));
    const int nl = m->layer_end - m->layer_begin;
    // consecutive launches walk through the layers so that every launch streams its weights from HBM
    // (one layer's 235 MB gate/up matrix would otherwise sit in the 256 MiB Infinity Cache)
    auto run = [&](int i) -> int {
        int l = m->layer_begin + (knob(Knob::PROFILE_SAME_LAYER) ? 0 : (i % nl));
        if (which == K_HEAD) return enqueue_head(c, 0, 1);
        if (which == K_LAYER) { for (int k = K_QKV; k <= K_W2; k++) if (enqueue_layer_kernel(c, l, 1, k)) return -1; return 0; }
        return enqueue_layer_kernel(c, l, 1, which);
    };
    for (int i = 0; i < 3; i++) if (run(i)) return -1;
    HIPCHK(hipEventRecord(c->ev0, st));
    for (int i = 0; i < iters; i++) if (run(i + 3)) return -1;
    HIPCHK(hipEventRecord(c->ev1, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *avg_ms_out = ms / (float)iters;
    const bool timing = knob(Knob::GEMV_TIMING) != 0;
    if (timing && which == K_ATTN) {
        Dev<long long> dbuf;
        HIPCHK(dev_alloc(dbuf, 64 * 8)); HIPCHK(hipMemsetAsync(dbuf, 0, 64 * 8, st));
        g_dbg = dbuf;
        int rc = run(7);
        g_dbg = nullptr;
        if (rc) return -1;
        HIPCHK(hipStreamSynchronize(st));
        long long h[64] = {0};
        HIPCHK(hipMemcpy(h, dbuf, sizeof h, hipMemcpyDeviceToHost));
        for (int w = 0; w < 4; w++) {
            fprintf(stderr, "[timing] attention pos %d wave %d phases (s_memtime ticks):", pos, w);
            for (int k = 1; k < 7; k++) fprintf(stderr, " %lld", h[w * 16 + k] - h[w * 16 + k - 1]);
            fprintf(stderr, " | first pass: chain %lld exp %lld", h[w * 16 + 7] - h[w * 16 + 1], h[w * 16 + 8] - h[w * 16 + 7]);
            fprintf(stderr, "\n");
        }
    }
    if (timing && which != K_ATTN && which != K_LAYER) {
        double v[8 * 16];
        if (gemv_stamps(c, which, v, 1)) return -1;
        fprintf(stderr, "[timing] kernel class %d: per-wave s_memtime ticks (avg over workgroups)\n", which);
        for (int w = 0; w < 8; w++) {
            const double* d = v + w * 16;
            if (d[0] > 0) fprintf(stderr, "[timing]   wave %d: n=%d total=%.0f (max %.0f) barrier_wait=%.0f x_or_vmwait=%.0f rms_fold_or_walk=%.0f\n", w, (int)d[0], d[1], d[2], d[3], d[4], d[5]);
            if (d[0] > 0) { fprintf(stderr, "[timing]     stamps (since kernel start):"); for (int k = 0; k < 8; k++) fprintf(stderr, " %.0f", d[6 + k]); fprintf(stderr, "\n"); }
        }
    }
    return 0;
}


// ---- batched exact decode: several independent sequences per pass over the weights --------------------------------------------------
// The reference runs one generation per InferenceContext (src/inference/inference.go:174) and shares the weight matrix across the rows of
// a call (src/ml/operations_lineartransform.go:173-193).  A batch groups up to LNB_BATCH_MAX (128) contexts of ONE whole-model handle: per step every
// sequence's one-token Forward + Argmax happens in a single pass over the weights -- the sequences are the 16 columns of
// v_mfma_f32_16x16x4_f32, which evaluates each column's k-ordered chain exactly (lnb_batch_kernels.h) -- with per-sequence position, RoPE
// row, KV append and attention.  Every sequence's tokens and caches are bit-identical to its single-sequence run.
struct lnb_batch {
    lnb_model* m = nullptr; int n = 0; std::vector<lnb_ctx*> ctxs;
    Stream stream; Event ev0, ev1;         // (the stream is declared before everything enqueued on it: released last)
    Dev<BatchTab> tab; Dev<BatchKV> kv;    // (everything INSIDE the two tables aliases the members' state words, token words, logs and caches)
    Dev<uint16_t> x, h, xt, q, att_xt, ffn_xt, logits;
    Dev<int> derr; Dev<int32_t> d_tokens, d_pos; Pinned<int32_t> h_io;   // pinned: [0..MAX) tokens, [MAX..2 MAX) positions, [2 MAX] error word (MAX = LNB_BATCH_MAX)
    // the captured steps: greedy (a verify batch: the verify pass) / sampling (lnb_batch_decode_sample_until; a verify batch: lnb_decode_speculative_sample_until) /
    // pipeline stage (lnb_pipeline_tick_batch), each per attention form; the rows form is a verify batch's whose columns run the multi-row long-context pair
    Graphs graphs;
    int lds_T = 0; bool counted = false;   // lds_T: what the one-workgroup kernels' LDS arrays are sized for = min(maxT, their cap)
    // attention form (lnb_batch_set_attention).  maxT: the largest member seq_len; must_long: a member is beyond the one-workgroup kernels' reach;
    // attn_long: the form the NEXT enqueue / capture takes (chosen on the host per call: a captured graph fixes the kernel), one graph per form;
    // e_buf [n][H][maxT] / z_part [n][H][ceil(maxT/256)]: allocated when the long form is first needed, never inside a capture (a verify batch
    // borrows its context's: scratch_owned false)
    int maxT = 0; bool must_long = false, attn_long = false, tick_long = false, scratch_owned = true;
    int attn_long_T = 0x7FFFFFFF, force_zseq = 0, last_form = 0;
    Dev<double> e_own, z_own;              // the batch's own scratch (scratch_owned)
    double* e_buf = nullptr; double* z_part = nullptr;     // what the launches take: e_own / z_own, or (a verify batch) its context's sp_e_buf / sp_z_part
    Dev<LnbSampler> d_smp;                 // the device array of n samplers the sampling steps point at
    // a verify batch whose columns run the multi-row long-context pair (lnb_ctx_set_rows_attention, flags bit 1)
    bool attn_rows = false; int rows_zseq = 0;
    bool rows_form = false;                // the model carries no matrix-core copy: every product runs as ROWS of gemm_stream_kernel on the resident layouts, whatever n
    // pipeline stage (lnb_pipeline_tick_batch): the contiguous token words exchanged between the last and the first stage, the stage step
    // as a captured graph, events towards / from the exchange stream (as lnb_ctx has them for single-sequence ticks)
    Dev<int32_t> ring;
    PipeLink link;
    // token probabilities (the members' lnb_ctx_set_token_probs, one top_k for all): one row per sequence into its context's log (the records' members alias the contexts' logs)
    int top_k = 0; Dev<TokProbOut> tp_out; Dev<double> tp_zpart; Dev<uint64_t> tp_kpart; Dev<unsigned> tp_cnt;
    // speculative verify batch (lnb_decode_speculative_until): every column is ONE context (ctxs[s] = it, the same caches); columns s >= 1 take
    // their state and token word from col_st + s / col_tok + s instead of the context's own (the context's sp_st / sp_tok: it owns them)
    StepState* col_st = nullptr; int32_t* col_tok = nullptr;
    int* zseq = nullptr;                   // lnb_forward_append_many's pass batch has no member contexts: the serial-sum counter the attention launches get instead of ctxs[0]'s (AppendMany::zseq owns it)
};
// What every batched step asks of the model stage it runs on (who: the caller, as its message names it).  A whole-model handle is a stage of whole blocks.
static int batch_shape_check(const lnb_model* m, const char* who) {
    if (m->part_begin % 3 || m->part_end % 3) return fail("batched decode needs a stage of whole blocks (this one is cut inside a block: parts [%d, %d))", m->part_begin, m->part_end);
    if (m->a.dim % 128 || m->q_dim % 128 || m->ffn_hidden % 128)
        return fail("%s streams the weights in 128-step chunks: dim (%d), n_heads*head_dim (%d) and the FFN hidden size (%d) must be multiples of 128", who, m->a.dim, m->q_dim, m->ffn_hidden);
    return 0;
}
static int m16_copy(lnb_model* m, const TiledDesc& t, int rows, uint16_t** out) {
    const size_t bytes = m16_elems(rows, t.k, t.nch) * 2;
    if (arena_alloc(m->m16, out, bytes)) return -1;
    HIPCHK(hipMemsetAsync(*out, 0, bytes, m->stream));
    HIPCHK(lnbk_m16_from_tiled(t.w, *out, rows, t.k, t.rw, t.nch, m->stream));
    m->batch_bytes += (int64_t)bytes;
    return 0;
}
extern "C" int lnb_model_enable_batch(lnb_model* m) {
    if (!m) return fail("null argument");
    if (!m->finalized) return fail("model not finalized");
    if (m->batch_enabled) return 0;
    if (batch_shape_check(m, "batched decode")) return -1;
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(lnbk_batch_prepare());
    int rc = 0;
    for (auto& L : m->layers) {
        rc |= m16_copy(m, L.wqkv, L.wqkv.n_rows, &L.m_wqkv) | m16_copy(m, L.wo, m->a.dim, &L.m_wo) | m16_copy(m, L.w13, m->ffn_hidden, &L.m_w13) | m16_copy(m, L.w2, m->a.dim, &L.m_w2);
        if (rc) break;
    }
    if (!rc && m->last()) rc = m16_copy(m, m->output, m->a.vocab_size, &m->m_output);
    hipError_t e = hipStreamSynchronize(m->stream);
    if (!rc && e == hipSuccess) {                            // the prefill products find the copy through the matrix descriptors
        for (auto& L : m->layers) { L.wqkv.w16 = L.m_wqkv; L.wo.w16 = L.m_wo; L.w13.w16 = L.m_w13; L.w2.w16 = L.m_w2; }
        m->output.w16 = m->m_output;
    }
    if (rc || e != hipSuccess) {                             // (out of memory on a model that fills the HBM: the single-sequence paths stay usable)
        m->m16.reset();
        for (auto& L : m->layers) L.m_wqkv = L.m_wo = L.m_w13 = L.m_w2 = nullptr;
        m->m_output = nullptr; m->batch_bytes = 0;
        (void)hipGetLastError();                             // the failed hipMalloc leaves the thread's last-error set: every launcher ends with hipGetLastError()
        if (!rc) return fail("lnb_model_enable_batch: %s", hipGetErrorString(e));
        return -1;
    }
    m->batch_enabled = true;
    return 0;
}
extern "C" int64_t lnb_model_batch_bytes(lnb_model* m) { return m ? m->batch_bytes : 0; }

// The activation buffers of a batched step, N columns each (N a multiple of 16: the column forms keep B-operand layouts per group of 16),
// with the logits of a stage that owns the head and the error word.  All zero when allocated: the columns past n are never written by a
// live batch, whose width is fixed; a caller whose width changes re-zeroes the six (not the logits: every pass writes the rows it reads).
struct BatchBuf { Dev<uint16_t>* p; size_t bytes; };
static std::array<BatchBuf, 6> batch_bufs(lnb_batch* b, size_t N) {
    const lnb_model* m = b->m; const size_t dim = m->a.dim;
    return {{{&b->x, N * dim * 2}, {&b->h, N * dim * 2}, {&b->xt, N * dim * 2}, {&b->q, N * m->q_dim * 2}, {&b->att_xt, N * m->q_dim * 2}, {&b->ffn_xt, N * m->ffn_hidden * 2}}};
}
static int batch_bufs_zero(lnb_batch* b, size_t N) {
    for (const BatchBuf& f : batch_bufs(b, N)) HIPCHK(hipMemsetAsync(f.p->get(), 0, f.bytes, b->stream));
    return 0;
}
static int batch_bufs_alloc(lnb_batch* b, size_t N) {
    for (const BatchBuf& f : batch_bufs(b, N)) HIPCHK(dev_alloc(*f.p, f.bytes));
    if (batch_bufs_zero(b, N)) return -1;
    if (b->m->last()) {
        const size_t bytes = N * (size_t)b->m->a.vocab_size * 2;
        HIPCHK(dev_alloc(b->logits, bytes)); HIPCHK(hipMemsetAsync(b->logits, 0, bytes, b->stream));
    }
    HIPCHK(dev_alloc(b->derr, 16)); HIPCHK(hipMemsetAsync(b->derr, 0, 16, b->stream));
    return 0;
}
extern "C" int lnb_batch_destroy(lnb_batch* b) {
    if (!b) return 0;
    hipSetDevice(b->m->device);
    if (b->stream) hipStreamSynchronize(b->stream);
    if (b->counted) for (lnb_ctx* c : b->ctxs) c->batch_users--;
    delete b;
    return 0;
}
static int batch_alloc(lnb_batch* b) {
    lnb_model* m = b->m; const int n = b->n;
    HIPCHK(stream_create(b->stream, hipStreamNonBlocking));
    HIPCHK(event_create(b->ev0)); HIPCHK(event_create(b->ev1));
    HIPCHK(pinned_alloc(b->h_io, (2 * LNB_BATCH_MAX + 8) * 4, hipHostMallocDefault));
    BatchTab t{}; t.n = n;
    std::vector<BatchKV> kv(m->layers.size());
    for (int s = 0; s < LNB_BATCH_MAX; s++) {
        lnb_ctx* c = b->ctxs[s < n ? s : 0];                // (unused columns point at sequence 0's words: never dereferenced, never null)
        t.st[s] = c->st; t.dtok[s] = c->dtok; t.dout[s] = c->dout; t.dout_cap[s] = c->dout_cap; t.seq_len[s] = c->seq_len;
        if (b->col_st && s >= 1 && s < n) { t.st[s] = b->col_st + s; t.dtok[s] = b->col_tok + s; }
        for (size_t l = 0; l < m->layers.size(); l++) { kv[l].ck[s] = c->ck[l]; kv[l].cv[s] = c->cv[l]; }
    }
    HIPCHK(dev_alloc(b->tab, sizeof t)); HIPCHK(hipMemcpyAsync(b->tab, &t, sizeof t, hipMemcpyHostToDevice, b->stream));
    HIPCHK(dev_alloc(b->kv, kv.size() * sizeof(BatchKV)));
    HIPCHK(hipMemcpyAsync(b->kv, kv.data(), kv.size() * sizeof(BatchKV), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));                 // (the host copies above are stack / vector memory)
    // 1..16 sequences: activations in the B-operand layout [K][16 sequences], the columns past n stay zero for ever; 17..128: plain rows [n][K]
    // (whole column groups of 16: the 17..32-sequence form keeps B-operand layouts per group)
    if (batch_bufs_alloc(b, (size_t)((std::max(n, LNB_STREAM_COLS) + 15) / 16) * 16)) return -1;
    HIPCHK(dev_alloc(b->d_tokens, LNB_BATCH_MAX * 4)); HIPCHK(dev_alloc(b->d_pos, LNB_BATCH_MAX * 4));
    HIPCHK(dev_alloc(b->ring, LNB_BATCH_MAX * 4)); HIPCHK(hipMemsetAsync(b->ring, 0, LNB_BATCH_MAX * 4, b->stream));
    std::vector<TokProbOut> to(b->top_k > 0 ? n : 0);
    if (b->top_k > 0) {
        const size_t G = (size_t)lnb_tokprob_slices(n);
        for (int s = 0; s < n; s++) {
            const lnb_ctx* c = b->ctxs[s];
            to[s].st = c->st; to[s].ids = c->tp.ids; to[s].logit = c->tp.logit; to[s].prob = c->tp.prob; to[s].log_z = c->tp.logz;
            to[s].walks = c->zseq_count + 2; to[s].cap = c->dout_cap;
        }
        HIPCHK(dev_alloc(b->tp_out, n * sizeof(TokProbOut)));
        HIPCHK(hipMemcpyAsync(b->tp_out, to.data(), n * sizeof(TokProbOut), hipMemcpyHostToDevice, b->stream));
        HIPCHK(dev_alloc(b->tp_zpart, n * LNB_TOKPROB_MAX_G * 8)); HIPCHK(dev_alloc(b->tp_kpart, n * G * b->top_k * 8));
        HIPCHK(dev_alloc(b->tp_cnt, n * 4)); HIPCHK(hipMemsetAsync(b->tp_cnt, 0, n * 4, b->stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}
extern "C" int lnb_batch_create(lnb_ctx* const* ctxs, int n, lnb_batch** out) {
    if (!ctxs || !out) return fail("null argument");
    *out = nullptr;
    if (n < 1 || n > LNB_BATCH_MAX) return fail("a batch holds 1..%d sequences (got %d)", LNB_BATCH_MAX, n);
    for (int s = 0; s < n; s++) {
        if (!ctxs[s]) return fail("null context at index %d", s);
        if (ctxs[s]->m != ctxs[0]->m) return fail("context %d belongs to another model handle", s);
        for (int r = 0; r < s; r++) if (ctxs[r] == ctxs[s]) return fail("context %d appears twice in the batch", s);
        if (ctxs[s]->mode != LNB_MODE_EXACT) return fail("context %d is in the tolerance mode: batched decode is exact-order only", s);
        if (ctxs[s]->top_k != ctxs[0]->top_k)
            return fail("context %d records top-%d token probabilities, context 0 top-%d: a batch needs one setting", s, ctxs[s]->top_k, ctxs[0]->top_k);
    }
    lnb_model* m = ctxs[0]->m;
    HIPCHK(hipSetDevice(m->device));
    if (!m->batch_enabled) {
        // Round 5: a batch on a model WITHOUT the matrix-core copy runs every product as rows of the streaming product, which reads the RESIDENT
        // weight layouts (gemm_stream_kernel, SRC 1 / 2) -- any number of sequences.  The copy (lnb_model_enable_batch) is a pure performance
        // option: the column forms of up to 32 sequences (mfma_stream_kernel / mfma_pair_kernel) read it and are faster there.
        if (batch_shape_check(m, "batched decode")) return -1;
        HIPCHK(lnbk_batch_prepare());
    }
    lnb_batch* b = new lnb_batch();
    b->m = m; b->n = n; b->ctxs.assign(ctxs, ctxs + n); b->rows_form = !m->batch_enabled; b->top_k = ctxs[0]->top_k;
    for (int s = 0; s < n; s++) {
        if (lnbk_attn_long_layout_lds(ctxs[s]->seq_len) > 160 * 1024) {       // (neither lnb_ctx_create nor lnb_ctx_create_long makes such a context: cannot happen)
            const int sl = ctxs[s]->seq_len; delete b;
            return fail("context %d: seq_len %d is beyond what the long-context attention keeps in the LDS", s, sl);
        }
        b->maxT = std::max(b->maxT, ctxs[s]->seq_len);
        if (ctxs[s]->seq_len > ctxs[s]->attn_short_cap) b->must_long = true;
    }
    b->lds_T = std::min(b->maxT, ctxs[0]->attn_short_cap);
    b->tick_long = b->must_long;
    if (batch_alloc(b)) { lnb_batch_destroy(b); return -1; }
    for (lnb_ctx* c : b->ctxs) c->batch_users++;
    b->counted = true;
    *out = b;
    return 0;
}
// ---- attention form of a batched step (same bits either way).  The one-workgroup kernels (attn_exact_kernel / attn_gqa_kernel) stage a whole
// head in the LDS and stop at attn_short_cap positions; the long-context pair with a sequence dimension (lnb_kernels.hip, BATCH forms of
// attn_long_scores_kernel / attn_long_pv[2]_kernel) reaches every context lnb_ctx_create accepts.  A call takes the long form when a member's
// CAPACITY is beyond the cap (the short kernels cannot be launched for it) or when its largest position + 1 exceeds the batch's threshold
// (default: never -- a batch that fits the short kernels runs exactly what it ran before the long form existed).
static bool batch_want_long(const lnb_batch* b, int max_pos) { return b->must_long || max_pos + 1 > b->attn_long_T; }
// the e_buf [n][H][maxT] / z_part [n][H][ceil(maxT/256)] scratch of the batched long form (a batch's own, or the one a context's verify batches share)
static int attn_long_scratch(int n, int H, int maxT, Dev<double>& e_buf, Dev<double>& z_part, const char* whose, bool quiet) {
    if (e_buf && z_part) return 0;
    const size_t rows = (size_t)n * H, eb = rows * (size_t)maxT * 8, zb = rows * (size_t)((maxT + 255) / 256) * 8;
    hipError_t e = dev_alloc(e_buf, eb);
    if (e == hipSuccess) e = dev_alloc(z_part, zb);
    if (e != hipSuccess) {
        e_buf.reset(); z_part.reset(); (void)hipGetLastError();
        if (quiet) return -1;                                // (the caller has another way and records nothing)
        return fail("the long-context attention of %s needs %.1f MB of scratch (%d sequences x %d heads x %d positions): %s", whose, (double)(eb + zb) / 1e6,
                    n, H, maxT, hipGetErrorString(e));
    }
    return 0;
}
// a batch's OWN scratch for n columns of maxT positions (what it held before goes first), and the pointers its launches take
static int batch_own_scratch(lnb_batch* b, int n, int maxT, const char* whose) {
    b->e_own.reset(); b->z_own.reset(); b->e_buf = nullptr; b->z_part = nullptr;
    if (attn_long_scratch(n, b->m->a.n_heads, maxT, b->e_own, b->z_own, whose)) return -1;
    b->e_buf = b->e_own; b->z_part = b->z_own;
    return 0;
}
static int batch_long_scratch(lnb_batch* b) {
    if (b->e_buf && b->z_part) return 0;
    if (!b->scratch_owned) return fail("internal error: verify batch without its context's attention scratch");
    return batch_own_scratch(b, b->n, b->maxT, "this batch");
}
// selects the form of what is enqueued / captured next; allocates the scratch (host side of a call, outside any capture).  last_form (what
// lnb_batch_attention_form reports) is set by the callers once their launches have been accepted.
static int batch_select_form(lnb_batch* b, bool want_long) {
    if (want_long && batch_long_scratch(b)) return -1;
    b->attn_long = want_long;
    return 0;
}
// ... for a run that starts at these positions: the largest decides (a frozen sequence's negative position does not move the form)
static int batch_select_form_at(lnb_batch* b, const int32_t* start_pos) {
    int max_pos = 0;
    for (int s = 0; s < b->n; s++) max_pos = std::max(max_pos, start_pos[s]);
    return batch_select_form(b, batch_want_long(b, max_pos));
}
// A call that writes a member's caches from another stream: whatever the context's own stream still does to them comes first, and the call
// advances (or leaves behind) a device-side position the host no longer knows.
static int member_drain(lnb_ctx* c) {
    HIPCHK(hipStreamSynchronize(c->stream));
    c->dev_pos = -1; c->call_T = 0;
    return 0;
}
static void batch_attn_form(const lnb_batch* b, AttnParams& ap) {
    ap.lds_T = b->lds_T; ap.seq_len = b->attn_long ? b->maxT : b->lds_T;
    ap.longctx = b->attn_long ? 1 : 0; ap.force_zseq = b->attn_long ? (b->force_zseq & 1) : 0;
    ap.e_buf = b->e_buf; ap.z_part = b->z_part;
}
// the attention launch of a batched step: a verify batch in the rows form (its columns are consecutive rows of ONE context) runs the multi-row pair
static hipError_t batch_attn_launch(const lnb_batch* b, AttnParams& ap, hipStream_t st) {
    batch_attn_form(b, ap);
    if (!b->attn_rows) return lnbk_attn(&ap, st);
    ap.seq_len = b->maxT; ap.longctx = 1; ap.force_zseq = b->rows_zseq;
    return lnbk_attn_rows(&ap, -1, st);
}
static BatchPlan batch_plan_of(const lnb_batch* b) { return batch_plan(b->n, !b->rows_form, knob(Knob::BATCH_GROUPS)); }
static bool stream_acc2(const StreamParams& p) { return p.nch == 2 || p.n_chains > 4 * g_num_cus; }   // thin matrices: one tile per wave, every tile on its own SIMD
// One product of a batched step: what is multiplied and where the result goes.  Through which feed is the plan's business (lnb_batchplan.h).
// norm_w: the RMSNorm of `in` into b->xt runs in front and the product reads b->xt; nullptr: the product reads `in`.
struct BatchProd {
    BatchProduct id; const uint16_t* norm_w; const uint16_t* in;
    const TiledDesc* t; const uint16_t* m16; int K, n_rows, nch, epi;
    uint16_t* out = nullptr; uint16_t* out_xt = nullptr; const uint16_t* res = nullptr;
    const BatchKV* kv = nullptr;           // EPI_QKV_ROPE: the layer's caches
};
// The norm launch and the product launch of one product, through the feed the plan gives it.
// COLUMN with plan.groups (17 .. 32 sequences, LNB_BATCH_GROUPS=0: off): the thin matrices -- one k-ordered chain per 16-row tile and 16 columns -- as
// TWO column groups of mfma_pair_kernel on disjoint CUs (256-384 tiles x 2 groups: every CU carries two chains) instead of rows of gemm_stream_kernel
// (one chain per wave, its operands unpacked by the same wave); the fat matrices stay rows.  The activations between them change layout at their
// producers: norm -> xt groups (batch_rmsnorm_xt_kernel), attention -> out_xt groups, SiLU*up epilogue -> out_xt groups.
// ROW: the batch's rows through the prefill's streaming product (gemm_stream_kernel: weights M16 -> A operand, 1 / 2 / 4 batch tiles of 16 sequences
// per wave), plain row-major activations.  Same chains per sequence; EPI_QKV_ROPE and the attention take each row's position and caches from the
// batch tables.  (xt / att_xt / ffn_xt hold rows here, not the B-operand layout; m16 == nullptr -- no matrix-core copy: the resident layout t feeds
// the same kernel, gemm_stream_kernel SRC 1 / 2.)
static int enqueue_batch_product(lnb_batch* b, const BatchPlan& plan, const BatchProd& d) {
    lnb_model* m = b->m; hipStream_t st = b->stream;
    const bool column = plan.feed[d.id] == FEED_COLUMN;
    const uint16_t* x = d.in;
    if (d.norm_w) {
        if (column) HIPCHK(lnbk_batch_rmsnorm(d.in, d.norm_w, m->a.norm_eps, b->xt, d.K, b->n, st));
        else HIPCHK(lnbk_rmsnorm_rows(d.in, d.norm_w, b->xt, b->n, d.K, m->a.norm_eps, st));
        x = b->xt;
    }
    if (column) {
        const int G = plan.groups;
        StreamParams p{}; p.w = d.m16; p.xt = x; p.K = d.K; p.n_rows = d.n_rows; p.nch = G ? 1 : d.nch; p.n_chains = ((d.n_rows + 15) / 16) * p.nch;
        p.nseq = b->n; p.n_groups = G; p.dbg = G ? nullptr : g_dbg;
        p.out = d.out; p.out_xt = d.out_xt; p.res = d.res;
        if (d.epi == EPI_SILU_MUL) p.silu = m->silu;
        if (d.epi == EPI_QKV_ROPE) { p.cis = m->cis; p.q_out = b->q; p.tab = b->tab; p.kv = d.kv; p.q_dim = m->q_dim; p.kv_dim = m->kv_dim; p.head_dim = m->head_dim; }
        HIPCHK(lnbk_stream(&p, d.epi, G ? 0 : stream_acc2(p), g_num_cus, st));
        return 0;
    }
    GemmParams g{}; g.w16 = d.m16; g.w = d.t->w; g.rw = d.t->rw; g.nch = d.nch; g.x = x; g.K = d.K; g.n_rows = d.n_rows; g.S = b->n;
    g.out = d.out; g.out_xt = d.out_xt; g.res = d.res;
    if (d.epi == EPI_SILU_MUL) g.silu = m->silu;
    if (d.epi == EPI_QKV_ROPE) { g.cis = m->cis; g.q_out = b->q; g.btab = b->tab; g.bkv = d.kv; g.q_dim = m->q_dim; g.kv_dim = m->kv_dim; g.head_dim = m->head_dim; }
    HIPCHK(lnbk_gemm_stream(&g, d.epi, g_num_cus, st));
    return 0;
}
// which: K_QKV (attention norm + wq|wk|wv + RoPE + KV append), K_ATTN, K_WO, K_W13 (ffn norm + w1|w3 + SiLU*up), K_W2, K_HEAD (norm + output)
// A producer writes the layout its consumer's feed reads: the attention for wo, the SiLU*up epilogue of w1|w3 for w2.
static int enqueue_batch_kernel(lnb_batch* b, int l, int which) {
    lnb_model* m = b->m; const lnb_model_args& a = m->a;
    const int dim = a.dim, F = m->ffn_hidden;
    const BatchPlan plan = batch_plan_of(b);
    if (which == K_HEAD) {
        BatchProd d{BP_HEAD, m->norm, b->x, &m->output, m->m_output, dim, a.vocab_size, 1, EPI_STORE}; d.out = b->logits;
        return enqueue_batch_product(b, plan, d);
    }
    LayerW& L = m->layers[l - m->layer_begin];
    const BatchKV* kv = b->kv + (l - m->layer_begin);
    switch (which) {
    case K_QKV: {
        BatchProd d{BP_QKV, L.attn_norm, b->x, &L.wqkv, L.m_wqkv, dim, L.wqkv.n_rows, 1, EPI_QKV_ROPE}; d.kv = kv;
        return enqueue_batch_product(b, plan, d); }
    case K_ATTN: {
        const bool wo_column = plan.feed[BP_WO] == FEED_COLUMN;
        AttnParams ap{}; ap.q = b->q; ap.out = wo_column ? nullptr : b->att_xt; ap.out_xt = wo_column ? b->att_xt : nullptr; ap.btab = b->tab; ap.bkv = kv; ap.dbg = nullptr;
        ap.S = b->n; ap.H = a.n_heads; ap.KVH = a.n_kv_heads; ap.hd = m->head_dim; ap.host_T = 0;
        ap.divisor = bf_wide_h(bf_trunc_h((float)std::sqrt((double)m->head_dim)));
        ap.zseq_count = b->zseq ? b->zseq : b->ctxs[0]->zseq_count; ap.exp_tab = m->exp_tab;     // (attn_gqa_kernel looks exp up)
        HIPCHK(batch_attn_launch(b, ap, b->stream)); return 0; }
    case K_WO: {
        BatchProd d{BP_WO, nullptr, b->att_xt, &L.wo, L.m_wo, m->q_dim, dim, 1, EPI_RESID}; d.out = b->h; d.res = b->x;
        return enqueue_batch_product(b, plan, d); }
    case K_W13: {
        BatchProd d{BP_W13, L.ffn_norm, b->h, &L.w13, L.m_w13, dim, F, 2, EPI_SILU_MUL};
        if (plan.feed[BP_W2] == FEED_COLUMN) d.out_xt = b->ffn_xt; else d.out = b->ffn_xt;
        return enqueue_batch_product(b, plan, d); }
    case K_W2: {
        BatchProd d{BP_W2, nullptr, b->ffn_xt, &L.w2, L.m_w2, F, dim, 1, EPI_RESID}; d.out = b->x; d.res = b->h;
        return enqueue_batch_product(b, plan, d); }
    }
    return fail("bad kernel id");
}
// One batched pass over this model STAGE's weights: the embedding gather on the first stage (otherwise the hidden states [n, dim] are
// already in b->x: received from the stage before), the owned blocks, and on the last stage norm + output.  What follows the logits
// (token probabilities, argmax, commit, ...) is the caller's.
static int enqueue_batch_blocks(lnb_batch* b, int l) {
    for (int k = K_QKV; k <= K_W2; k++) if (enqueue_batch_kernel(b, l, k)) return -1;
    return 0;
}
static int enqueue_batch_pass(lnb_batch* b) {
    lnb_model* m = b->m;
    if (m->first()) HIPCHK(lnbk_batch_embed(m->tok_embd, b->tab, b->x, b->n, m->a.dim, m->a.vocab_size, b->derr, b->stream));
    for (int l = m->layer_begin; l < m->layer_end; l++) if (enqueue_batch_blocks(b, l)) return -1;
    return m->last() ? enqueue_batch_kernel(b, 0, K_HEAD) : 0;
}
// One batched step of this model STAGE: the pass, and on the last stage the argmax (which advances every sequence's position); a stage
// without the head advances the positions itself.  ring_in: the first stage of a multi-stage pipeline takes the tokens from the contiguous
// words the last stage sent (lnb_pipeline_tick_batch).
static int enqueue_batch_step(lnb_batch* b, bool ring_in = false, bool sample = false) {
    lnb_model* m = b->m;
    if (ring_in && m->first()) HIPCHK(lnbk_batch_scatter_ring(b->tab, b->ring, b->stream));
    if (enqueue_batch_pass(b)) return -1;
    if (m->last() && sample) {                               // every member's own sampler (lnb_batch_decode_sample_until: a whole model, no token probabilities)
        HIPCHK(lnbk_batch_sample(b->logits, m->a.vocab_size, m->prob_etab, b->d_smp, b->tab, b->n, b->stream));
    } else if (m->last()) {
        if (b->top_k > 0) {                                  // (ticks refuse such batches: only lnb_batch_decode[_until] gets here with it)
            TokProbParams p = tp_params(m, b->logits, b->n, b->top_k, b->tp_zpart, b->tp_kpart, b->tp_cnt, b->tp_out, 1);
            HIPCHK(lnbk_token_probs(&p, b->stream));
        }
        HIPCHK(lnbk_batch_argmax(b->logits, m->a.vocab_size, b->tab, b->n, b->ring, b->stream));
    } else HIPCHK(lnbk_batch_advance(b->tab, b->stream));
    return 0;
}
static int batch_decode_impl(lnb_batch* b, const int32_t* tokens, const int32_t* start_pos, int n_steps, int32_t* out_tokens, int32_t* n_generated, int32_t* finished, float* ms_out,
                             const lnb_sampler* smp = nullptr);
extern "C" int lnb_batch_decode(lnb_batch* b, const int32_t* tokens, const int32_t* start_pos, int n_steps, int32_t* out_tokens, float* ms_out) {
    return batch_decode_impl(b, tokens, start_pos, n_steps, out_tokens, nullptr, nullptr, ms_out);     // n_steps tokens per sequence: stop ids are not compared
}
// with per-sequence stop ids (lnb_ctx_set_stop_ids on the member contexts): n_generated[s] tokens of row s of out_tokens are valid; a finished
// sequence's column keeps computing its last step (the pass over the weights is shared), its state and caches stay where they stopped
// finished[s] (optional) = 1 if a stop id ended sequence s: n_generated[s] == max_steps alone cannot tell a run that stopped on its last step from
// one that did not.  A caller that decodes in chunks passes start_pos[s] < 0 for a sequence that has finished: it stays frozen (nothing of it is
// touched, n_generated[s] = 0, finished[s] = 1) instead of being restarted from its stop token.
extern "C" int lnb_batch_decode_until(lnb_batch* b, const int32_t* tokens, const int32_t* start_pos, int max_steps, int32_t* out_tokens, int32_t* n_generated, int32_t* finished, float* ms_out) {
    if (!n_generated) return fail("null argument");
    return batch_decode_impl(b, tokens, start_pos, max_steps, out_tokens, n_generated, finished, ms_out);
}
// lnb_batch_decode_until with one sampler per member (include/lnb.h).  The samplers are checked as far as the caller's n reaches: the batch's own n is
// behind the handle, so the loop over them runs after the NULL checks and before anything else of the batch is used.
extern "C" int lnb_batch_decode_sample_until(lnb_batch* b, const lnb_sampler* samplers, const int32_t* tokens, const int32_t* start_pos, int max_steps, int32_t* out_tokens,
                                             int32_t* n_generated, int32_t* finished, float* ms_out) {
    if (!b || !samplers || !tokens || !start_pos || !out_tokens || !n_generated) return fail("null argument");
    return batch_decode_impl(b, tokens, start_pos, max_steps, out_tokens, n_generated, finished, ms_out, samplers);
}
static int batch_decode_impl(lnb_batch* b, const int32_t* tokens, const int32_t* start_pos, int n_steps, int32_t* out_tokens, int32_t* n_generated, int32_t* finished, float* ms_out,
                             const lnb_sampler* smp) {
    if (!b || !tokens || !start_pos || !out_tokens) return fail("null argument");
    lnb_model* m = b->m;
    if (smp) {
        char who[32];
        for (int s = 0; s < b->n; s++) { snprintf(who, sizeof who, "sequence %d: ", s); if (sampler_check(smp + s, who)) return -1; }
    }
    if (!m->first() || !m->last()) return fail("%s needs a whole-model handle; pipeline stages run their batches through lnb_pipeline_tick_batch", smp ? "lnb_batch_decode_sample_until" : "lnb_batch_decode");
    if (smp) {
        if (sample_vocab_check(m->a.vocab_size)) return -1;
        for (int s = 0; s < b->n; s++) if (b->ctxs[s]->top_k > 0) return fail("sequence %d: its context %s", s, k_sample_probs_advice);
    }
    HIPCHK(hipSetDevice(m->device));
    if (n_steps <= 0) return fail("n_steps must be positive");
    for (int s = 0; s < b->n; s++) {
        lnb_ctx* c = b->ctxs[s];
        if (n_steps > c->dout_cap) return fail("sequence %d: n_steps %d exceeds the context length %d", s, n_steps, c->dout_cap);
        const bool frozen = start_pos[s] < 0;                 // an ended sequence of a chunked run (lnb_batch_decode_until): nothing of it is touched
        if (frozen && !n_generated) return fail("sequence %d: negative start position (only lnb_batch_decode_until takes one, for a sequence that has finished)", s);
        if (!frozen && (check_call(c, 1, start_pos[s]) || check_call(c, 1, start_pos[s] + n_steps - 1))) return -1;
        if (!frozen && (tokens[s] < 0 || tokens[s] >= m->a.vocab_size)) return fail("sequence %d: token id at index 0 is outside the vocabulary", s);
        if (c->pending) return fail("sequence %d: a lnb_forward_stage_begin has not been ended", s);
        if (member_drain(c)) return -1;
    }
    for (lnb_ctx* c : b->ctxs) { c->tp_last_k = 0; c->tp_last_n = 0; }
    hipStream_t st = b->stream;
    if (batch_select_form_at(b, start_pos)) return -1;
    const bool use_graph = knob(Knob::NO_GRAPH) == 0;
    GraphExec& gslot = b->graphs.slot(smp ? GL_SAMPLE : GL_GREEDY, b->attn_long ? GF_LONG : GF_SHORT);       // one captured step per form
    if (smp && !b->d_smp) HIPCHK(dev_alloc(b->d_smp, (size_t)LNB_BATCH_MAX * sizeof(LnbSampler)));
    if (use_graph && capture_once(gslot, st, [&] { return enqueue_batch_step(b, false, smp != nullptr); })) return -1;
    if (smp) HIPCHK(hipMemcpyAsync(b->d_smp, smp, (size_t)b->n * sizeof(LnbSampler), hipMemcpyHostToDevice, st));
    memcpy(b->h_io, tokens, (size_t)b->n * 4); memcpy(b->h_io + LNB_BATCH_MAX, start_pos, (size_t)b->n * 4);
    HIPCHK(hipMemcpyAsync(b->d_tokens, b->h_io, (size_t)b->n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->d_pos, b->h_io + LNB_BATCH_MAX, (size_t)b->n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b->derr, 0, 4, st));
    HIPCHK(lnbk_batch_set_state(b->tab, b->d_tokens, b->d_pos, b->ring, n_generated ? 1 : 0, st));
    HIPCHK(hipEventRecord(b->ev0, st));
    for (int i = 0; i < n_steps; i++) {
        if (use_graph) HIPCHK(hipGraphLaunch(gslot, st));
        else if (enqueue_batch_step(b, false, smp != nullptr)) return -1;
    }
    HIPCHK(hipEventRecord(b->ev1, st));
    b->last_form = b->attn_long ? 1 : 0;
    for (int s = 0; s < b->n; s++)
        HIPCHK(hipMemcpyAsync(out_tokens + (size_t)s * n_steps, b->ctxs[s]->dout, (size_t)n_steps * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b->h_io + 2 * LNB_BATCH_MAX, b->derr, 4, hipMemcpyDeviceToHost, st));
    std::vector<StepState> hs(n_generated ? b->n : 0);
    for (int s = 0; s < (int)hs.size(); s++) HIPCHK(hipMemcpyAsync(&hs[s], b->ctxs[s]->st, sizeof(StepState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms_out) HIPCHK(hipEventElapsedTime(ms_out, b->ev0, b->ev1));
    if (b->h_io[2 * LNB_BATCH_MAX]) return fail("sequence %d: generated token id is outside the vocabulary", b->h_io[2 * LNB_BATCH_MAX] - 1);
    for (int s = 0; s < (int)hs.size(); s++) { n_generated[s] = hs[s].n_out; if (finished) finished[s] = hs[s].finished; }
    for (int s = 0; s < b->n; s++) { b->ctxs[s]->tp_last_k = b->top_k; b->ctxs[s]->tp_last_n = n_generated ? n_generated[s] : n_steps; }
    return 0;
}
// what a batched tick exchanges, for a host layer that moves it itself (lnb_pipeline_init_host)
extern "C" void* lnb_batch_boundary_ptr(lnb_batch* b, int which) {
    if (!b) { fail("null argument"); return nullptr; }
    if (which == 0) return b->x;
    if (which == 1) return b->ring;
    fail("lnb_batch_boundary_ptr: which = %d (0: hidden states [n, dim] bf16, 1: the n token words)", which);
    return nullptr;
}
extern "C" int lnb_batch_check_error(lnb_batch* b) {
    if (!b) return fail("null argument");
    HIPCHK(hipSetDevice(b->m->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    int h = 0;
    HIPCHK(hipMemcpy(&h, b->derr, 4, hipMemcpyDeviceToHost));
    if (h) {
        HIPCHK(hipMemset(b->derr, 0, 4));
        return fail("batched pipeline step: a token id outside the vocabulary (or an all-NaN logits row) in one of the batch's sequences since the last check");
    }
    return 0;
}
// Every sequence's position (and, on the first stage, optionally its next input token) before a run of lnb_pipeline_tick_batch steps: the
// positions then advance on the device with every step.  tokens == NULL keeps what each context's token word holds (what the
// single-sequence prefill ticks left there).
extern "C" int lnb_batch_set_state(lnb_batch* b, const int32_t* tokens, const int32_t* start_pos) {
    if (!b || !start_pos) return fail("null argument");
    HIPCHK(hipSetDevice(b->m->device));
    HIPCHK(hipMemsetAsync(b->derr, 0, 4, b->stream));        // a fresh run: forget what an earlier one latched
    const bool one_stage = b->m->first() && b->m->last();
    for (int s = 0; s < b->n; s++) {
        lnb_ctx* c = b->ctxs[s];
        if (check_call(c, 1, start_pos[s])) return -1;
        if (tokens && (tokens[s] < 0 || tokens[s] >= b->m->a.vocab_size)) return fail("sequence %d: token id at index 0 is outside the vocabulary", s);
        // only the LAST stage's argmax sees a stop id: the other stages would go on advancing their positions, re-embedding the stale ring token
        // and appending KV rows behind the stop.  Stop ids in a multi-stage batched pipeline belong to the host: it reads the tokens.
        if (c->top_k > 0 && !one_stage)
            return fail("sequence %d: its context records token probabilities, which pipeline stages do not support (lnb_ctx_set_token_probs(ctx, 0))", s);
        if (c->n_stop > 0 && !one_stage)
            return fail("sequence %d: its context carries %d stop ids, which a batched tick of a multi-stage pipeline cannot honour (only the last stage sees the "
                        "token): clear them (lnb_ctx_set_stop_ids(ctx, NULL, 0)) and end the sequence on the host", s, c->n_stop);
        c->dev_pos = -1; c->call_T = 0;
    }
    if (batch_select_form_at(b, start_pos)) return -1;
    b->tick_long = b->attn_long;                             // the ticks that follow run the form this start calls for (lnb_pipeline_tick_batch)
    HIPCHK(hipDeviceSynchronize());                          // a setup call: whatever the contexts' streams and the pipe's exchange stream still do
                                                             // (the prefill's token hand-off into the contexts' token words) comes first
    if (tokens) memcpy(b->h_io, tokens, (size_t)b->n * 4);
    memcpy(b->h_io + LNB_BATCH_MAX, start_pos, (size_t)b->n * 4);
    if (tokens) HIPCHK(hipMemcpyAsync(b->d_tokens, b->h_io, (size_t)b->n * 4, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->d_pos, b->h_io + LNB_BATCH_MAX, (size_t)b->n * 4, hipMemcpyHostToDevice, b->stream));
    HIPCHK(lnbk_batch_set_state(b->tab, tokens ? b->d_tokens : nullptr, b->d_pos, b->ring, one_stage ? 1 : 0, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}
// measurement aid (bench.py): average HIP-event time of ONE kernel class of the batched step (which as in lnb_profile_kernel; the norm
// launches count with the product they feed), consecutive launches cycling through the layers; every sequence is placed at `pos`
extern "C" int lnb_batch_profile_kernel(lnb_batch* b, int which, int pos, int iters, float* avg_ms_out) {
    if (!b || !avg_ms_out) return fail("null argument");
    lnb_model* m = b->m;
    HIPCHK(hipSetDevice(m->device));
    if (iters <= 0 || which < 0 || which > K_LAYER) return fail("bad arguments");
    if (which == K_HEAD && !m->last()) return fail("this stage does not own output.weight");
    for (int s = 0; s < b->n; s++) { if (check_call(b->ctxs[s], 1, pos)) return -1; b->h_io[s] = 0; b->h_io[LNB_BATCH_MAX + s] = pos; b->ctxs[s]->dev_pos = -1; }
    if (batch_select_form_at(b, b->h_io + LNB_BATCH_MAX)) return -1;
    hipStream_t st = b->stream;
    HIPCHK(hipMemcpyAsync(b->d_tokens, b->h_io, (size_t)b->n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->d_pos, b->h_io + LNB_BATCH_MAX, (size_t)b->n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(lnbk_batch_set_state(b->tab, b->d_tokens, b->d_pos, b->ring, 0, st));
    const int nl = m->layer_end - m->layer_begin;
    auto run = [&](int i) -> int {
        const int l = m->layer_begin + i % nl;
        if (which == K_HEAD) return enqueue_batch_kernel(b, 0, K_HEAD);
        if (which == K_LAYER) return enqueue_batch_blocks(b, l);
        return enqueue_batch_kernel(b, l, which);
    };
    for (int i = 0; i < 3; i++) if (run(i)) return -1;
    HIPCHK(hipEventRecord(b->ev0, st));
    for (int i = 0; i < iters; i++) if (run(i + 3)) return -1;
    HIPCHK(hipEventRecord(b->ev1, st));
    b->last_form = b->attn_long ? 1 : 0;
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    *avg_ms_out = ms / (float)iters;
    return 0;
}

// ---- lnb_forward_append_many (include/lnb.h): n contexts extended by n_rows[s] rows each, in passes of up to LNB_APPEND_MANY_COLS rows over the weights.
// A pass IS a batched step (enqueue_batch_kernel: the column forms, the column groups, rows of gemm_stream_kernel -- whatever its width selects) on a
// lnb_batch that has no member contexts: its buffers hold 128 columns, its column states and token words are the call's own, and its BatchTab / BatchKV
// are rewritten on the device at the start of every pass (append_many_setup_kernel) from the row and member tables the call uploaded once.  Two things
// differ from a live batch (and are why this is not lnb_batch_decode on a temporary batch):
//   * the width changes from pass to pass on ONE set of activation buffers, so "columns past n stay zero for ever" (batch_alloc) has to be re-established:
//     the buffers are zeroed whenever a pass is narrower than the one before or changes layout (B-operand columns / column groups / rows);
//   * nothing may advance a position or log a token: batch_argmax_kernel and spec_commit_kernel are never launched, the tab's token logs point at a
//     dummy with capacity 0, and only append_many_finish_kernel reads the logits.
// lnb_decode_speculative_many's own tables beside the pass object (created on its first call): SmPass's device arrays in one allocation, the
// members' text heads (history ++ token, concatenated; grown on demand), the pinned block the pack kernel reports into, the events of the loop
struct SpecMany {
    Dev<char> dev; SmPass p{};              // (p's device arrays are carved out of dev; p.word is the device address of `word`)
    DevGrown<int32_t> text;
    Pinned<int32_t> word; Event ev, ev0, ev1;
};
struct AppendMany {
    lnb_batch* b = nullptr;                 // stream, activation buffers and logits for LNB_BATCH_MAX columns, tab / kv filled per pass (append_many_free destroys it)
    Dev<StepState> st; Dev<int32_t> tok, dummy_log; Dev<int> zseq;
    DevGrown<AmRow> rows;                   // the call's row table (grown on demand)
    Dev<char> members;                      // AmMembers + one BatchKV per layer, indexed by member
    Dev<int32_t> d_arg; Pinned<int32_t> h_arg;              // [LNB_BATCH_MAX] argmax per member: device, pinned host
    Pinned<uint16_t> pin[2]; Event ev[2];   // logits of a pass on their way to the host, two passes in flight
    int scratch_n = 0, scratch_T = 0;       // what b->e_own / b->z_own hold: columns x positions of the long-context pair
    int last_layout = -1, last_width = 0;   // what the activation buffers were last used as
    int passes = 0, max_columns = 0, long_passes = 0;      // lnb_model_append_many_info
    SpecMany* sm = nullptr;                 // lnb_decode_speculative_many runs its passes on this object (append_many_free deletes it)
};
// everything the object holds was enqueued on its batch's stream: that drains first, the batch (and its stream) goes last
static void append_many_free(lnb_model* m) {
    AppendMany* am = m->am;
    if (!am) return;
    if (am->b && am->b->stream) hipStreamSynchronize(am->b->stream);
    delete am->sm;
    lnb_batch* b = am->b;
    delete am;
    if (b) lnb_batch_destroy(b);
    m->am = nullptr;
}
static int append_many_alloc(lnb_model* m) {
    if (m->am) return 0;
    AppendMany* am = new AppendMany();
    m->am = am;                                              // (a failure below leaves a partial object: lnb_model_destroy frees it, the next call starts over)
    auto bail = [&]() { append_many_free(m); return -1; };
    lnb_batch* b = new lnb_batch();
    am->b = b; b->m = m; b->n = 1; b->scratch_owned = true;
    const size_t N = LNB_BATCH_MAX, L = m->layers.size();
    auto dalloc = [&](auto& p, size_t bytes) -> int { HIPCHK(dev_alloc(p, bytes)); HIPCHK(hipMemsetAsync(p.get(), 0, bytes, b->stream)); return 0; };
    if (stream_create(b->stream, hipStreamNonBlocking) != hipSuccess) { fail("lnb_forward_append_many: no stream"); return bail(); }
    if (batch_bufs_alloc(b, N) || dalloc(b->tab, sizeof(BatchTab)) || dalloc(b->kv, L * sizeof(BatchKV)) ||
        dalloc(am->st, N * sizeof(StepState)) || dalloc(am->tok, N * 4) || dalloc(am->dummy_log, 64) || dalloc(am->zseq, 16) ||
        dalloc(am->members, sizeof(AmMembers) + L * sizeof(BatchKV)) || dalloc(am->d_arg, N * 4)) return bail();
    b->zseq = am->zseq;
    if (pinned_alloc(am->h_arg, N * 4, hipHostMallocDefault) != hipSuccess) { fail("lnb_forward_append_many: no pinned host memory"); return bail(); }
    for (int i = 0; i < 2; i++) if (event_create(am->ev[i], hipEventDisableTiming) != hipSuccess) { fail("lnb_forward_append_many: no event"); return bail(); }
    BatchTab t{};                                            // the pointers of a column never change: its own state and token word, the dummy log (capacity 0: nothing is ever logged)
    for (int c = 0; c < LNB_BATCH_MAX; c++) { t.st[c] = am->st + c; t.dtok[c] = am->tok + c; t.dout[c] = am->dummy_log; t.dout_cap[c] = 0; t.seq_len[c] = 0; }
    if (hipMemcpyAsync(b->tab, &t, sizeof t, hipMemcpyHostToDevice, b->stream) != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess) {
        fail("lnb_forward_append_many: uploading the column table failed"); return bail();
    }
    return 0;
}
extern "C" int lnb_model_append_many_info(const lnb_model* m, int* passes, int* max_columns, int* long_passes) {
    if (!m) return fail("lnb_model_append_many_info: null argument (model)");
    const AppendMany* am = m->am;
    if (passes) *passes = am ? am->passes : 0;
    if (max_columns) *max_columns = am ? am->max_columns : 0;
    if (long_passes) *long_passes = am ? am->long_passes : 0;
    return 0;
}
extern "C" int lnb_forward_append_many(lnb_ctx* const* ctxs, int n, const int32_t* tokens, const int32_t* n_rows, const int32_t* start_pos,
                                       float* logits_out, int32_t* argmax_out) {
    const char* const name = "lnb_forward_append_many";
    // ---- the arguments alone: no handle is dereferenced
    if (!ctxs || !tokens || !n_rows || !start_pos) return fail("%s: null argument (%s)", name, !ctxs ? "ctxs" : !tokens ? "tokens" : !n_rows ? "n_rows" : "start_pos");
    if (n < 1 || n > LNB_BATCH_MAX) return fail("%s: a call takes 1..%d contexts (got %d)", name, LNB_BATCH_MAX, n);
    for (int s = 0; s < n; s++) {
        if (!ctxs[s]) return fail("%s: null context at index %d", name, s);
        if (n_rows[s] < 1) return fail("%s: member %d: n_rows must be positive (got %d)", name, s, n_rows[s]);
        if (start_pos[s] < 0) return fail("%s: member %d: negative start position %d", name, s, start_pos[s]);
        for (int r = 0; r < s; r++) if (ctxs[r] == ctxs[s]) return fail("%s: context %d appears twice (also at index %d)", name, s, r);
    }
    const int W = knob(Knob::APPEND_MANY_COLS);
    if (W < 1 || W > LNB_BATCH_MAX) return fail("%s: LNB_APPEND_MANY_COLS=%d is not a pass width (1..%d)", name, W, LNB_BATCH_MAX);
    // ---- the handles: everything is checked before any cache is written
    lnb_model* m = ctxs[0]->m;
    for (int s = 0; s < n; s++) if (ctxs[s]->m != m) return fail("%s: context %d belongs to another lnb_model handle", name, s);
    if (!m->first() || !m->last()) return fail("%s needs a whole-model handle: pipeline stages have no append", name);
    if (batch_shape_check(m, name)) return -1;
    const int V = m->a.vocab_size;
    int64_t total = 0;
    for (int s = 0; s < n; s++) {
        const lnb_ctx* c = ctxs[s];
        if (c->mode != LNB_MODE_EXACT) return fail("%s: context %d is in the tolerance mode: the call is exact-mode only", name, s);
        if (c->pending) return fail("%s: context %d: a lnb_forward_stage_begin has not been ended", name, s);
        const int64_t T = (int64_t)start_pos[s] + n_rows[s];
        if (T > m->cis_rows) return fail("%s: member %d: position %lld is beyond the %d-row RoPE table", name, s, (long long)T, m->cis_rows);
        if (T > c->seq_len) return fail("%s: member %d: position %lld is beyond the KV cache of %d", name, s, (long long)T, c->seq_len);
        if (lnbk_attn_long_layout_lds(c->seq_len) > 160 * 1024) return fail("%s: member %d: seq_len %d is beyond what the long-context attention keeps in the LDS", name, s, c->seq_len);
        total += n_rows[s];
    }
    for (int64_t i = 0; i < total; i++)
        if (tokens[i] < 0 || tokens[i] >= V) return fail("%s: token id %d at row %lld is outside the vocabulary", name, tokens[i], (long long)i);
    // ---- the call's tables on the host: one AmRow per row, the members' cache lengths and cache pointers; per pass its attention form
    std::vector<AmRow> rows((size_t)total);
    { size_t i = 0;
      for (int s = 0; s < n; s++) for (int r = 0; r < n_rows[s]; r++, i++) rows[i] = AmRow{s, start_pos[s] + r, tokens[i], r == n_rows[s] - 1 ? 1 : 0}; }
    const size_t L = m->layers.size();
    std::vector<char> members(sizeof(AmMembers) + L * sizeof(BatchKV));
    { AmMembers* hm = (AmMembers*)members.data(); BatchKV* hk = (BatchKV*)(members.data() + sizeof(AmMembers));
      hm->n = n;
      for (int s = 0; s < LNB_BATCH_MAX; s++) {
          const lnb_ctx* c = ctxs[s < n ? s : 0];
          hm->seq_len[s] = c->seq_len;
          for (size_t l = 0; l < L; l++) { hk[l].ck[s] = c->ck[l]; hk[l].cv[s] = c->cv[l]; }
      } }
    RowPackWalk walk; RowSeg segs[ROWPACK_MAX_W]; int width = 0; int64_t row0 = 0;
    int need_n = 0, need_T = 0;                              // the long-context pair's scratch over every pass that runs it
    if (rowpack_begin(&walk, n, n_rows, W)) return fail("%s: internal error: the rows could not be packed", name);
    while (int ns = rowpack_next(&walk, segs, &width, &row0)) {
        bool lng = false; int maxT = 0;
        for (int g = 0; g < ns; g++) { const lnb_ctx* c = ctxs[segs[g].member]; maxT = std::max(maxT, c->seq_len); lng = lng || c->seq_len > c->attn_short_cap; }
        if (lng) { need_n = std::max(need_n, width); need_T = std::max(need_T, maxT); }
    }
    std::lock_guard<std::mutex> lock(m->am_mu);
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(lnbk_batch_prepare());
    if (append_many_alloc(m)) return -1;
    AppendMany* am = m->am; lnb_batch* b = am->b; hipStream_t st = b->stream;
    if (need_n > am->scratch_n || need_T > am->scratch_T) {
        const int sn = std::max(need_n, am->scratch_n), sT = std::max(need_T, am->scratch_T);
        am->scratch_n = am->scratch_T = 0;
        if (batch_own_scratch(b, sn, sT, name)) return -1;
        am->scratch_n = sn; am->scratch_T = sT;
    }
    // (every call ends with the stream drained: nothing reads the old row table)
    if (dev_reserve(am->rows, (size_t)total * sizeof(AmRow)) != hipSuccess) { (void)hipGetLastError(); return fail("%s: no device memory for the row table (%zu bytes)", name, (size_t)total * sizeof(AmRow)); }
    if (logits_out && !am->pin[0])
        for (int i = 0; i < 2; i++)
            if (pinned_alloc(am->pin[i], (size_t)LNB_BATCH_MAX * V * 2, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError(); am->pin[0].reset();
                return fail("%s: no pinned host memory for the logits of a pass (%zu bytes)", name, (size_t)LNB_BATCH_MAX * V * 2);
            }
    // ---- from here on the caches are written
    for (int s = 0; s < n; s++) if (member_drain(ctxs[s])) return -1;
    struct SyncOnExit { hipStream_t s; ~SyncOnExit() { hipStreamSynchronize(s); } } sync_on_exit{st};     // (the uploads below read `rows` and `members`: no way out before the stream has drained)
    HIPCHK(hipMemcpyAsync(am->rows, rows.data(), (size_t)total * sizeof(AmRow), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(am->members, members.data(), members.size(), hipMemcpyHostToDevice, st));
    b->rows_form = !m->batch_enabled; b->force_zseq = 0; b->attn_rows = false;
    am->passes = am->max_columns = am->long_passes = 0;
    auto fetch = [&](int slot, int64_t r0, int w) -> int {  // the logits of a pass, once its copy has landed: output.ToFloat32() :175
        HIPCHK(hipEventSynchronize(am->ev[slot]));
        const uint16_t* src = am->pin[slot]; float* dst = logits_out + (size_t)r0 * V;
        for (size_t i = 0, e = (size_t)w * V; i < e; i++) dst[i] = bf_wide_h(src[i]);
        return 0;
    };
    int pass = 0, prev_w = 0; int64_t prev_r0 = 0;
    rowpack_begin(&walk, n, n_rows, W);
    while (int ns = rowpack_next(&walk, segs, &width, &row0)) {
        bool lng = false; int maxT = 0;
        for (int g = 0; g < ns; g++) { const lnb_ctx* c = ctxs[segs[g].member]; maxT = std::max(maxT, c->seq_len); lng = lng || c->seq_len > c->attn_short_cap; }
        b->n = width; b->maxT = maxT; b->lds_T = std::min(maxT, ctxs[0]->attn_short_cap); b->must_long = lng; b->attn_long = lng;
        const int layout = batch_plan_layout(batch_plan_of(b));      // what the activation buffers of this pass hold: B-operand columns, column groups or rows
        if (am->last_layout >= 0 && (layout != am->last_layout || width < am->last_width) && batch_bufs_zero(b, LNB_BATCH_MAX)) return -1;       // dead columns are zero again
        am->last_layout = layout; am->last_width = width;
        AmPass ap{}; ap.rows = am->rows + row0; ap.members = (const AmMembers*)am->members.get(); ap.member_kv = (const BatchKV*)(am->members + sizeof(AmMembers));
        ap.tab = b->tab; ap.kv = b->kv; ap.st = am->st; ap.tok = am->tok; ap.width = width; ap.n_layers = (int)L;
        HIPCHK(lnbk_append_many_setup(&ap, st));
        if (enqueue_batch_pass(b)) return -1;
        HIPCHK(lnbk_append_many_finish(b->logits, V, am->rows + row0, width, am->d_arg, st));
        if (logits_out) {
            HIPCHK(hipMemcpyAsync(am->pin[pass & 1], b->logits, (size_t)width * V * 2, hipMemcpyDeviceToHost, st));
            HIPCHK(hipEventRecord(am->ev[pass & 1], st));
            if (pass > 0 && fetch((pass - 1) & 1, prev_r0, prev_w)) return -1;        // the pass before, while this one runs
        }
        prev_w = width; prev_r0 = row0; pass++;
        am->passes = pass; am->max_columns = std::max(am->max_columns, width); am->long_passes += lng ? 1 : 0;
    }
    if (logits_out && fetch((pass - 1) & 1, prev_r0, prev_w)) return -1;
    HIPCHK(hipMemcpyAsync(am->h_arg, am->d_arg, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (argmax_out) memcpy(argmax_out, am->h_arg, (size_t)n * 4);
    return 0;
}

// lnb_batch_set_attention: long_threshold < 0 keeps the current value (default: never).  The threshold only picks between the two captured graphs;
// force_zseq is baked into the long form's launches, so a change of it drops the long graphs (and nothing else).
static int attention_args(int force_zseq) {
    if (force_zseq & ~1) return fail("force_zseq must be 0 or 1 (got %d)", force_zseq);
    return 0;
}
extern "C" int lnb_batch_set_attention(lnb_batch* b, int long_threshold, int force_zseq) {
    if (attention_args(force_zseq)) return -1;
    if (!b) return fail("null argument");
    for (int s = 0; s < b->n; s++) if (b->ctxs[s]->pending) return fail("sequence %d: a lnb_forward_stage_begin has not been ended", s);
    HIPCHK(hipSetDevice(b->m->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (long_threshold >= 0) b->attn_long_T = long_threshold;
    if (force_zseq != b->force_zseq) {
        b->graphs.drop(GF_LONG);
        b->force_zseq = force_zseq;
    }
    return 0;
}
extern "C" int lnb_batch_attention_form(const lnb_batch* b, int* out) {
    if (!b || !out) return fail("null argument");
    *out = b->last_form;
    return 0;
}
extern "C" int lnb_ctx_set_batched_attention(lnb_ctx* c, int long_threshold, int force_zseq) {
    if (attention_args(force_zseq)) return -1;
    if (!c) return fail("null argument");
    if (c->pending) return fail("a lnb_forward_stage_begin has not been ended");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (long_threshold >= 0) c->sp_attn_long_T = long_threshold;
    if (force_zseq != c->sp_force_zseq) {
        for (lnb_batch* b : c->sp_b) if (b) { b->force_zseq = force_zseq; b->graphs.drop(GF_LONG); }      // (the greedy pass and its sampling twin; a verify batch has no stage step)
        c->sp_force_zseq = force_zseq;
    }
    return 0;
}
// lnb_ctx_set_rows_attention: which appends run the multi-row long-context pair, and whether the verify passes do.  Bit 0 of flags is baked into the
// verify passes' rows graphs, so a change of it drops those (and nothing else); the threshold and bit 1 only pick a form per call.
extern "C" int lnb_ctx_set_rows_attention(lnb_ctx* c, int long_threshold, int flags) {
    if (flags & ~3) return fail("flags must be a combination of bit 0 (walk the serial sum) and bit 1 (verify passes) (got %d)", flags);
    if (!c) return fail("null argument");
    if (c->pending) return fail("a lnb_forward_stage_begin has not been ended");
    if ((flags & 2) && rows_rpw_invalid()) return fail("LNB_ATTN_ROWS_RPW=%d is not a form of the multi-row long-context attention (1, 2 or 4)", knob(Knob::ATTN_ROWS_RPW));
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (long_threshold >= 0) c->rows_T = long_threshold;
    if ((flags & 1) != (c->rows_flags & 1))
        for (lnb_batch* b : c->sp_b) if (b) b->graphs.drop(GF_ROWS);
    c->rows_flags = flags;
    return 0;
}
// the attention of the last lnb_forward_append / lnb_forward_score_append: 0 none yet or one row, 1 row-per-workgroup, 2 matrix cores, 3 one-token steps, 4 the multi-row long-context pair
extern "C" int lnb_ctx_append_attention_form(const lnb_ctx* c, int* out) {
    if (!c || !out) return fail("null argument");
    *out = c->last_append_form;
    return 0;
}
extern "C" int lnb_ctx_verify_attention_form(const lnb_ctx* c, int* out) {
    if (!c || !out) return fail("null argument");
    *out = c->sp_last_form;
    return 0;
}

// ---- speculative greedy decoding: n-gram drafts verified by one batched pass over the weights (include/lnb.h) -------------------------
// A verify pass of width w = draft_len + 1 is a batched decode step whose columns all alias THIS context: column i takes d_i (d_0 = the
// current token) at position pos + i, every column has the context's caches, column 0 the context's own StepState and token word.  The
// wq|wk|wv epilogue of a layer writes every column's K / V row before that layer's attention launch starts, so column i attends over
// positions 0 .. pos + i: the one-token step at pos + i, the same bits (a batched column is bit-identical to its single-sequence run).
// Rows a rejected column wrote beyond the accepted position are stale and are overwritten before anything reads them.
static int spec_check_draft_args(int max_draft, int ngram_min, int ngram_max, int n_corpus) {
    if (max_draft < 0 || max_draft > LNB_MAX_DRAFT) return fail("max_draft must be 0..%d (got %d)", LNB_MAX_DRAFT, max_draft);
    if (ngram_min < 1 || ngram_min > ngram_max || ngram_max > LNB_SPEC_MAX_NGRAM)
        return fail("n-gram lengths must satisfy 1 <= ngram_min <= ngram_max <= %d (got %d, %d)", LNB_SPEC_MAX_NGRAM, ngram_min, ngram_max);
    if (n_corpus < 0) return fail("negative corpus length %d", n_corpus);
    return 0;
}
extern "C" int lnb_ctx_set_draft(lnb_ctx* c, int max_draft, int ngram_min, int ngram_max, const int32_t* corpus, int n_corpus) {
    if (max_draft < 0 || max_draft > LNB_MAX_DRAFT) return fail("max_draft must be 0..%d (got %d)", LNB_MAX_DRAFT, max_draft);
    if (max_draft > 0 && spec_check_draft_args(max_draft, ngram_min, ngram_max, n_corpus)) return -1;
    if (n_corpus < 0) return fail("negative corpus length %d", n_corpus);
    if (!c || (n_corpus > 0 && !corpus)) return fail("null argument");
    HIPCHK(hipSetDevice(c->m->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->sp_corpus.reset(); c->sp_n_corpus = 0;
    c->sp_max_draft = 0;
    if (max_draft == 0) return 0;
    HIPCHK(dev_alloc(c->sp_corpus, (size_t)std::max(n_corpus, 1) * 4));
    if (n_corpus > 0) HIPCHK(hipMemcpy(c->sp_corpus, corpus, (size_t)n_corpus * 4, hipMemcpyHostToDevice));
    c->sp_n_corpus = n_corpus; c->sp_max_draft = max_draft; c->sp_ngram_min = ngram_min; c->sp_ngram_max = ngram_max;
    return 0;
}
// the per-context buffers of the drafting loop (the text head grows with the history)
static int spec_alloc(lnb_ctx* c, int text_len) {
    if (!c->sp_st) {
        HIPCHK(dev_alloc(c->sp_st, (LNB_MAX_DRAFT + 1) * sizeof(StepState)));
        HIPCHK(hipMemsetAsync(c->sp_st, 0, (LNB_MAX_DRAFT + 1) * sizeof(StepState), c->stream));
        HIPCHK(dev_alloc(c->sp_tok, (LNB_MAX_DRAFT + 1) * 4)); HIPCHK(hipMemsetAsync(c->sp_tok, 0, (LNB_MAX_DRAFT + 1) * 4, c->stream));
        HIPCHK(dev_alloc(c->sp_g, (LNB_MAX_DRAFT + 1) * 4));
        HIPCHK(dev_alloc(c->sp_best, 2 * LNB_SPEC_MAX_NGRAM * 4));
        HIPCHK(dev_alloc(c->sp_cnt, 16)); HIPCHK(hipMemsetAsync(c->sp_cnt, 0, 16, c->stream));
        HIPCHK(pinned_alloc(c->sp_word, 16, hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer((void**)&c->sp_word_dev, c->sp_word, 0));
        HIPCHK(event_create(c->sp_ev));
    }
    if (!c->sp_text.fits((size_t)text_len * 4)) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(dev_reserve(c->sp_text, (size_t)text_len * 4));
    }
    return 0;
}
// the verify batch of width w, its graph captured on first use: embedding gather of the w column tokens, the blocks, the head, the
// columns' argmax, the commit.  With the matrix-core copy the products are its column forms, without it rows of gemm_stream_kernel.
// form 1: the pass runs the long-context pair, 2: the multi-row pair (one graph per form and width); their scratch is the context's, shared by all widths
static int spec_verify_batch(lnb_ctx* c, int w, GraphForm form, bool sample, lnb_batch** out, hipGraphExec_t* graph_out) {
    lnb_model* m = c->m;
    const bool long_form = form != GF_SHORT;
    if (long_form && attn_long_scratch(LNB_MAX_DRAFT + 1, m->a.n_heads, c->seq_len, c->sp_e_buf, c->sp_z_part, "the verify passes")) return -1;   // (host side of the call, outside any capture)
    lnb_batch* b = c->sp_b[w];
    const bool fresh = !b;
    if (fresh) {
        b = new lnb_batch();
        b->m = m; b->n = w; b->ctxs.assign(w, c); b->rows_form = !m->batch_enabled;
        b->maxT = c->seq_len; b->lds_T = std::min(c->seq_len, c->attn_short_cap); b->must_long = c->seq_len > c->attn_short_cap;
        b->scratch_owned = false; b->force_zseq = c->sp_force_zseq;
        b->col_st = c->sp_st; b->col_tok = c->sp_tok;
        if (batch_alloc(b)) { lnb_batch_destroy(b); return -1; }
        c->sp_b[w] = b;
    }
    b->e_buf = c->sp_e_buf; b->z_part = c->sp_z_part;
    b->attn_long = long_form; b->attn_rows = form == GF_ROWS; b->rows_zseq = c->rows_flags & 1;
    GraphExec& gslot = b->graphs.slot(sample ? GL_SAMPLE : GL_GREEDY, form);
    auto body = [&]() -> int {
        if (enqueue_batch_pass(b)) return -1;
        if (sample) {                                        // the token launch is the one difference: every column's sampled token at its own position, then the same acceptance
            HIPCHK(lnbk_spec_sample_commit(b->logits, m->a.vocab_size, w, m->prob_etab, c->d_smp, c->sp_g, b->tab, c->sp_cnt + 1, b->stream));
            return 0;
        }
        HIPCHK(lnbk_spec_argmax(b->logits, m->a.vocab_size, w, c->sp_g, b->stream));
        HIPCHK(lnbk_spec_commit(c->sp_g, w, b->tab, b->stream));
        return 0;
    };
    if (capture_once(gslot, b->stream, body)) {
        if (fresh) { c->sp_b[w] = nullptr; lnb_batch_destroy(b); }      // (a batch without a graph is not kept)
        return -1;
    }
    *out = b; *graph_out = gslot;
    return 0;
}
static DraftParams spec_draft_params(lnb_ctx* c, int n_text, int max_steps) {
    DraftParams p{}; p.text = c->sp_text; p.n_text = n_text; p.gen = c->dout; p.st = c->st;
    p.corpus = c->sp_corpus; p.n_corpus = c->sp_n_corpus; p.ngram_min = c->sp_ngram_min; p.ngram_max = c->sp_ngram_max; p.max_draft = c->sp_max_draft;
    p.max_steps = max_steps; p.seq_len = c->seq_len; p.out = c->sp_tok; p.col_st = c->sp_st; p.word = c->sp_word_dev; p.best = c->sp_best; p.cnt = c->sp_cnt;
    return p;
}
// lnb_decode_speculative_until (smp null) and lnb_decode_speculative_sample_until: one loop; the sampler picks the token launch of a pass -- the sampling
// one-token graph or the verify batch's sampling graph -- and nothing else
static int spec_decode_impl(lnb_ctx* c, const lnb_sampler* smp, const int32_t* history, int n_history, int32_t token, int start_pos, int max_steps,
                            int32_t* out_tokens, int* n_generated, int* finished, lnb_spec_stats* stats, float* ms_out) {
    if (n_history < 0) return fail("negative history length %d", n_history);
    if (max_steps <= 0) return fail("max_steps must be positive");
    if (!c || !out_tokens || !n_generated || (n_history > 0 && !history)) return fail("null argument");
    lnb_model* m = c->m;
    if (!m->first() || !m->last()) return fail("speculative decoding needs a whole-model handle");
    if (c->mode != LNB_MODE_EXACT) return fail("speculative decoding is exact-mode only: its verify pass is the batched exact step (the tolerance mode has none)");
    if (c->top_k > 0) return fail("speculative decoding does not record token probabilities: lnb_ctx_set_token_probs(ctx, 0) first");
    if (c->batch_users > 0) return fail("context is a member of %d live batch(es): speculative decoding runs it alone (lnb_batch_destroy first)", c->batch_users);
    if (c->pending) return fail("a lnb_forward_stage_begin has not been ended");
    if (smp && sample_vocab_check(m->a.vocab_size)) return -1;
    if (stats) *stats = lnb_spec_stats{};
    if (c->sp_max_draft == 0) {                              // drafting off: the greedy (the sampling) loop itself, one pass per token
        if (decode_greedy_impl(c, token, start_pos, max_steps, out_tokens, n_generated, finished, ms_out, smp)) return -1;
        if (stats) stats->passes = *n_generated;
        return 0;
    }
    HIPCHK(hipSetDevice(m->device));
    if (max_steps > c->dout_cap) return fail("max_steps %d exceeds the context length %d", max_steps, c->dout_cap);
    if (check_call(c, 1, start_pos) || check_call(c, 1, start_pos + max_steps - 1)) return -1;
    if (token < 0 || token >= m->a.vocab_size) return fail("token id at index 0 is outside the vocabulary");
    if (batch_shape_check(m, "the verify pass")) return -1;
    if (!m->batch_enabled) HIPCHK(lnbk_batch_prepare());
    const int n_text = n_history + 1;
    if (smp && !c->d_smp) HIPCHK(dev_alloc(c->d_smp, sizeof(LnbSampler)));
    if (spec_alloc(c, n_text) || capture_decode_graphs(c, start_pos, max_steps, smp != nullptr)) return -1;
    hipStream_t st = c->stream;
    c->tp_last_k = 0; c->tp_last_n = 0;
    if (smp) HIPCHK(hipMemcpyAsync(c->d_smp, smp, sizeof(LnbSampler), hipMemcpyHostToDevice, st));       // (the captured graphs hold the pointer: another sampler replays them)
    if (n_history > 0) HIPCHK(hipMemcpyAsync(c->sp_text, history, (size_t)n_history * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->sp_text + n_history, &token, 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->dtok, &token, 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(c->derr, 0, 4, st));
    for (lnb_batch* b : c->sp_b) if (b) HIPCHK(hipMemsetAsync(b->derr, 0, 4, st));
    HIPCHK(ctx_set_state(c, start_pos, 0, false, true));
    c->call_T = 0;
    const DraftParams dp = spec_draft_params(c, n_text, max_steps);
    HIPCHK(hipEventRecord(c->ev0, st));
    HIPCHK(lnbk_ngram_draft(&dp, st));
    HIPCHK(hipEventRecord(c->sp_ev, st));
    lnb_spec_stats s{};
    int n_out = 0, fin = 0;
    for (;;) {
        // the one host round trip of a pass: the draft kernel's word {draft_len, n_out, finished}
        HIPCHK(hipEventSynchronize(c->sp_ev));
        const volatile int32_t* wd = c->sp_word;
        const int k = wd[0]; n_out = wd[1]; fin = wd[2];
        if (fin || n_out >= max_steps) break;
        if (k < 0 || k > c->sp_max_draft) return fail("internal error: draft length %d", k);
        s.passes++;
        if (k == 0) {
            const bool lg = want_long_attention(c, 1, start_pos + n_out);
            HIPCHK(hipGraphLaunch(c->graphs.slot(smp ? GL_SAMPLE : GL_GREEDY, lg ? GF_LONG : GF_SHORT), st));
        } else {
            lnb_batch* b = nullptr; hipGraphExec_t pass = nullptr;
            // the pass's last column sits at start_pos + n_out + k: the long form when the context is beyond the one-workgroup kernels' reach or past the threshold
            const bool lf = c->seq_len > c->attn_short_cap || start_pos + n_out + k + 1 > c->sp_attn_long_T;
            const GraphForm form = !lf ? GF_SHORT : (c->rows_flags & 2) ? GF_ROWS : GF_LONG;     // (rows: lnb_ctx_set_rows_attention's opt-in -- K and V read once for all columns)
            if (spec_verify_batch(c, k + 1, form, smp != nullptr, &b, &pass)) return -1;
            HIPCHK(hipGraphLaunch(pass, st));
            c->sp_last_form = form; b->last_form = lf ? 1 : 0;
            s.verify_passes++; s.drafted += k;
        }
        HIPCHK(lnbk_ngram_draft(&dp, st));
        HIPCHK(hipEventRecord(c->sp_ev, st));
    }
    HIPCHK(hipEventRecord(c->ev1, st));
    HIPCHK(hipMemcpyAsync(out_tokens, c->dout, (size_t)n_out * 4, hipMemcpyDeviceToHost, st));
    int err = 0;
    HIPCHK(hipMemcpyAsync(c->h_io + 1, c->derr, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    err |= c->h_io[1];
    for (lnb_batch* b : c->sp_b) if (b) {
        HIPCHK(hipMemcpyAsync(c->h_io + 1, b->derr, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        err |= c->h_io[1];
    }
    if (ms_out) HIPCHK(hipEventElapsedTime(ms_out, c->ev0, c->ev1));
    c->dev_pos = -1;
    if (err) return fail("generated token id is outside the vocabulary");
    *n_generated = n_out;
    if (finished) *finished = fin;
    s.accepted = (int64_t)n_out - s.passes;                  // every pass emits its column 0 token plus the drafts it accepted
    if (stats) *stats = s;
    return 0;
}
extern "C" int lnb_decode_speculative_until(lnb_ctx* c, const int32_t* history, int n_history, int32_t token, int start_pos, int max_steps,
                                            int32_t* out_tokens, int* n_generated, int* finished, lnb_spec_stats* stats, float* ms_out) {
    return spec_decode_impl(c, nullptr, history, n_history, token, start_pos, max_steps, out_tokens, n_generated, finished, stats, ms_out);
}
// the same loop with the sampler's token per column (include/lnb.h): the tokens of lnb_decode_sample_until, because its draw is u(seed, pos) alone
extern "C" int lnb_decode_speculative_sample_until(lnb_ctx* c, const lnb_sampler* sampler, const int32_t* history, int n_history, int32_t token, int start_pos,
                                                   int max_steps, int32_t* out_tokens, int* n_generated, int* finished, lnb_spec_stats* stats, float* ms_out) {
    if (!sampler) return fail("null argument (sampler)");
    if (sampler_check(sampler, "")) return -1;
    return spec_decode_impl(c, sampler, history, n_history, token, start_pos, max_steps, out_tokens, n_generated, finished, stats, ms_out);
}
// ngram_draft_kernel on host arrays (a test aid, as lnb_op_argmax): the draft that follows text, with no decode limits
extern "C" int lnb_op_ngram_draft(int device, const int32_t* text, int n_text, const int32_t* corpus, int n_corpus,
                                  int ngram_min, int ngram_max, int max_draft, int32_t* out, int* n_out) {
    if (n_text < 0) return fail("negative text length %d", n_text);
    if (spec_check_draft_args(max_draft, ngram_min, ngram_max, n_corpus)) return -1;
    if ((n_text > 0 && !text) || (n_corpus > 0 && !corpus) || !out || !n_out) return fail("null argument");
    if (op_device(device)) return -1;
    DevArena a;
    int32_t* dt = a.alloc<int32_t>((size_t)std::max(n_text, 1)); int32_t* dc = a.alloc<int32_t>((size_t)std::max(n_corpus, 1));
    int32_t* dout = a.alloc<int32_t>(LNB_MAX_DRAFT + 1); int32_t* dword = a.alloc<int32_t>(4);
    int* best = a.alloc<int>(2 * LNB_SPEC_MAX_NGRAM); unsigned* cnt = a.alloc<unsigned>(4);
    HIPCHK(a.error());
    HIPCHK(hipMemset(cnt, 0, 16));
    if (n_text > 0) HIPCHK(hipMemcpy(dt, text, (size_t)n_text * 4, hipMemcpyHostToDevice));
    if (n_corpus > 0) HIPCHK(hipMemcpy(dc, corpus, (size_t)n_corpus * 4, hipMemcpyHostToDevice));
    int32_t h[LNB_MAX_DRAFT + 1] = {}, word[4] = {};
    DraftParams p{}; p.text = dt; p.n_text = n_text; p.corpus = dc; p.n_corpus = n_corpus;
    p.ngram_min = ngram_min; p.ngram_max = ngram_max; p.max_draft = max_draft; p.out = dout; p.word = dword; p.best = best; p.cnt = cnt;
    HIPCHK(lnbk_ngram_draft(&p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(word, dword, 12, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h, dout, sizeof h, hipMemcpyDeviceToHost));
    if (word[0] < 0 || word[0] > max_draft) return fail("internal error: draft length %d", word[0]);
    for (int i = 0; i < word[0]; i++) out[i] = h[1 + i];
    *n_out = word[0];
    return 0;
}

// ---- lnb_decode_speculative_many (include/lnb.h): speculative greedy decoding of n contexts together.  Every pass is a pass of lnb_forward_append_many on
// the model handle's AppendMany object -- same buffers, stream, mutex and "dead columns are zero" duty -- whose row table the device writes itself:
//   spec_many_draft_kernel (every member's n-gram draft) -> spec_many_pack_kernel (the grant rule of lnb_specpack.h, the AmRow table, the pinned block)
//   -> [host: reads {width, any_draft, running, largest seq_len}, its one round trip per pass] -> append_many_setup_kernel -> the batched step
//   -> spec_many_commit_kernel (argmax per column, acceptance and emission per member into the member's OWN state, token word and log).
// The launches are eager, as lnb_forward_append_many's are (profiles/spec_many.md).
static int spec_many_build(SpecMany* sm, hipStream_t st) {
    const size_t N = LNB_BATCH_MAX;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_mem = carve(N * sizeof(SmMember)), o_want = carve(N * 4), o_run = carve(N * 4), o_draft = carve(N * LNB_SPEC_MAX_DRAFT * 4),
                 o_best = carve(N * 2 * LNB_SPEC_MAX_NGRAM * 4), o_cnt = carve((N + 1) * 4), o_rows = carve(N * sizeof(AmRow)), o_seg = carve(N * sizeof(SmSeg)),
                 o_stats = carve(N * sizeof(SmStats)), o_g = carve(N * 4), o_smp = carve(N * sizeof(LnbSampler));
    HIPCHK(dev_alloc(sm->dev, off));
    HIPCHK(hipMemsetAsync(sm->dev, 0, off, st));
    HIPCHK(pinned_alloc(sm->word, 16, hipHostMallocMapped));
    int32_t* word_dev = nullptr;
    HIPCHK(hipHostGetDevicePointer((void**)&word_dev, sm->word, 0));
    HIPCHK(event_create(sm->ev));
    HIPCHK(event_create(sm->ev0)); HIPCHK(event_create(sm->ev1));
    HIPCHK(hipStreamSynchronize(st));
    SmPass& p = sm->p; char* d = sm->dev;
    p.members = (const SmMember*)(d + o_mem); p.want = (int32_t*)(d + o_want); p.running = (int32_t*)(d + o_run); p.draft = (int32_t*)(d + o_draft);
    p.best = (int*)(d + o_best); p.cnt = (unsigned*)(d + o_cnt); p.rows = (AmRow*)(d + o_rows); p.seg = (SmSeg*)(d + o_seg);
    p.stats = (SmStats*)(d + o_stats); p.g = (int32_t*)(d + o_g); p.word = word_dev; p.smp = (const LnbSampler*)(d + o_smp);
    return 0;
}
// the object is published only when all of it exists: a failed allocation leaves the handle as it was, and the next call starts over
static int spec_many_alloc(AppendMany* am) {
    if (am->sm) return 0;
    SpecMany* sm = new SpecMany();
    if (spec_many_build(sm, am->b->stream)) { (void)hipGetLastError(); delete sm; return -1; }
    am->sm = sm;
    return 0;
}
// lnb_decode_speculative_many (sampling false) and lnb_decode_speculative_sample_many: one loop; the commit launch of a pass is the one difference
static int spec_many_impl(bool sampling, lnb_ctx* const* ctxs, int n, const lnb_sampler* samplers, const int32_t* const* history, const int32_t* n_history,
                          const int32_t* tokens, const int32_t* start_pos, int max_steps, int col_budget,
                          int32_t* out_tokens, int32_t* n_generated, int32_t* finished,
                          lnb_spec_stats* stats, lnb_spec_many_info* info, float* ms_out) {
    const char* const name = sampling ? "lnb_decode_speculative_sample_many" : "lnb_decode_speculative_many";
    if (sampling && !samplers) return fail("%s: null argument (samplers)", name);
    // ---- the arguments alone: no handle is dereferenced
    if (!ctxs || !history || !n_history || !tokens || !start_pos || !out_tokens || !n_generated)
        return fail("%s: null argument (%s)", name, !ctxs ? "ctxs" : !history ? "history" : !n_history ? "n_history" : !tokens ? "tokens" : !start_pos ? "start_pos" :
                    !out_tokens ? "out_tokens" : "n_generated");
    if (n < 1 || n > LNB_BATCH_MAX) return fail("%s: a call takes 1..%d contexts (got %d)", name, LNB_BATCH_MAX, n);
    if (sampling) {
        char who[96];
        for (int s = 0; s < n; s++) { snprintf(who, sizeof who, "%s: member %d: ", name, s); if (sampler_check(samplers + s, who)) return -1; }
    }
    if (max_steps <= 0) return fail("%s: max_steps must be positive (got %d)", name, max_steps);
    if (col_budget != 0 && (col_budget < n || col_budget > LNB_BATCH_MAX))
        return fail("%s: col_budget must be 0 (the default) or %d..%d, one column per member at least (got %d)", name, n, LNB_BATCH_MAX, col_budget);
    for (int s = 0; s < n; s++) {
        if (!ctxs[s]) return fail("%s: null context at index %d", name, s);
        if (n_history[s] < 0) return fail("%s: member %d: negative history length %d", name, s, n_history[s]);
        if (n_history[s] > 0 && !history[s]) return fail("%s: member %d: null history of %d tokens", name, s, n_history[s]);
        for (int r = 0; r < s; r++) if (ctxs[r] == ctxs[s]) return fail("%s: context %d appears twice (also at index %d)", name, s, r);
    }
    // ---- the handles: everything is checked before any cache is written
    lnb_model* m = ctxs[0]->m;
    for (int s = 0; s < n; s++) if (ctxs[s]->m != m) return fail("%s: context %d belongs to another lnb_model handle", name, s);
    if (!m->first() || !m->last()) return fail("%s needs a whole-model handle: pipeline stages have no speculative decoding", name);
    if (batch_shape_check(m, name)) return -1;
    if (sampling && sample_vocab_check(m->a.vocab_size)) return -1;
    const int V = m->a.vocab_size, cap = ctxs[0]->attn_short_cap;
    const int budget = col_budget ? col_budget : LNB_STREAM_COLS * ((n + LNB_STREAM_COLS - 1) / LNB_STREAM_COLS);
    int n_levels = 1, need_T = 0; bool any_long = false; size_t text_total = 0;
    for (int s = 0; s < n; s++) {
        const lnb_ctx* c = ctxs[s];
        if (c->mode != LNB_MODE_EXACT) return fail("%s: context %d is in the tolerance mode: the call is exact-mode only", name, s);
        if (c->top_k > 0) return fail("%s: context %d records token probabilities, which the call does not: lnb_ctx_set_token_probs(ctx, 0) first", name, s);
        if (c->pending) return fail("%s: context %d: a lnb_forward_stage_begin has not been ended", name, s);
        if (c->batch_users > 0) return fail("%s: context %d is a member of %d live batch(es): lnb_batch_destroy first", name, s, c->batch_users);
        if (max_steps > c->dout_cap) return fail("%s: member %d: max_steps %d exceeds its token log of %d", name, s, max_steps, c->dout_cap);
        if (start_pos[s] < 0) continue;                      // skipped: a member that finished in an earlier call of a chunked run
        if (tokens[s] < 0 || tokens[s] >= V) return fail("%s: member %d: token id %d is outside the vocabulary", name, s, tokens[s]);
        const int64_t T = (int64_t)start_pos[s] + max_steps;
        if (T > m->cis_rows) return fail("%s: member %d: position %lld is beyond the %d-row RoPE table", name, s, (long long)T, m->cis_rows);
        if (T > c->seq_len) return fail("%s: member %d: position %lld is beyond the KV cache of %d", name, s, (long long)T, c->seq_len);
        if (lnbk_attn_long_layout_lds(c->seq_len) > 160 * 1024) return fail("%s: member %d: seq_len %d is beyond what the long-context attention keeps in the LDS", name, s, c->seq_len);
        if (c->sp_max_draft > 0) n_levels = std::max(n_levels, c->sp_ngram_max - c->sp_ngram_min + 1);
        need_T = std::max(need_T, c->seq_len); any_long = any_long || c->seq_len > c->attn_short_cap;
        text_total += (size_t)n_history[s] + 1;
    }
    std::lock_guard<std::mutex> lock(m->am_mu);
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(lnbk_batch_prepare());
    if (append_many_alloc(m)) return -1;
    AppendMany* am = m->am; lnb_batch* b = am->b; hipStream_t st = b->stream;
    if (spec_many_alloc(am)) return -1;
    SpecMany* sm = am->sm;
    if (any_long && (budget > am->scratch_n || need_T > am->scratch_T)) {
        const int sn = std::max(budget, am->scratch_n), sT = std::max(need_T, am->scratch_T);
        am->scratch_n = am->scratch_T = 0;
        if (batch_own_scratch(b, sn, sT, name)) return -1;
        am->scratch_n = sn; am->scratch_T = sT;
    }
    if (dev_reserve(sm->text, text_total * 4) != hipSuccess) { (void)hipGetLastError(); return fail("%s: no device memory for the members' histories (%zu bytes)", name, text_total * 4); }
    // ---- the call's tables on the host: the members' cache lengths and pointers (as lnb_forward_append_many's), their SmMember, their text heads
    const size_t L = m->layers.size();
    std::vector<char> members(sizeof(AmMembers) + L * sizeof(BatchKV));
    std::vector<SmMember> smm(LNB_BATCH_MAX, SmMember{});
    std::vector<int32_t> text(std::max<size_t>(text_total, 1));
    { AmMembers* hm = (AmMembers*)members.data(); BatchKV* hk = (BatchKV*)(members.data() + sizeof(AmMembers));
      hm->n = n;
      size_t t0 = 0;
      for (int s = 0; s < LNB_BATCH_MAX; s++) {
          const lnb_ctx* c = ctxs[s < n ? s : 0];
          hm->seq_len[s] = c->seq_len;
          for (size_t l = 0; l < L; l++) { hk[l].ck[s] = c->ck[l]; hk[l].cv[s] = c->cv[l]; }
          if (s >= n || start_pos[s] < 0) continue;
          SmMember& e = smm[s];
          e.st = c->st; e.tok = c->dtok; e.log = c->dout; e.log_cap = c->dout_cap; e.seq_len = c->seq_len; e.active = 1;
          e.text = sm->text + t0; e.n_text = n_history[s] + 1;
          if (n_history[s] > 0) memcpy(text.data() + t0, history[s], (size_t)n_history[s] * 4);
          text[t0 + n_history[s]] = tokens[s];
          t0 += (size_t)e.n_text;
          e.max_draft = c->sp_max_draft; e.ngram_min = c->sp_ngram_min; e.ngram_max = c->sp_ngram_max; e.corpus = c->sp_corpus; e.n_corpus = c->sp_n_corpus;
          if (e.max_draft == 0) { e.ngram_min = e.ngram_max = 1; e.corpus = nullptr; e.n_corpus = 0; }
      } }
    // ---- from here on the members' states and caches are written
    for (int s = 0; s < n; s++) if (start_pos[s] >= 0) { if (member_drain(ctxs[s])) return -1; ctxs[s]->tp_last_k = 0; ctxs[s]->tp_last_n = 0; }
    struct SyncOnExit { hipStream_t s; ~SyncOnExit() { hipStreamSynchronize(s); } } sync_on_exit{st};     // (the uploads below read host vectors: no way out before the stream has drained)
    HIPCHK(hipMemcpyAsync(am->members, members.data(), members.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync((void*)sm->p.members, smm.data(), smm.size() * sizeof(SmMember), hipMemcpyHostToDevice, st));
    if (text_total) HIPCHK(hipMemcpyAsync(sm->text, text.data(), text_total * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(sm->p.stats, 0, LNB_BATCH_MAX * sizeof(SmStats), st));
    if (sampling) HIPCHK(hipMemcpyAsync((void*)sm->p.smp, samplers, (size_t)n * sizeof(LnbSampler), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b->derr, 0, 4, st));
    for (int s = 0; s < n; s++) if (start_pos[s] >= 0) {
        HIPCHK(hipMemcpyAsync(ctxs[s]->dtok, tokens + s, 4, hipMemcpyHostToDevice, st));
        HIPCHK(lnbk_set_state(ctxs[s]->st, start_pos[s], 0, 1, st));
    }
    b->rows_form = !m->batch_enabled; b->force_zseq = 0; b->attn_rows = false;
    SmPass sp = sm->p; sp.n = n; sp.max_steps = max_steps; sp.budget = budget; sp.n_levels = n_levels; sp.logits = b->logits; sp.V = V;
    if (sampling) sp.etab = m->prob_etab; else sp.smp = nullptr;
    lnb_spec_many_info inf{};
    HIPCHK(hipEventRecord(sm->ev0, st));
    HIPCHK(lnbk_spec_many_draft(&sp, st));
    HIPCHK(lnbk_spec_many_pack(&sp, st));
    HIPCHK(hipEventRecord(sm->ev, st));
    for (;;) {
        // the one host round trip of a pass: the pack kernel's block {width, any_draft, running members, largest seq_len of a running member}
        HIPCHK(hipEventSynchronize(sm->ev));
        const volatile int32_t* wd = sm->word;
        const int width = wd[0], any = wd[1], running = wd[2], maxT = wd[3];
        if (width < 0 || running < 0 || running > n || width < running || width > budget || (running > 0 && inf.passes >= max_steps)) return fail("%s: internal error: a pass of %d columns for %d running members", name, width, running);
        if (running == 0) break;
        const bool lng = maxT > cap;
        b->n = width; b->maxT = maxT; b->lds_T = std::min(maxT, cap); b->must_long = lng; b->attn_long = lng;
        const int layout = batch_plan_layout(batch_plan_of(b));
        if (am->last_layout >= 0 && (layout != am->last_layout || width < am->last_width) && batch_bufs_zero(b, LNB_BATCH_MAX)) return -1;       // dead columns are zero again
        am->last_layout = layout; am->last_width = width;
        AmPass ap{}; ap.rows = sp.rows; ap.members = (const AmMembers*)am->members.get(); ap.member_kv = (const BatchKV*)(am->members + sizeof(AmMembers));
        ap.tab = b->tab; ap.kv = b->kv; ap.st = am->st; ap.tok = am->tok; ap.width = width; ap.n_layers = (int)L;
        HIPCHK(lnbk_append_many_setup(&ap, st));
        if (enqueue_batch_pass(b)) return -1;
        sp.width = width;
        HIPCHK(sampling ? lnbk_spec_many_sample_commit(&sp, st) : lnbk_spec_many_commit(&sp, st));
        HIPCHK(lnbk_spec_many_draft(&sp, st));
        HIPCHK(lnbk_spec_many_pack(&sp, st));
        HIPCHK(hipEventRecord(sm->ev, st));
        inf.passes++; inf.verify_passes += any ? 1 : 0; inf.columns += width; inf.max_columns = std::max<int64_t>(inf.max_columns, width); inf.long_passes += lng ? 1 : 0;
    }
    HIPCHK(hipEventRecord(sm->ev1, st));
    std::vector<StepState> hs(n); std::vector<SmStats> hst(n);
    for (int s = 0; s < n; s++) if (start_pos[s] >= 0) {
        HIPCHK(hipMemcpyAsync(out_tokens + (size_t)s * max_steps, ctxs[s]->dout, (size_t)max_steps * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&hs[s], ctxs[s]->st, sizeof(StepState), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(hst.data(), sm->p.stats, (size_t)n * sizeof(SmStats), hipMemcpyDeviceToHost, st));
    int32_t err = 0;
    HIPCHK(hipMemcpyAsync(&err, b->derr, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms_out) HIPCHK(hipEventElapsedTime(ms_out, sm->ev0, sm->ev1));
    if (err) return fail("%s: a generated token id is outside the vocabulary", name);
    for (int s = 0; s < n; s++) {
        const bool skipped = start_pos[s] < 0;
        n_generated[s] = skipped ? 0 : hs[s].n_out;
        if (finished) finished[s] = skipped ? 1 : hs[s].finished;
        if (stats) stats[s] = skipped ? lnb_spec_stats{} : lnb_spec_stats{hst[s].passes, hst[s].verify_passes, hst[s].drafted, (int64_t)hs[s].n_out - hst[s].passes};
    }
    if (info) *info = inf;
    return 0;
}
extern "C" int lnb_decode_speculative_many(lnb_ctx* const* ctxs, int n, const int32_t* const* history, const int32_t* n_history,
                                           const int32_t* tokens, const int32_t* start_pos, int max_steps, int col_budget,
                                           int32_t* out_tokens, int32_t* n_generated, int32_t* finished,
                                           lnb_spec_stats* stats, lnb_spec_many_info* info, float* ms_out) {
    return spec_many_impl(false, ctxs, n, nullptr, history, n_history, tokens, start_pos, max_steps, col_budget, out_tokens, n_generated, finished, stats, info, ms_out);
}
// the same call with one sampler per member (include/lnb.h): every member's tokens are those of its own lnb_decode_sample_until
extern "C" int lnb_decode_speculative_sample_many(lnb_ctx* const* ctxs, int n, const lnb_sampler* samplers, const int32_t* const* history, const int32_t* n_history,
                                                  const int32_t* tokens, const int32_t* start_pos, int max_steps, int col_budget,
                                                  int32_t* out_tokens, int32_t* n_generated, int32_t* finished,
                                                  lnb_spec_stats* stats, lnb_spec_many_info* info, float* ms_out) {
    return spec_many_impl(true, ctxs, n, samplers, history, n_history, tokens, start_pos, max_steps, col_budget, out_tokens, n_generated, finished, stats, info, ms_out);
}

// ---- layer-sharded pipeline: the exchange behind the C ABI ---------------------------------------------------------------------
// The reference runs its 32 blocks in one loop (llamatransformer.go:156-164); a pipeline cuts that loop over the GPUs of a node.  Rank r
// holds a stage (lnb_model_create_parts) and one lnb_ctx per sequence in flight; a TICK enqueues, without ever blocking the host:
//   * the stage step of one sequence on that context's stream (one-token steps replay a captured hipGraph; the position lives on the
//     device), gated by the event of the receive that delivered its input;
//   * ONE RCCL group on the pipe's exchange stream: ncclSend of the previous result to rank r+1 straight from the context's hidden
//     state buffer (the last rank sends the 4-byte argmax token to rank 0 straight from device memory) and ncclRecv of the next input
//     from rank r-1 straight into the target context's buffer (rank 0: the token, into the device word the embedding gather reads).
// No staging copies, no host round trip for the token ring, no stream synchronisation per tick: the host only enqueues, and reads the
// generated tokens from a pinned log after lnb_pipeline_sync.  RCCL is loaded on first use (lnb_pipeline.cpp).
// In-process transport (lnb_pipeline_init_loopback): every stage of a pipeline lives in ONE process (all on one GPU, or one per GPU) and a
// "send" meets its "receive" in a mailbox; whichever side is posted second enqueues the device copy.  Same tick code, same events, same
// graphs as the RCCL transport -- what it replaces is only ncclSend / ncclRecv.  Used to test host schedules where RCCL cannot run
// (two ranks need two GPUs) and by single-process multi-GPU hosts.
// What crosses a boundary (the hidden state, the gate*up activations behind a gate/up part, the token word between the last and the first
// stage) and when a send fits a receive is decided in lnb_handoff.h; pipe_exchange below enqueues what it says, for either transport.
struct LoopGroup { HandoffBox box; int users = 0; int device = -1; };   // (a posted hand-off's owner is its unit's PipeLink)
static std::map<std::string, LoopGroup> g_loops;
static std::mutex g_loops_mu;

struct lnb_pipe {
    lnb_model* m = nullptr; int rank = 0, world = 1;
    LoopGroup* loop = nullptr; std::string loop_tag;
    void* comm = nullptr; const lnb_rccl_api* api = nullptr;
    Stream xs;                             // exchange stream
    Pinned<int32_t> h_tok; int tok_cap = 0, tok_n = 0;   // pinned RING of the tokens the last stage produced, in tick order: slot s lives at s % tok_cap
    bool use_graph = true;
    bool host = false;                     // no transport: the host layer moves the boundary buffers (lnb_pipeline_init_host)
};
static bool pipe_use_graph() { return knob(Knob::PIPELINE_GRAPH) != 0; }
static int pipe_log_cap() { const int v = knob(Knob::PIPELINE_LOG_CAP); return v < 4 ? 4 : v; }   // (the env knob is for the wrap-around test)
#define NCCLCHK(p_, expr) do { int r_ = (expr); if (r_ != 0) return fail("%s failed: %s (%s:%d)", #expr, (p_)->api->GetErrorString(r_), __FILE__, __LINE__); } while (0)

extern "C" int lnb_pipeline_unique_id(void* id128) {
    if (!id128) return fail("null argument");
    const lnb_rccl_api* api = lnb_rccl_load();
    if (!api) return -1;
    lnb_nccl_id id; memset(&id, 0, sizeof id);
    int r = api->GetUniqueId(&id);
    if (r != 0) return fail("ncclGetUniqueId failed: %s", api->GetErrorString(r));
    memcpy(id128, &id, sizeof id);
    return 0;
}
// What the three kinds of pipe share: the argument checks, the exchange stream and the pinned token log.  *out holds the pipe on success.
static int pipe_new(lnb_model* m, int rank, int world, lnb_pipe** out) {
    if (!m || !out) return fail("null argument");
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world) return fail("rank %d out of range for %d pipeline stages", rank, world);
    if (!m->finalized) return fail("model not finalized");
    if ((rank == 0) != m->first()) return fail("pipeline rank %d: only the first stage owns tok_embeddings (this stage starts at block part %d)", rank, m->part_begin);
    if ((rank == world - 1) != m->last()) return fail("pipeline rank %d of %d: only the last stage owns norm + output (this stage ends at block part %d)", rank, world, m->part_end);
    HIPCHK(hipSetDevice(m->device));
    lnb_pipe* p = new lnb_pipe();
    p->m = m; p->rank = rank; p->world = world; p->use_graph = pipe_use_graph();
    hipError_t e = stream_create(p->xs, hipStreamNonBlocking);
    if (e == hipSuccess) { p->tok_cap = pipe_log_cap(); e = pinned_alloc(p->h_tok, (size_t)p->tok_cap * 4, hipHostMallocDefault); }
    if (e != hipSuccess) { fail("pipeline init: %s", hipGetErrorString(e)); delete p; return -1; }
    *out = p;
    return 0;
}
// an entry point whose own part failed (the error is set; no communicator, no group joined): what pipe_new made goes, nothing enqueued yet
static int pipe_abandon(lnb_pipe** out) { delete *out; *out = nullptr; return -1; }
extern "C" int lnb_pipeline_init(lnb_model* m, int rank, int world, const void* id128, lnb_pipe** out) {
    if (pipe_new(m, rank, world, out)) return -1;
    lnb_pipe* p = *out;
    if (world > 1) {
        if (!id128) { fail("null unique id"); return pipe_abandon(out); }
        p->api = lnb_rccl_load();
        if (!p->api) return pipe_abandon(out);
        lnb_nccl_id id; memcpy(&id, id128, sizeof id);
        int r = p->api->CommInitRank(&p->comm, world, id, rank);
        if (r != 0) { fail("ncclCommInitRank failed: %s", p->api->GetErrorString(r)); p->comm = nullptr; return pipe_abandon(out); }
    }
    return 0;
}
extern "C" int lnb_pipeline_init_loopback(lnb_model* m, int rank, int world, const char* group, lnb_pipe** out) {
    if (!group) return fail("null argument");
    if (pipe_new(m, rank, world, out)) return -1;
    lnb_pipe* p = *out;
    if (world > 1) {
        // The mailbox transport records a unit's events on whichever pipe's exchange stream posts second, and a unit's flags are
        // plain fields: every stage of a group must live on ONE device and be ticked from ONE host thread in lock-step order (what the
        // tests and single-process hosts do).  One stage per GPU is the RCCL transport's job (lnb_pipeline_init).
        std::lock_guard<std::mutex> lock(g_loops_mu);
        LoopGroup& g = g_loops[group];
        if (g.users > 0 && g.device != m->device) {
            fail("in-process pipeline group \"%s\" lives on device %d: a stage on device %d cannot join it (use lnb_pipeline_init for one stage per GPU)", group, g.device, m->device);
            return pipe_abandon(out);                        // (it has not joined the group)
        }
        g.device = m->device;
        p->loop_tag = group; p->loop = &g; p->loop->users++;
    }
    return 0;
}
// The pipe WITHOUT a transport: stage steps, graphs, positions and the token log as in the other two, but what crosses the stage boundary is
// moved by the host layer (pipeline.py's torch.distributed fallback: staging tensors + batch_isend_irecv) between lnb_pipeline_sync calls.
extern "C" int lnb_pipeline_init_host(lnb_model* m, int rank, int world, lnb_pipe** out) {
    if (pipe_new(m, rank, world, out)) return -1;
    (*out)->host = true;
    return 0;
}
extern "C" int lnb_pipeline_destroy(lnb_pipe* p) {
    if (!p) return 0;
    hipSetDevice(p->m->device);
    hipDeviceSynchronize();
    if (p->loop) { std::lock_guard<std::mutex> lock(g_loops_mu); if (--p->loop->users == 0) g_loops.erase(p->loop_tag); }
    if (p->comm) p->api->CommDestroy(p->comm);
    delete p;
    return 0;
}
// one stage step on the context's stream; tokens != NULL: host tokens (prefill on rank 0); NULL on rank 0: the token already sits in
// c->dtok (received from the last rank).  The last stage leaves the argmax token in c->dnext.
static int enqueue_stage_step(lnb_pipe* p, lnb_ctx* c, const int32_t* tokens, int rows, int pos) {
    lnb_model* m = c->m; const int V = m->a.vocab_size; hipStream_t st = c->stream;
    const bool longctx = want_long_attention(c, rows, pos);
    auto body = [&](bool host_tokens) -> int {
        if (m->first()) {
            if (host_tokens) {                               // a second multi-row tick (chunked prefill) must not overwrite words a queued copy still reads
                if (staging_acquire(c)) return -1;
                memcpy(c->h_io + 2, tokens, (size_t)rows * 4);
                HIPCHK(hipMemcpyAsync(c->dtok, c->h_io + 2, (size_t)rows * 4, hipMemcpyHostToDevice, st));
                if (staging_release(c)) return -1;
            }
            HIPCHK(lnbk_embed(m->tok_embd, c->dtok, c->x, rows, m->a.dim, V, c->derr, st));   // Fwd_Get_Rows :118
        }
        if (enqueue_layers(c, rows, false)) return -1;
        if (m->last()) {
            if (enqueue_head(c, rows - 1, 1)) return -1;
            HIPCHK(lnbk_argmax(c->logits, V, c->dnext, c->st, c->dout, c->dout_cap, 0, st));   // inference.go:207-211
        }
        return 0;
    };
    c->attn_long = longctx;
    if (rows == 1 && !tokens && p->use_graph) {
        GraphExec& slot = c->graphs.slot(GL_STAGE, longctx ? GF_LONG : GF_SHORT);
        if (capture_once(slot, st, [&]() -> int {
                if (body(false)) return -1;
                return lnbk_advance_state(c->st, 1, st) != hipSuccess ? fail("advance_state launch failed") : 0;
            })) return -1;
        if (c->dev_pos != pos) HIPCHK(ctx_set_state(c, pos, 0, true));
        c->call_T = 0;
        form_ran(Form::PIPELINE_REPLAY);
        HIPCHK(hipGraphLaunch(slot, st));
        c->dev_pos = pos + 1;                                // (the graph ends with advance_state)
        return 0;
    }
    HIPCHK(ctx_set_state(c, pos, 0, true));
    if (rows == 1 && !tokens) form_ran(Form::PIPELINE_EAGER);
    return body(tokens != nullptr);
}
// n tokens of the last stage, device words at src, appended to the pinned ring on stream st (the ring keeps the newest tok_cap tokens)
static int pipe_log_tokens(lnb_pipe* p, const int32_t* src, int n, hipStream_t st, int* slot_out) {
    const int slot = p->tok_n, at = slot % p->tok_cap, fit = std::min(n, p->tok_cap - at);
    HIPCHK(hipMemcpyAsync(p->h_tok + at, src, (size_t)fit * 4, hipMemcpyDeviceToHost, st));
    if (fit < n) HIPCHK(hipMemcpyAsync(p->h_tok, src + fit, (size_t)(n - fit) * 4, hipMemcpyDeviceToHost, st));
    if (slot_out) *slot_out = slot;
    p->tok_n += n;
    return 0;
}
// One side of a tick's exchange: the unit's link and stream, what lnb_handoff.h says crosses the boundary, and where those segments live.
struct PipeSide { PipeLink* link; hipStream_t stream; HandoffPlan plan; void* ptr[2]; };
static void* ctx_buf(lnb_ctx* c, HandoffBuf which) { return which == HB_HIDDEN ? (void*)c->x : which == HB_ACTS ? (void*)c->ffn : which == HB_TOKEN_OUT ? (void*)c->dnext : (void*)c->dtok; }
static PipeSide pipe_side(lnb_pipe* p, lnb_ctx* c, int rows, bool sending) {
    const lnb_model* m = p->m;
    PipeSide s{&c->link, c->stream, handoff_plan(p->rank, p->world, m->part_begin, m->part_end, sending, HU_SEQUENCE, rows, m->a.dim, m->ffn_hidden), {nullptr, nullptr}};
    for (int i = 0; i < s.plan.nseg; i++) s.ptr[i] = ctx_buf(c, s.plan.seg[i].buf);
    return s;
}
static PipeSide pipe_side(lnb_pipe* p, lnb_batch* b, bool sending) {
    const lnb_model* m = p->m;
    PipeSide s{&b->link, b->stream, handoff_plan(p->rank, p->world, m->part_begin, m->part_end, sending, HU_BATCH, b->n, m->a.dim, m->ffn_hidden), {nullptr, nullptr}};
    for (int i = 0; i < s.plan.nseg; i++) s.ptr[i] = s.plan.seg[i].buf == HB_RING ? (void*)b->ring : (void*)b->x;
    return s;
}
// The exchange of a tick, after its run part: send and / or recv (NULL: none) on the pipe's exchange stream.
static int pipe_exchange(lnb_pipe* p, const PipeSide* send, const PipeSide* recv) {
    if (p->world < 2 || (!send && !recv)) return 0;
    if (p->loop) {                                           // in-process transport: whichever side is posted second enqueues the copy
        if (recv) HIPCHK(hipEventRecord(recv->link->ev_done, recv->stream));
        for (const PipeSide* mine : {send, recv}) if (mine) {
            std::lock_guard<std::mutex> lock(g_loops_mu);
            const HandoffMsg msg{mine->link, mine->plan, {mine->ptr[0], mine->ptr[1]}};
            HandoffMsg other; char why[320];
            const HandoffBox::Result res = p->loop->box.post(p->rank, msg, &other, why, sizeof why);
            if (res == HandoffBox::QUEUED) { if (mine == recv) mine->link->recv_unmatched = true; continue; }
            const HandoffMsg &s = mine == send ? msg : other, &r = mine == send ? other : msg;
            PipeLink *sl = (PipeLink*)s.owner, *rl = (PipeLink*)r.owner;
            rl->recv_unmatched = false;                      // (its message has left the mailbox, matched or refused)
            if (res == HandoffBox::REFUSED) return fail("%s", why);
            HIPCHK(hipStreamWaitEvent(p->xs, sl->ev_done, 0));   // the result has been computed
            HIPCHK(hipStreamWaitEvent(p->xs, rl->ev_done, 0));   // nothing still reads the buffers being overwritten
            for (int i = 0; i < s.plan.nseg; i++) HIPCHK(hipMemcpyAsync(r.ptr[i], s.ptr[i], s.plan.seg[i].bytes, hipMemcpyDeviceToDevice, p->xs));
            HIPCHK(hipEventRecord(sl->ev_sent, p->xs)); sl->sent_pending = true;
            HIPCHK(hipEventRecord(rl->ev_in, p->xs)); rl->in_pending = true;
        }
        return 0;
    }
    // RCCL: ONE group with every segment of the send and of the receive; GroupEnd is called whenever GroupStart succeeded
    if (send) HIPCHK(hipStreamWaitEvent(p->xs, send->link->ev_done, 0));
    if (recv) { HIPCHK(hipEventRecord(recv->link->ev_done, recv->stream)); HIPCHK(hipStreamWaitEvent(p->xs, recv->link->ev_done, 0)); }
    NCCLCHK(p, p->api->GroupStart());
    int bad = 0; const PipeSide* failed = nullptr;
    for (const PipeSide* side : {send, recv}) if (side)
        for (int i = 0; i < side->plan.nseg && !bad; i++) {
            bad = side == send ? p->api->Send(side->ptr[i], side->plan.seg[i].bytes, LNB_NCCL_INT8, side->plan.peer, p->comm, p->xs)
                               : p->api->Recv(side->ptr[i], side->plan.seg[i].bytes, LNB_NCCL_INT8, side->plan.peer, p->comm, p->xs);
            if (bad) failed = side;
        }
    const int end = p->api->GroupEnd();
    if (bad) return fail("RCCL exchange failed: %s rank %d: %s", failed == send ? "send to" : "receive from", failed->plan.peer, p->api->GetErrorString(bad));
    if (end) return fail("RCCL exchange failed: ncclGroupEnd: %s", p->api->GetErrorString(end));
    if (send) { HIPCHK(hipEventRecord(send->link->ev_sent, p->xs)); send->link->sent_pending = true; }
    if (recv) { HIPCHK(hipEventRecord(recv->link->ev_in, p->xs)); recv->link->in_pending = true; }
    return 0;
}
extern "C" int lnb_pipeline_tick(lnb_pipe* p, lnb_ctx* run, int run_rows, int run_pos, const int32_t* run_tokens,
                                 lnb_ctx* send, int send_rows, lnb_ctx* recv, int recv_rows, int* token_slot_out) {
    if (!p) return fail("null argument");
    lnb_model* m = p->m;
    HIPCHK(hipSetDevice(m->device));
    const bool first = p->rank == 0, last = p->rank == p->world - 1;
    for (lnb_ctx* c : {run, send, recv}) if (c) { if (c->m != m) return fail("context of another model stage"); if (c->link.ensure()) return -1; }
    if (p->host && (send || recv)) return fail("this pipe has no transport (lnb_pipeline_init_host): the host layer moves lnb_ctx_hidden_ptr's buffers itself; send and recv must be NULL");
    if (token_slot_out) *token_slot_out = -1;
    if (send && send_rows > send->max_rows) return fail("a hand-off of %d rows from a context whose activation buffers hold %d rows (lnb_ctx_create_long's max_rows)", send_rows, send->max_rows);
    if (recv && recv_rows > recv->max_rows) return fail("a hand-off of %d rows into a context whose activation buffers hold %d rows (lnb_ctx_create_long's max_rows)", recv_rows, recv->max_rows);
    if (run) {
        if (run->top_k > 0) return fail("the context records token probabilities, which pipeline ticks do not support (lnb_ctx_set_token_probs(ctx, 0))");
        if (check_call(run, run_rows, run_pos)) return -1;
        if (run_tokens && !first) return fail("tokens given to a stage that does not own tok_embeddings");
        if (!run_tokens && first && run_rows != 1) return fail("the first stage needs host tokens for a multi-row step");
        if (run->link.await(run->stream, "sequence")) return -1;
        if (enqueue_stage_step(p, run, run_tokens, run_rows, run_pos)) return -1;
        if (last) {
            if (p->tok_n == 0x7FFFFFFF) return fail("pipeline token log: slot counter exhausted (2^31 tokens): create a new pipe");
            if (pipe_log_tokens(p, run->dnext, 1, run->stream, token_slot_out)) return -1;
            if (p->world == 1) HIPCHK(hipMemcpyAsync(run->dtok, run->dnext, 4, hipMemcpyDeviceToDevice, run->stream));    // the ring of a one-stage pipe
        }
        HIPCHK(hipEventRecord(run->link.ev_done, run->stream));
    }
    PipeSide ss{}, rs{};
    if (send) ss = pipe_side(p, send, send_rows, true);
    if (recv) rs = pipe_side(p, recv, recv_rows, false);
    return pipe_exchange(p, send ? &ss : nullptr, recv ? &rs : nullptr);
}

// ---- the pipeline with BATCHES as the unit that moves through the stages ---------------------------------------------------------------
// Every rank holds, per group of sequences in flight, one lnb_batch over its stage's contexts of those sequences (prefill them one by one
// with the single-sequence ticks above, then lnb_batch_set_state on every rank).  A batched tick enqueues, like lnb_pipeline_tick:
//   run : one decode step of the group on this stage -- ONE pass over the stage's weights for all its sequences (captured graph); the
//         positions advance on the device; on the last rank the n tokens are appended to the pinned log (*token_slot_out = first slot);
//   send: the group's hidden states [n, dim] to rank + 1 (the last rank: its n token words to rank 0);   recv: the mirror image.
extern "C" int lnb_pipeline_tick_batch(lnb_pipe* p, lnb_batch* run, lnb_batch* send, lnb_batch* recv, int* token_slot_out) {
    if (!p) return fail("null argument");
    lnb_model* m = p->m;
    HIPCHK(hipSetDevice(m->device));
    const bool first = p->rank == 0, last = p->rank == p->world - 1;
    for (lnb_batch* b : {run, send, recv}) if (b) { if (b->m != m) return fail("batch of another model stage"); if (b->link.ensure()) return -1; }
    if (p->host && (send || recv)) return fail("this pipe has no transport (lnb_pipeline_init_host): the host layer moves lnb_batch_boundary_ptr's buffers itself; send and recv must be NULL");
    if (token_slot_out) *token_slot_out = -1;
    if (run) {
        if (run->top_k > 0) return fail("the batch's contexts record token probabilities, which pipeline ticks do not support (lnb_ctx_set_token_probs(ctx, 0))");
        hipStream_t st = run->stream;
        if (run->link.await(st, "batch")) return -1;
        const bool ring_in = first && p->world > 1;
        if (batch_select_form(run, run->tick_long)) return -1;       // the form lnb_batch_set_state chose for this run of ticks
        if (p->use_graph) {
            GraphExec& gslot = run->graphs.slot(GL_STAGE, run->attn_long ? GF_LONG : GF_SHORT);
            if (capture_once(gslot, st, [&] { return enqueue_batch_step(run, ring_in); })) return -1;
            form_ran(Form::PIPELINE_REPLAY);
            HIPCHK(hipGraphLaunch(gslot, st));
        } else { form_ran(Form::PIPELINE_EAGER); if (enqueue_batch_step(run, ring_in)) return -1; }
        run->last_form = run->attn_long ? 1 : 0;
        if (last) {
            if (p->tok_n > 0x7FFFFFFF - LNB_BATCH_MAX) return fail("pipeline token log: slot counter exhausted (2^31 tokens): create a new pipe");
            if (pipe_log_tokens(p, run->ring, run->n, st, token_slot_out)) return -1;
        }
        HIPCHK(hipEventRecord(run->link.ev_done, st));
    }
    PipeSide ss{}, rs{};
    if (send) ss = pipe_side(p, send, true);
    if (recv) rs = pipe_side(p, recv, false);
    return pipe_exchange(p, send ? &ss : nullptr, recv ? &rs : nullptr);
}
// The RCCL binding on real hardware without a second GPU: a one-rank communicator and the pipeline's own grouped exchange -- one
// ncclSend + one ncclRecv, here both to rank 0 (itself) -- on a non-blocking stream, device buffer to device buffer, then a byte
// compare.  Exercises dlopen, the by-value unique id, the group calls and a RCCL kernel launch from a process that never loaded torch.
extern "C" int lnb_pipeline_selftest(int device, int n_bytes) {
    if (n_bytes <= 0 || n_bytes > (1 << 26)) return fail("n_bytes out of range");
    if (op_device(device)) return -1;
    const lnb_rccl_api* api = lnb_rccl_load();
    if (!api) return -1;
    lnb_nccl_id id; memset(&id, 0, sizeof id);
    int r = api->GetUniqueId(&id);
    if (r != 0) return fail("ncclGetUniqueId failed: %s", api->GetErrorString(r));
    void* comm = nullptr;
    r = api->CommInitRank(&comm, 1, id, 0);
    if (r != 0) return fail("ncclCommInitRank failed: %s", api->GetErrorString(r));
    std::vector<unsigned char> h((size_t)n_bytes), back((size_t)n_bytes);
    for (int i = 0; i < n_bytes; i++) h[i] = (unsigned char)((i * 131 + 7) >> 3);
    Stream xs; Dev<unsigned char> src, dst;
    int rc = 0;
    hipError_t e = dev_alloc(src, (size_t)n_bytes);
    if (e == hipSuccess) e = dev_alloc(dst, (size_t)n_bytes);
    if (e == hipSuccess) e = stream_create(xs, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemcpy(src, h.data(), (size_t)n_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dst, 0, (size_t)n_bytes);
    if (e != hipSuccess) rc = fail("selftest setup: %s", hipGetErrorString(e));
    if (!rc) {
        int r0 = api->GroupStart(), r1 = api->Send(src, (size_t)n_bytes, LNB_NCCL_INT8, 0, comm, xs), r2 = api->Recv(dst, (size_t)n_bytes, LNB_NCCL_INT8, 0, comm, xs), r3 = api->GroupEnd();
        const int bad = r0 ? r0 : r1 ? r1 : r2 ? r2 : r3;
        if (bad) rc = fail("RCCL self exchange failed: %s", api->GetErrorString(bad));
    }
    if (!rc && (e = hipStreamSynchronize(xs)) != hipSuccess) rc = fail("selftest sync: %s", hipGetErrorString(e));
    if (!rc && (e = hipMemcpy(back.data(), dst, (size_t)n_bytes, hipMemcpyDeviceToHost)) != hipSuccess) rc = fail("selftest readback: %s", hipGetErrorString(e));
    if (!rc && memcmp(back.data(), h.data(), (size_t)n_bytes) != 0) rc = fail("RCCL self exchange delivered different bytes");
    api->CommDestroy(comm);
    return rc;
}
// how many ranks the exchange spans, asked of the transport itself: ncclCommCount of the RCCL communicator (world > 1), the number of pipes
// that joined the in-process group (loopback), 1 for a one-stage pipe (no communicator exists)
extern "C" int lnb_pipeline_comm_count(lnb_pipe* p, int* out) {
    if (!p || !out) return fail("null argument");
    *out = 1;
    if (p->world == 1) return 0;
    if (p->host) { *out = 0; return 0; }                     // no transport of its own
    if (p->loop) { std::lock_guard<std::mutex> lock(g_loops_mu); *out = p->loop->users; return 0; }
    int n = 0;
    NCCLCHK(p, p->api->CommCount(p->comm, &n));
    *out = n;
    return 0;
}
// block until everything enqueued so far (stage steps and exchanges) has finished
extern "C" int lnb_pipeline_sync(lnb_pipe* p) {
    if (!p) return fail("null argument");
    HIPCHK(hipSetDevice(p->m->device));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}
// tokens the last stage produced, by log slot (lnb_pipeline_tick's token_slot_out); valid after lnb_pipeline_sync
extern "C" int lnb_pipeline_read_tokens(lnb_pipe* p, int first_slot, int n, int32_t* out) {
    if (!p || !out) return fail("null argument");
    if (first_slot < 0 || n < 0 || n > p->tok_n - first_slot) return fail("token slots [%d, %d) out of range (%d logged)", first_slot, first_slot + n, p->tok_n);
    if (p->tok_n - first_slot > p->tok_cap) return fail("token slot %d has been overwritten: the log keeps the newest %d tokens (%d logged)", first_slot, p->tok_cap, p->tok_n);
    HIPCHK(hipSetDevice(p->m->device));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < n; i++) out[i] = p->h_tok[(first_slot + i) % p->tok_cap];
    return 0;
}

// ---- single-op entry points for the parity tests ------------------------------------------------------
static int op_linear_impl(int device, const uint16_t* x, const uint16_t* norm_w, float eps, const uint16_t* w, uint16_t* y,
                          int rows, int n_out, int k_in, int rw, int mode = LNB_MODE_EXACT) {
    if (!x || !w || !y) return fail("null argument");
    if (rows <= 0 || n_out <= 0 || k_in <= 0) return fail("empty operand");
    if (k_in % 8) return fail("in_features must be a multiple of 8");
    if (op_device(device)) return -1;
    HIPCHK(lnbk_init());
    HIPCHK(lnbk_fast_init());
    if (mode != LNB_MODE_EXACT && mode != LNB_MODE_FAST) return fail("unknown mode %d", mode);
    if (rw == 0) rw = auto_rw(n_out, Knob::RW_OP, k_in, norm_w == nullptr);
    if (rw != 16 && rw != 32 && rw != 64 && !(rw == 4 && !norm_w && gemv_layout_takes(4, k_in)) && !(rw == 24 && gemv_layout_takes(24, k_in)))
        return fail("rw must be 16, 32 or 64 (or 4: row-broadcast layout, no fused norm, in_features a multiple of 128; or 24: quad layout, in_features a multiple of 256)");
    if ((size_t)k_in * 4 > 120 * 1024) return fail("in_features %d does not fit the LDS staging", k_in);
    DevArena a;                                             // every buffer of the call: released on every way out
    TiledDesc t{}; int64_t bytes = 0;
    if (alloc_tiled(a, t, n_out, k_in, rw, 1, bytes)) return -1;
    uint16_t* dx = a.alloc<uint16_t>((size_t)rows * k_in); uint16_t* dw = a.alloc<uint16_t>((size_t)n_out * k_in);
    uint16_t* dy = a.alloc<uint16_t>((size_t)rows * n_out); StepState* st = a.alloc<StepState>(1);
    uint16_t* dn = nullptr;
    HIPCHK(a.error());
    HIPCHK(hipMemset(st, 0, sizeof(StepState)));
    HIPCHK(hipMemcpy(dx, x, (size_t)rows * k_in * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw, w, (size_t)n_out * k_in * 2, hipMemcpyHostToDevice));
    if (norm_w) { if (arena_alloc(a, &dn, (size_t)k_in * 2)) return -1; HIPCHK(hipMemcpy(dn, norm_w, (size_t)k_in * 2, hipMemcpyHostToDevice)); }
    HIPCHK(lnbk_tile(dw, t.w, n_out, k_in, 0, 0, rw, 1, 0, nullptr));
    if (use_mfma(rows) && knob(Knob::OP_STREAM) && k_in % 128 == 0) {      // (tests: the same operator through gemm_stream_kernel)
        HIPCHK(lnbk_batch_prepare());
        const size_t mb = m16_elems(n_out, k_in, 1) * 2;
        if (arena_alloc(a, &t.w16, mb)) return -1;
        HIPCHK(hipMemset(t.w16, 0, mb));
        HIPCHK(lnbk_m16_from_tiled(t.w, t.w16, n_out, k_in, rw, 1, nullptr));
    }
    if (use_mfma(rows)) {                                   // 16 or more rows: the matrix-core path of the prefill
        uint16_t* dxn = nullptr;
        if (norm_w) { if (arena_alloc(a, &dxn, (size_t)rows * k_in * 2)) return -1; HIPCHK(lnbk_rmsnorm_rows(dx, dn, dxn, rows, k_in, eps, nullptr)); }
        GemmParams gm = gemm_of(t, norm_w ? dxn : dx, k_in, n_out, rows, st); gm.out = dy;
        HIPCHK(gemm_dispatch(mode, &gm, EPI_STORE, nullptr));
        HIPCHK(hipDeviceSynchronize());
    } else {
    GemvParams g{}; g.w = t.w; g.x = dx; g.norm_w = dn; g.eps = eps; g.K = k_in; g.n_rows = n_out; g.S = rows; g.st = st; g.out = dy;
    set_grid(g, t);
    if (mode == LNB_MODE_FAST) HIPCHK(lnbk_fast_gemv(&g, rw, 1, EPI_STORE, norm_w ? 1 : 0, nullptr));
    else HIPCHK(lnbk_gemv(&g, rw, 1, EPI_STORE, norm_w ? 1 : 0, nullptr));
    }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(y, dy, (size_t)rows * n_out * 2, hipMemcpyDeviceToHost));
    return 0;
}
// The fused ffn_norm + w1|w3 + SiLU*up launch of a one-token step on its own: y[n_out] from one row x.  packed = 0: the raw 56-row kernel; 1: from the
// 13-bit copy when the w1|w3 matrix is packable.  *status = WPACK_* of the matrix (WPACK_OK: the packed kernel ran when asked for).
extern "C" int lnb_op_rmsnorm_gate_up(int device, const uint16_t* x, const uint16_t* norm_w, float eps, const uint16_t* w1, const uint16_t* w3, uint16_t* y,
                                      int n_out, int k_in, int packed, int* status) {
    if (!x || !norm_w || !w1 || !w3 || !y) return fail("null argument");
    if (n_out <= 0 || k_in <= 0) return fail("empty operand");
    if (k_in % 8) return fail("in_features must be a multiple of 8");
    if (op_device(device)) return -1;
    HIPCHK(lnbk_init());
    if (!lnbk_w13p_supported(56, k_in)) return fail("in_features %d does not fit the LDS staging of the 56-row gate|up kernel", k_in);
    DevArena a;
    TiledDesc t{}; int64_t bytes = 0;
    if (alloc_tiled(a, t, n_out, k_in, 56, 2, bytes)) return -1;
    const size_t wn = (size_t)n_out * k_in * 2;
    uint16_t* dx = a.alloc<uint16_t>((size_t)k_in); uint16_t* dw = a.alloc<uint16_t>(wn / 2); uint16_t* dn = a.alloc<uint16_t>((size_t)k_in);
    uint16_t* dy = a.alloc<uint16_t>((size_t)n_out); StepState* st = a.alloc<StepState>(1); float* dsilu = a.alloc<float>(65536);
    unsigned* dstats = (unsigned*)a.alloc<WpackStats>(1); void* wp = nullptr;
    HIPCHK(a.error());
    HIPCHK(hipMemset(st, 0, sizeof(StepState)));
    std::vector<float> silu(1 << 16);
    for (int i = 0; i < (1 << 16); i++) { double v = (double)bf_wide_h((uint16_t)i); silu[i] = (float)(v / (1.0 + std::exp(-v))); }
    HIPCHK(hipMemcpy(dsilu, silu.data(), silu.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dx, x, (size_t)k_in * 2, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dn, norm_w, (size_t)k_in * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw, w1, wn, hipMemcpyHostToDevice)); HIPCHK(lnbk_tile(dw, t.w, n_out, k_in, 0, 0, 56, 2, 0, nullptr)); HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dw, w3, wn, hipMemcpyHostToDevice)); HIPCHK(lnbk_tile(dw, t.w, n_out, k_in, 0, 1, 56, 2, 0, nullptr)); HIPCHK(hipDeviceSynchronize());
    HIPCHK(lnbk_wpack_stats(t.w, tiled_elems(n_out, k_in, 56, 2), dstats, nullptr));
    WpackStats ws; HIPCHK(hipMemcpy(&ws, dstats, sizeof ws, hipMemcpyDeviceToHost));
    unsigned base = 0;
    const int why = wpack_window(&ws, &base);
    if (status) *status = why;
    GemvParams g{}; g.w = t.w; g.x = dx; g.norm_w = dn; g.eps = eps; g.K = k_in; g.n_rows = n_out; g.S = 1; g.st = st; g.out = dy; g.silu = dsilu;
    set_grid(g, t);
    if (packed && why == WPACK_OK) {
        if (arena_alloc(a, &wp, lnbk_wpack_w13_bytes(t.n_blocks, k_in))) return -1;
        HIPCHK(lnbk_wpack_w13(t.w, wp, k_in, t.n_blocks, base, nullptr));
        g.wp = wp; g.wp_base4 = base * 0x01010101u;
        HIPCHK(lnbk_gemv_w13p(&g, nullptr));
    } else HIPCHK(lnbk_gemv(&g, 56, 2, EPI_SILU_MUL, 1, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(y, dy, (size_t)n_out * 2, hipMemcpyDeviceToHost));
    return 0;
}
// The fused final norm + output projection launch of a one-token step on its own: y[n_out] from one row x, w = [n_out][k_in] row-major.  packed = 0: the raw
// 64-row kernel; 1: from the 13-bit copy in 128-row blocks when the matrix is packable.  n_wg > 0 caps the workgroups (a small matrix then still walks several
// blocks per workgroup); 0: one per block up to the CU count.  *status = WPACK_* of the matrix (WPACK_OK: the packed kernel ran when asked for).
extern "C" int lnb_op_rmsnorm_head(int device, const uint16_t* x, const uint16_t* norm_w, float eps, const uint16_t* w, uint16_t* y,
                                   int n_out, int k_in, int packed, int n_wg, int* status) {
    if (!x || !norm_w || !w || !y) return fail("null argument");
    if (n_out <= 0 || k_in <= 0) return fail("empty operand");
    if (k_in % 8) return fail("in_features must be a multiple of 8");
    if (n_wg < 0) return fail("n_wg must not be negative");
    if (op_device(device)) return -1;
    HIPCHK(lnbk_init());
    if (!lnbk_headp_supported(k_in)) return fail("in_features %d does not fit the LDS staging of the packed LM-head kernel", k_in);
    DevArena a;
    TiledDesc t{}; int64_t bytes = 0;
    if (alloc_tiled(a, t, n_out, k_in, 64, 1, bytes)) return -1;
    const size_t wn = (size_t)n_out * k_in * 2;
    uint16_t* dx = a.alloc<uint16_t>((size_t)k_in); uint16_t* dw = a.alloc<uint16_t>(wn / 2); uint16_t* dn = a.alloc<uint16_t>((size_t)k_in);
    uint16_t* dy = a.alloc<uint16_t>((size_t)n_out); StepState* st = a.alloc<StepState>(1); unsigned* dstats = (unsigned*)a.alloc<WpackStats>(1); void* wp = nullptr;
    HIPCHK(a.error());
    HIPCHK(hipMemset(st, 0, sizeof(StepState))); HIPCHK(hipMemset(dy, 0xFF, (size_t)n_out * 2));        // (a row the kernel does not write reads back as a NaN pattern)
    HIPCHK(hipMemcpy(dx, x, (size_t)k_in * 2, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dn, norm_w, (size_t)k_in * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw, w, wn, hipMemcpyHostToDevice)); HIPCHK(lnbk_tile(dw, t.w, n_out, k_in, 0, 0, 64, 1, 0, nullptr)); HIPCHK(hipDeviceSynchronize());
    HIPCHK(lnbk_wpack_stats(t.w, tiled_elems(n_out, k_in, 64, 1), dstats, nullptr));
    WpackStats ws; HIPCHK(hipMemcpy(&ws, dstats, sizeof ws, hipMemcpyDeviceToHost));
    unsigned base = 0;
    const int why = wpack_window(&ws, &base);
    if (status) *status = why;
    GemvParams g{}; g.w = t.w; g.x = dx; g.norm_w = dn; g.eps = eps; g.K = k_in; g.n_rows = n_out; g.S = 1; g.st = st; g.out = dy;
    set_grid(g, t);
    if (packed && why == WPACK_OK) {
        if (arena_alloc(a, &wp, lnbk_wpack_head_bytes(n_out, k_in))) return -1;
        HIPCHK(lnbk_wpack_head(t.w, wp, n_out, k_in, base, nullptr));
        g.wp = wp; g.wp_base4 = base * 0x01010101u;
        g.n_blocks = (n_out + 127) / 128; g.n_wg = g.n_blocks < g_num_cus ? g.n_blocks : g_num_cus;
        if (n_wg > 0 && n_wg < g.n_wg) g.n_wg = n_wg;
        HIPCHK(lnbk_gemv_headp(&g, nullptr));
    } else {
        if (n_wg > 0 && n_wg < g.n_wg) g.n_wg = n_wg;
        HIPCHK(lnbk_gemv(&g, 64, 1, EPI_STORE, 1, nullptr));
    }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(y, dy, (size_t)n_out * 2, hipMemcpyDeviceToHost));
    return 0;
}
// ml.Argmax (operations_impl.go:513-548) of one row of bf16 logits through argmax_kernel, the kernel of the greedy loop
extern "C" int lnb_op_argmax(int device, const uint16_t* logits_bf16, int n, int32_t* out) {
    if (!logits_bf16 || !out) return fail("null argument");
    if (n <= 0) return fail("empty operand");
    if (op_device(device)) return -1;
    DevArena a;
    uint16_t* d = a.alloc<uint16_t>((size_t)n + 8); int32_t* dn = a.alloc<int32_t>(4); StepState* st = a.alloc<StepState>(1);
    HIPCHK(a.error());
    HIPCHK(hipMemset(st, 0, sizeof(StepState)));
    HIPCHK(hipMemcpy(d, logits_bf16, (size_t)n * 2, hipMemcpyHostToDevice));
    HIPCHK(lnbk_argmax(d, n, dn, st, nullptr, 0, 0, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dn, 4, hipMemcpyDeviceToHost));
    return 0;
}
// token_probs_kernel on host rows (test aid): the records the greedy loop keeps, per row; targets (optional) as lnb_forward_score
extern "C" int lnb_op_token_probs(int device, const uint16_t* logits_bf16, int rows, int V, int top_k, const int32_t* targets,
                                  int force_serial, int32_t* ids, float* logits, float* probs, float* target_prob, double* log_z, int* serial_walks) {
    if (!logits_bf16 || !log_z || (top_k > 0 && (!ids || !logits || !probs)) || (targets && !target_prob)) return fail("null argument");
    if (rows <= 0 || V <= 0) return fail("empty operand");
    if (top_k < 0 || top_k > LNB_MAX_TOP_K) return fail("top_k must be 0..%d (got %d)", LNB_MAX_TOP_K, top_k);
    if (targets) for (int i = 0; i < rows; i++) if (targets[i] >= V) return fail("target id %d at index %d is outside the row of %d", targets[i], i, V);
    if (op_device(device)) return -1;
    const size_t R = rows, K = top_k, G = lnb_tokprob_slices(rows);
    std::vector<double> et; prob_exp_table(et);
    const size_t o_et = align256(sizeof(TokProbOut)), o_x = o_et + align256(65536 * 8), o_z = o_x + align256(R * V * 2 + 16), o_k = o_z + align256(R * LNB_TOKPROB_MAX_G * 8),
                 o_cnt = o_k + align256(R * G * K * 8), o_ids = o_cnt + align256(R * 4), o_lg = o_ids + align256(R * K * 4), o_pr = o_lg + align256(R * K * 4),
                 o_lz = o_pr + align256(R * K * 4), o_tg = o_lz + align256(R * 8), o_tl = o_tg + align256(R * 4), o_tp = o_tl + align256(R * 4),
                 o_w = o_tp + align256(R * 4), need = o_w + 256;
    Dev<char> buf;
    HIPCHK(dev_alloc(buf, need));
    char* const b = buf;
    TokProbOut o{}; o.ids = (int32_t*)(b + o_ids); o.logit = (float*)(b + o_lg); o.prob = (float*)(b + o_pr); o.log_z = (double*)(b + o_lz); o.walks = (int*)(b + o_w); o.cap = rows;
    TokProbParams p{};
    p.logits = (const uint16_t*)(b + o_x); p.V = V; p.rows = rows; p.k = top_k; p.G = (int)G; p.etab = (const double*)(b + o_et);
    p.zpart = (double*)(b + o_z); p.kpart = (uint64_t*)(b + o_k); p.cnt = (unsigned*)(b + o_cnt); p.out = (const TokProbOut*)b; p.per_row_out = 0;
    if (targets) { p.targets = (const int32_t*)(b + o_tg); p.tlogit = (float*)(b + o_tl); p.tprob = (float*)(b + o_tp); }
    p.force_serial = force_serial ? 1 : 0;
    int walks = 0;
    HIPCHK(hipMemcpy(b, &o, sizeof o, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_et, et.data(), 65536 * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_x, logits_bf16, R * V * 2, hipMemcpyHostToDevice));
    if (targets) HIPCHK(hipMemcpy(b + o_tg, targets, R * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(b + o_cnt, 0, R * 4));
    HIPCHK(hipMemset(b + o_w, 0, 4));
    HIPCHK(lnbk_token_probs(&p, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (K) HIPCHK(hipMemcpy(ids, b + o_ids, R * K * 4, hipMemcpyDeviceToHost));
    if (K) HIPCHK(hipMemcpy(logits, b + o_lg, R * K * 4, hipMemcpyDeviceToHost));
    if (K) HIPCHK(hipMemcpy(probs, b + o_pr, R * K * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(log_z, b + o_lz, R * 8, hipMemcpyDeviceToHost));
    if (targets) HIPCHK(hipMemcpy(target_prob, b + o_tp, R * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&walks, b + o_w, 4, hipMemcpyDeviceToHost));
    if (serial_walks) *serial_walks = walks;
    return 0;
}
// sample_kernel on host rows (test aid): row i with samplers[i] at pos[i] (or with u = draws[i]); info optional
extern "C" int lnb_op_sample(int device, const uint16_t* logits_bf16, int rows, int V, const lnb_sampler* samplers, const int32_t* pos, const uint64_t* draws,
                             int32_t* tokens_out, lnb_sample_info* info) {
    if (!logits_bf16 || !samplers || !pos || !tokens_out) return fail("null argument");
    if (rows <= 0) return fail("empty operand");
    if (sample_vocab_check(V)) return -1;
    char who[32];
    for (int i = 0; i < rows; i++) { snprintf(who, sizeof who, "row %d: ", i); if (sampler_check(samplers + i, who)) return -1; }
    if (op_device(device)) return -1;
    const size_t R = rows;
    std::vector<double> et; prob_exp_table(et);
    const size_t o_x = align256(65536 * 8), o_s = o_x + align256(R * V * 2 + 16), o_p = o_s + align256(R * sizeof(LnbSampler)), o_u = o_p + align256(R * 4),
                 o_t = o_u + align256(R * 8), o_i = o_t + align256(R * 4), need = o_i + align256(R * sizeof(LnbSampleInfo));
    Dev<char> buf;
    HIPCHK(dev_alloc(buf, need));
    char* const b = buf;
    HIPCHK(hipMemcpy(b, et.data(), 65536 * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_x, logits_bf16, R * V * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_s, samplers, R * sizeof(LnbSampler), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_p, pos, R * 4, hipMemcpyHostToDevice));
    if (draws) HIPCHK(hipMemcpy(b + o_u, draws, R * 8, hipMemcpyHostToDevice));
    HIPCHK(lnbk_sample((const uint16_t*)(b + o_x), V, rows, (const double*)b, (const LnbSampler*)(b + o_s), (int32_t*)(b + o_t), nullptr, nullptr, 0, 0,
                       (const int32_t*)(b + o_p), draws ? (const unsigned long long*)(b + o_u) : nullptr, info ? (LnbSampleInfo*)(b + o_i) : nullptr, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(tokens_out, b + o_t, R * 4, hipMemcpyDeviceToHost));
    if (info) HIPCHK(hipMemcpy(info, b + o_i, R * sizeof(LnbSampleInfo), hipMemcpyDeviceToHost));
    return 0;
}
// spec_sample_commit_kernel on host rows (test aid): the w columns of a verify pass whose column i holds logits row i, takes col_tokens[i] and sits at
// pos0 + i, with a generation state that honours stop_ids -> what the pass emits
extern "C" int lnb_op_spec_sample_accept(int device, const uint16_t* logits_bf16, int w, int V, const lnb_sampler* sampler, int pos0, const int32_t* col_tokens,
                                         const int32_t* stop_ids, int n_stop, int32_t* emitted, int* n_emitted, int* finished) {
    if (!logits_bf16 || !sampler || !col_tokens || !emitted || !n_emitted || (n_stop > 0 && !stop_ids)) return fail("null argument");
    if (w < 1 || w > LNB_MAX_DRAFT + 1) return fail("a verify pass has 1..%d columns (got %d)", LNB_MAX_DRAFT + 1, w);
    if (sample_vocab_check(V)) return -1;
    if (sampler_check(sampler, "")) return -1;
    if (pos0 < 0 || n_stop < 0 || n_stop > LNB_MAX_STOP_IDS) return fail("bad arguments: pos0 %d, %d stop ids (at most %d)", pos0, n_stop, LNB_MAX_STOP_IDS);
    if (op_device(device)) return -1;
    const size_t W = w;
    std::vector<double> et; prob_exp_table(et);
    const size_t o_x = align256(65536 * 8), o_s = o_x + align256(W * V * 2 + 16), o_st = o_s + align256(sizeof(LnbSampler)), o_tok = o_st + align256(W * sizeof(StepState)),
                 o_g = o_tok + align256(W * 4), o_log = o_g + align256(W * 4), o_tab = o_log + align256(W * 4), o_cnt = o_tab + align256(sizeof(BatchTab)), need = o_cnt + 256;
    Dev<char> buf;
    HIPCHK(dev_alloc(buf, need));
    char* const b = buf;
    std::vector<StepState> hst(W, StepState{});
    for (int i = 0; i < w; i++) hst[i].pos = pos0 + i;
    hst[0].n_stop = n_stop; hst[0].honour_stop = 1;
    for (int k = 0; k < n_stop; k++) hst[0].stop[k] = stop_ids[k];
    std::vector<BatchTab> tab(1, BatchTab{});
    for (int i = 0; i < w; i++) { tab[0].st[i] = (StepState*)(b + o_st) + i; tab[0].dtok[i] = (int32_t*)(b + o_tok) + i; }
    tab[0].dout[0] = (int32_t*)(b + o_log); tab[0].dout_cap[0] = w; tab[0].n = w;
    HIPCHK(hipMemset(b + o_g, 0, need - o_g));
    HIPCHK(hipMemcpy(b, et.data(), 65536 * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_x, logits_bf16, W * V * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_s, sampler, sizeof(LnbSampler), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_st, hst.data(), W * sizeof(StepState), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_tok, col_tokens, W * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_tab, tab.data(), sizeof(BatchTab), hipMemcpyHostToDevice));
    HIPCHK(lnbk_spec_sample_commit((const uint16_t*)(b + o_x), V, w, (const double*)b, (const LnbSampler*)(b + o_s), (int32_t*)(b + o_g),
                                   (const BatchTab*)(b + o_tab), (unsigned*)(b + o_cnt), nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(hst.data(), b + o_st, sizeof(StepState), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(emitted, b + o_log, W * 4, hipMemcpyDeviceToHost));
    if (hst[0].n_out < 1 || hst[0].n_out > w) return fail("internal error: a pass of %d columns emitted %d tokens", w, hst[0].n_out);
    *n_emitted = hst[0].n_out;
    if (finished) *finished = hst[0].finished;
    return 0;
}
extern "C" int lnb_op_exp_table(int device, float divisor, double* out65536) {
    if (!out65536) return fail("null argument");
    if (!(divisor > 0.0f)) return fail("divisor must be positive");
    if (op_device(device)) return -1;
    Dev<double> d;
    HIPCHK(dev_alloc(d, (size_t)65536 * 8));
    HIPCHK(lnbk_exp_table(d, divisor, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out65536, d, (size_t)65536 * 8, hipMemcpyDeviceToHost));
    return 0;
}
// What the norm of a kernel form computed (include/lnb.h): each form through its own launch function, in the kernel's REPORT instantiation -- the production
// template arguments with the walker's report compiled in.  The fused forms get a zero weight matrix of one row block; the product is discarded.
extern "C" int lnb_op_rmsnorm_sum(int device, const uint16_t* x, int rows, int k_in, float eps, int form, uint32_t* sum_bits, uint32_t* scale_bits, int32_t* walk) {
    if (!x || !sum_bits || !scale_bits || !walk) return fail("null argument");
    if (rows <= 0 || k_in <= 0) return fail("empty operand");
    if (k_in % 8) return fail("in_features must be a multiple of 8");
    if (form < 0 || form >= LNB_NORM_FORMS) return fail("unknown norm form %d", form);
    if (op_device(device)) return -1;
    HIPCHK(lnbk_init());
    if (form == LNB_NORM_BATCH_XT) HIPCHK(lnbk_batch_prepare());
    const bool alone = form == LNB_NORM_ROWS_WIDE || form == LNB_NORM_BATCH_XT || form == LNB_NORM_ROWS_WAVE;
    // the smallest matrix the form takes: one row block of its row in lnb_gemv_geom.h, in the resident layout that row reads (the packed head: one block of 128 rows)
    const GemvGeom geom = alone ? GemvGeom{} : gemv_geom(gemv_report_geom(form));
    const bool packed = geom.packed;
    const int rw = geom.rw, nch = geom.resident_nch(), n_out = alone ? 0 : geom.block_rows();
    if (form == LNB_NORM_GATE_UP56_PACKED && !lnbk_w13p_supported(56, k_in)) return 1;
    if (form == LNB_NORM_HEAD_PACKED && !lnbk_headp_supported(k_in)) return 1;
    const size_t out_rows = alone ? (size_t)((rows + 15) & ~15) : 15;      // (batch_rmsnorm_xt_kernel<true> writes whole groups of 16 columns)
    std::vector<uint16_t> ones((size_t)k_in, (uint16_t)0x3F80);
    std::vector<uint32_t> got((size_t)rows * 3);
    DevArena a;
    // the launches; a runtime error comes back as its code (refused: the launch function does not take this K)
    bool refused = false;
    auto run = [&]() -> hipError_t {
        uint16_t* dx = a.alloc<uint16_t>((size_t)rows * k_in); uint16_t* dn = a.alloc<uint16_t>((size_t)k_in);
        uint16_t* dy = a.alloc<uint16_t>(out_rows * (size_t)(alone ? k_in : n_out)); uint32_t* dno = a.alloc<uint32_t>(got.size());
        StepState* st = a.alloc<StepState>(1);
        hipError_t e = a.error();
        if (e == hipSuccess) e = hipMemset(st, 0, sizeof(StepState));
        if (e == hipSuccess) e = hipMemset(dno, 0, got.size() * 4);                     // (the walker ADDS its path word)
        if (e == hipSuccess) e = hipMemcpy(dx, x, (size_t)rows * k_in * 2, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dn, ones.data(), (size_t)k_in * 2, hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        if (alone) {
            e = form == LNB_NORM_BATCH_XT ? lnbk_batch_rmsnorm_out(dx, dn, eps, dy, k_in, rows, dno, nullptr)
                                          : lnbk_rmsnorm_rows_form(dx, dn, dy, rows, k_in, eps, form == LNB_NORM_ROWS_WIDE ? 1 : 2, dno, nullptr);
        } else {
            TiledDesc t{}; int64_t bytes = 0; float* dsilu = nullptr;
            if (alloc_tiled(a, t, n_out, k_in, rw, nch, bytes)) return hipErrorOutOfMemory;
            if (nch == 2) {
                if (!(dsilu = a.alloc<float>(65536))) return a.error();
                if ((e = hipMemset(dsilu, 0, (size_t)65536 * 4)) != hipSuccess) return e;
            }
            GemvParams g{}; g.w = t.w; g.norm_w = dn; g.eps = eps; g.K = k_in; g.n_rows = n_out; g.st = st; g.out = dy; g.silu = dsilu;
            g.n_blocks = 1; g.n_wg = 1; g.sched = form == LNB_NORM_QUAD24_SCHED ? 1 : 0;
            if (packed) {                                                 // the 13-bit copy of the zero matrix (window base 0)
                void* wp = a.alloc<char>(form == LNB_NORM_HEAD_PACKED ? lnbk_wpack_head_bytes(n_out, k_in) : lnbk_wpack_w13_bytes(1, k_in));
                if (!wp) return a.error();
                e = form == LNB_NORM_HEAD_PACKED ? lnbk_wpack_head(t.w, wp, n_out, k_in, 0, nullptr) : lnbk_wpack_w13(t.w, wp, k_in, 1, 0, nullptr);
                if (e != hipSuccess) return e;
                g.wp = wp; g.wp_base4 = 0;
            }
            const int per = packed ? 1 : 15;                              // rows per launch, as production launches them
            for (int r0 = 0; r0 < rows && e == hipSuccess; r0 += per) {
                g.S = rows - r0 < per ? rows - r0 : per; g.x = dx + (size_t)r0 * k_in; g.norm_out = dno + (size_t)r0 * 3;
                e = lnbk_gemv_norm_report(&g, form, nullptr);
            }
        }
        if (e == hipErrorInvalidValue) { refused = true; return hipSuccess; }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(got.data(), dno, got.size() * 4, hipMemcpyDeviceToHost);
        return e;
    };
    const hipError_t e = run();
    if (e != hipSuccess) return fail("lnb_op_rmsnorm_sum: %s", hipGetErrorString(e));
    if (refused) return 1;
    for (int r = 0; r < rows; r++) { sum_bits[r] = got[(size_t)r * 3]; scale_bits[r] = got[(size_t)r * 3 + 1]; walk[r] = (int32_t)got[(size_t)r * 3 + 2]; }
    return 0;
}
extern "C" int lnb_op_linear(int device, const uint16_t* x, const uint16_t* w, uint16_t* y, int rows, int n_out, int k_in, int rw) {
    return op_linear_impl(device, x, nullptr, 0.0f, w, y, rows, n_out, k_in, rw);
}
// the same two operators in a given arithmetic mode (LNB_MODE_FAST: the split-K kernels; norm_w may be NULL)
extern "C" int lnb_op_linear_mode(int device, const uint16_t* x, const uint16_t* norm_w, float eps, const uint16_t* w, uint16_t* y,
                                  int rows, int n_out, int k_in, int rw, int mode) {
    return op_linear_impl(device, x, norm_w, eps, w, y, rows, n_out, k_in, rw, mode);
}
extern "C" int lnb_op_rmsnorm_linear(int device, const uint16_t* x, const uint16_t* norm_w, float eps, const uint16_t* w, uint16_t* y,
                                     int rows, int n_out, int k_in, int rw) {
    if (!norm_w) return fail("null argument");
    return op_linear_impl(device, x, norm_w, eps, w, y, rows, n_out, k_in, rw);
}
