/*
 * lnb.h -- C ABI of liblnb_hip.so: the MI355X-native replacement for the LlamaTransformer.Forward
 * hot path of adalkiran/llama-nuts-and-bolts (reference file:line citations are relative to that repo).
 *
 * This is the drop-in boundary: the reference has no plugin registry, the seam is
 * the Go method itself, so each entry point below is what the body of one Go function becomes through
 * cgo (binding shown in INTEGRATION.md).  Plain pointers and sizes only; no torch / HIP types.
 *
 * Conventions: every function returns 0 on success, <0 on error; lnb_last_error() returns a
 * thread-local message (the Go side wraps it in errors.New, mirroring the reference's fmt.Errorf paths).
 * The library owns DEVICE memory only: host pointers are never retained after a call returns
 * (the reference's weight tensors are sub-slices of an mmap, src/torch/types.go:51-55).
 * Handles: lnb_model is immutable after lnb_model_finalize and may be shared by several lnb_ctx
 * (reference: the transformer is read-only after construction, one InferenceContext per GenerateString
 * call, src/inference/inference.go:174); an lnb_ctx must be used by one thread at a time.  The entry points
 * may be mixed on one context (ticks, lnb_forward, lnb_decode_greedy, lnb_profile_kernel): each one re-establishes the device-side position.
 */
#ifndef LNB_H
#define LNB_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct lnb_model lnb_model;
typedef struct lnb_ctx lnb_ctx;

/* mirrors model.ModelArgs (src/model/modelargs.go:12-27; defaults :29-44) */
typedef struct lnb_model_args {
    int32_t dim;                 /* 4096 */
    int32_t n_layers;            /* 32 */
    int32_t n_heads;             /* 32 */
    int32_t n_kv_heads;          /* 8; <0 => n_heads (llamatransformer.go:73-75) */
    int32_t vocab_size;          /* 128256 */
    int32_t multiple_of;         /* 1024 */
    double  ffn_dim_multiplier;  /* 1.3; <= -1 => unset (llamatransformer.go:573-575) */
    float   norm_eps;            /* 1e-5 */
    int32_t use_scaled_rope;     /* 1 */
    double  rope_theta;          /* 500000; <=0 => 500000 (llamatransformer.go:80-82) */
    int32_t max_seq_len;         /* 2048; RoPE table has 2*max_seq_len rows (llamatransformer.go:109) */
} lnb_model_args;

/* ABI version of this header.  A binding (cgo, ctypes, JNI ...) compares it with lnb_abi_version() of the library it loaded and refuses a mismatch:
 * round 5 changed lnb_batch_decode_until's signature (`finished` in the middle) -- a stale binding would have passed a float* where the library writes
 * n int32 values.  Bumped whenever an existing entry point changes its arguments; additions do not bump it.
 *   6: lnb_batch_decode_until(..., n_generated, finished, ms_out); lnb_runtime_info; lnb_abi_version itself. */
#define LNB_ABI_VERSION 6
int lnb_abi_version(void);

const char* lnb_last_error(void);
int lnb_device_count(int* out_count);
/* Runtime facts a host needs before it trusts a run with SEVERAL contexts in flight (one InferenceContext per generation, one goroutine each:
 * src/inference/inference.go:163-174).  The HIP runtime spreads a process's streams over a fixed number of hardware queues (its default: 4,
 * read from the process environment when the runtime initialises) and streams that share a queue serialise; the library leaves that setting
 * to the host.  hw_queues_measured (probe_queues != 0, 4-20 ms): streams that really ran concurrently.
 * A host warns when contexts in flight > min(hw_queues_expected, hw_queues_measured or expected) (bench.py, go/inferencecontext_hip.go do). */
typedef struct lnb_runtime_info_t {
    int32_t abi_version;
    int32_t device, n_cus;
    int32_t shader_clock_khz, memory_clock_khz, wall_clock_khz;   /* hipDeviceAttributeClockRate / MemoryClockRate / WallClockRate */
    int32_t hw_queues_env;                 /* GPU_MAX_HW_QUEUES in the process environment now (0: unset = the runtime's default 4) */
    int32_t hw_queues_set_by_library;      /* always 0: the library sets no default (kept for the ABI) */
    int32_t hip_initialised_before_load;   /* 1: /dev/kfd was already open when the library was loaded (HIP was in use before) */
    int32_t hw_queues_expected;            /* what the runtime will have honoured: hw_queues_env, or 4 when unset */
    int32_t hw_queues_measured;            /* probe: 32 spinning one-wave kernels on 32 streams ran in 32 / this many rounds (0: not probed) */
    float   probe_ms;
    char    device_name[64];
    char    arch[32];
} lnb_runtime_info_t;
int lnb_runtime_info(int device, int probe_queues, lnb_runtime_info_t* out);
/* preflight of a multi-GPU host (bench.py --gpus N prints it per rank before any timing): the device behind an index (any out pointer may be
 * NULL) and whether `device` can map `peer`'s memory -- the peer-to-peer path RCCL's ncclSend / ncclRecv ride on (xGMI inside a node) */
int lnb_device_info(int device, char* name, int name_cap, int64_t* hbm_bytes, int* n_cus, char* arch, int arch_cap);
int lnb_device_can_access_peer(int device, int peer, int* out);
/* The PCI bus id of a device index ("0000:c1:00.0"): what tells two ranks apart that both say "device 0" because their launcher gave each of them
 * one visible GPU (a multi-GPU preflight compares these, not the indices). */
int lnb_device_pci_bus_id(int device, char* out, int cap);

/* ---- model: replaces model.NewLlamaTransformer (src/model/llamatransformer.go:64-113) --------------
 * A model handle owns the device copy of one pipeline STAGE: transformer blocks [layer_begin,layer_end),
 * plus tok_embeddings when layer_begin == 0 and norm + output when layer_end == n_layers.
 * layer_begin=0, layer_end=n_layers is the whole model on one GPU. */
int lnb_model_create(const lnb_model_args* args, int device, int layer_begin, int layer_end, lnb_model** out);
/* The same with the range in THIRDS of a block: 3l = attention part of block l (attention_norm, wq|wk|wv, attention, wo + residual,
 * llamatransformer.go:222-232), 3l+1 = gate/up part (ffn_norm, w1|w3, SiLU*up, :237, :601-617), 3l+2 = down part (w2 + residual,
 * :619, :248).  A pipeline stage may start or end inside a block: after the attention part the live state is again one [S, dim]
 * vector; after the gate/up part it is that vector plus the [S, ffn_hidden] activations (lnb_ctx_hidden_ptr(c, 2)).  The parts cost
 * about the same HBM time, so pipeline.stage_parts balances the stages to a third of a block.
 * lnb_model_create(.., lb, le, ..) == lnb_model_create_parts(.., 3*lb, 3*le, ..). */
int lnb_model_create_parts(const lnb_model_args* args, int device, int part_begin, int part_end, lnb_model** out);
int lnb_model_destroy(lnb_model* m);

/* FFN hidden size derivation (llamatransformer.go:569-577) */
int lnb_model_ffn_hidden_dim(const lnb_model_args* args);

/* Bind one checkpoint tensor by its Meta key (the names the reference binds with getTensor/getLayerTensor,
 * llamatransformer.go:84,98,105,191,202,273-283,580-587; shape check = loader.go:183-192).
 * host_bf16 is the reference layout: row-major [out_features,in_features] bf16 bits; it is copied to the
 * device and re-tiled; the caller keeps ownership.  Tensors of layers outside this stage are rejected. */
int lnb_model_set_tensor(lnb_model* m, const char* name, const uint16_t* host_bf16, const int64_t* shape, int rank);
/* read a tensor back in the reference layout (tests / debugging) */
int lnb_model_get_tensor(lnb_model* m, const char* name, uint16_t* host_bf16, int64_t nelem);
/* the tensors this model stage binds: index 0..n-1 -> checkpoint name, expected shape (rank 1: [n]; rank 2: [out,in]) */
int lnb_model_num_tensors(const lnb_model* m);
int lnb_model_tensor_info(const lnb_model* m, int index, const char** name, int64_t* shape2, int* rank);
/* random-init every tensor of this stage on the device with the counter-based generator of DESIGN.md
 * ("Synthetic weights"): no checkpoint is needed for benchmarking */
int lnb_model_fill_synthetic(lnb_model* m, uint64_t seed);
/* builds PrecomputedFreqsCis (llamatransformer.go:109,694-751) and the SiLU table (src/ml/activations.go:15-20);
 * rope_rows <= 0 selects the reference's 2*max_seq_len rows, a larger value extends the table by the same formula */
int lnb_model_finalize(lnb_model* m, int rope_rows);
/* LlamaTransformer.PrecomputedFreqsCis as [rows][head_dim/2][2] f32 (exported field, llamatransformer.go:24) */
int lnb_model_rope_table(lnb_model* m, float* out, int64_t nfloats, int* rows_out);
int64_t lnb_model_weight_bytes(lnb_model* m);

/* ---- context: replaces model.NewInferenceContext (src/model/inferencecontext.go:17-46) ---------------
 * device-resident, zero-filled CacheK/CacheV [seq_len, n_kv_heads, head_dim] bf16 per owned layer.
 * Context length: up to about 23000 positions (23552: the long-context decode attention keeps 4 bytes per position in the LDS here); head_dim 32, 64
 * or 128.  One-token calls, calls of 16 or more rows, batched decode (lnb_batch_*) and speculative decode reach that far: beyond what the
 * one-workgroup-per-head attention stages in the LDS (12 bytes per position: ~7800 positions at head_dim 128, ~10800 at 64) they run the
 * long-context kernels.  Calls of 2..15 rows use a kernel that stages 12 bytes per position and fail beyond ~7800 positions (head_dim 128; ~10800 at 64)
 * (lnb_forward_append runs the multi-row long-context attention there: still one pass over the weights, lnb_ctx_set_rows_attention).  A longer seq_len is refused ("... too long ..."): lnb_ctx_create_long goes further. */
int lnb_ctx_create(lnb_model* m, int seq_len, lnb_ctx** out);
/* A context of up to LNB_MAX_SEQ_LEN (131072) positions whose per-call activation buffers hold max_rows rows instead of seq_len.
 * Capacity: seq_len 1..LNB_MAX_SEQ_LEN (<= 0: the model's max_seq_len); above, the call fails ("... too long ..."); the model's RoPE table must have at
 * least seq_len rows (lnb_model_finalize's rope_rows), else the call fails and says so.  Beyond lnb_ctx_create's ~23000 positions the PV kernel of the
 * long-context decode attention takes an LDS layout that does not grow with the context (72 KB: the p_j are evaluated where they are used); up to that
 * capacity such a context launches exactly what lnb_ctx_create's does.  Everything reaches the whole context: one-token steps, lnb_decode_greedy[_until],
 * calls of 16 or more rows, lnb_forward_append of any row count (2..15 rows beyond ~7800 positions run the multi-row long-context attention, whose LDS does not grow with the context),
 * token probabilities, scoring, stop ids, lnb_batch_* and lnb_decode_speculative_until; every result is bit-identical to what a context of another
 * capacity gives.  The attention forms that stage the whole context in the LDS (lnb_ctx_set_attention bits 2 / 3, LNB_ATTN_ONE, LNB_ATTN_LAZY=0) run the
 * default pair beyond ~23000 positions of capacity.
 * max_rows: the rows of x, h, xn, q, att, ffn (and of lnb_ctx_hidden_ptr's buffers); <= 0 or > seq_len: seq_len.  Every entry point that takes `seq` rows
 * -- lnb_forward[_stage[_begin]], lnb_forward_append, lnb_forward_score[_append], the rows of a lnb_pipeline_tick -- refuses seq > max_rows up front, with
 * both numbers in the message.  A 131072-position context of the 8B shape would otherwise carry ~9 GB of activation buffers beside its 17 GB of KV cache:
 * feed a long prompt as lnb_forward_append calls of max_rows rows.  The KV caches, the token log and the attention scratch stay sized by seq_len. */
#define LNB_MAX_SEQ_LEN 131072
int lnb_ctx_create_long(lnb_model* m, int seq_len, int max_rows, lnb_ctx** out);
int lnb_ctx_max_rows(const lnb_ctx* c, int* out);
int lnb_ctx_destroy(lnb_ctx* c);
int lnb_ctx_reset(lnb_ctx* c);                                       /* zero the caches again */
/* InferenceContext.CacheK/CacheV[layer] (exported, poked by llamatransformer_simulated_test.go:527-538) */
int lnb_ctx_read_kv(lnb_ctx* c, int layer, int which /*0=K 1=V*/, uint16_t* host_bf16);
/* ---- a computed prefix shared between contexts ("a shared prefix followed by per-user text") -------------------------------------------
 * A KV row depends on the tokens up to it and on nothing a context owns, so the rows one context computed for a text are, bit for bit, the rows
 * any other context of the same model handle would compute for it: sharing a prefix is a copy, exact by construction.
 * lnb_ctx_fork: when it returns, the KV rows [0, n_pos) of every layer the stage owns are, in each of the n_dst destinations, the source's bits;
 *   rows at and beyond n_pos of a destination and the whole source are untouched.  ONE kernel launch (kv_fork_kernel: every source vector is
 *   read once and stored to every destination); LNB_FORK_COPY=1 runs the same contract on the copy engine.  Nothing else is copied -- not the
 *   token log, the device position, stop ids, draft settings or token-probability logs: every entry point re-establishes the position itself, so
 *   lnb_forward_append, lnb_decode_greedy[_until], lnb_decode_speculative_until (history = the prefix's tokens) and lnb_batch_* continue a
 *   destination at n_pos.  Capacities may differ in either direction (lnb_ctx_create_long's included); members of a live batch may be source and
 *   destinations (a batch holds pointers, not contents); the arithmetic mode does not matter (both modes share the cache).  The call waits for
 *   the streams of the source and of every destination, copies on the source's stream and returns when the copy has finished; no captured
 *   graph is dropped.  n_pos == 0 succeeds and copies nothing.
 *   Refused, each with a message, arguments before any handle is touched: NULL src, dsts or entry; n_dst outside 1..LNB_MAX_FORK; a negative
 *   n_pos; a destination that is the source or appears twice; a destination of another lnb_model handle (a stage's contexts fork among
 *   themselves); n_pos beyond the source's or a destination's capacity; a source or destination whose lnb_forward_stage_begin has not been
 *   ended.  If the call's device table cannot be allocated it fails with every cache as it was.
 * lnb_ctx_save_prefix / lnb_ctx_load_prefix: the same rows in host memory (a prefix cache in RAM or on disk), by strided copies, no kernel.
 *   The blob is capacity-independent and deterministic (the same rows always give the same bytes):
 *     bytes 0..63   header, little-endian: "LNBKV1" and two zero bytes; then 32-bit words: format version (1), n_pos, the stage's part_begin and
 *                   part_end (lnb_model_create_parts), n_kv_heads, head_dim, the number of cached layers; 28 reserved zero bytes;
 *     then per cached layer, in layer order: K as [kv head][head_dim/8][n_pos][8] bf16 (the device layout of a context of capacity n_pos),
 *                   V as [n_pos][n_kv_heads * head_dim] bf16.
 *   lnb_ctx_prefix_bytes: the blob's size for n_pos positions (64 + cached layers * 2 * n_pos * kv_dim * 2), < 0 on error.
 *   lnb_ctx_save_prefix refuses a `cap` below that.  lnb_ctx_load_prefix writes rows [0, n_pos) and reports n_pos (n_pos_out may be NULL); it
 *   refuses, before anything is written: a short or over-long blob, a wrong magic or version, a geometry or stage range that differs from the
 *   context's model, n_pos beyond the context's capacity.
 *   The blob carries NO model identity: loading rows that were computed with other weights is the caller's mistake and is not detected. */
#define LNB_MAX_FORK 128
int lnb_ctx_fork(lnb_ctx* src, int n_pos, lnb_ctx* const* dsts, int n_dst);
int64_t lnb_ctx_prefix_bytes(const lnb_ctx* c, int n_pos);
int lnb_ctx_save_prefix(lnb_ctx* c, int n_pos, void* host, int64_t cap);
int lnb_ctx_load_prefix(lnb_ctx* c, const void* host, int64_t nbytes, int* n_pos_out);
/* Arithmetic mode of a context.  LNB_MODE_EXACT (default): every matmul output is the reference's single k-ordered f32 chain
 * (src/ml/operations_lineartransform.go:46-65), every intermediate bit-identical to the Go CPU path.  LNB_MODE_FAST: the same
 * operators and bf16 truncation points with split-K f32 sums (decode) and bf16 matrix-core GEMMs (prefill): HBM / MFMA bound instead
 * of add-latency bound.  NOT a parity mode: per operator it stays within one bf16 ulp of the chain, but after 32 blocks the logits are
 * NOT within the north star's 1e-2 of the reference's (measured on the 8B shape: max |dlogit| 0.578, argmax differs in 13.9 % of
 * teacher-forced steps -- NOTES.md 6.2) and token ids diverge.  Opt-in, per context, switchable between calls; the KV cache is
 * shared by both modes. */
enum { LNB_MODE_EXACT = 0, LNB_MODE_FAST = 1 };
int lnb_ctx_set_mode(lnb_ctx* c, int mode);
int lnb_ctx_get_mode(const lnb_ctx* c);
/* Kernel FORMS of the exact one-token steps of a context (same arithmetic, same bits).  LNB_SCHED_LATENCY (default): one generation owns the
 * chip -- every launch takes all CUs with eight or nine waves and 91..124 KB of LDS per workgroup.  LNB_SCHED_THROUGHPUT: for several
 * generations in flight on one GPU, one context and stream each (the reference's one InferenceContext per generation, inference.go:174; what
 * every pipeline rank runs): every workgroup stays at or below 57 KB of LDS, so that a chain-bound launch of one context shares the CUs with
 * the HBM-bound gate|up launch of another.  Slower for a single stream, faster in aggregate (bench.py: sequences_in_flight).  Switchable
 * between calls; the context's captured graphs are dropped. */
enum { LNB_SCHED_LATENCY = 0, LNB_SCHED_THROUGHPUT = 1 };
int lnb_ctx_set_schedule(lnb_ctx* c, int sched);
int lnb_ctx_get_schedule(const lnb_ctx* c);
/* Decode attention form (both bit-identical to the reference arithmetic): one-token calls whose context exceeds long_threshold
 * positions use the long-context kernels (scores over all CUs, PV per (head, 16-dim slice), softmax denominator certified against
 * the reference's serial f64 sum instead of walked).  long_threshold < 0: keep (default 512, env LNB_ATTN_LONG_T).  force_zseq is a set of
 * test / experiment switches: bit 0 (1) = always walk the serial sum; bit 3 (8) = run both phases in ONE launch (attn_one_kernel, round 6: the
 * (head, slice) workgroups exchange the scores inside the launch behind a BOUNDED poll -- a workgroup whose peers are not resident computes their
 * share itself, so two contexts can never wait for each other; same bits; measured slower than the two launches, hence opt-in, also by
 * LNB_ATTN_ONE=1; latency schedule only); bit 2 (4) = one launch with every poll timing out; bit 1 (2) = two launches whatever the environment says.
 * A context beyond lnb_ctx_create's capacity (lnb_ctx_create_long) cannot stage itself in the one-launch form's LDS: bits 2 / 3 run the two launches there.
 * lnb_ctx_zseq_count: rows that could not be certified and walked the serial sum. */
int lnb_ctx_set_attention(lnb_ctx* c, int long_threshold, int force_zseq);
int lnb_ctx_zseq_count(lnb_ctx* c, int* out);
/* Diagnostics of the fused RMSNorm (llamatransformer.go:222, :237, :166: RMSNorm in front of wq|wk|wv, w1|w3, output): rows of one-token calls
 * whose sum of squares left the branch-free item walk for the slower record walk (same bits either way; ~2.5 % of gaussian rows). */
int lnb_ctx_norm_fallbacks(lnb_ctx* c, int* out);
/* Which matrix-core attention the context's LAST multi-row call (llamatransformer.go:409-514 with S >= 16, exact mode) ran: 3 = attn_mfma3_kernel (the scores
 * computed once, their 16-bit exp-table indices kept in the context's scratch), 1 = attn_mfma_kernel (the scores computed twice: the scratch was refused --
 * above LNB_ATTN_SIDX_MB, or no device memory for it), 0 = none (no such call yet, fewer than 16 rows, head_dim 32, tolerance mode).  Same bits either way;
 * a bench prints it so that a silently refused scratch shows.  The scratch is 512 bytes per (head, 16 query rows, 16 positions) -- 1.07 GB for a 4096-row prompt of the
 * 8B shape --, one per context, grown on demand; a context's first one-token call after the prompt frees it when it is larger than LNB_ATTN_SIDX_KEEP_MB (default 256). */
int lnb_ctx_prefill_attention_form(const lnb_ctx* c, int* out);
/* The launch tally: which kernel FORM the launch layer picked (csrc/lnb_forms.h lists the forms: one row per arm of a launch function's choice by shape or by
 * LNB_* knob -- "gemm_mfma.t64", "gemm_stream.chain.ntw2", "rmsnorm_rows.wave" ...).  Process-wide counters, incremented on the host where the kernel is chosen; a
 * launch recorded during a graph capture counts once, at capture, and replays do not count.  What it is for: a test (or a bench) that sets a knob asserts that the
 * form it meant really ran -- a ONCE knob set after its first use is silently without effect.
 *   lnb_form_count: launches of `form` since the last reset with epilogue `epi` (0 store, 1 RoPE + KV append, 2 residual, 3 SiLU*up; forms that are no product count
 *   under 0), epi = -1: the sum.  An unknown name is an error whose message names it.
 *   lnb_form_name: the name of row `index` (0 .. until it fails): enumeration. */
int lnb_form_count(const char* form, int epi, int64_t* out);
int lnb_form_count_reset(void);
int lnb_form_name(int index, const char** name);
/* optional per-layer progress hook = infContext.Logf("Transformer block layer %d / %d was run, took %.4f sec(s)")
 * (llamatransformer.go:157-163); forces a per-layer stream sync, so it is off by default */
typedef void (*lnb_layer_cb)(int layer_1based, int n_layers, double secs, void* user);
int lnb_ctx_set_layer_callback(lnb_ctx* c, lnb_layer_cb cb, void* user);

/* ---- forward: replaces (*LlamaTransformer).Forward (src/model/llamatransformer.go:145-180) -------------
 * tokens: [seq] int32 (caller-owned, not retained, inference.go:195-202); start_pos as in the reference.
 * logits_out: caller-allocated [seq, vocab_size] f32, bf16-representable values (llamatransformer.go:170-177);
 *   NULL => only the last row is evaluated and only argmax_last_out is produced.
 * argmax_last_out: ml.Argmax of the last row (first maximum wins, operations_impl.go:529-541); may be NULL.
 * Errors (same conditions as the reference): seq == 0 "empty token array" (llamatransformer.go:146-148);
 * start_pos+seq beyond the RoPE table or the KV cache (tensor.go:275-279; the reference silently drops the
 * SetSlice error at llamatransformer.go:402-403 and then fails in Slice :409 -- here it fails up front);
 * seq > 1 with (start_pos+seq) % seq != 0 "two tensor shapes cannot be broadcasted" (tensor.go:414-428).
 * Requires a whole-model handle (layer_begin == 0 && layer_end == n_layers).
 * Non-finite rows: the multi-row attention kernels rest on finite K / V rows (a masked entry is e = 0 without its score, positions beyond the
 *   diagonal are skipped).  The reference ADDS the mask (NaN + -inf = NaN) and multiplies p = +0 by every V row of the call, so one NaN row makes
 *   every row of a modulo-mask call NaN.  A multi-row call therefore scans the K / V rows each layer writes (as lnb_ctx_load_prefix scans the rows
 *   it loads; lnb_ctx_fork hands the source's flag on; lnb_ctx_reset clears it), and a context that holds an inf or a NaN recomputes the attention
 *   of its multi-row calls the reference's way, row by row (slow; the same bits as the reference, tests/test_gpu_attention_crafted.py).  Calls on
 *   finite rows launch one scan and one early-returning kernel per layer beyond what they launched before.
 *   Stated limit: rows written by ONE-TOKEN calls, batched and speculative decode are not scanned, and a +inf SCORE of finite rows (|k| ~ 1e38) at
 *   a masked position is not seen by the scan; a later modulo-mask call at start_pos > 0 over such rows may keep rows finite that the reference
 *   makes NaN.  lnb_forward_append is not affected: every earlier row is unmasked for every row of an append. */
int lnb_forward(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, float* logits_out, int32_t* argmax_last_out);

/* ---- causal multi-row append: extend a live context by seq tokens in ONE call, at any start position -------------------------------
 * lnb_forward restates the reference's attention mask: the [seq, seq] upper triangle broadcast by modulo over the [seq, start_pos + seq]
 * scores (tensoriterators.go:47-55).  At start_pos > 0 that is not a continuation of the cached text (and it is refused unless
 * (start_pos + seq) % seq == 0); it is the correct behaviour for Forward and it stays.  lnb_forward_append is the other thing a caller wants:
 * row i attends to every cached position 0 .. start_pos + i.
 *   Contract: logits_out ([seq, vocab_size], may be NULL as for lnb_forward), the KV rows [start_pos, start_pos + seq) of every layer and
 *   argmax_last_out are BIT-IDENTICAL to seq consecutive one-token lnb_forward calls at start_pos, start_pos + 1, ...; cache rows below
 *   start_pos are read and never written.  Any seq >= 1 with start_pos + seq within the KV cache and the RoPE table is accepted: there is no
 *   (start_pos + seq) % seq condition.  At start_pos == 0 the result equals lnb_forward of the same rows.
 *   Why it is exact: the linear layers are per-row chains already; the reference's softmax subtracts no maximum, so a masked entry adds +0 to
 *   the f64 sum and to the PV chain -- a row masked to j <= start_pos + i IS the shorter row of the one-token step.
 *   That argument holds for finite V rows; +0 x NaN is NaN.  A call whose own rows hold an inf or a NaN (scanned as they are written, see
 *   lnb_forward) is recomputed row by row with each row's own T, so the contract holds there too: the rows before a NaN row stay finite.
 *   Afterwards lnb_decode_greedy[_until], lnb_decode_speculative_until, lnb_batch_* and further appends continue the context.
 *   Kernels: 16 or more rows at head_dim 64 / 128 run the matrix-core attention with the causal mask (tiles above the shifted diagonal are
 *   skipped); 2..15 rows, and any row count at head_dim 32, the row-per-workgroup kernel.  Where that kernel cannot stage the context (see
 *   lnb_ctx_create) the call runs the multi-row long-context attention (lnb_ctx_set_rows_attention below): one pass over the weights, K and V
 *   read once for all rows; only if its scratch cannot be allocated do the rows run as one-token steps inside the call.
 *   Refused, each with a message: a stage handle that is not the whole model; LNB_MODE_FAST (the tolerance mode is frozen and its flash
 *   kernel keeps the modulo mask); NULL tokens, seq <= 0 or a negative start_pos (checked before the handle is touched); positions beyond the
 *   KV cache or the RoPE table.
 * lnb_forward_score_append: the same call with lnb_forward_score's outputs -- per row the target's logit and probability and ln Z, the bits
 *   of seq one-row lnb_forward_score calls (targets[i] < 0: NaN logit and prob for that row; targets[i] >= V is an error). */
int lnb_forward_append(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, float* logits_out, int32_t* argmax_last_out);
int lnb_forward_score_append(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, const int32_t* targets,
                             float* target_logit, float* target_prob, double* log_z, int32_t* argmax_last_out);
/* Multi-row long-context attention: up to 16 consecutive rows of one context per launch pair, every K and V row read once for all of them; each
 * row is the one-token step at its position, bit for bit (certified softmax per row, serial sum where certification fails).
 * Appends of 2..15 rows (any row count at head_dim 32) whose start_pos + seq exceeds long_threshold run it; long_threshold < 0 keeps the current
 * value; the default is what the row-per-workgroup kernel stages in the LDS (~7800 positions at head_dim 128), i.e. exactly the calls that kernel
 * cannot take; 0 sends every such call there.  Calls beyond the row-per-workgroup kernel's reach run it whatever the threshold.  flags bit 0:
 * every row walks the serial sum (counted per (row, head) in lnb_ctx_zseq_count).  flags bit 1: the verify passes of lnb_decode_speculative_until
 * run it wherever they would run the long-context pair (off by default).  The scratch (16 * n_heads * seq_len * 8 bytes, shared with the verify
 * passes) is allocated when a call first needs it.  Arguments are checked before the handle; refused while a lnb_forward_stage_begin is pending.
 * Rows per PV workgroup: LNB_ATTN_ROWS_RPW. */
int lnb_ctx_set_rows_attention(lnb_ctx* c, int long_threshold, int flags);
/* the attention of the last lnb_forward_append / lnb_forward_score_append: 0 none yet or a one-row call, 1 the row-per-workgroup kernel,
 * 2 the matrix-core kernel, 3 one-token steps inside the call, 4 the multi-row long-context pair */
int lnb_ctx_append_attention_form(const lnb_ctx* c, int* out);

/* ---- ragged append to many contexts: n contexts extended by n_rows[s] tokens each, in passes of up to 128 rows over the weights -----------
 * After lnb_ctx_fork has put a shared prefix into many contexts, each of them still needs its own text appended.  One lnb_forward_append per
 * context walks the weights once per context (and, below 16 rows, once per row); this call packs the rows of ALL members, in member order, into
 * batched steps of up to 128 columns -- the kernels of lnb_batch_decode, each column the one-token step of one row with its own position, token
 * and KV caches -- so 256 rows cost two passes over the weights.
 *   Member s is extended by n_rows[s] tokens at start_pos[s]; tokens is the concatenation of the members' rows in member order (sum(n_rows)
 *   entries).
 *   Contract: for every member, the KV rows [start_pos[s], start_pos[s] + n_rows[s]) of every layer, its rows of logits_out
 *   ([sum(n_rows), vocab_size] f32 in the row order of tokens; may be NULL) and argmax_out[s] (ml.Argmax of its last row; the array may be NULL)
 *   are BIT-IDENTICAL to lnb_forward_append(ctxs[s], its tokens, n_rows[s], start_pos[s], ...) on a context holding the same rows below
 *   start_pos[s] -- hence to n_rows[s] one-token steps.  Cache rows below start_pos[s] are read and never written; rows at and beyond
 *   start_pos[s] + n_rows[s] are untouched.  Nothing else of a member changes (token log, stop ids, draft settings, token-probability logs); its
 *   cached device position is invalidated, as lnb_batch_decode does.  Afterwards lnb_decode_greedy[_until], lnb_decode_speculative_until,
 *   lnb_batch_* and further appends continue a member.  Members may have any capacities (lnb_ctx_create_long's included) and may belong to a
 *   live batch.  A member's max_rows does NOT limit n_rows[s]: the rows live in the call's own buffers (kept in the model handle, created on
 *   first use, freed by lnb_model_destroy), not in the member's.
 *   The call waits for every member's stream, runs on a stream of its own and returns when everything has finished.  Calls on one model handle
 *   serialise on a mutex (two threads with disjoint contexts do not race); lnb_model_enable_batch must not run concurrently with a call.
 *   How it runs: passes of at most W = LNB_APPEND_MANY_COLS (default 128) columns; a member's rows may straddle two passes, the later one reads
 *   the KV rows the earlier one wrote.  A pass of up to 16 columns (17..32: two column groups) runs the column forms when lnb_model_enable_batch
 *   was called, rows of the streaming product otherwise and above 32.  A pass runs the long-context attention pair when one of its members has a
 *   capacity beyond the one-workgroup kernels' reach (~7800 positions at head_dim 128), else the one-workgroup kernels: same bits.
 *   Refused, each with a message, arguments before any handle is dereferenced and everything before any cache is written: NULL ctxs, tokens,
 *   n_rows, start_pos or entry of ctxs; n outside 1..128; an n_rows[s] < 1 or a negative start_pos[s]; a context that appears twice; a pass width
 *   outside 1..128; members of different lnb_model handles; a handle that is not the whole model; a member in LNB_MODE_FAST; a member with a
 *   pending lnb_forward_stage_begin; start_pos[s] + n_rows[s] beyond the member's KV cache or the RoPE table; a token id outside the vocabulary
 *   (checked on the host, the message carries the row index); dim, n_heads*head_dim or the FFN hidden size not a multiple of 128; long-context
 *   attention scratch that cannot be allocated (the message carries the size).
 * lnb_model_append_many_info: of the last call on that model handle, the number of passes, the widest pass and the passes that ran the
 *   long-context attention pair (any pointer may be NULL).
 * Which calls belong here and which to lnb_forward_append: profiles/append_many.md. */
int lnb_forward_append_many(lnb_ctx* const* ctxs, int n, const int32_t* tokens, const int32_t* n_rows, const int32_t* start_pos,
                            float* logits_out, int32_t* argmax_out);
int lnb_model_append_many_info(const lnb_model* m, int* passes, int* max_columns, int* long_passes);

/* ---- greedy loop on the device: the decode half of InferenceEngine.generateTokensInternal
 * (src/inference/inference.go:194-252).  Starting from `token` at position start_pos (its KV is computed by
 * the first step), runs n_steps one-token Forward+Argmax steps as replays of one captured hipGraph without
 * any host round trip; out_tokens[i] is the token generated by step i.  ms_out (optional) = device time of
 * the n_steps measured with HIP events on the library's stream. */
int lnb_decode_greedy(lnb_ctx* c, int32_t token, int start_pos, int n_steps, int32_t* out_tokens, float* ms_out);
/* (lnb_decode_greedy and lnb_batch_decode always produce n_steps tokens: stop ids of the context are NOT compared by them -- use the
 * _until forms, which report how far the run got.) */
/* Stop ids ON THE DEVICE (inference.go:233-252: generation ends with the first token that is one of model.StopTokenIds -- <|eot_id|>,
 * <|eom_id|> -- and that token is emitted).  lnb_ctx_set_stop_ids gives a context up to 8 of them (0: none); the token-feedback kernel then
 * freezes the generation (position, token word, token log) at the first match, so a run of any length can be enqueued without a host check
 * per token.  lnb_decode_greedy_until = lnb_decode_greedy that reports how far it got: *n_generated tokens are valid (max_steps unless a
 * stop id ended the run; the stop token is the last of them), *finished (optional) = 1 if one did.  Same tokens whatever the chunking. */
int lnb_ctx_set_stop_ids(lnb_ctx* c, const int32_t* ids, int n);
int lnb_decode_greedy_until(lnb_ctx* c, int32_t token, int start_pos, int max_steps, int32_t* out_tokens, int* n_generated, int* finished, float* ms_out);

/* ---- speculative greedy decoding with n-gram drafts: the same tokens, logits and KV rows as lnb_decode_greedy_until, fewer passes ----
 * Each PASS guesses the next tokens by n-gram lookup (prompt lookup: no second model) and verifies them all in ONE batched pass over the
 * weights whose w = draft_len + 1 columns alias this context: column i takes d_i (d_0 = the current token) at position pos + i with the
 * context's caches, so it is exactly the one-token step at pos + i, bit for bit (DESIGN.md "Speculative decoding").  The argmax of columns
 * 0 .. a is emitted, a = the longest prefix of columns whose argmax equals the next column's input, with the context's stop ids applied as
 * the greedy loop applies them.  A pass without a draft replays the context's one-token step.  The host reads one pinned word per pass.
 * Draft rule (ngram_draft_kernel; the running text R = history, token, the tokens generated so far; C = the corpus):
 *   for n = ngram_max down to ngram_min, the first n with a match wins; a match is an earlier occurrence of R's last n tokens that is
 *   followed by at least one token of its array (R's own final suffix is no match), searched in R before C, the latest start winning
 *   within an array; the draft is up to max_draft tokens after the match, cut at the end of that array, at max_steps - generated - 1
 *   and at seq_len - pos - 1.  No match: no draft.
 * lnb_ctx_set_draft: max_draft 0..LNB_MAX_DRAFT (0 = off, the default: lnb_decode_speculative_until is then lnb_decode_greedy_until);
 *   1 <= ngram_min <= ngram_max <= 16; the corpus (may be empty) is copied to the device.  Arguments are checked before the handle.
 * lnb_decode_speculative_until: outputs as lnb_decode_greedy_until from `token` at start_pos (history: the n_history tokens before it,
 *   e.g. the prompt); afterwards the cache rows [0, start_pos + *n_generated) hold that call's bits and lnb_decode_greedy / lnb_forward
 *   continue the context.  Requires a whole-model handle, the exact mode and dim, n_heads*head_dim, FFN hidden size multiples of 128 (any
 *   seq_len lnb_ctx_create accepts: a context beyond the one-workgroup attention's reach -- ~7.8 K positions at head_dim 128 -- verifies on
 *   the long-context kernels, lnb_ctx_set_batched_attention); refuses token probabilities, the tolerance mode and a
 *   member of a live batch.  With or without lnb_model_enable_batch (its column forms, or rows of the streaming product; same bits).
 *   stats (optional): passes, verify_passes (passes with a draft), drafted (draft tokens verified), accepted (draft tokens emitted:
 *   *n_generated - passes).  ms_out (optional): HIP-event time of the whole loop.
 * lnb_op_ngram_draft: the draft kernel on host arrays (a test aid): R = text, no decode limits; out[0 .. *n_out), out has max_draft entries. */
#define LNB_MAX_DRAFT 15
typedef struct lnb_spec_stats { int64_t passes, verify_passes, drafted, accepted; } lnb_spec_stats;
int lnb_ctx_set_draft(lnb_ctx* c, int max_draft, int ngram_min, int ngram_max, const int32_t* corpus, int n_corpus);
int lnb_decode_speculative_until(lnb_ctx* c, const int32_t* history, int n_history, int32_t token, int start_pos,
                                 int max_steps, int32_t* out_tokens, int* n_generated, int* finished,
                                 lnb_spec_stats* stats, float* ms_out);
int lnb_op_ngram_draft(int device, const int32_t* text, int n_text, const int32_t* corpus, int n_corpus,
                       int ngram_min, int ngram_max, int max_draft, int32_t* out, int* n_out);

/* ---- speculative greedy decoding of MANY contexts: every member drafts for itself, one pass over the weights verifies them all --------------
 * lnb_decode_speculative_until reads the weights once per pass of ONE context; lnb_batch_decode_until serves many contexts per pass, one column
 * each.  This call joins them: a pass of up to col_budget columns whose columns are consecutive rows of several members -- a pass of
 * lnb_forward_append_many, column i of a member the one-token step at pos + i, bit for bit -- with the n-gram draft, the packing and the commit
 * done per member on the device (DESIGN.md "Speculative decoding of many contexts").
 *   Contract: for every member s, out_tokens[s * max_steps .. + n_generated[s]), n_generated[s], finished[s] and the KV rows
 *   [0, start_pos[s] + n_generated[s]) of every layer are BIT-IDENTICAL to lnb_decode_greedy_until(ctxs[s], tokens[s], start_pos[s], max_steps, ...)
 *   run alone on a context holding the same rows below start_pos[s]; the member's stop ids are applied as that loop applies them.  Rows beyond
 *   that range may hold rejected drafts (as after lnb_decode_speculative_until).  start_pos[s] < 0: member s is skipped -- nothing of it is
 *   touched, n_generated[s] = 0, finished[s] = 1 (a member that finished in an earlier call of a chunked run, as in lnb_batch_decode_until).
 *   Nothing else of a member changes; its cached device position is invalidated; afterwards every entry point continues it.
 *   Drafts: each member's own lnb_ctx_set_draft settings (max_draft 0: it never drafts and takes one column per pass); its draft is exactly
 *   ngram_draft_kernel's for it -- R = history[s], tokens[s], its generated tokens; the same match rule and cuts.
 *   One pass: A = the members still running (not skipped, not finished, fewer than max_steps tokens), in member order; each gets one column for
 *   its current token; the budget - |A| columns left are granted level by level -- for j = 1..15, for s in A in order: if member s's draft has at
 *   least j tokens and a column is left, s gets one more.  Members occupy consecutive columns in member order at positions pos, pos + 1, ...
 *   After the pass a_s = the longest prefix of member s's columns whose argmax equals the next column's input; the argmax of its columns 0 .. a_s
 *   is emitted as the greedy loop emits (token log, position, token word; a stop token is emitted and freezes the member).  Finished members
 *   contribute no columns: passes narrow as a run drains.  The call returns when A is empty.  The host reads one pinned block per pass.
 *   col_budget: n..128, or 0 = the default 16 * ceil(n / 16) -- the products work in tiles of 16 columns (with n = 16 the default grants no drafts).
 *   stats[s] (the array may be NULL): passes = passes in which s had a column, verify_passes = those in which it had a granted draft, drafted =
 *   granted draft tokens, accepted = n_generated[s] - passes.  info (may be NULL): the passes of the call, those with any draft, the sum and the
 *   maximum of their widths, the passes that ran the long-context attention pair (a running member's capacity beyond the one-workgroup kernels'
 *   reach, as in lnb_forward_append_many).  ms_out (optional): HIP-event time of the whole loop.
 *   The call waits for every member's stream, runs on the stream of lnb_forward_append_many's pass object and under its mutex, and returns when
 *   everything has finished.
 *   Refused, each with a message, arguments before any handle is dereferenced and everything before any cache is written: a NULL array or entry
 *   (history[s] may be NULL when n_history[s] is 0; finished, stats, info, ms_out may be NULL); n outside 1..128; a context that appears twice; a
 *   negative n_history[s]; max_steps <= 0 or beyond a member's token log; col_budget outside {0, n..128}; members of different lnb_model handles;
 *   a handle that is not the whole model; a member in LNB_MODE_FAST, with token probabilities on, with a pending lnb_forward_stage_begin or in a
 *   live batch; a token outside the vocabulary; start_pos[s] + max_steps beyond the member's KV cache or the RoPE table; dim, n_heads*head_dim or
 *   the FFN hidden size not a multiple of 128; long-context attention scratch that cannot be allocated.
 * Which callers belong here, which to lnb_batch_decode_until and which to lnb_decode_speculative_until: profiles/spec_many.md. */
typedef struct lnb_spec_many_info { int64_t passes, verify_passes, columns, max_columns, long_passes; } lnb_spec_many_info;
int lnb_decode_speculative_many(lnb_ctx* const* ctxs, int n, const int32_t* const* history, const int32_t* n_history,
                                const int32_t* tokens, const int32_t* start_pos, int max_steps, int col_budget,
                                int32_t* out_tokens, int32_t* n_generated, int32_t* finished,
                                lnb_spec_stats* stats, lnb_spec_many_info* info, float* ms_out);

/* ---- token probabilities: how likely each generated (or given) token was, exactly as the reference's own Softmax gives it ----------
 * For one logits row x[0..V) (bf16 values widened to f32: what lnb_forward returns -- the reference's Forward, llamatransformer.go:170-177):
 *   Z       = sum_{j ascending} exp(f64(x_j)) in f64: ml.Softmax's serial rowExpSum (operations_impl.go:478-511);
 *   prob(j) = float32(exp(f64(x_j)) / Z): BIT-IDENTICAL to the oracle's orc_softmax_f32 of that row with its default exp (the host C
 *             library's; the device looks exp up in a 65536-entry table built on the host with it, once per model);
 *   top-k   = candidates are the values ml.Argmax can select (operations_impl.go:529-541: strict '<' from -MaxFloat32): not NaN and strictly
 *             greater than -MaxFloat32; value descending, lowest index first on ties.  Entry 0 is the ml.Argmax token -- the generated one.
 *             Fewer than k candidates: the missing entries have id -1, logit NaN, prob NaN;
 *   log_z   = ln Z in f64 from a sum in any order: |log_z - ln Z| <= (V + 8) 2^-52 (about 3e-11 at V = 128256).  logit - log_z is a
 *             log-probability that stays usable where prob underflows f32.
 * Non-finite rows give what orc_softmax_f32 gives: an x above 709.78 makes Z = +inf (other entries 0, the overflowing one NaN); a NaN
 * anywhere makes Z and every prob NaN; top-k ids follow the candidate rule.  In the tolerance mode (lnb_ctx_set_mode) the same kernel runs
 * on that mode's logits; bit-identity to the oracle is claimed for the exact mode only.  None of this changes which token is generated.
 *
 * lnb_ctx_set_token_probs: top_k 0..LNB_MAX_TOP_K (0, the default: nothing is recorded and the captured decode step is the plain one).
 *   Whole-model contexts only; drops the context's captured decode graphs; refused while the context belongs to a live batch.  Every step
 *   of lnb_decode_greedy[_until] / lnb_batch_decode[_until] then records its token's row: a device log of seq_len x top_k records beside the
 *   token log (a batch needs all members at one top_k).  Pipeline ticks refuse such contexts.
 * lnb_ctx_read_token_probs: records [first, first + n) of the last lnb_decode_greedy[_until] or lnb_batch_decode[_until] call that ran the
 *   context (for a batch: read each member context).  ids / logits / probs: [n * k], log_z: [n], k = the top_k that call ran with;
 *   ids[i * k] == out_tokens[i].  Fails if that call ran with top_k 0 or first + n exceeds the tokens it generated (n_generated of _until).
 * lnb_ctx_token_prob_walks: rows (decode steps, scored rows) of this context that walked the serial sum (the certified estimate of Z could
 *   not settle one of their reported probabilities; DESIGN.md "Token probabilities").
 * lnb_forward_score: lnb_forward (same work, errors and KV effects, the same argmax_last_out) with the head on every row; instead of the
 *   logits, for each row i with 0 <= targets[i] < V: target_logit[i], target_prob[i] = prob(targets[i]) of row i, and log_z[i].  A row with
 *   targets[i] < 0 reports NaN logit and prob (log_z is still reported); targets[i] >= V is an error.  Scoring a text: targets = tokens[1:]
 *   followed by the next token or -1.
 * lnb_op_token_probs: the same kernel on host rows [rows][V] (a test aid, as lnb_op_argmax): ids / logits / probs [rows * top_k] (may be
 *   NULL when top_k is 0), log_z [rows]; targets (optional) -> target_prob [rows]; force_serial: every row walks the serial sum (the fallback
 *   gives the same bits); *serial_walks (optional) = rows that walked. */
#define LNB_MAX_TOP_K 16
int lnb_ctx_set_token_probs(lnb_ctx* c, int top_k);
int lnb_ctx_read_token_probs(lnb_ctx* c, int first, int n, int32_t* ids, float* logits, float* probs, double* log_z);
int lnb_ctx_token_prob_walks(lnb_ctx* c, int* out);
int lnb_forward_score(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, const int32_t* targets,
                      float* target_logit, float* target_prob, double* log_z, int32_t* argmax_last_out);
int lnb_op_token_probs(int device, const uint16_t* logits_bf16, int rows, int V, int top_k, const int32_t* targets,
                       int force_serial, int32_t* ids, float* logits, float* probs, float* target_prob, double* log_z, int* serial_walks);

/* ---- batched exact decode: several generations per pass over the weights ----------------------------------
 * The reference runs one generation per InferenceContext (src/inference/inference.go:174) and shares the weight matrix across the rows of a
 * call (src/ml/operations_lineartransform.go:173-193).  A batch groups 1..128 contexts of ONE whole-model handle; per step, every
 * sequence's one-token Forward + Argmax (inference.go:194-252) is evaluated in a single pass over the weights: up to 16 sequences are the 16
 * columns of the f32 matrix-core instruction, which computes each column's k-ordered chain exactly; 17..128 sequences are the rows of the
 * prefill's streaming product (1 / 2 / 4 tiles of 16 sequences per wave, same instruction, same chains) -- except that 17..32 sequences keep
 * the column form, as two groups of 16, for the matrices with few output rows (wq|wk|wv, wo, w2).  Per-sequence position, RoPE row, KV
 * append and attention; every sequence's tokens, logits and caches are bit-identical to its single-sequence run (and the CPU reference).
 * lnb_model_enable_batch: builds the weights' second, matrix-core friendly copy on the device (once, after lnb_model_finalize; it costs the
 *   model's matrix bytes again -- 15 GB for the 8B shape; fails cleanly when that does not fit, the other entry points stay usable).  Works
 *   on a whole model and on a pipeline stage of whole blocks.  Since round 5 it is a pure PERFORMANCE option: prompts (lnb_forward with 16 or
 *   more rows) stream the resident weight layouts, and lnb_batch_create on a model without the copy runs every product of the batch as rows of
 *   that streaming kernel, whatever the number of sequences (64..128 sequences: 3-8 % slower than with the copy; up to 32 the column forms,
 *   which read the copy, are the faster ones by more).  Same bits either way.
 * lnb_batch_create: the contexts keep their own KV caches and positions (prefill each with lnb_forward first); any seq_len lnb_ctx_create accepts,
 *   the members' may differ (a batch with a member beyond the one-workgroup attention's reach, ~7.8 K positions at head_dim 128, runs the
 *   long-context attention: lnb_batch_set_attention).  A context must not be used by another call while a batch call that contains it runs.
 * lnb_batch_decode: sequence s continues from tokens[s] at position start_pos[s] (different positions are fine); n_steps greedy steps for
 *   all of them as replays of one captured hipGraph; out_tokens[s * n_steps + i] = token i of sequence s.  Afterwards every context's
 *   cache holds its new rows: lnb_forward / lnb_decode_greedy / another batch may continue it.
 * Lifetime: a batch holds its member contexts' device pointers (tables, captured graphs): lnb_ctx_destroy on a member FAILS while the
 * batch is alive -- destroy the batch first (the Go binding's Close does it in that order). */
typedef struct lnb_batch lnb_batch;
int lnb_model_enable_batch(lnb_model* m);
int64_t lnb_model_batch_bytes(lnb_model* m);
/* One-token decode streams the gate|up matrices from a lossless 13-bit planar copy (csrc/lnb_wpack.h: low byte raw, a 4-bit exponent code in a per-matrix
 * window of 30 binades, the sign), built on the device by lnb_model_finalize unless LNB_W13_PACKED=0.  Every weight decodes to its own 16 bits, so every
 * product and every chain is what the raw kernel computes.  The raw layouts stay resident: prefill, batches, appends, the throughput schedule and the
 * tolerance mode read them.  A matrix that cannot be packed -- it holds a subnormal or an exponent of 1, an Inf / NaN, or non-zero weights more than 30
 * binades apart -- or whose copy cannot be allocated keeps the raw kernel, and says so here:
 *   lnb_model_wpack_bytes   device bytes of the copies (13/16 of the matrices they cover)
 *   lnb_model_wpack_info    counts6[0] = matrices decoding from their copy; [1] refused for a subnormal / exponent 1, [2] Inf / NaN, [3] out of window,
 *                           [4] no memory; [5] never tried (knob off at finalize, or not the 56-row layout the packed kernel reads)
 * Bind every tensor before lnb_model_finalize: a gate|up tensor bound afterwards is re-packed in place if it fits the copy's window, else the call fails. */
int64_t lnb_model_wpack_bytes(lnb_model* m);
int lnb_model_wpack_info(lnb_model* m, int32_t* counts6);
/* The LM head has a copy of the same format (unless LNB_HEAD_PACKED=0), cut into 128-row blocks that the one-token head walks as two chains per lane.  It is
 * built when the head's resident layout is the 64-row one, a row fits the kernel's 128-step stages (dim 8192 does not) and the vocabulary gives every CU a
 * 128-row block.  The two queries above count gate|up matrices only; the head reports here:
 *   lnb_model_wpack_head_bytes    device bytes of the head's copy (13/16 of the matrix for whole blocks and stages; 0: none)
 *   lnb_model_wpack_head_status   0 the one-token head streams its copy; 1 subnormal / exponent 1, 2 Inf / NaN, 3 out of window, 4 no memory; 5 never tried
 *                                 (knob off at finalize, a stage without output.weight, a shape without a packed form); -1 null argument
 * output.weight bound after lnb_model_finalize is re-packed in place if it fits the copy's window, else the call fails and the head streams the raw weights. */
int64_t lnb_model_wpack_head_bytes(lnb_model* m);
int lnb_model_wpack_head_status(lnb_model* m);
int lnb_batch_create(lnb_ctx* const* ctxs, int n, lnb_batch** out);
int lnb_batch_destroy(lnb_batch* b);
int lnb_batch_decode(lnb_batch* b, const int32_t* tokens, const int32_t* start_pos, int n_steps, int32_t* out_tokens, float* ms_out);
/* ... with per-sequence stop ids (lnb_ctx_set_stop_ids on the member contexts, above): n_generated[s] tokens of row s are valid, the last one
 * the stop token if the sequence finished; finished[s] (optional, may be NULL) = 1 if a stop id ended sequence s -- n_generated[s] == max_steps
 * alone cannot tell.  A finished sequence's position and caches stay where they stopped.  Decoding in chunks: pass start_pos[s] < 0 for a
 * sequence that has finished -- it stays frozen (n_generated[s] = 0, finished[s] = 1) instead of restarting from its stop token; its
 * tokens[s] is ignored.  (Stop ids are a single-GPU feature of the batch: lnb_batch_set_state on a stage of a multi-stage pipeline refuses
 * contexts that carry any -- only the last stage would see the token.) */
int lnb_batch_decode_until(lnb_batch* b, const int32_t* tokens, const int32_t* start_pos, int max_steps, int32_t* out_tokens, int32_t* n_generated, int32_t* finished, float* ms_out);
/* measurement aid: average HIP-event time of one kernel class of the batched step (which as lnb_profile_kernel; a norm launch counts
 * with the product it feeds), every sequence placed at `pos`; overwrites the caches' row `pos` */
int lnb_batch_profile_kernel(lnb_batch* b, int which, int pos, int iters, float* avg_ms_out);

/* ---- seeded temperature / top-k / top-p sampling in the device loops ----------------------------------------
 * The reference generates with ml.Argmax alone (inference.go:207-226).  A sampler {temperature, top_k, top_p, seed} replaces that argmax in the
 * device-resident loop and in the batched loop; the sampled token is a pure function of the step's bf16 logits row x[0..V), the sampler and
 * the position pos of the step's input token (csrc/lnb_sample.h holds the definition in plain C++; tests/sampler_ref.py restates it):
 *   1. y_j = trunc_bf16(f32(x_j) / temperature) -- ml.DivToScalar (operations_impl.go:273-289); temperature 1 leaves the row as it is
 *   2. candidates are ml.Argmax's: y_j not NaN and > -MaxFloat32.  No candidate: token -1, which the loops treat as an all-NaN row
 *   3. e_j = exp(f64(y_j)) of the host C library (the 65536-entry table of the token probabilities); a = ml.Argmax(y), e_max = e_a; a
 *      DEGENERATE row -- e_max +inf or below 2^-1022 -- gives token a
 *   4. w_j = floor(e_j * 2^(45 - E)) as unsigned 64-bit integers, E = floor(log2(e_max)); S = {j: w_j >= 1}.  V <= 131072 keeps every sum below 2^63
 *   5. S is ordered by y descending, the lowest index first among equal values (the order of the token-probability top-k)
 *   6. top_k > 0 keeps the first min(top_k, |S|) entries, top_k == 0 all of S; W1 = their weight sum
 *   7. top_p < 1 keeps the shortest prefix of those whose weight sum is >= P = uint64(floor(f64(top_p) * f64(W1))), at least one; top_p == 1 is off
 *   8. W_K = the kept weight sum, u = splitmix64(splitmix64(seed) ^ (uint64(pos) * 0x9E3779B97F4A7C15)), r = (u * W_K) >> 64 (128-bit product);
 *      the token is the first kept index, walking the kept set in INDEX order, at which the running weight sum exceeds r
 * Everything behind the table lookup is integer arithmetic -- associative -- so the parallel kernel, the serial walk and the Python restatement
 * agree bit for bit: no tolerance, no statistics.  temperature == 0 means greedy: the token is ml.Argmax(x), the other fields are ignored.
 * The draw depends on (seed, pos) only: a run gives the same tokens whatever its chunking, a batch member the tokens of its own single-context
 * run; two members with the same seed, positions and logits draw alike (seeds are the caller's business).
 * The sampler is an ARGUMENT of the call, not context state: the greedy, speculative, append and pipeline entry points know nothing of it.
 * The FIRST token of a generation is the prompt's: lnb_forward reports its argmax only.  A caller that wants it sampled too takes the prompt's last
 *   logits row (lnb_forward / lnb_forward_append with logits) through lnb_op_sample at the position of the last prompt token, as the Python
 *   InferenceEngine(..., sampler=) does; the loops below sample every token after it.
 * lnb_decode_sample_until: lnb_decode_greedy_until with step 8's token in place of the argmax -- same arguments, stop ids, finished flag,
 *   token log, error latch and n_generated.  The sampling step has captured graphs of its own (the greedy ones are neither dropped nor
 *   recaptured); the graph holds a pointer to the sampler, so another sampler replays the same graph.
 * lnb_batch_decode_sample_until: lnb_batch_decode_until with one sampler per member (samplers[n]); a temperature-0 member is greedy;
 *   start_pos[s] < 0 freezes a finished member.
 * lnb_op_sample: the kernel on host rows [rows][V] (a test aid, as lnb_op_token_probs).  draws (optional): u of step 8 given per row instead
 *   of derived from (seed, pos).  info (optional), per row: w_all = the weight sum over S, n_candidates = |S|, w_topk = W1, w_kept = W_K,
 *   n_kept, degenerate (a degenerate, greedy or candidate-less row reports zeros elsewhere).
 * Refused, each with a message, before any handle is dereferenced or any device touched: NULL pointers; temperature negative, NaN or infinite;
 *   top_k < 0; top_p NaN, <= 0 or > 1; reserved != 0; V > 131072 or V < 1.  (lnb_batch_decode_sample_until: the NULL checks come before the
 *   handle is used; how many samplers there are is the batch's own n, so they are checked right after it is read and before anything else.)  Then: a stage handle that is not the whole model; a context or a
 *   member that records token probabilities (the record promises ids[i * k] == out_tokens[i], which a sampled token does not keep: switch it
 *   off with lnb_ctx_set_token_probs(ctx, 0)); a pending lnb_forward_stage_begin; max_steps beyond the token log, the KV cache or the RoPE table.
 * Sampling in the speculative loops (lnb_decode_speculative_sample_until / _many, below) needs NO rejection sampling: the draw is u(seed, pos), so the
 *   token lnb_decode_sample_until emits at position p is sample(row_p, sampler, p) and depends on nothing else; column i of a verify pass has
 *   row_{pos + i} exactly, so the greedy acceptance rule holds with "the sampler's token of column i at position pos + i" in place of the argmax.
 *   No distribution is compared and there is no tolerance: the output is the sampling loop's token sequence, the same bits, in fewer passes.
 * Out of scope: rejection sampling against a draft MODEL, pipeline ticks, recording the sampled token's probability, min-p, repetition penalties,
 *   logit bias. */
#define LNB_SAMPLE_MAX_VOCAB 131072
typedef struct lnb_sampler { float temperature; float top_p; int32_t top_k; int32_t reserved; uint64_t seed; } lnb_sampler;
typedef struct lnb_sample_info { uint64_t w_all, w_topk, w_kept; int32_t n_candidates, n_kept, degenerate, pad; } lnb_sample_info;
int lnb_decode_sample_until(lnb_ctx* c, const lnb_sampler* sampler, int32_t token, int start_pos, int max_steps,
                            int32_t* out_tokens, int* n_generated, int* finished, float* ms_out);
int lnb_batch_decode_sample_until(lnb_batch* b, const lnb_sampler* samplers, const int32_t* tokens, const int32_t* start_pos, int max_steps,
                                  int32_t* out_tokens, int32_t* n_generated, int32_t* finished, float* ms_out);
int lnb_op_sample(int device, const uint16_t* logits_bf16, int rows, int V, const lnb_sampler* samplers, const int32_t* pos,
                  const uint64_t* draws, int32_t* tokens_out, lnb_sample_info* info);
/* ---- sampling in the speculative loops ----
 * lnb_decode_speculative_sample_until: out_tokens[0 .. *n_generated), *n_generated, *finished and the KV rows [0, start_pos + *n_generated) of every
 *   layer are bit-identical to lnb_decode_sample_until(c, sampler, token, start_pos, max_steps, ...) on a context holding the same rows below
 *   start_pos; stop ids apply as there.  The result does not depend on the draft settings or on chunking.  Rows beyond that range may hold rejected
 *   drafts, as after the greedy form.  Draft rule, draft cuts and stats are lnb_decode_speculative_until's (accepted = *n_generated - passes);
 *   temperature 0 gives that call's tokens and stats; max_draft 0 (lnb_ctx_set_draft) runs lnb_decode_sample_until itself.  A verify pass samples
 *   every column in ONE launch (column i at position pos + i; the last workgroup to arrive accepts and emits); it has captured graphs of its own per
 *   (width, attention form) beside the greedy ones, which a sampling call neither drops nor recaptures (and vice versa), and which hold a pointer
 *   to the sampler: another sampler replays them.  A pass without a draft replays the context's sampling one-token graph.
 * lnb_decode_speculative_sample_many: the contract of lnb_decode_speculative_many with lnb_decode_sample_until(ctxs[s], &samplers[s], ...) as member
 *   s's reference; grant rule, col_budget, the start_pos[s] < 0 skip, stats and info are unchanged; a temperature-0 member is greedy.
 * lnb_op_spec_sample_accept (a test aid, as lnb_op_sample / lnb_op_ngram_draft): the accept-and-emit rule on host rows -- column i of a pass of w
 *   columns has logits row i, took col_tokens[i] (col_tokens[0] = the current token) and sits at pos0 + i -> the tokens the pass emits.
 * Refused, each with a message, argument checks before any handle is dereferenced and everything before any cache is written: whatever the greedy
 *   speculative form refuses and whatever lnb_decode_sample_until refuses (a NULL sampler; temperature negative, NaN or infinite; top_k < 0; top_p
 *   NaN, <= 0 or > 1; reserved != 0; V > LNB_SAMPLE_MAX_VOCAB; a context that records token probabilities).  The many form checks its samplers right
 *   after n is known to be valid. */
int lnb_decode_speculative_sample_until(lnb_ctx* c, const lnb_sampler* sampler, const int32_t* history, int n_history, int32_t token, int start_pos,
                                        int max_steps, int32_t* out_tokens, int* n_generated, int* finished, lnb_spec_stats* stats, float* ms_out);
int lnb_decode_speculative_sample_many(lnb_ctx* const* ctxs, int n, const lnb_sampler* samplers /* [n] */, const int32_t* const* history,
                                       const int32_t* n_history, const int32_t* tokens, const int32_t* start_pos, int max_steps, int col_budget,
                                       int32_t* out_tokens, int32_t* n_generated, int32_t* finished, lnb_spec_stats* stats, lnb_spec_many_info* info,
                                       float* ms_out);
int lnb_op_spec_sample_accept(int device, const uint16_t* logits_bf16 /* [w][V] */, int w, int V, const lnb_sampler* sampler, int pos0,
                              const int32_t* col_tokens /* [w] */, const int32_t* stop_ids, int n_stop, int32_t* emitted /* [w] */, int* n_emitted,
                              int* finished);
/* measurement aid: average HIP-event time of a decode step's token launch alone -- sample_kernel with this sampler, or argmax_kernel (sampler
 * NULL) -- on the logits row the context's last step left; the launches advance the context's device state from `pos` as steps do.  Whole-model
 * contexts with no lnb_forward_stage_begin pending; a bad sampler is refused as above. */
int lnb_profile_sample(lnb_ctx* c, const lnb_sampler* sampler, int pos, int iters, float* avg_ms_out);
/* Attention form of a batch's steps (same bits either way): the one-workgroup-per-head kernels, or the long-context pair with the sequences as a
 * grid dimension (its scratch -- n * n_heads * max seq_len * 8 bytes -- is allocated when a call first needs it; a call that cannot get it fails).
 * The form is chosen per call (lnb_batch_decode[_until], lnb_batch_set_state for the ticks that follow, lnb_batch_profile_kernel): long when the
 * largest start position + 1 exceeds long_threshold.  long_threshold < 0: keep; default: never, except that a batch with a member
 * whose seq_len exceeds the short kernels' reach always runs the long form.  force_zseq bit 0: every (sequence, head) walks the serial sum
 * (counted in lnb_ctx_zseq_count of the batch's first context).  Arguments are checked before the handle; refused while a
 * lnb_forward_stage_begin of a member has not been ended. */
int lnb_batch_set_attention(lnb_batch* b, int long_threshold, int force_zseq);
/* the same for the verify passes of lnb_decode_speculative_until on this context (chosen per pass; one scratch for all widths) */
int lnb_ctx_set_batched_attention(lnb_ctx* c, int long_threshold, int force_zseq);
/* 0: the last batched call / verify pass ran the one-workgroup kernels, 1: the long-context pair (a test and a bench print it);
 * lnb_ctx_verify_attention_form also 2: the multi-row long-context pair (lnb_ctx_set_rows_attention, flags bit 1) */
int lnb_batch_attention_form(const lnb_batch* b, int* out);
int lnb_ctx_verify_attention_form(const lnb_ctx* c, int* out);

/* ---- pipeline-stage form (layer-sharded multi-GPU) -------------------------------
 * hidden state buffers live on the device and are owned by the ctx: [seq_len, dim] bf16.
 * which: 0 = stage input, 1 = stage output, 2 = the [seq_len, ffn_hidden] gate*up activations, part of the hand-off when the
 * stage boundary lies between a block's gate/up and down parts.  RCCL send/recv (done by the host layer) targets these pointers. */
void* lnb_ctx_hidden_ptr(lnb_ctx* c, int which);
/* A test aid: the attention launch of `layer` on the caller's query rows.  Copies q_bf16 [seq][n_heads][head_dim] into the context's query buffer, sets the
 * device position and enqueues what a Forward of `seq` rows at start_pos enqueues for the attention of that block (the same function: the context's mode,
 * the one-row / row-per-workgroup / matrix-core / long-context dispatch and the non-finite rescan apply), then copies the [seq][n_heads][head_dim] result to
 * out_bf16.  The K / V rows [0, start_pos + seq) are what the context holds (lnb_ctx_load_prefix).  A Forward's checks apply (the reference's broadcast rule:
 * seq divides start_pos + seq); only a call that reaches the tolerance mode's flash kernel, whose mask is defined at any length, may break that rule. */
int lnb_ctx_attention(lnb_ctx* c, int layer, const uint16_t* q_bf16, int seq, int start_pos, uint16_t* out_bf16);
/* Runs this stage's layers.  tokens != NULL only on the first stage (embedding gather); otherwise the input
 * hidden state must already be in hidden_ptr(0).  On the last stage logits_out/argmax_last_out behave as in
 * lnb_forward; on other stages they must be NULL and the result is left in hidden_ptr(1). */
int lnb_forward_stage(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, float* logits_out, int32_t* argmax_last_out);
/* The same in two halves, for a pipeline rank that exchanges hidden states with its neighbours WHILE the stage computes: _begin
 * enqueues the stage on the ctx's stream and returns (want_argmax: last stage only, norm + output + argmax of the last row, as
 * inference.go:207-211 needs); _end blocks until it has finished and returns the token.  One begin per end. */
int lnb_forward_stage_begin(lnb_ctx* c, const int32_t* tokens, int seq, int start_pos, int want_argmax);
int lnb_forward_stage_end(lnb_ctx* c, int32_t* argmax_last_out);
/* block the calling thread until everything enqueued for this ctx has finished */
int lnb_ctx_synchronize(lnb_ctx* c);
/* raw HIP stream (hipStream_t) the ctx enqueues on, for event timing by the caller */
void* lnb_ctx_stream(lnb_ctx* c);

/* ---- the pipeline's exchange behind the boundary (RCCL point-to-point over xGMI; librccl.so.1 is loaded on first use) -----------
 * The reference runs its blocks in one loop (llamatransformer.go:156-164); here rank r of `world` holds the stage created with
 * lnb_model_create_parts and one lnb_ctx per sequence in flight.  A host layer in any language only needs a way to hand rank 0's
 * 128-byte id to the other ranks (a file, a socket, MPI, torch.distributed ...).
 * lnb_pipeline_tick ENQUEUES and returns (no stream is synchronised):
 *   run   != NULL: the stage step of that sequence -- run_rows rows at position run_pos; run_tokens: host token ids (rank 0, prompt rows)
 *                  or NULL (other ranks: the input is the received hidden state; rank 0, one-token steps: the token received from the
 *                  last rank, already on the device).  One-token steps replay a captured hipGraph.  On the last rank the argmax token is
 *                  appended to a pinned log; *token_slot_out = its slot (lnb_pipeline_read_tokens).
 *   send  != NULL: ncclSend of that context's result to rank+1 (hidden state [send_rows, dim], plus the [send_rows, ffn_hidden]
 *                  activations when the stage ends between a block's gate/up and down parts); on the LAST rank: the 4-byte token to rank 0.
 *   recv  != NULL: ncclRecv from rank-1 into that context's input buffers; on rank 0: the token from the last rank.
 * send and recv go into ONE ncclGroupStart/End on the pipe's exchange stream, ordered against the compute streams by events; the
 * schedule (which sequence runs / is sent / is received in which tick) belongs to the host layer -- every rank must post matching
 * sends and receives in the same tick order (llama-nuts-and-bolts_amd/pipeline.py: run_ticks_native). */
typedef struct lnb_pipe lnb_pipe;
int lnb_pipeline_unique_id(void* id128);                       /* rank 0: ncclGetUniqueId */
int lnb_pipeline_init(lnb_model* stage, int rank, int world, const void* id128, lnb_pipe** out);   /* world == 1: no communicator, the token ring is a device copy */
/* the same pipe with an IN-PROCESS transport instead of RCCL: every stage lives in this process (pipes that name the same `group`), a send
 * meets its receive in a mailbox and becomes a device-to-device copy.  Same ticks, events and graphs; for single-process hosts and for
 * testing a schedule where RCCL cannot run (it wants one GPU per rank).  All stages of a group must live on ONE device and be ticked from
 * ONE host thread in lock-step order (a stage on another device is refused; running a sequence whose input has been requested but not
 * yet posted by its sender is an error, not a read of stale data) */
int lnb_pipeline_init_loopback(lnb_model* stage, int rank, int world, const char* group, lnb_pipe** out);
/* the same pipe WITHOUT a transport, for a host layer that moves what crosses the stage boundary itself (pipeline.py's torch.distributed
 * fallback when RCCL cannot form its communicator: staging tensors + batch_isend_irecv between lnb_pipeline_sync calls): ticks take `run`
 * only (send / recv are refused), everything else -- captured stage steps, positions advancing on the device, the first stage reading the
 * ring's token words, the last stage's token log -- as above.  The buffers to move: lnb_ctx_hidden_ptr (a sequence), lnb_batch_boundary_ptr
 * (a batch).  lnb_pipeline_comm_count reports 0. */
int lnb_pipeline_init_host(lnb_model* stage, int rank, int world, lnb_pipe** out);
int lnb_pipeline_destroy(lnb_pipe* p);
int lnb_pipeline_tick(lnb_pipe* p, lnb_ctx* run, int run_rows, int run_pos, const int32_t* run_tokens,
                      lnb_ctx* send, int send_rows, lnb_ctx* recv, int recv_rows, int* token_slot_out);
/* The same with a BATCH of sequences as the unit that moves through the stages (lnb_batch over this rank's stage model and its contexts of
 * those sequences; lnb_model_enable_batch works on stages of whole blocks).  Prefill each sequence with single-sequence ticks, call
 * lnb_batch_set_state on every rank (tokens: rank 0 only, or NULL to keep what the prefill's token ring left in the contexts), then per step:
 * run = ONE pass over the stage's weights for all the batch's sequences (captured graph; positions advance on the device; on the last rank
 * the n tokens go to the pinned log, *token_slot_out = the first of n consecutive slots), send = hidden states [n, dim] to rank + 1 (last
 * rank: the n token words to rank 0), recv = the mirror image.  Same grouping, events and transports as lnb_pipeline_tick. */
int lnb_batch_set_state(lnb_batch* b, const int32_t* tokens, const int32_t* start_pos);
/* pipeline ticks only enqueue: a token id outside the vocabulary (its embedding row is not gathered) or an all-NaN logits row (argmax -1,
 * operations_impl.go:529-541) is latched in a device word instead of failing a call.  lnb_batch_check_error waits for the batch's stream,
 * returns an error if the word was set since the last check (or the last lnb_batch_set_state) and clears it.  Call it after
 * lnb_pipeline_sync, before trusting lnb_pipeline_read_tokens.  (lnb_batch_decode checks for itself.) */
int lnb_batch_check_error(lnb_batch* b);
/* device pointers of what a batched tick exchanges (owned by the batch).  which: 0 = the hidden states [n, dim] bf16 -- the stage's input
 * before `run`, its output after; 1 = the n int32 token words the last stage's argmax leaves and the first stage of a multi-stage pipe reads */
void* lnb_batch_boundary_ptr(lnb_batch* b, int which);
int lnb_pipeline_tick_batch(lnb_pipe* p, lnb_batch* run, lnb_batch* send, lnb_batch* recv, int* token_slot_out);
int lnb_pipeline_sync(lnb_pipe* p);
/* the number of ranks the exchange spans as the TRANSPORT reports it (ncclCommCount of the communicator; pipes joined to an in-process
 * group; 1 for a one-stage pipe): lets a host check that N processes really formed ONE N-rank communicator */
int lnb_pipeline_comm_count(lnb_pipe* p, int* out);
/* tokens by log slot (token_slot_out of the tick that produced them); synchronises the device.  The log is a ring of the newest 65536
 * tokens: slots count up for the life of the pipe, reading never has to "drain" anything, a slot older than that is refused */
int lnb_pipeline_read_tokens(lnb_pipe* p, int first_slot, int n, int32_t* out);
/* diagnostic: the same grouped ncclSend + ncclRecv as a tick, on a one-rank communicator (to itself), n_bytes device to device and
 * compared -- checks the RCCL binding on a box with a single GPU, where a multi-rank communicator cannot be formed */
int lnb_pipeline_selftest(int device, int n_bytes);

/* ---- measurement aid (bench.py roofline leg): average HIP-event time of ONE kernel class of the decode step.
 * which: 0 attn_norm+QKV+RoPE GEMV, 1 attention, 2 wo GEMV, 3 ffn_norm+w1|w3 GEMV, 4 w2 GEMV, 5 norm+output GEMV,
 * 6 the five kernels of a whole block.  Consecutive launches cycle through this stage's layers so every launch
 * streams its weights from HBM instead of the 256 MiB Infinity Cache.  The KV cache content at `pos` is overwritten. */
int lnb_profile_kernel(lnb_ctx* c, int which, int pos, int iters, float* avg_ms_out);
/* ... and of the gate|up (w1|w3) and down (w2) kernels of a block launched on TWO streams, w2 `w2_delay_us` behind w1|w3: the time a
 * w1|w3 -> w2 streaming stage (llamatransformer.go:593-624) would have to beat, measured without building it (w2 reads stale activations:
 * only the time means anything; w2_delay_us < 0: w2 first, w1|w3 that long behind it).  w2_lds_pad: extra dynamic LDS for the w2 launch (forces one workgroup of each kernel per CU). */
int lnb_profile_ffn_pair(lnb_ctx* c, int pos, int iters, int w2_delay_us, int w2_lds_pad, float* avg_ms_out);
/* ... and the in-kernel cycle stamps of ONE launch of a GEMV class (which 0, 2, 3, 4 or 5): out[8 waves][16] doubles, per wave = {workgroups
 * that reported, avg total shader cycles, max total, avg barrier wait, avg "x staged / prologue end", avg "norm fold or walk" (wo / w2 chain
 * waves: chain start), avg phase stamps 0..6, stamp 7 = the same launch on the constant-rate wall clock}; *wall_clock_khz = that clock's rate
 * (hipDeviceAttributeWallClockRate).  bench.py turns them into the measured prologue / per-step / boundary terms of roofline.measured_model. */
int lnb_profile_kernel_stamps(lnb_ctx* c, int which, int pos, double* out, int* wall_clock_khz);

/* ---- single-op entry points (the src/ml operators on the hot path), used by the parity tests --------
 * y[rows,n] = trunc(sum_k x[rows,k]*w[n,k])  == ml.LinearTransformation (operations_impl.go:427-447);
 * host buffers in the reference layout; rw in {0(auto),16,32,64} selects the tiling */
int lnb_op_linear(int device, const uint16_t* x, const uint16_t* w, uint16_t* y, int rows, int n_out, int k_in, int rw);
/* RMSNorm.Forward (llamatransformer.go:633-639) followed by a linear layer, as the fused kernel computes it */
int lnb_op_rmsnorm_linear(int device, const uint16_t* x, const uint16_t* norm_w, float eps, const uint16_t* w,
                          uint16_t* y, int rows, int n_out, int k_in, int rw);
/* the fused ffn_norm + w1|w3 + SiLU(gate)*up launch of a one-token step on one row x[k_in] -> y[n_out] (llamatransformer.go:601-617), 56-row layout.
 * packed 0: the raw kernel; 1: from the 13-bit copy when the w1|w3 matrix is packable.  *status (may be NULL): 0 packable, 1 subnormal / exponent 1,
 * 2 Inf / NaN, 3 out of window -- a refused matrix runs the raw kernel */
int lnb_op_rmsnorm_gate_up(int device, const uint16_t* x, const uint16_t* norm_w, float eps, const uint16_t* w1, const uint16_t* w3, uint16_t* y,
                           int n_out, int k_in, int packed, int* status);
/* the fused final norm + output projection launch of a one-token step on one row x[k_in] -> y[n_out] (llamatransformer.go:166-170), w = [n_out][k_in].
 * packed 0: the raw 64-row kernel; 1: from the 13-bit copy in 128-row blocks when the matrix is packable.  n_wg > 0 caps the workgroups, so that a small
 * matrix still walks several blocks per workgroup (0: no cap).  *status as above */
int lnb_op_rmsnorm_head(int device, const uint16_t* x, const uint16_t* norm_w, float eps, const uint16_t* w, uint16_t* y,
                        int n_out, int k_in, int packed, int n_wg, int* status);
/* What the RMSNorm of a kernel form computed, per row of x[rows][k_in] (Mean of llamatransformer.go:641-660, operations_impl.go:236-251): the raw f32 bits of
 * the serial sum of squares as the kernel holds it in front of the division by k_in, the raw bits of r = f32(1 / sqrt(f64(sum / k_in + eps))), and the
 * walker's path word.  form picks the launch function and the kernel: the production template arguments in an instantiation of their own that has the
 * report compiled in (the production instantiations carry none of it).  A fused form runs with a zero weight matrix of one row block (the packed forms: its
 * 13-bit copy) and its product is discarded; the fused forms take up to 15 rows per launch (the packed ones a single row), more rows are looped over here.
 * Path word (csrc/lnb_seqsum.h, RMS_PATH_*): no bit of 0x70000000 set -- the branch-free item list was walked to its end: items << 16 | split leaves << 8 |
 * single-term items (a split leaf is two items; it is counted by its second one, the only kind that carries both a term and a binade).  Otherwise the row
 * took the record walk: 0x10000000 a folding wave flagged its segment (0x80000 its items do not fit the 128-entry segment, 0x40000 a leaf no item
 * covers: a non-finite tree sum, 0x20000 a failed scan composition), 0x20000000 more than 64 items, 0x40000000 an item's check failed; bits 20..27 the
 * flagging waves, bits 8..15 the item total & 0xFF, bits 0..7 the leaves replayed by the record walk (at most 255).
 * LNB_NORM_ROWS_WAVE has no item list: its path word is -1.
 * Returns 0; 1 when the form's launch function refuses k_in (nothing is written); -1 on an error. */
enum { LNB_NORM_CHAIN16 = 0, LNB_NORM_CHAIN32 = 1, LNB_NORM_CHAIN64 = 2,      /* gemv_chain_kernel<16 / 32 / 64, 1, ...>: 2 / 6 / 6 folding waves */
       LNB_NORM_QUAD24 = 3, LNB_NORM_QUAD24_SCHED = 4,                        /* gemv_quad_kernel<24, 256, 6, ...> / <24, 128, 6, 10, ...>: 6 */
       LNB_NORM_GATE_UP56 = 5, LNB_NORM_GATE_UP28 = 6,                        /* gemv_chain_kernel<56 / 28, 2, 14336, 7, 8, SILU_MUL>: 7 */
       LNB_NORM_GATE_UP56_PACKED = 7, LNB_NORM_HEAD_PACKED = 8,               /* gemv_chain_pk_kernel, gate|up: 7; the LM head: 8 */
       LNB_NORM_ROWS_WIDE = 9, LNB_NORM_BATCH_XT = 10,                        /* batch_rmsnorm_xt_kernel<false> / <true>: 6 */
       LNB_NORM_ROWS_WAVE = 11, LNB_NORM_FORMS = 12 };                        /* rmsnorm_rows_kernel: the plain serial loop */
int lnb_op_rmsnorm_sum(int device, const uint16_t* x, int rows, int k_in, float eps, int form,
                       uint32_t* sum_bits, uint32_t* scale_bits, int32_t* walk);

/* either operator in a given arithmetic mode (norm_w == NULL: plain linear); LNB_MODE_FAST runs the split-K kernels */
int lnb_op_linear_mode(int device, const uint16_t* x, const uint16_t* norm_w, float eps, const uint16_t* w, uint16_t* y,
                       int rows, int n_out, int k_in, int rw, int mode);
/* ml.Argmax (operations_impl.go:513-548) of n bf16 values: strict '<' scan from -MaxFloat32, so the FIRST maximum wins and
 * NaN / -inf are never selected (-1 when nothing qualifies); the kernel the device greedy loop uses (inference.go:207-211) */
int lnb_op_argmax(int device, const uint16_t* logits_bf16, int n, int32_t* out);
/* The softmax numerator as the device evaluates it, over ALL 65536 possible bf16 raw scores s: out[s] = exp(float64(trunc_bf16(float32(s) / divisor)))
 * (llamatransformer.go:464 DivToScalar, operations_impl.go:498 math.Exp) -- the table every attention kernel either looks up or computes inline with the same
 * instructions.  divisor = 1: the device's f64 exp on every bf16 value, which a test compares bit for bit with the host libm the oracle uses. */
int lnb_op_exp_table(int device, float divisor, double* out65536);

/* ---- weight ingestion: replaces torch.TorchModelReader + model.loadModelArgsFromFile (SURVEY.md 8f "next" #2) -------
 * src/torch/torchmodelreader.go:39-145, src/torch/types.go:9-56, src/pickle/pickledispatch.go:13-78,
 * src/common/memorymapper_unix.go:18-41, src/model/loader.go:183-192, src/model/modelargs.go:12-65.
 * A checkpoint handle is a read-only mmap of a PyTorch zip file (Meta's consolidated.00.pth): entries must be STORED,
 * exactly one *.pkl, tensors rebuilt by torch._utils._rebuild_tensor_v2 over torch.BFloat16Storage (Half/Float storages
 * are listed but not loadable into a model).  Tensor data pointers point INTO the mmap and stay valid until
 * lnb_checkpoint_close; lnb_model_set_tensor / lnb_model_load_checkpoint copy from there straight to the device. */
typedef struct lnb_checkpoint lnb_checkpoint;
enum { LNB_DTYPE_BF16 = 0, LNB_DTYPE_F16 = 1, LNB_DTYPE_F32 = 2 };
int lnb_checkpoint_open(const char* path, lnb_checkpoint** out);
void lnb_checkpoint_close(lnb_checkpoint* c);
int lnb_checkpoint_num_tensors(const lnb_checkpoint* c);
/* index of a tensor by its key, -1 if absent */
int lnb_checkpoint_find(const lnb_checkpoint* c, const char* name);
/* any out pointer may be NULL; shape has room for 4 dims; fails for non-contiguous tensors */
int lnb_checkpoint_tensor(const lnb_checkpoint* c, int index, const char** name, int* dtype, int64_t* shape4, int* rank,
                          const void** data, int64_t* nbytes);
/* bind every tensor the model stage owns (getTensor semantics: "tensor \"x\" not found", "... has incorrect shape;
 * expected [a b], got [c d]"); the model still needs lnb_model_finalize afterwards */
int lnb_model_load_checkpoint(lnb_model* m, const lnb_checkpoint* c);
/* params.json -> lnb_model_args with NewModelArgs' defaults for absent keys (n_kv_heads -1, vocab_size -1, multiple_of 256,
 * ffn_dim_multiplier -1, norm_eps 1e-5, rope_theta 500000, use_scaled_rope false, max_seq_len 2048) */
int lnb_model_args_from_json(const char* params_json_path, lnb_model_args* out);

/* ---- prompt tokenisation (SURVEY.md 8f "next" #3): tiktoken reader + split pattern + byte-pair merge + chat template --------
 * src/tiktoken/tiktokenreader.go:12-85, src/model/vocabulary.go:22-50, src/inference/tokenize.go:27-197.  Host code only.
 * tokenizer.model = lines "<base64 token> <rank>"; 256 special tokens follow the mergeable ranks.  Pieces are BYTES. */
typedef struct lnb_tokenizer lnb_tokenizer;
int lnb_tokenizer_load(const char* tokenizer_model_path, lnb_tokenizer** out);
void lnb_tokenizer_free(lnb_tokenizer* t);
int lnb_tokenizer_vocab_size(const lnb_tokenizer* t);
/* ids of <|begin_of_text|>, <|end_of_text|>, <|eot_id|>, <|eom_id|> (the last two are the stop ids); any pointer may be NULL */
int lnb_tokenizer_special(const lnb_tokenizer* t, int32_t* bos, int32_t* eos, int32_t* eot, int32_t* eom);
int lnb_tokenizer_token_id(const lnb_tokenizer* t, const char* bytes, int len);            /* -1 if absent */
int lnb_tokenizer_piece(const lnb_tokenizer* t, int32_t id, const char** bytes, int* len);  /* Vocabulary.IdToToken */
/* InferenceEngine.TokenizeString: returns the number of tokens written to out (capacity cap), < 0 on error */
int lnb_tokenizer_encode(const lnb_tokenizer* t, const char* text, int len, int32_t* out, int cap);
/* InferenceEngine.Tokenize(promptParts): <|begin_of_text|>, then per non-empty part <|start_header_id|> header <|end_header_id|>
 * "\n\n" content <|eot_id|>, then the open assistant header */
int lnb_tokenizer_encode_chat(const lnb_tokenizer* t, const char* const* headers, const char* const* contents, int n_parts,
                              int32_t* out, int cap);
/* Detokeniser = InferenceEngine.TokenToString (src/inference/tokenize.go:197-239) with its generationDecodingContext.waitingBytes
 * (inference.go:35): a piece that is not valid UTF-8 by itself (byte-fallback tokens; pieces ending inside a character) is buffered until the
 * buffered bytes are valid UTF-8, then ONE rune is released; valid pieces pass through.  lnb_tokenizer_decode_stream returns the number of
 * bytes written to out (0 while waiting; *added_to_waiting = the reference's third result), < 0 on error.  One stream per generation.
 * Not restated: processEmoji's aliases and its buffering of combining marks / ZWJ sequences (emoji.go) -- those pieces come out as text. */
typedef struct lnb_detok lnb_detok;
int lnb_tokenizer_stream_create(const lnb_tokenizer* t, lnb_detok** out);
void lnb_tokenizer_stream_free(lnb_detok* d);
int lnb_tokenizer_decode_stream(lnb_detok* d, int32_t token_id, char* out, int cap, int* added_to_waiting);
int lnb_tokenizer_stream_pending(const lnb_detok* d, const char** bytes, int* len);       /* the bytes still waiting */

#ifdef __cplusplus
}
#endif
#endif
