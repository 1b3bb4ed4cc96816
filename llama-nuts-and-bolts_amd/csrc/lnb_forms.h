// Every kernel FORM a launch function decides between, one row each: name, purpose.  Plain C++17, no HIP (tests/native/forms_test.cpp).
// A form is one arm of a branch in a launch function: the same operation, the same bits, another kernel (or another instantiation of it) picked by shape or
// by an LNB_* knob.  The tally answers "which arm did this call take": a test that forces a form asserts that it ran (tests/form_tally.py), because half of
// the knobs are ONCE and setting one after its first use changes nothing.
//   Counters are process-wide relaxed atomics, one per (form, epilogue); forms that are no product count under epilogue 0.  form_ran() is called on the HOST at
//   the branch where the launch function picks the kernel, just before the launch: nothing on the device changes.  A launch recorded while a stream is being
//   captured counts ONCE, at capture; replays of the graph do not count (the launch function does not run again).  The two pipeline.* rows count a stage step
//   per call instead: a replay is what they are about.
// Names are dotted paths and no name is a path prefix of another, so that "gemm_stream" or "gemm_stream.copy" can stand for everything below it.
// C ABI (include/lnb.h): lnb_form_count / lnb_form_count_reset / lnb_form_name.
#pragma once
#include <atomic>
#include <cstring>
#define LNB_FORMS(X) \
    /* prefill products, LDS-tiled (launch_gemm) */ \
    X(GEMM_MFMA_T16, "gemm_mfma.t16", "gemm_mfma_kernel<*, *, 1, 128>: 16 weight rows per workgroup, the four waves split the batch rows (few tiles)") \
    X(GEMM_MFMA_T64, "gemm_mfma.t64", "gemm_mfma_kernel<*, *, 4, 64>: 64 weight rows x 64 batch rows per workgroup") \
    X(GEMM_MFMA_T128, "gemm_mfma.t128", "gemm_mfma_kernel<*, *, 4, 128>: 64 weight rows x 128 batch rows per workgroup") \
    /* prefill products, streaming feed (launch_gemm_stream): A-operand source x batch tiles per wave x two weight tiles per wave */ \
    X(GS_COPY_1, "gemm_stream.copy.ntw1", "gemm_stream_kernel from the matrix-core copy, one batch tile per wave") \
    X(GS_COPY_2, "gemm_stream.copy.ntw2", "the same, two batch tiles per wave") \
    X(GS_COPY_4, "gemm_stream.copy.ntw4", "the same, four batch tiles per wave") \
    X(GS_COPY_4_TT, "gemm_stream.copy.ntw4_tt", "the same, four batch tiles and two weight tiles per wave") \
    X(GS_ROWCAST_1, "gemm_stream.rowcast.ntw1", "gemm_stream_kernel from the resident row-broadcast layout, one batch tile per wave") \
    X(GS_ROWCAST_2, "gemm_stream.rowcast.ntw2", "the same, two batch tiles per wave") \
    X(GS_ROWCAST_4, "gemm_stream.rowcast.ntw4", "the same, four batch tiles per wave") \
    X(GS_ROWCAST_4_TT, "gemm_stream.rowcast.ntw4_tt", "the same, four batch tiles and two weight tiles per wave") \
    X(GS_CHAIN_1, "gemm_stream.chain.ntw1", "gemm_stream_kernel from a resident chain layout (transposed inside the quad), one batch tile per wave") \
    X(GS_CHAIN_2, "gemm_stream.chain.ntw2", "the same, two batch tiles per wave") \
    X(GS_CHAIN_4, "gemm_stream.chain.ntw4", "the same, four batch tiles per wave") \
    X(GS_ORDER_ROWS, "gemm_stream_order.rows", "a gemm_stream_kernel launch dispatched row groups fastest") \
    X(GS_ORDER_TILES, "gemm_stream_order.tiles", "a gemm_stream_kernel launch dispatched weight-tile groups fastest") \
    X(GEMM_BLGP, "gemm_blgp", "gemm_blgp_kernel: chain-layout prefill product with the B operand broadcast by BLGP (LNB_GEMM_BLGP)") \
    /* batched decode products (lnbk_stream) */ \
    X(MFMA_PAIR, "mfma_pair", "mfma_pair_kernel: thin batched product, chain wave + helper wave per tile") \
    X(MFMA_STREAM_C1, "mfma_stream.c1", "mfma_stream_kernel<1, *>: one tile chain per wave (LNB_STREAM_PAIR=0)") \
    X(MFMA_STREAM_C2, "mfma_stream.c2", "mfma_stream_kernel<2, *>: two tile chains per wave (fat matrices, gate|up)") \
    /* norms */ \
    X(RMSNORM_ROWS_WAVE, "rmsnorm_rows.wave", "rmsnorm_rows_kernel: one wave per row (K no multiple of 128, LNB_NORM_ROWS_WIDE=0)") \
    X(RMSNORM_ROWS_WIDE, "rmsnorm_rows.wide", "batch_rmsnorm_xt_kernel<false>: seven waves per row, the prefill norm") \
    X(BATCH_RMSNORM, "batch_rmsnorm", "batch_rmsnorm_xt_kernel<true>: the batched step's norm, output as f32 columns") \
    /* one-token products (lnbk_gemv) */ \
    X(ROWCAST, "rowcast", "rowcast_kernel: row-broadcast GEMV, self-feeding (K no multiple of 1024, throughput schedule, LNB_ROWCAST_LDS=0)") \
    X(ROWCAST_LDS, "rowcast_lds", "rowcast_lds_kernel: row-broadcast GEMV, chain waves fed by helpers through the LDS") \
    X(GEMV_QUAD, "gemv_quad", "gemv_quad_kernel: quad-DPP chain waves (24-row blocks; 16-row blocks with LNB_W2_QUAD)") \
    X(GEMV_CHAIN_16, "gemv_chain.rw16", "gemv_chain_kernel, 16 rows per block") \
    X(GEMV_CHAIN_28, "gemv_chain.rw28", "gemv_chain_kernel, 28 rows per block, two chains (LNB_RW_W13=28)") \
    X(GEMV_CHAIN_32, "gemv_chain.rw32", "gemv_chain_kernel, 32 rows per block") \
    X(GEMV_CHAIN_56, "gemv_chain.rw56", "gemv_chain_kernel, 56 rows per block, two chains, eight ring stages (gate|up from the raw bf16)") \
    X(GEMV_CHAIN_56_TP, "gemv_chain.rw56_tp", "the same with six ring stages: the throughput schedule's gate|up kernel (LNB_TP_W13=0: the eight-stage one)") \
    X(GEMV_CHAIN_64, "gemv_chain.rw64", "gemv_chain_kernel, 64 rows per block") \
    X(GEMV_CHAIN_PK, "gemv_chain_pk", "gemv_chain_pk_kernel: gate|up from the 13-bit planar copy") \
    X(GEMV_HEAD_PK, "gemv_head_pk", "gemv_chain_pk_kernel, 128-row blocks as two chains of 64: the LM head from its 13-bit planar copy (LNB_HEAD_PACKED)") \
    /* short-context attention of a batched step (launch_attn_short with a batch table) */ \
    X(ATTN_BATCH_PLAIN, "attn_batch.plain", "attn_exact_kernel<HD>: one workgroup per (head, sequence), the one-token kernel (head_dim 64 / 32, few workgroups, LNB_ATTN_BATCH_DENSE=0)") \
    X(ATTN_BATCH_DENSE, "attn_batch.dense", "attn_exact_kernel<128, DENSE>: head_dim 128 and more than 256 (head, sequence) workgroups, dispatched tile-major") \
    X(ATTN_BATCH_DENSE_HM, "attn_batch.dense_headmajor", "the same kernel dispatched head-major (LNB_ATTN_BATCH_HEADMAJOR=1)") \
    X(ATTN_BATCH_GQA, "attn_batch.gqa", "attn_gqa_kernel<128, 4>: one workgroup per (KV head, sequence) for four query heads per KV head") \
    /* prefix sharing (lnb_ctx_fork) */ \
    X(KV_FORK_PLAIN, "kv_fork.plain", "kv_fork_kernel<false>, one destination group") \
    X(KV_FORK_NT, "kv_fork.nt", "kv_fork_kernel<true>: non-temporal loads and stores (LNB_FORK_NT)") \
    X(KV_FORK_SPLIT, "kv_fork.split", "kv_fork_kernel with the destinations dealt over several workgroup groups (LNB_FORK_SPLIT; counted beside plain / nt)") \
    X(KV_FORK_COPY, "kv_fork.copy", "the copy engine, no kernel (LNB_FORK_COPY)") \
    /* the token of a sampling decode step (lnb_decode_sample_until; greedy steps launch argmax_kernel and count nothing) */ \
    X(SAMPLE_ROW, "sample.row", "sample_kernel: one workgroup per logits row -- the one-token sampling step, rows of lnb_op_sample") \
    X(SAMPLE_BATCH, "sample.batch", "batch_sample_kernel: one workgroup per member of a batched sampling step, each with its own sampler") \
    X(SAMPLE_SPEC, "sample.spec", "spec_sample_commit_kernel: one workgroup per column of a verify pass, each at its own position; the last one accepts and emits") \
    X(SAMPLE_SPEC_MANY, "sample.spec_many", "spec_many_sample_commit_kernel: the same per column of a many-context pass, each member with its own sampler") \
    /* the tolerance mode (lnb_fast.hip: launch_a, launch_b, launch_gemm_fast, lnbk_fast_attn) */ \
    X(FAST_GEMV_A_RG8, "fast_gemv_a.rg8", "fast_gemv_a<*, *, *, 8>: split-K GEMV over a chain layout, 8 rows per work unit (few units, LNB_FAST_RG=8)") \
    X(FAST_GEMV_A_RG16, "fast_gemv_a.rg16", "the same, 16 rows per work unit") \
    X(FAST_GEMV_A_RG32, "fast_gemv_a.rg32", "the same, 32 rows per work unit") \
    X(FAST_GEMV_A_RG64, "fast_gemv_a.rg64", "the same, 64 rows per work unit (1024 and more 64-row blocks: the LM head)") \
    X(FAST_GEMV_B, "fast_gemv_b", "fast_gemv_b: split-K GEMV over the row-broadcast layout") \
    X(FAST_GEMM_A_MT4_WB2, "fast_gemm.a.mt4_wb2", "fast_gemm_kernel<*, *, false, 4, 2>: bf16 matrix-core GEMM from a chain layout, 128 batch rows, two workgroups per CU") \
    X(FAST_GEMM_A_MT4_WB3, "fast_gemm.a.mt4_wb3", "fast_gemm_kernel<*, *, false, 4, 3>: 128 batch rows, one workgroup per CU (LNB_FAST_GEMM_2WG=0, up to 128 rows)") \
    X(FAST_GEMM_A_MT8_WB3, "fast_gemm.a.mt8_wb3", "fast_gemm_kernel<*, *, false, 8, 3>: 256 batch rows, one workgroup per CU (1024 rows and more)") \
    X(FAST_GEMM_B_MT4_WB2, "fast_gemm.b.mt4_wb2", "fast_gemm_kernel<*, 1, true, 4, 2>: the same three from the row-broadcast layout") \
    X(FAST_GEMM_B_MT4_WB3, "fast_gemm.b.mt4_wb3", "fast_gemm_kernel<*, 1, true, 4, 3>") \
    X(FAST_GEMM_B_MT8_WB3, "fast_gemm.b.mt8_wb3", "fast_gemm_kernel<*, 1, true, 8, 3>") \
    X(FAST_ATTN_HD64, "fast_attn.hd64", "fast_attn_prefill_kernel<64>: flash attention on the bf16 matrix cores") \
    X(FAST_ATTN_HD128, "fast_attn.hd128", "fast_attn_prefill_kernel<128>") \
    /* pipeline stage step */ \
    X(PIPELINE_REPLAY, "pipeline.replay", "a one-token or batched pipeline stage step replayed from its captured graph (counted per step)") \
    X(PIPELINE_EAGER, "pipeline.eager", "such a step launched eagerly (LNB_PIPELINE_GRAPH=0; counted per step)")
#define X(id, name, purpose) id,
enum class Form { LNB_FORMS(X) COUNT };
#undef X
#define X(id, name, purpose) {name, purpose},
constexpr struct FormInfo { const char* name; const char* purpose; } LNB_FORM_TABLE[] = {LNB_FORMS(X)};
#undef X
constexpr int LNB_FORM_EPIS = 4;                             // EPI_STORE, EPI_QKV_ROPE, EPI_RESID, EPI_SILU_MUL (lnb_device.h)
inline std::atomic<long long> g_form_tally[(int)Form::COUNT][LNB_FORM_EPIS];
inline void form_ran(Form f, int epi = 0) { g_form_tally[(int)f][epi >= 0 && epi < LNB_FORM_EPIS ? epi : 0].fetch_add(1, std::memory_order_relaxed); }
inline int form_index(const char* name) {
    for (int i = 0; name && i < (int)Form::COUNT; i++) if (!strcmp(LNB_FORM_TABLE[i].name, name)) return i;
    return -1;
}
// epi -1: the sum over the epilogues; a form index or an epilogue out of range: -1
inline long long form_count(int form, int epi) {
    if (form < 0 || form >= (int)Form::COUNT || epi < -1 || epi >= LNB_FORM_EPIS) return -1;
    long long n = 0;
    for (int e = 0; e < LNB_FORM_EPIS; e++) if (epi < 0 || e == epi) n += g_form_tally[form][e].load(std::memory_order_relaxed);
    return n;
}
inline void form_count_reset() { for (auto& row : g_form_tally) for (auto& c : row) c.store(0, std::memory_order_relaxed); }
