// Every LNB_* environment variable the shared library reads, one row each: name (without LNB_), default, lifetime, purpose.  Plain C++17, no HIP
// (tests/native/knobs_test.cpp); INTEGRATION.md "Environment knobs" lists the same rows (tests/test_knobs.py).  Python-side variables are not here.
//   ONCE: read at first use and kept for the process.   LIVE: read at every query (a test may switch it inside one process).
// One parse rule: unset or empty = the default, anything else through atoi.
#pragma once
#include <atomic>
#include <cstdlib>
#define LNB_KNOBS(X) \
    /* layout choice at load */ \
    X(RW_QKV, 0, LIVE, "rows per block of the resident wq|wk|wv layout (16 / 24 / 32 / 64; 0: by shape)") \
    X(RW_WO, 0, LIVE, "rows per block of the resident wo layout (4: row-broadcast; 0: by shape)") \
    X(RW_W13, 0, LIVE, "rows per block of the resident gate|up layout (28: the half-height band order, measurement; 0: by shape)") \
    X(RW_W2, 0, LIVE, "rows per block of the resident w2 layout (16 with W2_QUAD: measurement; 0: by shape)") \
    X(RW_OUT, 0, LIVE, "rows per block of the resident LM-head layout (0: by shape)") \
    X(RW_OP, 0, LIVE, "rows per block of a stand-alone lnb_op_linear operand (0: by shape)") \
    /* one-token decode */ \
    X(W13_PACKED, 1, LIVE, "0: lnb_model_finalize builds no 13-bit planar copy of the gate|up matrices; the one-token step streams the raw bf16 (lnb_model_wpack_info)") \
    X(HEAD_PACKED, 1, LIVE, "0: lnb_model_finalize builds no 13-bit planar copy of the LM head; the one-token step streams the raw bf16 (lnb_model_wpack_head_status)") \
    /* prefill form */ \
    X(PREFILL_MFMA, 1, ONCE, "0: calls of 16+ rows stay on the one-row kernels (what the parity tests compare the matrix-core forms with)") \
    X(PREFILL_STREAM, 1, ONCE, "0: prefill products on the LDS-tiled gemm_mfma_kernel, never the streaming feed") \
    X(PREFILL_NATIVE, 1, ONCE, "0: the streaming feed only from the matrix-core copy, not from the resident layouts") \
    X(GEMM_TILE, 0, ONCE, "force the gemm_mfma_kernel tile: 1 (16-row) / 64 / 128; 0: by tile count") \
    X(GS_NTW, 0, LIVE, "force gemm_stream_kernel's batch tiles per wave: 1 / 2 / 4") \
    X(GS_NTW_CHAIN, 0, ONCE, "the same, for the chain layouts only") \
    X(GS_TT, -1, LIVE, "two weight tiles per wave in gemm_stream_kernel: 0 never, 1 whenever the form exists, -1 by workgroup count") \
    X(GS_ORDER, -1, ONCE, "gemm_stream_kernel dispatch order: 1 row groups fastest, 0 tile groups fastest, -1 by row-group count") \
    X(GEMM_BLGP, 0, LIVE, "1 / 2: chain-layout prefill products through gemm_blgp_kernel (bit-exact, measured slower)") \
    X(NORM_ROWS_WIDE, 1, ONCE, "0: prefill RMSNorm on the one-wave rmsnorm_rows_kernel") \
    X(ATTN_MFMA2, 0, LIVE, "N > 0: prefill attention of N+ rows on the two-tile attn_mfma2_kernel (measured slower); 0: never") \
    X(ATTN_SIDX_MB, 4096, LIVE, "largest score-index scratch (MiB) the scores-kept prefill attention may allocate") \
    X(ATTN_SIDX_KEEP_MB, 256, LIVE, "a score-index scratch above this (MiB) is given back at the next one-token call") \
    X(OP_STREAM, 0, LIVE, "1: lnb_op_linear of 16+ rows through gemm_stream_kernel (tests)") \
    /* decode attention form */ \
    X(ATTN_LONG_T, 512, LIVE, "context length from which a new context decodes with the long-context attention kernels") \
    X(ATTN_ONE, 0, ONCE, "1: long-context decode attention in one launch (attn_one_kernel; measured slower); a context beyond lnb_ctx_create's capacity keeps the two launches") \
    X(ATTN_LAZY, 1, LIVE, "0: the long-context PV pass without the lazy certificate (attn_long_pv_kernel); a context beyond lnb_ctx_create's capacity keeps the lazy one") \
    X(ATTN_TOUCH, 1, LIVE, "0: the long-context scores pass does not touch V ahead of the PV pass (A/B)") \
    X(ATTN_ROWS_RPW, 4, ONCE, "query rows per PV workgroup of the multi-row long-context attention (attn_rows_pv_kernel): 1, 2 or 4 -- any other value makes the calls that would run it fail with a message naming this knob") \
    /* batched decode */ \
    X(BATCH_GROUPS, 1, ONCE, "0: 17..32 sequences decode as rows, not as two column groups") \
    X(STREAM_PAIR, 1, LIVE, "0: thin batched products on the one-wave mfma_stream_kernel, not mfma_pair_kernel") \
    X(ATTN_GQA, -1, LIVE, "batched decode attention per (KV head, sequence): 0 never, 1 always, -1 from 256 workgroups on") \
    X(ATTN_GQA_FORCE_ZSEQ, 0, LIVE, "1: every head of attn_gqa_kernel walks the serial denominator (tests)") \
    X(ATTN_BATCH_DENSE, 1, LIVE, "0: batched decode attention never takes the dense-dispatch attn_exact_kernel form") \
    X(ATTN_BATCH_HEADMAJOR, 0, LIVE, "1: that form dispatches head-major (A/B)") \
    X(APPEND_MANY_COLS, 128, LIVE, "columns per pass of lnb_forward_append_many (1..128; any other value makes the call fail with a message naming this knob): tests reach every width form and the pass boundary with few rows, the bench sweeps it") \
    /* prefix sharing */ \
    X(FORK_COPY, 0, LIVE, "1: lnb_ctx_fork on the copy engine (hipMemcpy2DAsync per layer and destination, no kernel launch): the comparison kv_fork_kernel has to beat (2.5x slower at 4096 positions into 127 contexts, 7.6 - 52x at 128 positions, 1.4x at its best: no crossover), and a cross-check on its bits") \
    X(FORK_NT, 0, LIVE, "1: kv_fork_kernel with non-temporal loads and stores (measurement: from 3 % faster to 20 % slower than the plain form)") \
    X(FORK_SPLIT, 0, LIVE, "N > 1: kv_fork_kernel deals the destinations over N workgroup groups, each reading the source (measurement: slower from 1024 positions on)") \
    /* tolerance mode */ \
    X(FAST_GEMM_MIN_ROWS, 192, ONCE, "rows from which the tolerance mode uses its bf16 GEMM instead of the exact one") \
    X(FAST_GEMM_2WG, -1, ONCE, "bf16 GEMM batch tile: 1 = 128 rows and two workgroups per CU, 0 = 256 rows, -1 by row count") \
    X(FAST_RG, 0, ONCE, "force the rows per unit of the split-K GEMV: 8 / 16 / 32 / 64") \
    X(FAST_GRID_CAP, 2048, ONCE, "largest grid.x of the split-K GEMV") \
    /* pipeline */ \
    X(PIPELINE_GRAPH, 1, LIVE, "0: pipeline stages launch eagerly instead of replaying captured graphs") \
    X(PIPELINE_LOG_CAP, 1 << 16, LIVE, "entries of a pipeline stage's event log ring (the wrap-around test shrinks it)") \
    /* measurement only */ \
    X(NO_GRAPH, 0, LIVE, "1: greedy and batched decode launch every step eagerly") \
    X(GEMV_TIMING, 0, LIVE, "1: lnb_profile_kernel dumps the per-wave stamps of the profiled launch") \
    X(PROFILE_SAME_LAYER, 0, LIVE, "1: lnb_profile_kernel stays on one layer (weights served from the Infinity Cache)") \
    X(MEASURE_SKIP_TOKEN_KERNELS, 0, LIVE, "1: the decode step without its embedding and argmax launches (timing only: tokens are garbage)") \
    X(ROWCAST_LDS, 1, ONCE, "0: the row-broadcast GEMV always on the self-feeding rowcast_kernel") \
    X(TP_W13, 1, ONCE, "0: the throughput schedule keeps the eight-stage gate|up kernel (A/B)") \
    X(W2_QUAD, 0, LIVE, "1 / 2: a 16-row w2 layout on gemv_quad_kernel with 128- / 256-step stages (measurement only)") \
    X(W2_PRIO, 0, LIVE, "wave priority handed to the w2 launch of a block (measurement)") \
    X(W2_LDS_PAD, 28 * 1024, LIVE, "LDS padding of the w2 launch in the profiled w1|w3 + w2 pair (measurement)") \
    X(ATTN_GQA_DBG, 0, LIVE, "1: attn_gqa_kernel stamps the phases of one workgroup (lnbk_attn_gqa_dbg_dump prints them)")
enum KnobLife { ONCE, LIVE };
#define X(n, d, l, p) n,
enum class Knob { LNB_KNOBS(X) COUNT };
#undef X
#define X(n, d, l, p) {"LNB_" #n, d, l},
constexpr struct KnobInfo { const char* name; int dflt; KnobLife life; } LNB_KNOB_TABLE[] = {LNB_KNOBS(X)};
#undef X
inline int knob(Knob k) {
    const KnobInfo& i = LNB_KNOB_TABLE[(int)k];
    auto read = [&] { const char* s = getenv(i.name); return s && *s ? atoi(s) : i.dflt; };
    if (i.life == LIVE) return read();
    static std::atomic<long long> cache[(int)Knob::COUNT];   // 0: not read yet, else bit 32 + the value
    long long c = cache[(int)k].load(std::memory_order_relaxed);
    if (!c) { c = (1LL << 32) | (unsigned)read(); cache[(int)k].store(c, std::memory_order_relaxed); }
    return (int)(unsigned)c;
}
