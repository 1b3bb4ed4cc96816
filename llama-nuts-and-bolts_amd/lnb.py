"""ctypes plumbing over liblnb_hip.so (the C ABI of include/lnb.h) for tests and bench.py.

This is NOT a compute path: every call goes straight into the HIP library.  There is no CPU
fallback -- if the shared library is missing or no MI355X is visible, the calls raise.
Names mirror the reference's Go API (src/model: LlamaTransformer / InferenceContext,
src/inference: InferenceEngine) so the parity tests read like the reference's own tests.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("LNB_SO") or os.path.join(_HERE, "liblnb_hip.so")     # LNB_SO: measurement aid (A/B builds of the same ABI)
_CSRC = os.path.join(_HERE, "csrc")


MODE_EXACT, MODE_FAST = 0, 1


class LnbError(RuntimeError):
    pass


def build(force=False):
    """hipcc --offload-arch=gfx950 build of the library, in-tree (the .so travels with the repo snapshot)."""
    # every source and header under csrc/ plus the ABI header: a stale git-ignored .so must never be what the tests validate
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".cpp", ".h", ".hpp")) or f == "Makefile"]
    srcs.append(os.path.join(_HERE, "..", "include", "lnb.h"))
    if os.environ.get("LNB_SO"):
        return _SO
    if force or not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
        subprocess.check_call(["make", "-C", _CSRC, "-s"])
    return _SO


class ModelArgs(C.Structure):
    """model.ModelArgs (src/model/modelargs.go:12-27)"""
    _fields_ = [("dim", C.c_int32), ("n_layers", C.c_int32), ("n_heads", C.c_int32), ("n_kv_heads", C.c_int32),
                ("vocab_size", C.c_int32), ("multiple_of", C.c_int32), ("ffn_dim_multiplier", C.c_double),
                ("norm_eps", C.c_float), ("use_scaled_rope", C.c_int32), ("rope_theta", C.c_double),
                ("max_seq_len", C.c_int32)]


LLAMA_8B = dict(dim=4096, n_layers=32, n_heads=32, n_kv_heads=8, vocab_size=128256, multiple_of=1024,
                ffn_dim_multiplier=1.3, norm_eps=1e-5, use_scaled_rope=1, rope_theta=500000.0, max_seq_len=2048)

_lib = None
EXPORTS = [
    "lnb_last_error", "lnb_device_count", "lnb_device_info", "lnb_device_can_access_peer", "lnb_device_pci_bus_id", "lnb_model_create", "lnb_model_create_parts", "lnb_model_destroy", "lnb_model_ffn_hidden_dim",
    "lnb_model_set_tensor", "lnb_model_get_tensor", "lnb_model_fill_synthetic", "lnb_model_finalize",
    "lnb_model_rope_table", "lnb_model_weight_bytes", "lnb_ctx_create", "lnb_ctx_destroy", "lnb_ctx_reset",
    "lnb_ctx_read_kv", "lnb_ctx_set_layer_callback", "lnb_forward", "lnb_decode_greedy", "lnb_ctx_hidden_ptr",
    "lnb_forward_stage", "lnb_forward_stage_begin", "lnb_forward_stage_end", "lnb_ctx_synchronize", "lnb_ctx_stream", "lnb_op_linear", "lnb_op_rmsnorm_linear", "lnb_op_argmax", "lnb_op_exp_table", "lnb_op_linear_mode", "lnb_ctx_set_mode", "lnb_ctx_get_mode", "lnb_ctx_set_schedule", "lnb_ctx_get_schedule", "lnb_ctx_set_attention", "lnb_ctx_zseq_count", "lnb_ctx_norm_fallbacks", "lnb_ctx_prefill_attention_form",
    "lnb_profile_kernel", "lnb_profile_kernel_stamps", "lnb_model_num_tensors", "lnb_model_tensor_info",
    "lnb_checkpoint_open", "lnb_checkpoint_close", "lnb_checkpoint_num_tensors", "lnb_checkpoint_find", "lnb_checkpoint_tensor",
    "lnb_model_load_checkpoint", "lnb_model_args_from_json",
    "lnb_tokenizer_load", "lnb_tokenizer_free", "lnb_tokenizer_vocab_size", "lnb_tokenizer_special", "lnb_tokenizer_token_id",
    "lnb_tokenizer_piece", "lnb_tokenizer_encode", "lnb_tokenizer_encode_chat",
    "lnb_tokenizer_stream_create", "lnb_tokenizer_stream_free", "lnb_tokenizer_decode_stream", "lnb_tokenizer_stream_pending",
    "lnb_pipeline_unique_id", "lnb_pipeline_init", "lnb_pipeline_init_loopback", "lnb_pipeline_destroy", "lnb_pipeline_tick", "lnb_pipeline_sync", "lnb_pipeline_read_tokens", "lnb_pipeline_selftest", "lnb_pipeline_comm_count",
    "lnb_model_enable_batch", "lnb_model_batch_bytes", "lnb_batch_create", "lnb_batch_destroy", "lnb_batch_decode", "lnb_batch_decode_until", "lnb_ctx_set_stop_ids", "lnb_decode_greedy_until", "lnb_batch_profile_kernel", "lnb_batch_set_state", "lnb_batch_check_error", "lnb_pipeline_tick_batch",
    "lnb_pipeline_init_host", "lnb_batch_boundary_ptr",
    "lnb_abi_version", "lnb_runtime_info", "lnb_profile_ffn_pair",
    "lnb_model_wpack_bytes", "lnb_model_wpack_info", "lnb_op_rmsnorm_gate_up",
    "lnb_model_wpack_head_bytes", "lnb_model_wpack_head_status", "lnb_op_rmsnorm_head",
    "lnb_ctx_set_token_probs", "lnb_ctx_read_token_probs", "lnb_ctx_token_prob_walks", "lnb_forward_score", "lnb_op_token_probs",
    "lnb_decode_sample_until", "lnb_batch_decode_sample_until", "lnb_op_sample", "lnb_profile_sample",
    "lnb_forward_append", "lnb_forward_score_append",
    "lnb_ctx_set_draft", "lnb_decode_speculative_until", "lnb_op_ngram_draft",
    "lnb_batch_set_attention", "lnb_ctx_set_batched_attention", "lnb_batch_attention_form", "lnb_ctx_verify_attention_form",
    "lnb_ctx_create_long", "lnb_ctx_max_rows",
    "lnb_ctx_set_rows_attention", "lnb_ctx_append_attention_form",
    "lnb_ctx_fork", "lnb_ctx_prefix_bytes", "lnb_ctx_save_prefix", "lnb_ctx_load_prefix",
    "lnb_forward_append_many", "lnb_model_append_many_info",
    "lnb_decode_speculative_many",
    "lnb_decode_speculative_sample_until", "lnb_decode_speculative_sample_many", "lnb_op_spec_sample_accept",
    "lnb_form_count", "lnb_form_count_reset", "lnb_form_name",
    "lnb_op_rmsnorm_sum",
    "lnb_ctx_attention",
]
EPILOGUES = {"store": 0, "qkv_rope": 1, "resid": 2, "silu_mul": 3}      # EPI_* of csrc/lnb_device.h: the second index of the launch tally
MAX_TOP_K = 16           # LNB_MAX_TOP_K of include/lnb.h (tests/test_token_probs_cpu.py compares them)
MAX_DRAFT = 15           # LNB_MAX_DRAFT of include/lnb.h (tests/test_speculative_cpu.py compares them)
MAX_SEQ_LEN = 131072     # LNB_MAX_SEQ_LEN of include/lnb.h (tests/test_long_context_cpu.py compares them)
MAX_FORK = 128           # LNB_MAX_FORK of include/lnb.h (tests/test_prefix_fork_cpu.py compares them)
ABI_VERSION = 6          # LNB_ABI_VERSION of include/lnb.h this binding was written against (tests/test_cabi.py compares it with the header's)


class SpecStats(C.Structure):
    """lnb_spec_stats (include/lnb.h)"""
    _fields_ = [("passes", C.c_int64), ("verify_passes", C.c_int64), ("drafted", C.c_int64), ("accepted", C.c_int64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class SpecManyInfo(C.Structure):
    """lnb_spec_many_info (include/lnb.h)"""
    _fields_ = [("passes", C.c_int64), ("verify_passes", C.c_int64), ("columns", C.c_int64), ("max_columns", C.c_int64), ("long_passes", C.c_int64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Sampler(C.Structure):
    """lnb_sampler (include/lnb.h): temperature 0 = greedy, top_k 0 = off, top_p 1 = off; the token is a function of the logits row, these four numbers and the position"""
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]

    def __init__(self, temperature=1.0, top_k=0, top_p=1.0, seed=0):
        super().__init__(float(temperature), float(top_p), int(top_k), 0, int(seed) & 0xFFFFFFFFFFFFFFFF)


class SampleInfo(C.Structure):
    """lnb_sample_info (include/lnb.h)"""
    _fields_ = [("w_all", C.c_uint64), ("w_topk", C.c_uint64), ("w_kept", C.c_uint64), ("n_candidates", C.c_int32), ("n_kept", C.c_int32), ("degenerate", C.c_int32),
                ("pad", C.c_int32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "pad"}


def _samplers(samplers, n):
    """n lnb_sampler structs from Sampler objects or (temperature, top_k, top_p, seed) tuples"""
    ss = list(samplers)
    if len(ss) != n:
        raise LnbError("%d samplers for %d rows" % (len(ss), n))
    arr = (Sampler * n)()
    for i, s in enumerate(ss):
        s = s if isinstance(s, Sampler) else Sampler(*s)
        arr[i] = s
    return arr


class RuntimeInfo(C.Structure):
    """lnb_runtime_info_t (include/lnb.h)"""
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("n_cus", C.c_int32),
                ("shader_clock_khz", C.c_int32), ("memory_clock_khz", C.c_int32), ("wall_clock_khz", C.c_int32),
                ("hw_queues_env", C.c_int32), ("hw_queues_set_by_library", C.c_int32), ("hip_initialised_before_load", C.c_int32),
                ("hw_queues_expected", C.c_int32), ("hw_queues_measured", C.c_int32), ("probe_ms", C.c_float),
                ("device_name", C.c_char * 64), ("arch", C.c_char * 32)]



def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise LnbError("liblnb_hip.so is not built (run __graft_entry__.build()); there is no fallback path")
    L = C.CDLL(_SO)
    vp, i32p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    # a stale library behind a newer binding (or the reverse) must fail HERE, not write through a mistyped pointer later
    if not hasattr(L, "lnb_abi_version") or L.lnb_abi_version() != ABI_VERSION:
        raise LnbError("liblnb_hip.so reports ABI version %s, this binding is written against %d: rebuild the library (make -C csrc)"
                       % (L.lnb_abi_version() if hasattr(L, "lnb_abi_version") else "none", ABI_VERSION))
    L.lnb_runtime_info.argtypes = [C.c_int, C.c_int, C.POINTER(RuntimeInfo)]
    L.lnb_profile_ffn_pair.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, f32p]
    L.lnb_last_error.restype = C.c_char_p
    L.lnb_device_count.argtypes = [C.POINTER(C.c_int)]
    L.lnb_device_info.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    L.lnb_device_can_access_peer.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.lnb_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]
    L.lnb_model_create.argtypes = [C.POINTER(ModelArgs), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.lnb_model_create_parts.argtypes = [C.POINTER(ModelArgs), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.lnb_model_destroy.argtypes = [vp]
    L.lnb_model_ffn_hidden_dim.argtypes = [C.POINTER(ModelArgs)]
    L.lnb_model_set_tensor.argtypes = [vp, C.c_char_p, vp, C.POINTER(C.c_int64), C.c_int]
    L.lnb_model_get_tensor.argtypes = [vp, C.c_char_p, vp, C.c_int64]
    L.lnb_model_fill_synthetic.argtypes = [vp, C.c_uint64]
    L.lnb_model_finalize.argtypes = [vp, C.c_int]
    L.lnb_model_rope_table.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int)]
    L.lnb_model_weight_bytes.argtypes = [vp]
    L.lnb_model_weight_bytes.restype = C.c_int64
    L.lnb_ctx_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.lnb_ctx_create_long.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.lnb_ctx_max_rows.argtypes = [vp, C.POINTER(C.c_int)]
    L.lnb_ctx_destroy.argtypes = [vp]
    L.lnb_ctx_reset.argtypes = [vp]
    L.lnb_ctx_read_kv.argtypes = [vp, C.c_int, C.c_int, vp]
    L.lnb_ctx_set_layer_callback.argtypes = [vp, vp, vp]
    L.lnb_forward.argtypes = [vp, vp, C.c_int, C.c_int, vp, i32p]
    L.lnb_decode_greedy.argtypes = [vp, C.c_int32, C.c_int, C.c_int, vp, f32p]
    L.lnb_ctx_hidden_ptr.argtypes = [vp, C.c_int]
    L.lnb_ctx_hidden_ptr.restype = vp
    L.lnb_ctx_attention.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp]
    L.lnb_forward_stage.argtypes = [vp, vp, C.c_int, C.c_int, vp, i32p]
    L.lnb_forward_stage_begin.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.lnb_forward_stage_end.argtypes = [vp, i32p]
    L.lnb_ctx_synchronize.argtypes = [vp]
    L.lnb_ctx_stream.argtypes = [vp]
    L.lnb_ctx_stream.restype = vp
    L.lnb_profile_kernel.argtypes = [vp, C.c_int, C.c_int, C.c_int, f32p]
    L.lnb_profile_kernel_stamps.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(C.c_int)]
    L.lnb_op_linear.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.lnb_op_rmsnorm_linear.argtypes = [C.c_int, vp, vp, C.c_float, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.lnb_ctx_set_mode.argtypes = [vp, C.c_int]
    L.lnb_ctx_get_mode.argtypes = [vp]
    L.lnb_ctx_set_schedule.argtypes = [vp, C.c_int]
    L.lnb_ctx_get_schedule.argtypes = [vp]
    L.lnb_ctx_set_attention.argtypes = [vp, C.c_int, C.c_int]
    L.lnb_ctx_zseq_count.argtypes = [vp, C.POINTER(C.c_int)]
    L.lnb_ctx_norm_fallbacks.argtypes = [vp, C.POINTER(C.c_int)]
    L.lnb_ctx_prefill_attention_form.argtypes = [vp, C.POINTER(C.c_int)]
    L.lnb_pipeline_unique_id.argtypes = [vp]
    L.lnb_pipeline_init.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.lnb_pipeline_init_loopback.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.POINTER(vp)]
    L.lnb_pipeline_init_host.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.lnb_batch_boundary_ptr.argtypes = [vp, C.c_int]
    L.lnb_batch_boundary_ptr.restype = C.c_void_p
    L.lnb_pipeline_selftest.argtypes = [C.c_int, C.c_int]
    L.lnb_pipeline_destroy.argtypes = [vp]
    L.lnb_pipeline_tick.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
    L.lnb_pipeline_sync.argtypes = [vp]
    L.lnb_pipeline_comm_count.argtypes = [vp, C.POINTER(C.c_int)]
    L.lnb_model_enable_batch.argtypes = [vp]
    L.lnb_model_batch_bytes.argtypes = [vp]
    L.lnb_model_batch_bytes.restype = C.c_int64
    L.lnb_model_wpack_bytes.argtypes = [vp]
    L.lnb_model_wpack_bytes.restype = C.c_int64
    L.lnb_model_wpack_info.argtypes = [vp, i32p]
    L.lnb_op_rmsnorm_gate_up.argtypes = [C.c_int, vp, vp, C.c_float, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.lnb_model_wpack_head_bytes.argtypes = [vp]
    L.lnb_model_wpack_head_bytes.restype = C.c_int64
    L.lnb_model_wpack_head_status.argtypes = [vp]
    L.lnb_op_rmsnorm_sum.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp]
    L.lnb_op_rmsnorm_head.argtypes = [C.c_int, vp, vp, C.c_float, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.lnb_batch_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp)]
    L.lnb_batch_destroy.argtypes = [vp]
    L.lnb_batch_decode.argtypes = [vp, i32p, i32p, C.c_int, vp, f32p]
    L.lnb_batch_decode_until.argtypes = [vp, i32p, i32p, C.c_int, vp, vp, vp, f32p]
    L.lnb_ctx_set_stop_ids.argtypes = [vp, vp, C.c_int]
    L.lnb_decode_greedy_until.argtypes = [vp, C.c_int32, C.c_int, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), f32p]
    L.lnb_batch_profile_kernel.argtypes = [vp, C.c_int, C.c_int, C.c_int, f32p]
    L.lnb_batch_set_state.argtypes = [vp, i32p, i32p]
    L.lnb_batch_check_error.argtypes = [vp]
    L.lnb_batch_set_attention.argtypes = [vp, C.c_int, C.c_int]
    L.lnb_ctx_set_batched_attention.argtypes = [vp, C.c_int, C.c_int]
    L.lnb_batch_attention_form.argtypes = [vp, C.POINTER(C.c_int)]
    L.lnb_ctx_verify_attention_form.argtypes = [vp, C.POINTER(C.c_int)]
    L.lnb_ctx_set_rows_attention.argtypes = [vp, C.c_int, C.c_int]
    L.lnb_ctx_append_attention_form.argtypes = [vp, C.POINTER(C.c_int)]
    L.lnb_ctx_fork.argtypes = [vp, C.c_int, C.POINTER(vp), C.c_int]
    L.lnb_ctx_prefix_bytes.argtypes = [vp, C.c_int]
    L.lnb_ctx_prefix_bytes.restype = C.c_int64
    L.lnb_ctx_save_prefix.argtypes = [vp, C.c_int, vp, C.c_int64]
    L.lnb_ctx_load_prefix.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int)]
    L.lnb_forward_append_many.argtypes = [C.POINTER(vp), C.c_int, vp, vp, vp, vp, vp]
    L.lnb_model_append_many_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lnb_decode_speculative_many.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp), vp, vp, vp, C.c_int, C.c_int, vp, vp, vp,
                                              C.POINTER(SpecStats), C.POINTER(SpecManyInfo), f32p]
    L.lnb_pipeline_tick_batch.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.lnb_pipeline_read_tokens.argtypes = [vp, C.c_int, C.c_int, vp]
    L.lnb_op_linear_mode.argtypes = [C.c_int, vp, vp, C.c_float, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.lnb_op_argmax.argtypes = [C.c_int, vp, C.c_int, i32p]
    L.lnb_op_exp_table.argtypes = [C.c_int, C.c_float, vp]
    L.lnb_ctx_set_token_probs.argtypes = [vp, C.c_int]
    L.lnb_ctx_read_token_probs.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.lnb_ctx_token_prob_walks.argtypes = [vp, C.POINTER(C.c_int)]
    L.lnb_forward_score.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, i32p]
    L.lnb_forward_append.argtypes = [vp, vp, C.c_int, C.c_int, vp, i32p]
    L.lnb_forward_score_append.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, i32p]
    L.lnb_decode_sample_until.argtypes = [vp, C.POINTER(Sampler), C.c_int32, C.c_int, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), f32p]
    L.lnb_batch_decode_sample_until.argtypes = [vp, C.POINTER(Sampler), i32p, i32p, C.c_int, vp, vp, vp, f32p]
    L.lnb_op_sample.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.POINTER(Sampler), vp, vp, vp, C.POINTER(SampleInfo)]
    L.lnb_profile_sample.argtypes = [vp, C.POINTER(Sampler), C.c_int, C.c_int, f32p]
    L.lnb_op_token_probs.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.lnb_ctx_set_draft.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int]
    L.lnb_decode_speculative_until.argtypes = [vp, vp, C.c_int, C.c_int32, C.c_int, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                               C.POINTER(SpecStats), f32p]
    L.lnb_op_ngram_draft.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_int)]
    L.lnb_decode_speculative_sample_until.argtypes = [vp, C.POINTER(Sampler), vp, C.c_int, C.c_int32, C.c_int, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                      C.POINTER(SpecStats), f32p]
    L.lnb_decode_speculative_sample_many.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Sampler), C.POINTER(vp), vp, vp, vp, C.c_int, C.c_int, vp, vp, vp,
                                                     C.POINTER(SpecStats), C.POINTER(SpecManyInfo), f32p]
    L.lnb_op_spec_sample_accept.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.POINTER(Sampler), C.c_int, vp, vp, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lnb_model_num_tensors.argtypes = [vp]
    L.lnb_model_tensor_info.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    L.lnb_checkpoint_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.lnb_checkpoint_close.argtypes = [vp]
    L.lnb_checkpoint_close.restype = None
    L.lnb_checkpoint_num_tensors.argtypes = [vp]
    L.lnb_checkpoint_find.argtypes = [vp, C.c_char_p]
    L.lnb_checkpoint_tensor.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                        C.POINTER(vp), C.POINTER(C.c_int64)]
    L.lnb_model_load_checkpoint.argtypes = [vp, vp]
    L.lnb_model_args_from_json.argtypes = [C.c_char_p, C.POINTER(ModelArgs)]
    L.lnb_tokenizer_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.lnb_tokenizer_free.argtypes = [vp]
    L.lnb_tokenizer_free.restype = None
    L.lnb_tokenizer_vocab_size.argtypes = [vp]
    L.lnb_tokenizer_special.argtypes = [vp, i32p, i32p, i32p, i32p]
    L.lnb_tokenizer_token_id.argtypes = [vp, C.c_char_p, C.c_int]
    L.lnb_tokenizer_piece.argtypes = [vp, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.lnb_tokenizer_encode.argtypes = [vp, C.c_char_p, C.c_int, i32p, C.c_int]
    L.lnb_tokenizer_encode_chat.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int, i32p, C.c_int]
    L.lnb_tokenizer_stream_create.argtypes = [vp, C.POINTER(vp)]
    L.lnb_tokenizer_stream_free.argtypes = [vp]
    L.lnb_tokenizer_stream_free.restype = None
    L.lnb_tokenizer_decode_stream.argtypes = [vp, C.c_int32, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.lnb_tokenizer_stream_pending.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.lnb_form_count.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int64)]
    L.lnb_form_count_reset.argtypes = []
    L.lnb_form_name.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    _lib = L
    return L


def _chk(rc):
    if rc != 0:
        raise LnbError(lib().lnb_last_error().decode("utf-8", "replace"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def form_names():
    """the names of the launch tally's rows (csrc/lnb_forms.h), in table order"""
    L, out, name = lib(), [], C.c_char_p()
    while L.lnb_form_name(len(out), C.byref(name)) == 0:
        out.append(name.value.decode())
    return out


def form_count(form, epi=None):
    """launches of the kernel form `form` since the last form_count_reset(); epi: one of EPILOGUES (a name or its number), None = the sum"""
    n = C.c_int64(0)
    _chk(lib().lnb_form_count(form.encode(), -1 if epi is None else EPILOGUES.get(epi, epi), C.byref(n)))
    return n.value


def form_count_reset():
    _chk(lib().lnb_form_count_reset())


def device_count():
    n = C.c_int(0)
    _chk(lib().lnb_device_count(C.byref(n)))
    return n.value


def device_info(device=0):
    """{name, arch, hbm_bytes, n_cus} of a device index (lnb_device_info)"""
    name, arch = C.create_string_buffer(256), C.create_string_buffer(256)
    hbm, cus = C.c_int64(0), C.c_int(0)
    _chk(lib().lnb_device_info(device, name, 256, C.byref(hbm), C.byref(cus), arch, 256))
    return {"name": name.value.decode(), "arch": arch.value.decode(), "hbm_bytes": hbm.value, "n_cus": cus.value}


def runtime_info(device=0, probe_queues=False):
    """lnb_runtime_info as a dict: hardware queues the HIP runtime was told to use / really uses, clocks, device"""
    ri = RuntimeInfo()
    _chk(lib().lnb_runtime_info(device, 1 if probe_queues else 0, C.byref(ri)))
    d = {k: getattr(ri, k) for k, _ in RuntimeInfo._fields_}
    d["device_name"] = ri.device_name.decode("utf-8", "replace"); d["arch"] = ri.arch.decode("utf-8", "replace")
    d["probe_ms"] = round(float(ri.probe_ms), 3)
    return d


def queue_warning(contexts_in_flight, info):
    """the sentence a host prints when it keeps more contexts in flight than the runtime has hardware queues (streams on one queue serialise)"""
    q = info.get("hw_queues_measured") or info.get("hw_queues_expected") or 4
    if contexts_in_flight <= q:
        return None
    return "%d contexts in flight on %d hardware queues: streams that share a queue run one after the other" % (contexts_in_flight, q)


def can_access_peer(device, peer):
    out = C.c_int(0)
    _chk(lib().lnb_device_can_access_peer(device, peer, C.byref(out)))
    return bool(out.value)


def pci_bus_id(device):
    buf = C.create_string_buffer(32)
    _chk(lib().lnb_device_pci_bus_id(device, buf, 32))
    return buf.value.decode()


def rccl_selftest(device=0, n_bytes=1 << 20):
    """one-rank RCCL communicator, the pipeline's grouped send + recv to itself, bytes compared (lnb_pipeline_selftest)"""
    _chk(lib().lnb_pipeline_selftest(device, n_bytes))


DTYPES = {0: ("bf16", np.uint16), 1: ("f16", np.uint16), 2: ("f32", np.float32)}


class Checkpoint:
    """Read-only mmap of a PyTorch zip checkpoint (torch.TorchModelReader, src/torch/torchmodelreader.go:39-145)."""

    def __init__(self, path):
        self.L = lib()
        self.h = C.c_void_p()
        _chk(self.L.lnb_checkpoint_open(os.fsencode(path), C.byref(self.h)))

    def __len__(self):
        return self.L.lnb_checkpoint_num_tensors(self.h)

    def tensor(self, i):
        """(name, dtype string, shape, numpy view of the mmap'ed bytes -- valid until close())"""
        name, dt, shape, rank, data, nb = C.c_char_p(), C.c_int(), (C.c_int64 * 4)(), C.c_int(), C.c_void_p(), C.c_int64()
        _chk(self.L.lnb_checkpoint_tensor(self.h, i, C.byref(name), C.byref(dt), shape, C.byref(rank), C.byref(data), C.byref(nb)))
        dname, npdt = DTYPES[dt.value]
        shp = tuple(shape[:rank.value])
        n = nb.value // np.dtype(npdt).itemsize
        arr = np.ctypeslib.as_array(C.cast(data.value, C.POINTER(C.c_uint16 if npdt is np.uint16 else C.c_float)), shape=(n,)) if n else np.empty(0, npdt)
        return name.value.decode("utf-8", "replace"), dname, shp, arr.reshape(shp)

    def find(self, name):
        return self.L.lnb_checkpoint_find(self.h, name.encode())

    def close(self):
        if self.h:
            self.L.lnb_checkpoint_close(self.h)
            self.h = C.c_void_p()


class Tokenizer:
    """tiktoken vocabulary + the reference's TokenizeString / Tokenize (src/inference/tokenize.go)."""

    def __init__(self, path):
        self.L = lib()
        self.h = C.c_void_p()
        _chk(self.L.lnb_tokenizer_load(os.fsencode(path), C.byref(self.h)))
        self.vocab_size = self.L.lnb_tokenizer_vocab_size(self.h)
        b, e, t, m = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _chk(self.L.lnb_tokenizer_special(self.h, C.byref(b), C.byref(e), C.byref(t), C.byref(m)))
        self.bos, self.eos, self.eot, self.eom = b.value, e.value, t.value, m.value

    def encode(self, text):
        raw = text if isinstance(text, bytes) else text.encode("utf-8")
        cap = 4 * len(raw) + 16
        out = (C.c_int32 * cap)()
        n = self.L.lnb_tokenizer_encode(self.h, raw, len(raw), out, cap)
        if n < 0:
            raise LnbError(self.L.lnb_last_error().decode("utf-8", "replace"))
        return list(out[:n])

    def encode_chat(self, parts):
        """parts: [(header, content), ...] -> ids with the chat template of Tokenize(promptParts)"""
        hs = (C.c_char_p * len(parts))(*[h.encode("utf-8") for h, _ in parts])
        cs = (C.c_char_p * len(parts))(*[c.encode("utf-8") for _, c in parts])
        cap = 4 * sum(len(h) + len(c) for h, c in parts) + 64 * (len(parts) + 2)
        out = (C.c_int32 * cap)()
        n = self.L.lnb_tokenizer_encode_chat(self.h, hs, cs, len(parts), out, cap)
        if n < 0:
            raise LnbError(self.L.lnb_last_error().decode("utf-8", "replace"))
        return list(out[:n])

    def piece(self, tid):
        p, n = C.c_void_p(), C.c_int()
        _chk(self.L.lnb_tokenizer_piece(self.h, tid, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def token_id(self, piece_bytes):
        return self.L.lnb_tokenizer_token_id(self.h, piece_bytes, len(piece_bytes))

    def stream(self):
        """a TokenToString decoding context (one per generation): .feed(token_id) -> (bytes released, added_to_waiting)"""
        return DecodeStream(self)

    def close(self):
        if self.h:
            self.L.lnb_tokenizer_free(self.h)
            self.h = C.c_void_p()


class DecodeStream:
    """InferenceEngine.TokenToString + generationDecodingContext.waitingBytes (src/inference/tokenize.go:197-239)"""

    def __init__(self, tok):
        self.L, self.h = tok.L, C.c_void_p()
        _chk(self.L.lnb_tokenizer_stream_create(tok.h, C.byref(self.h)))
        self.buf = C.create_string_buffer(1 << 16)

    def feed(self, tid):
        w = C.c_int(0)
        n = self.L.lnb_tokenizer_decode_stream(self.h, int(tid), self.buf, len(self.buf), C.byref(w))
        if n < 0:
            raise LnbError(self.L.lnb_last_error().decode("utf-8", "replace"))
        return self.buf.raw[:n], bool(w.value)

    def pending(self):
        p, n = C.c_void_p(), C.c_int()
        _chk(self.L.lnb_tokenizer_stream_pending(self.h, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def close(self):
        if self.h:
            self.L.lnb_tokenizer_stream_free(self.h)
            self.h = C.c_void_p()


def model_args_from_json(path):
    """params.json -> dict of ModelArgs fields with the reference's defaults (src/model/modelargs.go:29-65)"""
    a = ModelArgs()
    _chk(lib().lnb_model_args_from_json(os.fsencode(path), C.byref(a)))
    return {f: getattr(a, f) for f, _ in ModelArgs._fields_}


class LlamaTransformer:
    """Device-resident model (one pipeline stage): model.NewLlamaTransformer, llamatransformer.go:64-113."""

    def __init__(self, device=0, layer_begin=0, layer_end=None, part_begin=None, part_end=None, **kw):
        """[layer_begin, layer_end) in blocks, or [part_begin, part_end) in thirds of a block (3l = attention part of block l,
        3l+1 = gate/up part, 3l+2 = down part: lnb_model_create_parts)"""
        d = dict(LLAMA_8B)
        d.update(kw)
        self.args = ModelArgs(**d)
        self.L = lib()
        self.h = C.c_void_p()
        self.device = int(device)
        if part_begin is None and part_end is None:
            part_begin, part_end = 3 * layer_begin, 3 * (self.args.n_layers if layer_end is None else layer_end)
        self.part_begin, self.part_end = int(part_begin), int(part_end)
        self.layer_begin, self.layer_end = self.part_begin // 3, (self.part_end + 2) // 3
        _chk(self.L.lnb_model_create_parts(C.byref(self.args), device, self.part_begin, self.part_end, C.byref(self.h)))
        self.ffn_hidden = self.L.lnb_model_ffn_hidden_dim(C.byref(self.args))
        self.head_dim = self.args.dim // self.args.n_heads

    def set_tensor(self, name, arr_u16, shape=None):
        a = np.ascontiguousarray(arr_u16, dtype=np.uint16)
        shp = tuple(shape) if shape is not None else a.shape
        s = (C.c_int64 * len(shp))(*shp)
        _chk(self.L.lnb_model_set_tensor(self.h, name.encode(), _p(a), s, len(shp)))

    def get_tensor(self, name, nelem):
        out = np.empty(nelem, dtype=np.uint16)
        _chk(self.L.lnb_model_get_tensor(self.h, name.encode(), _p(out), nelem))
        return out

    def fill_synthetic(self, seed=1234):
        _chk(self.L.lnb_model_fill_synthetic(self.h, seed))
        return self

    def load_checkpoint(self, ckpt):
        """bind every tensor of this stage from an open Checkpoint (torch.TorchModelReader + getTensor, loader.go:183-192)"""
        _chk(self.L.lnb_model_load_checkpoint(self.h, ckpt.h))
        return self

    def tensor_infos(self):
        out = []
        for k in range(self.L.lnb_model_num_tensors(self.h)):
            name, shape, rank = C.c_char_p(), (C.c_int64 * 2)(), C.c_int()
            _chk(self.L.lnb_model_tensor_info(self.h, k, C.byref(name), shape, C.byref(rank)))
            out.append((name.value.decode(), tuple(shape[:rank.value])))
        return out

    def finalize(self, rope_rows=0):
        _chk(self.L.lnb_model_finalize(self.h, rope_rows))
        return self

    @property
    def PrecomputedFreqsCis(self):
        rows = C.c_int(0)
        _chk(self.L.lnb_model_rope_table(self.h, None, 0, C.byref(rows)))
        out = np.empty((rows.value, self.head_dim // 2, 2), dtype=np.float32)
        _chk(self.L.lnb_model_rope_table(self.h, _p(out), out.size, C.byref(rows)))
        return out

    def weight_bytes(self):
        return int(self.L.lnb_model_weight_bytes(self.h))

    def enable_batch(self):
        """build the matrix-core friendly copy of the weights that batched decode streams (lnb_model_enable_batch); after finalize()"""
        _chk(self.L.lnb_model_enable_batch(self.h))
        return self

    def batch_bytes(self):
        return int(self.L.lnb_model_batch_bytes(self.h))

    def wpack_bytes(self):
        """device bytes of the 13-bit planar copies of the gate|up matrices (lnb_model_wpack_bytes)"""
        return int(self.L.lnb_model_wpack_bytes(self.h))

    def wpack_info(self):
        """gate|up matrices by what the one-token step streams them from (lnb_model_wpack_info)"""
        c = np.zeros(6, dtype=np.int32)
        _chk(self.L.lnb_model_wpack_info(self.h, c.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(zip(("packed", "subnormal", "infnan", "window", "no_memory", "not_tried"), (int(v) for v in c)))

    def wpack_head_bytes(self):
        """device bytes of the LM head's 13-bit planar copy, 0 without one (lnb_model_wpack_head_bytes)"""
        return int(self.L.lnb_model_wpack_head_bytes(self.h))

    def wpack_head_status(self):
        """what the one-token LM head streams (lnb_model_wpack_head_status): "packed", the reason its copy was refused, or "not_tried" """
        s = int(self.L.lnb_model_wpack_head_status(self.h))
        if s < 0:
            _chk(s)
        return ("packed", "subnormal", "infnan", "window", "no_memory", "not_tried")[s]

    def append_many_info(self):
        """of the last ForwardAppendMany on this transformer: {passes, max_columns, long_passes} (lnb_model_append_many_info)"""
        p, w, g = C.c_int(0), C.c_int(0), C.c_int(0)
        _chk(self.L.lnb_model_append_many_info(self.h, C.byref(p), C.byref(w), C.byref(g)))
        return {"passes": p.value, "max_columns": w.value, "long_passes": g.value}

    def close(self):
        if self.h:
            self.L.lnb_model_destroy(self.h)
            self.h = C.c_void_p()


class InferenceContext:
    """model.NewInferenceContext (inferencecontext.go:17-46): device KV cache for one generation.
    max_rows / long_context select lnb_ctx_create_long: up to MAX_SEQ_LEN positions (the transformer finalized with that many rope_rows), the per-call
    activation buffers sized for max_rows rows (None: seq_len) -- calls of more rows are refused.  The two-argument form is lnb_ctx_create (~23 K positions)."""

    def __init__(self, transformer, seq_len, max_rows=None, long_context=False):
        self.t, self.L = transformer, transformer.L
        self.SequenceLength = seq_len
        self.h = C.c_void_p()
        if long_context or max_rows is not None:
            _chk(self.L.lnb_ctx_create_long(transformer.h, seq_len, int(max_rows or 0), C.byref(self.h)))
        else:
            _chk(self.L.lnb_ctx_create(transformer.h, seq_len, C.byref(self.h)))

    def max_rows(self):
        """rows per call the activation buffers hold (lnb_ctx_max_rows): seq_len unless the context was created with max_rows"""
        n = C.c_int(0)
        _chk(self.L.lnb_ctx_max_rows(self.h, C.byref(n)))
        return n.value

    def set_mode(self, mode):
        """MODE_EXACT (default, bit-identical to the reference) or MODE_FAST (split-K / bf16-MFMA tolerance mode)"""
        _chk(self.L.lnb_ctx_set_mode(self.h, {"exact": 0, "fast": 1}.get(mode, mode)))
        return self

    def set_schedule(self, sched):
        """'latency' (default: one generation owns the chip) or 'throughput' (several contexts in flight on one GPU share the CUs); same bits"""
        _chk(self.L.lnb_ctx_set_schedule(self.h, {"latency": 0, "throughput": 1}.get(sched, sched)))
        return self

    def set_attention(self, long_threshold=-1, force_zseq=0):
        """contexts above long_threshold use the long-context decode attention; force_zseq: always walk the serial f64 sum"""
        _chk(self.L.lnb_ctx_set_attention(self.h, long_threshold, force_zseq))
        return self

    def zseq_count(self):
        n = C.c_int(0)
        _chk(self.L.lnb_ctx_zseq_count(self.h, C.byref(n)))
        return n.value

    def norm_fallbacks(self):
        """fused-RMSNorm rows (decode) that left the branch-free item walk for the record walk since the context was created"""
        n = C.c_int(0)
        _chk(self.L.lnb_ctx_norm_fallbacks(self.h, C.byref(n)))
        return n.value

    def prefill_attention_form(self):
        """3: the last multi-row call ran attn_mfma3_kernel (scores once), 1: attn_mfma_kernel (scores twice: scratch refused), 0: neither"""
        n = C.c_int(0)
        _chk(self.L.lnb_ctx_prefill_attention_form(self.h, C.byref(n)))
        return n.value

    def attention(self, layer, q_u16, start_pos):
        """lnb_ctx_attention (a test aid): the attention launch of `layer` on q_u16 [S, n_heads, head_dim] over the context's K / V rows -> uint16 [S, n_heads, head_dim]"""
        q = np.ascontiguousarray(q_u16, dtype=np.uint16)
        assert q.ndim == 3
        out = np.empty_like(q)
        _chk(self.L.lnb_ctx_attention(self.h, layer, q.ctypes.data, q.shape[0], start_pos, out.ctypes.data))
        return out

    def Forward(self, tokens, start_pos, want_logits=True):
        """(*LlamaTransformer).Forward (llamatransformer.go:145-180) -> (logits f32 [S,V] | None, argmax of last row)."""
        tok = np.ascontiguousarray(tokens, dtype=np.int32)
        S, V = tok.size, self.t.args.vocab_size
        logits = np.empty((S, V), dtype=np.float32) if want_logits else None
        am = C.c_int32(-2)
        _chk(self.L.lnb_forward(self.h, _p(tok), S, start_pos, _p(logits) if want_logits else None, C.byref(am)))
        return logits, am.value

    def ForwardAppend(self, tokens, start_pos, want_logits=True):
        """Extend the context by len(tokens) rows at ANY start_pos under the true causal mask (lnb_forward_append): row i is the one-token
        Forward at start_pos + i, bit for bit -> (logits f32 [S,V] | None, argmax of last row)."""
        tok = np.ascontiguousarray(tokens, dtype=np.int32)
        S, V = tok.size, self.t.args.vocab_size
        logits = np.empty((S, V), dtype=np.float32) if want_logits else None
        am = C.c_int32(-2)
        _chk(self.L.lnb_forward_append(self.h, _p(tok) if S else None, S, start_pos, _p(logits) if want_logits and S else None, C.byref(am)))
        return logits, am.value

    def decode_greedy(self, token, start_pos, n_steps):
        out = np.empty(n_steps, dtype=np.int32)
        ms = C.c_float(0)
        _chk(self.L.lnb_decode_greedy(self.h, int(token), start_pos, n_steps, _p(out), C.byref(ms)))
        return out, ms.value

    def profile_kernel(self, which, pos, iters):
        ms = C.c_float(0)
        _chk(self.L.lnb_profile_kernel(self.h, which, pos, iters, C.byref(ms)))
        return ms.value

    def profile_ffn_pair(self, pos, iters, w2_delay_us=0, w2_lds_pad=0):
        """gate|up and down kernels of a block on two streams, w2 launched w2_delay_us behind w1|w3 (lnb_profile_ffn_pair): ms per pair"""
        ms = C.c_float(0)
        _chk(self.L.lnb_profile_ffn_pair(self.h, pos, iters, w2_delay_us, w2_lds_pad, C.byref(ms)))
        return ms.value

    def profile_kernel_stamps(self, which, pos):
        """in-kernel cycle stamps of one launch of a GEMV class -> (float64 [8 waves, 16], wall clock kHz); layout: include/lnb.h"""
        out = np.zeros((8, 16), dtype=np.float64)
        khz = C.c_int(0)
        _chk(self.L.lnb_profile_kernel_stamps(self.h, which, pos, _p(out), C.byref(khz)))
        return out, khz.value

    def set_stop_ids(self, ids):
        """model.StopTokenIds on the device (inference.go:233-252)"""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        _chk(self.L.lnb_ctx_set_stop_ids(self.h, _p(a) if a.size else None, int(a.size)))
        return self

    def decode_greedy_until(self, token, start_pos, max_steps):
        """-> (tokens generated: max_steps of them unless a stop id ended the run, finished flag, device ms)"""
        out = np.empty(max_steps, dtype=np.int32)
        ms, n, fin = C.c_float(0), C.c_int(0), C.c_int(0)
        _chk(self.L.lnb_decode_greedy_until(self.h, int(token), start_pos, max_steps, _p(out), C.byref(n), C.byref(fin), C.byref(ms)))
        return out[:n.value].copy(), bool(fin.value), ms.value

    def decode_sample_until(self, sampler, token, start_pos, max_steps):
        """decode_greedy_until with the sampler's token in place of the argmax (lnb_decode_sample_until): sampler = a Sampler or (temperature, top_k, top_p, seed)
        -> (tokens generated, finished flag, device ms)"""
        s = _samplers([sampler], 1)
        out = np.empty(max(int(max_steps), 0), dtype=np.int32)
        ms, n, fin = C.c_float(0), C.c_int(0), C.c_int(0)
        _chk(self.L.lnb_decode_sample_until(self.h, s, int(token), start_pos, max_steps, _p(out), C.byref(n), C.byref(fin), C.byref(ms)))
        return out[:n.value].copy(), bool(fin.value), ms.value

    def profile_sample(self, sampler, pos, iters):
        """average device ms of the step's token launch alone: sample_kernel with this sampler, argmax_kernel with None (lnb_profile_sample)"""
        ms = C.c_float(0)
        _chk(self.L.lnb_profile_sample(self.h, None if sampler is None else _samplers([sampler], 1), pos, iters, C.byref(ms)))
        return ms.value

    def set_token_probs(self, k):
        """record the top k token probabilities (0..MAX_TOP_K; 0 = off, the default) of every token the greedy loops generate (include/lnb.h)"""
        _chk(self.L.lnb_ctx_set_token_probs(self.h, int(k)))
        self.top_k = int(k)
        return self

    def token_probs(self, n, first=0):
        """records [first, first + n) of the last decode call: (ids int32 [n, k], logits f32 [n, k], probs f32 [n, k], log_z f64 [n]);
        ids[:, 0] are the generated tokens.  k is the top_k that call ran with (the current setting: changing it drops the records)."""
        k = getattr(self, "top_k", 0)
        ids = np.empty((n, max(k, 1)), dtype=np.int32)
        lg = np.empty((n, max(k, 1)), dtype=np.float32)
        pr = np.empty((n, max(k, 1)), dtype=np.float32)
        lz = np.empty(max(n, 1), dtype=np.float64)
        _chk(self.L.lnb_ctx_read_token_probs(self.h, int(first), int(n), _p(ids), _p(lg), _p(pr), _p(lz)))
        return ids[:, :k], lg[:, :k], pr[:, :k], lz[:n]

    def set_draft(self, max_draft, ngram_min=1, ngram_max=4, corpus=()):
        """n-gram drafts for decode_speculative_until: up to max_draft (0..MAX_DRAFT; 0 = off, the default) tokens per pass, looked up with
        n-grams of ngram_min..ngram_max tokens in the running text, then in corpus (copied to the device)"""
        a = np.ascontiguousarray(corpus, dtype=np.int32)
        _chk(self.L.lnb_ctx_set_draft(self.h, int(max_draft), int(ngram_min), int(ngram_max), _p(a) if a.size else None, int(a.size)))
        return self

    def set_batched_attention(self, long_threshold=-1, force_zseq=0):
        """attention form of decode_speculative_until's verify passes: past long_threshold positions (default: never, unless the context is
        beyond the one-workgroup kernels' reach) the long-context kernels; force_zseq: always walk the serial f64 sum.  Same bits."""
        _chk(self.L.lnb_ctx_set_batched_attention(self.h, int(long_threshold), int(force_zseq)))
        return self

    def verify_attention_form(self):
        """0: the last verify pass ran the one-workgroup attention kernels, 1: the long-context pair, 2: the multi-row long-context pair"""
        n = C.c_int(0)
        _chk(self.L.lnb_ctx_verify_attention_form(self.h, C.byref(n)))
        return n.value

    def set_rows_attention(self, long_threshold=-1, flags=0):
        """multi-row long-context attention (lnb_ctx_set_rows_attention): appends of 2..15 rows (any row count at head_dim 32) past long_threshold
        positions run it (default: what the row-per-workgroup kernel cannot stage; 0: all of them).  flags bit 0: every row walks the serial
        f64 sum; bit 1: the verify passes of decode_speculative_until run it wherever they would run the long form.  Same bits."""
        _chk(self.L.lnb_ctx_set_rows_attention(self.h, int(long_threshold), int(flags)))
        return self

    def append_attention_form(self):
        """the attention of the last forward_append / score_append: 0 none yet or one row, 1 row-per-workgroup kernel, 2 matrix-core kernel,
        3 one-token steps inside the call, 4 the multi-row long-context pair"""
        n = C.c_int(0)
        _chk(self.L.lnb_ctx_append_attention_form(self.h, C.byref(n)))
        return n.value

    def decode_speculative_until(self, history, token, start_pos, max_steps):
        """decode_greedy_until with drafts verified in batched passes (lnb_decode_speculative_until): the same tokens, logits and KV rows.
        history: the tokens before `token` (e.g. the prompt) -> (tokens, finished flag, stats dict, device ms)"""
        h = np.ascontiguousarray(history, dtype=np.int32)
        out = np.empty(max_steps, dtype=np.int32)
        ms, n, fin, st = C.c_float(0), C.c_int(0), C.c_int(0), SpecStats()
        _chk(self.L.lnb_decode_speculative_until(self.h, _p(h) if h.size else None, int(h.size), int(token), start_pos, max_steps, _p(out),
                                                 C.byref(n), C.byref(fin), C.byref(st), C.byref(ms)))
        return out[:n.value].copy(), bool(fin.value), st.as_dict(), ms.value

    def decode_speculative_sample_until(self, sampler, history, token, start_pos, max_steps):
        """decode_sample_until with drafts verified in batched passes (lnb_decode_speculative_sample_until): the same tokens and KV rows, because the
        sampler's draw depends on (seed, position) only.  sampler = a Sampler or (temperature, top_k, top_p, seed); None reaches the library as NULL
        -> (tokens, finished flag, stats dict, device ms)"""
        s = None if sampler is None else _samplers([sampler], 1)
        h = np.ascontiguousarray(history, dtype=np.int32)
        out = np.empty(max(int(max_steps), 0), dtype=np.int32)
        ms, n, fin, st = C.c_float(0), C.c_int(0), C.c_int(0), SpecStats()
        _chk(self.L.lnb_decode_speculative_sample_until(self.h, s, _p(h) if h.size else None, int(h.size), int(token), start_pos, max_steps, _p(out),
                                                        C.byref(n), C.byref(fin), C.byref(st), C.byref(ms)))
        return out[:n.value].copy(), bool(fin.value), st.as_dict(), ms.value

    def token_prob_walks(self):
        """rows of this context (decode steps, scored rows) whose probabilities walked the reference's serial sum"""
        n = C.c_int(0)
        _chk(self.L.lnb_ctx_token_prob_walks(self.h, C.byref(n)))
        return n.value

    def score(self, tokens, start_pos, targets):
        """Forward(tokens, start_pos) reporting, per row, the target's logit and probability and ln Z instead of the logits (lnb_forward_score):
        -> (target_logit f32 [S], target_prob f32 [S], log_z f64 [S], argmax of the last row).  targets[i] < 0: NaN for that row."""
        tok = np.ascontiguousarray(tokens, dtype=np.int32)
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        S = tok.size
        if tg.size != S:
            raise LnbError("score: %d targets for %d tokens" % (tg.size, S))
        tl = np.empty(max(S, 1), dtype=np.float32); tp = np.empty(max(S, 1), dtype=np.float32); lz = np.empty(max(S, 1), dtype=np.float64)
        am = C.c_int32(-2)
        _chk(self.L.lnb_forward_score(self.h, _p(tok), S, start_pos, _p(tg), _p(tl), _p(tp), _p(lz), C.byref(am)))
        return tl[:S], tp[:S], lz[:S], am.value

    def score_append(self, tokens, start_pos, targets):
        """score() of rows appended at any start_pos under the true causal mask (lnb_forward_score_append): the bits of one-row score calls
        -> (target_logit f32 [S], target_prob f32 [S], log_z f64 [S], argmax of the last row)"""
        tok = np.ascontiguousarray(tokens, dtype=np.int32)
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        S = tok.size
        if tg.size != S:
            raise LnbError("score_append: %d targets for %d tokens" % (tg.size, S))
        tl = np.empty(max(S, 1), dtype=np.float32); tp = np.empty(max(S, 1), dtype=np.float32); lz = np.empty(max(S, 1), dtype=np.float64)
        am = C.c_int32(-2)
        _chk(self.L.lnb_forward_score_append(self.h, _p(tok) if S else None, S, start_pos, _p(tg), _p(tl), _p(tp), _p(lz), C.byref(am)))
        return tl[:S], tp[:S], lz[:S], am.value

    def ForkPrefix(self, dsts, n_pos):
        """copy this context's KV rows [0, n_pos) of every layer into the contexts `dsts` (1..MAX_FORK, same transformer, any capacities) in one
        kernel launch (lnb_ctx_fork).  Nothing else moves: continue each destination at n_pos."""
        dsts = list(dsts)
        arr = (C.c_void_p * max(len(dsts), 1))(*[d.h for d in dsts])
        _chk(self.L.lnb_ctx_fork(self.h, int(n_pos), arr, len(dsts)))
        return self

    def SavePrefix(self, n_pos):
        """the KV rows [0, n_pos) as a capacity-independent blob (lnb_ctx_save_prefix; layout in lnb.h) -> numpy uint8 array"""
        n = self.L.lnb_ctx_prefix_bytes(self.h, int(n_pos))
        if n < 0:
            _chk(-1)
        blob = np.empty(n, dtype=np.uint8)
        _chk(self.L.lnb_ctx_save_prefix(self.h, int(n_pos), _p(blob), n))
        return blob

    def LoadPrefix(self, blob):
        """write a saved prefix into rows [0, n_pos) of this context (lnb_ctx_load_prefix) -> n_pos.  The blob carries no model identity."""
        b = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, dtype=np.uint8)
        n = C.c_int(-1)
        _chk(self.L.lnb_ctx_load_prefix(self.h, _p(b) if b.size else None, int(b.size), C.byref(n)))
        return n.value

    def CacheK(self, layer):
        return self._kv(layer, 0)

    def CacheV(self, layer):
        return self._kv(layer, 1)

    def _kv(self, layer, which):
        a = self.t.args
        out = np.empty((self.SequenceLength, a.n_kv_heads, self.t.head_dim), dtype=np.uint16)
        _chk(self.L.lnb_ctx_read_kv(self.h, layer, which, _p(out)))
        return out

    def reset(self):
        _chk(self.L.lnb_ctx_reset(self.h))

    def close(self):
        if self.h:
            _chk(self.L.lnb_ctx_destroy(self.h))             # refused while a live Batch holds the context: the handle (and the device memory) stays
            self.h = C.c_void_p()


def ForwardAppendMany(ctxs, token_lists, start_pos, want_logits=True):
    """Extend the contexts `ctxs` (1..128, one transformer, any capacities) in ONE call: context s takes token_lists[s] at start_pos[s], the rows of
    all of them packed into batched passes of up to 128 rows over the weights (lnb_forward_append_many).  Every context's KV rows, logits and
    last-row argmax are the bits of its own ForwardAppend -> (list of per-context logits f32 [rows_s, V] | None, int32 argmax [n])."""
    ctxs = list(ctxs)
    lists = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in token_lists]
    if not ctxs or len(lists) != len(ctxs) or len(start_pos) != len(ctxs):
        raise LnbError("ForwardAppendMany: %d contexts, %d token lists, %d start positions" % (len(ctxs), len(lists), len(start_pos)))
    L, V = ctxs[0].L, ctxs[0].t.args.vocab_size
    flat = np.ascontiguousarray(np.concatenate(lists), dtype=np.int32)
    rows = np.array([t.size for t in lists], dtype=np.int32)
    pos = np.ascontiguousarray(start_pos, dtype=np.int32)
    arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    logits = np.empty((max(flat.size, 1), V), dtype=np.float32) if want_logits else None
    am = np.full(len(ctxs), -2, dtype=np.int32)
    _chk(L.lnb_forward_append_many(arr, len(ctxs), _p(flat), _p(rows), _p(pos), _p(logits) if want_logits else None, _p(am)))
    if not want_logits:
        return None, am
    ends = np.cumsum(rows)
    return [logits[e - r:e] for e, r in zip(ends, rows)], am


def DecodeSpeculativeSampleMany(ctxs, samplers, histories, tokens, start_pos, max_steps, col_budget=0):
    """DecodeSpeculativeMany with one sampler per context (lnb_decode_speculative_sample_many): every context's tokens, finished flag and KV rows are the
    bits of its own decode_sample_until; a temperature-0 member is greedy -> the same tuple"""
    ctxs = list(ctxs)
    ss = None if samplers is None else _samplers(samplers, len(ctxs))
    return _decode_speculative_many(ctxs, histories, tokens, start_pos, max_steps, col_budget, True, ss)


def DecodeSpeculativeMany(ctxs, histories, tokens, start_pos, max_steps, col_budget=0):
    """decode_greedy_until of the contexts `ctxs` (1..128, one transformer) together, every context drafting for itself with its own set_draft
    settings and ONE batched pass over the weights verifying all of them (lnb_decode_speculative_many).  Context s continues from tokens[s] at
    start_pos[s] (histories[s]: the tokens before it; start_pos[s] < 0: skipped); col_budget: columns per pass, 0 = 16 * ceil(n / 16).  Every
    context's tokens, finished flag and KV rows are the bits of its own decode_greedy_until
    -> (list of int32 token arrays, list of finished flags, list of stats dicts, info dict, device ms)"""
    return _decode_speculative_many(ctxs, histories, tokens, start_pos, max_steps, col_budget, False, None)


def _decode_speculative_many(ctxs, histories, tokens, start_pos, max_steps, col_budget, sample, ss):
    ctxs = list(ctxs)
    n = len(ctxs)
    hist = [np.ascontiguousarray(h, dtype=np.int32).reshape(-1) for h in histories]
    if not ctxs or len(hist) != n or len(tokens) != n or len(start_pos) != n:
        raise LnbError("DecodeSpeculativeMany: %d contexts, %d histories, %d tokens, %d start positions" % (n, len(hist), len(tokens), len(start_pos)))
    L = ctxs[0].L
    arr = (C.c_void_p * n)(*[c.h for c in ctxs])
    harr = (C.c_void_p * n)(*[h.ctypes.data if h.size else None for h in hist])
    nh = np.array([h.size for h in hist], dtype=np.int32)
    tok = np.ascontiguousarray(tokens, dtype=np.int32)
    pos = np.ascontiguousarray(start_pos, dtype=np.int32)
    out = np.zeros((n, max(int(max_steps), 1)), dtype=np.int32)
    ng = np.zeros(n, dtype=np.int32); fin = np.zeros(n, dtype=np.int32)
    st = (SpecStats * n)(); info = SpecManyInfo(); ms = C.c_float(0)
    if sample:
        _chk(L.lnb_decode_speculative_sample_many(arr, n, ss, harr, _p(nh), _p(tok), _p(pos), int(max_steps), int(col_budget), _p(out), _p(ng), _p(fin),
                                                  st, C.byref(info), C.byref(ms)))
    else:
        _chk(L.lnb_decode_speculative_many(arr, n, harr, _p(nh), _p(tok), _p(pos), int(max_steps), int(col_budget), _p(out), _p(ng), _p(fin),
                                           st, C.byref(info), C.byref(ms)))
    return ([out[s, :ng[s]].copy() for s in range(n)], [bool(f) for f in fin], [st[s].as_dict() for s in range(n)], info.as_dict(), ms.value)


class Batch:
    """1..128 InferenceContexts of one transformer decoded together: one pass over the weights per step for all of them, every sequence
    bit-identical to its single-sequence run (lnb_batch_*).  The contexts keep their own caches and positions."""

    def __init__(self, contexts):
        self.ctxs = list(contexts)
        self.L = self.ctxs[0].L
        arr = (C.c_void_p * len(self.ctxs))(*[c.h for c in self.ctxs])
        self.h = C.c_void_p()
        _chk(self.L.lnb_batch_create(arr, len(self.ctxs), C.byref(self.h)))

    def decode(self, tokens, start_pos, n_steps):
        """sequence s continues from tokens[s] at position start_pos[s]; -> (int32 [n, n_steps], device ms of the n_steps)"""
        n = len(self.ctxs)
        tok = np.ascontiguousarray(tokens, dtype=np.int32); pos = np.ascontiguousarray(start_pos, dtype=np.int32)
        assert tok.size == n and pos.size == n
        out = np.empty((n, n_steps), dtype=np.int32)
        ms = C.c_float(0)
        _chk(self.L.lnb_batch_decode(self.h, tok.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.POINTER(C.c_int32)), n_steps, _p(out), C.byref(ms)))
        return out, ms.value

    def decode_until(self, tokens, start_pos, max_steps):
        """decode with the member contexts' stop ids: -> (list of per-sequence token arrays (their valid lengths differ), device ms)"""
        n = len(self.ctxs)
        tok = np.ascontiguousarray(tokens, dtype=np.int32); pos = np.ascontiguousarray(start_pos, dtype=np.int32)
        out = np.empty((n, max_steps), dtype=np.int32)
        cnt = np.zeros(n, dtype=np.int32)
        ms = C.c_float(0)
        fin = np.zeros(n, dtype=np.int32)
        _chk(self.L.lnb_batch_decode_until(self.h, tok.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.POINTER(C.c_int32)), max_steps, _p(out), _p(cnt), _p(fin), C.byref(ms)))
        self.finished = [bool(f) for f in fin]               # per sequence: a stop id ended it (start_pos[s] < 0 keeps an ended sequence frozen in the next chunk)
        return [out[s, :cnt[s]].copy() for s in range(n)], ms.value

    def decode_sample_until(self, samplers, tokens, start_pos, max_steps):
        """decode_until with one sampler per member (lnb_batch_decode_sample_until; a temperature-0 member is greedy): -> (per-sequence token arrays, device ms)"""
        n = len(self.ctxs)
        ss = _samplers(samplers, n)
        tok = np.ascontiguousarray(tokens, dtype=np.int32); pos = np.ascontiguousarray(start_pos, dtype=np.int32)
        assert tok.size == n and pos.size == n
        out = np.empty((n, max(int(max_steps), 0)), dtype=np.int32)
        cnt = np.zeros(n, dtype=np.int32); fin = np.zeros(n, dtype=np.int32)
        ms = C.c_float(0)
        _chk(self.L.lnb_batch_decode_sample_until(self.h, ss, tok.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.POINTER(C.c_int32)), max_steps, _p(out), _p(cnt),
                                                  _p(fin), C.byref(ms)))
        self.finished = [bool(f) for f in fin]
        return [out[s, :cnt[s]].copy() for s in range(n)], ms.value

    def profile_kernel(self, which, pos, iters):
        ms = C.c_float(0)
        _chk(self.L.lnb_batch_profile_kernel(self.h, which, pos, iters, C.byref(ms)))
        return ms.value

    def set_attention(self, long_threshold=-1, force_zseq=0):
        """calls whose largest start position + 1 exceeds long_threshold run the long-context attention (default: never, unless a member is
        beyond the one-workgroup kernels' reach); force_zseq: every (sequence, head) walks the serial f64 sum.  Same bits either way."""
        _chk(self.L.lnb_batch_set_attention(self.h, int(long_threshold), int(force_zseq)))
        return self

    def attention_form(self):
        """0: the last call of this batch ran the one-workgroup attention kernels, 1: the long-context pair"""
        n = C.c_int(0)
        _chk(self.L.lnb_batch_attention_form(self.h, C.byref(n)))
        return n.value

    def set_state(self, tokens, start_pos):
        """positions (and optionally next input tokens) of the sequences before a run of Pipeline.tick_batch steps"""
        pos = np.ascontiguousarray(start_pos, dtype=np.int32)
        tok = None if tokens is None else np.ascontiguousarray(tokens, dtype=np.int32)
        _chk(self.L.lnb_batch_set_state(self.h, None if tok is None else tok.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.POINTER(C.c_int32))))
        return self

    def boundary_ptr(self, which):
        """device address of what a batched tick exchanges: 0 = hidden states [n, dim] bf16 (stage input / output), 1 = the n int32 token words"""
        ptr = self.L.lnb_batch_boundary_ptr(self.h, which)
        if not ptr:
            _chk(-1)
        return int(ptr)

    def check_error(self):
        """after Pipeline.sync(): raises if a pipeline tick of this batch met a token outside the vocabulary / an all-NaN logits row"""
        _chk(self.L.lnb_batch_check_error(self.h))
        return self

    def close(self):
        if self.h:
            self.L.lnb_batch_destroy(self.h)
            self.h = C.c_void_p()


class Pipeline:
    """One rank of the layer-sharded pipeline behind the C ABI (lnb_pipeline_*): RCCL send / recv straight from / into the stage's
    device buffers, stage steps as captured graphs, nothing synchronised per tick."""

    def __init__(self, transformer, rank, world, unique_id=None, loopback_group=None, host_transport=False):
        """unique_id: rank 0's 128 RCCL id bytes (world > 1); loopback_group: a name -- the in-process transport instead of RCCL;
        host_transport: no transport at all -- ticks only `run`, the caller moves the boundary buffers (pipeline.run_ticks_batched_torch)"""
        self.L, self.rank, self.world = transformer.L, rank, world
        self.h = C.c_void_p()
        if host_transport:
            _chk(self.L.lnb_pipeline_init_host(transformer.h, rank, world, C.byref(self.h)))
            return
        if loopback_group is not None:
            _chk(self.L.lnb_pipeline_init_loopback(transformer.h, rank, world, loopback_group.encode(), C.byref(self.h)))
            return
        idp = C.c_char_p(bytes(unique_id)) if unique_id is not None else None
        _chk(self.L.lnb_pipeline_init(transformer.h, rank, world, idp, C.byref(self.h)))

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _chk(lib().lnb_pipeline_unique_id(buf))
        return bytes(buf.raw)

    def tick(self, run=None, run_rows=0, run_pos=0, run_tokens=None, send=None, send_rows=0, recv=None, recv_rows=0):
        slot = C.c_int(-1)
        tok = None if run_tokens is None else np.ascontiguousarray(run_tokens, dtype=np.int32)
        _chk(self.L.lnb_pipeline_tick(self.h, run.h if run else None, run_rows, run_pos, _p(tok) if tok is not None else None,
                                      send.h if send else None, send_rows, recv.h if recv else None, recv_rows, C.byref(slot)))
        return slot.value

    def tick_batch(self, run=None, send=None, recv=None):
        """the tick with a Batch as the unit: one pass over the stage's weights for all its sequences; -> first token-log slot (last rank)"""
        slot = C.c_int(-1)
        _chk(self.L.lnb_pipeline_tick_batch(self.h, run.h if run else None, send.h if send else None, recv.h if recv else None, C.byref(slot)))
        return slot.value

    def sync(self):
        _chk(self.L.lnb_pipeline_sync(self.h))

    def comm_count(self):
        """ranks the exchange spans, as the transport itself reports it (ncclCommCount)"""
        n = C.c_int(0)
        _chk(self.L.lnb_pipeline_comm_count(self.h, C.byref(n)))
        return n.value

    def read_tokens(self, first_slot, n):
        out = np.empty(n, dtype=np.int32)
        _chk(self.L.lnb_pipeline_read_tokens(self.h, first_slot, n, _p(out)))
        return out

    def close(self):
        if self.h:
            self.L.lnb_pipeline_destroy(self.h)
            self.h = C.c_void_p()


class InferenceEngine:
    """Greedy generation loop of src/inference/inference.go:173-254 over the device path:
    prefill(prompt) through Forward, then the decode steps as hipGraph replays on the device.
    prefill_chunk: 0 = the prompt goes in one Forward; n > 0 = it is ingested as ForwardAppend calls of at most n rows (the same tokens out:
    every row is the same one-token step either way; the prefill attention's score scratch is then sized for n rows instead of the prompt).
    long_context: the generation's context is a long one (lnb_ctx_create_long, up to MAX_SEQ_LEN positions) whose activation buffers hold
    prefill_chunk rows, or the prompt when the chunk is 0."""

    def __init__(self, transformer, seq_len, stop_token_ids=(), prefill_chunk=0, long_context=False, sampler=None, draft=None):
        if int(prefill_chunk) < 0:
            raise LnbError("prefill_chunk must be 0 (one Forward) or a positive row count")
        self.t, self.seq_len, self.stop, self.prefill_chunk = transformer, seq_len, set(stop_token_ids), int(prefill_chunk)
        self.long_context = bool(long_context)
        self.sampler = sampler                               # None: greedy.  A Sampler (or its tuple): EVERY generated token is sampled, the prompt's own next token included
        if draft is not None and len(tuple(draft)) != 3:
            raise LnbError("draft must be None or (max_draft, ngram_min, ngram_max)")
        self.draft = None if draft is None else tuple(int(v) for v in draft)      # None: one pass per token.  Else the speculative loop drafts from the running text: the same tokens

    def GenerateTokens(self, prompt_tokens, max_new=None):
        prompt = list(prompt_tokens)
        if len(prompt) >= self.seq_len:
            raise LnbError("context SequenceLength %d must be higher than prompt tokens length %d" % (self.seq_len, len(prompt)))
        if self.long_context:
            ctx = InferenceContext(self.t, self.seq_len, max_rows=self.prefill_chunk or max(len(prompt), 1), long_context=True)
        else:
            ctx = InferenceContext(self.t, self.seq_len)
        try:
            n_new = self.seq_len - len(prompt) if max_new is None else min(max_new, self.seq_len - len(prompt))
            if self.prefill_chunk > 0:
                for p0 in range(0, len(prompt), self.prefill_chunk):
                    _, first = ctx.ForwardAppend(prompt[p0:p0 + self.prefill_chunk], p0, want_logits=False)
            else:
                _, first = ctx.Forward(prompt, 0, want_logits=False)
            if self.sampler is not None:
                # the prompt's next token by the same rule, at the position of the row's input token: the last prompt row once more as a one-token step
                # (the same bits into the same KV row) for its logits, then sample_kernel on that row
                row, _ = ctx.ForwardAppend(prompt[-1:], len(prompt) - 1, want_logits=True)
                row16 = (np.ascontiguousarray(row[0], dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)
                first = int(op_sample(row16, [self.sampler], [len(prompt) - 1], want_info=False, device=self.t.device)[0][0])
                if first < 0:
                    raise LnbError("the prompt's last logits row has no candidate to sample (all NaN or -inf)")
            out = [first]
            if first not in self.stop and n_new > 1:
                if self.draft is not None:
                    ctx.set_draft(*self.draft)
                    if self.sampler is None:
                        more, _, _, _ = ctx.decode_speculative_until(prompt, first, len(prompt), n_new - 1)
                    else:
                        more, _, _, _ = ctx.decode_speculative_sample_until(self.sampler, prompt, first, len(prompt), n_new - 1)
                elif self.sampler is None:
                    more, _ = ctx.decode_greedy(first, len(prompt), n_new - 1)
                else:
                    more, _, _ = ctx.decode_sample_until(self.sampler, first, len(prompt), n_new - 1)
                for t in more:
                    out.append(int(t))
                    if int(t) in self.stop:
                        break
            return out
        finally:
            ctx.close()


def op_linear(x_u16, w_u16, rw=0, device=0):
    x = np.ascontiguousarray(x_u16, dtype=np.uint16)
    w = np.ascontiguousarray(w_u16, dtype=np.uint16)
    rows, k = x.shape
    n = w.shape[0]
    y = np.empty((rows, n), dtype=np.uint16)
    _chk(lib().lnb_op_linear(device, _p(x), _p(w), _p(y), rows, n, k, rw))
    return y


def op_rmsnorm_linear(x_u16, norm_w_u16, eps, w_u16, rw=0, device=0):
    x = np.ascontiguousarray(x_u16, dtype=np.uint16)
    w = np.ascontiguousarray(w_u16, dtype=np.uint16)
    nw = np.ascontiguousarray(norm_w_u16, dtype=np.uint16)
    rows, k = x.shape
    n = w.shape[0]
    y = np.empty((rows, n), dtype=np.uint16)
    _chk(lib().lnb_op_rmsnorm_linear(device, _p(x), _p(nw), np.float32(eps), _p(w), _p(y), rows, n, k, rw))
    return y


def op_linear_mode(x_u16, w_u16, mode, norm_w_u16=None, eps=1e-5, rw=0, device=0):
    x = np.ascontiguousarray(x_u16, dtype=np.uint16)
    w = np.ascontiguousarray(w_u16, dtype=np.uint16)
    nw = None if norm_w_u16 is None else np.ascontiguousarray(norm_w_u16, dtype=np.uint16)
    rows, k = x.shape
    n = w.shape[0]
    y = np.empty((rows, n), dtype=np.uint16)
    _chk(lib().lnb_op_linear_mode(device, _p(x), None if nw is None else _p(nw), np.float32(eps), _p(w), _p(y), rows, n, k, rw, mode))
    return y


def op_argmax(logits_u16, device=0):
    a = np.ascontiguousarray(logits_u16, dtype=np.uint16).ravel()
    out = C.c_int32(-2)
    _chk(lib().lnb_op_argmax(device, _p(a), a.size, C.byref(out)))
    return out.value


def op_sample(logits_u16, samplers, pos, draws=None, want_info=True, device=0):
    """sample_kernel on rows of bf16 logits [rows, V] (lnb_op_sample): row i with samplers[i] at position pos[i], or with u = draws[i] given instead of derived
    -> (tokens int32 [rows], list of info dicts or None)"""
    a = np.ascontiguousarray(logits_u16, dtype=np.uint16)
    if a.ndim == 1:
        a = a[None, :]
    rows, V = a.shape
    ss = _samplers(samplers, rows)
    p = np.ascontiguousarray(pos, dtype=np.int32)
    u = None if draws is None else np.array([int(d) & 0xFFFFFFFFFFFFFFFF for d in draws], dtype=np.uint64)
    if p.size != rows or (u is not None and u.size != rows):
        raise LnbError("%d rows, %d positions%s" % (rows, p.size, "" if u is None else ", %d draws" % u.size))
    tok = np.full(rows, -2, dtype=np.int32)
    info = (SampleInfo * rows)() if want_info else None
    _chk(lib().lnb_op_sample(device, _p(a), rows, V, ss, _p(p), None if u is None else _p(u), _p(tok), info))
    return tok, ([i.as_dict() for i in info] if want_info else None)


def op_token_probs(logits_u16, top_k, targets=None, force_serial=False, device=0):
    """token_probs_kernel on rows of bf16 logits [rows, V] (lnb_op_token_probs) -> dict of ids / logits / probs [rows, k], log_z [rows],
    target_prob [rows] (with targets), serial_walks"""
    a = np.ascontiguousarray(logits_u16, dtype=np.uint16)
    if a.ndim == 1:
        a = a[None, :]
    rows, V = a.shape
    k = int(top_k)
    ids = np.empty((rows, max(k, 1)), dtype=np.int32)
    lg = np.empty((rows, max(k, 1)), dtype=np.float32)
    pr = np.empty((rows, max(k, 1)), dtype=np.float32)
    lz = np.empty(rows, dtype=np.float64)
    tg = None if targets is None else np.ascontiguousarray(targets, dtype=np.int32)
    tp = np.empty(rows, dtype=np.float32)
    walks = C.c_int(0)
    _chk(lib().lnb_op_token_probs(device, _p(a), rows, V, k, None if tg is None else _p(tg), 1 if force_serial else 0,
                                  _p(ids), _p(lg), _p(pr), _p(tp) if tg is not None else None, _p(lz), C.byref(walks)))
    out = dict(ids=ids[:, :k], logits=lg[:, :k], probs=pr[:, :k], log_z=lz, serial_walks=walks.value)
    if tg is not None:
        out["target_prob"] = tp
    return out


def op_ngram_draft(text, corpus=(), ngram_min=1, ngram_max=4, max_draft=MAX_DRAFT, device=0):
    """ngram_draft_kernel on host arrays (lnb_op_ngram_draft): the draft that follows `text` -> int32 array"""
    t = np.ascontiguousarray(text, dtype=np.int32)
    c = np.ascontiguousarray(corpus, dtype=np.int32)
    out = np.empty(max(int(max_draft), 1), dtype=np.int32)
    n = C.c_int(0)
    _chk(lib().lnb_op_ngram_draft(device, _p(t) if t.size else None, int(t.size), _p(c) if c.size else None, int(c.size),
                                  int(ngram_min), int(ngram_max), int(max_draft), _p(out), C.byref(n)))
    return out[:n.value].copy()


def op_spec_sample_accept(logits_u16, sampler, pos0, col_tokens, stop_ids=(), device=0):
    """spec_sample_commit_kernel on host rows (lnb_op_spec_sample_accept): column i of a verify pass has logits row i, took col_tokens[i] and sits at pos0 + i
    -> (the tokens the pass emits as an int32 array, finished flag)"""
    a = np.ascontiguousarray(logits_u16, dtype=np.uint16)
    w, V = a.shape
    ct = np.ascontiguousarray(col_tokens, dtype=np.int32)
    if ct.size != w:
        raise LnbError("%d column tokens for %d rows" % (ct.size, w))
    stop = np.ascontiguousarray(stop_ids, dtype=np.int32)
    out = np.zeros(w, dtype=np.int32)
    n, fin = C.c_int(0), C.c_int(0)
    _chk(lib().lnb_op_spec_sample_accept(device, _p(a), w, V, _samplers([sampler], 1), int(pos0), _p(ct), _p(stop) if stop.size else None, int(stop.size),
                                         _p(out), C.byref(n), C.byref(fin)))
    return out[:n.value].copy(), bool(fin.value)


def op_exp_table(divisor=1.0, device=0):
    """out[s] = exp(float64(trunc_bf16(float32(bf16 s) / divisor))) for all 65536 raw scores, as the attention kernels evaluate it (lnb_op_exp_table)"""
    out = np.empty(65536, dtype=np.float64)
    _chk(lib().lnb_op_exp_table(device, C.c_float(divisor), _p(out)))
    return out


_M64 = (1 << 64) - 1


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def synth_tokens(seed, n, vocab):
    """Synthetic prompt of DESIGN.md ("Synthetic weights"): tok[i] = splitmix64(seed ^ i*golden) mod vocab."""
    return np.array([_splitmix64(seed ^ ((i * 0x9E3779B97F4A7C15) & _M64)) % vocab for i in range(n)], dtype=np.int32)


# LNB_NORM_* of include/lnb.h: name -> (form, the launch tally's row, its epilogue, folding waves; None: the plain serial loop)
NORM_FORMS = {
    "chain16": (0, "gemv_chain.rw16", "store", 2), "chain32": (1, "gemv_chain.rw32", "store", 6), "chain64": (2, "gemv_chain.rw64", "store", 6),
    "quad24": (3, "gemv_quad", "store", 6), "quad24_sched": (4, "gemv_quad", "store", 6),
    "gate_up56": (5, "gemv_chain.rw56", "silu_mul", 7), "gate_up28": (6, "gemv_chain.rw28", "silu_mul", 7),
    "gate_up56_packed": (7, "gemv_chain_pk", "silu_mul", 7), "head_packed": (8, "gemv_head_pk", "store", 8),
    "rows_wide": (9, "rmsnorm_rows.wide", "store", 6), "batch_xt": (10, "batch_rmsnorm", "store", 6),
    "rows_wave": (11, "rmsnorm_rows.wave", "store", None),
}


def op_rmsnorm_sum(x_u16, eps, form, device=0):
    """what the norm of the kernel form `form` (a key of NORM_FORMS) computed for every row of x [rows][K] -> (sum_bits uint32 [rows],
    scale_bits uint32 [rows], walk int32 [rows]: the path words of include/lnb.h), or None when the form's launch function refuses this K"""
    x = np.ascontiguousarray(x_u16, dtype=np.uint16)
    rows, k = x.shape
    sb, rb, wk = np.empty(rows, dtype=np.uint32), np.empty(rows, dtype=np.uint32), np.empty(rows, dtype=np.int32)
    rc = lib().lnb_op_rmsnorm_sum(device, _p(x), rows, k, np.float32(eps), NORM_FORMS[form][0], _p(sb), _p(rb), _p(wk))
    if rc == 1:
        return None
    _chk(rc)
    return sb, rb, wk


def op_rmsnorm_head(x_u16, norm_w_u16, eps, w_u16, packed=1, n_wg=0, device=0):
    """final norm + output projection of one row, as the one-token step launches it -> (y uint16 [n_out], WPACK status of the matrix); n_wg > 0 caps the workgroups"""
    x = np.ascontiguousarray(x_u16, dtype=np.uint16).reshape(-1)
    nw = np.ascontiguousarray(norm_w_u16, dtype=np.uint16)
    w = np.ascontiguousarray(w_u16, dtype=np.uint16)
    n, k = w.shape
    assert x.shape == (k,) and nw.shape == (k,)
    y = np.empty(n, dtype=np.uint16)
    st = C.c_int(0)
    _chk(lib().lnb_op_rmsnorm_head(device, _p(x), _p(nw), np.float32(eps), _p(w), _p(y), n, k, int(packed), int(n_wg), C.byref(st)))
    return y, st.value


def op_rmsnorm_gate_up(x_u16, norm_w_u16, eps, w1_u16, w3_u16, packed=1, device=0):
    """ffn_norm + w1|w3 + SiLU(gate)*up of one row, as the one-token step launches it -> (y uint16 [n_out], WPACK status of the matrix)"""
    x = np.ascontiguousarray(x_u16, dtype=np.uint16).reshape(-1)
    nw = np.ascontiguousarray(norm_w_u16, dtype=np.uint16)
    w1 = np.ascontiguousarray(w1_u16, dtype=np.uint16)
    w3 = np.ascontiguousarray(w3_u16, dtype=np.uint16)
    n, k = w1.shape
    assert w3.shape == (n, k) and x.shape == (k,) and nw.shape == (k,)
    y = np.empty(n, dtype=np.uint16)
    st = C.c_int(0)
    _chk(lib().lnb_op_rmsnorm_gate_up(device, _p(x), _p(nw), np.float32(eps), _p(w1), _p(w3), _p(y), n, k, int(packed), C.byref(st)))
    return y, st.value
