#!/usr/bin/env python3
"""Batched exact decode of the 8B shape in isolation (run under rocprofv3 by tools/gpu_profile_r03.sh): n prompts of --prompt-len tokens,
then --steps batched greedy steps; prints one JSON line (aggregate tokens/s, per-kernel-class times of the batched step).
--prefix N: prompts of N tokens (as --prompt-len); --seq-len N: the contexts' capacity (beyond ~7.8 K the batch runs the long-context
attention); --long-threshold N: lnb_batch_set_attention (0 = the long-context form at every position); --steps 0: profile only."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "llama-nuts-and-bolts_amd")]
import lnb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16)
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--prompt-len", type=int, default=128)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--profile-iters", type=int, default=0)
ap.add_argument("--prefix", type=int, default=None, help="prompt length (overrides --prompt-len)")
ap.add_argument("--seq-len", type=int, default=None, help="capacity of every context (default: prompt + steps + 12)")
ap.add_argument("--long-threshold", type=int, default=None, help="lnb_batch_set_attention(N): calls past N positions run the long-context attention")
ap.add_argument("--no-copy", action="store_true", help="batches from the resident chain layouts (no lnb_model_enable_batch: weights_second_copy_bytes = 0)")
ap.add_argument("--share-prefix", action="store_true", help="one source context prefilled with prompt-len - 4 tokens, the members forked from it and extended by 4 "
                "tokens of their own; attention us per layer and step ms with lnb_batch_set_shared_prefix set and cleared, alternately in this process")
ap.add_argument("--repeats", type=int, default=5, help="--share-prefix: alternations (median (min..max) is reported)")
a = ap.parse_args()
if a.prefix is not None:
    a.prompt_len = a.prefix
lnb.build()


def share_prefix():
    """shared against cleared on the SAME forked members: the cleared runs are the one-workgroup kernels (or, beyond their reach, the batched long pair)"""
    cfg = dict(lnb.LLAMA_8B, n_layers=a.layers)
    pos, npos = a.prompt_len, a.prompt_len - 4
    m = lnb.LlamaTransformer(**cfg).fill_synthetic(1234).finalize(pos + a.steps + 32 if pos + a.steps + 32 > 2 * cfg["max_seq_len"] else 0)
    if not a.no_copy:
        m.enable_batch()
    cap = a.seq_len or pos + 2 * a.repeats * (a.steps + 1) + 16
    src = lnb.InferenceContext(m, cap)
    src.Forward(lnb.synth_tokens(99, npos, cfg["vocab_size"]), 0, want_logits=False)
    ctxs = [lnb.InferenceContext(m, cap) for _ in range(a.n)]
    src.ForkPrefix(ctxs, npos)
    firsts = [c.ForwardAppend(lnb.synth_tokens(500 + s, 4, cfg["vocab_size"]), npos, want_logits=False)[1] for s, c in enumerate(ctxs)]
    b = lnb.Batch(ctxs)
    if a.long_threshold is not None:
        b.set_attention(a.long_threshold, 0)
    rows = {"shared": {"attention_us": [], "step_ms": []}, "cleared": {"attention_us": [], "step_ms": []}}
    forms = {}
    at = pos
    for _ in range(a.repeats):
        for mode in ("shared", "cleared"):
            b.set_shared_prefix(src if mode == "shared" else None, npos)
            rows[mode]["attention_us"].append(1e3 * b.profile_kernel(1, pos, a.profile_iters or 40))
            forms[mode] = b.attention_form()
            if a.steps:
                _, ms = b.decode(firsts, [at] * a.n, a.steps)     # (what the steps write is never read back: the tokens do not matter, the shapes do)
                rows[mode]["step_ms"].append(ms / a.steps)
                at += a.steps
    stat = lambda v: {"median": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3), "max": round(max(v), 3)} if v else None
    # the floor from shapes: both launches issue KVH * tiles * (hd / 16) * (P16 / 4) dependent-chain matrix instructions of 32 cycles, over 4 SIMDs per CU
    G, hd = cfg["n_heads"] // cfg["n_kv_heads"], cfg["dim"] // cfg["n_heads"]
    mfmas = cfg["n_kv_heads"] * ((a.n * G + 15) // 16) * (hd // 16) * ((npos & ~15) // 4)
    cus, mhz = lnb.device_info(0)["n_cus"], 2400            # (the MI355X's peak engine clock)
    floor_us = 2 * mfmas * 32 / (4 * cus) / mhz
    res = {"n": a.n, "pos": pos, "n_pos": npos, "seq_len": cap, "layers": a.layers, "attention_forms": forms,
           "shared": {k: stat(v) for k, v in rows["shared"].items()}, "cleared": {k: stat(v) for k, v in rows["cleared"].items()},
           "mfma_chain_floor_us": round(floor_us, 2), "share_of_floor": round(floor_us / sorted(rows["shared"]["attention_us"])[a.repeats // 2], 3)}
    if a.steps:
        res["tokens_per_s"] = {k: round(a.n / (1e-3 * stat(rows[k]["step_ms"])["median"]), 1) for k in rows}
    print(json.dumps(res))


if a.share_prefix:
    share_prefix()
    sys.exit(0)
cfg = dict(lnb.LLAMA_8B, n_layers=a.layers)
need = a.prompt_len + a.steps + 12
m = lnb.LlamaTransformer(**cfg).fill_synthetic(1234).finalize(need if need > 2 * cfg["max_seq_len"] else 0)    # (RoPE table: the reference's 2 * max_seq_len rows unless the run goes further)
if not a.no_copy:
    m.enable_batch()
ctxs = [lnb.InferenceContext(m, a.seq_len or a.prompt_len + a.steps + 12) for _ in range(a.n)]
firsts = [c.Forward(lnb.synth_tokens(99 + s, a.prompt_len, cfg["vocab_size"]), 0, want_logits=False)[1] for s, c in enumerate(ctxs)]
b = lnb.Batch(ctxs)
if a.long_threshold is not None:
    b.set_attention(a.long_threshold, 0)
warm, _ = b.decode(firsts, [a.prompt_len] * a.n, 4)
t0 = time.perf_counter()
got, ms = b.decode([int(w[-1]) for w in warm], [a.prompt_len + 4] * a.n, max(a.steps, 1))
wall = time.perf_counter() - t0
a.steps = max(a.steps, 1)
res = {"n": a.n, "prompt_len": a.prompt_len, "seq_len": ctxs[0].SequenceLength, "attention_form": b.attention_form() if hasattr(b, "attention_form") else 0, "second_copy": not a.no_copy, "LNB_GS_NTW": os.environ.get("LNB_GS_NTW", ""), "steps": a.steps, "layers": a.layers, "tokens_per_s": round(a.n * a.steps / wall, 1), "ms_per_step": round(1e3 * wall / a.steps, 4), "hip_event_ms_per_step": round(ms / a.steps, 4)}
if a.profile_iters:
    names = ["norm+wqkv+rope", "attention", "wo+residual", "norm+w1|w3+silu", "w2+residual", "norm+output", "whole block"]
    res["kernels_us"] = {names[w]: round(1e3 * b.profile_kernel(w, a.prompt_len + 4, a.profile_iters), 2) for w in range(7)}
print(json.dumps(res))
