#!/usr/bin/env python3
"""bench.py -- decode tokens/s of the MI355X-native LlamaTransformer.Forward path.

Metric (BASELINE.json): "decode tokens/s Llama-3.1-8B bf16 @1/2/4/8 MI355X; % HBM roofline".
Workload (configs[1]): Llama-3.1-8B shape, synthetic weights (seed 1234), single-prompt greedy decode:
prefill of --prompt-len synthetic tokens, then W warm-up + K timed one-token Forward+Argmax steps
(a "step" = one decoded token per in-flight sequence).  Weights, KV cache and the token feedback loop
are resident in HBM before the timed region starts; nothing is skipped inside it (32 blocks + final
norm + LM head + argmax per token, arithmetic = the reference's exact f32-chain / bf16-truncation
contract, validated token-for-token against the CPU oracle by tests/test_gpu_full_8b.py).

N GPUs (torchrun, one rank per GPU): the 32 blocks are sharded by layer into N pipeline stages with
RCCL point-to-point hidden-state hand-offs (llama-nuts-and-bolts_amd/pipeline.py); N independent
sequences are kept in flight, so per-GPU bytes per step are constant ("weak" scaling).

Prints ONE JSON line on rank 0.  On one GPU a plain run (`--gpus 1 --steps K --warmup W`) does only what that line's headline needs: it
builds the model, prefills, runs the W warm-up steps, times the K steps (`--repeats` times, the median repeat reported), writes
`--dump-outputs` if asked and prints.  `--full` adds everything else on the same line: the oracle-golden and device self-checks, per-kernel
times, the roofline and its measured model, the sequences in flight, configs[2], configs[4]'s shape, the runtime record and the CPU baseline.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "llama-nuts-and-bolts_amd"))


PEAK_HBM_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
KERNEL_NAMES = ["attn_norm+wqkv+rope GEMV", "attention", "wo+residual GEMV", "ffn_norm+w1|w3+silu GEMV",
                "w2+residual GEMV", "norm+output GEMV", "whole block (5 launches)"]


def algorithmic_bytes_per_token(a, ffn_hidden, T):
    """weights streamed once + one embedding row + KV read/write (bf16)."""
    hd = a["dim"] // a["n_heads"]
    kvd = a["n_kv_heads"] * hd
    per_layer = (a["dim"] * a["dim"] * 2 + 2 * kvd * a["dim"] + 3 * ffn_hidden * a["dim"] + 2 * a["dim"]) * 2
    weights = a["n_layers"] * per_layer + a["dim"] * 2 + a["vocab_size"] * a["dim"] * 2
    kv = a["n_layers"] * 2 * kvd * 2
    return weights + a["dim"] * 2 + kv * T + kv


def kernel_bytes(a, ffn_hidden, T):
    hd = a["dim"] // a["n_heads"]
    kvd = a["n_kv_heads"] * hd
    d = a["dim"]
    return [(d * d + 2 * kvd * d + d) * 2, 2 * kvd * T * 2, d * d * 2, (2 * ffn_hidden * d + d) * 2, ffn_hidden * d * 2,
            (a["vocab_size"] * d + d) * 2, None]


def cpu_baseline(model_cfg, prompt, n_steps):
    """Reference-equivalent CPU path (oracle/ = C restatement of src/ml + src/model, same arithmetic and order,
    outputs spread over all host cores like the reference's goroutine fan-out) on a bounded sample."""
    from oracle import oracle as orc
    ncores = orc.default_threads()        # threads actually used (capped at 64, see oracle/oracle.py)
    t0 = time.time()
    om = orc.Model(**model_cfg).fill_synthetic(1234, ncores).finalize()
    oc = orc.Context(om, len(prompt) + n_steps + 1, ncores)
    _, tok = oc.forward(prompt, 0, want_logits=False)
    t1 = time.time()
    done = 0
    for i in range(n_steps):                                  # bounded sample: stop after ~25 s of steps on a host with few cores
        _, tok = oc.forward([tok], len(prompt) + i, want_logits=False)
        done += 1
        if done >= 2 and time.time() - t1 > 25.0:
            break
    n_steps = done
    t2 = time.time()
    oc.close(); om.close()
    return {"value": round(n_steps / (t2 - t1), 4), "unit": "tokens/s", "cores": ncores, "kind": "port",
            "sample": "configs[0]-sized run (context %d = %d-token prompt + %d greedy steps) of the Llama-3.1-8B shape with synthetic weights seed 1234: "
                      "prefill %.1f s incl. weight generation, then the %d one-token Forward+Argmax steps timed (%.2f s/token).  C restatement of the Go "
                      "reference (no Go toolchain on this box), parallel over output elements like the reference's goroutine fan-out but with 8 outputs "
                      "interleaved per thread and capped at 64 threads -- faster than one goroutine per output; a stand-in, not the Go binary"
                      % (len(prompt) + n_steps, len(prompt), n_steps, t1 - t0, n_steps, (t2 - t1) / n_steps)}


# kernel symbol (prefix) of each decode kernel class of the 8B shape, for the PMC traffic lookup
KERNEL_SYMBOLS = {"attn_norm+wqkv+rope GEMV": "attn_norm+wqkv+rope GEMV", "attention": "attention", "wo+residual GEMV": "wo+residual GEMV",
                  "ffn_norm+w1|w3+silu GEMV": "ffn_norm+w1|w3+silu GEMV", "w2+residual GEMV": "w2+residual GEMV",
                  "norm+output GEMV": "norm+output GEMV"}


def pmc_traffic(kernel_name, model_name, mode):
    """HBM bytes per launch of the dominant kernel from the newest committed rocprofv3 --pmc FETCH_SIZE pass
    (profiles/rNN[_fast]_traffic.json, written by tools/summarize_profile.py, keyed by kernel CLASS -- wo and w2 are separate rows).
    PMC counters cannot be read from inside the process, so this is NOT measured in this run (the JSON line says so and names the
    git head the profile was taken at).  (None, None, None) if no profile covers the kernel."""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    if model_name != "Llama-3.1-8B" or not os.path.isdir(d):
        return None, None, None
    want_fast = mode == "fast"
    for fn in sorted((f for f in os.listdir(d) if f.endswith("_traffic.json") and (("_fast_" in f) == want_fast)), reverse=True):
        j = json.load(open(os.path.join(d, fn)))
        v = j.get("classes", {}).get(KERNEL_SYMBOLS.get(kernel_name, ""))
        if v:
            return v["hbm_read_bytes_per_launch"], "profiles/" + fn, j.get("git_head")
    return None, None, None


GOLDENS = {("llama8b", 128): "configs1_tokens.json", ("llama8b-2l", 4096): "configs2_2layer_tokens.json", ("llama8b-8l", 4096): "configs2_8layer_tokens.json",
           ("llama8b", 4096): "configs2_32layer_tokens.json",
           ("llama70b-like", 16): "configs4_80layer_tokens.json"}     # configs[4] at FULL depth (80 layers, 141 GB in the oracle's memory: made on the GPU box's host, make_configs4_cut_tokens.py 80)      # configs[2] at FULL depth: made once by tests/golden/make_configs2_cut_tokens.py 32 (hours of host cores)


def check_golden(args, first_tok, warm_toks, timed_toks, key=None):
    """The tokens this run produced against the CPU ORACLE's continuation committed under tests/golden/: configs[1] exactly (8B shape,
    seed-1234 weights, the 128-token synthetic prompt; make_configs1_tokens.py) or the configs[2] workload on the two-layer cut of the
    shape (`--model llama8b-2l --prompt-len 4096`; make_configs2_2layer_tokens.py).  exact mode: a mismatch is a parity failure and the
    bench refuses to print a number; fast mode: reports how many leading tokens agree.  None when no golden covers the workload (then
    device_self_check below is what stands behind the number, and the line says so)."""
    fn = GOLDENS.get(key or (args.model, args.prompt_len))
    path = os.path.join(ROOT, "tests", "golden", fn) if fn else None
    if not path or not os.path.exists(path):
        return None
    gold = json.load(open(path))["tokens"]
    got = [int(first_tok)] + [int(t) for t in warm_toks] + [int(t) for t in timed_toks]
    n = min(len(got), len(gold))
    agree = next((i for i in range(n) if got[i] != gold[i]), n)
    if args.mode == "exact" and agree < n:
        sys.stderr.write("PARITY FAILURE: token %d of the run is %d, the CPU oracle's is %d (tests/golden/%s)\n" % (agree, got[agree], gold[agree], fn))
        sys.exit(3)
    return {"compared": n, "identical_prefix": agree, "golden": "tests/golden/%s (CPU oracle)" % fn}


_MULTI = {}


def check_multi_golden(args, P, seqs, what):
    """Sequences of a multi-prompt section (sequence s has the prompt synth_tokens(99 + s, P)) against the CPU ORACLE's continuation of THEIR prompts on the full
    32-layer model -- the sequences the sparse file holds (0, 32, 64, 96 at P = 128: one in every quarter of a 128-batch): tests/golden/configs1_multi_P<P>_tokens.json (made on the GPU box's host cores by tests/golden/make_multi_prompt_tokens.py).  `seqs` = one token list
    per sequence, first token first.  exact mode: a mismatch is a parity failure and the bench refuses to print; None when no file covers the section."""
    if args.model != "llama8b":
        return None
    path = os.path.join(ROOT, "tests", "golden", "configs1_multi_P%d_tokens.json" % P)
    if path not in _MULTI:
        _MULTI[path] = json.load(open(path)) if os.path.exists(path) else None
    g = _MULTI[path]
    if not g:
        return None
    ids, agree_all, per = [k for k in g["sequences"] if k < len(seqs)], 0, 0
    if not ids:
        return None
    for s_ in ids:
        got, gold = [int(t) for t in seqs[s_]], g["tokens"][str(s_)]
        m_ = min(len(got), len(gold))
        per = m_
        agree = next((i for i in range(m_) if got[i] != gold[i]), m_)
        if agree < m_ and args.mode == "exact":
            sys.stderr.write("PARITY FAILURE (%s): token %d of sequence %d is %d, the CPU oracle's is %d (tests/golden/configs1_multi_P%d_tokens.json)\n" % (what, agree, s_, got[agree], gold[agree], P))
            sys.exit(3)
        agree_all += int(agree == m_)
    return {"sequences_compared": ids, "sequences_identical": agree_all, "tokens_each": per, "golden": "tests/golden/configs1_multi_P%d_tokens.json (CPU oracle: each of these sequences against the continuation of ITS prompt)" % P}


def device_self_check(lnb, model, args, prompt, seq_len, run_tokens):
    """No oracle golden exists for this workload (the CPU oracle cannot walk a 32-layer model over thousands of positions in a test's
    time): the number is backed by a DEVICE-side consistency check instead, and says so.  The same continuation is replayed on fresh
    contexts through the OTHER forms of the decode attention -- the reference's serial f64 softmax denominator forced (no certified
    estimate), and, where the context fits its LDS staging, the one-workgroup-per-head kernel instead of the chip-wide pair -- all of
    which are oracle-checked at smaller sizes (tests/test_gpu_round3.py: the same head geometry on two layers).  Tokens must be identical;
    a mismatch is a parity failure and the bench refuses to print a number."""
    n = min(len(run_tokens) - 1, 24)
    forms = [("serial f64 softmax denominator forced", (-1, 1))]
    forms.append(("one-workgroup-per-head attention kernel", (10 ** 9, 0)) if args.prompt_len + n + 1 < 7000 else ("long-context kernels at every context", (0, 0)))
    agree = {}
    for label, (thr, zseq) in forms:
        c = lnb.InferenceContext(model, seq_len).set_mode(args.mode).set_attention(thr, zseq)
        _, f = c.Forward(prompt, 0, want_logits=False)
        got, _ = c.decode_greedy(f, len(prompt), n)
        c.close()
        mine = [f] + [int(t) for t in got]
        same = next((i for i in range(n + 1) if mine[i] != run_tokens[i]), n + 1)
        agree[label] = {"compared": n + 1, "identical_prefix": same}
        if args.mode == "exact" and same < n + 1:
            sys.stderr.write("PARITY FAILURE (device self-check, %s): token %d is %d, the run's is %d\n" % (label, same, mine[same], run_tokens[same]))
            sys.exit(3)
    return {"oracle": "none at this size (no CPU-oracle golden for %s at prompt length %d)" % (args.model, args.prompt_len), "forms": agree}


CFG2_P, CFG2_W, CFG2_K = 4096, 4, 64


def configs2_record(lnb, model, cfg, args, a):
    """BASELINE configs[2] inside the --full line, so that it is timed by whoever runs `python bench.py --full` (VERDICT r4 #1c): the 4096-token prompt
    in one Forward (exact chains on the f32 matrix cores), then 4 warm-up + 64 timed greedy steps at T = 4101 ... 4164 through the long-context
    attention kernels (three repeats of the same 64 steps, median), every token compared with the CPU oracle's continuation of the FULL 32-layer
    model (tests/golden/configs2_32layer_tokens.json, made once on the host by tests/golden/make_configs2_cut_tokens.py 32).  A mismatch in exact
    mode is a parity failure: the bench refuses to print."""
    P, W, K = CFG2_P, CFG2_W, CFG2_K
    seq_len = P + W + K + 8
    ctx = lnb.InferenceContext(model, seq_len).set_mode(args.mode)
    prompt = lnb.synth_tokens(99, P, cfg["vocab_size"])
    lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx.h))
    t0 = time.perf_counter()
    _, first = ctx.Forward(prompt, 0, want_logits=False)
    t_pf = time.perf_counter() - t0
    att_form = ctx.prefill_attention_form()
    # ... and once more on a second context: the WARM time (kernels loaded, clocks up, allocator settled) next to the cold first call
    ctx_w = lnb.InferenceContext(model, P + 8).set_mode(args.mode)
    lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx_w.h))
    t0 = time.perf_counter()
    _, first_w = ctx_w.Forward(prompt, 0, want_logits=False)
    t_pf_warm = time.perf_counter() - t0
    ctx_w.reset()                                            # ... and the steady state: the same context again (see the 128-row record)
    lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx_w.h))
    t0 = time.perf_counter()
    ctx_w.Forward(prompt, 0, want_logits=False)
    t_pf_steady = time.perf_counter() - t0
    ctx_w.close()
    if first_w != first:
        sys.stderr.write("PARITY FAILURE (configs[2]): the second prefill of the same prompt gave another first token\n")
        sys.exit(3)
    warm, _ = ctx.decode_greedy(first, P, W)
    tok, pos = int(warm[-1]), P + W
    reps = []
    for rep in range(3):
        lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx.h))
        t0 = time.perf_counter()
        o_, ev_ = ctx.decode_greedy(tok, pos, K)
        reps.append((time.perf_counter() - t0, ev_, [int(t) for t in o_]))
        if reps[-1][2] != reps[0][2]:
            sys.stderr.write("PARITY FAILURE (configs[2]): repeat %d of the timed region produced different tokens\n" % rep)
            sys.exit(3)
    wall, ev_ms, out = sorted(reps, key=lambda r: r[0])[1]
    golden = check_golden(args, first, [int(t) for t in warm], out, key=("llama8b", P))
    Tbar = pos + (K - 1) / 2.0 + 1.0
    B = algorithmic_bytes_per_token(a, model.ffn_hidden, Tbar)
    att_ms = ctx.profile_kernel(1, int(Tbar) - 1, 16)
    zseq = ctx.zseq_count()
    ctx.close()
    tps = K / wall
    hd = a["dim"] // a["n_heads"]
    mm = a["n_layers"] * (a["dim"] * (a["n_heads"] + 2 * a["n_kv_heads"]) * hd + a["dim"] * a["dim"] + 3 * a["dim"] * model.ffn_hidden)    # multiply-accumulates per row
    return {"workload": "Llama-3.1-8B bf16, 1xMI355X, long-prefill seq_len=%d + %d decode (configs[2]; %d warm-up steps first)" % (P, K, W),
            "prefill": {"rows": P, "ms": round(1e3 * t_pf, 1), "TFLOP/s": round(2.0 * P * mm / t_pf / 1e12, 1), "peak_TFLOP/s": 157.3,
                        "frac_of_f32_mfma_peak": round(2.0 * P * mm / t_pf / 1e12 / 157.3, 4),
                        "warm_ms": round(1e3 * t_pf_warm, 1), "warm_frac_of_f32_mfma_peak": round(2.0 * P * mm / t_pf_warm / 1e12 / 157.3, 4), "steady_ms": round(1e3 * t_pf_steady, 1),
                        "frac_of_bf16_mfma_peak_2500": round(2.0 * P * mm / t_pf_warm / 1e12 / 2500.0, 4),
                        "note": "ms = the first call of the process at this row count (cold: what a driver sees), warm_ms = the same prompt again on a second context; the exact "
                                "order forces the f32 matrix instruction (1/16 of the bf16 rate): both peaks are quoted",
                        "attention_kernel": {3: "attn_mfma3_kernel (scores computed once, exp-table indices kept in the context's scratch)",
                                             1: "attn_mfma_kernel (scores computed twice: the score-index scratch was REFUSED -- LNB_ATTN_SIDX_MB or no device memory; ~35 ms slower, same bits)"}.get(att_form, "form %d" % att_form),
                        "kernel": "gemm_stream_kernel fed from the RESIDENT weight layouts (no second copy; wo / w2 two weight tiles per wave) + the matrix-core attention above; v_mfma_f32_16x16x4_f32 = the k-ordered chain; matmul FLOPs only"},
            "decode": {"steps": K, "tokens_per_s": round(tps, 2), "ms_per_step": round(1e3 * wall / K, 4), "hip_event_ms_per_step": round(ev_ms / K, 4),
                       "repeats_ms_per_step": [round(1e3 * r[0] / K, 4) for r in reps], "mean_context": Tbar,
                       "frac_of_hbm_roofline": round(tps * B / 1e9 / PEAK_HBM_GBS, 4), "algorithmic_bytes_per_token": int(B),
                       "attention_us_per_layer": round(1e3 * att_ms, 2), "softmax_rows_that_walked_the_serial_sum": zseq},
            "tokens_vs_oracle_golden": golden if golden else {"compared": 0, "note": "tests/golden/configs2_32layer_tokens.json is missing"},
            "first_token": int(first)}


CFG4 = dict(dim=8192, n_layers=80, n_heads=64, n_kv_heads=8, multiple_of=4096)
CFG4_P, CFG4_W, CFG4_K = 16, 2, 16


def configs4_record(lnb, args):
    """BASELINE configs[4]'s shape (random-init Llama shape dim 8192 x 80 layers, "70B-like") on ONE GPU, inside the --full line: 141 GB of synthetic
    weights resident, a 16-token prompt (one Forward on the f32 matrix cores), 2 warm-up + 16 timed greedy steps (two repeats, the faster one).  The
    run's 19 tokens are compared with the CPU oracle's continuation of the FULL 80-layer model (tests/golden/configs4_80layer_tokens.json, made once on the
    GPU box's host: the oracle holds the 141 GB in memory); the 10-layer cut (one pipeline stage) is pinned too.  Next to it the device self-check: the same
    continuation through the throughput kernel forms and through the forced serial softmax denominator, token for token."""
    cfg = dict(lnb.LLAMA_8B, **CFG4)
    P, W, K = CFG4_P, CFG4_W, CFG4_K
    t0 = time.time()
    try:
        model = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize()
    except lnb.LnbError as e:
        return {"skipped": str(e)[:300]}
    t_build = time.time() - t0
    a = {k: cfg[k] for k in ("dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size")}
    prompt = lnb.synth_tokens(99, P, cfg["vocab_size"])
    ctx = lnb.InferenceContext(model, P + W + K + 8).set_mode(args.mode)
    _, first = ctx.Forward(prompt, 0, want_logits=False)
    warm, _ = ctx.decode_greedy(first, P, W)
    tok, pos = int(warm[-1]), P + W
    reps = []
    for rep in range(2):
        lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx.h))
        t0 = time.perf_counter()
        o_, ev_ = ctx.decode_greedy(tok, pos, K)
        reps.append((time.perf_counter() - t0, ev_, [int(t) for t in o_]))
    if reps[0][2] != reps[1][2]:
        sys.stderr.write("PARITY FAILURE (configs[4] shape): two repeats of the timed region produced different tokens\n")
        sys.exit(3)
    wall, ev_ms, out = min(reps, key=lambda r: r[0])
    run = [int(first)] + [int(t) for t in warm] + out
    golden = check_golden(args, first, [int(t) for t in warm], out, key=("llama70b-like", CFG4_P))      # exact mode: a mismatch ends the bench (PARITY FAILURE)
    n_rows = (W + 2 * K) * (2 * cfg["n_layers"] + 1)
    fb = ctx.norm_fallbacks() if args.mode == "exact" else None
    forms = {}
    for label, setup in (("throughput kernel forms", lambda c: c.set_schedule("throughput")), ("serial f64 softmax denominator forced", lambda c: c.set_attention(-1, 1))):
        c2 = setup(lnb.InferenceContext(model, P + W + K + 8).set_mode(args.mode))
        _, f2 = c2.Forward(prompt, 0, want_logits=False)
        t2, _ = c2.decode_greedy(f2, P, W + K)
        got = [int(f2)] + [int(t) for t in t2]
        same = 0
        while same < len(run) and got[same] == run[same]:
            same += 1
        forms[label] = {"compared": len(run), "identical_prefix": same}
        c2.close()
        if args.mode == "exact" and same != len(run):
            sys.stderr.write("PARITY FAILURE (configs[4] shape): the %s disagree with the latency forms at token %d\n" % (label, same))
            sys.exit(3)
    Tbar = pos + (K - 1) / 2.0 + 1.0
    B = algorithmic_bytes_per_token(a, model.ffn_hidden, Tbar)
    tps = K / wall
    wb = model.weight_bytes()
    ctx.close(); model.close()
    return {"workload": "random-init Llama shape dim=8192 n_layers=80 (configs[4]) bf16 on ONE MI355X: %d-token prompt, %d warm-up + %d timed greedy steps" % (P, W, K),
            "tokens_per_s": round(tps, 2), "ms_per_step": round(1e3 * wall / K, 3), "hip_event_ms_per_step": round(ev_ms / K, 3),
            "frac_of_hbm_roofline": round(tps * B / 1e9 / PEAK_HBM_GBS, 4), "algorithmic_bytes_per_token": int(B), "weight_bytes_resident": wb, "model_build_s": round(t_build, 1),
            "norm_item_walk": {"rows": n_rows, "fallback_rows": fb}, "device_self_check": forms,
            "tokens_vs_oracle_golden": golden if golden else {"compared": 0, "note": "tests/golden/configs4_80layer_tokens.json is missing"},
            "oracle_evidence": "this run's tokens against the CPU oracle's continuation of the FULL 80-layer model (tests/golden/configs4_80layer_tokens.json, made on the GPU box's "
                               "host cores); the 10-layer cut (one stage of the 8-GPU pipeline) is pinned as well (configs4_10layer_tokens.json); both replayed by tests/test_gpu_round6.py",
            "last_tokens": out[-4:]}


def _c_getenv(name):
    """the process environment as the C runtime sees it (os.environ is a snapshot taken at interpreter start and misses what native code
    changed since)"""
    import ctypes
    g = ctypes.CDLL(None).getenv
    g.restype = ctypes.c_char_p
    v = g(name.encode())
    return v.decode() if v else None


def concurrent_sequences(lnb, model, cfg, args, a, single_run_tokens, n_seq=None, sched="throughput"):
    """Not the headline (configs[1] is ONE prompt): the same resident model decoding `--concurrent` independent prompts at once, one
    context and stream each, through the one-GPU form of the pipeline tick path (lnb_pipeline_tick: captured stage graphs, device-side
    token ring).  Their kernels overlap -- one sequence's chain-bound launches under another's HBM-bound ones -- which is what every
    pipeline rank gets per stage.  Sequence 0 has the headline run's prompt: its tokens are compared with that run's."""
    import pipeline
    n_seq, P, W, K = n_seq or args.concurrent, args.prompt_len, min(args.warmup, 4), min(args.steps, 48)
    seq_len = P + W + K + 8
    # the contexts take the THROUGHPUT forms of the one-token kernels (lnb_ctx_set_schedule: every workgroup <= 57 KB of LDS, so that one
    # context's chain-bound launch shares the CUs with another's HBM-bound gate|up launch); sched="latency" = the single stream's forms, for the A/B
    ctxs = [lnb.InferenceContext(model, seq_len).set_mode(args.mode).set_schedule(sched) for _ in range(n_seq)]
    pipe = lnb.Pipeline(model, 0, 1, None)
    prompts = [lnb.synth_tokens(99 + s, P, cfg["vocab_size"]) for s in range(n_seq)]
    n_decode = W + K
    t_split, t_end = n_seq * (1 + W), n_seq * (1 + W + K)
    st = pipeline.run_ticks_native(0, 1, pipe, ctxs, prompts, n_decode, 0, t_split)
    pipe.sync()
    t0 = time.perf_counter()
    pipeline.run_ticks_native(0, 1, pipe, ctxs, prompts, n_decode, t_split, t_end, st)
    pipe.sync()
    wall = time.perf_counter() - t0
    toks0 = [int(pipe.read_tokens(q, 1)[0]) for q in st["slots"][0]]
    multi = check_multi_golden(args, P, [[int(pipe.read_tokens(q, 1)[0]) for q in st["slots"][s_]] for s_ in range(n_seq)], "%d sequences in flight (%s forms)" % (n_seq, sched))
    n_cmp = min(len(toks0), len(single_run_tokens))
    same = 0
    while same < n_cmp and toks0[same] == single_run_tokens[same]:
        same += 1
    pipe.close()
    for c in ctxs:
        c.close()
    tps = n_seq * K / wall
    Tbar = P + W + (K - 1) / 2.0 + 1.0
    B = algorithmic_bytes_per_token(a, model.ffn_hidden, Tbar)
    return {"n": n_seq, "schedule": sched, "GPU_MAX_HW_QUEUES": _c_getenv("GPU_MAX_HW_QUEUES"), "tokens_per_s": round(tps, 2), "steps_each": K, "ms_per_token": round(1e3 * wall / (n_seq * K), 4),
            "frac_of_hbm_roofline": round(tps * B / 1e9 / PEAK_HBM_GBS, 4),
            "sequence0_tokens_vs_single_run": {"compared": n_cmp, "identical_prefix": same}, "sequences_vs_oracle_golden": multi,
            "note": "aggregate of independent prompts on ONE GPU; weights are re-read per sequence (no batching: every token keeps its own exact chains)"}


def batched_sequences(lnb, model, cfg, args, a, single_run_tokens):
    """Sequences in flight, BATCHED (lnb_batch_*): n independent prompts decoded together, one pass over the weights per step for all of them
    -- each sequence is a column of the f32 matrix-core product, whose k-ordered chain is the reference's (bit-identical per sequence;
    tests/test_gpu_batch.py).  Not the headline (configs[1] is one prompt); it is what a server, and every pipeline rank, runs.
    Sequence 0 has the headline's prompt: its tokens are compared with the single run's."""
    P, W, K = args.prompt_len, min(args.warmup, 4), min(args.steps, 48)
    seq_len = P + W + K + 8
    n_max = max(args.batch_sizes)
    ctxs = [lnb.InferenceContext(model, seq_len) for _ in range(n_max)]
    prompts = [lnb.synth_tokens(99 + s, P, cfg["vocab_size"]) for s in range(n_max)]

    def one(n, with_kernels):
        firsts = []
        for s in range(n):
            ctxs[s].reset()
            firsts.append(ctxs[s].Forward(prompts[s], 0, want_logits=False)[1])
        b = lnb.Batch(ctxs[:n])
        warm, _ = b.decode(firsts, [P] * n, W) if W > 0 else (np.zeros((n, 0), dtype=np.int32), 0.0)
        toks = [int(warm[s][-1]) if W > 0 else firsts[s] for s in range(n)]
        lnb._chk(lnb.lib().lnb_ctx_synchronize(ctxs[0].h))
        t1 = time.perf_counter()
        got, ev_ms = b.decode(toks, [P + W] * n, K)
        wall = time.perf_counter() - t1
        seq0 = [firsts[0]] + [int(t) for t in warm[0]] + [int(t) for t in got[0]]
        multi = check_multi_golden(args, P, [[firsts[s]] + [int(t) for t in warm[s]] + [int(t) for t in got[s]] for s in range(n)], "batch of %d" % n)
        n_cmp = min(len(seq0), len(single_run_tokens))
        same = next((i for i in range(n_cmp) if seq0[i] != single_run_tokens[i]), n_cmp)
        Tbar = P + W + (K - 1) / 2.0 + 1.0
        per_seq = algorithmic_bytes_per_token(a, model.ffn_hidden, Tbar)
        kv = a["n_layers"] * 2 * (a["n_kv_heads"] * (a["dim"] // a["n_heads"])) * 2
        own = a["dim"] * 2 + kv * Tbar + kv                  # a sequence's own traffic: its embedding row, its KV read and write
        step_bytes = (per_seq - own) + n * own               # the weights ONCE per step + every sequence's own bytes
        tps = n * K / wall
        run = {"n": n, "tokens_per_s": round(tps, 1), "ms_per_step": round(1e3 * wall / K, 4), "hip_event_ms_per_step": round(ev_ms / K, 4), "steps": K,
               "hbm_frac_of_bytes_actually_needed": round(step_bytes * (K / wall) / 1e9 / PEAK_HBM_GBS, 4),
               "equivalent_frac_if_each_sequence_read_the_weights": round(tps * per_seq / 1e9 / PEAK_HBM_GBS, 4),
               "sequence0_tokens_vs_single_run": {"compared": n_cmp, "identical_prefix": same}}
        if multi:
            run["sequences_vs_oracle_golden"] = multi
        if with_kernels:
            names = ["norm+wqkv+rope", "attention", "wo+residual", "norm+w1|w3+silu", "w2+residual", "norm+output", "whole block"]
            run["kernels_us"] = {names[w]: round(1e3 * b.profile_kernel(w, int(Tbar) - 1, 16), 2) for w in range(7)}
        b.close()
        return run

    # a batch on a model WITHOUT the second copy runs its products as rows of the streaming kernel on the RESIDENT layouts (round 5): measured first
    no_copy = [one(n, False) for n in args.batch_sizes if n in (16, 64, 128) or n == n_max] if model.batch_bytes() == 0 else []
    t0 = time.perf_counter()
    model.enable_batch()
    t_enable = time.perf_counter() - t0
    out = {"weights_second_copy_bytes": model.batch_bytes(), "enable_batch_s": round(t_enable, 2),
           "runs_without_the_second_copy": {"weights_second_copy_bytes": 0, "runs": no_copy,
                                            "note": "every product of the batch as rows of gemm_stream_kernel on the resident weight layouts (row-broadcast / chain); the matrix-core "
                                                    "copy is a performance option: the column forms of up to 32 sequences read it"},
           "runs": [one(n, n == n_max) for n in args.batch_sizes]}
    # the prompt's prefill again, now that the matrix-core copy exists: every product of 16 or more rows streams it (gemm_stream_kernel:
    # weights HBM -> registers -> A operand, f32 activation rows in the LDS); same chains, same first token as the headline's prefill
    best, tok_pf = 1e9, -1
    for rep in range(2):
        ctxs[0].reset()
        lnb._chk(lnb.lib().lnb_ctx_synchronize(ctxs[0].h))
        t1 = time.perf_counter()
        _, tok_pf = ctxs[0].Forward(prompts[0], 0, want_logits=False)
        best = min(best, time.perf_counter() - t1)
    mm = a["n_layers"] * (a["dim"] * (a["n_heads"] + 2 * a["n_kv_heads"]) * (a["dim"] // a["n_heads"]) + a["dim"] * a["dim"] + 3 * a["dim"] * model.ffn_hidden)   # multiply-accumulates per row
    out["prefill_streamed"] = {"rows": P, "ms": round(1e3 * best, 2), "TFLOP/s": round(2.0 * P * mm / best / 1e12, 2), "peak_TFLOP/s": 157.3, "frac_of_f32_mfma_peak": round(2.0 * P * mm / best / 1e12 / 157.3, 4),
                               "kernel": "gemm_stream_kernel fed from the M16 copy", "first_token_same_as_headline_prefill": bool(single_run_tokens and int(tok_pf) == int(single_run_tokens[0]))}
    out["weight_bytes_resident_with_the_second_copy"] = model.weight_bytes() + model.batch_bytes()
    if args.model == "llama8b" and not args.no_configs2 and P < CFG2_P:
        # configs[2]'s prompt again on the streaming feed (the --full line's configs2.prefill ran before the copy existed)
        c2 = lnb.InferenceContext(model, CFG2_P + 8)
        p2 = lnb.synth_tokens(99, CFG2_P, cfg["vocab_size"])
        lnb._chk(lnb.lib().lnb_ctx_synchronize(c2.h))
        t1 = time.perf_counter()
        _, tok2 = c2.Forward(p2, 0, want_logits=False)
        dt = time.perf_counter() - t1
        c2.close()
        out["prefill_streamed_4096"] = {"rows": CFG2_P, "ms": round(1e3 * dt, 1), "TFLOP/s": round(2.0 * CFG2_P * mm / dt / 1e12, 1), "frac_of_f32_mfma_peak": round(2.0 * CFG2_P * mm / dt / 1e12 / 157.3, 4),
                                        "first_token": int(tok2)}
    for c in ctxs:
        c.close()
    out["note"] = ("aggregate tokens/s of n independent prompts decoded together on ONE GPU: one pass over the weights per step, each sequence a "
                   "column of v_mfma_f32_16x16x4_f32 (exact k-ordered chains; token-identical per sequence)")
    return out


# Bare cost of one dependent add of a k-ordered f32 chain on gfx950, in shader cycles per k-step of ONE chain wave with nothing else in its way
# (micro-benchmarks tools/chainbench3.hip / chainbench4.hip, logs profiles/r04_chainbench3.log; hardware numbers, not this library's kernels)
CHAIN_CYCLES = {"row_newbcast": 5.56,  # v_add_f32_dpp row_newbcast, products fetched from the LDS 64 steps per ds_read_b128: wo, w2
                "quad_perm": 6.81}     # v_add_f32_dpp quad_perm, 16 steps per ds_read_b128: wq|wk|wv (24 rows per CU need 16 rows per chain wave)
HBM_ACHIEVABLE_GBS = 6700.0            # the best streaming READ rate on record for this chip (MI355X_MICROARCH.md price list: 6.5-6.8 TB/s for an nt weight stream; the float4 COPY figure is 6.29)
NOMINAL_GHZ = 2.344                    # shader clock the r04 chain figures were quoted at; used only where a launch's own clock could not be measured
GEMV_CLASSES = {0: ("attn_norm+wqkv+rope GEMV", "quad_perm"), 2: ("wo+residual GEMV", "row_newbcast"), 3: ("ffn_norm+w1|w3+silu GEMV", None),
                4: ("w2+residual GEMV", "row_newbcast"), 5: ("norm+output GEMV", None)}


def measured_model(ctx, a, ffn_hidden, Tbar, kernels, tps):
    """Two things, kept apart (VERDICT r4 #2f):
    * `hardware_bound` -- depends on the chip and the arithmetic only: per launch max(K x the bare DPP chain step at the launch's measured shader
      clock, algorithmic bytes / 6.7 TB/s), NO prologue, NO kernel boundary; the attention as measured (latency-bound, no bound claimed).
      Every output is one k-ordered chain of K dependent f32 adds (operations_lineartransform.go:46-65): nothing that keeps the bits goes below it.
    * `per_kernel` -- the CURRENT kernels taken apart with stamps of THIS run (lnb_profile_kernel_stamps: one launch per class with the per-wave
      cycle stamps armed; stamp 7 = the same launch on the constant-rate wall clock, so cycles become microseconds at the clock the launch really
      ran at): prologue (kernel start -> the chain wave's first add), main loop (cycles per k-step for the chain-bound launches, GB/s for the
      HBM-bound ones), and boundary = HIP-event launch-to-launch time minus the longest wave's in-kernel time.  `floor_us` = the hardware bound
      of the launch + ITS measured prologue + ITS measured boundary: what the launch would take with a perfect main loop and nothing else
      changed -- a statement about these kernels, not about the chip."""
    d, hd = a["dim"], a["dim"] // a["n_heads"]
    kb = kernel_bytes(a, ffn_hidden, Tbar)
    Ksteps = {0: d, 2: a["n_heads"] * hd, 3: d, 4: ffn_hidden, 5: d}
    per, hw_rows, fl_rows, cur_rows = {}, {}, {}, {}
    for which, (name, chain) in GEMV_CLASSES.items():
        got_us = 1e3 * kernels[name]["ms"]
        try:
            v, khz = ctx.profile_kernel_stamps(which, int(Tbar) - 1)
        except Exception as e:                                     # the model is a report, never a reason to lose the line
            v, khz = None, 0
        rec = {"us": round(got_us, 2)}
        ghz = NOMINAL_GHZ
        prologue_us = boundary_us = None
        if v is not None and khz > 0:
            cw = next((w for w in range(8) if v[w][0] > 0 and v[w][12] > 0), None)       # a chain wave: stamp 6 = the cycle its main loop starts
            if cw is not None and v[cw][13] > 0:
                wall_us = v[cw][13] / khz * 1e3
                ghz = v[cw][1] / wall_us * 1e-3                    # shader cycles per wall microsecond of the same wave, same launch
                in_kernel_us = max(v[w][2] for w in range(8)) / ghz * 1e-3
                prologue_us = v[cw][12] / ghz * 1e-3
                main_cycles = v[cw][1] - v[cw][12]
                boundary_us = max(0.0, got_us - in_kernel_us)
                rec.update({"shader_clock_GHz": round(ghz, 3), "in_kernel_us": round(in_kernel_us, 2), "prologue_us": round(prologue_us, 2),
                            "main_loop_us": round(main_cycles / ghz * 1e-3, 2), "boundary_us": round(boundary_us, 2)})
                if chain:
                    rec["cycles_per_k_step"] = round(main_cycles / Ksteps[which], 3)
                else:
                    rec["main_loop_GBps"] = round(kb[which] / (main_cycles / ghz) , 1)
        hw = max(Ksteps[which] * CHAIN_CYCLES[chain] / ghz * 1e-3 if chain else 0.0, kb[which] / HBM_ACHIEVABLE_GBS * 1e-3)
        rec["hardware_bound_us"] = round(hw, 2)
        if prologue_us is not None:
            rec["floor_us"] = round(hw + prologue_us + boundary_us, 2)
            rec["achieved_over_floor"] = round((hw + prologue_us + boundary_us) / got_us, 3)
        per[name] = rec
        hw_rows[which], cur_rows[which] = hw, got_us
        fl_rows[which] = rec.get("floor_us", got_us)
    att = 1e3 * kernels[KERNEL_NAMES[1]]["ms"]
    per["attention"] = {"us": round(att, 2), "note": "latency-bound at this context: taken as measured in both sums"}
    B = algorithmic_bytes_per_token(a, ffn_hidden, Tbar)

    def token(rows):
        t = 1e-6 * (a["n_layers"] * (rows[0] + att + rows[2] + rows[3] + rows[4]) + rows[5])
        return {"ms_per_token": round(1e3 * t, 4), "tokens_per_s": round(1.0 / t, 1), "frac_of_hbm_roofline": round(B / t / 1e9 / PEAK_HBM_GBS, 4)}

    hwb, flr = token(hw_rows), token(fl_rows)
    return {"hardware_bound": dict(hwb, note="per launch max(K x bare DPP chain step at the measured clock, bytes / 6.7 TB/s); no prologue, no boundary; attention as measured",
                                   achieved_frac_of_bound=round(tps / hwb["tokens_per_s"], 4)),
            "floor_with_measured_prologues_and_boundaries": dict(flr, achieved_frac_of_floor=round(tps / flr["tokens_per_s"], 4),
                                                                  note="hardware bound + each launch's prologue and boundary as stamped in this run: a model of the current kernels, not of the chip"),
            "per_kernel": per,
            "constants": {"bare_chain_cycles_per_step": CHAIN_CYCLES, "hbm_achievable_GBps": HBM_ACHIEVABLE_GBS, "source": "tools/chainbench3.hip, profiles/r04_chainbench3.log; MI355X_MICROARCH.md"}}


def traffic_child(lnb, cfg, args):
    """Runs under `rocprofv3 --pmc FETCH_SIZE` (probe_traffic): the same shape cut to two layers, a short prompt, then the dominant decode
    kernel class launched 24 times, alternating between the layers so that every launch streams its weights from HBM."""
    cfg = dict(cfg, n_layers=min(cfg["n_layers"], 2))
    pos = args.traffic_pos
    model = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize(rope_rows=max(pos + 16, 2 * cfg["max_seq_len"]))
    ctx = lnb.InferenceContext(model, pos + 8).set_mode(args.mode)
    ctx.Forward(lnb.synth_tokens(99, 16, cfg["vocab_size"]), 0, want_logits=False)
    for which in [int(w) for w in str(args.traffic_child).split(",")]:
        ctx.profile_kernel(which, pos, 24)
    ctx.close(); model.close()
    return 0


def probe_traffic(args, classes, pos):
    """HBM bytes per launch of the dominant kernel symbol (its launch classes, e.g. wo and w2 of rowcast_lds_kernel), measured in THIS run: PMC counters cannot be read from inside a process, so a child
    (traffic_child) is run under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` (a counter pass of its own, no other trace domains) and its
    counter file is read back.  FETCH_SIZE is in KiB and tallies wide coalesced reads at half their bytes on gfx950 (MI355X_MICROARCH.md,
    section HBM): bytes = KiB x 1024 x 2.  None when rocprofv3 is missing, when this process already runs under it, or on any failure
    (the committed profile's number is reported then, flagged as not measured in the run)."""
    import csv
    import shutil
    import subprocess
    import tempfile
    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if os.environ.get("ROCP_TOOL_LIBRARIES") or not os.path.exists(rp):
        return None
    tmp = tempfile.mkdtemp(prefix="lnb_traffic_", dir="/tmp")
    try:
        cmd = [rp, "--kernel-trace", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", tmp, "-o", "pmc", "--", sys.executable,
               os.path.abspath(__file__), "--traffic-child", ",".join(str(c) for c in classes), "--traffic-pos", str(pos), "--model", args.model, "--mode", args.mode]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            return None
        per = {}
        for root, _, files in os.walk(tmp):
            for fn in files:
                if fn.endswith("counter_collection.csv"):
                    for row in csv.DictReader(open(os.path.join(root, fn))):
                        if row.get("Counter_Name") == "FETCH_SIZE":
                            per.setdefault(row["Kernel_Name"], []).append(float(row["Counter_Value"]))
        per = {k: v for k, v in per.items() if len(v) >= 20}          # the looped classes (24 + 3 warm-up launches each); the prompt's kernels ran twice
        if not per:
            return None
        kname, vals = max(per.items(), key=lambda kv: sum(kv[1]))     # (the long-context attention is two kernels: the heavier one)
        total = sum(sum(v) / len(v) for v in per.values())            # (one symbol looped as two classes: the mean over all its launches)
        return {"bytes_per_launch": int(total * 1024 * 2), "launches": len(vals),
                "source": "this run: rocprofv3 --pmc FETCH_SIZE over %d launches of %s (child process, two layers of the shape), KiB x 1024 x 2 (gfx950 correction)"
                          % (len(vals), kname.split("(")[0][:80])}
    except Exception:                                                  # the probe must never take the bench line down
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N copies of this command, one rank per GPU (RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* in the environment, exactly what torch.distributed.run would set -- which keeps working: under it WORLD_SIZE is already set and
    no one spawns).  Rank 0's stdout is this process's stdout (the ONE JSON line); the other ranks' stdout goes to stderr.  The exit code is
    the first non-zero one; if a rank dies the others are terminated (their peers would wait for it for minutes)."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
    env0 = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = []
    for r in range(n):
        env = dict(env0, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stdout=None if r == 0 else sys.stderr))
    rc, live = 0, set(range(n))
    while live:
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0 and rc == 0:
                rc = code
                sys.stderr.write("bench.py: rank %d exited with code %d; stopping the other ranks\n" % (r, code))
                for q in live:
                    procs[q].terminate()
        time.sleep(0.05)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run everything else the bench measures and checks on one GPU: the oracle-golden and device "
                         "self-checks, the long run, warm / steady prefill, per-kernel times, roofline and measured model, the rocprofv3 traffic probe, "
                         "sequences in flight (concurrent and batched), configs[2], configs[4]'s shape, runtime info and the CPU baseline. "
                         "Without it a one-GPU run sets up, warms up, times the steps, dumps its outputs if asked and prints the headline line")
    ap.add_argument("--cpu-steps", type=int, default=24, help="decode steps of the CPU baseline sample (0 = skip; --full only)")
    ap.add_argument("--profile-iters", type=int, default=64, help="launches per kernel class of the per-kernel timings (--full only)")
    ap.add_argument("--repeats", type=int, default=3, help="repeats of the timed K steps; the median repeat is reported (SURVEY.md 8(d))")
    ap.add_argument("--concurrent", type=int, default=8, help="also time this many independent prompts in flight on the one GPU (0/1 = skip; --full only)")
    ap.add_argument("--batch-sizes", type=lambda v: [int(x) for x in v.split(",") if x], default=[2, 4, 8, 16, 32, 64, 128],
                    help="also time BATCHED exact decode of this many prompts (comma list, each 1..128; empty = skip; --full only)")
    ap.add_argument("--no-traffic-probe", action="store_true", help="do not run the rocprofv3 FETCH_SIZE pass of the dominant kernel (--full only)")
    ap.add_argument("--no-configs2", action="store_true", help="leave the configs[2] record (4096-token prompt + 64 steps, oracle-golden checked) out of the --full line")
    ap.add_argument("--no-configs4", action="store_true", help="leave the configs4_one_gpu record (the 70B-like shape, 141 GB, 16 timed steps) out of the --full line")
    ap.add_argument("--traffic-child", default="", help=argparse.SUPPRESS)      # internal: kernel class(es) to loop under rocprofv3, comma separated
    ap.add_argument("--traffic-pos", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--model", default="llama8b", choices=["llama8b", "llama8b-2l", "llama8b-8l", "tiny", "llama70b-like"])
    ap.add_argument("--mode", default="exact", choices=["exact", "fast"],
                    help="exact (default, headline): the reference's k-ordered chains, token-identical to the CPU path; "
                         "fast: split-K / bf16-MFMA tolerance mode (opt-in, measured distance in NOTES.md 6.2)")
    ap.add_argument("--dry-run", action="store_true", help=argparse.SUPPRESS)   # launcher check without a GPU: every rank reports its environment and exits
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed repeat returned to its caller (the K greedy token ids) as DIR/decode_tokens.npy "
                         "(float64; the single-GPU path only)")
    args = ap.parse_args()
    if args.dump_outputs and (args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("LNB_FORCE_PIPELINE") == "1"):
        ap.error("--dump-outputs covers the single-GPU path only")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args.gpus)                        # `python bench.py --gpus N` as ONE plain command: this process becomes the launcher
    if args.dry_run:
        info = {k: os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
        if int(info["RANK"] or 0) == 0:
            print(json.dumps({"dry_run": True, "n_gpus": args.gpus, "env": info}))
        else:
            print("rank %s of %s up" % (info["RANK"], info["WORLD_SIZE"]))
        return 7 if os.environ.get("LNB_DRY_RUN_FAIL_RANK") == (info["RANK"] or "0") else 0

    import lnb
    lnb.build()
    cfg = dict(lnb.LLAMA_8B)
    name = "Llama-3.1-8B"
    if args.model == "tiny":
        cfg.update(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=1024, multiple_of=64)
        name = "tiny-256x2"
    elif args.model in ("llama8b-2l", "llama8b-8l"):
        cfg.update(n_layers=2 if args.model == "llama8b-2l" else 8)   # the 8B shape's geometry on 2 / 8 layers: the sizes the CPU oracle reaches at a 4096-token prompt
        name = "Llama-3.1-8B shape cut to %d layers" % cfg["n_layers"]
    elif args.model == "llama70b-like":
        cfg.update(dim=8192, n_layers=80, n_heads=64, n_kv_heads=8, multiple_of=4096)
        name = "random-init Llama-shape dim=8192 n_layers=80"

    if args.traffic_child:
        return traffic_child(lnb, cfg, args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 or world > 1 or os.environ.get("LNB_FORCE_PIPELINE") == "1":     # (the env switch runs the N-GPU code path on one GPU)
        import pipeline
        return pipeline.bench_main(args, cfg, name)

    P, W, K = args.prompt_len, args.warmup, args.steps
    # --full: a short timed region (the driver passes --steps 20) is followed by a 256-step one, reported next to it (not under rocprofv3: its
    # kernel trace has crashed inside the tool on runs of tens of thousands of graph-launched kernels)
    K_LONG = 256 if (K < 64 and args.model in ("llama8b", "llama8b-2l", "llama8b-8l") and not os.environ.get("ROCP_TOOL_LIBRARIES")) else 0
    seq_len = P + W + K + K_LONG + 8
    # --full also carries configs[2] (4096-token prompt + 64 steps): one model serves both, its RoPE table long enough for either
    with_cfg2 = args.model == "llama8b" and P < CFG2_P and not args.no_configs2 and not os.environ.get("ROCP_TOOL_LIBRARIES")
    # ... and configs[4]'s shape on ONE GPU (141 GB resident, built after the 8B model has been released): VERDICT r5 #4b
    with_cfg4 = with_cfg2 and not args.no_configs4
    # The context and the RoPE table are sized as above with or without --full, so that the timed steps run on the same model and context
    # (the context's length picks the attention kernels' LDS staging) whether or not the sections after them run
    t_load = time.time()
    model = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize(rope_rows=max(seq_len, 2 * cfg["max_seq_len"], (CFG2_P + CFG2_W + CFG2_K + 8) if with_cfg2 else 0))
    ctx = lnb.InferenceContext(model, seq_len).set_mode(args.mode)
    t_load = time.time() - t_load
    prompt = lnb.synth_tokens(99, P, cfg["vocab_size"])
    t_pf = time.perf_counter()
    _, tok = ctx.Forward(prompt, 0, want_logits=False)            # prefill (outside the timed region; reported separately)
    t_pf = time.perf_counter() - t_pf
    t_pf_warm = t_pf_steady = None
    if args.full and P >= 16:                                     # the same prompt again on a second context: warm prefill next to the cold first call
        ctx_w = lnb.InferenceContext(model, P + 8).set_mode(args.mode)
        lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx_w.h))
        tw = time.perf_counter()
        ctx_w.Forward(prompt, 0, want_logits=False)
        t_pf_warm = time.perf_counter() - tw
        # ... and a third time on that SAME context after lnb_ctx_reset: the steady state of a server that reuses its contexts (no per-context first-call
        # allocations -- score-index scratch, logits row -- inside the timed call); tools/prefill_bench.py measures this form
        ctx_w.reset()
        lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx_w.h))
        tw = time.perf_counter()
        ctx_w.Forward(prompt, 0, want_logits=False)
        t_pf_steady = time.perf_counter() - tw
        ctx_w.close()
    pos = P
    first_tok, warm_toks = tok, []
    if W > 0:
        out, _ = ctx.decode_greedy(tok, pos, W)                   # untimed warm-up steps (captures the graph)
        warm_toks = [int(t) for t in out]
        tok, pos = int(out[-1]), pos + W
    # the timed region, `--repeats` times over the SAME K steps (>= 3 repeats, median): every repeat restarts at the
    # same token and position (the steps overwrite the same KV rows with the same values), must produce the same tokens, and the median
    # repeat is the one reported -- value, ms_per_step and hip_event_ms_per_step all come from that single repeat of exactly K steps
    reps = []
    for rep in range(max(1, args.repeats)):
        lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx.h))            # barrier + synchronize before the timed region
        t0 = time.perf_counter()
        o_, ev_ = ctx.decode_greedy(tok, pos, K)                  # EXACTLY K steps; returns after stream sync
        t1 = time.perf_counter()
        reps.append((t1 - t0, ev_, [int(t) for t in o_]))
        if reps[-1][2] != reps[0][2]:
            sys.stderr.write("PARITY FAILURE: repeat %d of the timed region produced different tokens\n" % rep)
            sys.exit(3)
    if args.dump_outputs:
        # what decode_greedy handed its caller in the last timed repeat: K token ids (exact in float64).  The model (fill_synthetic(1234)) and
        # the prompt (synth_tokens(99, P)) are seeded, so the same arguments give the same inputs on every run and every build
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "decode_tokens.npy"), np.asarray(reps[-1][2], dtype=np.float64))
    order = sorted(range(len(reps)), key=lambda i: reps[i][0])
    med = order[len(order) // 2]
    t0, t1, ev_ms, out = 0.0, reps[med][0], reps[med][1], np.array(reps[med][2], dtype=np.int32)
    wall = t1 - t0
    tps = K / wall
    config = {"workload": "%s bf16, 1xMI355X, single-prompt greedy decode, seq_len=%d -> +%d tokens (%s)"
                          % (name, P, K, ("configs[2] decode" if P >= 4096 else
                                          "configs[1] proper: +256 tokens" if K == 256 else
                                          "configs[1]'s prompt and kernels with the caller's --steps %d; with --full the same context's next %d steps -- configs[1]'s +256 -- are `long_run`" % (K, K_LONG) if K_LONG else
                                          "configs[1]'s prompt, --steps %d" % K) if args.model == "llama8b" else "shape of configs[4] on one GPU" if args.model == "llama70b-like" else
                             "configs[2] workload on the %d-layer cut the CPU oracle reaches" % cfg["n_layers"] if args.model in ("llama8b-2l", "llama8b-8l") else "test shape"),
              "prompt_len": P, "sequences_in_flight": 1, "parallelism": "single GPU",
              "mode": "exact-order (token-id identical to the CPU reference path)" if args.mode == "exact" else
                      "fast (opt-in tolerance mode: split-K f32 sums, same bf16 truncation points; NOT token-identical, see NOTES.md 6.2)",
              "hip_event_ms_per_step": round(ev_ms / K, 4),
              "timed_region_repeats_ms_per_step": [round(1e3 * r[0] / K, 4) for r in reps], "reported_repeat": "median",
              "weight_bytes_resident": model.weight_bytes(), "model_build_s": round(t_load, 1)}     # (+ sequences_in_flight_batched.weights_second_copy_bytes once that section has run)
    res = {"metric": "decode tokens/s Llama-3.1-8B bf16 @1/2/4/8 MI355X; % HBM roofline", "value": round(tps, 2), "unit": "tokens/s",
           "n_gpus": 1, "steps": K, "warmup": W, "ms_per_step": round(1000.0 * wall / K, 4), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
           "schema": "lnb-bench/6 (without --full: the headline and its timed repeats only; --full adds roofline = the kernel symbol with the largest share of GPU time, "
                     "configs2 = configs[2] in the same line, sequences_in_flight = throughput forms)",
           "config": config}
    if not args.full:
        # the plain line: what the headline needs and nothing that takes a run of its own
        res["last_tokens"] = [int(t) for t in out[-4:]]
        res["prefill"] = {"rows": P, "ms": round(1e3 * t_pf, 2), "note": "the process's first call (cold); --full adds the warm and steady figures"}
        ctx.close(); model.close()
        print(json.dumps(res))
        return 0
    # fused-RMSNorm rows of the decode steps so far (2 per block + 1 per token) whose sum left the branch-free item walk (same bits, slower walk)
    n_norm_rows = (W + K * len(reps)) * (2 * cfg["n_layers"] + 1)
    norm_walk = {"rows": n_norm_rows, "fallback_rows": ctx.norm_fallbacks(), "note": "rows summed by the record walk instead of the branch-free item list (more than 64 items or non-finite terms; round 6: a leaf too close to a binade edge is replayed as single-term items inside the list)"} if args.mode == "exact" else None
    long_run = None
    if K_LONG:
        lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx.h))
        tl = time.perf_counter()
        out_long, _ = ctx.decode_greedy(int(out[-1]), pos + K, K_LONG)
        tl = time.perf_counter() - tl
        long_run = {"steps": K_LONG, "tokens_per_s": round(K_LONG / tl, 2), "ms_per_step": round(1e3 * tl / K_LONG, 4),
                    "note": "the same context continued for %d more steps after the %d timed ones (mean context %.1f)" % (K_LONG, K, pos + K + (K_LONG - 1) / 2.0 + 1.0)}
        golden_long = check_golden(args, first_tok, warm_toks, list(out) + list(out_long))
        if golden_long:
            long_run["tokens_vs_oracle_golden"] = golden_long
    golden_ok = check_golden(args, first_tok, warm_toks, out)
    self_check = None
    if golden_ok is None and args.model != "tiny":
        self_check = device_self_check(lnb, model, args, prompt, seq_len, [first_tok] + warm_toks + [int(t) for t in out])
    Tbar = pos + (K - 1) / 2.0 + 1.0
    a = {k: cfg[k] for k in ("dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size")}
    B = algorithmic_bytes_per_token(a, model.ffn_hidden, Tbar)

    # per-kernel HIP-event timings on the library's stream (eager launches cycling through the layers)
    kb = kernel_bytes(a, model.ffn_hidden, Tbar)
    kernels = {}
    for which in range(7):
        ms = ctx.profile_kernel(which, int(Tbar) - 1, args.profile_iters)
        kernels[KERNEL_NAMES[which]] = {"ms": round(ms, 5), "GB/s": (round(kb[which] / ms / 1e6, 1) if kb[which] else None)}
    dom = max(range(6), key=lambda i: (1 if i == 5 else cfg["n_layers"]) * kernels[KERNEL_NAMES[i]]["ms"])
    dom_ms = kernels[KERNEL_NAMES[dom]]["ms"]
    # The `roofline` object is that of the kernel SYMBOL with the largest share of the token's GPU time -- what rocprofv3 --stats ranks first
    # (wo and w2 are two launches of ONE symbol per block: VERDICT r3 #1d, r4 weak #3) -- per launch: algorithmic bytes and HIP-event time
    # averaged over the symbol's launches of one token.  The single heaviest launch CLASS (gate|up) is reported next to it as `dominant_class`.
    rc = "rowcast_lds_kernel (wo, w2)" if os.environ.get("LNB_ROWCAST_LDS", "1") != "0" else "rowcast_kernel (wo, w2)"
    sym_of = {0: "gemv_quad_kernel / gemv_chain_kernel (attn_norm+wq|wk|wv)", 1: "attn_exact_kernel", 2: rc, 3: "gemv_chain_kernel<56,2,..> (w1|w3)",
              4: rc, 5: "gemv_chain_kernel<64,1,..> (output)"}
    sym_t, sym_b, sym_n, sym_cls = {}, {}, {}, {}
    for i in range(6):
        nrep = 1 if i == 5 else cfg["n_layers"]
        sym_t[sym_of[i]] = sym_t.get(sym_of[i], 0.0) + nrep * kernels[KERNEL_NAMES[i]]["ms"]
        sym_b[sym_of[i]] = sym_b.get(sym_of[i], 0.0) + nrep * kb[i]
        sym_n[sym_of[i]] = sym_n.get(sym_of[i], 0) + nrep
        sym_cls.setdefault(sym_of[i], []).append(i)
    tot_t = sum(sym_t.values())
    top = max(sym_t, key=lambda k: sym_t[k])
    top_ms, top_bytes = sym_t[top] / sym_n[top], sym_b[top] / sym_n[top]           # per launch of the symbol
    traffic_live = None if args.no_traffic_probe else probe_traffic(args, sym_cls[top], int(Tbar) - 1)
    traffic, traffic_src, traffic_head = None, None, None
    if traffic_live:
        traffic, traffic_src = traffic_live["bytes_per_launch"], traffic_live["source"]
    else:                                                                          # the committed PMC pass, per class, averaged over the symbol's launches
        got = [pmc_traffic(KERNEL_NAMES[i], name, args.mode) for i in sym_cls[top]]
        if all(g[0] for g in got):
            traffic, traffic_src, traffic_head = int(sum(g[0] for g in got) / len(got)), got[0][1], got[0][2]
    symbols = {k: {"share_of_gpu_time": round(sym_t[k] / tot_t, 4), "launches_per_token": sym_n[k], "avg_launch_us": round(1e3 * sym_t[k] / sym_n[k], 2),
                   "frac": round(sym_b[k] / sym_t[k] / 1e6 / PEAK_HBM_GBS, 4)} for k in sym_t}
    roofline = {"bound": "hbm", "kernel": top, "share_of_gpu_time": round(sym_t[top] / tot_t, 4),
                "achieved": round(top_bytes / top_ms / 1e6, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(top_bytes / top_ms / 1e6 / PEAK_HBM_GBS, 4),
                "traffic": traffic, "traffic_source": traffic_src, "traffic_measured_in_run": bool(traffic_live), "traffic_profile_git_head": traffic_head,
                "algorithmic_bytes_per_launch": int(top_bytes), "avg_launch_ms": round(top_ms, 5),
                "note": "the kernel symbol with the largest share of a token's GPU time; bytes and time per launch are averages over its %d launches per token "
                        "(classes: %s)" % (sym_n[top], ", ".join(KERNEL_NAMES[i] for i in sym_cls[top])),
                "symbols": symbols,
                "dominant_class": {"kernel": KERNEL_NAMES[dom], "achieved": round(kb[dom] / dom_ms / 1e6, 1), "frac": round(kb[dom] / dom_ms / 1e6 / PEAK_HBM_GBS, 4),
                                   "algorithmic_bytes_per_launch": kb[dom], "avg_launch_ms": dom_ms},
                "whole_step": {"achieved": round(tps * B / 1e9, 1), "frac": round(tps * B / 1e9 / PEAK_HBM_GBS, 4),
                               "algorithmic_bytes_per_token": int(B), "mean_context": Tbar,
                               "roofline_tokens_per_s": round(PEAK_HBM_GBS * 1e9 / B, 1)}}
    config.update({"tokens_vs_oracle_golden": golden_ok, "device_self_check": self_check, "norm_item_walk": norm_walk})
    res.update({
           "roofline": roofline, "kernels": kernels, "last_tokens": [int(t) for t in out[-4:]], "long_run": long_run,
           # prefill of the prompt: the same exact f32 chains on the matrix cores (v_mfma_f32_16x16x4_f32, bit-identical to the
           # k-ordered loop); FLOPs = 2 x rows x layer-matmul elements; peak = f32 MFMA (MI355X_MICROARCH.md: 157.3 TFLOP/s)
           "prefill": {"rows": P, "ms": round(1e3 * t_pf, 2), "warm_ms": round(1e3 * t_pf_warm, 2) if t_pf_warm else None,
                       "steady_ms": round(1e3 * t_pf_steady, 2) if t_pf_steady else None,
                       "note": "ms = the process's first call (cold), warm_ms = the same prompt on a second, NEW context (its first call: per-context allocations inside), steady_ms = once more on that context after lnb_ctx_reset",
                       "TFLOP/s": round(2.0 * P * 6979321856 / t_pf / 1e12, 2) if name == "Llama-3.1-8B" else None,
                       "warm_frac_of_f32_mfma_peak": round(2.0 * P * 6979321856 / t_pf_warm / 1e12 / 157.3, 4) if (t_pf_warm and name == "Llama-3.1-8B") else None,
                       "peak_TFLOP/s": 157.3 if args.mode == "exact" else 2500.0,
                       "frac_of_bf16_mfma_peak_2500": round(2.0 * P * 6979321856 / t_pf / 1e12 / 2500.0, 4) if name == "Llama-3.1-8B" else None,
                       "kernel": "gemm_stream_kernel fed from the resident weight layouts (round 5: no second copy; LNB_PREFILL_NATIVE=0 = the LDS-tiled gemm_mfma_kernel)" if args.mode == "exact" else "fast_gemm_kernel",
                       "bound": "mfma (f32, exact order: v_mfma_f32_16x16x4_f32 is the k-ordered chain; the bf16 instructions are not)" if args.mode == "exact"
                                else "mfma (bf16, tolerance mode) / HBM at small row counts"}})
    if args.concurrent > 1 and os.environ.get("ROCP_TOOL_LIBRARIES") and os.environ.get("LNB_BENCH_CONCURRENT_UNDER_PROFILER") != "1":
        # rocprofv3 --kernel-trace --stats of this section (8 streams x captured stage graphs) has crashed inside the tool on long runs;
        # a profile is of the headline path anyway
        res["sequences_in_flight"] = {"skipped": "running under rocprofv3 (set LNB_BENCH_CONCURRENT_UNDER_PROFILER=1 to force)"}
    elif args.concurrent > 1:
        # several independent prompts in flight on the one GPU, one context and stream each (what a pipeline rank runs per stage; the N = 2
        # pipeline's regime is n = 2): the contexts take the THROUGHPUT forms of the one-token kernels; the same run with the single stream's
        # latency forms next to it (round 4 had only those: 308 -> 272 tokens/s at n = 8)
        run_toks = [first_tok] + warm_toks + [int(t) for t in out]
        res["sequences_in_flight"] = concurrent_sequences(lnb, model, cfg, args, a, run_toks)
        res["sequences_in_flight"]["latency_forms_same_run"] = {k: v for k, v in concurrent_sequences(lnb, model, cfg, args, a, run_toks, sched="latency").items()
                                                                if k in ("schedule", "tokens_per_s", "ms_per_token", "frac_of_hbm_roofline")}
        if args.concurrent != 2:
            two = concurrent_sequences(lnb, model, cfg, args, a, run_toks, n_seq=2)
            res["sequences_in_flight"]["n2"] = {k: v for k, v in two.items() if k != "note"}
            res["sequences_in_flight"]["n2"]["latency_forms_same_run"] = {k: v for k, v in concurrent_sequences(lnb, model, cfg, args, a, run_toks, n_seq=2, sched="latency").items()
                                                                          if k in ("schedule", "tokens_per_s", "ms_per_token", "frac_of_hbm_roofline")}
    if with_cfg2:
        res["configs2"] = configs2_record(lnb, model, cfg, args, a)
    roofline["measured_model"] = measured_model(ctx, a, model.ffn_hidden, Tbar, kernels, tps)
    if args.batch_sizes and args.mode == "exact" and not os.environ.get("ROCP_TOOL_LIBRARIES"):
        try:
            res["sequences_in_flight_batched"] = batched_sequences(lnb, model, cfg, args, a, [first_tok] + warm_toks + [int(t) for t in out])
        except lnb.LnbError as e:                                # (e.g. the second weight copy does not fit next to a 141 GB model)
            res["sequences_in_flight_batched"] = {"skipped": str(e)}
        ps = res["sequences_in_flight_batched"].get("prefill_streamed_4096")
        if ps and "configs2" in res:
            ps["first_token_same_as_configs2"] = bool(ps["first_token"] == res["configs2"]["first_token"])
    # what the HIP runtime gives this process's streams (lnb_runtime_info): the sequences_in_flight figures above depend on it
    rt = lnb.runtime_info(0, probe_queues=True)
    res["runtime"] = {k: rt[k] for k in ("abi_version", "device_name", "arch", "n_cus", "shader_clock_khz", "memory_clock_khz", "hw_queues_env", "hw_queues_set_by_library",
                                          "hip_initialised_before_load", "hw_queues_expected", "hw_queues_measured", "probe_ms")}
    warn = lnb.queue_warning(max(args.concurrent, 2), rt) if args.concurrent > 1 else None
    if warn:
        res["runtime"]["warning"] = warn
        sys.stderr.write("WARNING: " + warn + "\n")
    ctx.close(); model.close()
    if with_cfg4:
        res["configs4_one_gpu"] = configs4_record(lnb, args)
    if args.cpu_steps > 0:
        res["cpu_baseline"] = cpu_baseline(cfg, prompt[:8], args.cpu_steps)        # 8 + 24 = configs[0]'s seq_len of 32
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
