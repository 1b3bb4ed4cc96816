#!/usr/bin/env python3
"""Sharing a computed prefix (lnb_ctx_fork) at the 8B synthetic shape, one process.  Per cell (prefix positions x fan-out), wall time around the call,
median of 5 after one warm-up:
  (a) lnb_ctx_fork on kv_fork_kernel (the default), and the kernel's other forms: non-temporal instead of plain accesses (LNB_FORK_NT=1), the
      destinations dealt over four workgroup groups (LNB_FORK_SPLIT=4);
  (b) the same call on the copy engine (LNB_FORK_COPY=1: hipMemcpy2DAsync for K, hipMemcpyAsync for V, per layer and destination);
  (c) what the fork replaces: n_dst x one measured prefill of that prefix (lnb_forward, want_logits off).
(a) and (b) also as moved bytes per second, (1 + n_dst) x prefix bytes over the time, beside the 6.29 TB/s of a plain 16-byte copy on this chip.
The source has the prefix's capacity; the destinations are lnb_ctx_create_long contexts of another capacity (so every K run is re-strided) with
16-row activation buffers, so that 127 of them fit beside the weights.  The rows forked are whatever the source's prefill left: contents do not matter.
    python tools/fork_bench.py [--layers 32] [--prefixes 128,1024,4096] [--fanouts 1,16,127] [--md profiles/prefix_fork.md] [--out x.json]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "llama-nuts-and-bolts_amd"))
import lnb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--prefixes", default="128,1024,4096")
ap.add_argument("--fanouts", default="1,16,127")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--copy-bw-tbs", type=float, default=6.29, help="the plain 16-byte copy this chip reaches, TB/s")
ap.add_argument("--out", default="")
ap.add_argument("--md", default="")
a = ap.parse_args()
T0 = time.time()
prefixes = [int(s) for s in a.prefixes.split(",")]
fanouts = [int(s) for s in a.fanouts.split(",")]
PMAX, NMAX = max(prefixes), max(fanouts)
cfg = dict(lnb.LLAMA_8B, n_layers=a.layers)
m = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize(rope_rows=2 * PMAX)
kv_dim = cfg["n_kv_heads"] * (cfg["dim"] // cfg["n_heads"])
pos_bytes = 2 * 2 * kv_dim * a.layers
src = lnb.InferenceContext(m, PMAX)
dsts = [lnb.InferenceContext(m, PMAX + 256, max_rows=16, long_context=True) for _ in range(NMAX)]
toks = lnb.synth_tokens(99, PMAX, cfg["vocab_size"])
# name -> environment of the call
FORMS = [("kernel", {}), ("kernel_nt", {"LNB_FORK_NT": "1"}), ("kernel_four_groups", {"LNB_FORK_SPLIT": "4"}), ("copy_engine", {"LNB_FORK_COPY": "1"})]
KNOBS = ("LNB_FORK_COPY", "LNB_FORK_NT", "LNB_FORK_SPLIT")


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


res = {"shape": {k: cfg[k] for k in ("dim", "n_layers", "n_heads", "n_kv_heads")}, "bytes_per_position": pos_bytes, "cells": [], "prefill_ms": {}}
for P in prefixes:
    res["prefill_ms"][P] = round(timed(lambda: src.Forward(toks[:P], 0, want_logits=False), 3), 3)
    print(json.dumps({"prefix": P, "prefill_ms": res["prefill_ms"][P]}), flush=True)
    for n in fanouts:
        cell = {"prefix": P, "n_dst": n, "moved_bytes": (1 + n) * P * pos_bytes, "replaces_ms": round(n * res["prefill_ms"][P], 1)}
        for name, env in FORMS:
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            ms = timed(lambda: src.ForkPrefix(dsts[:n], P), a.reps)
            cell[name + "_ms"] = round(ms, 4)
            cell[name + "_tbs"] = round(cell["moved_bytes"] / (ms * 1e-3) / 1e12, 3)
        for k in KNOBS:
            os.environ.pop(k, None)
        print(json.dumps(cell), flush=True)
        res["cells"].append(cell)
for c in dsts:
    c.close()
src.close(); m.close()
res["seconds"] = round(time.time() - T0, 1)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
if a.md:
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as f:
        f.write("# Sharing a computed prefix (`lnb_ctx_fork`): measurements\n\n`python tools/fork_bench.py --layers %d --prefixes %s --fanouts %s --md profiles/prefix_fork.md`, 8B synthetic shape, one process, "
                "MI355X.  Wall time around the call (it returns when the copy has finished), median of %d after one warm-up.  %d bytes per position per context; moved bytes = "
                "(1 + n_dst) x prefix bytes.  The plain 16-byte copy of this chip: %.2f TB/s.\n\n" % (a.layers, a.prefixes, a.fanouts, a.reps, pos_bytes, a.copy_bw_tbs))
        f.write("## The kernel (a), the copy engine (b), the prefills they replace (c)\n\n| prefix | n_dst | (a) kernel ms | TB/s | of the plain copy | (b) copy engine ms | TB/s | (b) / (a) | (c) n_dst x prefill ms | (c) / (a) |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for c in res["cells"]:
            f.write("| %d | %d | %.3f | %.2f | %.0f %% | %.3f | %.2f | %.1f | %.1f | %.0f |\n" % (c["prefix"], c["n_dst"], c["kernel_ms"], c["kernel_tbs"], 100 * c["kernel_tbs"] / a.copy_bw_tbs,
                    c["copy_engine_ms"], c["copy_engine_tbs"], c["copy_engine_ms"] / c["kernel_ms"], c["replaces_ms"], c["replaces_ms"] / c["kernel_ms"]))
        f.write("\nOne prefill: %s.\n" % ", ".join("%d positions %.1f ms" % (P, res["prefill_ms"][P]) for P in prefixes))
        f.write("\n## The kernel's forms\n\n| prefix | n_dst | default (plain accesses, one destination group) ms | non-temporal loads and stores ms | four destination groups ms |\n|---|---|---|---|---|\n")
        for c in res["cells"]:
            f.write("| %d | %d | %.3f | %.3f | %.3f |\n" % (c["prefix"], c["n_dst"], c["kernel_ms"], c["kernel_nt_ms"], c["kernel_four_groups_ms"]))
        # what the table decides (ISSUE: the kernel's reference is path (b) and the plain copy, not its own earlier runs)
        wide = [c for c in res["cells"] if c["n_dst"] >= 16]
        worst = min(res["cells"], key=lambda c: c["copy_engine_ms"] / c["kernel_ms"])
        best = max(res["cells"], key=lambda c: c["copy_engine_ms"] / c["kernel_ms"])
        lost = [c for c in res["cells"] if c["copy_engine_ms"] < c["kernel_ms"]]
        f.write("\n## What the table decides\n\n* **Kernel or copy engine.**  ")
        if lost:
            f.write("The copy engine is faster in: %s -- the default has to follow this crossover.\n" % ", ".join("%d x %d" % (c["prefix"], c["n_dst"]) for c in lost))
        else:
            f.write("The kernel is faster in every cell: the copy engine takes %.1f times as long at its best (%d positions into %d) and %.0f times at its worst (%d into %d).  "
                    "There is no crossover, so `LNB_FORK_COPY` stays 0.\n" % (worst["copy_engine_ms"] / worst["kernel_ms"], worst["prefix"], worst["n_dst"],
                                                                             best["copy_engine_ms"] / best["kernel_ms"], best["prefix"], best["n_dst"]))
        nt_wins = [c for c in res["cells"] if c["kernel_nt_ms"] < c["kernel_ms"]]
        nt_span = [100.0 * (c["kernel_nt_ms"] / c["kernel_ms"] - 1.0) for c in res["cells"]]
        f.write("* **Non-temporal or plain accesses.**  Non-temporal loads and stores are faster in %d of %d cells and between %+.1f %% and %+.1f %% of the plain form's time: "
                "the default is plain (`LNB_FORK_NT=0`).\n" % (len(nt_wins), len(res["cells"]), min(nt_span), max(nt_span)))
        sp_span = [100.0 * (c["kernel_four_groups_ms"] / c["kernel_ms"] - 1.0) for c in wide]
        f.write("* **Destinations over a grid dimension.**  At this shape the 64 arrays already fill the capped grid of 2048 workgroups at every prefix; four destination groups, "
                "each reading the source again, take %+.1f %% to %+.1f %% of the one-group time from 16 destinations on: the default is one group (`LNB_FORK_SPLIT=0`).\n"
                % (min(sp_span or [0.0]), max(sp_span or [0.0])))
        head = [c for c in res["cells"] if c["prefix"] == PMAX and c["n_dst"] == NMAX][0]
        f.write("* **Headline.**  %d positions into %d contexts: %.2f ms, %.2f TB/s of moved bytes = %.0f %% of the plain copy figure; the %d prefills it replaces take %.1f s, the copy engine %.2f ms.\n"
                % (head["prefix"], head["n_dst"], head["kernel_ms"], head["kernel_tbs"], 100 * head["kernel_tbs"] / a.copy_bw_tbs, head["n_dst"], head["replaces_ms"] / 1e3, head["copy_engine_ms"]))
        if head["kernel_tbs"] < 0.5 * a.copy_bw_tbs:
            f.write("\nThe kernel reaches less than half of the plain copy figure in the headline cell.  Of reads, stores and launch shape: the reads are 1 / %d of the traffic, so the "
                    "stores or the launch shape hold it back -- compare the one-destination row (launch shape alone) with this one (the store loop).\n" % (1 + head["n_dst"]))
        f.write("\nThe short prefixes: a K tile is 1024 vectors of ONE run, so at 128 positions a K workgroup has 128 of its 256 lanes busy in one of four unroll steps; the "
                "128-position rows above are what that costs.\n")
