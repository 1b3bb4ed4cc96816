#!/usr/bin/env python3
"""Host cost of a pipeline tick (what bench.py reports as host_enqueue_us_per_tick): a two-stage in-process pipeline of the tiny config on one
GPU, once with single-sequence ticks (4 sequences in flight) and once with batched ticks (4 groups of 3 sequences).  Timed: the wall time of
the tick loops only -- windows of 64 schedule steps, each ended by an untimed lnb_pipeline_sync.  Prints one JSON line; LNB_SO=<other build>
runs another build of the same ABI.
    python tools/pipeline_tick_host_bench.py [--decode 750]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "llama-nuts-and-bolts_amd")]
import lnb
from oracle import oracle as orc
import pipeline

ap = argparse.ArgumentParser()
ap.add_argument("--decode", type=int, default=750)
ap.add_argument("--window", type=int, default=64)
a = ap.parse_args()
cfg, world, P = dict(orc.TINY), 2, 6
V = cfg["vocab_size"]
stages = [lnb.LlamaTransformer(part_begin=x, part_end=y, **cfg).fill_synthetic(1234).finalize().enable_batch() for x, y in ((0, 3), (3, 6))]


def timed(step, pipes, n_steps):
    """step(t) enqueues schedule step t on both ranks; -> (seconds inside the loops, pipe ticks)"""
    spent = 0.0
    for lo in range(0, n_steps, a.window):
        t0 = time.perf_counter()
        for t in range(lo, min(lo + a.window, n_steps)):
            step(t)
        spent += time.perf_counter() - t0
        for p_ in pipes:
            p_.sync()
    return spent


def single():
    n_seq = 2 * world
    ctxs = [[lnb.InferenceContext(st, P + a.decode + 2) for _ in range(n_seq)] for st in stages]
    pipes = [lnb.Pipeline(stages[r], r, world, loopback_group="hostbench_single") for r in range(world)]
    prompts = [lnb.synth_tokens(70 + s, P, V) for s in range(n_seq)]
    state = [None] * world

    def step(t):
        for r in range(world):
            state[r] = pipeline.run_ticks_native(r, world, pipes[r], ctxs[r], prompts, a.decode, t, t + 1, state[r])
    n_steps = (1 + a.decode) * n_seq + 2 * (world - 1)
    s = timed(step, pipes, n_steps)
    for x in pipes + [c for cs in ctxs for c in cs]:
        x.close()
    return s * 1e6 / (n_steps * world)


def batched():
    G, n = 2 * world, 3
    ctxs = [[[lnb.InferenceContext(st, P + a.decode + 2) for _ in range(n)] for _ in range(G)] for st in stages]
    pipes = [lnb.Pipeline(stages[r], r, world, loopback_group="hostbench_batched") for r in range(world)]
    for g in range(G):
        for s in range(n):
            for r in range(world):
                pipeline.prefill_through_pipeline(r, world, pipes[r], ctxs[r][g][s], lnb.synth_tokens(900 + 16 * g + s, P, V))
    batches = [[lnb.Batch(ctxs[r][g]).set_state(None, [P] * n) for g in range(G)] for r in range(world)]
    state = [None] * world

    def step(t):
        for r in range(world):
            state[r] = pipeline.run_ticks_native_batched(r, world, pipes[r], batches[r], a.decode, t, t + 1, state[r])
    n_steps = a.decode * G + 2 * (world - 1)
    s = timed(step, pipes, n_steps)
    for x in [b for bs in batches for b in bs] + pipes + [c for cs in ctxs for grp in cs for c in grp]:
        x.close()
    return s * 1e6 / (n_steps * world)


single(); batched()                                          # warm-up: kernels loaded, graphs captured once per context anyway
print(json.dumps({"so": os.environ.get("LNB_SO", "in-tree"), "decode": a.decode, "single_us_per_tick": round(single(), 3), "batched_us_per_tick": round(batched(), 3)}), flush=True)
