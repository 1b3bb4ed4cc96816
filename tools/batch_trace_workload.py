#!/usr/bin/env python3
"""Every host path of the batched step once, on the tiny config, to be run under a kernel trace (rocprofv3 --kernel-trace -- python tools/batch_trace_workload.py;
LNB_SO=<other build> for the build to compare with; tools/compare_kernel_traces.py compares two such traces).  Sections, in this order: lnb_batch_decode at
3 / 17 / 33 sequences with the matrix-core copy, 3 without it, a speculative run with verify passes, lnb_forward_append_many calls whose passes change
width and layout (B-operand columns, column groups, rows), batched ticks of a two-stage in-process pipeline, single-sequence ticks of a two-stage
pipeline cut behind a gate/up part (two segments per hand-off).  A section starts with a marker: two exp-table
launches back to back, which nothing else issues."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "llama-nuts-and-bolts_amd")]
import numpy as np
import lnb
from oracle import oracle as orc
import pipeline

cfg = dict(orc.TINY)
V = cfg["vocab_size"]


def mark(name):
    lnb.op_exp_table(1.0); lnb.op_exp_table(1.0)
    print("section", name, flush=True)


def batched(gm, n, steps=3):
    plens = [3 + (5 * s) % 11 for s in range(n)]
    ctxs = [lnb.InferenceContext(gm, 32) for _ in range(n)]
    firsts = [ctxs[s].Forward(lnb.synth_tokens(7000 + s, plens[s], V), 0, want_logits=False)[1] for s in range(n)]
    b = lnb.Batch(ctxs)
    got, _ = b.decode(firsts, plens, steps)
    b.close()
    for c in ctxs:
        c.close()
    return got


plain = lnb.LlamaTransformer(**cfg).fill_synthetic(707).finalize()
copied = lnb.LlamaTransformer(**cfg).fill_synthetic(707).finalize().enable_batch()
for n in (3, 17, 33):
    mark("batch_copy_n%d" % n)
    batched(copied, n)
mark("batch_nocopy_n3")
batched(plain, 3)

mark("speculative")
c = lnb.InferenceContext(copied, 64)
prompt = lnb.synth_tokens(99, 8, V)
_, first = c.Forward(prompt, 0, want_logits=False)
want, _, _ = c.decode_greedy_until(first, 8, 24)
c.set_draft(5, 1, 4, want)
out, _, st, _ = c.decode_speculative_until(prompt, first, 8, 24)
assert (out == want).all() and st["verify_passes"] >= 1, st
print("spec stats", st, flush=True)
c.close()

mark("append_many")
ctxs = [lnb.InferenceContext(copied, 64) for _ in range(6)]
for W, rows in ((20, [9, 9, 9, 9, 9]), (40, [10, 10, 10, 10, 10]), (128, [1, 2, 3, 4, 5, 6])):
    os.environ["LNB_APPEND_MANY_COLS"] = str(W)
    m = ctxs[:len(rows)]
    lnb.ForwardAppendMany(m, [lnb.synth_tokens(300 + s, r, V) for s, r in enumerate(rows)], [0] * len(rows), want_logits=False)
    print("append_many", W, copied.append_many_info(), flush=True)
os.environ.pop("LNB_APPEND_MANY_COLS")
for x in ctxs:
    x.close()

mark("pipeline_two_stage")
cuts, n, P, n_decode = (0, 3, 6), 3, 6, 4
pcfg = dict(orc.TINY, n_layers=2)
world, G = 2, 4
stages = [lnb.LlamaTransformer(part_begin=a, part_end=b, **pcfg).fill_synthetic(1234).finalize().enable_batch() for a, b in zip(cuts[:-1], cuts[1:])]
pctx = [[[lnb.InferenceContext(st_, P + n_decode + 2) for _ in range(n)] for _ in range(G)] for st_ in stages]
pipes = [lnb.Pipeline(stages[r], r, world, loopback_group="trace") for r in range(world)]
prompts = [[lnb.synth_tokens(900 + 16 * g + s, P, V) for s in range(n)] for g in range(G)]
for g in range(G):
    for s in range(n):
        for r in range(world):
            pipeline.prefill_through_pipeline(r, world, pipes[r], pctx[r][g][s], prompts[g][s])
batches = [[lnb.Batch(pctx[r][g]).set_state(None, [P] * n) for g in range(G)] for r in range(world)]
state = [None] * world
for t in range(n_decode * G + 2 * (world - 1)):
    for r in range(world):
        state[r] = pipeline.run_ticks_native_batched(r, world, pipes[r], batches[r], n_decode, t, t + 1, state[r])
for p_ in pipes:
    p_.sync()

mark("pipeline_single_gate_up_cut")
cuts, P, n_decode = (0, 2, 6), 5, 4                          # the cut lies behind a gate/up part: hidden state + gate*up activations cross it
sstages = [lnb.LlamaTransformer(part_begin=a, part_end=b, **pcfg).fill_synthetic(1234).finalize() for a, b in zip(cuts[:-1], cuts[1:])]
n_seq = 2 * world
sctx = [[lnb.InferenceContext(st_, P + n_decode + 2) for _ in range(n_seq)] for st_ in sstages]
spipes = [lnb.Pipeline(sstages[r], r, world, loopback_group="trace_single") for r in range(world)]
sprompts = [lnb.synth_tokens(70 + s, P, V) for s in range(n_seq)]
state = [None] * world
for t in range((1 + n_decode) * n_seq + 2 * (world - 1)):
    for r in range(world):
        state[r] = pipeline.run_ticks_native(r, world, spipes[r], sctx[r], sprompts, n_decode, t, t + 1, state[r])
for p_ in spipes:
    p_.sync()
mark("end")
print("trace workload done", flush=True)
