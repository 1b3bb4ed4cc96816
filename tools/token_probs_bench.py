#!/usr/bin/env python3
"""Cost of the token probabilities (include/lnb.h) on the 8B shape (configs[1]: synthetic weights seed 1234, 128-token prompts):
  * the single-sequence decode step with top-k 0 / 1 / 16 (device events of lnb_decode_greedy, runs of the settings alternated);
  * the batched step at 16 and 128 sequences with top-k 0 / 4 (device events of lnb_batch_decode);
  * lnb_forward_score against lnb_forward without logits at 128 and 4096 rows (host wall clock around the synchronous calls);
  * how many recorded rows walked the serial sum.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "llama-nuts-and-bolts_amd")]
import lnb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=64, help="decode steps per measured run")
ap.add_argument("--repeats", type=int, default=3, help="measured runs per setting (settings alternated)")
ap.add_argument("--batch-steps", type=int, default=16)
ap.add_argument("--batches", default="16,128")
a = ap.parse_args()
lnb.build()
V = 128256
m = lnb.LlamaTransformer(**lnb.LLAMA_8B).fill_synthetic(1234).finalize()
res = {"what": "token probabilities on configs[1] (8B shape, synthetic weights 1234)", "steps": a.steps, "repeats": a.repeats}

# ---- single sequence ----
c = lnb.InferenceContext(m, 128 + a.steps + 8)
_, first = c.Forward(lnb.synth_tokens(99, 128, V), 0, want_logits=False)
ks = (0, 1, 16)
times = {k: [] for k in ks}
walks = {k: 0 for k in ks}
recorded = {k: 0 for k in ks}
for k in ks:                                                 # warm-up: captures each setting's graph once
    c.set_token_probs(k)
    c.decode_greedy(first, 128, 8)
for _ in range(a.repeats):
    for k in ks:
        c.set_token_probs(k)                                 # (drops and re-captures the graph: the warm-up replay below absorbs it)
        c.decode_greedy(first, 128, 4)
        w0 = c.token_prob_walks()
        _, ms = c.decode_greedy(first, 128, a.steps)
        times[k].append(ms / a.steps)
        walks[k] += c.token_prob_walks() - w0
        recorded[k] += a.steps if k else 0
c.close()
res["single_ms_per_step"] = {str(k): min(v) for k, v in times.items()}
res["single_overhead_us"] = {str(k): 1e3 * (min(times[k]) - min(times[0])) for k in ks if k}
res["single_walks"] = {str(k): "%d of %d steps" % (walks[k], recorded[k]) for k in ks if k}

# ---- batches ----
for n in [int(x) for x in a.batches.split(",") if x]:
    ctxs = [lnb.InferenceContext(m, 128 + a.batch_steps + 8) for _ in range(n)]
    firsts = [cc.Forward(lnb.synth_tokens(99 + s, 128, V), 0, want_logits=False)[1] for s, cc in enumerate(ctxs)]
    bt = {0: [], 4: []}
    bw = 0
    for rep in range(a.repeats + 1):
        for k in (0, 4):
            for cc in ctxs:
                cc.set_token_probs(k)
            b = lnb.Batch(ctxs)
            b.decode(firsts, [128] * n, 2)                   # warm-up (graph capture)
            w0 = sum(cc.token_prob_walks() for cc in ctxs)
            _, ms = b.decode(firsts, [128] * n, a.batch_steps)
            b.close()
            if rep:
                bt[k].append(ms / a.batch_steps)
                if k:
                    bw += sum(cc.token_prob_walks() for cc in ctxs) - w0
    for cc in ctxs:
        cc.close()
    res["batch%d_ms_per_step" % n] = {str(k): min(v) for k, v in bt.items()}
    res["batch%d_overhead_us" % n] = 1e3 * (min(bt[4]) - min(bt[0]))
    res["batch%d_walks" % n] = "%d of %d rows" % (bw, a.repeats * a.batch_steps * n)

# ---- scoring ----
for P in (128, 4096):
    tok = lnb.synth_tokens(5, P, V)
    tg = np.concatenate([tok[1:], [-1]]).astype(np.int32)
    cc = lnb.InferenceContext(m, P)
    tf, ts = [], []
    w0 = cc.token_prob_walks()
    for rep in range(a.repeats + 1):
        t0 = time.perf_counter(); cc.Forward(tok, 0, want_logits=False); t1 = time.perf_counter()
        cc.score(tok, 0, tg); t2 = time.perf_counter()
        if rep:
            tf.append(t1 - t0); ts.append(t2 - t1)
    res["score%d_wall_ms" % P] = {"forward": 1e3 * min(tf), "forward_score": 1e3 * min(ts)}
    res["score%d_walks" % P] = "%d of %d rows" % (cc.token_prob_walks() - w0, (a.repeats + 1) * P)
    cc.close()
m.close()
print(json.dumps(res))
