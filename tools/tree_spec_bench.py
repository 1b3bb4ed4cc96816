"""A tree of n-gram drafts per verify pass (lnb_ctx_set_draft_branches) on the 8B shape: lnb_decode_speculative_until with branches 1 / 2 / 4 against
lnb_decode_greedy_until, runs alternated in one process, medians [min .. max] of --reps runs, every run's tokens checked against the greedy run's.

  python tools/tree_spec_bench.py [--prefix 128] [--steps 192] [--reps 3] [--out profiles/tree_spec_bench.json]
  python tools/tree_spec_bench.py --pkg <a checkout of the parent commit>/llama-nuts-and-bolts_amd      # the parent's figures: its binding, its library

--pkg: the package directory (lnb.py beside its built liblnb_hip.so) to measure; a package without lnb_ctx_set_draft_branches gets the branches = 1 rows only.
Corpora (profiles/spec_many.md's, plus one): "none" = no corpus (the overhead of drafting); "true" = the continuation itself; "every8" = every 8th token
wrong; "diverge" = the true continuation, then a copy of it with every 8th token wrong: the LATEST occurrence of an n-gram goes wrong where the EARLIER one
goes right.  --prefix 4000 puts the passes at T ~ 4100.  loop ms / pass = the whole loop's time (draft kernel, host round trip, pass) over ALL its passes."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefix", type=int, default=128)
    ap.add_argument("--steps", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--max-draft", type=int, default=6, help="15 leaves no column for a second candidate: the chain alone fills the pass")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "llama-nuts-and-bolts_amd"), help="the package directory to measure (default: this tree's)")
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    lnb = importlib.import_module("lnb")
    lnb.build()
    args.chain_only = not hasattr(lnb.lib(), "lnb_ctx_set_draft_branches")
    P, N, V = args.prefix, args.steps, lnb.LLAMA_8B["vocab_size"]
    model = lnb.LlamaTransformer(**dict(lnb.LLAMA_8B, n_layers=args.layers, max_seq_len=max(2048, P + N + 1))).fill_synthetic(1234).finalize().enable_batch()
    prompt = lnb.synth_tokens(99, P, V)
    ctx = lnb.InferenceContext(model, P + N + 1)
    _, first = ctx.Forward(prompt, 0, want_logits=False)
    want, _, _ = ctx.decode_greedy_until(first, P, N)
    true = np.concatenate([[first], want]).astype(np.int32)
    every8 = true.copy(); every8[7::8] = (every8[7::8] + 1) % V
    corpora = {"none": [], "true": true, "every8": every8, "diverge": np.concatenate([true, every8])}

    def set_draft(C, b):
        a = np.ascontiguousarray(C, dtype=np.int32)
        lnb._chk(ctx.L.lnb_ctx_set_draft(ctx.h, args.max_draft, 1, 4, lnb._p(a) if a.size else None, int(a.size)))
        if not args.chain_only:
            lnb._chk(ctx.L.lnb_ctx_set_draft_branches(ctx.h, b))

    rows = {(k, b): [] for k in corpora for b in ((1,) if args.chain_only else (1, 2, 4))}
    greedy, stats = [], {}
    for rep in range(args.reps + 1):                         # (the first round captures the graphs and is dropped)
        greedy.append(ctx.decode_greedy_until(first, P, N)[2])
        for (k, b), runs in rows.items():
            set_draft(corpora[k], b)
            out, _, st, ms = ctx.decode_speculative_until(prompt, first, P, N)
            assert (out == want).all(), "tokens differ from the greedy run (%s, branches %d)" % (k, b)
            runs.append(ms); stats[(k, b)] = st
    med = lambda xs: (statistics.median(xs[1:]), min(xs[1:]), max(xs[1:]))
    g = med(greedy)
    res = {"workload": "Llama-3.1-8B shape (%d layers), synthetic weights seed 1234, %d-token prompt, %d generated tokens, max_draft %d, n-grams 1..4, %d alternated runs"
                       % (args.layers, P, N, args.max_draft, args.reps), "library": os.path.abspath(args.pkg),
           "greedy": {"tokens_per_s": round(N / g[0] * 1e3, 1), "ms": [round(x, 3) for x in g]}, "rows": {}}
    for (k, b), runs in rows.items():
        m, st = med(runs), stats[(k, b)]
        res["rows"]["%s, branches %d" % (k, b)] = dict(st, tokens_per_s=round(N / m[0] * 1e3, 1), tokens_per_s_min=round(N / m[2] * 1e3, 1), tokens_per_s_max=round(N / m[1] * 1e3, 1),
                                                       accepted_per_pass=round(st["accepted"] / st["passes"], 3), loop_ms_per_pass=round(m[0] / st["passes"], 4),
                                                       loop_ms_per_pass_min=round(m[1] / st["passes"], 4), loop_ms_per_pass_max=round(m[2] / st["passes"], 4))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close(); model.close()


if __name__ == "__main__":
    main()
