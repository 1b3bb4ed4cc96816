"""Speculative greedy decoding with n-gram drafts on configs[1] (the 8B shape, synthetic weights seed 1234, the 128-token prompt of bench.py):
lnb_decode_speculative_until against lnb_decode_greedy_until, with and without the batch copy (lnb_model_enable_batch).

  python tools/spec_bench.py [--steps 287] [--out profiles/spec_bench.json]

Rows: plain greedy (the reference figure); drafting with no corpus (synthetic weights never repeat themselves: the OVERHEAD of a drafting
pass); corpus = the golden continuation, max_draft 3 / 7 / 15 (the CEILING); the same corpus with every m-th token corrupted, m = 2 / 4 / 8
(tokens/s against acceptance); one run per verify width w = max_draft + 1 with the golden corpus (device ms per pass: nearly every pass is
a verify pass of width w).  Each row is the median of 3 repeats, interleaved with greedy runs in the same process; every run's tokens are
checked against tests/golden/configs1_tokens.json.

  python tools/spec_bench.py --prefix 4096 [--seq-len N] [--long-threshold N] [--steps 64]
the verify passes at a long context: a prompt of --prefix tokens, the corpus = the context's own greedy continuation (checked against it),
rows greedy and width 2 / 8 / 16 only.  --seq-len: the context's capacity (beyond ~7.8 K the passes run the long-context attention);
--long-threshold N: lnb_ctx_set_batched_attention (0 = the long-context form in every verify pass).
--rows-attention: every width twice -- the long-context pair with the columns as grid.z (verify_attention_form 1) and the multi-row pair that reads K and V
once for all columns (lnb_ctx_set_rows_attention flags bit 1, form 2) -- median ms per pass of --reps runs with min..max, next to the one-token step."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "llama-nuts-and-bolts_amd"))

import numpy as np  # noqa: E402

import lnb  # noqa: E402


def long_prefix(args):
    """verify passes at a long context (no golden there: the context's own greedy run is the reference)"""
    P, N, V = args.prefix, min(args.steps, 64), lnb.LLAMA_8B["vocab_size"]
    cfg = dict(lnb.LLAMA_8B, n_layers=args.layers)
    need = P + N + 1
    model = lnb.LlamaTransformer(**cfg).fill_synthetic(1234).finalize(need if need > 2 * cfg["max_seq_len"] else 0)
    prompt = lnb.synth_tokens(99, P, V)
    result = {"workload": "Llama-3.1-8B shape (%d layers), synthetic weights seed 1234, prompt synth_tokens(99, %d), %d generated tokens, corpus = the greedy continuation"
                          % (args.layers, P, N), "seq_len": args.seq_len or need, "long_threshold": args.long_threshold, "forms": {}}
    for form in ("rows", "columns"):
        if form == "columns":
            model.enable_batch()
        ctx = lnb.InferenceContext(model, args.seq_len or need)
        if args.long_threshold is not None:
            ctx.set_batched_attention(args.long_threshold, 0)
        _, first = ctx.Forward(prompt, 0, want_logits=False)
        want, _, _ = ctx.decode_greedy_until(first, P, N)
        rows = {}
        for md, rows_flag in [(md, f) for md in (1, 7, 15) for f in ((0, 2) if args.rows_attention else (None,))]:
            ctx.set_draft(md, 1, 4, want)
            if rows_flag is not None:
                ctx.set_rows_attention(-1, rows_flag)
            runs = []
            for rep in range(args.reps + 1):                 # (the first run captures the graphs)
                out, _, st, ms = ctx.decode_speculative_until(prompt, first, P, N)
                assert (out == want).all(), "speculative: tokens differ from the greedy run"
                runs.append(ms)
            ms = statistics.median(runs[1:])
            name = "width%d" % (md + 1) + ("" if rows_flag is None else "_form%d" % (2 if rows_flag else 1))
            rows[name] = dict(st, hip_event_ms=round(ms, 3), ms_per_pass=round(ms / st["passes"], 4),
                              verify_attention_form=ctx.verify_attention_form() if hasattr(ctx, "verify_attention_form") else 0)
            if rows_flag is not None:
                rows[name].update(ms_per_pass_min=round(min(runs[1:]) / st["passes"], 4), ms_per_pass_max=round(max(runs[1:]) / st["passes"], 4))
        g = [ctx.decode_greedy_until(first, P, N)[2] for _ in range(args.reps)]
        rows["greedy"] = {"ms_per_token": round(statistics.median(g) / N, 4)}
        result["forms"][form] = rows
        ctx.close()
    model.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=287)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--prefix", type=int, default=None, help="prompt length (default: the 128 tokens of configs[1])")
    ap.add_argument("--seq-len", type=int, default=None, help="capacity of the context (default: prompt + steps + 1)")
    ap.add_argument("--long-threshold", type=int, default=None, help="lnb_ctx_set_batched_attention(N)")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rows-attention", action="store_true", help="with --prefix: each width on the long pair (form 1) and on the multi-row pair (form 2)")
    args = ap.parse_args()
    if args.prefix is not None:
        return long_prefix(args)
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "configs1_tokens.json")))
    gold = np.array(g["tokens"], dtype=np.int32)
    N, P = min(args.steps, gold.size - 1), 128
    V = lnb.LLAMA_8B["vocab_size"]
    model = lnb.LlamaTransformer(**lnb.LLAMA_8B).fill_synthetic(g["weights_seed"]).finalize()
    prompt = lnb.synth_tokens(g["prompt_seed"], P, V)

    def corrupted(m):
        c = gold.copy()
        c[m - 1::m] = (c[m - 1::m] + 1) % V
        return c

    configs = [("no_corpus_md7", 7, np.zeros(0, np.int32))]
    configs += [("golden_md%d" % md, md, gold) for md in (3, 7, 15)]
    configs += [("golden_corrupt_every%d_md7" % m, 7, corrupted(m)) for m in (2, 4, 8)]
    configs += [("width%d_golden" % (md + 1), md, gold) for md in (1, 5, 11)]
    result = {"workload": "configs[1]: Llama-3.1-8B shape, synthetic weights seed %d, prompt synth_tokens(%d, %d), %d generated tokens, n-grams 1..4"
                          % (g["weights_seed"], g["prompt_seed"], P, N), "forms": {}}
    for form in ("rows", "columns"):
        if form == "columns":
            model.enable_batch()
        ctx = lnb.InferenceContext(model, P + N + 1)
        _, first = ctx.Forward(prompt, 0, want_logits=False)
        assert first == gold[0]

        def greedy():
            lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx.h))
            t0 = time.perf_counter()
            out, _, ms = ctx.decode_greedy_until(first, P, N)
            wall = time.perf_counter() - t0
            assert (out == gold[1:N + 1]).all(), "greedy: tokens differ from the golden"
            return wall, ms, None

        def spec(md, corpus):
            ctx.set_draft(md, 1, 4, corpus)
            lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx.h))
            t0 = time.perf_counter()
            out, _, st, ms = ctx.decode_speculative_until(prompt, first, P, N)
            wall = time.perf_counter() - t0
            assert (out == gold[1:N + 1]).all(), "speculative: tokens differ from the golden"
            return wall, ms, st

        greedy()                                             # warm-up: graphs captured, verify batches built
        for _, md, corpus in configs:
            spec(md, corpus)
        runs = {"greedy": []}
        runs.update({name: [] for name, _, _ in configs})
        for rep in range(args.reps):
            for name, md, corpus in configs:
                runs["greedy"].append(greedy())
                runs[name].append(spec(md, corpus))
        rows = {}
        for name, rs in runs.items():
            wall = statistics.median(r[0] for r in rs)
            ms = statistics.median(r[1] for r in rs)
            row = {"tokens_per_s": round(N / wall, 1), "hip_event_ms": round(ms, 2), "hip_event_tokens_per_s": round(N / (ms / 1e3), 1),
                   "repeats_wall_ms": [round(1e3 * r[0], 2) for r in rs]}
            st = rs[0][2]
            if st is not None:
                row.update(st)
                row["accepted_per_pass"] = round(st["accepted"] / st["passes"], 3)
                row["ms_per_pass"] = round(ms / st["passes"], 3)
                if st["verify_passes"]:
                    row["accepted_per_verify_pass"] = round(st["accepted"] / st["verify_passes"], 3)
            rows[name] = row
        base = rows["greedy"]
        for name, row in rows.items():
            if name != "greedy":
                row["speedup_vs_greedy"] = round(row["tokens_per_s"] / base["tokens_per_s"], 3)
        rows["greedy"]["ms_per_token"] = round(base["hip_event_ms"] / N, 3)
        result["forms"][form] = rows
        ctx.close()
    model.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
