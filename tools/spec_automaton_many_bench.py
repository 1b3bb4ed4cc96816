"""Speculative decoding of many contexts under token automata against the batched sampling loop under the same automata, on the same build (MI355X).

Shape: Llama 8B with synthetic weights (--layers of them).  Automaton: tools/spec_automaton_bench.py's schema -- a free state followed by a forced run of R
one-token states, four times round; R = 0 has no forced state.  Per (requests, R): n requests with different prompts and seeds run the same generations through
lnb_decode_speculative_automaton_many and through lnb_batch_decode_sample_rules_until (a live batch of n other contexts with the same rows) ALTERNATELY,
--reps times each after one warm-up of both; every member's tokens and end state are compared before anything is timed; the device time of each call (its
own events) is reported as median and range.

    python tools/spec_automaton_many_bench.py --out profiles/spec_automaton_many.json --md profiles/spec_automaton_many.md
    python tools/spec_automaton_many_bench.py --from-json profiles/spec_automaton_many.json --md profiles/spec_automaton_many.md      (no GPU: the table again)"""
import argparse, json, os, statistics, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llama-nuts-and-bolts_amd"))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--requests", default="4,8,16")
ap.add_argument("--runs", default="0,2,6,14", help="forced run lengths R")
ap.add_argument("--budgets", default="0,64", help="col_budget values; 0 = the default, 16 * ceil(n / 16), which leaves 16 requests no column to draft in")
ap.add_argument("--max-draft", type=int, default=15)
ap.add_argument("--out")
ap.add_argument("--md")
ap.add_argument("--from-json")
a = ap.parse_args()
P0, SEQ, SAMPLER, RULES = 32, 512, (0.7, 40, 0.9), (1.3, 0.5, 0.25, 0.02, ())


def schema(V, R, groups=4):
    """free state g * (R + 1) allows everything and leads to its forced run's first state; forced state j allows one token and leads on; the last wraps round"""
    n = groups * (R + 1)
    rows, nxt = [], []
    for s in range(n):
        free = s % (R + 1) == 0
        rows.append(np.arange(V, dtype=np.int32) if free else np.array([(7919 * s + 13) % V], dtype=np.int32))
        nxt.append(np.full(rows[-1].size, (s + 1) % n, dtype=np.int32))
    return np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64), np.concatenate(rows), np.concatenate(nxt)


def mmr(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def measure():
    import lnb
    cfg = dict(lnb.LLAMA_8B, n_layers=a.layers)
    V = cfg["vocab_size"]
    m = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize().enable_batch()
    res = {"layers": a.layers, "steps": a.steps, "reps": a.reps, "max_draft": a.max_draft, "sampler": SAMPLER, "rules": RULES[:4], "cells": []}
    for n in (int(v) for v in a.requests.split(",")):
        prompts = [[int(t) for t in lnb.synth_tokens(99 + s, P0, V)] for s in range(n)]
        smps = [SAMPLER + (777 + s,) for s in range(n)]
        many, live = ([lnb.InferenceContext(m, SEQ) for _ in range(n)] for _ in range(2))
        first = [int(c.Forward(p, 0, want_logits=False)[1]) for c, p in zip(many, prompts)]
        for c, p in zip(live, prompts):
            c.Forward(p, 0, want_logits=False)
        for c in many:
            c.set_draft(a.max_draft, 1, 3)
        for budget, R in ((int(b), int(r)) for b in a.budgets.split(",") for r in a.runs.split(",")):
            dfa = lnb.TokenAutomaton(m, *schema(V, R))
            for c in many + live:
                c.set_automaton(dfa, 0)
            bat = lnb.Batch(live)

            def spec():
                [c.set_automaton(dfa, 0) for c in many]
                got, fin, st, info, ms = lnb.DecodeSpeculativeAutomatonMany(many, smps, prompts, first, [P0] * n, a.steps, rules=[RULES] * n, counted=prompts, col_budget=budget)
                return got, [c.automaton_state() for c in many], (st, info), ms

            def loop():
                [c.set_automaton(dfa, 0) for c in live]
                got, ms = bat.decode_sample_until(smps, first, [P0] * n, a.steps, rules=[RULES] * n, counted=prompts)
                return got, [c.automaton_state() for c in live], None, ms

            (g1, s1, (st, info), _), (g2, s2, _, _) = spec(), loop()      # warm-up of both; the same tokens and end states or nothing is timed
            if s1 != s2 or any(len(x) != len(y) or (x != y).any() for x, y in zip(g1, g2)):
                raise SystemExit("n = %d, budget %d, R = %d: the speculative call and the batched sampling loop disagree" % (n, budget, R))
            t_spec, t_loop = [], []
            for _ in range(a.reps):                          # alternated: drift hits both alike
                t_spec.append(spec()[3]); t_loop.append(loop()[3])
            tokens = int(sum(len(x) for x in g1))
            cell = {"n": n, "budget": budget, "R": R, "tokens": tokens, "passes": info["passes"], "columns": info["columns"], "drafted": int(sum(s["drafted"] for s in st)),
                    "accepted": int(sum(s["accepted"] for s in st)), "spec_ms": mmr(t_spec), "loop_ms": mmr(t_loop),
                    "spec_tokens_per_s": round(tokens / statistics.median(t_spec) * 1e3, 1), "loop_tokens_per_s": round(tokens / statistics.median(t_loop) * 1e3, 1)}
            print(json.dumps(cell), flush=True)
            res["cells"].append(cell)
            bat.close()
            for c in many + live:
                c.set_automaton(None)
            dfa.close()
        for c in many + live:
            c.close()
    m.close()
    return res


def write_md(res, path):
    with open(path, "w") as f:
        f.write("# Speculative decoding of many contexts under token automata (`tools/spec_automaton_many_bench.py`)\n\n")
        f.write("Llama 8B shape, %d layers, synthetic weights; n requests with their own prompts and seeds, %d tokens each from position %d; sampler %s, rules %s;\n"
                "max_draft %d, n-grams 1..3; col_budget default = 16 * ceil(n / 16), which leaves 16 requests no column to draft in, or as stated.  The automaton is a free state (every token allowed) followed by a forced run of R one-token\n"
                "states, four times round.  `lnb_decode_speculative_automaton_many` and `lnb_batch_decode_sample_rules_until` under the same automata ran alternately on\n"
                "the same build, %d times each after a warm-up of both; every member's tokens and end state were compared first.  Device ms per call (the call's own\n"
                "events): median (min - max); tokens/s over all members.\n\n"
                % (res["layers"], res["steps"], P0, tuple(res["sampler"]), tuple(res["rules"]), res["max_draft"], res["reps"]))
        f.write("| requests | col_budget | R | passes | columns | drafted | accepted | speculative ms | batched loop ms | speculative tok/s | loop tok/s | ratio |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        fm = lambda d: "%.1f (%.1f - %.1f)" % (d["median"], d["min"], d["max"])
        for c in res["cells"]:
            f.write("| %d | %s | %d | %d | %d | %d | %d | %s | %s | %.1f | %.1f | %.2f |\n" % (c["n"], c["budget"] or "default", c["R"], c["passes"], c["columns"], c["drafted"], c["accepted"], fm(c["spec_ms"]),
                                                                                   fm(c["loop_ms"]), c["spec_tokens_per_s"], c["loop_tokens_per_s"],
                                                                                   c["spec_tokens_per_s"] / c["loop_tokens_per_s"]))
        lose = [c for c in res["cells"] if c["spec_tokens_per_s"] <= c["loop_tokens_per_s"]]
        f.write("\nRows where the call loses to the batched loop: %s.  At R = 0 no state is forced and a sampled text does not repeat, so every pass is one column per\n"
                "member plus the draft, filter and pack launches, the host's round trip and eager launches where the batched loop replays a captured graph.\n"
                "Where R > 0 loses, `drafted` is 0: the default col_budget of 16 gives 16 requests their one column each and none to draft in -- such a caller passes\n"
                "a larger col_budget.  The commit launch alone was not timed against `spec_many_sample_rules_commit_kernel`: no entry point repeats it between events.\n"
                % (", ".join("n = %d budget %s R = %d (%.3f)" % (c["n"], c["budget"] or "default", c["R"], c["spec_tokens_per_s"] / c["loop_tokens_per_s"]) for c in lose) or "none"))


res = json.load(open(a.from_json)) if a.from_json else measure()
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
if a.md:
    write_md(res, a.md)
