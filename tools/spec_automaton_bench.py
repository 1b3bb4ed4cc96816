"""Speculative decoding under a token automaton against the sampling loop under the same automaton, on the same build (MI355X).

Shape: Llama 8B with synthetic weights (--layers of them).  Automaton: schema-like -- a free state (every token allowed) followed by a forced run of R one-token
states, four times round; R = 0 is a grammar without forced states, where the call can only lose its filter launch unless the text repeats.  Per R:
lnb_decode_speculative_automaton_until and lnb_decode_sample_rules_until run the same generation ALTERNATELY, --reps times each after one warm-up of both; the
tokens and the end state are compared before anything is timed; the device time of each call (its own events) is reported as median and range.
Then the verify pass's token launch ALONE: spec_sample_dfa_commit_kernel under an automaton that allows everything (so both launches sample the same rows to
the same tokens: what differs is the mask row's staging and the rank) against spec_sample_rules_commit_kernel on the same host rows, w in {2, 16}, alternately.

    python tools/spec_automaton_bench.py --out profiles/spec_automaton.json --md profiles/spec_automaton.md
    python tools/spec_automaton_bench.py --from-json profiles/spec_automaton.json --md profiles/spec_automaton.md      (no GPU: the table again)"""
import argparse, json, os, statistics, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llama-nuts-and-bolts_amd"))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=200, help="launches per timing of the token launch alone")
ap.add_argument("--runs", default="0,2,6,14", help="forced run lengths R")
ap.add_argument("--max-draft", type=int, default=15)
ap.add_argument("--out")
ap.add_argument("--md")
ap.add_argument("--from-json")
a = ap.parse_args()
P0, SEQ, SAMPLER, RULES = 32, 512, (0.7, 40, 0.9, 777), (1.3, 0.5, 0.25, 0.02, ())


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
    prompt = [int(t) for t in lnb.synth_tokens(99, P0, V)]
    res = {"layers": a.layers, "steps": a.steps, "reps": a.reps, "max_draft": a.max_draft, "sampler": SAMPLER, "rules": RULES[:4], "cells": []}
    for R in (int(r) for r in a.runs.split(",")):
        dfa = lnb.TokenAutomaton(m, *schema(V, R))
        c = lnb.InferenceContext(m, SEQ)
        _, first = c.Forward(prompt, 0, want_logits=False)
        c.set_draft(a.max_draft, 1, 3)

        def spec():
            c.set_automaton(dfa, 0)
            got, fin, st, ms = c.decode_speculative_automaton_until(SAMPLER, prompt, int(first), P0, a.steps, rules=RULES, counted=prompt)
            return got, c.automaton_state(), st, ms

        def loop():
            c.set_automaton(dfa, 0)
            got, fin, ms = c.decode_sample_until(SAMPLER, int(first), P0, a.steps, rules=RULES, counted=prompt)
            return got, c.automaton_state(), None, ms

        (g1, s1, st, _), (g2, s2, _, _) = spec(), loop()      # warm-up of both: graphs captured; the same tokens and end state or nothing is timed
        if len(g1) != len(g2) or (g1 != g2).any() or s1 != s2:
            raise SystemExit("R = %d: the speculative call and the sampling loop disagree" % R)
        t_spec, t_loop = [], []
        for _ in range(a.reps):                              # alternated: drift hits both alike
            t_spec.append(spec()[3]); t_loop.append(loop()[3])
        cell = {"R": R, "tokens": int(len(g1)), "stats": st, "spec_ms": mmr(t_spec), "loop_ms": mmr(t_loop),
                "spec_tokens_per_s": round(len(g1) / statistics.median(t_spec) * 1e3, 1), "loop_tokens_per_s": round(len(g1) / statistics.median(t_loop) * 1e3, 1)}
        print(json.dumps(cell), flush=True)
        res["cells"].append(cell)
        c.set_automaton(None); c.close(); dfa.close()
    m.close()
    # the token launch alone, on gaussian rows: average device ms over --iters launches per call, the two kernels alternately
    rng = np.random.default_rng(5)
    free = (np.array([0, V], dtype=np.int64), np.arange(V, dtype=np.int32), np.zeros(V, dtype=np.int32))
    res["launch"] = []
    for w in (2, 16):
        rows = (rng.normal(0.0, 2.2, size=(w, V)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        col = [int(t) for t in rng.integers(0, V, size=w)]
        t_dfa, t_rules = [], []
        for i in range(a.reps + 1):
            d = lnb.profile_spec_automaton_verify(rows, SAMPLER, RULES, None, P0, col, free, 0, a.iters)
            r = lnb.profile_spec_verify(rows, SAMPLER, RULES, None, P0, col, a.iters)
            if i:                                            # (the first pair is the warm-up)
                t_dfa.append(d * 1e3); t_rules.append(r * 1e3)
        cell = {"w": w, "iters": a.iters, "dfa_us": mmr(t_dfa), "rules_us": mmr(t_rules)}
        print(json.dumps(cell), flush=True)
        res["launch"].append(cell)
    return res


def write_md(res, path):
    with open(path, "w") as f:
        f.write("# Speculative decoding under a token automaton (`tools/spec_automaton_bench.py`)\n\n")
        f.write("Llama 8B shape, %d layers, synthetic weights; %d tokens per run from position %d; sampler %s, rules %s; max_draft %d, n-grams 1..3.  The automaton\n"
                "is a free state (every token allowed) followed by a forced run of R one-token states, four times round.  `lnb_decode_speculative_automaton_until` and\n"
                "`lnb_decode_sample_rules_until` under the same automaton ran alternately on the same build, %d times each after a warm-up of both; tokens and end state\n"
                "were compared first.  Device ms per call (the call's own events): median (min - max).\n\n"
                % (res["layers"], res["steps"], P0, tuple(res["sampler"]), tuple(res["rules"]), res["max_draft"], res["reps"]))
        f.write("| R | passes | verify passes | drafted | accepted | speculative ms | sampling loop ms | speculative tok/s | loop tok/s | ratio |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for c in res["cells"]:
            s, fm = c["stats"], lambda d: "%.1f (%.1f - %.1f)" % (d["median"], d["min"], d["max"])
            f.write("| %d | %d | %d | %d | %d | %s | %s | %.1f | %.1f | %.2f |\n" % (c["R"], s["passes"], s["verify_passes"], s["drafted"], s["accepted"], fm(c["spec_ms"]), fm(c["loop_ms"]),
                                                                             c["spec_tokens_per_s"], c["loop_tokens_per_s"], c["spec_tokens_per_s"] / c["loop_tokens_per_s"]))
        f.write("\nThe verify pass's token launch alone, microseconds per launch (average of %d launches per timing, %d timings each, alternated), on gaussian rows under an\n"
                "automaton that allows everything, so that both kernels sample the same rows to the same tokens:\n\n"
                "| w | `spec_sample_dfa_commit_kernel` | `spec_sample_rules_commit_kernel` | difference |\n|---|---|---|---|\n" % (res["launch"][0]["iters"], res["reps"]))
        fu = lambda d: "%.2f (%.2f - %.2f)" % (d["median"], d["min"], d["max"])
        for c in res["launch"]:
            f.write("| %d | %s | %s | %+.2f |\n" % (c["w"], fu(c["dfa_us"]), fu(c["rules_us"]), c["dfa_us"]["median"] - c["rules_us"]["median"]))
        ratio = {c["R"]: c["spec_tokens_per_s"] / c["loop_tokens_per_s"] for c in res["cells"]}
        f.write("\nWhere the call pays: R = %s (%s times the sampling loop) -- a forced run is a certain draft, one pass emits it whole.  Where callers should stay with\n"
                "`lnb_decode_sample_rules_until`: R = %s (%s) -- no forced state and a sampled text without repeats, so every pass is the one-token graph plus the filter\n"
                "launch and the host's round trip.  The verify launch itself costs the difference column more than the rules form's per pass: the mask row's staging and\n"
                "the rank.\n" % (", ".join(str(r) for r, v in ratio.items() if v > 1), ", ".join("%.2f" % v for v in ratio.values() if v > 1),
                             ", ".join(str(r) for r, v in ratio.items() if v <= 1) or "none", ", ".join("%.3f" % v for v in ratio.values() if v <= 1) or "-"))

res = json.load(open(a.from_json)) if a.from_json else measure()
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
if a.md:
    write_md(res, a.md)
