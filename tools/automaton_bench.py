#!/usr/bin/env python3
"""What a token automaton costs in the sampling loops (include/lnb.h: lnb_ctx_set_automaton) on the 8B shape (synthetic weights seed 1234, 128-token prompts,
256 steps): lnb_decode_sample_rules_until with rules all off, with and without an automaton whose one state allows every token (the same tokens by
construction, asserted), for one context and for batches of 16 and 128.  The two variants are alternated, --repeats runs each (at least five); median / min /
max tokens/s.  Writes a markdown report (--out) and prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=256)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--batches", default="16,128")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_automaton.md"))
a = ap.parse_args()
assert a.repeats >= 5, "at least five runs per variant"
sys.path[:0] = [ROOT, os.path.join(ROOT, "llama-nuts-and-bolts_amd")]
import lnb  # noqa: E402

V, P, SMP, OFF = 128256, 128, (0.7, 40, 0.9, 1234), (1.0, 0.0, 0.0, 0.0)
lnb.build()
m = lnb.LlamaTransformer(**lnb.LLAMA_8B).fill_synthetic(1234).finalize()
free = lnb.TokenAutomaton(m, [0, V], np.arange(V), np.zeros(V))      # one state, every token allowed, back to itself
res = {}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def alternate(run):
    """run(constrained) -> (tokens, ms); -> {variant: tokens/s spread}, the tokens being the same"""
    run(False), run(True)                                    # captures
    rate = {False: [], True: []}
    for _ in range(a.repeats):
        toks = {}
        for on in (False, True):
            toks[on], ms = run(on)
            rate[on].append(sum(len(t) for t in toks[on]) / ms * 1e3)
        assert all((x == y).all() for x, y in zip(toks[False], toks[True])), "an allow-everything automaton changed a token"
    return {"rules off": spread(rate[False]), "rules off + automaton": spread(rate[True])}


c = lnb.InferenceContext(m, P + a.steps + 8)
_, first = c.Forward(lnb.synth_tokens(99, P, V), 0, want_logits=False)


def one(on):
    c.set_automaton(free if on else None, 0)
    t, _, ms = c.decode_sample_until(SMP, first, P, a.steps, rules=OFF)
    return [t], ms


res["1"] = alternate(one)
c.set_automaton(None)
c.close()
if a.batches:
    m.enable_batch()
for n in [int(x) for x in a.batches.split(",") if x]:
    ctxs = [lnb.InferenceContext(m, P + a.steps + 8) for _ in range(n)]
    firsts = [int(x.Forward(lnb.synth_tokens(100 + s, P, V), 0, want_logits=False)[1]) for s, x in enumerate(ctxs)]

    def many(on):                                            # which members hold an automaton is fixed while a batch lives: a batch per run, built outside the timed call
        for x in ctxs:
            x.set_automaton(free if on else None, 0)
        b = lnb.Batch(ctxs)
        b.decode_sample_until([SMP] * n, firsts, [P] * n, 2, rules=[OFF] * n)      # capture outside the timed call
        t, ms = b.decode_sample_until([SMP] * n, firsts, [P] * n, a.steps, rules=[OFF] * n)
        b.close()
        return t, ms

    res[str(n)] = alternate(many)
    for x in ctxs:
        x.set_automaton(None)
        x.close()
free.close()
m.close()
lines = ["# The cost of a token automaton in the sampling loops", "",
         "`python tools/automaton_bench.py --steps %d --repeats %d --batches %s` on one MI355X: the 8B shape with synthetic weights, %d-token prompts, %d steps," %
         (a.steps, a.repeats, a.batches, P, a.steps),
         "sampler (0.7, 40, 0.9), `lnb_decode_sample_rules_until` / `lnb_batch_decode_sample_rules_until` with rules all off, alternated with the same call under an",
         "automaton whose one state allows every token (the token sequences are asserted identical).  Tokens/s, median (min .. max) of %d runs." % a.repeats, "",
         "| generations | rules off | rules off + automaton | automaton / plain |", "|---|---|---|---|"]
for n, r in res.items():
    p, q = r["rules off"], r["rules off + automaton"]
    lines.append("| %s | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.4f |" % (n, p["median"], p["min"], p["max"], q["median"], q["min"], q["max"], q["median"] / p["median"]))
open(a.out, "w").write("\n".join(lines) + "\n")
print(json.dumps(res))
