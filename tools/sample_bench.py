#!/usr/bin/env python3
"""What sampling costs (include/lnb.h: lnb_decode_sample_until) on the 8B shape (configs[1]: synthetic weights seed 1234, 128-token prompts, 256 steps):
  * lnb_decode_sample_until tokens/s for (temperature, top_k, top_p) = (1, 0, 1) and (0.7, 40, 0.9) next to lnb_decode_greedy_until;
  * the same for batches of 16 and 128 (lnb_batch_decode_sample_until next to lnb_batch_decode_until);
  * the HIP-event time of the sample launch alone next to the argmax launch it replaces (lnb_profile_sample).
The variants are alternated, --repeats runs each (at least five), and median / min / max are reported.  --parent-pkg DIR (a build of the parent commit's
package directory): its greedy figures are taken in child processes before and after this commit's, the comparator for "sampling costs x".
--phases: the token launch alone for samplers that switch the rule's parts on one by one.
Writes a markdown report (--out) and prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=256)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--batches", default="16,128")
ap.add_argument("--pkg", default=os.path.join(ROOT, "llama-nuts-and-bolts_amd"), help="package directory to import lnb from")
ap.add_argument("--greedy-only", action="store_true", help="only the greedy figures (what a parent build can run)")
ap.add_argument("--parent-pkg", default="", help="package directory of a build of the parent commit")
ap.add_argument("--phases", action="store_true", help="only the token launch alone, for samplers that switch the kernel's phases on one by one (one JSON line)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling.md"))
a = ap.parse_args()
assert a.repeats >= 5, "at least five runs per variant"
sys.path[:0] = [ROOT, a.pkg]
import lnb  # noqa: E402

V, P = 128256, 128
SAMPLERS = {"sample(1, 0, 1)": (1.0, 0, 1.0, 1234), "sample(0.7, 40, 0.9)": (0.7, 40, 0.9, 1234)}
VARIANTS = ["greedy"] + ([] if a.greedy_only else list(SAMPLERS))


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def measure():
    lnb.build()
    m = lnb.LlamaTransformer(**lnb.LLAMA_8B).fill_synthetic(1234).finalize()
    res = {}
    # ---- one context ----
    c = lnb.InferenceContext(m, P + a.steps + 8)
    _, first = c.Forward(lnb.synth_tokens(99, P, V), 0, want_logits=False)

    def run(name):
        if name == "greedy":
            _, _, ms = c.decode_greedy_until(first, P, a.steps)
        else:
            _, _, ms = c.decode_sample_until(SAMPLERS[name], first, P, a.steps)
        return 1e3 * a.steps / ms
    for name in VARIANTS:
        run(name)                                            # warm-up: captures the variant's graph
    tps = {n: [] for n in VARIANTS}
    for _ in range(a.repeats):
        for name in VARIANTS:                                # alternated
            tps[name].append(run(name))
    res["single_tokens_per_s"] = {n: spread(v) for n, v in tps.items()}
    if not a.greedy_only:
        us = {n: [] for n in VARIANTS}
        for _ in range(a.repeats):
            for name in VARIANTS:
                us[name].append(1e3 * c.profile_sample(None if name == "greedy" else SAMPLERS[name], P, 200))
        res["token_launch_us"] = {("argmax" if n == "greedy" else n): spread(v) for n, v in us.items()}
    c.close()
    # ---- batches ----
    m.enable_batch()
    for n in [int(x) for x in a.batches.split(",") if x]:
        ctxs = [lnb.InferenceContext(m, P + a.steps + 8) for _ in range(n)]
        firsts = [cc.Forward(lnb.synth_tokens(99 + s, P, V), 0, want_logits=False)[1] for s, cc in enumerate(ctxs)]
        b = lnb.Batch(ctxs)

        def brun(name):
            if name == "greedy":
                _, ms = b.decode_until(firsts, [P] * n, a.steps)
            else:
                t, k, p, seed = SAMPLERS[name]
                _, ms = b.decode_sample_until([(t, k, p, seed + s) for s in range(n)], firsts, [P] * n, a.steps)
            return 1e3 * a.steps * n / ms
        for name in VARIANTS:
            brun(name)
        bt = {nm: [] for nm in VARIANTS}
        for _ in range(a.repeats):
            for name in VARIANTS:
                bt[name].append(brun(name))
        res["batch%d_tokens_per_s" % n] = {nm: spread(v) for nm, v in bt.items()}
        b.close()
        for cc in ctxs:
            cc.close()
    m.close()
    return res


def parent_run():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--greedy-only", "--pkg", a.parent_pkg, "--steps", str(a.steps), "--repeats", str(a.repeats),
                        "--batches", a.batches], capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise SystemExit("parent run failed:\n" + r.stdout[-2000:] + r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def fmt(s, unit=""):
    return "%.1f%s (%.1f .. %.1f, %d runs)" % (s["median"], unit, s["min"], s["max"], s["runs"])


def phases():
    """lnb_profile_sample on a real head row of 128256 entries (the 8B head over one layer): what each part of the rule adds to the launch"""
    m = lnb.LlamaTransformer(**dict(lnb.LLAMA_8B, n_layers=1)).fill_synthetic(1234).finalize()
    c = lnb.InferenceContext(m, 64)
    _, f = c.Forward(lnb.synth_tokens(99, 8, V), 0, want_logits=False)
    c.decode_greedy_until(f, 8, 2)
    S = {"argmax": None, "t1_k0_p1": (1.0, 0, 1.0, 1), "t0.7_k0_p1": (0.7, 0, 1.0, 1), "t1_k40_p1": (1.0, 40, 1.0, 1), "t1_k1_p1": (1.0, 1, 1.0, 1),
         "t1_k0_p0.9": (1.0, 0, 0.9, 1), "t1_k0_p0.5": (1.0, 0, 0.5, 1), "t1_k40_p0.9": (1.0, 40, 0.9, 1), "t0.7_k40_p0.9": (0.7, 40, 0.9, 1)}
    us = {k: [] for k in S}
    for _ in range(a.repeats):
        for k, s in S.items():
            us[k].append(1e3 * c.profile_sample(s, 8, 200))
    c.close(); m.close()
    return {k: spread(v) for k, v in us.items()}


if a.phases:
    lnb.build()
    print(json.dumps(phases()))
    sys.exit(0)
if a.greedy_only:
    print(json.dumps(measure()))
    sys.exit(0)
out = {"what": "sampling on configs[1] (8B shape, synthetic weights 1234, %d-token prompts, %d steps)" % (P, a.steps)}
if a.parent_pkg:
    out["parent_before"] = parent_run()
out["this"] = measure()
if a.parent_pkg:
    out["parent_after"] = parent_run()
lines = ["# Sampling in the device loop: measured", "",
         "`tools/sample_bench.py`: the 8B shape (configs[1], synthetic weights 1234), %d-token prompts, %d steps per run, the variants alternated, median (min .. max)" % (P, a.steps),
         "of %d runs each.  Tokens/s from the device events around the replays; the token launch alone from `lnb_profile_sample`." % a.repeats, ""]
keys = ["single_tokens_per_s"] + ["batch%s_tokens_per_s" % n for n in a.batches.split(",") if n]
lines += ["| workload | variant | tokens/s | against greedy |", "|---|---|---|---|"]
for k in keys:
    g = out["this"][k]["greedy"]["median"]
    for side in ("parent_before", "parent_after"):
        if side in out:
            lines.append("| %s | greedy, parent commit (%s) | %s | |" % (k.replace("_tokens_per_s", ""), side.split("_")[1], fmt(out[side][k]["greedy"])))
    for name, s in out["this"][k].items():
        lines.append("| %s | %s | %s | %+.2f %% |" % (k.replace("_tokens_per_s", ""), name, fmt(s), 100.0 * (s["median"] / g - 1.0)))
lines += ["", "| token launch alone | microseconds |", "|---|---|"]
for name, s in out["this"]["token_launch_us"].items():
    lines.append("| %s | %s |" % (name, fmt(s, " us")))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(json.dumps(out))
