#!/usr/bin/env python3
"""Sampling in the speculative loops at the 8B shape (configs[1]: synthetic weights seed 1234, the 128-token prompt of bench.py, with the matrix-core copy):
lnb_decode_speculative_sample_until against lnb_decode_sample_until -- the existing loop, the baseline -- on the same prompt and sampler in one process.

    python tools/spec_sample_bench.py [--steps 256] [--reps 5] [--layers 32] [--out profiles/spec_sample.json] [--md profiles/spec_sample.md]

Per sampler ((1, 0, 1) and (0.7, 40, 0.9), seed 777) the reference is the sampling loop's own continuation; the corpus is that continuation (the ceiling: what a
perfect draft source gives), the same with every 8th token wrong, or empty (no draft is ever right on synthetic weights: the overhead of drafting).  Every
run's tokens are compared with the reference before its time counts.  Rows are medians of --reps runs alternated with the baseline, with their range:
  * the sampling speculative loop, max_draft 7, n-grams 1..4, tokens/s against the baseline;
  * the greedy speculative loop of this build on the golden continuation (tests/golden/configs1_tokens.json, max_draft 7): the figure to hold against
    profiles/spec_bench_configs1.json of the parent commit;
  * a pass: device ms per pass at widths 2 / 8 / 16 (max_draft 1 / 7 / 15 on the true corpus: nearly every pass has that width) with the sampling launch
    and with the greedy pair of launches -- what sampling 16 rows in one launch costs over 16 argmaxes;
  * the many form: 4 and 16 requests (the golden's prompts, sampler (0.7, 40, 0.9), each member's own continuation as its corpus) at the default budget
    against lnb_batch_decode_sample_until on the same members."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "llama-nuts-and-bolts_amd"))
import numpy as np  # noqa: E402
import lnb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--members", default="4,16")
ap.add_argument("--out", default="")
ap.add_argument("--md", default="")
a = ap.parse_args()
SAMPLERS = {"(1, 0, 1)": (1.0, 0, 1.0, 777), "(0.7, 40, 0.9)": (0.7, 40, 0.9, 777)}
P, N, MD, NGRAM = 128, a.steps, 7, (1, 4)
V = lnb.LLAMA_8B["vocab_size"]


def stat(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def every(c, m):
    c = np.array(c, dtype=np.int32).copy()
    if m:
        c[m - 1::m] = (c[m - 1::m] + 1) % V
    return c


def main():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "configs1_tokens.json")))
    cfg = dict(lnb.LLAMA_8B, n_layers=a.layers)
    model = lnb.LlamaTransformer(**cfg).fill_synthetic(gold["weights_seed"]).finalize()
    model.enable_batch()
    prompt = lnb.synth_tokens(gold["prompt_seed"], P, V)
    ctx = lnb.InferenceContext(model, P + N + 1)
    _, first = ctx.Forward(prompt, 0, want_logits=False)
    res = {"workload": "Llama-3.1-8B shape (%d layers), synthetic weights seed %d, prompt synth_tokens(%d, %d), %d steps, max_draft %d, n-grams %d..%d, with the "
                       "matrix-core copy; medians of %d runs alternated with the baseline [min .. max]" % (a.layers, gold["weights_seed"], gold["prompt_seed"], P, N, MD,
                                                                                                      NGRAM[0], NGRAM[1], a.reps), "single": {}, "pass": {}, "many": {}}
    sync = lambda: lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx.h))
    # ---- the sampling speculative loop against the sampling loop
    for name, smp in SAMPLERS.items():
        want, _, _ = ctx.decode_sample_until(smp, first, P, N)
        chain = np.concatenate([[first], want]).astype(np.int32)

        def base():
            sync()
            ms, (out, _, dev) = wall(lambda: ctx.decode_sample_until(smp, first, P, N))
            assert (out == want).all()
            return ms

        def spec(corpus, md=MD):
            ctx.set_draft(md, NGRAM[0], NGRAM[1], corpus)
            sync()
            ms, (out, _, st, dev) = wall(lambda: ctx.decode_speculative_sample_until(smp, prompt, first, P, N))
            assert (out == want).all(), "the speculative loop's tokens differ from the sampling loop's"
            return ms, st, dev

        rows = {}
        for kind, corpus in (("true continuation", chain), ("every 8th token wrong", every(chain, 8)), ("no corpus", np.zeros(0, np.int32))):
            spec(corpus)                                     # (captures what the runs replay)
            b, s, st = [], [], None
            for _ in range(a.reps):
                b.append(base())
                ms, st, _ = spec(corpus)
                s.append(ms)
            rows[kind] = dict(st, baseline_ms=stat(b), spec_ms=stat(s), baseline_tokens_per_s=round(N / statistics.median(b) * 1e3, 1),
                              spec_tokens_per_s=round(N / statistics.median(s) * 1e3, 1), speedup=round(statistics.median(b) / statistics.median(s), 3))
        res["single"][name] = rows
        # ---- a pass at widths 2 / 8 / 16 with the sampling launch
        for md in (1, 7, 15):
            spec(chain, md)
            runs = [spec(chain, md) for _ in range(a.reps)]
            st = runs[0][1]
            res["pass"].setdefault("width %d" % (md + 1), {})[name] = dict(passes=st["passes"], verify_passes=st["verify_passes"],
                                                                             ms_per_pass=stat([r[2] / st["passes"] for r in runs]))
    # ---- the greedy speculative loop of this build on the golden continuation, and its passes
    g = np.array(gold["tokens"], dtype=np.int32)
    Ng = min(N, g.size - 1)
    assert first == g[0]

    def gspec(md):
        ctx.set_draft(md, NGRAM[0], NGRAM[1], g)
        sync()
        ms, (out, _, st, dev) = wall(lambda: ctx.decode_speculative_until(prompt, first, P, Ng))
        assert (out == g[1:Ng + 1]).all()
        return ms, st, dev

    for md in (1, 7, 15):
        gspec(md)
        runs = [gspec(md) for _ in range(a.reps)]
        st = runs[0][1]
        res["pass"]["width %d" % (md + 1)]["greedy"] = dict(passes=st["passes"], verify_passes=st["verify_passes"], ms_per_pass=stat([r[2] / st["passes"] for r in runs]))
        if md == MD:
            res["greedy_spec"] = dict(st, steps=Ng, ms=stat([r[0] for r in runs]), tokens_per_s=round(Ng / statistics.median([r[0] for r in runs]) * 1e3, 1),
                                      tokens_per_s_range=[round(Ng / max(r[0] for r in runs) * 1e3, 1), round(Ng / min(r[0] for r in runs) * 1e3, 1)])
    ctx.close()
    # ---- the many form against the batched sampling loop
    multi = json.load(open(os.path.join(ROOT, "tests", "golden", "configs1_multi_P128_tokens.json")))
    Pm = multi["prompt_len"]
    Nm = min(N, 64)
    smp = SAMPLERS["(0.7, 40, 0.9)"]
    for n in [int(v) for v in a.members.split(",") if v]:
        prompts = [lnb.synth_tokens(multi["prompt_seed_base"] + s, Pm, V) for s in range(n)]
        smps = [smp[:3] + (777 + s,) for s in range(n)]
        ctxs, firsts = [], []
        for s in range(n):
            c = lnb.InferenceContext(model, Pm + Nm + 1)
            _, f = c.Forward(prompts[s], 0, want_logits=False)
            ctxs.append(c); firsts.append(int(f))
        bat = lnb.Batch(ctxs)
        want, _ = bat.decode_sample_until(smps, firsts, [Pm] * n, Nm)

        def batch():
            ms, (out, _) = wall(lambda: bat.decode_sample_until(smps, firsts, [Pm] * n, Nm))
            assert all((o == w).all() for o, w in zip(out, want))
            return ms

        b = [batch() for _ in range(a.reps + 1)][1:]
        bat.close()
        cell = {"steps": Nm, "batch_ms": stat(b), "batch_tokens_per_s": round(n * Nm / statistics.median(b) * 1e3, 1)}
        for kind, m in (("true continuation", 0), ("every 8th token wrong", 8)):
            for s in range(n):
                ctxs[s].set_draft(15, NGRAM[0], NGRAM[1], every(np.concatenate([[firsts[s]], want[s]]), m))

            def many():
                ms, (out, _, st, info, _) = wall(lambda: lnb.DecodeSpeculativeSampleMany(ctxs, smps, prompts, firsts, [Pm] * n, Nm, 0))
                assert all((o == w).all() for o, w in zip(out, want)), "a member's tokens differ from the batched sampling loop's"
                return ms, st, info

            runs = [many() for _ in range(a.reps + 1)][1:]
            cell[kind] = dict(runs[0][2], accepted=sum(s["accepted"] for s in runs[0][1]), ms=stat([r[0] for r in runs]),
                              tokens_per_s=round(n * Nm / statistics.median([r[0] for r in runs]) * 1e3, 1),
                              speedup=round(statistics.median(b) / statistics.median([r[0] for r in runs]), 3))
        res["many"]["%d requests" % n] = cell
        for c in ctxs:
            c.close()
    model.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))


def rng(s):
    return "%.1f [%.1f .. %.1f]" % (s["median"], s["min"], s["max"])


def markdown(r):
    out = ["## Measured (`tools/spec_sample_bench.py`)", "", r["workload"], "", "### The sampling speculative loop against `lnb_decode_sample_until`", "",
           "| sampler | corpus | passes | drafted | accepted | baseline ms | speculative ms | baseline tok/s | speculative tok/s | speed-up |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name, rows in r["single"].items():
        for kind, c in rows.items():
            out.append("| %s | %s | %d | %d | %d | %s | %s | %.1f | %.1f | %.3f |" % (name, kind, c["passes"], c["drafted"], c["accepted"], rng(c["baseline_ms"]), rng(c["spec_ms"]),
                                                                                   c["baseline_tokens_per_s"], c["spec_tokens_per_s"], c["speedup"]))
    gs = r["greedy_spec"]
    out += ["", "### The greedy speculative loop of this build", "",
            "Golden corpus, max_draft 7, %d steps: %.1f tokens/s [%.1f .. %.1f over the runs], %d passes, %d accepted." % (gs["steps"], gs["tokens_per_s"], gs["tokens_per_s_range"][0],
                                                                                                                         gs["tokens_per_s_range"][1], gs["passes"], gs["accepted"]),
            "", "### A pass (device ms per pass, true corpus)", "", "| width | " + " | ".join(next(iter(r["pass"].values())).keys()) + " |", "|---|" + "---|" * len(next(iter(r["pass"].values())))]
    for w, cols in r["pass"].items():
        out.append("| %s | " % w + " | ".join("%.3f [%.3f .. %.3f] (%d passes)" % (c["ms_per_pass"]["median"], c["ms_per_pass"]["min"], c["ms_per_pass"]["max"], c["passes"]) for c in cols.values()) + " |")
    out += ["", "### The many form against `lnb_batch_decode_sample_until` (sampler (0.7, 40, 0.9), max_draft 15, default budget)", "",
            "| requests | corpus | passes | columns | accepted | batched loop ms | many ms | batched tok/s | many tok/s | speed-up |", "|---|---|---|---|---|---|---|---|---|---|"]
    for n, cell in r["many"].items():
        for kind in ("true continuation", "every 8th token wrong"):
            c = cell[kind]
            out.append("| %s | %s | %d | %d | %d | %s | %s | %.1f | %.1f | %.3f |" % (n, kind, c["passes"], c["columns"], c["accepted"], rng(cell["batch_ms"]), rng(c["ms"]),
                                                                                   cell["batch_tokens_per_s"], c["tokens_per_s"], c["speedup"]))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
