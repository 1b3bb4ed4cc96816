#!/usr/bin/env python3
"""Speculative decoding of many contexts (lnb_decode_speculative_many) at the 8B synthetic shape, one process, first without and then with the
matrix-core copy.  Prompts and corpora come from tests/golden/configs1_multi_P128_tokens.json: member s has the golden's prompt s (128 tokens) and
generates the golden's 29 tokens behind its first; its corpus is its own golden continuation, uncorrupted or with every 2nd / 4th / 8th token wrong
(the acceptance a real corpus would give is somewhere between).  Every member drafts with max_draft 15 and n-grams of 1..4 tokens; what it is
GRANTED is the budget's business.  Before anything is timed, every member's tokens of every form are compared with the golden: a run that differs
is not timed.  Per cell (members x budget x corpus), wall time around the call, median and range of --reps repeats after one warm-up, against
  (a) lnb_batch_decode_until on the same members (one column each, a captured graph per step), and
  (b) the members one after the other through lnb_decode_speculative_until (same draft settings),
and a run in which no member drafts (max_draft 0) against (a): the loop's own overhead.  Every measured step runs under its own time limit.
    python tools/spec_many_bench.py [--layers 32] [--members 2,4,8,16] [--budgets 0,32,128] [--forms rows,columns] [--md profiles/spec_many.md] [--out x.json]"""
import argparse, json, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "llama-nuts-and-bolts_amd"))
import numpy as np  # noqa: E402
import lnb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--members", default="2,4,8,16")
ap.add_argument("--budgets", default="0,32,128", help="0 = the default, 16 * ceil(n / 16)")
ap.add_argument("--corpora", default="0,8,4,2", help="every k-th corpus token wrong; 0 = uncorrupted")
ap.add_argument("--forms", default="rows,columns", help="rows = without the matrix-core copy, columns = with it (in this order: the copy cannot be dropped)")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--step-timeout", type=int, default=120)
ap.add_argument("--out", default="")
ap.add_argument("--md", default="")
ap.add_argument("--from-json", default="", help="write --md from the --out file of an earlier run instead of measuring")
a = ap.parse_args()
T0 = time.time()
ints = lambda s: [int(v) for v in s.split(",") if v != ""]
MEMBERS, BUDGETS, CORPORA, FORMS = ints(a.members), ints(a.budgets), ints(a.corpora), [f for f in a.forms.split(",") if f]
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "configs1_multi_P128_tokens.json")))
P, NMAX = GOLD["prompt_len"], max(MEMBERS)
STEPS = min(GOLD["n_tokens"][str(s)] for s in range(NMAX)) - 1
MD, NGRAM = 15, (1, 4)


def limited(fn):
    def on_alarm(*_):
        print(json.dumps({"error": "step exceeded %d s" % a.step_timeout}), flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(a.step_timeout)
    try:
        return fn()
    finally:
        signal.alarm(0)


def timed(fn):
    fn()
    out, last = [], None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        last = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(out), 3), "min": round(min(out), 3), "max": round(max(out), 3)}, last


def measure():
    cfg = dict(lnb.LLAMA_8B, n_layers=a.layers)
    V = cfg["vocab_size"]
    full = a.layers == 32                                     # the golden is the 32-layer model's: a cut model is timed against its own greedy tokens
    m = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(GOLD["weights_seed"]).finalize()
    prompts = [lnb.synth_tokens(GOLD["prompt_seed_base"] + s, P, V) for s in range(NMAX)]
    ctxs = [lnb.InferenceContext(m, P + STEPS + 1) for _ in range(NMAX)]
    firsts = [int(limited(lambda c=c, p=p: c.Forward(p, 0, want_logits=False))[1]) for c, p in zip(ctxs, prompts)]
    if full:
        want = [[int(t) for t in GOLD["tokens"][str(s)][:STEPS + 1]] for s in range(NMAX)]
        assert firsts == [w[0] for w in want], "prefill differs from the golden: nothing is timed"
    else:
        want = [[firsts[s]] + [int(t) for t in limited(lambda s=s: ctxs[s].decode_greedy(firsts[s], P, STEPS))[0]] for s in range(NMAX)]

    def corpus(s, k):
        c = np.array(want[s], dtype=np.int32)
        if k:
            c[k - 1::k] = (c[k - 1::k] + 1) % V
        return c

    def check(toks, n, what):
        for s in range(n):
            if [int(t) for t in toks[s]] != want[s][1:]:
                raise SystemExit("%s: member %d differs from the golden tokens: this run is not timed" % (what, s))

    res = {"shape": {k: cfg[k] for k in ("dim", "n_layers", "n_heads", "n_kv_heads")}, "reps": a.reps, "steps": STEPS, "prompt_len": P, "forms": {}}
    for form in FORMS:
        if form == "columns":
            limited(m.enable_batch)
        cells, base = [], {}
        for n in MEMBERS:
            mem, hist, pos = ctxs[:n], prompts[:n], [P] * n
            bat = lnb.Batch(mem)
            ta, got = limited(lambda: timed(lambda: bat.decode_until(firsts[:n], pos, STEPS)[0]))
            bat.close()
            check(got, n, "%s: lnb_batch_decode_until, %d members" % (form, n))
            for c in mem:
                c.set_draft(0)
            tn, r = limited(lambda: timed(lambda: lnb.DecodeSpeculativeMany(mem, hist, firsts[:n], pos, STEPS, 0)))
            check(r[0], n, "%s: no drafts, %d members" % (form, n))
            base[n] = {"members": n, "batch_ms": ta, "no_draft_ms": tn, "no_draft_passes": r[3]["passes"], "no_draft_device_ms": round(r[4], 3)}
            print(json.dumps(dict(base[n], form=form)), flush=True)
            for k in CORPORA:
                for s, c in enumerate(mem):
                    c.set_draft(MD, NGRAM[0], NGRAM[1], corpus(s, k))

                def seq():
                    return [c.decode_speculative_until(hist[s], firsts[s], P, STEPS)[0] for s, c in enumerate(mem)]
                tb, got = limited(lambda: timed(seq))
                check(got, n, "%s: lnb_decode_speculative_until, %d members, corpus %d" % (form, n, k))
                for B in BUDGETS:
                    if B and B < n:
                        continue
                    t, r = limited(lambda: timed(lambda: lnb.DecodeSpeculativeMany(mem, hist, firsts[:n], pos, STEPS, B)))
                    toks, _, stats, info, dev_ms = r
                    check(toks, n, "%s: %d members, budget %d, corpus %d" % (form, n, B, k))
                    mp = sum(st["passes"] for st in stats)
                    cell = {"members": n, "budget": B, "corrupt_every": k, "ms": t, "device_ms": round(dev_ms, 3), "sequential_spec_ms": tb,
                            "passes": info["passes"], "verify_passes": info["verify_passes"], "columns": info["columns"], "max_columns": info["max_columns"],
                            "ms_per_pass": round(t["median"] / info["passes"], 3), "mean_width": round(info["columns"] / info["passes"], 1),
                            "accepted_per_member_pass": round(sum(st["accepted"] for st in stats) / mp, 2),
                            "tokens_per_s": round(n * STEPS / t["median"] * 1e3), "batch_tokens_per_s": round(n * STEPS / ta["median"] * 1e3),
                            "sequential_tokens_per_s": round(n * STEPS / tb["median"] * 1e3)}
                    print(json.dumps(dict(cell, form=form)), flush=True)
                    cells.append(cell)
        res["forms"][form] = {"cells": cells, "base": [base[n] for n in MEMBERS]}
    for c in ctxs:
        c.close()
    m.close()
    res["seconds"] = round(time.time() - T0, 1)
    return res


def write_md(res, path):
    mmr = lambda d: "%.1f (%.1f - %.1f)" % (d["median"], d["min"], d["max"])
    steps = res["steps"]
    with open(path, "w") as f:
        f.write("# Speculative decoding of many contexts (`lnb_decode_speculative_many`): measurements\n\n")
        f.write("`python tools/spec_many_bench.py --layers %d --members %s --budgets %s --corpora %s --forms %s --reps %d --md profiles/spec_many.md`, 8B synthetic shape, one process, MI355X.  "
                "Member s continues the golden prompt s (%d tokens) by %d tokens; every member drafts with max_draft %d, n-grams %d..%d, from its own golden continuation with every k-th "
                "token wrong (k = 0: none).  Every run's tokens were compared with `tests/golden/configs1_multi_P128_tokens.json` before it was timed.  Wall time around the call in ms, median "
                "(fastest - slowest) of %d repeats after one warm-up.  (a) = `lnb_batch_decode_until` on the same members; (b) = the members one after the other through "
                "`lnb_decode_speculative_until`.  Budget 0 = the default, 16 * ceil(n / 16).\n\n"
                % (res["shape"]["n_layers"], a.members, a.budgets, a.corpora, a.forms, res["reps"], res["prompt_len"], steps, MD, NGRAM[0], NGRAM[1], res["reps"]))
        for form, R in res["forms"].items():
            f.write("## %s\n\n" % ("Without the matrix-core copy (rows of the streaming product)" if form == "rows" else "With the matrix-core copy (`lnb_model_enable_batch`)"))
            f.write("### No member drafts: the loop's own overhead against (a)\n\n| members | (a) ms | (a) ms per step | this call, max_draft 0, ms | ms per pass | overhead per pass ms |\n|---|---|---|---|---|---|\n")
            step = {}
            for b in R["base"]:
                step[b["members"]] = b["batch_ms"]["median"] / steps
                f.write("| %d | %s | %.3f | %s | %.3f | %+.3f |\n" % (b["members"], mmr(b["batch_ms"]), step[b["members"]], mmr(b["no_draft_ms"]), b["no_draft_ms"]["median"] / b["no_draft_passes"],
                                                             (b["no_draft_ms"]["median"] - b["batch_ms"]["median"]) / b["no_draft_passes"]))
            f.write("\n### Drafting\n\n| members | budget | every k-th wrong | ms | passes (widest, mean width) | ms per pass | accepted per member and pass | tokens/s | (a) tokens/s | (b) ms | (b) tokens/s | vs (a) | vs (b) |\n"
                    "|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for c in R["cells"]:
                f.write("| %d | %d | %d | %s | %d (%d, %.1f) | %.2f | %.2f | %d | %d | %s | %d | %.2fx | %.2fx |\n" % (
                    c["members"], c["budget"], c["corrupt_every"], mmr(c["ms"]), c["passes"], c["max_columns"], c["mean_width"], c["ms_per_pass"], c["accepted_per_member_pass"],
                    c["tokens_per_s"], c["batch_tokens_per_s"], mmr(c["sequential_spec_ms"]), c["sequential_tokens_per_s"],
                    c["tokens_per_s"] / c["batch_tokens_per_s"], c["tokens_per_s"] / c["sequential_tokens_per_s"]))
            f.write("\n### Break-even acceptance\n\nA pass of this call emits 1 + accepted tokens per member and costs its `ms per pass`; a step of (a) emits one and costs `(a) ms per step`.  "
                    "The call wins over (a) when accepted per member and pass exceeds `ms per pass / (a) ms per step - 1` (the pass time taken from the uncorrupted-corpus cell of the "
                    "budget, whose passes are the widest the budget gives).\n\n| members | budget | ms per pass | (a) ms per step | break-even accepted per member and pass |\n|---|---|---|---|---|\n")
            for c in R["cells"]:
                if c["corrupt_every"] == 0:
                    f.write("| %d | %d | %.2f | %.3f | %.2f |\n" % (c["members"], c["budget"], c["ms_per_pass"], step[c["members"]], max(c["ms_per_pass"] / step[c["members"]] - 1, 0)))
            lost_a = [c for c in R["cells"] if c["tokens_per_s"] < c["batch_tokens_per_s"]]
            lost_b = [c for c in R["cells"] if c["tokens_per_s"] < c["sequential_tokens_per_s"]]
            cell = lambda c: "%d members, budget %d, every %d-th wrong (%d against %d tokens/s)"
            f.write("\n### Which entry point\n\n")
            f.write("* Cells that LOSE to (a) `lnb_batch_decode_until`: %s.\n" % ("; ".join(cell(c) % (c["members"], c["budget"], c["corrupt_every"], c["tokens_per_s"], c["batch_tokens_per_s"]) for c in lost_a) or "none"))
            f.write("* Cells that LOSE to (b) sequential `lnb_decode_speculative_until`: %s.\n\n" % ("; ".join(cell(c) % (c["members"], c["budget"], c["corrupt_every"], c["tokens_per_s"], c["sequential_tokens_per_s"]) for c in lost_b) or "none"))
        F = res["forms"].get("columns") or next(iter(res["forms"].values()))
        which = "with the matrix-core copy" if "columns" in res["forms"] else "without the matrix-core copy"
        ratio = lambda c: c["tokens_per_s"] / c["batch_tokens_per_s"]
        by_b = lambda B: [c for c in F["cells"] if c["budget"] == B]
        over = [(b["no_draft_ms"]["median"] - b["batch_ms"]["median"]) / b["no_draft_passes"] for b in F["base"]]
        stepms = [b["batch_ms"]["median"] / steps for b in F["base"]]
        f.write("## Decisions (from the tables %s)\n\n" % which)
        f.write("* **The default budget stays at one tile of 16 columns.**  A pass of up to 16 columns costs what a step of (a) costs (%.2f - %.2f ms against %.2f - %.2f), so whatever the "
                "default budget grants is free: its worst cell is %.2fx of (a) and its best %.2fx.  A second tile is not free -- %.2f - %.2f ms per pass at budget 32, %.2f - %.2f at 128 -- "
                "and a run whose drafts are never accepted then falls to %.2fx (budget 32) and %.2fx (budget 128) of (a).  A larger budget is the caller's decision, taken from the acceptance "
                "it expects: the break-even tables above give the accepted drafts per member and pass it needs.  With 16 members the default grants no drafts and the call is (a) plus its "
                "own overhead; such a caller passes 32 or more.\n"
                % (min(c["ms_per_pass"] for c in by_b(0)), max(c["ms_per_pass"] for c in by_b(0)), min(stepms), max(stepms), min(map(ratio, by_b(0))), max(map(ratio, by_b(0))),
                   min(c["ms_per_pass"] for c in by_b(32)), max(c["ms_per_pass"] for c in by_b(32)), min(c["ms_per_pass"] for c in by_b(128)), max(c["ms_per_pass"] for c in by_b(128)),
                   min(map(ratio, by_b(32))), min(map(ratio, by_b(128)))))
        f.write("* **The loop stays eager.**  With no member drafting, a pass runs the step's kernels plus the draft, pack, setup and commit launches and one host round trip, eagerly launched, "
                "against (a)'s replayed graph: %+.3f to %+.3f ms per pass, %.1f %% of the step at most.  The launches do not show behind a %.1f ms pass; a graph per (width, form) would "
                "add up to 128 x 2 captures per model handle to save that.  The whole-buffer zeroing when a pass narrows is inside these figures as well and stays.\n"
                % (min(over), max(over), 100 * max(o / t for o, t in zip(over, stepms)), min(stepms)))
        f.write("* **Which entry point.**  Several requests whose text repeats itself or a corpus (code edits, retrieval, summaries): this call -- at the default budget it does not lose to (a) "
                "beyond its overhead, and it beats (b), the per-request speculative loops, in every cell measured %s because the weights are read once per pass for all members.  Requests whose "
                "drafts are rarely accepted, and 16 or more requests at the default budget: `lnb_batch_decode_until`, the same pass without the drafting work.  ONE request: "
                "`lnb_decode_speculative_until`, whose passes are captured graphs and whose no-draft pass is the context's own one-token step.\n\n" % which)
        f.write("Total run time of the measurement %.0f s.\n" % res["seconds"])


res = json.load(open(a.from_json)) if a.from_json else measure()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
if a.md:
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    write_md(res, a.md)
