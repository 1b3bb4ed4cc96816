#!/usr/bin/env python3
"""Ragged appends to many contexts (lnb_forward_append_many) at the 8B synthetic shape, one process, the matrix-core copy enabled.
A source context is prefilled to the prefix and forked (lnb_ctx_fork) into the members; per cell (members x rows per member at a prefix), wall time
around the call, median and range of --reps repeats after one warm-up:
  (a) the ONE call lnb_forward_append_many over all members (argmax only; selected cells also with the logits);
  (b) what it replaces: the loop of one lnb_forward_append per member on the same contexts (argmax only; the same bits, so the caches may be overwritten);
  (c) the batched decode step at the pass width and positions -- the same kernels under a captured graph, and launched eagerly (LNB_NO_GRAPH=1) --
      from lnb_batch_decode's own event time per step;
and the number of passes, so that (a) / passes stands next to (c).  Every measured step runs under its own time limit (--step-timeout, SIGALRM: a step
that overruns ends the process with status 124 after its partial results were printed).
    python tools/append_many_bench.py [--layers 32] [--members 8,32,127] [--rows 4,8,16] [--prefixes 128,1024] [--md profiles/append_many.md] [--out x.json]"""
import argparse, json, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "llama-nuts-and-bolts_amd"))
import lnb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--members", default="8,32,127")
ap.add_argument("--rows", default="4,8,16")
ap.add_argument("--prefixes", default="128,1024")
ap.add_argument("--extra", default="4x128", help="further cells, members x rows, comma separated (measured at every prefix)")
ap.add_argument("--logits-cells", default="32x8,4x128", help="cells that are also measured with the logits copied to the host")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=120, help="seconds one measured step (warm-up + repeats of one form of one cell) may take")
ap.add_argument("--out", default="")
ap.add_argument("--md", default="")
ap.add_argument("--from-json", default="", help="write --md from the --out file of an earlier run instead of measuring")
a = ap.parse_args()
T0 = time.time()
pairs = lambda s: [tuple(int(v) for v in c.split("x")) for c in s.split(",") if c]
prefixes = [int(s) for s in a.prefixes.split(",")]
cells = [(n, r) for n in (int(s) for s in a.members.split(",")) for r in (int(s) for s in a.rows.split(","))] + pairs(a.extra)
logit_cells = set(pairs(a.logits_cells))
NMAX, RMAX, PMAX = max(max(n for n, _ in cells), 128), max(r for _, r in cells), max(prefixes)
CAP = PMAX + RMAX + 64


def limited(fn):
    """one step under its own time limit"""
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
    out = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(out), 3), "min": round(min(out), 3), "max": round(max(out), 3)}


cfg = dict(lnb.LLAMA_8B, n_layers=a.layers)
V = cfg["vocab_size"]


def measure():
    m = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize(rope_rows=max(2048, CAP)).enable_batch()
    src = lnb.InferenceContext(m, CAP, max_rows=PMAX, long_context=True)
    ctxs = [lnb.InferenceContext(m, CAP, max_rows=max(RMAX, 16), long_context=True) for _ in range(NMAX)]     # 128 of them: a batch of the full pass width needs 128 members
    toks = lnb.synth_tokens(99, PMAX, V)
    user = [lnb.synth_tokens(1000 + s, RMAX, V) for s in range(NMAX)]
    batches = {}

    def batch_step(width, P, steps=4):
        """lnb_batch_decode's event time per step: `width` members at position P (the rows it writes are rewritten by every append that follows)"""
        if width not in batches:
            batches[width] = lnb.Batch(ctxs[:width])
        b = batches[width]
        first = [int(user[s][0]) for s in range(width)]
        b.decode(first, [P] * width, steps)
        ms = [b.decode(first, [P] * width, steps)[1] / steps for _ in range(a.reps)]
        return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}

    res = {"shape": {k: cfg[k] for k in ("dim", "n_layers", "n_heads", "n_kv_heads")}, "reps": a.reps, "cells": []}
    for P in prefixes:
        limited(lambda: src.Forward(toks[:P], 0, want_logits=False))
        limited(lambda: src.ForkPrefix(ctxs, P))
        for n, r in cells:
            members, lists, pos = ctxs[:n], [user[s][:r] for s in range(n)], [P] * n
            cell = {"prefix": P, "members": n, "rows": r, "total_rows": n * r}
            cell["one_call_ms"] = limited(lambda: timed(lambda: lnb.ForwardAppendMany(members, lists, pos, want_logits=False)))
            info = m.append_many_info()
            cell["passes"], cell["max_columns"], cell["long_passes"] = info["passes"], info["max_columns"], info["long_passes"]
            if (n, r) in logit_cells:
                cell["one_call_logits_ms"] = limited(lambda: timed(lambda: lnb.ForwardAppendMany(members, lists, pos, want_logits=True)))

            def loop():
                for c, t in zip(members, lists):
                    c.ForwardAppend(t, P, want_logits=False)
            cell["loop_ms"] = limited(lambda: timed(loop))
            width = info["max_columns"]
            os.environ.pop("LNB_NO_GRAPH", None)
            cell["batch_step_graph_ms"] = limited(lambda: batch_step(width, P))
            os.environ["LNB_NO_GRAPH"] = "1"
            cell["batch_step_eager_ms"] = limited(lambda: batch_step(width, P))
            os.environ.pop("LNB_NO_GRAPH", None)
            cell["per_pass_ms"] = round(cell["one_call_ms"]["median"] / cell["passes"], 3)
            cell["loop_min_over_call_median"] = round(cell["loop_ms"]["min"] / cell["one_call_ms"]["median"], 2)
            print(json.dumps(cell), flush=True)
            res["cells"].append(cell)
    for b in batches.values():
        b.close()
    for c in ctxs:
        c.close()
    src.close(); m.close()
    res["seconds"] = round(time.time() - T0, 1)
    return res


res = json.load(open(a.from_json)) if a.from_json else measure()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
if a.md:
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    mmr = lambda d: "%.1f (%.1f - %.1f)" % (d["median"], d["min"], d["max"])
    many = [c for c in res["cells"] if c["members"] >= 8]
    few = [c for c in res["cells"] if c["members"] < 8]
    lost = [c for c in many if not c["one_call_ms"]["median"] < c["loop_ms"]["min"]]
    ratios = [c["loop_min_over_call_median"] for c in many]
    with open(a.md, "w") as f:
        f.write("# Ragged appends to many contexts (`lnb_forward_append_many`): measurements\n\n")
        f.write("<!-- Advice this table supports.  lnb_forward_append_many: every call that extends SEVERAL contexts by a few rows each -- from 8 members on the one call's median is "
                "%s the per-member loop's fastest repeat in %d of %d cells (%.1f to %.1f times).  lnb_forward_append: ONE context (nothing to share a pass with), and few members "
                "with 100+ rows each, where its matrix-core attention reads K and V once per 16 query rows instead of once per row (%s): %s. -->\n\n"
                % ("below" if not lost else "NOT always below", len(many) - len(lost), len(many), min(ratios or [0]), max(ratios or [0]),
                   "the loop is faster in %d of the %d such cells measured" % (sum(c["loop_ms"]["median"] < c["one_call_ms"]["median"] for c in few), len(few)),
                   "; ".join("%d members x %d rows at prefix %d: one call %.1f ms, loop %.1f ms" % (c["members"], c["rows"], c["prefix"], c["one_call_ms"]["median"], c["loop_ms"]["median"]) for c in few) or "not measured"))
        f.write("`python tools/append_many_bench.py --layers %d --members %s --rows %s --prefixes %s --extra %s --logits-cells %s --reps %d --md profiles/append_many.md`, 8B synthetic shape, matrix-core "
                "copy enabled, one process, MI355X.  A source is prefilled to the prefix and forked into 128 contexts; every member then takes `rows` tokens of its own at the prefix.  Wall "
                "time around the call in ms, median (fastest - slowest) of %d repeats after one warm-up; argmax only unless said otherwise.  The batched step is `lnb_batch_decode`'s own event "
                "time per step for as many members as the widest pass has columns, at the same positions: the kernels a pass runs, replayed from a captured graph and launched eagerly "
                "(`LNB_NO_GRAPH=1`).\n\n" % (a.layers, a.members, a.rows, a.prefixes, a.extra, a.logits_cells, a.reps, a.reps))
        f.write("| prefix | members | rows | total rows | passes (widest) | one call ms | per-member loop ms | loop fastest / call median | call per pass ms | batched step, graph ms | batched step, eager ms |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for c in res["cells"]:
            f.write("| %d | %d | %d | %d | %d (%d) | %s | %s | %.1f | %.1f | %s | %s |\n" % (c["prefix"], c["members"], c["rows"], c["total_rows"], c["passes"], c["max_columns"], mmr(c["one_call_ms"]),
                    mmr(c["loop_ms"]), c["loop_min_over_call_median"], c["per_pass_ms"], mmr(c["batch_step_graph_ms"]), mmr(c["batch_step_eager_ms"])))
        withl = [c for c in res["cells"] if "one_call_logits_ms" in c]
        if withl:
            f.write("\n## With the logits\n\nEvery pass then copies `[width, %d]` bf16 to pinned host memory, and the host widens the rows of pass p - 1 to f32 while pass p runs.\n\n"
                    "| prefix | members | rows | argmax only ms | with logits ms |\n|---|---|---|---|---|\n" % V)
            for c in withl:
                f.write("| %d | %d | %d | %s | %s |\n" % (c["prefix"], c["members"], c["rows"], mmr(c["one_call_ms"]), mmr(c["one_call_logits_ms"])))
        f.write("\n## What the table says\n\n")
        if lost:
            f.write("* **The acceptance condition fails** in: %s.\n" % ", ".join("%d x %d at %d" % (c["members"], c["rows"], c["prefix"]) for c in lost))
        else:
            by_rows = {}
            for c in many:
                by_rows.setdefault(c["rows"], []).append(c["loop_min_over_call_median"])
            f.write("* **From 8 members on the one call is faster in every cell**: its median is below the loop's fastest repeat everywhere, by %.1f to %.1f times (%s).  The derivation's "
                    "\"about 10x and more\" holds where the loop walks the weights once per ROW (fewer than 16 rows per member); from 16 rows on the loop runs the matrix-core append, "
                    "one pass over the weights per MEMBER, and the gain is the ratio of members to passes less what a 16-row pass costs.\n"
                    % (min(ratios), max(ratios), "; ".join("%d rows per member: %.1f - %.1f" % (r, min(v), max(v)) for r, v in sorted(by_rows.items()))))
        over = [(c, c["per_pass_ms"] - c["batch_step_graph_ms"]["median"], c["batch_step_eager_ms"]["median"] - c["batch_step_graph_ms"]["median"]) for c in res["cells"]]
        worst = max(o[1] for o in over)
        f.write("* **A pass against the batched step.**  The call's time per pass is %+.1f to %+.1f ms of the graph-replayed step of the same width, and the same step launched eagerly is "
                "%+.1f to %+.1f ms of the replayed one: at these widths a step is long enough for the host to stay ahead of the device, so eager launches cost nothing, and %s"
                "The setup launch (1 + n_layers small workgroups), the table upload and the members' stream synchronisation (once per call) and the zeroing of the activation buffers "
                "(only when a pass is narrower than the one before) do not show at this resolution.\n"
                % (min(o[1] for o in over), worst, min(o[2] for o in over), max(o[2] for o in over),
                   "a pass costs no more than the step -- it ends with the argmax of the members' last rows alone, the step with every column's argmax and token feedback.  " if worst <= 0.05 else
                   "what a pass costs beyond the step is the call's own work.  "))
        if few:
            f.write("* **Few members with many rows** (the per-member loop is faster in %d of %d such cells): %s.  A column of a pass is a one-token step whose attention reads its member's K and V rows for "
                    "itself; the per-member matrix-core append shares them among 16 query rows.\n"
                    % (sum(c["loop_ms"]["median"] < c["one_call_ms"]["median"] for c in few), len(few),
                       "; ".join("%d x %d at prefix %d: one call %.1f ms, loop %.1f ms" % (c["members"], c["rows"], c["prefix"], c["one_call_ms"]["median"], c["loop_ms"]["median"]) for c in few)))
        f.write("\nTotal run time of the measurement %.0f s.\n" % res["seconds"])
