#!/usr/bin/env python3
"""Causal multi-row append (lnb_forward_append) of the 8B synthetic shape against the only other way to extend a live context: one-token
lnb_forward calls.  For S rows at prefix P (P cached positions in front of them), last-row argmax only, wall clock around the call:
  append    one lnb_forward_append of S rows at start position P
  one_token the same S rows as S lnb_forward calls of one row at P, P + 1, ...
  forward0  lnb_forward of S rows at position 0 on a second context (what the S rows cost without the P positions of attention in front)
One warm-up call per cell (the score-index scratch is grown there), then the median of --reps timed calls.
    python tools/append_bench.py [--sizes 16,64,128,512] [--prefixes 0,128,1024,4096] [--reps 5] [--out x.json] [--md x.md]

    python tools/append_bench.py --rows-long [--layers 32] [--reps 5] [--package DIR] [--out x.json]
short appends to a LONG context (capacity 16640): 2 / 4 / 8 / 15 rows at prefixes 8192 and 16384, beyond what the row-per-workgroup attention stages in the
LDS -- the calls that run the multi-row long-context attention (attention form 4; LNB_ATTN_ROWS_RPW picks the rows per PV workgroup, read once per process:
one run per value).  --package DIR: time another build of the package (a checkout of an earlier commit, whose fallback there is the one-token loop inside
the call).  The prefix is a real one (512-row appends); one warm-up call per cell, then --reps timed calls: median, min..max."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_pre = argparse.ArgumentParser(add_help=False)               # --package steers the import below: parsed first, by the same rules as the rest
_pre.add_argument("--package", default="")
_pkg = _pre.parse_known_args()[0].package
PACKAGE = os.path.abspath(_pkg) if _pkg else os.path.join(ROOT, "llama-nuts-and-bolts_amd")
sys.path.insert(0, ROOT); sys.path.insert(0, PACKAGE)
import lnb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="16,64,128,512")
ap.add_argument("--prefixes", default="0,128,1024,4096")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-reps", type=int, default=3, help="timed repeats of the one-token loop (S calls each)")
ap.add_argument("--layers", type=int, default=32, help="blocks of the model (fewer: a cheap run under the profiler -- the launches per block are the same)")
ap.add_argument("--only", default="append,one_token,forward0", help="which legs to run (a profiler run wants one)")
ap.add_argument("--out", default="")
ap.add_argument("--md", default="")
ap.add_argument("--rows-long", action="store_true", help="the short-append-to-a-long-context table (see above) instead of the default one")
ap.add_argument("--package", default="", help="directory of the lnb package to measure (default: this checkout's)")
a = ap.parse_args()
assert os.path.dirname(os.path.abspath(lnb.__file__)) == PACKAGE and (not a.package or os.path.abspath(a.package) == PACKAGE), "--package did not steer the import"


def rows_long():
    SL, rows, prefixes = 16640, (2, 4, 8, 15), (8192, 16384)
    m = lnb.LlamaTransformer(device=0, **dict(lnb.LLAMA_8B, n_layers=a.layers)).fill_synthetic(1234).finalize(rope_rows=SL + 64)
    c = lnb.InferenceContext(m, SL)
    toks = lnb.synth_tokens(99, SL, 128256)
    sync = lambda: lnb._chk(lnb.lib().lnb_ctx_synchronize(c.h))
    filled = max(prefixes) + max(rows)
    for p0 in range(0, filled, 512):                         # the cached text: 512-row appends up to the last position a timed call touches
        c.ForwardAppend(toks[p0:min(p0 + 512, filled)], p0, want_logits=False)
    res = []
    for P in prefixes:
        for S in rows:
            call = lambda: c.ForwardAppend(toks[P:P + S], P, want_logits=False)[1]
            first = call()                                   # warm-up (the scratch is allocated here)
            ts = []
            for _ in range(a.reps):
                sync()
                t0 = time.perf_counter()
                tok = call()
                ts.append((time.perf_counter() - t0) * 1e3)
            row = {"rows": S, "prefix": P, "layers": a.layers, "ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                   "next_token": int(tok), "stable": tok == first, "rpw": os.environ.get("LNB_ATTN_ROWS_RPW", "default"), "package": PACKAGE,
                   "attention_form": c.append_attention_form() if hasattr(c, "append_attention_form") else None}
            print(json.dumps(row), flush=True)
            res.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    c.close(); m.close()


if a.rows_long:
    rows_long()
    sys.exit(0)
sizes = [int(s) for s in a.sizes.split(",")]
prefixes = [int(s) for s in a.prefixes.split(",")]
legs = a.only.split(",")
SL = max(prefixes) + max(sizes) + 8
m = lnb.LlamaTransformer(device=0, **dict(lnb.LLAMA_8B, n_layers=a.layers)).fill_synthetic(1234).finalize(rope_rows=SL + 64)
c = lnb.InferenceContext(m, SL)
c0 = lnb.InferenceContext(m, max(sizes) + 8)
toks = lnb.synth_tokens(99, SL, 128256)
sync = lambda ctx: lnb._chk(lnb.lib().lnb_ctx_synchronize(ctx.h))


def timed(fn, reps):
    fn()                                                     # warm-up
    ts = []
    for _ in range(reps):
        sync(c); sync(c0)
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


if max(prefixes) > 0:                                        # the cached text in front of every append: one exact prefill
    c.Forward(toks[:max(prefixes)], 0, want_logits=False)
res = []
for P in prefixes:
    for S in sizes:
        row = {"rows": S, "prefix": P, "layers": a.layers}
        tok = {}

        def f_append():
            tok["append"] = c.ForwardAppend(toks[P:P + S], P, want_logits=False)[1]

        def f_loop():
            for i in range(S):
                tok["one_token"] = c.Forward(toks[P + i:P + i + 1], P + i, want_logits=False)[1]

        def f_fwd0():
            tok["forward0"] = c0.Forward(toks[P:P + S], 0, want_logits=False)[1]

        if "append" in legs:
            row["append_ms"], row["append_min_ms"], row["append_max_ms"] = (round(x, 3) for x in timed(f_append, a.reps))
            row["attention_form"] = c.prefill_attention_form()
        if "one_token" in legs:
            row["one_token_ms"], row["one_token_min_ms"], row["one_token_max_ms"] = (round(x, 3) for x in timed(f_loop, a.loop_reps))
        if "forward0" in legs:
            row["forward0_ms"], _, _ = (round(x, 3) for x in timed(f_fwd0, a.reps))
        if "append" in legs and "one_token" in legs:
            row["same_next_token"] = tok["append"] == tok["one_token"]
            row["speedup_vs_one_token"] = round(row["one_token_ms"] / row["append_ms"], 2)
        print(json.dumps(row), flush=True)
        res.append(row)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
if a.md:
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as f:
        f.write("| rows S | prefix P | append ms (min..max) | S one-token calls ms | speed-up | lnb_forward S rows at 0, ms | append - forward0, ms |\n|---|---|---|---|---|---|---|\n")
        for r in res:
            if "append_ms" in r and "one_token_ms" in r and "forward0_ms" in r:
                f.write("| %d | %d | %.2f (%.2f..%.2f) | %.2f | %.2fx | %.2f | %.2f |\n" % (
                    r["rows"], r["prefix"], r["append_ms"], r["append_min_ms"], r["append_max_ms"], r["one_token_ms"], r["speedup_vs_one_token"],
                    r["forward0_ms"], r["append_ms"] - r["forward0_ms"]))
c.close(); c0.close(); m.close()
