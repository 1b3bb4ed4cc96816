#!/usr/bin/env python3
"""Long contexts (lnb_ctx_create_long) of the 8B synthetic shape, one process:
  (a) decode at T = 4100 / 16 K / 32 K / 64 K / 128 K on a 131072-position context with 4096-row buffers: attention us per layer (lnb_profile_kernel, class 1),
      tokens/s of a 64-step captured greedy run, serial walks per token (lnb_ctx_zseq_count) -- beside the derived floors: 6 cycles per position of PV chain,
      K + V bytes of a layer over 6.7 TB/s;
  (b) the cost of capacity: the same steps at T = 4100 on a lnb_ctx_create(8192) context (per-position PV layout, 33-block scores grid per head) against the
      131072-position one (constant layout, 512-block grid);
  (d) lnb_forward_append of 4096 rows at prefixes 32 K / 64 K / 124 K: ms per call (one call each, no warm-up: seconds per call).
The caches are NOT prefilled (a 128 K exact prefill of the 8B shape takes minutes): the steps read zero K / V rows in front of their own, which costs the
same time but makes every score equal, so the walk counts of this tool say nothing about real text; tests/test_gpu_long_context.py prints them for real rows.
(c), the default path's headline, is bench.py's own line.  A cell that would start after --budget-s seconds of run time is skipped and reported as such.
    python tools/long_context_bench.py [--layers 32] [--steps 64] [--budget-s 400] [--md profiles/long_context.md] [--out x.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "llama-nuts-and-bolts_amd"))
import lnb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--positions", default="4100,16384,32768,65536,131000")
ap.add_argument("--append-prefixes", default="32768,65536,126976")
ap.add_argument("--append-rows", type=int, default=4096)
ap.add_argument("--budget-s", type=float, default=400.0)
ap.add_argument("--clock-mhz", type=float, default=2400.0, help="shader clock the derived chain floor is stated at")
ap.add_argument("--out", default="")
ap.add_argument("--md", default="")
a = ap.parse_args()
T0 = time.time()
CAP, ROWS = lnb.MAX_SEQ_LEN, 4096
cfg = dict(lnb.LLAMA_8B, n_layers=a.layers)
m = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize(rope_rows=CAP)
hd, kvh = cfg["dim"] // cfg["n_heads"], cfg["n_kv_heads"]
res = {"shape": {k: cfg[k] for k in ("dim", "n_layers", "n_heads", "n_kv_heads")}, "capacity": CAP, "max_rows": ROWS, "decode": [], "capacity_cost": {}, "append": [], "skipped": []}
over = lambda what: (time.time() - T0 > a.budget_s) and (res["skipped"].append(what) or True)


def decode_cell(ctx, T, steps):
    att_us = ctx.profile_kernel(1, T - 1, 20) * 1e3          # one-token attention at context T (position T - 1), per layer
    z0 = ctx.zseq_count()
    _, ms = ctx.decode_greedy(7, T - 1, steps)               # captured graph; device time of the whole run
    walks = ctx.zseq_count() - z0
    return {"T": T, "attention_us_per_layer": round(att_us, 2), "ms_per_token": round(ms / steps, 4), "tokens_per_s": round(1e3 * steps / ms, 2),
            "walks_per_token": round(walks / steps, 3),
            "derived_pv_chain_us": round(6.0 * T / a.clock_mhz, 1), "derived_kv_stream_us": round(2.0 * T * kvh * hd * 2 / 6.7e12 * 1e6, 1)}


long_ctx = lnb.InferenceContext(m, CAP, max_rows=ROWS)
for T in [int(s) for s in a.positions.split(",")]:
    if over("decode T=%d" % T):
        continue
    steps = min(a.steps, CAP - T + 1)
    row = decode_cell(long_ctx, T, steps)
    print(json.dumps(row), flush=True)
    res["decode"].append(row)
if not over("capacity cost"):
    short_ctx = lnb.InferenceContext(m, 8192)
    s_row, l_row = decode_cell(short_ctx, 4100, a.steps), decode_cell(long_ctx, 4100, a.steps)
    short_ctx.close()
    res["capacity_cost"] = {"lnb_ctx_create_8192": s_row, "lnb_ctx_create_long_131072": l_row,
                            "attention_us_difference": round(l_row["attention_us_per_layer"] - s_row["attention_us_per_layer"], 2),
                            "ms_per_token_difference": round(l_row["ms_per_token"] - s_row["ms_per_token"], 4)}
    print(json.dumps(res["capacity_cost"]), flush=True)
toks = lnb.synth_tokens(99, a.append_rows, cfg["vocab_size"])
for P in [int(s) for s in a.append_prefixes.split(",")]:
    if over("append prefix=%d" % P):
        continue
    lnb._chk(lnb.lib().lnb_ctx_synchronize(long_ctx.h))
    t0 = time.perf_counter()
    long_ctx.ForwardAppend(toks, P, want_logits=False)
    row = {"rows": a.append_rows, "prefix": P, "ms": round((time.perf_counter() - t0) * 1e3, 1), "attention_form": long_ctx.prefill_attention_form()}
    print(json.dumps(row), flush=True)
    res["append"].append(row)
long_ctx.close(); m.close()
res["seconds"] = round(time.time() - T0, 1)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
if a.md:
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as f:
        f.write("# Long contexts (`lnb_ctx_create_long`): measurements\n\n`tools/long_context_bench.py`, 8B synthetic shape, %d layers, one process, MI355X.  The caches in front of the measured "
                "positions are zero rows (no 128 K prefill), so the walk counts below are not those of real text.\n\n" % a.layers)
        f.write("## (a) Decode on a 131072-position context (`max_rows` 4096)\n\n| T | attention us / layer | ms / token | tokens/s | walks / token | derived: PV chain us (6 cycles / position at %.0f MHz) | derived: K + V of a layer over 6.7 TB/s, us |\n|---|---|---|---|---|---|---|\n" % a.clock_mhz)
        for r in res["decode"]:
            f.write("| %d | %.2f | %.4f | %.2f | %.3f | %.1f | %.1f |\n" % (r["T"], r["attention_us_per_layer"], r["ms_per_token"], r["tokens_per_s"], r["walks_per_token"], r["derived_pv_chain_us"], r["derived_kv_stream_us"]))
        f.write("\n## (b) The cost of capacity at T = 4100\n\n")
        if res["capacity_cost"]:
            cc = res["capacity_cost"]
            f.write("| context | attention us / layer | ms / token | tokens/s |\n|---|---|---|---|\n")
            for k in ("lnb_ctx_create_8192", "lnb_ctx_create_long_131072"):
                f.write("| `%s` | %.2f | %.4f | %.2f |\n" % (k, cc[k]["attention_us_per_layer"], cc[k]["ms_per_token"], cc[k]["tokens_per_s"]))
            f.write("\nDifference: %.2f us of attention per layer, %.4f ms per token.\n" % (cc["attention_us_difference"], cc["ms_per_token_difference"]))
        else:
            f.write("Not measured in this run.\n")
        f.write("\n## (d) `lnb_forward_append` of %d rows on the same context\n\n| prefix | ms per call | attention form |\n|---|---|---|\n" % a.append_rows)
        for r in res["append"]:
            f.write("| %d | %.1f | %d |\n" % (r["prefix"], r["ms"], r["attention_form"]))
        if res["skipped"]:
            f.write("\nSkipped (run-time budget of %.0f s reached): %s.\n" % (a.budget_s, ", ".join(res["skipped"])))
