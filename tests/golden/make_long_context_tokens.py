#!/usr/bin/env python3
"""Generates tests/golden/long_context_tiny_tokens.json: the CPU ORACLE's greedy continuation of a 23540-token prompt on a one-layer tiny model, so
that a device run on a long context (lnb_ctx_create_long) is pinned to the oracle ACROSS position 23552 -- the capacity at which lnb_ctx_create
stops and a 512-position batch edge of the long-context PV kernel (tests/test_gpu_long_context.py reads the file and never runs the oracle).

Stored: the token the prompt's Forward predicts, the 24 greedy tokens behind it, SHA-256 of the K and V rows [23540, 23564) those 24 steps
append, and the hashes of the first four steps' logits rows (raw f32 bits, as tests/golden/make_logits_hashes.py makes its own).

    python tests/golden/make_long_context_tokens.py [out_dir]          # ~2.5 minutes with 8 threads
"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as orc  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))
SEED_W, SEED_P, P, N, N_LOGITS = 777, 4000, 23540, 24, 4
CFG = dict(orc.TINY, n_heads=2, n_kv_heads=1, n_layers=1, max_seq_len=12288)       # head_dim 128; RoPE table of 24576 rows


def row_hash(row):
    return hashlib.sha256(np.ascontiguousarray(row, dtype=np.float32).view(np.uint32).astype("<u4").tobytes()).hexdigest()


def rows_hash(rows):
    return hashlib.sha256(np.ascontiguousarray(rows, dtype=np.uint16).astype("<u2").tobytes()).hexdigest()


t0 = time.time()
om = orc.Model(**CFG).fill_synthetic(SEED_W).finalize()
prompt = orc.synth_tokens(SEED_P, P, CFG["vocab_size"])
oc = orc.Context(om, P + N + 2)
_, first = oc.forward(prompt, 0, want_logits=False)
toks, steps = [int(first)], []
for k in range(N):
    lg, nxt = oc.forward(np.array([toks[-1]], dtype=np.int32), P + k)
    if k < N_LOGITS:
        steps.append({"input_token": toks[-1], "position": P + k, "logits_sha256": row_hash(lg[0]), "argmax": int(nxt)})
    toks.append(int(nxt))
out = {"what": "the oracle's greedy continuation of a %d-token prompt on dict(TINY, n_heads=2, n_kv_heads=1, n_layers=1, max_seq_len=12288), synthetic weights "
               "seed %d, prompt synth_tokens(%d, %d, vocab): first_token is the prompt's argmax, tokens the %d greedy tokens behind it; SHA-256 of the "
               "bf16 K / V rows [%d, %d) of layer 0 ([position][kv head][d], little-endian) and of the raw f32 bits of the first %d steps' logits rows"
               % (P, SEED_W, SEED_P, P, N, P, P + N, N_LOGITS),
       "generator": "tests/golden/make_long_context_tokens.py",
       "model": {k: CFG[k] for k in ("dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size", "multiple_of", "max_seq_len")},
       "prompt_len": P, "weights_seed": SEED_W, "prompt_seed": SEED_P,
       "prompt_head": [int(t) for t in prompt[:8]], "prompt_tail": [int(t) for t in prompt[-8:]],
       "first_token": toks[0], "tokens": toks[1:],
       "k_rows_sha256": rows_hash(oc.cache(0, 0)[P:P + N]), "v_rows_sha256": rows_hash(oc.cache(0, 1)[P:P + N]),
       "steps": steps, "oracle_seconds": round(time.time() - t0, 1), "oracle_threads": oc.nthreads}
os.makedirs(OUT, exist_ok=True)
json.dump(out, open(os.path.join(OUT, "long_context_tiny_tokens.json"), "w"), indent=1)
print("wrote %d tokens + %d logits hashes in %.0f s; tokens %s" % (N, N_LOGITS, time.time() - t0, toks))
