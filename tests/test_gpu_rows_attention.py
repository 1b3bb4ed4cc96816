"""Multi-row long-context attention (-m gpu): attn_rows_scores_kernel + attn_rows_pv_kernel behind lnb_forward_append, lnb_forward_score_append and,
opt-in, the verify passes of lnb_decode_speculative_until (lnb_ctx_set_rows_attention).  Every comparison is bit-exact: logits, the KV rows the call
wrote, the rows below start_pos, the last-row argmax.  References: the CPU oracle's one-token steps at start 0, the GPU's own one-token Forward
(pinned to the oracle by the rest of the suite) elsewhere.  set_rows_attention(0, ...) sends every 2..15-row call to the pair, so the start
positions can straddle the kernels' boundaries at a few hundred positions: 254 -> the 256-position scores block (and the 256-position PV batch of
RPW 2 / 4), 510 -> the 512-position PV batch of RPW 1, 1022 -> 1024, where the one-token step switches from its eager to its lazy PV body, 0 -> T = 1.
Seeds: model 909, tokens 5150; no row of these runs fails certification (zseq_count stays put unless flags bit 0 asks for the serial sums)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {
    128: dict(orc.TINY, n_heads=2, n_kv_heads=1),
    64: dict(orc.TINY),
    32: dict(orc.TINY, n_heads=8, n_kv_heads=2),
}
SL, P = 1100, 1040                                           # capacity, prefilled prefix
STARTS = (0, 254, 510, 1022)
COUNTS = (2, 3, 8, 15)
WIDE = (500, 40)                                             # head_dim 32: a 40-row call = three groups of the launcher (16 + 16 + 8), across 512
SEED_M, SEED_T = 909, 5150


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_REF = {}


def reference(lnb, hd):
    """per head_dim, once: the model, the tokens, a context that ran one-token steps at every position the tests append to (its caches hold the
    reference rows) and those steps' logits / argmax; position 0 .. 14 from the CPU oracle"""
    if hd in _REF:
        return _REF[hd]
    cfg = CFGS[hd]
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(SEED_M).finalize()
    toks = lnb.synth_tokens(SEED_T, SL, cfg["vocab_size"])
    rc = lnb.InferenceContext(gm, SL)
    rc.Forward(toks[:P], 0, want_logits=False)
    base = [(rc.CacheK(l).copy(), rc.CacheV(l).copy()) for l in range(cfg["n_layers"])]
    logits, arg = {}, {}
    spans = [(s, max(COUNTS)) for s in STARTS if s] + ([WIDE] if hd == 32 else [])
    for s, n in spans:
        for i in range(n):
            if s + i not in logits:
                lg, a = rc.Forward(toks[s + i:s + i + 1], s + i)
                logits[s + i] = lg[0].copy(); arg[s + i] = a
    om = orc.Model(**cfg).fill_synthetic(SEED_M).finalize()
    oc = orc.Context(om, 32)
    okv = None
    for i in range(max(COUNTS)):
        lg, a = oc.forward(toks[i:i + 1], i)
        logits[("o", i)] = lg[0].copy(); arg[("o", i)] = a
    okv = [(oc.cache(l, 0).copy(), oc.cache(l, 1).copy()) for l in range(cfg["n_layers"])]
    oc.close(); om.close()
    kv = [(rc.CacheK(l).copy(), rc.CacheV(l).copy()) for l in range(cfg["n_layers"])]
    rc.close()
    _REF[hd] = dict(cfg=cfg, gm=gm, toks=toks, base=base, kv=kv, logits=logits, arg=arg, okv=okv)
    return _REF[hd]


def check_append(ctx, R, start, seq, tag, form=4):
    cfg, toks = R["cfg"], R["toks"]
    lg, a = ctx.ForwardAppend(toks[start:start + seq], start)
    assert ctx.append_attention_form() == form, tag
    key = (lambda i: ("o", i)) if start == 0 else (lambda i: start + i)
    ref = np.stack([R["logits"][key(i)] for i in range(seq)])
    assert np.array_equal(bits(lg), bits(ref)), tag
    assert a == R["arg"][key(seq - 1)], tag
    for l in range(cfg["n_layers"]):
        k, v = ctx.CacheK(l), ctx.CacheV(l)
        if start == 0:
            assert np.array_equal(k[:seq], R["okv"][l][0][:seq]) and np.array_equal(v[:seq], R["okv"][l][1][:seq]), tag + (l, "new rows")
        else:
            assert np.array_equal(k[:start], R["base"][l][0][:start]) and np.array_equal(v[:start], R["base"][l][1][:start]), tag + (l, "rows below start_pos were written")
            assert np.array_equal(k[start:start + seq], R["kv"][l][0][start:start + seq]), tag + (l, "K")
            assert np.array_equal(v[start:start + seq], R["kv"][l][1][start:start + seq]), tag + (l, "V")


def prefilled(lnb, R):
    c = lnb.InferenceContext(R["gm"], SL)
    c.Forward(R["toks"][:P], 0, want_logits=False)
    return c


@pytest.mark.parametrize("hd", sorted(CFGS))
def test_rows_equal_one_token_steps_across_every_boundary(lnb, hd):
    R = reference(lnb, hd)
    c = prefilled(lnb, R).set_rows_attention(0, 0)
    assert c.append_attention_form() == 0
    z0 = c.zseq_count()
    for start in STARTS[1:]:
        for seq in COUNTS:
            check_append(c, R, start, seq, (hd, start, seq))
    if hd == 32:
        check_append(c, R, WIDE[0], WIDE[1], (hd,) + WIDE)
    assert c.zseq_count() == z0                               # every row certified
    c.close()
    f = lnb.InferenceContext(R["gm"], 32).set_rows_attention(0, 0)      # T_0 = 1 on an empty context
    for seq in COUNTS:
        check_append(f, R, 0, seq, (hd, 0, seq))
    f.close()


def test_serial_sums_give_the_same_bits_and_are_counted(lnb):
    R = reference(lnb, 128)
    cfg = R["cfg"]
    c = prefilled(lnb, R).set_rows_attention(0, 1)
    z0 = c.zseq_count()
    check_append(c, R, 254, 15, ("zseq", 254, 15))
    check_append(c, R, 1022, 3, ("zseq", 1022, 3))
    assert c.zseq_count() == z0 + (15 + 3) * cfg["n_heads"] * cfg["n_layers"]      # once per (row, head) and layer
    c.set_rows_attention(-1, 0)                               # the threshold stays, the serial sums go
    z1 = c.zseq_count()
    check_append(c, R, 510, 8, ("certified again", 510, 8))
    assert c.zseq_count() == z1
    c.close()


def test_default_threshold_keeps_the_row_per_workgroup_kernel(lnb):
    R = reference(lnb, 64)
    c = prefilled(lnb, R)
    check_append(c, R, 254, 8, ("default", 254, 8), form=1)
    check_append(c, R, 1022, 15, ("default", 1022, 15), form=1)
    c.set_rows_attention(600, 0)                              # only calls that end beyond 600 positions
    check_append(c, R, 254, 3, ("600", 254, 3), form=1)
    check_append(c, R, 1022, 3, ("600", 1022, 3), form=4)
    lg, _ = c.ForwardAppend(R["toks"][510:511], 510)          # a one-row call is the one-token step
    assert c.append_attention_form() == 0 and np.array_equal(bits(lg[0]), bits(R["logits"][510]))
    c.close()


def test_score_append_of_eight_rows_equals_eight_one_row_scores(lnb):
    R = reference(lnb, 64)
    toks = R["toks"]
    c, d = prefilled(lnb, R).set_rows_attention(0, 0), prefilled(lnb, R)
    start, n = 254, 8
    tl, tp, lz, am = c.score_append(toks[start:start + n], start, toks[start + 1:start + n + 1])
    assert c.append_attention_form() == 4
    for i in range(n):
        l1, p1, z1, a1 = d.score(toks[start + i:start + i + 1], start + i, toks[start + i + 1:start + i + 2])
        assert bits(tl[i:i + 1]) == bits(l1) and bits(tp[i:i + 1]) == bits(p1), i
        assert np.float64(lz[i]).view(np.uint64) == np.float64(z1[0]).view(np.uint64), i
    assert am == a1
    c.close(); d.close()


def test_8b_head_geometry_beyond_the_row_kernel_runs_the_pair_by_default(lnb):
    """32 query heads on 8 KV heads, head_dim 128, two layers, capacity 8400, prefix 8000: an 8-row call there used to run as one-token steps
    inside the entry point (form 3); by default it is now one multi-row call on the pair"""
    cfg = dict(orc.TINY, dim=4096, n_heads=32, n_kv_heads=8, multiple_of=1024, max_seq_len=4224)
    S, start, n = 8400, 8000, 8
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(77).finalize()
    toks = lnb.synth_tokens(31, S, cfg["vocab_size"])
    c = lnb.InferenceContext(gm, S)
    c.Forward(toks[:start], 0, want_logits=False)
    ref = np.empty((n, cfg["vocab_size"]), dtype=np.float32)
    for i in range(n):
        lg, a1 = c.Forward(toks[start + i:start + i + 1], start + i)
        ref[i] = lg[0]
    kv = [(c.CacheK(l).copy(), c.CacheV(l).copy()) for l in range(cfg["n_layers"])]
    z0 = c.zseq_count()
    lg, a = c.ForwardAppend(toks[start:start + n], start)
    assert c.append_attention_form() == 4
    assert np.array_equal(bits(lg), bits(ref)) and a == a1
    assert c.zseq_count() == z0
    for l in range(cfg["n_layers"]):
        assert np.array_equal(c.CacheK(l), kv[l][0]) and np.array_equal(c.CacheV(l), kv[l][1]), l
    c.close(); gm.close()


CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(pkg)r]
import numpy as np
import lnb
from oracle import oracle as orc
cfg = dict(orc.TINY, n_heads=2, n_kv_heads=1)
gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(909).finalize()
toks = lnb.synth_tokens(5150, 1100, cfg["vocab_size"])
a, b = lnb.InferenceContext(gm, 1100).set_rows_attention(0, 0), lnb.InferenceContext(gm, 1100)
for c in (a, b):
    c.Forward(toks[:1040], 0, want_logits=False)
z0 = a.zseq_count()
for start in (254, 510, 1022):
    ref = [b.Forward(toks[start + i:start + i + 1], start + i) for i in range(15)]
    for seq in (3, 15):
        lg, am = a.ForwardAppend(toks[start:start + seq], start)
        assert a.append_attention_form() == 4
        want = np.stack([r[0][0] for r in ref[:seq]])
        assert np.array_equal(lg.view(np.uint32), want.view(np.uint32)) and am == ref[seq - 1][1], (start, seq)
        for l in range(cfg["n_layers"]):
            assert np.array_equal(a.CacheK(l)[:start + seq], b.CacheK(l)[:start + seq]) and np.array_equal(a.CacheV(l)[:start + seq], b.CacheV(l)[:start + seq]), (start, seq, l)
assert a.zseq_count() == z0
print("rows child ok rpw=%(rpw)d")
"""


@pytest.mark.parametrize("rpw", [1, 2, 4])
def test_every_rows_per_workgroup_form_in_a_fresh_process(lnb, rpw):
    """LNB_ATTN_ROWS_RPW is read once per process: each form in a child of its own; 3 and 15 rows are no multiples of 2 or 4"""
    code = CHILD % dict(root=ROOT, pkg=os.path.join(ROOT, "llama-nuts-and-bolts_amd"), rpw=rpw)
    env = dict(os.environ, LNB_ATTN_ROWS_RPW=str(rpw))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "rows child ok rpw=%d" % rpw in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("copy", [True, False], ids=["columns", "rows"])
def test_speculative_verify_passes_on_the_pair_equal_greedy(lnb, copy):
    cfg = CFGS[128]
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(SEED_M).finalize()
    if copy:
        gm.enable_batch()
    plen, steps = 250, 40                                     # crosses position 256
    prompt = lnb.synth_tokens(SEED_T + 1, plen, cfg["vocab_size"])
    g = lnb.InferenceContext(gm, 300)
    first = g.Forward(prompt, 0, want_logits=False)[1]
    ref = [int(t) for t in g.decode_greedy(first, plen, steps)[0]]      # the context's own greedy continuation = the corpus
    gkv = [(g.CacheK(l).copy(), g.CacheV(l).copy()) for l in range(cfg["n_layers"])]
    g.close()
    c = lnb.InferenceContext(gm, 300).set_batched_attention(0, 0).set_rows_attention(-1, 2)
    assert c.Forward(prompt, 0, want_logits=False)[1] == first
    c.set_draft(7, 1, 4, [first] + ref)
    got, fin, st, _ = c.decode_speculative_until(prompt, first, plen, steps)
    assert [int(t) for t in got] == ref and not fin
    assert st["verify_passes"] > 0 and st["accepted"] > 0 and c.verify_attention_form() == 2
    for l in range(cfg["n_layers"]):
        assert np.array_equal(c.CacheK(l)[:plen + steps], gkv[l][0][:plen + steps]) and np.array_equal(c.CacheV(l)[:plen + steps], gkv[l][1][:plen + steps]), l
    # the serial sums inside a verify pass, then the long pair again with bit 1 clear
    for flags, form in ((3, 2), (0, 1)):
        c.set_rows_attention(-1, flags)
        z0 = c.zseq_count()
        got, _, st, _ = c.decode_speculative_until(prompt, first, plen, steps)
        assert [int(t) for t in got] == ref and c.verify_attention_form() == form, flags
        assert (c.zseq_count() > z0) == bool(flags & 1), flags
    c.close(); gm.close()


def test_argument_errors_come_before_the_handle(lnb):
    import ctypes as C
    L = lnb.lib()
    assert L.lnb_ctx_set_rows_attention(None, -1, 4) != 0 and b"flags" in L.lnb_last_error()
    assert L.lnb_ctx_set_rows_attention(None, -1, -1) != 0 and b"flags" in L.lnb_last_error()
    assert L.lnb_ctx_set_rows_attention(None, -1, 0) != 0 and b"null" in L.lnb_last_error()
    n = C.c_int(7)
    assert L.lnb_ctx_append_attention_form(None, C.byref(n)) != 0 and b"null" in L.lnb_last_error()
    R = reference(lnb, 64)
    c = lnb.InferenceContext(R["gm"], 32)
    assert L.lnb_ctx_append_attention_form(c.h, None) != 0 and b"null" in L.lnb_last_error()
    with pytest.raises(lnb.LnbError, match="flags"):
        c.set_rows_attention(0, 8)
    assert c.append_attention_form() == 0
    c.close()
