"""Prefix sharing (-m gpu): lnb_ctx_fork (kv_fork_kernel, and the copy engine under LNB_FORK_COPY=1) and lnb_ctx_save_prefix / lnb_ctx_load_prefix.
Every comparison is bit-exact.  Tiny models: oracle.TINY (head_dim 64) and its head-geometry variants of tests/test_gpu_rows_attention.py (head_dim 128
with one KV head, head_dim 32 with two of eight heads); model seed 909, token seed 5150.  The source has capacity 96 and holds 41 rows, 37 of them are
shared; the destinations have capacities 41, 64, 96 and 300 (below, between, equal to and above the source's: K's runs are re-strided every time) and
hold 41 rows of another text each, so a row that should have stayed is not zero.
A destination of capacity 41 cannot take the 5-row append at 37 (42 positions): it appends 4 rows, compared with the first 4 of the reference, and
does not decode; the other three run the whole continuation."""
import ctypes as C

import numpy as np
import pytest

from form_tally import ran
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

CFGS = {
    128: dict(orc.TINY, n_heads=2, n_kv_heads=1),
    64: dict(orc.TINY),
    32: dict(orc.TINY, n_heads=8, n_kv_heads=2),
}
SEED_M, SEED_T = 909, 5150
SRC_CAP, FILLED, NPOS = 96, 41, 37
DST_CAPS = (41, 64, 96, 300)
APPEND, STEPS = 5, 8


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def caches(ctx, n_layers):
    return [(ctx.CacheK(l).copy(), ctx.CacheV(l).copy()) for l in range(n_layers)]


def same_caches(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


_REF = {}


def reference(lnb, hd):
    """per head_dim, once and never changed afterwards: the model, the text, the source context (41 rows, kept alive) with its caches, and what a
    context that prefilled the 37 rows ITSELF gives for the continuation: the logits of 5 appended rows, 8 greedy tokens, its KV rows; the oracle's
    one-token logits at 37..41 after its own 37-row forward"""
    if hd in _REF:
        return _REF[hd]
    cfg = CFGS[hd]
    nl = cfg["n_layers"]
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(SEED_M).finalize()
    toks = lnb.synth_tokens(SEED_T, 64, cfg["vocab_size"])
    src = lnb.InferenceContext(gm, SRC_CAP)
    src.Forward(toks[:FILLED], 0, want_logits=False)
    skv = caches(src, nl)
    own = lnb.InferenceContext(gm, SRC_CAP)
    own.Forward(toks[:NPOS], 0, want_logits=False)
    lg, arg = own.ForwardAppend(toks[NPOS:NPOS + APPEND], NPOS)
    gen = [int(t) for t in own.decode_greedy(arg, NPOS + APPEND, STEPS)[0]]
    okv = caches(own, nl)
    own.close()
    om = orc.Model(**cfg).fill_synthetic(SEED_M).finalize()
    oc = orc.Context(om, 64)
    oc.forward(toks[:NPOS], 0, want_logits=False)
    olg = np.stack([oc.forward(toks[NPOS + i:NPOS + i + 1], NPOS + i)[0][0].copy() for i in range(APPEND)])
    oc.close(); om.close()
    assert np.array_equal(bits(lg), bits(olg))                  # the reference itself against the CPU oracle
    for l in range(nl):                                         # a row does not depend on the call that computed it: 41-row and 37-row prefill agree below 37
        assert np.array_equal(skv[l][0][:NPOS], okv[l][0][:NPOS]) and np.array_equal(skv[l][1][:NPOS], okv[l][1][:NPOS])
    _REF[hd] = dict(cfg=cfg, nl=nl, gm=gm, toks=toks, src=src, skv=skv, logits=lg, olg=olg, arg=arg, gen=gen, okv=okv)
    return _REF[hd]


def stale_context(lnb, R, cap, k, **kw):
    """a destination that already holds 41 rows (min(41, cap)) of another text"""
    c = lnb.InferenceContext(R["gm"], cap, **kw)
    other = lnb.synth_tokens(SEED_T + 1 + k, FILLED, R["cfg"]["vocab_size"])
    c.Forward(other[:min(FILLED, cap)], 0, want_logits=False)
    return c


def check_forked(R, ctx, before, tag):
    """rows [0, 37) are the source's, rows from 37 on are what the context held before"""
    for l, (k, v) in enumerate(caches(ctx, R["nl"])):
        assert np.array_equal(k[:NPOS], R["skv"][l][0][:NPOS]) and np.array_equal(v[:NPOS], R["skv"][l][1][:NPOS]), (tag, l, "shared rows")
        assert np.array_equal(k[NPOS:], before[l][0][NPOS:]) and np.array_equal(v[NPOS:], before[l][1][NPOS:]), (tag, l, "rows from n_pos on")


def check_continuation(R, ctx, cap, tag):
    """ForwardAppend of 5 rows at 37, then 8 greedy steps: logits, tokens and KV rows of a context that prefilled the 37 tokens itself, the logits
    also against the CPU oracle's one-token steps"""
    toks, n = R["toks"], min(APPEND, cap - NPOS)
    lg, arg = ctx.ForwardAppend(toks[NPOS:NPOS + n], NPOS)
    assert np.array_equal(bits(lg), bits(R["logits"][:n])) and np.array_equal(bits(lg), bits(R["olg"][:n])), tag
    end = NPOS + n
    if n == APPEND:
        assert arg == R["arg"], tag
        got = [int(t) for t in ctx.decode_greedy(arg, NPOS + APPEND, STEPS)[0]]
        assert got == R["gen"], tag
        end += STEPS
    for l, (k, v) in enumerate(caches(ctx, R["nl"])):
        assert np.array_equal(k[:end], R["okv"][l][0][:end]) and np.array_equal(v[:end], R["okv"][l][1][:end]), (tag, l)


# how lnb_ctx_fork copies: (LNB_FORK_COPY, LNB_FORK_NT, LNB_FORK_SPLIT) and the forms the launch tally must show (and, of the kv_fork forms, no other)
FORK_KNOBS = {0: (0, 0, 0), 1: (1, 0, 0), "nt": (0, 1, 0), "split2": (0, 0, 2), "split4": (0, 1, 4)}        # (split4: four destinations, one group each)
FORK_FORMS = {0: ("kv_fork.plain",), 1: ("kv_fork.copy",), "nt": ("kv_fork.nt",), "split2": ("kv_fork.plain", "kv_fork.split"), "split4": ("kv_fork.nt", "kv_fork.split")}


@pytest.mark.parametrize("engine", [0, 1, "nt", "split2", "split4"], ids=["kernel", "copy-engine", "nt", "split2", "split4"])
@pytest.mark.parametrize("hd", sorted(CFGS))
def test_fork_bits_and_continuation(lnb, hd, engine, monkeypatch):
    R = reference(lnb, hd)
    (copy, nt, split), forms = FORK_KNOBS[engine], FORK_FORMS[engine]
    others = tuple(f for f in ("kv_fork.plain", "kv_fork.nt", "kv_fork.split", "kv_fork.copy") if f not in forms)
    monkeypatch.setenv("LNB_FORK_COPY", str(copy))             # LIVE, all three: read by every call
    monkeypatch.setenv("LNB_FORK_NT", str(nt))
    monkeypatch.setenv("LNB_FORK_SPLIT", str(split))
    dsts = [stale_context(lnb, R, cap, k) for k, cap in enumerate(DST_CAPS)]
    before = [caches(d, R["nl"]) for d in dsts]
    with ran(lnb, FORK_FORMS[engine], not_ran=others):
        assert R["src"].ForkPrefix(dsts, NPOS) is R["src"]
    for d, b, cap in zip(dsts, before, DST_CAPS):
        check_forked(R, d, b, (hd, engine, cap))
    assert same_caches(caches(R["src"], R["nl"]), R["skv"])    # the source over its whole capacity
    for d, cap in zip(dsts, DST_CAPS):
        check_continuation(R, d, cap, (hd, engine, cap))
    assert same_caches(caches(R["src"], R["nl"]), R["skv"])
    for d in dsts:
        d.close()


def test_zero_positions_copy_nothing_and_a_fork_of_a_fork_is_the_source(lnb):
    R = reference(lnb, 64)
    a, b = stale_context(lnb, R, 64, 0), stale_context(lnb, R, 41, 1)
    ka, kb = caches(a, R["nl"]), caches(b, R["nl"])
    R["src"].ForkPrefix([a, b], 0)
    assert same_caches(caches(a, R["nl"]), ka) and same_caches(caches(b, R["nl"]), kb)
    R["src"].ForkPrefix([a], NPOS)
    a.ForkPrefix([b], NPOS)                                     # capacity 64 -> 41, the source of this call a destination of the last
    check_forked(R, b, kb, "second hand")
    a.close(); b.close()


def test_speculative_decode_continues_a_destination_with_the_prefix_as_history(lnb):
    R = reference(lnb, 128)
    toks = R["toks"]
    d = stale_context(lnb, R, 300, 2)
    R["src"].ForkPrefix([d], NPOS)
    _, arg = d.ForwardAppend(toks[NPOS:NPOS + APPEND], NPOS, want_logits=False)
    d.set_draft(4, 1, 3, [arg] + R["gen"])                      # the known continuation as the corpus: drafts are accepted
    got, fin, st, _ = d.decode_speculative_until(toks[:NPOS + APPEND], arg, NPOS + APPEND, STEPS)
    assert [int(t) for t in got] == R["gen"] and not fin and st["accepted"] > 0
    end = NPOS + APPEND + STEPS
    for l, (k, v) in enumerate(caches(d, R["nl"])):
        assert np.array_equal(k[:end], R["okv"][l][0][:end]) and np.array_equal(v[:end], R["okv"][l][1][:end]), l
    d.close()


def test_fan_out_into_seventeen_members_of_a_live_batch(lnb):
    """17 = one past a column group of 16; the destinations already belong to the batch when the rows arrive (a batch holds pointers, not contents)"""
    R = reference(lnb, 64)
    cfg, toks, n = R["cfg"], R["toks"], 17
    ctxs = [stale_context(lnb, R, 64, 10 + s) for s in range(n)]
    bat = lnb.Batch(ctxs)
    R["src"].ForkPrefix(ctxs, NPOS)
    firsts = [int(t) for t in lnb.synth_tokens(SEED_T + 99, n, cfg["vocab_size"])]
    assert len(set(firsts)) > 8
    got, _ = bat.decode(firsts, [NPOS] * n, 6)
    kv = [caches(c, R["nl"]) for c in ctxs]
    for s in range(n):
        for l in range(R["nl"]):
            assert np.array_equal(kv[s][l][0][:NPOS], R["skv"][l][0][:NPOS]) and np.array_equal(kv[s][l][1][:NPOS], R["skv"][l][1][:NPOS]), (s, l)
    for s in (0, 8, 15, 16):                                    # both column groups, and the last member of the first
        own = lnb.InferenceContext(R["gm"], 64)
        own.Forward(toks[:NPOS], 0, want_logits=False)
        ref = [int(t) for t in own.decode_greedy(firsts[s], NPOS, 6)[0]]
        assert [int(t) for t in got[s]] == ref, s
        okv = caches(own, R["nl"])
        for l in range(R["nl"]):
            assert np.array_equal(kv[s][l][0][:NPOS + 6], okv[l][0][:NPOS + 6]) and np.array_equal(kv[s][l][1][:NPOS + 6], okv[l][1][:NPOS + 6]), (s, l)
        own.close()
    bat.close()
    for c in ctxs:
        c.close()


def test_stride_extremes_capacity_64_to_131072_and_back(lnb):
    cfg = CFGS[64]
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(SEED_M).finalize(131072)
    toks = lnb.synth_tokens(SEED_T, 64, cfg["vocab_size"])
    src = lnb.InferenceContext(gm, 64)
    src.Forward(toks[:FILLED], 0, want_logits=False)
    skv = caches(src, cfg["n_layers"])
    big = lnb.InferenceContext(gm, lnb.MAX_SEQ_LEN, max_rows=64, long_context=True)
    src.ForkPrefix([big], NPOS)
    for l in range(cfg["n_layers"]):
        k, v = big.CacheK(l), big.CacheV(l)
        assert np.array_equal(k[:NPOS], skv[l][0][:NPOS]) and np.array_equal(v[:NPOS], skv[l][1][:NPOS]), l
        assert not k[NPOS:].any() and not v[NPOS:].any(), l    # a fresh context: zeros beyond the prefix, all 131035 rows of them
    back = lnb.InferenceContext(gm, 64)
    big.ForkPrefix([back], NPOS)
    for l, (k, v) in enumerate(caches(back, cfg["n_layers"])):
        assert np.array_equal(k[:NPOS], skv[l][0][:NPOS]) and np.array_equal(v[:NPOS], skv[l][1][:NPOS]), l
        assert not k[NPOS:].any() and not v[NPOS:].any(), l
    assert same_caches(caches(src, cfg["n_layers"]), skv)
    back.close(); big.close(); src.close(); gm.close()


def test_a_stage_forks_the_layers_it_owns(lnb):
    cfg = CFGS[64]
    stage = lnb.LlamaTransformer(device=0, layer_begin=0, layer_end=1, **cfg).fill_synthetic(SEED_M).finalize()
    toks = np.ascontiguousarray(lnb.synth_tokens(SEED_T, FILLED, cfg["vocab_size"]), dtype=np.int32)
    a, b = lnb.InferenceContext(stage, SRC_CAP), lnb.InferenceContext(stage, 64)
    lnb._chk(a.L.lnb_forward_stage(a.h, lnb._p(toks), FILLED, 0, None, None))
    a.ForkPrefix([b], NPOS)
    ka, va, kb, vb = a.CacheK(0), a.CacheV(0), b.CacheK(0), b.CacheV(0)
    assert ka[:NPOS].any() and va[:NPOS].any()
    assert np.array_equal(kb[:NPOS], ka[:NPOS]) and np.array_equal(vb[:NPOS], va[:NPOS]) and not kb[NPOS:].any() and not vb[NPOS:].any()
    for c in (a, b):
        with pytest.raises(lnb.LnbError, match="not owned"):
            c.CacheK(1)
    blob = a.SavePrefix(NPOS)                                   # one cached layer, and the stage range in the header
    assert blob.size == 64 + 4 * NPOS * cfg["n_kv_heads"] * 64
    assert b.LoadPrefix(blob) == NPOS
    whole = lnb.InferenceContext(reference(lnb, 64)["gm"], 64)
    with pytest.raises(lnb.LnbError, match="stage parts"):
        whole.LoadPrefix(blob)
    whole.close(); a.close(); b.close(); stage.close()


def test_save_and_load(lnb):
    R = reference(lnb, 64)
    cfg, nl, L = R["cfg"], R["nl"], lnb.lib()
    blob = R["src"].SavePrefix(NPOS)
    kv_dim = cfg["n_kv_heads"] * (cfg["dim"] // cfg["n_heads"])
    assert blob.dtype == np.uint8 and blob.size == L.lnb_ctx_prefix_bytes(R["src"].h, NPOS) == 64 + nl * 2 * 2 * NPOS * kv_dim
    assert bytes(blob[:8]) == b"LNBKV1\0\0" and not blob[36:64].any()
    assert [int(x) for x in blob[8:36].view("<u4")] == [1, NPOS, 0, 3 * nl, cfg["n_kv_heads"], cfg["dim"] // cfg["n_heads"], nl]
    # the arrays are the device layout of a context of capacity n_pos: layer 0's K, then its V
    k0 = blob[64:64 + 2 * NPOS * kv_dim].view(np.uint16).reshape(cfg["n_kv_heads"], -1, NPOS, 8)
    hd = cfg["dim"] // cfg["n_heads"]
    assert np.array_equal(k0.transpose(2, 0, 1, 3).reshape(NPOS, cfg["n_kv_heads"], hd), R["skv"][0][0][:NPOS])
    v0 = blob[64 + 2 * NPOS * kv_dim:64 + 4 * NPOS * kv_dim].view(np.uint16).reshape(NPOS, cfg["n_kv_heads"], hd)
    assert np.array_equal(v0, R["skv"][0][1][:NPOS])
    for cap in (41, 300):
        c = lnb.InferenceContext(R["gm"], cap)
        assert c.LoadPrefix(blob) == NPOS
        for l, (k, v) in enumerate(caches(c, nl)):
            assert np.array_equal(k[:NPOS], R["skv"][l][0][:NPOS]) and np.array_equal(v[:NPOS], R["skv"][l][1][:NPOS]), (cap, l)
            assert not k[NPOS:].any() and not v[NPOS:].any(), (cap, l)
        assert np.array_equal(c.SavePrefix(NPOS), blob), cap   # the same rows give the same bytes, whatever the capacity
        check_continuation(R, c, cap, ("loaded", cap))
        c.close()
    assert R["src"].SavePrefix(0).size == 64 == L.lnb_ctx_prefix_bytes(R["src"].h, 0)
    # refusals: each with a message, each before anything is written
    c = stale_context(lnb, R, 64, 5)
    small = stale_context(lnb, R, 16, 6)
    kc, ks = caches(c, nl), caches(small, nl)
    flipped = blob.copy(); flipped[3] ^= 0xFF
    version = blob.copy(); version[8] = 2
    other = reference(lnb, 128)["src"].SavePrefix(NPOS)
    assert other.size == blob.size                              # one KV head of 128 = two of 64: only the header tells them apart
    for bad, msg in ((blob[:-1], "bytes"), (np.concatenate([blob, np.zeros(1, np.uint8)]), "bytes"), (blob[:40], "header"), (flipped, "magic"),
                     (version, "version"), (other, "KV heads")):
        with pytest.raises(lnb.LnbError, match=msg):
            c.LoadPrefix(bad)
        assert len(L.lnb_last_error()) > 0
    with pytest.raises(lnb.LnbError, match="37 positions, the context 16"):
        small.LoadPrefix(blob)
    buf = np.zeros(blob.size, dtype=np.uint8)
    assert L.lnb_ctx_save_prefix(R["src"].h, NPOS, lnb._p(buf), blob.size - 1) < 0 and b"bytes" in L.lnb_last_error() and not buf.any()
    assert L.lnb_ctx_prefix_bytes(R["src"].h, SRC_CAP + 1) < 0 and L.lnb_ctx_prefix_bytes(R["src"].h, -1) < 0 and len(L.lnb_last_error()) > 0
    assert same_caches(caches(c, nl), kc) and same_caches(caches(small, nl), ks)
    c.close(); small.close()


def test_refusals_leave_every_destination_as_it_was(lnb):
    R = reference(lnb, 64)
    L, nl, src = lnb.lib(), R["nl"], R["src"]
    err = lambda: L.lnb_last_error().decode()
    a, b = stale_context(lnb, R, 64, 7), stale_context(lnb, R, 41, 8)
    before = [caches(a, nl), caches(b, nl)]
    arr = lambda *cs: (C.c_void_p * len(cs))(*[c.h if c is not None else None for c in cs])
    fork = lambda s, n_pos, cs, n=None: L.lnb_ctx_fork(s.h if s is not None else None, n_pos, arr(*cs) if cs is not None else None, len(cs) if n is None else n)
    assert fork(None, NPOS, [a, b]) < 0 and "null" in err()
    assert fork(src, NPOS, None, 2) < 0 and "null" in err()
    assert fork(src, NPOS, [a, None]) < 0 and "destination 1 is NULL" in err()
    assert fork(src, NPOS, [a, b], 0) < 0 and "n_dst" in err()
    assert fork(src, NPOS, [a, b], lnb.MAX_FORK + 1) < 0 and "n_dst" in err()
    assert fork(src, -1, [a, b]) < 0 and "n_pos" in err()
    assert fork(src, NPOS, [a, src]) < 0 and "destination 1 is the source" in err()
    assert fork(src, NPOS, [a, b, a]) < 0 and "0 and 2" in err()
    twin = lnb.LlamaTransformer(device=0, **R["cfg"]).fill_synthetic(SEED_M).finalize()      # the same weights behind another handle
    t = lnb.InferenceContext(twin, 64)
    assert fork(src, NPOS, [a, t]) < 0 and "destination 1" in err() and "another lnb_model" in err()
    assert fork(src, 42, [a, b]) < 0 and "42" in err() and "41" in err() and "destination 1" in err()
    assert fork(src, SRC_CAP + 1, [a]) < 0 and "97" in err() and "96" in err() and "source" in err()
    # a lnb_forward_stage_begin that has not been ended, on a destination and on the source (a stand-in context: the module's source stays as it is)
    toks = np.ascontiguousarray(R["toks"][:20], dtype=np.int32)
    p = lnb.InferenceContext(R["gm"], 64)
    lnb._chk(L.lnb_forward_stage_begin(p.h, lnb._p(toks), 20, 0, 1))
    assert fork(src, NPOS, [b, p]) < 0 and "destination 1" in err() and "lnb_forward_stage_begin" in err()
    assert fork(p, 10, [a, b]) < 0 and "source" in err() and "lnb_forward_stage_begin" in err()
    lnb._chk(L.lnb_forward_stage_end(p.h, C.byref(C.c_int32(0))))
    p.close()
    assert same_caches(caches(a, nl), before[0]) and same_caches(caches(b, nl), before[1])
    assert same_caches(caches(src, nl), R["skv"])
    assert fork(src, NPOS, [a, b]) == 0                        # and the same arguments, in order, are accepted
    check_forked(R, a, before[0], "a"); check_forked(R, b, before[1], "b")
    t.close(); twin.close(); a.close(); b.close()
