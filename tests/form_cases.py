"""Model-level cases shared by tests/test_gpu_forms.py and its child processes: small geometries whose sizes are NOT multiples of 128 (and two that are),
one oracle run per geometry -- multi-row Forward of 17 / 40 / 83 rows at position 0, then on the 83-row context four greedy one-token steps, appended rows
(3, then 20: the oracle's one-token steps, which is what lnb_forward_append promises), eight more greedy tokens -- and the checks of a device context
against it: every logit's bits, the argmax, the K and V bits of every layer."""
import numpy as np

from oracle import oracle as orc

GEOS = {
    # dim 192 = 1.5 x 128, three heads of 64, FFN hidden 704 = 5.5 x 128: NO product has a K that is a multiple of 128
    "odd192": dict(orc.TINY, dim=192, n_heads=3, n_kv_heads=3, multiple_of=64, vocab_size=520, n_layers=2),
    # dim 256, two heads of 128 on one KV head, FFN hidden 888 = 6.94 x 128: only w2 has such a K
    "odd_hidden": dict(orc.TINY, dim=256, n_heads=2, n_kv_heads=1, multiple_of=8, vocab_size=520, n_layers=2),
    # oracle.TINY with a ragged vocabulary (520 = 32.5 tiles of 16): every K a multiple of 128
    "tiny520": dict(orc.TINY, vocab_size=520, n_layers=2),
    # dim 1024, FFN hidden 3584: wo and w2 have K = a whole number of rowcast_lds_kernel's 512-step stages
    "wide1024": dict(orc.TINY, dim=1024, n_heads=8, n_kv_heads=2, vocab_size=520, n_layers=2),
}
HIDDEN = {"odd192": 704, "odd_hidden": 888, "tiny520": 896, "wide1024": 3584}
SEED, CAP, ROWS = 4321, 128, (17, 40, 83)
N_STEPS, APPENDS, N_GREEDY = 4, (3, 20), 8
_REF, _GM = {}, {}


def one(t):
    return np.array([int(t)], dtype=np.int32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def reference(geo):
    """the oracle's side, computed once per geometry and process and never changed"""
    if geo in _REF:
        return _REF[geo]
    cfg = GEOS[geo]
    V, nl = cfg["vocab_size"], cfg["n_layers"]
    om = orc.Model(**cfg).fill_synthetic(SEED).finalize()
    assert om.ffn_hidden == HIDDEN[geo]
    toks = orc.synth_tokens(77, ROWS[-1] + sum(APPENDS), V)
    R = {"cfg": cfg, "toks": toks, "prefill": {}}
    for rows in ROWS:                                            # (the last one stays open: everything below continues it)
        oc = orc.Context(om, CAP)
        lo, am = oc.forward(toks[:rows], 0)
        R["prefill"][rows] = (lo, am, [(oc.cache(l, 0)[:rows].copy(), oc.cache(l, 1)[:rows].copy()) for l in range(nl)])
        if rows != ROWS[-1]:
            oc.close()
    pos, tok = ROWS[-1], am
    R["steps"] = []                                              # (token fed, its logits row, the argmax)
    for _ in range(N_STEPS):
        lo1, t = oc.forward(one(tok), pos)
        R["steps"].append((tok, lo1[0].copy(), t))
        tok, pos = t, pos + 1
    R["appends"], at = [], ROWS[-1]                              # (start position, tokens, their logits rows, the argmax of the last)
    for n in APPENDS:
        rows_ = []
        for i in range(n):
            lo1, t = oc.forward(one(toks[at + i]), pos + i)
            rows_.append(lo1[0].copy())
        R["appends"].append((pos, toks[at:at + n], np.stack(rows_), t))
        at, pos = at + n, pos + n
    R["greedy"] = (t, pos, [])                                   # (first token, its position, the eight that follow)
    tok = t
    for i in range(N_GREEDY):
        _, tok = oc.forward(one(tok), pos + i, want_logits=False)
        R["greedy"][2].append(int(tok))
    R["end"] = pos + N_GREEDY
    assert R["end"] <= CAP
    R["kv"] = [(oc.cache(l, 0)[:R["end"]].copy(), oc.cache(l, 1)[:R["end"]].copy()) for l in range(nl)]
    oc.close(); om.close()
    _REF[geo] = R
    return R


def gpu_model(lnb, geo, copy=False):
    """one device model per (geometry, with or without the matrix-core copy) and process; built under the environment of its first use"""
    if (geo, copy) not in _GM:
        gm = lnb.LlamaTransformer(device=0, **GEOS[geo]).fill_synthetic(SEED).finalize()
        _GM[(geo, copy)] = gm.enable_batch() if copy else gm
        assert (gm.batch_bytes() > 0) == copy and gm.ffn_hidden == HIDDEN[geo]
    return _GM[(geo, copy)]


def kv_equal(gc, kv, upto, tag):
    for l, (k, v) in enumerate(kv):
        assert np.array_equal(gc.CacheK(l)[:upto], k[:upto]), tag + (l, "K")
        assert np.array_equal(gc.CacheV(l)[:upto], v[:upto]), tag + (l, "V")


def check_prefill(lnb, gm, R, rows, tag=()):
    """Forward of `rows` rows at position 0 on a fresh context -> the context"""
    gc = lnb.InferenceContext(gm, CAP)
    lg, am = gc.Forward(R["toks"][:rows], 0)
    lo, ao, kv = R["prefill"][rows]
    assert same(lg, lo), tag + (rows, "logits")
    assert am == ao, tag + (rows, "argmax")
    kv_equal(gc, kv, rows, tag + (rows,))
    return gc


def check_steps(gc, R, n=N_STEPS, tag=()):
    """n one-token steps behind the 83-row prefill: logits bits, argmax, the new KV rows"""
    pos = ROWS[-1]
    for tok, lo, t in R["steps"][:n]:
        lg, tg = gc.Forward(one(tok), pos)
        assert same(lg[0], lo) and tg == t, tag + ("step", pos)
        pos += 1
    kv_equal(gc, R["kv"], pos, tag + ("steps",))


def check_appends(gc, R, tag=()):
    for pos, toks, rows, t in R["appends"]:
        lg, tg = gc.ForwardAppend(toks, pos)
        assert same(lg, rows) and tg == t, tag + ("append", pos, len(toks))
        kv_equal(gc, R["kv"], pos + len(toks), tag + ("append", pos))


def check_greedy(gc, R, tag=()):
    first, pos, want = R["greedy"]
    got, _ = gc.decode_greedy(first, pos, N_GREEDY)
    assert [int(t) for t in got] == want, tag + ("greedy",)
    kv_equal(gc, R["kv"], R["end"], tag + ("greedy",))
