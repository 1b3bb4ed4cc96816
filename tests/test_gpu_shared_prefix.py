"""Shared-prefix attention of a batched decode (-m gpu): lnb_batch_set_shared_prefix reads positions [0, n_pos) of every member from ONE source
context (attn_shared_scores_kernel + attn_shared_pv_kernel).  Every comparison is bit-exact against the CPU oracle's own run of each member's
full text (the prefix plus the member's suffix): token lists, and raw KV rows with np.array_equal.
Shapes: n_pos 3 (no full 16-tile: all continuation), 37 (two tiles + a remainder that is no multiple of 4), 272 (an exact multiple of 16), 517 (beyond a
256-position scores block and 512); suffixes 0 / 1 / 20 inside one row tile; 1 / 5 / 17 / 40 members (a nearly empty tile, a ragged one, two
tiles and the column-groups feed, the rows feed); three member capacities, all different from the source's."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from form_tally import ran

pytestmark = pytest.mark.gpu

CFGS = {"tiny_hd64": dict(orc.TINY), "h8kv2_hd128": dict(orc.TINY, dim=1024, n_heads=8, n_kv_heads=2)}
SHARED_FORMS = ("attn_batch.shared_scores", "attn_batch.shared_pv")
NPOS, SUFFIX, CAPS, SRC_CAP = (3, 37, 272, 517), (0, 1, 20), (600, 640, 700), 560
STEPS = 11
N_REF = STEPS + 4
SEED = 909
# (members, with the matrix-core copy, force_zseq)
RUNS = [(1, True, 0), (5, True, 1), (5, False, 0), (17, True, 0), (17, False, 1), (40, True, 0)]


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


_ORACLE, _MODELS = {}, {}


def oracle_pool(name, n_pos):
    """per (config, prefix length), once: for each suffix length the text, the oracle's greedy tokens after it and its K / V rows"""
    if name not in _ORACLE:
        _ORACLE[name] = {"om": orc.Model(**CFGS[name]).fill_synthetic(SEED).finalize()}
    pool = _ORACLE[name]
    if n_pos not in pool:
        cfg, rows = CFGS[name], []
        prefix = [int(t) for t in orc.synth_tokens(9000 + n_pos, n_pos, cfg["vocab_size"])]
        for k, sl in enumerate(SUFFIX):
            text = prefix + [int(t) for t in orc.synth_tokens(9100 + k, sl, cfg["vocab_size"])]
            oc = orc.Context(pool["om"], len(text) + N_REF + 2)
            r, _ = oc.generate(text, N_REF)
            kv = [(oc.cache(l, 0).copy(), oc.cache(l, 1).copy()) for l in range(cfg["n_layers"])]
            oc.close()
            rows.append((text, [int(t) for t in r], kv))
        pool[n_pos] = rows
    return pool[n_pos]


def model(lnb, name, copy):
    if (name, copy) not in _MODELS:
        gm = lnb.LlamaTransformer(**CFGS[name]).fill_synthetic(SEED).finalize()
        _MODELS[name, copy] = gm.enable_batch() if copy else gm
    return _MODELS[name, copy]


def members(lnb, gm, pool, n_pos, n, fork_all=False):
    """the source with the prefix, and n members at the end of their texts: suffix lengths and capacities cycle; a member with an empty suffix is never
    forked (unless fork_all): its rows below n_pos stay zero.  -> (src, contexts, suffix class per member, first tokens, start positions)"""
    src = lnb.InferenceContext(gm, SRC_CAP)
    _, a0 = src.Forward(pool[0][0], 0, want_logits=False)
    kinds = [s % len(SUFFIX) for s in range(n)]
    ctxs = [lnb.InferenceContext(gm, CAPS[s % len(CAPS)]) for s in range(n)]
    forked = [c for c, k in zip(ctxs, kinds) if SUFFIX[k] or fork_all]
    if forked:
        src.ForkPrefix(forked, n_pos)
    firsts = [c.ForwardAppend(pool[k][0][n_pos:], n_pos, want_logits=False)[1] if SUFFIX[k] else a0 for c, k in zip(ctxs, kinds)]
    assert firsts == [pool[k][1][0] for k in kinds]
    return src, ctxs, kinds, firsts, [n_pos + SUFFIX[k] for k in kinds]


def assert_rows(ctx, kv, lo, hi, tag):
    for layer, (k, v) in enumerate(kv):
        assert np.array_equal(ctx.CacheK(layer)[lo:hi], k[lo:hi]), tag + (layer, "K")
        assert np.array_equal(ctx.CacheV(layer)[lo:hi], v[lo:hi]), tag + (layer, "V")


def close_all(b, src, ctxs):
    b.close()
    for c in ctxs + [src]:
        c.close()


@pytest.mark.parametrize("n,copy,zseq", RUNS)
@pytest.mark.parametrize("n_pos", NPOS)
@pytest.mark.parametrize("name", sorted(CFGS))
def test_shared_prefix_equals_the_oracle_per_member(lnb, name, n_pos, n, copy, zseq):
    cfg, pool = CFGS[name], oracle_pool(name, n_pos)
    src, ctxs, kinds, firsts, starts = members(lnb, model(lnb, name, copy), pool, n_pos, n)
    b = lnb.Batch(ctxs).set_shared_prefix(src, n_pos).set_attention(-1, zseq)
    before = ctxs[0].zseq_count()
    with ran(lnb, SHARED_FORMS, not_ran=("attn_batch.gqa", "attn_batch.plain", "attn_batch.dense")):
        got, _ = b.decode(firsts, starts, STEPS)
    assert b.attention_form() == 2
    if zseq:
        assert ctxs[0].zseq_count() >= before + n * cfg["n_heads"] * cfg["n_layers"] * STEPS
    more, _ = b.decode([pool[k][1][STEPS] for k in kinds], [p + STEPS for p in starts], 1)      # a second call goes on where the first stopped
    assert b.attention_form() == 2
    for s, k in enumerate(kinds):
        assert [int(t) for t in got[s]] + [int(more[s][0])] == pool[k][1][1:STEPS + 2], (name, n_pos, n, s)
        assert_rows(ctxs[s], pool[k][2], n_pos, starts[s] + STEPS + 1, (name, n_pos, n, s))
    close_all(b, src, ctxs)


def test_the_kernels_read_the_source_not_the_members(lnb):
    name, n_pos, n = "h8kv2_hd128", 37, 5
    pool, gm = oracle_pool(name, n_pos), model(lnb, name, True)
    src, ctxs, kinds, firsts, starts = members(lnb, gm, pool, n_pos, n)
    other = lnb.InferenceContext(gm, SRC_CAP)                # another prompt of the same length over every second member's rows [0, n_pos)
    other.Forward(orc.synth_tokens(4242, n_pos, CFGS[name]["vocab_size"]), 0, want_logits=False)
    other.ForkPrefix(ctxs[::2], n_pos)
    nl = CFGS[name]["n_layers"]
    held = [[(c.CacheK(l)[:n_pos].copy(), c.CacheV(l)[:n_pos].copy()) for l in range(nl)] for c in ctxs + [src]]
    assert not np.array_equal(held[0][0][0], held[-1][0][0])
    b = lnb.Batch(ctxs).set_shared_prefix(src, n_pos)
    with ran(lnb, SHARED_FORMS):
        got, _ = b.decode(firsts, starts, STEPS)
    assert b.attention_form() == 2
    for s, k in enumerate(kinds):
        assert [int(t) for t in got[s]] == pool[k][1][1:STEPS + 1], s
        assert_rows(ctxs[s], pool[k][2], n_pos, starts[s] + STEPS, (s,))
    for c, kv in zip(ctxs + [src], held):
        assert_rows(c, kv, 0, n_pos, ("rows below n_pos",))
    other.close()
    close_all(b, src, ctxs)


def test_clearing_returns_to_the_members_own_rows(lnb):
    name, n_pos, n = "tiny_hd64", 272, 5
    pool = oracle_pool(name, n_pos)
    src, ctxs, kinds, firsts, starts = members(lnb, model(lnb, name, True), pool, n_pos, n, fork_all=True)
    b = lnb.Batch(ctxs).set_shared_prefix(src, n_pos)
    with ran(lnb, SHARED_FORMS):
        got, _ = b.decode(firsts, starts, STEPS)
    assert b.attention_form() == 2
    b.set_shared_prefix(None, 0)
    last, _ = b.decode([pool[k][1][STEPS] for k in kinds], [p + STEPS for p in starts], 2)
    assert b.attention_form() == 0
    for s, k in enumerate(kinds):
        assert [int(t) for t in got[s]] + [int(t) for t in last[s]] == pool[k][1][1:STEPS + 3], s
        assert_rows(ctxs[s], pool[k][2], 0, starts[s] + STEPS + 2, (s,))
    src.reset()                                              # no longer attached
    close_all(b, src, ctxs)


def test_refusals_name_the_argument_and_change_nothing(lnb):
    name, n_pos, n = "tiny_hd64", 37, 5
    pool, gm = oracle_pool(name, n_pos), model(lnb, name, True)
    src, ctxs, kinds, firsts, starts = members(lnb, gm, pool, n_pos, n)
    L = lnb.lib()
    err = lambda: L.lnb_last_error().decode()
    b = lnb.Batch(ctxs).set_shared_prefix(src, n_pos)
    put = lambda s, p: L.lnb_batch_set_shared_prefix(b.h, s.h if s is not None else None, p)
    assert put(src, -1) < 0 and "n_pos" in err()
    assert put(src, SRC_CAP + 1) < 0 and "src" in err() and str(SRC_CAP) in err()
    wide = lnb.InferenceContext(gm, CAPS[0] + 100)
    assert put(wide, CAPS[0]) < 0 and "member 0" in err() and str(CAPS[0]) in err()
    wide.close()
    twin = lnb.LlamaTransformer(device=0, **CFGS[name]).fill_synthetic(SEED).finalize()       # the same weights behind another handle
    t = lnb.InferenceContext(twin, SRC_CAP)
    assert put(t, n_pos) < 0 and "src" in err() and "another model" in err()
    ctxs[2].set_mode("fast")
    assert put(src, n_pos) < 0 and "member 2" in err() and "tolerance" in err()
    ctxs[2].set_mode("exact")
    low = list(starts); low[1] = n_pos - 1
    out = np.zeros((n, 2), dtype=np.int32)
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert L.lnb_batch_decode(b.h, ip(firsts), ip(low), 2, lnb._p(out), None) < 0 and "start_pos" in err() and "sequence 1" in err()
    assert L.lnb_batch_set_state(b.h, None, ip(starts)) < 0 and "shared prefix" in err()
    assert L.lnb_ctx_reset(src.h) < 0 and "shared prefix" in err()
    assert L.lnb_ctx_destroy(src.h) < 0 and "shared prefix" in err()
    # nothing changed: the prefix set first still serves the batch
    with ran(lnb, SHARED_FORMS):
        got, _ = b.decode(firsts, starts, STEPS)
    assert b.attention_form() == 2
    for s, k in enumerate(kinds):
        assert [int(t) for t in got[s]] == pool[k][1][1:STEPS + 1], s
    t.close(); twin.close()
    close_all(b, src, ctxs)


def test_a_pending_stage_call_is_refused(lnb):
    name, n_pos, n = "tiny_hd64", 37, 2
    pool, gm = oracle_pool(name, n_pos), model(lnb, name, True)
    src, ctxs, kinds, firsts, starts = members(lnb, gm, pool, n_pos, n, fork_all=True)
    L = lnb.lib()
    err = lambda: L.lnb_last_error().decode()
    b = lnb.Batch(ctxs)
    one = np.ascontiguousarray([firsts[0]], dtype=np.int32)
    for who, word in ((src, "src"), (ctxs[0], "member 0")):
        lnb._chk(L.lnb_forward_stage_begin(who.h, lnb._p(one), 1, n_pos, 1))
        assert L.lnb_batch_set_shared_prefix(b.h, src.h, n_pos) < 0 and word in err() and "lnb_forward_stage_begin" in err()
        lnb._chk(L.lnb_forward_stage_end(who.h, C.byref(C.c_int32(0))))
    assert b.attention_form() == 0
    close_all(b, src, ctxs)
