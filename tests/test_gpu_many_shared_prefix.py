"""Shared prefix of the ragged passes (-m gpu): lnb_model_set_many_shared_prefix makes lnb_forward_append_many and the speculative-many calls read positions
[0, n_pos) of every column from ONE source context (attn_ragged_scores_kernel + attn_ragged_pv_kernel).  Every comparison is bit-exact against the CPU oracle's
own run of each member's full text.  n_pos 3 (no full tile), 37 (tiles + a remainder), 48 (no mixed tile); 0 / 5 / 40 positions of own text in each member (40
behind 37: segment C is exactly one tile); 9 / 1 / 3 / 4 new rows (G = 4: a 9-row member fills two uniform tiles, those behind it straddle tiles)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from form_tally import ran
from test_gpu_shared_prefix import CFGS, SEED, lnb, model  # noqa: F401  (that file's two configs, its library fixture and its model cache)

RAGGED_FORMS = ("attn_many.ragged_scores", "attn_many.ragged_pv")
NPOS, OWN, ROWS, CAPS, SRC_CAP = (3, 37, 48), (0, 5, 40), (9, 1, 3, 4), (120, 136, 160), 64
# (members, with the matrix-core copy, flags, LNB_APPEND_MANY_COLS or 0: in passes of 16 a member straddles two passes)
RUNS = [(1, True, 0, 0), (5, True, 1, 0), (5, False, 2, 0), (5, False, 0, 0), (33, True, 0, 0), (33, False, 0, 16)]
# speculative: member 0 stands beyond position 64 and asks for 8 columns, the others for 2 -- 16 in all, so the first tile of a pass is member 0's at G = 2 and 4
SPEC_N, SPEC_STEPS, SPEC_BUDGET, SPEC_SUFFIX, SPEC_DRAFT = 5, 24, 16, (33, 1, 7, 12, 20), (7, 1, 1, 1, 1)
gpu = pytest.mark.gpu
_ORACLE = {}
tokens = lambda seed, n, name: [int(t) for t in orc.synth_tokens(seed, n, CFGS[name]["vocab_size"])]


def test_the_symbols_and_the_scratch_formula():
    import lnb
    L, (tiles, kvh, T) = lnb.lib(), ((127 * 4 + 15) // 16, 8, 4100)      # 127 columns of 32 / 8 heads: a ragged last tile
    for sym in ("lnb_model_set_many_shared_prefix", "lnb_model_many_shared_info", "lnb_model_many_zseq_count", "lnb_many_shared_scratch_bytes"):
        assert sym in lnb.EXPORTS and hasattr(L, sym)
    # lnb_shared_idx_bytes + lnb_shared_z_bytes as include/lnb.h writes them out
    assert L.lnb_many_shared_scratch_bytes(127, 32, 8, T) == kvh * tiles * ((T + 15) // 16 * 512 + 16 * ((T + 255) // 256) * 8)
    assert L.lnb_many_shared_scratch_bytes(0, 32, 8, T) < 0 and L.lnb_many_shared_scratch_bytes(127, 32, 5, T) < 0


def oracle_run(name, text, n_out):
    """-> (the oracle's n_out greedy tokens after text, its K / V rows per layer); computed once per text"""
    pool = _ORACLE.setdefault(name, {})
    if "om" not in pool:
        pool["om"] = orc.Model(**CFGS[name]).fill_synthetic(SEED).finalize()
    if (tuple(text), n_out) not in pool:
        oc = orc.Context(pool["om"], len(text) + n_out + 2)
        r, _ = oc.generate(text, n_out)
        pool[tuple(text), n_out] = ([int(t) for t in r], [(oc.cache(l, 0).copy(), oc.cache(l, 1).copy()) for l in range(CFGS[name]["n_layers"])])
        oc.close()
    return pool[tuple(text), n_out]


def members(lnb, gm, name, n_pos, own, n):
    """the source with the prefix, and n members holding `own` positions of text of their own behind it; their new rows cycle over ROWS.  A member without own
    text is never forked: below n_pos every second one holds ANOTHER prompt's rows, the others zeros.  -> (src, contexts, texts so far, new rows)"""
    gm.set_many_shared_prefix(None, 0)
    prefix = tokens(9000 + n_pos, n_pos, name)
    src = lnb.InferenceContext(gm, SRC_CAP)
    src.Forward(prefix, 0, want_logits=False)
    ctxs = [lnb.InferenceContext(gm, CAPS[s % len(CAPS)]) for s in range(n)]
    heads = [prefix + tokens(9100 + s % 4, own, name) for s in range(n)]
    if own:
        for c0 in range(0, n, 32):
            src.ForkPrefix(ctxs[c0:c0 + 32], n_pos)
        lnb.ForwardAppendMany(ctxs, [h[n_pos:] for h in heads], [n_pos] * n, want_logits=False)
    else:
        other = lnb.InferenceContext(gm, SRC_CAP)
        other.Forward(tokens(4242, n_pos, name), 0, want_logits=False)
        other.ForkPrefix(ctxs[::2], n_pos)
        other.close()
    return src, ctxs, heads, [tokens(9200 + s % 4, ROWS[s % 4], name) for s in range(n)]


def assert_oracle(name, ctxs, heads, tails, am, n_pos):
    for s, c in enumerate(ctxs):
        (want, kv), rows = oracle_run(name, heads[s] + tails[s], 1), slice(n_pos, len(heads[s]) + len(tails[s]))
        assert int(am[s]) == want[0], (name, n_pos, s)
        for layer, (k, v) in enumerate(kv):
            assert np.array_equal(c.CacheK(layer)[rows], k[rows]) and np.array_equal(c.CacheV(layer)[rows], v[rows]), (name, n_pos, s, layer)


def has_own_tile(G, n_pos, start, rows, width):
    """does a pass hold a uniform tile -- 16 rows r = column * G + g, dead rows aliasing the last live one, all of ONE member -- with R16 > Q16"""
    cols = [(s, start + r) for s in range(len(rows)) for r in range(rows[s])]
    for pas in (cols[p0:p0 + width] for p0 in range(0, len(cols), width)):
        tiles = [[pas[min(r, len(pas) * G - 1) // G] for r in range(t, t + 16)] for t in range(0, len(pas) * G, 16)]
        if any(len({m for m, _ in t}) == 1 and ((min(p for _, p in t) + 1) & ~15) > ((n_pos + 15) & ~15) for t in tiles):
            return True
    return False


@gpu
@pytest.mark.parametrize("n,copy,flags,cols", RUNS)
@pytest.mark.parametrize("own", OWN)
@pytest.mark.parametrize("n_pos", NPOS)
@pytest.mark.parametrize("name", sorted(CFGS))
def test_append_many_behind_a_shared_prefix_equals_the_oracle(lnb, monkeypatch, name, n_pos, own, n, copy, flags, cols):
    cfg, gm = CFGS[name], model(lnb, name, copy)
    src, ctxs, heads, tails = members(lnb, gm, name, n_pos, own, n)
    monkeypatch.delenv("LNB_APPEND_MANY_COLS", raising=False)
    if cols:
        monkeypatch.setenv("LNB_APPEND_MANY_COLS", str(cols))
    below = [c.CacheK(0)[:n_pos].copy() for c in ctxs + [src]]
    assert own or (below[0].any() and not np.array_equal(below[0], below[-1]) and not any(b.any() for b in below[1:-1:2]))     # another prompt's rows; zeros
    before = gm.set_many_shared_prefix(src, n_pos, flags).many_shared_info()["zseq"]
    with ran(lnb, RAGGED_FORMS, not_ran="attn_batch"):
        _, am = lnb.ForwardAppendMany(ctxs, tails, [n_pos + own] * n, want_logits=False)
    info, rows = gm.many_shared_info(), sum(len(t) for t in tails)
    assert info["shared_passes"] == gm.append_many_info()["passes"] == -(-rows // (cols or 128))
    own_tile = not flags & 2 and has_own_tile(cfg["n_heads"] // cfg["n_kv_heads"], n_pos, n_pos + own, [len(t) for t in tails], cols or 128)
    assert (info["own_mfma_tiles"] > 0) == own_tile
    assert not flags & 1 or info["zseq"] >= before + rows * cfg["n_heads"] * cfg["n_layers"]
    assert_oracle(name, ctxs, heads, tails, am, n_pos)
    assert all(np.array_equal(c.CacheK(0)[:n_pos], b) for c, b in zip(ctxs + [src], below)), "the source is what is read: nobody's rows below n_pos change"
    gm.set_many_shared_prefix(None, 0)
    [c.close() for c in ctxs + [src]]


@gpu
@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("name", sorted(CFGS))
def test_speculative_many_behind_a_shared_prefix(lnb, name, sample):
    n_pos, gm, nl = 37, model(lnb, name, True), CFGS[name]["n_layers"]
    texts = [tokens(9000 + n_pos, n_pos, name) + tokens(9300 + s, SPEC_SUFFIX[s], name) for s in range(SPEC_N)]
    refs = [oracle_run(name, t, SPEC_STEPS + 2) for t in texts]
    def run(shared):
        src, ctxs, _, _ = members(lnb, gm, name, n_pos, 0, SPEC_N)
        if not shared:
            src.ForkPrefix(ctxs, n_pos)
        gm.set_many_shared_prefix(src if shared else None, n_pos)
        with ran(lnb, RAGGED_FORMS if shared else (), not_ran="attn_batch" if shared else RAGGED_FORMS):
            _, am = lnb.ForwardAppendMany(ctxs, [t[n_pos:] for t in texts], [n_pos] * SPEC_N, want_logits=False)
            assert [int(a) for a in am] == [r[0][0] for r in refs]
            for c, r, d in zip(ctxs, refs, SPEC_DRAFT):
                c.set_draft(d, 1, 4, r[0])                   # the draft corpus is the oracle's true continuation
            args = (texts, [r[0][0] for r in refs], [len(t) for t in texts], SPEC_STEPS, SPEC_BUDGET)
            samplers = [(0.8, 40, 0.95, 77 + s) for s in range(SPEC_N)]
            got = lnb.DecodeSpeculativeSampleMany(ctxs, samplers, *args) if sample else lnb.DecodeSpeculativeMany(ctxs, *args)
        info = gm.many_shared_info()
        assert info["shared_passes"] == (got[3]["passes"] if shared else 0)
        assert sample or (info["own_mfma_tiles"] > 0) == shared      # the device's own test of the packed columns found member 0's tile
        kv = [[(c.CacheK(l), c.CacheV(l)) for l in range(nl)] for c in ctxs]
        gm.set_many_shared_prefix(None, 0)
        [c.close() for c in ctxs + [src]]
        return got[:3], kv
    (tok, fin, stats), kv = run(True)
    (tok0, fin0, stats0), kv0 = run(False)
    assert fin == fin0 and stats == stats0
    for s in range(SPEC_N):
        rows = slice(n_pos, len(texts[s]) + len(tok[s]) - 1)
        assert [int(t) for t in tok[s]] == [int(t) for t in tok0[s]], s
        assert sample or ([int(t) for t in tok[s]] == refs[s][0][1:SPEC_STEPS + 1] and not fin[s]), s
        for l, w in ((l, w) for l in range(nl) for w in (0, 1)):
            assert np.array_equal(kv[s][l][w][rows], kv0[s][l][w][rows]) and (sample or np.array_equal(kv[s][l][w][rows], refs[s][1][l][w][rows])), (s, l, w)


def refusal(lnb, L, gm, kind, name, n_pos, own, src, ctxs, heads, tails):
    """-> the message of one refused call; a refused append or speculative call has written no cache"""
    err = lambda rc: L.lnb_last_error().decode() if rc < 0 else ""
    put = lambda m, s, p, f=0: err(L.lnb_model_set_many_shared_prefix(m.h, s.h, p, f))
    if kind in ("twin", "hd32"):                             # the same weights behind another handle; a model whose head_dim has no ragged form
        gm2 = lnb.LlamaTransformer(device=0, **(CFGS[name] if kind == "twin" else dict(orc.TINY, n_heads=8, n_kv_heads=2))).fill_synthetic(SEED).finalize()
        t = lnb.InferenceContext(gm2, SRC_CAP)
        msg = put(gm if kind == "twin" else gm2, t, n_pos)
        with ran(lnb, "attn_batch", not_ran=RAGGED_FORMS):   # ... goes on with the forms it had
            lnb.ForwardAppendMany([t], [tails[0]], [0], want_logits=False)
        t.close(); gm2.close()
        return msg
    if kind == "pending":
        lnb._chk(L.lnb_forward_stage_begin(src.h, lnb._p(np.ascontiguousarray([5], dtype=np.int32)), 1, n_pos, 1))
        msg = put(gm, src, n_pos)
        lnb._chk(L.lnb_forward_stage_end(src.h, C.byref(C.c_int32(0))))
        return msg
    if kind in ("below", "spec_below", "short"):             # member 1 starts below the prefix, or cannot hold it
        who, starts, small = list(ctxs), [n_pos + own, n_pos - 1, n_pos + own], lnb.InferenceContext(gm, n_pos)
        if kind == "short":
            who[1], starts[1] = small, 0
        kept = [c.CacheK(0).copy() for c in ctxs]
        with pytest.raises(lnb.LnbError, match="member 1") as x:
            lnb.DecodeSpeculativeMany(who, heads, [1] * 3, starts, 4) if kind == "spec_below" else lnb.ForwardAppendMany(who, tails, starts, want_logits=False)
        small.close()
        assert all(np.array_equal(c.CacheK(0), k) for c, k in zip(ctxs, kept))
        return str(x.value)
    return {"neg": lambda: put(gm, src, -1), "beyond": lambda: put(gm, src, SRC_CAP + 1), "flags": lambda: put(gm, src, n_pos, 4),
            "reset": lambda: err(L.lnb_ctx_reset(src.h)), "destroy": lambda: err(L.lnb_ctx_destroy(src.h))}[kind]()


REFUSALS = [("neg", "n_pos"), ("beyond", "src's capacity"), ("flags", "flags"), ("twin", "another model"), ("hd32", "head_dim"), ("pending", "lnb_forward_stage_begin"),
            ("below", "start_pos"), ("spec_below", "start_pos"), ("short", "capacity of"), ("reset", "shared prefix"), ("destroy", "shared prefix")]


@gpu
@pytest.mark.parametrize("kind,word", REFUSALS)
def test_refusals_change_nothing_and_clearing_restores_the_forms(lnb, kind, word):
    name, n_pos, own = "tiny_hd64", 37, 5
    gm, L = model(lnb, name, True), lnb.lib()
    src, ctxs, heads, tails = members(lnb, gm, name, n_pos, own, 3)
    gm.set_many_shared_prefix(src, n_pos)
    assert word in refusal(lnb, L, gm, kind, name, n_pos, own, src, ctxs, heads, tails)
    for forms, others in ((RAGGED_FORMS, ()), ("attn_batch", RAGGED_FORMS)):      # the prefix set first still serves; cleared, the forked members' own rows do
        with ran(lnb, forms, not_ran=others):
            _, am = lnb.ForwardAppendMany(ctxs, tails, [n_pos + own] * 3, want_logits=False)
        assert_oracle(name, ctxs, heads, tails, am, n_pos)
        gm.set_many_shared_prefix(None, 0)
    assert gm.many_shared_info()["shared_passes"] == 0 and L.lnb_ctx_destroy(src.h) == 0      # released by the clear
    src.h = C.c_void_p()
    [c.close() for c in ctxs]
