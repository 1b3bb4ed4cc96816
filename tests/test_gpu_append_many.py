"""Ragged append to many contexts (-m gpu): lnb_forward_append_many against lnb_forward_append, bit for bit.
Models: oracle.TINY (head_dim 64) and the head-geometry variants of tests/test_gpu_prefix_fork.py (head_dim 128 with one KV head, head_dim 32 with two of
eight heads); model seed 909, tokens from synth_tokens.  Every model exists twice with the same weights -- without and with enable_batch() -- so a pass runs
as rows of the streaming product on one handle and as matrix-core columns / column groups (up to 16 / 17..32 columns) on the other.
A member is described by (capacity, how it got its rows, start position, rows to append); the reference for it is a second context of the same capacity on
the same handle, brought to the same state, that takes the same rows through ForwardAppend.  References are computed once per (head_dim, member) and never
changed.  Members first hold 41 rows of another text, so a row that should have stayed is not zero."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

CFGS = {
    128: dict(orc.TINY, n_heads=2, n_kv_heads=1),
    64: dict(orc.TINY),
    32: dict(orc.TINY, n_heads=8, n_kv_heads=2),
}
SEED_M, SEED_T = 909, 7700
SRC_CAP, FILLED, NPOS = 96, 41, 37
STEPS = 8
LONG_CAP, LONG_FILL, LONG_CHUNK = 8192, 7990, 799
HDS = sorted(CFGS)


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_MODELS, _SRC, _REF, _TOK = {}, {}, {}, {}


def model(lnb, hd, batch):
    """the transformer of a head_dim, without / with the matrix-core copy (same weights); head_dim 128 carries RoPE rows for the long member"""
    if (hd, batch) not in _MODELS:
        gm = lnb.LlamaTransformer(device=0, **CFGS[hd]).fill_synthetic(SEED_M).finalize(LONG_CAP if hd == 128 else 0)
        if batch:
            gm.enable_batch()
        _MODELS[(hd, batch)] = gm
    return _MODELS[(hd, batch)]


def text(lnb, hd, k, n=64):
    """text k of a head_dim's vocabulary: k = 0 the shared prefix, 1.. the members' stale rows, 100.. the rows they append"""
    if (hd, k) not in _TOK:
        _TOK[(hd, k)] = lnb.synth_tokens(SEED_T + k, 8192 if k == 999 else 64, CFGS[hd]["vocab_size"])
    return _TOK[(hd, k)][:n]


def source(lnb, hd, batch):
    """per handle: a context of capacity 96 that holds 41 rows of text 0 (37 of them are shared by ForkPrefix)"""
    if (hd, batch) not in _SRC:
        c = lnb.InferenceContext(model(lnb, hd, batch), SRC_CAP)
        c.Forward(text(lnb, hd, 0, FILLED), 0, want_logits=False)
        _SRC[(hd, batch)] = c
    return _SRC[(hd, batch)]


def long_source(lnb, batch):
    """head_dim 128: a context of capacity 8192 filled to 7990 by chunked ForwardAppend (once per handle; members take its rows by ForkPrefix)"""
    if ("long", batch) not in _SRC:
        c = lnb.InferenceContext(model(lnb, 128, batch), LONG_CAP)
        t = text(lnb, 128, 999, LONG_FILL)
        for p in range(0, LONG_FILL, LONG_CHUNK):
            c.ForwardAppend(t[p:p + LONG_CHUNK], p, want_logits=False)
        _SRC[("long", batch)] = c
    return _SRC[("long", batch)]


def M(cap, k, start, rows, how="stale"):
    """a member: capacity, text id, start position, rows; how: 'stale' = it holds min(41, cap) rows of text k; 'fork' = those, then rows [0, 37) of the
    shared source; 'long' = the 7990 rows of the long source"""
    return (cap, k, start, rows, how)


def make_member(lnb, hd, batch, spec):
    cap, k, start, rows, how = spec
    c = lnb.InferenceContext(model(lnb, hd, batch), cap)
    if how == "long":
        long_source(lnb, batch).ForkPrefix([c], LONG_FILL)
        return c
    c.Forward(text(lnb, hd, k, min(FILLED, cap)), 0, want_logits=False)
    if how == "fork":
        source(lnb, hd, batch).ForkPrefix([c], NPOS)
    return c


def rows_of(lnb, hd, spec):
    return text(lnb, hd, 100 + spec[1], spec[3])


def caches(ctx, hd):
    return [(ctx.CacheK(l).copy(), ctx.CacheV(l).copy()) for l in range(CFGS[hd]["n_layers"])]


def reference(lnb, hd, spec):
    """once per (head_dim, member): logits, argmax and caches of a context in the member's state after ForwardAppend of its rows, and -- where the capacity
    allows 8 more positions -- the greedy continuation from that argmax (the caches are taken before it)"""
    if (hd, spec) not in _REF:
        cap, k, start, rows, how = spec
        c = make_member(lnb, hd, False, spec)
        lg, arg = c.ForwardAppend(rows_of(lnb, hd, spec), start)
        kv = caches(c, hd)
        gen = [int(t) for t in c.decode_greedy(arg, start + rows, STEPS)[0]] if start + rows + STEPS <= cap else None
        c.close()
        _REF[(hd, spec)] = dict(logits=lg, arg=arg, kv=kv, gen=gen)
    return _REF[(hd, spec)]


def run(lnb, hd, batch, specs, want_logits=True):
    """members in their states, ONE call, everything compared: -> the member contexts (the caller closes them)"""
    ctxs = [make_member(lnb, hd, batch, sp) for sp in specs]
    before = [caches(c, hd) for c in ctxs]
    lg, am = lnb.ForwardAppendMany(ctxs, [rows_of(lnb, hd, sp) for sp in specs], [sp[2] for sp in specs], want_logits=want_logits)
    for s, (sp, c) in enumerate(zip(specs, ctxs)):
        R, (cap, k, start, rows, how) = reference(lnb, hd, sp), sp
        tag = (hd, batch, s, sp)
        if want_logits:
            assert lg[s].shape == R["logits"].shape and np.array_equal(bits(lg[s]), bits(R["logits"])), tag
        assert int(am[s]) == R["arg"], tag
        for l, (kk, vv) in enumerate(caches(c, hd)):
            assert np.array_equal(kk[start:start + rows], R["kv"][l][0][start:start + rows]) and np.array_equal(vv[start:start + rows], R["kv"][l][1][start:start + rows]), (tag, l, "new rows")
            assert np.array_equal(kk[:start], before[s][l][0][:start]) and np.array_equal(vv[:start], before[s][l][1][:start]), (tag, l, "rows below start")
            assert np.array_equal(kk[start + rows:], before[s][l][0][start + rows:]) and np.array_equal(vv[start + rows:], before[s][l][1][start + rows:]), (tag, l, "rows behind the append")
            assert np.array_equal(kk, R["kv"][l][0]) and np.array_equal(vv, R["kv"][l][1]), (tag, l, "whole cache")
    return ctxs


def close(ctxs):
    for c in ctxs:
        c.close()


# rows (1, 5, 7) at (0, 37, 20), capacities (64, 96, 300); the 37 comes from ForkPrefix out of the capacity-96 source
CASE1 = (M(64, 1, 0, 1), M(96, 2, NPOS, 5, "fork"), M(300, 3, 20, 7))
# 17..32 columns: rows (3, 9, 1, 6, 8) = 27; every capacity leaves room for 8 greedy steps behind the append
CASE2 = (M(64, 4, 41, 3), M(96, 5, NPOS, 9, "fork"), M(300, 6, 0, 1), M(128, 7, 12, 6), M(64, 8, 33, 8))
# 33..128 columns, no multiple of 16: 83 rows; the first member's 40 rows at position 0 run the matrix-core attention in the reference
CASE3 = (M(64, 9, 0, 40), M(96, 10, NPOS, 3, "fork"), M(300, 11, 20, 11), M(64, 12, 41, 7), M(128, 13, 5, 9), M(41, 14, 40, 1), M(200, 15, 30, 12))
# more than one pass at the default width: 6 x 30 = 180 rows, the fifth member's rows 120..149 straddle the boundary at 128
CASE4 = (M(64, 16, 0, 30), M(96, 17, NPOS, 30, "fork"), M(300, 18, 20, 30), M(128, 19, 41, 30), M(64, 20, 10, 30), M(41, 21, 0, 30))
# the long form: 6 rows at 7990 of a capacity-8192 member beside two short members
CASE6 = (M(96, 22, NPOS, 5, "fork"), M(LONG_CAP, 999, LONG_FILL, 6, "long"), M(64, 23, 20, 7))


@pytest.mark.parametrize("batch", [False, True], ids=["rows", "columns"])
@pytest.mark.parametrize("hd", HDS)
def test_up_to_16_columns(lnb, hd, batch, monkeypatch):
    monkeypatch.delenv("LNB_APPEND_MANY_COLS", raising=False)
    close(run(lnb, hd, batch, CASE1))
    assert model(lnb, hd, batch).append_many_info() == {"passes": 1, "max_columns": 13, "long_passes": 0}


def test_up_to_16_columns_against_the_cpu_oracle(lnb):
    """head_dim 64: the reference's own logits against the oracle's one-token steps in the same three states"""
    hd = 64
    om = orc.Model(**CFGS[hd]).fill_synthetic(SEED_M).finalize()
    for sp in CASE1:
        cap, k, start, rows, how = sp
        oc = orc.Context(om, 64)
        below = text(lnb, hd, 0 if how == "fork" else k, start)
        if start:
            oc.forward(below, 0, want_logits=False)
        new = rows_of(lnb, hd, sp)
        olg = np.stack([oc.forward(new[i:i + 1], start + i)[0][0].copy() for i in range(rows)])
        oc.close()
        assert np.array_equal(bits(reference(lnb, hd, sp)["logits"]), bits(olg)), sp
    om.close()


@pytest.mark.parametrize("batch", [False, True], ids=["rows", "groups"])
@pytest.mark.parametrize("hd", HDS)
def test_17_to_32_columns_and_the_continuation(lnb, hd, batch, monkeypatch):
    """27 columns; then every member goes on: a Batch over the members for 8 steps, and each member's own greedy loop, both equal to the reference's"""
    monkeypatch.delenv("LNB_APPEND_MANY_COLS", raising=False)
    ctxs = run(lnb, hd, batch, CASE2)
    refs = [reference(lnb, hd, sp) for sp in CASE2]
    ends = [sp[2] + sp[3] for sp in CASE2]
    bat = lnb.Batch(ctxs)
    got, _ = bat.decode([r["arg"] for r in refs], ends, STEPS)
    bat.close()
    for s, r in enumerate(refs):
        assert r["gen"] is not None and [int(t) for t in got[s]] == r["gen"], (hd, batch, s, "batch")
        assert [int(t) for t in ctxs[s].decode_greedy(r["arg"], ends[s], STEPS)[0]] == r["gen"], (hd, batch, s, "greedy")
    close(ctxs)


@pytest.mark.parametrize("batch", [False, True], ids=["rows", "rows-m16"])
@pytest.mark.parametrize("hd", HDS)
def test_33_to_128_columns(lnb, hd, batch, monkeypatch):
    monkeypatch.delenv("LNB_APPEND_MANY_COLS", raising=False)
    close(run(lnb, hd, batch, CASE3))
    assert model(lnb, hd, batch).append_many_info() == {"passes": 1, "max_columns": 83, "long_passes": 0}


@pytest.mark.parametrize("batch", [False, True], ids=["rows", "columns"])
@pytest.mark.parametrize("hd", HDS)
def test_a_member_straddles_two_passes_at_the_default_width(lnb, hd, batch, monkeypatch):
    monkeypatch.delenv("LNB_APPEND_MANY_COLS", raising=False)
    close(run(lnb, hd, batch, CASE4))
    assert model(lnb, hd, batch).append_many_info() == {"passes": 2, "max_columns": 128, "long_passes": 0}


@pytest.mark.parametrize("W", [5, 16, 17])
@pytest.mark.parametrize("batch", [False, True], ids=["rows", "columns"])
@pytest.mark.parametrize("hd", HDS)
def test_pass_widths_from_the_knob(lnb, hd, batch, W, monkeypatch):
    monkeypatch.setenv("LNB_APPEND_MANY_COLS", str(W))
    close(run(lnb, hd, batch, CASE1))
    assert model(lnb, hd, batch).append_many_info() == {"passes": -(-13 // W), "max_columns": min(13, W), "long_passes": 0}


@pytest.mark.parametrize("W", [0, 129])
def test_a_width_outside_1_to_128_is_refused_with_the_knobs_name(lnb, W, monkeypatch):
    hd = 64
    ctxs = [make_member(lnb, hd, False, sp) for sp in CASE1]
    before = [caches(c, hd) for c in ctxs]
    monkeypatch.setenv("LNB_APPEND_MANY_COLS", str(W))
    with pytest.raises(lnb.LnbError, match="LNB_APPEND_MANY_COLS"):
        lnb.ForwardAppendMany(ctxs, [rows_of(lnb, hd, sp) for sp in CASE1], [sp[2] for sp in CASE1])
    for c, b in zip(ctxs, before):
        assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(caches(c, hd), b))
    close(ctxs)


@pytest.mark.parametrize("batch", [False, True], ids=["rows", "columns"])
@pytest.mark.parametrize("hd", HDS)
def test_narrow_after_wide_on_one_handle(lnb, hd, batch, monkeypatch):
    """83 columns, then 13, then 1 on the same buffers: what the wide pass left in the columns the narrow one does not use must not reach it"""
    monkeypatch.delenv("LNB_APPEND_MANY_COLS", raising=False)
    close(run(lnb, hd, batch, CASE3))
    close(run(lnb, hd, batch, CASE1))
    close(run(lnb, hd, batch, CASE1[:1]))
    close(run(lnb, hd, batch, CASE2, want_logits=False))      # and wider again, column groups, without the logits copy
    assert model(lnb, hd, batch).append_many_info() == {"passes": 1, "max_columns": 27, "long_passes": 0}


@pytest.mark.parametrize("batch", [False, True], ids=["rows", "groups"])
def test_long_form_beside_short_members(lnb, batch, monkeypatch):
    monkeypatch.delenv("LNB_APPEND_MANY_COLS", raising=False)
    close(run(lnb, 128, batch, CASE6))
    info = model(lnb, 128, batch).append_many_info()
    assert info == {"passes": 1, "max_columns": 18, "long_passes": 1} and info["long_passes"] == info["passes"]


def test_refusals_leave_every_cache_byte_unchanged(lnb, monkeypatch):
    monkeypatch.delenv("LNB_APPEND_MANY_COLS", raising=False)
    hd = 64
    ctxs = [make_member(lnb, hd, False, sp) for sp in CASE1]
    alien = make_member(lnb, hd, True, CASE1[0])             # the same weights behind ANOTHER model handle
    fast = make_member(lnb, hd, False, CASE1[0]).set_mode("fast")
    everyone = ctxs + [alien, fast]
    before = [caches(c, hd) for c in everyone]
    toks = [rows_of(lnb, hd, sp) for sp in CASE1]
    pos = [sp[2] for sp in CASE1]

    def refused(members, tokens, starts, *words):
        with pytest.raises(lnb.LnbError) as e:
            lnb.ForwardAppendMany(members, tokens, starts)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        for c, b in zip(everyone, before):
            assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(caches(c, hd), b)), words

    refused([ctxs[0], ctxs[1], ctxs[0]], toks, pos, "appears twice")
    refused([ctxs[0], alien, ctxs[2]], toks, pos, "another lnb_model handle")
    refused(ctxs, toks, [0, 96 - 4, 20], "member 1", "beyond the KV cache of 96")
    refused([ctxs[0], fast, ctxs[2]], toks, pos, "context 1", "tolerance mode")
    bad = [t.copy() for t in toks]
    bad[2][3] = CFGS[hd]["vocab_size"]
    refused(ctxs, bad, pos, "row 9", "outside the vocabulary")          # rows 0 | 1..5 | 6..12: member 2's fourth row is row 9 of the call
    bad[2][3] = -1
    refused(ctxs, bad, pos, "row 9", "outside the vocabulary")
    close(everyone)
