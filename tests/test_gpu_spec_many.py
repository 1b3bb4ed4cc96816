"""Speculative decoding of many contexts (-m gpu): lnb_decode_speculative_many against every member's own lnb_decode_greedy_until, bit for bit.
Models: oracle.TINY (head_dim 64; also against the CPU oracle's generate) and the head-geometry variants of tests/test_gpu_prefix_fork.py (head_dim 128
with one KV head, head_dim 32 with two of eight heads); model seed 909.  Every model exists twice with the same weights -- without and with
enable_batch() -- so a pass runs as rows of the streaming product on one handle and as matrix-core columns / column groups on the other.
Member k has a prompt of PROMPT_LEN[k] tokens (so positions differ); the reference for it is a fresh context of its capacity on the handle without the
copy: Forward of the prompt, decode_greedy_until from the first token.  References are computed once per (head_dim, member, capacity, stop ids) and
never changed.  The counters are compared with a Python restatement of the documented rule (ref_draft / simulate of tests/test_gpu_speculative.py,
extended to members and grants) over the known outputs."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

CFGS = {
    128: dict(orc.TINY, n_heads=2, n_kv_heads=1),
    64: dict(orc.TINY),
    32: dict(orc.TINY, n_heads=8, n_kv_heads=2),
}
SEED_M, SEED_T = 909, 8800
PROMPT_LEN = (8, 11, 5, 9, 6, 7, 10, 4, 12)
N, CAP, LONG_CAP = 40, 64, 8192
NMIN, NMAX = 1, 4


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


_MODELS, _REF, _ORC = {}, {}, {}


def model(lnb, hd, batch):
    if (hd, batch) not in _MODELS:
        gm = lnb.LlamaTransformer(device=0, **CFGS[hd]).fill_synthetic(SEED_M).finalize(LONG_CAP if hd == 128 else 0)
        if batch:
            gm.enable_batch()
        _MODELS[(hd, batch)] = gm
    return _MODELS[(hd, batch)]


def prompt(lnb, hd, k):
    return lnb.synth_tokens(SEED_T + k, PROMPT_LEN[k], CFGS[hd]["vocab_size"])


def caches(ctx, hd):
    return [(ctx.CacheK(l).copy(), ctx.CacheV(l).copy()) for l in range(CFGS[hd]["n_layers"])]


def same(a, b, rows=None):
    return all(np.array_equal(x[0][:rows], y[0][:rows]) and np.array_equal(x[1][:rows], y[1][:rows]) for x, y in zip(a, b))


def reference(lnb, hd, k, cap=CAP, stop=(), n=N):
    """member k alone: first token of its prompt, its greedy tokens (n of them unless a stop id ends the run), finished flag, caches afterwards"""
    key = (hd, k, cap, tuple(stop), n)
    if key not in _REF:
        c = lnb.InferenceContext(model(lnb, hd, False), cap)
        if stop:
            c.set_stop_ids(list(stop))
        p = prompt(lnb, hd, k)
        _, first = c.Forward(p, 0, want_logits=False)
        out, fin, _ = c.decode_greedy_until(first, len(p), n)
        _REF[key] = dict(prompt=p, first=int(first), out=np.array(out, dtype=np.int32), fin=bool(fin), kv=caches(c, hd), P=len(p))
        c.close()
    return _REF[key]


def oracle_tokens(lnb, k, n=N + 8):
    """head_dim 64: the CPU oracle's first token + n generated tokens for member k's prompt"""
    if k not in _ORC:
        om = orc.Model(**CFGS[64]).fill_synthetic(SEED_M).finalize()
        ref, _ = orc.Context(om, CAP).generate(prompt(lnb, 64, k), n + 1)
        om.close()
        _ORC[k] = [int(t) for t in ref]
    return _ORC[k]


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------------------
def ref_draft(R, C, nmin, nmax, max_draft):
    """longest n first; an earlier occurrence of R's last n tokens followed by at least one token of its array; R before C; latest start"""
    R, C = [int(t) for t in R], [int(t) for t in C]
    L = len(R)
    for n in range(nmax, nmin - 1, -1):
        if n > L:
            continue
        suf = R[L - n:]
        for arr in (R, C):
            for j in range(len(arr) - n - 1, -1, -1):
                if arr[j:j + n] == suf:
                    return arr[j + n:j + n + max_draft]
    return []


def simulate(members, budget, max_steps, short_cap=None, ends=None):
    """the passes of lnb_decode_speculative_many over its known outputs.  members: dicts with history, token, out (what the member's greedy loop
    emits in this call), corpus, md, seq_len, start (None: skipped) -> (per-member stats, info).  ends (a dict, optional) receives, per member, the
    pass in which its last token was emitted: col = the column of the member that emitted it, cols = the member's columns, a = the accepted drafts
    of that pass, draft = the granted draft"""
    n = len(members)
    budget = budget or 16 * -(-n // 16)
    g = [0] * n
    stats = [dict(passes=0, verify_passes=0, drafted=0, accepted=0) for _ in range(n)]
    info = dict(passes=0, verify_passes=0, columns=0, max_columns=0, long_passes=0)
    while True:
        A = [s for s in range(n) if members[s]["start"] is not None and g[s] < len(members[s]["out"])]
        if not A:
            break
        want = {}
        for s in A:
            m = members[s]
            out = [int(t) for t in m["out"]]
            R = [int(t) for t in m["history"]] + [int(m["token"])] + out[:g[s]]
            lim = min(max_steps - g[s] - 1, m["seq_len"] - (m["start"] + g[s]) - 1)
            want[s] = ref_draft(R, m["corpus"], NMIN, NMAX, m["md"])[:max(lim, 0)] if m["md"] > 0 else []
        cols = {s: 1 for s in A}
        left = budget - len(A)
        for j in range(1, 16):
            for s in A:
                if len(want[s]) >= j and left > 0:
                    cols[s] += 1
                    left -= 1
        width = sum(cols.values())
        info["passes"] += 1
        info["verify_passes"] += 1 if any(c > 1 for c in cols.values()) else 0
        info["columns"] += width
        info["max_columns"] = max(info["max_columns"], width)
        if short_cap is not None and any(members[s]["seq_len"] > short_cap for s in A):
            info["long_passes"] += 1
        for s in A:
            out = [int(t) for t in members[s]["out"]]
            d = want[s][:cols[s] - 1]
            st = stats[s]
            st["passes"] += 1
            st["verify_passes"] += 1 if d else 0
            st["drafted"] += len(d)
            a = 0
            while a < len(d) and g[s] + a < len(out) and d[a] == out[g[s] + a]:
                a += 1
            e = min(a + 1, len(out) - g[s])
            g[s] += e
            if ends is not None and g[s] == len(out):
                ends[s] = dict(col=e - 1, cols=cols[s], a=a, draft=d)
    for s in range(n):
        stats[s]["accepted"] = len(members[s]["out"]) - stats[s]["passes"] if members[s]["start"] is not None else 0
    return stats, info


def corpus_of(kind, R, V):
    """the member's reference continuation (first token + generated), uncorrupted / every 2nd / every 5th token corrupted / empty"""
    if kind == "none":
        return []
    c = np.concatenate([[R["first"]], R["out"]]).astype(np.int32)
    m = {"exact": 0, "every2": 2, "every5": 5}[kind]
    if m:
        c[m - 1::m] = (c[m - 1::m] + 1) % V
    return c


def start_members(lnb, hd, batch, ks, mds, kinds, caps=None, stops=None, n=N):
    """fresh contexts holding their prompts, with draft settings -> (contexts, references of an n-step call, simulation members)"""
    ctxs, refs, sims = [], [], []
    for i, k in enumerate(ks):
        cap = caps[i] if caps else CAP
        stop = stops[i] if stops else ()
        R = reference(lnb, hd, k, cap, stop, n)
        c = lnb.InferenceContext(model(lnb, hd, batch), cap)
        if stop:
            c.set_stop_ids(list(stop))
        _, first = c.Forward(R["prompt"], 0, want_logits=False)
        assert int(first) == R["first"]
        C = kinds[i] if not isinstance(kinds[i], str) else corpus_of(kinds[i], reference(lnb, hd, k), CFGS[hd]["vocab_size"])
        c.set_draft(mds[i], NMIN, NMAX, C)
        ctxs.append(c); refs.append(R)
        sims.append(dict(history=R["prompt"], token=R["first"], out=R["out"], corpus=C, md=mds[i], seq_len=cap, start=R["P"]))
    return ctxs, refs, sims


def run_and_check(lnb, hd, batch, ks, mds, kinds, budget, max_steps=N, caps=None, stops=None, short_cap=None):
    """one call over fresh members; tokens, n_generated, finished, the KV rows [0, start + n_generated) of every layer, stats and info"""
    ctxs, refs, sims = start_members(lnb, hd, batch, ks, mds, kinds, caps, stops, max_steps)
    toks, fins, stats, info, _ = lnb.DecodeSpeculativeMany(ctxs, [r["prompt"] for r in refs], [r["first"] for r in refs], [r["P"] for r in refs], max_steps, budget)
    tag = (hd, batch, ks, mds, budget)
    for s, (c, R) in enumerate(zip(ctxs, refs)):
        assert np.array_equal(toks[s], R["out"]) and fins[s] == R["fin"], (tag, s, list(toks[s]), list(R["out"]))
        assert same(caches(c, hd), R["kv"], R["P"] + len(R["out"])), (tag, s, "KV rows")
    want_stats, want_info = simulate(sims, budget, max_steps, short_cap)
    if short_cap is None:
        want_info["long_passes"] = info["long_passes"]
    assert stats == want_stats, (tag, stats, want_stats)
    assert info == want_info, (tag, info, want_info)
    return ctxs, refs, stats, info


def close(ctxs):
    for c in ctxs:
        c.close()


FORMS = pytest.mark.parametrize("batch", [False, True], ids=["rows", "columns"])
MDS = {"exact": (3, 0, 15), "every2": (7, 1, 0), "every5": (0, 15, 3), "none": (1, 7, 15)}


# ---- 1. three members, every corpus kind, every budget -------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("kind", ["exact", "every2", "every5", "none"])
def test_three_members_equal_their_greedy_runs(lnb, batch, kind):
    hd, ks = 64, (0, 1, 2)
    for k in ks:                                              # the reference itself against the CPU oracle
        R = reference(lnb, hd, k)
        assert [R["first"]] + [int(t) for t in R["out"]] == oracle_tokens(lnb, k)[:N + 1]
    for budget in (0, 3, 5, 128):                             # the default (16), n (no drafts possible), 5 (the budget binds: levels matter), 128
        ctxs, refs, stats, info = run_and_check(lnb, hd, batch, ks, MDS[kind], (kind,) * 3, budget)
        assert info["long_passes"] == 0
        if budget == 3:
            assert info["verify_passes"] == 0 and info["passes"] == N and all(st["drafted"] == 0 for st in stats)
        elif kind == "exact":                                 # follows from the rule: the first pass drafts the true continuation
            assert all(st["accepted"] > 0 for st, md in zip(stats, MDS[kind]) if md > 0)
        close(ctxs)


@FORMS
@pytest.mark.parametrize("hd", [128, 32])
def test_the_other_head_geometries(lnb, hd, batch):
    for budget in (0, 5):
        ctxs, _, stats, _ = run_and_check(lnb, hd, batch, (0, 1, 2), MDS["exact"], ("exact",) * 3, budget)
        assert all(st["accepted"] > 0 for st, md in zip(stats, MDS["exact"]) if md > 0)
        close(ctxs)


# ---- 2. widths beyond one tile ---------------------------------------------------------------------------------------------------------------
@FORMS
def test_widths_beyond_one_tile(lnb, batch):
    hd = 64
    # 5 members x max_draft 7 want 5 x 8 = 40 columns: budget 32 keeps the passes in 17..32 (column groups with the copy), budget 40 lets them have all
    ctxs, _, _, info = run_and_check(lnb, hd, batch, (0, 1, 2, 3, 4), (7,) * 5, ("exact",) * 5, 32)
    assert 17 <= info["max_columns"] <= 32, info
    close(ctxs)
    ctxs, _, _, info = run_and_check(lnb, hd, batch, (0, 1, 2, 3, 4), (7,) * 5, ("exact",) * 5, 40)
    assert info["max_columns"] == 40, info
    close(ctxs)
    # 9 members x max_draft 15 want 144: the rows form at 33..128
    ctxs, _, _, info = run_and_check(lnb, hd, batch, tuple(range(9)), (15,) * 9, ("exact",) * 9, 128)
    assert 33 <= info["max_columns"] <= 128, info
    close(ctxs)
    # and narrow again on the same buffers: what the wide passes left in the dead columns must not reach these
    ctxs, _, _, info = run_and_check(lnb, hd, batch, (0, 1, 2), MDS["every5"], ("every5",) * 3, 0)
    assert info["max_columns"] <= 16
    close(ctxs)


# ---- 3. stop ids -----------------------------------------------------------------------------------------------------------------------------
@FORMS
def test_stop_ids_on_an_accepted_draft_and_on_the_bonus_token(lnb, batch):
    hd, ks, V = 64, (0, 1, 2, 3), CFGS[64]["vocab_size"]
    plain = [reference(lnb, hd, k) for k in ks]

    # Which column emits a stop token follows from the rule alone, so the stop positions are CHOSEN by the restated rule: the first pair for which
    # member 0's stop token is an accepted draft (emitted by a column that is not its last, the next column carrying it as input) and member 1's is
    # the bonus token (emitted by the column whose draft was wrong: the corpus is corrupted exactly there).
    steps, mds = 24, (7, 7, 3, 15)

    def plan(ja, jb):
        sa, sb = int(plain[0]["out"][ja]), int(plain[1]["out"][jb])
        Cb = corpus_of("exact", plain[1], V)
        Cb[1 + jb] = (Cb[1 + jb] + 1) % V                     # wrong exactly at the stop token
        kinds = ("exact", Cb, "exact", "every2")
        outs = (plain[0]["out"][:ja + 1], plain[1]["out"][:jb + 1], plain[2]["out"][:steps], plain[3]["out"][:steps])
        sims = [dict(history=plain[s]["prompt"], token=plain[s]["first"], out=outs[s], corpus=kinds[s] if s == 1 else corpus_of(kinds[s], plain[s], V),
                     md=mds[s], seq_len=CAP, start=plain[s]["P"]) for s in range(4)]
        ends = {}
        simulate(sims, 0, steps, ends=ends)
        return sa, sb, kinds, ends

    def fresh(R, j):                                          # a token that does not occur before: the greedy run ends exactly there
        out = [int(t) for t in R["out"]]
        return out[j] not in out[:j] and out[j] != R["first"]

    def as_wanted(sa, sb, ends):
        e0, e1 = ends[0], ends[1]
        accepted = e0["col"] < e0["a"] and e0["draft"][e0["col"]] == sa                   # column col + 1 carried the stop token as its input and was accepted
        bonus = e1["col"] == e1["a"] < len(e1["draft"]) and e1["draft"][e1["a"]] != sb    # column a + 1 carried a wrong draft: column a's argmax is the bonus token
        return accepted and bonus

    pairs = [(ja, jb) for ja in range(6, steps - 2) for jb in range(8, steps - 2) if fresh(plain[0], ja) and fresh(plain[1], jb)]

    def wanted(p):
        sa, sb, _, ends = plan(*p)
        return as_wanted(sa, sb, ends)

    ja, jb = next((p for p in pairs if wanted(p)), (None, None))
    assert ja is not None, "no pair of stop positions puts one stop on an accepted draft and the other on the bonus token"
    sa, sb, kinds, ends = plan(ja, jb)
    stops = ((sa,), (sb,), (), ())
    assert ends[0]["col"] < ends[0]["a"] <= ends[0]["cols"] - 1 and ends[0]["draft"][ends[0]["col"]] == sa          # an inner column emitted member 0's stop
    assert ends[1]["col"] == ends[1]["a"] < ends[1]["cols"] - 1 and ends[1]["draft"][ends[1]["a"]] != sb            # the column before the wrong one emitted member 1's
    ctxs, refs, stats, info = run_and_check(lnb, hd, batch, ks, mds, kinds, 0, max_steps=steps, stops=stops)
    assert refs[0]["fin"] and len(refs[0]["out"]) == ja + 1 and refs[1]["fin"] and len(refs[1]["out"]) == jb + 1
    assert not refs[2]["fin"] and len(refs[2]["out"]) == steps
    assert stats[0]["passes"] < info["passes"] and stats[1]["passes"] < info["passes"]      # the others ran on in narrower passes
    # a second, chunked call: the finished members stay frozen, the others continue
    before = [caches(c, hd) for c in ctxs]
    pos = [-1, -1, refs[2]["P"] + steps, refs[3]["P"] + steps]
    tok = [sa, sb, int(refs[2]["out"][-1]), int(refs[3]["out"][-1])]
    hist = [np.concatenate([r["prompt"], [r["first"]], r["out"][:-1]]) for r in refs]
    toks, fins, st2, info2, _ = lnb.DecodeSpeculativeMany(ctxs, hist, tok, pos, N - steps, 0)
    assert [len(t) for t in toks[:2]] == [0, 0] and fins[:2] == [True, True] and st2[0] == st2[1] == dict(passes=0, verify_passes=0, drafted=0, accepted=0)
    assert same(caches(ctxs[0], hd), before[0]) and same(caches(ctxs[1], hd), before[1])
    for s in (2, 3):
        assert np.array_equal(toks[s], plain[s]["out"][steps:]) and not fins[s], s
        assert same(caches(ctxs[s], hd), plain[s]["kv"], plain[s]["P"] + N), s
    sims = [dict(history=hist[s], token=tok[s], out=toks[s], corpus=[] if s < 2 else corpus_of(kinds[s], plain[s], V), md=mds[s], seq_len=CAP,
                 start=None if s < 2 else pos[s]) for s in range(4)]
    assert (st2, info2) == simulate(sims, 0, N - steps, short_cap=10 ** 9)
    # the finished member's position and log are its greedy run's: its greedy loop goes on from the stop token as the unstopped run does
    ctxs[0].set_stop_ids([])
    more, _ = ctxs[0].decode_greedy(sa, plain[0]["P"] + ja + 1, 4)
    assert [int(t) for t in more] == [int(t) for t in plain[0]["out"][ja + 1:ja + 5]]
    close(ctxs)


# ---- 4. limits -------------------------------------------------------------------------------------------------------------------------------
@FORMS
def test_a_member_whose_cache_ends_at_the_last_step(lnb, batch):
    hd, steps = 64, 20
    for extra in (0, 1):                                      # seq_len == start_pos + max_steps (+ 1) beside a roomy member
        cap = PROMPT_LEN[0] + steps + extra
        ctxs, _, _, _ = run_and_check(lnb, hd, batch, (0, 1), (15, 15), ("exact", "exact"), 0, max_steps=steps, caps=(cap, CAP))
        close(ctxs)


# ---- 5. the long-context pair -----------------------------------------------------------------------------------------------------------------
@FORMS
def test_a_member_beyond_the_one_workgroup_kernels_beside_short_members(lnb, batch):
    """capacity alone selects the form: the long member holds a few positions only"""
    hd, steps = 128, 12
    short_cap = LONG_CAP - 1                                  # (the simulation only has to tell the members apart: any value in [CAP, LONG_CAP))
    # the long member never drafts, so it needs every one of the 12 passes: no pass is without it
    caps = (CAP, LONG_CAP, CAP)
    ctxs, _, _, info = run_and_check(lnb, hd, batch, (0, 1, 2), (7, 0, 15), ("exact",) * 3, 0, max_steps=steps, caps=caps, short_cap=short_cap)
    assert info["passes"] == steps and info["long_passes"] == info["passes"], info
    close(ctxs)
    # the long member drafts (its columns 1.. run the pair as well) beside members that do not: the passes after it has finished are short ones
    ctxs, _, stats, info = run_and_check(lnb, hd, batch, (0, 1, 2), (0, 15, 0), ("exact",) * 3, 0, max_steps=steps, caps=caps, short_cap=short_cap)
    assert stats[1]["accepted"] > 0 and info["long_passes"] == stats[1]["passes"] < info["passes"] == steps, (stats, info)
    close(ctxs)


# ---- 6. continuation -------------------------------------------------------------------------------------------------------------------------
@FORMS
def test_every_entry_point_continues_the_members(lnb, batch):
    hd, ks, steps = 64, (0, 1, 2), 20
    ctxs, refs, _, _ = run_and_check(lnb, hd, batch, ks, (7, 0, 15), ("every5",) * 3, 0, max_steps=steps)
    orc_t = [oracle_tokens(lnb, k) for k in ks]               # [first, g_0, g_1, ...]: g_i is generated at position P + i
    pos = [r["P"] + steps for r in refs]
    nxt = [t[steps] for t in orc_t]                           # the last token generated = the next input
    assert [int(r["out"][-1]) for r in refs] == nxt
    a, _ = ctxs[0].decode_greedy(nxt[0], pos[0], 3)
    assert [int(t) for t in a] == orc_t[0][steps + 1:steps + 4]
    pos[0] += 3; nxt[0] = int(a[-1])
    _, f = ctxs[1].Forward([nxt[1]], pos[1], want_logits=False)
    assert f == orc_t[1][steps + 1]
    pos[1] += 1; nxt[1] = f
    _, am = lnb.ForwardAppendMany(ctxs, [[t] for t in nxt], pos, want_logits=False)
    done = [p - r["P"] for p, r in zip(pos, refs)]
    assert [int(t) for t in am] == [orc_t[s][done[s] + 1] for s in range(3)]
    pos = [p + 1 for p in pos]; nxt = [int(t) for t in am]
    bat = lnb.Batch(ctxs)
    got, _ = bat.decode(nxt, pos, 3)
    bat.close()
    for s in range(3):
        d = pos[s] - refs[s]["P"]
        assert [int(t) for t in got[s]] == orc_t[s][d + 1:d + 4], s
    # and the call itself again, from where the batch left the members
    pos = [p + 3 for p in pos]; nxt = [int(got[s][-1]) for s in range(3)]
    hist = [orc_t[s][:0] for s in range(3)]
    toks, _, _, _, _ = lnb.DecodeSpeculativeMany(ctxs, hist, nxt, pos, 4, 0)
    for s in range(3):
        d = pos[s] - refs[s]["P"]
        assert [int(t) for t in toks[s]] == orc_t[s][d + 1:d + 5], s
    close(ctxs)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_handle_level_refusals_leave_every_cache_byte_unchanged(lnb):
    hd, ks = 64, (0, 1, 2)
    ctxs, refs, _ = start_members(lnb, hd, False, ks, (3, 7, 15), ("exact",) * 3)
    alien, _, _ = start_members(lnb, hd, True, (0,), (3,), ("exact",))                  # the same weights behind ANOTHER model handle
    fast, _, _ = start_members(lnb, hd, False, (0,), (3,), ("exact",))
    probs, _, _ = start_members(lnb, hd, False, (0,), (3,), ("exact",))
    live, _, _ = start_members(lnb, hd, False, (0, 1), (3, 3), ("exact",) * 2)
    fast[0].set_mode("fast"); probs[0].set_token_probs(4)
    bat = lnb.Batch(live)
    stage = lnb.LlamaTransformer(device=0, layer_begin=0, layer_end=1, **CFGS[hd]).fill_synthetic(SEED_M).finalize()
    sc = [lnb.InferenceContext(stage, CAP) for _ in range(3)]
    # a model whose RoPE table ends at 64 rows under contexts of capacity 128, and one whose dim is no multiple of 128 (its contexts stay empty)
    short_rope = lnb.LlamaTransformer(device=0, **CFGS[hd]).fill_synthetic(SEED_M).finalize(64)
    rope = [lnb.InferenceContext(short_rope, 128) for _ in range(3)]
    for c, r in zip(rope, refs):
        c.Forward(r["prompt"], 0, want_logits=False)
    odd = lnb.LlamaTransformer(device=0, **dict(CFGS[hd], dim=192, n_heads=3, n_kv_heads=3)).fill_synthetic(SEED_M).finalize()
    oddc = [lnb.InferenceContext(odd, CAP) for _ in range(3)]
    # a member with a lnb_forward_stage_begin that has not been ended: a stand-in (its caches are being written, so it is not among the compared)
    pend = lnb.InferenceContext(model(lnb, hd, False), CAP)
    everyone = ctxs + alien + fast + probs + live + rope + oddc
    before = [caches(c, hd) for c in everyone]
    hist = [r["prompt"] for r in refs]; tok = [r["first"] for r in refs]; pos = [r["P"] for r in refs]

    def refused(members, *words, tokens=tok, starts=pos, steps=N, budget=0):
        with pytest.raises(lnb.LnbError) as e:
            lnb.DecodeSpeculativeMany(members, hist, tokens, starts, steps, budget)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        for c, b in zip(everyone, before):
            assert same(caches(c, hd), b), words

    refused([ctxs[0], ctxs[1], ctxs[0]], "appears twice")
    refused([ctxs[0], alien[0], ctxs[2]], "another lnb_model handle")
    refused(sc, "whole-model handle")
    refused([ctxs[0], fast[0], ctxs[2]], "context 1", "tolerance mode")
    refused([ctxs[0], ctxs[1], probs[0]], "context 2", "token probabilities")
    refused([live[0], ctxs[1], ctxs[2]], "context 0", "live batch")
    refused(ctxs, "member 1", "outside the vocabulary", tokens=[tok[0], CFGS[hd]["vocab_size"], tok[2]])
    refused(ctxs, "member 2", "outside the vocabulary", tokens=[tok[0], tok[1], -1])
    refused(ctxs, "member 1", "beyond the KV cache of 64", starts=[pos[0], CAP - N + 1, pos[2]])
    refused(ctxs, "max_steps", "token log", steps=CAP + 1)
    refused(ctxs, "col_budget", budget=2)
    refused(ctxs, "col_budget", budget=129)
    refused(rope, "member 0", "beyond the 64-row RoPE table", steps=60)           # 8 + 60 positions: inside the cache of 128 and the log, beyond the table
    refused(oddc, "multiples of 128")
    L = lnb.lib()
    ptoks = np.ascontiguousarray(refs[1]["prompt"], dtype=np.int32)
    lnb._chk(L.lnb_forward_stage_begin(pend.h, lnb._p(ptoks), int(ptoks.size), 0, 1))
    refused([ctxs[0], pend, ctxs[2]], "context 1", "lnb_forward_stage_begin")
    lnb._chk(L.lnb_forward_stage_end(pend.h, C.byref(C.c_int32(0))))
    bat.close()
    # nothing above left anything behind: the call runs
    toks, _, _, _, _ = lnb.DecodeSpeculativeMany(ctxs, hist, tok, pos, N, 0)
    assert all(np.array_equal(toks[s], refs[s]["out"]) for s in range(3))
    close(everyone + sc + [pend])
    stage.close(); short_rope.close(); odd.close()
