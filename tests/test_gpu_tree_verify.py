"""A tree of n-gram drafts per verify pass on the MI355X (include/lnb.h, lnb_ctx_set_draft_branches; csrc/lnb_tree_verify.h).  Whatever the tree, the
tokens, the finished flag and every KV row must be the one-token loop's, with == on the bits; the draft kernel and the pass counts must follow the rule
restated in tests/test_tree_draft_cpu.py."""
import numpy as np
import pytest

from oracle import oracle as orc
from form_tally import count, ran
import kv_craft
from test_tree_draft_cpu import CASES, ref_tree, simulate

pytestmark = pytest.mark.gpu

GEO = {(64, 1): dict(n_heads=4, n_kv_heads=4), (64, 4): dict(n_heads=4, n_kv_heads=1), (128, 1): dict(n_heads=2, n_kv_heads=2),
       (128, 4): dict(dim=512, n_heads=4, n_kv_heads=1)}
N, SEP = 24, 3
seq_of = lambda start: 64 if start <= 40 else start + 32       # the contexts' capacity


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


@pytest.fixture(scope="module")
def models(lnb):
    made = {}

    def get(key, cfg=None):
        if key not in made:
            c = cfg or dict(orc.TINY, **GEO[key])
            made[key] = (lnb.LlamaTransformer(device=0, **c).fill_synthetic(1234).finalize().enable_batch(), c)
        return made[key]
    yield get
    for gm, _ in made.values():
        gm.close()


def _kv(ctx, cfg, rows):
    return [a[:rows].copy() for l in range(cfg["n_layers"]) for a in (ctx.CacheK(l), ctx.CacheV(l))]


def _same(a, b):
    return all((x == y).all() for x, y in zip(a, b))


def two_occurrences(R0, want, V, k=6):
    """for every step g the two tokens in front of want[g] twice: the EARLIER occurrence followed by the true continuation, the LATER one by a wrong token"""
    R, n0 = [int(t) for t in R0] + [int(t) for t in want], len(R0)
    steps = range(len(want))
    return (sum((R[n0 + g - 2:n0 + g + k] + [SEP] for g in steps), []) + sum((R[n0 + g - 2:n0 + g] + [(R[n0 + g] + 1) % V, SEP] for g in steps), []))


def _run(lnb, gm, prompt, start, n, C, branches, sampler=None, zseq=0):
    c = lnb.InferenceContext(gm, seq_of(start)).set_batched_attention(-1, zseq)
    _, f = c.Forward(prompt, 0, want_logits=False)
    if C is None:
        got, fin, _ = c.decode_sample_until(sampler, f, start, n) if sampler else c.decode_greedy_until(f, start, n)
        return c, f, got, fin, None
    c.set_draft(15, 2, 2, C, branches=branches)
    got, fin, st, _ = c.decode_speculative_sample_until(sampler, prompt, f, start, n) if sampler else c.decode_speculative_until(prompt, f, start, n)
    return c, f, got, fin, st


def _check(lnb, gm, cfg, prompt, start, n, make_corpus, branches, sampler=None, zseq=0):
    """the loop with `branches` against the one-token loop; -> (stats, simulated passes)"""
    g, f, want, wfin, _ = _run(lnb, gm, prompt, start, n, None, 1, sampler)
    kv_want = _kv(g, cfg, start + n)
    g.close()
    C = make_corpus(list(prompt) + [f], want)
    lnb.form_count_reset()
    c, _, got, fin, st = _run(lnb, gm, prompt, start, n, C, branches, sampler, zseq)
    sim, passes = simulate(prompt, f, want, C, 2, 2, 15, branches, n, seq_of(start), start)
    assert (got == want).all() and fin == wfin and st == sim, (st, sim)
    assert _same(_kv(c, cfg, start + n), kv_want)
    c.close()
    return st, passes


@pytest.mark.parametrize("branches", [2, 4])
@pytest.mark.parametrize("hd,G", list(GEO))
def test_tree_passes_give_the_greedy_loops_tokens_and_kv_rows_and_accept_more(lnb, models, hd, G, branches):
    gm, cfg = models((hd, G))
    prompt = lnb.synth_tokens(99, 8, cfg["vocab_size"])
    corpus = lambda R0, want: two_occurrences(R0, want, cfg["vocab_size"])
    chain, _ = _check(lnb, gm, cfg, prompt, 8, N, corpus, 1)
    assert count(lnb, "attn_tree") == 0                      # branches 1: nothing of the tree path runs
    with ran(lnb, ("attn_tree.scores", "attn_tree.pv")):
        tree, passes = _check(lnb, gm, cfg, prompt, 8, N, corpus, branches)
    assert tree["accepted"] > chain["accepted"], (tree, chain)
    assert any(p[1:] != list(range(1, len(p))) for _, p in passes)       # some accepted path was not candidate 0: its rows moved


# the first pass sits at pos = start: pos % 16 = 1, 0, 9, 15, 8; at 250 its eight slots straddle the 256-position block of the scores launch and the PV
# launch adds two z_part blocks; zseq: every row walks the serial f64 sum (the masked-slot arm of the walk)
@pytest.mark.parametrize("start,zseq", [(1, 0), (16, 0), (25, 0), (31, 0), (40, 0), (250, 0), (25, 1), (250, 1)])
@pytest.mark.parametrize("hd,G", [(128, 4), (64, 1)])
def test_accepted_rows_move_into_place_across_a_tile_edge(lnb, models, hd, G, start, zseq):
    gm, cfg = models((hd, G))
    V = cfg["vocab_size"]
    prompt = lnb.synth_tokens(7, start, V)
    corpus = lambda R0, want: R0[-2:] + [int(t) for t in want[:5]] + [SEP] + R0[-2:] + [(int(want[0]) + 1) % V, (int(want[0]) + 2) % V]
    _, passes = _check(lnb, gm, cfg, prompt, start, 6, corpus, 2, zseq=zseq)
    pos, path = passes[0]
    assert pos == start and len(path) > 1 and path[1] > 1    # the accepted depth-1 node is not node 1: its K / V row came from another slot


def test_sampling_loop_with_a_tree(lnb, models):
    gm, cfg = models((128, 4))
    prompt = lnb.synth_tokens(99, 8, cfg["vocab_size"])
    s = lnb.Sampler(temperature=0.9, top_p=0.95, seed=5)
    with ran(lnb, ("attn_tree.scores", "attn_tree.pv")):
        _check(lnb, gm, cfg, prompt, 8, N, lambda R0, want: two_occurrences(R0, want, cfg["vocab_size"]), 2, sampler=s)


def test_a_rules_call_ignores_the_branches_and_drafts_the_chain(lnb, models):
    gm, cfg = models((128, 4))
    prompt = lnb.synth_tokens(99, 8, cfg["vocab_size"])
    s, rules = lnb.Sampler(temperature=0.9, seed=5), lnb.LogitRules(repetition_penalty=1.3)
    g = lnb.InferenceContext(gm, 64)
    _, f = g.Forward(prompt, 0, want_logits=False)
    want, _, _ = g.decode_sample_until(s, f, 8, N, rules=rules)
    c = lnb.InferenceContext(gm, 64)
    c.Forward(prompt, 0, want_logits=False)
    c.set_draft(15, 2, 2, two_occurrences(list(prompt) + [f], want, cfg["vocab_size"]), branches=2)
    lnb.form_count_reset()
    got, _, st, _ = c.decode_speculative_sample_until(s, prompt, f, 8, N, rules=rules)
    assert (got == want).all() and st["verify_passes"] > 0 and count(lnb, "attn_tree") == 0
    g.close(); c.close()


@pytest.mark.parametrize("zseq", [0, 1])
def test_a_siblings_slot_holds_a_huge_finite_value_that_no_other_row_may_see(lnb, zseq):
    """A one-layer model (its V rows are all the V rows there are) in which ONE token, X, gets a V row of about 2^120: X alone has a non-zero embedding in
    dimension 0 and wv's column 0 is 2^116.  X is the wrong candidate (node 1, slot pos + 1); the accepted path sits beside it.  Any e > 0 for that slot in
    another row -- a leaked mask bit, in the sums or in the PV chain -- moves that row's output by many orders of magnitude, and a +0 * v would still be exact."""
    cfg, X = kv_craft.GEOMETRIES["hd64"], 1000
    V, dim, kvd = cfg["vocab_size"], cfg["dim"], cfg["n_kv_heads"] * kv_craft.head_dim(cfg)
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(kv_craft.SEED_MODEL)
    emb = gm.get_tensor("tok_embeddings.weight", V * dim).reshape(V, dim).copy()
    emb[:, 0] = 0; emb[X] = 0; emb[X, 0] = kv_craft.bf([1.0])[0]
    wv = gm.get_tensor("layers.0.attention.wv.weight", kvd * dim).reshape(kvd, dim).copy()
    wv[:, 0] = kv_craft.bf([2.0 ** 116])[0]
    gm.set_tensor("tok_embeddings.weight", emb); gm.set_tensor("layers.0.attention.wv.weight", wv)
    gm.finalize().enable_batch()
    probe = lnb.InferenceContext(gm, 8)
    probe.Forward([X], 0, want_logits=False)
    vx = np.abs(kv_craft.wide(probe.CacheV(0)[0]))
    assert np.isfinite(vx).all() and vx.min() >= 2.0 ** 112, vx.min()          # X's V row: huge, finite
    probe.close()
    prompt = lnb.synth_tokens(7, 40, V)
    corpus = lambda R0, want: R0[-2:] + [int(t) for t in want[:5]] + [SEP] + R0[-2:] + [X]
    st, passes = _check(lnb, gm, cfg, prompt, 40, 6, corpus, 2, zseq=zseq)
    assert X not in list(prompt) and passes[0][0] == 40 and passes[0][1][:2] == [0, 2] and st["accepted"] > 0      # node 1 = X, rejected; the path runs beside it
    gm.close()


def test_tree_draft_kernel_follows_the_restated_rule(lnb):
    cases = [a for a, _ in CASES.values()] + [
        ([], [1, 2, 3], 1, 4, 7, 2),                          # empty text
        ([7, 7, 7, 7, 7], [7, 7, 8], 1, 4, 15, 4),            # overlapping matches in R, then C: R latest first
        ([1, 2, 3], [9, 1, 2, 3], 1, 3, 5, 2),                # the match ends the corpus: nothing follows
        ([4, 5, 6], [4, 5, 6, 1, 2, 3, 4, 5, 6, 7], 2, 3, 15, 1),     # branches 1: the chain
        ([3, 1, 3], [3, 1, 3, 1], 2, 2, 0, 2),                # max_draft 0
    ]
    for R, C, nmin, nmax, md, b in cases:
        tok, par, dep = lnb.op_tree_draft(R, C, nmin, nmax, md, b)
        assert ([int(t) for t in tok], [int(t) for t in par], [int(t) for t in dep]) == ref_tree(R, C, nmin, nmax, md, b), (list(R), list(C), nmin, nmax, md, b)
