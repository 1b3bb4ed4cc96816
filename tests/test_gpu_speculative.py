"""Speculative greedy decoding on the MI355X (include/lnb.h "speculative greedy decoding"): n-gram drafts verified by batched passes whose
columns alias one context.  Whatever the drafts, the tokens, n_generated, finished and every KV row must be those of lnb_decode_greedy_until
(and of the oracle); the draft kernel and the pass counts must follow the documented rule exactly."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------
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


def simulate(history, token, out, corpus, nmin, nmax, max_draft, max_steps, seq_len, start_pos):
    """the passes of lnb_decode_speculative_until over its known output"""
    out = [int(t) for t in out]
    n, g = len(out), 0
    s = dict(passes=0, verify_passes=0, drafted=0, accepted=0)
    while g < n:
        R = [int(t) for t in history] + [int(token)] + out[:g]
        lim = min(max_steps - g - 1, seq_len - (start_pos + g) - 1)
        d = ref_draft(R, corpus, nmin, nmax, max_draft)[:max(lim, 0)]
        s["passes"] += 1
        if d:
            s["verify_passes"] += 1
            s["drafted"] += len(d)
        a = 0
        while a < len(d) and g + a < n and d[a] == out[g + a]:
            a += 1
        g += min(a + 1, n - g)
    s["accepted"] = n - s["passes"]
    return s


# ---- 1. the draft kernel ------------------------------------------------------------------------------------------------------------
def _check_op(lnb, R, C, nmin, nmax, md):
    got = lnb.op_ngram_draft(R, C, nmin, nmax, md)
    want = ref_draft(R, C, nmin, nmax, md)
    assert [int(t) for t in got] == want, (list(R), list(C), nmin, nmax, md)


def test_ngram_draft_kernel_follows_the_rule_on_random_arrays(lnb):
    rng = np.random.default_rng(11)
    for it in range(120):
        V = int(rng.choice([2, 3, 5, 20, 1000]))
        R = rng.integers(0, V, size=int(rng.integers(0, 300)))
        C = rng.integers(0, V, size=int(rng.integers(0, 300)))
        nmax = int(rng.integers(1, 17))
        nmin = int(rng.integers(1, nmax + 1))
        _check_op(lnb, R, C, nmin, nmax, int(rng.integers(0, 16)))
    # long arrays (the search is parallel over positions): about 8 K tokens in all
    R = rng.integers(0, 50, size=4000); C = rng.integers(0, 50, size=4200)
    for nmin, nmax in ((1, 4), (2, 8), (3, 16)):
        _check_op(lnb, R, C, nmin, nmax, 15)


def test_ngram_draft_kernel_on_adversarial_arrays(lnb):
    cases = [
        ([], [1, 2, 3], 1, 4, 7),                     # empty text: no suffix at all
        ([5], [5, 6, 7], 1, 1, 7),                    # a one-token text matched in the corpus
        ([5], [5], 1, 1, 7),                          # ... at the very end of the corpus: nothing follows, no match
        ([1, 2, 1, 2], [], 1, 3, 7),                  # overlapping match in the text itself
        ([7, 7, 7, 7, 7], [], 1, 4, 15),              # ties everywhere: the latest start wins
        ([7, 7, 7, 7, 7], [7, 7, 8], 1, 4, 15),       # R before C
        ([1, 2, 3, 9, 2, 3], [1, 2, 3, 4, 5], 1, 3, 5),   # longer n in C beats shorter n in R
        ([1, 2, 3], [9, 1, 2, 3], 1, 3, 5),           # the match ends the corpus: none for n = 3, n = 2 and 1 likewise, so nothing
        ([4, 5, 6], [4, 5, 6, 1, 2, 3, 4, 5, 6, 7], 2, 3, 15),   # two corpus matches: the latest
        ([1, 2], [1, 2, 3], 3, 5, 7),                 # n longer than the text
        (list(range(40)) + list(range(20)), [], 1, 16, 15),      # the draft cut at the end of the text
        ([3, 1, 3], [3, 1, 3, 1], 2, 2, 0),           # max_draft 0
    ]
    for R, C, nmin, nmax, md in cases:
        _check_op(lnb, R, C, nmin, nmax, md)


# ---- 2. tiny oracle model -----------------------------------------------------------------------------------------------------------
N_TINY = 40


@pytest.fixture(scope="module")
def tiny(lnb):
    cfg = dict(orc.TINY)
    om = orc.Model(**cfg).fill_synthetic(1234).finalize()
    prompt = lnb.synth_tokens(99, 8, cfg["vocab_size"])
    ref, _ = orc.Context(om, 64).generate(prompt, N_TINY + 1)
    om.close()
    ref = np.array([int(t) for t in ref], dtype=np.int32)
    models = {}
    for form in ("rows", "columns"):
        gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize()
        if form == "columns":
            gm.enable_batch()
        models[form] = gm
    yield models, prompt, ref, cfg
    for gm in models.values():
        gm.close()


def _kv(ctx, n_layers, rows):
    return [(ctx.CacheK(l)[:rows].copy(), ctx.CacheV(l)[:rows].copy()) for l in range(n_layers)]


def _corpus(kind, ref, V):
    if kind == "none":
        return []
    c = ref.copy()
    m = {"exact": 0, "every2": 2, "every5": 5}[kind]
    if m:
        c[m - 1::m] = (c[m - 1::m] + 1) % V
    return c


@pytest.mark.parametrize("form", ["rows", "columns"])
def test_tiny_speculative_equals_greedy_and_the_oracle(lnb, tiny, form):
    models, prompt, ref, cfg = tiny
    gm, P, seq_len, nmin, nmax = models[form], 8, 64, 1, 4
    g = lnb.InferenceContext(gm, seq_len)
    _, first = g.Forward(prompt, 0, want_logits=False)
    assert first == ref[0]
    want, wfin, _ = g.decode_greedy_until(first, P, N_TINY)
    assert (want == ref[1:]).all() and not wfin
    kv_want = _kv(g, cfg["n_layers"], P + N_TINY)
    g.close()
    for kind in ("none", "exact", "every2", "every5"):
        C = _corpus(kind, ref, cfg["vocab_size"])
        for md in (1, 3, 7, 15):
            c = lnb.InferenceContext(gm, seq_len)
            _, f = c.Forward(prompt, 0, want_logits=False)
            c.set_draft(md, nmin, nmax, C)
            got, fin, st, _ = c.decode_speculative_until(prompt, f, P, N_TINY)
            assert (got == want).all() and not fin, (kind, md)
            sim = simulate(prompt, f, want, C, nmin, nmax, md, N_TINY, seq_len, P)
            assert st == sim, (kind, md, st, sim)
            if kind == "exact":
                assert st["verify_passes"] > 0 and st["accepted"] > 0
            kv = _kv(c, cfg["n_layers"], P + N_TINY)
            for l in range(cfg["n_layers"]):
                assert (kv[l][0] == kv_want[l][0]).all() and (kv[l][1] == kv_want[l][1]).all(), (kind, md, l)
            c.close()


def test_tiny_stop_ids_as_accepted_draft_and_as_bonus_token(lnb, tiny):
    models, prompt, ref, cfg = tiny
    gm, P = models["rows"], 8
    out = ref[1:]
    j = next(i for i in range(6, N_TINY) if out[i] not in out[:i] and out[i] != ref[0])
    stop = int(out[j])
    for case in ("accepted", "bonus"):
        C = ref.copy()
        if case == "bonus":                                  # the draft is wrong exactly at the stop token: it comes from the column's argmax
            C[1 + j] = (C[1 + j] + 1) % cfg["vocab_size"]
        g = lnb.InferenceContext(gm, 64).set_stop_ids([stop])
        _, f = g.Forward(prompt, 0, want_logits=False)
        want, wfin, _ = g.decode_greedy_until(f, P, N_TINY)
        assert wfin and want.size == j + 1
        g.close()
        for md in (3, 7, 15):
            c = lnb.InferenceContext(gm, 64).set_stop_ids([stop])
            _, f = c.Forward(prompt, 0, want_logits=False)
            c.set_draft(md, 1, 4, C)
            got, fin, st, _ = c.decode_speculative_until(prompt, f, P, N_TINY)
            assert fin and (got == want).all(), (case, md)
            assert st == simulate(prompt, f, want, C, 1, 4, md, N_TINY, 64, P), (case, md)
            # a finished context stays usable: the greedy loop continues it from the stop token
            c.close()


def test_tiny_limits_and_continuation(lnb, tiny):
    models, prompt, ref, cfg = tiny
    gm, P = models["columns"], 8
    n = 20
    for extra in (0, 1):                                     # seq_len ends exactly at start_pos + max_steps (+ 1)
        seq_len = P + n + extra
        c = lnb.InferenceContext(gm, seq_len)
        _, f = c.Forward(prompt, 0, want_logits=False)
        c.set_draft(15, 1, 4, ref)
        got, fin, st, _ = c.decode_speculative_until(prompt, f, P, n)
        assert (got == ref[1:n + 1]).all() and not fin
        assert st == simulate(prompt, f, got, ref, 1, 4, 15, n, seq_len, P)
        c.close()
    # a greedy continuation after a speculative run, and lnb_forward after that: the oracle's tokens
    c = lnb.InferenceContext(gm, 64)
    _, f = c.Forward(prompt, 0, want_logits=False)
    c.set_draft(7, 1, 4, ref)
    a, _, _, _ = c.decode_speculative_until(prompt, f, P, 12)
    b, _ = c.decode_greedy(int(a[-1]), P + 12, 10)
    _, nxt = c.Forward([int(b[-1])], P + 22, want_logits=False)
    assert [int(t) for t in a] + [int(t) for t in b] + [nxt] == [int(t) for t in ref[1:24]]
    # drafting off: the greedy loop itself, one pass per token
    d = lnb.InferenceContext(gm, 64)
    _, f = d.Forward(prompt, 0, want_logits=False)
    got, _, st, _ = d.decode_speculative_until(prompt, f, P, 10)
    assert (got == ref[1:11]).all() and st == dict(passes=10, verify_passes=0, drafted=0, accepted=0)
    c.close(); d.close()


def test_refusals(lnb, tiny):
    models, prompt, ref, cfg = tiny
    gm = models["columns"]
    c = lnb.InferenceContext(gm, 64)
    _, f = c.Forward(prompt, 0, want_logits=False)
    c.set_draft(7, 1, 4, ref)
    c.set_token_probs(4)
    with pytest.raises(lnb.LnbError, match="token probabilities"):
        c.decode_speculative_until(prompt, f, 8, 8)
    c.set_token_probs(0)
    c.set_mode("fast")
    with pytest.raises(lnb.LnbError, match="exact"):
        c.decode_speculative_until(prompt, f, 8, 8)
    c.set_mode("exact")
    d = lnb.InferenceContext(gm, 64)
    bat = lnb.Batch([c, d])
    with pytest.raises(lnb.LnbError, match="live batch"):
        c.decode_speculative_until(prompt, f, 8, 8)
    bat.close()
    got, _, _, _ = c.decode_speculative_until(prompt, f, 8, 8)
    assert (got == ref[1:9]).all()
    for bad in ((16, 1, 4), (-1, 1, 4), (3, 0, 4), (3, 5, 4), (3, 1, 17)):
        with pytest.raises(lnb.LnbError):
            c.set_draft(*bad)
    c.close(); d.close()


# ---- 3. full shapes -----------------------------------------------------------------------------------------------------------------
def test_8b_configs1_golden_with_and_without_the_batch_copy(lnb):
    g = json.load(open(os.path.join(GOLD, "configs1_tokens.json")))
    gold = [int(t) for t in g["tokens"]]
    gm = lnb.LlamaTransformer(**lnb.LLAMA_8B).fill_synthetic(g["weights_seed"]).finalize()
    prompt = lnb.synth_tokens(g["prompt_seed"], 128, 128256)
    n = len(gold) - 1
    try:
        for form in ("rows", "columns"):
            if form == "columns":
                gm.enable_batch()
            c = lnb.InferenceContext(gm, 128 + n + 1)
            _, first = c.Forward(prompt, 0, want_logits=False)
            assert first == gold[0]
            c.set_draft(7, 1, 4, gold)
            got, fin, st, ms = c.decode_speculative_until(prompt, first, 128, n)
            assert [int(t) for t in got] == gold[1:], form
            assert st == simulate(prompt, first, got, gold, 1, 4, 7, n, 128 + n + 1, 128)
            assert st["verify_passes"] > 0 and st["accepted"] > n // 2
            c.close()
    finally:
        gm.close()


def test_32layer_configs2_golden_long_context(lnb):
    gold = json.load(open(os.path.join(GOLD, "configs2_32layer_tokens.json")))
    P, toks = gold["prompt_len"], [int(t) for t in gold["tokens"]]
    cfg = dict(orc.LLAMA_8B, n_layers=gold["n_layers"], max_seq_len=2304)
    gm = lnb.LlamaTransformer(**cfg).fill_synthetic(gold["weights_seed"]).finalize()
    try:
        prompt = lnb.synth_tokens(gold["prompt_seed"], P, cfg["vocab_size"])
        n = len(toks) - 1
        c = lnb.InferenceContext(gm, P + n + 1)
        _, first = c.Forward(prompt, 0, want_logits=False)
        assert first == toks[0]
        c.set_draft(7, 1, 4, toks)
        got, fin, st, _ = c.decode_speculative_until(prompt, first, P, n)
        assert [int(t) for t in got] == toks[1:]
        assert st == simulate(prompt, first, got, toks, 1, 4, 7, n, P + n + 1, P) and st["verify_passes"] > 0
        c.close()
    finally:
        gm.close()
