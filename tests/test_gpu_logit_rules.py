"""Logit bias, repetition / presence / frequency penalties and min-p in the device sampling loops (include/lnb.h), on the MI355X: the token is a pure function of
(logits row, sampler, rules, counted text, position) on integers behind the exp table, so everything is compared bit for bit with tests/logit_rules_ref.py -- the
kernel on host rows (tokens and every info field), and whole generations with the chain "oracle one-token step, restatement with running counts, feed the token"."""
import ctypes as C
import math

import numpy as np
import pytest

from form_tally import ran
from oracle import oracle as orc
import logit_rules_ref as lr
import sampler_ref as sr

pytestmark = pytest.mark.gpu
SEED, P0, STEPS, SEQ = 777, 8, 24, 64
SMP = (0.7, 40, 0.9)
RULES = (1.3, 0.5, 0.25, 0.02, ((5, 1.5), (17, -math.inf), (1023, -0.75)))


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


def op_check(lnb, cases):
    """cases: (row, counts, (t, k, p), rules, seed, pos, u or None) -- row i of ONE lnb_op_sample_rules call each, so that the rows' arrays are aligned differently"""
    tok, info = lnb.op_sample_rules(np.stack([c[0] for c in cases]), [c[2] + (c[4],) for c in cases], [c[3] for c in cases], np.stack([c[1] for c in cases]),
                                    [c[5] for c in cases], draws=[sr.draw(c[4], c[5]) if c[6] is None else c[6] for c in cases])
    for i, (row, counts, smp, rules, seed, pos, u) in enumerate(cases):
        want = lr.sample(row, smp + (seed,), rules, counts, pos, u)
        assert (int(tok[i]), info[i]) == want, (i, smp, rules, seed, pos, u, int(tok[i]), info[i], want)
    return tok


# ---- 1. the operator, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["repetition", "presence", "frequency", "bias", "min_p", "all"])
@pytest.mark.parametrize("V", [1000, 1001, 8200, 128256, 131072])
def test_op_sample_rules_equals_the_restatement(lnb, V, name):
    """1000: lanes without entries; 1001: row 1's three arrays start at 2002, 4004 and 2002 bytes; 8200: aligned groups and a tail group; the model's V; the cap"""
    rng = np.random.default_rng(20261126 + V)
    rows = sr.llama_like_rows(rng, 2, V)
    counts = lr.counted_rows(rng, rows)
    rules = lr.rule_sets(V)[name]
    cases = [(rows[j % 2], counts[j % 2], smp, rules, sr.SEEDS[j % 3], sr.POSITIONS[j % 3], None) for j, smp in enumerate(lr.SAMPLERS)]
    with ran(lnb, "sample.rules_row"):
        tok = op_check(lnb, cases)
    plain = [sr.sample(c[0], c[2] + (c[4],), c[5])[0] for c in cases]
    assert name not in ("repetition", "presence", "all") or list(tok) != plain      # (these move a token at every V here: a kernel that ignored them cannot pass)


@pytest.mark.parametrize("V", [1001, 8200])
def test_op_sample_rules_on_the_crafted_rows(lnb, V):
    cases, wants = [], []
    for name, row, counts, smp, rules, want, boundaries in lr.crafted(V):
        for u in [None] + (sr.boundary_draws(lr.prepare(row, *smp, rules, counts)) if boundaries else []):
            cases.append((row, counts, smp, rules, SEED, 8, u)); wants.append(want)
    with ran(lnb, "sample.rules_row"):
        tok = op_check(lnb, cases)
    assert all(w is None or int(t) == w for t, w in zip(tok, wants))
    # counts NULL = all zero; rules all off = lnb_op_sample
    rows = np.stack([c[0] for c in cases[:4]])
    smps = [c[2] + (SEED,) for c in cases[:4]]
    assert (lnb.op_sample_rules(rows, smps, [None] * 4, None, [8] * 4)[0] == lnb.op_sample(rows, smps, [8] * 4)[0]).all()


# ---- 2. the loops on the tiny model -------------------------------------------------------------------------------------------------------
def oracle_chain(om, prompt, smp, rules, steps, counted):
    """oracle one-token step, restatement with running counts, feed the token: what decode_sample_until(first, P0, steps, rules, counted) must emit"""
    c = orc.Context(om, SEQ)
    _, tok = c.forward(prompt, 0)
    counts = np.bincount(np.asarray(list(counted) + [tok], dtype=np.int64), minlength=orc.TINY["vocab_size"]).astype(np.uint32)
    toks = []
    for i in range(steps):
        row, _ = c.forward(np.array([tok], dtype=np.int32), len(prompt) + i)
        r16 = orc.f32_to_bf16(np.ascontiguousarray(row[-1], dtype=np.float32))
        tok, _ = lr.sample(r16, smp + (SEED,), rules, counts, pos=len(prompt) + i)
        counts[tok] += 1
        toks.append(tok)
    c.close()
    return np.array(toks, dtype=np.int32)


@pytest.fixture(scope="module")
def tiny(lnb):
    cfg = dict(orc.TINY)
    om = orc.Model(**cfg).fill_synthetic(1234).finalize()
    prompt = lnb.synth_tokens(99, 8, cfg["vocab_size"])
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize()
    want = {smp: oracle_chain(om, prompt, smp, RULES, STEPS, prompt) for smp in (SMP, (0.0, 0, 1.0))}
    yield gm, prompt, want
    gm.close(); om.close()


def fresh(lnb, gm, prompt):
    c = lnb.InferenceContext(gm, SEQ)
    _, first = c.Forward(prompt, 0, want_logits=False)
    return c, first


def test_tiny_generation_under_rules_equals_the_oracle_chain_in_any_chunking(lnb, tiny):
    gm, prompt, want = tiny
    for smp in want:
        c, f = fresh(lnb, gm, prompt)
        plain, _, _ = c.decode_sample_until(smp + (SEED,), f, P0, STEPS)
        greedy, _, _ = c.decode_greedy_until(f, P0, STEPS)
        with ran(lnb, "sample.rules_row"):
            got, fin, _ = c.decode_sample_until(smp + (SEED,), f, P0, STEPS, rules=RULES, counted=prompt)
        assert (got == want[smp]).all() and not fin and (got != plain).any(), (smp, got, want[smp])
        # rules all off = the plain sampling loop; the plain and greedy graphs survived the rules call
        assert (c.decode_sample_until(smp + (SEED,), f, P0, STEPS, rules=lr.OFF[:4], counted=prompt)[0] == plain).all()
        assert (c.decode_sample_until(smp + (SEED,), f, P0, STEPS)[0] == plain).all() and (c.decode_greedy_until(f, P0, STEPS)[0] == greedy).all()
        # chunks of uneven length: the earlier chunks' tokens come back in `counted`
        parts, tok, text = [], f, list(prompt)
        for k, n in enumerate((5, 1, 11, 7)):
            lnb.form_count_reset()
            part, _, _ = c.decode_sample_until(smp + (SEED,), tok, P0 + len(text) - len(prompt), n, rules=RULES, counted=text)
            assert lnb.form_count("sample.rules_row") == 0   # replays of the captured rules graph only
            parts.append(part); text += [tok] + [int(t) for t in part[:-1]]; tok = int(part[-1])
        assert (np.concatenate(parts) == want[smp]).all()
        c.close()


def test_tiny_a_stop_id_freezes_the_counts_and_a_second_call_continues(lnb, tiny):
    gm, prompt, want = tiny
    w = want[SMP]
    stop = int(w[5])
    n = int(np.nonzero(w == stop)[0][0]) + 1
    c, f = fresh(lnb, gm, prompt)
    c.set_stop_ids([stop])
    got, fin, _ = c.decode_sample_until(SMP + (SEED,), f, P0, STEPS, rules=RULES, counted=prompt)
    assert fin and (got == w[:n]).all()
    c.set_stop_ids([])
    text = list(prompt) + [f] + [int(t) for t in got[:-1]]
    more, fin, _ = c.decode_sample_until(SMP + (SEED,), int(got[-1]), P0 + n, STEPS - n, rules=RULES, counted=text)
    assert not fin and (more == w[n:]).all()                 # the frozen run left the context able to go on: the rest of the same chain
    c.close()


def test_batch_members_under_their_own_rules_equal_their_single_runs(lnb, tiny):
    gm, prompt, _ = tiny
    V = 1024
    prompts = [lnb.synth_tokens(300 + s, (5, 8, 11)[s], V) for s in range(3)]
    smps = [(0.7, 40, 0.9, 11), (0.0, 0, 1.0, 12), (1.0, 0, 1.0, 13)]
    rules = [RULES, (1.5, 0.0, 0.0, 0.0, ()), (1.0, 0.0, 0.5, 0.1, ((9, -math.inf),))]
    single, ctxs, firsts = [], [], []
    for s in range(3):
        c, f = fresh(lnb, gm, prompts[s])
        single.append(c.decode_sample_until(smps[s], f, len(prompts[s]), 12, rules=rules[s], counted=prompts[s])[0])
        c.close()
        c, f = fresh(lnb, gm, prompts[s])
        ctxs.append(c); firsts.append(f)
    bat = lnb.Batch(ctxs)
    with ran(lnb, "sample.rules_batch"):
        got, _ = bat.decode_sample_until(smps, firsts, [len(p) for p in prompts], 8, rules=rules, counted=prompts)
    assert all((got[s] == single[s][:8]).all() for s in range(3))
    texts = [list(prompts[s]) + [firsts[s]] + [int(t) for t in got[s][:-1]] for s in range(3)]
    more, _ = bat.decode_sample_until(smps, [int(g[-1]) for g in got], [len(prompts[0]) + 8, -1, len(prompts[2]) + 8], 4, rules=rules, counted=texts)      # member 1 frozen
    assert len(more[1]) == 0 and (more[0] == single[0][8:]).all() and (more[2] == single[2][8:]).all()
    bat.close()
    for c in ctxs:
        c.close()


def test_the_engine_counts_the_prompt_and_the_generated_text(lnb, tiny):
    gm, prompt, _ = tiny
    got = lnb.InferenceEngine(gm, SEQ, rules=lnb.LogitRules(*RULES[:4], bias=dict(RULES[4]))).GenerateTokens(prompt, max_new=10)      # no sampler: greedy under rules
    c, f = fresh(lnb, gm, prompt)
    row, _ = c.ForwardAppend(prompt[-1:], len(prompt) - 1, want_logits=True)
    first, _ = lr.sample(orc.f32_to_bf16(np.ascontiguousarray(row[0], dtype=np.float32)), (0.0, 0, 1.0, 0), RULES, np.bincount(prompt, minlength=1024), len(prompt) - 1)
    more, _, _ = c.decode_sample_until((0.0, 0, 1.0, 0), first, P0, 9, rules=RULES, counted=prompt)
    c.close()
    assert got == [first] + [int(t) for t in more]


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------------
NAN, INF = math.nan, math.inf
REFUSALS = [(dict(rules=None), "rules"), (dict(rp=NAN), "repetition_penalty"), (dict(presence=INF), "presence_penalty"), (dict(frequency=-INF), "frequency_penalty"),
            (dict(rp=0.0), "repetition_penalty"), (dict(rp=-1.0), "repetition_penalty"), (dict(min_p=NAN), "min_p"), (dict(min_p=-0.1), "min_p"), (dict(min_p=1.5), "min_p"),
            (dict(reserved=1), "reserved"), (dict(n_bias=-1), "n_bias"), (dict(n_bias=1025), "n_bias"), (dict(n_bias=2, null_bias=True), "null bias"),
            (dict(bias=((1024, 1.0),)), "outside the vocabulary"), (dict(bias=((-1, 1.0),)), "outside the vocabulary"), (dict(bias=((4, 1.0), (4, 2.0))), "twice"),
            (dict(bias=((4, NAN),)), "NaN or +inf"), (dict(bias=((4, INF),)), "NaN or +inf"), (dict(n_counted=-1), "n_counted"), (dict(n_counted=3, null_counted=True), "counted"),
            (dict(counted=[1, 1024]), "outside the vocabulary"), (dict(counted=[-5]), "outside the vocabulary"), (dict(temperature=-1.0), "temperature")]


@pytest.mark.parametrize("bad,word", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_leave_the_cache_alone(lnb, tiny, bad, word):
    gm, prompt, _ = tiny
    c, f = fresh(lnb, gm, prompt)
    before = (c.CacheK(0).copy(), c.CacheV(0).copy())
    r = lnb.LogitRules(bad.get("rp", 1.3), bad.get("presence", 0.5), bad.get("frequency", 0.25), bad.get("min_p", 0.02), bias=bad.get("bias", ((5, 1.5),)))
    r.reserved = bad.get("reserved", 0)
    r.n_bias = bad.get("n_bias", r.n_bias)
    if bad.get("null_bias"):
        r.bias_ids = None
    counted = np.array(bad.get("counted", prompt), dtype=np.int32)
    s = lnb.Sampler(bad.get("temperature", 0.7), 40, 0.9, SEED)
    out = np.zeros(4, dtype=np.int32); n = C.c_int(0)
    rc = c.L.lnb_decode_sample_rules_until(c.h, C.byref(s), None if "rules" in bad else C.byref(r), None if bad.get("null_counted") else lnb._p(counted),
                                           bad.get("n_counted", counted.size), f, P0, 4, lnb._p(out), C.byref(n), None, None)
    assert rc < 0 and word in c.L.lnb_last_error().decode(), c.L.lnb_last_error().decode()
    assert (c.CacheK(0) == before[0]).all() and (c.CacheV(0) == before[1]).all()
    c.close()
