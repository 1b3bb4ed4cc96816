"""Logit rules in the speculative sampling loops on the MI355X (include/lnb.h): the verify launch on bare rows against tests/logit_rules_ref.py column by column,
lnb_decode_speculative_sample_rules_until / _many against lnb_decode_sample_rules_until bit for bit -- tokens, n_generated, finished, KV rows -- and against the CPU
chain.  The inputs, and the conditions that keep these tests from being empty, are those of tests/test_spec_rules_cpu.py; contexts as in tests/test_gpu_spec_sample.py."""
import numpy as np
import pytest

from form_tally import ran
import logit_rules_ref as lr
import spec_sim as ss
import test_spec_rules_cpu as cpu
from test_gpu_spec_sample import fresh, kv_rows, lnb, same_kv, tiny  # noqa: F401 (lnb and tiny are its fixtures)

pytestmark = pytest.mark.gpu
P0, STEPS, SEQ, NMIN, NMAX = ss.P0, ss.STEPS, ss.SEQ, ss.NMIN, ss.NMAX


def rule_set(lnb, which, V):
    rules = cpu.full_rules(V) if which == "full" else lr.OFF
    return rules, lnb.LogitRules(*rules)


@pytest.mark.parametrize("which", ["full", "off"])
@pytest.mark.parametrize("name", list(cpu.SAMPLERS))
@pytest.mark.parametrize("V", [1001, 1024, 128256])
def test_op_verify_launch_counts_the_drafts_in_front_of_every_column(lnb, V, name, which):
    rows, base, _ = cpu.bare(V)
    smp, (rules, R) = cpu.SAMPLERS[name], rule_set(lnb, which, V)
    g = cpu.true_chain(rows, smp, rules, base)
    # accepted prefixes 0, 1, 7, 15; under the full rules (where the chain's tokens differ) a stop id on an accepted draft (column 3's token) and on the bonus token (column 7's)
    for a, stops in [(a, ()) for a in (0, 1, 7, 15)] + ([(7, (V + 5, int(g[3]))), (7, (V + 5, int(g[7])))] if which == "full" else []):
        with ran(lnb, "sample.spec_rules", not_ran=("sample.spec", "sample.rules_row")):
            got, fin, after = lnb.op_spec_sample_rules_accept(rows, smp, R, base, cpu.POS0, cpu.columns(g, a, V), stop_ids=stops)
        want, wfin, wafter = cpu.emitted(g, a, base, stops)
        assert ([int(t) for t in got], fin) == (want, wfin) and wfin == bool(stops) and np.array_equal(after, wafter), (a, stops, list(got), want)


def reference(lnb, gm, cfg, prompt, smp, R, steps=STEPS, stop=(), counted=None):
    """decode_sample_until(rules=, counted=) of a fresh context -> (first, tokens, finished, KV rows)"""
    c, f = fresh(lnb, gm, prompt, stop=stop)
    got, fin, _ = c.decode_sample_until(smp, f, len(prompt), steps, rules=R, counted=prompt if counted is None else counted)
    kv = kv_rows(c, cfg["n_layers"], len(prompt) + len(got))
    c.close()
    return f, got, fin, kv


@pytest.mark.parametrize("which", ["full", "off"])
@pytest.mark.parametrize("name", list(cpu.SAMPLERS))
@pytest.mark.parametrize("form", ["rows", "columns"])
def test_tiny_equals_the_rules_loop(lnb, tiny, form, name, which):
    models, prompt, _, cfg = tiny
    V, smp, gm = cfg["vocab_size"], cpu.SAMPLERS[name], models[form]
    rules, R = rule_set(lnb, which, V)
    first, want, _, kv_want = reference(lnb, gm, cfg, prompt, smp, R)
    if form == "rows" and which == "full":                   # held to the CPU chain: oracle one-token step, logit_rules_ref.sample, feed the token
        cfirst, chain = cpu.rules_chain(smp, rules)
        assert first == cfirst and np.array_equal(want, chain)
    for kind, md in [(k, m) for k in ("exact", "every8") for m in (3, 15)]:
        C = cpu.corpus(kind, [first] + [int(t) for t in want], V)
        c, f = fresh(lnb, gm, prompt)
        c.set_draft(md, NMIN, NMAX, C)
        with ran(lnb, "sample.spec_rules", not_ran=("sample.spec", "sample.row")):
            got, fin, st, _ = c.decode_speculative_sample_until(smp, prompt, f, P0, STEPS, rules=R, counted=prompt)
        assert np.array_equal(got, want) and not fin, (kind, md, list(got), list(want))
        assert st == ss.simulate(prompt, first, want, C, NMIN, NMAX, md, STEPS, SEQ, P0), (kind, md, st)
        assert same_kv(kv_rows(c, cfg["n_layers"], P0 + STEPS), kv_want), (kind, md, "KV rows")
        c.close()


def test_tiny_chunks_hand_their_tokens_back_and_a_stop_id_ends_the_run(lnb, tiny):
    models, prompt, _, cfg = tiny
    gm, smp = models["columns"], cpu.SAMPLERS["t07_k40_p09"]
    rules, R = rule_set(lnb, "full", cfg["vocab_size"])
    first, want, _, _ = reference(lnb, gm, cfg, prompt, smp, R)
    C = cpu.corpus("every8", [first] + [int(t) for t in want], cfg["vocab_size"])
    c, f = fresh(lnb, gm, prompt)
    c.set_draft(7, NMIN, NMAX, C)
    parts, text = [], [int(t) for t in prompt] + [f]
    for k in range(3):                                       # three calls of 8 steps: the counted text and the history are the text so far
        parts.append(c.decode_speculative_sample_until(smp, text[:-1], text[-1], P0 + 8 * k, 8, rules=R, counted=text[:-1])[0])
        text += [int(t) for t in parts[-1]]
    c.close()
    assert np.array_equal(np.concatenate(parts), want[:24])
    stop = int(want[9])
    _, swant, sfin, skv = reference(lnb, gm, cfg, prompt, smp, R, stop=[stop])
    assert sfin and swant[-1] == stop and len(swant) <= 10
    c, f = fresh(lnb, gm, prompt, stop=[stop])
    c.set_draft(7, NMIN, NMAX, C)
    got, fin, st, _ = c.decode_speculative_sample_until(smp, prompt, f, P0, STEPS, rules=R, counted=prompt)
    assert fin and np.array_equal(got, swant) and same_kv(kv_rows(c, cfg["n_layers"], P0 + len(got)), skv)
    assert st == ss.simulate(prompt, f, swant, C, NMIN, NMAX, 7, STEPS, SEQ, P0)
    c.close()


@pytest.mark.parametrize("budget", [16, 32])
def test_many_members_equal_their_own_rules_loops(lnb, tiny, budget):
    """five members with their own prompts, samplers, rule sets, counted texts and max_draft: member 1 at temperature 0, member 2 with all rules off, member 4 frozen"""
    models, _, _, cfg = tiny
    gm, V, steps, frozen = models["columns"], cfg["vocab_size"], 24, 4
    prompts = [lnb.synth_tokens(300 + s, n, V) for s, n in enumerate((5, 8, 11, 6, 9))]
    smps = [(1.0, 0, 1.0, 1000), (0.0, 0, 1.0, 1), (0.7, 40, 0.9, 1014), (1.5, 0, 0.5, 1021), (1.0, 0, 1.0, 1028)]
    Rs = [lnb.LogitRules(*r) for r in (cpu.full_rules(V), (1.5, 0.0, 0.5, 0.0, ()), lr.OFF, (1.0, 0.25, 0.0, 0.1, ((7, -np.inf),)), cpu.full_rules(V))]
    counted = [e + list(p) for e, p in zip(([], [5, 5, 9], [], [1, 2, 3, 1], []), prompts)]
    refs = [reference(lnb, gm, cfg, prompts[s], smps[s], Rs[s], steps, counted=counted[s]) for s in range(5)]
    ctxs = [fresh(lnb, gm, p)[0] for p in prompts]
    for s, md in enumerate((7, 15, 3, 1, 7)):
        ctxs[s].set_draft(md, NMIN, NMAX, cpu.corpus("every8" if s % 2 else "exact", [refs[s][0]] + [int(t) for t in refs[s][1]], V))
    kv_frozen = kv_rows(ctxs[frozen], cfg["n_layers"], SEQ)
    with ran(lnb, "sample.spec_many_rules", not_ran=("sample.spec_many", "sample.spec", "sample.rules_row", "sample.row")):
        toks, fins, stats, info, _ = lnb.DecodeSpeculativeSampleMany(ctxs, smps, prompts, [r[0] for r in refs], [-1 if s == frozen else len(prompts[s]) for s in range(5)],
                                                                     steps, budget, rules=Rs, counted=counted)
    for s in range(5):
        if s == frozen:
            assert len(toks[s]) == 0 and fins[s] and same_kv(kv_rows(ctxs[s], cfg["n_layers"], SEQ), kv_frozen)
        else:
            assert np.array_equal(toks[s], refs[s][1]) and not fins[s], (budget, s, list(toks[s]), list(refs[s][1]))
            assert same_kv(kv_rows(ctxs[s], cfg["n_layers"], len(prompts[s]) + steps), refs[s][3]), (budget, s, "KV rows")
        ctxs[s].close()
    assert sum(st["accepted"] for st in stats) > 0 and sum(st["drafted"] - st["accepted"] for st in stats) > 0 and info["max_columns"] <= budget


def test_all_off_rules_equal_the_plain_loops_and_the_engine_drafts_the_same_text(lnb, tiny):
    models, prompt, _, cfg = tiny
    gm, V, smp = models["columns"], cfg["vocab_size"], cpu.SAMPLERS["t07_k40_p09"]
    first, want, _, _ = reference(lnb, gm, cfg, prompt, smp, lnb.LogitRules())
    C = cpu.corpus("every8", [first] + [int(t) for t in want], V)
    one, many = [], []
    for kw, kwm in (({}, {}), (dict(rules=lnb.LogitRules(), counted=prompt), dict(rules=[None, None], counted=[prompt, prompt]))):
        ctxs = [fresh(lnb, gm, prompt)[0] for _ in range(3)]
        for c, md in zip(ctxs, (7, 7, 3)):
            c.set_draft(md, NMIN, NMAX, C)
        one.append(ctxs[0].decode_speculative_sample_until(smp, prompt, first, P0, STEPS, **kw)[:3])
        many.append(lnb.DecodeSpeculativeSampleMany(ctxs[1:], [smp, smp], [prompt, prompt], [first, first], [P0, P0], STEPS, 0, **kwm)[:4])
        for c in ctxs:
            c.close()
    assert np.array_equal(one[0][0], one[1][0]) and one[0][1:] == one[1][1:] and np.array_equal(one[0][0], want)
    assert all(np.array_equal(a, b) for a, b in zip(many[0][0], many[1][0])) and many[0][1:] == many[1][1:]
    R = lnb.LogitRules(*cpu.full_rules(V))                  # InferenceEngine(rules=, draft=): the text of the engine without a draft
    assert lnb.InferenceEngine(gm, SEQ, rules=R, draft=(7, NMIN, NMAX)).GenerateTokens(prompt, 24) == lnb.InferenceEngine(gm, SEQ, rules=R).GenerateTokens(prompt, 24)
