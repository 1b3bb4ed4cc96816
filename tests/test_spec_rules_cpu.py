"""Logit rules in the speculative sampling loops (include/lnb.h), without a GPU: the inputs tests/test_gpu_spec_rules.py runs, with the conditions that keep that test
from being empty asserted on the reference alone; the delta rule of csrc/lnb_sample.h as a stand-alone program under the sanitizers; refusals; exports."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import logit_rules_ref as lr
from oracle import oracle as orc
import sampler_ref as sr
import spec_sim as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, CUR, POS0 = 16, 3, 8
SAMPLERS = {"t0": (0.0, 0, 1.0, 1), "t07_k40_p09": ss.SAMPLERS[1] + (786,)}


def full_rules(V):
    return (1.3, 0.5, 4.0, 0.05, ((5, 2.5), (V // 2, -math.inf)))


def hist(tokens, V):
    return np.bincount(np.asarray(tokens, dtype=np.int64), minlength=V).astype(np.uint32)


def bare(V):
    """-> (rows [16][V], base counts, the chain greedy must emit under the full rules).  Every row has the same peaks over its own N(0, 1.5) body: V // 2 at 60 (banned
    by the full rules), H at 48 (base count 1: 32.25, 28.25, 24.25 after one, two, three occurrences) and fourteen more from 28.0 down in steps of 0.25 (17.0 or less
    once counted, base count 0): H, H, then the peaks in order -- if column i counts exactly the drafts in front of it.  The peaks sit on entry 0, on V - 1 (at
    V = 1001 in the group that crosses V), on the last entry of one lane's range and the first of the next."""
    per = ((-(-V // 1024)) + 7) & ~7
    peaks, H = [0, V - 1, 50 * per - 1, 50 * per] + [97 + 61 * k for k in range(10)], 700
    rows = orc.f32_to_bf16(np.random.default_rng(20261126 + V).normal(0.0, 1.5, size=(W, V)).astype(np.float32))
    rows[:, V // 2], rows[:, H] = sr.bf(60.0), sr.bf(48.0)
    for k, j in enumerate(peaks):
        rows[:, j] = sr.bf(28.0 - 0.25 * k)
    return rows, hist([CUR, H, 11, 11, 12, 13], V), [H, H] + peaks


def true_chain(rows, smp, rules, base):
    """g[i] = column i's token when every draft in front of it was right (the table plus g[:i]): what the rules loop emits"""
    g = []
    for i in range(W):
        g.append(lr.sample(rows[i], smp, rules, base + hist(g, base.size), POS0 + i)[0])
    return g


def columns(g, a, V):
    """column inputs whose accepted prefix is a: the true chain up to column a, wrong at a + 1"""
    col = [CUR] + [int(t) for t in g[:-1]]
    if a + 1 < len(col):
        col[a + 1] = (col[a + 1] + 1) % V
    return col


def emitted(g, a, base, stops=()):
    """-> (tokens, finished, the table after the commit)"""
    out = [int(t) for t in g[:a + 1]]
    cut = [i for i, t in enumerate(out) if t in stops]
    out = out[:cut[0] + 1] if cut else out
    return out, bool(cut), base + hist(out, base.size)


@pytest.mark.parametrize("V", [1001, 1024, 128256])
def test_bare_rows_tell_a_kernel_that_miscounts_the_drafts(V):
    rows, base, want = bare(V)
    smp, rules = SAMPLERS["t0"], full_rules(V)
    g = true_chain(rows, smp, rules, base)
    assert g == want and base[g[0]] > 0 and base[g[2]] == 0 and g[0] == g[1]           # the chain is accepted; a drafted token the table knows, one it does not, one twice
    for table in (base, base + hist(g[:W - 1], V)):                                  # a kernel that ignores the deltas; one that gives every column the whole draft
        assert sum(lr.sample(rows[i], smp, rules, table, POS0 + i)[0] != g[i] for i in range(W)) >= 3


_CHAINS = {}


def rules_chain(smp, rules):
    """oracle one-token step, logit_rules_ref.sample over prompt ++ first ++ emitted, feed the token -> (first, what lnb_decode_sample_rules_until must emit)"""
    if (smp, rules) not in _CHAINS:
        cfg, prompt, _ = ss.tiny_chains()
        om = orc.Model(**cfg).fill_synthetic(ss.MODEL_SEED).finalize()
        c = orc.Context(om, ss.SEQ, 1)
        _, first = c.forward(prompt, 0)
        counts, toks = hist(list(prompt) + [int(first)], cfg["vocab_size"]), [int(first)]
        for i in range(ss.STEPS):
            row, _ = c.forward(np.array(toks[-1:], dtype=np.int32), ss.P0 + i)
            toks.append(int(lr.sample(orc.f32_to_bf16(np.ascontiguousarray(row[-1], dtype=np.float32)), smp, rules, counts, ss.P0 + i)[0]))
            counts[toks[-1]] += 1
        c.close(); om.close()
        _CHAINS[(smp, rules)] = (toks[0], np.array(toks[1:], dtype=np.int32))
    return _CHAINS[(smp, rules)]


def corpus(kind, chain, V):
    """the true continuation, or the same with every 8th token wrong"""
    c = np.array(chain, dtype=np.int32).copy()
    if kind == "every8":
        c[7::8] = (c[7::8] + 1) % V
    return c


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_tiny_chains_move_under_the_rules_and_drafts_are_accepted_and_rejected(name):
    cfg, prompt, _ = ss.tiny_chains()
    V, smp = cfg["vocab_size"], SAMPLERS[name]
    first, want = rules_chain(smp, full_rules(V))
    assert (want != rules_chain(smp, lr.OFF)[1]).any()                          # the rules move the chain
    for md in (3, 15):
        st = {k: ss.simulate(prompt, first, want, corpus(k, [first] + list(want), V), ss.NMIN, ss.NMAX, md, ss.STEPS, ss.SEQ, ss.P0) for k in ("exact", "every8")}
        assert st["exact"]["accepted"] >= 10 and st["every8"]["accepted"] > 0 and st["every8"]["drafted"] - st["every8"]["accepted"] >= 3      # (rejected drafts: counting them diverges)


def test_the_delta_count_equals_bumping_the_table(tmp_path):
    exe, src = str(tmp_path / "spec_rules_test"), os.path.join(ROOT, "tests", "native", "spec_rules_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "spec_rules_test: ok" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


def test_exports_and_refusals_before_any_handle_is_touched():
    """the argument checks of the three entry points come before a handle is dereferenced: the context handles here are poison"""
    import lnb
    lnb.build()
    L, hdr = lnb.lib(), open(os.path.join(ROOT, "include", "lnb.h")).read()
    for n in ("lnb_decode_speculative_sample_rules_until", "lnb_decode_speculative_sample_rules_many", "lnb_op_spec_sample_rules_accept"):
        assert n in lnb.EXPORTS and "int %s(" % n in hdr, n
    assert "a verify pass would need per-column count deltas" not in hdr
    good, off, i32 = lnb.Sampler(0.7, 40, 0.9, 1), lnb.LogitRules(), ctypes.c_int32
    out, n, fin, one = (i32 * 8)(), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_void_p * 1

    def until(match, sampler=good, rules=off, counted=None, n_counted=0):
        rc = L.lnb_decode_speculative_sample_rules_until(0x10, sampler, rules, counted, n_counted, None, 0, 1, 8, 8, out, ctypes.byref(n), ctypes.byref(fin), None, None)
        assert rc != 0 and match in L.lnb_last_error().decode(), (match, L.lnb_last_error())

    def many(match, samplers=good, rules=off, counted=one(None), n_counted=(i32 * 1)(0), n_ctx=1):
        rc = L.lnb_decode_speculative_sample_rules_many(one(0x10), n_ctx, samplers, rules, counted, n_counted, one(None), (i32 * 1)(0), (i32 * 1)(1), (i32 * 1)(8), 8, 0, out,
                                                        ctypes.byref(n), ctypes.byref(fin), None, None, None)
        assert rc != 0 and match in L.lnb_last_error().decode(), (match, L.lnb_last_error())

    bad = [(lnb.LogitRules(0.0), "repetition_penalty"), (lnb.LogitRules(1.0, float("inf")), "presence_penalty"), (lnb.LogitRules(1.0, 0.0, float("nan")), "frequency_penalty"),
           (lnb.LogitRules(1.0, 0.0, 0.0, 1.5), "min_p"), (lnb.LogitRules(bias={-1: 1.0}), "bias id"), (lnb.LogitRules(bias={4: float("nan")}), "bias value")]
    for f in (until, many):
        for kw, word in [(dict(rules=r), w) for r, w in bad] + [(dict(rules=None), "rules"), (dict(n_counted=-1 if f is until else (i32 * 1)(-1)), "n_counted")]:
            f(word, **kw)
    until("sampler", sampler=None); until("temperature", sampler=lnb.Sampler(-1.0, 0, 1.0, 0)); until("counted id", counted=(i32 * 2)(1, -5), n_counted=2)
    many("samplers", samplers=None); many("counted", counted=None); many("top_p", samplers=lnb.Sampler(1.0, 0, 0.0, 0)); many("1..128", n_ctx=0)
    z = np.zeros((2, 64), dtype=np.uint16)
    for args, word in [((z, good, r, None, 0, [1, 2]), w) for r, w in bad] + [((z, good, off, None, 0, [1, 64]), "column token"), ((z, good, off, None, -1, [1, 2]), "pos0"),
                                                                              ((np.zeros((17, 64), dtype=np.uint16), good, off, None, 0, list(range(17))), "1..16 columns")]:
        with pytest.raises(lnb.LnbError, match=word):
            lnb.op_spec_sample_rules_accept(*args)
