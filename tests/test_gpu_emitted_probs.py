"""The emitted token's record on the MI355X (include/lnb.h: lnb_ctx_set_emitted_probs): tok_prob and the top k are the bits of the oracle's orc_softmax_f32 on
the step's RAW logits row, w_tok / w_kept are tests/sampler_ref.py's integers, the sampling loops' records are their rows' records, the speculative loops'
records are the sampling loop's bit for bit, and with the switch off nothing of it runs."""
import numpy as np
import pytest

from form_tally import ran, count
from oracle import oracle as orc
import sampler_ref as sr
import spec_sim as ss
from test_gpu_token_probs import lnb, orc_softmax, serial_ln_z, check_records, same_bits, _special_rows  # noqa: F401 (lnb: the module fixture)

pytestmark = pytest.mark.gpu
P0, SEQ, NMIN, NMAX, STEPS, K = ss.P0, ss.SEQ, ss.NMIN, ss.NMAX, 24, 5
GREEDY = (0.0, 0, 1.0)
SAMPLERS = (ss.SAMPLERS[0], ss.SAMPLERS[1], GREEDY)
SEEDS = {**ss.SEEDS, GREEDY: 5}
FIELDS = ("tok_logit", "tok_prob", "log_z", "w_tok", "w_kept", "ids", "logits", "probs")


def same_records(a, b, n=None):
    return all(np.array_equal(a[f][:n].view(np.uint8), b[f][:n].view(np.uint8)) for f in FIELDS)


def weights_of(row_u16, sampler, tok, u=None, pos=0):
    """(w_tok, w_kept) of sampler_ref for the token it picks on this row (0, 0: greedy, degenerate, no candidate)"""
    prep = sr.prepare(row_u16, *sampler[:3])
    assert sr.pick(prep, sr.draw(sampler[3], pos) if u is None else u) == tok
    if prep[0] is not None:
        return 0, 0
    _, ks, cs, info = prep
    i = int(np.nonzero(ks == tok)[0][0])
    return int(cs[i]) - (int(cs[i - 1]) if i else 0), info["w_kept"]


def check_emitted(row_u16, rec, i, tok, k):
    f = orc.bf16_to_f32(row_u16)                            # record i of rec against the oracle on its raw row
    ref = orc_softmax(f[None, :])[0]
    check_records(f, rec["ids"][i], rec["logits"][i], rec["probs"][i], k, ref)
    if tok < 0:
        assert np.isnan(rec["tok_logit"][i]) and np.isnan(rec["tok_prob"][i]) and rec["w_tok"][i] == 0 and rec["w_kept"][i] == 0
    else:
        assert same_bits(rec["tok_logit"][i], f[tok]) and same_bits(rec["tok_prob"][i], ref[tok]), (i, tok, rec["tok_prob"][i], ref[tok])
    lz = serial_ln_z(row_u16[None, :])[0]
    assert abs(rec["log_z"][i] - lz) <= (row_u16.size + 8) * 2.0 ** -52 if np.isfinite(lz) else same_bits(np.float32(rec["log_z"][i]), np.float32(lz))


@pytest.mark.parametrize("force_serial", [0, 1])
@pytest.mark.parametrize("V", [1001, 128256])
def test_op_against_the_oracle(lnb, V, force_serial):
    sp = _special_rows(V)                                    # 2: all NaN, 5: Z = +inf, 7: one dominant value, 8: every exp underflows
    g = sr.llama_like_rows(np.random.default_rng(11), 4, V)
    under = orc.f32_to_bf16(np.concatenate([[0.0, -95.0, -120.0], np.full(V - 3, -30.0)]).astype(np.float32))       # e^-95 / Z: an f32 denormal, e^-120 / Z: 0
    none = orc.f32_to_bf16(np.full(V, -np.inf, dtype=np.float32))                                                   # no candidate: token -1
    rows = np.stack([g[0], g[1], g[2], g[3], sp[2], sp[5], sp[7], sp[8], none])
    smp = [(1.0, 0, 1.0, 3), (0.7, 40, 0.9, 4), (1.5, 0, 0.5, 5), GREEDY + (0,), (1.0, 0, 1.0, 6), (1.0, 0, 1.0, 7), (1.0, 0, 1.0, 8), (1.0, 0, 1.0, 9), (1.0, 0, 1.0, 10)]
    draws = [sr.draw(s[3], 20 + i) for i, s in enumerate(smp)]
    with ran(lnb, ("emit.summary", "emit.row"), not_ran=("sample", "emit.batch", "emit.spec")):
        r = lnb.op_emitted_probs(rows, K, smp, [0] * len(smp), draws=draws, force_serial=bool(force_serial))
    assert not force_serial or r["serial_walks"] >= len(smp)
    assert r["tokens"][4] == -1 and r["tokens"][8] == -1 and r["tokens"][3] == lnb.op_argmax(rows[3])
    for i, s in enumerate(smp):
        tok = int(r["tokens"][i])
        check_emitted(rows[i], r, i, tok, K)
        assert (int(r["w_tok"][i]), int(r["w_kept"][i])) == weights_of(rows[i], s, tok, u=draws[i]), i
    # Under rules the token is the ADJUSTED row's and the record the RAW row's.  Row 0: the argmax banned (entry 0 of the top k is the banned token).  A token of
    # weight >= 1 has a probability above 2^-45 / V on the row it is sampled from, so an f32-denormal or zero tok_prob needs a bias: +200 on the entries at -95 / -120
    # Row 3: the same ban at temperature 0 -- the argmax of the adjusted row, both weights 0.
    a = lnb.op_argmax(g[0])
    rrows = np.stack([g[0], under, under, g[0]])
    bias = [{a: -np.inf}, {1: 200.0}, {2: 200.0}, {a: -np.inf}]
    q = lnb.op_emitted_probs(rrows, K, smp[:4], [0] * 4, draws=draws[:4], rules=[lnb.LogitRules(bias=b) for b in bias], force_serial=bool(force_serial))
    f8 = orc_softmax(orc.bf16_to_f32(under)[None, :])[0]
    assert 0 < f8[1] < 2.0 ** -126 and f8[2] == 0            # the denormal and the zero are really there
    assert q["tokens"][0] != a and q["ids"][0, 0] == a and q["tokens"][1] == 1 and q["tokens"][2] == 2 and q["tokens"][3] != a and q["w_kept"][3] == 0
    for i in range(4):
        adj = orc.bf16_to_f32(rrows[i])
        for j, v in bias[i].items():
            adj[j] += np.float32(v)
        check_emitted(rrows[i], q, i, int(q["tokens"][i]), K)
        assert (int(q["w_tok"][i]), int(q["w_kept"][i])) == weights_of(orc.f32_to_bf16(adj), smp[i], int(q["tokens"][i]), u=draws[i]), i


@pytest.fixture(scope="module")
def tiny(lnb):
    cfg = dict(orc.TINY)
    models = {form: lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(ss.MODEL_SEED).finalize() for form in ("rows", "columns")}
    models["columns"].enable_batch()
    yield models, lnb.synth_tokens(ss.PROMPT_SEED, P0, cfg["vocab_size"]), cfg
    [gm.close() for gm in models.values()]


def rules_of(lnb, rules, more=()):                           # token 7 banned, repeats penalised; more: what a later chunk counts of the earlier chunks
    return dict(rules=lnb.LogitRules(1.3, 0.2, 0.1, 0.02, bias={7: -np.inf}), counted=[1, 2, 3] + list(more)) if rules else {}


def plain_run(lnb, tiny, smp, rules, stop=(), fresh=False, _kept={}):
    """decode_sample_until with records on a fresh context -> (first token, tokens, finished, records); without a stop id the run is kept unless `fresh`"""
    if not stop and not fresh and (smp, rules) in _kept:
        return _kept[(smp, rules)]
    models, prompt, cfg = tiny
    c = lnb.InferenceContext(models["rows"], SEQ)
    if stop:
        c.set_stop_ids(list(stop))
    _, f = c.Forward(prompt, 0, want_logits=False)
    c.set_emitted_probs(K)
    with ran(lnb, ("emit.summary", "emit.row"), not_ran=("sample", "emit.batch", "emit.spec")):
        got, fin, _ = c.decode_sample_until(smp + (SEEDS[smp],), f, P0, STEPS, **rules_of(lnb, rules))
    out = int(f), got, fin, c.read_emitted_probs()
    c.close()
    assert len(out[3]["tok_prob"]) == len(got)
    return out if stop or fresh else _kept.setdefault((smp, rules), out)


@pytest.mark.parametrize("rules", [False, True], ids=["plain", "rules"])
@pytest.mark.parametrize("smp", SAMPLERS, ids=["t1", "t07_k40_p09", "greedy"])
@pytest.mark.parametrize("graph", ["graph", "nograph"])
def test_loop_records_are_the_rows_records(lnb, tiny, graph, smp, rules, monkeypatch):
    if graph == "nograph":
        monkeypatch.setenv("LNB_NO_GRAPH", "1")
    models, prompt, cfg = tiny
    f, got, fin, rec = plain_run(lnb, tiny, smp, rules, fresh=graph == "nograph")
    assert len(got) == STEPS and not fin
    # the loop's rows by the project's own contract: the emitted tokens teacher-forced through ForwardAppend on a second context
    c2 = lnb.InferenceContext(models["rows"], SEQ)
    c2.Forward(prompt, 0, want_logits=False)
    rows, _ = c2.ForwardAppend([f] + [int(t) for t in got[:-1]], P0)
    c2.close()
    for i in range(STEPS):
        check_emitted(orc.f32_to_bf16(rows[i]), rec, i, int(got[i]), K)
        if not rules:                                        # (sampler_ref has no rules: their integers are checked by the op test on an adjusted row)
            assert (int(rec["w_tok"][i]), int(rec["w_kept"][i])) == weights_of(orc.f32_to_bf16(rows[i]), smp + (SEEDS[smp],), int(got[i]), pos=P0 + i), i
    if smp == GREEDY:                                        # temperature 0, under rules too: both weights 0
        assert not rec["w_tok"].any() and not rec["w_kept"].any()
    # a stop id bounds the records: the stop token is the last one recorded
    stop = int(got[5])
    n = int(np.nonzero(got == stop)[0][0]) + 1
    _, g2, fin2, rec2 = plain_run(lnb, tiny, smp, rules, stop=(stop,))
    assert fin2 and len(g2) == n and same_records(rec2, rec, n)


def test_batch_members_record_their_own_runs(lnb, tiny):
    models, prompt, cfg = tiny
    ctxs = [lnb.InferenceContext(models["columns"], SEQ).set_emitted_probs(K) for _ in SAMPLERS]
    firsts = [c.Forward(prompt, 0, want_logits=False)[1] for c in ctxs]
    b = lnb.Batch(ctxs)
    with ran(lnb, ("emit.summary", "emit.batch"), not_ran=("sample", "emit.row", "emit.spec")):
        outs = b.decode_sample_until([s + (SEEDS[s],) for s in SAMPLERS], firsts, [P0] * 3, STEPS)[0]
    for s, smp in enumerate(SAMPLERS):
        f, got, _, rec = plain_run(lnb, tiny, smp, False)
        assert (outs[s] == got).all() and same_records(ctxs[s].read_emitted_probs(), rec), smp
    b.close()
    [c.close() for c in ctxs]


@pytest.mark.parametrize("md,kind,chunks", [(0, "exact", 1), (3, "exact", 1), (15, "exact", 1), (3, "none", 1), (15, "every2", 3), (3, "exact", 2)])
@pytest.mark.parametrize("mode", ["greedy", "sample", "rules"])
def test_speculative_records_equal_the_plain_loops(lnb, tiny, mode, md, kind, chunks):
    models, prompt, cfg = tiny
    smp, rules = (GREEDY if mode == "greedy" else ss.SAMPLERS[1]), mode == "rules"
    f, want, _, rec = plain_run(lnb, tiny, smp, rules)
    C = ss.corpus(kind, [f] + [int(t) for t in want], cfg["vocab_size"])
    c = lnb.InferenceContext(models["columns" if md != 3 else "rows"], SEQ).set_emitted_probs(K).set_draft(md, NMIN, NMAX, C)
    tok, hist, done, accepted = c.Forward(prompt, 0, want_logits=False)[1], [int(t) for t in prompt], 0, 0
    for ch in range(chunks):
        steps = STEPS // chunks if ch < chunks - 1 else STEPS - done        # (below: the tally counts a graph's launches once, at its capture -- the first chunk's)
        with ran(lnb, ("emit.summary", "emit.spec") if ch == 0 and md and kind == "exact" else (), not_ran=("sample", "emit.batch")):
            if mode == "greedy":
                got, fin, st, _ = c.decode_speculative_until(hist, tok, P0 + done, steps)
            else:
                got, fin, st, _ = c.decode_speculative_sample_until(smp + (SEEDS[smp],), hist, tok, P0 + done, steps, **rules_of(lnb, rules, hist[P0:]))
        assert (got == want[done:done + steps]).all() and same_records(c.read_emitted_probs(), {x: rec[x][done:done + steps] for x in FIELDS}), (ch, st)
        hist += [tok] + [int(t) for t in got[:-1]]; tok = int(got[-1]); done += steps; accepted += st["accepted"]
    assert accepted > 0 or not (md and kind == "exact")      # accepted columns really were recorded
    c.close()


@pytest.mark.parametrize("draft", [None, (3, NMIN, NMAX)])
def test_the_engine_returns_the_records_with_the_tokens(lnb, tiny, draft):
    (models, prompt, cfg), smp = tiny, SAMPLERS[1]
    out, r = lnb.InferenceEngine(models["rows"], SEQ, sampler=smp + (SEEDS[smp],), draft=draft, emitted_probs=K).GenerateTokens(prompt, max_new=8)
    c2 = lnb.InferenceContext(models["rows"], SEQ)           # record 0 is the prompt's last row, the others the rows of the tokens before them
    c2.Forward(prompt, 0, want_logits=False)
    rows = np.concatenate([c2.ForwardAppend(prompt[-1:], P0 - 1)[0], c2.ForwardAppend(out[:-1], P0)[0]])
    c2.close()
    assert len(out) == 8 and all(len(r[x]) == 8 for x in FIELDS)
    for i, t in enumerate(out):
        check_emitted(orc.f32_to_bf16(rows[i]), r, i, t, K)
        assert (int(r["w_tok"][i]), int(r["w_kept"][i])) == weights_of(orc.f32_to_bf16(rows[i]), smp + (SEEDS[smp],), t, pos=P0 - 1 + i), i


def test_switches_and_refusals(lnb, tiny):
    models, prompt, cfg = tiny
    smp = ss.SAMPLERS[0] + (1,)
    c = lnb.InferenceContext(models["columns"], SEQ)
    _, f = c.Forward(prompt, 0, want_logits=False)
    lnb.form_count_reset()
    off, _, _ = c.decode_sample_until(smp, f, P0, 8)         # the switch off: none of the new forms
    assert count(lnb, "emit") == 0 and count(lnb, "sample.row") > 0
    with pytest.raises(lnb.LnbError, match="lnb_ctx_set_emitted_probs"):
        c.read_emitted_probs(1)
    c.set_token_probs(2)
    with pytest.raises(lnb.LnbError, match="exclude each other"):
        c.set_emitted_probs(0)
    c.set_token_probs(0).set_emitted_probs(0)
    with pytest.raises(lnb.LnbError, match="exclude each other"):
        c.set_token_probs(2)
    d = lnb.InferenceContext(models["columns"], SEQ)
    with pytest.raises(lnb.LnbError, match="lnb_ctx_set_emitted_probs"):
        lnb.Batch([c, d])                                    # one value for all members
    b = lnb.Batch([c])
    refused = [lambda: c.decode_greedy(f, P0, 4), lambda: c.decode_greedy_until(f, P0, 4), lambda: lnb.ForwardAppendMany([c], [[f]], [P0]),
               lambda: lnb.DecodeSpeculativeMany([c], [prompt], [f], [P0], 4), lambda: b.decode_until([f], [P0], 4),
               lambda: lnb.DecodeSpeculativeSampleMany([c], [smp], [prompt], [f], [P0], 4),
               lambda: lnb.DecodeSpeculativeSampleMany([c], [smp], [prompt], [f], [P0], 4, rules=[None], counted=[[1]])]
    for call in refused:
        with pytest.raises(lnb.LnbError, match="lnb_ctx_set_emitted_probs"):
            call()
    b.close()
    on, _, _ = c.decode_sample_until(smp, f, P0, 8)          # top_k 0: the token's own fields alone
    r = c.read_emitted_probs(8)
    assert (on == off).all() and r["ids"].shape == (8, 0) and np.isfinite(r["tok_prob"]).all()
    c.set_emitted_probs(-1)
    lnb.form_count_reset()
    again, _, _ = c.decode_sample_until(smp, f, P0, 8)
    assert (again == off).all() and count(lnb, "emit") == 0
    c.close(); d.close()
