"""The one-token LM head from its 13-bit planar weight copy (the gemv_head_pk form: gemv_chain_pk_kernel on 128-row blocks as two chains of 64 rows,
csrc/lnb_wpack.h) against the raw 64-row kernel on the same weights and against the oracle, bit for bit.

Through lnb_op_rmsnorm_head, at the smallest shapes at which the packed path can go wrong: one stage (K 128), two (256), a last stage that is mostly padding
(264), more stages than ring slots so that every slot is refilled (896); chain 1 entirely past the end (N 64), one row into it (65), a whole block (128),
a second, partial block (130), and six blocks on two workgroups with the last one partial (641, n_wg = 2: persistence over blocks).  Weight kinds as for
the gate|up copy: gaussian, rows and scattered elements of +-0, both ends of a full window, and matrices the format must refuse -- which have to say so,
run the raw form and still compute the oracle's result.

Through one small model whose vocabulary gives every CU a 128-row block: the copy is built at finalize and reported, LNB_HEAD_PACKED turns it off, greedy
decode and the logits of a one-row Forward are the same bits either way and the oracle's, multi-row calls and the throughput schedule keep the raw form,
a poisoned or a small head is reported as such, and the gate|up queries do not count the head."""
import numpy as np
import pytest

from form_tally import ran

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

EPS = np.float32(1e-5)
OK, SUBNORMAL, INFNAN, WINDOW = 0, 1, 2, 3


def bf(a):
    return orc.f32_to_bf16(np.asarray(a, dtype=np.float32))


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    return _lnb


def oracle_head(x, nw, w):
    """RMSNorm -> output projection, truncated (oracle/lnb_oracle.c)"""
    L = orc.lib()
    k = x.shape[0]
    xn = np.zeros((1, k), dtype=np.uint16)
    L.orc_rmsnorm_bf16(orc._p(x.reshape(1, k)), orc._p(nw), orc._p(xn), 1, k, EPS, None)
    y = np.zeros((1, w.shape[0]), dtype=np.uint16)
    L.orc_linear_bf16(orc._p(xn), orc._p(w), orc._p(y), 1, w.shape[0], k, 4)
    return y[0]


def weights(kind, n, k, rng):
    """(w, expected status)"""
    w = bf(rng.standard_normal((n, k)) * 0.05)
    if kind == "gaussian":
        return w, OK
    if kind == "zeros":                     # whole rows and scattered elements of +0 and -0 (code 0 beside every other code)
        w[::5] = 0x0000; w[1::7] = 0x8000
        w[rng.random((n, k)) < 0.1] = 0x8000; w[rng.random((n, k)) < 0.1] = 0x0000
        return w, OK
    if kind == "edges":                     # every weight in the lowest or the highest binade pair of a full window: codes 1 and 15, both exponent parities
        lo = 48                             # (exponents 96 / 97 and 124 / 125: 2^-31 .. 2^-2, so that no sum overflows)
        e = np.where(rng.random((n, k)) < 0.5, 2 * lo, 2 * (lo + 14)) + rng.integers(0, 2, (n, k))
        return ((rng.integers(0, 2, (n, k)) << 15) | (e << 7) | rng.integers(0, 128, (n, k))).astype(np.uint16), OK
    if kind == "refused_window":            # one weight one step below what a window ending at the largest weight admits
        e2 = (w.ravel() >> 8) & 0x7F
        assert e2.min() > e2.max() - 15
        w[n - 1, k - 1] = ((2 * (int(e2.max()) - 15) + 1) << 7) | 5
        return w, WINDOW
    if kind == "refused_subnormal":
        w[n // 2, k // 2] = 0x0003
        return w, SUBNORMAL
    raise ValueError(kind)


# (rows, dim, workgroup cap)
SHAPES = [(n, k, 0) for k in (128, 256, 264, 896) for n in (64, 65, 128, 130)] + [(641, 256, 2), (641, 896, 2)]


@pytest.mark.parametrize("kind", ["gaussian", "zeros", "edges", "refused_window", "refused_subnormal"])
@pytest.mark.parametrize("n,k,n_wg", SHAPES)
def test_packed_head_is_the_raw_kernel_and_the_oracle_bit_for_bit(lnb, n, k, n_wg, kind):
    rng = np.random.default_rng(n * 1000 + k + len(kind))
    x = bf(rng.standard_normal(k) * 2.0)
    nw = bf(1 + 0.1 * rng.standard_normal(k))
    w, want = weights(kind, n, k, rng)
    with ran(lnb, "gemv_chain.rw64", epi="store", not_ran=("gemv_head_pk", "gemv_chain_pk")):
        y_raw, st_raw = lnb.op_rmsnorm_head(x, nw, EPS, w, packed=0, n_wg=n_wg)
    # a packable matrix runs the packed form when asked; a refused one keeps the raw kernel
    with ran(lnb, "gemv_head_pk" if want == 0 else "gemv_chain.rw64", epi="store", not_ran=("gemv_chain.rw64" if want == 0 else "gemv_head_pk", "gemv_chain_pk")):
        y_pk, st_pk = lnb.op_rmsnorm_head(x, nw, EPS, w, packed=1, n_wg=n_wg)
    ref = oracle_head(x, nw, w)
    assert st_pk == want == st_raw                          # a refused matrix is reported, with its reason
    assert (y_raw == ref).all()
    assert (y_pk == ref).all(), (kind, n, k, int((y_pk != ref).sum()))


@pytest.fixture(scope="module")
def model_runs(lnb):
    """the model of the cases below, run once per setting; the oracle once"""
    import os
    V = 128 * lnb.device_info(0)["n_cus"]           # the smallest vocabulary the packed head takes: one 128-row block per CU
    cfg = dict(lnb.LLAMA_8B, dim=256, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=V, multiple_of=64, max_seq_len=64)
    prompt = lnb.synth_tokens(5, 8, V)
    seven = lnb.synth_tokens(6, 7, V)

    def poison(m):
        w = m.get_tensor("output.weight", V * 256)
        w[3 * 256 + 7] = 0x0001                             # a subnormal: the head must keep the raw kernel
        m.set_tensor("output.weight", w, shape=(V, 256))

    def run(knob, mutate=None, cfg=cfg):
        old = os.environ.get("LNB_HEAD_PACKED")
        os.environ["LNB_HEAD_PACKED"] = knob
        try:
            m = lnb.LlamaTransformer(**cfg).fill_synthetic(11)
            if mutate:
                mutate(m)
            m.finalize()
        finally:
            if old is None:
                del os.environ["LNB_HEAD_PACKED"]
            else:
                os.environ["LNB_HEAD_PACKED"] = old
        r = dict(status=m.wpack_head_status(), nbytes=m.wpack_head_bytes(), info=m.wpack_info(), w13_bytes=m.wpack_bytes())
        packed = r["status"] == "packed"
        raw_form = "gemv_chain.rw64" if cfg["vocab_size"] == V else "gemv_chain"      # (the 512-row head takes a thinner resident layout)
        head = "gemv_head_pk" if packed else raw_form
        other = raw_form if packed else "gemv_head_pk"
        c = lnb.InferenceContext(m, 64)
        _, first = c.Forward(prompt % cfg["vocab_size"], 0, want_logits=False)
        with ran(lnb, head, epi="store", not_ran=(other,)):                     # one eager row, with its logits
            lg, _ = c.Forward(np.array([first], dtype=np.int32), 8)
        with ran(lnb, head, epi="store", not_ran=(other,)):                     # the greedy loop (a capture counts once)
            toks, _ = c.decode_greedy(first, 8, 12)
        r.update(first=int(first), logits=lg.view(np.uint32).copy(), tokens=[int(t) for t in toks])
        if cfg["vocab_size"] == V and mutate is None:
            with ran(lnb, "gemv_chain.rw64", epi="store", not_ran=("gemv_head_pk",)):      # seven rows of logits: the raw 64-row kernel, one launch row each
                lg7, _ = c.Forward(seven, 14)                                       # (positions 14..20: everything in front of them has been written)
            c.set_schedule("throughput")
            with ran(lnb, "gemv_chain.rw64", epi="store", not_ran=("gemv_head_pk",)):      # the throughput schedule keeps the raw layouts
                lgt, _ = c.Forward(np.array([first], dtype=np.int32), 8)
            c.set_schedule("latency")
            r.update(logits7=lg7.view(np.uint32).copy(), logits_tp=lgt.view(np.uint32).copy())
        r["m"], r["c"] = m, c
        return r

    runs = {"pk": run("1"), "raw": run("0"), "poison_pk": run("1", poison), "poison_raw": run("0", poison),
            "small": run("1", cfg=dict(cfg, vocab_size=512))}
    om = orc.Model(**cfg).fill_synthetic(11).finalize()
    oc = orc.Context(om, 64)
    _, t = oc.forward(prompt, 0, want_logits=False)
    lo, _ = oc.forward(np.array([t], dtype=np.int32), 8)
    otoks, first = [], t
    for i in range(12):
        _, t = oc.forward(np.array([t], dtype=np.int32), 8 + i, want_logits=False)
        otoks.append(int(t))
    oc.close(); om.close()
    runs["oracle"] = dict(first=int(first), logits=lo.view(np.uint32).copy(), tokens=otoks)
    runs["V"] = V
    yield runs
    for k in ("pk", "raw", "poison_pk", "poison_raw", "small"):
        runs[k]["c"].close(); runs[k]["m"].close()


def test_model_reports_its_head_copy_and_the_knob_turns_it_off(model_runs):
    V = model_runs["V"]
    pk, raw = model_runs["pk"], model_runs["raw"]
    assert pk["status"] == "packed" and pk["nbytes"] == V * 256 * 2 * 13 // 16
    assert raw["status"] == "not_tried" and raw["nbytes"] == 0
    # the gate|up queries count gate|up matrices only: two layers, and nothing of the head's bytes
    for r in (pk, raw):
        assert sum(r["info"].values()) == 2
    assert pk["info"] == raw["info"] and pk["w13_bytes"] == raw["w13_bytes"]


def test_tokens_and_logits_are_the_raw_head_s_and_the_oracle_s(model_runs):
    pk, raw, o = model_runs["pk"], model_runs["raw"], model_runs["oracle"]
    assert pk["first"] == raw["first"] == o["first"]
    assert pk["tokens"] == raw["tokens"] == o["tokens"]
    assert (pk["logits"] == o["logits"]).all() and (raw["logits"] == o["logits"]).all()
    # rows the packed head never computes are the same bits with and without the copy
    assert (pk["logits7"] == raw["logits7"]).all() and (pk["logits_tp"] == o["logits"]).all() and (raw["logits_tp"] == o["logits"]).all()


def test_a_head_that_cannot_be_packed_says_why_and_decodes_the_same_tokens(model_runs):
    p1, p0, small = model_runs["poison_pk"], model_runs["poison_raw"], model_runs["small"]
    assert p1["status"] == "subnormal" and p1["nbytes"] == 0 and p0["status"] == "not_tried"
    assert p1["first"] == p0["first"] and p1["tokens"] == p0["tokens"] and (p1["logits"] == p0["logits"]).all()
    assert small["status"] == "not_tried" and small["nbytes"] == 0        # 512 rows: fewer than one 128-row block per CU


def test_rebinding_the_head_after_finalize_repacks_in_place_or_fails_loudly(lnb, model_runs):
    V, pk = model_runs["V"], model_runs["pk"]
    m, c = pk["m"], pk["c"]
    w = m.get_tensor("output.weight", V * 256)
    m.set_tensor("output.weight", w, shape=(V, 256))                          # the same weights again: inside the window, re-packed in place
    assert m.wpack_head_status() == "packed"
    with ran(lnb, "gemv_head_pk", epi="store", not_ran=("gemv_chain.rw64",)):
        lg, _ = c.Forward(np.array([pk["first"]], dtype=np.int32), 8)
    assert (lg.view(np.uint32) == pk["logits"]).all()
    bad = w.copy(); bad[5 * 256 + 1] = 0x7F80                                 # an Inf: the copy cannot hold it
    with pytest.raises(lnb.LnbError, match="13-bit copy"):
        m.set_tensor("output.weight", bad, shape=(V, 256))
    assert m.wpack_head_status() == "infnan"
    m.set_tensor("output.weight", w, shape=(V, 256))                          # the head stays raw from now on, with the good weights back
    with ran(lnb, "gemv_chain.rw64", epi="store", not_ran=("gemv_head_pk",)):
        lg, _ = c.Forward(np.array([pk["first"]], dtype=np.int32), 8)
    assert (lg.view(np.uint32) == pk["logits"]).all()
