"""The one-token gate|up launch from the 13-bit planar weight copy (gemv_chain_pk_kernel, csrc/lnb_wpack.h) against the raw kernel on the same weights
and against the oracle, bit for bit, at the smallest shapes at which the packed path can go wrong: two, three and four stages (dim 256 / 384 / 512; 264 =
a last stage that is mostly padding), one and two 56-row blocks and a partial last block; gaussian weights, rows of +-0, weights at both ends of the
window, and a matrix the format must refuse -- which has to say so and still compute the oracle's result."""
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


def oracle_gate_up(x, nw, w1, w3):
    """RMSNorm -> w1, w3 -> trunc(SiLU table) * up, truncated (oracle/lnb_oracle.c ffn_forward)"""
    L = orc.lib()
    k = x.shape[0]
    xn = np.zeros((1, k), dtype=np.uint16)
    L.orc_rmsnorm_bf16(orc._p(x.reshape(1, k)), orc._p(nw), orc._p(xn), 1, k, EPS, None)
    g = np.zeros((1, w1.shape[0]), dtype=np.uint16); u = np.zeros_like(g)
    L.orc_linear_bf16(orc._p(xn), orc._p(w1), orc._p(g), 1, w1.shape[0], k, 4)
    L.orc_linear_bf16(orc._p(xn), orc._p(w3), orc._p(u), 1, w3.shape[0], k, 4)
    import ctypes as C
    L.orc_silu_table.restype = C.POINTER(C.c_float)
    silu = np.ctypeslib.as_array(L.orc_silu_table(), shape=(1 << 16,))
    gs = orc.bf16_to_f32(bf(silu[g[0]]))
    return bf(gs * orc.bf16_to_f32(u[0]))


def weights(kind, n, k, rng):
    """(w1, w3, expected status)"""
    w1 = bf(rng.standard_normal((n, k)) * 0.05); w3 = bf(rng.standard_normal((n, k)) * 0.05)
    if kind == "gaussian":
        return w1, w3, OK
    if kind == "zeros":                     # whole rows and scattered elements of +0 and -0 (code 0 beside every other code)
        w1[::5] = 0x0000; w3[1::7] = 0x8000
        w1[rng.random((n, k)) < 0.1] = 0x8000; w3[rng.random((n, k)) < 0.1] = 0x0000
        return w1, w3, OK
    if kind == "edges":                     # every weight in the lowest or the highest binade pair of a full window: codes 1 and 15, both exponent parities
        lo = 48                             # (exponents 96 / 97 and 124 / 125: 2^-31 .. 2^-2, so that no sum overflows)
        e = np.where(rng.random((2, n, k)) < 0.5, 2 * lo, 2 * (lo + 14)) + rng.integers(0, 2, (2, n, k))
        w = ((rng.integers(0, 2, (2, n, k)) << 15) | (e << 7) | rng.integers(0, 128, (2, n, k))).astype(np.uint16)
        return w[0], w[1], OK
    if kind == "refused_window":            # one weight one step below what a window ending at the largest weight admits
        e2 = (np.concatenate([w1.ravel(), w3.ravel()]) >> 8) & 0x7F
        assert e2.min() > e2.max() - 15
        w3[n - 1, k - 1] = ((2 * (int(e2.max()) - 15) + 1) << 7) | 5
        return w1, w3, WINDOW
    if kind == "refused_subnormal":
        w3[n // 2, k // 2] = 0x0003
        return w1, w3, SUBNORMAL
    raise ValueError(kind)


SHAPES = [(56, 256), (112, 512), (100, 384), (56, 264), (130, 512)]     # (row pairs, dim): one block / two / a partial last block / padded last stage / three blocks, the last partial


@pytest.mark.parametrize("kind", ["gaussian", "zeros", "edges", "refused_window", "refused_subnormal"])
@pytest.mark.parametrize("n,k", SHAPES)
def test_packed_gate_up_is_the_raw_kernel_and_the_oracle_bit_for_bit(lnb, n, k, kind):
    rng = np.random.default_rng(n * 1000 + k + len(kind))
    x = bf(rng.standard_normal(k) * 2.0)
    nw = bf(1 + 0.1 * rng.standard_normal(k))
    w1, w3, want = weights(kind, n, k, rng)
    with ran(lnb, "gemv_chain.rw56", epi="silu_mul", not_ran=("gemv_chain_pk",)):
        y_raw, st_raw = lnb.op_rmsnorm_gate_up(x, nw, EPS, w1, w3, packed=0)
    # a packable matrix runs the packed kernel when asked; a refused one keeps the raw kernel
    with ran(lnb, "gemv_chain_pk" if want == 0 else "gemv_chain.rw56", epi="silu_mul", not_ran=("gemv_chain.rw56" if want == 0 else "gemv_chain_pk",)):
        y_pk, st_pk = lnb.op_rmsnorm_gate_up(x, nw, EPS, w1, w3, packed=1)
    ref = oracle_gate_up(x, nw, w1, w3)
    assert st_pk == want == st_raw                          # a refused matrix is reported, with its reason
    assert (y_raw == ref).all()
    assert (y_pk == ref).all(), (kind, n, k, int((y_pk != ref).sum()))


def test_model_reports_what_it_packed_and_decodes_the_same_tokens(lnb, monkeypatch):
    """a model whose gate|up matrices take the 56-row layout: the copy is built at finalize and reported, the knob turns it off, a refused layer is
    counted with its reason, and greedy decode gives the same tokens in all three"""
    import ctypes as C
    F = 56 * lnb.device_info(0)["n_cus"]          # the shape that takes the 56-row layout: one block per CU
    cfg = dict(lnb.LLAMA_8B, dim=256, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, multiple_of=F, ffn_dim_multiplier=1.0, max_seq_len=64)
    assert lnb.lib().lnb_model_ffn_hidden_dim(C.byref(lnb.ModelArgs(**cfg))) == F
    prompt = lnb.synth_tokens(5, 8, cfg["vocab_size"])

    def run(mutate=None):
        m = lnb.LlamaTransformer(**cfg).fill_synthetic(11)
        if mutate:
            mutate(m)
        m.finalize()
        c = lnb.InferenceContext(m, 64)
        _, first = c.Forward(prompt, 0, want_logits=False)
        toks, _ = c.decode_greedy(first, 8, 12)
        info, nbytes = m.wpack_info(), m.wpack_bytes()
        c.close(); m.close()
        return [first] + [int(t) for t in toks], info, nbytes

    monkeypatch.setenv("LNB_W13_PACKED", "1")
    t_pk, info, nbytes = run()
    assert info["packed"] == 2 and sum(info.values()) == 2 and nbytes == 2 * (2 * F * 256 * 2) * 13 // 16
    monkeypatch.setenv("LNB_W13_PACKED", "0")
    t_raw, info0, nbytes0 = run()
    monkeypatch.setenv("LNB_W13_PACKED", "1")
    assert info0["packed"] == 0 and info0["not_tried"] == 2 and nbytes0 == 0

    def poison(m):
        w = m.get_tensor("layers.1.feed_forward.w3.weight", F * 256)
        w[3 * 256 + 7] = 0x0001                             # a subnormal: layer 1 must keep the raw kernel
        m.set_tensor("layers.1.feed_forward.w3.weight", w, shape=(F, 256))

    t_ref, info1, nbytes1 = run(poison)
    assert info1["packed"] == 1 and info1["subnormal"] == 1 and nbytes1 == nbytes // 2
    assert t_pk == t_raw
    monkeypatch.setenv("LNB_W13_PACKED", "0")
    t_ref0, _, _ = run(poison)
    assert t_ref == t_ref0
