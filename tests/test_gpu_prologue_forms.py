"""The decode kernels after their measurement code moved to instantiations of their own (-m gpu; profiles/prologue_fetch.md).

(a) every norm-fused form the launch layer can pick, through the operator entry points of the parity tests, against the oracle's bits -- at K = 8 (every rolled
    loop of the prologue runs once or not at all), 264 (ragged last unit: clamp and zero pad), 4096 (two x chunks per stager wave) and 8192 (the deeper chunk
    counts), each with one gaussian row and one row of tests/norm_craft.py (climb: leaves split at binade crossings between runs).  A K the launch function of
    a form refuses is refused with an error, and the set of refusals is fixed here.
(b) the wo / w2 form (rowcast_lds_kernel) at K = 1024 (two stages, the least it takes), 4096 and 14336, with 16 and 48 output rows.
(c) the TIMING instantiations against production's: on a two-layer cut of the tiny model a context whose classes 0, 2, 3, 4, 5 were stamped
    (lnb_profile_kernel_stamps) shows a chain wave (stamp 6 > 0) with stamps that rise in order, and then decodes the four greedy tokens and leaves the KV bits
    of a context that was never armed.
No tolerance anywhere: outputs are compared as bits."""
import ctypes as C

import numpy as np
import pytest

import norm_craft as nc
from form_tally import ran
from linear_cases import bf, orc_linear
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

EPS = 1e-5
K_NORM = (8, 264, 4096, 8192)
# form -> (launch tally row, epilogue, folding waves, output rows); the quad kernel walks whole 256-step stages, the packed head's two 64 KB product stages leave
# no room for 8192 f32 of x (lnbk_headp_supported refuses for the raw 64-row head of the same entry point too)
NORM_OPS = {"chain16": ("gemv_chain.rw16", "store", 2, 48), "chain32": ("gemv_chain.rw32", "store", 6, 96), "chain64": ("gemv_chain.rw64", "store", 6, 128),
            "quad24": ("gemv_quad", "store", 6, 48), "gate_up56": ("gemv_chain.rw56", "silu_mul", 7, 112), "gate_up56_packed": ("gemv_chain_pk", "silu_mul", 7, 112),
            "head64": ("gemv_chain.rw64", "store", 6, 200), "head_packed": ("gemv_head_pk", "store", 8, 200)}
REFUSED = {"quad24": {8, 264}, "head64": {8192}, "head_packed": {8192}}


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


_cases = {}


def norm_case(K, nh, n):
    """(x [2][K]: a gaussian row and a crafted one, norm weight, w [n][K], a second w, the oracle's normalised x), computed once and left unchanged"""
    if (K, nh, n) not in _cases:
        rng = np.random.default_rng(7 * K + nh + n)
        with np.errstate(over="ignore", invalid="ignore"):
            x = np.stack([bf(rng.standard_normal(K) * 3.0), nc.bf16_bits(nc.climb(rng, K, nh, 12))])
        nw = bf(1 + 0.1 * rng.standard_normal(K))
        w, w3 = bf(rng.standard_normal((n, K)) * 0.05), bf(rng.standard_normal((n, K)) * 0.05)
        xn = np.zeros_like(x)
        orc.lib().orc_rmsnorm_bf16(orc._p(x), orc._p(nw), orc._p(xn), 2, K, np.float32(EPS), None)
        for a in (x, nw, w, w3, xn):
            a.setflags(write=False)
        _cases[(K, nh, n)] = (x, nw, w, w3, xn)
    return _cases[(K, nh, n)]


def silu_mul(g, u):
    """trunc(SiLU table[gate]) * up, truncated (oracle/lnb_oracle.c ffn_forward)"""
    L = orc.lib()
    L.orc_silu_table.restype = C.POINTER(C.c_float)
    silu = np.ctypeslib.as_array(L.orc_silu_table(), shape=(1 << 16,))
    return bf(orc.bf16_to_f32(bf(silu[g])) * orc.bf16_to_f32(u))


def run_norm_form(lnb, form, x, nw, w, w3):
    """the operator of `form` on every row of x -> [rows][n]"""
    if form in ("chain16", "chain32", "chain64", "quad24"):
        return lnb.op_rmsnorm_linear(x, nw, EPS, w, rw={"chain16": 16, "chain32": 32, "chain64": 64, "quad24": 24}[form])
    out = []
    for row in x:
        if form.startswith("gate_up"):
            y, st = lnb.op_rmsnorm_gate_up(row, nw, EPS, w, w3, packed=int(form.endswith("packed")))
        else:
            y, st = lnb.op_rmsnorm_head(row, nw, EPS, w, packed=int(form.endswith("packed")))
        assert st == 0, (form, "the gaussian weights pack", st)
        out.append(y)
    return np.stack(out)


@pytest.mark.parametrize("K", K_NORM)
@pytest.mark.parametrize("form", sorted(NORM_OPS))
def test_norm_fused_forms_are_the_oracles_bits(lnb, form, K):
    tally, epi, nh, n = NORM_OPS[form]
    x, nw, w, w3, xn = norm_case(K, nh, n)
    if K in REFUSED.get(form, ()):
        with pytest.raises(lnb.LnbError):
            run_norm_form(lnb, form, x, nw, w, w3)
        return
    others = tuple(t for t in {v[0] for v in NORM_OPS.values()} if t != tally)
    with ran(lnb, tally, epi=epi, not_ran=others + ("rmsnorm_rows", "gemm_mfma", "gemm_stream")):
        y = run_norm_form(lnb, form, x, nw, w, w3)
    ref = silu_mul(orc_linear(xn, w), orc_linear(xn, w3)) if form.startswith("gate_up") else orc_linear(xn, w)
    bad = np.argwhere(y != ref)
    assert bad.size == 0, "%s K %d: %d outputs differ; first (row, col, got, oracle): %s" % (
        form, K, len(bad), [(int(i), int(j), hex(int(y[i, j])), hex(int(ref[i, j]))) for i, j in bad[:6]])


@pytest.mark.parametrize("n", [16, 48])
@pytest.mark.parametrize("K", [1024, 4096, 14336])
def test_wo_w2_form_is_the_oracles_bits(lnb, K, n):
    rng = np.random.default_rng(K + n)
    x = bf(np.stack([rng.standard_normal(K) * 2.0, rng.standard_normal(K) * 10.0 ** rng.uniform(-3, 3, K)]))
    w = bf(rng.standard_normal((n, K)) * 0.05)
    with ran(lnb, "rowcast_lds", epi="store", not_ran=("rowcast", "gemv_chain", "gemv_quad")):
        y = lnb.op_linear(x, w, rw=4)
    ref = orc_linear(x, w)
    bad = np.argwhere(y != ref)
    assert bad.size == 0, "K %d, %d rows: %d outputs differ; first (row, col, got, oracle): %s" % (
        K, n, len(bad), [(int(i), int(j), hex(int(y[i, j])), hex(int(ref[i, j]))) for i, j in bad[:6]])


def test_stamped_context_decodes_what_an_unarmed_one_does(lnb):
    cfg = dict(orc.TINY, n_layers=2)
    gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(1234).finalize()
    prompt = lnb.synth_tokens(99, 8, cfg["vocab_size"])

    def run(arm):
        c = lnb.InferenceContext(gm, 32)
        _, first = c.Forward(prompt, 0, want_logits=False)
        if arm:
            for which in (0, 2, 3, 4, 5):
                v, khz = c.profile_kernel_stamps(which, len(prompt))
                chain = [w for w in range(8) if v[w][0] > 0 and v[w][12] > 0]
                assert khz > 0 and chain, (which, "no wave reported stamp 6", v[:, 12].tolist())
                for w in chain:
                    s = [t for t in v[w][6:13] if t > 0]                    # stamps 0 .. 6 that this kernel sets (stamp 7 is the wall clock's)
                    assert s == sorted(s) and 0 < v[w][12] < v[w][1], (which, w, v[w].tolist())
        toks, _ = c.decode_greedy(first, len(prompt), 4)
        kv = [(c.CacheK(l).copy(), c.CacheV(l).copy()) for l in range(cfg["n_layers"])]
        c.close()
        return [first] + [int(t) for t in toks], kv

    t_ref, kv_ref = run(False)
    t_arm, kv_arm = run(True)
    gm.close()
    assert t_arm == t_ref
    for l, ((k0, v0), (k1, v1)) in enumerate(zip(kv_ref, kv_arm)):
        n = len(prompt) + 4
        assert (k0[:n] == k1[:n]).all() and (v0[:n] == v1[:n]).all(), "layer %d: the KV rows differ" % l
