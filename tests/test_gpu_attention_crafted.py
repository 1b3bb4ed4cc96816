"""Every attention kernel on crafted KV rows (-m gpu): tests/kv_craft.py writes the same hand-made K / V rows into a device context
(lnb_ctx_load_prefix) and into the oracle's cache, one call follows at position n_pos, and logits, argmax and the cache rows are compared with
the oracle bit for bit, NaN for NaN.  What the rows are and why the oracle's side can fail is tests/test_attention_crafted_cpu.py's business.

Forms: the one-token step (attn_exact_kernel, the long pair with both PV kernels, attn_one_kernel in a child process, each with the serial sums
forced), batched decode (plain, DENSE, attn_gqa_kernel, the batched long pair) with one case per member -- a NaN member beside finite ones --,
lnb_forward_append on the row kernel, the causal matrix-core kernels and the rows pair (every LNB_ATTN_ROWS_RPW in a child process), the
modulo-mask lnb_forward at start_pos > 0 on attn_mfma3_kernel / attn_mfma_kernel / attn_mfma2_kernel / the row kernel, speculative verify passes.
Then the poison token: a vocabulary id whose embedding row is NaN, inside multi-row calls."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kv_craft as kc
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")
same, same16 = kc.eq_or_both_nan_f32, kc.eq_or_both_nan_bf16


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    return _lnb


_GM = {}


def gpu_model(lnb, geometry):
    """one device model per geometry and module"""
    if geometry not in _GM:
        _GM[geometry] = lnb.LlamaTransformer(device=0, **kc.GEOMETRIES[geometry]).fill_synthetic(kc.SEED_MODEL).finalize().enable_batch()
    return _GM[geometry]


def heads_layers(geometry):
    cfg = kc.GEOMETRIES[geometry]
    return cfg["n_heads"] * cfg["n_layers"]


def kv_rows_equal(ctx, kv, upto, tag):
    for l, (k, v) in enumerate(kv):
        assert same16(ctx.CacheK(l)[:upto], k[:upto]), tag + (l, "K")
        assert same16(ctx.CacheV(l)[:upto], v[:upto]), tag + (l, "V")


def load(ctx, ref, case):
    ctx.reset()
    return kc.inject(None, ctx, ref["K"], ref["V"], poison_beyond=case in kc.POISON_BEYOND)


# ---- one-token decode ---------------------------------------------------------------------------------------------------------------------------
ONE_FORMS = {                                   # name: (long threshold or None, LNB_ATTN_LAZY or None)
    "default": (None, None),                    # attn_exact_kernel up to 512 positions, the long pair at 513
    "long_lazy": (0, "1"),                      # attn_long_scores_kernel + attn_long_pv2_kernel at every T
    "long_eager": (0, "0"),                     # ... + attn_long_pv_kernel
}


@pytest.mark.parametrize("zseq", [0, 1], ids=["certified", "serial"])
@pytest.mark.parametrize("form", sorted(ONE_FORMS))
@pytest.mark.parametrize("geometry", sorted(kc.GEOMETRIES))
def test_one_token_step_on_every_case_and_edge(lnb, monkeypatch, geometry, form, zseq):
    threshold, lazy = ONE_FORMS[form]
    if lazy is not None:
        monkeypatch.setenv("LNB_ATTN_LAZY", lazy)
    ctx = lnb.InferenceContext(gpu_model(lnb, geometry), kc.CAPACITY)
    if threshold is not None or zseq:
        ctx.set_attention(-1 if threshold is None else threshold, zseq)
    per_call = heads_layers(geometry)
    for case, T in kc.grid():
        ref = kc.oracle_run(case, geometry, T)
        load(ctx, ref, case)
        z0 = ctx.zseq_count()
        lg, am = ctx.Forward([kc.TOKEN], T - 1)
        tag = (geometry, form, zseq, case, T)
        assert same(lg, ref["logits"]), tag
        assert am == ref["am"], tag
        kv_rows_equal(ctx, ref["kv"], T, tag)                # the crafted rows untouched, the new row the oracle's
        dz = ctx.zseq_count() - z0
        assert (dz == per_call) if zseq else (0 <= dz <= per_call), tag + (dz,)      # forced: every (head, layer) walked the serial sum
    ctx.close()


ONE_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
import numpy as np
import lnb
import kv_craft as kc
for geometry in ("hd64", "hd128"):
    gm = lnb.LlamaTransformer(device=0, **kc.GEOMETRIES[geometry]).fill_synthetic(kc.SEED_MODEL).finalize()
    for zseq in (0, 1):
        ctx = lnb.InferenceContext(gm, kc.CAPACITY).set_attention(0, zseq)
        for case, T in kc.grid():
            ref = kc.oracle_run(case, geometry, T)
            ctx.reset()
            kc.inject(None, ctx, ref["K"], ref["V"], poison_beyond=case in kc.POISON_BEYOND)
            lg, am = ctx.Forward([kc.TOKEN], T - 1)
            assert kc.eq_or_both_nan_f32(lg, ref["logits"]) and am == ref["am"], (geometry, zseq, case, T)
            for l, (k, v) in enumerate(ref["kv"]):
                assert kc.eq_or_both_nan_bf16(ctx.CacheK(l)[:T], k[:T]) and kc.eq_or_both_nan_bf16(ctx.CacheV(l)[:T], v[:T]), (geometry, zseq, case, T, l)
        ctx.close()
print("one-launch child ok")
"""


def run_child(code, env, marker):
    r = subprocess.run([sys.executable, "-c", code % dict(root=ROOT, pkg=PKG, tests=os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_one_launch_form_in_a_fresh_process(lnb):
    """LNB_ATTN_ONE is read once per process: attn_one_kernel at every T of the grid, certified and with the serial sums"""
    run_child(ONE_CHILD, {"LNB_ATTN_ONE": "1"}, "one-launch child ok")


# ---- batched decode: member m gets case m, so one pass holds a NaN row beside finite ones ---------------------------------------------------------
def batch_step(lnb, geometry, members, long_threshold=None, zseq=0, want_form=0):
    """one lnb_batch_decode step of the members [(case, T)], each against its own oracle run: the token (a member whose logits row is all NaN
    gets -1, the oracle's argmax, and the single step succeeds -- only a FOLLOWING step would refuse to gather row -1) and the cache rows."""
    gm = gpu_model(lnb, geometry)
    refs = [kc.oracle_run(case, geometry, T) for case, T in members]
    ctxs = [lnb.InferenceContext(gm, kc.CAPACITY) for _ in members]
    for c, (case, T), ref in zip(ctxs, members, refs):
        load(c, ref, case)
    bat = lnb.Batch(ctxs)
    if long_threshold is not None:
        bat.set_attention(long_threshold, zseq)
    n = len(members)
    tok = np.full(n, kc.TOKEN, dtype=np.int32); pos = np.array([T - 1 for _, T in members], dtype=np.int32)
    out = np.full((n, 1), -7, dtype=np.int32)
    ms = C.c_float(0)
    z0 = ctxs[0].zseq_count()
    rc = lnb.lib().lnb_batch_decode(bat.h, tok.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.POINTER(C.c_int32)), 1, out.ctypes.data_as(C.c_void_p), C.byref(ms))
    assert rc == 0, lnb.lib().lnb_last_error().decode()
    assert bat.attention_form() == want_form, (geometry, members)
    for s, (c, (case, T), ref) in enumerate(zip(ctxs, members, refs)):
        assert out[s, 0] == ref["am"], (geometry, case, T, "token of member %d" % s, int(out[s, 0]), ref["am"])
        kv_rows_equal(c, ref["kv"], T, (geometry, case, T, "member %d" % s))
    dz = ctxs[0].zseq_count() - z0
    if zseq:
        assert dz == n * heads_layers(geometry), (geometry, members, dz)
    bat.close()
    for c in ctxs:
        c.close()


def members_at(Ts):
    """every case of the table, case m at Ts[m % len(Ts)] -- (case, T) pairs the grid leaves out are moved to T = 65"""
    out = []
    for m, case in enumerate(sorted(kc.CASES)):
        T = Ts[m % len(Ts)]
        out.append((case, T if (case, T) not in kc.LEFT_OUT else 65))
    return out


@pytest.mark.parametrize("geometry", sorted(kc.GEOMETRIES))
def test_batched_decode_gives_each_member_its_own_oracle_run(lnb, geometry):
    batch_step(lnb, geometry, [("one_inf", 17), ("denormal_visible", 17)])          # two members
    batch_step(lnb, geometry, members_at((65,)))                                    # every case at one T
    batch_step(lnb, geometry, members_at((2, 15, 16, 63, 64, 255, 256, 257, 511, 512)))
    batch_step(lnb, geometry, [(c, 64) for c in sorted(kc.CASES) if c != "one_inf"])          # no NaN member: the call succeeds, form and tokens asserted


def test_batched_decode_on_the_dense_dispatch(lnb):
    """attn_exact_kernel<128, DENSE>: head_dim 128 and more than 256 (head, sequence) workgroups -- 35 members of 8 heads"""
    Ts = (15, 17, 64, 257, 512)
    batch_step(lnb, "h8kv2_hd128", [(case, T) for T in Ts for case in sorted(kc.CASES)])
    batch_step(lnb, "h8kv2_hd128", [(case, T) for T in Ts for case in sorted(kc.CASES) if case != "one_inf"] + [("ties", 63)] * 5)


@pytest.mark.parametrize("force_z", ["0", "1"])
def test_batched_decode_per_kv_head_kernel(lnb, monkeypatch, force_z):
    """attn_gqa_kernel (head_dim 128, four query heads per KV head), forced on at one member per case"""
    monkeypatch.setenv("LNB_ATTN_GQA", "1")
    monkeypatch.setenv("LNB_ATTN_GQA_FORCE_ZSEQ", force_z)
    batch_step(lnb, "h8kv2_hd128", members_at((65,)))
    batch_step(lnb, "h8kv2_hd128", members_at((15, 16, 17, 63, 64, 255, 256, 257, 511, 512)))
    batch_step(lnb, "h8kv2_hd128", [(c, 256) for c in sorted(kc.CASES) if c != "one_inf"])


@pytest.mark.parametrize("zseq", [0, 1], ids=["certified", "serial"])
@pytest.mark.parametrize("geometry", ["hd64", "h8kv2_hd128", "hd64_two_layers"])
def test_batched_decode_on_the_long_pair(lnb, geometry, zseq):
    batch_step(lnb, geometry, [(c, 257) for c in sorted(kc.CASES) if c != "one_inf"], long_threshold=0, zseq=zseq, want_form=1)
    batch_step(lnb, geometry, members_at((15, 17, 64, 256, 513)), long_threshold=0, zseq=zseq, want_form=1)


# ---- lnb_forward_append after crafted rows: row i is the oracle's one-token step at n_pos + i -------------------------------------------------------
APPEND_POS = (13, 62, 254)


def check_append(ctx, geometry, case, n_pos, n, form, tag):
    ref = kc.oracle_steps(case, geometry, n_pos, 20)
    load(ctx, ref, case)
    lg, am = ctx.ForwardAppend(ref["toks"][:n], n_pos)
    assert ctx.append_attention_form() == form, tag
    assert same(lg, ref["logits"][:n]), tag
    assert am == ref["am"][n - 1], tag
    kv_rows_equal(ctx, ref["kv"], n_pos + n, tag)


@pytest.mark.parametrize("geometry", sorted(kc.GEOMETRIES))
def test_append_of_3_and_20_rows_after_crafted_rows(lnb, geometry):
    ctx = lnb.InferenceContext(gpu_model(lnb, geometry), kc.CAPACITY)
    for case in sorted(kc.CASES):
        for n_pos in APPEND_POS:
            check_append(ctx, geometry, case, n_pos, 3, 1, (geometry, case, n_pos, 3))
            check_append(ctx, geometry, case, n_pos, 20, 1 if geometry == "hd32" else 2, (geometry, case, n_pos, 20))
    ctx.close()


@pytest.mark.parametrize("geometry", ["hd64", "hd128", "hd32"])
def test_append_on_the_rows_pair_after_crafted_rows(lnb, geometry):
    ctx = lnb.InferenceContext(gpu_model(lnb, geometry), kc.CAPACITY).set_rows_attention(0, 0)
    for case in sorted(kc.CASES):
        for n_pos in (254, 520):                            # across the 256-position block; beyond LNB_ATTN_LONG_T
            check_append(ctx, geometry, case, n_pos, 3, 4, (geometry, case, n_pos, 3))
            check_append(ctx, geometry, case, n_pos, 15, 4, (geometry, case, n_pos, 15))
    ctx.set_rows_attention(-1, 1)                            # every row walks the serial sum
    z0 = ctx.zseq_count()
    check_append(ctx, geometry, "spread", 520, 3, 4, (geometry, "serial"))
    assert ctx.zseq_count() == z0 + 3 * heads_layers(geometry)
    ctx.close()


ROWS_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
import numpy as np
import lnb
import kv_craft as kc
geometry = "hd128"
gm = lnb.LlamaTransformer(device=0, **kc.GEOMETRIES[geometry]).fill_synthetic(kc.SEED_MODEL).finalize()
ctx = lnb.InferenceContext(gm, kc.CAPACITY).set_rows_attention(0, 0)
for case in sorted(kc.CASES):
    for n_pos in (254, 520):
        ref = kc.oracle_steps(case, geometry, n_pos, 15)
        for n in (3, 15):
            ctx.reset()
            kc.inject(None, ctx, ref["K"], ref["V"], poison_beyond=case in kc.POISON_BEYOND)
            lg, am = ctx.ForwardAppend(ref["toks"][:n], n_pos)
            assert ctx.append_attention_form() == 4
            assert kc.eq_or_both_nan_f32(lg, ref["logits"][:n]) and am == ref["am"][n - 1], (case, n_pos, n)
            for l, (k, v) in enumerate(ref["kv"]):
                assert kc.eq_or_both_nan_bf16(ctx.CacheK(l)[:n_pos + n], k[:n_pos + n]) and kc.eq_or_both_nan_bf16(ctx.CacheV(l)[:n_pos + n], v[:n_pos + n]), (case, n_pos, n, l)
print("rows child ok")
"""


@pytest.mark.parametrize("rpw", [1, 2, 4])
def test_every_rows_per_workgroup_form_in_a_fresh_process(lnb, rpw):
    run_child(ROWS_CHILD, {"LNB_ATTN_ROWS_RPW": str(rpw)}, "rows child ok")


# ---- the modulo-mask lnb_forward at start_pos = n_pos = 32 ----------------------------------------------------------------------------------------
_MODULO = {}


def oracle_modulo(case, geometry, S):
    key = (case, geometry, S)
    if key not in _MODULO:
        om = kc.oracle_model(geometry)
        K, V = kc.rows(case, geometry, 33, om)
        oc = orc.Context(om, 32 + S)
        kc.inject(oc, None, K, V)
        toks = kc.step_tokens(geometry, S)
        lg, am = oc.forward(toks, 32)
        kv = [(oc.cache(l, 0).copy(), oc.cache(l, 1).copy()) for l in range(len(K))]
        oc.close()
        _MODULO[key] = dict(K=K, V=V, toks=toks, logits=lg, am=am, kv=kv)
    return _MODULO[key]


def check_modulo(lnb, geometry, form):
    ctx = lnb.InferenceContext(gpu_model(lnb, geometry), kc.CAPACITY)
    for case in sorted(kc.CASES):
        for S in (16, 32):
            ref = oracle_modulo(case, geometry, S)
            load(ctx, ref, case)
            lg, am = ctx.Forward(ref["toks"], 32)
            tag = (geometry, form, case, S)
            if form is not None:
                assert ctx.prefill_attention_form() == (0 if geometry == "hd32" else form), tag
            assert same(lg, ref["logits"]), tag
            assert am == ref["am"], tag
            kv_rows_equal(ctx, ref["kv"], 32 + S, tag)
    ctx.close()


@pytest.mark.parametrize("geometry", sorted(kc.GEOMETRIES))
def test_modulo_mask_forward_scores_once(lnb, geometry):
    check_modulo(lnb, geometry, 3)                           # attn_mfma3_kernel (hd32: the row kernel)


@pytest.mark.parametrize("geometry", ["hd64", "hd128", "h8kv2_hd128"])
def test_modulo_mask_forward_scores_twice(lnb, monkeypatch, geometry):
    monkeypatch.setenv("LNB_ATTN_SIDX_MB", "0")
    check_modulo(lnb, geometry, 1)                           # attn_mfma_kernel


@pytest.mark.parametrize("geometry", ["hd64", "hd128", "h8kv2_hd128"])
def test_modulo_mask_forward_two_tiles_per_wave(lnb, monkeypatch, geometry):
    monkeypatch.setenv("LNB_ATTN_MFMA2", "16")
    check_modulo(lnb, geometry, None)                        # attn_mfma2_kernel


MODULO_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
import lnb
import kv_craft as kc
import test_gpu_attention_crafted as t
for geometry in ("hd64", "hd128"):
    t.check_modulo(lnb, geometry, 0)
print("modulo child ok")
"""


def test_modulo_mask_forward_on_the_row_kernel_in_a_fresh_process(lnb):
    """LNB_PREFILL_MFMA=0 (read once per process): calls of 16+ rows stay on attn_exact_kernel"""
    run_child(MODULO_CHILD, {"LNB_PREFILL_MFMA": "0"}, "modulo child ok")


# ---- speculative verify passes after crafted rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["spread", "denormal_visible", "huge_finite", "ties", "signed_zero_v", "minus_masked_tail", "v_order"])
@pytest.mark.parametrize("geometry", ["hd128", "h8kv2_hd128"])
def test_speculative_decode_after_crafted_rows_equals_greedy(lnb, geometry, case):
    gm = gpu_model(lnb, geometry)
    n_pos, steps = 62, 24
    ref = kc.oracle_run(case, geometry, n_pos + 1)
    g = lnb.InferenceContext(gm, kc.CAPACITY)
    load(g, ref, case)
    want, fin, _ = g.decode_greedy_until(kc.TOKEN, n_pos, steps)
    assert want[0] == ref["am"] and not fin
    gkv = [(g.CacheK(l).copy(), g.CacheV(l).copy()) for l in range(kc.GEOMETRIES[geometry]["n_layers"])]
    g.close()
    for long_form in (False, True):
        c = lnb.InferenceContext(gm, kc.CAPACITY)
        load(c, ref, case)
        if long_form:
            c.set_batched_attention(0, 0)
        c.set_draft(7, 1, 4, [kc.TOKEN] + [int(t) for t in want])
        got, fin, st, _ = c.decode_speculative_until([], kc.TOKEN, n_pos, steps)
        assert [int(t) for t in got] == [int(t) for t in want] and not fin, (geometry, case, long_form)
        assert st["verify_passes"] > 0 and st["accepted"] > 0 and c.verify_attention_form() == (1 if long_form else 0)
        for l, (k, v) in enumerate(gkv):
            assert same16(c.CacheK(l)[:n_pos + steps], k[:n_pos + steps]) and same16(c.CacheV(l)[:n_pos + steps], v[:n_pos + steps]), (geometry, case, l)
        c.close()


# ---- poison tokens: a vocabulary id whose embedding row is NaN ------------------------------------------------------------------------------------------
POISON_ID = 77
_POISON = {}


def poison_pair(lnb):
    """two-layer TINY on both sides with the embedding row of POISON_ID set to NaN"""
    if not _POISON:
        cfg = dict(orc.TINY)
        om = orc.Model(**cfg).fill_synthetic(kc.SEED_MODEL)
        gm = lnb.LlamaTransformer(device=0, **cfg).fill_synthetic(kc.SEED_MODEL)
        emb = om.get_tensor("tok_embeddings.weight").copy().reshape(cfg["vocab_size"], cfg["dim"])
        emb[POISON_ID] = kc.QNAN
        om.set_tensor("tok_embeddings.weight", emb); gm.set_tensor("tok_embeddings.weight", emb)
        om.finalize(); gm.finalize().enable_batch()
        _POISON.update(cfg=cfg, om=om, gm=gm)
    return _POISON["cfg"], _POISON["om"], _POISON["gm"]


def poison_tokens(cfg, seed, n, at=()):
    toks = orc.synth_tokens(seed, n, cfg["vocab_size"]).copy()
    toks[toks == POISON_ID] = POISON_ID + 1
    for i in at:
        toks[i] = POISON_ID
    return toks


def oracle_one_token_rows(om, cfg, toks, start=0, prefix=None):
    oc = orc.Context(om, start + len(toks))
    if prefix is not None:
        oc.forward(prefix, 0, want_logits=False)
    lg = np.empty((len(toks), cfg["vocab_size"]), dtype=np.float32); am = []
    for i, t in enumerate(toks):
        l1, a1 = oc.forward([t], start + i)
        lg[i] = l1[0]; am.append(a1)
    kv = [(oc.cache(l, 0).copy(), oc.cache(l, 1).copy()) for l in range(cfg["n_layers"])]
    oc.close()
    return lg, am, kv


@pytest.mark.parametrize("S,at", [(20, 17), (20, 5), (12, 5), (12, 11)])
def test_forward_with_a_poison_row_is_the_reference_row_for_row(lnb, S, at):
    """the reference's modulo-mask call adds the mask to a NaN score and multiplies p = +0 by the NaN V row: EVERY row of the call is NaN"""
    cfg, om, gm = poison_pair(lnb)
    toks = poison_tokens(cfg, 4242, S, (at,))
    oc = orc.Context(om, S)
    lo, ao = oc.forward(toks, 0)
    assert np.isnan(lo).all() and ao == -1
    gc = lnb.InferenceContext(gm, 64)
    lg, ag = gc.Forward(toks, 0)
    bad = [i for i in range(S) if not same(lg[i], lo[i])]
    assert not bad and ag == ao, (S, at, "rows that differ from the oracle's", bad)
    for l in range(cfg["n_layers"]):
        assert same16(gc.CacheK(l)[:S], oc.cache(l, 0)[:S]) and same16(gc.CacheV(l)[:S], oc.cache(l, 1)[:S]), l
    gc.close(); oc.close()


@pytest.mark.parametrize("n,at", [(20, 17), (20, 5), (12, 5), (40, 33)])
def test_append_with_a_poison_row_equals_one_token_steps(lnb, n, at):
    """row i of lnb_forward_append is the one-token step at start_pos + i, which never sees a later row: the rows before the poison row are finite"""
    cfg, om, gm = poison_pair(lnb)
    toks = poison_tokens(cfg, 4242, n, (at,))
    lo, ao, okv = oracle_one_token_rows(om, cfg, toks)
    assert not np.isnan(lo[:at]).any() and np.isnan(lo[at:]).all()
    for start, prefix in ((0, None), (7, poison_tokens(cfg, 99, 7))):
        if prefix is not None:
            lo, ao, okv = oracle_one_token_rows(om, cfg, toks, start, prefix)
        gc = lnb.InferenceContext(gm, 64)
        if prefix is not None:
            gc.Forward(prefix, 0, want_logits=False)
        lg, ag = gc.ForwardAppend(toks, start)
        bad = [i for i in range(n) if not same(lg[i], lo[i])]
        assert not bad and ag == ao[-1], (n, at, start, "rows that differ from the one-token steps", bad)
        for l in range(cfg["n_layers"]):
            assert same16(gc.CacheK(l)[:start + n], okv[l][0][:start + n]) and same16(gc.CacheV(l)[:start + n], okv[l][1][:start + n]), l
        gc.close()


def test_append_many_with_poison_rows_equals_one_token_steps(lnb):
    cfg, om, gm = poison_pair(lnb)
    lists = [poison_tokens(cfg, 11, 20, (17,)), poison_tokens(cfg, 12, 20), poison_tokens(cfg, 13, 3, (1,)), poison_tokens(cfg, 14, 33, (30,))]
    ctxs = [lnb.InferenceContext(gm, 64) for _ in lists]
    got, am = lnb.ForwardAppendMany(ctxs, lists, [0] * len(lists))
    for s, toks in enumerate(lists):
        lo, ao, okv = oracle_one_token_rows(om, cfg, toks)
        bad = [i for i in range(len(toks)) if not same(got[s][i], lo[i])]
        assert not bad and am[s] == ao[-1], (s, bad)
        for l in range(cfg["n_layers"]):
            assert same16(ctxs[s].CacheK(l)[:len(toks)], okv[l][0][:len(toks)]) and same16(ctxs[s].CacheV(l)[:len(toks)], okv[l][1][:len(toks)]), (s, l)
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("long_form", [False, True], ids=["short", "long"])
def test_a_drafted_poison_token_is_judged_as_greedy_would(lnb, long_form):
    """the corpus makes every pass draft the poison token right after the current one: the verify pass computes a NaN column beside the real one,
    rejects the draft as greedy would have, and the stale NaN rows it leaves beyond the accepted position change nothing afterwards"""
    cfg, om, gm = poison_pair(lnb)
    P, steps = 20, 16
    prompt = poison_tokens(cfg, 321, P)
    g = lnb.InferenceContext(gm, 64)
    first = g.Forward(prompt, 0, want_logits=False)[1]
    want, fin, _ = g.decode_greedy_until(first, P, steps)
    assert POISON_ID not in [int(t) for t in want] and first != POISON_ID
    gkv = [(g.CacheK(l).copy(), g.CacheV(l).copy()) for l in range(cfg["n_layers"])]
    g.close()
    corpus = []
    for t in [first] + [int(t) for t in want]:
        corpus += [t, POISON_ID, POISON_ID]
    c = lnb.InferenceContext(gm, 64)
    if long_form:
        c.set_batched_attention(0, 0)
    assert c.Forward(prompt, 0, want_logits=False)[1] == first
    c.set_draft(4, 1, 1, corpus)
    got, fin, st, _ = c.decode_speculative_until(prompt, first, P, steps)
    assert [int(t) for t in got] == [int(t) for t in want] and not fin
    assert st["verify_passes"] > 0 and st["drafted"] > st["accepted"]
    for l, (k, v) in enumerate(gkv):
        assert same16(c.CacheK(l)[:P + steps], k[:P + steps]) and same16(c.CacheV(l)[:P + steps], v[:P + steps]), l
    c.close()
