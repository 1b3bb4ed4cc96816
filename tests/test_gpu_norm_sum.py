"""The f32 sum of squares of the RMSNorm, bit for bit, from every kernel form that carries a norm (-m gpu).  lnb_op_rmsnorm_sum runs each form through its own
launch function -- the launch tally proves which -- in the instantiation of the production template arguments that has the walker's report compiled in, and
returns per row the sum as the walker holds it in front of the division by K, the scale r, and the walker's path word.  The reference is the oracle's plain
sequential loop (orc_rmsnorm_stats), never the emulation of tests/native/seqsum_host.cpp.  Division and square root are correctly rounded in both
arithmetics: there is no tolerance; a NaN compares as a NaN.

Rows: tests/norm_craft.py -- the families the suite already had and one builder per way out of the branch-free item walk, each also reversed and rotated by
one to three positions -- at every K of norm_craft.K_SET that the form's launch function accepts.  tests/test_norm_sum_cpu.py proves on the emulation that
the builders reach their path classes; here the path words the DEVICE returns must show every class per folding-wave count (set-level: the device sums its
approximate prefix in its own order, a borderline row may take another path than in the emulation)."""
import numpy as np
import pytest

import norm_craft as nc
from form_tally import ran
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

EPS = 1e-5
NAMES = ("chain16", "chain32", "chain64", "quad24", "quad24_sched", "gate_up56", "gate_up28", "gate_up56_packed", "head_packed", "rows_wide", "batch_xt", "rows_wave")
# what the launch functions refuse: the quad kernel walks whole stages of 256 (128 under the throughput schedule) terms; the wide row norms take multiples of 128
REFUSED = {"quad24": {8, 64, 200, 1000}, "quad24_sched": {8, 64, 200, 1000}, "rows_wide": {8, 64, 200, 1000}, "batch_xt": {8, 64, 200, 1000},
           "head_packed": {8192}}                                # two 64 KB product stages + 8192 f32 of x exceed the 160 KB of LDS (lnbk_headp_supported)


@pytest.fixture(scope="module")
def lnb():
    import lnb as _lnb
    _lnb.build()
    assert _lnb.device_count() >= 1
    assert tuple(_lnb.NORM_FORMS) == NAMES
    return _lnb


_rows, _runs = {}, {}


def rows_for(K, nh):
    """(names, x, the oracle's sum bits, the oracle's scale bits), computed once per (K, folding waves) and left unchanged"""
    if (K, nh) not in _rows:
        names, _, x = nc.row_set(K, nh)
        s, r = np.empty(x.shape[0], dtype=np.float32), np.empty(x.shape[0], dtype=np.float32)
        orc.lib().orc_rmsnorm_stats(orc._p(x), x.shape[0], K, np.float32(EPS), orc._p(s), orc._p(r))
        x.setflags(write=False)
        _rows[(K, nh)] = (names, x, s.view(np.uint32), r.view(np.uint32))
    return _rows[(K, nh)]


def run_form(lnb, form):
    """{K: (sum_bits, scale_bits, walk) or None where the launch function refuses K}, every call inside a `ran` block of the form's own tally row"""
    if form not in _runs:
        _, tally, epi, nh = lnb.NORM_FORMS[form]
        out = {}
        for K in nc.K_SET:
            _, x, _, _ = rows_for(K, nh)
            if K in REFUSED.get(form, ()):
                out[K] = lnb.op_rmsnorm_sum(x, EPS, form)                    # (None when refused; the bit test asserts that it was)
                continue
            with ran(lnb, {tally: epi}):
                out[K] = lnb.op_rmsnorm_sum(x, EPS, form)
            only = {n for n in lnb.form_names() if lnb.form_count(n)}        # this form's row of the tally and no other kernel's
            assert only == {tally}, (form, K, only)
        _runs[form] = out
    return _runs[form]


def _differ(got, ref):
    g, r = got.view(np.float32), ref.view(np.float32)
    return np.flatnonzero(~((got == ref) | (np.isnan(g) & np.isnan(r))))


@pytest.mark.parametrize("form", NAMES)
def test_sum_and_scale_are_the_sequential_loops_bits(lnb, form):
    nh = lnb.NORM_FORMS[form][3]
    runs = run_form(lnb, form)
    refused = {K for K, v in runs.items() if v is None}
    assert refused == REFUSED.get(form, set()), (form, sorted(refused))
    for K, v in runs.items():
        if v is None:
            continue
        names, x, s_ref, r_ref = rows_for(K, nh)
        sb, rb, wk = v
        bad = _differ(sb, s_ref)
        assert bad.size == 0, "%s K %d: the sum differs in %d of %d rows; first (row, name, got, oracle, path): %s" % (
            form, K, bad.size, len(names), [(int(i), names[i], hex(int(sb[i])), hex(int(s_ref[i])), hex(int(wk[i]) & 0xFFFFFFFF)) for i in bad[:6]])
        bad = _differ(rb, r_ref)
        assert bad.size == 0, "%s K %d: the scale differs in %d of %d rows; first (row, name, got, oracle): %s" % (
            form, K, bad.size, len(names), [(int(i), names[i], hex(int(rb[i])), hex(int(r_ref[i]))) for i in bad[:6]])
        if nh is None:
            assert (wk == -1).all()                              # the plain serial loop has no item list


@pytest.mark.parametrize("nh", [2, 6, 7, 8])
def test_the_device_took_every_path_at_this_folding_wave_count(lnb, nh):
    """from the path words the kernels returned: (a) item list of runs only, (b) with a split leaf, (c) with single-term items, (d) record walk because of the
    item count or a full list segment, (e) because of a failed item check, (f) because of a non-finite leaf, (g) a replay inside rms_walk_fast -- each in at
    least one row, for EVERY form that folds on nh waves.  rms_walk_heap (a failed scan composition) is expected to be unreachable and is only reported."""
    forms = [f for f in NAMES if lnb.NORM_FORMS[f][3] == nh]
    assert forms
    for form in forms:
        counts, heap = dict.fromkeys(nc.CLASSES, 0), 0
        for K, v in run_form(lnb, form).items():
            if v is None:
                continue
            for w in v[2]:
                for c in nc.classes_of(w):
                    counts[c] += 1
                heap += bool((int(w) & 0xFFFFFFFF) != 0xFFFFFFFF and int(w) & nc.LEFT and int(w) & nc.SCANFAIL)
        print("%-17s %d waves: rows per path class %s; rms_walk_heap %d" % (form, nh, counts, heap))
        assert all(counts.values()), (form, counts)
