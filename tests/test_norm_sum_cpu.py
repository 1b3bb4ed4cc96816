"""No GPU: the rows of tests/norm_craft.py against the lane-by-lane emulation of the norm's item walk (tests/native/seqsum_host.cpp), the reference's
orc_rmsnorm_stats, and the measurement that explains why lnb_op_rmsnorm_sum exists -- a sum of squares that is a few ulps off changes no bf16 output."""
import ctypes as C

import numpy as np
import pytest

import norm_craft as nc
from oracle import oracle as orc
from test_seqsum import lib, shipped_folding_waves  # noqa: F401  (the fixture that builds the emulation)


def _emulate(L, sq, K, nh):
    path = C.c_uint32(0)
    s = L.seqsum_device(sq.ctypes.data, K, nh, nc.RMS_HEAD, C.byref(path), None)
    return np.float32(s).view(np.uint32), path.value


def _same(a, b):
    return a == b or (np.isnan(np.uint32(a).view(np.float32)) and np.isnan(np.uint32(b).view(np.float32)))


def oracle_stats(x_u16, eps=1e-5):
    rows, K = x_u16.shape
    s, r = np.empty(rows, dtype=np.float32), np.empty(rows, dtype=np.float32)
    orc.lib().orc_rmsnorm_stats(orc._p(x_u16), rows, K, np.float32(eps), orc._p(s), orc._p(r))
    return s, r


def test_every_builder_reaches_its_path_class_at_every_shipped_wave_count(lib):  # noqa: F811
    """(i) per folding-wave count, over the K set: every row's emulated sum is the sequential loop's; every builder reaches the class it is built for in at
    least one row; all seven classes are reached -- so the device-side assertion of tests/test_gpu_norm_sum.py is not vacuous"""
    report = []
    for nh in shipped_folding_waves(lib):
        by_builder, reached = {}, set()
        for K in nc.K_SET:
            names, want, x = nc.row_set(K, nh)
            sq = nc.squares(x)
            for i in range(x.shape[0]):
                ref = np.float32(lib.seqsum_ref(sq[i].ctypes.data, K)).view(np.uint32)
                got, path = _emulate(lib, sq[i], K, nh)
                assert _same(got, ref), (nh, K, names[i], hex(path))
                cls = nc.classes_of(path)
                reached |= cls
                if want[i]:
                    by_builder.setdefault((names[i], want[i]), []).append(want[i] in cls)
        for (name, cls), hits in sorted(by_builder.items()):
            report.append("nh %d  %-20s %-10s %3d of %3d rows" % (nh, name, cls, sum(hits), len(hits)))
            assert any(hits), (nh, name, cls)
        assert reached == set(nc.CLASSES), (nh, sorted(set(nc.CLASSES) - reached))
    print("\n".join(report))


def _moved(s, n):
    return (s.view(np.uint32) + np.uint32(n)).view(np.float32)


def _norm_out(x_u16, s, eps=np.float32(1e-5)):
    K = x_u16.shape[1]
    mean = (s / np.float32(K)).astype(np.float32) + eps
    r = (1.0 / np.sqrt(mean.astype(np.float64))).astype(np.float32)
    xf = (x_u16.astype(np.uint32) << 16).view(np.float32)
    return nc.bf16_bits(xf * r[:, None])


@pytest.mark.parametrize("K", [256, 4096])
def test_the_old_outputs_hide_a_sum_that_is_a_few_ulps_off(K):
    """(ii) 200 gaussian rows of varied scale, the true sequential sum moved by n ulps, counting changed bf16 values of trunc(x * r): 1 and 2 ulps change
    nothing, 16 ulps almost nothing, 4096 ulps show in most rows.  Every GPU test of the norm before lnb_op_rmsnorm_sum read the sum through these outputs."""
    rng = np.random.default_rng(5 + K)
    x = nc.bf16_bits(rng.standard_normal((200, K)) * np.exp(rng.uniform(-6, 6, (200, 1))))
    s, _ = oracle_stats(x)
    ref = _norm_out(x, s)
    changed = {}
    for n in (1, 2, 16, 256, 4096):
        d = _norm_out(x, _moved(s, n)) != ref
        changed[n] = (int(d.sum()), int(d.any(axis=1).sum()))
    print("K = %d: changed (elements, rows) of %d, 200: %s" % (K, x.size, changed))
    assert changed[1] == (0, 0) and changed[2] == (0, 0)
    assert changed[16][1] <= 2                                   # at most a row or two of 200
    assert changed[4096][1] > 150


def test_orc_rmsnorm_stats_is_the_loop_of_orc_rmsnorm_bf16(lib):  # noqa: F811
    """(iii) the factored statistics: the sum is the plain sequential f32 loop (seqsum_ref on the exact squares), and the norm re-derived from rs is
    orc_rmsnorm_bf16's output bit for bit -- finite rows and the non-finite family alike"""
    L = lib
    for K in (8, 200, 1000, 4096):
        rng = np.random.default_rng(K)
        with np.errstate(over="ignore", invalid="ignore"):
            x = np.stack([nc.bf16_bits(r) for _, _, r in nc.old_families(rng, K)])
        s, rs = oracle_stats(x)
        sq = nc.squares(x)
        for i in range(x.shape[0]):
            assert _same(s[i].view(np.uint32), np.float32(L.seqsum_ref(sq[i].ctypes.data, K)).view(np.uint32)), (K, i)
        nw = nc.bf16_bits(1 + 0.1 * rng.standard_normal(K))
        y, pre = np.zeros_like(x), np.zeros_like(x)
        orc.lib().orc_rmsnorm_bf16(orc._p(x), orc._p(nw), orc._p(y), x.shape[0], K, np.float32(1e-5), orc._p(pre))
        xf, wf = (x.astype(np.uint32) << 16).view(np.float32), (nw.astype(np.uint32) << 16).view(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            mine_pre = nc.bf16_bits(xf * rs[:, None])
            mine = nc.bf16_bits((mine_pre.astype(np.uint32) << 16).view(np.float32) * wf[None, :])

        def nan16(a):
            return np.isnan((a.astype(np.uint32) << 16).view(np.float32))
        assert (((mine_pre == pre) | (nan16(mine_pre) & nan16(pre))).all() and ((mine == y) | (nan16(mine) & nan16(y))).all()), K
