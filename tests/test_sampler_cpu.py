"""Seeded temperature / top-k / top-p sampling (include/lnb.h), what can be checked without a GPU: the serial C++ walk of the rule (csrc/lnb_sample.h, run by
tests/native/sample_test.cpp as a stand-alone program under the address and undefined-behaviour sanitizers) against the numpy restatement (tests/sampler_ref.py)
on llama-like rows, crafted rows and the sampler grid; properties of the rule itself; the symbols, the struct layouts and every refusal that needs no device."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import sampler_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llama-nuts-and-bolts_amd")
NAMES = ("lnb_decode_sample_until", "lnb_batch_decode_sample_until", "lnb_op_sample", "lnb_profile_sample")


@pytest.fixture(scope="module")
def lnb():
    import lnb as m
    m.build()
    return m


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    hdr = open(os.path.join(PKG, "csrc", "lnb_sample.h")).read()
    code = re.sub(r"//.*", "", hdr)
    assert "hip" not in code.lower() and "#include" not in code          # plain C++ that includes nothing
    exe = str(tmp_path_factory.mktemp("sample") / "sample_test")
    src = os.path.join(ROOT, "tests", "native", "sample_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    return exe


def run_native(exe, path, rows, cases):
    """cases: (row, (t, k, p), seed, pos or None, u or None) -> [(token, info dict)]"""
    rows = np.ascontiguousarray(rows, dtype=np.uint16)
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", rows.shape[0], rows.shape[1], len(cases)))
        f.write(rows.tobytes())
        for r, (t, k, p), seed, pos, u in cases:
            f.write(struct.pack("<iffiQiiQ", r, t, p, k, seed, 0 if u is None else 1, 0, (pos & sr.MASK) if u is None else u))
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "sample_test: ok (%d cases)" % len(cases) in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    out = []
    for line in res.stdout.splitlines()[:len(cases)]:
        v = [int(x) for x in line.split()]
        out.append((v[0], dict(zip(sr.INFO_FIELDS, v[1:]))))
    return out


def check_against_ref(rows, cases, got):
    preps = {}
    for (r, tkp, seed, pos, u), (tok, info) in zip(cases, got):
        key = (r, tkp)
        if key not in preps:
            preps[key] = sr.prepare(rows[r], *tkp)
        want = sr.pick(preps[key], sr.draw(seed, pos) if u is None else u)
        assert info == preps[key][3], (r, tkp, info, preps[key][3])
        assert tok == want, (r, tkp, seed, pos, u, tok, want)


@pytest.mark.parametrize("V", [1001, 128256])
def test_the_serial_walk_equals_the_restatement_on_llama_like_rows_over_the_grid(native, tmp_path, V):
    rows = sr.llama_like_rows(np.random.default_rng(20261019 + V), 64, V)
    cases = []
    for n, (r, tkp) in enumerate(sr.grid_cases(V)):
        for j in range(3):                                                   # every position and every seed on every grid point
            cases.append((r, tkp, sr.SEEDS[(n + j) % 3], sr.POSITIONS[j], None))
    got = run_native(native, str(tmp_path / "grid.bin"), rows, cases)
    check_against_ref(rows, cases, got)
    assert len({t for t, _ in got}) > 50                                     # (it samples: not one token for everything)


@pytest.mark.parametrize("V", [1001, 128256])
def test_the_serial_walk_equals_the_restatement_on_the_crafted_rows(native, tmp_path, V):
    crafted = sr.crafted(V)
    rows = np.stack([c[1] for c in crafted])
    cases, checks = [], []
    for r, (name, row, tkp, check, boundaries) in enumerate(crafted):
        prep = sr.prepare(row, *tkp)
        for seed, pos in ((0, 0), (777, 8), (12345, 131071)):
            cases.append((r, tkp, seed, pos, None)); checks.append((name, check))
        for u in (sr.boundary_draws(prep) if boundaries else []):
            cases.append((r, tkp, 0, None, u)); checks.append((name, check))
    got = run_native(native, str(tmp_path / "crafted.bin"), rows, cases)
    check_against_ref(rows, cases, got)
    for (name, check), (tok, info), case in zip(checks, got, cases):
        if check:
            check(tok, info, rows[case[0]])


def test_the_all_equal_row_of_131072_entries_stays_below_2_to_63(native, tmp_path):
    V = 131072
    rows = np.full((1, V), sr.bf(0.6875), dtype=np.uint16)                   # exp(0.6875) = 1.989: every weight just under 2^46
    cases = [(0, (1.0, 0, 1.0), 1, 5, None), (0, (1.0, 0, 0.9), 2, 6, None), (0, (1.0, 0, 1.0), 0, None, sr.MASK), (0, (1.0, 70000, 0.5), 3, 7, None)]
    got = run_native(native, str(tmp_path / "equal.bin"), rows, cases)
    check_against_ref(rows, cases, got)
    w = int(np.floor(np.ldexp(sr.exp_table()[sr.bf(0.6875)], 45)))
    assert got[0][1]["w_all"] == V * w and 2 ** 62 < V * w < 2 ** 63 and got[0][1]["n_candidates"] == V
    assert got[2][0] == V - 1                                                # u = 2^64 - 1: r = W_K - 1, the last entry
    assert got[3][1]["n_kept"] in (35000, 35001) and got[3][0] < got[3][1]["n_kept"]      # ties at both cuts: the lowest indices (f64(W1) may round up by one weight)


# ---- properties of the rule, on the restatement --------------------------------------------------------------------------------------------
def test_top_k_1_is_argmax_and_temperature_0_is_argmax():
    rows = sr.llama_like_rows(np.random.default_rng(5), 16, 1001)
    for i, row in enumerate(rows):
        for t in (1.0, 0.7, 1.5):
            tok, info = sr.sample(row, (t, 1, 1.0, i), pos=i)
            assert tok == sr.argmax(row) and info["n_kept"] == 1
        assert sr.sample(row, (0.0, 40, 0.5, i), pos=i)[0] == sr.argmax(row)


def test_raising_top_p_never_shrinks_the_kept_set_and_the_sums_are_consistent():
    rows = sr.llama_like_rows(np.random.default_rng(6), 8, 1001)
    for row in rows:
        for t in (0.7, 1.5):
            for k in (0, 40):
                last, last_set = 0, set()
                for p in (1e-6, 0.1, 0.5, 0.9, 0.99, 1.0):
                    _, ks, cs, info = sr.prepare(row, t, k, p)
                    assert info["n_kept"] >= last and last_set <= set(ks.tolist())
                    last, last_set = info["n_kept"], set(ks.tolist())
                    assert 1 <= info["n_kept"] <= (min(k, info["n_candidates"]) if k else info["n_candidates"])
                    assert 2 ** 45 <= info["w_kept"] <= info["w_topk"] <= info["w_all"] < 2 ** 63
                    if p < 1:
                        assert info["w_kept"] >= int(np.floor(np.float64(np.float32(p)) * np.float64(info["w_topk"])))
                    else:
                        assert info["w_kept"] == info["w_topk"]
                    if k == 0:
                        assert info["w_topk"] == info["w_all"]


def test_the_draw_frequencies_follow_the_weights():
    """20 000 draws (seeds 0..19999) on an 8-entry row: each entry's frequency within 5 binomial standard deviations of w_j / W_K"""
    row = np.full(8, 0xFF80, dtype=np.uint16)
    row[:] = [sr.bf(v) for v in (0.0, 1.0, -1.0, 2.0, 0.5, -3.0, 1.5, 0.25)]
    prep = sr.prepare(row, 1.0, 0, 1.0)
    _, ks, cs, info = prep
    w = np.diff(np.concatenate([[0], cs.astype(np.float64)]))
    N = 20000
    counts = np.bincount([sr.pick(prep, sr.draw(seed, 3)) for seed in range(N)], minlength=8)
    p = w / float(info["w_kept"])
    assert (np.abs(counts - N * p) <= 5 * np.sqrt(N * p * (1 - p))).all(), (counts, N * p)


def test_the_draw_is_a_function_of_seed_and_position_and_the_product_is_128_bit():
    assert sr.splitmix64(0) == 0xE220A8397B1DCDAF
    assert sr.draw(777, 8) == sr.splitmix64(sr.splitmix64(777) ^ ((8 * sr.GOLDEN) & sr.MASK))
    assert sr.draw(1, 2) != sr.draw(2, 1) and sr.draw(5, 0) == sr.splitmix64(sr.splitmix64(5))
    for W in (1, 2 ** 45, 2 ** 62 + 12345, 2 ** 63 - 1):
        for r in (0, W // 2, W - 1):
            assert (sr.u_for(r, W) * W) >> 64 == r


def test_the_restatement_reproduces_the_cross_check_table():
    """orc.TINY, weights 1234, prompt synth_tokens(99, 8, 1024): the prompt's last logits row sampled at pos 8, then teacher-forced one-token steps, seed 777 --
    the first tokens, how often the sampled token is its row's argmax and how many entries are kept, as computed by the rule's authors"""
    from oracle import oracle as orc
    om = orc.Model(**dict(orc.TINY)).fill_synthetic(1234).finalize()
    prompt = orc.synth_tokens(99, 8, 1024)
    table = {(1.0, 0, 1.0): ([369, 351, 199, 337, 809, 64, 713, 548], 0, (1024, 1024)), (0.7, 40, 0.9): ([394, 488, 168, 394, 831, 56, 746, 638], 4, (35, 36)),
             (1.5, 0, 0.5): (None, 0, (421, 427)), (1.0, 1, 1.0): (None, 24, (1, 1))}
    for smp, (first8, n_greedy, kept_range) in table.items():
        c = orc.Context(om, 64)
        row, _ = c.forward(prompt, 0)
        toks, greedy, kept = [], 0, []
        for i in range(24):
            r16 = orc.f32_to_bf16(np.ascontiguousarray(row[-1], dtype=np.float32))
            tok, info = sr.sample(r16, smp + (777,), pos=8 + i)
            greedy += tok == sr.argmax(r16); kept.append(info["n_kept"]); toks.append(tok)
            row, _ = c.forward(np.array([tok], dtype=np.int32), 8 + i)
        c.close()
        assert first8 is None or toks[:8] == first8, (smp, toks[:8])
        assert greedy == n_greedy and (min(kept), max(kept)) == kept_range, (smp, greedy, min(kept), max(kept))
    om.close()


# ---- exports, layouts, refusals ---------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported(lnb):
    L = lnb.lib()
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    for name, nargs in zip(NAMES, (9, 9, 9, 5)):
        assert name in lnb.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, hdr)
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == nargs
    assert re.search(r"#define\s+LNB_ABI_VERSION\s+6\b", hdr) and L.lnb_abi_version() == 6 == lnb.ABI_VERSION
    assert callable(lnb.InferenceContext.decode_sample_until) and callable(lnb.Batch.decode_sample_until) and callable(lnb.op_sample)
    assert "sampler" in lnb.InferenceEngine.__init__.__code__.co_varnames


def test_the_structs_have_the_headers_layout(lnb):
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    assert "typedef struct lnb_sampler { float temperature; float top_p; int32_t top_k; int32_t reserved; uint64_t seed; } lnb_sampler;" in hdr
    assert "typedef struct lnb_sample_info { uint64_t w_all, w_topk, w_kept; int32_t n_candidates, n_kept, degenerate, pad; } lnb_sample_info;" in hdr
    assert [f[0] for f in lnb.Sampler._fields_] == ["temperature", "top_p", "top_k", "reserved", "seed"] and C.sizeof(lnb.Sampler) == 24
    assert [f[0] for f in lnb.SampleInfo._fields_] == ["w_all", "w_topk", "w_kept", "n_candidates", "n_kept", "degenerate", "pad"] and C.sizeof(lnb.SampleInfo) == 40
    assert lnb.Sampler.seed.offset == 16 and lnb.SampleInfo.n_candidates.offset == 24
    s = lnb.Sampler(0.7, 40, 0.9, 777)
    assert (round(s.temperature, 3), s.top_k, round(s.top_p, 3), s.reserved, s.seed) == (0.7, 40, 0.9, 0, 777)


@pytest.mark.parametrize("rel", ["llama-nuts-and-bolts_amd/host/lnb_host.hpp", "llama-nuts-and-bolts_amd/go/inferencecontext_hip.go", "README.md", "DESIGN.md",
                                 "INTEGRATION.md", "NOTES.md"])
def test_every_layer_and_document_names_the_call(rel):
    assert "lnb_decode_sample_until" in open(os.path.join(ROOT, rel)).read(), rel


def _fails(rc, L, *words):
    assert rc < 0
    msg = L.lnb_last_error().decode()
    assert msg, "no error message"
    for w in words:
        assert w in msg, (w, msg)


BAD_SAMPLERS = [(dict(temperature=-0.5), "temperature"), (dict(temperature=float("nan")), "temperature"), (dict(temperature=float("inf")), "temperature"),
                (dict(top_k=-1), "top_k"), (dict(top_p=float("nan")), "top_p"), (dict(top_p=0.0), "top_p"), (dict(top_p=-0.1), "top_p"), (dict(top_p=1.5), "top_p"),
                (dict(reserved=1), "reserved")]


def _sampler(lnb, **kw):
    s = lnb.Sampler(0.7, 40, 0.9, 1)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_arguments_are_refused_before_any_handle_is_dereferenced(lnb):
    """The handles below are NULL or point at 64 bytes of 0xFF (a model pointer of all ones: dereferencing it would end the process)."""
    L = lnb.lib()
    junk = np.full(64, 0xFF, dtype=np.uint8)
    fake = C.c_void_p(junk.ctypes.data)
    out = np.zeros(8, dtype=np.int32); n = C.c_int(0)
    good = _sampler(lnb)
    # lnb_decode_sample_until
    call = lambda c, s, o, ng: L.lnb_decode_sample_until(c, s, 1, 4, 8, o, ng, None, None)
    _fails(call(None, C.byref(good), lnb._p(out), C.byref(n)), L, "null")
    _fails(call(fake, None, lnb._p(out), C.byref(n)), L, "null")
    _fails(call(fake, C.byref(good), None, C.byref(n)), L, "null")
    _fails(call(fake, C.byref(good), lnb._p(out), None), L, "null")
    for kw, word in BAD_SAMPLERS:
        _fails(call(fake, C.byref(_sampler(lnb, **kw)), lnb._p(out), C.byref(n)), L, "sampler", word)
    # lnb_batch_decode_sample_until (the samplers are behind the batch's own n: NULL pointers are what can be refused without it)
    i32 = np.zeros(4, dtype=np.int32); ip = i32.ctypes.data_as(C.POINTER(C.c_int32))
    arr = (lnb.Sampler * 2)(good, good)
    bcall = lambda b, s, t, p, o, ng: L.lnb_batch_decode_sample_until(b, s, t, p, 8, o, ng, None, None)
    _fails(bcall(None, arr, ip, ip, lnb._p(out), lnb._p(i32)), L, "null")
    _fails(bcall(fake, None, ip, ip, lnb._p(out), lnb._p(i32)), L, "null")
    _fails(bcall(fake, arr, None, ip, lnb._p(out), lnb._p(i32)), L, "null")
    _fails(bcall(fake, arr, ip, None, lnb._p(out), lnb._p(i32)), L, "null")
    _fails(bcall(fake, arr, ip, ip, None, lnb._p(i32)), L, "null")
    _fails(bcall(fake, arr, ip, ip, lnb._p(out), None), L, "null")
    # lnb_op_sample: everything is checked before a device is looked for
    row = np.zeros((2, 16), dtype=np.uint16); pos = np.zeros(2, dtype=np.int32); tok = np.zeros(2, dtype=np.int32)
    ocall = lambda x, rows, V, s, p, t: L.lnb_op_sample(0, x, rows, V, s, p, None, t, None)
    _fails(ocall(None, 2, 16, arr, lnb._p(pos), lnb._p(tok)), L, "null")
    _fails(ocall(lnb._p(row), 2, 16, None, lnb._p(pos), lnb._p(tok)), L, "null")
    _fails(ocall(lnb._p(row), 2, 16, arr, None, lnb._p(tok)), L, "null")
    _fails(ocall(lnb._p(row), 2, 16, arr, lnb._p(pos), None), L, "null")
    _fails(ocall(lnb._p(row), 0, 16, arr, lnb._p(pos), lnb._p(tok)), L, "empty")
    for V in (0, -3, 131073):
        _fails(ocall(lnb._p(row), 2, V, arr, lnb._p(pos), lnb._p(tok)), L, "131072")
    for kw, word in BAD_SAMPLERS:
        bad = (lnb.Sampler * 2)(good, _sampler(lnb, **kw))
        _fails(ocall(lnb._p(row), 2, 16, bad, lnb._p(pos), lnb._p(tok)), L, "row 1", "sampler", word)
    with pytest.raises(lnb.LnbError, match="1 samplers for 2 rows"):
        lnb.op_sample(row, [good], pos)


def test_the_makefile_names_the_header():
    hdrs = re.search(r"^HDRS = (.*)$", open(os.path.join(PKG, "csrc", "Makefile")).read(), re.M).group(1)
    assert "lnb_sample.h" in hdrs
