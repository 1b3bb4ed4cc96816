"""Logit rules (include/lnb.h), without a GPU: the serial C++ definition (csrc/lnb_sample.h, run by tests/native/sample_rules_test.cpp as a stand-alone program under
the address and undefined-behaviour sanitizers) against the numpy restatement (tests/logit_rules_ref.py), case for case -- tokens and every info field."""
import os
import struct
import subprocess

import numpy as np

import logit_rules_ref as lr
import sampler_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_serial_definition_equals_the_restatement(tmp_path):
    exe, path = str(tmp_path / "sample_rules_test"), str(tmp_path / "cases.bin")
    src = os.path.join(ROOT, "tests", "native", "sample_rules_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    V = 1001
    rng = np.random.default_rng(20261126)
    like = sr.llama_like_rows(rng, 4, V)
    crafted = lr.crafted(V)
    rows = np.concatenate([like, np.stack([c[1] for c in crafted])])
    counts = np.concatenate([lr.counted_rows(rng, like), np.stack([c[2] for c in crafted])])
    cases = []                                               # (row = count row, (t, k, p), rules, seed, pos, u)
    for n, (name, rules) in enumerate(lr.rule_sets(V).items()):
        for j, smp in enumerate(lr.SAMPLERS):
            cases.append(((n + j) % 4, smp, rules, sr.SEEDS[j % 3], sr.POSITIONS[(n + j) % 3], None))
    for i, (name, row, c, smp, rules, want, boundaries) in enumerate(crafted):
        cases.append((4 + i, smp, rules, 777, 8, None))
        for u in (sr.boundary_draws(lr.prepare(row, *smp, rules, c)) if boundaries else []):
            cases.append((4 + i, smp, rules, 0, 0, u))
    bias_rows = []
    with open(path, "wb") as f:
        body = b""
        for r, (t, k, p), (rp, pres, freq, min_p, bias), seed, pos, u in cases:
            brow = -1
            if bias:
                b = np.zeros(V, dtype=np.uint16)
                for j, v in bias:
                    b[j] = lr.trunc(np.array([v], dtype=np.float32))[0]
                brow = len(bias_rows); bias_rows.append(b)
            body += struct.pack("<iiiffiQffffiiQ", r, r, brow, t, p, k, seed, rp, pres, freq, min_p, 0 if u is None else 1, 0, pos if u is None else u)
        f.write(struct.pack("<iiiii", rows.shape[0], V, counts.shape[0], len(bias_rows), len(cases)))
        f.write(rows.tobytes() + counts.tobytes() + b"".join(b.tobytes() for b in bias_rows) + body)
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "sample_rules_test: ok (%d cases)" % len(cases) in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    flips = 0
    for (r, smp, rules, seed, pos, u), line in zip(cases, res.stdout.splitlines()):
        v = [int(x) for x in line.split()]
        want, info = lr.sample(rows[r], smp + (seed,), rules, counts[r], pos, u)
        assert (v[0], dict(zip(sr.INFO_FIELDS, v[1:]))) == (want, info), (r, smp, rules, seed, pos, u, v, want, info)
        flips += want != sr.sample(rows[r], smp + (seed,), pos, u)[0]
    assert flips > len(cases) // 4                           # the rules change tokens: a walk that ignored them cannot pass
    for i, (name, row, c, smp, rules, want, _) in enumerate(crafted):      # the crafted rows do what their names say, in the restatement itself
        tok, info = lr.sample(row, smp + (777,), rules, c, 8)
        assert want is None or (tok == want and (sr.sample(row, smp + (777,), 8)[0] != want or "tied" in name)), name
        if name.startswith("min_p_bar"):
            assert info["n_candidates"] == (5 if name.endswith("kept") else 4), (name, info)
