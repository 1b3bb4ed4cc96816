"""The pass structure of the speculative loops, restated (a helper module, as sampler_ref.py): the n-gram draft rule, the passes of
lnb_decode_speculative_until and the passes and grants of lnb_decode_speculative_many over a KNOWN output -- so the stats of a run follow from its tokens
alone, whether the tokens are argmaxes or a sampler's.  Shared by tests/test_spec_sample_cpu.py (the CPU chains: the conditions that keep the GPU test from
being empty) and tests/test_gpu_spec_sample.py.  Also the CPU chain itself: oracle one-token step, sampler_ref.sample, feed the token."""
import numpy as np

from oracle import oracle as orc
import sampler_ref as sr

SAMPLERS = ((1.0, 0, 1.0), (0.7, 40, 0.9), (1.5, 0, 0.5))    # (temperature, top_k, top_p)
P0, STEPS, SEQ, NMIN, NMAX = 8, 40, 64, 1, 4
# The seed of each sampler's chain: the first seed from 777 upwards whose chain meets every condition of tests/test_spec_sample_cpu.py (that file says why 777 itself
# meets them for no sampler, and lists what the simulation gave for the seeds in use).
SEEDS = {SAMPLERS[0]: 1083, SAMPLERS[1]: 786, SAMPLERS[2]: 955}
PROMPT_SEED, MODEL_SEED = 99, 1234


def ref_draft(R, C, nmin, nmax, max_draft):
    """longest n first; an earlier occurrence of R's last n tokens followed by at least one token of its array; R before C; latest start"""
    R, C = [int(t) for t in R], [int(t) for t in C]
    L = len(R)
    for n in range(nmax, nmin - 1, -1):
        if n > L:
            continue
        suf = R[L - n:]
        for arr in (R, C):
            for j in range(len(arr) - n - 1, -1, -1):
                if arr[j:j + n] == suf:
                    return arr[j + n:j + n + max_draft]
    return []


def simulate(history, token, out, corpus, nmin, nmax, max_draft, max_steps, seq_len, start_pos, widths=None):
    """the passes of lnb_decode_speculative[_sample]_until over its known output; widths (a set, optional) receives the column counts of the passes with a draft"""
    out = [int(t) for t in out]
    n, g = len(out), 0
    s = dict(passes=0, verify_passes=0, drafted=0, accepted=0)
    while g < n:
        R = [int(t) for t in history] + [int(token)] + out[:g]
        lim = min(max_steps - g - 1, seq_len - (start_pos + g) - 1)
        d = ref_draft(R, corpus, nmin, nmax, max_draft)[:max(lim, 0)] if max_draft > 0 else []
        s["passes"] += 1
        if d:
            s["verify_passes"] += 1
            s["drafted"] += len(d)
            if widths is not None:
                widths.add(len(d) + 1)
        a = 0
        while a < len(d) and g + a < n and d[a] == out[g + a]:
            a += 1
        g += min(a + 1, n - g)
    s["accepted"] = n - s["passes"]
    return s


def simulate_many(members, budget, max_steps, nmin, nmax):
    """the passes of lnb_decode_speculative[_sample]_many over its known outputs.  members: dicts with history, token, out (what the member's own loop
    emits in this call), corpus, md, seq_len, start (None: skipped) -> (per-member stats, info without long_passes)"""
    n = len(members)
    budget = budget or 16 * -(-n // 16)
    g = [0] * n
    stats = [dict(passes=0, verify_passes=0, drafted=0, accepted=0) for _ in range(n)]
    info = dict(passes=0, verify_passes=0, columns=0, max_columns=0)
    while True:
        A = [s for s in range(n) if members[s]["start"] is not None and g[s] < len(members[s]["out"])]
        if not A:
            break
        want = {}
        for s in A:
            m = members[s]
            out = [int(t) for t in m["out"]]
            R = [int(t) for t in m["history"]] + [int(m["token"])] + out[:g[s]]
            lim = min(max_steps - g[s] - 1, m["seq_len"] - (m["start"] + g[s]) - 1)
            want[s] = ref_draft(R, m["corpus"], nmin, nmax, m["md"])[:max(lim, 0)] if m["md"] > 0 else []
        cols = {s: 1 for s in A}
        left = budget - len(A)
        for j in range(1, 16):                               # the grant rule: level by level, members in order, while columns are left
            for s in A:
                if len(want[s]) >= j and left > 0:
                    cols[s] += 1
                    left -= 1
        width = sum(cols.values())
        info["passes"] += 1
        info["verify_passes"] += 1 if any(c > 1 for c in cols.values()) else 0
        info["columns"] += width
        info["max_columns"] = max(info["max_columns"], width)
        for s in A:
            out = [int(t) for t in members[s]["out"]]
            d = want[s][:cols[s] - 1]
            st = stats[s]
            st["passes"] += 1
            st["verify_passes"] += 1 if d else 0
            st["drafted"] += len(d)
            a = 0
            while a < len(d) and g[s] + a < len(out) and d[a] == out[g[s] + a]:
                a += 1
            g[s] += min(a + 1, len(out) - g[s])
    for s in range(n):
        stats[s]["accepted"] = len(members[s]["out"]) - stats[s]["passes"] if members[s]["start"] is not None else 0
    return stats, info


def corpus(kind, chain, V):
    """chain = first token + the generated tokens: uncorrupted / every 2nd / every 5th token wrong / empty"""
    if kind == "none":
        return []
    c = np.array(chain, dtype=np.int32).copy()
    m = {"exact": 0, "every2": 2, "every5": 5}[kind]
    if m:
        c[m - 1::m] = (c[m - 1::m] + 1) % V
    return c


def oracle_chain(om, prompt, smp, seed, steps, seq_len=SEQ, nthreads=None):
    """oracle one-token step, sampler_ref.sample, feed the token: what lnb_decode_sample_until(first, len(prompt), steps) must emit
    -> (the prompt's argmax, the sampled tokens, how many of them are their row's argmax)"""
    c = orc.Context(om, seq_len, nthreads)
    row, first = c.forward(prompt, 0)
    tok, toks, greedy = first, [], 0
    for i in range(steps):
        row, _ = c.forward(np.array([tok], dtype=np.int32), len(prompt) + i)
        r16 = orc.f32_to_bf16(np.ascontiguousarray(row[-1], dtype=np.float32))
        tok, _ = sr.sample(r16, tuple(smp) + (seed,), pos=len(prompt) + i)
        greedy += tok == sr.argmax(r16)
        toks.append(tok)
    c.close()
    return int(first), np.array(toks, dtype=np.int32), int(greedy)


_CHAINS = {}


def tiny_chains():
    """the three samplers' chains on oracle.TINY (computed once per process) -> (cfg, prompt, {sampler: (first, tokens, greedy count)})"""
    if not _CHAINS:
        cfg = dict(orc.TINY)
        om = orc.Model(**cfg).fill_synthetic(MODEL_SEED).finalize()
        prompt = orc.synth_tokens(PROMPT_SEED, P0, cfg["vocab_size"])
        _CHAINS["v"] = (cfg, prompt, {smp: oracle_chain(om, prompt, smp, SEEDS[smp], STEPS, nthreads=1) for smp in SAMPLERS})
        om.close()
    return _CHAINS["v"]
