"""Speculative decoding under a token automaton (include/lnb.h: lnb_decode_speculative_automaton_until) in numpy -- a helper module shared by
tests/test_spec_automaton_cpu.py and tests/test_gpu_spec_automaton.py: the draft filter (walk, cut, extend) and one verify pass (column states, delta counts,
acceptance, emission), on tests/automaton_ref.py's CSR triples and tests/logit_rules_ref.py's sampler."""
import numpy as np

import automaton_ref as ar
import logit_rules_ref as lr


def final(dfa, s):
    return dfa[0][s + 1] == dfa[0][s]


def filter_draft(dfa, state, draft, max_draft):
    """-> (the kept and extended draft, the column states s_0 .. s_k); state is not final (the call refuses a final state up front)"""
    out, states, s = [], [state], state
    for t in draft:
        if t not in ar.allowed(dfa, s):
            break                                            # a forbidden guess never takes a column
        s = ar.walk(dfa, s, t)
        out.append(int(t)); states.append(s)
        if final(dfa, s):
            break
    while len(out) < max_draft and not final(dfa, s) and ar.allowed(dfa, s).size == 1:
        out.append(int(ar.allowed(dfa, s)[0]))
        s = int(dfa[2][dfa[0][s]])
        states.append(s)
    return out, states


def verify_pass(rows, dfa, s0, smp, rules, counts, pos0, col_tokens, stop=()):
    """one verify pass -> (emitted tokens, finished, end state, counts after, accepted columns a)"""
    w, states = len(col_tokens), [s0]
    for t in col_tokens[1:]:
        states.append(ar.walk(dfa, states[-1], t))
    g = []
    for i in range(w):                                       # column i: the rules step on the row masked by its state, the drafts in front of it counted
        c = np.asarray(counts, dtype=np.uint32) + np.bincount(np.asarray(col_tokens[1:i + 1], dtype=np.int64), minlength=rows.shape[1]).astype(np.uint32)
        g.append(int(lr.sample(ar.mask_row(rows[i], dfa, states[i]), smp, rules, c, pos0 + i)[0]))
    a = 0
    while a < w - 1 and g[a] == col_tokens[a + 1]:
        a += 1
    out, state, after, fin = [], s0, np.array(counts, dtype=np.uint32), False
    for i in range(a + 1):
        out.append(g[i])
        if g[i] >= 0:
            after[g[i]] += 1
            state = ar.walk(dfa, states[i], g[i])
        if g[i] in stop or (g[i] >= 0 and final(dfa, state)):
            fin = True
            break
    return out, fin, state, after, a
