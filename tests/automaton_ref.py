"""The token automaton of include/lnb.h ("a token automaton in the sampling loops") in numpy -- a helper module shared by tests/test_automaton_cpu.py and
tests/test_gpu_automaton.py.  An automaton is (row_ptr int64 [n + 1], edge_token int32, edge_next int32): CSR over states, tokens ascending inside a row,
an empty row = a final state.  Step 0d = "every entry outside the state's row is -inf", so the reference is tests/logit_rules_ref.py on a pre-masked row."""
import functools

import numpy as np

import logit_rules_ref as lr
import sampler_ref as sr

N_STATES = 61            # prime: edge_next = (a + rank) mod 61 inside a row, so a rank off by one, a 32-bit word or a lane's words lands in another state
SAMPLERS = ((0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 40, 0.9))
PENALTIES = (1.3, 0.5, 0.25, 0.02, ())


def build(rows, n_states=N_STATES):
    """rows: one ascending id array per state (missing states: final) -> the CSR triple"""
    rows = [np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, dtype=np.int32)] * (n_states - len(rows))
    row_ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    nxt = [(7 * s + 3 + np.arange(r.size)) % n_states for s, r in enumerate(rows)]
    return row_ptr, np.concatenate(rows).astype(np.int32), np.concatenate(nxt).astype(np.int32)


def random_rows(rng, n, V, density=1 / 8):
    return [np.nonzero(rng.random(V) < density)[0] for _ in range(n)]


def allowed(dfa, state):
    return dfa[1][dfa[0][state]:dfa[0][state + 1]]


def mask_row(row_u16, dfa, state):
    out = np.full(row_u16.size, lr.NINF, dtype=np.uint16)
    ids = allowed(dfa, state)
    out[ids] = np.asarray(row_u16, dtype=np.uint16)[ids]
    return out


def walk(dfa, state, tok):
    """the state behind token tok (-1: the state itself)"""
    if tok < 0:
        return state
    ids = allowed(dfa, state)
    k = int(np.searchsorted(ids, tok))
    assert k < ids.size and ids[k] == tok, "token %d is not allowed in state %d" % (tok, state)
    return int(dfa[2][dfa[0][state] + k])


@functools.lru_cache(maxsize=None)
def op_cases(V):
    """-> (dfa, cases): every (row, state) pair of two llama-like and two crafted rows with the states 0 = one allowed token, 1 = everything, 2 = {0, 31, 32,
    33, V - 1}, 3..6 = random rows of density 1/8; samplers and rule sets (off / penalties) alternate over the pairs.
    case = (row, counts, sampler + (seed,), rules, pos, state, token wanted, state wanted, unconstrained token)"""
    rng = np.random.default_rng(20261127 + V)
    llama = sr.llama_like_rows(rng, 2, V)
    crafted = [c for c in lr.crafted(V) if c[0] in ("repetition_flips_a_positive_maximum", "presence_flips_the_maximum")][:2]
    rows = [(llama[i], lr.counted_rows(rng, llama)[i]) for i in range(2)] + [(c[1], c[2]) for c in crafted]
    dfa = build([[V // 3], np.arange(V), [0, 31, 32, 33, V - 1]] + random_rows(rng, 4, V))
    cases = []
    for i, ((row, counts), state) in enumerate((r, s) for r in rows for s in range(7)):
        smp = SAMPLERS[i % 3] + (sr.SEEDS[i % 3],)
        rules = (lr.OFF, PENALTIES)[(i // 3) % 2]
        pos = sr.POSITIONS[i % 3]
        tok = lr.sample(mask_row(row, dfa, state), smp, rules, counts, pos)[0]
        cases.append((row, counts, smp, rules, pos, state, tok, walk(dfa, state, tok), lr.sample(row, smp, rules, counts, pos)[0]))
    return dfa, cases
