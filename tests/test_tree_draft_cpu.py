"""A tree of n-gram drafts per verify pass (include/lnb.h, lnb_ctx_set_draft_branches / lnb_op_tree_draft): the trie rule restated in numpy and held to
hand-made tries, the loop's passes simulated from it, and what can be checked of the two calls without a GPU.  tests/test_gpu_tree_verify.py compares
tree_draft_kernel and the decode loop's stats with ref_tree / simulate."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lnb_ctx_set_draft_branches", "lnb_op_tree_draft")


def ref_tree(R, C, nmin, nmax, max_draft, branches, cap=16):
    """longest n first; the up to `branches` latest starts of R's last n tokens, R latest first, then C; merged in that order while a node is left"""
    R, C, cands = [int(t) for t in R], [int(t) for t in C], []
    for n in range(nmax, nmin - 1, -1):
        if n <= len(R):
            cands = [a[j + n:j + n + max_draft] for a in (R, C) for j in range(len(a) - n - 1, -1, -1) if a[j:j + n] == R[len(R) - n:]][:branches]
        if cands:
            break
    tok, par, dep = [-1], [-1], [0]
    for cand in cands:
        cur = 0
        for x in cand:
            kid = next((i for i in range(1, len(tok)) if par[i] == cur and tok[i] == x), None)
            if kid is None:
                if len(tok) >= cap:
                    break
                tok.append(x); par.append(cur); dep.append(dep[cur] + 1); kid = len(tok) - 1
            cur = kid
    return tok, par, dep


def simulate(history, token, out, C, nmin, nmax, max_draft, branches, max_steps, seq_len, start_pos):
    """the passes of the speculative loop over its known output -> (lnb_spec_stats as a dict, [(pos, accepted path)] per pass)"""
    out, g, s, passes = [int(t) for t in out], 0, dict(passes=0, verify_passes=0, drafted=0, accepted=0), []
    while g < len(out):
        pos = start_pos + g
        lim = max(min(max_draft, max_steps - g - 1, seq_len - pos - 1), 0)
        tok, par, _ = ref_tree([int(t) for t in history] + [int(token)] + out[:g], C, nmin, nmax, lim, branches, min(16, seq_len - pos))
        path = [0]
        while g + len(path) <= len(out):
            kid = next((i for i in range(1, len(tok)) if par[i] == path[-1] and tok[i] == out[g + len(path) - 1]), None)
            if kid is None or g + len(path) == len(out):
                break
            path.append(kid)
        s["passes"] += 1; s["verify_passes"] += len(tok) > 1; s["drafted"] += len(tok) - 1
        passes.append((pos, path))
        g += len(path)
    s["accepted"] = len(out) - s["passes"]
    return s, passes


CASES = {   # (R, C, nmin, nmax, max_draft, branches) -> (tokens, parent, depth)
    "one match": (([1, 2, 3, 9, 1, 2], [], 2, 2, 4, 4), ([-1, 3, 9, 1, 2], [-1, 0, 1, 2, 3], [0, 1, 2, 3, 4])),
    "two matches sharing a prefix": (([5, 6], [5, 6, 7, 8, 1, 0, 5, 6, 7, 9, 2], 1, 2, 3, 2), ([-1, 7, 9, 2, 8, 1], [-1, 0, 1, 2, 1, 4], [0, 1, 2, 3, 2, 3])),
    "four matches overflowing 16 nodes": (([4], sum(([4] + [10 * b + i for i in range(6)] for b in range(4)), []) + [0], 1, 1, 6, 4),
                                          ([-1] + [30 + i for i in range(6)] + [20 + i for i in range(6)] + [10, 11, 12],
                                           [-1, 0, 1, 2, 3, 4, 5, 0, 7, 8, 9, 10, 11, 0, 13, 14], [0, 1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6, 1, 2, 3])),
    "a match cut at the array end": (([1, 2, 8, 8, 1, 2], [1, 2, 3], 2, 2, 5, 2), ([-1, 8, 8, 1, 2, 3], [-1, 0, 1, 2, 3, 0], [0, 1, 2, 3, 4, 1])),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_restated_rule_builds_the_hand_made_trie(name):
    args, want = CASES[name]
    assert ref_tree(*args) == want


def test_the_calls_are_declared_bound_documented_and_check_their_arguments_first():
    import lnb
    lnb.build()
    L = lnb.lib()
    hdr = open(os.path.join(ROOT, "include", "lnb.h")).read()
    for name in NEW:
        assert name in lnb.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, hdr) and hasattr(L, name)
    for rel in ("llama-nuts-and-bolts_amd/host/lnb_host.hpp", "llama-nuts-and-bolts_amd/go/inferencecontext_hip.go", "README.md", "DESIGN.md", "INTEGRATION.md"):
        assert NEW[0] in open(os.path.join(ROOT, rel)).read(), rel
    assert re.search(r"#define\s+LNB_MAX_DRAFT_BRANCHES\s+%d\b" % lnb.MAX_DRAFT_BRANCHES, hdr)
    junk = np.full(4096, 0xFF, dtype=np.uint8)               # a handle of all ones: touching it would end the process
    for bad in (0, -1, 5):
        assert L.lnb_ctx_set_draft_branches(junk.ctypes.data, bad) < 0 and b"1..4" in L.lnb_last_error()
    assert L.lnb_ctx_set_draft_branches(None, 2) < 0 and b"null" in L.lnb_last_error()
    t = np.arange(16, dtype=np.int32); n = np.zeros(1, dtype=np.int32)
    for nb in (0, 5):
        assert L.lnb_op_tree_draft(0, lnb._p(t), 4, None, 0, 1, 4, 7, nb, lnb._p(t), lnb._p(t), lnb._p(t), n.ctypes.data_as(lnb.C.POINTER(lnb.C.c_int))) < 0
        assert b"n_branches" in L.lnb_last_error()
