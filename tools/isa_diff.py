#!/usr/bin/env python3
"""Proof that a host-side change left the device code alone: python tools/isa_diff.py <tree A> <tree B>

Compiles csrc/lnb_kernels.hip and csrc/lnb_fast.hip of both source trees to gfx950 assembly (isa_audit.compile_to_asm: the Makefile's code
generation flags), splits each listing into functions by symbol and compares the instruction text of every function.  Reports the symbols only one
tree has and the symbols whose text differs; exit status 0 only when there are none of either.  Needs no GPU.
A function's text = its lines without comments and blank lines, with the function counter taken out of the compiler's local labels
(.LBB12_3 -> .LBB_3: the counter is the function's position in the file, which a host-side change may move)."""
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_audit  # noqa: E402

FILES = ("lnb_kernels.hip", "lnb_fast.hip")


def functions(tree, name):
    with tempfile.TemporaryDirectory() as wd:
        txt = open(isa_audit.compile_to_asm(wd, os.path.join(tree, "llama-nuts-and-bolts_amd", "csrc", name))).read().split("\n")
    out = {}
    for sym, lines in isa_audit.split_functions(txt).items():
        body = (re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1_", ln.split(";")[0].rstrip()) for _, ln in lines)
        out[sym] = [ln for ln in body if ln.strip() and not ln.startswith(".Lfunc_end")]
    return out


def main(tree_a, tree_b):
    bad = 0
    for name in FILES:
        a, b = functions(tree_a, name), functions(tree_b, name)
        only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        differ = sorted(s for s in set(a) & set(b) if a[s] != b[s])
        print("%s: %d / %d functions, only in A %d, only in B %d, differing %d" % (name, len(a), len(b), len(only_a), len(only_b), len(differ)))
        for tag, syms in (("only in A", only_a), ("only in B", only_b), ("differs", differ)):
            for s in syms:
                print("    %s: %s" % (tag, s))
        bad += len(only_a) + len(only_b) + len(differ) + (0 if a else 1)
    print("isa_diff:", "identical" if not bad else "DIFFERENT")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
