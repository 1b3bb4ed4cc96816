"""The measurement code stays out of the production decode kernels (CPU; profiles/prologue_fetch.md).

Every decode kernel family exists twice: the production instantiation (TIMING = false: no clock read, no stamp, one s_barrier per barrier) and the TIMING
instantiation the launch functions pick when GemvParams.dbg / AttnParams.dbg is set (lnb_profile_kernel_stamps, LNB_GEMV_TIMING).  Read from the disassembly of
the gfx950 code object inside the built library (tools/code_footprint.py) -- the code that ships, not a second compile:
  * no production instantiation reads the shader clock or the wall clock,
  * every TIMING instantiation does, and every production instantiation has one,
  * the four kernels of an 8B decode token are smaller than they were with both timing modes compiled in."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "llama-nuts-and-bolts_amd"))
import code_footprint as cf  # noqa: E402

# ELF symbol sizes of the four production kernels in the parent of this change (hipcc -O3 --offload-arch=gfx950, the tree's flags), and the compiler they were
# measured with: another compiler's sizes say nothing about this change, so the comparison is skipped there
PARENT_BYTES = {"wq|wk|wv": 35420, "wo, w2": 39024, "gate|up": 35336, "head": 36116}
PARENT_HIPCC = ("HIP version: 7.2.26015-fc0010cf6a", "roc-7.2.0 26014 7b800a19466229b8479a78de19143dc33c3ab9b5")


@pytest.fixture(scope="module")
def kernels():
    import lnb
    lnb.build()
    ks = cf.load([])
    assert len(ks) >= 60, "the decode kernels of the built library: %d found" % len(ks)
    return ks


def clock_reads(ins):
    return [t for _, t in ins if t.split()[0] in cf.CLOCK_READS]


def test_no_production_decode_kernel_reads_a_clock(kernels):
    prod = {n: v for n, v in kernels.items() if not cf.is_timing(n)}
    assert {f for f in cf.DECODE_FAMILIES if any(re.match(r"_Z\d+%sI" % f, n) for n in prod)} == set(cf.DECODE_FAMILIES)
    bad = {n: clock_reads(ins)[:3] for n, (_, ins) in prod.items() if clock_reads(ins)}
    assert not bad, "production instantiations that read a clock: %s" % bad


def test_every_timing_instantiation_reads_the_clock_and_every_production_kernel_has_one(kernels):
    timing = {n: v for n, v in kernels.items() if cf.is_timing(n)}
    assert len(timing) >= 30
    dry = [n for n, (_, ins) in timing.items() if not clock_reads(ins)]
    assert not dry, "TIMING instantiations without a clock read: %s" % dry
    orphans = [n for n in timing if cf.timing_partner(n) not in kernels]
    assert not orphans, "TIMING instantiations without a production twin: %s" % orphans
    # the four kernels of a decode token and every other GEMV form: each can be stamped
    twins = {cf.timing_partner(n) for n in timing}
    gemv = [n for n in kernels if not cf.is_timing(n) and re.match(r"_Z\d+(?:gemv_chain|gemv_chain_pk|gemv_quad|rowcast|rowcast_lds)_kernelI", n)]
    assert len(gemv) >= 40 and not [n for n in gemv if n not in twins], [n for n in gemv if n not in twins]


def test_the_four_kernels_of_a_decode_token_are_smaller_than_with_the_timing_code(kernels):
    rows = cf.footprint(kernels)
    prod = {label.split("  ")[0].strip(): (total, at) for label, variant, total, at in rows if variant == "production"}
    timing = {label.split("  ")[0].strip(): total for label, variant, total, at in rows if variant == "timing"}
    assert set(prod) == set(PARENT_BYTES) == set(timing)
    for k, (total, at) in prod.items():
        print("%-10s production %6d bytes (parent %6d), main loop at %s; timing %6d" % (k, total, PARENT_BYTES[k], at, timing[k]))
        assert at is not None and 0 < at < total, "no main-loop marker in %s" % k
        assert total < timing[k], "%s: the production instantiation is no smaller than its TIMING twin" % k
    ver = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout
    if not all(s in ver for s in PARENT_HIPCC):
        pytest.skip("another hipcc than the parent's sizes were measured with: %s" % ver.split("\n")[0])
    for k, (total, _) in prod.items():
        assert total < PARENT_BYTES[k], "%s: %d bytes, the parent's %d" % (k, total, PARENT_BYTES[k])
