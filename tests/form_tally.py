"""The launch tally from a test (csrc/lnb_forms.h, lnb_form_count): `with ran(lnb, "gemm_mfma.t64", epi="resid", not_ran=("gemm_stream",)):` resets the
tally, runs the body and asserts that the named form was launched with that epilogue and that nothing under a `not_ran` prefix was.  A test that forces
a kernel form through an LNB_* knob says so this way: a ONCE knob set after its first use changes nothing, and without the tally the test would pass on
the default form.  tests/test_form_coverage_cpu.py reads the names written in these calls."""
import contextlib


def under(lnb, prefix):
    """the table's names a prefix stands for: the name itself, or every name below it ("gemm_stream" -> "gemm_stream.copy.ntw1", ...; never "gemm_stream_order.*")"""
    names = [n for n in lnb.form_names() if n == prefix or n.startswith(prefix + ".")]
    assert names, "no kernel form is called %r or lies under it (csrc/lnb_forms.h)" % prefix
    return names


def count(lnb, prefix, epi=None):
    return sum(lnb.form_count(n, epi) for n in under(lnb, prefix))


def snapshot(lnb):
    """{(form, epilogue name): launches} of everything that ran since the last reset (for messages)"""
    return {(n, e): lnb.form_count(n, e) for n in lnb.form_names() for e in lnb.EPILOGUES if lnb.form_count(n, e)}


def _tuple(x):
    return (x,) if isinstance(x, (str, int)) or x is None else tuple(x)


@contextlib.contextmanager
def ran(lnb, form, epi=None, not_ran=()):
    """form: a name or prefix, or several (each must have run); epi: an epilogue name of lnb.EPILOGUES, several (each form must have run with each), or None
    (any).  form may also be a dict {name or prefix: epilogue(s)} when the forms differ in their epilogues.  not_ran: names or prefixes with no launch at all
    in the body.  The tally is left as the body made it: the caller may go on to compare counts."""
    want = form if isinstance(form, dict) else {f: epi for f in _tuple(form)}
    lnb.form_count_reset()
    yield
    seen = snapshot(lnb)
    for f, epis in want.items():
        for e in _tuple(epis):
            assert count(lnb, f, e) > 0, "kernel form %s%s did not run; the tally: %s" % (f, "" if e is None else " with epilogue " + str(e), seen)
    for f in _tuple(not_ran):
        assert count(lnb, f) == 0, "kernel form %s ran and should not have; the tally: %s" % (f, seen)
