"""Scaffolding of tests/test_guarded_gpu.py (a plain module): the guarded-allocation switch of the parity library as a context manager.

Inside `with guarded():` every device allocation the parity library makes lies between two guard bands, and guards and payload start
as a poison pattern whose aligned 32-bit words are quiet NaNs (tandem_amd/csrc/guard_host.h).  On exit the guards of everything still
alive are compared with the pattern, together with what was found when buffers were freed inside the block.  Use it with the
`parity_hooks` fixture: the product library has no guards and answers DR_ERR_UNSUPPORTED."""
import contextlib
import ctypes as C

import numpy as np

POISON_WORD = 0x7FC5A5A5  # guard_host.h kWord (tests/test_guard_host.py holds the two together)


def check():
    """dr_guard_check: ({live, guarded, violations, bytes}, report text)."""
    from tandem_amd import _lib
    out = (C.c_uint64 * 4)()
    buf = C.create_string_buffer(1 << 16)
    _lib.check(_lib.lib().dr_guard_check(out, buf, len(buf)))
    return dict(live=int(out[0]), guarded=int(out[1]), violations=int(out[2]), bytes=int(out[3])), buf.value.decode(errors="replace")


@contextlib.contextmanager
def guarded(G=4096):
    """Guards of G bytes around every allocation made inside the block.  Leaves with guards off; asserts that nothing wrote into a
    guard and that the block did allocate under guards (so a test cannot pass by running unguarded)."""
    from tandem_amd import _lib
    L = _lib.lib()
    _lib.check(L.dr_guard_clear())
    _lib.check(L.dr_guard_set(G))
    try:
        yield
    except BaseException:
        L.dr_guard_set(0)
        L.dr_guard_clear()
        raise
    _lib.check(L.dr_guard_set(0))
    st, report = check()
    _lib.check(L.dr_guard_clear())
    assert st["violations"] == 0, "%d guard violation(s):\n%s" % (st["violations"], report)
    assert st["guarded"] > 0, "nothing was allocated under guards"


def bits(a):
    """The bit pattern of an output: uint32 for floats, the bytes themselves otherwise."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


def assert_no_nan(a, what):
    a = np.asarray(a)
    if a.dtype.kind == "f":
        n = int(np.isnan(a).sum())
        poison = int((bits(a) == POISON_WORD).sum()) if a.dtype == np.float32 else 0
        assert n == 0, "%s: %d NaN of %d, %d of them the poison word (elements nobody wrote)" % (what, n, a.size, poison)


def assert_same_bits(a, b, what):
    """a: computed under guards, b: the same call with guards off.  Bit-identical, and no NaN in either."""
    a, b = np.asarray(a), np.asarray(b)
    assert_no_nan(a, what + " (guards on)")
    assert_no_nan(b, what + " (guards off)")
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(bits(a), bits(b)), "%s: %d of %d elements differ between guards on and off" % (what, int((bits(a) != bits(b)).sum()), bits(a).size)
