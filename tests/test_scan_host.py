"""CPU tests of the scan's test hook (l3d_selftest_scan): the symbol, and the argument errors, which are returned before
any device call.  No device call is made here."""
import ctypes as C

import numpy as np

from line3dpp_amd import _lib
from tests.scan_cases import selftest_scan

L3D_ERR_ARG = -1


def test_library_exports_the_scan_hook():
    assert hasattr(_lib.load(), "l3d_selftest_scan") and "l3d_selftest_scan" in _lib.EXPORTS


def test_scan_hook_argument_errors_need_no_device():
    L = _lib.load()
    data = np.arange(10, dtype=np.uint32)
    n = np.array([3, 10], np.uint32)
    out = np.zeros(15, np.uint32); tot = np.zeros(2, np.uint32)
    dirty, guard = C.c_uint64(7), C.c_uint64(7)
    p = _lib.ptr

    def call(eb=4, data=p(data), n_in=10, n_calls=2, n=p(n), total=1, out=p(out), tot=p(tot), d=C.byref(dirty), g=C.byref(guard)):
        return L.l3d_selftest_scan(0, eb, data, n_in, n_calls, n, 0, total, out, tot, d, g)

    for eb in (0, 1, 2, 3, 5, 16):
        assert call(eb=eb) == L3D_ERR_ARG and "4 or 8" in _lib.last_error()
    for kw in (dict(data=None), dict(n=None), dict(out=None), dict(tot=None), dict(d=None), dict(g=None)):
        assert call(**kw) == L3D_ERR_ARG and "null" in _lib.last_error(), kw
    assert call(n_in=9) == L3D_ERR_ARG and "longer than the input" in _lib.last_error()
    long = np.array([11, 0], np.uint32)
    assert call(n=p(long)) == L3D_ERR_ARG
    assert not out.any() and not tot.any() and dirty.value == 7 and guard.value == 7
    rc, regions, totals, d, g = selftest_scan(np.zeros(4, np.uint64), [5])
    assert rc == L3D_ERR_ARG and (regions[0] == 0x77).all()           # untouched
    # no call at all: nothing to do, and no device is needed to say so
    assert call(n_calls=0) == 0 and dirty.value == 0 and guard.value == 0
