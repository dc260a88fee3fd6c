"""The test hook of the single-launch scan (k_scan.hip; l3d_selftest_scan) as a function, shared by the CPU and the GPU
tests of the scan."""
import ctypes as C

import numpy as np

from line3dpp_amd import _lib

TILE = 4096                       # elements of a scan tile: 1024 threads x 4 items
WINDOW = 64                       # predecessors a tile looks back at per step


def selftest_scan(data, lengths, in_place=False, pass_total=True, device=0):
    """-> (status, [out region of n + 1 elements per length], totals or None, non-zero work-space words, changed guard words)"""
    L = _lib.load()
    data = np.ascontiguousarray(data)
    assert data.dtype in (np.uint32, np.uint64)
    n = np.asarray(lengths, np.uint32)
    out = np.full(int(n.astype(np.int64).sum()) + len(n) + 1, 0x77, data.dtype)
    totals = np.full(len(n) + 1, 0x77, data.dtype)
    dirty, guard = C.c_uint64(99), C.c_uint64(99)
    rc = L.l3d_selftest_scan(device, data.dtype.itemsize, _lib.ptr(data), len(data), len(n), _lib.ptr(n), int(in_place), int(pass_total),
                             _lib.ptr(out), _lib.ptr(totals) if pass_total else None, C.byref(dirty), C.byref(guard))
    regions, at = [], 0
    for k in n:
        regions.append(out[at:at + int(k) + 1])
        at += int(k) + 1
    return rc, regions, totals[:len(n)] if pass_total else None, dirty.value, guard.value
