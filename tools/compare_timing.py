"""Times l3d_compare_lines on a BASELINE configuration after matchImages and reconstruct3Dlines(3): the
model against a copy of itself whose end points are jittered by 1e-4 of the extent, under four slicings of the
references -- one slice that holds all chunks (the unsliced form of §17, the baseline), slices for 1024 workgroups
(clamp(ceil(1024 / tiles), 1, chunks): the rule the stage started from), the library's default, and one chunk per slice.
Per slicing: the wall time of the call and the kernel time by HIP events (timing level 2), median of the last seven of
nine calls in a warm process, and the slices of the last direction.  With `model` the array form of the numpy model
(tests/compare_model.py) is timed on the same input and compared.
    python tools/compare_timing.py C1 model
    python tools/compare_timing.py C2
Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  -- first, as tests/conftest.py does
from line3dpp_amd import _lib, api
from line3dpp_amd.api import Line3D
from line3dpp_amd.scene import make_config
from tests import compare_model as M

cfg = sys.argv[1]; with_model = len(sys.argv) > 2 and sys.argv[2] == "model"
t0 = time.time()
sc = make_config(cfg)
g = Line3D(); g.add_scene(sc)
t1 = time.time()
assert g.matchImages() and g.reconstruct3Dlines(3)
t2 = time.time()
L = _lib.load()
segs, line = api.flatten_lines(g.get3Dlines())
extent = M.extent(segs)
other = np.ascontiguousarray(segs + np.random.default_rng(1).uniform(-1e-4 * extent, 1e-4 * extent, segs.shape))
max_distance = 1e-3 * extent
mine = np.zeros(len(segs), _lib.LINE_MATCH_DTYPE); theirs = np.zeros(len(segs), _lib.LINE_MATCH_DTYPE)
s_mine = _lib.CompareSummary(); s_other = _lib.CompareSummary()
g.setTimingLevel(2)
res = dict(config=cfg, build=L.l3d_build_info().decode(), segments_3d=len(segs), lines=int(line.max()) + 1 if len(line) else 0,
           extent=extent, max_distance=max_distance, pair_tests=2 * len(segs) * len(segs), setup_s=t1 - t0, match_reconstruct_s=t2 - t1)
first = None
n_tiles = n_chunks = -(-len(segs) // 256)
aim_1024 = -(-n_chunks // min(max(-(-1024 // n_tiles), 1), n_chunks))
for name, chunks in (("one_slice", 0xFFFFFFFF), ("aim_1024_workgroups", aim_1024), ("default", 0), ("one_chunk_per_slice", 1)):
    par = api.compare_params(max_distance, 10.0, 0.5, False, chunks)
    wall, kern = [], []
    for it in range(9):
        a = time.perf_counter()
        rc = L.l3d_compare_lines(g.h, len(other), _lib.ptr(other), _lib.ptr(line), C.byref(par), _lib.ptr(mine), _lib.ptr(theirs),
                                 C.byref(s_mine), C.byref(s_other))
        b = time.perf_counter()
        assert rc == 0, _lib.last_error()
        if it >= 2:
            wall.append((b - a) * 1e3); kern.append(L.l3d_debug_counter(b"compare_kernel_ns") / 1e6)
    if first is None:
        first = (mine.copy(), theirs.copy())
    res[name] = dict(slices=int(L.l3d_debug_counter(b"compare_slices")), wall_ms_median=float(np.median(wall)),
                     wall_ms_all=[round(w, 3) for w in wall], kernel_ms_median=float(np.median(kern)), kernel_ms_all=[round(k, 4) for k in kern],
                     same_bytes_as_one_slice=bool(mine.tobytes() == first[0].tobytes() and theirs.tobytes() == first[1].tobytes()))
g.setTimingLevel(1)
res["summary_mine"] = api.summary_dict(s_mine); res["summary_other"] = api.summary_dict(s_other)
if with_model:
    a = time.perf_counter()
    want = M.compare_both(segs, line, other, line, max_distance, par.min_cos2, 0.5)
    res["numpy_model_ms"] = (time.perf_counter() - a) * 1e3
    res["equals_model"] = bool(mine.tobytes() == want[0].tobytes() and theirs.tobytes() == want[1].tobytes())
print(json.dumps(res))
g.close()
