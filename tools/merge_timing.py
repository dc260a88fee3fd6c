"""Times l3d_merge_lines on a BASELINE configuration after matchImages and reconstruct3Dlines(3), with
max_distance = 1e-3 of the extent, 10 degrees and 0.5.  The call replaces the context's lines, so every timed call is
preceded by a fresh reconstruct3Dlines(3) outside the timed region: nine calls in a warm process, the median of the last
seven with its range, of the wall time of the whole call and of the kernel time by HIP events (timing level 2: the count
pass with its scan, and the write pass).  The stateless l3d_merge_segments on the same model is timed beside it (wall
only), and with `model` the numpy model (tests/merge_model.py) on the same input, which is compared byte for byte.
    python tools/merge_timing.py C1 model
    python tools/merge_timing.py C2
Prints one JSON line."""
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
from tests import merge_model as M

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
max_distance = 1e-3 * extent
res = dict(config=cfg, build=L.l3d_build_info().decode(), segments_3d=len(segs), lines=int(line.max()) + 1 if len(line) else 0,
           extent=extent, max_distance=max_distance, pair_tests=len(segs) * len(segs), setup_s=t1 - t0, match_reconstruct_s=t2 - t1)


def spread(v):
    return dict(median=float(np.median(v)), lo=float(min(v)), hi=float(max(v)), all=[round(x, 4) for x in v])


g.setTimingLevel(2)
wall, kern = [], []
summary = None
for it in range(9):
    if it:
        assert g.reconstruct3Dlines(3)
    a = time.perf_counter()
    summary = g.mergeLines(max_distance)
    b = time.perf_counter()
    assert summary is not None
    if it >= 2:
        wall.append((b - a) * 1e3); kern.append(L.l3d_debug_counter(b"merge_kernel_ns") / 1e6)
g.setTimingLevel(1)
merged_segs, merged_line = api.flatten_lines(g.get3Dlines())
res["context"] = dict(slices=int(L.l3d_debug_counter(b"merge_slices")), wall_ms=spread(wall), kernel_ms=spread(kern))
res["summary"] = summary
free = None
wall = []
for it in range(9):
    a = time.perf_counter()
    free = api.merge_segments(segs, line, max_distance)
    b = time.perf_counter()
    if it >= 2:
        wall.append((b - a) * 1e3)
res["stateless"] = dict(wall_ms=spread(wall), same_bytes_as_context=bool(free[0].tobytes() == merged_segs.tobytes() and
                                                                        free[1].tobytes() == merged_line.tobytes()))
if with_model:
    a = time.perf_counter()
    want = M.merge(segs, line, max_distance, M.min_cos2_of(10.0), 0.5)
    res["numpy_model_ms"] = (time.perf_counter() - a) * 1e3
    res["equals_model"] = bool(all(np.ascontiguousarray(free[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes() for k in range(4))
                               and free[4] == want[4])
print(json.dumps(res))
g.close()
