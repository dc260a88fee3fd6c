"""Times l3d_wireframe_lines on a BASELINE configuration after matchImages and reconstruct3Dlines(3), with
max_distance = max_extension = 1e-3 of the extent and 10 degrees.  The call leaves the context as it is: nine calls in a
warm process, the median of the last seven with its range, of the wall time of the whole call and of the kernel time by
HIP events (timing level 2: the count pass with its scan, and the write pass).  The stateless
l3d_wireframe_segments on the same model is timed beside it (wall only), and with `model` the numpy model
(tests/wireframe_model.py) on the same input, which is compared byte for byte.
    python tools/wireframe_timing.py C1 model
    python tools/wireframe_timing.py C2
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
from tests import wireframe_model as M

cfg = sys.argv[1]; with_model = len(sys.argv) > 2 and sys.argv[2] == "model"
t0 = time.time()
sc = make_config(cfg)
g = Line3D(); g.add_scene(sc)
t1 = time.time()
assert g.matchImages() and g.reconstruct3Dlines(3)
t2 = time.time()
L = _lib.load()
segs, line = api.flatten_lines(g.get3Dlines())
n = len(segs)
extent = M.extent(segs)
max_distance = 1e-3 * extent
tiles = -(-n // 256)
res = dict(config=cfg, build=L.l3d_build_info().decode(), segments_3d=n, lines=int(line.max()) + 1 if n else 0, extent=extent,
           max_distance=max_distance, pair_tests=n * (n - 1) // 2, setup_s=t1 - t0, match_reconstruct_s=t2 - t1)


def spread(v):
    return dict(median=float(np.median(v)), lo=float(min(v)), hi=float(max(v)), all=[round(x, 4) for x in v])


g.setTimingLevel(2)
wall, kern, kern_count = [], [], []
mine = None
for it in range(9):
    a = time.perf_counter()
    mine = g.wireframe(max_distance)
    b = time.perf_counter()
    assert mine is not None
    if it >= 2:
        wall.append((b - a) * 1e3); kern.append(L.l3d_debug_counter(b"wf_kernel_ns") / 1e6)
        kern_count.append(L.l3d_debug_counter(b"wf_count_ns") / 1e6)
g.setTimingLevel(1)
slices = int(L.l3d_debug_counter(b"wf_slices"))
res["context"] = dict(tiles=tiles, slices=slices, workgroups=tiles * slices, skipped=int(L.l3d_debug_counter(b"wf_skipped_blocks")),
                      wall_ms=spread(wall), kernel_ms=spread(kern), count_scan_ms=spread(kern_count),
                      write_ms=spread([a - b for a, b in zip(kern, kern_count)]))
res["summary"] = mine["summary"]
free = None
wall = []
for it in range(9):
    a = time.perf_counter()
    free = api.build_wireframe(segs, line, max_distance)
    b = time.perf_counter()
    if it >= 2:
        wall.append((b - a) * 1e3)


def same(x, y):
    return bool(all(x[k].tobytes() == y[k].tobytes() for k in ("junctions", "vertices", "edges")) and x["summary"] == y["summary"])


res["stateless"] = dict(wall_ms=spread(wall), same_bytes_as_context=same(free, mine))
if with_model:
    a = time.perf_counter()
    want = M.wireframe(segs, line, max_distance, max_distance, M.min_sin2_of(10.0))
    res["numpy_model_ms"] = (time.perf_counter() - a) * 1e3
    res["equals_model"] = same(free, want)
print(json.dumps(res))
g.close()
