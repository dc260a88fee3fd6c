"""Times the direction detection.
Always: the stateless l3d_direction_segments on the generated case of 5 000 segments (tests/directions_cases.large_case),
nine calls in a warm process, the median of the last seven with its range, wall time only -- a stateless call has no timing
level -- beside the numpy model (tests/directions_model.py) on the same input, which is compared byte for byte.
With a BASELINE configuration: l3d_direction_lines on its lines after matchImages and reconstruct3Dlines(3), at max_angle =
2 degrees, nine calls, wall time and the kernel time by HIP events (timing level 2: dir_kernel_ns = k_dir_units +
k_dir_score + k_pl_merge).
    python tools/directions_timing.py
    python tools/directions_timing.py C1
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  -- first, as tests/conftest.py does
from line3dpp_amd import _lib, api
from tests import directions_cases as Cs
from tests import directions_model as M

cfg = sys.argv[1] if len(sys.argv) > 1 else None
L = _lib.load()


def spread(v):
    return dict(median=float(np.median(v)), lo=float(min(v)), hi=float(max(v)), all=[round(x, 4) for x in v])


def same(x, y):
    return bool(all(x[k].tobytes() == y[k].tobytes() for k in ("directions", "members", "seg_directions", "scores", "R")) and
                M.pack_summary(x["summary"]) == M.pack_summary(y["summary"]))


segs, line, _ = Cs.large_case()
wall, free = [], None
for it in range(9):
    a = time.perf_counter()
    free = api.detect_directions(segs, line, Cs.MAX_ANGLE, min_segments=Cs.PAR["min_segments"])
    b = time.perf_counter()
    if it >= 2:
        wall.append((b - a) * 1e3)
a = time.perf_counter()
want = M.detect(segs, line, Cs.PAR)
model_ms = (time.perf_counter() - a) * 1e3
n_h = int(L.l3d_debug_counter(b"dir_hypotheses")); slices = int(L.l3d_debug_counter(b"dir_slices"))
res = dict(build=L.l3d_build_info().decode(),
           generated=dict(segments=len(segs), hypotheses=n_h, tiles=-(-n_h // 256), slices=slices, direction_tests=n_h * len(segs),
                          wall_ms=spread(wall), numpy_model_ms=model_ms, equals_model=same(free, want), summary=free["summary"]))
if cfg:
    from line3dpp_amd.api import Line3D
    from line3dpp_amd.scene import make_config
    g = Line3D(); g.add_scene(make_config(cfg))
    assert g.matchImages() and g.reconstruct3Dlines(3)
    segs, line = api.flatten_lines(g.get3Dlines())
    angle = 2.0
    g.setTimingLevel(2)
    wall, kern, mine = [], [], None
    for it in range(9):
        a = time.perf_counter()
        mine = g.detectDirections(angle)
        b = time.perf_counter()
        assert mine is not None
        if it >= 2:
            wall.append((b - a) * 1e3); kern.append(L.l3d_debug_counter(b"dir_kernel_ns") / 1e6)
    g.setTimingLevel(1)
    n_h = int(L.l3d_debug_counter(b"dir_hypotheses"))
    res["context"] = dict(config=cfg, segments=len(segs), max_angle=angle, hypotheses=n_h, slices=int(L.l3d_debug_counter(b"dir_slices")),
                          direction_tests=n_h * len(segs), wall_ms=spread(wall), dir_kernel_ms=spread(kern),
                          same_bytes_as_stateless=same(api.detect_directions(segs, line, angle), mine), summary=mine["summary"])
    g.close()
print(json.dumps(res))
