"""Times the refit of the 3D lines against the views on a BASELINE configuration after matchImages and
reconstruct3Dlines(3): l3d_refit_view_lines with all views, their own cameras, max_distance = 2.5 px, visibility 3.  The
call replaces the context's lines, so reconstruct3Dlines(3) runs again before every call, outside the timed region: every
call refits the same model.  Nine calls in a warm process, the median of the last seven: the wall time of the call, the
kernel time by HIP events (timing level 2) and how it splits across the projection and association, the observation list
(k_refit_flag, k_scan, k_refit_compact), k_refit_obs, k_lineopt and k_refit_spans.
    python tools/refit_timing.py C1
    python tools/refit_timing.py C2
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

PARTS = ("refit_associate_ns", "refit_list_ns", "refit_obs_ns", "refit_lineopt_ns", "refit_spans_ns")

cfg = sys.argv[1]
t0 = time.time()
sc = make_config(cfg)
g = Line3D(); g.add_scene(sc)
t1 = time.time()
assert g.matchImages() and g.reconstruct3Dlines(3)
t2 = time.time()
L = _lib.load()
segs, line = api.flatten_lines(g.get3Dlines())
ids = np.ascontiguousarray(sorted(v.cam for v in sc.views), np.uint32)
par = api.refit_params(2.5)
summary = _lib.RefitSummary()
wall, kern, parts = [], [], {k: [] for k in PARTS}
g.setTimingLevel(2)
for it in range(9):
    if it:
        assert g.reconstruct3Dlines(3)
    a = time.perf_counter()
    rc = L.l3d_refit_view_lines(g.h, len(ids), _lib.ptr(ids), None, C.byref(par), C.byref(summary), None)
    b = time.perf_counter()
    assert rc == 0, _lib.last_error()
    if it >= 2:
        wall.append((b - a) * 1e3)
        kern.append(L.l3d_debug_counter(b"refit_kernel_ns") / 1e6)
        for k in PARTS:
            parts[k].append(L.l3d_debug_counter(k.encode()) / 1e6)
g.setTimingLevel(1)
res = dict(config=cfg, build=L.l3d_build_info().decode(), views=len(ids), segments_3d=len(segs), lines=int(line.max()) + 1 if len(line) else 0,
           segments_2d=int(sum(len(v.segs) for v in sc.views)), setup_s=t1 - t0, match_reconstruct_s=t2 - t1,
           summary=api.refit_summary_dict(summary), wall_ms_median=float(np.median(wall)), wall_ms_all=[round(w, 3) for w in wall],
           kernel_ms_median=float(np.median(kern)), kernel_ms_all=[round(k, 4) for k in kern],
           kernel_ms_parts={k[6:-3]: float(np.median(v)) for k, v in parts.items()})
print(json.dumps(res))
g.close()
