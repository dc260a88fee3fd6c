"""Times l3d_associate_view_segments on a BASELINE configuration after matchImages and reconstruct3Dlines(3):
the wall time of the call and the kernel time by HIP events (timing level 2), median of the last seven of nine calls in a
warm process, with the counts of records and segments per view and the shares of segments assigned and ambiguous.  With
`model` the array form of the numpy model (tests/associate_model.py) is timed on the same records and compared.
    python tools/associate_timing.py C1 model
    python tools/associate_timing.py C2
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
from tests import associate_model as M

cfg = sys.argv[1]; with_model = len(sys.argv) > 2 and sys.argv[2] == "model"
t0 = time.time()
sc = make_config(cfg)
g = Line3D(); g.add_scene(sc)
t1 = time.time()
assert g.matchImages() and g.reconstruct3Dlines(3)
t2 = time.time()
L = _lib.load()
lines = g.get3Dlines()
ids = np.array(sorted(v.cam for v in sc.views), np.uint32)
par = api.associate_params(2.5, 10.0, 0.5)
off = np.zeros(len(ids) + 1, np.uint64)
assert L.l3d_associate_view_segments(g.h, len(ids), _lib.ptr(ids), C.byref(par), 1e-6, _lib.ptr(off), None, None, None) == 0
out = np.zeros(int(off[-1]), _lib.ASSOCIATION_DTYPE)
ss = np.zeros(len(lines), np.uint32); sv = np.zeros(len(lines), np.uint32)
g.setTimingLevel(2)
wall, kern = [], []
for it in range(9):
    a = time.perf_counter()
    rc = L.l3d_associate_view_segments(g.h, len(ids), _lib.ptr(ids), C.byref(par), 1e-6, _lib.ptr(off), _lib.ptr(out), _lib.ptr(ss), _lib.ptr(sv))
    b = time.perf_counter()
    assert rc == 0, _lib.last_error()
    if it >= 2:
        wall.append((b - a) * 1e3); kern.append(L.l3d_debug_counter(b"associate_kernel_ns") / 1e6)
g.setTimingLevel(1)
rec = g.projectLines([int(c) for c in ids])
a = time.perf_counter(); g.projectLines([int(c) for c in ids]); proj_ms = (time.perf_counter() - a) * 1e3
n_rec = [len(r) for r in rec]
res = dict(config=cfg, build=L.l3d_build_info().decode(), views=len(ids), lines=len(lines), segments_3d=int(sum(len(l["collinear3Dsegments"]) for l in lines)),
           segs_per_view=[int(min(np.diff(off))), int(max(np.diff(off)))], records_per_view=[min(n_rec), int(np.median(n_rec)), max(n_rec)],
           pair_tests=int(sum(int(n) * int(m) for n, m in zip(n_rec, np.diff(off)))),
           wall_ms_median=float(np.median(wall)), wall_ms_all=[round(w, 3) for w in wall], kernel_ms_median=float(np.median(kern)), kernel_ms_all=[round(k, 4) for k in kern],
           project_lines_python_ms=proj_ms, assigned_share=float((out["record"] >= 0).mean()), ambiguous_share=float((out["n_accepted"] > 1).mean()),
           assigned=int((out["record"] >= 0).sum()), ambiguous=int((out["n_accepted"] > 1).sum()), supported_lines=int((ss > 0).sum()),
           setup_s=t1 - t0, match_reconstruct_s=t2 - t1)
if with_model:
    segs = {v.cam: np.asarray(v.segs, np.float32).reshape(-1, 4) for v in sc.views}
    a = time.perf_counter()
    want = [M.associate(rec[k], segs[int(c)], 2.5, par.min_cos2, 0.5) for k, c in enumerate(ids)]
    res["numpy_model_ms"] = (time.perf_counter() - a) * 1e3
    res["equals_model"] = bool(all(np.array_equal(out[int(off[k]):int(off[k + 1])], want[k]) for k in range(len(ids))))
print(json.dumps(res))
g.close()
