"""Times l3d_align_lines on a BASELINE configuration after matchImages and reconstruct3Dlines(3): the
context's model against a copy of itself that is moved by a known similarity and whose end points are jittered by 1e-4
of the extent, from a start 2 degrees, 2 % and 0.01 of the diagonal off, max_distance = 1e-3 x extent of the copy, the
gate starting 32 times as wide.  Reported: the wall time of the call and the kernel time by HIP events (timing level 2),
median of the last seven of nine calls in a warm process, each also per iteration (the delivery pass counted as one), the
iterations, the status and the end-point error against the known similarity.  With `model` the array form of the numpy
model (tests/align_model.py) is timed on the same input and compared.
    python tools/align_timing.py C1 model
    python tools/align_timing.py C2
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
from tests import align_cases as Cs
from tests import align_model as A
from tests import compare_model as CM

cfg = sys.argv[1]; with_model = len(sys.argv) > 2 and sys.argv[2] == "model"
t0 = time.time()
sc = make_config(cfg)
g = Line3D(); g.add_scene(sc)
t1 = time.time()
assert g.matchImages() and g.reconstruct3Dlines(3)
t2 = time.time()
L = _lib.load()
segs, line = api.flatten_lines(g.get3Dlines())
rng = np.random.default_rng(1)
T_true = A.entry(A.similarity(1.4, Cs.axis_angle([0.5, 1.0, -0.25], 60.0), (3.0, -2.0, 5.0)))
other = A.transform(segs, T_true)
extent = CM.extent(other)
other = np.ascontiguousarray(other + rng.uniform(-1e-4 * extent, 1e-4 * extent, other.shape))
c, diag = A.bounding_box(other)
initial = Cs.perturbed(T_true, c, diag, 2.0, 0.02, 0.01, rng)
max_distance = 1e-3 * extent; start_distance = 32 * max_distance
par = api.align_params(max_distance, start_distance)
init = api._similarity_struct(initial)
out = api._AlignOutputs(len(segs), len(other), par.max_iterations)
g.setTimingLevel(2)
wall, kern = [], []
for it in range(9):
    a = time.perf_counter()
    rc = L.l3d_align_lines(g.h, len(other), _lib.ptr(other), _lib.ptr(line), C.byref(par), init, *out.pointers())
    b = time.perf_counter()
    assert rc == 0, _lib.last_error()
    if it >= 2:
        wall.append((b - a) * 1e3); kern.append(L.l3d_debug_counter(b"align_kernel_ns") / 1e6)
g.setTimingLevel(1)
got = out.result()
passes = got["summary"]["iterations"] + 1
res = dict(config=cfg, build=L.l3d_build_info().decode(), segments_3d=len(segs), extent=extent, diag=diag, max_distance=max_distance,
           start_distance=start_distance, setup_s=t1 - t0, match_reconstruct_s=t2 - t1, status=got["summary"]["status"],
           iterations=got["summary"]["iterations"], n_matched=got["summary"]["n_matched"], rms=got["summary"]["rms"],
           end_point_error=A.end_point_error(segs, got["similarity"], T_true, diag),
           start_error=A.end_point_error(segs, initial, T_true, diag),
           wall_ms_median=float(np.median(wall)), wall_ms_all=[round(w, 3) for w in wall], kernel_ms_median=float(np.median(kern)),
           kernel_ms_all=[round(k, 4) for k in kern], wall_ms_per_pass=float(np.median(wall)) / passes,
           kernel_ms_per_pass=float(np.median(kern)) / passes)
if with_model:
    a = time.perf_counter()
    want = A.align(segs, line, other, line, max_distance, initial=initial, start_distance=start_distance)
    res["numpy_model_ms"] = (time.perf_counter() - a) * 1e3
    try:
        Cs.same_result(got, want, "device / model")
        res["equals_model"] = True
    except AssertionError as e:
        res["equals_model"] = str(e)
print(json.dumps(res))
g.close()
