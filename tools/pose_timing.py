"""Times the refinement of camera poses on a BASELINE configuration after matchImages and
reconstruct3Dlines(3), all views in one call, max_distance = 2.5 px, the gate from 10 px:
  context   l3d_refine_view_cameras from the views' own cameras: the wall time of the call and the kernel time by HIP
            events (timing level 2);
  perturbed l3d_refine_cameras (stateless: it allocates its work space per call, wall time only) on the context's lines
            and the views' segments, from the views' cameras turned by 0.1 degrees and moved by 0.2 % of their median depth;
            the pose differences against the context form's result are reported.
Nine calls each in a warm process, the median of the last seven; each also per pass, a pass being one launch of
k_pose_normal with the projection and the association in front of it (an iteration of the cameras still active, or the
delivery pass).
    python tools/pose_timing.py C1
    python tools/pose_timing.py C2
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
from tests import pose_cases as Cs
from tests import pose_model as P

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
by_id = {v.cam: v for v in sc.views}
obs = [np.ascontiguousarray(by_id[int(c)].segs, np.float32).reshape(-1, 4) for c in ids]
n_seg = np.array([len(o) for o in obs] + [0], np.uint32)
seg4 = np.concatenate(obs + [np.zeros((1, 4), np.float32)])
own = [g.viewCamera(int(c)) for c in ids]
rng = np.random.default_rng(Cs.SEED)
depth = [float(by_id[int(c)].median_depth) for c in ids]
start = [Cs.perturbed(P.camera(c["K"], c["R"], c["t"], c["width"], c["height"]), 0.1, 0.002 * z, rng) for c, z in zip(own, depth)]
par = api.pose_params(2.5, 10.0)
out = api._PoseOutputs(len(ids), n_seg[:len(ids)], par.max_iterations)
off = np.zeros(len(ids) + 1, np.uint64)


def timed(call, counter):
    wall, kern, passes = [], [], 0
    for it in range(9):
        n0 = L.l3d_debug_counter(b"pose_normal_launches")
        a = time.perf_counter()
        rc = call()
        b = time.perf_counter()
        assert rc == 0, _lib.last_error()
        passes = L.l3d_debug_counter(b"pose_normal_launches") - n0
        if it >= 2:
            wall.append((b - a) * 1e3)
            if counter:
                kern.append(L.l3d_debug_counter(b"pose_kernel_ns") / 1e6)
    return wall, kern, passes


def summary(res):
    st = {}
    for s in res["summaries"]:
        st[s["status"]] = st.get(s["status"], 0) + 1
    its = [s["iterations"] for s in res["summaries"]]
    return dict(status=st, iterations_min_median_max=[min(its), int(np.median(its)), max(its)],
                n_matched=int(sum(s["n_matched"] for s in res["summaries"])),
                rms_min_max=[min(s["rms"] for s in res["summaries"]), max(s["rms"] for s in res["summaries"])])


g.setTimingLevel(2)
wall, kern, passes = timed(lambda: L.l3d_refine_view_cameras(g.h, len(ids), _lib.ptr(ids), C.byref(par), out.cams, _lib.ptr(out.summaries),
                                                             _lib.ptr(off), _lib.ptr(out.assoc), _lib.ptr(out.trace)), True)
g.setTimingLevel(1)
ctx = out.result()
res = dict(config=cfg, build=L.l3d_build_info().decode(), views=len(ids), segments_3d=len(segs), segments_2d=int(n_seg.sum()),
           setup_s=t1 - t0, match_reconstruct_s=t2 - t1,
           context=dict(summary(ctx), passes=int(passes), wall_ms_median=float(np.median(wall)), wall_ms_all=[round(w, 3) for w in wall],
                        kernel_ms_median=float(np.median(kern)), kernel_ms_all=[round(k, 4) for k in kern],
                        wall_ms_per_pass=float(np.median(wall)) / passes, kernel_ms_per_pass=float(np.median(kern)) / passes))
arr = api.camera_array(start)
wall, _, passes = timed(lambda: L.l3d_refine_cameras(0, len(segs), _lib.ptr(segs), _lib.ptr(line), len(ids), arr, _lib.ptr(n_seg), _lib.ptr(seg4),
                                                     C.byref(par), out.cams, _lib.ptr(out.summaries), _lib.ptr(out.assoc), _lib.ptr(out.trace)), False)
got = out.result()
d = [P.pose_difference(a, b, z) for a, b, z in zip(got["cameras"], ctx["cameras"], depth)]
d0 = [P.pose_difference(a, b, z) for a, b, z in zip(start, own, depth)]
res["perturbed"] = dict(summary(got), passes=int(passes), wall_ms_median=float(np.median(wall)), wall_ms_all=[round(w, 3) for w in wall],
                        wall_ms_per_pass=float(np.median(wall)) / passes,
                        start_angle_deg_max=max(v[0] for v in d0), start_centre_max=max(v[1] for v in d0),
                        angle_deg_to_context_result_max=max(v[0] for v in d), centre_to_context_result_max=max(v[1] for v in d))
print(json.dumps(res))
g.close()
