"""Wall time of Line3D.renderLines (k_project.hip, l3d_project.hip) per view, uploads and the download of both
planes included: the golden scene's lines (tests/golden/make_golden.golden_scene, reconstruct3Dlines(3)) in its own ten
views of 3072 x 2304, and the same lines repeated to a line count of a real dataset.
    python tools/project_timing.py [copies]              (one GPU process; run it under a time limit)
Kernel times come from a trace of the same sequence, in a run of its own:
    rocprofv3 --kernel-trace --stats -f csv -d <dir> -- python tools/project_timing.py
    python tools/project_timing.py --trace <dir>
The second command sums the launches of a csv trace (-f csv) per library call of the sequence, in time order, and all
launches per kernel of k_project.hip (and the scans between them)."""
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3
KERNELS = ("k_project_lines", "k_project_compact", "k_raster_count", "k_raster_lines", "k_map_decode", "k_overlay", "k_scan")


def run(copies):
    from line3dpp_amd import api
    from line3dpp_amd.api import Line3D
    from tests.golden.make_golden import golden_scene
    sc = golden_scene()
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages() and g.reconstruct3Dlines(3)
    cam_ids = [v.cam for v in sc.views]
    lines = g.get3Dlines()
    g.renderLines(cam_ids[:1])                                   # first call of the process: code object, copy paths
    walls = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        maps = g.renderLines(cam_ids)
        walls.append(time.perf_counter() - t)
    w, h = maps[0][0].shape[1], maps[0][0].shape[0]
    drawn = int(np.mean([(m[0] >= 0).sum() for m in maps]))
    print(f"renderLines, {len(lines)} lines, {len(cam_ids)} views of {w} x {h}: wall {1e3 * min(walls) / len(cam_ids):.2f} ms "
          f"per view min / {1e3 * np.median(walls) / len(cam_ids):.2f} median; {drawn} pixels drawn per view", flush=True)
    # the stateless stages on the same cameras with the lines repeated (shifted a little each time): a real line count
    cams = [g.viewCamera(c) for c in cam_ids]
    P1 = np.concatenate([L["collinear3Dsegments"]["P1"] for L in lines]); P2 = np.concatenate([L["collinear3Dsegments"]["P2"] for L in lines])
    rng = np.random.default_rng(1)
    shift = rng.normal(0, 0.5, (copies, 1, 3))
    Q1 = (P1[None] + shift).reshape(-1, 3); Q2 = (P2[None] + shift).reshape(-1, 3)
    line = np.arange(len(Q1), dtype=np.uint32)
    for what, fn in (("project_segments", lambda: api.project_segments(cams, Q1, Q2, line)),):
        walls = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            rec = fn()
            walls.append(time.perf_counter() - t)
        print(f"{what}, {len(Q1)} segments x {len(cams)} views: wall {1e3 * min(walls):.2f} ms min, "
              f"{sum(len(r) for r in rec)} records", flush=True)
    walls = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        maps = api.render_line_maps(cams, rec, 1)
        walls.append(time.perf_counter() - t)
    drawn = int(np.mean([(m[0] >= 0).sum() for m in maps]))
    print(f"render_line_maps, {len(Q1)} lines: wall {1e3 * min(walls) / len(cams):.2f} ms per view min / "
          f"{1e3 * np.median(walls) / len(cams):.2f} median; {drawn} pixels drawn per view", flush=True)
    g.close()


def per_call(launches, views):
    """launches: (start, kernel, ns, grid.y) of one process -> the sums per kernel of every library call of run(): a call
    begins at a k_project_lines launch (stage 1) or, for the stateless stage 2, after the k_map_decode launches of the
    call before it have covered all `views` cameras (grid.y of k_map_decode is the cameras of a group).  A fill of the
    scan work space ahead of a projection is listed alone, and the first stateless stage 2 with the stage 1 before it."""
    calls, cur, decoded = [], {}, 0
    for _, name, ns, gy in sorted(launches):
        k = next((k for k in KERNELS + ("fillBuffer",) if k in name), None)
        if k is None or (not calls and not cur and k != "k_project_lines"):
            continue                                             # copies; whatever ran before the first projection
        if cur and (k == "k_project_lines" or (decoded >= views and k != "k_map_decode")):
            calls.append(cur); cur, decoded = {}, 0
        cur[k] = cur.get(k, 0) + ns
        decoded += gy if k == "k_map_decode" else 0
    calls.append(cur)
    for i, c in enumerate(calls):
        print(f"call {i}: " + ", ".join(f"{k} {v / 1e3:.1f}" for k, v in c.items()) + f"; {sum(c.values()) / 1e3:.1f} us in all")


def trace(folder, views=10):
    found = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows = list(csv.DictReader(f))
        found += [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows]
        per_call([(int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"]),
                   int(r["Grid_Size_Y"])) for r in rows], views)
    for path in glob.glob(os.path.join(folder, "**", "*_results.db"), recursive=True):      # rocprofv3's default output: rocpd
        import sqlite3
        with sqlite3.connect(path) as db:
            found += list(db.execute("select name, duration from kernels"))
    for k in KERNELS:
        ns = [d for name, d in found if k in name]
        if ns:
            print(f"{k}: {len(ns)} launches, {sum(ns) / 1e3:.1f} us in all, {np.median(ns) / 1e3:.1f} us median, {max(ns) / 1e3:.1f} us longest")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--trace"]:
        trace(args[1])
    else:
        run(int(args[0]) if args else 100)
