"""Wall time of api.triangulate_points (k_triangulate.hip), upload and download included, for 10^4, 10^6 and 10^7 points
at 5 observations each, and beside it the same normal matrices through batched numpy.linalg.eigh on the host (the
matrices are formed outside the timed part on both sides' behalf: the host figure is the solve alone).
    python tools/triangulate_timing.py [sizes]           (one GPU process; run it under a time limit)
Kernel times come from a trace of the same sequence, in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/triangulate_timing.py --gpu-only
    python tools/triangulate_timing.py --trace <dir>
The second command lists the k_triangulate launches of the trace in order (one warm-up, then REPEATS per size)."""
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3
SIZES = (10**4, 10**6, 10**7)
N_OBS, N_CAMS = 5, 300
HOST_CHUNK = 1 << 18            # matrices per eigh call: keeps the host side's work space small


def problem(n, seed=3):
    """n points in a box of half side 10, each seen by N_OBS of N_CAMS cameras on a ring of radius 25, 0.5 px noise"""
    from line3dpp_amd.scene import _lookat
    rng = np.random.default_rng(seed)
    K = np.array([[620.0, 0, 512.0], [0, 620.0, 384.0], [0, 0, 1.0]])
    P = np.zeros((N_CAMS, 3, 4))
    for j in range(N_CAMS):
        phi = 2 * np.pi * j / N_CAMS
        C = np.array([25.0 * np.cos(phi), 25.0 * np.sin(phi), rng.uniform(-2, 2)])
        R = _lookat(C, rng.normal(0, 0.5, 3))
        P[j] = K @ np.column_stack([R, -R @ C])
    X = rng.uniform(-10, 10, (n, 3))
    cam = ((rng.integers(0, N_CAMS, (n, 1)) + 17 * np.arange(N_OBS)[None, :]) % N_CAMS).astype(np.uint32).reshape(-1)
    xy = np.empty((n * N_OBS, 2))
    Xh = np.column_stack([X, np.ones(n)])
    for k in range(0, n, HOST_CHUNK):
        c = cam.reshape(n, N_OBS)[k:k + HOST_CHUNK]
        x = np.einsum("nkij,nj->nki", P[c], Xh[k:k + HOST_CHUNK])
        xy.reshape(n, N_OBS, 2)[k:k + HOST_CHUNK] = x[..., :2] / x[..., 2:3]
    xy += rng.normal(0, 0.5, xy.shape)
    off = (np.arange(n + 1, dtype=np.uint64) * N_OBS)
    return P, off, cam, xy


def host_eigh(P, off, cam, xy):
    """seconds of batched numpy.linalg.eigh over all normal matrices (formed chunk by chunk, outside the clock)"""
    n = len(off) - 1
    spent = 0.0
    for k in range(0, n, HOST_CHUNK):
        m = min(HOST_CHUNK, n - k)
        Pc = P[cam[k * N_OBS:(k + m) * N_OBS]]
        q = xy[k * N_OBS:(k + m) * N_OBS]
        r1 = q[:, 1:2] * Pc[:, 2] - Pc[:, 1]
        r2 = Pc[:, 0] - q[:, 0:1] * Pc[:, 2]
        M = (r1[:, :, None] * r1[:, None, :] + r2[:, :, None] * r2[:, None, :]).reshape(m, N_OBS, 4, 4).sum(1)
        t = time.perf_counter()
        w, V = np.linalg.eigh(M)
        v = V[np.arange(m), :, np.abs(w).argmin(1)]
        X = v[:, :3] / v[:, 3:4]
        spent += time.perf_counter() - t
    return spent


def run(sizes, gpu_only):
    from line3dpp_amd.api import triangulate_points
    triangulate_points(*problem(1000))                                   # first call of the process: runtime set-up
    for n in sizes:
        P, off, cam, xy = problem(n)
        walls = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            X, valid = triangulate_points(P, off, cam, xy)
            walls.append(time.perf_counter() - t)
        line = (f"{n} points x {N_OBS} observations: triangulate_points wall {1e3 * min(walls):.2f} ms min / "
                f"{1e3 * np.median(walls):.2f} ms median, {int(valid.sum())} valid")
        if not gpu_only:
            line += f"; numpy.linalg.eigh on the host {1e3 * host_eigh(P, off, cam, xy):.2f} ms"
        print(line, flush=True)


def trace(folder):
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "k_triangulate" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    found = [(r.get("Grid_Size") or r.get("Grid_Size_X") or "?", int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows]
    for path in glob.glob(os.path.join(folder, "**", "*_results.db"), recursive=True):      # rocprofv3's default output: rocpd
        import sqlite3
        with sqlite3.connect(path) as db:
            found += list(db.execute("select grid_x, duration from kernels where name like '%k_triangulate%' order by start"))
    for k, (grid, ns) in enumerate(found):
        print(f"launch {k}: grid {grid}: {ns / 1e3:.1f} us")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--trace"]:
        trace(args[1])
    else:
        gpu_only = "--gpu-only" in args
        sizes = [int(float(a)) for a in args if not a.startswith("--")] or SIZES
        run(sizes, gpu_only)
