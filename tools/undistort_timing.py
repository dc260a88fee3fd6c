"""Wall time of undistort_images (k_undistort.hip) on full-size images, copies included: batches of 1, 8 and 26 grey
3072x2304 images and one RGB image, each run REPEATS times.  Kernel times come from a trace of the same sequence, in a
run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/undistort_timing.py
    python tools/undistort_timing.py --trace <dir>
The second command matches the k_undistort launches of the trace to the sequence below (one launch per call) and prints
the kernel time per image and the algorithmic bytes (input + output) per second against the 6.29 TB/s copy figure of
the MI355X."""
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from line3dpp_amd.lsd import read_image_gray, undistort_images  # noqa: E402

REPEATS = 3
CONFIGS = [("grey", 1), ("grey", 8), ("grey", 26), ("rgb", 1)]
K = np.array([[2600.0, 0, 1536.0], [0, 2600.0, 1152.0], [0, 0, 1]])
RADIAL, TANGENTIAL = (-0.05, 0.01, 0.0), (0.001, -0.0005)      # an OPENCV camera of a COLMAP model
COPY_TBS = 6.29                                                 # MI355X_MICROARCH.md: float4 copy, measured


def images():
    gold = os.path.join(ROOT, "tests", "golden", "lsd")
    grey = [read_image_gray(os.path.join(gold, n)) for n in ("img000055.jpg", "img000056.jpg")]
    return grey, np.ascontiguousarray(np.stack([grey[0], grey[1], grey[0][::-1]], axis=2))


def batch(grey, rgb, kind, n):
    return [rgb] if kind == "rgb" else [grey[k % 2] for k in range(n)]


def run():
    grey, rgb = images()
    undistort_images([grey[0]], [K], [RADIAL], [TANGENTIAL])           # first call of the process: runtime set-up
    for kind, n in CONFIGS:
        imgs = batch(grey, rgb, kind, n)
        walls = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            undistort_images(imgs, [K] * n, [RADIAL] * n, [TANGENTIAL] * n)
            walls.append(time.perf_counter() - t)
        mb = sum(im.nbytes for im in imgs) / 1e6
        print(f"{kind} batch of {n}: wall {1e3 * min(walls):.1f} ms min / {1e3 * np.median(walls):.1f} ms median "
              f"({1e3 * min(walls) / n:.2f} ms per image), {mb:.1f} MB each way", flush=True)


def trace(folder):
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "k_undistort" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
    expected = 1 + REPEATS * len(CONFIGS)
    if len(ns) != expected:
        raise SystemExit(f"{len(ns)} k_undistort launches in {folder}, the sequence has {expected}")
    grey, rgb = images()
    k = 1
    for kind, n in CONFIGS:
        t = sorted(ns[k:k + REPEATS])
        k += REPEATS
        nbytes = 2 * sum(im.nbytes for im in batch(grey, rgb, kind, n))
        print(f"{kind} batch of {n}: kernel {t[0] / 1e6:.3f} ms min / {t[len(t) // 2] / 1e6:.3f} ms median "
              f"({t[0] / 1e6 / n:.3f} ms per image); {nbytes / t[0] / 1e3:.2f} TB/s of algorithmic bytes "
              f"= {nbytes / t[0] / 1e3 / COPY_TBS:.2f} of the {COPY_TBS} TB/s copy figure")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        trace(sys.argv[2])
    else:
        run()
