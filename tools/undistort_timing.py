"""Wall time of undistort_images (k_undistort.hip) on full-size images, copies included: batches of 1, 8 and 26 grey
3072x2304 images and one RGB image, each run REPEATS times.  Kernel times come from a trace of the same sequence, in a
run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/undistort_timing.py
    python tools/undistort_timing.py --trace <dir>
The second command matches the k_undistort launches of the trace to the sequence below (one launch per call) and prints
the kernel time per image and the algorithmic bytes (input + output) per second against the 6.29 TB/s copy figure of
the MI355X.

With --models the sequence is the one of DESIGN §15 instead: for a batch of 1 and of 8 grey images, undistort_images
(k_undistort, the yardstick, from the same run) and then undistort_images_model (k_undistort_model) for each of the five
camera models, each REPEATS times:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/undistort_timing.py --models
    python tools/undistort_timing.py --models --trace <dir>"""
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from line3dpp_amd.lsd import read_image_gray, undistort_images, undistort_images_model  # noqa: E402

REPEATS = 3
CONFIGS = [("grey", 1), ("grey", 8), ("grey", 26), ("rgb", 1)]
K = np.array([[2600.0, 0, 1536.0], [0, 2600.0, 1152.0], [0, 0, 1]])
RADIAL, TANGENTIAL = (-0.05, 0.01, 0.0), (0.001, -0.0005)      # an OPENCV camera of a COLMAP model
COPY_TBS = 6.29                                                 # MI355X_MICROARCH.md: float4 copy, measured
MODEL_CONFIGS = [("grey", 1), ("grey", 8)]
MODELS = [("FULL_OPENCV", (-0.1, 0.02, 1e-3, -2e-3, 3e-3, 0.01, -0.002, 0.0005)), ("OPENCV_FISHEYE", (-0.03, 0.005, -0.001, 0.0002)),
          ("RADIAL_FISHEYE", (-0.03, 0.006)), ("SIMPLE_RADIAL_FISHEYE", (-0.04,)), ("FOV", (0.9,))]


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
            rows += [r for r in csv.DictReader(f) if "k_undistort" in r["Kernel_Name"] and "k_undistort_model" not in r["Kernel_Name"]]
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


def _timed(fn, *args):
    walls = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        fn(*args)
        walls.append(time.perf_counter() - t)
    return walls


def run_models():
    grey, rgb = images()
    undistort_images([grey[0]], [K], [RADIAL], [TANGENTIAL])           # first call of the process: runtime set-up
    for kind, n in MODEL_CONFIGS:
        imgs = batch(grey, rgb, kind, n)
        walls = _timed(undistort_images, imgs, [K] * n, [RADIAL] * n, [TANGENTIAL] * n)
        print(f"{kind} batch of {n}: undistort_images wall {1e3 * min(walls):.1f} ms min / {1e3 * np.median(walls):.1f} ms median", flush=True)
        for model, params in MODELS:
            walls = _timed(undistort_images_model, imgs, [model] * n, [K] * n, [params] * n)
            print(f"{kind} batch of {n}: undistort_images_model {model} wall {1e3 * min(walls):.1f} ms min / "
                  f"{1e3 * np.median(walls):.1f} ms median", flush=True)


def trace_models(folder):
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "k_undistort" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ns = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), "k_undistort_model" in r["Kernel_Name"]) for r in rows]
    expected = 1 + REPEATS * len(MODEL_CONFIGS) * (1 + len(MODELS))
    if len(ns) != expected:
        raise SystemExit(f"{len(ns)} undistortion launches in {folder}, the sequence has {expected}")
    k = 1
    for kind, n in MODEL_CONFIGS:
        base = None
        for name in ["k_undistort"] + [m for m, _ in MODELS]:
            part = ns[k:k + REPEATS]
            k += REPEATS
            assert all(is_model == (name != "k_undistort") for _, is_model in part), "the trace does not follow the sequence"
            t = sorted(d for d, _ in part)
            base = t[0] if base is None else base
            print(f"{kind} batch of {n}: {name} kernel {t[0] / 1e6:.3f} ms min / {t[len(t) // 2] / 1e6:.3f} ms median "
                  f"({t[0] / 1e6 / n:.3f} ms per image), {t[0] / base:.2f} x k_undistort")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--models"]
    models = len(args) < len(sys.argv) - 1
    if len(args) > 1 and args[0] == "--trace":
        (trace_models if models else trace)(args[1])
    else:
        (run_models if models else run)()
