"""Writes tests/golden/ref_c0_models.npz: the two 3D line models the reference publishes for its bundled testdata
(BASELINE config C0, 26 images) -- its result with and without line optimisation -- as flat segments [n, 6] float64
(P1, P2) with the index of each segment's line, the form line3dpp_amd.api.flatten_lines gives.  They are recorded
results: tests/test_compare_host.py compares them with each other without the reference tree.
Run where /root/reference exists:
    python tests/golden/make_ref_models.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from line3dpp_amd.api import flatten_lines  # noqa: E402
from line3dpp_amd.io import read_3d_lines_txt  # noqa: E402

REF_DIR = "/root/reference/testdata/Line3D++_ref/"
STEM = "Line3D++__W_FULL__N_10__sigmaP_2.5__sigmaA_10__epiOverlap_0.25__kNN_10__"
OUT = os.path.join(ROOT, "tests", "golden", "ref_c0_models.npz")


def main():
    arrays = {}
    for key, name in (("optimized", STEM + "OPTIMIZED__vis_3.txt"), ("plain", STEM + "vis_3.txt")):
        segs, line = flatten_lines(read_3d_lines_txt(os.path.join(REF_DIR, name)))
        arrays[key + "_segs"] = segs
        arrays[key + "_line"] = line
        print(f"{key}: {len(segs)} segments on {int(line.max()) + 1} lines")
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
