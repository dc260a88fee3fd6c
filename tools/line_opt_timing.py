"""Line bundling (reconstruct3Dlines(use_CERES=True)) on the BASELINE configurations: residuals per line, stopping rules,
kernel time and the wall time of reconstruct3Dlines with and without the stage.  One JSON line per configuration.

    python tools/line_opt_timing.py [C0 C1 C2]     (one GPU process; run it under a time limit)

Wall times: median of 3 calls of reconstruct3Dlines after one untimed call, each after the same matchImages.  Kernel
time: the stage's event pair at timing level 2 (l3d_line_opt_stats), from a separate call."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from line3dpp_amd.api import Line3D  # noqa: E402
from line3dpp_amd.scene import make_config  # noqa: E402


def wall(g, **kw):
    g.reconstruct3Dlines(3, **kw)
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        assert g.reconstruct3Dlines(3, **kw)
        ts.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ts))


def main(names):
    for name in names:
        sc = make_config(name)
        g = Line3D()
        g.add_scene(sc)
        assert g.matchImages()
        off_ms = wall(g)
        on_ms = wall(g, use_CERES=True)
        lines = g.get3Dlines()
        st = g.lineOptStats()
        g.L.l3d_set_timing_level(g.h, 2)
        assert g.reconstruct3Dlines(3, use_CERES=True)
        kst = g.lineOptStats()
        nres = np.array([len(L["residuals"]) for L in lines])
        b = max(st["lines_bundled"], 1)
        out = dict(config=name, lines_out=len(lines), recon_ms_off=round(off_ms, 2), recon_ms_on=round(on_ms, 2),
                   kernel_ms=round(kst["kernel_ms"], 3), stats=st,
                   stop_fraction={k: round(st[k] / b, 4) for k in ("stop_gradient", "stop_function", "stop_parameter",
                                                                   "stop_max_iter", "stop_other")},
                   residuals_per_output_line=dict(mean=round(float(nres.mean()), 2),
                                                  pct={q: int(np.percentile(nres, q)) for q in (10, 50, 90, 99, 100)},
                                                  le16=round(float((nres <= 16).mean()), 4),
                                                  le64=round(float((nres <= 64).mean()), 4)))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or ["C0", "C1", "C2"])
