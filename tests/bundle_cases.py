"""Scenes for the joint bundle of cameras and 3D lines, built from the generators of tests/pose_cases.py and
tests/refit_cases.py: a ring of cameras about random segments whose 2D segments are exact projections of sub-intervals, with
chosen lines per camera, chosen numbers of eligible lines, of cells per camera, of observations per cell and of 2D segments
in all, and the scenes whose step control rejects a step or holds a line for a step.  Every case is a dict: segs, line,
cams, obs, fixed (or None) and par (the wrappers' arguments).  Shared by tests/test_bundle_host.py (the numpy model alone,
which asserts that every case has the shape it claims) and tests/test_gpu_bundle.py (the library against the model)."""
import math

import numpy as np

from tests import bundle_model as BM
from tests import pose_cases as PC
from tests import pose_model as PO
from tests import refit_cases as RC
from tests import refit_model as RM

SEED = 29


def model_par(max_distance=2.5, max_angle=10.0, min_overlap=0.5, near=1e-6, **kw):
    """the wrappers' arguments as the numpy model takes them"""
    return dict(BM.DEFAULTS, max_distance=max_distance, min_cos2=RM.AM.min_cos2_of(max_angle), min_overlap=min_overlap, near_plane=near, **kw)


def ring(n_lines, n_cams, seed=SEED, sees=None, clutter=0, cam_degrees=0.05, cam_shift=0.004, line_degrees=0.2, line_shift=0.003,
         half=0.8, visibility=3, **par):
    """n_lines random segments in a cube, n_cams cameras on a ring about it; camera k observes the lines sees(k) (None:
    all) through exact projections of sub-intervals, plus `clutter` unrelated 2D segments; the start cameras and the model
    are the truth perturbed"""
    rng = np.random.default_rng(seed)
    truth = PC.random_segments(n_lines, rng, half)
    cams, obs, true_cams = [], [], []
    for k in range(n_cams):
        ang = 2.0 * math.pi * k / n_cams + 0.3
        cam = PC.look_at(np.array([4.0 * math.cos(ang), 4.0 * math.sin(ang), 0.8 * (k % 2) + 0.4]), [0.0, 0.0, 0.0], 1000.0, 1280, 960)
        mine = np.arange(n_lines) if sees is None else np.asarray(sees(k), int)
        true_cams.append(cam)
        obs.append(PC.observed(cam, truth[mine], rng, clutter))
        cams.append(PC.perturbed(cam, cam_degrees, cam_shift, rng))
    return dict(truth=truth, segs=RC.perturbed_lines(truth, line_degrees, line_shift, rng), line=np.arange(n_lines, dtype=np.uint32),
                cams=cams, true_cams=true_cams, obs=obs, fixed=None, par=dict(max_distance=6.0, visibility=visibility, **par))


def problem(s, **kw):
    """the model's tables of a case (the numpy association)"""
    par = model_par(**dict(s["par"], **kw))
    assoc = RM.associations(s["segs"], s["line"], s["cams"], s["obs"], par)
    return BM.prepare(s["segs"], s["line"], s["cams"], s["obs"], assoc, s["fixed"], par)


def with_eligible(n, n_cams=3, seed=SEED, **kw):
    """a ring scene with exactly n lines, all of them eligible: the first n eligible lines of a larger scene (what is taken
    out only makes the matches of what stays less ambiguous)"""
    s = ring(n + n // 2 + 16, n_cams, seed, **kw)
    if n > 100:
        s["par"]["max_distance"] = 3.0               # (so many lines in the cube: a narrower gate keeps the matches unique)
    keep = problem(s).eligible[:n]
    assert len(keep) == n
    s["segs"] = np.ascontiguousarray(s["segs"][keep]); s["truth"] = s["truth"][keep]; s["line"] = np.arange(n, dtype=np.uint32)
    return s


def cells_in_camera(n, seed=SEED):
    """four cameras; camera 0 keeps the 2D segments of exactly n cells"""
    s = with_eligible(n + 12, 4, seed)
    P = problem(s)
    mine = P.obs_rec[P.obs_rec["camera"] == 0]
    lines = np.unique(mine["line"])[:n]
    keep = np.sort(mine["segment"][np.isin(mine["line"], lines)])
    s["obs"][0] = np.ascontiguousarray(s["obs"][0][keep])
    return s


def split_cells(seed=SEED):
    """camera 0's first five 2D segments cut into two collinear pieces, the next five into three: cells of 1, 2 and 3
    observations"""
    s = with_eligible(24, 3, seed)
    out = []
    for i, sg in enumerate(s["obs"][0].astype(np.float64)):
        parts = 2 if i < 5 else 3 if i < 10 else 1
        a, b = sg[:2], sg[2:]
        for j in range(parts):
            out.append(np.concatenate([a + (b - a) * (j / parts), a + (b - a) * ((j + 1) / parts)]))
    s["obs"][0] = np.ascontiguousarray(out, np.float32)
    return s


def disjoint(seed=SEED):
    """six cameras, two groups of three that share no line"""
    n = 24
    return ring(n, 6, seed, sees=lambda k: np.arange(0, n // 2) if k < 3 else np.arange(n // 2, n))


def odd_cameras(seed=SEED):
    """five cameras: camera 1 has no 2D segment, camera 3 looks away from the scene and matches nothing"""
    s = ring(30, 5, seed)
    s["obs"][1] = np.zeros((0, 4), np.float32)
    c = s["cams"][3]
    R = np.diag([-1.0, 1.0, -1.0]) @ np.asarray(c["R"], np.float64)          # turned about its y axis: the scene lies behind it
    C = -np.asarray(c["R"], np.float64).T @ np.asarray(c["t"], np.float64)
    s["cams"][3] = PO.camera(c["K"], R, -R @ C, c["width"], c["height"])
    return s


def many_segments(total, seed=SEED):
    """three cameras with `total` 2D segments in all, most of them clutter"""
    s = ring(40, 3, seed)
    rng = np.random.default_rng(seed + 1)
    have = sum(len(o) for o in s["obs"])
    extra = total - have
    assert extra > 0
    per = [extra // 3, extra // 3, extra - 2 * (extra // 3)]
    for k in range(3):
        w, h = s["cams"][k]["width"], s["cams"][k]["height"]
        c0 = rng.uniform([0, 0], [w - 1, h - 1], (per[k], 2))
        ang = rng.uniform(0, np.pi, per[k]); ln = rng.uniform(20, 120, per[k])
        clutter = np.concatenate([c0, c0 + ln[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)], 1).astype(np.float32)
        s["obs"][k] = np.ascontiguousarray(np.concatenate([s["obs"][k], clutter]))
    assert sum(len(o) for o in s["obs"]) == total
    return s


def held_among_eligible(seed=SEED):
    """four cameras, visibility 3: a third of the lines is seen by two cameras only and is held"""
    n = 36
    return ring(n, 4, seed, sees=lambda k: np.arange(n) if k < 2 else [i for i in range(n) if i % 3])


def with_fixed(which, seed=SEED):
    s = ring(30, 4, seed)
    s["fixed"] = np.array([1 if k in which else 0 for k in range(4)], np.uint8)
    return s


def reject():
    """the second round of the alternation scene of §28: cameras and model as the numpy model leaves them after one call.
    With twice the observations of the first round and the damping back at its start, steps at a damping of 1e-7 overshoot
    and are rejected, the ones at 1e-6 are accepted"""
    s = alternation()
    first = BM.bundle(s["segs"], s["line"], s["cams"], s["obs"], **model_par(**s["par"]))
    s["segs"], s["line"], s["cams"] = first["segments"], first["line"], first["cameras"]
    return s


def pivot(seed=SEED):
    """two cameras, visibility 2, every camera fixed, next to no damping at all: a line's four parameters are determined by
    two views only where the line is not in a plane with both centres, and line 0 is: its 4 x 4 factor has a pivot that
    fails, so it is held for the step while the others move"""
    s = ring(12, 2, seed, visibility=2, initial_damping=1e-300, min_damping=1e-300, max_iterations=4)
    C = [-np.asarray(c["R"], np.float64).T @ np.asarray(c["t"], np.float64) for c in s["true_cams"]]
    base = C[1] - C[0]
    mid = np.array([0.1, -0.05, 0.2])
    d = 0.3 * (base / np.linalg.norm(base)) + 0.05 * (mid - C[0])
    seg = np.concatenate([mid - d, mid + d])
    rng = np.random.default_rng(seed + 2)
    s["truth"][0] = seg
    s["segs"][0] = seg
    for k in range(2):
        first = PC.observed(s["true_cams"][k], seg[None], rng, 0)
        assert len(first) == 1
        s["obs"][k] = np.ascontiguousarray(np.concatenate([first, s["obs"][k][1:]]))
    s["cams"] = list(s["true_cams"])
    s["fixed"] = np.ones(2, np.uint8)
    return s


def shifted(s, shift):
    out = RC.shifted(s, shift)
    out["fixed"] = s["fixed"]
    return out


def fan():
    s = RC.fan()
    s["fixed"] = None
    return s


def alternation():
    s = RC.alternation()
    s["fixed"] = None
    return s


# name -> builder of the cases that tests/test_gpu_bundle.py compares with the model at tolerance 0
CASES = {
    "1 line x 2 cameras": lambda: with_eligible(1, 2, visibility=2),
    **{f"{n} eligible lines": (lambda n=n: with_eligible(n)) for n in (63, 64, 65, 255, 256, 257)},
    "a camera with 64 cells": lambda: cells_in_camera(64),
    "a camera with 65 cells": lambda: cells_in_camera(65),
    "fan": fan,
    "cells of 1, 2 and 3 observations": split_cells,
    "two groups of cameras that share no line": disjoint,
    "a camera without segments, one that matches nothing": odd_cameras,
    **{f"{n} 2D segments": (lambda n=n: many_segments(n)) for n in (4095, 4096, 4097)},
    "held lines among eligible ones": held_among_eligible,
    "one camera fixed": lambda: with_fixed({1}),
    "some cameras fixed": lambda: with_fixed({0, 2}),
    "all cameras fixed": lambda: with_fixed({0, 1, 2, 3}),
    "no eligible line": lambda: ring(20, 3, visibility=4),
    "max_iterations = 0": lambda: ring(20, 3, max_iterations=0),
    "reject": reject,
    "pivot": pivot,
    "a shift of 1e5": lambda: shifted(ring(30, 3), 1e5),
    "ambiguous segments used": lambda: ring(60, 3, half=0.35, use_ambiguous=True),
    "ambiguous segments left out": lambda: ring(60, 3, half=0.35, use_ambiguous=False),
}
