"""Scenes for the refit of the 3D lines against cameras and their 2D segments, built from the generators of
tests/pose_cases.py: the recovery scenes (every line turned and moved, true cameras), a small scene for the stage-by-stage
comparisons, a fan of cameras that gives lines chosen numbers of observations, and the alternation scene.  Shared by
tests/test_refit_host.py (the numpy model and the host hooks) and tests/test_gpu_refit.py (the library against the model)."""
import math

import numpy as np

from tests import pose_cases as PC
from tests import pose_model as PO

SEED = 28                                        # of the perturbations of the lines


def perturbed_lines(segs, degrees, shift, rng):
    """every segment turned by `degrees` about a random axis through its mid point and moved by `shift` in a random direction"""
    out = np.empty_like(segs)
    for i, s in enumerate(segs):
        mid = 0.5 * (s[:3] + s[3:])
        R = PC.axis_angle(rng.normal(size=3), degrees)
        d = rng.normal(size=3); d = d / np.linalg.norm(d) * shift
        out[i, :3] = mid + R @ (s[:3] - mid) + d
        out[i, 3:] = mid + R @ (s[3:] - mid) + d
    return np.ascontiguousarray(out)


def recovery(noise=0.0, n_lines=300, n_cams=6, degrees=0.5, shift=0.01, seed=SEED):
    """recovery_scene with its true cameras; the model is the truth with every line turned and moved"""
    s = PC.recovery_scene(noise=noise, n_lines=n_lines, n_cams=n_cams)
    rng = np.random.default_rng(seed)
    return dict(truth=s["segs"], segs=perturbed_lines(s["segs"], degrees, shift, rng), line=s["line"], cams=s["truth"], obs=s["obs"],
                par=dict(max_distance=6.0, visibility=3))


def small(n_lines=40, n_cams=3, seed=SEED, **kw):
    """a small recovery scene for the comparisons against the numpy model"""
    return recovery(n_lines=n_lines, n_cams=n_cams, seed=seed, **kw)


def alternation(n_lines=300, n_cams=6, seed=SEED):
    """cameras 0.1 degrees / 1 % of the distance off, lines 0.3 degrees / 0.005 off"""
    s = PC.recovery_scene(n_lines=n_lines, n_cams=n_cams, degrees=0.1, offset=0.01)
    rng = np.random.default_rng(seed)
    return dict(truth=s["segs"], segs=perturbed_lines(s["segs"], 0.3, 0.005, rng), line=s["line"], cams=s["cams"],
                true_cams=s["truth"], obs=s["obs"], par=dict(max_distance=6.0, visibility=3))


FAN_COUNTS = (0, 1, 16, 17, 64, 65)


def fan(counts=FAN_COUNTS, seed=SEED):
    """len(counts) nearly vertical lines stacked above one another, which every camera of a ring sees from the side and
    apart from the others, and max(counts) cameras on that ring: line j is seen by the first counts[j] cameras, each
    through the exact projection of a sub-interval; the model is the truth turned by 0.2 degrees"""
    rng = np.random.default_rng(seed)
    n = len(counts)
    truth = np.array([[0.1 * j - 0.2, 0.05 * j, 0.5 * j - 0.25 * n, 0.1 * j - 0.15, 0.05 * j + 0.03, 0.5 * j - 0.25 * n + 0.35] for j in range(n)])
    cams, obs = [], []
    for k in range(max(counts)):
        ang = 2.0 * math.pi * k / max(counts)
        cam = PC.look_at(np.array([5.0 * math.cos(ang), 5.0 * math.sin(ang), 1.0 + 0.5 * (k % 3)]), [0.0, 0.0, 0.0], 900.0, 1280, 960)
        seen = np.array([j for j in range(n) if counts[j] > k], int)
        cams.append(cam); obs.append(PC.observed(cam, truth[seen], rng, 0))
    return dict(truth=truth, segs=perturbed_lines(truth, 0.2, 0.002, rng), line=np.arange(n, dtype=np.uint32), cams=cams, obs=obs,
                par=dict(max_distance=6.0, visibility=3))


def shifted(scene, shift):
    """the scene moved by (shift, -shift, shift / 2): model and cameras"""
    s = np.array([shift, -shift, 0.5 * shift])
    out = dict(scene)
    out["segs"] = np.ascontiguousarray(scene["segs"] + np.tile(s, 2))
    out["cams"] = [PO.camera(c["K"], c["R"], c["t"] - c["R"] @ s, c["width"], c["height"]) for c in scene["cams"]]
    return out


def carrier_errors(lines, truth):
    """the largest distance of each true segment's end points from the carrier (P1, P2) of its line"""
    out = np.zeros(len(truth))
    for l, t in enumerate(truth):
        P1, P2 = np.asarray(lines["P1"][l], np.float64), np.asarray(lines["P2"][l], np.float64)
        d = (P2 - P1) / np.linalg.norm(P2 - P1)
        w = t.reshape(2, 3) - P1
        out[l] = np.linalg.norm(w - np.outer(w @ d, d), axis=1).max()
    return out
