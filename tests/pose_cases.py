"""Scenes for the refinement of camera poses against a 3D line model: seeded synthetic scenes whose 2D
segments are exact projections of sub-intervals of the model's lines plus clutter, shapes at the lane, wave and tile edges
of k_pose_normal, hand cases from small integers in which every quantity is exact, and the real-data fixtures.  Shared by
tests/test_pose_host.py (the numpy model alone) and tests/test_gpu_pose.py (the library against the model)."""
import math
import os

import numpy as np

from tests import pose_model as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (2D segments, 3D segments) of one camera: a lane, a wave and its neighbours, a tile and its neighbours, three tiles
EDGE_SHAPES = [(1, 1), (63, 300), (64, 300), (65, 300), (255, 513), (256, 512), (257, 513), (513, 1025)]
SEED = 27                                        # of the perturbations of the recovery runs


def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {a.shape} / {b.dtype} {b.shape}"
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero(np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8))
        raise AssertionError(f"{what}: {len(bad)} bytes differ, the first at {bad[0]} of {a.nbytes}")


def same_camera(a, b, what):
    for k in ("K", "R", "t"):
        same_bytes(np.asarray(a[k], np.float64).reshape(-1), np.asarray(b[k], np.float64).reshape(-1), f"{what}: {k}")
    assert (int(a["width"]), int(a["height"])) == (int(b["width"]), int(b["height"])), what


def same_result(got, want, what):
    """every field of two results (the library's or the model's) equal bit for bit"""
    assert len(got["cameras"]) == len(want["cameras"]), what
    for k in range(len(want["cameras"])):
        w = f"{what}: camera {k}"
        same_camera(got["cameras"][k], want["cameras"][k], w)
        g, s = got["summaries"][k], want["summaries"][k]
        assert tuple(g[f] for f in ("status", "iterations", "n_matched")) == tuple(s[f] for f in ("status", "iterations", "n_matched")), \
            (w, g, s)
        for f in ("rms", "last_step", "q", "t"):
            same_bytes(np.asarray(g[f], np.float64).reshape(-1), np.asarray(s[f], np.float64).reshape(-1), f"{w}: summary {f}")
        same_bytes(got["associations"][k], want["associations"][k], f"{w}: associations")
        same_bytes(got["trace"][k], want["trace"][k], f"{w}: trace")


def axis_angle(axis, degrees):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    h = math.radians(degrees) / 2.0
    q = (math.cos(h), a[0] * math.sin(h), a[1] * math.sin(h), a[2] * math.sin(h))
    return np.array(P.rotation(P.unit(q))).reshape(3, 3)


def look_at(centre, target, f, width, height):
    """a camera at `centre` that looks at `target`, y down"""
    z = np.asarray(target, np.float64) - centre; z = z / np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z); x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    K = np.array([[f, 0.0, (width - 1) / 2.0], [0.0, f, (height - 1) / 2.0], [0.0, 0.0, 1.0]])
    return P.camera(K, R, -R @ np.asarray(centre, np.float64), width, height)


def perturbed(cam, degrees, shift, rng):
    """the camera turned by `degrees` about a random axis through its centre, the centre moved by `shift` in a random
    direction"""
    R, t = np.asarray(cam["R"], np.float64), np.asarray(cam["t"], np.float64)
    C = -R.T @ t
    d = rng.normal(size=3); d = d / np.linalg.norm(d)
    R2 = axis_angle(rng.normal(size=3), degrees) @ R
    return P.camera(cam["K"], R2, -R2 @ (C + shift * d), cam["width"], cam["height"])


def project_exact(cam, X):
    """pixels of the points X [n, 3] and their depths, plain numpy"""
    Y = X @ np.asarray(cam["R"], np.float64).T + np.asarray(cam["t"], np.float64)
    x = Y @ np.asarray(cam["K"], np.float64).T
    return x[:, :2] / x[:, 2:3], Y[:, 2]


def observed(cam, segs, rng, n_clutter, noise=0.0, lo=(0.0, 0.3), hi=(0.7, 1.0)):
    """2D segments of a camera: the projection of a sub-interval of every 3D segment that lies in front of it and inside
    the image, then n_clutter unrelated ones; float32 [M, 4]"""
    a = rng.uniform(*lo, len(segs))[:, None]; b = rng.uniform(*hi, len(segs))[:, None]
    A = segs[:, :3] + a * (segs[:, 3:] - segs[:, :3]); B = segs[:, :3] + b * (segs[:, 3:] - segs[:, :3])
    pa, za = project_exact(cam, A); pb, zb = project_exact(cam, B)
    w, h = cam["width"], cam["height"]
    ok = (za > 0.1) & (zb > 0.1)
    for p in (pa, pb):
        ok &= (p[:, 0] > 1) & (p[:, 0] < w - 2) & (p[:, 1] > 1) & (p[:, 1] < h - 2)
    out = np.concatenate([pa[ok], pb[ok]], 1)
    out = out + noise * rng.normal(size=out.shape)
    c0 = rng.uniform([0, 0], [w - 1, h - 1], (n_clutter, 2))
    ang = rng.uniform(0, np.pi, n_clutter); ln = rng.uniform(20, 120, n_clutter)
    clutter = np.concatenate([c0, c0 + ln[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)], 1)
    return np.ascontiguousarray(np.concatenate([out, clutter]), np.float32)


def random_segments(n, rng, half=1.0):
    mid = rng.uniform(-half, half, (n, 3))
    d = rng.normal(size=(n, 3)); d = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.15, 0.5, n)[:, None]
    return np.ascontiguousarray(np.concatenate([mid - d, mid + d], 1))


def recovery_scene(noise=0.0, shift=0.0, n_lines=300, n_cams=3, degrees=0.2, offset=0.02, seed=5):
    """n_lines random segments in a cube, n_cams cameras around it whose 2D segments are exact projections (float32) of
    sub-intervals plus 60 unrelated ones; the start poses are `degrees` / `offset` (of the distance 4) off the truth"""
    rng = np.random.default_rng(seed)
    segs = random_segments(n_lines, rng)
    line = np.arange(n_lines, dtype=np.uint32)
    truth, start, obs = [], [], []
    for k in range(n_cams):
        ang = 2.0 * np.pi * k / n_cams + 0.3
        cam = look_at(np.array([4.0 * math.cos(ang), 4.0 * math.sin(ang), 0.8 * (k % 2) + 0.4]), [0.0, 0.0, 0.0], 1000.0, 1280, 960)
        truth.append(cam)
        obs.append(observed(cam, segs, rng, 60, noise))
        start.append(perturbed(cam, degrees, offset * 4.0, rng))
    if shift:
        s = np.array([shift, -shift, 0.5 * shift])
        segs = np.ascontiguousarray(segs + np.tile(s, 2))

        def moved(cam):
            return P.camera(cam["K"], cam["R"], cam["t"] - cam["R"] @ s, cam["width"], cam["height"])
        truth = [moved(c) for c in truth]; start = [moved(c) for c in start]
    return dict(segs=segs, line=line, truth=truth, cams=start, obs=obs, depth=4.0,
                par=dict(max_distance=2.5, start_distance=20.0))


RECOVERY = dict(plain=dict(), noisy=dict(noise=0.3), shifted=dict(shift=1e5))


def edge_scene(n2d, n3d, seed=3):
    """one camera, n3d random 3D segments, n2d 2D segments: slightly displaced projections of 3D segments drawn at random
    (with repetition), every fifth one unrelated"""
    rng = np.random.default_rng(seed + 1000 * n2d + n3d)
    segs = random_segments(n3d, rng)
    cam = look_at(np.array([3.5, 1.0, 0.7]), [0.0, 0.0, 0.0], 900.0, 1280, 960)
    pick = rng.integers(0, n3d, n2d)
    obs = observed(cam, segs[pick], rng, 0, noise=0.4, lo=(0.0, 0.2), hi=(0.8, 1.0))
    while len(obs) < n2d:                        # (a projection that left the image: an unrelated segment in its place)
        obs = np.concatenate([obs, observed(cam, segs[:0], rng, n2d - len(obs))])
    obs = obs[:n2d].copy()
    unrelated = np.arange(n2d) % 5 == 4
    obs[unrelated] = observed(cam, segs[:0], rng, int(unrelated.sum()))
    return dict(segs=segs, line=np.arange(n3d, dtype=np.uint32) // 2, cams=[perturbed(cam, 0.05, 0.004, rng)], obs=[obs])


def gap_scene():
    """640 segments of one camera of which the waves 1 and 2 of the first tile (64 .. 191) and the whole second tile
    (256 .. 511) are points, which match nothing"""
    s = edge_scene(640, 400, seed=9)
    obs = s["obs"][0]
    dead = np.zeros(640, bool); dead[64:192] = True; dead[256:512] = True
    obs[dead, 2:] = obs[dead, :2]
    return s, dead


def mixed_scene():
    """seven cameras with 0, 300 (none matched: points), 1, 257, 64, 5 and 0 segments against one model"""
    rng = np.random.default_rng(12)
    segs = random_segments(300, rng)
    counts = (0, 300, 1, 257, 64, 5, 0)
    cams, obs = [], []
    for k, n in enumerate(counts):
        ang = 0.9 * k + 0.2
        cam = look_at(np.array([3.8 * math.cos(ang), 3.8 * math.sin(ang), 0.5]), [0.0, 0.0, 0.0], 900.0, 1280, 960)
        o = observed(cam, segs[rng.integers(0, 300, n)], rng, 0, noise=0.3)
        while len(o) < n:
            o = np.concatenate([o, observed(cam, segs[:0], rng, n - len(o))])
        o = o[:n].copy()
        if k == 1:
            o[:, 2:] = o[:, :2]
        cams.append(perturbed(cam, 0.05, 0.004, rng)); obs.append(o)
    return dict(segs=segs, line=np.arange(300, dtype=np.uint32), cams=cams, obs=obs)


# ---- hand cases: K = (64, 0, 64; 0, 64, 64; 0, 0, 1), R = I, t = 0, a 129 x 129 image; every quantity is exact ---------------
HAND_K = ((64.0, 0.0, 64.0), (0.0, 64.0, 64.0), (0.0, 0.0, 1.0))


def hand_camera(R=None):
    return P.camera(HAND_K, np.eye(3) if R is None else R, (0.0, 0.0, 0.0), 129, 129)


def parallel_scene():
    """nine 3D lines along x at depths 2, 4 and 8, each seen by a 2D segment that lies exactly on its projection: the
    shift along x is free.  The centre of the model's box is (0, -0.125, 5): X - c and t + R c are exact."""
    segs, obs = [], []
    for z in (2.0, 4.0, 8.0):
        for y in (-1.0, -0.375, 0.75):           # (nine distinct image rows)
            segs.append((-1.0, y, z, 1.0, y, z))
            v = 64.0 * y / z + 64.0
            obs.append((64.0 - 32.0 / z, v, 64.0 + 48.0 / z, v))
    return dict(segs=np.array(segs), line=np.arange(9, dtype=np.uint32), cams=[hand_camera()], obs=[np.array(obs, np.float32)])


def crossing_scene():
    """nine 3D lines in three directions at three depths, each seen by a 2D segment on its projection (exact)"""
    segs, obs = [], []
    for z in (2.0, 4.0, 8.0):
        for a, b in (((-1.0, -0.5), (1.0, -0.5)), ((0.5, -1.0), (0.5, 1.0)), ((-1.0, -0.75), (1.0, 0.25))):
            segs.append((a[0], a[1], z, b[0], b[1], z))
            obs.append((64.0 * a[0] / z + 64.0, 64.0 * a[1] / z + 64.0, 64.0 * b[0] / z + 64.0, 64.0 * b[1] / z + 64.0))
    return dict(segs=np.array(segs), line=np.arange(9, dtype=np.uint32), cams=[hand_camera()], obs=[np.array(obs, np.float32)])


# ---- the real-data fixtures -----------------------------------------------------------------------------------------------
def real_scene(degrees=0.0, depth_share=0.0):
    """the 26 cameras and their 17 603 segments of real_scene_c0.npz against the 2 503 segments of the reference's optimised
    model (ref_c0_models.npz); the start poses `degrees` / `depth_share` of the view's median depth off the fixture's, from
    SEED"""
    d = np.load(os.path.join(GOLDEN, "real_scene_c0.npz"))
    m = np.load(os.path.join(GOLDEN, "ref_c0_models.npz"))
    rng = np.random.default_rng(SEED)
    w, h = int(d["width"]), int(d["height"])
    fixture = [P.camera(d["K"][i], d["R"][i], d["t"][i], w, h) for i in range(len(d["cam"]))]
    depth = [float(v) for v in d["median_depth"]]
    cams = [perturbed(c, degrees, depth_share * z, rng) if degrees or depth_share else c for c, z in zip(fixture, depth)]
    obs = [np.ascontiguousarray(d["segs"][d["seg_off"][i]:d["seg_off"][i + 1]], np.float32) for i in range(len(fixture))]
    return dict(segs=np.ascontiguousarray(m["optimized_segs"], np.float64), line=np.ascontiguousarray(m["optimized_line"], np.uint32),
                cams=cams, fixture=fixture, obs=obs, depth=depth)


REAL = dict(tenth=dict(degrees=0.1, depth_share=0.002, start_distance=10.0), fifth=dict(degrees=0.2, depth_share=0.004, start_distance=20.0))


def pose_errors(cams, refs, depths):
    """the largest angle (degrees) and the largest centre distance (share of the depth) between cameras and references"""
    d = [P.pose_difference(c, r, z) for c, r, z in zip(cams, refs, depths)]
    return max(v[0] for v in d), max(v[1] for v in d)
