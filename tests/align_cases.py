"""Scenes of the alignment of two 3D line models, shared by tests/test_align_host.py and
tests/test_gpu_align.py: built from seeds (numpy.random.default_rng), and hand cases from small integers in which every
quantity of the contract is exact."""
import math
import os

import numpy as np

from tests import align_model as A
from tests import compare_model as CM

TILE = 256
# (n_Q, n_R, slice_chunks) of the one-iteration cases: a lone lane, a wave edge, a tile edge, lanes past n_q in the last
# tile, three tiles for the host's sequential sum, sliced references
EDGE_SHAPES = [(1, 1, 0), (63, 300, 1), (64, 300, 1), (65, 300, 1), (255, 513, 1), (256, 256, 0), (257, 513, 2), (513, 1025, 0)]
SLICING_SHAPE = (255, 768)
SLICINGS = [1, 2, 3, 0, 0xFFFFFFFF]


def axis_angle(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(degrees) / 2.0
    return (math.cos(h),) + tuple(math.sin(h) * a)


def perturbed(T, c, diag, degrees, scale_off, shift, rng):
    """T followed by a rotation of `degrees` about a random axis and a scaling by 1 + scale_off about c, and a shift of
    `shift` x diag in a random direction: the model's own update with that step"""
    def direction():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)
    w = math.radians(degrees) * direction()
    tau = shift * diag * direction()
    return A.update(T, [w[0], w[1], w[2], scale_off, tau[0], tau[1], tau[2]], c)


def random_segments(rng, n, lo=0.0, hi=1.0):
    return np.ascontiguousarray(rng.uniform(lo, hi, (n, 6)))


def recovery_scene(seed=7, noise=0.0, shift=0.0, estimate_scale=True, n=300, dropped=0.2, added=60, start=(4.0, 0.03, 0.02)):
    """Q: n random segments in the unit cube.  R = T*(Q) with scale 1.3 and a rotation of 25 degrees, a share `dropped`
    of the lines left out and `added` unrelated ones put in, end points moved by `noise` x N(0, 1) and the whole by
    `shift` along every axis; the start is T* taken `start` = (degrees, share of scale, share of diag) off.
    -> dict(q, ql, r, rl, T_true, initial, diag, par): par = the keyword arguments of the model and the wrapper"""
    rng = np.random.default_rng(seed)
    q = random_segments(rng, n)
    ql = np.arange(n, dtype=np.uint32)
    t = rng.uniform(-1.0, 1.0, 3) + shift
    T_true = A.entry(A.similarity(1.3, axis_angle(rng.normal(size=3), 25.0), t))
    keep = np.flatnonzero(rng.random(n) >= dropped)
    r = A.transform(q[keep], T_true)
    lo, hi = r.reshape(-1, 3).min(0), r.reshape(-1, 3).max(0)
    extra = np.concatenate([rng.uniform(lo, hi, (added, 3)), rng.uniform(lo, hi, (added, 3))], 1)
    r = np.concatenate([r, extra])
    if noise:
        r = r + noise * rng.normal(size=r.shape)
    order = rng.permutation(len(r))
    r = np.ascontiguousarray(r[order])
    rl = np.arange(len(r), dtype=np.uint32)
    c, diag = A.bounding_box(r)
    degrees, scale_off, off = start
    initial = perturbed(T_true, c, diag, degrees, scale_off if estimate_scale else 0.0, off, rng)
    par = dict(max_distance=0.005 * diag, start_distance=0.1 * diag, estimate_scale=1 if estimate_scale else 0)
    return dict(q=q, ql=ql, r=r, rl=rl, T_true=T_true, initial=initial, diag=diag, par=par, n_kept=len(keep))


RECOVERY = dict(plain=dict(), noisy=dict(noise=1e-3), shifted=dict(shift=1e5), fixed_scale=dict(estimate_scale=False))
# the start of the start-distance case: so far off that the gate of max_distance alone finds too few lines
FAR_START = (12.0, 0.08, 0.06)


def edge_scene(n_q, n_r, seed=None):
    """n_q queries and n_r references of which min(n_q, n_r) correspond under a similarity, the rest unrelated, the
    references in random order; the start a little off, so that one iteration has most correspondences matched and a
    step to take.  -> dict(q, ql, r, rl, initial, par)"""
    rng = np.random.default_rng(1000 * n_q + n_r if seed is None else seed)
    q = random_segments(rng, n_q)
    T_true = A.entry(A.similarity(0.8, axis_angle(rng.normal(size=3), 40.0), rng.uniform(-2.0, 2.0, 3)))
    both = min(n_q, n_r)
    r = np.concatenate([A.transform(q[:both], T_true), random_segments(rng, n_r - both, -1.0, 2.0)])
    r = np.ascontiguousarray(r[rng.permutation(n_r)])
    c, diag = A.bounding_box(r)
    initial = perturbed(T_true, c, diag, 0.3, 0.003, 0.002, rng)
    return dict(q=q, ql=np.arange(n_q, dtype=np.uint32) // 2, r=r, rl=np.arange(n_r, dtype=np.uint32) // 3, initial=initial,
                T_true=T_true, diag=diag, par=dict(max_distance=0.02 * diag))


def gap_scene():
    """three tiles of queries in which waves 1 and 2 of the first tile and the whole second tile have no match (they are
    moved far away): their sums are 37 times +0.0"""
    s = edge_scene(3 * TILE, 3 * TILE, seed=99)
    far = np.r_[64:192, 256:512]
    s["q"][far] += 50.0
    s["far"] = far
    return s


def parallel_scene():
    """small integers: every reference runs along x, so the translation along x is free -> DEGENERATE (the pivot of
    column 4 is exactly 0: d x ((d . e_0) / L2) = (8, 0, 0) x (8 / 64) = e_0)"""
    r = np.array([[0, y, z, 8, y, z] for y in (0, 4, 8) for z in (0, 4, 8)], np.float64)
    q = r.copy()
    q[:, [1, 4]] += 0.25
    return dict(q=q, ql=np.arange(9, dtype=np.uint32), r=r, rl=np.arange(9, dtype=np.uint32), par=dict(max_distance=1.0, min_matches=1))


def displaced_case():
    """one query, the reference (0,0,0)-(8,0,0) moved by (0, 0, 3): r = (0, 0, 3) at both end points, cost = 18"""
    r = np.array([[0, 0, 0, 8, 0, 0]], np.float64)
    q = np.array([[0, 0, 3, 8, 0, 3]], np.float64)
    one = np.zeros(1, np.uint32)
    return q, one, r, one


def same_bytes(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if got.tobytes() != want.tobytes():
        a = got.reshape(-1).view(np.uint8).reshape(got.size, -1); b = want.reshape(-1).view(np.uint8).reshape(want.size, -1)
        bad = np.flatnonzero((a != b).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ, first at {bad[0]}: "
                             f"{got.reshape(-1)[bad[0]]!r} != {want.reshape(-1)[bad[0]]!r}")


def similarity_array(T):
    """a similarity dict (the model's, or the wrapper's) as one SIMILARITY_DTYPE record"""
    out = np.zeros((), A.SIMILARITY_DTYPE)
    out["scale"] = T["scale"]; out["q"] = T["q"]; out["t"] = T["t"]
    return out


def same_result(got, want, what):
    """a result of the library's wrapper against the model's: every field, tolerance 0"""
    same_bytes(similarity_array(got["similarity"]), similarity_array(want["similarity"]), what + ": similarity")
    gs, ws = got["summary"], want["summary"]
    assert (gs["status"], gs["iterations"], gs["n_matched"]) == (ws["status"], ws["iterations"], ws["n_matched"]), f"{what}: {gs} != {ws}"
    for k in ("rms", "last_step", "diag"):
        same_bytes(np.float64(gs[k]), np.float64(ws[k]), f"{what}: summary {k}")
    same_bytes(np.asarray(gs["center"], np.float64), np.asarray(ws["center"], np.float64), what + ": center")
    same_bytes(got["segments"], want["segments"], what + ": transformed segments")
    for k in ("matches_q", "matches_r"):
        assert got[k].dtype == CM.LINE_MATCH_DTYPE
        same_bytes(got[k], want[k], f"{what}: {k}")
    assert len(got["trace"]) == len(want["trace"]), what
    for name in A.ITERATION_DTYPE.names:
        same_bytes(got["trace"][name], want["trace"][name], f"{what}: trace {name}")


def real_scene():
    """the reference's two published models of its testdata: Q = the optimised result taken into another
    frame by the inverse of a known similarity T_true, R = the plain result; the start is T_true 2 degrees, 2 % and 0.01
    of the diagonal off.  max_distance = 0.002 x extent, the figure §18 asserts on the two models in one frame."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_c0_models.npz"))
    a, al, r, rl = d["optimized_segs"], d["optimized_line"], d["plain_segs"], d["plain_line"]
    rng = np.random.default_rng(18)
    T_true = A.entry(A.similarity(0.4, axis_angle(rng.normal(size=3), 130.0), (3.0, -7.0, 11.0)))
    M = np.linalg.inv(A.matrix(T_true))
    q = np.ascontiguousarray(np.concatenate([a[:, :3] @ M[:3, :3].T + M[:3, 3], a[:, 3:] @ M[:3, :3].T + M[:3, 3]], 1))
    c, diag = A.bounding_box(r)
    ext = CM.extent(a)
    initial = perturbed(T_true, c, diag, 2.0, 0.02, 0.01, rng)
    return dict(q=q, ql=al, r=np.ascontiguousarray(r), rl=rl, T_true=T_true, initial=initial, diag=diag, extent=ext,
                par=dict(max_distance=0.002 * ext, start_distance=0.032 * ext))
