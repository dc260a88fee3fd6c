"""Inputs for l3d_triangulate_points (k_triangulate.hip) at its edges, and the high-precision reference they are judged by
(tests/test_triangulate_cases.py on the CPU, tests/test_gpu_triangulate.py on the device).

The reference, `truth(M)`: per point the 4x4 M exactly as triangulate_model.normal_matrices returns it -- the doubles the
kernel also forms: same order of the sums, no fused multiply-add -- through mpmath.eigsy at 60 digits; the eigenvector of
the eigenvalue of smallest magnitude; X = v[0:3] / v[3], rounded to double.  mpmath is needed to make the fixture and to
check it again on the CPU, not to run the GPU test: tests/golden/triangulate_truth.npz holds every case's inputs and its
truth.  Regenerate with
    python -m tests.triangulate_cases
Every case is built from its seed with elementwise arithmetic, libm's sin and cos and numpy's Generator only (no BLAS, no
vectorised transcendental), so the stored inputs can be required bit for bit.

Accuracy: over the valid finite points of a case, with `extent` the largest side of the point box before any shift,
    e_x   = largest |X_x - T| / extent                        for x = the device, solve_svd, solve_eigh
    bound = max(4 min(e_svd, e_eigh), 4 eps max(1, max|T| / extent))
The device has to be no worse than four times the better of two standard fp64 host solvers, each measured against the
high-precision eigenvector of the same matrix; the floor is what storing X in a double costs.  A case says something only
while min(e_svd, e_eigh) <= YARDSTICK_MAX."""
import math
import os

import numpy as np

from tests import triangulate_model as TM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "triangulate_truth.npz")
WIDTH, HEIGHT, FOCAL, HALF, RADIUS = 1024, 768, 620.0, 10.0, 25.0
K = np.array([[FOCAL, 0.0, WIDTH / 2], [0.0, FOCAL, HEIGHT / 2], [0.0, 0.0, 1.0]])
SHIFT = np.array([1.0, -0.7, 0.3])
NOISE = 0.5
EPS = float(np.finfo(np.float64).eps)
YARDSTICK_MAX = 1e-5
DPS = 60
LDS_CAMERAS = 341                           # kTriLdsBytes / 96: the most cameras k_triangulate stages in LDS
FIELDS = ("P", "off", "cam", "xy")

EDGE_PREFIXES = (1, 255, 256, 257, 513)
EDGE_TWO_OBSERVATIONS = (254, 255, 256, 512)
LONG_OBSERVATIONS = 5000

# the contract batch: where the special points sit among the ordinary ones (two waves of 64 lanes, both mixed) and which
# cameras beyond the ring of 12 they use
CONTRACT_POINTS = 128
AT_INFINITY, ONE_CAMERA, DIAGONAL_2, DIAGONAL_3, NAN_PIXEL, INF_PIXEL, NAN_P = 3, 17, 31, 32, 63, 64, 65
SPECIAL = (AT_INFINITY, ONE_CAMERA, DIAGONAL_2, DIAGONAL_3, NAN_PIXEL, INF_PIXEL, NAN_P)
CAM_INFINITY, CAM_DIAGONAL_2, CAM_DIAGONAL_3, CAM_NAN, CAM_UNUSED, CONTRACT_CAMERAS = 12, 18, 19, 20, 21, 22
CAM_ONE = 7
INFINITY_K = np.array([[512.0, 0.0, 256.0], [0.0, 512.0, 128.0], [0.0, 0.0, 1.0]])
INFINITY_CENTRES = ((4.0, 1.0, 0.5), (-2.0, 3.0, 1.0), (0.5, -1.5, 2.0))
INFINITY_DIRECTION = (1.0, 1.0, 2.0)
INFINITY_M33 = 17629184.0


# ---- geometry, elementwise ---------------------------------------------------------------------------------------------
def _mm(A, B):
    """A [r, 3] @ B [3, c] as three ordered elementwise products: the same doubles on every machine"""
    return (A[:, 0:1] * B[0] + A[:, 1:2] * B[1]) + A[:, 2:3] * B[2]


def _unit(v):
    return v / math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def _lookat(C, target):
    z = _unit(target - C)
    x = _unit(np.cross(z, np.array([0.0, 0.0, 1.0])))
    return np.stack([x, np.cross(z, x), z], 0)


def camera(Kc, R, C):
    """P = Kc [R | -R C]"""
    return _mm(Kc, np.column_stack([R, -_mm(R, C.reshape(3, 1))[:, 0]]))


def ring(n_cams, rng, shift=None):
    """cameras on a circle of radius 25 around the origin, heights within +-2, looking at a point near the centre; with
    `shift` the whole ring stands that far away: -> (P [n, 3, 4], centres [n, 3])"""
    Ps, Cs = [], []
    for j in range(n_cams):
        phi = 2 * math.pi * j / n_cams
        C = np.array([RADIUS * math.cos(phi), RADIUS * math.sin(phi), rng.uniform(-2, 2)])
        R = _lookat(C, rng.normal(0, 0.5, 3))
        if shift is not None:
            C = C + shift
        Ps.append(camera(K, R, C)); Cs.append(C)
    return np.array(Ps), np.array(Cs)


def observe(Ps, X, seen, rng, noise=NOISE):
    """CSR observations: seen[i] = the cameras of point i in order, repeats allowed; every observation its own noise"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in seen])]).astype(np.uint64)
    cam = np.array([c for s in seen for c in s], np.uint32)
    Xo = X[np.repeat(np.arange(len(X)), [len(s) for s in seen])]
    Pc = Ps[cam]
    x = ((Pc[:, :, 0] * Xo[:, 0:1] + Pc[:, :, 1] * Xo[:, 1:2]) + Pc[:, :, 2] * Xo[:, 2:3]) + Pc[:, :, 3]
    xy = x[:, :2] / x[:, 2:3]
    if noise:
        xy = xy + rng.normal(0.0, noise, xy.shape)
    return off, cam, np.ascontiguousarray(xy)


def _pack(P, off, cam, xy, X, **more):
    return dict(P=np.ascontiguousarray(P), off=off, cam=cam, xy=xy, extent=np.float64(np.ptp(X, axis=0).max()), **more)


def _ring_points(seed, n_points, n_cams, lo, hi, shift=None):
    """the ring, n_points in the scene's box, each seen by lo .. hi cameras: -> (rng, P, centres, X, seen)"""
    rng = np.random.default_rng(seed)
    Ps, Cs = ring(n_cams, rng, shift)
    X = rng.uniform(-HALF, HALF, (n_points, 3))
    seen = [np.sort(rng.choice(n_cams, size=rng.integers(lo, hi + 1), replace=False)) for _ in range(n_points)]
    return rng, Ps, Cs, X, seen


# ---- the accuracy cases --------------------------------------------------------------------------------------------------
def _origin(shift=None, seed=2201):
    rng, Ps, _, X, seen = _ring_points(seed, 64, 12, 3, 9, shift)
    return _pack(Ps, *observe(Ps, X if shift is None else X + shift, seen, rng), X)


def _scaled_P():
    c = _origin()
    c["P"][0::3] *= 2.0 ** -4                   # P is homogeneous: the pixels stay, M's rows change weight
    c["P"][1::3] *= 2.0 ** 4
    return c


def _edges():
    rng, Ps, _, X, seen = _ring_points(2202, 513, 40, 3, 9)
    for i in EDGE_TWO_OBSERVATIONS:
        seen[i] = seen[i][:2]
    return _pack(Ps, *observe(Ps, X, seen, rng), X)


def _lds_edge():
    """342 cameras: camera 340 is the last one staged in LDS when 341 are passed, camera 341 exists in the cache form only"""
    rng = np.random.default_rng(2203)
    Ps, _ = ring(LDS_CAMERAS + 1, rng)
    X = rng.uniform(-HALF, HALF, (128, 3))
    seen = []
    for i in range(128):
        fixed = [LDS_CAMERAS - 1] if i < 64 else [LDS_CAMERAS - 1, LDS_CAMERAS]
        others = rng.choice(LDS_CAMERAS - 1, size=rng.integers(3, 13) - len(fixed), replace=False)
        seen.append(np.sort(np.concatenate([others, fixed])))
    return _pack(Ps, *observe(Ps, X, seen, rng), X)


def _long_list():
    rng = np.random.default_rng(2204)
    Ps, _ = ring(300, rng)
    X = rng.uniform(-HALF, HALF, (64, 3))
    seen = [rng.integers(0, 300, LONG_OBSERVATIONS), np.zeros(0, np.int64)]
    seen += [np.sort(rng.choice(300, size=3, replace=False)) for _ in range(62)]
    return _pack(Ps, *observe(Ps, X, seen, rng), X)


# ---- the contract batch --------------------------------------------------------------------------------------------------
def _contract():
    """128 points: ordinary ones as in `origin`, and at SPECIAL the points whose results the contract spells out"""
    rng, Ps, Cs, X, seen = _ring_points(2205, CONTRACT_POINTS, 12, 3, 9)
    P = np.zeros((CONTRACT_CAMERAS, 3, 4))
    P[:12] = Ps
    for j, C in enumerate(INFINITY_CENTRES):                                     # +C1, -C1, +C2, -C2, +C3, -C3
        P[CAM_INFINITY + 2 * j] = camera(INFINITY_K, np.eye(3), np.array(C))
        P[CAM_INFINITY + 2 * j + 1] = camera(INFINITY_K, np.eye(3), -np.array(C))
    P[CAM_DIAGONAL_2] = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]]               # M = diag(4, 4, 0, 8) under `corners`
    P[CAM_DIAGONAL_3] = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]               # M = diag(4, 4, 8, 0)
    P[CAM_NAN] = Ps[5]
    P[CAM_NAN, 1, 2] = np.nan
    P[CAM_UNUSED] = Ps[0]                                                        # finite here; the test poisons a copy
    seen[ONE_CAMERA] = np.array([CAM_ONE] * 3)
    seen[NAN_P] = np.array([2, 5, 9])                                            # observed through camera 5's finite twin
    off, cam, xy = observe(P, X, seen, rng)
    off = off.astype(np.int64)
    cams = [list(cam[off[i]:off[i + 1]]) for i in range(CONTRACT_POINTS)]
    pix = [[tuple(p) for p in xy[off[i]:off[i + 1]]] for i in range(CONTRACT_POINTS)]
    d = _mm(INFINITY_K, np.array(INFINITY_DIRECTION).reshape(3, 1))[:, 0]
    corners = [(1.0, 1.0), (-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0)]
    cams[AT_INFINITY], pix[AT_INFINITY] = list(range(CAM_INFINITY, CAM_INFINITY + 6)), [(d[0] / d[2], d[1] / d[2])] * 6
    cams[DIAGONAL_2], pix[DIAGONAL_2] = [CAM_DIAGONAL_2] * 4, corners
    cams[DIAGONAL_3], pix[DIAGONAL_3] = [CAM_DIAGONAL_3] * 4, corners
    cams[NAN_P][1] = CAM_NAN
    pix[NAN_PIXEL][1] = (pix[NAN_PIXEL][1][0], np.nan)
    pix[INF_PIXEL][0] = (np.inf, pix[INF_PIXEL][0][1])
    off = np.concatenate([[0], np.cumsum([len(c) for c in cams])]).astype(np.uint64)
    cam = np.array([c for cs in cams for c in cs], np.uint32)
    xy = np.array([p for ps in pix for p in ps], np.float64).reshape(-1, 2)
    return _pack(P, off, cam, xy, np.delete(X, SPECIAL, axis=0), centre=Cs[CAM_ONE])


def ordinary():
    """the contract batch's points that are not special"""
    return [i for i in range(CONTRACT_POINTS) if i not in SPECIAL]


BUILDERS = {"origin": _origin, "shift_1e3": lambda: _origin(1e3 * SHIFT), "shift_1e5": lambda: _origin(1e5 * SHIFT),
            "scaled_P": _scaled_P, "edges": _edges, "lds_edge": _lds_edge, "long_list": _long_list, "contract": _contract}
ACCURACY = ("origin", "shift_1e3", "shift_1e5", "scaled_P", "edges", "lds_edge", "long_list", "contract")


def build(name):
    """the case from its seed: dict(P, off, cam, xy, extent[, centre])"""
    return BUILDERS[name]()


def load():
    """every case with its stored truth: name -> dict(P, off, cam, xy, extent, truth[, centre])"""
    with np.load(GOLDEN) as z:
        names = sorted({k.split("__")[0] for k in z.files})
        return {n: {k.split("__")[1]: z[k] for k in z.files if k.split("__")[0] == n} for n in names}


# ---- CSR surgery ---------------------------------------------------------------------------------------------------------
def select(c, points):
    """(off, cam, xy) of the given points in the given order"""
    off = c["off"].astype(np.int64)
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in points] + [np.zeros(0, np.int64)]).astype(np.int64)
    new = np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in points])]).astype(np.uint64)
    return new, np.ascontiguousarray(c["cam"][idx]), np.ascontiguousarray(c["xy"][idx])


def prefix(c, n):
    end = int(c["off"][n])
    return c["off"][:n + 1].copy(), c["cam"][:end].copy(), c["xy"][:end].copy()


# ---- the reference and the yardsticks ------------------------------------------------------------------------------------
def truth(M, counts=None):
    """-> T [n, 3]: per M the eigenvector of the eigenvalue of smallest magnitude at 60 digits, dehomogenised and rounded
    to double.  NaN where M is not finite or the point has at most two observations; a last component of exactly zero
    gives the infinities of the first three's signs."""
    import mpmath
    from mpmath import mp
    T = np.full((len(M), 3), np.nan)
    with mp.workdps(DPS):
        for i, m in enumerate(M):
            if (counts is not None and counts[i] <= 2) or not np.isfinite(m).all():
                continue
            E, Q = mpmath.eigsy(mp.matrix([[mp.mpf(float(x)) for x in row] for row in m]))
            k = min(range(4), key=lambda j: abs(E[j]))
            v = [Q[j, k] for j in range(4)]
            if v[3] == 0:
                T[i] = [math.copysign(math.inf, float(x)) if x != 0 else math.nan for x in v[:3]]
            else:
                T[i] = [float(x / v[3]) for x in v[:3]]
    return T


def matrices(c, points=None):
    """(M, counts) of the case, or of some of its points in their order"""
    off, cam, xy = (c["off"], c["cam"], c["xy"]) if points is None else select(c, points)
    return TM.normal_matrices(c["P"], off, cam, xy), np.diff(off.astype(np.int64))


def judged(c, points=None):
    """the points an accuracy figure runs over: more than two observations and a finite truth"""
    T = c["truth"] if points is None else c["truth"][points]
    return np.isfinite(T).all(axis=1)


def error(X, c, points=None):
    """e_x of the positions X (of all points, or of `points`): the largest distance to the truth over the judged points,
    as a fraction of the extent.  A position that is not finite there gives inf."""
    T = c["truth"] if points is None else c["truth"][points]
    j = judged(c, points)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(((X[j] - T[j]) ** 2).sum(axis=1))
    d[~np.isfinite(d)] = np.inf
    return float(d.max() / c["extent"])


def yardsticks(c, points=None):
    """-> (e_svd, e_eigh, bound) over the case's points or some of them"""
    M, counts = matrices(c, points)
    T = c["truth"] if points is None else c["truth"][points]
    e_svd, e_eigh = error(TM.solve_svd(M, counts)[0], c, points), error(TM.solve_eigh(M, counts)[0], c, points)
    reach = float(np.sqrt((T[judged(c, points)] ** 2).sum(axis=1)).max() / c["extent"])
    return e_svd, e_eigh, max(4 * min(e_svd, e_eigh), 4 * EPS * max(1.0, reach))


def make():
    out = {}
    for name in BUILDERS:
        c = build(name)
        c["truth"] = truth(*matrices(c))
        for k, v in c.items():
            out[f"{name}__{k}"] = v
        e_svd, e_eigh, bound = yardsticks(c)
        print(f"{name}: {len(c['off']) - 1} points, {len(c['cam'])} observations, {int(judged(c).sum())} judged; "
              f"e_svd {e_svd:.3g}, e_eigh {e_eigh:.3g}, bound {bound:.3g}")
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    make()
