"""Hand-built scenes for the epipolar-band culling of phase A, the geometry make_scene's ring never reaches:
views of different size and intrinsics, principal points off the image centre, segments far outside their image and beyond
the pole line of the tau parametrisation, degenerate segments, empty and zero-width quantisation spans, a rectified pair,
views that share a centre, the class cuts of the three layouts, the 64-bit key path, and a pair without kPairFastMath.

scene(name) builds a case (cached, never modified); condition(name) asserts on the host model (tests/cull_model.py) that the
case reaches what it is named for and returns what it found.  tests/test_cull_cases.py runs every condition on the CPU;
tests/test_gpu_cull.py runs the scenes."""
import functools

import numpy as np

from line3dpp_amd.scene import Scene, ViewData, _lookat, _scene_lines
from tests import cull_model as CM

EPI = 1e-6          # overlap threshold of the soundness claim: every match with any overlap at all
KNN = 10


# ---- cameras and segments ------------------------------------------------------------------------------------------------------
def _K(fx, fy, ppx, ppy):
    return np.array([[fx, 0.0, ppx], [0.0, fy, ppy], [0.0, 0.0, 1.0]])


def _pose(C, target=(0.0, 0.0, 0.0), roll_deg=0.0):
    C = np.asarray(C, np.float64)
    a = np.deg2rad(roll_deg)
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    R = Rz @ _lookat(C, np.asarray(target, np.float64))
    return R, -R @ C


def _ring(phi_deg, radius=30.0, z=1.0):
    p = np.deg2rad(phi_deg)
    return np.array([radius * np.cos(p), radius * np.sin(p), z])


@functools.lru_cache(maxsize=None)
def _world(S=1500, seed=5):
    return _scene_lines(np.random.default_rng(seed), S)


def _clutter(rng, n, w, h, outside):
    out = np.zeros((0, 4))
    lim = np.array([-outside * w, -outside * h, (1 + outside) * w, (1 + outside) * h])
    while len(out) < n:
        x = _clutter_draw(rng, 2 * (n - len(out)) + 8, w, h, outside)
        pts = x.reshape(-1, 2)
        ok = ((pts >= lim[:2]) & (pts <= lim[2:])).all(1).reshape(-1, 2).all(1)
        out = np.concatenate([out, x[ok]], 0)
    return out[:n]


def _clutter_draw(rng, n, w, h, outside):
    c = np.stack([rng.uniform(-outside * w, (1 + outside) * w, n), rng.uniform(-outside * h, (1 + outside) * h, n)], 1)
    length = np.clip(np.exp(rng.normal(np.log(0.03 * max(w, h)), 0.7, n)), 0.006 * max(w, h), 0.6 * max(w, h))
    ang = rng.uniform(0, np.pi, n)
    hv = 0.5 * length[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    flip = np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None]
    return np.concatenate([c - flip * hv, c + flip * hv], 1)


def _observe(K, R, t, w, h, n, rng, outside=0.0, real_fraction=0.6, world=None, integer=False):
    """n segments of a view: the world's 3D segments in front of the camera whose end points fall within `outside` image
    sizes of the image, noise, and clutter up to n"""
    P, Q, N = world if world is not None else _world()
    C = -R.T @ t
    facing = ((C[None, :] - P) * N).sum(1) > 0.5
    Xp, Xq = (R @ P.T).T + t, (R @ Q.T).T + t
    front = (Xp[:, 2] > 1.0) & (Xq[:, 2] > 1.0) & facing
    xp, xq = (K @ Xp[front].T).T, (K @ Xq[front].T).T
    p2, q2 = xp[:, :2] / xp[:, 2:3], xq[:, :2] / xq[:, 2:3]
    lo, hi = np.array([-outside * w, -outside * h]), np.array([(1 + outside) * w, (1 + outside) * h])
    ok = ((p2 >= lo) & (p2 <= hi) & (q2 >= lo) & (q2 <= hi)).all(1) & (np.hypot(*(p2 - q2).T) >= 0.006 * max(w, h))
    real = np.concatenate([p2, q2], 1)[ok]
    # (which of the visible 3D segments a view keeps is decided by ONE ranking of the world, so that views share them)
    rank = np.random.default_rng(1234).permutation(len(P))[np.nonzero(front)[0][ok]]
    real = real[np.argsort(rank)[:int(n * real_fraction)]]
    real = real + rng.normal(0, 0.4, real.shape)
    segs = np.concatenate([real, _clutter(rng, n - len(real), w, h, outside)], 0)
    return (np.rint(segs) if integer else segs).astype(np.float32)


def _view(cam, K, R, t, w, h, segs, neighbors):
    return ViewData(cam, np.ascontiguousarray(segs, np.float32).reshape(-1, 4), K.copy(), R.copy(), t.copy(), int(w), int(h),
                    float(np.linalg.norm(R.T @ t)), sorted(int(x) for x in neighbors))


def reversed_scene(sc, name):
    """the same views with their camera IDs in the opposite order: matchImages visits every pair in the other direction"""
    n = len(sc.views)
    views = [ViewData(n - 1 - v.cam, v.segs, v.K, v.R, v.t, v.width, v.height, v.median_depth, sorted(n - 1 - x for x in v.neighbors))
             for v in sc.views]
    return Scene(sorted(views, key=lambda v: v.cam), name)


def pair_list(sc):
    return sc.pair_tests()[1]


def views_of(sc):
    return {v.cam: v for v in sc.views}


# ---- the model of one directed pair ----------------------------------------------------------------------------------------------
def model_pair(sc, s, t, fm=None):
    """every stage of the model for the pair of cameras (s, t); fm: forms to use instead of the model's own (the dumped ones)"""
    V = views_of(sc)
    own, reason, detail = CM.pair_forms(V[s], V[t])
    fm = own if fm is None else fm
    out = dict(forms=fm, reason=reason, detail=detail, enabled=fm is not None)
    if fm is not None:
        out["src"] = CM.src_bands(fm, V[s].segs)
        out["span"] = CM.src_span(out["src"][0], out["src"][1])
        out["tgt"] = CM.tgt_bands(fm, V[t].segs, out["span"])
    return out


def _den_point(B, near, target, below):
    """a float32 point whose denominator B.x lies next to `target`, on the side of MIN_DEN asked for: `near` is moved along
    the gradient of B onto the line B.x == target, then 4 096 points along that line (0.1 px apart: each rounds to float32 in
    its own way) are tried and the closest one is taken"""
    g = np.array([B[0], B[1]])
    near = np.asarray(near, np.float64)
    p = near + (target - (g @ near + B[2])) / (g @ g) * g
    tangent = np.array([-g[1], g[0]]) / np.hypot(*g)
    P = (p[None, :] + 0.1 * np.arange(4096)[:, None] * tangent[None, :]).astype(np.float32).astype(np.float64)
    den = B[0] * P[:, 0] + B[1] * P[:, 1] + B[2]
    side = (den < CM.MIN_DEN) if below else (den > CM.MIN_DEN)
    err = np.where(side, np.abs(den - target), np.inf)
    i = int(np.argmin(err))
    assert err[i] < 0.25e-6 * CM.MIN_DEN, err[i]
    return P[i].astype(np.float32)


# ---- mixed_cameras -----------------------------------------------------------------------------------------------------------------
MIXED = (  # width, height, fx, fy, principal point as a fraction of the size, roll, ring angle, segments
    (960, 720, 900.0, 780.0, (0.62, 0.38), 30.0, 0.0, 420),
    (4000, 3000, 3600.0, 3720.0, (0.37, 0.60), -20.0, 38.0, 560),
    (1600, 1200, 1500.0, 1380.0, (0.65, 0.40), 75.0, 80.0, 500),
)


def _mixed_views(extra=None, outside=0.0, seed=21):
    rng = np.random.default_rng(seed)
    views = []
    for i, (w, h, fx, fy, pp, roll, phi, n) in enumerate(MIXED):
        K = _K(fx, fy, pp[0] * w, pp[1] * h)
        R, t = _pose(_ring(phi, z=1.0 + i), roll_deg=roll)
        segs = _observe(K, R, t, w, h, n, rng, outside=outside)
        if extra is not None:
            segs = np.concatenate([segs, np.asarray(extra, np.float32).reshape(1, 4)], 0)
        views.append(_view(i, K, R, t, w, h, segs, [j for j in range(len(MIXED)) if j != i]))
    return views


def _mixed_cameras():
    return Scene(_mixed_views(), "mixed_cameras")


def _cond_mixed(sc):
    V = sc.views
    assert len({(v.width, v.height) for v in V}) == len(V) and all(max(v.width, v.height) >= 800 for v in V)
    for v in V:
        assert v.K[0, 0] != v.K[1, 1]                                                         # non-square pixels
        off = np.abs(np.array([v.K[0, 2] / v.width, v.K[1, 2] / v.height]) - 0.5)
        assert (off >= 0.10 - 1e-12).all() and (off <= 0.15 + 1e-12).all(), off               # principal point 10-15 % off centre
    n = 0
    for s, t in pair_list(sc):
        assert model_pair(sc, s, t)["enabled"], (s, t)
        n += 1
    assert n == 3
    return dict(pairs=n)


# ---- epipole_sweep -----------------------------------------------------------------------------------------------------------------
SWEEP_W, SWEEP_H, SWEEP_F = 3072, 2304, 2400.0
_SWEEP_A, _SWEEP_B0, _SWEEP_B1 = np.array([30.0, 0.0, 0.0]), np.array([18.0, -24.0, 2.0]), np.array([50.0, 0.0, 0.0])


def sweep_cameras(s, swap):
    """camera A looks at the origin; camera B, turned as at the start of the sweep, moves from B0 (s = 0) onto A's optical
    axis behind A (s = 1), where the epipole in A's image reaches the principal point.  A is the source and B the target: the
    target-side form Bt is the one that fails first.  swap: B is the source, A the target, and the source-side form Bs fails."""
    K = _K(SWEEP_F, SWEEP_F, SWEEP_W / 2, SWEEP_H / 2)
    Ra, ta = _pose(_SWEEP_A)
    Rb, _ = _pose(_SWEEP_B0)
    Cb = _SWEEP_B0 + s * (_SWEEP_B1 - _SWEEP_B0)
    a, b = (K, Ra, ta), (K, Rb, -Rb @ Cb)
    return (b, a) if swap else (a, b)


class _Cam:
    def __init__(self, K, R, t):
        self.K, self.R, self.t, self.width, self.height = K, R, t, SWEEP_W, SWEEP_H


def sweep_forms(s, swap):
    a, b = sweep_cameras(s, swap)
    return CM.pair_forms(_Cam(*a), _Cam(*b))


@functools.lru_cache(maxsize=None)
def sweep_flip(swap):
    """(last culled s, first refused s) by bisection in the model, 2^-22 of the sweep apart"""
    lo, hi = 0.0, 1.0
    assert sweep_forms(lo, swap)[0] is not None and sweep_forms(hi, swap)[0] is None
    for _ in range(22):
        mid = 0.5 * (lo + hi)
        if sweep_forms(mid, swap)[0] is not None:
            lo = mid
        else:
            hi = mid
    return lo, hi


def _sweep_scene(swap, refused):
    name = f"epipole_sweep_{'src' if swap else 'tgt'}_{'refused' if refused else 'culled'}"
    s = sweep_flip(swap)[int(refused)]
    rng = np.random.default_rng(33)
    views = []
    for i, (K, R, t) in enumerate(sweep_cameras(s, swap)):
        views.append(_view(i, K, R, t, SWEEP_W, SWEEP_H, _observe(K, R, t, SWEEP_W, SWEEP_H, 450, rng), [1 - i]))
    return Scene(views, name)


def _cond_sweep(swap, refused):
    def cond(sc):
        m = model_pair(sc, 0, 1)
        assert m["enabled"] == (not refused)
        d = m["detail"]
        limit, other = ("min_Bs", "min_Bt") if swap else ("min_Bt", "min_Bs")
        # the form that decides sits within 1e-5 of the limit on the case's side of it, the other one is far from it
        assert 1e-8 < abs(d[limit] / CM.OK_MIN - 1.0) < 1e-5 and (d[limit] < CM.OK_MIN) == refused, d
        assert d[other] > 2 * CM.OK_MIN, d
        if refused:
            assert m["reason"] == ("source_denominator" if swap else "target_denominator")   # (source: ok(Bt) holds, ok(Bs) fails)
        return dict(s=sweep_flip(swap)[int(refused)], margin=d[limit] / CM.OK_MIN - 1.0)
    return cond


# ---- outside_segments --------------------------------------------------------------------------------------------------------------
OUTSIDE = 1.5


def _outside_cameras():
    cams = []
    for i, (w, h, fx, fy, pp, roll, phi) in enumerate(((960, 720, 820.0, 760.0, (0.55, 0.45), 30.0, 0.0),
                                                       (4000, 3000, 3300.0, 3450.0, (0.46, 0.56), 0.0, 84.0),
                                                       (1600, 1200, 700.0, 730.0, (0.52, 0.47), -15.0, 41.0))):
        R, t = _pose(_ring(phi, z=14.0 + 2 * i), roll_deg=roll)       # (from above: all three see the roof)
        cams.append((_K(fx, fy, pp[0] * w, pp[1] * h), R, t, w, h))
    return cams


def _special_outside(B, w, h, rng):
    """the four kinds of segment of the case for one view, from the form B (B.centre == 1) whose denominator decides the
    view's bands: one end point just below and just above MIN_DEN, end points on both sides of the pole line B.x == 0, a
    whole segment beyond it"""
    c = np.array([0.5 * w, 0.5 * h])
    g = np.array([B[0], B[1]])
    at = lambda den, side=0.0: c + (den - 1.0) / (g @ g) * g + side * np.array([-g[1], g[0]]) / np.hypot(*g)
    inside = lambda: np.array([rng.uniform(0.2 * w, 0.8 * w), rng.uniform(0.2 * h, 0.8 * h)])
    out = []
    for k in range(3):
        out.append(np.concatenate([inside(), _den_point(B, at(CM.MIN_DEN, 40.0 * k), CM.MIN_DEN * (1 - 1e-6), True)]))
        out.append(np.concatenate([_den_point(B, at(CM.MIN_DEN, -55.0 * k - 20.0), CM.MIN_DEN * (1 + 1e-6), False), inside()]))
        out.append(np.concatenate([inside(), at(-0.15 - 0.05 * k, 100.0 * (k - 1))]))                 # across the pole line
        out.append(np.concatenate([at(-0.1, 150.0 * k), at(-0.3, 150.0 * k - 200.0)]))                  # wholly beyond it
    segs = np.array(out, np.float32)
    lim = np.array([-OUTSIDE * w, -OUTSIDE * h, (1 + OUTSIDE) * w, (1 + OUTSIDE) * h])
    pts = segs.reshape(-1, 2)
    assert (pts >= lim[:2]).all() and (pts <= lim[2:]).all(), "the pole line lies within 1.5 image sizes of the border"
    return segs


def _outside_segments():
    rng = np.random.default_rng(44)
    cams = _outside_cameras()
    # the form whose denominator decides a view's bands: view 0 as the source of pair (0, 1), view 1 as its target, view 2
    # as the target of pair (1, 2)
    fm01, _, _ = CM.pair_forms(_CamWH(*cams[0]), _CamWH(*cams[1]))
    fm12, _, _ = CM.pair_forms(_CamWH(*cams[1]), _CamWH(*cams[2]))
    assert fm01 is not None and fm12 is not None
    views = []
    for i, (K, R, t, w, h) in enumerate(cams):
        segs = _observe(K, R, t, w, h, 560, rng, outside=OUTSIDE, real_fraction=0.8, world=_world(5000, 7))
        B = (fm01[1], fm01[3], fm12[3])[i]
        views.append(_view(i, K, R, t, w, h, np.concatenate([segs, _special_outside(B, w, h, rng)], 0), [j for j in range(3) if j != i]))
    return Scene(views, "outside_segments")


class _CamWH:
    def __init__(self, K, R, t, w, h):
        self.K, self.R, self.t, self.width, self.height = K, R, t, w, h


def _cond_outside(sc):
    V = views_of(sc)
    info = {}
    assert all(model_pair(sc, s, t)["enabled"] for s, t in pair_list(sc)) and len(pair_list(sc)) == 3
    for cam, (s, t), side in ((0, (0, 1), "src"), (1, (0, 1), "tgt"), (2, (1, 2), "tgt")):
        m = model_pair(sc, s, t)
        v, B = V[cam], m["forms"][1 if side == "src" else 3]
        S = v.segs.astype(np.float64)
        d1, d2 = CM._den(B, S[:, 0], S[:, 1]), CM._den(B, S[:, 2], S[:, 3])
        dmin, dmax = np.minimum(d1, d2), np.maximum(d1, d2)
        rel = dmin / CM.MIN_DEN - 1.0
        kinds = dict(just_below=int(((rel < 0) & (rel > -1.5e-6) & (dmax > 0.5)).sum()),
                     just_above=int(((rel > 0) & (rel < 1.5e-6)).sum()),
                     across=int(((dmin < -0.05) & (dmax > 0.5)).sum()), beyond=int((dmax < 0).sum()))
        assert all(n >= 1 for n in kinds.values()), (side, kinds)
        pts = S.reshape(-1, 2)
        reach = max(-(pts[:, 0].min()) / v.width, pts[:, 0].max() / v.width - 1, -(pts[:, 1].min()) / v.height, pts[:, 1].max() / v.height - 1)
        assert 1.0 < reach <= OUTSIDE + 1e-6, reach
        cls = m[side][2]
        # the model's class follows the denominators: just below is unbounded, just above is not (unless the other end is)
        assert (cls[(rel < 0)] == 0).all() and (cls[(rel > 0) & np.isfinite(m[side][0])] != 0).all()
        info[cam] = dict(kinds, unbounded=int((cls == 0).sum()))
    return info


# ---- degenerate_segments -----------------------------------------------------------------------------------------------------------
def _epipoles(F):
    """(right null vector: the epipole in the source image, left null vector: the epipole in the target image), as points"""
    U, _, Vt = np.linalg.svd(F)
    es, et = Vt[2], U[:, 2]
    return es[:2] / es[2], et[:2] / et[2]


def _degenerate_segments():
    rng = np.random.default_rng(55)
    w, h = 3072, 2304
    K = _K(2400.0, 2400.0, w / 2, h / 2)
    cams = [(K,) + _pose(_ring(0.0)), (K,) + _pose(_ring(42.0, z=3.0))]
    F = CM._fundamental(_CamWH(*cams[0], w, h), _CamWH(*cams[1], w, h))
    fm = CM.forms(F, w, h, w, h)
    es, et = _epipoles(F)
    c = np.array([w / 2, h / 2])
    S = [_observe(*cams[0], w, h, 400, rng)]
    T = [_observe(*cams[1], w, h, 400, rng)]
    zero = lambda: np.tile(np.array([rng.uniform(100, w - 100), rng.uniform(100, h - 100)]), 2)
    S.append(np.array([zero() for _ in range(3)])); T.append(np.array([zero() for _ in range(3)]))
    # targets parallel to the transversal: the direction on which Bt vanishes
    par = np.array([-fm[3][1], fm[3][0]]) / np.hypot(fm[3][0], fm[3][1])
    T.append(np.array([np.concatenate([p - 150 * par, p + 150 * par]) for p in (c + [300, 200], c - [500, 100])]))
    # targets collinear with the epipole of the target image
    ray = lambda e, p, a, b: np.concatenate([p + a * (e - p) / np.linalg.norm(e - p), p + b * (e - p) / np.linalg.norm(e - p)])
    T.append(np.array([ray(et, c + [200, -300], -200, 150), ray(et, c - [600, 400], 0, 320)]))
    # source segments that point at the epipole of the source image: a wedge of no width
    S.append(np.array([ray(es, c + [-250, 150], -120, 260), ray(es, c + [400, 500], 0, 200)]))
    # twenty copies of one segment on both sides: equal keys, ordered by element
    S.append(np.tile(S[0][7], (20, 1))); T.append(np.tile(T[0][11], (20, 1)))
    views = [_view(i, *cams[i], w, h, np.concatenate(x, 0), [1 - i]) for i, x in enumerate((S, T))]
    return Scene(views, "degenerate_segments")


def _cond_degenerate(sc):
    m = model_pair(sc, 0, 1)
    assert m["enabled"]
    V = views_of(sc)
    S, T = V[0].segs.astype(np.float64), V[1].segs.astype(np.float64)
    fm = m["forms"]
    zs, zt = (S[:, 0] == S[:, 2]) & (S[:, 1] == S[:, 3]), (T[:, 0] == T[:, 2]) & (T[:, 1] == T[:, 3])
    assert zs.sum() >= 3 and zt.sum() >= 3
    assert (m["tgt"][2][zt] == 0).all(), "a zero-length target has no direction: td is NaN, the band unbounded"
    assert (m["src"][2][zs] == 2).all() and (m["src"][1][zs] - m["src"][0][zs] < 0.03).all(), "a zero-length source row: the pad alone"
    dx, dy = T[:, 2] - T[:, 0], T[:, 3] - T[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        td = (fm[2][0] * dx + fm[2][1] * dy) / (fm[3][0] * dx + fm[3][1] * dy)
    span = m["span"]
    far = np.abs(td) > 1e4 * (float(span[1]) - float(span[0]))
    assert far.sum() >= 2 and (m["tgt"][2][far] == 2).all(), "parallel to the transversal: td = +-inf (or beyond any span), never widened"
    t1 = CM._den(fm[2], T[:, 0], T[:, 1]) / CM._den(fm[3], T[:, 0], T[:, 1])
    t2 = CM._den(fm[2], T[:, 2], T[:, 3]) / CM._den(fm[3], T[:, 2], T[:, 3])
    through = (np.abs(t1 - t2) < 1e-2) & ~zt & (np.hypot(dx, dy) > 100)
    assert through.sum() >= 2, "targets collinear with the epipole: one pencil line"
    s1 = CM._den(fm[0], S[:, 0], S[:, 1]) / CM._den(fm[1], S[:, 0], S[:, 1])
    s2 = CM._den(fm[0], S[:, 2], S[:, 3]) / CM._den(fm[1], S[:, 2], S[:, 3])
    thin = (np.abs(s1 - s2) < 1e-2) & ~zs & (np.hypot(S[:, 2] - S[:, 0], S[:, 3] - S[:, 1]) > 100)
    assert thin.sum() >= 2, "source rows that point at the source epipole: a wedge of zero width"
    for X in (V[0].segs, V[1].segs):
        _, cnt = np.unique(X, axis=0, return_counts=True)
        assert cnt.max() >= 21
    return dict(zero=(int(zs.sum()), int(zt.sum())), parallel=int(far.sum()), inf_td=int(np.isinf(td).sum()), through=int(through.sum()), thin=int(thin.sum()))


# ---- empty_span / single_span -----------------------------------------------------------------------------------------------------
def _span_scene(bounded_rows, name):
    rng = np.random.default_rng(66)
    w, h = 3072, 2304
    K = _K(2400.0, 2400.0, w / 2, h / 2)
    cams = [(K,) + _pose(_ring(0.0)), (K,) + _pose(_ring(80.0, z=2.0))]
    fm, _, _ = CM.pair_forms(_CamWH(*cams[0], w, h), _CamWH(*cams[1], w, h))
    Bs = fm[1]
    c = np.array([w / 2, h / 2]); g = np.array([Bs[0], Bs[1]])
    at = lambda den, side: c + (den - 1.0) / (g @ g) * g + side * np.array([-g[1], g[0]]) / np.hypot(*g)
    # every source row reaches over the pole line of the source form: it starts in the image and ends beyond B.x == MIN_DEN
    S = np.array([np.concatenate([[rng.uniform(0, w), rng.uniform(0, h)], at(rng.uniform(-0.4, 0.04), rng.uniform(-1500, 1500))])
                  for _ in range(200)])
    if bounded_rows:
        S = np.concatenate([S[:117], _observe(*cams[0], w, h, bounded_rows, rng), S[117:]], 0)
    T = _observe(*cams[1], w, h, 420, rng)
    return Scene([_view(0, *cams[0], w, h, S, [1]), _view(1, *cams[1], w, h, T, [0])], name)


def _cond_span(bounded_rows):
    def cond(sc):
        m = model_pair(sc, 0, 1)
        assert m["enabled"]
        cls = m["src"][2]
        assert int((cls != 0).sum()) == bounded_rows
        if bounded_rows == 0:
            assert m["span"] is None and (m["tgt"][2] != 1).all(), "no bounded row: nothing can be widened"
        else:
            lo = m["src"][0][cls != 0]
            assert CM.quant_step(lo.min(), lo.max(), len(cls)) == 0.0, "one bounded start: a span of zero width, scale 0"
            assert m["span"][1] > m["span"][0]
        return dict(unbounded=int((cls == 0).sum()))
    return cond


# ---- rectified ---------------------------------------------------------------------------------------------------------------------
def _rectified():
    rng = np.random.default_rng(77)
    w, h = 1600, 1200
    K = _K(1400.0, 1400.0, 800.0, 600.0)
    R = EXACT_R
    views = []
    for i, C in enumerate((np.array([-2.0, -30.0, 1.0]), np.array([2.0, -30.0, 1.0]))):   # a sideways baseline of 4
        t = -R @ C
        segs = _observe(K, R, t, w, h, 430, rng, integer=True)
        y = rng.integers(50, h - 50, 40).astype(np.float64); x = rng.integers(50, w - 400, 40).astype(np.float64)
        horiz = np.stack([x, y, x + rng.integers(60, 350, 40), y], 1)                     # horizontal: parallel to every epipolar line
        x = rng.integers(50, w - 50, 30).astype(np.float64); y = rng.integers(50, h - 400, 30).astype(np.float64)
        vert = np.stack([x, y, x, y + rng.integers(60, 350, 30)], 1)                      # vertical: parallel to the transversal
        segs = np.concatenate([segs, horiz, vert], 0)
        segs = segs[(segs[:, 0] != segs[:, 2]) | (segs[:, 1] != segs[:, 3])]
        views.append(_view(i, K, R, t, w, h, segs, [1 - i]))
    return Scene(views, "rectified")


def _cond_rectified(sc):
    V = views_of(sc)
    F = CM._fundamental(V[0], V[1])
    assert F[0, 0] == 0 and F[0, 1] == 0 and F[0, 2] == 0 and F[1, 0] == 0 and F[2, 0] == 0 and F[1, 1] == 0, F
    m = model_pair(sc, 0, 1)
    assert m["enabled"]
    fm = m["forms"]
    assert fm[3][0] == 0 and fm[3][1] == 0 and fm[1][0] == 0 and fm[1][1] == 0, "the epipole at infinity: both denominators constant"
    assert all((v.segs == np.rint(v.segs)).all() for v in sc.views)
    T = V[1].segs.astype(np.float64)
    dx, dy = T[:, 2] - T[:, 0], T[:, 3] - T[:, 1]
    assert ((dy == 0).sum() >= 40) and ((dx == 0).sum() >= 30)
    lo = m["tgt"][0]
    _, cnt = np.unique(lo, return_counts=True)
    assert (cnt > 1).sum() >= 20, "integer rows: many equal band starts"
    with np.errstate(divide="ignore", invalid="ignore"):
        td = (fm[2][0] * dx + fm[2][1] * dy) / (fm[3][0] * dx + fm[3][1] * dy)
    # Bt vanishes on every direction: td = +-inf and no target is widened -- but for a horizontal one At.d vanishes as well,
    # td = 0 / 0 = NaN, and its band is unbounded
    assert (np.isinf(td) | (dy == 0)).all() and np.isnan(td[dy == 0]).all()
    assert (m["tgt"][2][dy == 0] == 0).all() and (m["tgt"][2][dy != 0] == 2).all()
    return dict(equal_starts=int((cnt > 1).sum()), horizontal=int((dy == 0).sum()), vertical=int((dx == 0).sum()))


# ---- no_baseline -------------------------------------------------------------------------------------------------------------------
EXACT_R = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])   # looks along +y, image x to the right, image y down


def _no_baseline():
    """views 0 and 1: one centre and one (exactly representable) rotation, different intrinsics -- t' - R t is exactly 0 and so
    is F; view 2: 1e-9 away from them; view 3: the centre of view 2 under another rotation -- F is what the rounding of
    t' - R t leaves, about 1e-15"""
    rng = np.random.default_rng(88)
    w, h = 3072, 2304
    C = np.array([3.0, -30.0, 1.0])
    C2 = C + 1e-9 * np.array([1.0, 0.05, 0.1])       # (sideways: the epipole of a pair with view 0 or 1 lies far outside)
    R2, t2 = _pose(C2, target=(1.0, -2.0, 0.0))
    R3, t3 = _pose(C2, target=(-2.0, 1.0, 1.0), roll_deg=8.0)
    cams = [(_K(2400.0, 2400.0, w / 2, h / 2), EXACT_R, -EXACT_R @ C), (_K(2000.0, 2100.0, 0.45 * w, 0.55 * h), EXACT_R, -EXACT_R @ C),
            (_K(2400.0, 2400.0, w / 2, h / 2), R2, t2), (_K(2200.0, 2200.0, w / 2, h / 2), R3, t3)]
    views = [_view(i, K, R, t, w, h, _observe(K, R, t, w, h, 350, rng), [j for j in range(4) if j != i]) for i, (K, R, t) in enumerate(cams)]
    return Scene(views, "no_baseline")


def _cond_no_baseline(sc):
    V = views_of(sc)
    assert not CM._fundamental(V[0], V[1]).any() and model_pair(sc, 0, 1)["reason"] == "F_zero_or_not_finite"
    assert 0 < np.linalg.norm(V[0].R.T @ V[0].t - V[2].R.T @ V[2].t) < 2e-9
    F23 = CM._fundamental(V[2], V[3])
    assert 0 < np.abs(F23).max() < 1e-12, "one centre under two rotations: F is the rounding of t' - R t"
    return dict(F23=float(np.abs(F23).max()), reasons=[model_pair(sc, s, t)["reason"] for s, t in pair_list(sc)])


# ---- class_edges -------------------------------------------------------------------------------------------------------------------
CLASS_MS = (383, 384, 767, 768, 1535, 1536, 3071, 3072)     # Ms / 16 one below and at 24, 48, 192; Ms / 64 one below and at 24, 48
CLASS_MT = 300
CLASS_BINS = (0.17, 0.19, 0.23)                             # share of the bounded rows beyond 1/16, 1/32, 1/64 of (w + h) / 2
CLASS_UNBOUNDED = 21


def _stored_width(fm, seg):
    lo, hi, _ = CM.src_bands(fm, np.asarray(seg, np.float32).reshape(1, 4))
    return np.float32(hi[0] - lo[0])


def _row_of_width(fm, rng, w, h, lo_w, hi_w, edge=None):
    """a source segment inside the image whose STORED band is lo_w < width <= hi_w wide; edge = (cut, above): the width lies
    next to `cut` on the side asked for (the length is bisected until two float32 segments straddle the cut)"""
    while True:
        mid = np.array([rng.uniform(0.25 * w, 0.75 * w), rng.uniform(0.25 * h, 0.75 * h)])
        a = rng.uniform(0, np.pi)
        d = np.array([np.cos(a), np.sin(a)])
        seg = lambda L: np.concatenate([mid - 0.5 * L * d, mid + 0.5 * L * d]).astype(np.float32)
        if edge is None:                                  # (the width grows almost linearly with the length)
            want = np.exp(rng.uniform(np.log(max(float(lo_w), 6.0)), np.log(min(float(hi_w), 500.0))))
            w100 = float(_stored_width(fm, seg(100.0)))
            out = seg(100.0 * (want - 0.02) / max(w100 - 0.02, 1e-3))
        else:
            L0, L1 = 0.0, 0.45 * min(w, h)
            if not (_stored_width(fm, seg(L1)) > edge[0]):
                continue
            for _ in range(50):
                Lm = 0.5 * (L0 + L1)
                if _stored_width(fm, seg(Lm)) > edge[0]:
                    L1 = Lm
                else:
                    L0 = Lm
            out = seg(L1 if edge[1] else L0)
        wd = _stored_width(fm, out)
        if lo_w < wd <= hi_w and 2.0 < np.hypot(out[2] - out[0], out[3] - out[1]) < 0.45 * min(w, h):
            return out


def merged_classes(bins, items):
    """rows per class [5] from the rows per width bin (unbounded, beyond 1/16, 1/32, 1/64, narrow) at `items` = Ms / R: a cut
    that is not made at this size falls together with the next wider one"""
    n0, n1, n2, n3, n4 = bins
    if items < 24:
        return [n0, 0, 0, 0, n1 + n2 + n3 + n4]
    if items < 48:
        return [n0, n1, 0, 0, n2 + n3 + n4]
    if items < 192:
        return [n0, n1, 0, n2 + n3, n4]
    return [n0, n1, n2, n3, n4]


def _bin_counts(Ms):
    """bounded rows per width bin, near CLASS_BINS, such that no class of the layouts with R = 16 and R = 64 is a whole number of items"""
    nb = Ms - CLASS_UNBOUNDED
    base = [int(nb * f) for f in CLASS_BINS]
    for d in np.ndindex(6, 6, 6):
        c = [b + x for b, x in zip(base, d)]
        c.append(nb - sum(c))
        if all(n % R for R in (16, 64) for n in merged_classes([CLASS_UNBOUNDED] + c, Ms // R) if n):
            return c
    raise AssertionError(Ms)


def _class_edges():
    rng = np.random.default_rng(99)
    w, h = 3072, 2304
    K = _K(2400.0, 2400.0, w / 2, h / 2)
    tgt = (K,) + _pose(_ring(40.0, z=2.0))
    n_src = len(CLASS_MS)
    ref = np.float32(0.5 * w + 0.5 * h)
    cuts = [np.float32(np.inf), ref / np.float32(16), ref / np.float32(32), ref / np.float32(64), np.float32(0)]
    views = []
    for i, Ms in enumerate(CLASS_MS):
        src = (K,) + _pose(_ring(-2.0 + 0.5 * i, z=1.0))
        fm, _, _ = CM.pair_forms(_CamWH(*src, w, h), _CamWH(*tgt, w, h))
        Bs = fm[1]
        c = np.array([w / 2, h / 2]); g = np.array([Bs[0], Bs[1]])
        beyond = lambda: c + (rng.uniform(-0.5, 0.0) - 1.0) / (g @ g) * g + rng.uniform(-800, 800) * np.array([-g[1], g[0]]) / np.hypot(*g)
        rows = [np.concatenate([[rng.uniform(0, w), rng.uniform(0, h)], beyond()]).astype(np.float32) for _ in range(CLASS_UNBOUNDED)]
        counts = _bin_counts(Ms)
        for k, n in enumerate(counts):
            for j in range(n):
                edge = None
                if j < 4 and k < 3:
                    edge = (cuts[k + 1], True)            # just beyond the bin's lower cut
                elif j < 8 and k > 0:
                    edge = (cuts[k], False)               # just at or below its upper cut
                rows.append(_row_of_width(fm, rng, w, h, cuts[k + 1], cuts[k], edge))
        rows = np.array(rows, np.float32)
        views.append(_view(i, *src, w, h, rows[rng.permutation(len(rows))], [n_src]))
    views.append(_view(n_src, *tgt, w, h, _observe(*tgt, w, h, CLASS_MT, rng), list(range(n_src))))
    return Scene(views, "class_edges")


def _cond_class_edges(sc):
    V = views_of(sc)
    tv = V[len(CLASS_MS)]
    info = {}
    edges16 = {Ms // 16 for Ms in CLASS_MS}
    assert {23, 24, 47, 48, 191, 192} <= edges16 and {23, 24, 47, 48} <= {Ms // 64 for Ms in CLASS_MS}
    for (s, t), Ms in zip(pair_list(sc), CLASS_MS):
        assert len(V[s].segs) == Ms and t == len(CLASS_MS)
        m = model_pair(sc, s, t)
        assert m["enabled"]
        lo, hi, _ = m["src"]
        ref = np.float32(0.5 * tv.width + 0.5 * tv.height)
        wd = (hi - lo)[np.isfinite(lo)]
        for cut in (ref / np.float32(16), ref / np.float32(32), ref / np.float32(64)):
            assert ((wd > cut) & (wd < cut * np.float32(1.0001))).sum() >= 2 and ((wd <= cut) & (wd > cut * np.float32(0.9999))).sum() >= 2, (Ms, cut)
        for R in (16, 64):
            cls = CM.src_classes(lo, hi, Ms, R, tv.width, tv.height)
            counts = np.bincount(cls, minlength=5)
            items = Ms // R
            populated = 2 if items < 24 else 3 if items < 48 else 4 if items < 192 else 5
            assert (counts > 0).sum() == populated and (counts[counts > 0] % R != 0).all(), (Ms, R, counts)
            cap, base = CM.layout(counts, Ms, R)
            if populated == 5:   # the worst case tile_src_cap's c (R - 1) term reserves room for: five partial items
                assert base[-1] > Ms + 4 * (R - 1) - R
            info[(Ms, R)] = dict(counts=counts.tolist(), used=int(base[-1]), cap=cap)
    return info


# ---- big_keys ----------------------------------------------------------------------------------------------------------------------
def _big(n_big, name):
    rng = np.random.default_rng(111)
    w, h = 3072, 2304
    K = _K(2400.0, 2400.0, w / 2, h / 2)
    world = _world(24000, 6)
    cams = [(K,) + _pose(_ring(0.0)), (K,) + _pose(_ring(35.0, z=2.0))]
    views = [_view(0, *cams[0], w, h, _observe(*cams[0], w, h, 300, rng, world=world), [1]),
             _view(1, *cams[1], w, h, _observe(*cams[1], w, h, n_big, rng, world=world), [0])]
    return Scene(views, name)


def _cond_big(n_big):
    def cond(sc):
        sizes = sorted(len(v.segs) for v in sc.views)
        assert sizes == [300, n_big]
        assert model_pair(sc, *pair_list(sc)[0])["enabled"]
        assert CM.big_keys(*sizes) == (n_big > CM.LDS_SEGS) and CM.band_cache(n_big) == (n_big <= CM.BAND_CACHE_SEGS)
        return dict(big_keys=CM.big_keys(*sizes), band_cache=CM.band_cache(n_big), pair_tests=sizes[0] * sizes[1])
    return cond


# ---- slow_arithmetic ---------------------------------------------------------------------------------------------------------------
FAR = (2.0e7, 350.0, 2.0e7 + 400.0, 120.0)


def _slow_arithmetic():
    return Scene(_mixed_views(extra=FAR), "slow_arithmetic")


def _cond_slow(sc):
    base = scene("mixed_cameras")
    for v, b in zip(sc.views, base.views):
        assert np.array_equal(v.segs[:-1], b.segs) and np.abs(v.segs[-1]).max() == 2e7 + 400 and np.abs(v.segs).max() > 1e7
    return dict(coord_max=float(max(np.abs(v.segs).max() for v in sc.views)))


# ---- registry ----------------------------------------------------------------------------------------------------------------------
def _rev(name, cond=None):
    return (lambda: reversed_scene(scene(name), name + "_rev")), (cond or (lambda sc: dict(pairs=len(pair_list(sc)))))


CASES = {
    "mixed_cameras": (_mixed_cameras, _cond_mixed),
    "mixed_cameras_rev": _rev("mixed_cameras"),
    "epipole_sweep_tgt_culled": (lambda: _sweep_scene(False, False), _cond_sweep(False, False)),
    "epipole_sweep_tgt_refused": (lambda: _sweep_scene(False, True), _cond_sweep(False, True)),
    "epipole_sweep_src_culled": (lambda: _sweep_scene(True, False), _cond_sweep(True, False)),
    "epipole_sweep_src_refused": (lambda: _sweep_scene(True, True), _cond_sweep(True, True)),
    "outside_segments": (_outside_segments, _cond_outside),
    "outside_segments_rev": _rev("outside_segments"),
    "degenerate_segments": (_degenerate_segments, _cond_degenerate),
    "empty_span": (lambda: _span_scene(0, "empty_span"), _cond_span(0)),
    "single_span": (lambda: _span_scene(1, "single_span"), _cond_span(1)),
    "rectified": (_rectified, _cond_rectified),
    "no_baseline": (_no_baseline, _cond_no_baseline),
    "class_edges": (_class_edges, _cond_class_edges),
    "big_keys_4096": (lambda: _big(4096, "big_keys_4096"), _cond_big(4096)),
    "big_keys_4096_rev": _rev("big_keys_4096"),
    "big_keys_4097": (lambda: _big(4097, "big_keys_4097"), _cond_big(4097)),
    "big_keys_4097_rev": _rev("big_keys_4097"),
    "big_keys_16385": (lambda: _big(16385, "big_keys_16385"), _cond_big(16385)),
    "big_keys_16385_rev": _rev("big_keys_16385"),
    "slow_arithmetic": (_slow_arithmetic, _cond_slow),
}
# the model's decision is not asked of these: the baseline of 1e-9 leaves F to the rounding of t - R t'
DECISION_FREE = ("no_baseline",)


@functools.lru_cache(maxsize=None)
def scene(name):
    return CASES[name][0]()


def condition(name):
    return CASES[name][1](scene(name))


@functools.lru_cache(maxsize=None)
def oracle_pairs(name, kNN, epi=EPI):
    """the oracle's matches of every directed pair of a case, computed once and shared, never modified"""
    from oracle.oracle import Oracle
    sc = scene(name)
    o = Oracle(threads=16)
    o.add_scene(sc)
    o.begin_match(kNN=kNN, epi_overlap=epi)
    out = [o.match_pair(s, t)[0] for s, t in pair_list(sc)]
    o.end_match()
    return out
