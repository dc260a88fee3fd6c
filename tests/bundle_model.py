"""The contract of DESIGN §29 (cameras and 3D lines bundled jointly) restated in numpy from the text: the frame about the
model's centre, the cells of the observation list, eligibility and the free cameras, the residual with its ten columns, the
67 sums of a cell, the lines' 4 x 4 factors, the Schur complement with the wave tree of k_bundle_reduce, the dense Cholesky
solve, the update, the cost with its tile tree, the step control, the cameras' hand-out and §28's spans and sweep.  The
association comes from tests/refit_model.py, the pose state from tests/pose_model.py.  numpy's element-wise float64
operations round every operation on its own, as the library does when built with -ffp-contract=off; sums are written out
in the order of the text.

`bundle` runs a whole call; it can be handed the library's own associations and dense solve (`assoc`, `solve`), so that
tests/test_gpu_bundle.py pins everything behind them bit for bit."""
import math

import numpy as np

from tests import associate_model as AM
from tests import pose_model as PO
from tests import refit_model as RM

LINE_DTYPE = np.dtype([("status", "<u4"), ("n_observations", "<u4"), ("n_views", "<u4"), ("n_pieces", "<u4"), ("P1", "<f8", 3),
                       ("P2", "<f8", 3)])
ITERATION_DTYPE = np.dtype([("damping", "<f8"), ("cost", "<f8"), ("cost_trial", "<f8"), ("step_cameras", "<f8"),
                            ("step_lines", "<f8"), ("solved", "<u4"), ("accepted", "<u4"), ("n_held_for_step", "<u4"), ("pad", "<u4")])
LINE_STATUS = ("BUNDLED", "HELD", "NO_EXTENT", "EMPTY")
BUNDLED, HELD, NO_EXTENT, EMPTY = range(4)
STATUS = ("CONVERGED", "MAX_ITERATIONS", "STALLED", "NO_VARIABLES")
CC, BC, CL, LL, BL, RHO, COUNT, CELL = 0, 21, 27, 51, 61, 65, 66, 67
ROW6 = (0, 6, 11, 15, 18, 20)                    # where row i of the upper triangle of 6 x 6 begins
ROW4 = (0, 4, 7, 9)
MAX_FREE = 512
DEFAULTS = dict(max_distance=2.5, min_cos2=AM.min_cos2_of(10.0), min_overlap=0.5, near_plane=1e-6, min_length=0.0, visibility=3,
                max_iterations=10, use_ambiguous=False, initial_damping=1e-4, min_damping=1e-9, max_damping=1e8,
                function_tolerance=1e-6, capture_iteration=0)


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def mul33(R, v):
    return tuple((R[3 * i] * v[0] + R[3 * i + 1] * v[1]) + R[3 * i + 2] * v[2] for i in range(3))


def kt(M, v):
    """K^-T v"""
    return (M[0] * v[0], M[1] * v[0] + M[2] * v[1], (M[3] * v[0] + M[4] * v[1]) + v[2])


def norm3(c):
    return np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])


def basis(AB):
    """(e1, e2) of carriers AB [n, 6] (or one carrier of 6 floats): u = B - A, k the first index of the smallest |u_k|,
    e1 = (u x e_k) / |.|, e2 = (u x e1) / |.|; each a tuple of three arrays"""
    AB = np.asarray(AB, np.float64).reshape(-1, 6)
    u = tuple(AB[:, 3 + i] - AB[:, i] for i in range(3))
    m1 = np.abs(u[1]) < np.abs(u[0])
    k = np.where(m1, 1, 0); uk = np.where(m1, u[1], u[0])
    k = np.where(np.abs(u[2]) < np.abs(uk), 2, k)
    ek = tuple(np.where(k == i, 1.0, 0.0) for i in range(3))
    with np.errstate(all="ignore"):
        c = cross(u, ek)
        n1 = norm3(c)
        e1 = tuple(v / n1 for v in c)
        f = cross(u, e1)
        n2 = norm3(f)
        e2 = tuple(v / n2 for v in f)
    return e1, e2


def image_line(M, R, t, AB):
    """(Y1, Y2, lam, nu, ok) of carriers AB (six arrays) in cameras (M five, R nine, t three arrays)"""
    Y1 = tuple(v + t[i] for i, v in enumerate(mul33(R, AB[:3])))
    Y2 = tuple(v + t[i] for i, v in enumerate(mul33(R, AB[3:])))
    lam = kt(M, cross(Y1, Y2))
    nu = np.sqrt(lam[0] * lam[0] + lam[1] * lam[1])
    return Y1, Y2, lam, nu, (nu > 0.0) & np.isfinite(nu)


def huber(s):
    """(rho, rho') of lo_huber, element-wise"""
    with np.errstate(all="ignore"):
        r = np.sqrt(s)
        return np.where(s > 4.0, 4.0 * r - 4.0, s), np.where(s > 4.0, 2.0 / r, 1.0)


def columns(M, R, Y1, Y2, e1, e2):
    """the ten columns dN of §29.4: e_i x N, e_i x D, (R e_j) x Y2, Y1 x (R e_j)"""
    N = cross(Y1, Y2)
    D = tuple(Y2[i] - Y1[i] for i in range(3))
    z = np.zeros_like(N[0])
    r1, r2 = mul33(R, e1), mul33(R, e2)
    return [(z, -N[2], N[1]), (N[2], z, -N[0]), (-N[1], N[0], z), (z, -D[2], D[1]), (D[2], z, -D[0]), (-D[1], D[0], z),
            cross(r1, Y2), cross(r2, Y2), cross(Y1, r1), cross(Y1, r2)]


def residuals(M, R, t, AB, e1, e2, p):
    """for arrays of observations (their camera's M, R, t, their line's AB, e1, e2, the 2D end points p four arrays) ->
    (ok, rP, rQ, JP [10], JQ [10]) by §29.4"""
    with np.errstate(all="ignore"):
        Y1, Y2, lam, nu, ok = image_line(M, R, t, AB)
        dN = columns(M, R, Y1, Y2, e1, e2)
        nu3 = (nu * nu) * nu
        dl = [kt(M, c) for c in dN]
        B = [(lam[0] * d[0] + lam[1] * d[1]) / nu3 for d in dl]
        up = (lam[0] * p[0] + lam[1] * p[1]) + lam[2]; uq = (lam[0] * p[2] + lam[1] * p[3]) + lam[2]
        rp, rq = up / nu, uq / nu
        JP = [((d[0] * p[0] + d[1] * p[1]) + d[2]) / nu - up * b for d, b in zip(dl, B)]
        JQ = [((d[0] * p[2] + d[1] * p[3]) + d[2]) / nu - uq * b for d, b in zip(dl, B)]
    return ok, rp, rq, JP, JQ


class Problem:
    """the tables of a call: cells, eligibility, free cameras, the second CSR and the slot table"""


def prepare(segs, line, cams, segs_per_cam, assoc, fixed, par):
    model = np.asarray(segs, np.float64).reshape(-1, 6)
    line = np.asarray(line, np.uint32).reshape(-1)
    c, diag = PO.bounding_box(model)
    assert diag > 0.0
    n_lines, n_cams = int(line.max()) + 1, len(cams)
    seg2d = [np.asarray(s, np.float32).reshape(-1, 4) for s in segs_per_cam]
    flat = [(k, i) for k, a in enumerate(assoc) for i in range(len(a))
            if a["record"][i] >= 0 and (a["n_accepted"][i] == 1 or par["use_ambiguous"])]
    by_line = [[] for _ in range(n_lines)]
    for k, i in flat:
        by_line[int(assoc[k]["line"][i])].append((k, i))          # (stable: ascending flat index)
    P = Problem()
    P.c, P.n_lines, P.n_cams, P.seg2d = c, n_lines, n_cams, seg2d
    P.lines = np.zeros(n_lines, LINE_DTYPE)
    P.obs_rec = np.zeros(len(flat), RM.OBSERVATION_DTYPE)
    P.obs_off = np.zeros(n_lines + 1, np.int64)
    obs_p, obs_cam, obs_line, cell_off, cell_line, cell_cam = [], [], [], [], [], []
    P.line_cell_off = np.zeros(n_lines + 1, np.int64)
    P.AB = np.zeros((n_lines, 6))
    need = max(2, par["visibility"])
    eligible = []
    at = 0
    for l in range(n_lines):
        last = -1
        for k, i in by_line[l]:
            if k != last:
                cell_off.append(at); cell_line.append(l); cell_cam.append(k)
                last = k
            P.obs_rec[at] = (k, i, l, 0, 0.0, 0.0)
            obs_p.append(seg2d[k][i].astype(np.float64)); obs_cam.append(k); obs_line.append(l)
            at += 1
        P.obs_off[l + 1] = at
        P.line_cell_off[l + 1] = len(cell_line)
        L = P.lines[l]
        mine = np.flatnonzero(line == l)
        L["n_observations"] = len(by_line[l]); L["n_views"] = P.line_cell_off[l + 1] - P.line_cell_off[l]
        if not len(mine):
            L["status"] = EMPTY
            continue
        L["status"] = HELD
        L["P1"] = model[mine[0], :3]; L["P2"] = model[mine[-1], 3:]
        q = [float(L["P1"][k]) - c[k] for k in range(3)] + [float(L["P2"][k]) - c[k] for k in range(3)]
        P.AB[l] = q
        u = [q[3 + k] - q[k] for k in range(3)]
        uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
        if L["n_views"] >= need and uu > 0.0 and math.isfinite(uu):
            eligible.append(l)
    cell_off.append(at)
    P.n_obs, P.n_cells = at, len(cell_line)
    P.obs_p = np.array(obs_p, np.float64).reshape(-1, 4); P.obs_cam = np.array(obs_cam, np.int64); P.obs_line = np.array(obs_line, np.int64)
    P.cell_off = np.array(cell_off, np.int64); P.cell_line = np.array(cell_line, np.int64); P.cell_cam = np.array(cell_cam, np.int64)
    P.eligible = np.array(eligible, np.int64)
    P.is_eligible = np.zeros(n_lines, bool); P.is_eligible[P.eligible] = True
    order = np.argsort(P.cell_cam, kind="stable")                   # the second CSR: a stable counting sort by camera
    P.cam_cells = order
    P.cam_cell_off = np.concatenate([[0], np.cumsum(np.bincount(P.cell_cam, minlength=n_cams))]).astype(np.int64)
    P.slot = np.full((n_lines, n_cams), -1, np.int64)
    P.slot[P.cell_line, P.cell_cam] = np.arange(P.n_cells)
    fixed = np.zeros(n_cams, bool) if fixed is None else np.asarray(fixed).astype(bool)
    P.free_cam = np.array([k for k in range(n_cams) if not fixed[k] and P.cam_cell_off[k + 1] > P.cam_cell_off[k]], np.int64)
    P.cam_free = np.full(n_cams, -1, np.int64); P.cam_free[P.free_cam] = np.arange(len(P.free_cam))
    P.M = np.array([PO.inverse_transpose(cam["K"]) for cam in cams], np.float64).reshape(-1, 5)
    return P


def pose_table(cams, states):
    """[n_cams, 12]: R (9) and t' (3) of every camera about the centre"""
    out = np.zeros((len(cams), 12))
    for k, (cam, s) in enumerate(zip(cams, states)):
        R, tc = PO.pose_about_centre(cam, s)
        out[k, :9] = R; out[k, 9:] = tc
    return out


def cell_sums(P, pose, AB):
    """k_bundle_cells: [n_cells, 67]"""
    acc = np.zeros((P.n_cells, CELL))
    if not P.n_cells:
        return acc
    cam, ln = P.cell_cam, P.cell_line
    M = tuple(P.M[cam, i] for i in range(5)); R = tuple(pose[cam, i] for i in range(9)); t = tuple(pose[cam, 9 + i] for i in range(3))
    ab = tuple(AB[ln, i] for i in range(6))
    e1, e2 = basis(AB[ln])
    count = P.cell_off[1:] - P.cell_off[:-1]
    elig = P.is_eligible[ln]
    for o in range(int(count.max())):
        m = np.flatnonzero(count > o)
        r = P.cell_off[m] + o
        p = tuple(P.obs_p[r, i] for i in range(4))
        sub = lambda tup: tuple(v[m] for v in tup)
        ok, rp, rq, JP, JQ = residuals(sub(M), sub(R), sub(t), sub(ab), sub(e1), sub(e2), p)
        rho, w = huber(rp * rp + rq * rq)
        with np.errstate(all="ignore"):
            term = np.zeros((len(m), CELL))
            k = CC
            for i in range(6):
                for j in range(i, 6):
                    term[:, k] = w * (JP[i] * JP[j] + JQ[i] * JQ[j]); k += 1
            for i in range(6):
                term[:, BC + i] = w * (JP[i] * rp + JQ[i] * rq)
            for i in range(6):
                for j in range(4):
                    term[:, CL + 4 * i + j] = w * (JP[i] * JP[6 + j] + JQ[i] * JQ[6 + j])
            k = LL
            for i in range(4):
                for j in range(i, 4):
                    term[:, k] = w * (JP[6 + i] * JP[6 + j] + JQ[6 + i] * JQ[6 + j]); k += 1
            for i in range(4):
                term[:, BL + i] = w * (JP[6 + i] * rp + JQ[6 + i] * rq)
            term[:, RHO] = rho; term[:, COUNT] = 1.0
            term[~elig[m], CL:RHO] = 0.0                            # a held line's cell: its line parts stay +0.0
            mm = m[ok]
            acc[mm] = acc[mm] + term[ok]
    return acc


def line_factors(P, cells, mu):
    """k_bundle_lines -> (ok [n_lines] bool, L [n_lines, 4, 4], v [n_lines, 4], W [n_cells, 6, 4])"""
    nl = P.n_lines
    ok = np.zeros(nl, bool); L = np.zeros((nl, 4, 4)); v = np.zeros((nl, 4)); W = np.zeros((P.n_cells, 6, 4))
    e = P.eligible
    if not len(e):
        return ok, L, v, W
    H = np.zeros((len(e), 10)); b = np.zeros((len(e), 4))
    c0 = P.line_cell_off[e]; n = P.line_cell_off[e + 1] - c0
    for j in range(int(n.max())):
        m = np.flatnonzero(n > j)
        H[m] = H[m] + cells[c0[m] + j, LL:LL + 10]; b[m] = b[m] + cells[c0[m] + j, BL:BL + 4]
    good = np.ones(len(e), bool)
    Le = np.zeros((len(e), 4, 4))
    with np.errstate(all="ignore"):
        for j in range(4):
            h = H[:, ROW4[j]]
            p = h + mu * h
            for k in range(j):
                p = p - Le[:, j, k] * Le[:, j, k]
            good &= (p > 0.0) & np.isfinite(p)
            Le[:, j, j] = np.sqrt(p)
            for i in range(j + 1, 4):
                x = H[:, ROW4[j] + (i - j)]
                for k in range(j):
                    x = x - Le[:, i, k] * Le[:, j, k]
                Le[:, i, j] = x / Le[:, j, j]
        ve = np.zeros((len(e), 4))
        for i in range(4):
            x = b[:, i]
            for k in range(i):
                x = x - Le[:, i, k] * ve[:, k]
            ve[:, i] = x / Le[:, i, i]
    ok[e[good]] = True; L[e[good]] = Le[good]; v[e[good]] = ve[good]
    cl = np.flatnonzero(ok[P.cell_line])                             # the cells of the lines whose factor stands
    Lc = L[P.cell_line[cl]]
    with np.errstate(all="ignore"):
        for col in range(6):
            y = np.zeros((len(cl), 4))
            for i in range(4):
                x = cells[cl, CL + 4 * col + i]
                for k in range(i):
                    x = x - Lc[:, i, k] * y[:, k]
                y[:, i] = x / Lc[:, i, i]
            W[cl, col] = y
    return ok, L, v, W


def wave_tree(lanes):
    """[64, K] -> [K]: v[i] = v[i] + v[i + stride] for stride 32 .. 1"""
    v = lanes
    stride = 32
    while stride >= 1:
        v = v[:stride] + v[stride:2 * stride]
        stride //= 2
    return v[0]


def lane_sums(terms):
    """[m, K] terms of a camera's cells in order -> [64, K]: lane j adds the terms j, j + 64, .. from +0.0"""
    m, K = terms.shape
    rounds = -(-m // 64) if m else 0
    pad = np.zeros((rounds * 64, K)); pad[:m] = terms
    acc = np.zeros((64, K))
    for r in range(rounds):
        acc = acc + pad[64 * r:64 * r + 64]
    return acc


def dot4(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]


def reduce_system(P, cells, ok, v, W, mu):
    """k_bundle_reduce and the host's assembly -> (S [n, n] with the upper triangle set, g [n])"""
    F = len(P.free_cam)
    n = 6 * F
    S = np.zeros((n, n)); g = np.zeros(n)
    with np.errstate(all="ignore"):
        for fa in range(F):
            ca = P.free_cam[fa]
            mine = P.cam_cells[P.cam_cell_off[ca]:P.cam_cell_off[ca + 1]]
            ln = P.cell_line[mine]
            lok = ok[ln]
            Wa = W[mine]
            for fb in range(fa, F):
                cb = P.free_cam[fb]
                other = mine if fa == fb else P.slot[ln, cb]
                use = lok & (other >= 0)
                Wb = W[np.where(use, other, 0)]
                ww = dot4(Wa[:, :, None, :], Wb[:, None, :, :]).reshape(len(mine), 36)
                ww[~use] = 0.0
                wsum = wave_tree(lane_sums(ww)).reshape(6, 6)
                if fa != fb:
                    S[6 * fa:6 * fa + 6, 6 * fb:6 * fb + 6] = 0.0 - wsum
                    continue
                hc = wave_tree(lane_sums(cells[mine, :27]))
                wv = dot4(Wa, v[ln][:, None, :])
                wv[~lok] = 0.0
                wv = wave_tree(lane_sums(wv))
                for i in range(6):
                    for j in range(6):
                        h = hc[ROW6[i] + (j - i)] if i <= j else hc[ROW6[j] + (i - j)]
                        val = (h + mu * h if i == j else h) - wsum[i, j]
                        if i <= j:
                            S[6 * fa + i, 6 * fa + j] = val
                    g[6 * fa + i] = hc[21 + i] - wv[i]
    return S, g


def dense_solve(S, g):
    """S delta = -g by the Cholesky factorisation of §23 on the upper triangle of S -> delta, or None at a pivot that is not
    finite and > 0.  Every entry meets its subtractions in ascending k, as the loops of the text do."""
    n = len(g)
    if n == 0:
        return np.zeros(0)
    A = np.triu(np.asarray(S, np.float64)).T.copy()                 # A[i, j], i >= j: what is left of H(j, i)
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            p = A[j, j]
            if not (p > 0.0 and math.isfinite(p)):
                return None
            L[j, j] = math.sqrt(p)
            L[j + 1:, j] = A[j + 1:, j] / L[j, j]
            col = L[j + 1:, j]
            if len(col):
                A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - col[:, None] * col[None, :]
        y = -np.asarray(g, np.float64)
        for i in range(n):
            y[i] = y[i] / L[i, i]
            y[i + 1:] = y[i + 1:] - L[i + 1:, i] * y[i]
        z = np.zeros(n)
        for i in range(n - 1, -1, -1):
            x = float(y[i])
            for k in range(i + 1, n):
                x = x - float(L[k, i]) * float(z[k])
            z[i] = x / float(L[i, i])
    return z


def update_lines(P, AB, ok, L, v, W, delta_c):
    """k_bundle_update -> (trial AB [n_lines, 6], delta_l [n_lines, 4])"""
    out = AB.copy(); dl = np.zeros((P.n_lines, 4))
    e = P.eligible[ok[P.eligible]] if len(P.eligible) else P.eligible
    if not len(e):
        return out, dl
    t = -v[e]
    c0 = P.line_cell_off[e]; n = P.line_cell_off[e + 1] - c0
    with np.errstate(all="ignore"):
        for j in range(int(n.max())):
            cell = c0 + j
            fc = np.where(n > j, P.cam_free[P.cell_cam[np.minimum(cell, P.n_cells - 1)]], -1)
            m = np.flatnonzero(fc >= 0)
            if not len(m):
                continue
            for i in range(6):
                for r in range(4):
                    t[m, r] = t[m, r] - W[cell[m], i, r] * delta_c[fc[m], i]
        x = np.zeros((len(e), 4))
        for i in range(3, -1, -1):
            s = t[:, i]
            for k in range(i + 1, 4):
                s = s - L[e, k, i] * x[:, k]
            x[:, i] = s / L[e, i, i]
        e1, e2 = basis(AB[e])
        for k in range(3):
            out[e, k] = AB[e, k] + (x[:, 0] * e1[k] + x[:, 1] * e2[k])
            out[e, 3 + k] = AB[e, 3 + k] + (x[:, 2] * e1[k] + x[:, 3] * e2[k])
    dl[e] = x
    return out, dl


def rho_of(P, pose, AB):
    """[n_obs]: rho(s) of every observation; +0.0 where its image line has no norm"""
    if not P.n_obs:
        return np.zeros(0)
    cam, ln = P.obs_cam, P.obs_line
    M = tuple(P.M[cam, i] for i in range(5)); R = tuple(pose[cam, i] for i in range(9)); t = tuple(pose[cam, 9 + i] for i in range(3))
    p = tuple(P.obs_p[:, i] for i in range(4))
    with np.errstate(all="ignore"):
        _, _, lam, nu, ok = image_line(M, R, t, tuple(AB[ln, i] for i in range(6)))
        rp = ((lam[0] * p[0] + lam[1] * p[1]) + lam[2]) / nu
        rq = ((lam[0] * p[2] + lam[1] * p[3]) + lam[2]) / nu
        rho, _ = huber(rp * rp + rq * rq)
    return np.where(ok, rho, 0.0)


def cost_of(rho):
    """k_bundle_cost's tiles of 256 (every wave of 64 folded by halves, then (W0 + W1) + (W2 + W3)) added in ascending order"""
    n = len(rho)
    tiles = -(-n // 256)
    v = np.zeros(tiles * 256); v[:n] = rho
    v = v.reshape(tiles, 4, 64)
    stride = 32
    while stride >= 1:
        v = v[:, :, :stride] + v[:, :, stride:2 * stride]
        stride //= 2
    v = v[:, :, 0]
    t = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
    s = 0.0
    for x in t:
        s = s + float(x)
    return s


def bundle(segs, line, cams, segs_per_cam, fixed=None, assoc=None, solve=dense_solve, **kw):
    """what one call of the library returns (a non-empty model, at least one camera with a segment), as a dict: cameras,
    segments, line, lines, observations, trace, system / rhs (of capture_iteration; None), summary, associations"""
    par = dict(DEFAULTS, **kw)
    if assoc is None:
        assoc = RM.associations(segs, line, cams, segs_per_cam, par)
    model = np.asarray(segs, np.float64).reshape(-1, 6)
    line = np.asarray(line, np.uint32).reshape(-1)
    P = prepare(segs, line, cams, segs_per_cam, assoc, fixed, par)
    c = P.c
    states = [PO.State(cam, c, 0.0) for cam in cams]
    pose = pose_table(cams, states)
    AB = P.AB.copy()
    F, ne = len(P.free_cam), len(P.eligible)
    cost = cost_of(rho_of(P, pose, AB))
    summary = dict(status="MAX_ITERATIONS" if (F or ne) else "NO_VARIABLES", iterations=0, accepted_steps=0, rejected_steps=0,
                   cost0=cost, n_observations=P.n_obs, n_cells=P.n_cells, n_eligible_lines=ne, n_free_cameras=F, n_lines=P.n_lines)
    mu = par["initial_damping"]
    trace, system, rhs, cells = [], None, None, None
    held_steps = 0
    for it in range(par["max_iterations"] if (F or ne) else 0):
        T = np.zeros((), ITERATION_DTYPE)
        T["damping"] = mu; T["cost"] = cost
        summary["iterations"] += 1
        if cells is None:
            cells = cell_sums(P, pose, AB)
        ok, L, v, W = line_factors(P, cells, mu)
        T["n_held_for_step"] = ne - int(ok.sum())
        held_steps += int(T["n_held_for_step"])
        delta = np.zeros(0)
        if F:
            S, g = reduce_system(P, cells, ok, v, W, mu)
            if par["capture_iteration"] == it + 1:
                system, rhs = S, g
            delta = solve(S, g)
        accept = False
        T["solved"] = delta is not None
        if delta is not None:
            trial_states = [_copy_state(s) for s in states]
            for f, k in enumerate(P.free_cam):
                PO.update(trial_states[k], [float(x) for x in delta[6 * f:6 * f + 6]])
            pose_t = pose.copy()
            for k in P.free_cam:
                R, tc = PO.pose_about_centre(cams[k], trial_states[k])
                pose_t[k, :9] = R; pose_t[k, 9:] = tc
            AB_t, dl = update_lines(P, AB, ok, L, v, W, np.asarray(delta, np.float64).reshape(-1, 6))
            T["step_cameras"] = float(np.abs(delta).max()) if len(delta) else 0.0
            T["step_lines"] = float(np.abs(dl[P.eligible]).max()) if ne else 0.0
            T["cost_trial"] = cost_of(rho_of(P, pose_t, AB_t))
            accept = bool(T["cost_trial"] < cost)
        T["accepted"] = accept
        trace.append(T)
        if accept:
            summary["accepted_steps"] += 1
            states, pose, AB, cells = trial_states, pose_t, AB_t, None
            mu = max(mu / 10.0, par["min_damping"])
            converged = (cost - float(T["cost_trial"])) <= par["function_tolerance"] * cost
            cost = float(T["cost_trial"])
            if converged:
                summary["status"] = "CONVERGED"
                break
        else:
            summary["rejected_steps"] += 1
            mu = mu * 10.0
            if mu > par["max_damping"]:
                summary["status"] = "STALLED"
                break
    summary["cost1"] = cost; summary["damping"] = mu; summary["held_for_step"] = held_steps
    out_cams = [PO.camera_now(cam, s, c) for cam, s in zip(cams, states)]
    lines, obs_rec = P.lines.copy(), P.obs_rec.copy()
    cams16 = [RM.lo_camera(cam, c) for cam in out_cams]
    pieces = {}
    for l in P.eligible:
        Lr = lines[l]
        q = [float(x) for x in AB[l]]
        if summary["accepted_steps"]:
            Lr["P1"] = [q[k] + c[k] for k in range(3)]; Lr["P2"] = [q[3 + k] + c[k] for k in range(3)]
        Lr["status"] = NO_EXTENT
        if not all(math.isfinite(x) for x in q):
            continue
        Mv = [q[k] * 0.5 + q[3 + k] * 0.5 for k in range(3)]
        u = [(q[k] - q[3 + k]) * 0.5 for k in range(3)]
        lo, hi, cam_v = [], [], []
        for r in range(int(P.obs_off[l]), int(P.obs_off[l + 1])):
            ob = obs_rec[r]
            k = int(ob["camera"])
            s_lo, s_hi, valid = RM.span(cams16[k], P.seg2d[k][int(ob["segment"])], Mv, u)
            ob["s_lo"], ob["s_hi"], ob["valid"] = s_lo, s_hi, valid
            if valid:
                lo.append(s_lo); hi.append(s_hi); cam_v.append(k)
        cut = RM.sweep(lo, hi, cam_v, par["visibility"], par["min_length"], math.sqrt(RM.dot3(u, u)))
        if cut:
            Lr["status"] = BUNDLED
            pieces[int(l)] = [[(Mv[k] + a * u[k]) + c[k] for k in range(3)] + [(Mv[k] + b * u[k]) + c[k] for k in range(3)] for a, b in cut]
    out_segs, out_line = [], []
    for l in range(P.n_lines):
        rows = pieces[l] if lines[l]["status"] == BUNDLED else [model[i] for i in np.flatnonzero(line == l)]
        out_segs.extend(rows); out_line.extend([l] * len(rows))
        lines[l]["n_pieces"] = len(rows)
    summary["lines"] = {name: int((lines["status"] == k).sum()) for k, name in enumerate(LINE_STATUS)}
    return dict(cameras=out_cams, segments=np.array(out_segs, np.float64).reshape(-1, 6), line=np.array(out_line, np.uint32), lines=lines,
                observations=obs_rec, trace=np.array(trace, ITERATION_DTYPE).reshape(-1), system=system, rhs=rhs, summary=summary,
                associations=assoc, problem=P)


def _copy_state(s):
    t = PO.State.__new__(PO.State)
    t.__dict__.update(s.__dict__)
    return t


def transform_cameras(cams, scale, Rs, ts):
    """R' = R Rs^T, t' = s t - R' ts"""
    out = []
    for cam in cams:
        R = np.asarray(cam["R"], np.float64).reshape(3, 3) @ np.asarray(Rs, np.float64).T
        out.append(PO.camera(cam["K"], R, scale * np.asarray(cam["t"], np.float64) - R @ np.asarray(ts, np.float64), cam["width"], cam["height"]))
    return out
