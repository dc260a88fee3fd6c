"""Independent numpy model of the line bundling stage (the checker of tests/test_line_opt.py and
tests/test_gpu_line_opt.py), written from the reference's optimization.{h,cc}:

  to_cayley         LineOptimizer::optimize, optimization.cc:31-95 (Plücker, then Cayley; FullPivLU kernel for lines
                    through the origin; NaN -> held constant)
  write_back        optimization.cc:209-295
  residual          LineReprojectionError::operator() (optimization.h), the camera rotation applied as R directly
  cost              1/2 sum HuberLoss(2)(|r_i|^2)
  minimise          scipy.optimize.minimize of that scalar cost from a start point
"""
import numpy as np

EPS = 1e-12


def _inv3(A):
    """3x3 inverse by cofactors (what Eigen does for a fixed 3x3): singular -> inf / NaN entries, no exception"""
    a = A.reshape(-1)
    c00 = a[4] * a[8] - a[5] * a[7]
    c10 = a[5] * a[6] - a[3] * a[8]
    c20 = a[3] * a[7] - a[4] * a[6]
    det = a[0] * c00 + (a[1] * c10 + a[2] * c20)
    with np.errstate(divide="ignore", invalid="ignore"):
        idet = 1.0 / det
        return np.array([[c00, a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4]],
                         [c10, a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5]],
                         [c20, a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]]]) * idet


def to_cayley(P1, P2):
    """-> (x = (omega, s), constant)"""
    P1 = np.asarray(P1, np.float64); P2 = np.asarray(P2, np.float64)
    l = (P2 - P1) / np.linalg.norm(P2 - P1)
    m = np.cross(0.5 * (P1 + P2), l)
    omega = np.linalg.norm(m)
    if omega < EPS:
        # null space of the 1x3 row l^T by full-pivot LU: pivot column k = first largest |l_k|, columns 0 and k swapped;
        # basis vector c has a 1 at the c-th free (permuted) column and -u_c / u_pivot at row k
        k = int(np.argmax(np.abs(l)))
        perm = [0, 1, 2]; perm[0], perm[k] = perm[k], perm[0]
        E = np.zeros((3, 2))
        for c in range(2):
            E[k, c] = -(l[perm[c + 1]] / l[perm[0]])
            E[perm[c + 1], c] = 1.0
        e1, e2 = E[:, 0], E[:, 1]
    else:
        e1 = m / np.linalg.norm(m)
        n = np.cross(l, m)
        e2 = n / np.linalg.norm(n)
    Q = np.stack([l, e1, e2], 1)
    I = np.eye(3)
    with np.errstate(invalid="ignore", over="ignore"):
        sx = (Q - I) @ _inv3(Q + I)
    x = np.array([omega, sx[2, 1], sx[0, 2], sx[1, 0]])
    if np.any(np.isnan(x)):
        return np.array([-1.0, 0.0, 0.0, 0.0]), True
    return x, False


def plucker(x):
    """(l, m) of the Cayley parameters"""
    omega, s = x[0], np.asarray(x[1:4], np.float64)
    nm = s @ s
    S = np.array([[0, -s[2], s[1]], [s[2], 0, -s[0]], [-s[1], s[0], 0]])
    Q = 1.0 / (1.0 + nm) * ((1.0 - nm) * np.eye(3) + 2.0 * S + 2.0 * np.outer(s, s))
    return Q[:, 0], omega * Q[:, 1]


def write_back(x, P1_old, P2_old):
    """-> (P1, P2, kept)"""
    P1_old = np.asarray(P1_old, np.float64); P2_old = np.asarray(P2_old, np.float64)
    P1, P2 = P1_old, P2_old
    omega = x[0]
    if not (omega < 0.0 or abs(omega) < EPS):
        l, m = plucker(x)
        if np.any(np.abs(l) > EPS):
            Pm = 0.5 * (P1_old + P2_old)
            a = np.abs(l)
            if a[0] > a[1] and a[0] > a[2]:
                x1 = Pm[0]; x3 = (-m[1] - x1 * l[2]) / -l[0]; x2 = (m[2] - x1 * l[1]) / -l[0]
            elif a[1] > a[0] and a[1] > a[2]:
                x2 = Pm[1]; x3 = (m[0] - x2 * l[2]) / -l[1]; x1 = (m[2] + x2 * l[0]) / l[1]
            else:
                x3 = Pm[2]; x2 = (m[0] + x3 * l[1]) / l[2]; x1 = (-m[1] + x3 * l[0]) / l[2]
            P = np.array([x1, x2, x3])
            P1, P2 = P + l, P - l
    return P1, P2, bool(np.linalg.norm(P1 - P2) > EPS)


def observation(seg):
    """(p1x, p1y, p2x, p2y, nx, ny) of a float segment (x1, y1, x2, y2): optimization.cc:150-162"""
    p = np.asarray(seg, np.float32).astype(np.float64)
    d = p[2:4] - p[0:2]
    n = np.linalg.norm(d)
    if n > 0:
        d = d / n
    return np.array([p[0], p[1], p[2], p[3], -d[1], d[0]])


def camera(R, C, K):
    """the 16 numbers of l3d_line_opt_eval: R row-major, C, fx, fy, px, py"""
    K = np.asarray(K, np.float64)
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(C, np.float64), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]])


def residual(x, cam, obs, angle_weight=True):
    """LineReprojectionError for one observation -> (ok, r[2]); angle_weight=False: the weight held at 1"""
    omega = x[0]
    l, m = plucker(x)
    if abs(omega) < EPS:
        return False, np.zeros(2)
    R = cam[0:9].reshape(3, 3); C = cam[9:12]; fx, fy, px, py = cam[12:16]
    m = m - np.cross(C, l)
    q = R @ m
    pl = np.array([fy * q[0], fx * q[1], -fy * px * q[0] - fx * py * q[1] + fx * fy * q[2]])
    d = np.sqrt(pl[0] * pl[0] + pl[1] * pl[1])
    if d < EPS:
        return False, np.zeros(2)
    aw = 1.0
    dotp = pl[0] / d * obs[4] + pl[1] / d * obs[5]
    with np.errstate(invalid="ignore"):
        angle = np.arccos(dotp)
    if angle_weight and np.isfinite(angle):
        if angle > np.pi / 2:
            angle = np.pi - angle
        aw = np.exp(2.0 * angle)
    r = np.array([(pl[0] * obs[0] + pl[1] * obs[1] + pl[2]) / d * aw, (pl[0] * obs[2] + pl[1] * obs[3] + pl[2]) / d * aw])
    return True, r


def huber(s):
    return s if s <= 4.0 else 4.0 * np.sqrt(s) - 4.0


def cost(x, cams, obs):
    """1/2 sum rho(|r_i|^2); inf when an evaluation fails (the residuals of residual(), all observations at once)"""
    cams = np.asarray(cams, np.float64).reshape(-1, 16); obs = np.asarray(obs, np.float64).reshape(-1, 6)
    if abs(x[0]) < EPS:
        return np.inf
    l, m = plucker(x)
    R = cams[:, 0:9].reshape(-1, 3, 3); C = cams[:, 9:12]; fx, fy, px, py = cams[:, 12], cams[:, 13], cams[:, 14], cams[:, 15]
    q = np.einsum("nij,nj->ni", R, m[None, :] - np.cross(C, l[None, :]))
    pl0 = fy * q[:, 0]; pl1 = fx * q[:, 1]; pl2 = -fy * px * q[:, 0] - fx * py * q[:, 1] + fx * fy * q[:, 2]
    d = np.sqrt(pl0 * pl0 + pl1 * pl1)
    if np.any(d < EPS):
        return np.inf
    dotp = pl0 / d * obs[:, 4] + pl1 / d * obs[:, 5]
    with np.errstate(invalid="ignore"):
        angle = np.arccos(dotp)
    fin = np.isfinite(angle)
    angle = np.where(angle > np.pi / 2, np.pi - angle, angle)
    aw = np.where(fin, np.exp(2.0 * np.where(fin, angle, 0.0)), 1.0)
    r1 = (pl0 * obs[:, 0] + pl1 * obs[:, 1] + pl2) / d * aw
    r2 = (pl0 * obs[:, 2] + pl1 * obs[:, 3] + pl2) / d * aw
    s = r1 * r1 + r2 * r2
    return 0.5 * float(np.sum(np.where(s <= 4.0, s, 4.0 * np.sqrt(np.maximum(s, 4.0)) - 4.0)))


def minimise(x0, cams, obs):
    """scipy's optimum of the scalar robust cost from x0 -> (x, cost, converged): BFGS, polished by Nelder-Mead;
    converged = either reports success"""
    from scipy.optimize import minimize
    f = lambda x: cost(x, cams, obs)
    r = minimize(f, np.asarray(x0, np.float64), method="BFGS", jac="3-point", options=dict(gtol=1e-10, maxiter=400))
    r2 = minimize(f, r.x, method="Nelder-Mead", options=dict(xatol=1e-12, fatol=1e-14, maxiter=1500))
    best = r2 if r2.fun <= r.fun else r
    return best.x, float(best.fun), bool(r.success or r2.success)


def infinite_line(P1, P2):
    """(unit direction with its largest component positive, point of the line closest to the origin)"""
    P1 = np.asarray(P1, np.float64); P2 = np.asarray(P2, np.float64)
    d = (P2 - P1) / np.linalg.norm(P2 - P1)
    if d[np.argmax(np.abs(d))] < 0:
        d = -d
    return d, P1 - (P1 @ d) * d
