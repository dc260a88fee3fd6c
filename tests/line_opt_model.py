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


# ---- the solver -------------------------------------------------------------------------------------------------------
# Written from the rule list of k_lineopt.hip's header comment and DESIGN §10, in the precision `dtype` (np.float64, or
# np.longdouble as the model's own yardstick of how much rounding moves a run):
#
#   evaluation   residuals r_i (2 each) and their 2x4 Jacobians J_i by forward-mode derivatives; at |dotp| >= 1 the angle
#                weight is 1 and its derivative 0.  It fails when |omega| < 1e-12 or a projected line has length < 1e-12.
#   robust loss  Triggs: with s_i = |r_i|^2, r_i and J_i are scaled by sqrt(rho'(s_i)) (Huber: rho'' <= 0, no curvature
#                term); cost = 1/2 sum rho(s_i); H = sum J_i^T J_i, g = sum J_i^T r_i of the scaled quantities, summed one
#                residual after the other.
#   scaling      Jacobi: column j by 1 / (1 + sqrt(H_jj)) of the start point, kept for the whole run.
#   step         (A + D) y = -b with A, b the scaled H, g and D = clamp(diag A, 1e-6, 1e32) / radius, radius = 1e4 at the
#                start, by Cholesky; model decrease = -(y.b + y.A y / 2); step = scaling * y.
#   acceptance   gain ratio q = (cost - new cost) / model decrease > 1e-3.  Accepted: radius /= max(1/3, 1 - (2q - 1)^3),
#                at most 1e16, decrease factor back to 2.  Rejected (also: model decrease not positive, A + D not positive
#                definite, the new point cannot be evaluated): radius /= factor, factor *= 2.
#   stopping     in this order within an iteration: [gradient] max |g_j| <= 1e-10, looked at once per point -- at the start
#                and at every accepted point; [max_iter] before a step is computed, iterations (accepted and rejected
#                alike) >= max_iter; [parameter] |step| <= 1e-8 (|x| + 1e-8), before the step is evaluated; [function]
#                |cost - new cost| <= 1e-6 cost for every step that could be evaluated, taken or not (a taken one is taken
#                first, and the function rule goes before the gradient rule at the new point); [other] after a rejected
#                step, radius < 1e-32.  A start that cannot be evaluated: other, x = x0, no iteration.

GRADIENT, FUNCTION, PARAMETER, MAX_ITER, OTHER = 1, 2, 3, 4, 5
TINY = float(np.finfo(np.float64).tiny)


class _Dual:
    """forward-mode number over n residuals at once: a [n], d [n, 4] = derivative in the 4 line parameters"""
    __slots__ = ("a", "d")
    __array_ufunc__ = None          # array * _Dual is _Dual.__rmul__, not an array of objects

    def __init__(self, a, d):
        self.a, self.d = a, d

    @staticmethod
    def _lift(o, like):
        return o if isinstance(o, _Dual) else _Dual(np.broadcast_to(np.asarray(o, like.a.dtype), like.a.shape), np.zeros_like(like.d))

    def __add__(self, o):
        o = _Dual._lift(o, self); return _Dual(self.a + o.a, self.d + o.d)
    __radd__ = __add__

    def __sub__(self, o):
        o = _Dual._lift(o, self); return _Dual(self.a - o.a, self.d - o.d)

    def __rsub__(self, o):
        return _Dual._lift(o, self) - self

    def __neg__(self):
        return _Dual(-self.a, -self.d)

    def __mul__(self, o):
        o = _Dual._lift(o, self); return _Dual(self.a * o.a, self.a[:, None] * o.d + self.d * o.a[:, None])
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _Dual._lift(o, self)
        q = self.a / o.a
        return _Dual(q, (self.d - q[:, None] * o.d) / o.a[:, None])

    def sqrt(self):
        r = np.sqrt(self.a); return _Dual(r, self.d / (2 * r)[:, None])


def _evaluate(x, cams, obs, dtype):
    """residuals of one line in all its observations -> (ok, r [n, 2], J [n, 2, 4]) in dtype"""
    cams = np.asarray(cams, np.float64).reshape(-1, 16).astype(dtype); obs = np.asarray(obs, np.float64).reshape(-1, 6).astype(dtype)
    n = len(obs)
    x = np.asarray(x, dtype)
    if abs(x[0]) < EPS:
        return False, np.zeros((n, 2), dtype), np.zeros((n, 2, 4), dtype)
    one = np.ones(n, dtype)
    par = [_Dual(x[j] * one, np.tile(np.eye(4, dtype=dtype)[j], (n, 1))) for j in range(4)]
    omega, s = par[0], par[1:]
    nm = s[0] * s[0] + s[1] * s[1] + s[2] * s[2]
    # Q = ((1 - |s|^2) I + 2 [s]x + 2 s s^T) / (1 + |s|^2): l its first column, m = omega times its second
    l = [((1 - nm) + 2 * s[0] * s[0]) / (1 + nm), (2 * s[2] + 2 * s[1] * s[0]) / (1 + nm), (-2 * s[1] + 2 * s[2] * s[0]) / (1 + nm)]
    m = [omega * (-2 * s[2] + 2 * s[0] * s[1]) / (1 + nm), omega * ((1 - nm) + 2 * s[1] * s[1]) / (1 + nm),
         omega * (2 * s[0] + 2 * s[2] * s[1]) / (1 + nm)]
    C = [cams[:, 9], cams[:, 10], cams[:, 11]]
    mc = [m[0] - (C[1] * l[2] - C[2] * l[1]), m[1] - (C[2] * l[0] - C[0] * l[2]), m[2] - (C[0] * l[1] - C[1] * l[0])]
    q = [cams[:, 3 * i] * mc[0] + cams[:, 3 * i + 1] * mc[1] + cams[:, 3 * i + 2] * mc[2] for i in range(3)]
    fx, fy, px, py = cams[:, 12], cams[:, 13], cams[:, 14], cams[:, 15]
    pl0 = fy * q[0]; pl1 = fx * q[1]; pl2 = -(fy * px) * q[0] - (fx * py) * q[1] + (fx * fy) * q[2]
    d = (pl0 * pl0 + pl1 * pl1).sqrt()
    if n and np.any(d.a < EPS):
        return False, np.zeros((n, 2), dtype), np.zeros((n, 2, 4), dtype)
    dotp = pl0 / d * obs[:, 4] + pl1 / d * obs[:, 5]
    inside = np.abs(dotp.a) < 1                      # False for NaN too: weight 1, derivative 0
    c = np.where(inside, dotp.a, 0 * one)
    angle = np.arccos(c)
    dangle = -1 / np.sqrt(1 - c * c)
    fold = angle > dtype(np.pi) / 2
    angle = np.where(fold, dtype(np.pi) - angle, angle)
    dangle = np.where(fold, -dangle, dangle)
    w = np.where(inside, np.exp(2 * angle), one)
    aw = _Dual(w, np.where(inside, 2 * w * dangle, 0 * one)[:, None] * dotp.d)
    r1 = (pl0 * obs[:, 0] + pl1 * obs[:, 1] + pl2) / d * aw
    r2 = (pl0 * obs[:, 2] + pl1 * obs[:, 3] + pl2) / d * aw
    return True, np.stack([r1.a, r2.a], 1), np.stack([r1.d, r2.d], 1)


def jacobian(x, cam, obs):
    """the 2x4 Jacobian of residual(x, cam, obs) in x = (omega, s), before the loss (zeros where residual() fails)"""
    return _evaluate(x, [cam], [obs], np.float64)[2][0]


def _seq(a):
    """sum over axis 0, one term after the other in the array's own precision"""
    return np.cumsum(a, axis=0)[-1] if len(a) else np.zeros(a.shape[1:], a.dtype)


def _normal_equations(x, cams, obs, dtype):
    """-> (ok, cost, H [4, 4], g [4]) of the Triggs-scaled problem at x"""
    ok, r, J = _evaluate(x, cams, obs, dtype)
    if not ok:
        return False, dtype(np.inf), None, None
    s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    out = s > 4
    root = np.sqrt(np.where(out, s, 4 + 0 * s))
    rho = np.where(out, 4 * root - 4, s)
    w = np.sqrt(np.where(out, 2 / root, 1 + 0 * s))            # sqrt(rho')
    f = w[:, None] * r; Jw = w[:, None, None] * J
    H = _seq(Jw[:, 0, :, None] * Jw[:, 0, None, :] + Jw[:, 1, :, None] * Jw[:, 1, None, :])
    g = _seq(Jw[:, 0, :] * f[:, 0, None] + Jw[:, 1, :] * f[:, 1, None])
    cost = _seq(rho / 2)
    if not np.isfinite(cost):
        return False, cost, None, None
    return True, cost, H, g


class _Margin:
    """smallest relative distance of a compared quantity from its threshold over the decisions of a run"""

    def __init__(self):
        self.least = np.inf

    def __call__(self, q, t):
        self.least = min(self.least, float(abs(q - t)) / max(float(abs(t)), TINY))


def _cholesky_solve(A, rhs, dtype, margin):
    """y of A y = rhs for a symmetric positive definite A, else None"""
    n = len(rhs)
    L = np.zeros((n, n), dtype)
    for i in range(n):
        for j in range(i + 1):
            v = A[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            if i == j:
                margin(v, 0.0)
                if not v > 0:
                    return None
                L[i, i] = np.sqrt(v)
            else:
                L[i, j] = v / L[j, j]
    z = np.zeros(n, dtype); y = np.zeros(n, dtype)
    for i in range(n):
        v = rhs[i]
        for k in range(i):
            v = v - L[i, k] * z[k]
        z[i] = v / L[i, i]
    for i in reversed(range(n)):
        v = z[i]
        for k in range(i + 1, n):
            v = v - L[k, i] * y[k]
        y[i] = v / L[i, i]
    return y


def lm_solve(x0, cams, obs, max_iter, dtype=np.float64, trace=None):
    """Levenberg-Marquardt on one line by the rules above -> (x, cost0, cost1, iters, status, min_margin).  cams [n, 16] is
    the camera of every observation, obs [n, 6].  min_margin: the least |q - t| / max(|t|, tiny) over the threshold
    decisions the run took (gain ratio against 1e-3, |cost change| against 1e-6 cost, step norm against its bound,
    gradient max-norm against 1e-10, model decrease against 0, Cholesky pivots against 0).  trace: a list that receives
    'accepted' / 'rejected' per iteration ('stopped' for the step of the parameter rule)."""
    margin = _Margin()
    c = lambda v: dtype(v)
    x = np.asarray(x0, np.float64).astype(dtype)
    ok, cost, H, g = _normal_equations(x, cams, obs, dtype)
    if not ok:
        return np.asarray(x0, np.float64).copy(), float(cost), float(cost), 0, OTHER, np.inf
    cost0 = cost
    scale = 1 / (1 + np.sqrt(np.diag(H)))
    radius, factor = c(1e4), c(2.0)
    iters = 0

    def finish(status):
        return x.astype(np.float64), float(cost0), float(cost), iters, status, margin.least

    gmax = np.max(np.abs(g))
    margin(gmax, 1e-10)
    if gmax <= c(1e-10):
        return finish(GRADIENT)
    while True:
        if iters >= max_iter:
            return finish(MAX_ITER)
        iters += 1
        A = scale[:, None] * H * scale[None, :]
        b = scale * g
        D = A + np.diag(np.minimum(np.maximum(np.diag(A), c(1e-6)), c(1e32)) / radius)
        y = _cholesky_solve(D, -b, dtype, margin)
        taken = False
        if y is not None:
            yb = c(0); yAy = c(0)
            for p in range(4):
                yb = yb + y[p] * b[p]
                t = c(0)
                for q_ in range(4):
                    t = t + A[p, q_] * y[q_]
                yAy = yAy + y[p] * t
            decrease = -(yb + yAy / 2)
            margin(decrease, 0.0)
            if decrease > 0 and np.isfinite(decrease):
                step = scale * y
                ns = c(0); nx = c(0)
                for j in range(4):
                    ns = ns + step[j] * step[j]; nx = nx + x[j] * x[j]
                bound = c(1e-8) * (np.sqrt(nx) + c(1e-8))
                margin(np.sqrt(ns), bound)
                if np.sqrt(ns) <= bound:
                    if trace is not None:
                        trace.append("stopped")
                    return finish(PARAMETER)
                xn = x + step
                okn, costn, Hn, gn = _normal_equations(xn, cams, obs, dtype)
                if okn:
                    dc = cost - costn
                    margin(abs(dc), c(1e-6) * cost)
                    small = abs(dc) <= c(1e-6) * cost
                    ratio = dc / decrease
                    margin(ratio, 1e-3)
                    if ratio > c(1e-3):
                        x, cost, H, g = xn, costn, Hn, gn
                        t = 2 * ratio - 1
                        radius = min(c(1e16), radius / max(c(1.0) / c(3.0), 1 - t * t * t))
                        factor = c(2.0)
                        taken = True
                        if trace is not None:
                            trace.append("accepted")
                        if small:
                            return finish(FUNCTION)
                        gmax = np.max(np.abs(g))
                        margin(gmax, 1e-10)
                        if gmax <= c(1e-10):
                            return finish(GRADIENT)
                    elif small:
                        if trace is not None:
                            trace.append("rejected")
                        return finish(FUNCTION)
        if not taken:
            if trace is not None:
                trace.append("rejected")
            radius = radius / factor
            factor = factor * 2
            if radius < c(1e-32):
                return finish(OTHER)
