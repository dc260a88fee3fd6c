"""The contract of DESIGN §27 (camera poses refined against the 3D line model by iterated closest lines) restated in numpy
from the text: the frame about the model's centre, the pose as a delta on the input, the 29 sums of an iteration with the
tile tree of k_pose_normal, the Cholesky solve, the update, the gate that halves on a stall, the stop rules and the delivery
pass.  The projection comes from tests/project_lines_model.py / project_lines_model_vec.py, the association from
tests/associate_model.py.  Two forms: `form="scalar"` walks the segments one by one with Python floats and projects and
associates pair by pair, `form="array"` runs the same expressions on arrays; tests/test_pose_host.py shows the two
byte-identical.  Python floats and numpy's element-wise float64 operations round every operation on its own, as the
library does when built with -ffp-contract=off; dot products are written out left to right."""
import math

import numpy as np

from tests import associate_model as AM
from tests import project_lines_model as PM
from tests import project_lines_model_vec as PV

SUMMARY_DTYPE = np.dtype([("status", "<u4"), ("iterations", "<u4"), ("n_matched", "<u8"), ("rms", "<f8"), ("last_step", "<f8"),
                          ("q", "<f8", 4), ("t", "<f8", 3)])
ITERATION_DTYPE = np.dtype([("gate", "<f8"), ("sums", "<f8", 29), ("delta", "<f8", 6), ("R", "<f8", 9), ("t", "<f8", 3),
                            ("n_matched", "<u8")])
STATUS = ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW", "DEGENERATE")
SUMMARY_KEYS = ("status", "iterations", "n_matched", "rms", "last_step", "q", "t")
TILE, WAVE, TERMS = 256, 64, 29
ROW = (0, 6, 11, 15, 18, 20)                     # where row i of the upper triangle begins
DEFAULTS = dict(max_distance=2.5, min_cos2=AM.min_cos2_of(10.0), min_overlap=0.5, start_distance=0.0, stall_tolerance=1e-4,
                step_tolerance=1e-9, near_plane=1e-6, max_iterations=50, min_matches=8)


def unit(q):
    """q / sqrt(q.q)"""
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(((w * w + x * x) + y * y) + z * z)
    return (w / n, x / n, y / n, z / n)


def rotation(q):
    """R(q) of a unit quaternion: the nine expressions of §23, row-major"""
    w, x, y, z = q
    return (1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y))


def mul33(A, v):
    return tuple((A[3 * i] * v[0] + A[3 * i + 1] * v[1]) + A[3 * i + 2] * v[2] for i in range(3))


def camera(K, R, t, width, height):
    return dict(K=np.array(K, np.float64).reshape(3, 3), R=np.array(R, np.float64).reshape(3, 3), t=np.array(t, np.float64).reshape(3),
                width=int(width), height=int(height))


def floats(a):
    return tuple(float(v) for v in np.asarray(a, np.float64).reshape(-1))


def bounding_box(segs):
    """(c, diag): the midpoint and the diagonal of the box of all end points"""
    pts = np.asarray(segs, np.float64).reshape(-1, 3)
    lo = [float(v) for v in pts.min(0)]; hi = [float(v) for v in pts.max(0)]
    c = tuple((lo[k] + hi[k]) * 0.5 for k in range(3))
    e = [hi[k] - lo[k] for k in range(3)]
    return c, math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])


def inverse_transpose(K):
    """the entries m00, m10, m11, m20, m21 of K^-T for an upper-triangular K with K22 = 1"""
    K = floats(K)
    m00 = 1.0 / K[0]
    m11 = 1.0 / K[4]
    m10 = -((K[1] * m00) * m11)
    m20 = -(K[2] * m00) - K[5] * m10
    m21 = -(K[5] * m11)
    return (m00, m10, m11, m20, m21)


class State:
    """the delta (q, tau) on a camera's input pose, t'_in = t_in + R_in c, the gate, and how far the camera has come"""

    def __init__(self, cam, c, gate):
        self.q, self.tau = (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
        R, t = floats(cam["R"]), floats(cam["t"])
        rc = mul33(R, c)
        self.tin = tuple(t[i] + rc[i] for i in range(3))
        self.gate, self.last_step, self.status, self.iterations, self.updated = gate, 0.0, "TOO_FEW", 0, False


def pose_about_centre(cam, s):
    """R = R(q^) R_in, t' = R(q^) t'_in + tau"""
    Rd = rotation(unit(s.q))
    Rin = floats(cam["R"])
    R = tuple((Rd[3 * i] * Rin[j] + Rd[3 * i + 1] * Rin[3 + j]) + Rd[3 * i + 2] * Rin[6 + j] for i in range(3) for j in range(3))
    u = mul33(Rd, s.tin)
    return R, tuple(u[i] + s.tau[i] for i in range(3))


def camera_now(cam, s, c):
    """the camera as it is handed out: the input itself while no update has been made; else K, R, t = t' - R c"""
    if not s.updated:
        return camera(cam["K"], cam["R"], cam["t"], cam["width"], cam["height"])
    R, tc = pose_about_centre(cam, s)
    rc = mul33(R, c)
    return camera(cam["K"], R, tuple(tc[i] - rc[i] for i in range(3)), cam["width"], cam["height"])


def update(s, delta):
    """step 5: q <- dq (x) q, normalised; tau <- dR tau + delta_3..5"""
    dq = unit((1.0, delta[0] * 0.5, delta[1] * 0.5, delta[2] * 0.5))
    dR = rotation(dq)
    q = s.q
    s.q = unit((((dq[0] * q[0] - dq[1] * q[1]) - dq[2] * q[2]) - dq[3] * q[3],
                ((dq[0] * q[1] + dq[1] * q[0]) + dq[2] * q[3]) - dq[3] * q[2],
                ((dq[0] * q[2] - dq[1] * q[3]) + dq[2] * q[0]) + dq[3] * q[1],
                ((dq[0] * q[3] + dq[1] * q[2]) - dq[2] * q[1]) + dq[3] * q[0]))
    u = mul33(dR, s.tau)
    s.tau = tuple(u[i] + delta[3 + i] for i in range(3))
    s.updated = True


def pose_line(M, v):
    """K^-T v"""
    return (M[0] * v[0], M[1] * v[0] + M[2] * v[1], (M[3] * v[0] + M[4] * v[1]) + v[2])


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def point_term(x, y, lam, nu, dl, B):
    """the 28 sums of one 2D end point (H 21, b 6, cost); floats or arrays"""
    u = (lam[0] * x + lam[1] * y) + lam[2]
    r = u / nu
    J = [((dl[i][0] * x + dl[i][1] * y) + dl[i][2]) / nu - u * B[i] for i in range(6)]
    out = [J[i] * J[j] for i in range(6) for j in range(i, 6)]
    out += [J[i] * r for i in range(6)]
    out.append(r * r)
    return out


def line_of(M, R, t, X1, X2):
    """(lam, nu, dl, B) of a 3D segment in the pose (R, t); floats or arrays"""
    Y1 = tuple(v + t[i] for i, v in enumerate(mul33(R, X1)))
    Y2 = tuple(v + t[i] for i, v in enumerate(mul33(R, X2)))
    N = cross(Y1, Y2)
    D = (Y2[0] - Y1[0], Y2[1] - Y1[1], Y2[2] - Y1[2])
    lam = pose_line(M, N)
    nu = np.sqrt(lam[0] * lam[0] + lam[1] * lam[1])
    dN = ((0.0, -N[2], N[1]), (N[2], 0.0, -N[0]), (-N[1], N[0], 0.0),
          (0.0, -D[2], D[1]), (D[2], 0.0, -D[0]), (-D[1], D[0], 0.0))
    nu3 = (nu * nu) * nu
    dl = [pose_line(M, dN[i]) for i in range(6)]
    with np.errstate(all="ignore"):
        B = [(lam[0] * dl[i][0] + lam[1] * dl[i][1]) / nu3 for i in range(6)]
    return lam, nu, dl, B


def segment_terms(M, R, t, model, segs2d, assoc, form="array"):
    """[n, 29]: term(P) + term(Q) and count 1.0 of a matched 2D segment whose image line has a norm that is finite and
    > 0, 29 times +0.0 of every other one"""
    model = np.asarray(model, np.float64).reshape(-1, 6)
    sg = np.asarray(segs2d, np.float32).reshape(-1, 4).astype(np.float64)
    out = np.zeros((len(sg), TERMS))
    hit = np.flatnonzero((assoc["record"] >= 0) & (assoc["segment"] < len(model)))
    if form == "scalar":
        for i in hit:
            X = [float(v) for v in model[assoc["segment"][i]]]
            lam, nu, dl, B = line_of(M, R, t, X[:3], X[3:])
            nu = float(nu)
            if not (nu > 0.0 and math.isfinite(nu)):
                continue
            B = [float(b) for b in B]
            p = [float(v) for v in sg[i]]
            t1 = point_term(p[0], p[1], lam, nu, dl, B); t2 = point_term(p[2], p[3], lam, nu, dl, B)
            out[i, :28] = [a + b for a, b in zip(t1, t2)]
            out[i, 28] = 1.0
        return out
    if len(hit):
        X = model[assoc["segment"][hit]]
        with np.errstate(all="ignore"):
            lam, nu, dl, B = line_of(M, R, t, (X[:, 0], X[:, 1], X[:, 2]), (X[:, 3], X[:, 4], X[:, 5]))
            ok = (nu > 0.0) & np.isfinite(nu)
            p = sg[hit]
            t1 = point_term(p[:, 0], p[:, 1], lam, nu, dl, B); t2 = point_term(p[:, 2], p[:, 3], lam, nu, dl, B)
        rows = hit[ok]
        for k in range(28):
            out[rows, k] = (t1[k] + t2[k])[ok]
        out[rows, 28] = 1.0
    return out


def tile_sums(terms):
    """the tree of k_pose_normal: per tile of 256 segments (lanes past the end hold +0.0) every wave of 64 folded by
    halves, stride 32 .. 1, then (W0 + W1) + (W2 + W3) -> [n_tiles, 29]"""
    n = len(terms)
    n_tiles = -(-n // TILE)
    v = np.zeros((n_tiles * TILE, TERMS))
    v[:n] = terms
    v = v.reshape(n_tiles, TILE // WAVE, WAVE, TERMS)
    stride = WAVE // 2
    while stride >= 1:
        v = v[:, :, :stride] + v[:, :, stride:2 * stride]
        stride //= 2
    v = v[:, :, 0]
    return (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])


def tile_sums_walk(terms):
    """the same tree walked lane by lane with Python floats"""
    n = len(terms)
    out = []
    for t0 in range(0, n, TILE):
        waves = []
        for w0 in range(t0, t0 + TILE, WAVE):
            v = [[float(terms[i][k]) if i < n else 0.0 for k in range(TERMS)] for i in range(w0, w0 + WAVE)]
            stride = WAVE // 2
            while stride >= 1:
                for i in range(stride):
                    v[i] = [a + b for a, b in zip(v[i], v[i + stride])]
                stride //= 2
            waves.append(v[0])
        out.append([(waves[0][k] + waves[1][k]) + (waves[2][k] + waves[3][k]) for k in range(TERMS)])
    return np.array(out, np.float64).reshape(-1, TERMS)


def host_sum(tiles):
    """the host's sum: from +0.0, tile after tile in ascending order"""
    s = np.zeros(TERMS)
    for t in tiles:
        s = s + t
    return s


def solve(sums):
    """H delta = -b by the Cholesky factorisation of §23 (n = 6) -> delta (6 floats), or None at a pivot that is not
    finite and > 0"""
    s = [float(v) for v in sums]
    n = 6

    def H(i, j):                                 # i <= j
        return s[ROW[i] + (j - i)]
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        p = H(j, j)
        for k in range(j):
            p = p - L[j][k] * L[j][k]
        if not (p > 0.0 and math.isfinite(p)):
            return None
        L[j][j] = math.sqrt(p)
        for i in range(j + 1, n):
            v = H(j, i)
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    y = [0.0] * n
    for i in range(n):
        v = -s[21 + i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, n):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    return x


def step_of(delta, diag):
    return max(max(abs(v) for v in delta[:3]), max(abs(v) / diag for v in delta[3:]))


def one_pass(model, line, K, R, t, width, height, segs2d, gate, par, form):
    """steps 2-4 for one camera in the pose (R, t) on `model` -> (records, associations, sums)"""
    cam = camera(K, R, t, width, height)
    P1, P2 = model[:, :3], model[:, 3:]
    if form == "scalar":
        rec = PM.project_segments([cam], P1, P2, line, par["near_plane"])[0]
        assoc = AM.associate_scalar(rec, segs2d, gate, par["min_cos2"], par["min_overlap"])
    else:
        rec = PV.project_camera(cam, P1, P2, line, par["near_plane"])
        assoc = AM.associate(rec, segs2d, gate, par["min_cos2"], par["min_overlap"])
    terms = segment_terms(inverse_transpose(K), floats(R), floats(t), model, segs2d, assoc, form)
    return rec, assoc, host_sum(tile_sums(terms))


def refine_camera(model, centred, line, cam, segs2d, par, c, diag, form="array"):
    """one camera, independently of every other -> (camera, summary, associations, trace)"""
    segs2d = np.asarray(segs2d, np.float32).reshape(-1, 4)
    s = State(cam, c, max(par["max_distance"], par["start_distance"]))
    trace = np.zeros(par["max_iterations"], ITERATION_DTYPE)
    K, w, h = cam["K"], cam["width"], cam["height"]
    if len(segs2d) and len(model):
        for k in range(par["max_iterations"]):
            R, tc = pose_about_centre(cam, s)
            _, _, sums = one_pass(centred, line, K, R, tc, w, h, segs2d, s.gate, par, form)
            s.iterations = k + 1
            n_matched = int(sums[28])
            trace[k]["gate"] = s.gate; trace[k]["sums"] = sums; trace[k]["n_matched"] = n_matched
            delta, done = None, True
            if n_matched < par["min_matches"]:
                s.status = "TOO_FEW"
            else:
                delta = solve(sums)
                if delta is None:
                    s.status = "DEGENERATE"
            if delta is not None:
                update(s, delta)
                s.last_step = step_of(delta, diag)
                trace[k]["delta"] = delta
                if s.gate == par["max_distance"] and s.last_step <= par["step_tolerance"]:
                    s.status = "CONVERGED"
                elif k + 1 == par["max_iterations"]:
                    s.status = "MAX_ITERATIONS"
                else:
                    done = False
                    if s.last_step <= par["stall_tolerance"]:
                        s.gate = max(par["max_distance"], s.gate * 0.5)
            now = camera_now(cam, s, c)
            trace[k]["R"] = now["R"].reshape(9); trace[k]["t"] = now["t"]
            if done:
                break
    out = camera_now(cam, s, c)
    summary = dict(status=s.status, iterations=s.iterations, n_matched=0, rms=0.0, last_step=s.last_step,
                   q=np.array(s.q), t=np.array(s.tau))
    assoc = AM.nothing(len(segs2d))
    if len(segs2d) and len(model):
        # the delivery pass: the model as given, the camera as it is handed out, at max_distance
        _, assoc, sums = one_pass(model, line, K, out["R"], out["t"], w, h, segs2d, par["max_distance"], par, form)
        summary["n_matched"] = int(sums[28])
        summary["rms"] = math.sqrt(float(sums[27]) / (2.0 * float(sums[28]))) if summary["n_matched"] else 0.0
    return out, summary, assoc, trace[:s.iterations]


def refine(segs, line, cams, segs_per_cam, form="array", **kw):
    """what one call of the library returns, as a dict: cameras, summaries (status as a name), associations, trace (one
    ITERATION_DTYPE array per camera, one entry per iteration run)"""
    par = dict(DEFAULTS, **kw)
    model = np.asarray(segs, np.float64).reshape(-1, 6)
    line = np.asarray(line, np.uint32).reshape(-1)
    c, diag = bounding_box(model) if len(model) else ((0.0, 0.0, 0.0), 0.0)
    assert diag > 0.0 or not len(model)
    centred = (model.reshape(-1, 3) - np.array(c)).reshape(-1, 6)
    res = dict(cameras=[], summaries=[], associations=[], trace=[])
    for cam, s2 in zip(cams, segs_per_cam):
        out = refine_camera(model, centred, line, cam, s2, par, c, diag, form)
        for key, v in zip(("cameras", "summaries", "associations", "trace"), out):
            res[key].append(v)
    return res


def pose_difference(cam, ref, depth):
    """(angle between the two rotations in degrees, distance of the two camera centres as a share of `depth`)"""
    Ra, Rb = np.asarray(cam["R"], np.float64).reshape(3, 3), np.asarray(ref["R"], np.float64).reshape(3, 3)
    dR = Ra @ Rb.T
    sine = 0.5 * math.sqrt((dR[2, 1] - dR[1, 2]) ** 2 + (dR[0, 2] - dR[2, 0]) ** 2 + (dR[1, 0] - dR[0, 1]) ** 2)
    Ca = -Ra.T @ np.asarray(cam["t"], np.float64).reshape(3); Cb = -Rb.T @ np.asarray(ref["t"], np.float64).reshape(3)
    return math.degrees(math.atan2(sine, (float(np.trace(dR)) - 1.0) * 0.5)), float(np.linalg.norm(Ca - Cb)) / depth
