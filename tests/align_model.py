"""The contract of DESIGN §23 (two 3D line models aligned by iterated closest lines) restated in numpy from the text: the
transform, the 37 sums of an iteration with the tile tree of k_align_normal, the Cholesky solve, the update, the stop
rule and the delivery pass.  The matches come from tests/compare_model.py.  Two forms: `form="scalar"` walks the queries
one by one with Python floats and matches pair by pair, `form="array"` runs the same expressions on arrays;
tests/test_align_host.py shows the two byte-identical.  Python floats and numpy's element-wise float64 operations round
every operation on its own, as the library does when built with -ffp-contract=off; dot products are written out left to
right."""
import math

import numpy as np

from tests import compare_model as CM

SIMILARITY_DTYPE = np.dtype([("scale", "<f8"), ("q", "<f8", 4), ("t", "<f8", 3)])
ITERATION_DTYPE = np.dtype([("gate", "<f8"), ("sums", "<f8", 37), ("delta", "<f8", 7), ("similarity", SIMILARITY_DTYPE),
                            ("n_matched", "<u8")])
STATUS = ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW", "DEGENERATE")
SUMMARY_KEYS = ("status", "iterations", "n_matched", "rms", "last_step", "diag", "center")
TILE, WAVE, TERMS = 256, 64, 37
IDENTITY = dict(scale=1.0, q=(1.0, 0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0))
DEFAULTS = dict(min_cos2=CM.min_cos2_of(10.0), min_overlap=0.5, start_distance=0.0, step_tolerance=1e-9, max_iterations=50,
                min_matches=8, estimate_scale=1)


def similarity(scale, q, t):
    return dict(scale=float(scale), q=tuple(float(v) for v in q), t=tuple(float(v) for v in t))


def unit(q):
    """q / sqrt(q.q)"""
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(((w * w + x * x) + y * y) + z * z)
    return (w / n, x / n, y / n, z / n)


def entry(T):
    """the similarity a call starts from: the quaternion normalised; None = identity"""
    if T is None:
        return similarity(**IDENTITY)
    return similarity(T["scale"], unit(T["q"]), T["t"])


def rotation(q):
    """R(q) of a unit quaternion: the nine expressions, row-major"""
    w, x, y, z = q
    return (1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y))


def point(scale, R, t, x0, x1, x2):
    """y_i = scale * ((R_i0 x0 + R_i1 x1) + R_i2 x2) + t_i; floats or arrays"""
    return tuple(scale * ((R[3 * i] * x0 + R[3 * i + 1] * x1) + R[3 * i + 2] * x2) + t[i] for i in range(3))


def transform(segs, T, form="array"):
    """both end points of every segment under T, whose quaternion is divided by its norm first -> [n, 6]"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    R = rotation(unit(T["q"]))
    s, t = float(T["scale"]), tuple(float(v) for v in T["t"])
    out = np.zeros_like(segs)
    if form == "scalar":
        for i in range(len(segs)):
            v = [float(c) for c in segs[i]]
            out[i] = point(s, R, t, *v[:3]) + point(s, R, t, *v[3:])
        return out
    for k in (0, 3):
        y = point(s, R, t, segs[:, k], segs[:, k + 1], segs[:, k + 2])
        for i in range(3):
            out[:, k + i] = y[i]
    return out


def matrix(T):
    """[[scale R(q), t], [0 0 0 1]]"""
    M = np.eye(4)
    M[:3, :3] = float(T["scale"]) * np.array(rotation(unit(T["q"]))).reshape(3, 3)
    M[:3, 3] = T["t"]
    return M


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def point_term(x, B, d, L2, c):
    """the 36 sums of one end point x of a matched query (H 28, b 7, cost); floats or arrays"""
    w = (x[0] - B[0], x[1] - B[1], x[2] - B[2])
    sw = dot3(d, w) / L2
    r = (w[0] - d[0] * sw, w[1] - d[1] * sw, w[2] - d[2] * sw)
    z = (x[0] - c[0], x[1] - c[1], x[2] - c[2])
    a = ((0.0, -z[2], z[1]), (z[2], 0.0, -z[0]), (-z[1], z[0], 0.0), (z[0], z[1], z[2]),
         (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    g = []
    for i in range(7):
        s = dot3(d, a[i]) / L2
        g.append((a[i][0] - d[0] * s, a[i][1] - d[1] * s, a[i][2] - d[2] * s))
    out = [dot3(g[i], g[j]) for i in range(7) for j in range(i, 7)]
    out += [dot3(g[i], r) for i in range(7)]
    out.append(dot3(r, r))
    return out


def query_terms(moved, r_segs, matches, c, form="array"):
    """[n_q, 37]: term(P1) + term(P2) and count 1.0 of a matched query, 37 times +0.0 of an unmatched one"""
    moved = np.asarray(moved, np.float64).reshape(-1, 6); r_segs = np.asarray(r_segs, np.float64).reshape(-1, 6)
    out = np.zeros((len(moved), TERMS))
    hit = np.flatnonzero(matches["segment"] >= 0)
    c = tuple(float(v) for v in c)
    if form == "scalar":
        for i in hit:
            ref = [float(v) for v in r_segs[matches["segment"][i]]]
            x = [float(v) for v in moved[i]]
            B = ref[:3]
            d = (ref[3] - B[0], ref[4] - B[1], ref[5] - B[2])
            L2 = dot3(d, d)
            t1 = point_term(x[:3], B, d, L2, c); t2 = point_term(x[3:], B, d, L2, c)
            out[i, :36] = [u + v for u, v in zip(t1, t2)]
            out[i, 36] = 1.0
        return out
    if len(hit):
        ref = r_segs[matches["segment"][hit]]
        B = (ref[:, 0], ref[:, 1], ref[:, 2])
        d = (ref[:, 3] - B[0], ref[:, 4] - B[1], ref[:, 5] - B[2])
        L2 = dot3(d, d)
        x = moved[hit]
        t1 = point_term((x[:, 0], x[:, 1], x[:, 2]), B, d, L2, c); t2 = point_term((x[:, 3], x[:, 4], x[:, 5]), B, d, L2, c)
        for k in range(36):
            out[hit, k] = t1[k] + t2[k]
        out[hit, 36] = 1.0
    return out


def tile_sums(terms):
    """the tree of k_align_normal: per tile of 256 queries (lanes past n_q hold +0.0) every wave of 64 folded by halves,
    stride 32 .. 1, then (W0 + W1) + (W2 + W3) -> [n_tiles, 37]"""
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


def host_sum(tiles):
    """the host's sum: from +0.0, tile after tile in ascending order"""
    s = np.zeros(TERMS)
    for t in tiles:
        s = s + t
    return s


ROW = (0, 7, 13, 18, 22, 25, 27)                 # where row i of the upper triangle begins


def solve(sums, estimate_scale):
    """H delta = -b by the Cholesky factorisation of the text -> delta (7 floats), or None at a pivot that is not finite
    and > 0.  Without the scale row and column 3 are left out and delta[3] = 0."""
    s = [float(v) for v in sums]
    idx = [i for i in range(7) if estimate_scale or i != 3]
    n = len(idx)

    def H(i, j):                                 # i <= j
        return s[ROW[idx[i]] + (idx[j] - idx[i])]
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
        v = -s[28 + idx[i]]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, n):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    delta = [0.0] * 7
    for i in range(n):
        delta[idx[i]] = x[i]
    return delta


def update(T, delta, c):
    """step 6: the transform after the update about c"""
    dq = unit((1.0, delta[0] * 0.5, delta[1] * 0.5, delta[2] * 0.5))
    dR = rotation(dq)
    m = 1.0 + delta[3]
    q = T["q"]
    qn = unit((((dq[0] * q[0] - dq[1] * q[1]) - dq[2] * q[2]) - dq[3] * q[3],
               ((dq[0] * q[1] + dq[1] * q[0]) + dq[2] * q[3]) - dq[3] * q[2],
               ((dq[0] * q[2] - dq[1] * q[3]) + dq[2] * q[0]) + dq[3] * q[1],
               ((dq[0] * q[3] + dq[1] * q[2]) - dq[2] * q[1]) + dq[3] * q[0]))
    u = (T["t"][0] - c[0], T["t"][1] - c[1], T["t"][2] - c[2])
    t = tuple((c[i] + m * ((dR[3 * i] * u[0] + dR[3 * i + 1] * u[1]) + dR[3 * i + 2] * u[2])) + delta[4 + i] for i in range(3))
    return similarity(T["scale"] * m, qn, t)


def step_of(delta, diag):
    return max(max(abs(v) for v in delta[:4]), max(abs(v) / diag for v in delta[4:]))


def bounding_box(r_segs):
    """(c, diag): the midpoint and the diagonal of the box of all end points"""
    pts = np.asarray(r_segs, np.float64).reshape(-1, 3)
    lo = [float(v) for v in pts.min(0)]; hi = [float(v) for v in pts.max(0)]
    c = tuple((lo[k] + hi[k]) * 0.5 for k in range(3))
    e = [hi[k] - lo[k] for k in range(3)]
    return c, math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])


def one_pass(q_segs, q_line, r_segs, r_line, T, gate, par, c, form):
    """steps 2-4 -> (moved, matches, sums)"""
    moved = transform(q_segs, T, form)
    cmp = CM.compare_scalar if form == "scalar" else CM.compare
    m = cmp(moved, q_line, r_segs, r_line, gate, par["min_cos2"], par["min_overlap"])
    return moved, m, host_sum(tile_sums(query_terms(moved, r_segs, m, c, form)))


def align(q_segs, q_line, r_segs, r_line, max_distance, initial=None, form="array", **kw):
    """what one call of the library returns, as a dict: similarity, summary (status as a name), segments, matches_q,
    matches_r, trace (ITERATION_DTYPE, one entry per iteration run)"""
    par = dict(DEFAULTS, max_distance=float(max_distance), **kw)
    q_segs = np.asarray(q_segs, np.float64).reshape(-1, 6); r_segs = np.asarray(r_segs, np.float64).reshape(-1, 6)
    q_line = np.asarray(q_line, np.uint32).reshape(-1); r_line = np.asarray(r_line, np.uint32).reshape(-1)
    T = entry(initial)
    trace = np.zeros(par["max_iterations"], ITERATION_DTYPE)
    if not len(q_segs) or not len(r_segs):
        c, diag = bounding_box(r_segs) if len(r_segs) else ((0.0, 0.0, 0.0), 0.0)
        return dict(similarity=T, summary=dict(status="TOO_FEW", iterations=0, n_matched=0, rms=0.0, last_step=0.0, diag=diag, center=c),
                    segments=transform(q_segs, T, form), matches_q=CM.nothing(len(q_segs)), matches_r=CM.nothing(len(r_segs)),
                    trace=trace[:0])
    c, diag = bounding_box(r_segs)
    assert diag > 0.0
    status, g, last_step, n_it = "MAX_ITERATIONS", float(par["start_distance"]), 0.0, 0
    for k in range(par["max_iterations"]):
        gate = max(par["max_distance"], g)
        g = g * 0.5
        _, _, sums = one_pass(q_segs, q_line, r_segs, r_line, T, gate, par, c, form)
        n_it = k + 1
        n_matched = int(sums[36])
        trace[k]["gate"] = gate; trace[k]["sums"] = sums; trace[k]["n_matched"] = n_matched
        delta = None
        if n_matched < par["min_matches"]:
            status = "TOO_FEW"
        else:
            delta = solve(sums, par["estimate_scale"])
            if delta is None:
                status = "DEGENERATE"
        if delta is not None:
            T = update(T, delta, c)
            last_step = step_of(delta, diag)
            trace[k]["delta"] = delta
        trace[k]["similarity"] = (T["scale"], T["q"], T["t"])
        if delta is None:
            break
        if gate == par["max_distance"] and last_step <= par["step_tolerance"]:
            status = "CONVERGED"
            break
    moved, mq, sums = one_pass(q_segs, q_line, r_segs, r_line, T, par["max_distance"], par, c, form)
    cmp = CM.compare_scalar if form == "scalar" else CM.compare
    mr = cmp(r_segs, r_line, moved, q_line, par["max_distance"], par["min_cos2"], par["min_overlap"])
    n_matched = int(sums[36])
    rms = math.sqrt(float(sums[35]) / (2.0 * float(sums[36]))) if n_matched else 0.0
    return dict(similarity=T, summary=dict(status=status, iterations=n_it, n_matched=n_matched, rms=rms, last_step=last_step, diag=diag, center=c),
                segments=moved, matches_q=mq, matches_r=mr, trace=trace[:n_it])


def end_point_error(segs, T, T_true, diag):
    """the largest distance between the end points under T and under T_true, as a share of diag"""
    a = transform(segs, T).reshape(-1, 3); b = transform(segs, T_true).reshape(-1, 3)
    return float(np.sqrt(((a - b) ** 2).sum(1)).max() / diag) if len(a) else 0.0
