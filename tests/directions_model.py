"""The contract of DESIGN §26 (the directions the 3D lines run in) restated in numpy, from its text.  Stage 0, the integer
weights, is §25's (tests/planes_model.weights); stages 1 and 2, the unit direction of every segment and the score of every
direction against every segment, in a scalar form over Python floats and in an array form chunked over the hypotheses
(tests/test_directions_host.py shows the two identical); stage 3, the selection, the refit and the frame, as plain loops
over Python floats.  All arithmetic is fp64 in the order of the text: Python floats and numpy's element-wise float64
operations round every operation on its own, as the library does when built with -ffp-contract=off; dot products are
written out left to right, cross products component by component, and sums over members run one after another in
ascending index order."""
import math

import numpy as np

from tests import planes_model as P
from tests import wireframe_model as W

SCORE_DTYPE = np.dtype([("weight", "<u8"), ("count", "<u4"), ("reserved", "<u4")])
DIRECTION_DTYPE = np.dtype([("hypothesis", "<u4"), ("n_segments", "<u4"), ("n_lines", "<u4"), ("reserved", "<u4"), ("weight", "<u8"),
                            ("D", "<f8", 3), ("length", "<f8"), ("rms_sin", "<f8"), ("D_fit", "<f8", 3), ("rms_sin_fit", "<f8"),
                            ("centroid", "<f8", 3), ("t_min", "<f8"), ("t_max", "<f8")])
MEMBER_DTYPE = np.dtype([("direction", "<u4"), ("segment", "<u4")])
SUMMARY_KEYS = ("n_segments", "n_point_segments", "n_candidates", "n_tested", "n_dropped", "n_rejected", "n_directions", "n_memberships",
                "n_segments_in_directions", "n_segments_in_several", "truncated", "scale_exponent", "length_total",
                "length_in_directions", "frame_axes", "frame", "R")
SUMMARY_FORMAT = "<11Qq2d4I9d"
NONE = 0xFFFFFFFF
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
assert SCORE_DTYPE.itemsize == 16 and DIRECTION_DTYPE.itemsize == 136 and MEMBER_DTYPE.itemsize == 8

sin2_of = W.min_sin2_of
extent = W.extent
weights = P.weights
dot = P.dot


def params(max_sin2, min_length=0.0, max_frame_cos2=None, min_segments=4, max_directions=16, max_tests=4096, frame_search=16):
    """the parameters as the model's functions take them: None = 5 degrees"""
    return dict(max_sin2=float(max_sin2), min_length=float(min_length),
                max_frame_cos2=float(sin2_of(5.0) if max_frame_cos2 is None else max_frame_cos2), min_segments=int(min_segments),
                max_directions=int(max_directions), max_tests=int(max_tests), frame_search=int(frame_search))


def cross(x, y):
    return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]


def sin2(x, y):
    X = cross(x, y)
    return dot(X, X)


# ---- stage 1 ----------------------------------------------------------------------------------------------------------
def units_scalar(segs):
    """-> [n, 3] float64: e / sqrt(E2) per component, 0 for a point"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    out = np.zeros((len(segs), 3))
    for k, v in enumerate(segs):
        e = [float(v[3 + c]) - float(v[c]) for c in range(3)]
        E2 = dot(e, e)
        if E2 > 0.0:
            root = math.sqrt(E2)
            out[k] = [e[c] / root for c in range(3)]
    return out


def units(segs):
    """the array form of units_scalar"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    with np.errstate(all="ignore"):
        e = [segs[:, 3 + c] - segs[:, c] for c in range(3)]
        E2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        live = E2 > 0.0
        root = np.sqrt(np.where(live, E2, 1.0))
        return np.stack([np.where(live, e[c] / root, 0.0) for c in range(3)], 1).reshape(-1, 3)


# ---- stage 2 ----------------------------------------------------------------------------------------------------------
def inliers(D, w, Dh, max_sin2):
    """the members of the direction Dh: the live segments with |Dh x D_s|^2 <= max_sin2, ascending.  D as lists of floats"""
    return [s for s in range(len(D)) if w["live"][s] and sin2(Dh, D[s]) <= max_sin2]


def scores_scalar(D, w, max_sin2):
    out = np.zeros(len(D), SCORE_DTYPE)
    rows = [[float(x) for x in d] for d in D]
    for h in range(len(rows)):
        if w["live"][h]:
            m = inliers(rows, w, rows[h], float(max_sin2))
            out[h]["count"] = len(m); out[h]["weight"] = sum(w["q"][s] for s in m)
    return out


def relation(D, w, max_sin2, h0=0, h1=None):
    """[h1 - h0, n] bool: segment s is an inlier of hypothesis h"""
    D = np.asarray(D, np.float64).reshape(-1, 3)
    live = np.asarray(w["live"], bool)
    H = D[h0:h1]
    with np.errstate(all="ignore"):
        hx, hy, hz = (H[:, c, None] for c in range(3))
        sx, sy, sz = (D[None, :, c] for c in range(3))
        X0 = hy * sz - hz * sy; X1 = hz * sx - hx * sz; X2 = hx * sy - hy * sx
        x2 = (X0 * X0 + X1 * X1) + X2 * X2
        return (x2 <= np.float64(max_sin2)) & live[None, :] & live[h0:h1, None]


def scores(D, w, max_sin2, chunk=256):
    """the array form of scores_scalar: `chunk` hypotheses against all segments at a time"""
    out = np.zeros(len(D), SCORE_DTYPE)
    if not len(D):
        return out
    q = np.asarray(w["q"], np.uint64)
    for h0 in range(0, len(D), chunk):
        ok = relation(D, w, max_sin2, h0, h0 + chunk)
        out["count"][h0:h0 + chunk] = ok.sum(1)
        out["weight"][h0:h0 + chunk] = (ok * q[None, :]).sum(1, dtype=np.uint64)
    return out


# ---- stage 3 ----------------------------------------------------------------------------------------------------------
def jacobi(S):
    """§25's Jacobi on S = (xx, xy, xz, yy, yz, zz) -> (A, V): the diagonal of A holds the eigenvalues, the columns of V the
    eigenvectors"""
    A = [[S[0], S[1], S[2]], [S[1], S[3], S[4]], [S[2], S[4], S[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(P.JACOBI_SWEEPS):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            root = math.sqrt(theta * theta + 1.0)
            t = 1.0 / (theta + root) if theta >= 0.0 else -1.0 / (root - theta)
            c = 1.0 / math.sqrt(t * t + 1.0); s = t * c
            A[p][p] = A[p][p] - t * apq
            A[q][q] = A[q][q] + t * apq
            A[p][q] = A[q][p] = 0.0
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
            for i in range(3):
                vip, viq = V[i][p], V[i][q]
                V[i][p] = c * vip - s * viq
                V[i][q] = s * vip + c * viq
    return A, V


def largest_eigenvector(S):
    """-> the unit eigenvector of the largest eigenvalue: the column of the largest diagonal entry, the first of equals"""
    A, V = jacobi(S)
    m = 0
    if A[1][1] > A[m][m]:
        m = 1
    if A[2][2] > A[m][m]:
        m = 2
    v = [V[0][m], V[1][m], V[2][m]]
    length = math.sqrt(dot(v, v))
    return [v[c] / length for c in range(3)]


def _rms_sin(D, mem, axis):
    acc = 0.0
    for s in mem:
        acc += sin2(axis, D[s])
    return math.sqrt(acc / float(len(mem)))


def describe(segs, line, w, D, h, weight, mem):
    """step 3: the record of an accepted direction; segs and D as lists of Python floats"""
    R = np.zeros((), DIRECTION_DTYPE)
    Dh = D[h]
    R["hypothesis"] = h; R["n_segments"] = len(mem); R["weight"] = weight; R["D"] = Dh
    R["n_lines"] = len({int(line[s]) for s in mem})
    length = 0.0
    for s in mem:
        length += w["len"][s]
    R["length"] = length
    R["rms_sin"] = _rms_sin(D, mem, Dh)
    S = [0.0] * 6
    for s in mem:
        d, L = D[s], w["len"][s]
        S[0] += L * (d[0] * d[0]); S[1] += L * (d[0] * d[1]); S[2] += L * (d[0] * d[2])
        S[3] += L * (d[1] * d[1]); S[4] += L * (d[1] * d[2]); S[5] += L * (d[2] * d[2])
    F = largest_eigenvector(S)
    if dot(F, Dh) < 0.0:
        F = [-x for x in F]
    R["D_fit"] = F; R["rms_sin_fit"] = _rms_sin(D, mem, F)
    count = 2.0 * float(len(mem))
    total = [0.0, 0.0, 0.0]
    for s in mem:
        for end in range(2):
            for c in range(3):
                total[c] += segs[s][3 * end + c]
    cen = [total[c] / count for c in range(3)]
    t = [dot([segs[s][3 * end + c] - cen[c] for c in range(3)], F) for s in mem for end in range(2)]
    R["centroid"] = cen; R["t_min"] = min(t); R["t_max"] = max(t)
    return R


def frame(directions, par):
    """step 5 -> (frame_axes, frame [3], R [9])"""
    if not len(directions):
        return 0, [NONE] * 3, list(IDENTITY)
    F = min(len(directions), par["frame_search"])
    fit = [[float(x) for x in d["D_fit"]] for d in directions[:F]]
    wt = [int(d["weight"]) for d in directions[:F]]

    def orthogonal(i, j):
        c = dot(fit[i], fit[j])
        return c * c <= par["max_frame_cos2"]
    triples = [(i, j, k) for i in range(F) for j in range(i + 1, F) for k in range(j + 1, F)
               if orthogonal(i, j) and orthogonal(i, k) and orthogonal(j, k)]
    pairs = [(i, j) for i in range(F) for j in range(i + 1, F) if orthogonal(i, j)]
    pick = (0,)
    for found in (triples, pairs):
        if found:
            pick = min(found, key=lambda t: (-sum(wt[i] for i in t), t))         # the heaviest; among equals the first
            break
    x = fit[pick[0]]
    if len(pick) >= 2:
        second = fit[pick[1]]
    else:
        m = 0
        for c in (1, 2):
            if abs(x[c]) < abs(x[m]):
                m = c
        second = [1.0 if c == m else 0.0 for c in range(3)]
    along = dot(second, x)
    yp = [second[c] - along * x[c] for c in range(3)]
    length = math.sqrt(dot(yp, yp))
    y = [yp[c] / length for c in range(3)]
    return len(pick), list(pick) + [NONE] * (3 - len(pick)), x + y + cross(x, y)


def empty_summary():
    s = dict.fromkeys(SUMMARY_KEYS[:12], 0)
    s.update(length_total=0.0, length_in_directions=0.0, frame_axes=0, frame=[NONE] * 3, R=list(IDENTITY))
    return s


def select(segs, line, w, score, par):
    """stage 3 -> dict(directions, members, seg_directions, scores, summary, R)"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    n = len(segs)
    rows = [[float(x) for x in v] for v in segs]
    D = [[float(x) for x in d] for d in units_scalar(segs)]
    s = empty_summary()
    s.update(n_segments=n, n_point_segments=w["n_points"], scale_exponent=w["e"], length_total=w["length_total"])
    cand = [h for h in range(n) if w["live"][h] and int(score[h]["count"]) >= par["min_segments"]
            and math.ldexp(float(int(score[h]["weight"])), -w["e"]) >= par["min_length"]]
    s["n_candidates"] = len(cand)
    cand.sort(key=lambda h: (-int(score[h]["weight"]), -int(score[h]["count"]), h))
    directions, members, in_dir = [], [], []
    seg_directions = np.zeros(n, np.uint32)
    for h in cand:
        if len(directions) >= par["max_directions"]:
            break
        if any(h in m for m in in_dir):
            s["n_dropped"] += 1
            continue
        if s["n_tested"] == par["max_tests"]:
            s["truncated"] = 1
            break
        s["n_tested"] += 1
        mem = inliers(D, w, D[h], par["max_sin2"])
        weight = sum(w["q"][i] for i in mem)
        assert len(mem) == int(score[h]["count"]) and weight == int(score[h]["weight"]), h
        if any(2 * sum(w["q"][i] for i in mem if i in m) > weight for m in in_dir):
            s["n_rejected"] += 1
            continue
        directions.append(describe(rows, line, w, D, h, weight, mem))
        in_dir.append(set(mem))
        members += [(len(directions) - 1, i) for i in mem]
        seg_directions[mem] += 1
    directions = np.array(directions, DIRECTION_DTYPE).reshape(-1)
    s["frame_axes"], s["frame"], s["R"] = frame(directions, par)
    s["n_directions"] = len(directions); s["n_memberships"] = len(members)
    s["n_segments_in_directions"] = int((seg_directions > 0).sum()); s["n_segments_in_several"] = int((seg_directions > 1).sum())
    for i in np.flatnonzero(seg_directions):
        s["length_in_directions"] += w["len"][i]
    return dict(directions=directions, members=np.array(members, MEMBER_DTYPE).reshape(-1), seg_directions=seg_directions,
                scores=np.asarray(score, SCORE_DTYPE), summary=s, R=np.array(s["R"], np.float64).reshape(3, 3))


def detect(segs, line, par, form="array"):
    """the whole of §26 -> the dict of select; form: "array" or "scalar" for stages 1 and 2"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6); line = np.asarray(line, np.uint32).reshape(-1)
    if not len(segs):
        return dict(directions=np.zeros(0, DIRECTION_DTYPE), members=np.zeros(0, MEMBER_DTYPE), seg_directions=np.zeros(0, np.uint32),
                    scores=np.zeros(0, SCORE_DTYPE), summary=empty_summary(), R=np.eye(3))
    w = weights(segs)
    if form == "array":
        score = scores(units(segs), w, par["max_sin2"])
    else:
        score = scores_scalar(units_scalar(segs), w, par["max_sin2"])
    return select(segs, line, w, score, par)


def pack_summary(s):
    """the 200 bytes of l3d_directions_summary"""
    import struct
    return struct.pack(SUMMARY_FORMAT, *[s[k] for k in SUMMARY_KEYS[:15]], *s["frame"], *s["R"])


def obj_text(result):
    out = []
    for k, p in enumerate(result["directions"]):
        c = [float(x) for x in p["centroid"]]; d = [float(x) for x in p["D_fit"]]
        for t in (float(p["t_min"]), float(p["t_max"])):
            out.append("v %.17g %.17g %.17g\n" % (c[0] + t * d[0], c[1] + t * d[1], c[2] + t * d[2]))
        out.append("l %d %d\n" % (2 * k + 1, 2 * k + 2))
    return "".join(out)
