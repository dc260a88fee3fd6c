"""The contract of DESIGN §25 (the planes the 3D lines lie in) restated in numpy, from its text.  Stage 0, the integer
weights; stages 1 and 2, the plane of every junction and its score against every segment, in a scalar form over Python
floats and in an array form chunked over the hypotheses (tests/test_planes_host.py shows the two identical); stage 3, the
selection, as plain loops over Python floats.  The junctions are those of tests/wireframe_model.py.  All arithmetic is
fp64 in the order of the text: Python floats and numpy's element-wise float64 operations round every operation on its
own, as the library does when built with -ffp-contract=off; dot products are written out left to right and sums over
members run one after another in ascending index order."""
import math

import numpy as np

from tests import wireframe_model as W

HYP_DTYPE = np.dtype([("N", "<f8", 3), ("J", "<f8", 3), ("a", "<u4"), ("b", "<u4"), ("live", "<u4"), ("pad", "<u4")])
SCORE_DTYPE = np.dtype([("weight", "<u8"), ("count", "<u4"), ("reserved", "<u4")])
PLANE_DTYPE = np.dtype([("hypothesis", "<u4"), ("a", "<u4"), ("b", "<u4"), ("n_segments", "<u4"), ("n_lines", "<u4"), ("reserved", "<u4"),
                        ("weight", "<u8"), ("N", "<f8", 3), ("J", "<f8", 3), ("d", "<f8"), ("length", "<f8"), ("rms", "<f8"),
                        ("centroid", "<f8", 3), ("N_fit", "<f8", 3), ("d_fit", "<f8"), ("rms_fit", "<f8"), ("corners", "<f8", (4, 3))])
MEMBER_DTYPE = np.dtype([("plane", "<u4"), ("segment", "<u4")])
SUMMARY_KEYS = ("n_segments", "n_point_segments", "n_hypotheses", "n_dead", "n_candidates", "n_tested", "n_dropped", "n_rejected",
                "n_planes", "n_memberships", "n_segments_in_planes", "n_segments_in_several", "truncated", "scale_exponent",
                "length_total", "length_in_planes", "max_rms")
SUMMARY_FORMAT = "<13Qq3d"
JACOBI_SWEEPS = 8
assert HYP_DTYPE.itemsize == 64 and SCORE_DTYPE.itemsize == 16 and PLANE_DTYPE.itemsize == 264 and MEMBER_DTYPE.itemsize == 8

min_sin2_of = W.min_sin2_of
extent = W.extent


def params(max_distance, junction_distance=None, junction_extension=None, min_sin2=None, min_length=0.0, min_segments=4,
           max_planes=64, max_tests=4096):
    """the parameters as the model's functions take them: None = max_distance, 10 degrees"""
    return dict(max_distance=float(max_distance), junction_distance=float(max_distance if junction_distance is None else junction_distance),
                junction_extension=float(max_distance if junction_extension is None else junction_extension),
                min_sin2=float(min_sin2_of(10.0) if min_sin2 is None else min_sin2), min_length=float(min_length),
                min_segments=int(min_segments), max_planes=int(max_planes), max_tests=int(max_tests))


def dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


# ---- stage 0 ----------------------------------------------------------------------------------------------------------
def weights(segs):
    """-> dict(len [n] floats, q [n] ints, live [n] bools, length_total, e, n_points)"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    length, live, total = [], [], 0.0
    for v in segs:
        e = [float(v[3 + c]) - float(v[c]) for c in range(3)]
        E2 = dot(e, e)
        length.append(math.sqrt(E2)); live.append(E2 > 0.0)
        total += length[-1]
    if not len(segs):
        return dict(len=[], q=[], live=[], length_total=0.0, e=0, n_points=0)
    e = 52 - math.frexp(total)[1]
    q = [int(math.floor(math.ldexp(L, e))) if ok else 0 for L, ok in zip(length, live)]
    assert sum(q) < 1 << 53
    return dict(len=length, q=q, live=live, length_total=total, e=e, n_points=live.count(False))


# ---- stage 1 ----------------------------------------------------------------------------------------------------------
def hypotheses_scalar(segs, rec):
    """the plane of every junction record, one by one -> HYP_DTYPE array"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    out = np.zeros(len(rec), HYP_DTYPE)
    for k, r in enumerate(rec):
        va, vb = [float(x) for x in segs[r["a"]]], [float(x) for x in segs[r["b"]]]
        sa, sb = float(r["sa"]), float(r["sb"])
        ea = [va[3 + c] - va[c] for c in range(3)]; eb = [vb[3 + c] - vb[c] for c in range(3)]
        J = [((va[c] + sa * ea[c]) + (vb[c] + sb * eb[c])) * 0.5 for c in range(3)]
        M = [ea[1] * eb[2] - ea[2] * eb[1], ea[2] * eb[0] - ea[0] * eb[2], ea[0] * eb[1] - ea[1] * eb[0]]
        m2 = dot(M, M)
        out[k]["a"] = r["a"]; out[k]["b"] = r["b"]
        if m2 > 0.0 and math.isfinite(m2):
            root = math.sqrt(m2)
            out[k]["N"] = [M[c] / root for c in range(3)]; out[k]["J"] = J; out[k]["live"] = 1
    return out


def hypotheses(segs, rec):
    """the array form of hypotheses_scalar"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    out = np.zeros(len(rec), HYP_DTYPE)
    if not len(rec):
        return out
    va, vb = segs[rec["a"]], segs[rec["b"]]
    with np.errstate(all="ignore"):
        ea = [va[:, 3 + c] - va[:, c] for c in range(3)]; eb = [vb[:, 3 + c] - vb[:, c] for c in range(3)]
        J = [((va[:, c] + rec["sa"] * ea[c]) + (vb[:, c] + rec["sb"] * eb[c])) * 0.5 for c in range(3)]
        M = [ea[1] * eb[2] - ea[2] * eb[1], ea[2] * eb[0] - ea[0] * eb[2], ea[0] * eb[1] - ea[1] * eb[0]]
        m2 = (M[0] * M[0] + M[1] * M[1]) + M[2] * M[2]
        live = (m2 > 0.0) & np.isfinite(m2)
        root = np.sqrt(np.where(live, m2, 1.0))
        for c in range(3):
            out["N"][:, c] = np.where(live, M[c] / root, 0.0); out["J"][:, c] = np.where(live, J[c], 0.0)
    out["a"] = rec["a"]; out["b"] = rec["b"]; out["live"] = live
    return out


# ---- stage 2 ----------------------------------------------------------------------------------------------------------
def inliers(segs, w, N, J, max_distance):
    """the members of the plane (N, J): the live segments with both end points within max_distance, ascending"""
    N = [float(x) for x in N]; J = [float(x) for x in J]
    out = []
    for s, v in enumerate(segs):
        if not w["live"][s]:
            continue
        h1 = dot(N, [float(v[c]) - J[c] for c in range(3)]); h2 = dot(N, [float(v[3 + c]) - J[c] for c in range(3)])
        if abs(h1) <= max_distance and abs(h2) <= max_distance:
            out.append(s)
    return out


def scores_scalar(segs, w, hyp, max_distance):
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    out = np.zeros(len(hyp), SCORE_DTYPE)
    for k, h in enumerate(hyp):
        if h["live"]:
            m = inliers(segs, w, h["N"], h["J"], float(max_distance))
            out[k]["count"] = len(m); out[k]["weight"] = sum(w["q"][s] for s in m)
    return out


def scores(segs, w, hyp, max_distance, chunk=256):
    """the array form of scores_scalar: `chunk` hypotheses against all segments at a time"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    out = np.zeros(len(hyp), SCORE_DTYPE)
    if not len(hyp) or not len(segs):
        return out
    md = np.float64(max_distance)
    live_s = np.asarray(w["live"], bool)[None, :]
    q = np.asarray(w["q"], np.uint64)
    with np.errstate(all="ignore"):
        for h0 in range(0, len(hyp), chunk):
            H = hyp[h0:h0 + chunk]
            N = [H["N"][:, c, None] for c in range(3)]; J = [H["J"][:, c, None] for c in range(3)]
            h1 = (N[0] * (segs[None, :, 0] - J[0]) + N[1] * (segs[None, :, 1] - J[1])) + N[2] * (segs[None, :, 2] - J[2])
            h2 = (N[0] * (segs[None, :, 3] - J[0]) + N[1] * (segs[None, :, 4] - J[1])) + N[2] * (segs[None, :, 5] - J[2])
            ok = (np.abs(h1) <= md) & (np.abs(h2) <= md) & live_s & (H["live"][:, None] != 0)
            out["count"][h0:h0 + chunk] = ok.sum(1)
            out["weight"][h0:h0 + chunk] = (ok * q[None, :]).sum(1, dtype=np.uint64)
    return out


# ---- stage 3 ----------------------------------------------------------------------------------------------------------
def smallest_eigenvector(S):
    """S = (xx, xy, xz, yy, yz, zz) -> the unit eigenvector of the smallest eigenvalue, by JACOBI_SWEEPS cyclic sweeps"""
    A = [[S[0], S[1], S[2]], [S[1], S[3], S[4]], [S[2], S[4], S[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(JACOBI_SWEEPS):
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
    m = 0
    if A[1][1] < A[m][m]:
        m = 1
    if A[2][2] < A[m][m]:
        m = 2
    v = [V[0][m], V[1][m], V[2][m]]
    length = math.sqrt(dot(v, v))
    return [v[c] / length for c in range(3)]


def _rms(segs, mem, N, O):
    acc = 0.0
    for s in mem:
        v = segs[s]
        h1 = dot(N, [v[c] - O[c] for c in range(3)]); h2 = dot(N, [v[3 + c] - O[c] for c in range(3)])
        acc += h1 * h1 + h2 * h2
    return math.sqrt(acc / (2.0 * float(len(mem))))


def describe(segs, line, w, index, h, weight, mem):
    """step 3: the record of an accepted plane; segs as lists of Python floats"""
    P = np.zeros((), PLANE_DTYPE)
    N = [float(x) for x in h["N"]]; J = [float(x) for x in h["J"]]
    P["hypothesis"] = index; P["a"] = h["a"]; P["b"] = h["b"]; P["n_segments"] = len(mem); P["weight"] = weight
    P["N"] = N; P["J"] = J; P["d"] = dot(N, J)
    P["n_lines"] = len({int(line[s]) for s in mem})
    length = 0.0
    for s in mem:
        length += w["len"][s]
    P["length"] = length
    P["rms"] = _rms(segs, mem, N, J)
    count = 2.0 * float(len(mem))
    total = [0.0, 0.0, 0.0]
    for s in mem:
        for end in range(2):
            for c in range(3):
                total[c] += segs[s][3 * end + c]
    cen = [total[c] / count for c in range(3)]
    S = [0.0] * 6
    for s in mem:
        for end in range(2):
            d = [segs[s][3 * end + c] - cen[c] for c in range(3)]
            S[0] += d[0] * d[0]; S[1] += d[0] * d[1]; S[2] += d[0] * d[2]; S[3] += d[1] * d[1]; S[4] += d[1] * d[2]; S[5] += d[2] * d[2]
    F = smallest_eigenvector(S)
    if not dot(F, N) >= 0.0:
        F = [-x for x in F]
    P["centroid"] = cen; P["N_fit"] = F; P["d_fit"] = dot(F, cen); P["rms_fit"] = _rms(segs, mem, F, cen)
    va = segs[int(h["a"])]
    ea = [va[3 + c] - va[c] for c in range(3)]
    La = math.sqrt(dot(ea, ea))
    U = [ea[c] / La for c in range(3)]
    V = [N[1] * U[2] - N[2] * U[1], N[2] * U[0] - N[0] * U[2], N[0] * U[1] - N[1] * U[0]]
    cu, cv = [], []
    for s in mem:
        for end in range(2):
            u = [segs[s][3 * end + c] - J[c] for c in range(3)]
            cu.append(dot(u, U)); cv.append(dot(u, V))
    for k, (x, y) in enumerate(((min(cu), min(cv)), (max(cu), min(cv)), (max(cu), max(cv)), (min(cu), max(cv)))):
        P["corners"][k] = [(J[c] + x * U[c]) + y * V[c] for c in range(3)]
    return P


def select(segs, line, w, hyp, score, par):
    """stage 3 -> dict(planes, members, seg_planes, scores, summary)"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    n = len(segs)
    rows = [[float(x) for x in v] for v in segs]
    s = dict.fromkeys(SUMMARY_KEYS, 0)
    s.update(n_segments=n, n_point_segments=w["n_points"], n_hypotheses=len(hyp), scale_exponent=w["e"], length_total=w["length_total"],
             length_in_planes=0.0, max_rms=0.0)
    cand = []
    for h in range(len(hyp)):
        if not hyp[h]["live"]:
            s["n_dead"] += 1
        elif int(score[h]["count"]) >= par["min_segments"] and math.ldexp(float(int(score[h]["weight"])), -w["e"]) >= par["min_length"]:
            cand.append(h)
    s["n_candidates"] = len(cand)
    cand.sort(key=lambda h: (-int(score[h]["weight"]), -int(score[h]["count"]), h))
    planes, members, in_plane = [], [], []
    seg_planes = np.zeros(n, np.uint32)
    for h in cand:
        if len(planes) >= par["max_planes"]:
            break
        a, b = int(hyp[h]["a"]), int(hyp[h]["b"])
        if any(a in m and b in m for m in in_plane):
            s["n_dropped"] += 1
            continue
        if s["n_tested"] == par["max_tests"]:
            s["truncated"] = 1
            break
        s["n_tested"] += 1
        mem = inliers(rows, w, hyp[h]["N"], hyp[h]["J"], par["max_distance"])
        weight = sum(w["q"][i] for i in mem)
        assert len(mem) == int(score[h]["count"]) and weight == int(score[h]["weight"]), h
        if any(2 * sum(w["q"][i] for i in mem if i in m) > weight for m in in_plane):
            s["n_rejected"] += 1
            continue
        planes.append(describe(rows, line, w, h, hyp[h], weight, mem))
        in_plane.append(set(mem))
        members += [(len(planes) - 1, i) for i in mem]
        seg_planes[mem] += 1
        s["max_rms"] = max(s["max_rms"], float(planes[-1]["rms"]))
    s["n_planes"] = len(planes); s["n_memberships"] = len(members)
    s["n_segments_in_planes"] = int((seg_planes > 0).sum()); s["n_segments_in_several"] = int((seg_planes > 1).sum())
    for i in np.flatnonzero(seg_planes):
        s["length_in_planes"] += w["len"][i]
    return dict(planes=np.array(planes, PLANE_DTYPE).reshape(-1), members=np.array(members, MEMBER_DTYPE).reshape(-1),
                seg_planes=seg_planes, scores=np.asarray(score, SCORE_DTYPE), summary=s)


def detect(segs, line, par, form="array"):
    """the whole of §25 -> the dict of select; form: "array" or "scalar" for stages 1 and 2"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6); line = np.asarray(line, np.uint32).reshape(-1)
    if not len(segs):
        return dict(planes=np.zeros(0, PLANE_DTYPE), members=np.zeros(0, MEMBER_DTYPE), seg_planes=np.zeros(0, np.uint32),
                    scores=np.zeros(0, SCORE_DTYPE), summary=dict.fromkeys(SUMMARY_KEYS[:-3], 0) | dict.fromkeys(SUMMARY_KEYS[-3:], 0.0))
    w = weights(segs)
    stage1 = W.junctions if form == "array" else W.junctions_scalar
    rec = stage1(segs, line, par["junction_distance"], par["junction_extension"], par["min_sin2"])
    hyp = (hypotheses if form == "array" else hypotheses_scalar)(segs, rec)
    score = (scores if form == "array" else scores_scalar)(segs, w, hyp, par["max_distance"])
    return select(segs, line, w, hyp, score, par)


def obj_text(result):
    out = []
    for k, p in enumerate(result["planes"]):
        out += ["v %.17g %.17g %.17g\n" % tuple(float(x) for x in c) for c in p["corners"]]
        out.append("f %d %d %d %d\n" % (4 * k + 1, 4 * k + 2, 4 * k + 3, 4 * k + 4))
    return "".join(out)
