"""The contract of DESIGN §18 (two 3D line models compared segment by segment) restated in numpy: a scalar form that
follows the text pair by pair, and an array form, chunked over the queries, for the large cases.
tests/test_compare_host.py shows the two byte-identical.  All arithmetic is fp64 in the order of the text; Python floats
and numpy's element-wise float64 operations round every operation on its own (no contraction), as the library does when
built with -ffp-contract=off.  Sums of three products are written out left to right."""
import numpy as np

LINE_MATCH_DTYPE = np.dtype([("segment", "<i4"), ("line", "<u4"), ("n_accepted", "<u4"), ("overlap", "<f4"),
                             ("distance", "<f8")])
NONE = 0xFFFFFFFF
SUMMARY_KEYS = ("n_segments", "n_matched", "n_ambiguous", "n_lines", "n_lines_matched", "length_total", "length_matched")


def min_cos2_of(max_angle):
    """the squared cosine the wrappers hand to the library for an angle in degrees"""
    c = float(np.cos(np.radians(np.float64(max_angle))))
    return c * c


def nothing(n):
    out = np.zeros(n, LINE_MATCH_DTYPE)
    out["segment"] = -1
    out["line"] = NONE
    return out


def pair(q, q_line, r, r_line, max_distance, min_cos2, min_overlap, exclude_same_line):
    """steps 1-6 for one pair -> (accepted, D2, frac); q, r = 6 doubles (P1, P2)"""
    # 1. reference vector and length
    bx, by, bz = float(r[0]), float(r[1]), float(r[2])
    dx, dy, dz = float(r[3]) - bx, float(r[4]) - by, float(r[5]) - bz
    L2 = dx * dx + dy * dy + dz * dz
    if not L2 > 0.0:
        return False, 0.0, 0.0
    # 2. query vector and length
    px, py, pz = float(q[0]), float(q[1]), float(q[2])
    sx, sy, sz = float(q[3]), float(q[4]), float(q[5])
    ex, ey, ez = sx - px, sy - py, sz - pz
    E2 = ex * ex + ey * ey + ez * ez
    if not E2 > 0.0:
        return False, 0.0, 0.0
    # 3. the same line
    if exclude_same_line and int(q_line) == int(r_line):
        return False, 0.0, 0.0
    # 4. angle
    dot = dx * ex + dy * ey + dz * ez
    if not dot * dot >= min_cos2 * (L2 * E2):
        return False, 0.0, 0.0
    # 5. distance
    wx, wy, wz = px - bx, py - by, pz - bz
    ux, uy, uz = sx - bx, sy - by, sz - bz
    c1 = (dy * wz - dz * wy, dz * wx - dx * wz, dx * wy - dy * wx)
    c2 = (dy * uz - dz * uy, dz * ux - dx * uz, dx * uy - dy * ux)
    m1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]
    m2 = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]
    D2 = max(m1, m2) / L2
    if not D2 <= max_distance * max_distance:
        return False, D2, 0.0
    # 6. overlap
    t1 = (dx * wx + dy * wy + dz * wz) / L2
    t2 = (dx * ux + dy * uy + dz * uz) / L2
    lo, hi = min(t1, t2), max(t1, t2)
    ov = min(hi, 1.0) - max(lo, 0.0)
    if not ov > 0.0:
        return False, D2, 0.0
    frac = ov / (hi - lo)
    return frac >= min_overlap, D2, frac


def compare_scalar(q_segs, q_line, r_segs, r_line, max_distance, min_cos2, min_overlap, exclude_same_line=False):
    """one direction, pair by pair -> LINE_MATCH_DTYPE [n_q]"""
    q_segs = np.asarray(q_segs, np.float64).reshape(-1, 6); r_segs = np.asarray(r_segs, np.float64).reshape(-1, 6)
    out = nothing(len(q_segs))
    for s in range(len(q_segs)):
        best = None
        n = 0
        for r in range(len(r_segs)):
            ok, D2, frac = pair(q_segs[s], q_line[s], r_segs[r], r_line[r], float(max_distance), float(min_cos2),
                                float(min_overlap), exclude_same_line)
            if not ok:
                continue
            n += 1
            # D2 is a non-negative finite double: its bit pattern orders as an integer; of equal D2 the first stays
            bits = int(np.float64(D2).view(np.uint64))
            if best is None or bits < best[0]:
                best = (bits, r, D2, frac)
        if best is not None:
            _, r, D2, frac = best
            out[s] = (r, r_line[r], n, np.float32(frac), np.sqrt(np.float64(D2)))
    return out


def compare(q_segs, q_line, r_segs, r_line, max_distance, min_cos2, min_overlap, exclude_same_line=False, chunk=512):
    """the array form of compare_scalar: all references against `chunk` queries at a time"""
    q_segs = np.asarray(q_segs, np.float64).reshape(-1, 6); r_segs = np.asarray(r_segs, np.float64).reshape(-1, 6)
    q_line = np.asarray(q_line, np.uint32).reshape(-1); r_line = np.asarray(r_line, np.uint32).reshape(-1)
    out = nothing(len(q_segs))
    if not len(r_segs) or not len(q_segs):
        return out
    md2 = np.float64(max_distance) * np.float64(max_distance)
    min_cos2 = np.float64(min_cos2); min_overlap = np.float64(min_overlap)
    bx, by, bz = r_segs[None, :, 0], r_segs[None, :, 1], r_segs[None, :, 2]
    dx, dy, dz = r_segs[None, :, 3] - bx, r_segs[None, :, 4] - by, r_segs[None, :, 5] - bz
    L2 = dx * dx + dy * dy + dz * dz
    used = L2 > 0.0
    L2s = np.where(used, L2, 1.0)                          # (a reference that matches nothing is masked, not divided by)
    for s0 in range(0, len(q_segs), chunk):
        sg = q_segs[s0:s0 + chunk]
        px, py, pz, sx, sy, sz = (sg[:, k:k + 1] for k in range(6))
        ex, ey, ez = sx - px, sy - py, sz - pz
        E2 = ex * ex + ey * ey + ez * ez
        ok = used & (E2 > 0.0)
        if exclude_same_line:
            ok &= q_line[s0:s0 + chunk, None] != r_line[None, :]
        dot = dx * ex + dy * ey + dz * ez
        ok &= dot * dot >= min_cos2 * (L2 * E2)
        wx, wy, wz = px - bx, py - by, pz - bz
        ux, uy, uz = sx - bx, sy - by, sz - bz
        c1x, c1y, c1z = dy * wz - dz * wy, dz * wx - dx * wz, dx * wy - dy * wx
        c2x, c2y, c2z = dy * uz - dz * uy, dz * ux - dx * uz, dx * uy - dy * ux
        m1 = c1x * c1x + c1y * c1y + c1z * c1z
        m2 = c2x * c2x + c2y * c2y + c2z * c2z
        D2 = np.maximum(m1, m2) / L2s
        ok &= D2 <= md2
        t1 = (dx * wx + dy * wy + dz * wz) / L2s
        t2 = (dx * ux + dy * uy + dz * uz) / L2s
        lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
        ov = np.minimum(hi, 1.0) - np.maximum(lo, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = ov / (hi - lo)
        ok &= (ov > 0.0) & (frac >= min_overlap)
        n = ok.sum(1)
        key = np.where(ok, D2, np.inf)
        best = key.argmin(1)                               # the first of equal minima: the smaller reference index
        rows = np.flatnonzero(n > 0)
        b = best[rows]
        o = out[s0:s0 + len(sg)]
        o["segment"][rows] = b
        o["line"][rows] = r_line[b]
        o["distance"][rows] = np.sqrt(D2[rows, b])
        o["overlap"][rows] = frac[rows, b].astype(np.float32)
        o["n_accepted"] = n
    return out


def summary(q_segs, q_line, matches):
    """l3d_compare_summary of one direction as a dict; the lengths are added one after another in ascending index order"""
    q_segs = np.asarray(q_segs, np.float64).reshape(-1, 6); q_line = np.asarray(q_line, np.uint32).reshape(-1)
    e = q_segs[:, 3:6] - q_segs[:, 0:3]
    length = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
    matched = matches["segment"] >= 0
    total = np.cumsum(length)                              # (sequential; np.sum adds pairwise)
    got = np.cumsum(length[matched])
    return dict(n_segments=len(q_segs), n_matched=int(matched.sum()), n_ambiguous=int((matches["n_accepted"] > 1).sum()),
                n_lines=len(np.unique(q_line)), n_lines_matched=len(np.unique(q_line[matched])),
                length_total=float(total[-1]) if len(total) else 0.0, length_matched=float(got[-1]) if len(got) else 0.0)


def compare_both(q_segs, q_line, r_segs, r_line, max_distance, min_cos2, min_overlap, exclude_same_line=False, form=compare):
    """what one call of the library returns: (matches_q, matches_r, summary_q, summary_r); with an empty side the
    summaries are all zero"""
    mq = form(q_segs, q_line, r_segs, r_line, max_distance, min_cos2, min_overlap, exclude_same_line)
    mr = form(r_segs, r_line, q_segs, q_line, max_distance, min_cos2, min_overlap, exclude_same_line)
    if not len(mq) or not len(mr):
        zero = dict.fromkeys(SUMMARY_KEYS, 0)
        zero["length_total"] = zero["length_matched"] = 0.0
        return mq, mr, dict(zero), dict(zero)
    return mq, mr, summary(q_segs, q_line, mq), summary(r_segs, r_line, mr)


def extent(segs):
    """the norm of the 95th minus the 5th percentile of the end points (as tests/test_gpu_parity.py defines it)"""
    pts = np.asarray(segs, np.float64).reshape(-1, 3)
    return float(np.linalg.norm(np.percentile(pts, 95, axis=0) - np.percentile(pts, 5, axis=0)))
