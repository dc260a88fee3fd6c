"""The contract of DESIGN §17 (the 2D segments of a camera assigned to the projected 3D lines they observe) restated in
numpy: a scalar form that follows the text pair by pair, and an array form, chunked over the segments, for the large
cases.  tests/test_associate_host.py shows the two byte-identical.  All arithmetic is fp64 in the order of the text;
Python floats and numpy's element-wise float64 operations round every operation on its own (no contraction), as the
library does when built with -ffp-contract=off."""
import numpy as np

RECORD_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("inv_depth1", "<f4"),
                         ("inv_depth2", "<f4"), ("line", "<u4"), ("segment", "<u4")])
ASSOCIATION_DTYPE = np.dtype([("record", "<i4"), ("line", "<u4"), ("segment", "<u4"), ("distance", "<f4"),
                              ("overlap", "<f4"), ("n_accepted", "<u4")])
SEGMENT_MASK = 0x3FFFFFFF
NONE = 0xFFFFFFFF


def min_cos2_of(max_angle):
    """the squared cosine the wrappers hand to the library for an angle in degrees"""
    c = float(np.cos(np.radians(np.float64(max_angle))))
    return c * c


def nothing(n):
    out = np.zeros(n, ASSOCIATION_DTYPE)
    out["record"] = -1
    out["line"] = NONE
    out["segment"] = NONE
    return out


def pair(seg, r, max_distance, min_cos2, min_overlap):
    """steps 1-5 for one pair -> (accepted, D2, frac); seg = 4 float32, r = one record"""
    # 1. record vector and length
    ax, ay = float(r["x1"]), float(r["y1"])
    dx, dy = float(r["x2"]) - ax, float(r["y2"]) - ay
    L2 = dx * dx + dy * dy
    if L2 < 1.0:
        return False, 0.0, 0.0
    # 2. segment vector and length
    px, py, qx, qy = float(seg[0]), float(seg[1]), float(seg[2]), float(seg[3])
    ex, ey = qx - px, qy - py
    E2 = ex * ex + ey * ey
    if not E2 > 0.0:
        return False, 0.0, 0.0
    # 3. distance
    c1 = dx * (py - ay) - dy * (px - ax)
    c2 = dx * (qy - ay) - dy * (qx - ax)
    D2 = max(c1 * c1, c2 * c2) / L2
    if not D2 <= max_distance * max_distance:
        return False, D2, 0.0
    # 4. angle
    dot = dx * ex + dy * ey
    if not dot * dot >= min_cos2 * (L2 * E2):
        return False, D2, 0.0
    # 5. overlap
    t1 = (dx * (px - ax) + dy * (py - ay)) / L2
    t2 = (dx * (qx - ax) + dy * (qy - ay)) / L2
    lo, hi = min(t1, t2), max(t1, t2)
    ov = min(hi, 1.0) - max(lo, 0.0)
    if not ov > 0.0:
        return False, D2, 0.0
    frac = ov / (hi - lo)
    return frac >= min_overlap, D2, frac


def associate_scalar(rec, segs, max_distance, min_cos2, min_overlap):
    """one camera, pair by pair: rec = RECORD_DTYPE array, segs = float32 [M, 4] -> ASSOCIATION_DTYPE [M]"""
    segs = np.asarray(segs, np.float32).reshape(-1, 4)
    out = nothing(len(segs))
    for s in range(len(segs)):
        best = None
        n = 0
        for r in range(len(rec)):
            ok, D2, frac = pair(segs[s], rec[r], float(max_distance), float(min_cos2), float(min_overlap))
            if not ok:
                continue
            n += 1
            # D2 is a non-negative finite double: its bit pattern orders as an integer; of equal D2 the first stays
            bits = int(np.float64(D2).view(np.uint64))
            if best is None or bits < best[0]:
                best = (bits, r, D2, frac)
        if best is not None:
            _, r, D2, frac = best
            with np.errstate(over="ignore"):
                d2f = np.float32(D2)
            out[s] = (r, rec["line"][r], int(rec["segment"][r]) & SEGMENT_MASK, np.sqrt(d2f), np.float32(frac), n)
    return out


def associate(rec, segs, max_distance, min_cos2, min_overlap, chunk=1024):
    """the array form of associate_scalar: all records against `chunk` segments at a time"""
    segs = np.asarray(segs, np.float32).reshape(-1, 4)
    out = nothing(len(segs))
    if not len(rec) or not len(segs):
        return out
    md2 = np.float64(max_distance) * np.float64(max_distance)
    min_cos2 = np.float64(min_cos2); min_overlap = np.float64(min_overlap)
    ax = rec["x1"].astype(np.float64)[None, :]; ay = rec["y1"].astype(np.float64)[None, :]
    dx = rec["x2"].astype(np.float64)[None, :] - ax; dy = rec["y2"].astype(np.float64)[None, :] - ay
    L2 = dx * dx + dy * dy
    used = ~(L2 < 1.0)
    L2s = np.where(used, L2, 1.0)                          # (a record that supports nothing is masked, not divided by)
    for s0 in range(0, len(segs), chunk):
        sg = segs[s0:s0 + chunk].astype(np.float64)
        px, py, qx, qy = sg[:, 0:1], sg[:, 1:2], sg[:, 2:3], sg[:, 3:4]
        ex, ey = qx - px, qy - py
        E2 = ex * ex + ey * ey
        ok = used & (E2 > 0.0)
        c1 = dx * (py - ay) - dy * (px - ax)
        c2 = dx * (qy - ay) - dy * (qx - ax)
        D2 = np.maximum(c1 * c1, c2 * c2) / L2s
        ok &= D2 <= md2
        dot = dx * ex + dy * ey
        ok &= dot * dot >= min_cos2 * (L2 * E2)
        t1 = (dx * (px - ax) + dy * (py - ay)) / L2s
        t2 = (dx * (qx - ax) + dy * (qy - ay)) / L2s
        lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
        ov = np.minimum(hi, 1.0) - np.maximum(lo, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = ov / (hi - lo)
        ok &= (ov > 0.0) & (frac >= min_overlap)
        n = ok.sum(1)
        key = np.where(ok, D2, np.inf)
        best = key.argmin(1)                               # the first of equal minima: the smaller record index
        rows = np.flatnonzero(n > 0)
        b = best[rows]
        o = out[s0:s0 + len(sg)]
        o["record"][rows] = b
        o["line"][rows] = rec["line"][b]
        o["segment"][rows] = rec["segment"][b] & np.uint32(SEGMENT_MASK)
        with np.errstate(over="ignore"):
            o["distance"][rows] = np.sqrt(D2[rows, b].astype(np.float32))
        o["overlap"][rows] = frac[rows, b].astype(np.float32)
        o["n_accepted"] = n
    return out


def associate_cameras(recs, segs, max_distance, min_cos2, min_overlap, form=associate):
    return [form(r, s, max_distance, min_cos2, min_overlap) for r, s in zip(recs, segs)]
