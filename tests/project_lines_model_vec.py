"""Array forms of the numpy model of DESIGN §16 (tests/project_lines_model.py), for inputs the loop model is too slow for:
the same float64 operations in the same order, the branches as np.where, stage 2 by expanding the major-axis steps with
np.repeat and taking np.maximum.at on a plane of 64-bit keys.  The loop model stays the contract: this file is admitted
as a checker only because tests/test_project_host.py shows it byte-identical to the loop model, on every case the loop
model is used for and on samples of the large cases."""
import numpy as np

from tests import project_lines_model as M

f8 = np.float64


def mul33(A, v):
    """(a0 x + a1 y) + a2 z per row, v = three arrays"""
    A = np.asarray(A, f8).reshape(9)
    return [(A[3 * i] * v[0] + A[3 * i + 1] * v[1]) + A[3 * i + 2] * v[2] for i in range(3)]


def project_point(K, X):
    q = mul33(K, [X[0] / X[2], X[1] / X[2], np.ones_like(X[2])])
    return q[0] / q[2], q[1] / q[2], f8(1.0) / X[2]


def project_camera(cam, P1, P2, line_of_segment, near=1e-6):
    """stage 1 for one camera and all segments -> RECORD_DTYPE array, visible records in ascending segment order"""
    K, R, t = (np.asarray(cam[k], f8).reshape(-1) for k in ("K", "R", "t"))
    near = f8(near)
    P1 = np.asarray(P1, f8).reshape(-1, 3); P2 = np.asarray(P2, f8).reshape(-1, 3)
    n = len(P1)
    with np.errstate(all="ignore"):
        X1 = [rp + t[i] for i, rp in enumerate(mul33(R, [P1[:, 0], P1[:, 1], P1[:, 2]]))]
        X2 = [rp + t[i] for i, rp in enumerate(mul33(R, [P2[:, 0], P2[:, 1], P2[:, 2]]))]
        b1, b2 = X1[2] < near, X2[2] < near
        visible = ~(b1 & b2)
        c1, c2 = b1 & ~b2, b2 & ~b1
        s1 = (near - X1[2]) / (X2[2] - X1[2])
        s2 = (near - X2[2]) / (X1[2] - X2[2])
        Y1 = [np.where(c1, X1[0] + s1 * (X2[0] - X1[0]), X1[0]), np.where(c1, X1[1] + s1 * (X2[1] - X1[1]), X1[1]),
              np.where(c1, near, X1[2])]
        Y2 = [np.where(c2, X2[0] + s2 * (X1[0] - X2[0]), X2[0]), np.where(c2, X2[1] + s2 * (X1[1] - X2[1]), X2[1]),
              np.where(c2, near, X2[2])]
        flags = np.where(c1 | c2, M.CLIPPED_NEAR, 0).astype(np.uint32)
        x1, y1, iz1 = project_point(K, Y1)
        x2, y2, iz2 = project_point(K, Y2)
        dx, dy = x2 - x1, y2 - y1
        xmax, ymax = f8(cam["width"] - 1), f8(cam["height"] - 1)
        t0, t1 = np.zeros(n, f8), np.ones(n, f8)
        for p, q in ((-dx, x1), (dx, xmax - x1), (-dy, y1), (dy, ymax - y1)):      # left, right, top, bottom
            zero = p == 0.0
            visible &= ~(zero & (q < 0.0))
            r = q / p
            t0 = np.where(~zero & (p < 0.0) & (r > t0), r, t0)
            t1 = np.where(~zero & ~(p < 0.0) & (r < t1), r, t1)
        visible &= t0 < t1
        lo, hi = t0 > 0.0, t1 < 1.0
        o = [np.where(lo, x1 + t0 * dx, x1), np.where(lo, y1 + t0 * dy, y1), np.where(hi, x1 + t1 * dx, x2),
             np.where(hi, y1 + t1 * dy, y2), np.where(lo, iz1 + t0 * (iz2 - iz1), iz1), np.where(hi, iz1 + t1 * (iz2 - iz1), iz2)]
        flags |= np.where(lo | hi, M.CLIPPED_RECT, 0).astype(np.uint32)
        o32 = [v.astype(np.float32) for v in o]
        for v in o32:
            visible &= np.isfinite(v)                                                # step 5
    keep = np.flatnonzero(visible)
    rec = np.zeros(len(keep), M.RECORD_DTYPE)
    for name, v in zip(("x1", "y1", "x2", "y2", "inv_depth1", "inv_depth2"), o32):
        rec[name] = v[keep]
    rec["line"] = np.asarray(line_of_segment, np.uint32)[keep]
    rec["segment"] = keep.astype(np.uint32) | flags[keep]
    return rec


def project_segments(cams, P1, P2, line_of_segment, near=1e-6):
    """stage 1 -> one RECORD_DTYPE array per camera"""
    return [project_camera(cam, P1, P2, line_of_segment, near) for cam in cams]


def raster_steps(records, width, height):
    """major-axis steps of every record: (count [n], first integer major coordinate [n]) -- 0 for one that draws nothing"""
    rec = np.asarray(records, M.RECORD_DTYPE).reshape(-1)
    x1, y1, x2, y2 = (rec[k].astype(f8) for k in ("x1", "y1", "x2", "y2"))
    dx, dy = x2 - x1, y2 - y1
    draws = ~((dx == 0.0) & (dy == 0.0))
    xmajor = np.abs(dx) >= np.abs(dy)
    m1, m2 = np.where(xmajor, x1, y1), np.where(xmajor, x2, y2)
    am, bm = np.where(m1 <= m2, m1, m2), np.where(m1 <= m2, m2, m1)
    msize = np.where(xmajor, width, height).astype(np.int64)
    lo = np.maximum(np.ceil(am).astype(np.int64), 0)
    hi = np.minimum(np.floor(bm).astype(np.int64), msize - 1)
    return np.where(draws, np.maximum(hi - lo + 1, 0), 0), lo


def record_keys(records, width, height, thickness=1):
    """stage 2, steps 1-5 for all records of one camera -> (pixel index y * width + x, 64-bit key) of every pixel drawn"""
    rec = np.asarray(records, M.RECORD_DTYPE).reshape(-1)
    count, lo = raster_steps(rec, width, height)
    idx = np.repeat(np.arange(len(rec)), count)
    if len(idx) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    k = np.arange(len(idx)) - np.repeat(np.cumsum(count) - count, count)
    r = rec[idx]
    x1, y1, x2, y2 = (r[name].astype(f8) for name in ("x1", "y1", "x2", "y2"))
    z1, z2 = r["inv_depth1"].astype(f8), r["inv_depth2"].astype(f8)
    xmajor = np.abs(x2 - x1) >= np.abs(y2 - y1)
    m1, n1 = np.where(xmajor, x1, y1), np.where(xmajor, y1, x1)
    m2, n2 = np.where(xmajor, x2, y2), np.where(xmajor, y2, x2)
    first = m1 <= m2
    am, an, az = np.where(first, m1, m2), np.where(first, n1, n2), np.where(first, z1, z2)
    bm, bn, bz = np.where(first, m2, m1), np.where(first, n2, n1), np.where(first, z2, z1)
    nsize = np.where(xmajor, height, width).astype(np.int64)
    m = lo[idx] + k
    s = (m.astype(f8) - am) / (bm - am)
    n = np.floor(an + s * (bn - an) + f8(0.5)).astype(np.int64)
    iz = (az + s * (bz - az)).astype(np.float32)
    key = (iz.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - r["line"].astype(np.uint64))
    half = (thickness - 1) // 2
    pix, keys = [], []
    for o in range(-half, half + 1):
        ok = (n + o >= 0) & (n + o <= nsize - 1)
        x, y = np.where(xmajor, m, n + o)[ok], np.where(xmajor, n + o, m)[ok]
        pix.append(y * width + x); keys.append(key[ok])
    return np.concatenate(pix), np.concatenate(keys)


def key_plane(records, width, height, thickness=1):
    plane = np.zeros(width * height, np.uint64)
    pix, key = record_keys(records, width, height, thickness)
    np.maximum.at(plane, pix, key)
    return plane


def decode(plane, width, height):
    drawn = plane != 0
    line_id = np.where(drawn, np.uint64(0xFFFFFFFF) - (plane & np.uint64(0xFFFFFFFF)), 0).astype(np.int64)
    line_id = np.where(drawn, line_id, -1).astype(np.int32).reshape(height, width)
    inv_depth = (plane >> np.uint64(32)).astype(np.uint32).view(np.float32).reshape(height, width)
    return line_id, inv_depth


def render_line_maps(records, width, height, thickness=1):
    """stage 2 for one camera -> (line_id int32 [height, width], inv_depth float32 [height, width])"""
    return decode(key_plane(records, width, height, thickness), width, height)


def draw_line_map(image, line_id, alpha=255, colors=None):
    """stage 3 for one camera: image uint8 [h, w] or [h, w, 3] -> packed RGB uint8 [h, w, 3]"""
    img = np.asarray(image)
    out = np.ascontiguousarray(np.repeat(img[:, :, None], 3, 2) if img.ndim == 2 else img[:, :, :3], np.uint8).copy()
    drawn = line_id >= 0
    lid = line_id[drawn].astype(np.int64)
    h = ((lid + 1) * 0x9E3779B1) & 0xFFFFFFFF
    col = np.stack([64 + ((h >> s) & 255) * 3 // 4 for s in (24, 16, 8)], 1)
    if colors is not None and len(colors):
        table = np.asarray(colors, np.int64).reshape(-1, 3)
        listed = lid < len(table)
        col[listed] = table[lid[listed]]
    out[drawn] = ((alpha * col + (255 - alpha) * out[drawn].astype(np.int64) + 127) // 255).astype(np.uint8)
    return out
