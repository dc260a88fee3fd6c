"""numpy restatement of DESIGN §16 (the 3D lines projected into cameras), written from the contract, not from the kernels:
plain loops, float64 in the order the contract writes the operations, the three stages one after the other.  The tests
of the device code (tests/test_gpu_project.py) compare against it with tolerance 0."""
import numpy as np

RECORD_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("inv_depth1", "<f4"),
                         ("inv_depth2", "<f4"), ("line", "<u4"), ("segment", "<u4")])
CLIPPED_NEAR = 0x80000000
CLIPPED_RECT = 0x40000000
SEGMENT_MASK = 0x3FFFFFFF

f8 = np.float64


def mul33(A, v):
    """(a0 x + a1 y) + a2 z per row: the order of the library's 3x3 product"""
    A = np.asarray(A, f8).reshape(9)
    return [(A[3 * i] * v[0] + A[3 * i + 1] * v[1]) + A[3 * i + 2] * v[2] for i in range(3)]


def project_point(K, X):
    """step 3 of stage 1: pixel and inverse depth of a point in the camera frame"""
    q = mul33(K, [X[0] / X[2], X[1] / X[2], f8(1.0)])
    return q[0] / q[2], q[1] / q[2], f8(1.0) / X[2]


def project_segment(cam, P1, P2, near=1e-6):
    """stage 1 for one camera and one 3D segment -> None (not visible) or
    (x1, y1, x2, y2, iz1, iz2, flags, t0, t1, unclipped end points) in float64"""
    K, R, t = (np.asarray(cam[k], f8).reshape(-1) for k in ("K", "R", "t"))
    near = f8(near)
    X = []
    for P in (P1, P2):
        P = np.asarray(P, f8)
        rp = mul33(R, P)
        X.append([rp[0] + t[0], rp[1] + t[1], rp[2] + t[2]])
    X1, X2 = X
    flags = 0
    b1, b2 = X1[2] < near, X2[2] < near
    if b1 and b2:
        return None
    if b1:
        s = (near - X1[2]) / (X2[2] - X1[2])
        X1 = [X1[0] + s * (X2[0] - X1[0]), X1[1] + s * (X2[1] - X1[1]), near]
        flags |= CLIPPED_NEAR
    elif b2:
        s = (near - X2[2]) / (X1[2] - X2[2])
        X2 = [X2[0] + s * (X1[0] - X2[0]), X2[1] + s * (X1[1] - X2[1]), near]
        flags |= CLIPPED_NEAR
    with np.errstate(all="ignore"):
        x1, y1, iz1 = project_point(K, X1)
        x2, y2, iz2 = project_point(K, X2)
        return clip_to_rectangle(cam, x1, y1, x2, y2, iz1, iz2, flags)


def clip_to_rectangle(cam, x1, y1, x2, y2, iz1, iz2, flags):
    """steps 4 and 5 of stage 1"""
    dx, dy = x2 - x1, y2 - y1
    xmax, ymax = f8(cam["width"] - 1), f8(cam["height"] - 1)
    t0, t1 = f8(0.0), f8(1.0)
    for p, q in ((-dx, x1), (dx, xmax - x1), (-dy, y1), (dy, ymax - y1)):      # left, right, top, bottom
        if p == 0.0:
            if q < 0.0:
                return None
        else:
            r = q / p
            if p < 0.0:
                t0 = r if r > t0 else t0
            else:
                t1 = r if r < t1 else t1
    if not t0 < t1:
        return None
    o = [x1, y1, x2, y2, iz1, iz2]
    if t0 > 0.0:
        o[0], o[1], o[4] = x1 + t0 * dx, y1 + t0 * dy, iz1 + t0 * (iz2 - iz1)
        flags |= CLIPPED_RECT
    if t1 < 1.0:
        o[2], o[3], o[5] = x1 + t1 * dx, y1 + t1 * dy, iz1 + t1 * (iz2 - iz1)
        flags |= CLIPPED_RECT
    if not all(np.isfinite(np.float32(v)) for v in o):                          # step 5: a non-finite record is not visible
        return None
    return tuple(o) + (flags, t0, t1, (x1, y1, x2, y2))


def project_segments(cams, P1, P2, line_of_segment, near=1e-6):
    """stage 1 -> one RECORD_DTYPE array per camera, visible records in ascending segment order"""
    out = []
    for cam in cams:
        rec = []
        for s in range(len(P1)):
            r = project_segment(cam, P1[s], P2[s], near)
            if r is not None:
                rec.append(tuple(np.float32(v) for v in r[:6]) + (int(line_of_segment[s]), s | r[6]))
        out.append(np.array(rec, RECORD_DTYPE).reshape(-1))
    return out


def record_pixels(rec, width, height, thickness=1):
    """stage 2, steps 1-5 for one record: [(x, y, float32 inverse depth)] of the pixels it draws, inside the image"""
    x1, y1, x2, y2 = (f8(rec[k]) for k in ("x1", "y1", "x2", "y2"))
    z1, z2 = f8(rec["inv_depth1"]), f8(rec["inv_depth2"])
    dx, dy = x2 - x1, y2 - y1
    if dx == 0.0 and dy == 0.0:
        return []
    xmajor = abs(dx) >= abs(dy)
    e1, e2 = ((x1, y1, z1), (x2, y2, z2)) if xmajor else ((y1, x1, z1), (y2, x2, z2))
    a, b = (e1, e2) if e1[0] <= e2[0] else (e2, e1)
    msize, nsize = (width, height) if xmajor else (height, width)
    half = (thickness - 1) // 2
    out = []
    for m in range(max(int(np.ceil(a[0])), 0), min(int(np.floor(b[0])), msize - 1) + 1):   # outside the image: dropped
        s = (f8(m) - a[0]) / (b[0] - a[0])
        n = int(np.floor(a[1] + s * (b[1] - a[1]) + f8(0.5)))
        iz = np.float32(a[2] + s * (b[2] - a[2]))
        for o in range(-half, half + 1):
            if 0 <= n + o <= nsize - 1:
                out.append((m, n + o, iz) if xmajor else (n + o, m, iz))
    return out


def pixel_key(iz, line):
    return (int(np.float32(iz).view(np.uint32)) << 32) | (0xFFFFFFFF - int(line))


def render_line_maps(records, width, height, thickness=1):
    """stage 2 for one camera -> (line_id int32 [height, width], inv_depth float32 [height, width])"""
    keys = {}
    for rec in records:
        for x, y, iz in record_pixels(rec, width, height, thickness):
            k = pixel_key(iz, rec["line"])
            if k > keys.get((x, y), 0):
                keys[(x, y)] = k
    line_id = np.full((height, width), -1, np.int32)
    inv_depth = np.zeros((height, width), np.float32)
    for (x, y), k in keys.items():
        line_id[y, x] = 0xFFFFFFFF - (k & 0xFFFFFFFF)
        inv_depth[y, x] = np.array([k >> 32], np.uint32).view(np.float32)[0]
    return line_id, inv_depth


def palette(line):
    h = ((int(line) + 1) * 0x9E3779B1) & 0xFFFFFFFF
    return tuple(64 + ((h >> s) & 255) * 3 // 4 for s in (24, 16, 8))


def draw_line_map(image, line_id, alpha=255, colors=None):
    """stage 3 for one camera: image uint8 [h, w] or [h, w, 3] -> packed RGB uint8 [h, w, 3]"""
    img = np.asarray(image)
    out = np.ascontiguousarray(np.repeat(img[:, :, None], 3, 2) if img.ndim == 2 else img[:, :, :3], np.uint8).copy()
    for y, x in np.argwhere(line_id >= 0):        # elsewhere the source pixel is copied
        lid = int(line_id[y, x])
        col = [int(v) for v in colors[lid]] if colors is not None and lid < len(colors) else palette(lid)
        out[y, x] = [(alpha * col[c] + (255 - alpha) * int(out[y, x, c]) + 127) // 255 for c in range(3)]
    return out
