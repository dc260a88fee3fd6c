"""Independent numpy model of Line3D::undistortImage (line3D.cc:83-109) as DESIGN §12 defines it: cv::invert's closed form
of the camera matrix, the column table, the CV_16SC2 map of initUndistortRectifyMap and the 15-bit fixed-point remap
(INTER_LINEAR, BORDER_CONSTANT 0) for 8-bit grey or interleaved RGB images.  Written from §12, not from the kernel;
vectorised, so it handles full-size images.  Every floating-point step is a separate rounded float64 numpy operation in
the order §12 gives (numpy fuses nothing)."""
import numpy as np

INT_MIN = -2 ** 31


def inverse(K):
    """cv::invert's closed-form 3x3 terms (adjugate x 1/det) for cvK = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]"""
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    det = fx * fy
    d = 1.0 / det
    return dict(ir0=fy * d, ir2=(-(cx * fy)) * d, ir4=fx * d, ir5=(-(fx * cy)) * d, ir8=(fx * fy) * d)


def column_table(ir0, ir2, cols):
    """X[0] = ir2, X[j+1] = X[j] + ir0: OpenCV's `_x += ir[0]` along a row, one addition at a time"""
    X = np.empty(cols, np.float64)
    acc = float(ir2)
    for j in range(cols):
        X[j] = acc
        acc = acc + ir0
    return X


def cv_round(t):
    """cvRound as x86 cvtsd2si: half to even; NaN or outside int32 -> INT_MIN (int64 array)"""
    ok = (t >= -2147483648.5) & (t < 2147483647.5)
    return np.where(ok, np.rint(np.where(ok, t, 0.0)), float(INT_MIN)).astype(np.int64)


def fixed_map(cols, rows, K, radial, tangential):
    """the CV_16SC2 map and its fractions for a cols x rows image: (sx, sy, a, b), int64 arrays of shape (rows, cols);
    sx, sy wrapped to int16 as OpenCV stores them, a, b in 1/32 px"""
    ir = inverse(K)
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    k1, k2, k3 = (float(v) for v in radial)
    p1, p2 = (float(v) for v in tangential)
    w = 1.0 / ir["ir8"]
    X = column_table(ir["ir0"], ir["ir2"], cols)
    Y = np.arange(rows, dtype=np.float64) * ir["ir4"] + ir["ir5"]
    with np.errstate(all="ignore"):
        x, y = np.broadcast_arrays((X * w)[None, :], (Y * w)[:, None])
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = (2 * x) * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
        fin = np.isfinite(xd) & np.isfinite(yd)
        u = np.where(fin, fx * xd + cx, np.nan)
        v = np.where(fin, fy * yd + cy, np.nan)
        iu = cv_round(u * 32)
        iv = cv_round(v * 32)
    sx = (iu >> 5).astype(np.int16).astype(np.int64)
    sy = (iv >> 5).astype(np.int16).astype(np.int64)
    return sx, sy, iu & 31, iv & 31


def weights(a, b, opencv_table=False):
    """(w00, w10, w01, w11), summing to 32768; opencv_table: the a = b = 0 entry as OpenCV's short table holds it,
    {32767, 0, 0, 1} (32768 saturates in a short)"""
    w = [(32 - a) * (32 - b) * 32, a * (32 - b) * 32, (32 - a) * b * 32, a * b * 32]
    if opencv_table:
        z = (a == 0) & (b == 0)
        w[0] = np.where(z, 32767, w[0])
        w[3] = np.where(z, 1, w[3])
    return w


def remap(img, sx, sy, a, b, opencv_table=False):
    """remap of an 8-bit HxW or HxWx3 image through the map: all four neighbours when 0 <= sx <= W-2 and 0 <= sy <= H-2;
    0 when sx >= W, sx < -1, sy >= H or sy < -1; else each neighbour inside the image contributes its pixel and each one
    outside contributes 0.  out = clamp((sum w p + 16384) >> 15, 0, 255)"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    src = img.reshape(H, W, -1).astype(np.int64)
    acc = np.zeros(sx.shape + (src.shape[2],), np.int64)
    for (dx, dy), wt in zip(((0, 0), (1, 0), (0, 1), (1, 1)), weights(a, b, opencv_table)):
        X, Y = sx + dx, sy + dy
        inside = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
        p = src[np.clip(Y, 0, H - 1), np.clip(X, 0, W - 1)] * inside[..., None]
        acc += p * np.asarray(wt)[..., None]
    out = np.clip((acc + 16384) >> 15, 0, 255)
    out[(sx >= W) | (sx < -1) | (sy >= H) | (sy < -1)] = 0
    return out.astype(np.uint8).reshape(img.shape)


def undistort(img, K, radial, tangential, opencv_table=False):
    """Line3D::undistortImage of an 8-bit HxW (grey) or HxWx3 image; the result has the input's shape"""
    img = np.asarray(img, np.uint8)
    sx, sy, a, b = fixed_map(img.shape[1], img.shape[0], K, radial, tangential)
    return remap(img, sx, sy, a, b, opencv_table)


def from_strided(buf, cols, rows, channels, row_stride):
    """the image an l3d_image with a row stride describes: rows of row_stride bytes, of which cols * channels are
    pixels"""
    a = np.frombuffer(bytes(buf), np.uint8)[:rows * row_stride].reshape(rows, row_stride)[:, :cols * channels]
    return a.reshape(rows, cols) if channels == 1 else a.reshape(rows, cols, channels)
