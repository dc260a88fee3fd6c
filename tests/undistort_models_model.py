"""Independent numpy model of undistortion by camera model as DESIGN §15 defines it: COLMAP's FULL_OPENCV, OPENCV_FISHEYE,
RADIAL_FISHEYE, SIMPLE_RADIAL_FISHEYE and FOV forward distortion per destination pixel, then §12's CV_16SC2 map and
fixed-point remap (tests/undistort_model.py).  Written from §15, not from the kernel.  Every floating-point step is a
separate rounded float64 numpy operation in the order §15 gives.

`ulp` moves the result of every sqrt, atan and division by that many units in the last place (np.nextafter): the
operations whose device forms are not glibc's.  tests/test_undistort_models_host.py uses it to show that the agreement
cap of the GPU tests is robust on their inputs."""
import math

import numpy as np

from tests.undistort_model import column_table, cv_round, inverse, remap

MODELS = ("FULL_OPENCV", "OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "FOV")
N_PARAMS = {"FULL_OPENCV": 8, "OPENCV_FISHEYE": 4, "SIMPLE_RADIAL_FISHEYE": 1, "RADIAL_FISHEYE": 2, "FOV": 1}
DBL_EPSILON = 2.220446049250313e-16


def _moved(v, ulp):
    if not ulp:
        return v
    v = np.asarray(v, np.float64)
    target = np.full(v.shape, np.inf if ulp > 0 else -np.inf)
    for _ in range(abs(ulp)):
        v = np.nextafter(v, target)
    return v


def distort(model, params, x, y, ulp=0):
    """(xd, yd) of normalised (x, y) by the model's forward formula; params in COLMAP's order, missing ones 0"""
    p = [float(v) for v in params] + [0.0] * 8
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        if model == "FULL_OPENCV":
            k1, k2, p1, p2, k3, k4, k5, k6 = p[:8]
            _2xy = (2 * x) * y
            kr = _moved((1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2), ulp)
            xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
            yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
            return xd, yd
        if model == "FOV":
            om = p[0]
            om2 = om * om
            T = math.tan(om / 2)
            if om2 < 1e-4:
                s = _moved((om2 * r2) / 3, ulp) - _moved(np.float64(om2 / 12), ulp) + 1
            else:
                r = _moved(np.sqrt(r2), ulp)
                far = _moved(_moved(np.arctan(r * (2 * T)), ulp) / (r * om), ulp)
                near = _moved((-2 * T * (4 * r2 * T * T - 3)) / (3 * om), ulp)
                s = np.where(r2 < 1e-4, near, far)
            return x * s, y * s
        if model in ("OPENCV_FISHEYE", "RADIAL_FISHEYE", "SIMPLE_RADIAL_FISHEYE"):
            k1, k2, k3, k4 = (p + [0.0] * 4)[:4] if model == "OPENCV_FISHEYE" else (p[0], p[1], 0.0, 0.0) \
                if model == "RADIAL_FISHEYE" else (p[0], 0.0, 0.0, 0.0)
            r = _moved(np.sqrt(r2), ulp)
            th = _moved(np.arctan(r), ulp)
            th2 = th * th
            thd = th * (1 + (((k4 * th2 + k3) * th2 + k2) * th2 + k1) * th2)
            s = np.where(r > DBL_EPSILON, _moved(thd / r, ulp), 1.0)
            return x * s, y * s
    raise ValueError(f"camera model {model} unknown!")


def fixed_map(cols, rows, model, K, params, K_new=None, ulp=0):
    """the CV_16SC2 map and its fractions: (sx, sy, a, b) as tests/undistort_model.fixed_map gives them.  X, Y and w come
    from K_new (None or all zero: K), u and v from K"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    Kn = K if K_new is None or not np.asarray(K_new, np.float64).any() else np.asarray(K_new, np.float64).reshape(3, 3)
    ir = inverse(Kn)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    w = 1.0 / ir["ir8"]
    X = column_table(ir["ir0"], ir["ir2"], cols)
    Y = np.arange(rows, dtype=np.float64) * ir["ir4"] + ir["ir5"]
    with np.errstate(all="ignore"):
        x, y = np.broadcast_arrays((X * w)[None, :], (Y * w)[:, None])
        xd, yd = distort(model, params, x, y, ulp)
        fin = np.isfinite(xd) & np.isfinite(yd)
        u = np.where(fin, fx * xd + cx, np.nan)
        v = np.where(fin, fy * yd + cy, np.nan)
        iu = cv_round(u * 32)
        iv = cv_round(v * 32)
    sx = (iu >> 5).astype(np.int16).astype(np.int64)
    sy = (iv >> 5).astype(np.int16).astype(np.int64)
    return sx, sy, iu & 31, iv & 31


def undistort(img, model, K, params, K_new=None, ulp=0):
    """the undistorted image of an 8-bit HxW (grey) or HxWx3 image; the result has the input's shape"""
    img = np.asarray(img, np.uint8)
    sx, sy, a, b = fixed_map(img.shape[1], img.shape[0], model, K, params, K_new, ulp)
    return remap(img, sx, sy, a, b)


def undistort_point(model, params, xd, yd, iterations=100):
    """the numeric inverse of `distort`: Newton's iteration with a finite-difference Jacobian, on arrays"""
    xd = np.asarray(xd, np.float64)
    yd = np.asarray(yd, np.float64)
    x, y = xd.copy(), yd.copy()
    h = 1e-7
    for _ in range(iterations):
        fx0, fy0 = distort(model, params, x, y)
        ax, ay = distort(model, params, x + h, y)
        bx, by = distort(model, params, x, y + h)
        j00, j10 = (ax - fx0) / h, (ay - fy0) / h
        j01, j11 = (bx - fx0) / h, (by - fy0) / h
        det = j00 * j11 - j01 * j10
        ex, ey = fx0 - xd, fy0 - yd
        x = x - (j11 * ex - j01 * ey) / det
        y = y - (-j10 * ex + j00 * ey) / det
    return x, y
