"""Undistortion on the MI355X (k_undistort.hip, l3d_undistort_images): Line3D::undistortImage against the independent
numpy model of tests/undistort_model.py byte for byte, model-free properties, straight lines made straight again for
the detector, the C++ facade from several threads, and the error paths.  DESIGN §12."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib
from line3dpp_amd.api import Line3D
from line3dpp_amd.lsd import as_image, detect_line_segments, distortion, read_image_gray, undistort_images
from tests import undistort_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lsd")


def _K(w, h, f=None, fy=None, cx=None, cy=None):
    f = 0.9 * w if f is None else f
    return np.array([[f, 0.0, w / 2 if cx is None else cx], [0.0, f if fy is None else fy, h / 2 if cy is None else cy],
                     [0.0, 0.0, 1.0]])


COEFFS = {   # (radial, tangential)
    "barrel": ((-0.25, 0.06, 0.0), (0.0, 0.0)),
    "pincushion": ((0.18, 0.02, 0.0), (0.0, 0.0)),
    "tangential": ((0.0, 0.0, 0.0), (0.004, -0.003)),
    "all_five": ((-0.12, 0.03, -0.005), (0.0012, -0.0009)),
    "vsfm": ((-0.0873, 0.0, 0.0), (0.0, 0.0)),
}
SIZES = [(64, 48), (65, 49), (641, 479), (1920, 1080)]


def _image(w, h, seed, rgb=False):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (40 + 30 * np.sin(xx / 7.0) + 25 * np.cos(yy / 5.0) + ((xx // 16 + yy // 16) % 2) * 90).astype(np.int64)
    img = np.clip(base[..., None] + rng.integers(0, 40, (h, w, 3)), 0, 255) if rgb else np.clip(base + rng.integers(0, 40, (h, w)), 0, 255)
    return img.astype(np.uint8)


def _check(imgs, Ks, coeffs, what):
    got = undistort_images(imgs, Ks, [c[0] for c in coeffs], [c[1] for c in coeffs])
    for k, (img, K, (r, t), g) in enumerate(zip(imgs, Ks, coeffs, got)):
        want = M.undistort(img, K, r, t)
        assert g.shape == want.shape and g.dtype == np.uint8
        diff = int((g != want).sum())
        assert diff == 0, f"{what} [{k}]: {diff} bytes differ from the model"
    return got


@pytest.mark.parametrize("w,h", SIZES)
def test_equals_the_model(w, h):
    names = sorted(COEFFS)
    imgs = [_image(w, h, k) for k in range(len(names))]
    Ks = [_K(w, h)] * len(names)
    got = _check(imgs, Ks, [COEFFS[n] for n in names], f"{w}x{h}")
    assert not any(np.array_equal(g, i) for g, i in zip(got, imgs))


@pytest.mark.parametrize("w,h", [(2, 5), (3, 7), (5, 2)])
def test_images_narrower_than_a_thread_equal_the_model(w, h):
    """a thread writes 4 adjacent pixels of the packed image: here they cross one or more row ends"""
    for rgb in (False, True):
        imgs = [_image(w, h, 40 + k, rgb=rgb) for k in range(3)]
        Ks = [_K(w, h), _K(w, h, f=0.7 * w, fy=0.9 * h, cx=0.3 * w, cy=0.6 * h), _K(w, h)]
        _check(imgs, Ks, [COEFFS["all_five"], COEFFS["barrel"], COEFFS["pincushion"]], f"{w}x{h} rgb={rgb}")


def test_off_centre_principal_point_fx_ne_fy_rgb_and_strides():
    w, h = 641, 479
    K = _K(w, h, f=560.0, fy=602.5, cx=281.25, cy=260.75)
    grey, rgb = _image(w, h, 11), _image(w, h, 12, rgb=True)
    padded = np.zeros((h, w + 37), np.uint8)
    padded[:, :w] = grey
    view = padded[:, :w]
    assert view.strides[0] == w + 37 and as_image(view)[0].row_stride == w + 37
    padded_rgb = np.zeros((h, w + 5, 3), np.uint8)
    padded_rgb[:, :w] = rgb
    coeffs = [COEFFS["all_five"], COEFFS["barrel"], COEFFS["all_five"], COEFFS["pincushion"]]
    got = _check([grey, rgb, view, padded_rgb[:, :w]], [K] * 4, coeffs, "off-centre / RGB / stride")
    assert np.array_equal(got[0], got[2])


def test_strong_distortion_wraps_int16_and_full_size_image():
    """small fx with k1 = k2 = 1: the corners of the map leave int16 and wrap; and the full 3072x2304 image"""
    img = read_image_gray(os.path.join(GOLD, "img000055.jpg"))
    assert img.shape == (2304, 3072)
    strong = ((1.0, 1.0, 0.0), (0.0, 0.0))
    Ks = [_K(640, 480, f=40.0), _K(3072, 2304, f=2600.0), _K(3072, 2304, f=2600.0, cx=1500.0, cy=1170.0)]
    x, y = -320 / 40.0, -240 / 40.0                                 # the top-left corner, normalised
    r2 = x * x + y * y
    assert abs(40.0 * x * (1 + r2 + r2 * r2) + 320) > 2 ** 15        # its u is beyond int16
    _check([_image(640, 480, 3), img, img], Ks, [strong, COEFFS["vsfm"], COEFFS["all_five"]], "strong / full size")


def test_model_free_properties():
    w, h = 641, 479
    grey = _image(w, h, 21)
    rgb = _image(w, h, 22, rgb=True)
    K = _K(w, h, f=600.0, fy=580.0, cx=300.0, cy=250.0)
    zero = ((0.0, 0.0, 0.0), (0.0, 0.0))
    # zero coefficients return the input, whatever K
    for Kz in (K, _K(w, h, f=3.0), _K(w, h, f=2000.0, cx=-40.0, cy=900.0)):
        out = undistort_images([grey, rgb], [Kz, Kz], [zero[0]] * 2, [zero[1]] * 2)
        assert np.array_equal(out[0], grey) and np.array_equal(out[1], rgb)
    r, t = COEFFS["all_five"]
    # RGB = three grey undistortions
    planes = undistort_images([np.ascontiguousarray(rgb[..., c]) for c in range(3)], [K] * 3, [r] * 3, [t] * 3)
    col = undistort_images([rgb], [K], [r], [t])[0]
    assert all(np.array_equal(col[..., c], planes[c]) for c in range(3))
    # a batch of mixed sizes = one call per image; two runs give equal bytes
    imgs = [_image(64, 48, 1), rgb, _image(1920, 1080, 2), _image(65, 49, 3, rgb=True), grey]
    Ks = [_K(64, 48), K, _K(1920, 1080), _K(65, 49), K]
    cs = [COEFFS[n] for n in ("barrel", "all_five", "pincushion", "tangential", "vsfm")]
    batch = undistort_images(imgs, Ks, [c[0] for c in cs], [c[1] for c in cs])
    again = undistort_images(imgs, Ks, [c[0] for c in cs], [c[1] for c in cs])
    for k, img in enumerate(imgs):
        one = undistort_images([img], [Ks[k]], [cs[k][0]], [cs[k][1]])[0]
        assert one.tobytes() == batch[k].tobytes() == again[k].tobytes()
    # out may be the input's own memory
    L = _lib.load()
    h_ = C.c_void_p(L.l3d_create(0, None))
    try:
        mine = grey.copy()
        im, keep = as_image(mine)
        d = distortion(K, r, t)
        outp = (C.c_void_p * 1)(mine.ctypes.data)
        assert L.l3d_undistort_images(h_, 1, C.byref(im), C.byref(d), outp) == 0
        assert np.array_equal(mine, undistort_images([grey], [K], [r], [t])[0])
    finally:
        L.l3d_destroy(h_)
    # the static facade method of the Python mirror
    assert np.array_equal(Line3D.undistortImage(grey, r, t, K), undistort_images([grey], [K], [r], [t])[0])


def _errors(img_struct, K, r, t):
    L = _lib.load()
    h = C.c_void_p(L.l3d_create(0, None))
    try:
        out = np.zeros(16, np.uint8)
        d = distortion(K, r, t)
        outp = (C.c_void_p * 1)(out.ctypes.data)
        return L.l3d_undistort_images(h, 1, C.byref(img_struct), C.byref(d), outp), _lib.last_error()
    finally:
        L.l3d_destroy(h)


def test_error_paths():
    img = np.zeros((48, 64 * 2), np.uint8)
    two = _lib.Image(img.ctypes.data, 64, 48, 2, 128)
    rc, msg = _errors(two, _K(64, 48), (0.1, 0, 0), (0, 0))
    assert rc == -1 and "not supported" in msg                     # L3D_ERR_ARG
    grey, _ = as_image(img[:, :64])
    rc, msg = _errors(grey, _K(64, 48, f=0.0), (0.1, 0, 0), (0, 0))
    assert rc == -1 and "fx * fy" in msg
    rc, msg = _errors(grey, _K(64, 48), (0.1, float("nan"), 0), (0, 0))
    assert rc == -1 and "non-finite" in msg
    rc, msg = _errors(grey, _K(64, 48, cy=float("inf")), (0.1, 0, 0), (0, 0))
    assert rc == -1
    wide = np.zeros((2, 40000), np.uint8)                          # 80 kB: refused before anything is allocated
    rc, msg = _errors(as_image(wide)[0], _K(40000, 2), (0.1, 0, 0), (0, 0))
    assert rc == -9 and "SHRT_MAX" in msg                          # L3D_ERR_LIMIT
    # the Python mirror prints and returns None, as the facade prints and leaves its output empty
    assert Line3D.undistortImage(img[:, :64], (0.1, float("nan"), 0), (0, 0), _K(64, 48)) is None
    with pytest.raises(TypeError):
        undistort_images([np.zeros((4, 4, 2), np.uint8)], [_K(4, 4)], [(0, 0, 0)], [(0, 0)])


# ---- straight lines stay straight -----------------------------------------------------------------------------------
SCENE_W, SCENE_H = 1024, 768
SCENE_K = np.array([[700.0, 0, 512.0], [0, 700.0, 384.0], [0, 0, 1]])
SCENE_RADIAL = (-0.2, 0.0, 0.0)
# detected endpoints within T px of a true line for at least P of the segments.  Measured on the MI355X:
# undistorted 100 % of 40 segments (still 100 % at 0.5 px), distorted 0 % of 54 (still 0 % at 2 px), clean 100 % of 40
T_PX = 1.0
P_FRAC = 0.90


def _scene_lines():
    """8 straight lines (a, b, c), a x + b y = c with |(a, b)| = 1, across the whole image: 4 near-horizontal ones close to
    the top and bottom, where the distortion bends them most, and 4 near-vertical ones"""
    out = []
    for k, (y0, ang) in enumerate([(70, 0.02), (230, -0.03), (540, 0.025), (700, -0.015)]):
        out.append((-np.sin(ang), np.cos(ang), -np.sin(ang) * 512 + np.cos(ang) * y0))
    for k, (x0, ang) in enumerate([(80, 0.02), (350, -0.025), (690, 0.03), (950, -0.02)]):
        out.append((np.cos(ang), np.sin(ang), np.cos(ang) * x0 + np.sin(ang) * 384))
    return np.array(out)


def _pattern(x, y, lines):
    """the XOR of the lines' half-planes: every line is an edge of contrast 110 along its whole length"""
    par = np.zeros(x.shape, np.int64)
    for a, b, c in lines:
        par ^= (a * x + b * y > c).astype(np.int64)
    return 70.0 + 110.0 * par


def _inverse_map(u, v, K, radial):
    """the undistorted pixel whose §12 map lands on (u, v): fixed-point iteration of x = xd / kr(x) (radial only)"""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    xd, yd = (u - cx) / fx, (v - cy) / fy
    x, y = xd.copy(), yd.copy()
    k1, k2, k3 = radial
    for _ in range(40):
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        x, y = xd / kr, yd / kr
    return fx * x + cx, fy * y + cy


def straight_scene(distorted, s=4):
    """the clean scene (distorted=False) or the image a camera with SCENE_RADIAL takes of it, anti-aliased by s x s
    supersampling"""
    lines = _scene_lines()
    yy, xx = np.mgrid[0:SCENE_H, 0:SCENE_W].astype(np.float64)
    acc = np.zeros((SCENE_H, SCENE_W))
    for dy in range(s):
        for dx in range(s):
            u, v = xx + (dx + 0.5) / s - 0.5, yy + (dy + 0.5) / s - 0.5
            if distorted:
                u, v = _inverse_map(u, v, SCENE_K, SCENE_RADIAL)
            acc += _pattern(u, v, lines)
    return np.clip(np.rint(acc / (s * s)), 0, 255).astype(np.uint8)


def straight_fraction(segs, tol):
    """the share of segments whose two endpoints both lie within tol px of one true line"""
    lines = _scene_lines()
    d1 = np.abs(segs[:, None, 0] * lines[None, :, 0] + segs[:, None, 1] * lines[None, :, 1] - lines[None, :, 2])
    d2 = np.abs(segs[:, None, 2] * lines[None, :, 0] + segs[:, None, 3] * lines[None, :, 1] - lines[None, :, 2])
    return float((np.maximum(d1, d2).min(axis=1) <= tol).mean())


def test_undistortion_straightens_lines_for_the_detector():
    distorted = straight_scene(True)
    und = undistort_images([distorted], [SCENE_K], [SCENE_RADIAL], [(0.0, 0.0)])[0]
    s_und, s_dist, s_clean = detect_line_segments([und, distorted, straight_scene(False)])
    f_und, f_dist, f_clean = (straight_fraction(s, T_PX) for s in (s_und, s_dist, s_clean))
    print(f"segments within {T_PX} px of a true line: undistorted {100 * f_und:.1f} % of {len(s_und)}, distorted "
          f"{100 * f_dist:.1f} % of {len(s_dist)}, clean scene {100 * f_clean:.1f} % of {len(s_clean)}")
    assert len(s_und) >= 8 and f_und >= P_FRAC
    assert f_dist < P_FRAC                                          # the same test tells the distorted image apart


# ---- the C++ facade (include/line3dpp/line3D.h) ---------------------------------------------------------------------
def test_facade_undistorts_from_threads_and_addImage_detects_on_the_result(tmp_path):
    exe = str(tmp_path / "undistort_facade")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "undistort_facade.cpp"), "-o", exe, "-L" + lib_dir,
                           "-ll3dpp_hip", "-Wl,-rpath," + lib_dir, "-pthread"])
    base = straight_scene(True)
    imgs = [base, np.ascontiguousarray(base[:, ::-1]), _image(SCENE_W, SCENE_H, 31, rgb=True), np.ascontiguousarray(base[::-1])]
    coeffs = [(SCENE_RADIAL, (0.0, 0.0)), COEFFS["all_five"], COEFFS["barrel"], COEFFS["pincushion"]]
    Ks = [SCENE_K, _K(SCENE_W, SCENE_H, f=650.0, fy=660.0, cx=500.0, cy=390.0), SCENE_K, SCENE_K]
    path_in, path_out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(path_in, "wb") as f:
        f.write(struct.pack("<I", len(imgs)))
        for img, K, (r, t) in zip(imgs, Ks, coeffs):
            ch = 1 if img.ndim == 2 else 3
            f.write(struct.pack("<3I", img.shape[1], img.shape[0], ch))
            f.write(np.concatenate([np.asarray(K, np.float64).reshape(9), np.asarray(r, np.float64), np.asarray(t, np.float64)]).tobytes())
            f.write(np.ascontiguousarray(img).tobytes())
    run = subprocess.run([exe, path_in, path_out], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    want = undistort_images(imgs, Ks, [c[0] for c in coeffs], [c[1] for c in coeffs])
    segs = detect_line_segments(want)
    raw = open(path_out, "rb").read()
    pos = 0
    for k, w in enumerate(want):
        got = np.frombuffer(raw, np.uint8, w.size, pos).reshape(w.shape)
        pos += w.size
        assert np.array_equal(got, w), f"image {k}: the facade's bytes differ from undistort_images'"
    for k, s in enumerate(segs):
        got = np.frombuffer(raw, np.float32, 4 * 3001, pos).reshape(3001, 4)
        pos += 4 * 3001 * 4
        assert len(s) > 0 and np.array_equal(got[:len(s)], s), f"view {k}: addImage found other segments"
        assert not got[len(s):].any()
    assert pos == len(raw)
    assert "[L3D++] ERROR: undistortImage" in run.stdout and "RESULT undistorted=4 error_left_empty=1" in run.stdout
