"""Undistortion by camera model on the MI355X (k_undistort_model, l3d_undistort_images_model): the device
against the numpy model of tests/undistort_models_model.py under §15's agreement condition, exact model-free properties,
curved lines made straight again for the detector, the C++ facade from four threads, and the error paths."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib
from line3dpp_amd.api import Line3D
from line3dpp_amd.lsd import as_image, camera_model, detect_line_segments, undistort_images, undistort_images_model
from tests import undistort_models_cases as CASES
from tests import undistort_models_model as M
from tests.test_gpu_undistort import P_FRAC, SCENE_H, SCENE_K, SCENE_W, T_PX, _pattern, _scene_lines, straight_fraction

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _eq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("model", CASES.MODELS)
def test_device_agrees_with_the_model(model):
    """§15's agreement condition: the device's atan, sqrt and division are not glibc's, so at most 1 pixel in 100 000 of
    an image may differ (at least 1 allowed), each by at most 16 grey levels.  Counts measured on the MI355X are in
    DESIGN §15."""
    cases = CASES.cases(model)
    got = undistort_images_model([c[1] for c in cases], [model] * len(cases), [c[2] for c in cases],
                                 [c[3] for c in cases], [c[4] for c in cases])
    bad = []
    for (name, img, K, p, K_new), g in zip(cases, got):
        want = M.undistort(img, model, K, p, K_new)
        assert g.shape == want.shape and g.dtype == np.uint8
        n, worst = CASES.compare(g, want)
        print(f"{model} {name}: {n} of {img.shape[0] * img.shape[1]} pixels differ from the model (largest difference {worst}, cap {CASES.cap(img)})")
        if n > CASES.cap(img) or worst > 16:
            bad.append((name, n, worst))
        assert not _eq(g, np.ascontiguousarray(img)) or img.size < 64
    assert not bad, bad


def test_exact_equalities_between_models():
    w, h = 641, 479
    K = CASES.K_of(w, h, f=560.0, fy=602.5, cx=281.25, cy=260.75)
    grey, rgb = CASES.image(w, h, 5), CASES.image(w, h, 6, rgb=True)
    # FULL_OPENCV with k4 = k5 = k6 = 0 is Line3D::undistortImage's five coefficients
    radial, tangential = (-0.12, 0.03, -0.005), (0.0012, -0.0009)
    params = (radial[0], radial[1], tangential[0], tangential[1], radial[2], 0.0, 0.0, 0.0)
    a = undistort_images_model([grey, rgb], ["FULL_OPENCV"] * 2, [K, K], [params, params])
    b = undistort_images([grey, rgb], [K, K], [radial] * 2, [tangential] * 2)
    assert _eq(a[0], b[0]) and _eq(a[1], b[1]) and not _eq(a[0], grey)
    # the fisheye family is one formula
    Kf = CASES.K_of(w, h, f=500.0, cx=300.0, cy=250.0)               # fx = fy
    s, r0, r, o = undistort_images_model([grey] * 4, ["SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "RADIAL_FISHEYE", "OPENCV_FISHEYE"],
                                         [Kf] * 4, [(-0.04,), (-0.04, 0.0), (-0.03, 0.006), (-0.03, 0.006, 0.0, 0.0)])
    assert _eq(s, r0) and _eq(r, o) and not _eq(s, r) and not _eq(s, grey)
    # FOV with omega = 0 is the identity, whatever K
    for Kz in (K, CASES.K_of(w, h, f=3.0), CASES.K_of(w, h, f=2000.0, cx=-40.0, cy=900.0)):
        out = undistort_images_model([grey, rgb], ["FOV"] * 2, [Kz, Kz], [(0.0,)] * 2)
        assert _eq(out[0], grey) and _eq(out[1], rgb)
    # K_new = K is the all-zero K_new
    for model in CASES.MODELS:
        p = CASES.PARAMS[model]
        x, y = undistort_images_model([grey, grey], [model] * 2, [K, K], [p, p], [K, None])
        assert _eq(x, y)


def test_model_free_properties():
    w, h = 641, 479
    K = CASES.K_of(w, h, f=600.0, fy=580.0, cx=300.0, cy=250.0)
    grey, rgb = CASES.image(w, h, 21), CASES.image(w, h, 22, rgb=True)
    for model in CASES.MODELS:
        p = CASES.PARAMS[model]
        # RGB = three grey undistortions
        planes = undistort_images_model([np.ascontiguousarray(rgb[..., c]) for c in range(3)], [model] * 3, [K] * 3, [p] * 3)
        col = undistort_images_model([rgb], [model], [K], [p])[0]
        assert all(np.array_equal(col[..., c], planes[c]) for c in range(3)), model
    # a batch of all five models and mixed sizes = one call per image; two runs give equal bytes
    imgs = [CASES.image(64, 48, 1), rgb, CASES.image(1920, 1080, 2), CASES.image(65, 49, 3, rgb=True), grey, CASES.image(5, 2, 4)]
    Ks = [CASES.K_of(64, 48), K, CASES.K_of(1920, 1080), CASES.K_of(65, 49), K, CASES.K_of(5, 2)]
    models = list(CASES.MODELS) + ["OPENCV_FISHEYE"]
    ps = [CASES.PARAMS[m] for m in models]
    half = K.copy(); half[0, 0] /= 2; half[1, 1] /= 2
    K_new = [None, half, None, None, K, None]
    batch = undistort_images_model(imgs, models, Ks, ps, K_new)
    again = undistort_images_model(imgs, models, Ks, ps, K_new)
    for k, img in enumerate(imgs):
        one = undistort_images_model([img], [models[k]], [Ks[k]], [ps[k]], [K_new[k]])[0]
        assert one.tobytes() == batch[k].tobytes() == again[k].tobytes(), k
    # out may be the input's own memory
    L = _lib.load()
    h_ = C.c_void_p(L.l3d_create(0, None))
    try:
        for model in ("OPENCV_FISHEYE", "FOV"):
            mine = grey.copy()
            im, keep = as_image(mine)
            m = camera_model(model, K, CASES.PARAMS[model])
            outp = (C.c_void_p * 1)(mine.ctypes.data)
            assert L.l3d_undistort_images_model(h_, 1, C.byref(im), C.byref(m), outp) == 0
            assert np.array_equal(mine, undistort_images_model([grey], [model], [K], [CASES.PARAMS[model]])[0])
        assert L.l3d_undistort_images_model(h_, 0, None, None, None) == 0          # an empty batch
    finally:
        L.l3d_destroy(h_)
    # the static method of the Python mirror
    assert np.array_equal(Line3D.undistortImageModel(grey, "FOV", K, (0.9,)), undistort_images_model([grey], ["FOV"], [K], [(0.9,)])[0])
    assert np.array_equal(Line3D.undistortImageModel(grey, "FOV", K, (0.9,), half),
                          undistort_images_model([grey], ["FOV"], [K], [(0.9,)], [half])[0])


def _errors(img_structs, cams):
    """-> (status, message, outputs untouched): every output starts as 0xA5 and must still be so after a refusal"""
    L = _lib.load()
    h = C.c_void_p(L.l3d_create(0, None))
    try:
        n = len(cams)
        outs = [np.full(64 * 48 * 3, 0xA5, np.uint8) for _ in range(n)]
        outp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        rc = L.l3d_undistort_images_model(h, n, (_lib.Image * n)(*img_structs), (_lib.CameraModel * n)(*cams), outp)
        return rc, _lib.last_error(), all((o == 0xA5).all() for o in outs)
    finally:
        L.l3d_destroy(h)


def test_error_paths_leave_the_outputs_alone():
    img = np.zeros((48, 64 * 2), np.uint8)
    grey, _ = as_image(img[:, :64])
    K = CASES.K_of(64, 48)
    good = camera_model("FOV", K, (0.9,))

    def cam(model="OPENCV_FISHEYE", K=K, params=(0.1,), K_new=None, number=None):
        m = camera_model(model, K, params, K_new)
        if number is not None:
            m.model = number
        return m

    two = _lib.Image(img.ctypes.data, 64, 48, 2, 128)
    nan_new = K.copy(); nan_new[0, 2] = float("nan")
    for what, image, c, status, text in (
            ("channels", two, cam(), -1, "not supported"),
            ("unknown model", grey, cam(number=6), -1, "unknown camera model"),
            ("model 0", grey, cam(number=0), -1, "unknown camera model"),
            ("fx * fy", grey, cam(K=CASES.K_of(64, 48, f=0.0)), -1, "fx * fy"),
            ("K_new singular", grey, cam(K_new=CASES.K_of(64, 48, f=0.0)), -1, "fx * fy"),
            ("NaN parameter", grey, cam(params=(0.1, float("nan"))), -1, "non-finite"),
            ("inf in K", grey, cam(K=CASES.K_of(64, 48, cy=float("inf"))), -1, "non-finite"),
            ("NaN in K_new", grey, cam(K_new=nan_new), -1, "non-finite")):
        # the bad image is the SECOND of the batch: the first one's output must not have been written either
        rc, msg, untouched = _errors([grey, image], [good, c])
        assert rc == status and text in msg and untouched, (what, rc, msg, untouched)
    wide = np.zeros((2, 40000), np.uint8)                          # refused before anything is allocated
    rc, msg, untouched = _errors([grey, as_image(wide)[0]], [good, cam(K=CASES.K_of(40000, 2))])
    assert rc == -9 and "SHRT_MAX" in msg and untouched            # L3D_ERR_LIMIT
    # a NaN in a parameter the model does not read is not an error: RADIAL_FISHEYE reads two
    m = cam("RADIAL_FISHEYE", params=(0.1, 0.01))
    m.params[5] = float("nan")
    rc, msg, untouched = _errors([grey], [m])
    assert rc == 0 and not untouched
    # the Python mirror prints and returns None
    assert Line3D.undistortImageModel(img[:, :64], "FOV", K, (float("nan"),)) is None
    assert Line3D.undistortImageModel(img[:, :64], "THIN_PRISM_FISHEYE", K, (0.1,)) is None
    with pytest.raises(ValueError):
        undistort_images_model([img[:, :64]], ["PINHOLE"], [K], [()])
    with pytest.raises(ValueError):
        undistort_images_model([img[:, :64]], ["FOV"], [K], [(0.1, 0.2)])
    with pytest.raises(TypeError):
        undistort_images_model([np.zeros((4, 4, 2), np.uint8)], ["FOV"], [CASES.K_of(4, 4)], [(0.1,)])


# ---- curved lines made straight again -------------------------------------------------------------------------------
# coefficients for which the numpy models (undistort_models_model + lsd_model) meet the thresholds on the CPU: DESIGN §15
STRAIGHT = {"OPENCV_FISHEYE": (-0.03, 0.005, -0.001, 0.0002), "FOV": (0.9,)}


def curved_scene(model, params, s=4):
    """the image a camera of this model takes of the 8-line scene of tests/test_gpu_undistort.py, anti-aliased by s x s
    supersampling: every sample of the distorted image is brought back by the numeric inverse of the forward formula"""
    lines = _scene_lines()
    fx, fy, cx, cy = SCENE_K[0, 0], SCENE_K[1, 1], SCENE_K[0, 2], SCENE_K[1, 2]
    yy, xx = np.mgrid[0:SCENE_H, 0:SCENE_W].astype(np.float64)
    acc = np.zeros((SCENE_H, SCENE_W))
    for dy in range(s):
        for dx in range(s):
            u, v = xx + (dx + 0.5) / s - 0.5, yy + (dy + 0.5) / s - 0.5
            x, y = M.undistort_point(model, params, (u - cx) / fx, (v - cy) / fy, iterations=8)
            acc += _pattern(fx * x + cx, fy * y + cy, lines)
    return np.clip(np.rint(acc / (s * s)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("model", sorted(STRAIGHT))
def test_undistortion_straightens_lines_for_the_detector(model):
    distorted = curved_scene(model, STRAIGHT[model])
    und = undistort_images_model([distorted], [model], [SCENE_K], [STRAIGHT[model]])[0]
    s_und, s_dist = detect_line_segments([und, distorted])
    f_und, f_dist = straight_fraction(s_und, T_PX), straight_fraction(s_dist, T_PX)
    print(f"{model}: segments within {T_PX} px of a true line: undistorted {100 * f_und:.1f} % of {len(s_und)}, distorted "
          f"{100 * f_dist:.1f} % of {len(s_dist)}")
    assert len(s_und) >= 8 and f_und >= P_FRAC
    assert f_dist < P_FRAC                                          # the same test tells the distorted image apart


# ---- the C++ facade (include/line3dpp/line3D.h) ---------------------------------------------------------------------
def test_facade_overload_from_four_threads_gives_pythons_bytes(tmp_path):
    exe = str(tmp_path / "undistort_models_facade")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "undistort_models_facade.cpp"), "-o", exe, "-L" + lib_dir,
                           "-ll3dpp_hip", "-Wl,-rpath," + lib_dir, "-pthread"])
    w, h = 1024, 768
    K = CASES.K_of(w, h, f=650.0, fy=660.0, cx=500.0, cy=390.0)
    half = K.copy(); half[0, 0] /= 2; half[1, 1] /= 2
    imgs = [CASES.image(w, h, 31), CASES.image(w, h, 32, rgb=True), CASES.image(641, 479, 33), CASES.image(w, h, 34)]
    models = ["OPENCV_FISHEYE", "FOV", "FULL_OPENCV", "RADIAL_FISHEYE"]
    Ks = [K, K, CASES.K_of(641, 479), K]
    K_new = [None, half, None, half]
    ps = [CASES.PARAMS[m] for m in models]
    path_in, path_out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(path_in, "wb") as f:
        f.write(struct.pack("<I", len(imgs)))
        for img, m, Kk, Kn, p in zip(imgs, models, Ks, K_new, ps):
            ch = 1 if img.ndim == 2 else 3
            f.write(struct.pack("<5I", img.shape[1], img.shape[0], ch, _lib.CAMERA_MODELS[m], int(Kn is not None)))
            f.write(np.concatenate([Kk.reshape(9), (np.zeros(9) if Kn is None else Kn.reshape(9)),
                                    np.array(list(p) + [0.0] * (8 - len(p)))]).astype(np.float64).tobytes())
            f.write(np.ascontiguousarray(img).tobytes())
    run = subprocess.run([exe, path_in, path_out], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    want = undistort_images_model(imgs, models, Ks, ps, K_new)
    raw = open(path_out, "rb").read()
    pos = 0
    for k, wnt in enumerate(want):
        got = np.frombuffer(raw, np.uint8, wnt.size, pos).reshape(wnt.shape)
        pos += wnt.size
        assert np.array_equal(got, wnt), f"image {k}: the facade's bytes differ from undistort_images_model's"
    assert pos == len(raw)
    assert run.stdout.count("[L3D++] ERROR: undistortImage") == 2
    assert "RESULT undistorted=4 fov_zero_is_identity=1 errors_left_empty=1" in run.stdout
