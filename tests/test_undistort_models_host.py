"""CPU checks of undistortion by camera model on the numpy model of tests/undistort_models_model.py: the
equalities between the models, an independent numeric inverse of every forward formula, the robustness of the GPU
tests' agreement cap on the GPU tests' own inputs, and io.front_end_camera_model.  No GPU."""
import numpy as np
import pytest

from line3dpp_amd import io
from tests import undistort_model as M12
from tests import undistort_models_cases as CASES
from tests import undistort_models_model as M
from tests.sfm_readers_model import _colmap_camera


def _eq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_full_opencv_without_k4_k5_k6_is_section_12():
    w, h = 641, 479
    K = CASES.K_of(w, h, f=560.0, fy=602.5, cx=281.25, cy=260.75)
    for rgb in (False, True):
        img = CASES.image(w, h, 5, rgb=rgb)
        radial, tangential = (-0.12, 0.03, -0.005), (0.0012, -0.0009)
        params = (radial[0], radial[1], tangential[0], tangential[1], radial[2], 0.0, 0.0, 0.0)
        assert _eq(M.undistort(img, "FULL_OPENCV", K, params), M12.undistort(img, K, radial, tangential))
    assert not _eq(M.undistort(img, "FULL_OPENCV", K, params[:5] + (0.01, 0.0, 0.0)), M12.undistort(img, K, radial, tangential))


def test_fisheye_family_is_one_formula():
    w, h = 641, 479
    img = CASES.image(w, h, 6)
    K = CASES.K_of(w, h, f=500.0, cx=300.0, cy=250.0)          # fx = fy
    a = M.undistort(img, "RADIAL_FISHEYE", K, (-0.04, 0.0))
    assert _eq(a, M.undistort(img, "SIMPLE_RADIAL_FISHEYE", K, (-0.04,)))
    b = M.undistort(img, "OPENCV_FISHEYE", K, (-0.03, 0.006, 0.0, 0.0))
    assert _eq(b, M.undistort(img, "RADIAL_FISHEYE", K, (-0.03, 0.006)))
    assert not _eq(a, b) and not _eq(a, img)
    # zero coefficients: still an equidistant image, not a pinhole one
    assert not _eq(M.undistort(img, "SIMPLE_RADIAL_FISHEYE", K, (0.0,)), img)


def test_fov_with_omega_zero_and_K_new():
    w, h = 641, 479
    K = CASES.K_of(w, h, f=560.0, fy=602.5, cx=281.25, cy=260.75)
    for rgb in (False, True):
        img = CASES.image(w, h, 7, rgb=rgb)
        assert _eq(M.undistort(img, "FOV", K, (0.0,)), img)
    for model in M.MODELS:
        p = CASES.PARAMS[model]
        assert _eq(M.undistort(img, model, K, p, K_new=K), M.undistort(img, model, K, p, K_new=np.zeros((3, 3))))
        assert _eq(M.undistort(img, model, K, p, K_new=K), M.undistort(img, model, K, p))
        half = K.copy(); half[0, 0] /= 2; half[1, 1] /= 2
        assert not _eq(M.undistort(img, model, K, p, K_new=half), M.undistort(img, model, K, p))


def test_fov_branches_meet():
    """the three forms of FOV's factor agree where they hand over: the definitions' thresholds are harmless"""
    x = np.array([0.00999, 0.0099999, 0.01, 0.0100001, 0.01001])       # r2 around 1e-4
    xd, _ = M.distort("FOV", (0.9,), x, np.zeros_like(x))
    assert np.ptp(xd / x) < 1e-6                 # (the series' remainder at the hand-over is of the order of 1e-9)
    s_small = M.distort("FOV", (0.00999,), np.array([0.3]), np.array([0.2]))[0] / 0.3      # omega^2 < 1e-4
    s_large = M.distort("FOV", (0.01001,), np.array([0.3]), np.array([0.2]))[0] / 0.3
    # COLMAP's series for a small omega, which §15 restates, has the signs of its two omega^2 terms the other way round
    # from the expansion of the closed form (1 + omega^2 / 12 - omega^2 r^2 / 3), so the hand-over is a step of
    # 2 omega^2 |r^2 / 3 - 1 / 12| = 8.7e-6 here: far below a pixel's 1 / 32 at any focal length this library accepts
    assert abs(s_small - s_large) < 2 * 1e-4 * abs(0.13 / 3 - 1 / 12) * 1.01


@pytest.mark.parametrize("model", M.MODELS)
def test_numeric_inverse_returns_to_the_start(model):
    """guards against a formula typed wrongly in both model and kernel: the inverse is Newton's iteration on the forward
    formula with a finite-difference Jacobian, and the forward formula is checked against known values first"""
    rng = np.random.default_rng(3)
    x, y = rng.uniform(-0.8, 0.8, 500), rng.uniform(-0.6, 0.6, 500)
    p = CASES.PARAMS[model]
    xd, yd = M.distort(model, p, x, y)
    assert np.abs(xd - x).max() > 1e-3
    bx, by = M.undistort_point(model, p, xd, yd)
    assert np.abs(bx - x).max() < 1e-9 and np.abs(by - y).max() < 1e-9
    # the forward formulas against their textbook forms at one point, computed another way
    r = np.hypot(0.3, 0.4)
    got = M.distort(model, p, np.array([0.3]), np.array([0.4]))
    if model == "FOV":
        s = np.arctan(2 * r * np.tan(p[0] / 2)) / (r * p[0])
    elif model == "FULL_OPENCV":
        k1, k2, p1, p2, k3, k4, k5, k6 = p
        r2 = r * r
        kr = np.polyval([k3, k2, k1, 1], r2) / np.polyval([k6, k5, k4, 1], r2)
        want = (0.3 * kr + 2 * p1 * 0.12 + p2 * (r2 + 0.18), 0.4 * kr + p1 * (r2 + 0.32) + 2 * p2 * 0.12)
        assert np.allclose([got[0][0], got[1][0]], want, rtol=0, atol=1e-14)
        return
    else:
        k = list(p) + [0.0] * 4
        th = np.arctan(r)
        s = th * np.polyval([k[3], k[2], k[1], k[0], 1], th * th) / r
    assert np.allclose([got[0][0], got[1][0]], [0.3 * s, 0.4 * s], rtol=0, atol=1e-14)


def test_strong_cases_leave_the_image():
    for model in M.MODELS:
        w, h, f, p = CASES.STRONG[model]
        sx, sy, _, _ = M.fixed_map(w, h, model, CASES.K_of(w, h, f=f), p)
        for i, j in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            assert not (0 <= sx[i, j] < w and 0 <= sy[i, j] < h), (model, i, j)


@pytest.mark.parametrize("model", M.MODELS)
def test_the_agreement_cap_is_robust_on_the_gpu_tests_inputs(model):
    """The device's sqrt, atan and division are not glibc's.  Every input of tests/test_gpu_undistort_models.py goes
    through the model once more with the result of each of them moved by +-1 and +-4 ulp: the cap (1 pixel in 100 000, at
    least 1, at most 16 grey levels) must hold between the two."""
    for name, img, K, p, K_new in CASES.cases(model):
        want = M.undistort(img, model, K, p, K_new)
        for ulp in (-4, -1, 1, 4):
            n, worst = CASES.compare(M.undistort(img, model, K, p, K_new, ulp=ulp), want)
            print(f"{model} {name} ulp {ulp:+d}: {n} pixels differ (largest {worst})")
            assert n <= CASES.cap(img) and worst <= 16, (model, name, ulp, n, worst)


# ---- io.front_end_camera_model -----------------------------------------------------------------------------------------
def _entry(model, params):
    cam = _colmap_camera(model, list(params), 640, 480)
    return dict(id=1, camera=1, name="a.jpg", worldpoints=[1, 2], **cam)


def test_front_end_camera_model():
    f = io.front_end_camera_model
    # the fisheye family: always, zero coefficients included
    for model, params, want in (("OPENCV_FISHEYE", (500, 510, 320, 240, -0.03, 0.005, -0.001, 0.0002), [-0.03, 0.005, -0.001, 0.0002]),
                                ("OPENCV_FISHEYE", (500, 510, 320, 240, 0, 0, 0, 0), [0, 0, 0, 0]),
                                ("SIMPLE_RADIAL_FISHEYE", (500, 320, 240, -0.04), [-0.04]),
                                ("SIMPLE_RADIAL_FISHEYE", (500, 320, 240, 0), [0]),
                                ("RADIAL_FISHEYE", (500, 320, 240, -0.03, 0.006), [-0.03, 0.006]),
                                ("RADIAL_FISHEYE", (500, 320, 240, 0, 0), [0, 0])):
        e = _entry(model, params)
        m, K, p = f("colmap", e, 640, 480)
        assert m == model and p == [float(v) for v in want] and np.array_equal(K, e["K"])
        assert K[0, 0] == 500 and K[1, 1] == (510 if model == "OPENCV_FISHEYE" else 500) and K[0, 2] == 320 and K[1, 2] == 240
        assert not e["radial"].any() and not e["tangential"].any()
        assert io.front_end_undistortion("colmap", e, 640, 480) is None
    # FOV: when |omega| exceeds L3D_EPS
    m, K, p = f("colmap", _entry("FOV", (500, 510, 320, 240, -0.9)), 640, 480)
    assert m == "FOV" and p == [-0.9] and K[1, 1] == 510
    assert f("colmap", _entry("FOV", (500, 510, 320, 240, 0.0)), 640, 480) is None
    assert f("colmap", _entry("FOV", (500, 510, 320, 240, 5e-13)), 640, 480) is None
    # FULL_OPENCV: when k4, k5 or k6 exceeds L3D_EPS; with zeros it takes the five coefficients' path as before
    base = (500, 510, 320, 240, -0.1, 0.02, 1e-3, -2e-3, 3e-3)
    for tail in ((0.01, 0, 0), (0, -0.002, 0), (0, 0, 0.0005)):
        m, K, p = f("colmap", _entry("FULL_OPENCV", base + tail), 640, 480)
        assert m == "FULL_OPENCV" and p == [-0.1, 0.02, 1e-3, -2e-3, 3e-3] + [float(v) for v in tail]
    for tail in ((0, 0, 0), (5e-13, -5e-13, 0), ()):
        e = _entry("FULL_OPENCV", base + tail)
        assert f("colmap", e, 640, 480) is None
        K, radial, tangential = io.front_end_undistortion("colmap", e, 640, 480)
        assert list(radial) == [-0.1, 0.02, 3e-3] and list(tangential) == [1e-3, -2e-3]
    # the reference's models never, and neither any other front end
    for model, params in (("SIMPLE_PINHOLE", (500, 320, 240)), ("PINHOLE", (500, 510, 320, 240)), ("SIMPLE_RADIAL", (500, 320, 240, 0.1)),
                          ("RADIAL", (500, 320, 240, 0.1, 0.01)), ("OPENCV", (500, 510, 320, 240, 0.1, 0.01, 0.001, 0.002))):
        e = _entry(model, params)
        assert f("colmap", e, 640, 480) is None
        und = io.front_end_undistortion("colmap", e, 640, 480)
        assert (und is None) == (model in ("SIMPLE_PINHOLE", "PINHOLE"))
    e = _entry("OPENCV_FISHEYE", (500, 510, 320, 240, -0.03, 0.005, -0.001, 0.0002))
    for kind in ("nvm", "bundler", "openmvg", "pix4d", "mavmap"):
        assert f(kind, e, 640, 480) is None
