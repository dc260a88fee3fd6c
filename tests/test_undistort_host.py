"""CPU checks of the undistortion contract on the numpy model of tests/undistort_model.py, and of
io.front_end_undistortion against the reference's own front ends (main_vsfm.cpp, main_colmap.cpp, main_bundler.cpp run
against the recorder of tests/test_front_ends_pinned.py).  No GPU."""
import numpy as np
import pytest

from line3dpp_amd import io
from tests import undistort_model as M
from tests.test_front_ends_pinned import _calls, _front, _m, _run, _touch
from tests.test_input_formats import _colmap_scene, _write_bundler, _write_colmap, _write_nvm

CASES = [   # (K, radial, tangential)
    (np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]), (-0.2, 0.05, 0.0), (0.0, 0.0)),
    (np.array([[480.0, 0.3, 300.5], [0, 510, 251.25], [0, 0, 1]]), (0.15, -0.02, 0.001), (0.0, 0.0)),
    (np.array([[620.0, 0, 330], [0, 600, 230], [0, 0, 1]]), (0.0, 0.0, 0.0), (0.002, -0.0015)),
    (np.array([[700.0, 0, 310], [0, 690, 245], [0, 0, 1]]), (-0.1, 0.03, -0.004), (0.001, 0.0007)),
]


def _direct(cols, rows, K, radial, tangential):
    """the distortion polynomial evaluated directly in float64 at every destination pixel (no column table, no
    inverse): (u, v) in source pixels"""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, k3 = radial
    p1, p2 = tangential
    jj, ii = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    x, y = (jj - cx) / fx, (ii - cy) / fy
    r2 = x * x + y * y
    kr = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


@pytest.mark.parametrize("k", range(len(CASES)))
def test_map_agrees_with_the_distortion_polynomial(k):
    K, radial, tangential = CASES[k]
    cols, rows = 641, 479
    sx, sy, a, b = M.fixed_map(cols, rows, K, radial, tangential)
    u, v = _direct(cols, rows, K, radial, tangential)
    ok = (np.abs(u) < 32000) & (np.abs(v) < 32000)
    assert ok.mean() > 0.99
    tol = 1 / 64 + 1e-6
    assert np.abs(sx + a / 32 - u)[ok].max() <= tol
    assert np.abs(sy + b / 32 - v)[ok].max() <= tol


def test_strong_distortion_wraps_int16_at_the_corners():
    """small fx and k1 = k2 = 1: the corners map far outside int16 and wrap as OpenCV's (short) cast does"""
    K = np.array([[40.0, 0, 320], [0, 40, 240], [0, 0, 1]])
    sx, sy, a, b = M.fixed_map(640, 480, K, (1.0, 1.0, 0.0), (0.0, 0.0))
    u, _ = _direct(640, 480, K, (1.0, 1.0, 0.0), (0.0, 0.0))
    corner = np.abs(u) > 40000
    assert corner.any()
    iu = np.floor(u[corner] * 32 + 0.5).astype(np.int64)         # far from half-integers here: same as half-even
    fits = np.abs(u[corner] * 32) < 2 ** 31
    assert np.array_equal(sx[corner][fits], ((iu[fits] >> 5) + 2 ** 15) % 2 ** 16 - 2 ** 15)


@pytest.mark.parametrize("K", [np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]),
                               np.array([[812.5, 0, 17.25], [0, 799.0, 400.75], [0, 0, 1]]),
                               np.array([[3.0, 0, 1000.0], [0, 2.5, -3.0], [0, 0, 1]]),
                               np.array([[2400.0, 0, 1536.0], [0, 2400.0, 1152.0], [0, 0, 1]])])
def test_zero_coefficients_give_the_input(K):
    rng = np.random.default_rng(1)
    for shape in [(48, 64), (49, 65), (37, 41, 3)]:
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        sx, sy, a, b = M.fixed_map(shape[1], shape[0], K, (0, 0, 0), (0, 0))
        assert not a.any() and not b.any()
        assert np.array_equal(sx, np.broadcast_to(np.arange(shape[1]), sx.shape))
        assert np.array_equal(M.undistort(img, K, (0, 0, 0), (0, 0)), img)


def test_constant_image_stays_constant_away_from_the_border():
    K, radial, tangential = CASES[0]
    img = np.full((480, 640), 137, np.uint8)
    out = M.undistort(img, K, radial, tangential)
    sx, sy, a, b = M.fixed_map(640, 480, K, radial, tangential)
    inside = (sx >= 0) & (sx <= 638) & (sy >= 0) & (sy <= 478)
    assert inside.mean() > 0.9
    assert (out[inside] == 137).all()
    assert (out[(sx >= 640) | (sx < -1) | (sy >= 480) | (sy < -1)] == 0).all()


def test_opencv_weight_table_gives_the_same_bytes():
    """a = b = 0: OpenCV's short table holds {32767, 0, 0, 1}; (32767 p00 + p11 + 16384) >> 15 == p00 for 8-bit p"""
    rng = np.random.default_rng(2)
    for k, (K, radial, tangential) in enumerate(CASES):
        img = rng.integers(0, 256, (120, 160, 3) if k % 2 else (120, 160), dtype=np.uint8)
        sx, sy, a, b = M.fixed_map(160, 120, K * 0.25 + np.diag([0, 0, 0.75]), radial, tangential)
        assert ((a == 0) & (b == 0)).any()
        assert np.array_equal(M.remap(img, sx, sy, a, b), M.remap(img, sx, sy, a, b, opencv_table=True))
    p = np.arange(256)
    assert all(np.array_equal((32767 * p + q + 16384) >> 15, p) for q in (0, 255))


def test_rgb_is_three_grey_undistortions_and_strides_read_the_same_pixels():
    K, radial, tangential = CASES[3]
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    out = M.undistort(rgb, K * 0.2 + np.diag([0, 0, 0.8]), radial, tangential)
    for c in range(3):
        assert np.array_equal(out[..., c], M.undistort(rgb[..., c], K * 0.2 + np.diag([0, 0, 0.8]), radial, tangential))
    padded = np.zeros((97, 131 * 3 + 13), np.uint8)
    padded[:, :131 * 3] = rgb.reshape(97, -1)
    assert np.array_equal(M.from_strided(padded.tobytes(), 131, 97, 3, 131 * 3 + 13), rgb)


# ---- what the reference's front ends hand to undistortImage ---------------------------------------------------------
def _undistorted(ev):
    return [(np.array(u["radial"]), np.array(u["tangential"]), _m(u, "K")) for u in _calls(ev, "undistortImage")]


def _same(got, want):
    assert len(got) == len(want)
    for (r, t, K), w in zip(got, want):
        assert np.array_equal(K, w[0]) and np.array_equal(r, w[1]) and np.array_equal(t, w[2])


def _followed_by_its_addImage(ev, cams):
    """every undistortImage is followed by the addImage of the image it undistorted (the front end's loop body)"""
    names = [(e["call"], e.get("camID")) for e in ev]
    k = 0
    for i, (name, _) in enumerate(names):
        if name == "undistortImage":
            assert names[i + 1] == ("addImage", cams[k])
            k += 1
    assert k == len(cams)


def test_front_end_undistortion_equals_main_vsfm(tmp_path):
    rng = np.random.default_rng(13)
    cams = []
    for i in range(6):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        dist = [0.02, 0.0, -0.013, 5e-13, 0.0071, 0.03][i]      # 5e-13: below L3D_EPS, no undistortImage
        cams.append(dict(filename=f"img_{i}.jpg", focal=1800.0 + 3.5 * i, q=q, C=rng.normal(size=3) * 4, distortion=dist))
    points = []
    for k in range(80):
        seen = sorted(rng.choice(5, size=rng.integers(2, 4), replace=False).tolist())   # camera 5 sees nothing
        points.append((rng.normal(size=3) * 3, [(c, k, 10.0 + k, 20.0) for c in seen]))
    path = tmp_path / "r.nvm"
    _write_nvm(path, cams, points)
    _touch(tmp_path / "imgs", [f"img_{i}.jpg" for i in range(6)])
    rc, ev = _run(_front(), "vsfm", ["-i", str(tmp_path / "imgs"), "-m", str(path), "-o", str(tmp_path / "out")])
    assert rc == 0
    got = io.read_nvm(path)
    want = [io.front_end_undistortion("nvm", g, 640, 480) for g in got]      # the recorder's images are 640 x 480
    assert [w is not None for w in want] == [True, False, True, False, True, False]
    _same(_undistorted(ev), [w for w in want if w is not None])
    _followed_by_its_addImage(ev, [i for i, w in enumerate(want) if w is not None])


def test_front_end_undistortion_equals_main_bundler(tmp_path):
    rng = np.random.default_rng(14)
    cams = []
    for i in range(6):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        k1, k2 = [(-0.02, 0.003), (0.0, 0.0), (0.0, 0.0011), (3e-13, -2e-13), (0.015, 0.0), (-0.01, 0.001)][i]
        cams.append(dict(f=1000.0 + 7.25 * i, k1=k1, k2=k2, R=io.rotation_from_q(*q), t=rng.normal(size=3) * 2))
    points = []
    for k in range(100):
        seen = sorted(rng.choice(5, size=rng.integers(2, 4), replace=False).tolist())   # camera 5 sees nothing
        points.append((rng.normal(size=3) * 5, [(c, k, 1.0 + k, -2.5) for c in seen]))
    path = tmp_path / "bundle.rd.out"
    _write_bundler(path, cams, points)
    _touch(tmp_path / "imgs", [f"{i:08d}.jpg" for i in range(6)])
    rc, ev = _run(_front(), "bundler", ["-i", str(tmp_path / "imgs"), "-b", str(path), "-o", str(tmp_path / "out")])
    assert rc == 0
    got = io.read_bundler(str(path))
    want = [io.front_end_undistortion("bundler", g, 640, 480) for g in got]
    assert [w is not None for w in want] == [True, False, True, False, True, False]
    _same(_undistorted(ev), [w for w in want if w is not None])
    _followed_by_its_addImage(ev, [i for i, w in enumerate(want) if w is not None])


def test_front_end_undistortion_equals_main_colmap(tmp_path):
    rng = np.random.default_rng(4)
    cams, images, points = _colmap_scene(rng)
    _write_colmap(tmp_path / "sfm", cams, images, points)
    _touch(tmp_path / "imgs", [im[4] for im in images])
    rc, ev = _run(_front(), "colmap", ["-i", str(tmp_path / "imgs"), "-m", str(tmp_path / "sfm"), "-o", str(tmp_path / "out")])
    assert rc == 0
    got = io.read_colmap(str(tmp_path / "sfm"))
    want = [io.front_end_undistortion("colmap", g, 640, 480) for g in got]
    # PINHOLE-type cameras have no coefficients; the image without worldpoints is undistorted all the same
    assert sum(w is not None for w in want) == 4 and any(w is not None and not g["worldpoints"] for g, w in zip(got, want))
    _same(_undistorted(ev), [w for w in want if w is not None])
    with pytest.raises(ValueError):
        io.front_end_undistortion("pix4d", got[0], 640, 480)
