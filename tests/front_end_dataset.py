"""The dataset of tests/test_gpu_front_end.py: a synthetic scene rendered to images and written as a VisualSfM .nvm, a
COLMAP text model and a bundler file.

`scene.make_scene` gives the cameras (the first views of a ring: an arc) and the 3D structure (its facade segments,
regenerated from its seed); `scene.add_worldpoints` the SfM points.  Of the structure only what every view sees is
drawn: a spaced-out subset of the segments of the +x facade, each as a dark bar several pixels thick on the bright
facade, so that every bar gives the detector two long edges and the facade four more.  The images are 1024 x 768 grey PNGs,
rendered through a pinhole at twice the size and box-filtered down.  Two cameras carry a radial distortion so small that
undistortion moves no pixel by a whole pixel (`corner_shift`), so the pinhole rendering stands for the distorted image.
"""
import numpy as np

from line3dpp_amd import scene as scene_mod

WIDTH, HEIGHT, FOCAL = 1024, 768, 620.0
N_VIEWS, RING, N_SEGS, SEED = 7, 36, 300, 20
HALF = 10.0                      # scene._scene_lines: the box's half side
BAR = 0.3                        # bar thickness in scene units: about 8 px at the cameras' distance
MIN_LENGTH, MIN_GAP = 1.5, 1.2   # which facade segments are drawn: long ones, no two closer than this
DISTORTION = {1: 5e-4, 4: -4e-4}   # camera -> k1 (bundler, COLMAP) = -d (.nvm)
N_POINTS = 600


def corner_shift(k1):
    """pixels by which undistortion with (k1, 0, 0) moves the image corner (the largest displacement in the image)"""
    r = np.hypot(WIDTH / 2, HEIGHT / 2) / FOCAL
    return abs(k1) * r * r * r * FOCAL


def _seg_distance(a, b, n=9):
    ta = np.linspace(0, 1, n)[:, None]
    pa = a[0] + ta * (a[1] - a[0]); pb = b[0] + ta * (b[1] - b[0])
    return np.min(np.linalg.norm(pa[:, None, :] - pb[None, :, :], axis=2))


def structure():
    """the drawn part of make_scene's 3D structure: [n, 2, 3] segments on the facade x = +HALF"""
    rng = np.random.default_rng(SEED)
    P, Q, N = scene_mod._scene_lines(rng, max(int(6 * N_SEGS * 1.0), 64))
    on = (N[:, 0] == 1) & (np.linalg.norm(P - Q, axis=1) >= MIN_LENGTH)
    margin = HALF - 1.0
    chosen = []
    for p, q in zip(P[on], Q[on]):
        if np.abs(p[1:]).max() > margin or np.abs(q[1:]).max() > margin:
            continue
        if all(_seg_distance((p, q), c) >= MIN_GAP for c in chosen):
            chosen.append((p, q))
    return np.array(chosen)


def make():
    """-> (scene with the arc's cameras at WIDTH x HEIGHT and worldpoint lists, the worldpoints [n,3], the drawn segments)"""
    sc = scene_mod.make_scene(RING, N_SEGS, real_fraction=1.0, seed=SEED, max_views=N_VIEWS)
    for v in sc.views:
        v.K = np.array([[FOCAL, 0, WIDTH / 2], [0, FOCAL, HEIGHT / 2], [0, 0, 1.0]])
        v.width, v.height = WIDTH, HEIGHT
    X = scene_mod.add_worldpoints(sc, n_points=N_POINTS)
    return sc, X, structure()


def render(view, segs, scale=2):
    """grey uint8 HEIGHT x WIDTH image of the facade and its bars as `view` sees them through a pinhole"""
    from PIL import Image, ImageDraw

    def project(pts):
        Xc = (view.R @ np.asarray(pts).T).T + view.t
        assert (Xc[:, 2] > 1.0).all()
        x = (view.K @ Xc.T).T
        return [((u / w + 0.5) * scale, (r / w + 0.5) * scale) for u, r, w in x]

    im = Image.new("L", (WIDTH * scale, HEIGHT * scale), 110)
    draw = ImageDraw.Draw(im)
    h = HALF
    draw.polygon(project([[h, -h, -h], [h, h, -h], [h, h, h], [h, -h, h]]), fill=225)
    for p, q in segs:
        d = (q - p) / np.linalg.norm(q - p)
        side = np.cross(d, [1.0, 0.0, 0.0]) * (BAR / 2)          # in the facade's plane, across the bar
        draw.polygon(project([p - side, q - side, q + side, p + side]), fill=30)
    return np.asarray(im.resize((WIDTH, HEIGHT), Image.BOX), np.uint8).copy()


def quaternion(R):
    """unit quaternion (w, x, y, z) of a rotation matrix, w >= 0"""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    q = np.array([w, np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1])])
    return q / np.linalg.norm(q)


def write(folder):
    """renders the images into folder/images (vsfm / COLMAP names) and folder/bundler_images (bundler's numbered names)
    and writes folder/model.nvm, folder/colmap/ and folder/bundle.rd.out -> the scene"""
    from PIL import Image
    from tests.test_input_formats import _write_bundler, _write_colmap, _write_nvm
    sc, X, segs = make()
    assert len(segs) >= 12 and all(corner_shift(k) < 1.0 for k in DISTORTION.values())
    (folder / "images").mkdir(parents=True)
    (folder / "bundler_images").mkdir()
    for v in sc.views:
        im = Image.fromarray(render(v, segs))
        im.save(folder / "images" / f"view_{v.cam}.png")
        im.save(folder / "bundler_images" / f"{v.cam:08d}.png")
    seen = {v.cam: set(v.worldpoints) for v in sc.views}
    k1 = {v.cam: DISTORTION.get(v.cam, 0.0) for v in sc.views}
    centre = {v.cam: -v.R.T @ v.t for v in sc.views}
    measures = [[(c, 0, 1.0, 1.0) for c in sorted(seen) if i in seen[c]] for i in range(len(X))]
    _write_nvm(folder / "model.nvm", [dict(filename=f"images/view_{v.cam}.png", focal=FOCAL, q=quaternion(v.R), C=centre[v.cam],
                                           distortion=-k1[v.cam]) for v in sc.views],
               [(X[i], m) for i, m in enumerate(measures)])
    flip = np.diag([1.0, -1.0, -1.0])
    _write_bundler(folder / "bundle.rd.out", [dict(f=FOCAL, k1=k1[v.cam], k2=0.0, R=flip @ v.R, t=flip @ v.t) for v in sc.views],
                   [(X[i], m) for i, m in enumerate(measures)])
    cams = [(v.cam + 1, "SIMPLE_RADIAL", WIDTH, HEIGHT, [FOCAL, WIDTH / 2, HEIGHT / 2, k1[v.cam]]) if k1[v.cam] else
            (v.cam + 1, "SIMPLE_PINHOLE", WIDTH, HEIGHT, [FOCAL, WIDTH / 2, HEIGHT / 2]) for v in sc.views]
    images = [(v.cam, quaternion(v.R), v.t, v.cam + 1, f"view_{v.cam}.png", [(1.0, 1.0, i) for i in v.worldpoints]) for v in sc.views]
    _write_colmap(folder / "colmap", cams, images, [(i, X[i]) for i in range(len(X))])
    return sc
