"""The dataset of tests/test_gpu_front_end_colmap_models.py: the scene of tests/front_end_dataset.py seen through cameras
whose distortion is real, written as a COLMAP binary model and as the text form of the same model.

Two views are taken through an OPENCV_FISHEYE camera, one through a FOV camera, the rest through pinholes.  The forward
models are closed form, so nothing is inverted to render: every polygon edge is sampled densely in 3D, each
sample goes through the pinhole projection and the camera's distortion, and the curved polygon is drawn at twice the
size and box-filtered down, as tests/front_end_dataset.py draws its straight ones.
"""
import numpy as np

from tests import undistort_models_model as M
from tests.front_end_dataset import BAR, FOCAL, HALF, HEIGHT, N_VIEWS, WIDTH, make, quaternion, structure  # noqa: F401

# camera -> (COLMAP model, its distortion parameters)
CAMERAS = {1: ("OPENCV_FISHEYE", (-0.03, 0.005, -0.001, 0.0002)), 4: ("OPENCV_FISHEYE", (-0.02, 0.004, 0.0, 0.0001)),
           2: ("FOV", (0.9,))}
EDGE_SAMPLES = 200


def colmap_camera(view):
    """(camera id, model, width, height, parameter list) of a view, in COLMAP's order"""
    fx, fy, cx, cy = view.K[0, 0], view.K[1, 1], view.K[0, 2], view.K[1, 2]
    if view.cam in CAMERAS:
        model, p = CAMERAS[view.cam]
        return (view.cam + 1, model, WIDTH, HEIGHT, [fx, fy, cx, cy] + list(p))
    return (view.cam + 1, "SIMPLE_PINHOLE", WIDTH, HEIGHT, [fx, cx, cy])


def render(view, segs, scale=2):
    """grey uint8 HEIGHT x WIDTH image of the facade and its bars as `view` sees them through its camera model"""
    from PIL import Image, ImageDraw
    model = CAMERAS.get(view.cam)

    def project(corners):
        corners = [np.asarray(c, np.float64) for c in corners]
        pts = []
        for a, b in zip(corners, corners[1:] + corners[:1]):          # every edge, sampled: it is a curve in the image
            n = EDGE_SAMPLES if model else 1
            pts += [a + (b - a) * (k / n) for k in range(n)]
        Xc = (view.R @ np.asarray(pts).T).T + view.t
        assert (Xc[:, 2] > 1.0).all()
        x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
        if model:
            x, y = M.distort(model[0], model[1], x, y)
        u, v = view.K[0, 0] * x + view.K[0, 2], view.K[1, 1] * y + view.K[1, 2]
        return [((a + 0.5) * scale, (b + 0.5) * scale) for a, b in zip(u, v)]

    im = Image.new("L", (WIDTH * scale, HEIGHT * scale), 110)
    draw = ImageDraw.Draw(im)
    h = HALF
    draw.polygon(project([[h, -h, -h], [h, h, -h], [h, h, h], [h, -h, h]]), fill=225)
    for p, q in segs:
        d = (q - p) / np.linalg.norm(q - p)
        side = np.cross(d, [1.0, 0.0, 0.0]) * (BAR / 2)
        draw.polygon(project([p - side, q - side, q + side, p + side]), fill=30)
    return np.asarray(im.resize((WIDTH, HEIGHT), Image.BOX), np.uint8).copy()


def model_records(sc, X):
    """(cameras, images, points) as the writers of tests/test_colmap_binary.py take them"""
    cams = [colmap_camera(v) for v in sc.views]
    images = [(v.cam, quaternion(v.R), v.t, v.cam + 1, f"view_{v.cam}.png", [(1.0, 1.0, i) for i in v.worldpoints]) for v in sc.views]
    return cams, images, [(i, X[i]) for i in range(len(X))]


def write(folder):
    """renders the images into folder/images and writes folder/colmap_bin (cameras.bin, images.bin, points3D.bin) and
    folder/colmap_txt (the same model as text) -> the scene"""
    from PIL import Image
    from tests.test_colmap_binary import binary_files, write_binary, write_text
    sc, X, segs = make()
    assert len(segs) >= 12
    (folder / "images").mkdir(parents=True)
    for v in sc.views:
        Image.fromarray(render(v, segs)).save(folder / "images" / f"view_{v.cam}.png")
    cams, images, points = model_records(sc, X)
    write_binary(folder / "colmap_bin", binary_files(cams, images, points))
    write_text(folder / "colmap_txt", cams, images, points)
    return sc
