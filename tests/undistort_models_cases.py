"""The inputs of the device-against-model comparison of undistortion by camera model, shared by
tests/test_gpu_undistort_models.py (device against tests/undistort_models_model.py) and
tests/test_undistort_models_host.py (the model against itself with every sqrt, atan and division moved by a few ulp),
so that the agreement cap is shown to be robust on exactly the inputs it is applied to."""
import numpy as np

MODELS = ("FULL_OPENCV", "OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "FOV")
PARAMS = {
    "FULL_OPENCV": (-0.1, 0.02, 1e-3, -2e-3, 3e-3, 0.01, -0.002, 0.0005),
    "OPENCV_FISHEYE": (-0.03, 0.005, -0.001, 0.0002),
    "SIMPLE_RADIAL_FISHEYE": (-0.04,),
    "RADIAL_FISHEYE": (-0.03, 0.006),
    "FOV": (0.9,),
}
# (width, height, focal length, parameters): the corners of the map leave the image (asserted on the model)
STRONG = {
    "FULL_OPENCV": (640, 480, 40.0, (1.0, 1.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.0)),
    "OPENCV_FISHEYE": (640, 480, 40.0, (1.0, 1.0, 0.0, 0.0)),
    "SIMPLE_RADIAL_FISHEYE": (640, 480, 40.0, (10.0,)),
    "RADIAL_FISHEYE": (640, 480, 40.0, (1.0, 1.0)),
    "FOV": (640, 480, 2000.0, (2.5,)),
}
SIZES = [(64, 48), (65, 49), (641, 479), (1920, 1080)]
NARROW = [(3, 7), (5, 2)]           # a thread's 4 pixels cross row ends


def K_of(w, h, f=None, fy=None, cx=None, cy=None):
    f = 0.9 * w if f is None else f
    return np.array([[f, 0.0, w / 2 if cx is None else cx], [0.0, f if fy is None else fy, h / 2 if cy is None else cy],
                     [0.0, 0.0, 1.0]])


def image(w, h, seed, rgb=False):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (40 + 30 * np.sin(xx / 7.0) + 25 * np.cos(yy / 5.0) + ((xx // 16 + yy // 16) % 2) * 90).astype(np.int64)
    img = np.clip(base[..., None] + rng.integers(0, 40, (h, w, 3)), 0, 255) if rgb else np.clip(base + rng.integers(0, 40, (h, w)), 0, 255)
    return img.astype(np.uint8)


def padded(img, extra):
    """the same pixels as a view with a longer row stride"""
    shape = (img.shape[0], img.shape[1] + extra) + img.shape[2:]
    big = np.zeros(shape, np.uint8)
    big[:, :img.shape[1]] = img
    return big[:, :img.shape[1]]


def cases(model):
    """-> list of (name, image, K, params, K_new or None) for one camera model"""
    p = PARAMS[model]
    seed = 100 * MODELS.index(model)
    out = []
    for k, (w, h) in enumerate(SIZES):
        out.append((f"{w}x{h}", image(w, h, seed + k), K_of(w, h), p, None))
    for k, (w, h) in enumerate(NARROW):
        out.append((f"{w}x{h}", image(w, h, seed + 10 + k), K_of(w, h), p, None))
        out.append((f"{w}x{h} rgb", image(w, h, seed + 12 + k, rgb=True), K_of(w, h, f=0.7 * w, fy=0.9 * h, cx=0.3 * w, cy=0.6 * h), p, None))
    w, h = 641, 479
    K = K_of(w, h, f=560.0, fy=602.5, cx=281.25, cy=260.75)
    grey, rgb = image(w, h, seed + 20), image(w, h, seed + 21, rgb=True)
    out.append(("off-centre grey", grey, K, p, None))
    out.append(("off-centre rgb", rgb, K, p, None))
    out.append(("off-centre grey padded", padded(grey, 37), K, p, None))
    out.append(("off-centre rgb padded", padded(rgb, 5), K, p, None))
    half = K.copy()
    half[0, 0] /= 2
    half[1, 1] /= 2
    out.append(("K_new half focal", grey, K, p, half))
    sw, sh, sf, sp = STRONG[model]
    out.append(("strong", image(sw, sh, seed + 30), K_of(sw, sh, f=sf), sp, None))
    return out


def cap(img):
    """the agreement condition of DESIGN §15: at most 1 pixel in 100 000 of an image may differ, at least 1 allowed"""
    n_pix = img.shape[0] * img.shape[1]
    return max(1, n_pix // 100000)


def compare(got, want):
    """(number of differing pixels, largest difference in grey levels)"""
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    if d.ndim == 3:
        d = d.max(axis=2)
    return int((d != 0).sum()), int(d.max()) if d.size else 0
