"""Line-segment detection: Line3D::detectLineSegments (line3D.cc:243-370) on the GPU (k_lsd.hip), batched over images.

`detect_line_segments` is the stage on its own: grey conversion, the max-width downscale, LSD (lsd_opencv.cpp,
LSD_REFINE_ADV), the length filter, the length order and the cap.  `Line3D.addImage` / `addImages` (api.py) run the
same stage, with the segment cache, when they are given an image and no segments.  Detection expects undistorted
images: `undistort_images` is Line3D::undistortImage (line3D.cc:83-109) on the GPU (k_undistort.hip), batched over images,
which the reference's front ends call before addImage.  `undistort_images_model` is the same for COLMAP's
camera models beyond those five coefficients: FULL_OPENCV, the fisheye family and FOV.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr

L3D_DEF_MAX_NUM_SEGMENTS = 3000


def as_image(img):
    """uint8 HxW (grey) or HxWx3 (first channel = R) ndarray -> (l3d_image, the array it points into).  Rows may be
    padded (a view such as big[:, :w] keeps its row stride); an array whose rows are not packed pixels is copied."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise TypeError("image type not supported! must be uint8 HxW (gray) or HxWx3 (RGB)")
    ch = 1 if a.ndim == 2 else 3
    if not (a.strides[-1] == 1 and (ch == 1 or a.strides[1] == 3) and a.strides[0] >= a.shape[1] * ch):
        a = np.ascontiguousarray(a)
    return _lib.Image(a.ctypes.data, a.shape[1], a.shape[0], ch, a.strides[0]), a


def image_array(images):
    """-> (ctypes array of l3d_image, arrays that must stay alive while it is used)"""
    imgs, keep = zip(*[as_image(im) for im in images]) if len(images) else ((), ())
    arr = (_lib.Image * max(len(imgs), 1))(*imgs)
    return arr, keep


def fetch(L, h, counts):
    """the segments of the last detection on context h, split per image"""
    n = C.c_uint64(0)
    L.l3d_get_detected_segments(h, None, 0, C.byref(n))
    flat = np.zeros((max(n.value, 1), 4), np.float32)
    if n.value:
        L.l3d_get_detected_segments(h, ptr(flat), n.value, C.byref(n))
    out, o = [], 0
    for c in counts:
        out.append(flat[o:o + int(c)].copy())
        o += int(c)
    return out


def detect_line_segments(images, max_image_width=-1, max_segments=L3D_DEF_MAX_NUM_SEGMENTS, device=0, stats=False):
    """LSD on a list of images in one batch -> list of [n,4] float32 (x1, y1, x2, y2), longest first, as
    Line3D::detectLineSegments hands them to the view.  stats=True also returns the per-image l3d_detect_stats."""
    L = _lib.load()
    images = list(images)
    h = L.l3d_create(int(device), None)
    if not h:
        raise RuntimeError("l3d_create failed: " + _lib.last_error())
    h = C.c_void_p(h)
    try:
        arr, keep = image_array(images)
        counts = np.zeros(max(len(images), 1), np.uint32)
        rc = L.l3d_detect_segments(h, len(images), arr, int(max_image_width), int(max_segments), ptr(counts))
        if rc != 0:
            raise RuntimeError(f"l3d_detect_segments failed [{rc}]: {_lib.last_error()}")
        segs = fetch(L, h, counts[:len(images)])
        if not stats:
            return segs
        return segs, last_stats(L, h)
    finally:
        L.l3d_destroy(h)


def last_stats(L, h):
    n = C.c_uint32(0)
    L.l3d_get_detect_stats(h, None, 0, C.byref(n))
    st = (_lib.DetectStats * max(n.value, 1))()
    L.l3d_get_detect_stats(h, st, n.value, C.byref(n))
    return [{k: getattr(st[i], k) for k, _ in _lib.DetectStats._fields_ if k != "reserved"} for i in range(n.value)]


def lsd_stages(images, max_image_width=-1, device=0):
    """l3d_debug_lsd_stages (test hook): what every device stage of one detection batch left behind -> per image a dict
    of gray, small (u8), blur (f64), deg (f32, -1024 = undefined), mod (f64), raw ([n,4] f32 in detection order,
    LSD-input pixels) and the kernel's counts: raw_segments, overflow, seeds, nfa_evals, max_grad_bits, down, stats"""
    L = _lib.load()
    images = list(images)
    n = len(images)
    h = L.l3d_create(int(device), None)
    if not h:
        raise RuntimeError("l3d_create failed: " + _lib.last_error())
    h = C.c_void_p(h)
    try:
        arr, keep = image_array(images)
        st = (_lib.LsdStages * max(n, 1))()
        for query in (1, 0):
            rc = L.l3d_debug_lsd_stages(h, n, arr, int(max_image_width), query, st)
            if rc != 0:
                raise RuntimeError(f"l3d_debug_lsd_stages failed [{rc}]: {_lib.last_error()}")
            if query:
                maps = [{"gray": np.zeros((a.shape[0], a.shape[1]), np.uint8),
                         "small": np.zeros((s.gh, s.gw), np.uint8), "blur": np.zeros((s.gh, s.gw), np.float64),
                         "deg": np.zeros((s.sh, s.sw), np.float32), "mod": np.zeros((s.sh, s.sw), np.float64),
                         "raw": np.zeros((s.raw_cap, 4), np.float32)} for s, a in zip(st, keep)]
                for s, m in zip(st, maps):
                    s.gray, s.small_gray, s.blur = m["gray"].ctypes.data, m["small"].ctypes.data, m["blur"].ctypes.data
                    s.deg, s.mod, s.raw4 = m["deg"].ctypes.data, m["mod"].ctypes.data, m["raw"].ctypes.data
        out = []
        for s, m in zip(st, maps):
            m["raw"] = m["raw"][:s.raw_segments].copy()
            m.update({k: getattr(s, k) for k in ("raw_segments", "overflow", "seeds", "nfa_evals", "max_grad_bits", "down")})
            m["stats"] = {k: getattr(s.stats, k) for k, _ in _lib.DetectStats._fields_ if k != "reserved"}
            out.append(m)
        return out
    finally:
        L.l3d_destroy(h)


def distortion(K, radial, tangential):
    """l3d_distortion of undistortImage's arguments: K 3x3, radial (k1, k2, k3), tangential (p1, p2)"""
    d = _lib.Distortion()
    d.K[:] = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
    d.radial[:] = [float(v) for v in np.asarray(radial, np.float64).reshape(3)]
    d.tangential[:] = [float(v) for v in np.asarray(tangential, np.float64).reshape(2)]
    return d


def undistort_images(images, Ks, radials, tangentials, device=0):
    """Line3D::undistortImage (line3D.cc:83-109) for a list of images in one batch on the GPU -> list of uint8 ndarrays of
    the inputs' shapes.  Per image: K 3x3 (fx, fy, cx, cy are read), radial = (k1, k2, k3), tangential = (p1, p2), as
    the front ends hand them to undistortImage (io.front_end_undistortion).  DESIGN §12 defines the result."""
    L = _lib.load()
    images = list(images)
    n = len(images)
    if not len(Ks) == len(radials) == len(tangentials) == n:
        raise ValueError("one K, radial and tangential per image")
    views = [as_image(im) for im in images]
    arr = (_lib.Image * max(n, 1))(*[v[0] for v in views])
    dist = (_lib.Distortion * max(n, 1))(*[distortion(*a) for a in zip(Ks, radials, tangentials)])
    outs = [np.empty(v[1].shape, np.uint8) for v in views]
    ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    h = L.l3d_create(int(device), None)
    if not h:
        raise RuntimeError("l3d_create failed: " + _lib.last_error())
    h = C.c_void_p(h)
    try:
        rc = L.l3d_undistort_images(h, n, arr, dist, ptrs)
        if rc != 0:
            raise RuntimeError(f"l3d_undistort_images failed [{rc}]: {_lib.last_error()}")
        return outs
    finally:
        L.l3d_destroy(h)


def camera_model(model, K, params, K_new=None):
    """l3d_camera_model: model = COLMAP's name, K 3x3 of the input image, params = the model's distortion parameters in
    COLMAP's order (missing ones 0), K_new 3x3 of the output image (None: K)"""
    if model not in _lib.CAMERA_MODELS:
        raise ValueError(f"camera model {model} unknown!")
    p = [float(v) for v in np.asarray(params, np.float64).reshape(-1)]
    if len(p) > _lib.CAMERA_MODEL_PARAMS[model]:
        raise ValueError(f"camera model {model} takes {_lib.CAMERA_MODEL_PARAMS[model]} distortion parameter(s), not {len(p)}")
    m = _lib.CameraModel()
    m.model = _lib.CAMERA_MODELS[model]
    m.K[:] = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
    m.params[:] = p + [0.0] * (8 - len(p))
    if K_new is not None:
        m.K_new[:] = [float(v) for v in np.asarray(K_new, np.float64).reshape(9)]
    return m


def undistort_images_model(images, models, Ks, params, K_new=None, device=0):
    """Undistortion by camera model for a list of images in one batch on the GPU (k_undistort_model) -> list
    of uint8 ndarrays of the inputs' shapes.  Per image: COLMAP's model name (FULL_OPENCV, OPENCV_FISHEYE,
    SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE, FOV), K 3x3, the model's distortion parameters in COLMAP's order
    (io.front_end_camera_model); K_new: None, or per image the camera matrix of the output image (None: K)."""
    L = _lib.load()
    images = list(images)
    n = len(images)
    K_new = [None] * n if K_new is None else list(K_new)
    if not len(models) == len(Ks) == len(params) == len(K_new) == n:
        raise ValueError("one model, K and parameter list per image")
    views = [as_image(im) for im in images]
    arr = (_lib.Image * max(n, 1))(*[v[0] for v in views])
    cams = (_lib.CameraModel * max(n, 1))(*[camera_model(*a) for a in zip(models, Ks, params, K_new)])
    outs = [np.empty(v[1].shape, np.uint8) for v in views]
    ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
    h = L.l3d_create(int(device), None)
    if not h:
        raise RuntimeError("l3d_create failed: " + _lib.last_error())
    h = C.c_void_p(h)
    try:
        rc = L.l3d_undistort_images_model(h, n, arr, cams, ptrs)
        if rc != 0:
            raise RuntimeError(f"l3d_undistort_images_model failed [{rc}]: {_lib.last_error()}")
        return outs
    finally:
        L.l3d_destroy(h)


def read_image_gray(path):
    """8-bit grey image of a file as cv::imread(path, CV_LOAD_IMAGE_GRAYSCALE) gives it to the reference: for JPEG,
    libjpeg's own grey decode (the Y channel, through PIL's draft mode) rather than a conversion of the RGB decode."""
    from PIL import Image
    with Image.open(path) as im:
        if im.format == "JPEG":
            im.draft("L", im.size)
        if im.mode != "L":
            im = im.convert("L")
        return np.asarray(im, np.uint8).copy()
