"""Line-segment detection on the MI355X (k_lsd.hip, l3d_lsd.hip): Line3D::detectLineSegments with the LSD of
lsd_opencv.cpp, checked against the independent model of tests/lsd_model.py, on the reference's own images, end to
end through Line3D, and with the segment cache."""
import json
import os

import numpy as np
import pytest

from line3dpp_amd import _lib, io
from line3dpp_amd.api import Line3D
from line3dpp_amd.lsd import detect_line_segments, read_image_gray
from tests import lsd_model as M
from tests.lsd_scenes import edge_at_border, polygons

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lsd")
CAMS = json.load(open(os.path.join(GOLD, "cameras.json")))      # image file -> camera index in real_scene_c0.npz
# largest endpoint difference GPU vs model allowed (px); see DESIGN §11 for where differences can come from
EP_TOL = 0.0


def _compare(got, want, what):
    assert got.shape == want.shape, f"{what}: {len(got)} segments on the GPU, {len(want)} in the model"
    d = float(np.abs(got - want).max()) if len(got) else 0.0
    assert d <= EP_TOL, f"{what}: largest endpoint difference {d} px"


SYNTH = [(64, 48, 0), (65, 49, 1), (97, 131, 2), (160, 120, 3), (241, 179, 4), (320, 240, 5), (480, 360, 6)]


@pytest.mark.parametrize("w,h,seed", SYNTH)
def test_synthetic_images_equal_the_model(w, h, seed):
    img = polygons(w, h, seed)
    got = detect_line_segments([img])[0]
    want = M.detect(img)
    assert len(want) > 0 or w < 100
    _compare(got, want, f"{w}x{h}")


def test_flat_border_rgb_and_downscale_equal_the_model():
    flat = np.full((120, 160), 128, np.uint8)
    border = edge_at_border(173, 129)
    rgb = polygons(200, 150, 7, rgb=True)
    big = polygons(400, 300, 8)
    got = detect_line_segments([flat, border, rgb])
    assert len(got[0]) == 0
    _compare(got[1], M.detect(border), "edge in the last row / column")
    _compare(got[2], M.detect(rgb), "RGB")
    g2 = detect_line_segments([M.gray_rgb(rgb)])[0]
    assert np.array_equal(g2, got[2])
    dn = detect_line_segments([big], max_image_width=250)[0]
    _compare(dn, M.detect(big, max_image_width=250), "8U downscale")
    assert not np.array_equal(dn, detect_line_segments([big])[0])


def test_real_image_crops_equal_the_model():
    img = read_image_gray(os.path.join(GOLD, "img000055.jpg"))
    crops = [img[y:y + 240, x:x + 320] for (y, x) in [(0, 0), (1000, 1400), (2064, 2752)]]
    got = detect_line_segments(crops)
    for k, c in enumerate(crops):
        _compare(got[k], M.detect(c), f"crop {k}")


def _fixture_segments(cam):
    d = np.load(os.path.join(ROOT, "tests", "golden", "real_scene_c0.npz"))
    i = int(np.nonzero(d["cam"] == cam)[0][0])
    return d["segs"][d["seg_off"][i]:d["seg_off"][i + 1]]


def _coverage(fix, det):
    """per fixture segment: distance to the nearest detected segment (max of both endpoint distances, either
    orientation)"""
    a = np.linalg.norm(fix[:, None, :2] - det[None, :, :2], axis=2)
    b = np.linalg.norm(fix[:, None, 2:] - det[None, :, 2:], axis=2)
    c = np.linalg.norm(fix[:, None, :2] - det[None, :, 2:], axis=2)
    e = np.linalg.norm(fix[:, None, 2:] - det[None, :, :2], axis=2)
    return np.minimum(np.maximum(a, b), np.maximum(c, e)).min(axis=1)


COVER_FLOOR = 0.70     # measured on the MI355X: 75.9 % (img000055, cam 4) and 80.4 % (img000056, cam 3)


def test_full_size_images():
    names = sorted(CAMS)
    imgs = [read_image_gray(os.path.join(GOLD, n)) for n in names]
    assert all(im.shape == (2304, 3072) for im in imgs)
    batch, stats = detect_line_segments(imgs, stats=True)
    for n, segs, st in zip(names, batch, stats):
        assert 0 < len(segs) <= 3000 and st["segments"] == len(segs) and st["raw_segments"] >= len(segs)
        ln = np.hypot(segs[:, 0] - segs[:, 2], segs[:, 1] - segs[:, 3])
        assert (np.diff(ln) <= 0).all()
        dist = _coverage(_fixture_segments(CAMS[n]), segs)
        frac = float((dist <= 2.0).mean())
        print(f"{n} cam {CAMS[n]}: {len(segs)} segments ({st['raw_segments']} raw), {100 * frac:.1f} % of the fixture "
              f"within 2 px, median {np.median(dist):.2f} px")
        assert frac >= COVER_FLOOR
    single = [detect_line_segments([im])[0] for im in imgs]
    for a, b in zip(batch, single):
        assert a.tobytes() == b.tobytes()
    again = detect_line_segments(imgs)
    for a, b in zip(batch, again):
        assert a.tobytes() == b.tobytes()


def _views():
    d = np.load(os.path.join(ROOT, "tests", "golden", "real_scene_c0.npz"))
    out = []
    for n in sorted(CAMS):
        i = int(np.nonzero(d["cam"] == CAMS[n])[0][0])
        out.append((CAMS[n], read_image_gray(os.path.join(GOLD, n)), d["K"][i], d["R"][i], d["t"][i], d["median_depth"][i]))
    return out


def _result(g):
    assert g.matchImages()
    g.reconstruct3Dlines()
    ms = {cam: g.matches(cam) for cam in sorted(CAMS.values())}
    return ms, g.get3Dlines()


def _same(ra, rb):
    for cam in ra[0]:
        (ma, oa), (mb, ob) = ra[0][cam], rb[0][cam]
        assert ma.tobytes() == mb.tobytes() and np.array_equal(oa, ob)
    assert len(ra[1]) == len(rb[1])
    for a, b in zip(ra[1], rb[1]):
        for k in ("collinear3Dsegments", "residuals", "cluster_line"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
        assert a["reference_view"] == b["reference_view"]


def test_line3d_detects_when_given_images():
    views = _views()
    cams = [v[0] for v in views]
    segs = detect_line_segments([v[1] for v in views])
    g_img, g_seg, g_batch = Line3D(), Line3D(), Line3D()
    for (cam, img, K, R, t, md), s in zip(views, segs):
        nb = [c for c in cams if c != cam]
        g_img.addImage(cam, img, K, R, t, md, nb)
        assert g_img.last_status == 0
        g_seg.addImage(cam, (img.shape[1], img.shape[0]), K, R, t, md, nb, s)
    g_batch.addImages(cams, [v[1] for v in views], [v[2] for v in views], [v[3] for v in views], [v[4] for v in views],
                      [v[5] for v in views], [[c for c in cams if c != cam] for cam in cams])
    r = _result(g_seg)
    _same(_result(g_img), r)
    _same(_result(g_batch), r)
    # a flat image: no segments, a warning, and no view
    g_img.addImage(99, np.full((900, 1200), 10, np.uint8), views[0][2], views[0][3], views[0][4], 1.0, [cams[0]])
    assert g_img.last_status == _lib.L3D_ERR_NO_SEGMENTS and 99 not in g_img._M


def test_image_views_added_from_threads_keep_their_own_counts():
    """addImage from several threads on one Line3D (the reference's front ends call it from an OpenMP loop): each
    view is added with, and reports, its own segments -- not those of whichever detection ran last."""
    import threading
    views = _views()
    cams = [v[0] for v in views]
    segs = detect_line_segments([v[1] for v in views])
    assert len({len(s) for s in segs}) == len(segs)          # the images differ in segment count
    g = Line3D()
    ths = [threading.Thread(target=g.addImage, args=(cam, img, K, R, t, md, [c for c in cams if c != cam]))
           for (cam, img, K, R, t, md) in views]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    coords = np.zeros(4, np.float32)
    for (cam, *_), s in zip(views, segs):
        assert g._M[cam] == len(s)
        assert _lib.load().l3d_get_segment_coords2d(g.h, cam, len(s) - 1, _lib.ptr(coords)) == 0
        assert np.array_equal(coords, s[-1])
    assert g.matchImages()
    for (cam, *_), s in zip(views, segs):
        m, off = g.matches(cam)
        assert len(off) == len(s) + 1


def test_cap_against_the_model():
    """max_segments below the number of filtered segments: the host cap keeps the first ones in the reference's
    priority-queue order, as the model's does"""
    imgs = [polygons(320, 240, 5), polygons(241, 179, 4, rgb=True)]
    for cap in (1, 5):
        got = detect_line_segments(imgs, max_segments=cap)
        for img, g in zip(imgs, got):
            want = M.detect(img, max_segments=cap)
            assert len(want) == cap
            _compare(g, want, f"cap {cap}")


def test_segment_cache(tmp_path):
    L = _lib.load()
    img = polygons(900, 700, 11)
    K = np.array([[800, 0, 450], [0, 800, 350], [0, 0, 1]], np.float64)
    R, t = np.eye(3), np.zeros(3)
    det0 = L.l3d_debug_counter(b"lsd_images_detected")
    g = Line3D(output_folder=str(tmp_path), load_segments=True, max_img_width=800)
    g.addImage(3, img, K, R, t, 1.0, [1])
    assert g.last_status == 0 and L.l3d_debug_counter(b"lsd_images_detected") == det0 + 1
    path = tmp_path / "L3D++_data" / io.segment_cache_name(3, 800, 622)
    assert path.exists()
    want = detect_line_segments([img], max_image_width=800)[0]
    assert np.array_equal(io.read_segment_cache(str(path)), want)
    det1, load1 = L.l3d_debug_counter(b"lsd_images_detected"), L.l3d_debug_counter(b"lsd_cache_loads")
    g2 = Line3D(output_folder=str(tmp_path), load_segments=True, max_img_width=800)
    g2.addImage(3, img, K, R, t, 1.0, [1])
    assert g2.last_status == 0 and g2._M[3] == len(want)
    assert L.l3d_debug_counter(b"lsd_images_detected") == det1 and L.l3d_debug_counter(b"lsd_cache_loads") == load1 + 1
    # a cache written by someone else wins over detection
    foreign = np.array([[10, 10, 300, 20], [50, 400, 60, 30]], np.float32)
    path.write_bytes(io.format_segment_cache(foreign))
    g3 = Line3D(output_folder=str(tmp_path), load_segments=True, max_img_width=800)
    g3.addImage(3, img, K, R, t, 1.0, [1])
    assert g3._M[3] == 2
    coords = np.zeros(4, np.float32)
    for k in range(2):
        assert L.l3d_get_segment_coords2d(g3.h, 3, k, _lib.ptr(coords)) == 0
        assert np.array_equal(coords, foreign[k])
    # without load_segments nothing is read or written
    g4 = Line3D(output_folder=str(tmp_path / "other"), load_segments=False)
    g4.addImage(3, img, K, R, t, 1.0, [1])
    assert not (tmp_path / "other").exists()


def test_facade_detects_when_given_images(tmp_path):
    import struct
    import subprocess
    exe = str(tmp_path / "lsd_facade")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "lsd_facade.cpp"), "-o", exe, "-L" + lib_dir,
                           "-ll3dpp_hip", "-Wl,-rpath," + lib_dir, "-pthread"])
    views = _views()
    cams = [v[0] for v in views]
    segs = detect_line_segments([v[1] for v in views])
    path = str(tmp_path / "scene.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(views)))
        for (cam, img, K, R, t, md), s in zip(views, segs):
            nb = [c for c in cams if c != cam]
            f.write(struct.pack("<5I", cam, img.shape[1], img.shape[0], len(nb), len(s)))
            for a in (K, R, t):
                f.write(np.ascontiguousarray(a, np.float64).tobytes())
            f.write(struct.pack("<f", float(md)))
            f.write(np.asarray(nb, np.uint32).tobytes())
            f.write(np.ascontiguousarray(img).tobytes())
            f.write(np.ascontiguousarray(s, np.float32).tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "counts=1" in out.stdout and "identical=1" in out.stdout
