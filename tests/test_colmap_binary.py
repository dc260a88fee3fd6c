"""COLMAP's binary model (cameras.bin, images.bin, points3D.bin) and its camera models beyond the reference's six, through
l3d_sfm_open_colmap, io.read_colmap that wraps it, and the Python model of the format, tests/sfm_readers_model.py (M
below).  What is pinned on hand-computed values is pinned for the wrapper and for the model.  The files are
written here from the documented layout: no file written by COLMAP itself is at hand.  No GPU."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from line3dpp_amd import _lib as L
from line3dpp_amd import io
from tests import sfm_readers_model as M

READERS = (io, M)          # the package's wrapper of the library, and the model
NO_POINT = 2 ** 64 - 1
MODEL_IDS = {name: k for k, (name, _) in enumerate(io.COLMAP_MODEL_IDS)}


def _lib():
    return L.load()


def scene(rng):
    """one camera of each of the ten accepted model ids; images with and without points, a 2D point without a 3D point,
    a track that points3D does not hold, an image of an unknown camera and a repeated image id"""
    f, cx, cy = 1250.125, 960.5, 540.25
    cams = [(1, "SIMPLE_PINHOLE", 1920, 1080, [f, cx, cy]), (2, "PINHOLE", 1920, 1080, [f, f * 1.01, cx, cy]),
            (3, "SIMPLE_RADIAL", 1920, 1080, [f, cx, cy, -0.05]), (4, "RADIAL", 1920, 1080, [f, cx, cy, -0.05, 0.01]),
            (5, "OPENCV", 1920, 1080, [f, f * 1.01, cx, cy, -0.05, 0.01, 1e-3, -2e-3]),
            (6, "OPENCV_FISHEYE", 1920, 1080, [f, f * 1.01, cx, cy, -0.03, 0.005, -0.001, 0.0002]),
            (7, "FULL_OPENCV", 3072, 2304, [f, f * 1.01, cx, cy, -0.1, 0.02, 1e-3, -2e-3, 3e-3, 0.01, -0.002, 0.0005]),
            (8, "FOV", 1280, 720, [f, f * 1.01, cx, cy, 0.9]),
            (9, "SIMPLE_RADIAL_FISHEYE", 1280, 720, [f, cx, cy, -0.04]),
            (12, "RADIAL_FISHEYE", 1280, 720, [f, cx, cy, -0.03, 0.006])]
    points = [(100 + 3 * k, rng.normal(size=3) * 4) for k in range(120)]
    images = []
    cam_ids = [c[0] for c in cams] + [77, 3, 6]                  # camera 77 does not exist: the image is dropped
    for i, cid in enumerate(cam_ids):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        if i == 2:
            q *= 3.0
        pts = [(float(rng.uniform(0, 1900)), float(rng.uniform(0, 1000)), points[k][0])
               for k in rng.choice(len(points), size=30, replace=False)]
        pts += [(1.0, 2.0, NO_POINT), (3.0, 4.0, 99999)]          # an unmatched feature; a track that points3D does not hold
        if i == 4:
            pts = [(5.0, 6.0, NO_POINT)]                         # an image without worldpoints
        if i == 7:
            pts = []                                             # an image without 2D points at all
        iid = 10 + 5 * i if i != 11 else 20                      # the image of index 11 repeats the id of index 2
        images.append((iid, q, rng.normal(size=3) * 6, cid, f"sub/img_{i}.jpg", pts))
    return cams, images, points


def _g(x):
    return f"{float(x):.17g}"


def write_text(folder, cams, images, points):
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for cid, model, w, h, params in cams:
            f.write(f"{cid} {model} {w} {h} " + " ".join(_g(p) for p in params) + "\n")
    with open(os.path.join(folder, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n")
        for iid, q, t, cid, name, pts in images:
            f.write(f"{iid} " + " ".join(_g(x) for x in list(q) + list(t)) + f" {cid} {name}\n")
            f.write(" ".join(f"{_g(x)} {_g(y)} {-1 if pid == NO_POINT else pid}" for x, y, pid in pts) + "\n")
    with open(os.path.join(folder, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n")
        for pid, X in points:
            f.write(f"{pid} " + " ".join(_g(x) for x in X) + " 128 128 128 0.5 1 2 3 4\n")


def binary_files(cams, images, points, model_ids=MODEL_IDS):
    """-> dict(file name -> bytes) in COLMAP's documented little-endian layout"""
    c = struct.pack("<Q", len(cams))
    for cid, model, w, h, params in cams:
        c += struct.pack("<IiQQ", cid, model_ids[model] if isinstance(model, str) else model, w, h)
        c += struct.pack(f"<{len(params)}d", *params)
    i = struct.pack("<Q", len(images))
    for iid, q, t, cid, name, pts in images:
        i += struct.pack("<I7dI", iid, *q, *t, cid) + name.encode() + b"\0" + struct.pack("<Q", len(pts))
        for x, y, pid in pts:
            i += struct.pack("<ddQ", x, y, pid)
    p = struct.pack("<Q", len(points))
    for k, (pid, X) in enumerate(points):
        track = [(7, 11), (8, 12), (9, 13)][:k % 4]
        p += struct.pack("<Q3d3BdQ", pid, *X, 128, 127, 126, 0.5, len(track))
        for a, b in track:
            p += struct.pack("<II", a, b)
    return {"cameras.bin": c, "images.bin": i, "points3D.bin": p}


def write_binary(folder, files):
    os.makedirs(folder, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(folder, name), "wb") as f:
            f.write(data)


def _same_python(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y)                                    # the same keys in the same order
        for k in ("id", "camera", "name", "width", "height", "model", "params", "worldpoints", "median_depth"):
            assert x[k] == y[k] and type(x[k]) is type(y[k]), k
        for k in ("K", "R", "t", "C", "radial", "tangential"):
            assert x[k].dtype == np.float64 and x[k].tobytes() == y[k].tobytes(), k


def c_read(folder):
    """l3d_sfm_open_colmap -> (status, message, list of dicts like read_colmap's)"""
    lib = _lib()
    h = C.c_void_p()
    rc = lib.l3d_sfm_open_colmap(str(folder).encode(), C.byref(h))
    if rc != 0:
        assert not h.value
        return rc, lib.l3d_last_error().decode(), None
    out = []
    for i in range(lib.l3d_sfm_num_images(h)):
        im = L.SfmImage()
        assert lib.l3d_sfm_get_image(h, i, C.byref(im)) == 0
        ids = np.zeros(max(im.n_worldpoints, 1), np.uint32)
        assert lib.l3d_sfm_get_worldpoints(h, i, L.ptr(ids), im.n_worldpoints) == 0
        n = C.c_uint32(0)
        params = (C.c_double * 12)()
        model = lib.l3d_sfm_get_camera_params(h, i, params, 12, C.byref(n))
        cm = L.CameraModel()
        assert lib.l3d_sfm_get_camera_model(h, i, C.byref(cm)) == 0
        out.append(dict(id=im.id, camera=im.camera, name=im.name.decode(), width=im.width, height=im.height,
                        K=np.array(im.K).reshape(3, 3), R=np.array(im.R).reshape(3, 3), t=np.array(im.t), C=np.array(im.C),
                        radial=np.array(im.radial), tangential=np.array(im.tangential), model=model.decode(),
                        params=list(params[:n.value]), worldpoints=ids[:im.n_worldpoints].tolist(),
                        median_depth=np.float32(im.median_depth) if im.n_worldpoints else None,
                        camera_model=(cm.model, list(cm.K), list(cm.params), list(cm.K_new))))
    assert lib.l3d_sfm_get_camera_model(h, len(out), C.byref(L.CameraModel())) != 0
    lib.l3d_sfm_close(h)
    return 0, "", out


def _same_c(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in ("id", "camera", "name", "width", "height", "model", "params", "worldpoints", "median_depth", "camera_model"):
            assert x[k] == y[k], k
        for k in ("K", "R", "t", "C", "radial", "tangential"):
            assert x[k].tobytes() == y[k].tobytes(), k


def test_binary_and_text_read_identically(tmp_path):
    cams, images, points = scene(np.random.default_rng(8))
    write_text(tmp_path / "txt", cams, images, points)
    write_binary(tmp_path / "bin", binary_files(cams, images, points))
    for reader in READERS:
        txt, bin_ = reader.read_colmap(str(tmp_path / "txt")), reader.read_colmap(str(tmp_path / "bin"))
        _same_python(txt, bin_)
        _read_as_written(bin_, cams, images)
    # the C-ABI: text and binary identical, and equal to the model
    bin_ = M.read_colmap(str(tmp_path / "bin"))
    rc, _, ctxt = c_read(tmp_path / "txt")
    rc2, _, cbin = c_read(tmp_path / "bin")
    assert rc == 0 and rc2 == 0
    _same_c(ctxt, cbin)
    for c, p in zip(cbin, bin_):
        for k in ("id", "camera", "name", "width", "height", "model", "params", "worldpoints"):
            assert c[k] == p[k], k
        for k in ("K", "R", "t", "radial", "tangential"):
            assert c[k].tobytes() == p[k].tobytes(), k
        assert np.allclose(c["C"], p["C"], rtol=0, atol=1e-12)          # (Eigen's product order against numpy's)
        if p["median_depth"] is None:
            assert c["median_depth"] is None
        else:
            assert abs(float(c["median_depth"]) - float(p["median_depth"])) <= 2e-7 * float(p["median_depth"])
        # l3d_sfm_get_camera_model is io.front_end_camera_model's answer without its thresholds
        number, K, params, K_new = c["camera_model"]
        assert K == list(p["K"].reshape(9)) and not any(K_new)
        if p["model"] in L.CAMERA_MODELS:
            first, n = io._COLMAP_DISTORTION[p["model"]]
            assert number == L.CAMERA_MODELS[p["model"]] and params == p["params"][first:first + n] + [0.0] * (8 - n)
        else:
            assert number == 0 and not any(params)


def _read_as_written(bin_, cams, images):
    # what was read: file order, the image of camera 77 dropped, both entries of the repeated id 20 with the last pose
    assert [g["id"] for g in bin_] == [10, 15, 20, 25, 30, 35, 40, 45, 50, 55, 20, 70]
    assert bin_[2]["camera"] == bin_[10]["camera"] == 3 and bin_[2]["R"].tobytes() == bin_[10]["R"].tobytes()
    assert bin_[2]["worldpoints"] == bin_[10]["worldpoints"] == [p for _, _, p in images[11][5] if p != NO_POINT]
    by_cam = {g["camera"]: g for g in bin_}
    for cid, model, w, h, params in cams:
        g = by_cam[cid]
        assert g["model"] == model and g["params"] == params and (g["width"], g["height"]) == (w, h)
    for g, idx in zip(bin_, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12]):
        want = [p for _, _, p in images[idx][5] if p != NO_POINT] if g["id"] != 20 else bin_[10]["worldpoints"]
        assert g["worldpoints"] == want and 99999 in want or not want
        assert (g["median_depth"] is None) == (not want)
    assert bin_[4]["worldpoints"] == [] and bin_[7]["worldpoints"] == []
    # the new models: K from the focal lengths and the principal point, the five coefficients zero
    f, cx, cy = 1250.125, 960.5, 540.25
    for cid, fy in ((6, f * 1.01), (8, f * 1.01), (9, f), (12, f)):
        g = by_cam[cid]
        assert np.array_equal(g["K"], [[f, 0, cx], [0, fy, cy], [0, 0, 1]]) and not g["radial"].any() and not g["tangential"].any()
    assert np.array_equal(by_cam[7]["radial"], [-0.1, 0.02, 3e-3]) and by_cam[7]["params"][9:] == [0.01, -0.002, 0.0005]


def test_a_folder_with_text_and_binary_takes_the_text(tmp_path):
    rng = np.random.default_rng(9)
    cams, images, points = scene(rng)
    write_text(tmp_path / "both", cams, images, points)
    other = scene(rng)
    write_binary(tmp_path / "both", binary_files(*other))
    write_text(tmp_path / "txt", cams, images, points)
    for reader in READERS:
        _same_python(reader.read_colmap(str(tmp_path / "both")), reader.read_colmap(str(tmp_path / "txt")))
    _same_c(c_read(tmp_path / "both")[2], c_read(tmp_path / "txt")[2])
    # one .bin file missing and no cameras.txt: the text files are looked for.  The model fails on opening the first,
    # the library (and so the wrapper) with the reference's message
    files = binary_files(cams, images, points)
    del files["points3D.bin"]
    write_binary(tmp_path / "two", files)
    with pytest.raises(OSError, match="cameras.txt"):
        M.read_colmap(str(tmp_path / "two"))
    with pytest.raises(ValueError, match="does not exist"):
        io.read_colmap(str(tmp_path / "two"))
    rc, msg, _ = c_read(tmp_path / "two")
    assert rc == -1 and "does not exist" in msg


@pytest.mark.parametrize("model", [10, 11, -1])
def test_unknown_binary_model_ids(tmp_path, model):
    cams, images, points = scene(np.random.default_rng(10))
    cams[3] = (4, model, 640, 480, [1.0] * 12)
    write_binary(tmp_path / "bad", binary_files(cams, images, points))
    name = "THIN_PRISM_FISHEYE" if model == 10 else str(model)
    for reader in READERS:
        with pytest.raises(ValueError, match=f"camera model {name} unknown!"):
            reader.read_colmap(str(tmp_path / "bad"))
    rc, msg, _ = c_read(tmp_path / "bad")
    assert rc == -1 and msg == f"camera model {name} unknown!"


def test_unknown_text_models_keep_their_message(tmp_path):
    cams, images, points = scene(np.random.default_rng(10))
    for name in ("THIN_PRISM_FISHEYE", "FISHEYE"):
        cams[3] = (4, name, 640, 480, [1.0] * 12)
        write_text(tmp_path / name, cams, images, points)
        for reader in READERS:
            with pytest.raises(ValueError, match=f"camera model {name} unknown!"):
                reader.read_colmap(str(tmp_path / name))
        rc, msg, _ = c_read(tmp_path / name)
        assert rc == -1 and msg == f"camera model {name} unknown!"


def _refused(folder, file_name):
    for reader in READERS:
        with pytest.raises(ValueError, match=file_name.replace(".", r"\.")):
            reader.read_colmap(str(folder))
    rc, msg, _ = c_read(folder)
    assert rc == L.L3D_ERR_IO and file_name in msg, (rc, msg)


@pytest.mark.parametrize("file_name", ["cameras.bin", "images.bin", "points3D.bin"])
def test_truncated_and_overlong_files_are_refused_by_name(tmp_path, file_name):
    cams, images, points = scene(np.random.default_rng(11))
    files = binary_files(cams, images, points)
    data = files[file_name]
    n = 0
    # inside the count, inside the first record, in the middle, one byte short; one byte and one record too many
    for cut in (3, 8 + 5, len(data) // 2, len(data) - 1):
        folder = tmp_path / f"cut{n}"; n += 1
        write_binary(folder, dict(files, **{file_name: data[:cut]}))
        _refused(folder, file_name)
    for extra in (b"\0", data[8:60]):
        folder = tmp_path / f"long{n}"; n += 1
        write_binary(folder, dict(files, **{file_name: data + extra}))
        _refused(folder, file_name)
    # a count that exceeds the file: refused from the sizes alone, before anything is allocated
    for count in (len(data), 2 ** 40, 2 ** 64 - 1):
        folder = tmp_path / f"count{n}"; n += 1
        write_binary(folder, dict(files, **{file_name: struct.pack("<Q", count) + data[8:]}))
        _refused(folder, file_name)
    write_binary(tmp_path / "whole", files)
    assert all(len(reader.read_colmap(str(tmp_path / "whole"))) == 12 for reader in READERS) and c_read(tmp_path / "whole")[0] == 0


def test_inner_counts_that_exceed_the_file_are_refused(tmp_path):
    cams, images, points = scene(np.random.default_rng(12))
    files = binary_files(cams[:1], [(1, [1, 0, 0, 0], [0, 0, 0], 1, "a", [(1.0, 2.0, 5)])], [(5, np.ones(3))])
    i = files["images.bin"]
    at = i.index(b"a\0") + 2                                       # the number of 2D points
    write_binary(tmp_path / "m", dict(files, **{"images.bin": i[:at] + struct.pack("<Q", 2 ** 61) + i[at + 8:]}))
    _refused(tmp_path / "m", "images.bin")
    write_binary(tmp_path / "name", dict(files, **{"images.bin": i[:at - 1]}))      # the name's end is missing
    _refused(tmp_path / "name", "images.bin")
    p = files["points3D.bin"]
    write_binary(tmp_path / "t", dict(files, **{"points3D.bin": p[:-8] + struct.pack("<Q", 2 ** 62)}))
    _refused(tmp_path / "t", "points3D.bin")
    c = files["cameras.bin"]
    write_binary(tmp_path / "w", dict(files, **{"cameras.bin": c[:16] + struct.pack("<Q", 2 ** 32) + c[24:]}))
    _refused(tmp_path / "w", "cameras.bin")
    write_binary(tmp_path / "ok", files)
    for reader in READERS:
        got = reader.read_colmap(str(tmp_path / "ok"))
        assert len(got) == 1 and got[0]["worldpoints"] == [5] and got[0]["median_depth"] == np.float32(np.sqrt(3.0))


def test_point_ids_follow_the_text_readers_atoi(tmp_path):
    """a POINT3D_ID is handled as l3d_sfm_open_colmap's text reader handles the same number in decimal"""
    cams, _, _ = scene(np.random.default_rng(13))
    ids = [5, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 7, 2 ** 63 - 1, 2 ** 63, NO_POINT]
    images = [(1, [1, 0, 0, 0], [0, 0, 0], 1, "a", [(1.0, 2.0, p) for p in ids])]
    points = [(5, np.ones(3)), (7, 2 * np.ones(3)), (2 ** 32 + 7, 3 * np.ones(3))]
    write_binary(tmp_path / "bin", binary_files(cams[:1], images, points))
    os.makedirs(tmp_path / "txt")
    with open(tmp_path / "txt" / "cameras.txt", "w") as f:
        f.write(f"1 SIMPLE_PINHOLE 1920 1080 {_g(cams[0][4][0])} {_g(cams[0][4][1])} {_g(cams[0][4][2])}\n")
    with open(tmp_path / "txt" / "images.txt", "w") as f:
        f.write("1 1 0 0 0 0 0 0 1 a\n" + " ".join(f"1 2 {p}" for p in ids) + "\n")
    with open(tmp_path / "txt" / "points3D.txt", "w") as f:
        f.write("5 1 1 1 0 0 0 0\n7 2 2 2 0 0 0 0\n4294967303 3 3 3 0 0 0 0\n")
    want = [5, 2 ** 31 - 1, 7]                                      # atoi: 2^31 -> negative, 2^32 + 7 -> 7, the rest -> -1
    rc, _, ctxt = c_read(tmp_path / "txt")
    rc2, _, cbin = c_read(tmp_path / "bin")
    assert rc == 0 and rc2 == 0 and ctxt[0]["worldpoints"] == cbin[0]["worldpoints"] == want
    _same_c(ctxt, cbin)
    for reader in READERS:
        got = reader.read_colmap(str(tmp_path / "bin"))
        assert got[0]["worldpoints"] == want and float(got[0]["median_depth"]) == float(cbin[0]["median_depth"])
