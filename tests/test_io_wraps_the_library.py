"""line3dpp_amd/io.py reads .nvm files, COLMAP results, bundler files and the segment cache through the library
(l3d_nvm_*, l3d_sfm_*, l3d_*_segment_cache); what is its own is the marshalling: every record of the library as a dict of
numpy arrays and Python values, every error of the library as a ValueError with the library's text.  Each dict is held
against the Python model of the formats (tests/sfm_readers_model.py), key by key and type by type, on small files with the
corners the writers of tests/test_input_formats.py and tests/test_colmap_binary.py know.  Bit-equal except for the two
values the model sums in numpy's order: C within 1e-12 absolute, median_depth within 2e-7 relative.
No GPU."""
import numpy as np
import pytest

from line3dpp_amd import _lib, io
from tests import sfm_readers_model as M
from tests.test_colmap_binary import binary_files, scene, write_binary, write_text
from tests.test_input_formats import _colmap_scene, _write_bundler, _write_colmap, _write_nvm


def _same_value(g, w, key):
    if isinstance(w, np.ndarray):
        assert type(g) is np.ndarray and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), key
    elif isinstance(w, list):
        assert type(g) is list and g == w and [type(x) for x in g] == [type(x) for x in w], key
    else:
        assert type(g) is type(w) and g == w, key


def _same(got, want):
    """every key of every dict of the wrapper against the model's"""
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for key in w:
            if key == "C":
                assert g[key].dtype == np.float64 and g[key].shape == (3,) and np.abs(g[key] - w[key]).max() <= 1e-12
            elif key == "median_depth" and w[key] is not None:
                assert type(g[key]) is type(w[key]) is np.float32
                assert abs(float(g[key]) - float(w[key])) <= 2e-7 * float(w[key])
            else:
                _same_value(g[key], w[key], key)


def _refused(read, path, text):
    """ValueError whose text is the library's and holds `text`"""
    with pytest.raises(ValueError) as e:
        read(path)
    assert text in str(e.value) and str(e.value) == _lib.last_error()
    return str(e.value)


def test_nvm(tmp_path):
    rng = np.random.default_rng(21)
    cams = []
    for i in range(4):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        cams.append(dict(filename=f"dir/img_{i}.jpg", focal=1800.0 + 37.25 * i, q=q, C=rng.normal(size=3) * 5, distortion=0.0125 * i))
    points = []
    for k in range(40):
        seen = sorted(rng.choice(3, size=rng.integers(1, 4), replace=False).tolist())      # camera 3 sees nothing
        points.append((rng.normal(size=3) * 3, [(c, k, 100.0 + k, 50.0) for c in seen]))
    path = tmp_path / "model.nvm"
    _write_nvm(path, cams, points)
    want = M.read_nvm(path)
    assert want[3]["median_depth"] is None and want[3]["worldpoints"] == [] and all(w["worldpoints"] for w in want[:3])
    _same(io.read_nvm(path), want)
    _same(io.read_nvm(str(path)), want)
    for focal, width, height in ((want[1]["focal"], 3073, 2305), (1234.56789, 640, 480)):
        _same_value(io.nvm_intrinsics(focal, width, height), M.nvm_intrinsics(focal, width, height), "K")
    empty = tmp_path / "empty.nvm"
    empty.write_text("NVM_V3\n\n0\n\n0\n")
    _refused(io.read_nvm, empty, "No aligned cameras")


def test_colmap_text(tmp_path):
    """an image of an unknown camera, an image with no worldpoint among its 2D points, a non-normalised quaternion
    (_colmap_scene), an image line without 2D points and a repeated IMAGE_ID"""
    rng = np.random.default_rng(22)
    cams, images, points = _colmap_scene(rng, n_img=8)
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    images.append((90, q, rng.normal(size=3) * 6, 3, "bare.jpg", []))
    images.append((images[0][0], q, rng.normal(size=3) * 6, 2, "again.jpg", [(7.0, 8.0, points[3][0]), (9.0, 10.0, points[5][0])]))
    _write_colmap(tmp_path / "sfm", cams, images, points)
    want = M.read_colmap(str(tmp_path / "sfm"))
    assert len(want) == len(images) - 1                                            # (the image of camera 9)
    assert [w["name"] for w in want].count("again.jpg") == 2
    assert [w["median_depth"] is None for w in want].count(True) == 2 and want[-2]["worldpoints"] == []
    _same(io.read_colmap(str(tmp_path / "sfm")), want)
    _same(io.read_colmap(tmp_path / "sfm"), want)
    _write_colmap(tmp_path / "bad", [(1, "THIN_PRISM_FISHEYE", 100, 100, [1.0] * 12)], [], [])
    assert _refused(io.read_colmap, tmp_path / "bad", "unknown!") == "camera model THIN_PRISM_FISHEYE unknown!"
    _refused(io.read_colmap, tmp_path / "nowhere", "does not exist")


def test_colmap_binary_and_all_ten_models(tmp_path):
    cams, images, points = scene(np.random.default_rng(23))
    files = binary_files(cams, images, points)
    write_binary(tmp_path / "bin", files)
    write_text(tmp_path / "txt", cams, images, points)
    want = M.read_colmap(str(tmp_path / "bin"))
    assert io.COLMAP_MODEL_IDS == M.COLMAP_MODEL_IDS
    lengths = dict(M.COLMAP_MODEL_IDS)
    assert {w["model"] for w in want} == {c[1] for c in cams} and len(cams) == 10
    got = io.read_colmap(str(tmp_path / "bin"))
    _same(got, want)
    assert all(len(g["params"]) == lengths[g["model"]] for g in got)
    _same(io.read_colmap(str(tmp_path / "txt")), want)
    cams[3] = (4, 11, 640, 480, [1.0] * 12)
    write_binary(tmp_path / "bad", binary_files(cams, images, points))
    assert _refused(io.read_colmap, tmp_path / "bad", "unknown!") == "camera model 11 unknown!"
    data = files["images.bin"]
    write_binary(tmp_path / "cut", dict(files, **{"images.bin": data[:len(data) // 2]}))
    _refused(io.read_colmap, tmp_path / "cut", "images.bin")


def test_bundler(tmp_path):
    rng = np.random.default_rng(24)
    cams = []
    for i in range(4):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        cams.append(dict(f=900.0 + 11.5 * i, k1=-0.01 * i, k2=0.002 * i, R=M.rotation_from_q(*q), t=rng.normal(size=3) * 3))
        _same_value(io.rotation_from_q(*q), cams[-1]["R"], "R")
        _same_value(io.rotation_from_q(*(3.5 * q)), M.rotation_from_q(*(3.5 * q)), "R")         # not normalised
    points = []
    for k in range(40):
        seen = sorted(rng.choice(3, size=rng.integers(1, 4), replace=False).tolist())      # camera 3 sees nothing
        points.append((rng.normal(size=3) * 5, [(c, 7 * k, 10.0 + k, -3.5) for c in seen]))
    path = tmp_path / "bundle.rd.out"
    _write_bundler(path, cams, points)
    want = M.read_bundler(str(path))
    assert want[3]["median_depth"] is None and all(w["worldpoints"] for w in want[:3])
    _same(io.read_bundler(str(path)), want)
    _same(io.read_bundler(path), want)
    empty = tmp_path / "empty.out"
    empty.write_text("# Bundle file v0.3\n0 0\n")
    _refused(io.read_bundler, empty, "No cameras and/or points")


@pytest.mark.parametrize("n", [0, 1, 2, 7])
def test_segment_cache(tmp_path, n):
    segs = np.random.default_rng(30 + n).uniform(0, 3000, (n, 4)).astype(np.float32)
    name = io.segment_cache_name(5, 3072, 2304)
    _same_value(name, M.segment_cache_name(5, 3072, 2304), "name")
    _same_value(io.segment_cache_name(2 ** 32 - 1, 1, 2, 17), M.segment_cache_name(2 ** 32 - 1, 1, 2, 17), "name")
    path = tmp_path / name
    path.write_bytes(M.format_segment_cache(segs))
    _same_value(io.format_segment_cache(segs), M.format_segment_cache(segs), "bytes")
    _same_value(io.read_segment_cache(path), segs, "segments")
    _same_value(io.read_segment_cache(str(path)), M.read_segment_cache(path), "segments")


def test_a_junk_segment_cache_is_refused(tmp_path):
    path = tmp_path / "x.bin"
    path.write_bytes(b"not an archive at all, but long enough to be read as one........")
    _refused(io.read_segment_cache, path, "not a boost binary archive")
    _refused(io.read_segment_cache, tmp_path / "missing.bin", "cannot open")


def test_malformed_text_is_read_as_the_stream_parsers_read_it(tmp_path):
    """a token of images.txt that does not parse stops the stream of its line; the image stays, with what was
    read before it, where the camera id of the line before it is known.  A bundle file that ends inside its cameras
    gives as many cameras as its header states."""
    good, pts = "7 0.5 0.5 0.5 0.5 1 2 3 1 a.jpg", "1 1 5 2 2 6"

    def colmap(name, lines):
        folder = tmp_path / name
        folder.mkdir()
        (folder / "cameras.txt").write_text("1 PINHOLE 640 480 500 500 320 240\n")
        (folder / "images.txt").write_text("".join(line + "\n" for line in lines))
        (folder / "points3D.txt").write_text("5 1 2 3 0 0 0 0\n6 2 3 4 0 0 0 0\n")
        return io.read_colmap(folder)

    for name, bad, bad_id in (("id", "abc 1 0 0 0 1 2 3 1 b.jpg", 0), ("q", "8 1 x 0 0 1 2 3 1 b.jpg", 8)):
        first, second = colmap(name + "_behind", [good, pts, bad, pts])
        assert (first["id"], first["name"]) == (7, "a.jpg")
        assert (second["id"], second["camera"], second["name"], second["worldpoints"]) == (bad_id, 1, "", [5, 6])
        assert np.array_equal(second["R"], np.eye(3)) and not second["t"].any()
        assert [g["id"] for g in colmap(name + "_first", [bad, pts, good, pts])] == [7]
    assert [g["id"] for g in colmap("camera", [good, pts, "8 1 0 0 0 1 2 3 zz b.jpg", pts])] == [7]
    assert colmap("point", [good, "1 1 abc 2 2 6"])[0]["worldpoints"] == [0, 6]

    path = tmp_path / "bundle.out"
    path.write_text("# Bundle file v0.3\n3 1\n900 0.1 0.2\n1 0 0\n0 1 0\n0 0 1\n1 2 3\n800 0.1 0.2\n1 0 0\n")
    cams = io.read_bundler(path)
    assert [float(c["focal"]) for c in cams] == [900.0, 800.0, 0.0]
    assert np.array_equal(cams[0]["t"], [1.0, -2.0, -3.0]) and np.array_equal(cams[1]["R"][0], [1.0, 0.0, 0.0])
    assert not cams[1]["R"][1:].any() and not cams[2]["R"].any() and not cams[2]["t"].any()
    assert all(c["worldpoints"] == [] and c["median_depth"] is None for c in cams)
