"""The three programs of line3dpp_amd/front_end.py against the reference's own main_vsfm.cpp, main_colmap.cpp and
main_bundler.cpp (oracle/_ref/libl3d_ref_front.so: compiled in place against a recorder of the Line3D interface, see
tests/test_front_ends_pinned.py).  Both sides get the SAME argv on the same files.  Ours runs with a recording stand-in
for Line3D that writes events of the recorder's shape, and with an image reader that, like the recorder's cv::imread,
gives a 480 x 640 zero image for a file that exists and nothing otherwise.

The reference undistorts and adds image by image, ours per chunk, so the two event lists are compared per kind of call:
the undistortImage events form the same sequence on both sides, and so do the addImage events; the constructor call and
everything from matchImages on are the same calls in the same order.  Integers and strings are equal; K, R, t, radial
and tangential are equal as doubles; median_depth is equal as float32; the float flags are equal to the float32 the
reference holds (which the recorder prints as a double, exactly)."""
import json
import os

import numpy as np
import pytest

from tests.test_front_ends_pinned import _calls, _front, _run, _touch
from tests.test_input_formats import _colmap_scene, _write_bundler, _write_colmap, _write_nvm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = ["matchImages", "reconstruct3Dlines", "get3Dlines", "saveResultAsSTL", "saveResultAsOBJ", "save3DLinesAsTXT",
        "save3DLinesAsBIN"]


class Recorder:
    """stands in for line3dpp_amd.api.Line3D: every call becomes an event of the shape oracle/ref_shim_front/line3D.h writes"""

    def __init__(self):
        self.events = []
        self.constructed = 0

    def __call__(self, output_folder, load_segments, max_img_width, max_line_segments, neighbors_by_worldpoints, use_GPU):
        self.constructed += 1
        self.events.append(dict(call="Line3D", output_folder=output_folder, load_segments=int(load_segments),
                                max_img_width=max_img_width, max_line_segments=max_line_segments,
                                neighbors_by_worldpoints=int(neighbors_by_worldpoints), use_GPU=int(use_GPU)))
        return self

    def addImages(self, camIDs, images, Ks, Rs, ts, median_depths, wps_or_neighbors):
        for cam, im, K, R, t, md, wps in zip(camIDs, images, Ks, Rs, ts, median_depths, wps_or_neighbors):
            self.events.append(dict(call="addImage", camID=cam, cols=im.shape[1], rows=im.shape[0],
                                    K=np.asarray(K, np.float64).reshape(9).tolist(), R=np.asarray(R, np.float64).reshape(9).tolist(),
                                    t=np.asarray(t, np.float64).tolist(), median_depth=md, wps=list(wps), n_segments=0))

    def undistort(self, images, Ks, radials, tangentials):
        for K, r, t in zip(Ks, radials, tangentials):
            self.events.append(dict(call="undistortImage", radial=np.asarray(r, np.float64).tolist(),
                                    tangential=np.asarray(t, np.float64).tolist(), K=np.asarray(K, np.float64).reshape(9).tolist()))
        return list(images)

    def matchImages(self, sigma_position, sigma_angle, num_neighbors, epipolar_overlap, kNN, const_regularization_depth):
        self.events.append(dict(call="matchImages", sigma_position=sigma_position, sigma_angle=sigma_angle, num_neighbors=num_neighbors,
                                epipolar_overlap=epipolar_overlap, kNN=kNN, const_regularization_depth=const_regularization_depth))
        return True

    def reconstruct3Dlines(self, visibility_t, perform_diffusion, collinearity_t, use_CERES, max_iter_CERES=250):
        self.events.append(dict(call="reconstruct3Dlines", visibility_t=visibility_t, perform_diffusion=int(perform_diffusion),
                                collinearity_t=collinearity_t, use_CERES=int(use_CERES), max_iter_CERES=max_iter_CERES))
        return True

    def get3Dlines(self):
        self.events.append(dict(call="get3Dlines"))
        return []

    def _save(self, name, folder, max_image_width):
        # the library's writers take max_image_width for the file name; the reference's read it from the object
        assert max_image_width == self.events[0]["max_img_width"]
        self.events.append(dict(call=name, folder=folder))
        return True

    def saveResultAsSTL(self, folder, max_image_width=-1): return self._save("saveResultAsSTL", folder, max_image_width)
    def saveResultAsOBJ(self, folder, max_image_width=-1): return self._save("saveResultAsOBJ", folder, max_image_width)
    def save3DLinesAsTXT(self, folder, max_image_width=-1): return self._save("save3DLinesAsTXT", folder, max_image_width)
    def save3DLinesAsBIN(self, folder, max_image_width=-1): return self._save("save3DLinesAsBIN", folder, max_image_width)


def _read_image(path):
    return np.zeros((480, 640), np.uint8) if os.path.exists(path) else None


def _ours(which, args, chunk_bytes=None, monkeypatch=None):
    from line3dpp_amd import front_end
    rec = Recorder()
    if chunk_bytes is not None:
        monkeypatch.setenv(front_end.CHUNK_ENV, str(chunk_bytes))
    rc = front_end.main([which] + list(args), line3d_factory=rec, read_image=_read_image, undistort=rec.undistort)
    return rc, rec


def _same_call(a, b, floats=(), mats=()):
    assert a["call"] == b["call"] and set(a) == set(b), (a, b)
    for key in a:
        if key in mats:
            assert np.array_equal(np.array(a[key], np.float64), np.array(b[key], np.float64)), (a["call"], key, a[key], b[key])
        elif key == "median_depth":
            assert np.float32(a[key]) == np.float32(b[key]), (a["call"], key, a[key], b[key])
        elif key in floats:            # the reference holds a float32 and the recorder prints it exactly
            assert isinstance(a[key], float) and a[key] == float(np.float32(b[key])) == b[key], (a["call"], key, a[key], b[key])
        else:                          # integers and strings
            assert type(a[key]) is type(b[key]) and a[key] == b[key], (a["call"], key, a[key], b[key])


def _compare(which, args, expect=None, **kw):
    """runs both front ends on args; -> the reference's events, after holding ours against them"""
    rc_ref, ref = _run(_front(), which, args)
    rc, rec = _ours(which, args, **kw)
    ours = rec.events
    assert rc_ref == 0 and rc == 0 and rec.constructed == 1
    _same_call(ours[0], ref[0])
    for name, mats in (("undistortImage", ("radial", "tangential", "K")), ("addImage", ("K", "R", "t"))):
        a, b = _calls(ours, name), _calls(ref, name)
        assert len(a) == len(b), (name, len(a), len(b))
        for x, y in zip(a, b):
            _same_call(x, y, mats=mats)
    for events in (ours, ref):
        names = [e["call"] for e in events]
        k = names.index("matchImages")
        assert names[0] == "Line3D" and set(names[1:k]) <= {"undistortImage", "addImage"} and names[k:] == TAIL
    for x, y in zip(ours[-len(TAIL):], ref[-len(TAIL):]):
        _same_call(x, y, floats=("sigma_position", "sigma_angle", "epipolar_overlap", "const_regularization_depth", "collinearity_t"))
    if expect is not None:
        assert (len(_calls(ref, "undistortImage")), len(_calls(ref, "addImage"))) == expect
    return ref


DEFAULTS = ["-c", "0"]
# every numeric and boolean flag off its default; -n, -e, -a are changed by the normalisation, -p < 0 goes with -z
ALL = ["-w", "1200", "-n", "1", "-a", "-10", "-p", "-0.5", "-e", "-1.5", "-k", "3", "-y", "500", "-v", "4", "-d", "1",
       "-l", "0", "-r", "2.5", "-g", "0", "-c", "1", "-z", "12"]
LONG = ["--max_image_width", "1000", "--num_matching_neighbors", "7", "--sigma_a", "7.3", "--sigma_p", "1.1",
        "--min_epipolar_overlap", "0.4", "--knn_matches", "-1", "--num_segments_per_image", "1234", "--visibility_t", "5",
        "--diffusion", "1", "--load_and_store_flag", "1", "--collinearity_t", "0.7", "--use_cuda", "1", "--use_ceres", "1",
        "--const_reg_depth", "-1"]
FLAG_SETS = {"defaults": DEFAULTS, "all": ALL, "long": LONG}


def _check_values(ref, flags):
    """the reference's own normalisation, so that the comparison above is known to have compared the changed values"""
    if flags is not ALL:
        return
    m, r = _calls(ref, "matchImages")[0], _calls(ref, "reconstruct3Dlines")[0]
    assert (m["num_neighbors"], m["sigma_angle"], m["sigma_position"], m["kNN"], m["const_regularization_depth"]) == (2, 10.0, -0.5, 3, 12.0)
    assert m["epipolar_overlap"] == float(np.float32(0.99))
    assert (r["visibility_t"], r["perform_diffusion"], r["collinearity_t"], r["use_CERES"]) == (4, 1, 2.5, 1)
    assert (ref[0]["load_segments"], ref[0]["max_img_width"], ref[0]["max_line_segments"], ref[0]["use_GPU"]) == (0, 1200, 500, 0)


# ---- VisualSfM -------------------------------------------------------------------------------------------------------
def _nvm_scene(tmp_path, seed=3):
    rng = np.random.default_rng(seed)
    cams = []
    for i in range(6):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        cams.append(dict(filename=f"some/where/img_{i}.jpg", focal=2400.0 + 1.25 * i, q=q, C=rng.normal(size=3) * 5,
                         distortion=0.0 if i == 1 else 0.01 * (i + 1)))
    points = []
    for k in range(60):
        seen = sorted(rng.choice(5, size=rng.integers(2, 4), replace=False).tolist())      # camera 5 sees nothing
        points.append((rng.normal(size=3) * 3, [(c, k, 100.0 + k, 50.0) for c in seen]))
    path = tmp_path / "model" / "vsfm_result.nvm"
    path.parent.mkdir()
    _write_nvm(path, cams, points)
    return path


@pytest.mark.parametrize("flags", list(FLAG_SETS))
@pytest.mark.parametrize("with_o", [True, False])
def test_vsfm_with_image_folder(tmp_path, flags, with_o):
    path = _nvm_scene(tmp_path)
    _touch(tmp_path / "imgs", [f"img_{i}.jpg" for i in (0, 1, 2, 4, 5)])          # img_3.jpg is missing: an empty image
    args = ["-i", str(tmp_path / "imgs"), "-m", str(path)] + (["-o", str(tmp_path / "out")] if with_o else []) + FLAG_SETS[flags]
    ref = _compare("vsfm", args, expect=(4, 5))                                     # camera 1: no distortion, camera 5: no points
    assert ref[0]["output_folder"] == (str(tmp_path / "out") if with_o else str(tmp_path / "imgs") + "/Line3D++/")
    assert os.path.isdir(ref[0]["output_folder"])
    assert [(a["camID"], a["cols"], a["rows"]) for a in _calls(ref, "addImage")] == [(0, 640, 480), (1, 640, 480), (2, 640, 480), (3, 0, 0), (4, 640, 480)]
    _check_values(ref, FLAG_SETS[flags])


@pytest.mark.parametrize("with_o", [True, False])
def test_vsfm_with_the_paths_of_the_nvm_file(tmp_path, with_o):
    path = _nvm_scene(tmp_path, seed=5)
    _touch(path.parent, [f"some/where/img_{i}.jpg" for i in (0, 1, 3, 4)])
    _touch(path.parent, ["img_2.jpg"])                                              # not where the .nvm says: not found
    args = ["--nvm_file", str(path)] + (["--output_folder", str(tmp_path / "out")] if with_o else []) + DEFAULTS
    ref = _compare("vsfm", args, expect=(4, 5))
    assert ref[0]["output_folder"] == (str(tmp_path / "out") if with_o else str(path.parent) + "/Line3D++/")
    assert [a["cols"] for a in _calls(ref, "addImage")] == [640, 640, 0, 640, 640]


# ---- COLMAP ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", list(FLAG_SETS))
@pytest.mark.parametrize("with_m,with_o", [(True, True), (True, False), (False, True), (False, False)])
def test_colmap(tmp_path, flags, with_m, with_o):
    cams, images, points = _colmap_scene(np.random.default_rng(4))                   # one camera of each model, one unknown
    imgs = tmp_path / "imgs"
    sfm = tmp_path / "sfm" if with_m else imgs
    imgs.mkdir()
    _write_colmap(sfm, cams, images, points)
    _touch(imgs, [im[4] for k, im in enumerate(images) if k != 1])                   # the second image is missing
    args = ["-i", str(imgs)] + (["-m", str(sfm)] if with_m else []) + (["-o", str(tmp_path / "out")] if with_o else []) + FLAG_SETS[flags]
    # 6 images of known cameras: 4 with distortion (also the one without worldpoints), 5 with worldpoints
    ref = _compare("colmap", args, expect=(4, 5))
    assert ref[0]["output_folder"] == (str(tmp_path / "out") if with_o else str(sfm) + "/Line3D++/")
    assert [a["camID"] for a in _calls(ref, "addImage")] == [10, 15, 20, 25, 35]
    assert [a["cols"] for a in _calls(ref, "addImage")] == [640, 0, 640, 640, 640]
    _check_values(ref, FLAG_SETS[flags])


# ---- bundler ---------------------------------------------------------------------------------------------------------
def _bundler_scene(tmp_path, seed=6):
    from line3dpp_amd import io
    rng = np.random.default_rng(seed)
    cams = []
    for i in range(6):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        cams.append(dict(f=900.0 + 11.5 * i, k1=0.0 if i == 2 else -0.01 * (i + 1), k2=0.0 if i == 2 else 0.002 * i,
                         R=io.rotation_from_q(*q), t=rng.normal(size=3) * 3))
    points = []
    for k in range(120):
        seen = sorted(rng.choice(5, size=rng.integers(2, 4), replace=False).tolist())        # camera 5 sees nothing
        points.append((rng.normal(size=3) * 5, [(c, 7 * k, 10.0 + k, -3.5) for c in seen]))
    imgs = tmp_path / "data" / "imgs"
    imgs.mkdir(parents=True)
    _write_bundler(tmp_path / "data" / "bundle.rd.out", cams, points)                        # where -b is not needed
    _write_bundler(tmp_path / "elsewhere.out", cams, points)
    return imgs


@pytest.mark.parametrize("flags", list(FLAG_SETS))
@pytest.mark.parametrize("with_b,with_o", [(True, True), (False, False)])
def test_bundler_with_the_extension_probe(tmp_path, flags, with_b, with_o):
    imgs = _bundler_scene(tmp_path)
    # camera 0 has two files: the probe takes .JPG before .png; camera 3 has none: skipped; camera 4 a .bmp
    _touch(imgs, ["00000000.JPG", "00000000.png", "00000001.jpeg", "00000002.PNG", "00000004.bmp", "00000005.jpg"])
    args = (["-i", str(imgs)] + (["-b", str(tmp_path / "elsewhere.out")] if with_b else [])
            + (["-o", str(tmp_path / "out")] if with_o else []) + FLAG_SETS[flags])
    ref = _compare("bundler", args, expect=(3, 4))
    assert ref[0]["output_folder"] == (str(tmp_path / "out") if with_o else str(imgs) + "/Line3D++/")
    assert [a["camID"] for a in _calls(ref, "addImage")] == [0, 1, 2, 4]
    _check_values(ref, FLAG_SETS[flags])


def test_bundler_probe_reads_the_file_the_reference_reads(tmp_path):
    """00000000.JPG and 00000000.png both exist: which of them is read shows only in the reader's argument"""
    from line3dpp_amd import front_end
    imgs = _bundler_scene(tmp_path)
    _touch(imgs, ["00000000.JPG", "00000000.png", "00000001.BMP"])
    seen = []

    def read(path):
        seen.append(path)
        return _read_image(path)
    rec = Recorder()
    assert front_end.main(["bundler", "-i", str(imgs), "-c", "0"], line3d_factory=rec, read_image=read, undistort=rec.undistort) == 0
    assert seen == [str(imgs) + "/00000000.JPG", str(imgs) + "/00000001.BMP"]          # main_bundler.cpp:301-308: .jpg .JPG .png ...


@pytest.mark.parametrize("ext", ["png", ".png"])
def test_bundler_with_an_extension(tmp_path, ext):
    imgs = _bundler_scene(tmp_path)
    _touch(imgs, ["00000000.png", "00000001.jpg", "00000002.png", "00000003.PNG", "00000004.png"])   # only .png counts
    ref = _compare("bundler", ["-i", str(imgs), "-t", ext, "-o", str(tmp_path / "out")] + DEFAULTS, expect=(2, 3))
    assert [a["camID"] for a in _calls(ref, "addImage")] == [0, 2, 4]


def test_bundler_with_an_image_list(tmp_path):
    imgs = _bundler_scene(tmp_path)
    # line index = camera id; first token = file; an empty line leaves camera 1 to the probe; camera 3's file is missing
    (tmp_path / "list.txt").write_text("a/first.jpg 0 1234.5\n\nthird.png\nnot_there.jpg\n  fifth.bmp  \nsixth.jpg\n")
    _touch(imgs, ["a/first.jpg", "00000001.png", "third.png", "fifth.bmp", "sixth.jpg", "00000000.jpg"])
    ref = _compare("bundler", ["-i", str(imgs), "-f", str(tmp_path / "list.txt"), "--image_extension", "png"] + ALL, expect=(4, 5))
    assert [(a["camID"], a["cols"]) for a in _calls(ref, "addImage")] == [(0, 640), (1, 640), (2, 640), (3, 0), (4, 640)]


# ---- the chunking leaves the calls alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_bytes", [1, 2 * 480 * 640, 5 * 480 * 640])
def test_chunking_does_not_change_the_calls(tmp_path, monkeypatch, chunk_bytes):
    cams, images, points = _colmap_scene(np.random.default_rng(8), n_img=13)
    _write_colmap(tmp_path / "sfm", cams, images, points)
    _touch(tmp_path / "imgs", [im[4] for im in images])
    args = ["-i", str(tmp_path / "imgs"), "-m", str(tmp_path / "sfm"), "-o", str(tmp_path / "out")] + DEFAULTS
    _compare("colmap", args, chunk_bytes=chunk_bytes, monkeypatch=monkeypatch)
    _, rec = _ours("colmap", args, chunk_bytes=chunk_bytes, monkeypatch=monkeypatch)
    # an addImage of a chunk comes after the undistortImage calls of that chunk, and chunks hold what the budget allows
    names = [e["call"] for e in rec.events if e["call"] in ("undistortImage", "addImage")]
    runs = sum(1 for a, b in zip(names, names[1:]) if a == "addImage" and b == "undistortImage") + 1
    assert runs >= {1: 5, 2 * 480 * 640: 4, 5 * 480 * 640: 2}[chunk_bytes]


# ---- errors --------------------------------------------------------------------------------------------------------------
def _both_fail(which, args, capsys, message=None):
    rc_ref, _ = _run(_front(), which, args)
    rc, rec = _ours(which, args)
    assert rc_ref != 0 and rc != 0 and rec.constructed == 0 and not rec.events
    if message is not None:
        assert message in capsys.readouterr().err


def test_wrong_command_lines_end_both(tmp_path, capsys):
    path = _nvm_scene(tmp_path)
    imgs = _bundler_scene(tmp_path)
    _both_fail("vsfm", ["-i", str(tmp_path)] + DEFAULTS, capsys, "required argument missing")           # -m is required
    _both_fail("colmap", ["-m", str(tmp_path)] + DEFAULTS, capsys, "required argument missing")         # -i is required
    _both_fail("bundler", ["-b", str(tmp_path / "elsewhere.out")] + DEFAULTS, capsys, "required argument missing")
    _both_fail("vsfm", ["-m", str(path), "-q", "1"], capsys, "unknown argument -q")
    _both_fail("colmap", ["-i", str(tmp_path), "--sfm", str(tmp_path)], capsys, "unknown argument --sfm")   # no abbreviations
    _both_fail("bundler", ["-i", str(imgs), "-m", "x"], capsys, "unknown argument -m")                  # another program's flag


def test_errors_the_reference_ends_on(tmp_path, capsys):
    _both_fail("vsfm", ["-m", str(tmp_path / "none.nvm")], capsys, "does not exist!")
    empty = tmp_path / "empty.nvm"
    _write_nvm(empty, [], [])
    _both_fail("vsfm", ["-m", str(empty), "-o", str(tmp_path / "o")], capsys, "No aligned cameras in NVM file!")
    _both_fail("bundler", ["-i", str(tmp_path), "-b", str(tmp_path / "none.out")], capsys, "does not exist!")
    _both_fail("bundler", ["-i", str(tmp_path / "imgs")], capsys, "does not exist!")                    # the default bundle file
    _write_bundler(tmp_path / "empty.out", [], [])
    _both_fail("bundler", ["-i", str(tmp_path), "-b", str(tmp_path / "empty.out"), "-o", str(tmp_path / "o")], capsys,
               "No cameras and/or points in bundle file!")
    _both_fail("colmap", ["-i", str(tmp_path), "-m", str(tmp_path / "missing")], capsys, "does not exist!")
    cams, images, points = _colmap_scene(np.random.default_rng(4))
    _write_colmap(tmp_path / "part", cams, images, points)
    os.remove(tmp_path / "part" / "points3D.txt")
    _both_fail("colmap", ["-i", str(tmp_path), "-m", str(tmp_path / "part"), "-o", str(tmp_path / "o")], capsys,
               "at least one of the colmap result files does not exist")
    _write_colmap(tmp_path / "bad", [(1, "THIN_PRISM_FISHEYE", 100, 100, [1.0] * 12)], [], [])
    _both_fail("colmap", ["-i", str(tmp_path), "-m", str(tmp_path / "bad"), "-o", str(tmp_path / "o")], capsys,
               "camera model THIN_PRISM_FISHEYE unknown!")


# ---- the flag tables --------------------------------------------------------------------------------------------------------
def test_flag_tables_are_the_reference_mains(capsys):
    """tests/golden/front_end_flags.json: written by hand from the TCLAP::ValueArg lines of the three mains"""
    from line3dpp_amd import front_end
    with open(os.path.join(ROOT, "tests", "golden", "front_end_flags.json")) as f:
        want = json.load(f)
    kinds = {str: "string", int: "int", float: "float", bool: "bool"}
    for program in ("vsfm", "colmap", "bundler"):
        got = [dict(short=s, long=n, type=kinds[t], required=r, default=d) for s, n, t, r, d, _ in front_end.FLAGS[program]]
        assert got == want[program], program
        for g, w in zip(got, want[program]):
            assert type(g["default"]) is type(w["default"]), (program, g["long"])
        # the parser holds the defaults the table names, floats as the float32 TCLAP::ValueArg<float> holds
        required = [x for s, n, t, r, d, _ in front_end.FLAGS[program] if r for x in ("-" + s, "here")]
        values = front_end.parse_args(program, required)
        for s, n, t, r, d, _ in front_end.FLAGS[program]:
            if not r:
                assert values[n] == (np.float32(d) if t is float else d) and (t is not float or type(values[n]) is np.float32)
        # the two flags that cannot mean here what they mean there say so
        text = front_end.usage(program)
        assert "no CPU path" in text and "without Ceres" in text
    assert front_end.main(["vsfm", "-m", "x.nvm", "-d", "yes"]) != 0 and "0 or 1" in capsys.readouterr().err   # booleans are 0 / 1
