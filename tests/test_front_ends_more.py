"""The Pix4D, OpenMVG and mavmap front ends of line3dpp_amd/front_end.py without a GPU: the flag tables against the
reference's mains, the readers of io.py on hand-written files (tests/golden/front_ends_more/, one test per quirk of the
mains, expected values worked out here from the files' numbers), the three programs on the dataset of
tests/front_end_dataset_more.py against the `vsfm` program on the same scene (whose calls
tests/test_front_end_programs.py pins on the reference's own main), the numpy model of the triangulation, and the three
static helpers through the C-ABI and the C++ facade.  The reference's three mains cannot be compiled here (no recorder
build of them exists and main_openmvg.cpp needs RapidJSON), so their behaviour is pinned by these hand-made cases.

The Pix4D reader runs with tests/triangulate_model.py in place of the GPU's triangulate_points."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from line3dpp_amd import front_end, io
from tests import front_end_dataset as D
from tests import front_end_dataset_more as DM
from tests import triangulate_model as TM
from tests.sfm_readers_model import rotation_from_q
from tests.test_front_end_programs import Recorder, TAIL
from tests.test_front_ends_pinned import _calls, _touch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "front_ends_more")
EPS = np.finfo(np.float64).eps


def _ulps32(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(max(abs(a), abs(b))))


# ---- 1. the flag tables ------------------------------------------------------------------------------------------------
def test_flag_tables_are_the_reference_mains():
    """tests/golden/front_end_flags_more.json: written by hand from the TCLAP::ValueArg lines of the three mains"""
    with open(os.path.join(ROOT, "tests", "golden", "front_end_flags_more.json")) as f:
        want = json.load(f)
    kinds = {str: "string", int: "int", float: "float", bool: "bool"}
    for program in ("pix4d", "openmvg", "mavmap"):
        got = [dict(short=s, long=n, type=kinds[t], required=r, default=d) for s, n, t, r, d, _ in front_end.FLAGS[program]]
        assert got == want[program], program
        for g, w in zip(got, want[program]):
            assert type(g["default"]) is type(w["default"]), (program, g["long"])
        assert program in front_end.PROGRAMS and f"front_end {program} " in front_end.usage(program)
    assert "mavmap needs it" in front_end.usage("mavmap")
    assert sorted(front_end.PROGRAMS) == ["bundler", "colmap", "mavmap", "openmvg", "pix4d", "vsfm"]


def test_usage_names_six_programs(capsys):
    assert front_end.main([]) == 1
    err = capsys.readouterr().err
    assert "{vsfm|colmap|bundler|pix4d|openmvg|mavmap}" in err
    assert front_end.main(["pix4d", "-i", "x", "-b", "y"]) == 1 and "required argument missing: -f" in capsys.readouterr().err


# ---- 2. quirks of the mains on hand-written files ----------------------------------------------------------------------
def _read_image(path):
    return np.zeros((480, 640), np.uint8) if os.path.exists(path) else None


def _program(which, args, read_image=_read_image):
    rec = Recorder()
    rc = front_end.main([which] + list(args), line3d_factory=rec, read_image=read_image, undistort=rec.undistort)
    return rc, rec


def _rpy_matrix(r, p, y):
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def test_mavmap_tokens_lose_their_last_character_cy_included():
    cams = io.read_mavmap(os.path.join(GOLDEN, "mavmap_basic.txt"))
    a, d = cams[0], cams[3]
    assert a["name"] == "img_a"
    # "500.5," "501.5," "320.25," and the last token "240.57" without a comma: 240.5
    assert np.array_equal(a["K"], [[500.5, 0, 320.25], [0, 501.5, 240.5], [0, 0, 1]])
    # "400," "410," "300," "200,"
    assert np.array_equal(d["K"], [[400, 0, 300], [0, 410, 200], [0, 0, 1]])
    # pose: the inverse of [R t; 0 1] with R = Rz(0.3) Ry(-0.2) Rx(0.1), t = (1.5, -2.5, 3.5)
    Rw, C = _rpy_matrix(0.1, -0.2, 0.3), np.array([1.5, -2.5, 3.5])
    assert np.abs(a["R"] - Rw.T).max() <= 4 * EPS and np.abs(a["t"] + Rw.T @ C).max() <= 16 * EPS and np.array_equal(a["C"], C)
    assert np.array_equal(d["R"], np.eye(3)) and np.array_equal(d["t"], [-4.5, 2.5, -3.75])
    assert all(c["median_depth"] is None and not c["radial"].any() and not c["tangential"].any() for c in cams)


def test_mavmap_list_ends_at_a_short_line():
    cams = io.read_mavmap(os.path.join(GOLDEN, "mavmap_basic.txt"))
    assert [c["name"] for c in cams] == ["img_a", "img_b", "img_c", "img_d"]       # img_e stands behind a 17-character line
    assert [c["id"] for c in cams] == [0, 1, 2, 3]


def test_mavmap_other_camera_model_ends_the_program(tmp_path, capsys):
    with pytest.raises(ValueError, match="only PINHOLE camera model supported..."):
        io.read_mavmap(os.path.join(GOLDEN, "mavmap_fisheye.txt"))
    _touch(tmp_path, ["img_a.png", "img_b.png"])
    rc, rec = _program("mavmap", ["-i", str(tmp_path), "-b", os.path.join(GOLDEN, "mavmap_fisheye.txt"), "-t", "png"])
    assert rc == 1 and rec.constructed == 0 and "only PINHOLE camera model supported..." in capsys.readouterr().err


def test_mavmap_skipped_camera_keeps_the_indices_of_the_others(tmp_path):
    _touch(tmp_path, ["img_a.png", "img_b.png", "img_d.png"])                      # img_c has no file
    rc, rec = _program("mavmap", ["-i", str(tmp_path), "-b", os.path.join(GOLDEN, "mavmap_basic.txt"), "-t", "png", "-n", "2"])
    assert rc == 0
    added = _calls(rec.events, "addImage")
    assert [a["camID"] for a in added] == [0, 1, 3]
    # neighbors = 2: one before, then following ones until the list holds two -- positions in the file, camera 2 included
    assert [a["wps"] for a in added] == [[1, 2], [0, 2], [2]]
    assert rec.events[0]["neighbors_by_worldpoints"] == 0 and not _calls(rec.events, "undistortImage")
    assert [e["call"] for e in rec.events][-len(TAIL):] == TAIL


def test_mavmap_needs_its_extension(tmp_path, capsys):
    _touch(tmp_path, ["img_a.png", "img_b.png", "img_c.jpg", "img_d.png"])
    base = ["-i", str(tmp_path), "-b", os.path.join(GOLDEN, "mavmap_basic.txt")]
    rc, rec = _program("mavmap", base)                 # the file looked for ends in a bare '.': the probe is never reached
    assert rc == 0 and not _calls(rec.events, "addImage")
    seen = {}
    for ext in ("png", ".png"):
        paths = []
        rc, rec = _program("mavmap", base + ["-t", ext], read_image=lambda p: (paths.append(p), _read_image(p))[1])
        assert rc == 0
        seen[ext] = (paths, [a["camID"] for a in _calls(rec.events, "addImage")])
    assert seen["png"] == seen[".png"] == ([str(tmp_path) + f"/img_{c}.png" for c in "abd"], [0, 1, 3])
    _touch(tmp_path, ["img_a."])
    rc, rec = _program("mavmap", base)
    assert [a["camID"] for a in _calls(rec.events, "addImage")] == [0]
    # the image prefix stands in front of the file name
    _touch(tmp_path, ["sub/x_img_b.png"])
    rc, rec = _program("mavmap", base + ["-t", "png", "-f", "sub/x_"])
    assert [a["camID"] for a in _calls(rec.events, "addImage")] == [1]


def test_mavmap_neighbour_rule():
    """main_mavmap.cpp:311-321"""
    nb = io.mavmap_neighbors
    assert nb(0, 10, 4) == [1, 2, 3, 4]                        # the start: nothing before, four following
    assert nb(1, 10, 4) == [0, 2, 3, 4]
    assert nb(5, 10, 4) == [4, 3, 6, 7]                        # two before, nearest first, then two following
    assert nb(9, 10, 4) == [8, 7]                              # the end: the list stays short
    assert nb(8, 10, 4) == [7, 6, 9]
    assert nb(5, 10, 5) == [4, 3, 6, 7, 8]                     # odd: 5 / 2 = 2 before, 3 following
    assert nb(5, 10, 3) == [4, 6, 7] and nb(0, 1, 10) == []
    cams = io.read_mavmap(os.path.join(GOLDEN, "mavmap_basic.txt"), neighbors=3)
    assert [c["worldpoints"] for c in cams] == [[1, 2, 3], [0, 2, 3], [1, 3], [2]]


def test_mavmap_depth_and_sigma_p(tmp_path, capsys):
    _touch(tmp_path, [f"img_{c}.png" for c in "abcd"])
    base = ["-i", str(tmp_path), "-b", os.path.join(GOLDEN, "mavmap_basic.txt"), "-t", "png"]
    rc, rec = _program("mavmap", base)
    assert rc == 0 and all(a["median_depth"] == -1.0 for a in _calls(rec.events, "addImage"))
    assert _calls(rec.events, "matchImages")[0]["sigma_position"] == 2.5 and "reverting" not in capsys.readouterr().out
    rc, rec = _program("mavmap", base + ["-p", "-0.5"])        # metric sigma_p without a depth: the two lines, 2.5 px
    assert _calls(rec.events, "matchImages")[0]["sigma_position"] == 2.5
    out = capsys.readouterr().out
    assert "when no valid regularization depth (--const_reg_depth) is given!" in out and "reverting to: sigma_p = 2.5px" in out
    rc, rec = _program("mavmap", base + ["-p", "-0.5", "-z", "12.5"])
    m = _calls(rec.events, "matchImages")[0]
    assert (m["sigma_position"], m["const_regularization_depth"]) == (-0.5, 12.5) and "reverting" not in capsys.readouterr().out
    assert all(a["median_depth"] == 12.5 for a in _calls(rec.events, "addImage"))
    assert rec.events[0]["output_folder"] == str(tmp_path) + "/Line3D++/"
    rc, rec = _program("mavmap", ["-i", str(tmp_path), "-b", str(tmp_path / "none.txt"), "-t", "png"])
    assert rc == 1 and rec.constructed == 0 and "does not exist!" in capsys.readouterr().err


def _openmvg(tmp_path, names=("a.png", "b.png", "d.png")):
    _touch(tmp_path / "imgs", names)
    return io.read_openmvg(os.path.join(GOLDEN, "openmvg_small.json"), str(tmp_path / "imgs"))


def test_openmvg_polymorphic_name_is_inherited(tmp_path):
    views = {v["id"]: v for v in _openmvg(tmp_path)}
    # group 0 is named pinhole_radial_k3; group 1 has no name and is read as the same model: its disto_k3 (all zero)
    assert np.array_equal(views[10]["radial"], [0.01, -0.002, 0.0003]) and not views[10]["tangential"].any()
    assert np.array_equal(views[11]["radial"], [0, 0, 0])
    assert np.array_equal(views[10]["K"], [[500.5, 0, 320.25], [0, 500.5, 240.75], [0, 0, 1]])
    assert np.array_equal(views[11]["K"], [[510.5, 0, 321.25], [0, 510.5, 241.75], [0, 0, 1]])
    # undistortion only where a coefficient exceeds L3D_EPS
    assert io.front_end_undistortion("openmvg", views[10], 640, 480) is not None
    assert io.front_end_undistortion("openmvg", views[11], 640, 480) is None


def test_openmvg_missing_file_and_orphaned_pose(tmp_path, capsys):
    views = _openmvg(tmp_path)
    err = capsys.readouterr().err
    assert "WARNING: image 'c.png' not found (ID=12)" in err and "WARNING: pose with ID 2 does not map to an image!" in err
    assert [v["id"] for v in views] == [10, 11, 13] and [v["path"] for v in views] == [str(tmp_path / "imgs") + "/" + n for n in ("a.png", "b.png", "d.png")]
    # worldpoints: the keys in file order; depths from the centres: view 10 at (0.5, 0.25, -1) sees 3, 5, 4 and 8 away
    assert [v["worldpoints"] for v in views] == [[7, 3, 9, 4], [7, 9], [3, 9]]
    assert [v["median_depth"] for v in views] == [np.float32(5.0), np.float32(np.sqrt(17.0)), np.float32(np.sqrt(34.0))]
    assert all(type(v["median_depth"]) is np.float32 for v in views)
    # t = -R C
    assert np.array_equal(views[1]["t"], [0.25, -1.5, 1.0]) and np.array_equal(views[0]["t"], [-0.5, -0.25, 1.0])
    assert np.array_equal(views[2]["R"], [[1, 0, 0], [0, 0, -1], [0, 1, 0]]) and np.array_equal(views[2]["C"], [3.5, 0.25, -1.0])
    # with c.png in place the view is read, and nothing is orphaned
    views = _openmvg(tmp_path, ("c.png",))
    assert [v["id"] for v in views] == [10, 11, 12, 13] and "WARNING" not in capsys.readouterr().err.replace("WARNING: camera model", "")


def test_openmvg_unknown_camera_model(tmp_path, capsys):
    views = _openmvg(tmp_path)
    assert "WARNING: camera model 'fisheye' for group 2 unknown! No distortion assumed..." in capsys.readouterr().err
    assert not views[2]["radial"].any() and not views[2]["tangential"].any()
    assert np.array_equal(views[2]["K"], [[520.5, 0, 322.25], [0, 520.5, 242.75], [0, 0, 1]])
    rc, rec = _program("openmvg", ["-i", str(tmp_path / "imgs"), "-j", os.path.join(GOLDEN, "openmvg_small.json")])
    assert rc == 0 and [a["camID"] for a in _calls(rec.events, "addImage")] == [10, 11, 13]
    assert len(_calls(rec.events, "undistortImage")) == 1 and rec.events[0]["neighbors_by_worldpoints"] == 1
    assert rec.events[0]["output_folder"] == str(tmp_path / "imgs") + "/Line3D++/"


@pytest.mark.parametrize("key,message", [("views", "No aligned cameras in json file!"), ("intrinsics", "No intrinsics in json file!"),
                                         ("extrinsics", "No extrinsics in json file!"), ("structure", "No worldpoints in json file!")])
def test_openmvg_empty_sections_end_the_program(tmp_path, capsys, key, message):
    with open(os.path.join(GOLDEN, "openmvg_small.json")) as f:
        d = json.load(f)
    d[key] = []
    (tmp_path / "sfm_data.json").write_text(json.dumps(d))
    _touch(tmp_path, ["a.png", "b.png", "d.png"])
    rc, rec = _program("openmvg", ["-i", str(tmp_path), "-j", str(tmp_path / "sfm_data.json")])
    assert rc == 1 and rec.constructed == 0 and message in capsys.readouterr().err
    rc, rec = _program("openmvg", ["-i", str(tmp_path), "-j", str(tmp_path / "none.json")])
    assert rc == 1 and "OpenMVG json file" in capsys.readouterr().err


def _pix4d(prefix="quirks", **kw):
    return io.read_pix4d(GOLDEN, prefix, triangulate=kw.pop("triangulate", TM.triangulate_points), **kw)


def test_pix4d_prefix_with_and_without_underscore(tmp_path, capsys):
    a, b = _pix4d("quirks"), _pix4d("quirks_")
    assert [c["id"] for c in a] == [c["id"] for c in b] == [0, 1, 2]
    assert io.pix4d_files("/p", "x") == io.pix4d_files("/p", "x_") == ("/p/x_calibrated_camera_parameters.txt", "/p/x_tp_pix4d.txt")
    shutil.copy(os.path.join(GOLDEN, "quirks_tp_pix4d.txt"), tmp_path / "only_tp_pix4d.txt")
    capsys.readouterr()
    rc, rec = _program("pix4d", ["-i", str(tmp_path), "-b", str(tmp_path), "-f", "only"])
    err = capsys.readouterr().err
    assert rc == 1 and rec.constructed == 0 and "pix4d file '" in err and "only_calibrated_camera_parameters.txt' or '\n" in err


def test_pix4d_camera_file():
    """the header ends at the empty line, the list at `end`; centre to t = -R C; the key is the name up to the LAST dot"""
    cams = _pix4d()
    assert [c["name"] for c in cams] == ["cam_a.jpg", "cam_b.v2.jpg", "cam_c.jpg"]          # cam_z stands behind `end`
    assert all(np.array_equal(c["K"], [[100, 0, 50], [0, 100, 50], [0, 0, 1]]) and np.array_equal(c["R"], np.eye(3)) for c in cams)
    assert [c["t"].tolist() for c in cams] == [[0, 0, 0], [-1, 0, 0], [-2, 0, 0]]
    assert np.array_equal(cams[1]["P"], [[100, 0, 50, -100], [0, 100, 50, 0], [0, 0, 1, 0]])


def test_pix4d_unknown_key_image_lands_on_position_0(capsys):
    calls = []

    def spy(P, off, cam, xy):
        calls.append((np.array(off), np.array(cam), np.array(xy)))
        return TM.triangulate_points(P, off, cam, xy)
    _pix4d(triangulate=spy)
    out = capsys.readouterr().out
    assert "Pix4D: #cameras = 5" in out and "Pix4D: #points  = 6" in out and "triangulating..." in out   # 4 cameras and `ghost`
    (off, cam, xy), = calls
    # features in order of first appearance: f01 f02 f03 f04 f04b f05; f05 was seen under `ghost`: camera 0, pixel (55, 55)
    assert off.tolist() == [0, 4, 8, 11, 13, 14, 15]
    assert cam[14] == 0 and xy[14].tolist() == [55.0, 55.0]
    assert cam[:4].tolist() == [0, 1, 2, 3] and xy[:4].tolist() == [[50, 50], [40, 50], [30, 50], [50, 40]]


def test_pix4d_line_that_starts_with_a_dash_and_the_end_of_the_file():
    cams = _pix4d()
    # `-f09 10 10 1.5` under cam_a is no feature; `x` ends the file, so f06 under the second `cam_c` is never read
    assert cams[0]["worldpoints"] == [0, 1, 2, 3] and cams[2]["worldpoints"] == [0, 1, 2]


def test_pix4d_feature_with_two_observations_is_invalid_and_stays_in_the_list():
    cams = _pix4d()
    # f04 (id 3) is seen by cam_a and cam_b only: not triangulated, no depth, but handed to addImage
    assert 3 in cams[0]["worldpoints"] and 3 in cams[1]["worldpoints"]
    # depths of cam_a at the origin to f01 (0,0,10), f02 (1,1,10), f03 (-2,1,10): 10, sqrt(102), sqrt(105); f04 would be sqrt(104)
    assert _ulps32(cams[0]["median_depth"], np.sqrt(102.0)) <= 1
    # cam_b at (1,0,0): sqrt(101), sqrt(101), sqrt(110); cam_c at (2,0,0): sqrt(104), sqrt(102), sqrt(117)
    assert _ulps32(cams[1]["median_depth"], np.sqrt(101.0)) <= 1 and _ulps32(cams[2]["median_depth"], np.sqrt(104.0)) <= 1
    assert all(type(c["median_depth"]) is np.float32 for c in cams)


def test_pix4d_camera_with_two_valid_depths_is_not_added():
    # cam_d sees f01, f02 (valid) and f04b (one observation): two depths, and the reference asks for more than two
    assert [c["id"] for c in _pix4d()] == [0, 1, 2]


def test_pix4d_undistorts_with_all_zero_coefficients(tmp_path, monkeypatch):
    cams = _pix4d()
    und = io.front_end_undistortion("pix4d", cams[0], 100, 100)
    assert und is not None and np.array_equal(und[0], cams[0]["K"]) and not und[1].any() and not und[2].any()
    read = io.read_pix4d
    # this kind always undistorts, so it takes read_pix4d's own entries only: another reader's entry is refused
    foreign = {k: v for k, v in cams[0].items() if k != "P"}
    with pytest.raises(ValueError, match="element of read_pix4d"):
        io.front_end_undistortion("pix4d", foreign, 100, 100)
    with pytest.raises(ValueError, match="unknown front end"):
        io.front_end_undistortion("photoscan", cams[0], 100, 100)
    monkeypatch.setattr(io, "read_pix4d", lambda folder, prefix, **kw: read(folder, prefix, triangulate=TM.triangulate_points))
    _touch(tmp_path, ["cam_a.jpg", "cam_b.v2.jpg", "cam_c.jpg", "cam_d.jpg"])
    rc, rec = _program("pix4d", ["-i", str(tmp_path), "-b", GOLDEN, "-f", "quirks"])
    assert rc == 0 and rec.events[0]["neighbors_by_worldpoints"] == 1
    assert [a["camID"] for a in _calls(rec.events, "addImage")] == [0, 1, 2] and len(_calls(rec.events, "undistortImage")) == 3
    assert all(u["radial"] == [0, 0, 0] and u["tangential"] == [0, 0] for u in _calls(rec.events, "undistortImage"))
    assert _calls(rec.events, "addImage")[0]["wps"] == [0, 1, 2, 3]


# ---- 3. the three programs against the vsfm program on the same scene ------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    folder = tmp_path_factory.mktemp("front_end_dataset_more")
    sc, X = DM.write(folder)
    return folder, sc, X


def _sized_image(path):
    return np.zeros((D.HEIGHT, D.WIDTH), np.uint8) if os.path.exists(path) else None


@pytest.fixture(scope="module")
def vsfm_calls(dataset, tmp_path_factory):
    folder, _, _ = dataset
    rc, rec = _program("vsfm", ["-m", str(folder / "model.nvm"), "-o", str(tmp_path_factory.mktemp("vsfm_out"))], read_image=_sized_image)
    assert rc == 0
    return rec.events


def _against_vsfm_and_scene(events, vsfm, sc, wps_of=None):
    ours, ref = _calls(events, "addImage"), _calls(vsfm, "addImage")
    assert [a["camID"] for a in ours] == [a["camID"] for a in ref] == [v.cam for v in sc.views]
    assert [(a["cols"], a["rows"]) for a in ours] == [(a["cols"], a["rows"]) for a in ref] == [(D.WIDTH, D.HEIGHT)] * D.N_VIEWS
    worst = dict(R_vsfm=0.0, t_vsfm=0.0, R_scene=0.0, t_scene=0.0)
    for a, b, v in zip(ours, ref, sc.views):
        assert a["K"] == b["K"]
        if wps_of is not None:
            assert wps_of(a["wps"]) == b["wps"] == v.worldpoints
        worst["R_vsfm"] = max(worst["R_vsfm"], np.abs(np.array(a["R"]) - np.array(b["R"])).max())
        worst["t_vsfm"] = max(worst["t_vsfm"], np.abs(np.array(a["t"]) - np.array(b["t"])).max())
        worst["R_scene"] = max(worst["R_scene"], np.abs(np.array(a["R"]).reshape(3, 3) - v.R).max())
        worst["t_scene"] = max(worst["t_scene"], np.abs(np.array(a["t"]) - v.t).max())
    print(worst)
    # the .nvm writer prints 12 significant digits: R within 1e-11, t within 1e-9 of the vsfm program's; the new files carry
    # the scene's cameras at full precision
    assert worst["R_vsfm"] <= 1e-11 and worst["t_vsfm"] <= 1e-9 and worst["R_scene"] <= 1e-13 and worst["t_scene"] <= 1e-13
    for x, y in zip(events[-len(TAIL):], vsfm[-len(TAIL):]):
        assert {k: v for k, v in x.items() if k != "folder"} == {k: v for k, v in y.items() if k != "folder"}
    return ours, ref


def test_openmvg_program_against_vsfm(dataset, vsfm_calls, tmp_path):
    folder, sc, _ = dataset
    rc, rec = _program("openmvg", DM.argv(folder, "openmvg", tmp_path / "out"), read_image=_sized_image)
    assert rc == 0 and rec.constructed == 1 and rec.events[0]["neighbors_by_worldpoints"] == 1
    ours, ref = _against_vsfm_and_scene(rec.events, vsfm_calls, sc, wps_of=lambda w: w)
    ulps = [_ulps32(a["median_depth"], b["median_depth"]) for a, b in zip(ours, ref)]
    print("median_depth, float32 ulps from vsfm:", ulps)
    assert max(ulps) <= 2
    # the same two cameras are undistorted, with K and (k1, 0, 0) -- the .nvm holds k1 as a float32
    a, b = _calls(rec.events, "undistortImage"), _calls(vsfm_calls, "undistortImage")
    assert len(a) == len(b) == len(D.DISTORTION)
    for x, y, k1 in zip(a, b, [D.DISTORTION[c] for c in sorted(D.DISTORTION)]):
        assert x["K"] == y["K"] and x["radial"] == [k1, 0.0, 0.0] and x["tangential"] == [0.0, 0.0]
        assert y["radial"] == [float(np.float32(k1)), 0.0, 0.0]


def test_pix4d_program_against_vsfm(dataset, vsfm_calls, tmp_path, monkeypatch):
    folder, sc, X = dataset
    read = io.read_pix4d
    monkeypatch.setattr(io, "read_pix4d", lambda params, prefix, **kw: read(params, prefix, triangulate=TM.triangulate_points))
    rc, rec = _program("pix4d", DM.argv(folder, "pix4d", tmp_path / "out"), read_image=_sized_image)
    assert rc == 0 and rec.constructed == 1 and rec.events[0]["neighbors_by_worldpoints"] == 1
    order = DM.pix4d_feature_order(sc)              # feature id -> worldpoint: Pix4D numbers features by first appearance
    ours, _ = _against_vsfm_and_scene(rec.events, vsfm_calls, sc, wps_of=lambda w: [order[f] for f in w])
    assert len(_calls(rec.events, "undistortImage")) == D.N_VIEWS               # every added view
    # the depths are those of the triangulated points with more than two observations
    count = np.zeros(len(X), int)
    for v in sc.views:
        count[v.worldpoints] += 1
    for a, v in zip(ours, sc.views):
        d = sorted(np.float32(np.linalg.norm(X[i] + v.R.T @ v.t)) for i in v.worldpoints if count[i] > 2)
        assert 386 <= len(d) <= 454 and _ulps32(a["median_depth"], d[len(d) // 2]) <= 1


def test_mavmap_program_against_vsfm(dataset, vsfm_calls, tmp_path):
    folder, sc, _ = dataset
    rc, rec = _program("mavmap", DM.argv(folder, "mavmap", tmp_path / "out") + ["-n", "4"], read_image=_sized_image)
    assert rc == 0 and rec.constructed == 1 and rec.events[0]["neighbors_by_worldpoints"] == 0      # constructed with False
    vsfm = [dict(e, num_neighbors=4) if e["call"] == "matchImages" else e for e in vsfm_calls]
    ours, _ = _against_vsfm_and_scene(rec.events, vsfm, sc)
    assert [a["wps"] for a in ours] == [io.mavmap_neighbors(i, D.N_VIEWS, 4) for i in range(D.N_VIEWS)]
    assert ours[0]["wps"] == [1, 2, 3, 4] and ours[3]["wps"] == [2, 1, 4, 5] and ours[6]["wps"] == [5, 4]
    assert all(a["median_depth"] == -1.0 for a in ours) and not _calls(rec.events, "undistortImage")
    rc, rec = _program("mavmap", DM.argv(folder, "mavmap", tmp_path / "out2") + ["-p", "-0.05", "-z", str(DM.MAVMAP_DISTANCE)],
                       read_image=_sized_image)
    assert rc == 0 and all(a["median_depth"] == DM.MAVMAP_DISTANCE for a in _calls(rec.events, "addImage"))


def test_chunking_does_not_change_the_calls(dataset, tmp_path, monkeypatch):
    folder, _, _ = dataset
    args = DM.argv(folder, "openmvg", tmp_path / "out")
    _, whole = _program("openmvg", args, read_image=_sized_image)
    monkeypatch.setenv(front_end.CHUNK_ENV, str(2 * D.WIDTH * D.HEIGHT))
    _, parts = _program("openmvg", args, read_image=_sized_image)
    for name in ("undistortImage", "addImage"):
        assert _calls(whole.events, name) == _calls(parts.events, name)
    names = [e["call"] for e in parts.events if e["call"] in ("undistortImage", "addImage")]
    assert sum(1 for a, b in zip(names, names[1:]) if a == "addImage" and b == "undistortImage") >= 1


# ---- 4. the numpy model of the triangulation --------------------------------------------------------------------------------
def _dataset_observations(sc, X, noise=0.0, seed=0):
    seen = [[v.cam for v in sc.views if i in set(v.worldpoints)] for i in range(len(X))]
    Ps = np.array([v.K @ np.column_stack([v.R, v.t]) for v in sc.views])
    return (Ps,) + TM.observations(Ps, X, seen, noise, np.random.default_rng(seed))


def test_model_gives_back_the_worldpoints_of_exact_observations(dataset):
    _, sc, X = dataset
    Ps, off, cam, xy = _dataset_observations(sc, X)
    Xm, valid = TM.triangulate_points(Ps, off, cam, xy)
    counts = np.diff(off.astype(np.int64))
    assert np.array_equal(valid, counts > 2) and valid.sum() == 578 and (~valid).sum() == 22
    assert not Xm[~valid].any()
    extent = np.ptp(X, axis=0).max()
    err = np.linalg.norm(Xm[valid] - X[valid], axis=1).max() / extent
    Xe, ve = TM.solve_eigh(TM.normal_matrices(Ps, off, cam, xy), counts)
    apart = np.linalg.norm(Xm[valid] - Xe[valid], axis=1).max() / extent
    print(f"model to worldpoints {err:.3g}, svd to eigh {apart:.3g} of the extent {extent:.3g}")
    assert np.array_equal(ve, valid)
    # exact observations: M's smallest singular value is rounding only; cond(M) 6.6e3 times eps, with room
    assert err <= 1e-10 and apart <= 1e-10
    per_view = [int(valid[v.worldpoints].sum()) for v in sc.views]
    assert min(per_view) >= 386 and max(per_view) <= 454


def test_model_validity_rule():
    P = np.array([[[100, 0, 50, -100.0 * c], [0, 100, 50, 0], [0, 0, 1, 0]] for c in range(4)], np.float64)
    X = np.array([[0.5, -0.25, 10.0], [0.0, 0.0, 0.0], [1.0, 2.0, 5.0], [1.0, 2.0, 5.0], [1.0, 2.0, 5.0]])
    seen = [[0, 1, 2, 3], [0, 1, 2], [0, 1], [2], []]
    off, cam, xy = TM.observations(P, X, seen)
    xy[4:7] = [[50.0, 50.0], [50.0, 50.0], [50.0, 50.0]]      # the origin lies in every camera's plane of centres: give it pixels
    Xm, valid = TM.triangulate_points(P, off, cam, xy)
    assert valid.tolist() == [True, False, False, False, False] and np.abs(Xm[0] - X[0]).max() < 1e-12 and not Xm[1:].any()
    xy[0, 0] = np.nan
    assert not TM.triangulate_points(P, off, cam, xy)[1][0]     # a NaN is invalid


# ---- 5. the static helpers ------------------------------------------------------------------------------------------------
def _lib():
    from line3dpp_amd import _lib as L
    return L.load(), L.ptr


def test_rotation_from_rpy_is_the_product_of_three_elementary_rotations():
    from line3dpp_amd.api import Line3D
    grid = np.linspace(-np.pi, np.pi, 9)
    for r in grid:
        for p in grid:
            for y in grid:
                R = Line3D.rotationFromRPY(r, p, y)
                # three products of entries bounded by 1, each a rounded sine or cosine: a few eps
                assert np.abs(R - _rpy_matrix(r, p, y)).max() <= 8 * EPS, (r, p, y)
                assert np.array_equal(R, io.rotation_from_rpy(r, p, y))
    assert np.array_equal(Line3D.rotationFromRPY(0, 0, 0), np.eye(3))


def test_rotation_from_q_equals_the_reader_s():
    from line3dpp_amd.api import Line3D
    rng = np.random.default_rng(5)
    for q in list(rng.normal(size=(50, 4))) + [np.array([1.0, 0, 0, 0]), np.zeros(4), np.array([0, 0, 0, 1e-7])]:
        assert np.array_equal(Line3D.rotationFromQ(*q), rotation_from_q(*q))


def _decompose_cases(sc):
    cases = [(v.K, v.R, v.t) for v in sc.views]
    K = np.array([[812.5, 3.75, 402.0], [0, 790.25, 297.5], [0, 0, 1.0]])           # with skew
    for v in sc.views[:3]:
        cases.append((K, v.R, v.t))
    return cases


def _check_decomposition(K, R, t, k, r, tt):
    assert (np.diag(k) > 0).all() and k[2, 2] == 1.0      # (below the diagonal the Givens steps leave rounding, as in the reference)
    # P carries rounding of eps |P|; recovering the factors multiplies it by the condition of K, the entries of K by |K|
    cond = np.linalg.cond(K)
    bound = 16 * EPS * cond
    assert np.abs(r - R).max() <= bound, (np.abs(r - R).max(), bound)
    assert np.abs(k - K).max() <= bound * np.abs(K).max(), (np.abs(k - K).max(), bound * np.abs(K).max())
    assert np.abs(tt - t).max() <= bound * max(1.0, np.abs(t).max()), (np.abs(tt - t).max(), bound)


def test_decompose_projection_matrix_gives_back_the_factors(dataset):
    from line3dpp_amd.api import Line3D
    _, sc, _ = dataset
    L, ptr = _lib()
    for K, R, t in _decompose_cases(sc):
        P = K @ np.column_stack([R, t])
        _check_decomposition(K, R, t, *Line3D.decomposeProjectionMatrix(P))
        k, r, tt = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3)
        assert L.l3d_decompose_projection_matrix(ptr(np.ascontiguousarray(P)), ptr(k), ptr(r), ptr(tt)) == 0
        assert all(np.array_equal(a, b) for a, b in zip((k, r, tt), Line3D.decomposeProjectionMatrix(P)))
    assert Line3D.decomposeProjectionMatrix(np.zeros((4, 3))) is None
    r9 = np.zeros(9)
    assert L.l3d_rotation_from_rpy(0.1, 0.2, 0.3, ptr(r9)) == 0 and np.array_equal(r9.reshape(3, 3), io.rotation_from_rpy(0.1, 0.2, 0.3))
    assert L.l3d_rotation_from_q(0.5, 0.5, -0.5, 0.5, ptr(r9)) == 0 and np.array_equal(r9.reshape(3, 3), rotation_from_q(0.5, 0.5, -0.5, 0.5))
    assert L.l3d_rotation_from_rpy(0.1, 0.2, 0.3, None) != 0


def test_helpers_through_the_cpp_facade(dataset, tmp_path):
    """tests/cpp/helpers_facade.cpp: the three static members of the facade's Line3D; host code, so it runs here"""
    _, sc, _ = dataset
    exe = str(tmp_path / "helpers_facade")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "helpers_facade.cpp"), "-o", exe, "-L" + lib_dir,
                           "-ll3dpp_hip", "-Wl,-rpath," + lib_dir])
    cases = _decompose_cases(sc)
    rows = ["%d" % len(cases)]
    for K, R, t in cases:
        rows.append(" ".join("%.17g" % x for x in (K @ np.column_stack([R, t])).reshape(-1)))
    angles = [(0.1, -0.2, 0.3), (-2.5, 1.25, 3.0), (0.0, 0.0, 0.0)]
    quats = [(0.5, 0.5, -0.5, 0.5), (0.3, -0.1, 0.9, 0.2), (0.0, 0.0, 0.0, 0.0)]
    rows.append("%d" % len(angles))
    rows += [" ".join("%.17g" % x for x in a + q) for a, q in zip(angles, quats)]
    run = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    out = [np.array(line.split(), np.float64) for line in run.stdout.strip().split("\n") if not line.startswith("P is not")]
    assert "P is not a 3x4 matrix! (4x3)" in run.stdout
    from line3dpp_amd.api import Line3D
    for (K, R, t), got in zip(cases, out):
        k, r, tt = Line3D.decomposeProjectionMatrix(K @ np.column_stack([R, t]))
        assert np.array_equal(got, np.concatenate([k.reshape(-1), r.reshape(-1), tt]))
        _check_decomposition(K, R, t, got[:9].reshape(3, 3), got[9:18].reshape(3, 3), got[18:])
    for a, q, got in zip(angles, quats, out[len(cases):]):
        assert np.array_equal(got[:9].reshape(3, 3), io.rotation_from_rpy(*a)) and np.array_equal(got[9:].reshape(3, 3), rotation_from_q(*q))
