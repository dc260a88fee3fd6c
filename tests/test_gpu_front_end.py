"""The front ends of line3dpp_amd/front_end.py end to end on the MI355X: a rendered dataset (tests/front_end_dataset.py:
7 views of 1024 x 768, two of them with a radial distortion) in the three SfM formats goes through the three programs,
each a fresh child process, and the STL / OBJ / TXT / BIN they leave are held against the same dataset pushed through
the library's API step by step (written out below, without front_end), against a run with one or two images per chunk,
and against what a reconstruction has to look like.  The CPU side (tests/test_front_end_programs.py) pins the calls on the
reference's mains; this pins that the calls, made on the real library, give the files.

No count of 3D lines and no distance to the synthetic structure is asserted: there is no reference run of this dataset
(the reference's detector needs OpenCV).  DESIGN §13 records what one run found, beside the count the reference's own
line3D.cc reconstructs from the CPU model's segments of the same images.

Time limits.  The first run of this file on an MI355X (one run, shared machine) took 2.0 s for the
dataset and the three child processes of check 1 together, 0.8 s for the chunked child and 5.7 s for the whole file: at
1024 x 768 with about a hundred segments per image the detection of a batch takes 0.14 s, not the seconds of a full-size
photograph.  CHILD_TIMEOUT_S is that with a wide margin for a shared machine whose process start-up
varies.  A child that runs into it, or dies by a signal, ends the session: nothing
else is started on that GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from line3dpp_amd import io
from tests import front_end_dataset as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120
SUFFIXES = (".stl", ".obj", ".txt", ".bin")
FORMATS = ("vsfm", "colmap", "bundler")


def _argv(data, fmt, out):
    return {"vsfm": ["-m", str(data / "model.nvm"), "-o", str(out)],                         # the .nvm's own image paths
            "colmap": ["-i", str(data / "images"), "-m", str(data / "colmap"), "-o", str(out)],
            "bundler": ["-i", str(data / "bundler_images"), "-b", str(data / "bundle.rd.out"), "-o", str(out)]}[fmt]


def _child(fmt, args, env=None):
    cmd = [sys.executable, "-m", "line3dpp_amd.front_end", fmt] + args
    try:
        run = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, **(env or {})), capture_output=True, text=True,
                             timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        pytest.exit(f"front end {fmt} did not finish within {CHILD_TIMEOUT_S} s: nothing more is started on this GPU", 3)
    if run.returncode < 0:
        pytest.exit(f"front end {fmt} died by signal {-run.returncode}: nothing more is started on this GPU\n{run.stderr[-2000:]}", 3)
    print(run.stdout[-3000:])
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout


def _files(folder):
    """name -> bytes of the files of a result folder (the segment cache lives in its L3D++_data directory)"""
    names = sorted(os.listdir(folder))
    assert [n for n in names if os.path.isdir(os.path.join(folder, n))] in ([], ["L3D++_data"])
    return {n: open(os.path.join(folder, n), "rb").read() for n in names if os.path.isfile(os.path.join(folder, n))}


def _longhand(data, fmt, out):
    """the dataset through the existing API, step by step: what a user had to write before there was a front end"""
    from line3dpp_amd.api import Line3D
    from line3dpp_amd.lsd import read_image_gray, undistort_images
    if fmt == "vsfm":
        entries = io.read_nvm(str(data / "model.nvm"))
        views = [(i, str(data / e["filename"]), e) for i, e in enumerate(entries)]
        kind = "nvm"
    elif fmt == "colmap":
        entries = io.read_colmap(str(data / "colmap"))
        views = [(e["id"], str(data / "images" / e["name"]), e) for e in entries]
        kind = "colmap"
    else:
        entries = io.read_bundler(str(data / "bundle.rd.out"))
        views = [(i, str(data / "bundler_images" / f"{i:08d}.png"), e) for i, e in enumerate(entries)]
        kind = "bundler"
    os.makedirs(out)
    images = [read_image_gray(path) for _, path, _ in views]
    assert all(e["worldpoints"] for e in entries) and all(im.shape == (D.HEIGHT, D.WIDTH) for im in images)
    und = [io.front_end_undistortion(kind, e, D.WIDTH, D.HEIGHT) for e in entries]
    todo = [i for i, u in enumerate(und) if u is not None]
    assert len(todo) == len(D.DISTORTION)
    done = undistort_images([images[i] for i in todo], [und[i][0] for i in todo], [und[i][1] for i in todo], [und[i][2] for i in todo])
    for i, im in zip(todo, done):
        assert im.shape == images[i].shape and not np.array_equal(im, images[i])      # the undistort branch did something
        images[i] = im
    g = Line3D(str(out), True, -1, 3000, True, True)
    for (cam, _, e), im in zip(views, images):
        K = e["K"] if kind == "colmap" else io.nvm_intrinsics(e["focal"], D.WIDTH, D.HEIGHT)
        g.addImage(cam, im, K, e["R"], e["t"], float(e["median_depth"]), e["worldpoints"])
    assert g.numImages() == D.N_VIEWS
    assert g.matchImages(2.5, 10.0, 10, 0.25, 10, -1.0)
    assert g.reconstruct3Dlines(3, False, -1.0, False)
    name = g.outputFilename()
    assert g.saveResultAsSTL(str(out)) and g.saveResultAsOBJ(str(out)) and g.save3DLinesAsTXT(str(out)) and g.save3DLinesAsBIN(str(out))
    g.close()
    return name


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    folder = tmp_path_factory.mktemp("front_end_dataset")
    D.write(folder)
    return folder


@pytest.fixture(scope="module")
def programs(data, tmp_path_factory):
    """check 1's three child processes, one after another: format -> (result folder, stdout)"""
    out = {}
    for fmt in FORMATS:
        folder = tmp_path_factory.mktemp("out_" + fmt)
        out[fmt] = (folder, _child(fmt, _argv(data, fmt, folder)))
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_program_leaves_the_four_files_and_they_are_the_longhand_pipelines(data, programs, tmp_path, fmt):
    folder, stdout = programs[fmt]
    got = _files(folder)
    name = _longhand(data, fmt, tmp_path / "longhand")
    assert sorted(got) == sorted(name + s for s in SUFFIXES)                 # exactly the four, named by outputFilename
    assert "seconds per stage: read " in stdout and all(s in stdout for s in ("undistort", "add", "match", "reconstruct", "save"))
    want = _files(tmp_path / "longhand")
    assert sorted(want) == sorted(got)
    for n in got:
        assert got[n] == want[n], f"{fmt}: {n} differs from the step-by-step pipeline's"


def test_chunking_does_not_change_the_result(data, programs, tmp_path):
    from line3dpp_amd import front_end
    budget = 2 * D.WIDTH * D.HEIGHT                                         # two images per chunk, one in the last
    _child("vsfm", _argv(data, "vsfm", tmp_path / "out"), env={front_end.CHUNK_ENV: str(budget)})
    assert _files(tmp_path / "out") == _files(programs["vsfm"][0])


def _lines(folder):
    (txt,) = [n for n in os.listdir(folder) if n.endswith(".txt")]
    return io.read_3d_lines_txt(os.path.join(folder, txt))


def _clusters(lines):
    return {frozenset((int(c), int(s)) for c, s in L["residuals"]) for L in lines}


@pytest.mark.parametrize("fmt", FORMATS)
def test_result_is_a_reconstruction(programs, fmt):
    lines = _lines(programs[fmt][0])
    print(f"{fmt}: {len(lines)} 3D lines, {sum(len(L['segments']) for L in lines)} 3D segments")
    assert len(lines) >= 1
    for L in lines:
        assert len(L["segments"]) >= 1 and len({int(c) for c, _ in L["residuals"]}) >= 3
        assert all(0 <= int(c) < D.N_VIEWS + 1 for c, _ in L["residuals"])


def test_visibility_4_keeps_a_subset_of_the_clusters(data, programs, tmp_path):
    from line3dpp_amd import front_end
    g, times = front_end.run_vsfm(_argv(data, "vsfm", tmp_path / "v4") + ["-v", "4"])
    g.close()
    v3, v4 = _lines(programs["vsfm"][0]), _lines(tmp_path / "v4")
    print(f"visibility 3: {len(v3)} lines, visibility 4: {len(v4)} lines; seconds per stage {times}")
    assert set(times) == set(front_end.STAGES) and all(t >= 0 for t in times.values())
    assert len(v4) >= 1 and _clusters(v4) <= _clusters(v3)
    for L in v4:
        assert len({int(c) for c, _ in L["residuals"]}) >= 4
    assert any(n.endswith("vis_4.txt") for n in os.listdir(tmp_path / "v4"))


def test_flags_reach_the_library(data, tmp_path):
    from line3dpp_amd import front_end
    g, _ = front_end.run_vsfm(_argv(data, "vsfm", tmp_path / "out") + ["-d", "1", "-r", "2", "-c", "1", "-k", "5", "-w", "1000"])
    stats = g.lineOptStats()
    name = g.outputFilename(1000)
    g.close()
    files = _files(tmp_path / "out")
    assert sorted(files) == sorted(name + s for s in SUFFIXES)
    for token in ("W_1000", "kNN_5", "COLLIN_2", "DIFFUSION", "OPTIMIZED"):   # Line3D::createOutputFilename, line3D.cc:2853-2893
        assert token in name, (token, name)
    print(f"line bundling: {stats}")
    assert stats["lines_bundled"] + stats["lines_constant"] >= 1 and stats["residuals"] >= 1
    assert len(io.read_3d_lines_txt(os.path.join(tmp_path / "out", name + ".txt"))) >= 1
