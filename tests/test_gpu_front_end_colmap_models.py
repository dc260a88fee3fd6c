"""`python -m line3dpp_amd.front_end colmap` end to end on the MI355X on a COLMAP binary model whose cameras are an
OPENCV_FISHEYE (two views), a FOV (one view) and pinholes (tests/front_end_dataset_models.py).  The program
runs as a child process under the limit of tests/test_gpu_front_end.py; its four files are held against the same dataset
pushed through the library step by step, against the text form of the same model, and against what a reconstruction has
to look like.  No count of 3D lines is asserted beyond "more than zero"; DESIGN §15 records what one run found."""
import os

import numpy as np
import pytest

from line3dpp_amd import io
from tests import front_end_dataset_models as D
from tests.test_gpu_front_end import SUFFIXES, _child, _files, _lines

pytestmark = pytest.mark.gpu

VISIBILITY_T = 3                  # the program's default -v


def _argv(data, form, out):
    return ["-i", str(data / "images"), "-m", str(data / ("colmap_" + form)), "-o", str(out)]


def _longhand(data, out):
    """the binary dataset through the API, step by step"""
    from line3dpp_amd.api import Line3D
    from line3dpp_amd.lsd import read_image_gray, undistort_images_model
    entries = io.read_colmap(str(data / "colmap_bin"))
    assert [e["model"] for e in entries] == [D.CAMERAS.get(k, ("SIMPLE_PINHOLE",))[0] for k in range(D.N_VIEWS)]
    os.makedirs(out)
    images = [read_image_gray(str(data / "images" / e["name"])) for e in entries]
    assert all(e["worldpoints"] for e in entries) and all(im.shape == (D.HEIGHT, D.WIDTH) for im in images)
    cm = [io.front_end_camera_model("colmap", e, D.WIDTH, D.HEIGHT) for e in entries]
    assert all(io.front_end_undistortion("colmap", e, D.WIDTH, D.HEIGHT) is None for e in entries)
    todo = [i for i, m in enumerate(cm) if m is not None]
    assert [entries[i]["id"] for i in todo] == sorted(D.CAMERAS)
    done = undistort_images_model([images[i] for i in todo], [cm[i][0] for i in todo], [cm[i][1] for i in todo], [cm[i][2] for i in todo])
    for i, im in zip(todo, done):
        assert im.shape == images[i].shape and not np.array_equal(im, images[i])
        images[i] = im
    g = Line3D(str(out), True, -1, 3000, True, True)
    for e, im in zip(entries, images):
        g.addImage(e["id"], im, e["K"], e["R"], e["t"], float(e["median_depth"]), e["worldpoints"])
    assert g.numImages() == D.N_VIEWS
    assert g.matchImages(2.5, 10.0, 10, 0.25, 10, -1.0)
    assert g.reconstruct3Dlines(VISIBILITY_T, False, -1.0, False)
    name = g.outputFilename()
    assert g.saveResultAsSTL(str(out)) and g.saveResultAsOBJ(str(out)) and g.save3DLinesAsTXT(str(out)) and g.save3DLinesAsBIN(str(out))
    g.close()
    return name


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    folder = tmp_path_factory.mktemp("front_end_dataset_models")
    D.write(folder)
    return folder


@pytest.fixture(scope="module")
def programs(data, tmp_path_factory):
    """the child processes, one after another: form of the model -> (result folder, stdout)"""
    out = {}
    for form in ("bin", "txt"):
        folder = tmp_path_factory.mktemp("out_" + form)
        out[form] = (folder, _child("colmap", _argv(data, form, folder)))
    return out


def test_binary_model_gives_the_longhand_pipelines_files(data, programs, tmp_path):
    folder, stdout = programs["bin"]
    got = _files(folder)
    name = _longhand(data, tmp_path / "longhand")
    assert sorted(got) == sorted(name + s for s in SUFFIXES)
    assert "seconds per stage: read " in stdout
    print(stdout[stdout.index("seconds per stage"):].splitlines()[0])
    want = _files(tmp_path / "longhand")
    for n in got:
        assert got[n] == want[n], f"{n} differs from the step-by-step pipeline's"


def test_text_form_of_the_model_gives_the_same_bytes(programs):
    assert _files(programs["txt"][0]) == _files(programs["bin"][0])


def test_result_is_a_reconstruction(programs):
    lines = _lines(programs["bin"][0])
    views = sorted({int(c) for L in lines for c, _ in L["residuals"]})
    print(f"colmap binary, fisheye / FOV cameras: {len(lines)} 3D lines, {sum(len(L['segments']) for L in lines)} 3D segments, "
          f"seen from views {views}")
    assert len(lines) > 0
    for L in lines:
        assert len(L["segments"]) >= 1 and len({int(c) for c, _ in L["residuals"]}) >= VISIBILITY_T
        assert all(0 <= int(c) < D.N_VIEWS for c, _ in L["residuals"])
