"""`python -m line3dpp_amd.overlays` end to end on the MI355X: the rendered dataset of tests/front_end_dataset.py in .nvm
form goes through the program as a child process; it leaves the front end's four result files, byte for byte, and one
PNG per selected view, which equal Line3D.drawLines on the same pipeline's object and images."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import front_end_dataset as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120            # tests/test_gpu_front_end.py: such a child takes about a second


def _child(module, args):
    cmd = [sys.executable, "-m", module] + args
    try:
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{module} did not finish within {CHILD_TIMEOUT_S} s: nothing more is started on this GPU", 3)
    if run.returncode < 0:
        pytest.exit(f"{module} died by signal {-run.returncode}: nothing more is started on this GPU\n{run.stderr[-2000:]}", 3)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout


def _files(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder)) if os.path.isfile(os.path.join(folder, n))}


def test_overlays_program(tmp_path):
    from PIL import Image
    from line3dpp_amd import front_end, overlays
    data = tmp_path / "data"
    data.mkdir()
    D.write(data)
    args = ["-m", str(data / "model.nvm")]
    out = _child("line3dpp_amd.overlays", ["vsfm"] + args + ["-o", str(tmp_path / "out"), "--views", "1,4", "--thickness", "3"])
    assert "2 overlays written" in out
    # exactly two PNGs of the image size
    assert sorted(os.listdir(tmp_path / "out" / "overlays")) == ["1.png", "4.png"]
    pngs = {c: np.asarray(Image.open(tmp_path / "out" / "overlays" / f"{c}.png")) for c in (1, 4)}
    assert all(p.shape == (D.HEIGHT, D.WIDTH, 3) and p.dtype == np.uint8 for p in pngs.values())
    # the four result files are those of the front end on the same arguments: the program adds files and changes none
    _child("line3dpp_amd.front_end", ["vsfm"] + args + ["-o", str(tmp_path / "plain")])
    got, want = _files(tmp_path / "out"), _files(tmp_path / "plain")
    assert len(want) == 4 and sorted(got) == sorted(want)
    for n in want:
        assert got[n] == want[n], f"{n} differs from the front end's"
    # each PNG is drawLines on the same pipeline's Line3D object and the images it was handed (undistorted: 1 and 4 are
    # the dataset's two distorted views)
    line3d, _ = front_end.run_vsfm(args + ["-o", str(tmp_path / "here")], line3d_factory=overlays.keeping_line3d({1, 4}))
    assert sorted(line3d.kept) == [1, 4]
    drawn = line3d.drawLines([1, 4], [line3d.kept[1], line3d.kept[4]], thickness=3)
    plain = line3d.drawLines([1, 4], [line3d.kept[1], line3d.kept[4]], thickness=1)
    for k, c in enumerate((1, 4)):
        assert np.array_equal(pngs[c], drawn[k]), f"{c}.png is not drawLines' image"
        grey = np.repeat(line3d.kept[c][:, :, None], 3, 2)
        assert (drawn[k] != grey).any(2).sum() > (plain[k] != grey).any(2).sum() > 500      # lines were drawn, thicker
    assert _files(tmp_path / "here") == want
    line3d.close()

