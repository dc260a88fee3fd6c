"""CPU tests of `python -m line3dpp_amd.overlays`: its own three flags and the exit status of a wrong command line.  No
device call is made here; the program end to end is tests/test_gpu_overlays.py."""
import pytest

from line3dpp_amd import overlays


def test_overlays_split_args():
    assert overlays.split_args(["-m", "x.nvm", "--views=3,5", "--alpha", "128", "-o", "y"]) == (
        ["-m", "x.nvm", "-o", "y"], dict(views=[3, 5], thickness=1, alpha=128))
    assert overlays.split_args(["--thickness=3", "-i", "a b"]) == (["-i", "a b"], dict(views=None, thickness=3, alpha=255))
    with pytest.raises(ValueError):
        overlays.split_args(["--alpha"])
    with pytest.raises(ValueError):
        overlays.split_args(["--views", "1,x"])


def test_overlays_usage_errors(capsys):
    assert overlays.main([]) == 1 and overlays.main(["nosuch"]) == 1
    assert overlays.main(["vsfm", "--thickness"]) == 1
    assert "--views id,id,..." in capsys.readouterr().err
