"""The scenes of tests/test_gpu_lsd_stages.py reach what they are for (CPU, the model of tests/lsd_model.py alone): ties in
the length order, segments on both sides of the length filter, every branch of refine and every exit of rect_improve,
defined gradients in the tiny images, and the geometry of the mixed batch.  A GPU comparison on a scene that misses its
branch would pass without testing it; these conditions are what makes it a test."""
import functools

import numpy as np
import pytest

from tests import lsd_model as M
from tests import lsd_scenes as S

F32 = np.float32
CASES = S.all_cases()


@functools.lru_cache(maxsize=None)
def model(name):
    img, mw = CASES[name]
    return M.stages(img, mw)


def final(name, max_segments=3000):
    st = model(name)
    rows, cols = st["gray"].shape
    return M.finish(st["raw"], rows, cols, st["upx"], st["upy"], max_segments)


def lengths(segs):
    """float32, as finish computes them"""
    dx, dy = segs[:, 0] - segs[:, 2], segs[:, 1] - segs[:, 3]
    return np.sqrt(dx * dx + dy * dy).astype(F32)


def upscaled_lengths(st):
    s = st["raw"].astype(F32).copy()
    s[:, [0, 2]] *= st["upx"]
    s[:, [1, 3]] *= st["upy"]
    return lengths(s)


def threshold(st):
    rows, cols = st["gray"].shape
    return F32(np.sqrt(F32(rows * rows) + F32(cols * cols)).astype(F32) * F32(0.005))


def test_stages_agree_with_detect():
    """stages() is detect() taken apart: the same final list, and its counters count what they say"""
    img, mw = CASES["tiles320"]
    assert np.array_equal(final("tiles320", 7), M.detect(img, mw, 7))
    img, mw = CASES["rings"]
    assert np.array_equal(final("rings"), M.detect(img, mw)) and np.array_equal(model("rings")["raw"], M.lsd(img))
    st = model("rings")
    w = st["walk"]
    assert st["seeds"] >= len(st["raw"]) > 0 and st["nfa_evals"] >= sum(w.improve_exits) >= len(st["raw"])
    assert w.regrown >= w.reduced and st["max_grad"] == float(st["mod"][st["deg"] != F32(M.NOTDEF)].max())


@pytest.mark.parametrize("name", S.TILES)
def test_tiles_have_tied_lengths(name):
    ln = lengths(final(name))
    _, counts = np.unique(ln, return_counts=True)
    assert int(counts[counts > 1].sum()) >= 1
    assert (np.diff(ln) <= 0).all()
    # a cap that cuts inside a run of equal lengths exists
    assert len([i for i in range(1, len(ln)) if ln[i - 1] == ln[i]]) >= 1


def test_downscaled_tiles_are_downscaled():
    st = model("tiles320")
    assert st["small"].shape == (150, 200) and st["upx"] == F32(1.6)


@pytest.mark.parametrize("name", ["bars", "bars_down"])
def test_bars_lie_on_both_sides_of_the_length_filter(name):
    st = model(name)
    ln, th = upscaled_lengths(st), threshold(st)
    assert abs(float(th) - 16.0) < 0.01
    assert int((ln > th).sum()) >= 1 and int((ln <= th).sum()) >= 1
    assert int(((ln > th) & (ln < th + F32(2))).sum()) >= 1
    assert int(((ln <= th) & (ln > th - F32(2))).sum()) >= 1
    assert len(final(name)) == int((ln > th).sum())


def test_one_bar_is_exactly_as_long_as_the_threshold():
    """the only input on which `length > min` and `length >= min` differ"""
    st = model("bars_on_threshold")
    ln, th = upscaled_lengths(st), threshold(st)
    assert int((ln == th).sum()) >= 1
    assert len(final("bars_on_threshold")) == int((ln > th).sum()) < int((ln >= th).sum())


def test_walk_scenes_reach_every_branch():
    walks = [model(name)["walk"] for name in S.walk_cases()]
    assert sum(w.regrown for w in walks) >= 1
    assert sum(w.reduced for w in walks) >= 1
    assert sum(w.refine_failed for w in walks) >= 1
    for k in range(6):
        assert sum(w.improve_exits[k] for w in walks) >= 1, f"rect_improve exit {k} is never taken"
    # the scenes named for a branch reach it themselves
    assert model("rings")["walk"].regrown >= 1 and model("rings")["walk"].reduced >= 1
    assert model("noise")["walk"].refine_failed >= 1


def test_tiny_images_have_defined_gradients():
    for (w, h, seed), img in zip(S.TINY, S.tiny_batch()):
        st = M.stages(img)
        defined = int((st["deg"] != F32(M.NOTDEF)).sum())
        assert st["deg"].shape == (M.resize_size(h, M.SCALE), M.resize_size(w, M.SCALE))
        if (w, h) == (2, 2):            # the one exception: kept as the image in which nothing is defined
            assert defined == 0 and st["max_grad"] == -1.0 and st["seeds"] == 0
        else:
            assert defined >= 1 and st["max_grad"] > 0 and st["seeds"] >= 1
    # widths below the blur's 7 taps reflect more than once
    assert any(M.reflect101(-3, w) != 3 for (w, h, s) in S.TINY) and M.reflect101(-3, 2) == 1 and M.reflect101(5, 3) == 1
    # the 0.8 resample's last destination index is clamped to source index n - 1 for an odd and for an even destination size
    clamped = set()
    for n in sorted({v for (w, h, s) in S.TINY for v in (w, h)}):
        sx, fx = M.resize_map(M.resize_size(n, M.SCALE), n, M.SCALE)
        if sx[-1] == n - 1 and fx[-1] == 0:
            clamped.add(M.resize_size(n, M.SCALE) % 2)
    assert clamped == {0, 1}
    assert max(w * h for (w, h, s) in S.TINY) > 256          # more than one 256-thread block in a row of 257


def test_mixed_batch_geometry():
    imgs = S.mixed_batch()
    sts = [M.stages(im, S.MIXED_WIDTH) for im in imgs]
    down = [st["small"].shape != st["gray"].shape for st in sts]
    assert down == [True, False, True, True, False, False]
    assert [im.ndim for im in imgs] == [2, 3, 2, 3, 2, 2]
    portrait = sts[2]
    assert portrait["gray"].shape == (301, 233) and portrait["small"].shape == (250, 194)
    assert portrait["upx"] != portrait["upy"]
    # an image hundreds of times smaller than its neighbour, in a grid sized by the largest
    assert imgs[0].size > 500 * imgs[4].size
    assert len(sts[5]["raw"]) == 0 and sts[5]["max_grad"] == -1.0
    assert all(len(M.finish(st["raw"], *st["gray"].shape, st["upx"], st["upy"])) >= 1 for st in sts[:4])
    # max_image_width = 3 on 400x300: 3x2, then 2x2 after the 0.8 resample, the smallest geometry accepted
    st = M.stages(imgs[0], 3)
    assert st["small"].shape == (2, 3) and st["deg"].shape == (2, 2) and len(st["raw"]) == 0
