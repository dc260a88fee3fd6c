"""Line-segment detection on the MI355X stage by stage (k_lsd.hip through l3d_debug_lsd_stages, the hook that runs the
detection's own launch and copies the stage maps out): every per-pixel map, the raw list in detection order and the
statistics against tests/lsd_model.py, at small and awkward sizes and in mixed batches; the host's length filter, tie
order and cap; padded rows; the argument checks of l3d_detect_segments.  Every comparison is exact: the stages use
only + * / sqrt and the float polynomial, and the library is built with -ffp-contract=off.
tests/test_lsd_cases.py shows on the CPU that each scene reaches what it is here for."""
import ctypes as C
import functools

import numpy as np
import pytest

from line3dpp_amd import _lib
from line3dpp_amd.lsd import as_image, detect_line_segments, fetch, image_array, last_stats, lsd_stages
from tests import lsd_model as M
from tests import lsd_scenes as S

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = S.all_cases()


@functools.lru_cache(maxsize=None)
def model(name):
    """the model's stages of a named case, computed once"""
    img, mw = CASES[name]
    return M.stages(img, mw)


def model_final(st, max_segments=3000):
    rows, cols = st["gray"].shape
    return M.finish(st["raw"], rows, cols, st["upx"], st["upy"], max_segments)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {got.size} differ, first at {tuple(bad[0])}: "
                           f"{got[tuple(bad[0])]!r} on the GPU, {want[tuple(bad[0])]!r} in the model")


def check_stages(got, want, what):
    """one image: the five maps, the raw list in detection order and the walk's statistics, GPU hook vs model"""
    for k in ("gray", "small", "blur", "deg", "mod"):
        same_bits(got[k], want[k], f"{what}: {k}")
    same_bits(got["raw"], want["raw"].astype(F32).reshape(-1, 4), f"{what}: raw segments")
    assert got["overflow"] == 0
    assert got["raw_segments"] == len(want["raw"]) == got["stats"]["raw_segments"], f"{what}: raw count"
    assert got["seeds"] == want["seeds"] == got["stats"]["seeds"], f"{what}: seeds {got['seeds']} vs {want['seeds']}"
    assert got["nfa_evals"] == want["nfa_evals"] == got["stats"]["nfa_evals"], \
        f"{what}: nfa_evals {got['nfa_evals']} vs {want['nfa_evals']}"
    same_bits(np.float64(got["stats"]["max_grad"]), np.float64(want["max_grad"]), f"{what}: max_grad")
    if want["max_grad"] < 0:
        assert got["max_grad_bits"] == 0
    else:
        assert got["max_grad_bits"] == int(np.float64(want["max_grad"]).view(np.uint64))
    gh, gw = want["small"].shape
    assert (got["stats"]["width"], got["stats"]["height"]) == (gw, gh), f"{what}: reported size"
    assert got["down"] == int(want["small"].shape != want["gray"].shape)


def check_stats(st, want, what):
    """l3d_detect_stats of the detection entry against the model's counts"""
    gh, gw = want["small"].shape
    assert (st["width"], st["height"]) == (gw, gh), what
    assert st["raw_segments"] == len(want["raw"]), f"{what}: raw {st['raw_segments']} vs {len(want['raw'])}"
    assert st["seeds"] == want["seeds"] and st["nfa_evals"] == want["nfa_evals"], what
    same_bits(np.float64(st["max_grad"]), np.float64(want["max_grad"]), f"{what}: max_grad")
    assert st["from_cache"] == 0


# ---- per-pixel stages ------------------------------------------------------------------------------------------------
def test_stages_at_small_and_awkward_sizes():
    """one batch: widths below the blur's 7 taps (more than one reflection), one row or column of gradient, rows longer
    than a 256-thread block, the resample's clamp at the last column for odd and even sizes; 2x2 has nothing defined"""
    imgs = S.tiny_batch()
    got = lsd_stages(imgs)
    assert len(got) == len(imgs)
    for k, (img, g) in enumerate(zip(imgs, got)):
        want = M.stages(img)
        check_stages(g, want, f"image {k} ({img.shape[1]}x{img.shape[0]})")
        assert g["small"].tobytes() == g["gray"].tobytes() == np.ascontiguousarray(img).tobytes()
    assert got[0]["stats"]["max_grad"] == -1.0 and got[0]["seeds"] == 0 and (got[0]["deg"] == F32(M.NOTDEF)).all()
    assert all(g["stats"]["max_grad"] > 0 for g in got[1:])
    # the detection entry reports the same statistics and no segment that the model does not have
    segs, stats = detect_line_segments(imgs, stats=True)
    for k, img in enumerate(imgs):
        want = M.stages(img)
        check_stats(stats[k], want, f"image {k}")
        same_bits(segs[k], model_final(want), f"image {k}: segments")


def test_stages_of_a_mixed_batch_with_downscale_and_colour():
    imgs = S.mixed_batch()
    wants = [M.stages(im, S.MIXED_WIDTH) for im in imgs]
    got = lsd_stages(imgs, max_image_width=S.MIXED_WIDTH)
    segs, stats = detect_line_segments(imgs, max_image_width=S.MIXED_WIDTH, stats=True)
    for k, (img, g, want) in enumerate(zip(imgs, got, wants)):
        check_stages(g, want, f"image {k}")
        check_stats(stats[k], want, f"image {k}")
        same_bits(segs[k], model_final(want), f"image {k}: segments")
        assert stats[k]["segments"] == len(segs[k])
        alone = detect_line_segments([img], max_image_width=S.MIXED_WIDTH)[0]
        assert alone.tobytes() == segs[k].tobytes(), f"image {k}: in the batch and alone"
    assert [g["down"] for g in got] == [1, 0, 1, 1, 0, 0]
    assert got[1]["small"].tobytes() == got[1]["gray"].tobytes()
    assert all(len(s) > 0 for s in segs[:4]) and len(segs[4]) == 0 and len(segs[5]) == 0
    # the batch in another order: the grid is sized by the largest image wherever it stands
    order = [4, 5, 1, 3, 2, 0]
    again = lsd_stages([imgs[i] for i in order], max_image_width=S.MIXED_WIDTH)
    for j, i in enumerate(order):
        check_stages(again[j], wants[i], f"image {i} at place {j}")
    # 400x300 under max_image_width = 3: 3x2, then 2x2 after the 0.8 resample, the smallest geometry accepted
    want = M.stages(imgs[0], 3)
    g = lsd_stages([imgs[0]], max_image_width=3)[0]
    check_stages(g, want, "max_image_width = 3")
    assert g["small"].shape == (2, 3) and g["deg"].shape == (2, 2)
    segs3, stats3 = detect_line_segments([imgs[0]], max_image_width=3, stats=True)
    assert len(segs3[0]) == 0 and stats3[0]["raw_segments"] == 0 and (stats3[0]["width"], stats3[0]["height"]) == (3, 2)


# ---- the walk: raw list in detection order, statistics ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.walk_cases()))
def test_raw_list_and_statistics_of_the_walk(name):
    img, mw = CASES[name]
    want = model(name)
    g = lsd_stages([img], max_image_width=mw)[0]
    assert len(want["raw"]) > 0 or img.shape[1] < 100
    check_stages(g, want, name)
    segs, stats = detect_line_segments([img], max_image_width=mw, stats=True)
    check_stats(stats[0], want, name)
    same_bits(segs[0], model_final(want), f"{name}: segments")


# ---- the host's filter, order and cap --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.BARS))
def test_length_filter_keeps_what_the_model_keeps(name):
    img, mw = CASES[name]
    want = model(name)
    segs, stats = detect_line_segments([img], max_image_width=mw, stats=True)
    same_bits(segs[0], model_final(want), name)
    assert stats[0]["raw_segments"] > stats[0]["segments"] > 0
    check_stats(stats[0], want, name)


@pytest.mark.parametrize("name", S.TILES)
def test_tied_lengths_pop_in_the_model_order_and_the_cap_cuts_inside_a_tie(name):
    img, mw = CASES[name]
    want = model_final(model(name))
    dx, dy = want[:, 0] - want[:, 2], want[:, 1] - want[:, 3]
    ln = np.sqrt(dx * dx + dy * dy).astype(F32)
    inside = [i for i in range(1, len(ln)) if ln[i - 1] == ln[i]]
    assert inside, "no tied lengths in the model's output"
    same_bits(detect_line_segments([img], max_image_width=mw)[0], want, name)
    for cap in (inside[0], inside[len(inside) // 2]):
        got = detect_line_segments([img], max_image_width=mw, max_segments=cap)[0]
        same_bits(got, model_final(model(name), cap), f"{name}: cap {cap}")
        assert len(got) == cap
    got, stats = detect_line_segments([img], max_image_width=mw, max_segments=0, stats=True)
    assert got[0].shape == (0, 4) and stats[0]["segments"] == 0 and stats[0]["raw_segments"] == len(model(name)["raw"])


# ---- padded rows -----------------------------------------------------------------------------------------------------
def test_padded_rows_equal_their_packed_copies():
    w, h = 161, 97
    grey, rgb = S.polygons(w, h, 21), S.polygons(w, h, 22, rgb=True)
    big = np.full((h, w + 37), 255, np.uint8)
    big[:, :w] = grey
    big_rgb = np.full((h, w + 5, 3), 255, np.uint8)
    big_rgb[:, :w] = rgb
    views = [big[:, :w], big_rgb[:, :w]]
    assert as_image(views[0])[0].row_stride == w + 37 > w
    assert as_image(views[1])[0].row_stride == 3 * (w + 5) > 3 * w and as_image(views[1])[0].channels == 3
    padded = detect_line_segments(views)
    packed = detect_line_segments([grey, rgb])
    maps = lsd_stages(views)
    for k, img in enumerate((grey, rgb)):
        want = M.stages(img)
        assert len(want["raw"]) > 0
        assert padded[k].tobytes() == packed[k].tobytes()
        same_bits(padded[k], model_final(want), f"padded image {k}")
        check_stages(maps[k], want, f"padded image {k}")


# ---- the arguments of l3d_detect_segments ----------------------------------------------------------------------------
L3D_ERR_ARG, L3D_ERR_LIMIT = -1, -9


def test_bad_arguments_fail_and_leave_the_last_detection():
    L = _lib.load()
    good = [S.polygons(97, 131, 2), S.polygons(64, 48, 0)]
    h = C.c_void_p(L.l3d_create(0, None))
    try:
        arr, keep = image_array(good)
        counts = np.zeros(2, np.uint32)
        assert L.l3d_detect_segments(h, 2, arr, -1, 3000, _lib.ptr(counts)) == 0
        before, before_stats = fetch(L, h, counts), last_stats(L, h)
        assert len(before[0]) > 0 and len(before_stats) == 2

        def refused(images, max_image_width, code, text):
            a = (_lib.Image * len(images))(*images)
            c = np.full(len(images), 77, np.uint32)
            rc = L.l3d_detect_segments(h, len(images), a, max_image_width, 3000, _lib.ptr(c))
            assert rc == code and text in _lib.last_error(), (rc, _lib.last_error())
            assert (c == 77).all()
            after = fetch(L, h, counts)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after)) and last_stats(L, h) == before_stats
            # the stage hook makes the same checks
            st = (_lib.LsdStages * len(images))()
            assert L.l3d_debug_lsd_stages(h, len(images), a, max_image_width, 1, st) == code and text in _lib.last_error()

        buf = np.zeros((48, 128), np.uint8)
        ok = as_image(good[1])[0]
        refused([_lib.Image(buf.ctypes.data, 64, 48, 2, 128)], -1, L3D_ERR_ARG, "not supported")
        refused([_lib.Image(buf.ctypes.data, 64, 48, 1, 63)], -1, L3D_ERR_ARG, "row stride")
        refused([_lib.Image(buf.ctypes.data, 42, 48, 3, 125)], -1, L3D_ERR_ARG, "row stride")
        refused([_lib.Image(buf.ctypes.data, 1, 48, 1, 128)], -1, L3D_ERR_ARG, "empty image")
        refused([_lib.Image(None, 64, 48, 1, 128)], -1, L3D_ERR_ARG, "empty image")
        big, _ = as_image(S.polygons(400, 300, 8))
        refused([big], 2, L3D_ERR_ARG, "too small for line-segment detection")
        # 30000 x 30000 x 3 >= 2^31 claimed over 6 kB: refused before a pixel is read, also behind good images
        huge = _lib.Image(buf.ctypes.data, 30000, 30000, 1, 30000)
        assert 30000 * 30000 * 3 >= 2 ** 31
        refused([huge], -1, L3D_ERR_LIMIT, "2^31")
        refused([ok, ok, huge], -1, L3D_ERR_LIMIT, "2^31")
        # one bad image in a batch of good ones fails the whole call
        refused([ok, _lib.Image(buf.ctypes.data, 64, 48, 2, 128), ok], -1, L3D_ERR_ARG, "not supported")
        refused([big, ok], 2, L3D_ERR_ARG, "too small")
        # the hook leaves the last detection too
        st = (_lib.LsdStages * 2)()
        assert L.l3d_debug_lsd_stages(h, 2, arr, -1, 0, st) == 0 and st[0].raw_segments == before_stats[0]["raw_segments"]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before, fetch(L, h, counts)))
        assert last_stats(L, h) == before_stats
        # no image: success, and the last detection is now the empty one
        assert L.l3d_detect_segments(h, 0, None, -1, 3000, None) == 0
        n = C.c_uint64(5)
        assert L.l3d_get_detected_segments(h, None, 0, C.byref(n)) == 0 and n.value == 0
        assert last_stats(L, h) == []
        assert L.l3d_debug_lsd_stages(h, 0, None, -1, 0, None) == 0
    finally:
        L.l3d_destroy(h)
    assert detect_line_segments([]) == []
