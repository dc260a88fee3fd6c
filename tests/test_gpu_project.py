"""The 3D lines projected into cameras on the MI355X (k_project.hip, l3d_project.hip): the three stages
against the numpy model of tests/project_lines_model.py with tolerance 0 (past one scan tile and one grid: against its
array form, tests/project_lines_model_vec.py), the context forms on the golden scene against
the stateless forms and the model, the argument checks, and the C++ facade."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from line3dpp_amd.api import Line3D
from tests import project_lines_cases as Cs
from tests import project_lines_model as M
from tests import project_lines_model_vec as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The sanity property of the context forms: the condition (95 % visible) and the bound (twice the CPU median of 0.15255 px
# on the reference's own lines) are those of tests/project_lines_cases.py, which tests/test_project_reference.py
# recomputes on the CPU.  Measured on the MI355X, on the lines of the GPU pipeline: 100.0 % and 0.15255 px.
SANITY_CPU_MEDIAN_PX = Cs.SANITY_CPU_MEDIAN_PX
SANITY_MIN_VISIBLE = Cs.SANITY_MIN_VISIBLE
SANITY_MAX_MEDIAN_PX = Cs.SANITY_MAX_MEDIAN_PX


def same_records(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} records on the GPU, {len(want)} in the model"
    for name in M.RECORD_DTYPE.names:
        bad = np.flatnonzero(got[name] != want[name])
        assert len(bad) == 0, f"{what}: {name} differs in {len(bad)} records, first {bad[0]}: {got[name][bad[0]]!r} != {want[name][bad[0]]!r}"


# ---- stage 1 ----------------------------------------------------------------------------------------------------------
def test_stage1_equals_the_model():
    cams = Cs.stage1_cameras()
    P1, P2, line = Cs.stage1_segments()
    want = M.project_segments(cams, P1, P2, line)
    got = api.project_segments(cams, P1, P2, line)
    assert len(got) == 4
    for c in range(4):
        same_records(got[c], want[c], f"camera {c}")
    flags = np.concatenate([g["segment"] for g in got]) & ~np.uint32(M.SEGMENT_MASK)
    assert (flags == M.CLIPPED_NEAR).any() and (flags == M.CLIPPED_RECT).any() and (flags == 0).any()
    # another near plane moves the clipped ends; one camera at a time gives the same records
    want_near = M.project_segments(cams[:1], P1, P2, line, near=0.75)
    same_records(api.project_segments(cams[:1], P1, P2, line, near=0.75)[0], want_near[0], "near = 0.75")
    assert len(want_near[0]) != len(want[0]) or (want_near[0] != want[0]).any()
    for c in range(4):
        same_records(api.project_segments(cams[c:c + 1], P1, P2, line)[0], want[c], f"camera {c} alone")


def test_stage1_projection_that_is_not_finite_is_not_visible():
    """A K whose third row gives q.z = 0 makes every pixel coordinate NaN or infinite, and a near plane below float32's
    range makes the inverse depth of an end clipped there infinite after the rounding.  NaN passes every comparison of
    the clipping, so step 5 of the contract drops such a record: no camera hands a non-finite record to stage 2."""
    cams = Cs.stage1_cameras()
    P1, P2, line = Cs.stage1_segments()
    flat = dict(cams[0]); flat["K"] = np.array(cams[0]["K"], np.float64).copy(); flat["K"][2] = 0.0
    want = M.project_segments([flat, cams[1]], P1, P2, line)
    got = api.project_segments([flat, cams[1]], P1, P2, line)
    assert len(want[0]) == 0 and len(want[1]) > 50
    usual = M.project_segments(cams[:1], P1, P2, line)[0]
    want.append(M.project_segments(cams[:1], P1, P2, line, near=1e-45)[0])
    got.append(api.project_segments(cams[:1], P1, P2, line, near=1e-45)[0])
    clipped = int(((usual["segment"] & M.CLIPPED_NEAR) != 0).sum())
    assert 0 < len(usual) - len(want[2]) <= clipped         # (an end clipped at the rectangle as well interpolates a finite one)
    for c in range(3):
        same_records(got[c], want[c], f"case {c}")
        for name in ("x1", "y1", "x2", "y2", "inv_depth1", "inv_depth2"):
            assert np.isfinite(got[c][name]).all()


def test_stage1_empty_inputs():
    cams = Cs.stage1_cameras()
    P1, P2, line = Cs.stage1_segments()
    none = api.project_segments(cams, P1[:0], P2[:0], line[:0])
    assert len(none) == 4 and all(len(r) == 0 for r in none)
    assert api.project_segments([], P1, P2, line) == []
    L = _lib.load()
    counts = np.full(4, 77, np.uint32); n = C.c_uint64(99)
    assert L.l3d_project_segments(0, 4, api.camera_array(cams), 0, None, None, 1e-6, _lib.ptr(counts), None, 0, C.byref(n)) == 0
    assert n.value == 0 and not counts.any()


# ---- stage 2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(200, 75), (97, 61)])
@pytest.mark.parametrize("thickness", [1, 3])
def test_stage2_equals_the_model(width, height, thickness):
    rec = Cs.stage2_records(width, height, seed=width)
    cam = dict(K=np.eye(3), R=np.eye(3), t=np.zeros(3), width=width, height=height)
    want_id, want_iz = M.render_line_maps(rec, width, height, thickness)
    (got_id, got_iz), = api.render_line_maps([cam], [rec], thickness)
    assert got_id.dtype == np.int32 and got_iz.dtype == np.float32 and got_id.shape == (height, width)
    assert np.array_equal(got_id, want_id), f"{(got_id != want_id).sum()} pixels with another line"
    assert np.array_equal(got_iz.view(np.uint32), want_iz.view(np.uint32))
    if width == 200:
        assert (want_id == 11).sum() > 100                         # the long record spans several work items
    assert (want_id == 13).sum() == 0 and (want_id == 14).sum() == 0             # sub-pixel, zero length: nothing
    assert (want_id >= 0).sum() > 1500


def test_stage2_cameras_share_launches_and_order_does_not_matter():
    cams, recs = Cs.stage2_multi_camera()                          # (the fourth camera has no records)
    got = api.render_line_maps(cams, recs, 3)
    for k in range(4):
        want = M.render_line_maps(recs[k], cams[k]["width"], cams[k]["height"], 3)
        assert np.array_equal(got[k][0], want[0]) and np.array_equal(got[k][1], want[1]), f"camera {k}"
    assert (got[3][0] == -1).all() and not got[3][1].any()
    back = api.render_line_maps(cams[:1], [recs[0][::-1].copy()], 3)[0]
    assert np.array_equal(back[0], got[0][0]) and np.array_equal(back[1], got[0][1])


# ---- stage 3 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [255, 128])
def test_stage3_equals_the_model(alpha):
    rng = np.random.default_rng(11)
    ids = [M.render_line_maps(Cs.stage2_records(97, 61, 8), 97, 61, 3)[0], M.render_line_maps(Cs.stage2_records(200, 75, 9), 200, 75, 1)[0]]
    grey = rng.integers(0, 256, (61, 128), np.uint8)[:, :97]              # padded stride
    rgb = rng.integers(0, 256, (75, 211, 3), np.uint8)[:, :200]
    assert not grey.flags["C_CONTIGUOUS"] and not rgb.flags["C_CONTIGUOUS"]
    table = rng.integers(0, 256, (40, 3), np.uint8)                       # shorter than the lines: the rest take the palette
    for colors in (None, table):
        got = api.draw_line_maps([grey, rgb], ids, alpha, colors)
        for k, img in enumerate((grey, rgb)):
            want = M.draw_line_map(img, ids[k], alpha, colors)
            assert got[k].shape == want.shape and np.array_equal(got[k], want), f"image {k}, colors {'table' if colors is not None else 'palette'}"
    assert api.draw_line_maps([], [], alpha) == []


# ---- past one scan tile and one grid: the large cases against the array form of the model --------------------------------
# (tests/project_lines_model_vec.py, shown byte-identical to the loop model by tests/test_project_host.py)
@pytest.fixture(scope="module")
def large1():
    cams, P1, P2, line = Cs.stage1_large()
    return dict(cams=cams, P1=P1, P2=P2, line=line, want=V.project_segments(cams, P1, P2, line))


def test_stage1_large_crosses_scan_tiles_and_look_back_windows(large1):
    """70 cameras x 4001 segments: the flags fill 69 scan tiles, cameras begin inside tiles, three cameras see nothing."""
    G = large1
    cams, want = G["cams"], G["want"]
    counts = np.array([len(r) for r in want])
    flags = np.concatenate([r["segment"] for r in want]) & ~np.uint32(M.SEGMENT_MASK)
    n_flags = len(cams) * len(G["P1"])
    share = counts.sum() / n_flags
    print(f"stage1_large: {n_flags} flags = {-(-n_flags // 4096)} scan tiles, visible share {share:.4f}, records per non-empty camera "
          f"{counts[counts > 0].min()} .. {counts.max()}, clipped near {int(((flags & M.CLIPPED_NEAR) != 0).sum())}, "
          f"clipped at the rectangle {int(((flags & M.CLIPPED_RECT) != 0).sum())}")
    # conditions on the input
    assert n_flags > 65 * 4096 + 1 and len(G["P1"]) % 256 and len(G["P1"]) % 4096
    assert tuple(np.flatnonzero(counts == 0)) == Cs.STAGE1_LARGE_EMPTY
    assert 0.3 <= share <= 0.8
    assert counts[counts > 0].min() >= 500
    assert ((flags & M.CLIPPED_NEAR) != 0).any() and ((flags & M.CLIPPED_RECT) != 0).any()
    got = api.project_segments(cams, G["P1"], G["P2"], G["line"])
    assert [len(r) for r in got] == list(counts)
    for c in range(len(cams)):
        same_records(got[c], want[c], f"camera {c}")
    # grouping changes nothing; the slices begin with an empty camera, are one, and end with one
    for a, b in ((0, 23), (23, 24), (24, 70), (33, 34), (33, 36)):
        part = api.project_segments(cams[a:b], G["P1"], G["P2"], G["line"])
        assert sum(len(r) for r in part) == counts[a:b].sum(), f"cameras {a}:{b}: total"
        for c in range(a, b):
            same_records(part[c - a], want[c], f"camera {c} in the slice {a}:{b}")


@pytest.fixture(scope="module")
def large2():
    cams, recs = Cs.stage2_large()
    want = {t: [V.render_line_maps(recs[k], cams[k]["width"], cams[k]["height"], t) for k in range(3)] for t in (1, 3)}
    return dict(cams=cams, recs=recs, want=want)


def test_stage2_large_input_conditions(large2):
    cams, recs = large2["cams"], large2["recs"]
    w, h = cams[1]["width"], cams[1]["height"]
    count, _ = V.raster_steps(recs[1], w, h)
    zero = np.concatenate([[0], (count == 0).astype(np.int64), [0]])
    edges = np.flatnonzero(np.diff(zero))
    longest_run = int((edges[1::2] - edges[0::2]).max())
    pix, key = V.record_keys(recs[1], w, h, 1)
    winner = V.key_plane(recs[1], w, h, 1)[pix]
    tie = ((key >> np.uint64(32)) == (winner >> np.uint64(32))) & (key < winner)     # same depth, the larger line index lost
    print(f"stage2_large: {w * h} pixels, {len(recs[1])} records = {-(-len(recs[1]) // 4096)} scan tiles, {int(count.sum())} steps, "
          f"{int((count == 0).sum())} records without steps (longest run {longest_run}), longest record {int(count.max())} steps, "
          f"{len(np.unique(pix[tie]))} pixels with a tie in depth")
    assert len(recs[0]) == 0 and w * h > 524288 and len(recs[1]) > 4096
    assert count.sum() > 524288
    assert (count == 0).sum() >= 100 and longest_run >= 3 and count[0] == 0 and count[-1] == 0
    assert tie.any()
    assert (0xFFFFFFFF - (winner[tie] & np.uint64(0xFFFFFFFF)) < 0xFFFFFFFF - (key[tie] & np.uint64(0xFFFFFFFF))).all()


@pytest.mark.parametrize("thickness", [1, 3])
def test_stage2_large_strides_the_grid_and_starts_with_an_empty_camera(large2, thickness):
    cams, recs, want = large2["cams"], large2["recs"], large2["want"][thickness]
    got = api.render_line_maps(cams, recs, thickness)
    for k in range(3):
        assert np.array_equal(got[k][0], want[k][0]), f"camera {k}: {(got[k][0] != want[k][0]).sum()} pixels with another line"
        assert np.array_equal(got[k][1].view(np.uint32), want[k][1].view(np.uint32)), f"camera {k}: inverse depths"
    assert (got[0][0] == -1).all() and not got[0][1].view(np.uint32).any()
    assert (want[1][0] >= 0).sum() > 300000 and (want[2][0] >= 0).sum() > 1000
    back = api.render_line_maps(cams, [recs[0], recs[1][::-1].copy(), recs[2]], thickness)
    for k in range(3):
        assert np.array_equal(back[k][0], got[k][0]) and np.array_equal(back[k][1].view(np.uint32), got[k][1].view(np.uint32)), f"camera {k}: reversed"


def test_stage3_large_strides_the_grid(large2):
    ids = [w[0] for w in large2["want"][3]]
    rng = np.random.default_rng(12)
    imgs = [rng.integers(0, 256, (130, 64), np.uint8)[:, :33],                      # grey, padded stride
            rng.integers(0, 256, (500, 1111, 3), np.uint8)[:, :1100],              # RGB, padded stride
            rng.integers(0, 256, (61, 97), np.uint8)]                               # grey, contiguous
    assert not imgs[0].flags["C_CONTIGUOUS"] and not imgs[1].flags["C_CONTIGUOUS"] and imgs[2].flags["C_CONTIGUOUS"]
    table = rng.integers(0, 256, (40, 3), np.uint8)                                 # shorter than the ids: the rest take the palette
    assert max(int(p.max()) for p in ids) >= 40 and (ids[0] == -1).all()
    got = api.draw_line_maps(imgs, ids, 128, table)
    for k in range(3):
        want = V.draw_line_map(imgs[k], ids[k], 128, table)
        assert got[k].shape == want.shape and np.array_equal(got[k], want), f"image {k}"
    assert np.array_equal(got[0], np.repeat(imgs[0][:, :, None], 3, 2))


# ---- the context forms on the golden scene ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    from tests.golden.make_golden import golden_scene
    sc = golden_scene()
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages() and g.reconstruct3Dlines(3)
    lines = g.get3Dlines()
    cam_ids = [v.cam for v in sc.views]
    cams = [g.viewCamera(c) for c in cam_ids]
    P1 = np.concatenate([L["collinear3Dsegments"]["P1"] for L in lines])
    P2 = np.concatenate([L["collinear3Dsegments"]["P2"] for L in lines])
    line = np.concatenate([[i] * len(L["collinear3Dsegments"]) for i, L in enumerate(lines)]).astype(np.uint32)
    rec = g.projectLines(cam_ids)
    maps = g.renderLines(cam_ids)
    yield dict(sc=sc, g=g, lines=lines, cam_ids=cam_ids, cams=cams, P1=P1, P2=P2, line=line, rec=rec, maps=maps)
    g.close()


def test_context_view_camera_and_project_lines(golden):
    G = golden
    T = np.abs(G["g"].translation()).max()
    for v, cam in zip(G["sc"].views, G["cams"]):
        assert np.array_equal(cam["K"], v.K) and np.array_equal(cam["R"], v.R)
        assert (cam["width"], cam["height"]) == (v.width, v.height)
        # t is the view's own: matchImages moved the camera centre by the scene translation and back and formed
        # t = -R C again both times, as the reference's View::translate does -- a few roundings at the size of C and T
        t_in = np.asarray(v.t, np.float64).reshape(3)
        bound = 16 * np.finfo(np.float64).eps * (np.abs(v.R.T @ t_in).max() + T + np.abs(t_in).max())
        assert np.abs(cam["t"] - t_in).max() <= bound
    assert len(G["lines"]) > 20
    stateless = api.project_segments(G["cams"], G["P1"], G["P2"], G["line"])
    model = M.project_segments(G["cams"], G["P1"], G["P2"], G["line"])
    for k in range(len(G["cams"])):
        same_records(G["rec"][k], stateless[k], f"view {k}: context / stateless")
        same_records(G["rec"][k], model[k], f"view {k}: context / model")
    assert sum(len(r) for r in G["rec"]) > 0.9 * len(G["line"]) * len(G["cams"])


def test_context_sanity_of_the_residuals(golden):
    G = golden
    frac, median = Cs.residual_sanity(G["lines"], G["rec"], G["cam_ids"], {v.cam: v.segs for v in G["sc"].views})
    print(f"lines visible in their residuals' cameras: {100 * frac:.1f} %, median end point distance {median:.5f} px "
          f"(CPU, reference's lines: {SANITY_CPU_MEDIAN_PX} px)")
    assert frac >= SANITY_MIN_VISIBLE
    assert median < SANITY_MAX_MEDIAN_PX


def test_context_render_lines_and_groupings(golden):
    G = golden
    n = len(G["cams"])
    stateless = api.render_line_maps(G["cams"], G["rec"], 1)
    for k in range(n):
        want = M.render_line_maps(G["rec"][k], G["cams"][k]["width"], G["cams"][k]["height"], 1)
        assert np.array_equal(G["maps"][k][0], want[0]) and np.array_equal(G["maps"][k][1], want[1]), f"view {k}: model"
        assert np.array_equal(G["maps"][k][0], stateless[k][0]) and np.array_equal(G["maps"][k][1], stateless[k][1]), f"view {k}: stateless"
        assert (want[0] >= 0).sum() > 1000
    for k in range(n):                               # one at a time: the planes do not depend on the grouping
        (ids, iz), = G["g"].renderLines([G["cam_ids"][k]])
        assert np.array_equal(ids, G["maps"][k][0]) and np.array_equal(iz, G["maps"][k][1]), f"view {k} alone"


def test_context_small_budget_takes_stage1_in_several_groups(golden):
    """The default budget holds stage 1 of all ten views in one group (68 bytes per camera and segment) and the planes of
    four.  A budget of three cameras' records cuts stage 1 into four groups (3 + 3 + 3 + 1, appended with their offsets)
    and gives every view's planes a group of its own: records, planes and overlays stay what they were."""
    G = golden
    g, ids = G["g"], G["cam_ids"]
    assert len(ids) == 10
    rng = np.random.default_rng(8)
    imgs = [rng.integers(0, 256, (c["height"], c["width"]), np.uint8) for c in G["cams"][:5]]
    drawn = g.drawLines(ids[:5], imgs, 3, 200)
    g.set_projection_budget(68 * len(G["line"]) * 3 + 67)
    try:
        rec = g.projectLines(ids)
        maps = g.renderLines(ids)
        small = g.drawLines(ids[:5], imgs, 3, 200)
    finally:
        g.set_projection_budget(0)
    for k in range(10):
        same_records(rec[k], G["rec"][k], f"view {k}: small budget")
        assert np.array_equal(maps[k][0], G["maps"][k][0]) and np.array_equal(maps[k][1], G["maps"][k][1]), f"view {k}: small budget"
    for k in range(5):
        assert np.array_equal(small[k], drawn[k]), f"overlay {k}: small budget"


def test_context_draw_lines(golden):
    G = golden
    rng = np.random.default_rng(5)
    w, h = G["cams"][0]["width"], G["cams"][0]["height"]
    pick = [0, 4]
    imgs = [rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 256, (h, w + 5, 3), np.uint8)[:, :w]]
    colors = rng.integers(0, 256, (len(G["lines"]), 3), np.uint8)
    for thickness, alpha, col in ((1, 255, None), (3, 128, colors)):
        got = G["g"].drawLines([G["cam_ids"][k] for k in pick], imgs, thickness, alpha, col)
        maps = G["g"].renderLines([G["cam_ids"][k] for k in pick], thickness)
        stateless = api.draw_line_maps(imgs, [m[0] for m in maps], alpha, col)
        for i, k in enumerate(pick):
            ids = M.render_line_maps(G["rec"][k], w, h, thickness)[0]
            assert np.array_equal(maps[i][0], ids)
            assert np.array_equal(got[i], stateless[i]), f"view {k}: stateless"
            assert np.array_equal(got[i], M.draw_line_map(imgs[i], ids, alpha, col)), f"view {k}: model"


def test_context_camera_that_was_not_added(golden):
    G = golden
    centres = np.array([-c["R"].T @ c["t"] for c in G["cams"]])
    radius = np.linalg.norm(centres - centres.mean(0), axis=1).mean()
    cam = dict(G["cams"][2])
    cam["t"] = cam["t"] - np.array([0.1 * radius, 0, 0])       # the centre moves sideways along the camera's x axis
    cam["width"], cam["height"] = 641, 479
    cam["K"] = cam["K"].copy(); cam["K"][:2] *= 641 / G["cams"][2]["width"]
    rec = G["g"].projectLines([cam, G["cam_ids"][2]])
    want = M.project_segments([cam], G["P1"], G["P2"], G["line"])[0]
    same_records(rec[0], want, "new camera")
    same_records(rec[1], G["rec"][2], "added view beside it")
    assert len(want) > 10 and not np.array_equal(want["x1"][:10], G["rec"][2]["x1"][:10])
    (ids, iz), = G["g"].renderLines([cam], 3)
    wid, wiz = M.render_line_maps(want, 641, 479, 3)
    assert np.array_equal(ids, wid) and np.array_equal(iz, wiz)


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(golden):
    L = _lib.load()
    G = golden
    cams = Cs.stage1_cameras()
    P1, P2, line = Cs.stage1_segments()
    segs = np.zeros(len(P1), _lib.SEGMENT3D_DTYPE); segs["P1"] = P1; segs["P2"] = P2
    p = _lib.ptr

    def project(cam_list, near, segs=segs, line=line, counts_ok=True):
        counts = np.full(len(cam_list), 77, np.uint32); n = C.c_uint64(99)
        out = np.full(4000, 0x5A5A5A5A, np.uint32).view(_lib.PROJECTED_SEGMENT_DTYPE)
        rc = L.l3d_project_segments(0, len(cam_list), api.camera_array(cam_list), len(segs), p(segs), p(line), near,
                                    p(counts) if counts_ok else None, p(out), len(out), C.byref(n))
        assert (counts == 77).all() and n.value == 99 and (out.view(np.uint32) == 0x5A5A5A5A).all()
        return rc, _lib.last_error()

    for near in (0.0, -1.0, float("inf"), float("nan")):
        rc, msg = project(cams, near)
        assert rc == -1 and "near plane" in msg
    bad = dict(cams[1]); bad["width"] = 0
    assert project([cams[0], bad], 1e-6)[0] == -1
    bad = dict(cams[1]); bad["R"] = cams[1]["R"].copy(); bad["R"][1, 1] = np.nan
    rc, msg = project([cams[0], bad], 1e-6)
    assert rc == -1 and "non-finite" in msg
    bad = dict(cams[1]); bad["t"] = np.array([0, np.inf, 0])
    assert project([bad], 1e-6)[0] == -1
    nan_segs = segs.copy(); nan_segs["P2"][5, 1] = np.nan
    assert project(cams, 1e-6, segs=nan_segs)[0] == -1
    assert project(cams, 1e-6, counts_ok=False)[0] == -1
    # stage 2: an even or zero thickness, a null plane
    cam = dict(K=np.eye(3), R=np.eye(3), t=np.zeros(3), width=40, height=30)
    rec = Cs.stage2_records(40, 30, 1)[:5]
    cnt = np.array([5], np.uint32)
    ids = np.full((30, 40), 1234, np.int32); iz = np.full((30, 40), 5.5, np.float32)
    for thickness in (0, 2, 4):
        rc = L.l3d_render_line_maps(0, 1, api.camera_array([cam]), p(cnt), p(rec), thickness, api.pointer_array([ids]), api.pointer_array([iz]))
        assert rc == -1 and "thickness" in _lib.last_error()
    assert L.l3d_render_line_maps(0, 1, api.camera_array([cam]), p(cnt), p(rec), 1, None, api.pointer_array([iz])) == -1
    bad_rec = rec.copy(); bad_rec["y2"][3] = np.inf
    assert L.l3d_render_line_maps(0, 1, api.camera_array([cam]), p(cnt), p(bad_rec), 1, api.pointer_array([ids]), api.pointer_array([iz])) == -1
    assert (ids == 1234).all() and (iz == 5.5).all()
    # stage 3: alpha, a null image
    img = np.zeros((30, 40), np.uint8); out = np.full((30, 40, 3), 9, np.uint8)
    imgs, keep = api.lsd.image_array([img])
    plane = np.zeros((30, 40), np.int32)
    assert L.l3d_draw_line_maps(0, 1, imgs, api.pointer_array([plane]), 0, None, 256, api.pointer_array([out])) == -1
    assert "alpha" in _lib.last_error()
    assert L.l3d_draw_line_maps(0, 1, imgs, None, 0, None, 255, api.pointer_array([out])) == -1
    two_ch = _lib.Image(img.ctypes.data, 20, 30, 2, 40)
    assert L.l3d_draw_line_maps(0, 1, C.byref(two_ch), api.pointer_array([plane]), 0, None, 255, api.pointer_array([out])) == -1
    assert (out == 9).all()
    # the context forms: the same checks, and an image that is not of its camera's size
    g = G["g"]
    w, h = G["cams"][0]["width"], G["cams"][0]["height"]
    arr = api.camera_array(G["cams"][:1])
    small = np.zeros((h - 1, w), np.uint8); big_out = np.full((8, 8, 3), 9, np.uint8)
    imgs, keep = api.lsd.image_array([small])
    rc = L.l3d_draw_lines(g.h, 1, arr, imgs, 1e-6, 1, 255, None, api.pointer_array([big_out]))
    assert rc == -1 and "its camera" in _lib.last_error() and (big_out == 9).all()
    counts = np.full(1, 77, np.uint32)
    assert L.l3d_project_lines(g.h, 1, arr, 0.0, p(counts)) == -1 and counts[0] == 77
    assert L.l3d_render_lines(g.h, 1, arr, 1e-6, 2, api.pointer_array([ids]), None) == -1
    assert L.l3d_draw_lines(g.h, 1, arr, imgs, 1e-6, 1, 300, None, api.pointer_array([big_out])) == -1
    assert g.drawLines([G["cam_ids"][0]], [small]) is None and g.last_status == -1     # printed, None
    assert g.viewCamera(12345) is None


def test_context_forms_before_reconstruct3Dlines_return_the_state_error():
    from line3dpp_amd.scene import make_scene
    sc = make_scene(4, 60, n_neighbors=2, seed=2)
    g = Line3D()
    g.add_scene(sc)
    cam = g.viewCamera(sc.views[0].cam)
    assert cam is not None
    assert g.projectLines([sc.views[0].cam]) is None and g.last_status == -7
    assert "no 3D lines" in _lib.last_error()
    assert g.renderLines([cam]) is None and g.last_status == -7
    assert g.drawLines([cam], [np.zeros((cam["height"], cam["width"]), np.uint8)]) is None and g.last_status == -7
    g.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_project_and_draw(tmp_path):
    from line3dpp_amd.scene import make_scene
    exe = str(tmp_path / "project_facade")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "project_facade.cpp"), "-o", exe, "-L" + lib_dir,
                           "-ll3dpp_hip", "-Wl,-rpath," + lib_dir])
    sc = make_scene(8, 300, n_neighbors=4, seed=1)
    path = str(tmp_path / "scene.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", sc.n_views))
        for v in sc.views:
            f.write(struct.pack("<5I", v.cam, len(v.segs), v.width, v.height, len(v.neighbors)))
            f.write(np.ascontiguousarray(v.K, np.float64).tobytes()); f.write(np.ascontiguousarray(v.R, np.float64).tobytes())
            f.write(np.ascontiguousarray(v.t, np.float64).tobytes()); f.write(struct.pack("<f", v.median_depth))
            f.write(np.asarray(v.neighbors, np.uint32).tobytes()); f.write(np.ascontiguousarray(v.segs, np.float32).tobytes())
    w, h = sc.views[0].width, sc.views[0].height
    rng = np.random.default_rng(3)
    grey = rng.integers(0, 256, (h, w), np.uint8); rgb = rng.integers(0, 256, (h, w, 3), np.uint8)
    grey.tofile(str(tmp_path / "grey.raw")); rgb.tofile(str(tmp_path / "rgb.raw"))
    out_path = str(tmp_path / "out.bin")
    run = subprocess.run([exe, path, str(tmp_path / "grey.raw"), str(tmp_path / "rgb.raw"), out_path], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.count("[L3D++] ERROR:") == 2 and "no 3D lines" in run.stdout     # the two calls before the reconstruction
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages() and g.reconstruct3Dlines(3)
    c0, c1 = sc.views[0].cam, sc.views[1].cam
    rec = g.projectLines([c0, g.viewCamera(c1)])
    raw = open(out_path, "rb").read()
    n0, n1 = struct.unpack_from("<2I", raw, 0)
    assert (n0, n1) == (len(rec[0]), len(rec[1])) and n0 > 10
    pos = 8
    for r in rec:
        got = np.frombuffer(raw, _lib.PROJECTED_SEGMENT_DTYPE, len(r), pos)
        pos += 32 * len(r)
        assert np.array_equal(got, r)
    want = [g.drawLines([c0], [grey])[0], g.drawLines([c1], [rgb], 3, 128)[0]]
    for k in range(2):
        got = np.frombuffer(raw, np.uint8, 3 * w * h, pos).reshape(h, w, 3)
        pos += 3 * w * h
        assert np.array_equal(got, want[k]), f"overlay {k}: the facade's bytes differ from the Python front end's"
        assert not np.array_equal(got, np.repeat(grey[:, :, None], 3, 2) if k == 0 else rgb)
    assert pos == len(raw)
    g.close()
