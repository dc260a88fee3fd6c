"""Who holds device and pinned memory (l3d_host.h): the buffers of the library own their blocks, so a context gives back
everything it took when it is closed -- also one that is closed half way through a split call or after a detection --
and a stateless entry holds nothing once it has returned, whether it succeeded or refused its arguments.  Seen through
the two counters l3d_debug_counter("live_device_blocks") / ("live_pinned_blocks"): blocks held by buffers right now;
blocks lying in the process-wide cache are not counted."""
import ctypes as C
import gc

import numpy as np
import pytest

from line3dpp_amd import _lib, api, lsd
from line3dpp_amd._lib import ptr
from line3dpp_amd.api import Line3D
from line3dpp_amd.scene import make_scene
from tests import line_opt_model as LM
from tests import project_lines_cases as Cs
from tests import line_opt_cases, scan_cases, seam_cases
from tests import triangulate_model as TM
from tests.lsd_scenes import polygons

pytestmark = pytest.mark.gpu

L3D_ERR_LIMIT = -9


def live():
    """(device blocks, pinned blocks) held by the library's buffers"""
    L = _lib.load()
    out = (L.l3d_debug_counter(b"live_device_blocks"), L.l3d_debug_counter(b"live_pinned_blocks"))
    assert all(v != 2**64 - 1 for v in out), "l3d_debug_counter does not know the live-block counters"
    return out


def baseline():
    gc.collect()          # a Line3D of an earlier test may still await collection
    return live()


def settled():
    gc.collect()
    return live()


def scene():
    return make_scene(6, 300, n_neighbors=4, seed=1)


def whole_pipeline(g, sc):
    """bounded kNN, the ragged keep-all buffers, diffusion + collinear links + line bundling, the projection stages"""
    assert g.matchImages(kNN=10)
    assert g.matchImages(kNN=0)
    assert g.reconstruct3Dlines(3, True, 2.0, True)
    cams = [sc.views[0].cam, sc.views[1].cam]
    assert g.projectLines(cams) is not None
    assert g.renderLines(cams) is not None
    images = [np.full((v.height, v.width), 128, np.uint8) for v in sc.views[:2]]
    assert g.drawLines(cams, images) is not None


def split_call_left_open(g, sc):
    assert g.matchBegin()
    assert g.matchPairs(0, 1)          # closed between l3d_match_begin and l3d_match_finish


def detected_view_then_whole_pipeline(g, sc):
    """one more view through addImage with an 800 x 600 image and no segments (the detection arena), then the same calls"""
    K = np.array([[800, 0, 400], [0, 800, 300], [0, 0, 1]], np.float64)
    g.addImage(1000, polygons(800, 600, 11), K, np.eye(3), np.zeros(3), 1.0, [sc.views[0].cam])
    assert g.last_status == 0 and g._M[1000] > 0
    whole_pipeline(g, sc)


@pytest.mark.parametrize("use", [whole_pipeline, split_call_left_open, detected_view_then_whole_pipeline],
                         ids=["whole_pipeline", "closed_inside_a_split_call", "view_from_an_image"])
def test_a_context_gives_everything_back(use):
    sc = scene()
    base = baseline()
    g = Line3D()
    g.add_scene(sc)
    use(g, sc)
    held = live()
    assert held[0] > base[0] and held[1] > base[1], (base, held)
    g.close()
    assert settled() == base


def _diffuse():
    e = seam_cases.symmetric_edges(np.random.default_rng(3), 3, [(0, 1), (1, 2)])
    assert len(e) == 4 and len(api.diffuse_affinity(e, 3)) == 4


def _collinear():
    off, idx = api.find_collinear_segments(scene().views[0].segs[:64], 2.0)
    assert len(off) == 65


def _score():
    c = seam_cases.score_single_case()
    v = c.view
    out = api.score_matches(c.segs, c.matches4, c.ranges2, c.reg_tgt2, c.RtKinv, -v.R.T @ v.t, seam_cases.TWO_SIGA_SQR, c.k)
    assert len(out) == len(c.matches4)


def _pair_arguments(vs, vt):
    R = vt.R @ vs.R.T                             # Line3D::getFundamentalMatrix, line3D.cc:874-892
    tt = vt.t - R @ vs.t
    T = np.array([[0, -tt[2], tt[1]], [tt[2], 0, -tt[0]], [-tt[1], tt[0], 0]])
    F = np.linalg.inv(vt.K.T) @ (T @ R) @ np.linalg.inv(vs.K)
    return F, vs.R.T @ np.linalg.inv(vs.K), vt.R.T @ np.linalg.inv(vt.K), -vs.R.T @ vs.t, -vt.R.T @ vt.t


def _match_lines():
    vs, vt = scene().views[:2]
    slots, n = api.match_lines(vs.segs, vt.segs, *_pair_arguments(vs, vt), vs.width, vs.height, 0.25, 10)
    assert slots.shape == (len(vs.segs), 10)


def _triangulate():
    views = scene().views[:3]
    Ps = np.stack([v.K @ np.column_stack([v.R, v.t]) for v in views])
    X = np.array([[0.5, 0.2, 0.1], [-0.4, 0.3, 0.6], [0.1, -0.7, 0.2], [0.9, 0.8, -0.3]])
    off, cam, xy = TM.observations(Ps, X, [[0, 1, 2]] * 4)[:3]
    Xd, valid = api.triangulate_points(Ps, off, cam, xy)
    assert Xd.shape == (4, 3)


def _projection_stages():
    cams = Cs.stage1_cameras()[:2]
    P1, P2, line = Cs.stage1_segments()
    rec = api.project_segments(cams, P1[:8], P2[:8], line[:8])
    maps = api.render_line_maps(cams, rec)
    images = [np.full((c["height"], c["width"]), 90, np.uint8) for c in cams]
    assert len(api.draw_line_maps(images, [m[0] for m in maps])) == 2


def _selftests():
    data = np.arange(5000, dtype=np.uint32)      # two tiles of 4 096
    assert scan_cases.selftest_scan(data, [5000])[0] == 0
    counts = np.zeros(3, np.uint64)
    assert _lib.load().l3d_selftest_arith(0, 1000, 1, ptr(counts)) == 0


def _line_opt_eval():
    K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
    P1, P2 = np.array([0.3, 0.2, 6.0]), np.array([1.0, -0.4, 6.5])
    x, constant = LM.to_cayley(P1, P2)
    assert not constant
    n = 4
    cams = np.stack([LM.camera(np.eye(3), np.array([0.1 * i, 0.0, 0.0]), K) for i in range(n)])
    obs = np.stack([LM.observation(np.concatenate([(K @ (P1 - c[9:12]))[:2] / (P1 - c[9:12])[2],
                                                   (K @ (P2 - c[9:12]))[:2] / (P2 - c[9:12])[2]])) for c in cams])
    cost = np.zeros(1); r = np.zeros(2 * n); J = np.zeros(8 * n); ok = np.zeros(n, np.int32)
    assert _lib.load().l3d_line_opt_eval(0, n, ptr(np.asarray(x, np.float64)), ptr(np.ascontiguousarray(obs, np.float64)),
                                         ptr(np.ascontiguousarray(cams, np.float64)), ptr(cost), ptr(r), ptr(J), ptr(ok)) == 0


def _line_opt_solve():
    b = line_opt_cases.grid_batch(1, 1)
    x, cost0, cost1, iters, status = api.line_opt_solve(b.x0, b.res_off, b.obs, b.obs_cam, b.cams)
    assert x.shape == (2, 4) and np.all(cost1 <= cost0)


def _undistort():
    img = polygons(800, 600, 5)
    K = np.array([[700.0, 0, 400], [0, 700, 300], [0, 0, 1]])
    assert lsd.undistort_images([img], [K], [(-0.1, 0.01, 0.0)], [(1e-3, -1e-3)])[0].shape == img.shape
    assert lsd.undistort_images_model([img], ["OPENCV_FISHEYE"], [K], [(0.05, -0.01, 0.0, 0.0)])[0].shape == img.shape


@pytest.mark.parametrize("call", [_diffuse, _collinear, _score, _match_lines, _triangulate, _projection_stages, _selftests,
                                  _line_opt_eval, _line_opt_solve, _undistort], ids=lambda f: f.__name__.lstrip("_"))
def test_stateless_entries_hold_nothing_afterwards(call):
    """one successful small call of each (the wrappers raise on a status other than 0)"""
    base = baseline()
    call()
    assert settled() == base


def test_detection_on_a_live_context_holds_nothing_afterwards():
    L = _lib.load()
    g = Line3D()
    arr, keep = lsd.image_array([polygons(800, 600, 7)])
    counts = np.zeros(1, np.uint32)
    base = baseline()
    assert L.l3d_detect_segments(g.h, 1, arr, -1, 3000, ptr(counts)) == 0 and counts[0] > 0
    assert settled() == base
    g.close()


def test_a_refused_call_holds_nothing_either():
    """kNN = 1024 on 64 x 64 segments: the top-K tables of 64 rows would take 64 x 1024 x 8 B = 512 KiB of LDS against the
    limit of 160 KiB.  l3d_match_lines finds that out after it has reserved seven buffers; it launches nothing."""
    L = _lib.load()
    vs, vt = scene().views[:2]
    a, b = np.ascontiguousarray(vs.segs[:64]), np.ascontiguousarray(vt.segs[:64])
    args = [np.ascontiguousarray(x, np.float64) for x in _pair_arguments(vs, vt)]
    out = np.zeros((64, 1024), _lib.SLOT_DTYPE)
    n = C.c_uint64()
    base = baseline()
    rc = L.l3d_match_lines(0, ptr(a), 64, ptr(b), 64, *[ptr(x) for x in args], vs.width, vs.height, 0.25, 1024, ptr(out), C.byref(n))
    assert rc == L3D_ERR_LIMIT and _lib.last_error() == "kNN too large for the LDS top-K table"
    assert settled() == base


def test_the_cache_still_takes_a_contexts_blocks():
    L = _lib.load()
    sc = scene()
    gc.collect()
    L.l3d_trim_cache()
    g = Line3D()
    g.add_scene(sc)
    whole_pipeline(g, sc)
    g.close()
    assert L.l3d_trim_cache() > 0
