"""Cameras and 3D lines bundled jointly on the MI355X (k_bundle.hip, l3d_bundle.hip) against the numpy model
of tests/bundle_model.py at tolerance 0: the associations against l3d_project_segments + l3d_associate_segments, and from
them on the reduced system of the first iteration, the trace, the cameras, the carriers, the spans, the pieces, the
statuses and the output model.  The model is handed the library's own dense solve (l3d_bundle_solve, which
tests/test_bundle_host.py pins against the model's and against numpy.linalg.solve).  Then the context form on the golden
scene, the counters, the recovery on the alternation scene of §28 against the alternation itself, and the real data."""
import ctypes as C
import math

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from line3dpp_amd.api import Line3D
from tests import bundle_cases as BC
from tests import bundle_model as BM
from tests import pose_cases as PC
from tests import pose_model as PO
from tests import refit_cases as RC
from tests.pose_cases import same_bytes

pytestmark = pytest.mark.gpu

p = _lib.ptr


def lib_solve(S, g):
    n = len(g)
    if n == 0:
        return np.zeros(0)
    S = np.ascontiguousarray(S, np.float64); g = np.ascontiguousarray(g, np.float64); d = np.zeros(n)
    rc = _lib.load().l3d_bundle_solve(n, p(S), p(g), p(d))
    assert rc in (0, 1)
    return d if rc == 1 else None


def check(s, what, got=None, **kw):
    """one call against the model built from the library's own associations -> (the library's dict, the model's)"""
    kw = dict(s["par"], **kw)
    segs, line, cams, obs, fixed = s["segs"], s["line"], s["cams"], s["obs"], s.get("fixed")
    if got is None:
        got = api.bundle_segments(segs, line, cams, obs, fixed, capture_iteration=1, **kw)
    rec = api.project_segments(cams, segs[:, :3], segs[:, 3:], line, near=kw.get("near", 1e-6))
    chain = api.associate_segments(rec, obs, kw["max_distance"], kw.get("max_angle", 10.0), kw.get("min_overlap", 0.5))
    assert len(got["associations"]) == len(cams)
    for k in range(len(cams)):
        same_bytes(got["associations"][k], chain[k], f"{what}: associations of camera {k}")
    want = BM.bundle(segs, line, cams, obs, fixed=fixed, assoc=chain, solve=lib_solve, **BC.model_par(capture_iteration=1, **kw))
    sm, wm = got["summary"], want["summary"]
    for f in ("status", "iterations", "accepted_steps", "rejected_steps", "n_observations", "n_cells", "n_eligible_lines", "n_free_cameras",
              "n_lines", "lines"):
        assert sm[f] == wm[f], (what, f, sm[f], wm[f])
    if wm["n_free_cameras"] and wm["iterations"]:
        same_bytes(got["system"], want["system"], f"{what}: the reduced system of iteration 1")
        same_bytes(got["rhs"], want["rhs"], f"{what}: its right-hand side")
    same_bytes(got["trace"], want["trace"], f"{what}: trace")
    for f in ("cost0", "cost1", "damping"):
        same_bytes(np.float64(sm[f]), np.float64(wm[f]), f"{what}: summary {f}")
    for k in range(len(cams)):
        PC.same_camera(got["cameras"][k], want["cameras"][k], f"{what}: camera {k}")
    same_bytes(got["observations"], want["observations"], f"{what}: observations and spans")
    same_bytes(got["lines"], want["lines"], f"{what}: lines")
    same_bytes(got["segments"], want["segments"], f"{what}: output segments")
    same_bytes(got["line"], want["line"], f"{what}: output line indices")
    # every line that is not BUNDLED comes back bit for bit, in input order; a camera no step moved comes back bit for bit
    assert (np.diff(got["line"].astype(np.int64)) >= 0).all()
    for l in np.flatnonzero(got["lines"]["status"] != BM.BUNDLED):
        same_bytes(got["segments"][got["line"] == l], segs[line == l], f"{what}: line {l} as given")
    P = want["problem"]
    for k in range(len(cams)):
        if P.cam_free[k] < 0 or not sm["accepted_steps"]:
            PC.same_camera(got["cameras"][k], cams[k], f"{what}: camera {k} as given")
    assert sm["n_segments_before"] == len(segs) and sm["n_segments_after"] == len(got["segments"])
    return got, want


@pytest.mark.parametrize("name", list(BC.CASES))
def test_case_equals_the_model(name):
    s = BC.CASES[name]()
    got, want = check(s, name)
    print(name, got["summary"])
    if name == "two groups of cameras that share no line":
        assert not got["system"][0:18, 18:36].any()
    if name == "reject":
        assert got["summary"]["rejected_steps"] >= 1 and got["summary"]["accepted_steps"] >= 1
    if name == "pivot":
        assert got["trace"]["n_held_for_step"].max() >= 1
    if name == "max_iterations = 0":
        assert len(got["trace"]) == 0 and got["summary"]["cost0"] == got["summary"]["cost1"]
    if name == "all cameras fixed":
        assert got["summary"]["n_free_cameras"] == 0 and got["summary"]["accepted_steps"] >= 1


def test_two_calls_in_a_row_are_equal():
    s = BC.ring(30, 3)
    a = api.bundle_segments(s["segs"], s["line"], s["cams"], s["obs"], **s["par"])
    b = api.bundle_segments(s["segs"], s["line"], s["cams"], s["obs"], **s["par"])
    for k in ("segments", "line", "lines", "observations", "trace"):
        same_bytes(a[k], b[k], f"two calls: {k}")
    for x, y in zip(a["cameras"], b["cameras"]):
        PC.same_camera(x, y, "two calls: cameras")


def test_counters_count():
    L = _lib.load()
    s = BC.CASES["one camera fixed"]()
    it0, rj0 = L.l3d_debug_counter(b"bundle_iterations"), L.l3d_debug_counter(b"bundle_rejected_steps")
    got = api.bundle_segments(s["segs"], s["line"], s["cams"], s["obs"], s["fixed"], **s["par"])
    assert L.l3d_debug_counter(b"bundle_iterations") - it0 == got["summary"]["iterations"] > 0
    assert L.l3d_debug_counter(b"bundle_rejected_steps") - rj0 == got["summary"]["rejected_steps"]


def test_device_refusals_leave_the_handle_alone():
    L = _lib.load()
    s = BC.ring(10, 2)
    with pytest.raises(RuntimeError, match="visibility"):
        api.bundle_segments(s["segs"], s["line"], s["cams"], s["obs"], visibility=0)
    with pytest.raises(RuntimeError, match="K01"):
        skew = [dict(c, K=np.array(c["K"]) + np.array([[0, 0.5, 0], [0, 0, 0], [0, 0, 0]])) for c in s["cams"]]
        api.bundle_segments(s["segs"], s["line"], skew, s["obs"])
    blocks = L.l3d_debug_counter(b"live_device_blocks")
    none = api.bundle_segments(s["segs"], s["line"], [], [])
    assert none["summary"]["status"] == "NO_VARIABLES" and none["segments"].tobytes() == s["segs"].tobytes()
    api.bundle_segments(s["segs"], s["line"], s["cams"], s["obs"], visibility=2)
    assert L.l3d_debug_counter(b"live_device_blocks") == blocks


# ---- recovery: the joint bundle against the alternation of §28 on its own scene -------------------------------------------
def yardstick(segs, line, cams, obs):
    """rms of the matched distances per camera: l3d_project_segments + l3d_associate_segments at 2.5 px"""
    rec = api.project_segments(cams, segs[:, :3], segs[:, 3:], line)
    assoc = api.associate_segments(rec, obs, 2.5)
    out = []
    for a in assoc:
        d = a["distance"][a["record"] >= 0].astype(np.float64)
        out.append(math.sqrt(float((d * d).mean())) if len(d) else 0.0)
    return out


def test_recovery_on_the_alternation_scene():
    """refit_cases.alternation() through bundle_model(rounds=3) and through refine_model(rounds=3), both measured by the
    largest per-camera rms of the distances that l3d_project_segments + l3d_associate_segments match at 2.5 px on the
    returned cameras and model.  Every round of the joint bundle equals the numpy model bit for bit.  Figures of the numpy
    models on the CPU: start 1.6582 px; joint 1.1154, 0.2050, 0.1825 after rounds 1 to 3; alternation 0.1827,
    0.1658, 0.1645.  The joint figure is not better than the alternation's."""
    s = BC.alternation()
    start = max(yardstick(s["segs"], s["line"], s["cams"], s["obs"]))
    # the joint bundle, round by round against the model, each round on the library's own result of the round before
    segs, line, cams = s["segs"], s["line"], s["cams"]
    for r in range(3):
        got, _ = check(dict(s, segs=segs, line=line, cams=cams), f"alternation scene, round {r}")
        segs, line, cams = got["segments"], got["line"], got["cameras"]
        print("round", r, got["summary"], "largest per-camera rms", max(yardstick(segs, line, cams, s["obs"])))
    joint = api.bundle_model(s["segs"], s["line"], s["cams"], s["obs"], rounds=3, keep_gauge=True, **s["par"])
    same_bytes(joint["bundle"]["segments"], segs, "the driver's last round")
    for a, b in zip(joint["bundle"]["cameras"], cams):
        PC.same_camera(a, b, "the driver's last round: cameras")
    alt = api.refine_model(s["segs"], s["line"], s["cams"], s["obs"], rounds=3, **s["par"])
    yj = yardstick(joint["segments"], joint["line"], joint["cameras"], s["obs"])
    yj_free = yardstick(segs, line, cams, s["obs"])
    ya = yardstick(alt["segments"], alt["line"], alt["cameras"], s["obs"])
    print(f"largest per-camera rms at 2.5 px: start {start:.4f}, alternation {max(ya):.4f}, joint {max(yj):.4f} (before the gauge step {max(yj_free):.4f})")
    # (the numpy models give joint 0.1825 against 0.1645 of the alternation: NOT better by this yardstick, as DESIGN §29
    # reports, so the joint result is held against the starting value only)
    assert max(yj) < start
    # the gauge: mean and scatter of the camera centres equal the input's
    assert joint["gauge"] is not None and joint["gauge_skipped"] is None
    diag = PO.bounding_box(s["segs"])[1]
    c0, c1 = api.camera_centres(s["cams"]), api.camera_centres(joint["cameras"])
    assert np.abs(c0.mean(0) - c1.mean(0)).max() <= 1e-9 * diag
    scatter = lambda c: math.sqrt(float(((c - c.mean(0)) ** 2).sum() / len(c)))
    assert abs(scatter(c0) - scatter(c1)) <= 1e-9 * diag
    two = api.bundle_model(s["segs"], s["line"], s["cams"][:2], s["obs"][:2], rounds=1, visibility=2, max_distance=6.0)
    assert two["gauge"] is None and "fewer than three" in two["gauge_skipped"]


# ---- real data ----------------------------------------------------------------------------------------------------------
def test_real_scene_cost_falls_and_statuses_equal_the_model():
    """golden scene C0 against the reference's optimised model, the fixture's poses with K01 = 0 as §28's test sets it,
    2.5 px, one round"""
    s = PC.real_scene()
    s["cams"] = [PO.camera(np.where(np.arange(9).reshape(3, 3) == 1, 0.0, c["K"]), c["R"], c["t"], c["width"], c["height"]) for c in s["cams"]]
    s["par"] = dict(max_distance=2.5, visibility=3)
    s["fixed"] = None
    got, want = check(s, "real scene")
    sm = got["summary"]
    print("real scene:", sm)
    assert sm["cost1"] <= sm["cost0"]
    assert got["lines"]["status"][::8].tolist() == want["lines"]["status"][::8].tolist()


# ---- the context form on the golden scene -----------------------------------------------------------------------------
@pytest.fixture()
def golden():
    from tests.golden.make_golden import golden_scene
    sc = golden_scene()
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages() and g.reconstruct3Dlines(3)
    yield dict(sc=sc, g=g, cam_ids=[v.cam for v in sc.views])
    g.close()


def test_context_form_replaces_the_model(golden):
    g, sc, ids = golden["g"], golden["sc"], golden["cam_ids"]
    L = _lib.load()
    order = sorted(ids)
    before = g.get3Dlines()
    segs, line = api.flatten_lines(before)
    cams = [g.viewCamera(c) for c in order]
    obs = [np.array([g.getSegmentCoords2D(c, k) for k in range(len(sc.views[ids.index(c)].segs))], np.float32).reshape(-1, 4) for c in order]
    name_before = g.outputFilename()
    free = api.bundle_segments(segs, line, cams, obs, max_distance=2.5)
    check(dict(segs=segs, line=line, cams=cams, obs=obs, par=dict(max_distance=2.5)), "golden scene")
    # (a first call sizes the context's own work space, which it keeps until it is closed; the model is then built again)
    assert g.bundleModel(max_distance=2.5, max_iterations=0) is not None and g.reconstruct3Dlines(3)
    same_bytes(api.flatten_lines(g.get3Dlines())[0], segs, "the lines after a second reconstruct3Dlines")
    blocks = L.l3d_debug_counter(b"live_device_blocks")
    g.set_projection_budget(64)                   # one camera per group at most
    try:
        assert g.setTimingLevel(2)
        ctx = g.bundleModel(max_distance=2.5)
    finally:
        g.set_projection_budget(0); g.setTimingLevel(1)
    assert ctx is not None and ctx["camIDs"] == order
    assert L.l3d_debug_counter(b"live_device_blocks") == blocks
    for k in ("segments", "line", "lines", "observations", "trace"):
        same_bytes(ctx[k], free[k], f"context / stateless: {k}")
    for a, b in zip(ctx["cameras"], free["cameras"]):
        PC.same_camera(a, b, "context / stateless: cameras")
    same_bytes(ctx["associations"], np.concatenate(free["associations"]), "context / stateless: associations")
    assert 0 < L.l3d_debug_counter(b"bundle_kernel_ns") < 10 ** 9
    # the views are unchanged, the model is replaced
    for c, cam in zip(order, cams):
        PC.same_camera(g.viewCamera(c), cam, f"view {c} after the call")
    after = g.get3Dlines()
    st = ctx["lines"]["status"]
    assert len(after) == len(before) and (st == BM.BUNDLED).sum() > 0
    seg2, line2 = api.flatten_lines(after)
    same_bytes(seg2, ctx["segments"], "the context's lines"); same_bytes(line2, ctx["line"], "the context's line indices")
    name = g.outputFilename()
    assert "BUNDLE_2.5__" in name and name.replace("BUNDLE_2.5__", "") == name_before
    assert g.reconstruct3Dlines(3) and g.outputFilename() == name_before
    # refusals as refitLines': printed, None, the model untouched
    segs_now = api.flatten_lines(g.get3Dlines())[0]
    assert g.bundleModel(visibility=0) is None and "visibility" in _lib.last_error()
    assert g.bundleModel([ids[0], 987654]) is None and "unknown camera ID" in _lib.last_error()
    assert g.bundleModel([ids[1], ids[0], ids[1]]) is None and "named twice" in _lib.last_error()
    assert api.flatten_lines(g.get3Dlines())[0].tobytes() == segs_now.tobytes() and "BUNDLE" not in g.outputFilename()


def test_context_errors(golden):
    """the context entry's refusals, which are refitLines': nothing of the context changes, neither its lines nor the
    records of the last projection"""
    g, ids = golden["g"], golden["cam_ids"]
    L = _lib.load()

    def records():
        n = C.c_uint64(0)
        assert L.l3d_get_projected_lines(g.h, None, 0, C.byref(n)) == 0
        rec = np.zeros(max(n.value, 1), api.PROJECTED_SEGMENT_DTYPE)
        assert L.l3d_get_projected_lines(g.h, _lib.ptr(rec), n.value, C.byref(n)) == 0
        return rec[:n.value].tobytes()

    assert sum(len(r) for r in g.projectLines([ids[0], ids[1]])) > 0
    segs, rec = api.flatten_lines(g.get3Dlines())[0], records()
    assert len(rec) > 0
    for what, arg, message in (("an ID named twice", [ids[1], ids[0], ids[1]], "a camera ID is named twice"),
                               ("an unknown ID", [ids[0], 987654], "unknown camera ID"),
                               ("both: named twice comes first", [987654, ids[0], 987654], "a camera ID is named twice")):
        assert g.bundleModel(arg) is None and g.last_status == -1 and _lib.last_error() == message, what
        assert api.flatten_lines(g.get3Dlines())[0].tobytes() == segs.tobytes() and records() == rec, what
        assert "BUNDLE" not in g.outputFilename(), what
    # before the lines exist, and while a split call is open
    from line3dpp_amd.scene import make_scene
    h = Line3D()
    h.add_scene(make_scene(4, 60, n_neighbors=2, seed=2))
    assert h.bundleModel() is None and h.last_status == -7 and _lib.last_error().startswith("no 3D lines to bundle")
    assert h.matchBegin()
    par = api.bundle_params()
    ids4 = np.arange(4, dtype=np.uint32)
    assert L.l3d_bundle_view_lines(h.h, 4, _lib.ptr(ids4), None, None, C.byref(par), None, None) == -7 and "split call" in _lib.last_error()
    h.matchAbort()
    h.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_bundle_model(tmp_path):
    import os
    import struct
    import subprocess
    from line3dpp_amd.scene import make_scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "bundle_smoke")
    lib_dir = os.path.join(root, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "bundle_smoke.cpp"), "-o", exe, "-L" + lib_dir,
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
    out_path = str(tmp_path / "out.bin")
    run_ = subprocess.run([exe, path, out_path], capture_output=True, text=True, timeout=300)
    assert run_.returncode == 0, run_.stdout[-2000:] + run_.stderr[-2000:]
    assert run_.stdout.count("[L3D++] ERROR:") == 2 and "bundleModel" in run_.stdout   # the call before the reconstruction, a bad angle
    raw = open(out_path, "rb").read()
    sm = _lib.BundleSummary.from_buffer_copy(raw, 0)
    pos, models = C.sizeof(_lib.BundleSummary), []
    for _ in range(2):
        n, = struct.unpack_from("<I", raw, pos); pos += 4
        segs = np.frombuffer(raw, np.float64, 6 * n, pos).reshape(n, 6); pos += 48 * n
        models.append((segs, np.frombuffer(raw, np.uint32, n, pos))); pos += 4 * n
    held, new = {}, {}
    for _ in range(sc.n_views):
        cam_id, = struct.unpack_from("<I", raw, pos); pos += 4
        held[cam_id] = api.camera_dict(_lib.Camera.from_buffer_copy(raw, pos)); pos += C.sizeof(_lib.Camera)
        new[cam_id] = api.camera_dict(_lib.Camera.from_buffer_copy(raw, pos)); pos += C.sizeof(_lib.Camera)
    assert pos == len(raw)
    views = sorted(sc.views, key=lambda v: v.cam)
    cams = [held[v.cam] for v in views]               # (the cameras as the context holds them: unchanged by the call)
    obs = [np.ascontiguousarray(v.segs, np.float32).reshape(-1, 4) for v in views]
    want = api.bundle_segments(models[0][0], models[0][1], cams, obs, max_distance=2.5)
    print(run_.stdout.strip().splitlines()[-1], want["summary"])
    same_bytes(models[1][0], want["segments"], "the facade's model / the stateless call")
    same_bytes(models[1][1], want["line"], "the facade's line indices / the stateless call")
    for v, cam in zip(views, want["cameras"]):
        PC.same_camera(new[v.cam], cam, f"the facade's camera {v.cam} / the stateless call")
    assert api.bundle_summary_dict(sm) == want["summary"] and sm.n_status[0] > 0
