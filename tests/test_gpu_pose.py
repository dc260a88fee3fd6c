"""Camera poses refined against the 3D line model on the MI355X (k_pose.hip, l3d_pose.hip) against the numpy
model of tests/pose_model.py: tolerance 0 on every output field and every trace field."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from line3dpp_amd.api import Line3D
from tests import pose_cases as Cs
from tests import pose_model as P
from tests.test_pose_host import GOOD, MEASURED, MEASURED_REAL, REAL_SUBSET

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A5A5A5A
COUNTERS = ("pose_iterations", "pose_normal_launches", "associate_launches")


def counters():
    L = _lib.load()
    return {k: L.l3d_debug_counter(k.encode()) for k in COUNTERS}


def run(s, cams=None, obs=None, **kw):
    return api.refine_cameras(s["segs"], s["line"], s["cams"] if cams is None else cams, s["obs"] if obs is None else obs, **kw)


def model(s, cams=None, obs=None, max_angle=10.0, near=1e-6, **kw):
    return P.refine(s["segs"], s["line"], s["cams"] if cams is None else cams, s["obs"] if obs is None else obs,
                    min_cos2=P.AM.min_cos2_of(max_angle), near_plane=near, **kw)


@pytest.mark.parametrize("n2d,n3d", Cs.EDGE_SHAPES)
def test_one_iteration_at_lane_wave_and_tile_edges(n2d, n3d):
    s = Cs.edge_scene(n2d, n3d)
    kw = dict(start_distance=6.0, max_iterations=1, min_matches=6)
    before = counters()
    got = run(s, **kw)
    after = counters()
    Cs.same_result(got, model(s, **kw), f"({n2d}, {n3d})")
    sm = got["summaries"][0]
    assert sm["iterations"] == 1 and len(got["trace"][0]) == 1
    if n2d >= 63:
        assert sm["status"] == "MAX_ITERATIONS" and got["trace"][0]["delta"][0].all() and got["trace"][0]["n_matched"][0] > n2d // 2
    else:
        assert sm["status"] == "TOO_FEW"
    assert after["pose_iterations"] == before["pose_iterations"] + 1
    assert after["pose_normal_launches"] == before["pose_normal_launches"] + 2          # the iteration and the delivery pass
    assert after["associate_launches"] == before["associate_launches"]                  # l3d_associate.hip's counter stays its own


def test_waves_and_a_tile_without_a_match():
    s, dead = Cs.gap_scene()
    kw = dict(start_distance=6.0, max_iterations=2, min_matches=6)
    got = run(s, **kw)
    Cs.same_result(got, model(s, **kw), "gaps")
    a = got["associations"][0]
    assert (a["record"][dead] == -1).all() and (a["record"][~dead] >= 0).sum() > 200


def test_seven_cameras_in_one_call_equal_the_model_and_each_camera_alone():
    s = Cs.mixed_scene()
    kw = dict(start_distance=6.0, max_iterations=6, min_matches=6)
    got = run(s, **kw)
    Cs.same_result(got, model(s, **kw), "seven cameras")
    assert [len(o) for o in s["obs"]] == [0, 300, 1, 257, 64, 5, 0]
    assert [x["status"] for x in got["summaries"]][:3] == ["TOO_FEW"] * 3 and got["summaries"][1]["iterations"] == 1
    assert got["summaries"][0]["iterations"] == 0 and got["summaries"][3]["iterations"] > 1
    for k in range(7):
        alone = run(s, cams=[s["cams"][k]], obs=[s["obs"][k]], **kw)
        Cs.same_result(alone, {key: [got[key][k]] for key in ("cameras", "summaries", "associations", "trace")}, f"camera {k} alone")
    for k in (0, 1, 2, 5, 6):                                                            # never updated: bit for bit as given
        Cs.same_camera(got["cameras"][k], s["cams"][k], f"camera {k}")


def test_cameras_that_finish_in_different_iterations():
    """perturbed cameras, the same cameras at their true poses, one whose segments are points and one seen twice with
    another gate history: the tile table shrinks, and several gates are in force in one iteration"""
    s = Cs.recovery_scene()
    points = s["obs"][0].copy(); points[:, 2:] = points[:, :2]
    cams = [s["cams"][0], s["truth"][0], s["cams"][1], s["cams"][0], s["truth"][2]]
    obs = [s["obs"][0], s["obs"][0], s["obs"][1], points, s["obs"][2]]
    got = run(s, cams=cams, obs=obs, **s["par"])
    Cs.same_result(got, model(s, cams=cams, obs=obs, **s["par"]), "different iterations")
    its = [x["iterations"] for x in got["summaries"]]
    assert its[3] == 1 and got["summaries"][3]["status"] == "TOO_FEW" and len(set(its)) >= 3, its
    print(its, [list(t["gate"]) for t in got["trace"]])
    assert len({t["gate"][2] for t in got["trace"] if len(t) > 2}) >= 2             # two gates in force in the third iteration


@pytest.mark.parametrize("name", list(Cs.RECOVERY))
def test_full_runs_equal_the_model_bit_for_bit(name):
    s = Cs.recovery_scene(**Cs.RECOVERY[name])
    got = run(s, **s["par"])
    Cs.same_result(got, model(s, **s["par"]), name)
    angle, centre = Cs.pose_errors(got["cameras"], s["truth"], [s["depth"]] * len(s["cams"]))
    its = max(x["iterations"] for x in got["summaries"])
    print(name, its, angle, centre)
    assert all(x["status"] == "CONVERGED" for x in got["summaries"])
    assert its <= 2 * MEASURED[name][0] and angle <= 10 * MEASURED[name][1] and centre <= 10 * MEASURED[name][2]


@pytest.fixture(scope="module")
def real_tenth():
    kw = dict(Cs.REAL["tenth"]); start_distance = kw.pop("start_distance")
    s = Cs.real_scene(**kw)
    return s, start_distance, run(s, start_distance=start_distance)


def test_real_cameras_equal_the_model_with_their_whole_trace(real_tenth):
    """six of the 26 cameras against the model (it takes 5 s for them); each equals what it got among all 26"""
    s, start_distance, full = real_tenth
    sub = REAL_SUBSET
    want = model(s, cams=[s["cams"][i] for i in sub], obs=[s["obs"][i] for i in sub], start_distance=start_distance)
    Cs.same_result({key: [full[key][i] for i in sub] for key in ("cameras", "summaries", "associations", "trace")}, want, "real subset")


@pytest.mark.parametrize("name", list(Cs.REAL))
def test_every_real_camera_is_recovered(name, real_tenth):
    if name == "tenth":
        s, _, got = real_tenth
    else:
        kw = dict(Cs.REAL[name]); start_distance = kw.pop("start_distance")
        s = Cs.real_scene(**kw)
        got = run(s, start_distance=start_distance)
    d = [P.pose_difference(c, f, z) for c, f, z in zip(got["cameras"], s["fixture"], s["depth"])]
    its = [x["iterations"] for x in got["summaries"]]
    print(name, "iterations", min(its), int(np.median(its)), max(its), "angle", max(a for a, _ in d), "centre", max(b for _, b in d),
          "rms", min(x["rms"] for x in got["summaries"]), max(x["rms"] for x in got["summaries"]))
    assert all(x["status"] == "CONVERGED" for x in got["summaries"]) and max(its) <= 2 * MEASURED_REAL[name]
    assert all(a <= 0.05 and b <= 1e-3 for a, b in d)
    assert all(x["n_matched"] >= 0.9 * len(o) and x["rms"] < 1.0 for x, o in zip(got["summaries"], s["obs"]))


def test_the_delivered_associations_are_those_of_the_public_chain(real_tenth):
    s, _, got = real_tenth
    pick = [0, 9, 25]
    cams = [got["cameras"][i] for i in pick]
    rec = api.project_segments(cams, s["segs"][:, :3], s["segs"][:, 3:], s["line"])
    chain = api.associate_segments(rec, [s["obs"][i] for i in pick])
    for k, i in enumerate(pick):
        Cs.same_bytes(got["associations"][i], chain[k], f"camera {i}: delivery pass / l3d_associate_segments")
        assert (chain[k]["record"] >= 0).sum() >= got["summaries"][i]["n_matched"] > 300


def test_degenerate_too_few_and_the_empty_forms():
    s = Cs.parallel_scene()
    got = run(s, min_matches=6)
    Cs.same_result(got, model(s, min_matches=6), "parallel lines")
    assert got["summaries"][0]["status"] == "DEGENERATE" and got["trace"][0]["sums"][0][P.ROW[3]] == 0.0
    Cs.same_camera(got["cameras"][0], s["cams"][0], "degenerate")
    s = Cs.crossing_scene()
    R = np.eye(3); R[0, 1] = -0.0; R[2, 0] = -0.0
    cams = [Cs.hand_camera(R)]
    got = run(s, cams=cams, min_matches=10)
    Cs.same_result(got, model(s, cams=cams, min_matches=10), "too few")
    assert got["summaries"][0]["status"] == "TOO_FEW" and got["summaries"][0]["n_matched"] == 9
    Cs.same_camera(got["cameras"][0], cams[0], "too few")
    assert np.signbit(got["cameras"][0]["R"][0, 1]) and np.signbit(got["cameras"][0]["R"][2, 0])
    got = run(s, cams=cams, min_matches=9)
    Cs.same_result(got, model(s, cams=cams, min_matches=9), "nine matches")
    assert got["summaries"][0]["status"] == "CONVERGED" and got["summaries"][0]["rms"] == 0.0
    none = np.zeros((0, 4), np.float32)
    for what, segs, line, cs, obs in (("an empty model", s["segs"][:0], s["line"][:0], cams * 2, [s["obs"][0], none]),
                                      ("one camera without segments", s["segs"], s["line"], cams * 2, [none, s["obs"][0]])):
        got = api.refine_cameras(segs, line, cs, obs, min_matches=9)
        Cs.same_result(got, P.refine(segs, line, cs, obs, min_matches=9), what)


def test_two_calls_in_a_row_give_equal_bytes():
    s = Cs.recovery_scene(noise=0.3)
    a, b = run(s, **s["par"]), run(s, **s["par"])
    Cs.same_result(b, a, "second call")


# ---- the context form on the golden scene -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    from tests.golden.make_golden import golden_scene
    sc = golden_scene()
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages() and g.reconstruct3Dlines(3)
    yield dict(sc=sc, g=g, cam_ids=[v.cam for v in sc.views])
    g.close()


def test_context_equals_the_stateless_call_and_leaves_the_context_alone(golden):
    g, sc, ids = golden["g"], golden["sc"], golden["cam_ids"]
    lines_before = api.flatten_lines(g.get3Dlines())
    cams_before = [g.viewCamera(c) for c in ids]
    kw = dict(start_distance=10.0)
    ctx = g.refineCameras(**kw)
    assert ctx is not None and ctx["camIDs"] == sorted(ids)
    segs, line = lines_before
    order = sorted(ids)
    cams = [g.viewCamera(c) for c in order]
    obs = [np.array([g.getSegmentCoords2D(c, k) for k in range(len(sc.views[ids.index(c)].segs))], np.float32).reshape(-1, 4) for c in order]
    free = api.refine_cameras(segs, line, cams, obs, **kw)
    Cs.same_result(ctx, free, "context / stateless")
    Cs.same_result(ctx, P.refine(segs, line, cams, obs, **kw), "context / model")
    lines_after = api.flatten_lines(g.get3Dlines())
    assert lines_before[0].tobytes() == lines_after[0].tobytes() and lines_before[1].tobytes() == lines_after[1].tobytes()
    for c, cam in zip(ids, cams_before):
        Cs.same_camera(g.viewCamera(c), cam, f"view {c} after the call")
    # one camera per group at most, and a subset in reversed order: nothing a camera gets changes
    g.set_projection_budget(64)
    try:
        small = g.refineCameras(**kw)
    finally:
        g.set_projection_budget(0)
    Cs.same_result(small, ctx, "small budget")
    pick = [order[7], order[4], order[1]]
    sub = g.refineCameras(pick, **kw)
    assert sub["camIDs"] == pick
    Cs.same_result(sub, {key: [ctx[key][order.index(c)] for c in pick] for key in ("cameras", "summaries", "associations", "trace")}, "a subset")
    # reported, not asserted: the matches and the rms at the views' own cameras and after the refinement
    own = g.refineCameras()
    assoc = g.associateSegments(order)[0]
    for k, c in enumerate(order):
        n0 = int((assoc[c]["record"] >= 0).sum())
        print("view", c, "matched", n0, "->", own["summaries"][k]["n_matched"], "rms", own["summaries"][k]["rms"], own["summaries"][k]["status"])
    assert sum(x["n_matched"] for x in own["summaries"]) > 200


def test_context_errors_and_the_kernel_time(golden):
    g, ids = golden["g"], golden["cam_ids"]
    L = _lib.load()
    assert g.refineCameras(max_angle=120.0) is None and g.last_status == -1
    assert g.refineCameras(max_distance=-1.0) is None and g.last_status == -1
    assert g.refineCameras(max_distance=2.0, start_distance=1.0) is None and "start_distance" in _lib.last_error()
    assert g.refineCameras([ids[0], 987654]) is None and "unknown camera ID" in _lib.last_error()
    assert g.refineCameras([ids[1], ids[0], ids[1]]) is None and "named twice" in _lib.last_error()
    none = g.refineCameras([])
    assert none is not None and none["cameras"] == [] and none["camIDs"] == []
    assert g.setTimingLevel(2)
    try:
        assert g.refineCameras(ids[:3]) is not None
        assert 0 < L.l3d_debug_counter(b"pose_kernel_ns") < 10 ** 9
    finally:
        g.setTimingLevel(1)
    from line3dpp_amd.scene import make_scene
    h = Line3D()
    h.add_scene(make_scene(4, 60, n_neighbors=2, seed=2))
    assert h.refineCameras() is None and h.last_status == -7
    assert h.matchBegin()
    par = api.pose_params()
    ids4 = np.arange(4, dtype=np.uint32)
    cams = (_lib.Camera * 4)(); sums = np.full(4 * 22, FILL, np.uint32); off = np.full(5, FILL, np.uint64)
    assert L.l3d_refine_view_cameras(h.h, 4, _lib.ptr(ids4), C.byref(par), cams, _lib.ptr(sums), _lib.ptr(off), None, None) == -7
    assert "split call" in _lib.last_error() and (sums == FILL).all() and (off == FILL).all()
    h.matchAbort()
    h.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_refine_cameras(tmp_path):
    from line3dpp_amd.scene import make_scene
    exe = str(tmp_path / "pose_smoke")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_smoke.cpp"), "-o", exe, "-L" + lib_dir,
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
    assert run_.stdout.count("[L3D++] ERROR:") == 2 and "refineCameras" in run_.stdout   # the call before the reconstruction, a bad angle
    raw = open(out_path, "rb").read()
    par = _lib.PoseParams.from_buffer_copy(raw, 0)
    nv, n_model = struct.unpack_from("<2I", raw, 72)
    pos = 80
    segs = np.frombuffer(raw, np.float64, 6 * n_model, pos).reshape(n_model, 6); pos += 48 * n_model
    line = np.frombuffer(raw, np.uint32, n_model, pos); pos += 4 * n_model
    cam_size = C.sizeof(_lib.Camera)
    by_id = {v.cam: v for v in sc.views}
    cams, obs, got = [], [], dict(cameras=[], summaries=[], associations=[])
    for _ in range(nv):
        cam_id, = struct.unpack_from("<I", raw, pos); pos += 4
        cams.append(api.camera_dict(_lib.Camera.from_buffer_copy(raw, pos))); pos += cam_size
        m, = struct.unpack_from("<I", raw, pos); pos += 4
        got["cameras"].append(api.camera_dict(_lib.Camera.from_buffer_copy(raw, pos))); pos += cam_size
        got["summaries"].append(np.frombuffer(raw, _lib.POSE_SUMMARY_DTYPE, 1, pos)[0]); pos += 88
        got["associations"].append(np.frombuffer(raw, _lib.ASSOCIATION_DTYPE, m, pos)); pos += 24 * m
        obs.append(np.ascontiguousarray(by_id[cam_id].segs, np.float32).reshape(-1, 4))
        assert m == len(obs[-1])
    assert pos == len(raw) and nv == 8 and n_model > 10
    want = P.refine(segs, line, cams, obs, max_distance=par.max_distance, min_cos2=par.min_cos2, min_overlap=par.min_overlap,
                    start_distance=par.start_distance, stall_tolerance=par.stall_tolerance, step_tolerance=par.step_tolerance,
                    near_plane=par.near_plane, max_iterations=par.max_iterations, min_matches=par.min_matches)
    print(run_.stdout.strip().splitlines()[-1], [x["status"] for x in want["summaries"]])
    for k in range(nv):
        Cs.same_camera(got["cameras"][k], want["cameras"][k], f"the facade's camera {k} / the model")
        Cs.same_bytes(got["associations"][k], want["associations"][k], f"the facade's associations {k} / the model")
        sm, w = got["summaries"][k], want["summaries"][k]
        assert (P.STATUS[sm["status"]], sm["iterations"], sm["n_matched"], sm["rms"], sm["last_step"]) == \
            (w["status"], w["iterations"], w["n_matched"], w["rms"], w["last_step"])
        assert sm["q"].tobytes() == w["q"].tobytes() and sm["t"].tobytes() == w["t"].tobytes()


def test_argument_errors_leave_the_outputs_untouched():
    """on a machine with a device as well: no launch, no output"""
    L = _lib.load()
    s = Cs.crossing_scene()
    cams = api.camera_array(s["cams"])
    n_seg = np.array([9], np.uint32)
    outs = [np.full(44, FILL, np.uint32), np.full(22, FILL, np.uint32), np.full(54, FILL, np.uint32), np.full(20 * 98, FILL, np.uint32)]
    before = counters()
    p = _lib.ptr
    for k, v in ((0, -1.0), (3, 1.0), (4, 0.0), (6, 0.0), (7, 0), (8, 5), (9, (1, 0))):
        vals = list(GOOD); vals[k] = v
        par = _lib.PoseParams(*vals)
        assert L.l3d_refine_cameras(0, 9, p(s["segs"]), p(s["line"]), 1, cams, p(n_seg), p(s["obs"][0]), C.byref(par), *[p(o) for o in outs]) == -1
    bad = api.camera_array(s["cams"]); bad[0].K[3] = 0.5
    par = _lib.PoseParams(*GOOD)
    assert L.l3d_refine_cameras(0, 9, p(s["segs"]), p(s["line"]), 1, bad, p(n_seg), p(s["obs"][0]), C.byref(par), *[p(o) for o in outs]) == -1
    assert "upper triangular" in _lib.last_error()
    assert all((o == FILL).all() for o in outs) and counters() == before
