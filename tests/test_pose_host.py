"""Camera poses refined against the 3D line model, as far as it goes without a device: the numpy model of
tests/pose_model.py against itself (scalar / array forms, the tile tree), hand cases from small integers, the recovery
figures of §27 measured with the model, and the library's exports, layouts, argument checks and empty forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from tests import associate_model as AM
from tests import pose_cases as Cs
from tests import pose_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A5A5A5A
# measured with the model: per synthetic scene the iterations of the slowest camera, the largest rotation error
# in degrees and the largest error of the camera centre as a share of the distance to the scene
MEASURED = dict(plain=(9, 5.5e-3, 1.1e-4), noisy=(9, 1.1e-2, 2.4e-4), shifted=(9, 5.5e-3, 1.1e-4))
# the real fixture from 0.1 deg / 0.2 % of the median depth off, the gate from 10: iterations of the slowest of the 26 cameras
MEASURED_REAL = dict(tenth=11, fifth=16)
REAL_SUBSET = [0, 5, 11, 17, 22, 25]


def one_association(segment):
    a = AM.nothing(1)
    a[0] = (0, 0, segment, 0.0, 1.0, 1)
    return a


def test_scalar_and_array_forms_agree_byte_for_byte():
    s = Cs.edge_scene(65, 40)
    kw = dict(start_distance=10.0, max_iterations=4, min_matches=6)
    a = P.refine(s["segs"], s["line"], s["cams"], s["obs"], form="scalar", **kw)
    b = P.refine(s["segs"], s["line"], s["cams"], s["obs"], form="array", **kw)
    Cs.same_result(a, b, "scalar / array")
    assert a["summaries"][0]["iterations"] == 4 and a["summaries"][0]["n_matched"] > 30 and a["trace"][0]["delta"].all()
    # the tile tree against a plain walk of it, past two tiles
    rng = np.random.default_rng(1)
    terms = rng.normal(size=(515, P.TERMS)) * 10.0 ** rng.integers(-8, 8, (515, 1))
    Cs.same_bytes(P.tile_sums(terms), P.tile_sums_walk(terms), "tile tree")
    assert P.tile_sums(terms).shape == (3, P.TERMS)


def test_a_segment_on_its_lines_projection_has_no_gradient():
    """the 3D segment (-1, 0, 2) - (1, 0, 2) projects onto the row y = 64; a 2D segment on that row has r = 0 at both ends"""
    M = P.inverse_transpose(Cs.HAND_K)
    model = np.array([[-1.0, 0.0, 2.0, 1.0, 0.0, 2.0]])
    for form in ("scalar", "array"):
        t = P.segment_terms(M, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0), model,
                            np.array([[40.0, 64.0, 80.0, 64.0]], np.float32), one_association(0), form)[0]
        assert (t[21:28] == 0.0).all() and t[28] == 1.0 and t[0] > 0.0


def test_a_displaced_segment_by_hand():
    """K = (64, 0, 64; 0, 64, 64; 0, 0, 1), R = I, t = 0; the 3D segment Y1 = (-1, 0, 2), Y2 = (1, 0, 2): N = Y1 x Y2 =
    (0, 4, 0), D = (2, 0, 0).  K^-T = (1/64, 0, 0; 0, 1/64, 0; -1, -1, 1): lambda = (0, 1/16, -4), the row y = 64, nu =
    1/16.  The 2D segment (40, 67) - (80, 67): u = 67/16 - 4 = 3/16, r = u / nu = 3 at both ends, cost = 2 x 9 = 18.
    Column 4 (shift along y): dN = e_1 x D = (0, 0, -2), dlambda = (0, 0, -2), B = 0, J_4 = -2 / nu = -32 (a shift of
    tau moves the row by f / Z = 32 tau pixels): H_44 = 2 x 1024 = 2048, b_4 = 2 x (-32 x 3) = -192.  Column 0 (rotation
    about x): dN = e_0 x N = (0, 0, 4), J_0 = 4 / nu = 64: H_00 = 8192, H_04 = 2 x 64 x (-32) = -4096.  Column 3 (shift
    along the line): dN = e_0 x D = 0, J_3 = 0: row and column 3 are 0."""
    M = P.inverse_transpose(Cs.HAND_K)
    assert M == (1.0 / 64.0, 0.0, 1.0 / 64.0, -1.0, -1.0)
    model = np.array([[-1.0, 0.0, 2.0, 1.0, 0.0, 2.0]])
    for form in ("scalar", "array"):
        t = P.segment_terms(M, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0), model,
                            np.array([[40.0, 67.0, 80.0, 67.0]], np.float32), one_association(0), form)[0]
        assert t[27] == 18.0 and t[28] == 1.0
        assert t[P.ROW[4]] == 2048.0 and t[21 + 4] == -192.0
        assert t[P.ROW[0]] == 8192.0 and t[P.ROW[0] + 4] == -4096.0 and t[21] == 384.0
        assert t[P.ROW[3]] == 0.0 and t[P.ROW[0] + 3] == 0.0 and t[21 + 3] == 0.0
    # a record that names a segment past the model, or none, contributes nothing
    none = P.segment_terms(M, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0), model,
                           np.array([[40.0, 67.0, 80.0, 67.0]], np.float32), one_association(1))[0]
    assert not none.any()


def test_parallel_lines_are_degenerate_with_a_pivot_of_exactly_zero():
    """nine lines along x: the shift along x moves no image line, column 3 of every term is 0 bit for bit, and so is the
    fourth pivot"""
    s = Cs.parallel_scene()
    for form in ("scalar", "array"):
        r = P.refine(s["segs"], s["line"], s["cams"], s["obs"], min_matches=6, form=form)
        sm, tr = r["summaries"][0], r["trace"][0]
        assert (sm["status"], sm["iterations"], sm["n_matched"]) == ("DEGENERATE", 1, 9)
        sums = tr["sums"][0]
        assert sums[P.ROW[3]] == 0.0 and all(sums[P.ROW[i] + 3 - i] == 0.0 for i in range(3)) and sums[24] == 0.0
        assert all(sums[P.ROW[i]] > 0.0 for i in (0, 1, 2, 4, 5)) and not tr["delta"].any()
        Cs.same_camera(r["cameras"][0], s["cams"][0], "degenerate: the camera comes back")
        assert P.solve(sums) is None


def test_too_few_matches_return_the_camera_bit_for_bit():
    s = Cs.crossing_scene()
    R = np.eye(3); R[0, 1] = -0.0; R[2, 0] = -0.0                      # (signed zeros survive: the camera is copied, not recomputed)
    cams = [Cs.hand_camera(R)]
    few = P.refine(s["segs"], s["line"], cams, s["obs"], min_matches=10)
    assert (few["summaries"][0]["status"], few["summaries"][0]["iterations"], few["trace"][0]["n_matched"][0]) == ("TOO_FEW", 1, 9)
    Cs.same_camera(few["cameras"][0], cams[0], "too few")
    assert np.signbit(few["cameras"][0]["R"][0, 1]) and few["summaries"][0]["n_matched"] == 9
    # with nine allowed: every segment lies on its line, the step is exactly 0
    enough = P.refine(s["segs"], s["line"], cams, s["obs"], min_matches=9)
    sm = enough["summaries"][0]
    assert (sm["status"], sm["iterations"], sm["n_matched"], sm["rms"], sm["last_step"]) == ("CONVERGED", 1, 9, 0.0, 0.0)
    assert (enough["associations"][0]["segment"] == np.arange(9)).all()


@pytest.mark.parametrize("name", list(Cs.RECOVERY))
def test_recovery_on_the_model(name):
    s = Cs.recovery_scene(**Cs.RECOVERY[name])
    r = P.refine(s["segs"], s["line"], s["cams"], s["obs"], **s["par"])
    angle, centre = Cs.pose_errors(r["cameras"], s["truth"], [s["depth"]] * len(s["cams"]))
    its = max(x["iterations"] for x in r["summaries"])
    print(name, its, angle, centre, [(x["status"], x["n_matched"], x["rms"], x["last_step"]) for x in r["summaries"]])
    assert all(x["status"] == "CONVERGED" for x in r["summaries"])
    assert its <= 2 * MEASURED[name][0] and angle <= 10 * MEASURED[name][1] and centre <= 10 * MEASURED[name][2]
    start = Cs.pose_errors(s["cams"], s["truth"], [s["depth"]] * len(s["cams"]))
    assert start[0] > 0.19 and start[1] > 0.019                         # (the start was off by what the scene says)


def test_the_gate_halves_on_a_stall_only():
    s = Cs.recovery_scene()
    r = P.refine(s["segs"], s["line"], s["cams"][:1], s["obs"][:1], **s["par"])
    tr = r["trace"][0]
    step = np.array([P.step_of(list(d), P.bounding_box(s["segs"])[1]) for d in tr["delta"]])
    for k in range(len(tr) - 1):
        want = max(2.5, tr["gate"][k] * 0.5) if step[k] <= 1e-4 else tr["gate"][k]
        assert tr["gate"][k + 1] == want
    assert tr["gate"][0] == 20.0 and tr["gate"][-1] == 2.5 and (np.diff(tr["gate"]) == 0.0).any()


def test_real_cameras_are_recovered_by_the_model():
    """six of the 26 cameras of the fixture (every camera is refined on its own; the whole set takes the model 25 s and is
    measured in DESIGN §27), 0.1 deg / 0.2 % of the median depth off"""
    kw = dict(Cs.REAL["tenth"]); start_distance = kw.pop("start_distance")
    s = Cs.real_scene(**kw)
    sub = REAL_SUBSET
    r = P.refine(s["segs"], s["line"], [s["cams"][i] for i in sub], [s["obs"][i] for i in sub], start_distance=start_distance)
    for k, i in enumerate(sub):
        angle, centre = P.pose_difference(r["cameras"][k], s["fixture"][i], s["depth"][i])
        sm = r["summaries"][k]
        print(i, sm["status"], sm["iterations"], sm["n_matched"], len(s["obs"][i]), sm["rms"], angle, centre)
        assert sm["status"] == "CONVERGED" and sm["iterations"] <= 2 * MEASURED_REAL["tenth"]
        assert angle <= 0.05 and centre <= 1e-3 and sm["n_matched"] >= 0.9 * len(s["obs"][i]) and sm["rms"] < 1.0


# ---- the library's side, as far as it goes without a device -----------------------------------------------------------
def test_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    L = _lib.load()
    for name in ("l3d_refine_cameras", "l3d_refine_view_cameras"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    for name in ("l3d_pose_params", "l3d_pose_summary", "l3d_pose_iteration"):
        assert "typedef struct " + name in hdr
    for name in ("pose_iterations", "pose_normal_launches", "pose_kernel_ns"):
        assert L.l3d_debug_counter(name.encode()) != L.l3d_debug_counter(b"no such counter")
    facade = open(os.path.join(ROOT, "include", "line3dpp", "line3D.h")).read()
    assert re.search(r"\bvoid refineCameras\s*\(", facade)


def test_struct_layouts():
    assert C.sizeof(_lib.PoseParams) == 72
    assert _lib.POSE_SUMMARY_DTYPE.itemsize == 88 and _lib.POSE_SUMMARY_DTYPE == P.SUMMARY_DTYPE
    assert _lib.POSE_ITERATION_DTYPE.itemsize == 392 and _lib.POSE_ITERATION_DTYPE == P.ITERATION_DTYPE
    assert _lib.POSE_STATUS == P.STATUS and P.SUMMARY_DTYPE.names == P.SUMMARY_KEYS
    p = api.pose_params(1.5, 12.0, 5.0, 0.25, 1e-3, 1e-7, 30, 7, 0.5)
    assert (p.max_distance, p.min_cos2, p.min_overlap, p.start_distance, p.stall_tolerance, p.step_tolerance, p.near_plane,
            p.max_iterations, p.min_matches, tuple(p.reserved)) == (1.5, AM.min_cos2_of(5.0), 0.25, 12.0, 1e-3, 1e-7, 0.5, 30, 7, (0, 0))
    d = api.pose_params()
    assert (d.max_distance, d.min_cos2, d.min_overlap, d.start_distance) == (2.5, AM.min_cos2_of(10.0), 0.5, 0.0)
    assert {k: getattr(d, k) for k in P.DEFAULTS} == P.DEFAULTS
    with pytest.raises(ValueError, match="max_angle"):
        api.pose_params(max_angle=91.0)


GOOD = (2.5, 0.97, 0.5, 0.0, 1e-4, 1e-9, 1e-6, 20, 6, (0, 0))


def test_argument_checks_need_no_device():
    """the checks come before any device work: they answer on a machine without a GPU as well"""
    L = _lib.load()
    s = Cs.crossing_scene()
    segs, line, seg4 = s["segs"], s["line"], s["obs"][0]
    cams = api.camera_array(s["cams"])
    n_seg = np.array([9], np.uint32)
    outs = dict(cams=np.full(C.sizeof(_lib.Camera) // 4, FILL, np.uint32), summaries=np.full(22, FILL, np.uint32),
                assoc=np.full(9 * 6, FILL, np.uint32), trace=np.full(256 * 98, FILL, np.uint32))
    p = _lib.ptr

    def untouched():
        return all((x == FILL).all() for x in outs.values())

    def call(par, segs=segs, n=9, cams=cams, seg4=seg4, null=()):
        a = dict(segs=p(segs), line=p(line), cams=cams, n_seg=p(n_seg), seg4=p(seg4), out_cams=p(outs["cams"]), summaries=p(outs["summaries"]))
        for k in null:
            a[k] = None
        rc = L.l3d_refine_cameras(0, n, a["segs"], a["line"], 1, a["cams"], a["n_seg"], a["seg4"], C.byref(par) if par is not None else None,
                                  a["out_cams"], a["summaries"], p(outs["assoc"]), p(outs["trace"]))
        assert untouched()
        return rc, _lib.last_error()

    inf, nan = float("inf"), float("nan")
    for k, name, bad in ((0, "max_distance", (-1.0, inf, nan)), (1, "min_cos2", (-0.1, 1.1, nan)), (2, "min_overlap", (-0.1, 1.1, nan)),
                         (3, "start_distance", (1.0, -1.0, inf, nan)), (4, "stall_tolerance", (0.0, -1e-9, inf, nan)),
                         (5, "step_tolerance", (0.0, -1e-9, inf, nan)), (6, "near plane", (0.0, -1.0, inf, nan)),
                         (7, "max_iterations", (0, 257, 0xFFFFFFFF)), (8, "min_matches", (0, 5)), (9, "reserved", ((1, 0), (0, 1)))):
        for v in bad:
            vals = list(GOOD); vals[k] = v
            rc, msg = call(_lib.PoseParams(*vals))
            assert rc == -1 and name in msg, (name, v, rc, msg)
    rc, msg = call(None)
    assert rc == -1 and "null" in msg
    good = _lib.PoseParams(*GOOD)
    for bad_value in (np.inf, np.nan, -(2.0 ** 101)):
        bad = segs.copy(); bad[2, 4] = bad_value
        rc, msg = call(good, segs=bad)
        assert rc == -1 and "segment 2" in msg, msg
    rc, msg = call(good, n=1 << 30)
    assert rc == -9 and "2^30" in msg
    for k in ("segs", "line", "cams", "n_seg", "seg4", "out_cams", "summaries"):
        rc, msg = call(good, null=(k,))
        assert rc == -1 and "null" in msg, k
    for word, change in (("K must be upper triangular", lambda c: c.K.__setitem__(3, 1e-9)), ("K must be upper triangular", lambda c: c.K.__setitem__(8, 2.0)),
                         ("K must be upper triangular", lambda c: c.K.__setitem__(0, 0.0)), ("K must be upper triangular", lambda c: c.K.__setitem__(7, 1.0)),
                         ("non-finite", lambda c: c.R.__setitem__(4, nan)), ("non-finite", lambda c: c.t.__setitem__(1, inf)),
                         ("zero pixels", lambda c: setattr(c, "width", 0)), ("65535", lambda c: setattr(c, "height", 65536))):
        other = api.camera_array(s["cams"])
        change(other[0])
        rc, msg = call(good, cams=other)
        assert rc in (-1, -9) and word in msg and "camera 0" in msg, (word, rc, msg)
    bad4 = seg4.copy(); bad4[2, 1] = np.nan
    rc, msg = call(good, seg4=bad4)
    assert rc == -1 and "camera 0" in msg and "segment 2" in msg
    point = np.tile(np.array([[1.0, 2.0, 3.0, 1.0, 2.0, 3.0]]), (9, 1))
    rc, msg = call(good, segs=point)
    assert rc == -1 and "bounding box" in msg
    # the context form checks its arguments first as well
    off = np.full(2, FILL, np.uint64)
    assert L.l3d_refine_view_cameras(None, 0, None, C.byref(good), None, None, p(off), None, None) == -1 and "null" in _lib.last_error()
    assert untouched() and (off == FILL).all()


def test_empty_forms_need_no_device():
    s = Cs.crossing_scene()
    none = np.zeros((0, 4), np.float32)
    for what, segs, line, cams, obs in (("an empty model", s["segs"][:0], s["line"][:0], s["cams"] * 2, [s["obs"][0], none]),
                                        ("no camera", s["segs"], s["line"], [], []),
                                        ("cameras without segments", s["segs"], s["line"], s["cams"] * 2, [none, none])):
        got = api.refine_cameras(segs, line, cams, obs)
        Cs.same_result(got, P.refine(segs, line, cams, obs), what)
        for sm, tr, a in zip(got["summaries"], got["trace"], got["associations"]):
            assert sm["status"] == "TOO_FEW" and sm["iterations"] == 0 and len(tr) == 0 and (a["record"] == -1).all()
            assert tuple(sm["q"]) == (1.0, 0.0, 0.0, 0.0) and not sm["t"].any()
