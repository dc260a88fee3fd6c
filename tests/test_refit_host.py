"""The refit of the 3D lines against cameras and their 2D segments, as far as it goes without a device: the host
hooks l3d_refit_span and l3d_refit_sweep -- the span function the device runs and the sweep of stage 9 -- against
tests/refit_model.py on hand cases, the exports, declarations and struct sizes, every refusal with its message, the forms
that need no launch, and the recovery figures of the numpy model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from tests import associate_model as AM
from tests import pose_cases as PC
from tests import refit_cases as RC
from tests import refit_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A5A5A5A
p = _lib.ptr


def lib_span(cam, seg4, M, u, Q):
    L = _lib.load()
    arr = api.camera_array([cam])
    lo, hi = C.c_double(7.0), C.c_double(7.0)
    seg = np.asarray(seg4, np.float32); M = np.asarray(M, np.float64); u = np.asarray(u, np.float64); Q = np.asarray(Q, np.float64)
    rc = L.l3d_refit_span(arr, p(seg), p(M), p(u), p(Q), C.byref(lo), C.byref(hi))
    assert rc in (0, 1)
    return lo.value, hi.value, rc


def lib_sweep(lo, hi, cam, visibility, min_length, u_norm):
    L = _lib.load()
    lo = np.asarray(lo, np.float64); hi = np.asarray(hi, np.float64); cam = np.asarray(cam, np.uint32)
    out = np.zeros(2 * max(len(lo), 1)); n = C.c_uint32(99)
    rc = L.l3d_refit_sweep(len(lo), p(lo), p(hi), p(cam), visibility, min_length, u_norm, p(out), C.byref(n))
    assert rc == 0, _lib.last_error()
    return [tuple(out[2 * k:2 * k + 2]) for k in range(n.value)]


# ---- the span hook -----------------------------------------------------------------------------------------------------
def test_span_by_hand():
    cam = PC.hand_camera()
    M, u, Q = (0.0, 0.0, 2.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    # the pixel (96, 64) looks along (0.5, 0, 1): it meets the line at x = 1; the pixel (64, 64) at x = 0
    assert lib_span(cam, (96.0, 64.0, 64.0, 64.0), M, u, Q) == (0.0, 1.0, 1)
    assert lib_span(cam, (64.0, 64.0, 96.0, 64.0), M, u, Q) == (0.0, 1.0, 1)
    assert lib_span(cam, (96.0, 64.0, 96.0, 64.0), M, u, Q) == (1.0, 1.0, 1)
    # A line along z through the camera centre.  The issue for this stage expected "invalid for every pixel"; by the rule
    # it states itself (valid iff den > 1e-12 a cc, the reference's test) only the ray ALONG the line is invalid: den =
    # |u x v|^2 = xn^2 + yn^2 is 0 for the principal point alone.  Every other ray meets the line in the centre, s = -2
    # exactly for both end points, a span without length, of which the sweep keeps nothing: the line gets no extent
    # either way.  What the rule gives is asserted, and that nothing is kept.
    z = (0.0, 0.0, 1.0)
    assert lib_span(cam, (64.0, 64.0, 64.0, 64.0), M, z, Q) == (0.0, 0.0, 0)
    assert lib_span(cam, (64.0, 64.0, 96.0, 64.0), M, z, Q) == (0.0, 0.0, 0)           # (one end point invalid)
    spans = [lib_span(cam, seg, M, z, Q) for seg in ((96.0, 64.0, 64.0, 96.0), (0.0, 0.0, 128.0, 1.0), (10.0, 20.0, 30.0, 40.0))]
    assert spans == [(-2.0, -2.0, 1)] * 3
    assert lib_sweep([s[0] for s in spans], [s[1] for s in spans], [0, 1, 2], 1, 0.0, 1.0) == []
    # a carrier that is a point
    assert lib_span(cam, (10.0, 20.0, 30.0, 40.0), M, (0.0, 0.0, 0.0), Q) == (0.0, 0.0, 0)


def test_span_equals_the_model_at_tolerance_zero():
    rng = np.random.default_rng(3)
    s = RC.small()
    c = (0.1, -0.2, 0.05)
    n = 0
    for cam, obs in zip(s["cams"], s["obs"]):
        cam16 = RM.lo_camera(cam, c)
        for seg in obs[:60]:
            M = rng.uniform(-1, 1, 3); u = rng.normal(size=3)
            want = RM.span(cam16, seg, M, u)
            got = lib_span(cam, seg, M, u, cam16[9:12])
            assert np.array(got[:2]).tobytes() == np.array(want[:2]).tobytes() and got[2] == want[2]
            n += got[2]
    assert n > 100
    assert _lib.load().l3d_refit_span(None, None, None, None, None, None, None) == -1


# ---- the sweep hook ----------------------------------------------------------------------------------------------------
SWEEPS = dict(
    three_of_three=(([0.0, 0.2, 0.1], [1.0, 0.9, 1.2], [0, 1, 2]), 3, 0.0, [(0.2, 0.9)]),
    two_of_three=(([0.0, 0.2], [1.0, 0.9], [0, 1]), 3, 0.0, []),
    one_camera_counts_once=(([0.0, 0.1, 0.2], [1.0, 0.9, 0.8], [0, 0, 1]), 3, 0.0, []),
    one_camera_twice_and_two_more=(([0.0, 0.5, 0.1, 0.2], [0.6, 1.0, 0.9, 0.8], [0, 0, 1, 2]), 3, 0.0, [(0.2, 0.8)]),
    touching_spans_join=(([0.0, 0.5, 0.0, 0.0], [0.5, 1.0, 1.0, 1.0], [0, 0, 1, 2]), 3, 0.0, [(0.0, 1.0)]),
    a_gap_makes_two=(([0.0, 0.6, 0.0, 0.0], [0.4, 1.0, 1.0, 1.0], [0, 0, 1, 2]), 3, 0.0, [(0.0, 0.4), (0.6, 1.0)]),
    min_length_met=(([0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0, 1, 2]), 3, 1.0, [(0.0, 0.5)]),
    min_length_missed=(([0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0, 1, 2]), 3, 1.0000001, []),
    visibility_one=(([0.0, 2.0], [1.0, 3.0], [5, 5]), 1, 0.0, [(0.0, 1.0), (2.0, 3.0)]),
    equal_s_everywhere=(([0.25, 0.25, 0.25], [0.25, 0.25, 0.25], [0, 1, 2]), 3, 0.0, []),
    nothing=(([], [], []), 3, 0.0, []),
)


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_sweep_by_hand(name):
    (lo, hi, cam), vis, min_length, want = SWEEPS[name]
    u_norm = 2.0                                    # (so that min_length 1 is exactly the piece of 0.5)
    assert RM.sweep(lo, hi, cam, vis, min_length, u_norm) == want
    assert lib_sweep(lo, hi, cam, vis, min_length, u_norm) == want


def test_sweep_equals_the_model_on_random_spans():
    rng = np.random.default_rng(9)
    for k in range(200):
        n = int(rng.integers(1, 30))
        lo = np.round(rng.uniform(0, 1, n), 1); hi = lo + np.round(rng.uniform(0, 0.5, n), 1)       # (many ties)
        cam = rng.integers(0, 5, n)
        vis = int(rng.integers(1, 5)); ml = float(rng.choice([0.0, 0.1, 0.3]))
        assert lib_sweep(lo, hi, cam, vis, ml, 1.0) == RM.sweep(lo, hi, cam, vis, ml, 1.0), k
    L = _lib.load()
    n = C.c_uint32()
    one = np.zeros(2)
    for args, word in (((1, p(one), p(one), p(np.zeros(1, np.uint32)), 0, 0.0, 1.0, p(one), C.byref(n)), "visibility"),
                       ((1, p(one), p(one), p(np.zeros(1, np.uint32)), 1, -1.0, 1.0, p(one), C.byref(n)), "min_length"),
                       ((1, p(one), p(one), p(np.zeros(1, np.uint32)), 1, 0.0, float("nan"), p(one), C.byref(n)), "u_norm"),
                       ((1, None, p(one), p(np.zeros(1, np.uint32)), 1, 0.0, 1.0, p(one), C.byref(n)), "null")):
        assert L.l3d_refit_sweep(*args) == -1 and word in _lib.last_error()


# ---- the library's side, as far as it goes without a device -----------------------------------------------------------
def test_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    L = _lib.load()
    for name in ("l3d_refit_segments", "l3d_refit_view_lines", "l3d_refit_counts", "l3d_refit_get", "l3d_refit_close", "l3d_refit_span",
                 "l3d_refit_sweep"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    for name in ("l3d_refit_params", "l3d_refit_line", "l3d_refit_observation", "l3d_refit_summary"):
        assert "typedef struct " + name in hdr
    for name in ("refit_observations", "refit_lines_solved", "refit_kernel_ns"):
        assert L.l3d_debug_counter(name.encode()) != L.l3d_debug_counter(b"no such counter")


def test_struct_layouts():
    assert C.sizeof(_lib.RefitParams) == 64 and C.sizeof(_lib.RefitSummary) == 104
    assert _lib.REFIT_LINE_DTYPE.itemsize == 152 and _lib.REFIT_LINE_DTYPE == RM.LINE_DTYPE
    assert _lib.REFIT_OBSERVATION_DTYPE.itemsize == 32 and _lib.REFIT_OBSERVATION_DTYPE == RM.OBSERVATION_DTYPE
    assert _lib.REFIT_STATUS == RM.STATUS
    q = api.refit_params(1.5, 5.0, 0.25, 0.5, 0.01, 4, 30, True)
    assert (q.max_distance, q.min_cos2, q.min_overlap, q.near_plane, q.min_length, q.visibility, q.max_iterations, q.use_ambiguous,
            tuple(q.reserved)) == (1.5, AM.min_cos2_of(5.0), 0.25, 0.5, 0.01, 4, 30, 1, (0, 0, 0))
    d = api.refit_params()
    assert {k: getattr(d, k) for k in RM.DEFAULTS} == dict(RM.DEFAULTS, use_ambiguous=0)
    with pytest.raises(ValueError, match="max_angle"):
        api.refit_params(max_angle=91.0)


GOOD = (2.5, 0.97, 0.5, 1e-6, 0.0, 3, 50, 0, (0, 0, 0))


def test_argument_checks_need_no_device():
    """the checks come before any device work: they answer on a machine without a GPU as well, and leave *out alone"""
    L = _lib.load()
    s = PC.crossing_scene()
    segs, line, seg4 = s["segs"], s["line"], s["obs"][0]
    cams = api.camera_array(s["cams"])
    n_seg = np.array([9], np.uint32)
    out = np.full(2, FILL, np.uint32)

    def call(par, segs=segs, line=line, n=9, cams=cams, seg4=seg4, null=()):
        a = dict(segs=p(segs), line=p(line), cams=cams, n_seg=p(n_seg), seg4=p(seg4), out=p(out))
        for k in null:
            a[k] = None
        rc = L.l3d_refit_segments(0, n, a["segs"], a["line"], 1, a["cams"], a["n_seg"], a["seg4"], C.byref(par) if par is not None else None,
                                  C.cast(a["out"], C.POINTER(C.c_void_p)) if a["out"] is not None else None)
        assert (out == FILL).all()
        return rc, _lib.last_error()

    inf, nan = float("inf"), float("nan")
    for k, name, bad in ((0, "max_distance", (-1.0, inf, nan)), (1, "min_cos2", (-0.1, 1.1, nan)), (2, "min_overlap", (-0.1, 1.1, nan)),
                         (3, "near plane", (0.0, -1.0, inf, nan)), (4, "min_length", (-1e-9, inf, nan)), (5, "visibility", (0,)),
                         (6, "max_iterations", (1001, 0xFFFFFFFF)), (7, "use_ambiguous", (2,)),
                         (8, "reserved", ((1, 0, 0), (0, 1, 0), (0, 0, 1)))):
        for v in bad:
            vals = list(GOOD); vals[k] = v
            rc, msg = call(_lib.RefitParams(*vals))
            assert rc == -1 and name in msg, (name, v, rc, msg)
    rc, msg = call(None)
    assert rc == -1 and "null" in msg
    good = _lib.RefitParams(*GOOD)
    for bad_value in (np.inf, np.nan, -(2.0 ** 101)):
        bad = segs.copy(); bad[2, 4] = bad_value
        rc, msg = call(good, segs=bad)
        assert rc == -1 and "segment 2" in msg, msg
    rc, msg = call(good, n=1 << 30)
    assert rc == -9 and "2^30" in msg
    high = line.copy(); high[4] = 1 << 31
    rc, msg = call(good, line=high)
    assert rc == -9 and "segment 4" in msg and "2^31" in msg
    for k in ("segs", "line", "cams", "n_seg", "seg4", "out"):
        rc, msg = call(good, null=(k,))
        assert rc == -1 and "null" in msg, k
    for word, change in (("K must be upper triangular", lambda c: c.K.__setitem__(3, 1e-9)), ("K must be upper triangular", lambda c: c.K.__setitem__(8, 2.0)),
                         ("K must be upper triangular", lambda c: c.K.__setitem__(0, 0.0)), ("K must be upper triangular", lambda c: c.K.__setitem__(7, 1.0)),
                         ("K01 must be 0", lambda c: c.K.__setitem__(1, 1e-9)),
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
    assert L.l3d_refit_view_lines(None, 0, None, None, C.byref(good), None, None) == -1 and "null" in _lib.last_error()


def test_empty_forms_need_no_device():
    s = PC.crossing_scene()
    none = np.zeros((0, 4), np.float32)
    line = s["line"].copy(); line[3] = 11                  # (line 3 is empty now, and so are 9 and 10)
    order = np.argsort(line, kind="stable")
    for what, segs, ln, cams, obs in (("an empty model", s["segs"][:0], line[:0], s["cams"] * 2, [s["obs"][0], none]),
                                      ("no camera", s["segs"], line, [], []),
                                      ("cameras without segments", s["segs"], line, s["cams"] * 2, [none, none])):
        got = api.refit_segments(segs, ln, cams, obs)
        n = len(ln)
        assert got["segments"].tobytes() == segs[order[:n]].tobytes() and got["line"].tobytes() == ln[order[:n]].tobytes(), what
        assert len(got["observations"]) == 0 and all((a["record"] == -1).all() for a in got["associations"])
        want = np.array([RM.TOO_FEW_VIEWS] * 12); want[[3, 9, 10]] = RM.EMPTY
        assert got["lines"]["status"].tolist() == (want.tolist() if n else [])
        sm = got["summary"]
        assert sm["n_segments_before"] == sm["n_segments_after"] == n and sm["n_observations"] == 0
        assert sm["status"]["EMPTY"] == (3 if n else 0) and sm["status"]["TOO_FEW_VIEWS"] == (9 if n else 0)
    # a line's segments need not be neighbours: grouped by ascending line index, in input order within a line, bit for bit
    segs = np.random.default_rng(7).uniform(-3.0, 3.0, (5, 6)); ln = np.array([2, 0, 2, 1, 0], np.uint32)
    got = api.refit_segments(segs, ln, [], [])
    assert got["segments"].tobytes() == segs[[1, 4, 3, 0, 2]].tobytes() and got["line"].tolist() == [0, 0, 1, 2, 2]
    assert got["lines"]["status"].tolist() == [RM.TOO_FEW_VIEWS] * 3 and got["lines"]["n_pieces"].tolist() == [2, 1, 2]
    assert got["lines"]["P1"].tobytes() == segs[[1, 3, 0], :3].tobytes() and got["lines"]["P2"].tobytes() == segs[[4, 3, 2], 3:].tobytes()


# ---- the recovery figures of the model -------------------------------------------------------------------------
RECOVERY_MODEL = dict(plain=(0.0, 7.6e-8, 1.5e-7), noisy=(0.3, 1.48e-3, 2.87e-3))      # noise, median, p90 as measured


@pytest.mark.parametrize("name", sorted(RECOVERY_MODEL))
def test_recovery_on_the_model(name):
    """every line turned by 0.5 degrees and moved by 0.01, true cameras, 6 px, visibility 3: all 300 lines are refit, none
    ends above its start cost, and the carriers come back to the truth (the figures are those written into §28)"""
    noise, median, p90 = RECOVERY_MODEL[name]
    s = RC.recovery(noise=noise)
    out = RM.refit(s["segs"], s["line"], s["cams"], s["obs"], **s["par"])
    assert (out["lines"]["status"] == RM.REFIT).all() and len(out["lines"]) == 300
    assert (out["lines"]["cost1"] <= out["lines"]["cost0"]).all()
    err = RC.carrier_errors(out["lines"], s["truth"])
    before = RC.carrier_errors(dict(P1=s["segs"][:, :3], P2=s["segs"][:, 3:]), s["truth"])
    print(f"{name}: median {np.median(before):.3e} -> {np.median(err):.3e}, p90 {np.percentile(err, 90):.3e}, max {err.max():.3e}")
    assert np.median(err) <= 1.05 * median and np.percentile(err, 90) <= 1.05 * p90
