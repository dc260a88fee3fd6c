"""The joint bundle of cameras and 3D lines, as far as it goes without a device: the numpy model of
tests/bundle_model.py on hand cases, its columns against central differences of its own residual, the host hook
l3d_bundle_solve against the model's solve and numpy.linalg.solve, the Schur identity, the shapes the scenes of
tests/bundle_cases.py claim, the exports, declarations and struct sizes, every refusal with its message, and the forms that
need no launch."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from tests import associate_model as AM
from tests import bundle_cases as BC
from tests import bundle_model as BM
from tests import pose_cases as PC
from tests import pose_model as PO
from tests import refit_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A5A5A5A
EPS = 2.0 ** -52
p = _lib.ptr


def lib_solve(S, g):
    n = len(g)
    S = np.ascontiguousarray(S, np.float64); g = np.ascontiguousarray(g, np.float64); d = np.full(max(n, 1), 7.0)
    rc = _lib.load().l3d_bundle_solve(n, p(S), p(g), p(d))
    assert rc in (0, 1)
    return d[:n] if rc == 1 else None


# ---- hand cases on §27's camera K = (64, 0, 64; 0, 64, 64; 0, 0, 1), R = 1, t = 0 -------------------------------------------
def hand_cell(seg2d, AB=(-1.0, 0.0, 2.0, 1.0, 0.0, 2.0)):
    """the 67 sums of the one cell of one camera, one line and one 2D segment (the carrier eligible)"""
    P = BM.Problem()
    P.n_cells, P.n_lines = 1, 1
    P.cell_cam = np.zeros(1, np.int64); P.cell_line = np.zeros(1, np.int64); P.cell_off = np.array([0, 1], np.int64)
    P.is_eligible = np.ones(1, bool)
    P.obs_p = np.array([seg2d], np.float64)
    P.M = np.array([PO.inverse_transpose(PC.hand_camera()["K"])])
    pose = np.array([[1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]])
    return BM.cell_sums(P, pose, np.array([AB]))[0]


def test_hand_case_gives_the_sums_of_the_pose_refinement_times_the_huber_weight():
    """§27's hand case: the 3D segment (-1, 0, 2)-(1, 0, 2) against the 2D segment (40, 67)-(80, 67).  Both end points lie
    3 px off, s = 18 > 4, so every sum carries the weight rho'(18) = 2 / sqrt(18); §27's H_44 = 2048, b_4 = -192 and
    H_00 = 8192 are the sums without it.  The line block from the columns derived by hand: u = (2, 0, 0), k = 1,
    e1 = (0, 0, 1), e2 = (0, -1, 0); moving A along e1 moves its image along the image line (no column), moving it along e2
    moves the image line at P by 7/8 and at Q by 1/4 of 32 px per unit, B's by 1/8 and 3/4"""
    c = hand_cell((40.0, 67.0, 80.0, 67.0))
    w = 2.0 / math.sqrt(18.0)
    H = lambda i, j: c[BM.CC + BM.ROW6[i] + (j - i)]
    assert H(4, 4) == w * 2048.0 and c[BM.BC + 4] == w * -192.0 and H(0, 0) == w * 8192.0
    Hl = lambda i, j: c[BM.LL + BM.ROW4[i] + (j - i)]
    assert Hl(0, 0) == 0.0 and Hl(2, 2) == 0.0 and Hl(0, 1) == 0.0 and Hl(0, 3) == 0.0 and Hl(2, 3) == 0.0
    assert Hl(1, 1) == w * (28.0 ** 2 + 8.0 ** 2) and Hl(3, 3) == w * (4.0 ** 2 + 24.0 ** 2) and Hl(1, 3) == w * (28.0 * 4.0 + 8.0 * 24.0)
    # e2 points against y: the columns of a2, b2 are -7/8, -1/4 and -1/8, -3/4 of the column of tau_y
    assert c[BM.BL + 1] == w * (-28.0 * -3.0 + -8.0 * -3.0) and c[BM.BL + 3] == w * (-4.0 * -3.0 + -24.0 * -3.0)
    assert c[BM.CL + 4 * 4 + 1] == w * (32.0 * -28.0 + 32.0 * -8.0) and c[BM.CL + 4 * 4 + 3] == w * (32.0 * -4.0 + 32.0 * -24.0)
    assert c[BM.RHO] == 4.0 * math.sqrt(18.0) - 4.0 and c[BM.COUNT] == 1.0
    # inside the Huber radius the weight is 1 and the sums are §27's
    c = hand_cell((40.0, 65.0, 80.0, 65.0))
    assert c[BM.CC + BM.ROW6[4]] == 2048.0 and c[BM.BC + 4] == -64.0 and c[BM.RHO] == 2.0


def test_zero_residual_gives_a_zero_right_hand_side():
    c = hand_cell((40.0, 64.0, 80.0, 64.0))
    assert not c[BM.BC:BM.BC + 6].any() and not c[BM.BL:BM.BL + 4].any() and c[BM.RHO] == 0.0
    assert c[BM.CC + BM.ROW6[4]] == 2048.0


def test_basis_rule():
    e1, e2 = BM.basis([0.0, 0.0, 0.0, 2.0, 0.0, 0.0])              # ties: the first index of the smallest |u_k| is 1
    assert [float(v[0]) for v in e1] == [0.0, 0.0, 1.0] and [float(v[0]) for v in e2] == [0.0, -1.0, 0.0]
    rng = np.random.default_rng(3)
    AB = rng.normal(size=(50, 6))
    e1, e2 = (np.array(e).T for e in BM.basis(AB))
    u = AB[:, 3:] - AB[:, :3]
    assert np.abs((e1 * u).sum(1)).max() < 1e-14 and np.abs((e2 * u).sum(1)).max() < 1e-14 and np.abs((e1 * e2).sum(1)).max() < 1e-14
    assert np.abs(np.linalg.norm(e1, axis=1) - 1).max() < 1e-14 and np.abs(np.linalg.norm(e2, axis=1) - 1).max() < 1e-14


# ---- every column against central differences of the model's own residual ---------------------------------------------
def residual_of(cam, state, AB, seg2d):
    R, tc = PO.pose_about_centre(cam, state)
    M = PO.inverse_transpose(cam["K"])
    one = lambda t: tuple(np.array([float(v)]) for v in t)
    e1, e2 = BM.basis(AB)
    ok, rp, rq, JP, JQ = BM.residuals(one(M), one(R), one(tc), one(AB), e1, e2, one(seg2d))
    assert ok[0]
    return np.array([rp[0], rq[0]]), np.array([[j[0] for j in JP], [j[0] for j in JQ]])


def test_columns_equal_central_differences():
    """h = 1e-5: the truncation error of a central difference is h^2 / 6 times the third derivative, the rounding error
    eps / h times the residual; with derivatives and residuals of the order of the columns themselves the bound is
    (1e3 h^2 + 1e3 eps / h) x max(|J|, |r|, 1)"""
    h = 1e-5
    s = BC.ring(12, 3, cam_degrees=0.3, line_degrees=1.0)
    c, _ = PO.bounding_box(s["segs"])
    worst = 0.0
    for l in range(12):
        cam = s["cams"][l % 3]
        st = PO.State(cam, c, 0.0)
        AB = np.array([float(v) - c[k % 3] for k, v in enumerate(s["segs"][l])])
        seg = s["obs"][l % 3][l].astype(np.float64)
        r0, J = residual_of(cam, st, AB, seg)
        tol = (1e3 * h * h + 1e3 * EPS / h) * max(float(np.abs(J).max()), float(np.abs(r0).max()), 1.0)
        e1, e2 = (np.array([float(v[0]) for v in e]) for e in BM.basis(AB))
        for i in range(10):
            r = []
            for sign in (1.0, -1.0):
                t = BM._copy_state(st); ab = AB.copy()
                if i < 6:
                    d = [0.0] * 6; d[i] = sign * h
                    PO.update(t, d)
                else:
                    e = e1 if i in (6, 8) else e2
                    o = 0 if i < 8 else 3
                    ab[o:o + 3] = ab[o:o + 3] + sign * h * e
                r.append(residual_of(cam, t, ab, seg)[0])
            fd = (r[0] - r[1]) / (2.0 * h)
            worst = max(worst, float(np.abs(fd - J[:, i]).max()) / tol)
            assert np.abs(fd - J[:, i]).max() <= tol, (l, i, fd, J[:, i], tol)
    print("largest difference over its bound:", worst)


# ---- the dense solve ----------------------------------------------------------------------------------------------------
def systems():
    for name in ("63 eligible lines", "two groups of cameras that share no line", "one camera fixed", "a camera without segments, one that matches nothing"):
        s = BC.CASES[name]()
        out = BM.bundle(s["segs"], s["line"], s["cams"], s["obs"], fixed=s["fixed"], **BC.model_par(capture_iteration=1, **s["par"]))
        yield name, out["system"], out["rhs"]


SOLVE_TOLERANCE = 0.04                          # x cond(S) x eps, relative to |delta|inf: ten times the 0.0037 measured here


def test_solve_hook_equals_the_model_and_numpy():
    worst = 0.0
    for name, S, g in systems():
        full = S + np.triu(S, 1).T
        d_lib, d_model = lib_solve(S, g), BM.dense_solve(S, g)
        assert d_lib is not None and d_lib.tobytes() == d_model.tobytes(), name
        d_np = np.linalg.solve(full, -g)
        cond = float(np.linalg.cond(full))
        err = float(np.abs(d_lib - d_np).max() / np.abs(d_np).max())
        print(f"{name}: n {len(g)}, cond {cond:.3e}, error {err:.3e} = {err / (cond * EPS):.3f} x cond x eps")
        worst = max(worst, err / (cond * EPS))
        assert err <= SOLVE_TOLERANCE * cond * EPS
    print("worst:", worst)
    # a pivot that is not positive is reported, delta untouched; so is one that is not finite
    for bad in (-1.0, 0.0, float("nan"), float("inf")):
        S = np.eye(3); S[1, 1] = bad
        assert lib_solve(S, np.ones(3)) is None and BM.dense_solve(S, np.ones(3)) is None
    assert _lib.load().l3d_bundle_solve(2, None, None, None) == -1
    assert _lib.load().l3d_bundle_solve(0, None, None, None) == 1


def test_schur_identity():
    """on a small scene the step of the reduced system equals the cameras' part of the step of the full (6 C + 4 L) system"""
    s = BC.ring(10, 3)
    par = BC.model_par(**s["par"])
    P = BC.problem(s)
    states = [PO.State(cam, P.c, 0.0) for cam in s["cams"]]
    pose = BM.pose_table(s["cams"], states)
    mu = 1e-4
    cells = BM.cell_sums(P, pose, P.AB)
    ok, L, v, W = BM.line_factors(P, cells, mu)
    S, g = BM.reduce_system(P, cells, ok, v, W, mu)
    F, E = len(P.free_cam), len(P.eligible)
    assert F == 3 and E >= 5 and ok[P.eligible].all()
    n = 6 * F + 4 * E
    H = np.zeros((n, n)); b = np.zeros(n)
    sym6 = lambda t: np.array([[t[BM.ROW6[min(i, j)] + abs(i - j)] for j in range(6)] for i in range(6)])
    sym4 = lambda t: np.array([[t[BM.ROW4[min(i, j)] + abs(i - j)] for j in range(4)] for i in range(4)])
    for cell in range(P.n_cells):
        f = int(P.cam_free[P.cell_cam[cell]]); l = int(P.cell_line[cell])
        H[6 * f:6 * f + 6, 6 * f:6 * f + 6] += sym6(cells[cell, BM.CC:BM.CC + 21]); b[6 * f:6 * f + 6] += cells[cell, BM.BC:BM.BC + 6]
        if not P.is_eligible[l]:
            continue
        e = 6 * F + 4 * int(np.searchsorted(P.eligible, l))
        cl = cells[cell, BM.CL:BM.CL + 24].reshape(6, 4)
        H[6 * f:6 * f + 6, e:e + 4] += cl; H[e:e + 4, 6 * f:6 * f + 6] += cl.T
        H[e:e + 4, e:e + 4] += sym4(cells[cell, BM.LL:BM.LL + 10]); b[e:e + 4] += cells[cell, BM.BL:BM.BL + 4]
    H = H + mu * np.diag(np.diag(H))
    full = np.linalg.solve(H, -b)
    reduced = BM.dense_solve(S, g)
    cond = float(np.linalg.cond(H))
    err = float(np.abs(reduced - full[:6 * F]).max() / np.abs(full).max())
    print(f"cond {cond:.3e}, error {err:.3e} = {err / (cond * EPS):.3f} x cond x eps")
    assert err <= SOLVE_TOLERANCE * cond * EPS
    AB_t, dl = BM.update_lines(P, P.AB, ok, L, v, W, reduced.reshape(-1, 6))
    err_l = float(np.abs(dl[P.eligible].reshape(-1) - full[6 * F:]).max() / np.abs(full).max())
    assert err_l <= SOLVE_TOLERANCE * cond * EPS


# ---- the scenes have the shapes they claim --------------------------------------------------------------------------------
def test_cases_have_the_shapes_they_claim():
    cells_of = lambda P: (P.cam_cell_off[1:] - P.cam_cell_off[:-1]).tolist()
    for n in (1, 63, 64, 65, 255, 256, 257):
        P = BC.problem(BC.CASES["1 line x 2 cameras" if n == 1 else f"{n} eligible lines"]())
        assert len(P.eligible) == n == P.n_lines
    for n in (64, 65):
        assert cells_of(BC.problem(BC.CASES[f"a camera with {n} cells"]()))[0] == n
    P = BC.problem(BC.fan())
    assert P.n_cams == 65 and len(P.free_cam) == 65 and P.lines["n_views"].tolist() == [0, 1, 16, 17, 64, 65]
    P = BC.problem(BC.split_cells())
    assert sorted(set((P.cell_off[1:] - P.cell_off[:-1]).tolist())) == [1, 2, 3]
    P = BC.problem(BC.disjoint())
    assert not ((P.slot[:, :3] >= 0).any(1) & (P.slot[:, 3:] >= 0).any(1)).any() and min(cells_of(P)) > 5
    s = BC.odd_cameras()
    P = BC.problem(s)
    assert len(s["obs"][1]) == 0 and len(s["obs"][3]) > 0 and cells_of(P)[1] == 0 and cells_of(P)[3] == 0 and P.free_cam.tolist() == [0, 2, 4]
    for n in (4095, 4096, 4097):
        assert sum(len(o) for o in BC.many_segments(n)["obs"]) == n
    P = BC.problem(BC.held_among_eligible())
    held = (P.lines["n_views"] > 0) & ~P.is_eligible
    assert held.sum() >= 8 and P.is_eligible.sum() >= 16
    assert len(BC.problem(BC.with_fixed({1})).free_cam) == 3 and len(BC.problem(BC.with_fixed({0, 1, 2, 3})).free_cam) == 0
    P = BC.problem(BC.CASES["no eligible line"]())
    assert len(P.eligible) == 0 and len(P.free_cam) == 3
    for flag in (True, False):
        s = BC.CASES["ambiguous segments used" if flag else "ambiguous segments left out"]()
        assoc = RM.associations(s["segs"], s["line"], s["cams"], s["obs"], BC.model_par(**s["par"]))
        assert sum(int(((a["record"] >= 0) & (a["n_accepted"] > 1)).sum()) for a in assoc) >= 5


def test_reject_and_pivot_scenes():
    s = BC.reject()
    out = BM.bundle(s["segs"], s["line"], s["cams"], s["obs"], **BC.model_par(**s["par"]))
    acc = out["trace"]["accepted"]
    assert (acc == 0).sum() >= 1 and (acc == 1).sum() >= 1 and (out["trace"]["solved"] == 1).all()
    s = BC.pivot()
    out = BM.bundle(s["segs"], s["line"], s["cams"], s["obs"], fixed=s["fixed"], **BC.model_par(**s["par"]))
    assert out["trace"]["n_held_for_step"].max() >= 1 and out["summary"]["n_free_cameras"] == 0 and out["summary"]["accepted_steps"] >= 1


def test_untouched_parts_of_the_model_result():
    s = BC.held_among_eligible()
    out = BM.bundle(s["segs"], s["line"], s["cams"], s["obs"], **BC.model_par(**s["par"]))
    for l in np.flatnonzero(out["lines"]["status"] != BM.BUNDLED):
        assert out["segments"][out["line"] == l].tobytes() == s["segs"][s["line"] == l].tobytes()
    s = BC.with_fixed({0, 2})
    out = BM.bundle(s["segs"], s["line"], s["cams"], s["obs"], fixed=s["fixed"], **BC.model_par(**s["par"]))
    for k in (0, 2):
        PC.same_camera(out["cameras"][k], s["cams"][k], f"fixed camera {k}")
    assert out["summary"]["cost1"] < out["summary"]["cost0"]


def test_transform_cameras_keeps_the_projections():
    s = BC.ring(8, 3)
    sim = dict(scale=1.7, q=np.array([0.9, 0.1, -0.3, 0.2]) / np.linalg.norm([0.9, 0.1, -0.3, 0.2]), t=np.array([0.3, -2.0, 5.0]))
    cams = api.transform_cameras(s["cams"], sim)
    Rs = np.array(PO.rotation(tuple(float(v) for v in sim["q"]))).reshape(3, 3)
    X = s["segs"][:, :3]
    X2 = sim["scale"] * X @ Rs.T + sim["t"]
    for a, b in zip(s["cams"], cams):
        pa, _ = PC.project_exact(a, X); pb, _ = PC.project_exact(b, X2)
        assert np.abs(pa - pb).max() < 1e-8
    want = BM.transform_cameras(s["cams"], sim["scale"], Rs, sim["t"])
    for a, b in zip(cams, want):
        assert np.abs(a["R"] - b["R"]).max() < 1e-15 and np.abs(a["t"] - b["t"]).max() < 1e-14


# ---- the library's side, as far as it goes without a device -----------------------------------------------------------
def test_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    L = _lib.load()
    for name in ("l3d_bundle_segments", "l3d_bundle_view_lines", "l3d_bundle_counts", "l3d_bundle_get", "l3d_bundle_close", "l3d_bundle_solve"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    for name in ("l3d_bundle_params", "l3d_bundle_line", "l3d_bundle_iteration", "l3d_bundle_summary"):
        assert "typedef struct " + name in hdr
    for name in ("bundle_iterations", "bundle_rejected_steps", "bundle_kernel_ns"):
        assert L.l3d_debug_counter(name.encode()) != L.l3d_debug_counter(b"no such counter")
    for name in ("bundle_params", "bundle_segments", "bundle_model", "transform_cameras"):
        assert callable(getattr(api, name))
    assert callable(api.Line3D.bundleModel)


def test_struct_layouts():
    assert C.sizeof(_lib.BundleParams) == 104 and C.sizeof(_lib.BundleSummary) == 144
    assert _lib.BUNDLE_LINE_DTYPE.itemsize == 64 and _lib.BUNDLE_LINE_DTYPE == BM.LINE_DTYPE
    assert _lib.BUNDLE_ITERATION_DTYPE.itemsize == 56 and _lib.BUNDLE_ITERATION_DTYPE == BM.ITERATION_DTYPE
    assert _lib.BUNDLE_LINE_STATUS == BM.LINE_STATUS and _lib.BUNDLE_STATUS == BM.STATUS
    d = api.bundle_params()
    assert {k: getattr(d, k) for k in BM.DEFAULTS} == dict(BM.DEFAULTS, use_ambiguous=0)
    assert tuple(d.reserved) == (0, 0, 0, 0)
    with pytest.raises(ValueError, match="max_angle"):
        api.bundle_params(max_angle=91.0)


GOOD = (2.5, 0.97, 0.5, 1e-6, 0.0, 1e-4, 1e-9, 1e8, 1e-6, 3, 10, 0, 0, (0, 0, 0, 0))


def test_argument_checks_need_no_device():
    """the checks come before any device work: they answer on a machine without a GPU as well, and leave *out alone"""
    L = _lib.load()
    s = PC.crossing_scene()
    segs, line, seg4 = s["segs"], s["line"], s["obs"][0]
    cams = api.camera_array(s["cams"])
    n_seg = np.array([9], np.uint32)
    out = np.full(2, FILL, np.uint32)

    def call(par, segs=segs, line=line, n=9, cams=cams, seg4=seg4, fixed=None, n_cams=1, n_seg=n_seg, null=()):
        a = dict(segs=p(segs), line=p(line), cams=cams, n_seg=p(n_seg), seg4=p(seg4), out=p(out))
        for k in null:
            a[k] = None
        rc = L.l3d_bundle_segments(0, n, a["segs"], a["line"], n_cams, a["cams"], p(fixed) if fixed is not None else None, a["n_seg"], a["seg4"],
                                   C.byref(par) if par is not None else None,
                                   C.cast(a["out"], C.POINTER(C.c_void_p)) if a["out"] is not None else None)
        assert (out == FILL).all()
        return rc, _lib.last_error()

    inf, nan = float("inf"), float("nan")
    for k, name, bad in ((0, "max_distance", (-1.0, inf, nan)), (1, "min_cos2", (-0.1, 1.1, nan)), (2, "min_overlap", (-0.1, 1.1, nan)),
                         (3, "near plane", (0.0, -1.0, inf, nan)), (4, "min_length", (-1e-9, inf, nan)),
                         (5, "initial_damping", (1e-10, 1e9, nan)), (6, "min_damping", (0.0, -1.0, inf, nan)),
                         (7, "max_damping", (1e-10, inf, nan)), (8, "function_tolerance", (-1e-9, inf, nan)), (9, "visibility", (0,)),
                         (10, "max_iterations", (257, 0xFFFFFFFF)), (11, "use_ambiguous", (2,)), (12, "capture_iteration", (257,)),
                         (13, "reserved", ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)))):
        for v in bad:
            vals = list(GOOD); vals[k] = v
            rc, msg = call(_lib.BundleParams(*vals))
            assert rc == -1 and name in msg, (name, v, rc, msg)
    rc, msg = call(None)
    assert rc == -1 and "null" in msg
    good = _lib.BundleParams(*GOOD)
    bad = segs.copy(); bad[2, 4] = np.nan
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
    for word, change in (("K must be upper triangular", lambda c: c.K.__setitem__(3, 1e-9)), ("K01 must be 0", lambda c: c.K.__setitem__(1, 1e-9)),
                         ("non-finite", lambda c: c.R.__setitem__(4, nan)), ("zero pixels", lambda c: setattr(c, "width", 0))):
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
    rc, msg = call(good, fixed=np.array([2, 0], np.uint8))
    assert rc == -1 and "fixed must be 0 or 1" in msg
    # more than 512 cameras that are not fixed: the limit; 513 of which one is fixed pass it (and stop at the next check)
    many = api.camera_array(s["cams"] * 513)
    counts = np.zeros(514, np.uint32); counts[0] = 9
    rc, msg = call(good, cams=many, n_cams=513, n_seg=counts)
    assert rc == -9 and "512 free cameras" in msg
    fx = np.zeros(514, np.uint8); fx[7] = 1
    rc, msg = call(good, cams=many, n_cams=513, n_seg=counts, fixed=fx, segs=point)
    assert rc == -1 and "bounding box" in msg
    assert L.l3d_bundle_view_lines(None, 0, None, None, None, C.byref(good), None, None) == -1 and "null" in _lib.last_error()


def test_empty_forms_need_no_device():
    s = PC.crossing_scene()
    none = np.zeros((0, 4), np.float32)
    line = s["line"].copy(); line[3] = 11                  # (line 3 is empty now, and so are 9 and 10)
    order = np.argsort(line, kind="stable")
    for what, segs, ln, cams, obs in (("an empty model", s["segs"][:0], line[:0], s["cams"] * 2, [s["obs"][0], none]),
                                      ("no camera", s["segs"], line, [], []),
                                      ("cameras without segments", s["segs"], line, s["cams"] * 2, [none, none])):
        got = api.bundle_segments(segs, ln, cams, obs)
        n = len(ln)
        assert got["segments"].tobytes() == segs[order[:n]].tobytes() and got["line"].tobytes() == ln[order[:n]].tobytes(), what
        assert len(got["observations"]) == 0 and all((a["record"] == -1).all() for a in got["associations"])
        want = np.array([BM.HELD] * 12); want[[3, 9, 10]] = BM.EMPTY
        assert got["lines"]["status"].tolist() == (want.tolist() if n else [])
        sm = got["summary"]
        assert sm["status"] == "NO_VARIABLES" and sm["iterations"] == 0 and len(got["trace"]) == 0 and got["system"] is None
        assert sm["n_segments_before"] == sm["n_segments_after"] == n and sm["n_observations"] == 0
        assert len(got["cameras"]) == len(cams)
        for a, b in zip(got["cameras"], cams):
            PC.same_camera(a, b, what)
    # a line's segments need not be neighbours: grouped by ascending line index, in input order within a line, bit for bit
    segs = np.random.default_rng(7).uniform(-3.0, 3.0, (5, 6)); ln = np.array([2, 0, 2, 1, 0], np.uint32)
    got = api.bundle_segments(segs, ln, [], [])
    assert got["segments"].tobytes() == segs[[1, 4, 3, 0, 2]].tobytes() and got["line"].tolist() == [0, 0, 1, 2, 2]
    assert got["lines"]["status"].tolist() == [BM.HELD] * 3 and got["lines"]["n_pieces"].tolist() == [2, 1, 2]
    assert got["lines"]["P1"].tobytes() == segs[[1, 3, 0], :3].tobytes() and got["lines"]["P2"].tobytes() == segs[[4, 3, 2], 3:].tobytes()
