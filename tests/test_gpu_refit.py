"""The 3D lines refit against cameras and their 2D segments on the MI355X (k_refit.hip, l3d_refit.hip), stage by
stage against the existing stateless entries and the numpy model of tests/refit_model.py: the associations against
l3d_project_segments + l3d_associate_segments, the observation list, the CSR, eligibility and the start parameters against
the model built from them, the solve against l3d_line_opt_solve on the model's tables, and the spans, the pieces, the
statuses and the output model against the model at tolerance 0."""
import ctypes as C
import os

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from line3dpp_amd.api import Line3D
from tests import pose_cases as PC
from tests import pose_model as PO
from tests import refit_cases as RC
from tests import refit_model as RM
from tests.pose_cases import same_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p = _lib.ptr


# the parametrisation and the write-back as the library's host runs them (l3d_line_to_cayley, l3d_cayley_to_segment; pinned
# against tests/line_opt_model.py to 1e-12 by tests/test_line_opt.py), so that the model follows a call bit for bit
def lib_to_cayley(P1, P2):
    x = np.zeros(4)
    rc = _lib.load().l3d_line_to_cayley(p(np.ascontiguousarray(P1, np.float64)), p(np.ascontiguousarray(P2, np.float64)), p(x))
    assert rc in (0, 1)
    return x, rc == 1


def lib_write_back(x, P1, P2):
    a = np.zeros(3); b = np.zeros(3)
    rc = _lib.load().l3d_cayley_to_segment(p(np.ascontiguousarray(x, np.float64)), p(np.ascontiguousarray(P1, np.float64)),
                                           p(np.ascontiguousarray(P2, np.float64)), p(a), p(b))
    assert rc in (0, 1)
    return a, b, rc == 1


def model_par(max_distance=2.5, max_angle=10.0, min_overlap=0.5, near=1e-6, min_length=0.0, visibility=3, max_iterations=50,
              use_ambiguous=False):
    return dict(max_distance=max_distance, min_cos2=RM.AM.min_cos2_of(max_angle), min_overlap=min_overlap, near_plane=near,
                min_length=min_length, visibility=visibility, max_iterations=max_iterations, use_ambiguous=use_ambiguous)


def check(s, what, got=None, **kw):
    """one call, every stage against its reference -> (the library's dict, the model's preparation)"""
    kw = dict(s["par"], **kw)
    par = model_par(**kw)
    segs, line, cams, obs = s["segs"], s["line"], s["cams"], s["obs"]
    if got is None:
        got = api.refit_segments(segs, line, cams, obs, **kw)
    # stage 2: the associations are the public chain's
    rec = api.project_segments(cams, segs[:, :3], segs[:, 3:], line, near=kw.get("near", 1e-6))
    chain = api.associate_segments(rec, obs, kw["max_distance"], kw.get("max_angle", 10.0), kw.get("min_overlap", 0.5))
    assert len(got["associations"]) == len(cams)
    for k in range(len(cams)):
        same_bytes(got["associations"][k], chain[k], f"{what}: associations of camera {k}")
    # stages 3 and 5: the observation list, the CSR, eligibility and x0 are the model's, built from those associations
    prep = RM.prepare(segs, line, cams, obs, chain, par, to_cayley=lib_to_cayley)
    for f in ("camera", "segment", "line"):
        same_bytes(got["observations"][f], prep["observations"][f], f"{what}: observations.{f}")
    for f in ("n_observations", "n_views", "x0"):
        same_bytes(got["lines"][f], prep["lines"][f], f"{what}: lines.{f}")
    solved = prep["solved"]
    not_solved = np.setdiff1d(np.arange(prep["n_lines"]), solved)
    same_bytes(got["lines"]["status"][not_solved], prep["lines"]["status"][not_solved], f"{what}: statuses before the solve")
    # stage 6: the solve is l3d_line_opt_solve on the model's tables (the same kernel: stage 4 and the work order)
    if len(solved):
        x, c0, c1, it, st = api.line_opt_solve(prep["x0"], prep["res_off"], prep["obs"], prep["obs_cam"], prep["cams16"],
                                               max_iter=par["max_iterations"], narrow_max=16)
        L = got["lines"][solved]
        same_bytes(L["x"], x, f"{what}: x"); same_bytes(L["cost0"], c0, f"{what}: cost0"); same_bytes(L["cost1"], c1, f"{what}: cost1")
        same_bytes(L["iterations"], it.astype(np.uint32), f"{what}: iterations")
        same_bytes(L["solver_status"], st.astype(np.uint32), f"{what}: solver status")
    # stages 7 to 10 from the device's x: spans, pieces, statuses and the output model at tolerance 0
    L = got["lines"][solved]
    fin = RM.finish(segs, line, prep, (L["x"], L["cost0"], L["cost1"], L["iterations"], L["solver_status"]), par, write_back=lib_write_back)
    same_bytes(got["observations"], fin["observations"], f"{what}: spans")
    same_bytes(got["lines"], fin["lines"], f"{what}: lines")
    same_bytes(got["segments"], fin["segments"], f"{what}: output segments")
    same_bytes(got["line"], fin["line"], f"{what}: output line indices")
    # every line that is not REFIT comes back bit for bit, in input order, and the output is grouped by line
    assert (np.diff(got["line"].astype(np.int64)) >= 0).all()
    for l in np.flatnonzero(got["lines"]["status"] != RM.REFIT):
        same_bytes(got["segments"][got["line"] == l], segs[line == l], f"{what}: line {l} as given")
    sm = got["summary"]
    assert sm["n_lines"] == prep["n_lines"] and sm["n_observations"] == len(got["observations"])
    assert [sm["status"][n] for n in RM.STATUS] == np.bincount(got["lines"]["status"], minlength=6).tolist()
    assert sm["n_segments_before"] == len(segs) and sm["n_segments_after"] == len(got["segments"])
    amb = sum(int(((a["record"] >= 0) & (a["n_accepted"] > 1)).sum()) for a in chain)
    assert sm["n_ambiguous_left_out"] == (0 if par["use_ambiguous"] else amb)
    return got, prep


@pytest.mark.parametrize("n_cams", (1, 2, 3))
@pytest.mark.parametrize("visibility", (1, 2, 3))
def test_cameras_and_visibility_on_both_sides_of_eligibility(n_cams, visibility):
    s = RC.small(n_cams=n_cams)
    got, _ = check(s, f"{n_cams} cameras, visibility {visibility}", visibility=visibility)
    st = got["lines"]["status"]
    if n_cams < max(2, visibility):
        assert (st == RM.TOO_FEW_VIEWS).all() and got["segments"].tobytes() == s["segs"].tobytes()
    else:
        print(n_cams, visibility, np.bincount(st, minlength=6).tolist())
        assert (st == RM.REFIT).sum() > 10


@pytest.fixture(scope="module")
def dense():
    """six cameras on 800 lines at 2.5 px: more than 4 097 segments that observe a line"""
    s = RC.recovery(n_lines=800, degrees=0.1, shift=0.002)
    s["par"] = dict(max_distance=2.5, visibility=3, use_ambiguous=True)
    rec = api.project_segments(s["cams"], s["segs"][:, :3], s["segs"][:, 3:], s["line"])
    chain = api.associate_segments(rec, s["obs"], 2.5)
    flags = np.concatenate([a["record"] >= 0 for a in chain])
    assert flags.sum() >= 4097
    return s, flags


@pytest.mark.parametrize("n_obs", (0, 1, 255, 256, 257, 4095, 4096, 4097))
def test_observation_counts_at_the_block_and_scan_tile_edges(dense, n_obs):
    s, flags = dense
    # the 2D segments up to the n-th observation; the cameras behind it have no segment
    keep = int(np.flatnonzero(np.cumsum(flags) == n_obs)[-1]) + 1 if n_obs else int(np.argmax(flags))
    if n_obs == 0 and keep == 0:
        keep = 1; s = dict(s, obs=[np.zeros((1, 4), np.float32)] + s["obs"][1:])              # (a point matches nothing)
    obs, at = [], 0
    for o in s["obs"]:
        obs.append(o[:max(0, min(len(o), keep - at))]); at += len(o)
    L = _lib.load()
    before = L.l3d_debug_counter(b"refit_lines_solved")
    got, prep = check(dict(s, obs=obs), f"{n_obs} observations")
    assert len(got["observations"]) == n_obs and L.l3d_debug_counter(b"refit_observations") == n_obs
    assert L.l3d_debug_counter(b"refit_lines_solved") == before + len(prep["solved"])
    if n_obs >= 4095:
        assert (got["lines"]["status"] == RM.REFIT).sum() > 400


@pytest.mark.parametrize("n_seg", (4095, 4096, 4097))
def test_2d_segments_at_the_scan_tile_edge(dense, n_seg):
    """k_scan ranks the flags of all 2D segments, 4 096 to a tile: one tile exactly, one short of it, and one past it"""
    s, flags = dense
    obs, at = [], 0
    for o in s["obs"]:
        obs.append(o[:max(0, min(len(o), n_seg - at))]); at += len(o)
    assert sum(len(o) for o in obs) == n_seg
    got, _ = check(dict(s, obs=obs), f"{n_seg} 2D segments")
    assert len(got["observations"]) == int(flags[:n_seg].sum()) > 3000 and sum(len(a) for a in got["associations"]) == n_seg


def test_lines_with_0_1_16_17_64_and_65_observations_in_one_call():
    s = RC.fan()
    got, prep = check(s, "fan")
    assert got["lines"]["n_observations"].tolist() == list(RC.FAN_COUNTS) == got["lines"]["n_views"].tolist()
    assert got["lines"]["status"].tolist() == [RM.TOO_FEW_VIEWS] * 2 + [RM.REFIT] * 4
    err = RC.carrier_errors(got["lines"], s["truth"])
    assert (err[2:] < 1e-5).all(), err


def test_a_camera_without_segments_and_one_that_matches_nothing():
    s = RC.small(n_cams=4)
    obs = list(s["obs"])
    obs[1] = np.zeros((0, 4), np.float32)
    obs[2] = obs[2].copy(); obs[2][:, 2:] = obs[2][:, :2]                       # (points match nothing)
    got, _ = check(dict(s, obs=obs), "silent cameras", visibility=2)
    assert set(got["observations"]["camera"].tolist()) == {0, 3} and (got["lines"]["status"] == RM.REFIT).sum() > 10
    assert (got["associations"][2]["record"] == -1).all() and len(got["associations"][1]) == 0


@pytest.mark.parametrize("use_ambiguous", (False, True))
def test_ambiguous_segments_are_left_out_or_used(use_ambiguous):
    s = RC.small(n_lines=150)
    got, _ = check(s, f"use_ambiguous {use_ambiguous}", use_ambiguous=use_ambiguous)
    amb = sum(int(((a["record"] >= 0) & (a["n_accepted"] > 1)).sum()) for a in got["associations"])
    assert amb > 5 and got["summary"]["n_ambiguous_left_out"] == (0 if use_ambiguous else amb)
    matched = sum(int((a["record"] >= 0).sum()) for a in got["associations"])
    assert len(got["observations"]) == (matched if use_ambiguous else matched - amb)


def test_split_lines_whose_halves_are_apart_and_indices_that_no_segment_carries():
    s = RC.small()
    n = len(s["segs"])
    mid = 0.5 * (s["segs"][:, :3] + s["segs"][:, 3:])
    segs = np.ascontiguousarray(np.concatenate([np.concatenate([s["segs"][:, :3], mid], 1), np.concatenate([mid, s["segs"][:, 3:]], 1)]))
    line = np.concatenate([2 * np.arange(n), 2 * np.arange(n)]).astype(np.uint32)     # (the odd indices are empty)
    got, prep = check(dict(s, segs=segs, line=line), "split lines")
    st = got["lines"]["status"]
    assert (st[1::2] == RM.EMPTY).all() and (st[0::2] == RM.REFIT).sum() > 20
    # the carrier is P1 of the first and P2 of the last segment in input order: the whole line
    whole = api.refit_segments(s["segs"], s["line"], s["cams"], s["obs"], **s["par"])
    # (where both calls find the line eligible: a 2D segment across the cut may be assigned to either half, or to both)
    both = (st[0::2] != RM.TOO_FEW_VIEWS) & (whole["lines"]["status"] != RM.TOO_FEW_VIEWS)
    assert both.sum() > 20
    same_bytes(got["lines"]["x0"][0::2][both], whole["lines"]["x0"][both], "carriers of the split lines")


def test_zero_iterations_cut_the_extents_about_the_unchanged_carrier():
    s = RC.small()
    got, prep = check(s, "max_iterations 0", max_iterations=0)
    L = got["lines"][prep["solved"]]
    assert (L["iterations"] == 0).all() and (L["solver_status"] == 4).all() and L["x"].tobytes() == L["x0"].tobytes()
    assert (L["cost0"] == L["cost1"]).all() and (L["status"] == RM.REFIT).sum() > 20
    before = RC.carrier_errors(dict(P1=s["segs"][:, :3], P2=s["segs"][:, 3:]), s["truth"])
    after = RC.carrier_errors(got["lines"], s["truth"])
    assert np.allclose(before[prep["solved"]], after[prep["solved"]], rtol=0, atol=1e-9)


def test_a_model_far_from_the_origin_and_two_calls_in_a_row():
    s = RC.small()
    near, _ = check(s, "at the origin")
    far, _ = check(RC.shifted(s, 1e5), "shifted by 1e5")
    assert far["lines"]["status"].tolist() == near["lines"]["status"].tolist()
    again = api.refit_segments(s["segs"], s["line"], s["cams"], s["obs"], **s["par"])
    for k in ("segments", "line", "lines", "observations"):
        same_bytes(again[k], near[k], f"second call: {k}")


# ---- recovery and alternation (the figures of the model: tests/test_refit_host.py) -----------------------------
@pytest.mark.parametrize("name", ("plain", "noisy"))
def test_recovery(name):
    """The device must refit what the model refits, within ten times the model's median and 90th percentile (the margin
    is for the solver's documented distance from its numpy model, §10), and no line may end above its start cost."""
    from tests.test_refit_host import RECOVERY_MODEL
    noise, median, p90 = RECOVERY_MODEL[name]
    s = RC.recovery(noise=noise)
    want = RM.refit(s["segs"], s["line"], s["cams"], s["obs"], **s["par"])
    assert (want["lines"]["status"] == RM.REFIT).all()
    got = api.refit_segments(s["segs"], s["line"], s["cams"], s["obs"], **s["par"])
    assert got["lines"]["status"].tolist() == want["lines"]["status"].tolist()
    err = RC.carrier_errors(got["lines"], s["truth"])
    print(f"{name}: median {np.median(err):.3e} (model {median:.3e}), p90 {np.percentile(err, 90):.3e} (model {p90:.3e}), max {err.max():.3e}")
    assert np.median(err) <= 10 * median and np.percentile(err, 90) <= 10 * p90
    assert (got["lines"]["cost1"] <= got["lines"]["cost0"]).all()
    assert got["summary"]["n_ambiguous_left_out"] > 50


def test_alternation_of_cameras_and_lines():
    """three rounds of refine_cameras and refit_segments: the cameras' rms falls, to at most twice what the models reach.
    Absolute errors are not asserted: the pair is free up to a similarity."""
    s = RC.alternation()
    got = api.refine_model(s["segs"], s["line"], s["cams"], s["obs"], rounds=3, max_distance=6.0, start_distance=12.0)
    model, line, cams = s["segs"], s["line"], s["cams"]
    for r in range(3):
        pose = PO.refine(model, line, cams, s["obs"], max_distance=6.0, start_distance=12.0 if r == 0 else 0.0)
        cams = pose["cameras"]
        fit = RM.refit(model, line, cams, s["obs"], **s["par"])
        model, line = fit["segments"], fit["line"]
    first = max(x["rms"] for x in got["rounds"][0][0]); last = max(x["rms"] for x in got["rounds"][2][0])
    want = max(x["rms"] for x in pose["summaries"])
    print(f"rms per camera at most: round 0 {first:.4f}, round 2 {last:.4f} (models {want:.4f})")
    assert len(got["rounds"]) == 3 and last < first and last <= 2.0 * want
    assert all(sm["status"]["REFIT"] == 300 for _, sm in got["rounds"])
    assert len(got["segments"]) == len(got["line"]) == got["rounds"][2][1]["n_segments_after"]


# ---- real data ----------------------------------------------------------------------------------------------------------
# The whole numpy model on this scene (numpy association, numpy solver on all 2 094 eligible lines: 16.5 s on a CPU, so it is
# not repeated here): lines per status, and no line among them a close call of §10 (a decision within 1e-6 of its threshold).
REAL_MODEL_STATUS = (2094, 396, 0, 0, 0, 0)
REAL_STRIDE = 8                                  # every eighth eligible line is solved by the numpy solver in the test


def test_real_scene_statuses_equal_the_model():
    """golden scene C0 against the reference's optimised model, the fixture's poses, 2.5 px.  Every stage equals its
    reference as in every other test.  The statuses are the model's: per status the counts of the whole numpy model, and
    line by line for every eighth eligible line, which the numpy solver (lm_solve) solves here from the same start.  For
    those lines §10's convention holds: stopping rule and iteration count equal the model's for every line that is no
    close call, and x and cost1 lie within 100 x the model's own fp64 / long double difference (T of
    tests/test_gpu_line_opt_solver.py) -- but for the lines the iteration limit stops, which are at no optimum: their
    distance is printed."""
    from tests import line_opt_model as LO
    from tests.test_gpu_line_opt_solver import T
    s = PC.real_scene()
    # (the fixture's K carry a skew of up to 1.4, which the solver's camera cannot hold: the stage refuses it, so it is dropped)
    s["cams"] = [PO.camera(np.where(np.arange(9).reshape(3, 3) == 1, 0.0, c["K"]), c["R"], c["t"], c["width"], c["height"]) for c in s["cams"]]
    kw = dict(max_distance=2.5, visibility=3)
    got = api.refit_segments(s["segs"], s["line"], s["cams"], s["obs"], **kw)
    s["par"] = kw
    _, prep = check(s, "real scene", got=got)
    st = np.bincount(got["lines"]["status"], minlength=6)
    assert tuple(st.tolist()) == REAL_MODEL_STATUS
    solved = prep["solved"]
    dev = got["lines"][solved]
    solve = [dev[f].copy() for f in ("x", "cost0", "cost1", "iterations", "solver_status")]
    pick = np.arange(0, len(solved), REAL_STRIDE)
    close, worst, worst_limit = 0, [0.0, 0.0], [0.0, 0.0]
    for i in pick:
        r = slice(int(prep["res_off"][i]), int(prep["res_off"][i + 1]))
        x, c0, c1, it, status, margin = LO.lm_solve(prep["x0"][i], prep["cams16"][prep["obs_cam"][r]], prep["obs"][r], 50)
        if margin < 1e-6:
            close += 1
            continue
        assert (int(dev["solver_status"][i]), int(dev["iterations"][i])) == (status, it), (int(solved[i]), status, it)
        dx = float(np.abs(dev["x"][i] - x).max()) / max(1.0, float(np.abs(x).max())); dc = abs(float(dev["cost1"][i]) - c1) / max(1.0, c1)
        into = worst_limit if status == 4 else worst
        into[0] = max(into[0], dx); into[1] = max(into[1], dc)
        solve[0][i], solve[1][i], solve[2][i], solve[3][i], solve[4][i] = x, c0, c1, it, status
    print(f"real scene: {len(pick)} lines against lm_solve, {close} close calls, x / cost1 within {worst[0]:.2e} / {worst[1]:.2e}"
          f" (T = {T:.2e}); stopped by the iteration limit: {worst_limit[0]:.2e} / {worst_limit[1]:.2e}")
    assert close <= 0.05 * len(pick) and worst[0] <= T and worst[1] <= T
    # ... and with the model's x in the place of the device's, those lines end with the same status
    par = model_par(**kw)
    fin = RM.finish(s["segs"], s["line"], prep, tuple(solve), par, write_back=lib_write_back)
    assert fin["lines"]["status"].tolist() == got["lines"]["status"].tolist()
    no = got["lines"]["n_observations"]
    print("real scene: observations per line mean", float(no.mean()), "median", float(np.median(no)), "max", int(no.max()),
          "of the REFIT lines", float(no[got["lines"]["status"] == RM.REFIT].mean()))
    length = lambda a: float(np.linalg.norm(a[:, :3] - a[:, 3:], axis=1).sum())
    print("real scene: lines per status", dict(zip(RM.STATUS, st.tolist())), "observations", len(got["observations"]),
          "per line", float(np.mean(got["lines"]["n_observations"])), "length", length(s["segs"]), "->", length(got["segments"]),
          "cost", got["summary"]["cost0"], "->", got["summary"]["cost1"])
    assert st[RM.REFIT] > 0 and (got["lines"]["cost1"] <= got["lines"]["cost0"])[got["lines"]["status"] == RM.REFIT].all()


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
    free = api.refit_segments(segs, line, cams, obs, max_distance=2.5)
    g.set_projection_budget(64)                   # one camera per group at most
    try:
        assert g.setTimingLevel(2)
        ctx = g.refitLines(max_distance=2.5)
    finally:
        g.set_projection_budget(0); g.setTimingLevel(1)
    assert ctx is not None and ctx["camIDs"] == order
    for k in ("segments", "line", "lines", "observations"):
        same_bytes(ctx[k], free[k], f"context / stateless: {k}")
    same_bytes(ctx["associations"], np.concatenate(free["associations"]), "context / stateless: associations")
    check(dict(segs=segs, line=line, cams=cams, obs=obs, par=dict(max_distance=2.5)), "golden scene", got=free)
    total = L.l3d_debug_counter(b"refit_kernel_ns")
    parts = [L.l3d_debug_counter(n) for n in (b"refit_associate_ns", b"refit_list_ns", b"refit_obs_ns", b"refit_lineopt_ns", b"refit_spans_ns")]
    assert 0 < total < 10 ** 9 and all(v > 0 for v in parts) and abs(sum(parts) - total) <= 5
    # the views are unchanged, the model is replaced as specified
    for c, cam in zip(order, cams):
        PC.same_camera(g.viewCamera(c), cam, f"view {c} after the call")
    after = g.get3Dlines()
    st = ctx["lines"]["status"]
    assert len(after) == len(before) and (st == RM.REFIT).sum() > 0
    seg2, line2 = api.flatten_lines(after)
    same_bytes(seg2, ctx["segments"], "the context's lines"); same_bytes(line2, ctx["line"], "the context's line indices")
    for l, (a, b) in enumerate(zip(before, after)):
        assert a["reference_view"] == b["reference_view"]
        if st[l] != RM.REFIT:
            assert a["collinear3Dsegments"].tobytes() == b["collinear3Dsegments"].tobytes() and a["residuals"].tobytes() == b["residuals"].tobytes()
            assert a["cluster_line"].tobytes() == b["cluster_line"].tobytes()
            continue
        same_bytes(np.concatenate([b["cluster_line"]["P1"], b["cluster_line"]["P2"]]), np.concatenate([ctx["lines"]["P1"][l], ctx["lines"]["P2"][l]]),
                   f"line {l}: cluster segment")
        o = ctx["observations"][ctx["observations"]["line"] == l]
        assert [(int(r["cam"]), int(r["seg"])) for r in b["residuals"]] == [(order[int(k)], int(i)) for k, i in zip(o["camera"], o["segment"])]
    # associateSegments afterwards agrees with the stored residuals: a stored residual is still assigned to its line unless
    # the refit moved the line away from it, and most are
    assoc = g.associateSegments(order)[0]
    kept = total_res = 0
    for l, b in enumerate(after):
        if st[l] != RM.REFIT:
            continue
        for r in b["residuals"]:
            total_res += 1
            kept += int(assoc[int(r["cam"])]["line"][int(r["seg"])] == l)
    print("residuals still assigned to their line:", kept, "of", total_res)
    assert kept >= 0.98 * total_res               # (280 of 280 when this was written)
    # the writers' names carry the tag until the next reconstruct3Dlines
    name = g.outputFilename()
    assert "REFIT_2.5__" in name and name.replace("REFIT_2.5__", "") == name_before
    assert g.reconstruct3Dlines(3) and g.outputFilename() == name_before
    same_bytes(api.flatten_lines(g.get3Dlines())[0], segs, "the lines after a second reconstruct3Dlines")


def test_context_errors(golden):
    g, ids = golden["g"], golden["cam_ids"]
    L = _lib.load()
    segs = api.flatten_lines(g.get3Dlines())[0]
    assert g.refitLines(max_angle=120.0) is None and g.last_status == -1
    assert g.refitLines(visibility=0) is None and "visibility" in _lib.last_error()
    assert g.refitLines([ids[0], 987654]) is None and "unknown camera ID" in _lib.last_error()
    assert g.refitLines([ids[1], ids[0], ids[1]]) is None and "named twice" in _lib.last_error()
    skew = g.viewCamera(ids[0]); skew["K"][0, 1] = 0.5
    assert g.refitLines([ids[0]], [skew]) is None and "K01" in _lib.last_error()
    assert api.flatten_lines(g.get3Dlines())[0].tobytes() == segs.tobytes() and "REFIT" not in g.outputFilename()
    none = g.refitLines([])
    assert none is not None and none["camIDs"] == [] and (none["lines"]["status"] == RM.TOO_FEW_VIEWS).all()
    assert none["segments"].tobytes() == segs.tobytes()
    # a call that refits no line leaves the model and its name alone: no camera, and one camera (fewer than two views)
    assert "REFIT" not in g.outputFilename()
    one = g.refitLines([ids[0]])
    assert one is not None and (one["lines"]["status"] == RM.TOO_FEW_VIEWS).all() and len(one["observations"]) > 0
    assert "REFIT" not in g.outputFilename() and api.flatten_lines(g.get3Dlines())[0].tobytes() == segs.tobytes()
    from line3dpp_amd.scene import make_scene
    h = Line3D()
    h.add_scene(make_scene(4, 60, n_neighbors=2, seed=2))
    assert h.refitLines() is None and h.last_status == -7
    assert h.matchBegin()
    par = api.refit_params()
    ids4 = np.arange(4, dtype=np.uint32)
    assert L.l3d_refit_view_lines(h.h, 4, p(ids4), None, C.byref(par), None, None) == -7 and "split call" in _lib.last_error()
    h.matchAbort()
    h.close()


def test_refine_model_on_the_context(golden):
    g = golden["g"]
    before = api.flatten_lines(g.get3Dlines())[0]
    res = g.refineModel(rounds=2, start_distance=5.0)
    assert res is not None and len(res["rounds"]) == 2 and "REFIT_2.5__" in g.outputFilename()
    after = api.flatten_lines(g.get3Dlines())[0]
    same_bytes(after, res["segments"], "the context's lines after refineModel")
    assert after.tobytes() != before.tobytes()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_refit_lines(tmp_path):
    import struct
    import subprocess
    from line3dpp_amd.scene import make_scene
    exe = str(tmp_path / "refit_smoke")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "refit_smoke.cpp"), "-o", exe, "-L" + lib_dir,
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
    assert run_.stdout.count("[L3D++] ERROR:") == 2 and "refitLines" in run_.stdout   # the call before the reconstruction, a bad angle
    raw = open(out_path, "rb").read()
    sm = _lib.RefitSummary.from_buffer_copy(raw, 0)
    pos, models = 104, []
    for _ in range(2):
        n, = struct.unpack_from("<I", raw, pos); pos += 4
        segs = np.frombuffer(raw, np.float64, 6 * n, pos).reshape(n, 6); pos += 48 * n
        models.append((segs, np.frombuffer(raw, np.uint32, n, pos))); pos += 4 * n
    held = {}
    for _ in range(sc.n_views):
        cam_id, = struct.unpack_from("<I", raw, pos); pos += 4
        held[cam_id] = api.camera_dict(_lib.Camera.from_buffer_copy(raw, pos)); pos += C.sizeof(_lib.Camera)
    assert pos == len(raw)
    views = sorted(sc.views, key=lambda v: v.cam)
    cams = [held[v.cam] for v in views]               # (the cameras as the context holds them)
    obs = [np.ascontiguousarray(v.segs, np.float32).reshape(-1, 4) for v in views]
    want = api.refit_segments(models[0][0], models[0][1], cams, obs, max_distance=2.5)
    print(run_.stdout.strip().splitlines()[-1], want["summary"]["status"])
    same_bytes(models[1][0], want["segments"], "the facade's model / the stateless call")
    same_bytes(models[1][1], want["line"], "the facade's line indices / the stateless call")
    assert api.refit_summary_dict(sm) == want["summary"] and sm.n_status[0] > 0


def test_argument_errors_leave_the_handle_untouched():
    """on a machine with a device as well: no launch, no handle"""
    L = _lib.load()
    s = RC.small()
    cams = api.camera_array(s["cams"])
    n_seg = np.array([len(o) for o in s["obs"]], np.uint32); seg4 = np.concatenate(s["obs"])
    out = np.full(2, 0x5A5A5A5A, np.uint32)
    before = L.l3d_debug_counter(b"refit_lines_solved")
    for vals, word in (((2.5, 0.97, 0.5, 1e-6, 0.0, 0, 50, 0, (0, 0, 0)), "visibility"), ((2.5, 0.97, 0.5, 0.0, 0.0, 3, 50, 0, (0, 0, 0)), "near plane"),
                       ((2.5, 0.97, 0.5, 1e-6, 0.0, 3, 1001, 0, (0, 0, 0)), "max_iterations")):
        par = _lib.RefitParams(*vals)
        rc = L.l3d_refit_segments(0, len(s["segs"]), p(s["segs"]), p(s["line"]), len(s["cams"]), cams, p(n_seg), p(seg4), C.byref(par),
                                  C.cast(p(out), C.POINTER(C.c_void_p)))
        assert rc == -1 and word in _lib.last_error() and (out == 0x5A5A5A5A).all()
    assert L.l3d_debug_counter(b"refit_lines_solved") == before
