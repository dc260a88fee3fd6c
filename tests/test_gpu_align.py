"""Two 3D line models aligned on the MI355X (k_align.hip, l3d_align.hip) against the numpy model of
tests/align_model.py with tolerance 0 on every field: one iteration at the lane, wave, tile and slice edges, every
slicing of one case, waves and a tile without a match, both settings of estimate_scale, the full runs of the recovery
scenes with their whole trace, the statuses and the empty forms, l3d_transform_segments, repeated calls, the context
form on the golden scene, the C++ facade, the real models, the counters and the argument refusals."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from line3dpp_amd.api import Line3D
from tests import align_cases as Cs
from tests import align_model as A
from tests import compare_model as CM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A5A5A5A
COUNTERS = ("align_iterations", "align_normal_launches", "compare_launches", "compare_merge_launches")


def counters():
    L = _lib.load()
    return {k: L.l3d_debug_counter(k.encode()) for k in COUNTERS}


def run(s, **kw):
    """api.align_segments on a scene of align_cases"""
    return api.align_segments(s["q"], s["ql"], s["r"], s["rl"], initial=s.get("initial"), **dict(s["par"], **kw))


def model(s, **kw):
    kw = dict(s["par"], **kw)
    kw.pop("slice_chunks", None)
    if "estimate_scale" in kw:
        kw["estimate_scale"] = int(kw["estimate_scale"])
    return A.align(s["q"], s["ql"], s["r"], s["rl"], initial=s.get("initial"), **kw)


# ---- one iteration at the edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q,n_r,slice_chunks", Cs.EDGE_SHAPES)
def test_one_iteration_at_lane_wave_tile_and_slice_edges(n_q, n_r, slice_chunks):
    s = Cs.edge_scene(n_q, n_r)
    kw = dict(max_iterations=1, min_matches=1)
    before = counters()
    got = run(s, slice_chunks=slice_chunks, **kw)
    after = counters()
    want = model(s, **kw)
    Cs.same_result(got, want, f"({n_q}, {n_r}, {slice_chunks})")
    assert len(got["trace"]) == 1 and got["trace"]["n_matched"][0] >= max(min(n_q, n_r) // 2, 1)
    if min(n_q, n_r) > 1:
        assert got["summary"]["status"] == "MAX_ITERATIONS" and got["trace"]["delta"][0].all()
    else:
        assert got["summary"]["status"] == "DEGENERATE"                    # one line leaves the shift along it free
    assert after["align_iterations"] == before["align_iterations"] + 1
    assert after["align_normal_launches"] == before["align_normal_launches"] + 2        # the iteration and the delivery pass
    assert after["compare_launches"] == before["compare_launches"]                      # l3d_compare.hip's own counters stay its own


def test_no_output_depends_on_the_slicing():
    s = Cs.edge_scene(*Cs.SLICING_SHAPE)
    results = [run(s, slice_chunks=sc, max_iterations=3) for sc in Cs.SLICINGS]
    for sc, res in zip(Cs.SLICINGS[1:], results[1:]):
        Cs.same_result(res, results[0], f"slice_chunks {sc} / 1")
    Cs.same_result(results[0], model(s, max_iterations=3), "every slicing / the model")
    assert len(results[0]["trace"]) == 3


def test_waves_and_a_tile_without_a_match():
    s = Cs.gap_scene()
    got = run(s, max_iterations=1)
    want = model(s, max_iterations=1)
    Cs.same_result(got, want, "gap scene")
    assert (got["matches_q"]["segment"][s["far"]] == -1).all() and got["summary"]["n_matched"] > 300
    # the sums of the empty waves and the empty tile are +0.0, and the model's tree shows them so
    c, _ = A.bounding_box(s["r"])
    moved, m, _ = A.one_pass(s["q"], s["ql"], s["r"], s["rl"], A.entry(s["initial"]), s["par"]["max_distance"], A.DEFAULTS, c, "array")
    tiles = A.tile_sums(A.query_terms(moved, s["r"], m, c))
    assert tiles[1].tobytes() == np.zeros(A.TERMS).tobytes() and tiles[0].any() and tiles[2].any()


@pytest.mark.parametrize("estimate_scale", [True, False])
def test_both_settings_of_estimate_scale(estimate_scale):
    s = Cs.edge_scene(300, 400)
    got = run(s, estimate_scale=estimate_scale, max_iterations=2)
    Cs.same_result(got, model(s, estimate_scale=estimate_scale, max_iterations=2), f"estimate_scale={estimate_scale}")
    assert got["trace"]["delta"][:, 3].any() == estimate_scale
    assert (got["similarity"]["scale"] == A.entry(s["initial"])["scale"]) == (not estimate_scale)


# ---- the full runs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.RECOVERY))
def test_full_runs_equal_the_model_bit_for_bit(name):
    s = Cs.recovery_scene(**Cs.RECOVERY[name])
    got = run(s)
    want = model(s)
    Cs.same_result(got, want, name)
    err = A.end_point_error(s["q"], got["similarity"], s["T_true"], s["diag"])
    print(name, got["summary"], "end-point error", err)
    assert got["summary"]["status"] == "CONVERGED" and got["summary"]["iterations"] == want["summary"]["iterations"] <= 12
    assert got["summary"]["n_matched"] == s["n_kept"]
    Cs.same_bytes(api.transform_segments(s["q"], got["similarity"]), got["segments"], "l3d_transform_segments / out_segs6")
    assert got["matrix"].tobytes() == A.matrix(want["similarity"]).tobytes()


def test_the_gate_schedule_on_the_device():
    s = Cs.recovery_scene(start=Cs.FAR_START)
    plain, scheduled = run(s, start_distance=0.0), run(s)
    Cs.same_result(plain, model(s, start_distance=0.0), "plain gate")
    Cs.same_result(scheduled, model(s), "gate schedule")
    assert plain["summary"]["status"] == "TOO_FEW" and scheduled["summary"]["status"] == "CONVERGED"


def test_degenerate_too_few_and_the_empty_forms():
    s = Cs.parallel_scene()
    got = run(s)
    Cs.same_result(got, model(s), "parallel references")
    assert got["summary"]["status"] == "DEGENERATE" and got["summary"]["iterations"] == 1 and got["summary"]["n_matched"] == 9
    assert tuple(got["similarity"]["q"]) == (1.0, 0.0, 0.0, 0.0) and got["similarity"]["scale"] == 1.0
    s = Cs.recovery_scene()
    n = int(model(s, max_iterations=1)["trace"]["n_matched"][0])
    got = run(s, min_matches=n + 1)
    Cs.same_result(got, model(s, min_matches=n + 1), "one match short")
    assert got["summary"]["status"] == "TOO_FEW" and got["summary"]["iterations"] == 1
    Cs.same_bytes(Cs.similarity_array(got["similarity"]), Cs.similarity_array(A.entry(s["initial"])), "T unchanged")
    Cs.same_bytes(got["segments"], api.transform_segments(s["q"], s["initial"]), "the delivery pass under the unchanged T")
    assert run(s, min_matches=n, max_iterations=1)["summary"]["status"] == "MAX_ITERATIONS"
    before = counters()
    for n_q, n_r in ((5, 0), (0, 4)):
        e = dict(s, q=s["q"][:n_q], ql=s["ql"][:n_q], r=s["r"][:n_r], rl=s["rl"][:n_r])
        Cs.same_result(run(e), model(e), f"empty form ({n_q}, {n_r})")
    assert counters() == before


def test_two_calls_in_a_row_give_equal_bytes():
    s = Cs.recovery_scene(noise=1e-3)
    a, b = run(s), run(s)
    Cs.same_result(b, a, "second call")


# ---- the context form on the golden scene -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    from tests.golden.make_golden import golden_scene
    g = Line3D()
    g.add_scene(golden_scene())
    assert g.matchImages() and g.reconstruct3Dlines(3)
    lines = g.get3Dlines()
    segs, line = api.flatten_lines(lines)
    T_true = A.entry(A.similarity(1.6, Cs.axis_angle([0.3, -1.0, 0.5], 35.0), (2.0, 1.0, -4.0)))
    other = A.transform(segs, T_true)
    c, diag = A.bounding_box(other)
    initial = Cs.perturbed(T_true, c, diag, 2.0, 0.02, 0.01, np.random.default_rng(23))
    other_lines = []
    for i in range(len(lines)):
        other_lines.append(dict(segments=other[line == i]))
    yield dict(g=g, lines=lines, segs=segs, line=line, other=other, other_lines=other_lines, T_true=T_true, initial=initial, diag=diag,
               par=dict(max_distance=1e-3 * diag, start_distance=0.064 * diag))
    g.close()


def test_context_equals_the_stateless_call_and_leaves_the_lines_alone(golden):
    G = golden
    g = G["g"]
    assert len(G["segs"]) > 50
    before = api.flatten_lines(g.get3Dlines())
    ctx = g.alignLines(G["other_lines"], initial=G["initial"], **G["par"])
    assert ctx is not None
    free = api.align_segments(G["segs"], G["line"], G["other"], G["line"], initial=G["initial"], **G["par"])
    Cs.same_result(ctx, free, "context / stateless")
    Cs.same_result(ctx, A.align(G["segs"], G["line"], G["other"], G["line"], initial=G["initial"], **G["par"]), "context / model")
    again = g.alignLines(G["other_lines"], initial=G["initial"], slice_chunks=1, **G["par"])
    Cs.same_result(again, ctx, "a second call on the context")
    after = api.flatten_lines(g.get3Dlines())
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert ctx["summary"]["status"] == "CONVERGED"
    err = A.end_point_error(G["segs"], ctx["similarity"], G["T_true"], G["diag"])
    print(ctx["summary"], "end-point error", err)
    assert err <= 1e-12                                                    # (exact correspondences: the recovery scenes' figure)
    # the same model as `other`, from a start that is off: the transformed copy comes back onto the context's own lines,
    # and compareLines on it matches every live segment
    c, diag = A.bounding_box(G["segs"])
    off = Cs.perturbed(A.entry(None), c, diag, 2.0, 0.02, 0.01, np.random.default_rng(24))
    home = g.alignLines(G["lines"], 1e-3 * diag, start_distance=0.064 * diag, initial=off)
    assert home["summary"]["status"] == "CONVERGED"
    copy = [dict(segments=home["segments"][G["line"] == i]) for i in range(len(G["lines"]))]
    mine, theirs, s_mine, s_theirs = g.compareLines(copy, 1e-6 * diag)
    live = (G["segs"][:, :3] != G["segs"][:, 3:]).any(1)
    assert live.sum() > 50 and (mine["segment"][live] >= 0).all() and (theirs["segment"][live] >= 0).all()


def test_context_errors_and_the_kernel_time(golden):
    G = golden
    g = G["g"]
    L = _lib.load()
    assert g.alignLines(G["other_lines"], 1e-3, max_angle=120.0) is None and g.last_status == -1
    assert g.alignLines(G["other_lines"], -1.0) is None and g.last_status == -1
    assert g.alignLines(G["other_lines"], 1.0, start_distance=0.5) is None and "start_distance" in _lib.last_error()
    none = g.alignLines([], 1e-3)
    assert none["summary"]["status"] == "TOO_FEW" and len(none["segments"]) == len(G["segs"]) and len(none["matches_r"]) == 0
    assert g.setTimingLevel(2)
    try:
        assert g.alignLines(G["other_lines"], initial=G["initial"], **G["par"]) is not None
        assert 0 < L.l3d_debug_counter(b"align_kernel_ns") < 10 ** 9
    finally:
        g.setTimingLevel(1)
    from line3dpp_amd.scene import make_scene
    h = Line3D()
    h.add_scene(make_scene(4, 60, n_neighbors=2, seed=2))
    assert h.alignLines(G["other_lines"], 0.1) is None and h.last_status == -7
    assert h.matchBegin()
    par = api.align_params(0.1)
    sim = _lib.Similarity(); summary = _lib.AlignSummary(iterations=99)
    assert L.l3d_align_lines(h.h, len(G["line"]), _lib.ptr(G["other"]), _lib.ptr(G["line"]), C.byref(par), None, C.byref(sim),
                             C.byref(summary), None, None, None, None) == -7
    assert "split call" in _lib.last_error() and summary.iterations == 99
    h.matchAbort()
    h.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_align_lines(tmp_path):
    from line3dpp_amd.scene import make_scene
    exe = str(tmp_path / "align_smoke")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "align_smoke.cpp"), "-o", exe, "-L" + lib_dir,
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
    assert run_.stdout.count("[L3D++] ERROR:") == 2 and "alignLines" in run_.stdout   # the call before the reconstruction, a bad angle
    raw = open(out_path, "rb").read()
    par = _lib.AlignParams.from_buffer_copy(raw, 0)
    start = np.frombuffer(raw, A.SIMILARITY_DTYPE, 1, 64)[0]
    n_q, n_r = struct.unpack_from("<2I", raw, 128)
    pos = 136
    parts = []
    for n in (n_q, n_r):
        parts.append(np.frombuffer(raw, np.float64, 6 * n, pos).reshape(n, 6)); pos += 48 * n
        parts.append(np.frombuffer(raw, np.uint32, n, pos)); pos += 4 * n
    sim = np.frombuffer(raw, A.SIMILARITY_DTYPE, 1, pos)[0]; pos += 64
    summary = _lib.AlignSummary.from_buffer_copy(raw, pos); pos += 64
    moved = np.frombuffer(raw, np.float64, 6 * n_q, pos).reshape(n_q, 6); pos += 48 * n_q
    mine = np.frombuffer(raw, _lib.LINE_MATCH_DTYPE, n_q, pos); pos += 24 * n_q
    theirs = np.frombuffer(raw, _lib.LINE_MATCH_DTYPE, n_r, pos); pos += 24 * n_r
    assert pos == len(raw) and n_q > 10 and n_r == n_q
    want = A.align(*parts, par.max_distance, initial=A.similarity(start["scale"], start["q"], start["t"]), min_cos2=par.min_cos2,
                   min_overlap=par.min_overlap, start_distance=par.start_distance, step_tolerance=par.step_tolerance,
                   max_iterations=par.max_iterations, min_matches=par.min_matches, estimate_scale=par.estimate_scale)
    print(run_.stdout.strip().splitlines()[-1], want["summary"])
    Cs.same_bytes(sim, Cs.similarity_array(want["similarity"]), "the facade's similarity / the model")
    Cs.same_bytes(moved, want["segments"], "the facade's moved segments / the model")
    Cs.same_bytes(mine, want["matches_q"], "the facade's records / the model")
    Cs.same_bytes(theirs, want["matches_r"], "the facade's records / the model (other side)")
    assert (A.STATUS[summary.status], summary.iterations, summary.n_matched) == tuple(want["summary"][k] for k in ("status", "iterations", "n_matched"))
    assert summary.n_matched > 10


# ---- real data ---------------------------------------------------------------------------------------------------------
def test_real_models_are_aligned_back():
    """the property tests/test_align_host.py asserts on the model, on the device and without the model"""
    s = Cs.real_scene()
    res = run(s)
    sm = res["summary"]
    err = A.end_point_error(s["q"], res["similarity"], s["T_true"], s["diag"])
    share_q = (res["matches_q"]["segment"] >= 0).mean(); share_r = (res["matches_r"]["segment"] >= 0).mean()
    print(sm, "matched share", share_q, share_r, "end-point error", err)
    assert sm["status"] == "CONVERGED" and sm["iterations"] <= 12
    assert share_q >= 0.99 and share_r >= 0.99
    assert err <= 10 * 1.2e-5                                              # ten times the model's measured value


# ---- the argument refusals --------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched():
    L = _lib.load()
    s = Cs.edge_scene(40, 30)
    q, ql, r, rl = s["q"], s["ql"], s["r"], s["rl"]
    outs = [np.full(n, FILL, np.uint32) for n in (16, 16, 40 * 12, 40 * 6, 30 * 6, 20 * 108)]
    p = _lib.ptr
    before = counters()

    def call(vals, initial=None, r=r):
        par = _lib.AlignParams(*vals)
        rc = L.l3d_align_segments(0, 40, p(q), p(ql), 30, p(r), p(rl), C.byref(par), C.byref(initial) if initial is not None else None,
                                  C.cast(p(outs[0]), C.POINTER(_lib.Similarity)), C.cast(p(outs[1]), C.POINTER(_lib.AlignSummary)),
                                  p(outs[2]), p(outs[3]), p(outs[4]), p(outs[5]))
        assert all((x == FILL).all() for x in outs)
        return rc, _lib.last_error()

    good = [s["par"]["max_distance"], 0.9, 0.5, 0.0, 1e-9, 20, 3, 1, 0, (0, 0)]
    for k, name, v in ((0, "max_distance", -1.0), (3, "start_distance", 0.5 * good[0]), (4, "step_tolerance", 0.0), (5, "max_iterations", 257),
                       (6, "min_matches", 0), (7, "estimate_scale", 2), (9, "reserved", (0, 7))):
        vals = list(good); vals[k] = v
        rc, msg = call(vals)
        assert rc == -1 and name in msg, (name, rc, msg)
    rc, msg = call(good, initial=_lib.Similarity(float("nan"), (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
    assert rc == -1 and "scale" in msg
    bad = r.copy(); bad[29, 5] = np.inf
    rc, msg = call(good, r=bad)
    assert rc == -1 and "reference" in msg and "segment 29" in msg
    assert counters() == before
    with pytest.raises(RuntimeError, match="start_distance"):
        api.align_segments(q, ql, r, rl, 1.0, start_distance=0.5)
    with pytest.raises(ValueError):
        api.align_segments(q, ql, r, rl, 1.0, max_angle=91.0)
