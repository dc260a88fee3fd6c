"""The numpy model of DESIGN §23 (tests/align_model.py) on its own: its scalar and array forms agree byte for byte, the
hand cases come out as the contract states them, it recovers a known similarity on generated scenes and on the
reference's two published models, and the gate schedule converges from a start that the plain gate cannot use; the
library exports the new entries, checks their arguments and transforms segments without a device; the Python helpers
and the command line.  CPU only."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from line3dpp_amd import _lib, align, api, io
from tests import align_cases as Cs
from tests import align_model as A
from tests import compare_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILL = 0x5A5A5A5A

# Measured with the model: iterations and the end-point error against the known transform, as a share of the
# diagonal.  The tests assert ten times the error and at most twice the iterations.
MEASURED = dict(plain=(6, 1.2e-16), noisy=(6, 9.8e-5), shifted=(6, 5.2e-12), fixed_scale=(6, 8.0e-17))
MEASURED_REAL = (6, 1.2e-5)


def run_model(s, **kw):
    return A.align(s["q"], s["ql"], s["r"], s["rl"], initial=s["initial"], **dict(s["par"], **kw))


# ---- the two forms of the model ---------------------------------------------------------------------------------------
def test_scalar_and_array_forms_agree_byte_for_byte():
    for kw in (dict(n=40, added=8), dict(n=40, added=8, shift=1e5, estimate_scale=False)):
        s = Cs.recovery_scene(seed=3, **kw)
        a = A.align(s["q"], s["ql"], s["r"], s["rl"], initial=s["initial"], form="scalar", **s["par"])
        b = A.align(s["q"], s["ql"], s["r"], s["rl"], initial=s["initial"], form="array", **s["par"])
        Cs.same_result(b, a, f"array / scalar {kw}")
        assert a["summary"]["status"] == "CONVERGED" and a["summary"]["n_matched"] >= 25
    # past one tile: the tile tree and the sequential sum against a plain walk of the same tree
    rng = np.random.default_rng(1)
    terms = rng.normal(size=(600, A.TERMS))
    tiles = A.tile_sums(terms)
    assert tiles.shape == (3, A.TERMS)
    padded = np.zeros((768, A.TERMS)); padded[:600] = terms
    for t in range(3):
        waves = []
        for w in range(4):
            v = [padded[t * 256 + w * 64 + i] for i in range(64)]
            for stride in (32, 16, 8, 4, 2, 1):
                for i in range(stride):
                    v[i] = v[i] + v[i + stride]
            waves.append(v[0])
        assert ((waves[0] + waves[1]) + (waves[2] + waves[3])).tobytes() == tiles[t].tobytes()
    assert A.host_sum(tiles).tobytes() == (((np.zeros(A.TERMS) + tiles[0]) + tiles[1]) + tiles[2]).tobytes()


# ---- hand cases from small integers -----------------------------------------------------------------------------------
def test_a_query_on_its_reference_has_no_gradient():
    r = np.array([[1, 2, 3, 5, 2, 3], [0, 0, 0, 0, 4, 0]], np.float64)
    line = np.arange(2, dtype=np.uint32)
    c, diag = A.bounding_box(r)
    for form in ("scalar", "array"):
        moved, m, sums = A.one_pass(r, line, r, line, A.entry(None), 0.5, A.DEFAULTS, c, form)
        assert (m["segment"] == [0, 1]).all() and sums[36] == 2.0
        assert not sums[28:36].any()                           # b = 0 and cost = 0
        assert sums[0] > 0.0 and sums[A.ROW[6]] > 0.0          # ... while H is not


def test_a_displaced_query_by_hand():
    """d = (8, 0, 0), the query (0, 0, 3) off: r = (0, 0, 3) at both end points.  g_4 = e_0 - d (8 / 64) = 0, g_5 = e_1,
    g_6 = e_2: H_44 = 0, H_55 = H_66 = 2, H_56 = 0, b = (.., 0, 0, 6), cost = 9 + 9."""
    q, ql, r, rl = Cs.displaced_case()
    c, diag = A.bounding_box(r)
    assert c == (4.0, 0.0, 0.0) and diag == 8.0
    for form in ("scalar", "array"):
        moved, m, sums = A.one_pass(q, ql, r, rl, A.entry(None), 5.0, A.DEFAULTS, c, form)
        assert m["segment"][0] == 0 and m["distance"][0] == 3.0
        H = lambda i, j: sums[A.ROW[i] + j - i]
        assert sums[35] == 18.0 and sums[36] == 1.0
        assert (H(4, 4), H(4, 5), H(4, 6), H(5, 5), H(5, 6), H(6, 6)) == (0.0, 0.0, 0.0, 2.0, 0.0, 2.0)
        assert tuple(sums[32:35]) == (0.0, 0.0, 6.0)
        # z = (-4, 0, 3) and (4, 0, 3): the scale column g_3 = z - d (d.z / 64) = (0, 0, 3) twice
        assert H(3, 3) == 18.0 and H(3, 6) == 6.0 and sums[31] == 18.0
        # the rotation about y: e_1 x z = (3, 0, 4) and (3, 0, -4), less their share along d: (0, 0, 4), (0, 0, -4)
        assert H(1, 1) == 32.0 and sums[29] == 0.0


def test_parallel_references_are_degenerate():
    s = Cs.parallel_scene()
    res = A.align(s["q"], s["ql"], s["r"], s["rl"], **s["par"])
    assert res["summary"]["status"] == "DEGENERATE" and res["summary"]["iterations"] == 1 and res["summary"]["n_matched"] == 9
    assert res["similarity"] == A.entry(None) and not res["trace"]["delta"].any() and res["summary"]["last_step"] == 0.0
    assert res["trace"]["n_matched"][0] == 9 and res["summary"]["rms"] == 0.25
    assert (res["matches_q"]["segment"] == np.arange(9)).all()           # the delivery pass ran with the unchanged T


def test_too_few_matches_return_the_start_unchanged():
    s = Cs.recovery_scene()
    first = run_model(s, max_iterations=1)
    n = int(first["trace"]["n_matched"][0])
    assert n > 100
    res = run_model(s, min_matches=n + 1)
    assert res["summary"]["status"] == "TOO_FEW" and res["summary"]["iterations"] == 1
    assert res["similarity"] == A.entry(s["initial"]) and not res["trace"]["delta"].any()
    assert run_model(s, min_matches=n, max_iterations=1)["summary"]["status"] == "MAX_ITERATIONS"
    empty = A.align(s["q"], s["ql"], s["r"][:0], s["rl"][:0], initial=s["initial"], **s["par"])
    assert empty["summary"]["status"] == "TOO_FEW" and empty["summary"]["iterations"] == 0 and empty["similarity"] == A.entry(s["initial"])


# ---- recovery ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.RECOVERY))
def test_recovery_on_the_model(name):
    s = Cs.recovery_scene(**Cs.RECOVERY[name])
    res = run_model(s)
    sm = res["summary"]
    err = A.end_point_error(s["q"], res["similarity"], s["T_true"], s["diag"])
    start = A.end_point_error(s["q"], s["initial"], s["T_true"], s["diag"])
    print(f"{name}: {sm['status']} after {sm['iterations']} iterations, {sm['n_matched']} of {len(s['q'])} matched, "
          f"end-point error {err:.3g} of diag (start {start:.3g}), last step {sm['last_step']:.3g}, rms {sm['rms']:.3g}")
    iterations, measured = MEASURED[name]
    assert start > 0.03
    assert sm["status"] == "CONVERGED" and sm["iterations"] <= 2 * iterations
    assert sm["n_matched"] == s["n_kept"] == 250                          # every line that has a counterpart, no other
    assert err <= 10 * measured
    if not s["par"]["estimate_scale"]:
        assert res["similarity"]["scale"] == s["initial"]["scale"] and not res["trace"]["delta"][:, 3].any()


def test_the_gate_schedule_converges_where_the_plain_gate_finds_too_few():
    s = Cs.recovery_scene(start=Cs.FAR_START)
    plain = run_model(s, start_distance=0.0)
    scheduled = run_model(s)
    err = A.end_point_error(s["q"], scheduled["similarity"], s["T_true"], s["diag"])
    print("start", A.end_point_error(s["q"], s["initial"], s["T_true"], s["diag"]), "plain gate:", plain["summary"],
          "\nschedule:", scheduled["summary"], "end-point error", err)
    # measured: the start is 0.14 of diag off; the plain gate matches 0 lines (TOO_FEW after one iteration), the schedule
    # converges in 6 iterations with 250 matched and an error of 1.6e-16 of diag
    assert plain["summary"]["status"] == "TOO_FEW" or plain["summary"]["n_matched"] < 0.5 * s["n_kept"]
    assert scheduled["summary"]["status"] == "CONVERGED" and scheduled["summary"]["n_matched"] == s["n_kept"]
    assert scheduled["summary"]["iterations"] <= 12 and err <= 1.7e-15
    assert list(scheduled["trace"]["gate"][:3]) == [s["par"]["start_distance"] * f for f in (1.0, 0.5, 0.25)]


def test_real_models_are_aligned_back():
    s = Cs.real_scene()
    assert len(s["q"]) == 2503 and len(s["r"]) == 2501
    res = run_model(s)
    sm = res["summary"]
    err = A.end_point_error(s["q"], res["similarity"], s["T_true"], s["diag"])
    share_q = (res["matches_q"]["segment"] >= 0).mean(); share_r = (res["matches_r"]["segment"] >= 0).mean()
    print(sm, "matched share", share_q, share_r, "end-point error", err, "start", A.end_point_error(s["q"], s["initial"], s["T_true"], s["diag"]))
    assert sm["status"] == "CONVERGED" and sm["iterations"] <= 2 * MEASURED_REAL[0]
    assert share_q >= 0.99 and share_r >= 0.99
    assert err <= 10 * MEASURED_REAL[1]


# ---- the library's side, as far as it goes without a device -----------------------------------------------------------
def test_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    L = _lib.load()
    for name in ("l3d_align_segments", "l3d_align_lines", "l3d_transform_segments"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    for name in ("l3d_similarity", "l3d_align_params", "l3d_align_summary", "l3d_align_iteration"):
        assert "typedef struct " + name in hdr
    for name in ("align_iterations", "align_normal_launches", "align_kernel_ns"):
        assert L.l3d_debug_counter(name.encode()) != L.l3d_debug_counter(b"no such counter")
    assert "l3d_align_segments" in hdr[hdr.index("similarity transform is estimated"):hdr.index("typedef struct l3d_compare_params")]


def test_struct_layouts():
    assert C.sizeof(_lib.Similarity) == 64 and C.sizeof(_lib.AlignParams) == 64 and C.sizeof(_lib.AlignSummary) == 64
    assert _lib.ALIGN_ITERATION_DTYPE.itemsize == 432 and _lib.ALIGN_ITERATION_DTYPE == A.ITERATION_DTYPE
    assert _lib.SIMILARITY_DTYPE == A.SIMILARITY_DTYPE and _lib.ALIGN_STATUS == A.STATUS
    assert tuple(f for f, _ in _lib.AlignSummary._fields_) == A.SUMMARY_KEYS
    p = api.align_params(0.25, 2.0, 10.0, 0.5, 1e-6, 30, 5, False, 3)
    assert (p.max_distance, p.min_cos2, p.min_overlap, p.start_distance, p.step_tolerance, p.max_iterations, p.min_matches,
            p.estimate_scale, p.slice_chunks, tuple(p.reserved)) == (0.25, CM.min_cos2_of(10.0), 0.5, 2.0, 1e-6, 30, 5, 0, 3, (0, 0))
    assert api.align_params(1.0).step_tolerance == 1e-9
    with pytest.raises(ValueError, match="max_angle"):
        api.align_params(1.0, max_angle=91.0)


GOOD = (0.5, 0.9, 0.5, 0.0, 1e-9, 20, 3, 1, 0, (0, 0))


def test_argument_checks_need_no_device():
    """the checks come before any device work: they answer on a machine without a GPU as well"""
    L = _lib.load()
    s = Cs.edge_scene(4, 3)
    q, ql, r, rl = s["q"], s["ql"], s["r"], s["rl"]
    outs = dict(sim=np.full(16, FILL, np.uint32), summary=np.full(16, FILL, np.uint32), segs=np.full(4 * 12, FILL, np.uint32),
                mq=np.full(4 * 6, FILL, np.uint32), mr=np.full(3 * 6, FILL, np.uint32), trace=np.full(256 * 108, FILL, np.uint32))
    p = _lib.ptr

    def untouched():
        return all((x == FILL).all() for x in outs.values())

    def call(par, q=q, ql=ql, r=r, rl=rl, n_q=4, n_r=3, null=(), initial=None):
        a = dict(q=p(q), ql=p(ql), r=p(r), rl=p(rl), sim=p(outs["sim"]), summary=p(outs["summary"]))
        for k in null:
            a[k] = None
        rc = L.l3d_align_segments(0, n_q, a["q"], a["ql"], n_r, a["r"], a["rl"], C.byref(par) if par is not None else None,
                                  C.byref(initial) if initial is not None else None,
                                  C.cast(a["sim"], C.POINTER(_lib.Similarity)), C.cast(a["summary"], C.POINTER(_lib.AlignSummary)),
                                  p(outs["segs"]), p(outs["mq"]), p(outs["mr"]), p(outs["trace"]))
        assert untouched()
        return rc, _lib.last_error()

    inf, nan = float("inf"), float("nan")
    for k, name, bad in ((0, "max_distance", (-1.0, inf, nan)), (1, "min_cos2", (-0.1, 1.1, nan)), (2, "min_overlap", (-0.1, 1.1, nan)),
                         (3, "start_distance", (0.25, -1.0, inf, nan)), (4, "step_tolerance", (0.0, -1e-9, inf, nan)),
                         (5, "max_iterations", (0, 257, 0xFFFFFFFF)), (6, "min_matches", (0,)), (7, "estimate_scale", (2, 0xFFFFFFFF)),
                         (9, "reserved", ((1, 0), (0, 1)))):
        for v in bad:
            vals = list(GOOD); vals[k] = v
            rc, msg = call(_lib.AlignParams(*vals))
            assert rc == -1 and name in msg, (name, v, rc, msg)
    rc, msg = call(None)
    assert rc == -1 and "null" in msg
    good = _lib.AlignParams(*GOOD)
    unit = ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    for word, sim in (("scale", (0.0,) + unit), ("scale", (-1.0,) + unit), ("scale", (nan,) + unit), ("scale", (inf,) + unit),
                      ("quaternion", (1.0, (0.0, 0.0, 0.0, 0.0), unit[1])), ("quaternion", (1.0, (1.0, nan, 0.0, 0.0), unit[1])),
                      ("quaternion", (1.0, (1e200, 0.0, 0.0, 0.0), unit[1])), ("translation", (1.0, unit[0], (0.0, inf, 0.0))),
                      ("translation", (1.0, unit[0], (nan, 0.0, 0.0)))):
        rc, msg = call(good, initial=_lib.Similarity(*sim))
        assert rc == -1 and "similarity" in msg and word in msg, (sim, rc, msg)
    for bad_value in (np.inf, np.nan, -(2.0 ** 101)):
        bad_q = q.copy(); bad_q[2, 4] = bad_value
        rc, msg = call(good, q=bad_q)
        assert rc == -1 and "query" in msg and "segment 2" in msg, msg
        bad_r = r.copy(); bad_r[1, 0] = bad_value
        rc, msg = call(good, r=bad_r)
        assert rc == -1 and "reference" in msg and "segment 1" in msg, msg
    rc, msg = call(good, n_r=1 << 30)
    assert rc == -9 and "2^30" in msg and "reference" in msg
    for k in ("q", "ql", "r", "rl", "sim", "summary"):
        rc, msg = call(good, null=(k,))
        assert rc == -1 and "null" in msg, k
    point = np.tile(np.array([[1.0, 2.0, 3.0, 1.0, 2.0, 3.0]]), (3, 1))
    rc, msg = call(good, r=point)
    assert rc == -1 and "bounding box" in msg
    # the context form and the host-only entry check their arguments first as well
    S, Y = C.cast(p(outs["sim"]), C.POINTER(_lib.Similarity)), C.cast(p(outs["summary"]), C.POINTER(_lib.AlignSummary))
    assert L.l3d_align_lines(None, 3, p(r), p(rl), C.byref(good), None, S, Y, None, None, None, None) == -1 and "null" in _lib.last_error()
    assert L.l3d_transform_segments(4, p(q), None, p(outs["segs"])) == -1 and "null" in _lib.last_error()
    assert L.l3d_transform_segments(4, None, C.byref(_lib.Similarity(1.0, *unit)), p(outs["segs"])) == -1
    assert L.l3d_transform_segments(4, p(q), C.byref(_lib.Similarity(0.0, *unit)), p(outs["segs"])) == -1 and "scale" in _lib.last_error()
    assert untouched()


def test_empty_forms_need_no_device():
    s = Cs.edge_scene(5, 4)
    start = dict(scale=2.0, q=(2.0, 0.0, 0.0, 2.0), t=(1.0, 2.0, 3.0))
    for n_q, n_r in ((5, 0), (0, 4), (0, 0)):
        res = api.align_segments(s["q"][:n_q], s["ql"][:n_q], s["r"][:n_r], s["rl"][:n_r], 0.5, initial=start)
        want = A.align(s["q"][:n_q], s["ql"][:n_q], s["r"][:n_r], s["rl"][:n_r], 0.5, initial=start)
        Cs.same_result(res, want, f"empty form ({n_q}, {n_r})")
        assert res["summary"]["status"] == "TOO_FEW" and res["summary"]["iterations"] == 0 and len(res["trace"]) == 0
        assert tuple(res["similarity"]["q"]) == A.unit(start["q"]) and (res["matches_q"]["segment"] == -1).all()


def test_transform_segments_equals_the_model_bit_for_bit():
    rng = np.random.default_rng(2)
    segs = rng.uniform(-5, 5, (300, 6))
    for T in (A.similarity(1.3, Cs.axis_angle([1, -2, 0.5], 25.0), (1e5, -3.0, 0.25)), A.similarity(0.01, (3.0, -1.0, 2.0, 0.5), (0.0, 0.0, 0.0)),
              A.similarity(**A.IDENTITY)):
        got = api.transform_segments(segs, T)
        Cs.same_bytes(got, A.transform(segs, T), "l3d_transform_segments / the array form")
        Cs.same_bytes(got[:20], A.transform(segs[:20], T, "scalar"), "l3d_transform_segments / the scalar form")
        M = api.similarity_matrix(T)
        assert M.tobytes() == A.matrix(T).tobytes()
        pts = segs.reshape(-1, 3) @ M[:3, :3].T + M[:3, 3]
        assert np.abs(pts - got.reshape(-1, 3)).max() <= 1e-10 * max(1.0, np.abs(pts).max())
    assert api.transform_segments(np.zeros((0, 6)), A.similarity(**A.IDENTITY)).shape == (0, 6)
    with pytest.raises(RuntimeError, match="quaternion"):
        api.transform_segments(segs, A.similarity(1.0, (0, 0, 0, 0), (0, 0, 0)))


# ---- the Python helpers -----------------------------------------------------------------------------------------------
def test_similarity_from_points_recovers_a_known_transform():
    """exact correspondences: Umeyama's closed form against the matrix that made them, within ten times the error of
    numpy's own least-squares solution of the same points (measured: lstsq 4.7e-15, Umeyama 7.1e-15)"""
    rng = np.random.default_rng(5)
    src = rng.uniform(-3, 3, (40, 3))
    T = A.entry(A.similarity(2.5, Cs.axis_angle([1, 2, 3], 70.0), (10.0, -20.0, 5.0)))
    M = A.matrix(T)
    dst = src @ M[:3, :3].T + M[:3, 3]
    X = np.linalg.lstsq(np.c_[src, np.ones(len(src))], dst, rcond=None)[0].T
    yard = float(np.abs(X - M[:3]).max())
    got = api.similarity_from_points(src, dst)
    dev = float(np.abs(api.similarity_matrix(got)[:3] - M[:3]).max())
    print("lstsq deviation", yard, "Umeyama deviation", dev)
    assert 0.0 < yard < 1e-13 and dev <= 10 * yard
    fixed = api.similarity_from_points(src, (dst - M[:3, 3]) / 2.5 + M[:3, 3], with_scale=False)
    assert fixed["scale"] == 1.0 and np.abs(fixed["q"] - np.array(T["q"])).max() <= 10 * yard
    back = api.similarity_from_matrix(M)
    assert abs(back["scale"] - 2.5) <= 10 * yard and np.abs(back["q"] - np.array(T["q"])).max() <= 10 * yard and (back["t"] == M[:3, 3]).all()
    assert api.similarity_from_matrix(M[:3])["scale"] == back["scale"]
    for bad in (np.zeros((3, 4)), np.eye(3), np.diag([1.0, 2.0, 3.0, 1.0]), -np.eye(4)):
        with pytest.raises(ValueError):
            api.similarity_from_matrix(bad)
    with pytest.raises(ValueError):
        api.similarity_from_points(src[:2], dst[:2])


# ---- the command line, with the model in the library's place -----------------------------------------------------------
def model_align_segments(q_segs, q_line, r_segs, r_line, max_distance, start_distance=0.0, initial=None, estimate_scale=True,
                         max_angle=10.0, min_overlap=0.5, step_tolerance=1e-9, max_iterations=50, min_matches=8, slice_chunks=0, device=0):
    if initial is not None and not isinstance(initial, dict):
        initial = api.similarity_from_matrix(initial)
    res = A.align(q_segs, q_line, r_segs, r_line, max_distance, initial=initial, start_distance=start_distance,
                  estimate_scale=int(estimate_scale), min_cos2=CM.min_cos2_of(max_angle), min_overlap=min_overlap,
                  step_tolerance=step_tolerance, max_iterations=max_iterations, min_matches=min_matches)
    res["matrix"] = A.matrix(res["similarity"])
    return res


def test_command_line(tmp_path, capsys):
    b = os.path.join(GOLDEN, "ref_lines3d_excerpt.txt")
    lines = io.read_3d_lines_txt(b)
    segs, line = api.flatten_lines(lines)
    c, diag = A.bounding_box(segs)
    T_true = A.entry(A.similarity(1.7, Cs.axis_angle([0.2, 1.0, -0.4], 50.0), (5.0, 6.0, -7.0)))
    Minv = np.linalg.inv(A.matrix(T_true))
    moved = [dict(L, segments=np.concatenate([L["segments"][:, :3] @ Minv[:3, :3].T + Minv[:3, 3],
                                              L["segments"][:, 3:] @ Minv[:3, :3].T + Minv[:3, 3]], 1)) for L in lines]
    a = str(tmp_path / "a.txt")
    with open(a, "w") as f:
        f.write(io.format_3d_lines_txt(moved))
    init = str(tmp_path / "init.txt")
    np.savetxt(init, A.matrix(Cs.perturbed(T_true, c, diag, 1.0, 0.01, 0.005, np.random.default_rng(4)))[:3], fmt="%.17g")
    out = str(tmp_path / "moved.txt")
    md = 0.002 * diag
    assert align.main([a, b, "-d", repr(md), "-s", repr(16 * md), "--init", init, "--out", out], align_segments=model_align_segments) == 0
    res = json.loads(capsys.readouterr().out)
    assert res["summary"]["status"] == "CONVERGED" and res["summary"]["n_matched"] == len(segs) == res["a_in_b"]["n_matched"]
    assert res["b_in_a"]["n_matched"] == len(segs) and res["a_in_b"]["n_lines_matched"] == len(lines)
    # (the text form of A keeps six digits: the transform is recovered to that)
    assert np.abs(np.array(res["matrix"]) - A.matrix(T_true)).max() <= 1e-5 * diag
    assert abs(res["similarity"]["scale"] - 1.7) < 1e-5 and res["max_distance"] == md and res["estimate_scale"] is True
    back, _ = api.flatten_lines(io.read_3d_lines_txt(out))
    assert back.shape == segs.shape and np.abs(back - segs).max() <= 1e-5 * diag      # (the text form keeps six digits)
    seen = {}

    def spy(*args, **kw):
        seen.update(kw)
        return model_align_segments(*args, **kw)
    assert align.main([b, b, "-d", "0.01", "--no-scale", "-a", "20", "-o", "0.25"], align_segments=spy) == 0
    res = json.loads(capsys.readouterr().out)
    assert seen["estimate_scale"] is False and seen["max_angle"] == 20.0 and seen["min_overlap"] == 0.25 and seen["initial"] is None
    assert res["similarity"]["scale"] == 1.0 and res["out"] is None
    with pytest.raises(SystemExit):
        align.main([a, b], align_segments=model_align_segments)
    assert "usage" in capsys.readouterr().err
    assert align.main([a, str(tmp_path / "none.txt"), "-d", "1"], align_segments=model_align_segments) == 1
    assert "no such file" in capsys.readouterr().err
    assert align.main([a, b, "-d", "1", "--out", str(tmp_path / "x.bin")], align_segments=model_align_segments) == 1
    assert ".txt" in capsys.readouterr().err
    np.savetxt(init, np.eye(3))
    assert align.main([a, b, "-d", "1", "--init", init], align_segments=model_align_segments) == 1
    assert "3x4 or 4x4" in capsys.readouterr().err
