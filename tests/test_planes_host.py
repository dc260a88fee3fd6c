"""The numpy model of DESIGN §25 (tests/planes_model.py) on its own: the scalar and array forms of stages 1 and 2 agree, the
generated cases meet the admission rule and the hand-built cases come out as the contract states them; stages 0 and 3 of
the library (l3d_planes.h), compiled into a stand-alone program, return the model's bytes; the library exports the new
entries and checks their arguments without a device; the command line.  CPU only."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib, api, io, planes
from tests import planes_cases as Cs
from tests import planes_model as M
from tests import wireframe_model as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_scalar_and_array_forms_are_identical():
    live = 0
    for n in (63, 256, 0, 1):
        segs, line, _ = Cs.sized_case(n)
        w = M.weights(segs)
        rec = W.junctions(segs, line, Cs.PAR["junction_distance"], Cs.PAR["junction_extension"], Cs.PAR["min_sin2"])
        a, b = M.hypotheses_scalar(segs, rec), M.hypotheses(segs, rec)
        assert a.dtype == b.dtype == M.HYP_DTYPE and a.tobytes() == b.tobytes(), n
        for chunk in (256, 7):
            sa, sb = M.scores_scalar(segs, w, a, Cs.MD), M.scores(segs, w, a, Cs.MD, chunk=chunk)
            assert sa.dtype == sb.dtype == M.SCORE_DTYPE and sa.tobytes() == sb.tobytes(), (n, chunk)
        assert not np.isnan(a["N"]).any() and not np.isnan(a["J"]).any()
        live += int((sa["count"] >= 8).sum())
    assert live >= 100                                          # the cases exercise the inliers, not only their absence
    # the dead hypotheses, both forms
    segs = Cs.segs(Cs.dead_fan(5)); line = np.arange(6, dtype=np.uint32)
    rec = W.junctions(segs, line, 0.25, 0.25, 0.03)
    assert len(rec) == 5 and M.hypotheses_scalar(segs, rec).tobytes() == M.hypotheses(segs, rec).tobytes()
    assert not M.hypotheses(segs, rec)["live"].any()


def test_the_weights_are_integers_below_2_53():
    for n in (513, 63):
        segs, _, _ = Cs.sized_case(n)
        w = M.weights(segs)
        assert 2 ** 51 - 2 * n <= sum(w["q"]) < 2 ** 53 and w["n_points"] == w["live"].count(False) and all(q == 0 for q, ok in zip(w["q"], w["live"]) if not ok)
        m, x = np.frexp(w["length_total"])
        assert 0.5 <= m < 1 and w["e"] == 52 - x
    # lengths at both ends of the range: 2^100 and 2^-300 in one model
    w = M.weights([[0, 0, 0, 2.0 ** 100, 0, 0], [0, 0, 0, 2.0 ** -300, 0, 0]])
    assert w["e"] == 52 - 101 and w["q"] == [2 ** 51, 0] and w["live"] == [True, True]


@pytest.mark.parametrize("n", Cs.EDGE_N + (Cs.SLICING_N,))
def test_generated_cases_are_admitted(n):
    segs, line, planted = Cs.sized_case(n)
    assert len(segs) == n
    assert Cs.admitted(M.detect(segs, line, Cs.PAR), planted) is None


def test_hand_built_cases():
    for name, segs, line, par, expected in Cs.hand_cases():
        for form in ("scalar", "array"):
            Cs.check_expected(f"{name} ({form})", M.detect(segs, line, par, form), expected)


def test_two_segments_of_length_2_pow_minus_300_span_a_dead_hypothesis():
    """m2 = |ea x eb|^2 underflows.  So does den = A C - B B of §24, which is the same number: stage 1 never hands such a
    pair on, and the record is made by hand here.  Cs.dead_fan is the pair that does reach stage 1."""
    s = 2.0 ** -300
    segs = Cs.segs([(0, 0, 0, s, 0, 0), (0, 0, 0, 0, s, 0)])
    assert len(W.junctions(segs, [0, 1], 0.25, 0.25, 0.0)) == 0
    rec = np.zeros(1, W.RECORD_DTYPE); rec["b"] = 1
    for form in (M.hypotheses_scalar, M.hypotheses):
        h = form(segs, rec)
        assert h["live"][0] == 0 and not h["N"].any() and not h["J"].any()
    w = M.weights(segs)
    assert M.scores(segs, w, h, 0.25).tobytes() == M.scores_scalar(segs, w, h, 0.25).tobytes() == bytes(16)


def test_the_comb_and_the_fan_have_the_hypotheses_they_state():
    for teeth in (255, 256, 257):
        g = Cs.segs(Cs.comb(teeth))
        rec = W.junctions(g, np.arange(len(g)), 0.25, 0.25, 0.03)
        assert len(rec) == teeth and (rec["a"] == 0).all()
    g = Cs.segs(Cs.dead_fan())
    rec = W.junctions(g, np.arange(len(g)), 0.25, 0.25, 0.03)
    assert len(rec) == 256 and (rec["sa"] == 0).all() and not M.hypotheses(g, rec)["live"].any()


# ---- stages 0 and 3 of the library against the model ------------------------------------------------------------------
@pytest.fixture(scope="module")
def select_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pl") / "planes_select")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cpp", "planes_select.cpp"),
                           "-o", exe])
    return exe


def c_params(par, slice_chunks=0):
    return _lib.PlanesParams(par["max_distance"], par["junction_distance"], par["junction_extension"], par["min_sin2"], par["min_length"],
                             par["min_segments"], par["max_planes"], par["max_tests"], slice_chunks, (0, 0))


def run_select_program(exe, tmp_path, segs, line, par, hyp, score, expect=0):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "planes.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<2I", len(segs), len(hyp))); f.write(bytes(c_params(par)))
        f.write(np.ascontiguousarray(segs, np.float64).tobytes()); f.write(np.ascontiguousarray(line, np.uint32).tobytes())
        f.write(np.ascontiguousarray(hyp, M.HYP_DTYPE).tobytes()); f.write(np.ascontiguousarray(score, M.SCORE_DTYPE).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == expect, out.stdout + out.stderr
    if expect:
        return out.stdout
    raw = open(dst, "rb").read()
    n_p, n_m, n_s = struct.unpack_from("<3Q", raw, 0)
    pos = 24
    got = {}
    for name, dtype, count in (("planes", M.PLANE_DTYPE, n_p), ("members", M.MEMBER_DTYPE, n_m), ("seg_planes", np.dtype("<u4"), n_s)):
        got[name] = np.frombuffer(raw, dtype, count, pos); pos += dtype.itemsize * count
    got["summary"] = dict(zip(M.SUMMARY_KEYS, struct.unpack_from(M.SUMMARY_FORMAT, raw, pos))); pos += 136
    got["weights"] = np.frombuffer(raw, "<u8", len(segs), pos)
    assert pos + 8 * len(segs) == len(raw)
    got["scores"] = np.ascontiguousarray(score, M.SCORE_DTYPE)
    return got


def model_stages(segs, line, par):
    w = M.weights(segs)
    rec = W.junctions(segs, line, par["junction_distance"], par["junction_extension"], par["min_sin2"])
    hyp = M.hypotheses(segs, rec)
    return w, hyp, M.scores(segs, w, hyp, par["max_distance"])


def test_stages_0_and_3_of_the_library_return_the_models_bytes(select_program, tmp_path):
    cases = [(name, segs, line, par) for name, segs, line, par, _ in Cs.hand_cases()]
    cases += [(f"generated {n}", *Cs.sized_case(n)[:2], par) for n, par in
              ((513, Cs.PAR), (768, dict(Cs.PAR, min_length=40.0)), (257, dict(Cs.PAR, min_segments=4, max_tests=3)), (63, M.params(0.2, min_segments=3)))]
    planes = 0
    for name, segs, line, par in cases:
        w, hyp, score = model_stages(segs, line, par)
        want = M.select(segs, line, w, hyp, score, par)
        got = run_select_program(select_program, tmp_path, segs, line, par, hyp, score)
        assert got["weights"].tolist() == w["q"], name
        Cs.same_result(got, want, name)
        planes += len(want["planes"])
    assert planes >= 30
    # the refit is a fit: its rms is not above the generating plane's by more than rounding, and its normal is a unit vector
    segs, line, _ = Cs.sized_case(513)
    P = M.detect(segs, line, Cs.PAR)["planes"]
    assert len(P) == 2 and (P["rms_fit"] <= P["rms"] * (1 + 1e-9)).all() and (P["rms_fit"] > 0).all()
    assert np.allclose((P["N_fit"] ** 2).sum(1), 1.0, rtol=0, atol=1e-15) and ((P["N_fit"] * P["N"]).sum(1) > 0.999).all()


def test_the_jacobi_finds_the_smallest_eigenvector():
    rng = np.random.default_rng(9)
    for _ in range(50):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        lam = np.sort(rng.uniform(0.1, 10.0, 3)) * [1e-6, 1.0, 1.0]
        S = (q * lam) @ q.T
        v = np.array(M.smallest_eigenvector([float(S[i, j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]))
        # the error of a Jacobi eigenvector is of the order of eps * |S| / the gap to the next eigenvalue: 1e-16 * 10 / 0.1
        assert abs(abs(v @ q[:, 0]) - 1.0) < 1e-12 and abs(v @ v - 1.0) < 1e-15
    assert M.smallest_eigenvector([3.0, 0.0, 0.0, 2.0, 0.0, 1.0]) == [0.0, 0.0, 1.0]      # a diagonal matrix: no rotation
    assert M.smallest_eigenvector([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]) == [1.0, 0.0, 0.0]      # the first of equals


def test_a_score_that_differs_from_the_members_is_named(select_program, tmp_path):
    name, segs, line, par, _ = Cs.hand_cases()[0]
    w, hyp, score = model_stages(segs, line, par)
    bad = score.copy(); bad["weight"][5] += 1
    assert "hypothesis 5" in run_select_program(select_program, tmp_path, segs, line, par, hyp, bad, expect=9)


# ---- the library's side, as far as it goes without a device -----------------------------------------------------------
ENTRIES = ("l3d_plane_segments", "l3d_plane_lines", "l3d_planes_counts", "l3d_planes_get", "l3d_planes_save_obj", "l3d_planes_close")
COUNTERS = ("pl_score_launches", "pl_slices", "pl_hypotheses", "pl_kernel_ns", "pl_junction_ns")


def test_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    L = _lib.load()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    for name in ("l3d_planes_params", "l3d_pl_plane", "l3d_pl_member", "l3d_pl_score", "l3d_planes_summary"):
        assert "typedef struct " + name in hdr
    for name in COUNTERS:
        assert L.l3d_debug_counter(name.encode()) != L.l3d_debug_counter(b"no such counter")
    facade = open(os.path.join(ROOT, "include", "line3dpp", "line3D.h")).read()
    assert re.search(r"\bdetectPlanes\s*\(", facade)


def test_struct_layouts():
    assert C.sizeof(_lib.PlanesParams) == 64 and C.sizeof(_lib.PlanesSummary) == 136
    assert _lib.PL_PLANE_DTYPE == M.PLANE_DTYPE and _lib.PL_MEMBER_DTYPE == M.MEMBER_DTYPE and _lib.PL_SCORE_DTYPE == M.SCORE_DTYPE
    assert (M.PLANE_DTYPE.itemsize, M.MEMBER_DTYPE.itemsize, M.SCORE_DTYPE.itemsize, M.HYP_DTYPE.itemsize) == (264, 8, 16, 64)
    assert tuple(f for f, _ in _lib.PlanesSummary._fields_) == M.SUMMARY_KEYS and struct.calcsize(M.SUMMARY_FORMAT) == 136
    assert [f for f, _ in _lib.PlanesParams._fields_] == ["max_distance", "junction_distance", "junction_extension", "min_sin2", "min_length",
                                                           "min_segments", "max_planes", "max_tests", "slice_chunks", "reserved"]


def test_planes_params_follow_wireframe_params():
    p = api.planes_params(0.25, 0.5, 0.75, 20.0, 3.0, 5, 6, 7, 2)
    assert (p.max_distance, p.junction_distance, p.junction_extension, p.min_sin2, p.min_length, p.min_segments, p.max_planes, p.max_tests,
            p.slice_chunks, tuple(p.reserved)) == (0.25, 0.5, 0.75, M.min_sin2_of(20.0), 3.0, 5, 6, 7, 2, (0, 0))
    p = api.planes_params(0.25)
    assert (p.junction_distance, p.junction_extension, p.min_sin2, p.min_length, p.min_segments, p.max_planes, p.max_tests, p.slice_chunks) == \
        (0.25, 0.25, M.min_sin2_of(10.0), 0.0, 4, 64, 4096, 0)
    assert api.planes_params(1.0, 0.0, 0.0).junction_distance == 0.0 and api.planes_params(1.0, 0.0, 0.0).junction_extension == 0.0
    for bad in (-1.0, 90.5, float("nan")):
        with pytest.raises(ValueError, match="min_angle"):
            api.planes_params(1.0, min_angle=bad)


FILL = 0x5A5A5A5A5A5A5A5A
OK = (0.5, 0.5, 0.5, 0.03, 0.0, 4, 64, 4096, 0, (0, 0))


def call(par, segs=None, line=None, n=None, null=()):
    """l3d_plane_segments with a handle slot filled with a pattern, which every refused call must leave as it was"""
    L = _lib.load()
    base_segs, base_line, _ = Cs.sized_case(8)
    segs = base_segs if segs is None else segs; line = base_line if line is None else line
    slot = C.c_void_p(FILL)
    rc = L.l3d_plane_segments(0, len(line) if n is None else n, None if "segs" in null else _lib.ptr(segs),
                              None if "line" in null else _lib.ptr(line), C.byref(par) if par is not None else None,
                              None if "out" in null else C.byref(slot))
    assert rc != 0 and slot.value == FILL
    return rc, _lib.last_error()


def test_argument_checks_need_no_device():
    """the checks come before any device work: they answer on a machine without a GPU as well"""
    not_a_distance = (-1.0, float("inf"), float("nan"))
    for k, name, bad in ((0, "max_distance", not_a_distance), (1, "junction_distance", not_a_distance), (2, "junction_extension", not_a_distance),
                         (3, "min_sin2", (-0.1, 1.1, float("nan"))), (4, "min_length", not_a_distance), (5, "min_segments", (0,)),
                         (6, "max_planes", (0,)), (7, "max_tests", (0,)), (9, "reserved", ((1, 0), (0, 1), (0xFFFFFFFF, 0)))):
        for v in bad:
            vals = list(OK); vals[k] = v
            rc, msg = call(_lib.PlanesParams(*vals))
            assert rc == -1 and name in msg, (name, v, rc, msg)
    rc, msg = call(None)
    assert rc == -1 and "null" in msg
    good = _lib.PlanesParams(*OK)
    base = Cs.sized_case(8)[0]
    for bad_value in (np.inf, -np.inf, np.nan, 2.0 ** 101, -(2.0 ** 101)):
        bad = base.copy(); bad[2, 4] = bad_value
        rc, msg = call(good, segs=bad)
        assert rc == -1 and "segment 2" in msg and "2^100" in msg, msg
    for n in (1 << 30, 0xFFFFFFFF):
        rc, msg = call(good, n=n)
        assert rc == -9 and "2^30" in msg, msg
    for k in ("segs", "line", "out"):
        rc, msg = call(good, null=(k,))
        assert rc == -1 and "null" in msg, k
    # the context form and the handle's entries check their arguments first as well
    L = _lib.load()
    slot = C.c_void_p(FILL)
    assert L.l3d_plane_lines(None, C.byref(good), C.byref(slot)) == -1 and "null" in _lib.last_error() and slot.value == FILL
    assert L.l3d_planes_counts(None, None, None, None) == -1 and L.l3d_planes_get(None, None, None, None, None, None) == -1
    assert L.l3d_planes_save_obj(None, b"x.obj") == -1
    L.l3d_planes_close(None)                                 # (as free(NULL))


def test_empty_model_needs_no_device(tmp_path):
    L = _lib.load()
    good = _lib.PlanesParams(*OK)
    h = C.c_void_p()
    assert L.l3d_plane_segments(0, 0, None, None, C.byref(good), C.byref(h)) == 0 and h.value
    n_p = C.c_uint64(7); n_m = C.c_uint64(7); n_h = C.c_uint64(7)
    s = _lib.PlanesSummary(n_segments=7, scale_exponent=-3, length_total=1.0, max_rms=2.0)
    assert L.l3d_planes_counts(h, C.byref(n_p), C.byref(n_m), C.byref(n_h)) == 0 and (n_p.value, n_m.value, n_h.value) == (0, 0, 0)
    assert L.l3d_planes_get(h, None, None, None, None, C.byref(s)) == 0 and all(getattr(s, f) == 0 for f in M.SUMMARY_KEYS)
    path = str(tmp_path / "empty.obj")
    assert L.l3d_planes_save_obj(h, path.encode()) == 0 and open(path).read() == ""
    assert L.l3d_planes_save_obj(h, str(tmp_path / "no" / "such" / "dir.obj").encode()) == -11 and "cannot write" in _lib.last_error()
    L.l3d_planes_close(h)
    got = api.detect_planes(np.zeros((0, 6)), np.zeros(0, np.uint32), 0.5)
    Cs.same_result(got, M.detect(np.zeros((0, 6)), np.zeros(0, np.uint32), M.params(0.5)), "the empty model")
    with pytest.raises(ValueError, match="one line index"):
        api.detect_planes(np.zeros((2, 6)), np.zeros(1, np.uint32), 0.5)


# ---- the command line, with the model in the library's place ----------------------------------------------------------
def model_detect_planes(segs, line, max_distance, junction_distance=None, junction_extension=None, min_angle=10.0, min_length=0.0,
                        min_segments=4, max_planes=64, max_tests=4096, slice_chunks=0, device=0, obj_path=None):
    p = api.planes_params(max_distance, junction_distance, junction_extension, min_angle, min_length, min_segments, max_planes, max_tests)
    return M.detect(segs, line, M.params(p.max_distance, p.junction_distance, p.junction_extension, p.min_sin2, p.min_length,
                                         p.min_segments, p.max_planes, p.max_tests))


def test_command_line(tmp_path, capsys):
    """the excerpt's lines and a rectangle with its two diagonals beside them"""
    lines = io.read_3d_lines_txt(os.path.join(GOLDEN, "ref_lines3d_excerpt.txt"))
    ex_segs, _ = api.flatten_lines(lines)
    size = M.extent(ex_segs)
    o = ex_segs.reshape(-1, 3).max(0) + size
    u, v = np.array([size, 0, 0]), np.array([0, size, size]) / 2

    def one(a, b):
        return dict(segments=np.concatenate([a, b]).reshape(1, 6), residuals=np.zeros((0, 2), np.uint32), coords2D=np.zeros((0, 4), np.float32))
    more = [one(o, o + u), one(o + u, o + u + v), one(o + u + v, o + v), one(o + v, o), one(o, o + u + v), one(o + u, o + v)]
    src = str(tmp_path / "model.txt")
    with open(src, "w") as f:
        f.write(io.format_3d_lines_txt(lines + more))
    seen = {}

    def spy(*args, **kw):
        seen.update(kw)
        return model_detect_planes(*args, **kw)
    out = str(tmp_path / "planes.obj")
    md = 1e-3 * size                                        # (the text file keeps six digits of every coordinate)
    argv = [src, out, "-d", repr(md), "-j", repr(2 * md), "-x", repr(3 * md), "-a", "20", "-l", repr(size), "-s", "5", "-p", "9"]
    assert planes.main(argv, detect_planes=spy) == 0
    res = json.loads(capsys.readouterr().out)
    assert (seen["max_distance"], seen["junction_distance"], seen["junction_extension"], seen["min_angle"], seen["min_length"],
            seen["min_segments"], seen["max_planes"]) == (md, 2 * md, 3 * md, 20.0, size, 5, 9)
    segs, line = api.flatten_lines(io.read_3d_lines_txt(src))
    want = M.detect(segs, line, M.params(md, 2 * md, 3 * md, M.min_sin2_of(20.0), size, 5, 9))
    for k in M.SUMMARY_KEYS:
        assert res[k] == want["summary"][k], k
    n0 = len(line) - 6
    assert res["n_planes"] >= 1 and want["members"]["segment"][want["members"]["plane"] == 0].tolist() == list(range(n0, n0 + 6))
    assert res["max_distance"] == md and res["junction_distance"] == 2 * md and res["input"] == src and res["output"] == out
    text = open(out).read()
    assert text == M.obj_text(want)
    rows = [ln.split() for ln in text.splitlines()]
    v_rows = [r for r in rows if r[0] == "v"]; f_rows = [r for r in rows if r[0] == "f"]
    assert len(v_rows) == 4 * res["n_planes"] and len(f_rows) == res["n_planes"] and len(rows) == 5 * res["n_planes"]
    assert np.array_equal(np.array([[float(x) for x in r[1:]] for r in v_rows]).reshape(-1, 4, 3), want["planes"]["corners"])   # %.17g reads back exactly
    assert [[int(x) for x in r[1:]] for r in f_rows] == [[4 * k + 1, 4 * k + 2, 4 * k + 3, 4 * k + 4] for k in range(res["n_planes"])]
    # -j and -x default to -d; a .bin input
    assert planes.main([os.path.join(GOLDEN, "ref_lines3d_excerpt.bin"), out, "-d", "0.5"], detect_planes=spy) == 0
    res = json.loads(capsys.readouterr().out)
    assert seen["junction_distance"] is None and seen["junction_extension"] is None and res["junction_distance"] == 0.5
    assert res["junction_extension"] == 0.5 and res["min_angle"] == 10.0 and res["min_segments"] == 4 and res["n_segments"] > 3
    # -d is required; both files; the extensions; a missing file; an angle outside [0, 90]
    for argv in ([src, out], [src, "-d", "1"]):
        with pytest.raises(SystemExit):
            planes.main(argv, detect_planes=model_detect_planes)
        assert "usage" in capsys.readouterr().err
    assert planes.main([str(tmp_path / "model.obj"), out, "-d", "1"], detect_planes=model_detect_planes) == 1
    assert ".txt or .bin" in capsys.readouterr().err
    assert planes.main([src, str(tmp_path / "planes.txt"), "-d", "1"], detect_planes=model_detect_planes) == 1
    assert "written as .obj" in capsys.readouterr().err
    assert planes.main([str(tmp_path / "none.txt"), out, "-d", "1"], detect_planes=model_detect_planes) == 1
    assert "no such file" in capsys.readouterr().err
    assert planes.main([src, out, "-d", "1", "-a", "120"], detect_planes=model_detect_planes) == 1
    assert "min_angle" in capsys.readouterr().err
