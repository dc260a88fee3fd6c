"""The numpy model of DESIGN §26 (tests/directions_model.py) on its own: the scalar and array forms of stages 1 and 2 agree,
the inlier relation is symmetric and every live hypothesis is its own inlier, the generated cases meet the admission rule
and the hand-built cases come out as the contract states them; stage 3 of the library (l3d_directions.h), compiled into a
stand-alone program, returns the model's bytes, the largest-eigenvector Jacobi included; the library exports the new
entries and checks their arguments without a device; the command line.  CPU only."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib, api, directions, io
from tests import directions_cases as Cs
from tests import directions_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_scalar_and_array_forms_are_identical():
    members = 0
    for n in (63, 256, 0, 1):
        segs, _, _ = Cs.sized_case(n)
        w = M.weights(segs)
        a, b = M.units_scalar(segs), M.units(segs)
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape == (n, 3) and a.tobytes() == b.tobytes(), n
        assert not np.isnan(a).any() and (~a.any(1)).sum() == w["n_points"]
        for max_sin2 in (Cs.PAR["max_sin2"], 0.0, 0.3):
            for chunk in (256, 7):
                sa, sb = M.scores_scalar(a, w, max_sin2), M.scores(a, w, max_sin2, chunk=chunk)
                assert sa.dtype == sb.dtype == M.SCORE_DTYPE and sa.tobytes() == sb.tobytes(), (n, max_sin2, chunk)
        members += int((M.scores(a, w, Cs.PAR["max_sin2"])["count"] >= 8).sum())
    assert members >= 150                                       # the cases exercise the inliers, not only their absence


def test_the_relation_is_symmetric_and_a_live_hypothesis_is_its_own_inlier():
    """D_s x D_h is the exact negation of D_h x D_s, so x2 is the same number either way round; D_h x D_h is 0"""
    segs, _, _ = Cs.sized_case(513)
    w = M.weights(segs)
    D = M.units(segs)
    live = np.asarray(w["live"], bool)
    assert 0 < (~live).sum() < 30
    for max_sin2 in (0.0, Cs.PAR["max_sin2"], 0.25, 1.0):
        ok = M.relation(D, w, max_sin2)
        assert np.array_equal(ok, ok.T) and np.array_equal(np.diag(ok), live), max_sin2
        assert not ok[~live].any() and not ok[:, ~live].any()
    rows = [[float(x) for x in d] for d in D]
    for h, s in ((0, 1), (5, 77), (100, 512), (3, 3)):
        assert M.sin2(rows[h], rows[s]) == M.sin2(rows[s], rows[h]) and [-x for x in M.cross(rows[h], rows[s])] == M.cross(rows[s], rows[h])
    assert all(M.sin2(d, d) == 0.0 for d in rows)
    assert M.relation(D, w, 1.0)[live][:, live].all()           # |X|^2 of two unit vectors stays within [0, 1] here


@pytest.mark.parametrize("n", Cs.EDGE_N + (Cs.SLICING_N,))
def test_generated_cases_are_admitted(n):
    segs, line, planted = Cs.sized_case(n)
    assert len(segs) == n and len(planted) == (4 if n >= 63 else 0)
    got = M.detect(segs, line, Cs.PAR)
    assert Cs.admitted(got, planted) is None
    if planted:
        R = got["R"]
        assert np.allclose(R @ R.T, np.eye(3), rtol=0, atol=1e-14) and abs(np.linalg.det(R) - 1.0) < 1e-14
        # the frame stands the orthogonal families on the axes: under R each of them runs along one coordinate axis
        for k, axis in enumerate(got["summary"]["frame"]):
            d = R @ got["directions"]["D_fit"][axis]
            assert abs(abs(d[k]) - 1.0) < 1e-3, (k, d)


def test_the_large_case_is_admitted():
    segs, line, planted = Cs.large_case()
    got = M.detect(segs, line, Cs.PAR)
    assert len(segs) == 5000 and Cs.admitted(got, planted) is None and got["summary"]["n_directions"] == 4


def test_hand_built_cases():
    for name, segs, line, par, expected in Cs.hand_cases():
        for form in ("scalar", "array"):
            Cs.check_expected(f"{name} ({form})", M.detect(segs, line, par, form), expected)


def test_the_cube_frame_is_a_signed_permutation():
    """whichever way the cube is turned by quarter turns and however its edges are reversed"""
    base = Cs.segs(Cs.cube())
    turn = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
    for g in (base, np.concatenate([base[:, 3:], base[:, :3]], 1), np.concatenate([base[:, :3] @ turn.T, base[:, 3:] @ turn.T], 1)):
        got = M.detect(g, np.arange(12), M.params(M.sin2_of(1.0)))
        R = got["R"]
        assert got["summary"]["frame_axes"] == 3 and got["summary"]["n_dropped"] == 9 and got["directions"]["n_segments"].tolist() == [4] * 3
        assert np.array_equal(np.abs(R).sum(0), np.ones(3)) and np.array_equal(np.abs(R).sum(1), np.ones(3)) and set(np.abs(R).ravel()) == {0.0, 1.0}
        assert np.linalg.det(R) == 1.0


def test_the_refit_is_a_fit():
    segs, line, _ = Cs.sized_case(513)
    P = M.detect(segs, line, Cs.PAR)["directions"]
    assert len(P) == 4 and (P["rms_sin_fit"] <= P["rms_sin"] * (1 + 1e-9)).all() and (P["rms_sin_fit"] > 0).all()
    assert np.allclose((P["D_fit"] ** 2).sum(1), 1.0, rtol=0, atol=1e-15) and ((P["D_fit"] * P["D"]).sum(1) > 0.9999).all()
    assert (P["t_min"] < 0).all() and (P["t_max"] > 0).all()


# ---- stage 3 of the library against the model -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def select_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dir") / "directions_select")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cpp", "directions_select.cpp"),
                           "-o", exe])
    return exe


def c_params(par, slice_chunks=0):
    return _lib.DirectionsParams(par["max_sin2"], par["min_length"], par["max_frame_cos2"], par["min_segments"], par["max_directions"],
                                 par["max_tests"], slice_chunks, par["frame_search"], (0,) * 5)


def run_select_program(exe, tmp_path, segs, line, par, score, expect=0):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "directions.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<2I", len(segs), 0)); f.write(bytes(c_params(par)))
        f.write(np.ascontiguousarray(segs, np.float64).tobytes()); f.write(np.ascontiguousarray(line, np.uint32).tobytes())
        f.write(np.ascontiguousarray(score, M.SCORE_DTYPE).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == expect, out.stdout + out.stderr
    if expect:
        return out.stdout
    raw = open(dst, "rb").read()
    n_d, n_m, n_s = struct.unpack_from("<3Q", raw, 0)
    pos = 24
    got = {}
    for name, dtype, count in (("directions", M.DIRECTION_DTYPE, n_d), ("members", M.MEMBER_DTYPE, n_m), ("seg_directions", np.dtype("<u4"), n_s)):
        got[name] = np.frombuffer(raw, dtype, count, pos); pos += dtype.itemsize * count
    got["summary_bytes"] = raw[pos:pos + 200]
    v = struct.unpack_from(M.SUMMARY_FORMAT, raw, pos); pos += 200
    got["summary"] = dict(zip(M.SUMMARY_KEYS[:15], v[:15]), frame=list(v[15:18]), R=list(v[18:27]))
    got["R"] = np.array(got["summary"]["R"]).reshape(3, 3)
    got["weights"] = np.frombuffer(raw, "<u8", len(segs), pos)
    assert pos + 8 * len(segs) == len(raw)
    got["scores"] = np.ascontiguousarray(score, M.SCORE_DTYPE)
    return got


def test_stage_3_of_the_library_returns_the_models_bytes(select_program, tmp_path):
    cases = [(name, segs, line, par) for name, segs, line, par, _ in Cs.hand_cases()]
    cases += [(f"generated {n}", *Cs.sized_case(n)[:2], par) for n, par in
              ((513, Cs.PAR), (768, dict(Cs.PAR, min_length=60.0)), (257, dict(Cs.PAR, max_tests=3)), (256, dict(Cs.PAR, frame_search=2)),
               (63, M.params(M.sin2_of(20.0), min_segments=3, max_frame_cos2=M.sin2_of(30.0))))]
    found = 0
    for name, segs, line, par in cases:
        w = M.weights(segs)
        score = M.scores(M.units(segs), w, par["max_sin2"])
        want = M.select(segs, line, w, score, par)
        got = run_select_program(select_program, tmp_path, segs, line, par, score)
        assert got["weights"].tolist() == w["q"], name
        Cs.same_result(got, want, name)
        assert got["summary_bytes"] == M.pack_summary(want["summary"]), name
        found += len(want["directions"])
    assert found >= 30


def test_the_jacobi_finds_the_largest_eigenvector(select_program, tmp_path):
    rng = np.random.default_rng(11)
    rows, vectors = [], []
    for _ in range(50):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        lam = np.sort(rng.uniform(0.1, 10.0, 3)) * [1e-6, 1e-6, 1.0]       # a scatter of nearly parallel directions
        S = (q * lam) @ q.T
        rows.append([float(S[i, j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]); vectors.append(q[:, 2])
    rows += [[1.0, 0.0, 0.0, 2.0, 0.0, 3.0], [1.0, 0.0, 0.0, 1.0, 0.0, 1.0], [2.0, 0.0, 0.0, 5.0, 0.0, 5.0]]
    model = np.array([M.largest_eigenvector(r) for r in rows])
    for v, q in zip(model, vectors):
        # the error of a Jacobi eigenvector is of the order of eps * |S| / the gap to the next eigenvalue: 1e-16 * 10 / 0.1
        assert abs(abs(v @ q) - 1.0) < 1e-12 and abs(v @ v - 1.0) < 1e-15
    assert model[50].tolist() == [0.0, 0.0, 1.0]                # a diagonal matrix: no rotation
    assert model[51].tolist() == [1.0, 0.0, 0.0]                # the first of equals
    assert model[52].tolist() == [0.0, 1.0, 0.0]                # ... of the two largest
    src, dst = str(tmp_path / "s.bin"), str(tmp_path / "v.bin")
    np.array(rows, np.float64).tofile(src)
    subprocess.check_call([select_program, "eigen", src, dst])
    assert open(dst, "rb").read() == model.tobytes()


def test_a_score_that_differs_from_the_members_is_named(select_program, tmp_path):
    name, segs, line, par, _ = Cs.hand_cases()[0]
    w = M.weights(segs)
    score = M.scores(M.units(segs), w, par["max_sin2"])
    for field in ("weight", "count"):
        bad = score.copy(); bad[field][4] += 1
        assert "hypothesis 4" in run_select_program(select_program, tmp_path, segs, line, par, bad, expect=9)


# ---- the library's side, as far as it goes without a device -----------------------------------------------------------
ENTRIES = ("l3d_direction_segments", "l3d_direction_lines", "l3d_directions_counts", "l3d_directions_get", "l3d_directions_save_obj",
           "l3d_directions_close")
COUNTERS = ("dir_score_launches", "dir_slices", "dir_hypotheses", "dir_kernel_ns")


def test_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    L = _lib.load()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    for name in ("l3d_directions_params", "l3d_dir_direction", "l3d_dir_member", "l3d_dir_score", "l3d_directions_summary"):
        assert "typedef struct " + name in hdr
    for name in COUNTERS:
        assert L.l3d_debug_counter(name.encode()) != L.l3d_debug_counter(b"no such counter")
    facade = open(os.path.join(ROOT, "include", "line3dpp", "line3D.h")).read()
    assert re.search(r"\bdetectDirections\s*\(", facade)


def test_struct_layouts():
    assert C.sizeof(_lib.DirectionsParams) == 64 and C.sizeof(_lib.DirectionsSummary) == 200
    assert _lib.DIR_DIRECTION_DTYPE == M.DIRECTION_DTYPE and _lib.DIR_MEMBER_DTYPE == M.MEMBER_DTYPE and _lib.DIR_SCORE_DTYPE == M.SCORE_DTYPE
    assert (M.DIRECTION_DTYPE.itemsize, M.MEMBER_DTYPE.itemsize, M.SCORE_DTYPE.itemsize) == (136, 8, 16)
    assert tuple(f for f, _ in _lib.DirectionsSummary._fields_) == M.SUMMARY_KEYS and struct.calcsize(M.SUMMARY_FORMAT) == 200
    assert [f for f, _ in _lib.DirectionsParams._fields_] == ["max_sin2", "min_length", "max_frame_cos2", "min_segments", "max_directions",
                                                               "max_tests", "slice_chunks", "frame_search", "reserved"]
    s = _lib.DirectionsSummary(n_segments=3, truncated=1, scale_exponent=-2, length_in_directions=0.5, frame_axes=2, frame=(4, 5, M.NONE),
                               R=tuple(float(k) for k in range(9)))
    assert bytes(s) == M.pack_summary(api.directions_summary_dict(s))


def test_directions_params_follow_the_degree_rule():
    p = api.directions_params(2.0, 3.0, 5, 6, 7, 8.0, 9, 2)
    assert (p.max_sin2, p.min_length, p.max_frame_cos2, p.min_segments, p.max_directions, p.max_tests, p.slice_chunks, p.frame_search,
            tuple(p.reserved)) == (M.sin2_of(2.0), 3.0, M.sin2_of(8.0), 5, 6, 7, 2, 9, (0,) * 5)
    p = api.directions_params(1.0)
    assert (p.min_length, p.max_frame_cos2, p.min_segments, p.max_directions, p.max_tests, p.slice_chunks, p.frame_search) == \
        (0.0, M.sin2_of(5.0), 4, 16, 4096, 0, 16)
    assert api.directions_params(0.0).max_sin2 == 0.0 and api.directions_params(90.0).max_sin2 == 1.0
    for bad in (-1.0, 90.5, float("nan")):
        with pytest.raises(ValueError, match="max_angle"):
            api.directions_params(bad)
        with pytest.raises(ValueError, match="frame_angle"):
            api.directions_params(1.0, frame_angle=bad)


FILL = 0x5A5A5A5A5A5A5A5A
OK = (0.01, 0.0, 0.01, 4, 16, 4096, 0, 16, (0,) * 5)


def call(par, segs=None, line=None, n=None, null=()):
    """l3d_direction_segments with a handle slot filled with a pattern, which every refused call must leave as it was"""
    L = _lib.load()
    base_segs, base_line, _ = Cs.sized_case(8)
    segs = base_segs if segs is None else segs; line = base_line if line is None else line
    slot = C.c_void_p(FILL)
    rc = L.l3d_direction_segments(0, len(line) if n is None else n, None if "segs" in null else _lib.ptr(segs),
                                  None if "line" in null else _lib.ptr(line), C.byref(par) if par is not None else None,
                                  None if "out" in null else C.byref(slot))
    assert rc != 0 and slot.value == FILL
    return rc, _lib.last_error()


def test_argument_checks_need_no_device():
    """the checks come before any device work: they answer on a machine without a GPU as well"""
    outside = (-0.1, 1.1, float("nan"), float("inf"))
    reserved = [tuple(1 if k == j else 0 for k in range(5)) for j in range(5)] + [(0xFFFFFFFF, 0, 0, 0, 0)]
    for k, name, bad in ((0, "max_sin2", outside), (1, "min_length", (-1.0, float("inf"), float("nan"))), (2, "max_frame_cos2", outside),
                         (3, "min_segments", (0,)), (4, "max_directions", (0,)), (5, "max_tests", (0,)), (7, "frame_search", (0, 65, 0xFFFFFFFF)),
                         (8, "reserved", reserved)):
        for v in bad:
            vals = list(OK); vals[k] = v
            rc, msg = call(_lib.DirectionsParams(*vals))
            assert rc == -1 and name in msg, (name, v, rc, msg)
    rc, msg = call(None)
    assert rc == -1 and "null" in msg
    good = _lib.DirectionsParams(*OK)
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
    # the bounds themselves are allowed: they fail on the model's coordinate instead, after the parameters
    for k, v in ((0, 0.0), (0, 1.0), (2, 0.0), (2, 1.0), (7, 1), (7, 64)):
        vals = list(OK); vals[k] = v
        bad = base.copy(); bad[0, 0] = np.nan
        rc, msg = call(_lib.DirectionsParams(*vals), segs=bad)
        assert rc == -1 and "segment 0" in msg, (k, v, msg)
    # the context form and the handle's entries check their arguments first as well
    L = _lib.load()
    slot = C.c_void_p(FILL)
    assert L.l3d_direction_lines(None, C.byref(good), C.byref(slot)) == -1 and "null" in _lib.last_error() and slot.value == FILL
    assert L.l3d_directions_counts(None, None, None, None) == -1 and L.l3d_directions_get(None, None, None, None, None, None) == -1
    assert L.l3d_directions_save_obj(None, b"x.obj") == -1
    L.l3d_directions_close(None)                             # (as free(NULL))


def test_empty_model_needs_no_device(tmp_path):
    L = _lib.load()
    good = _lib.DirectionsParams(*OK)
    h = C.c_void_p()
    assert L.l3d_direction_segments(0, 0, None, None, C.byref(good), C.byref(h)) == 0 and h.value
    n_d = C.c_uint64(7); n_m = C.c_uint64(7); n_h = C.c_uint64(7)
    s = _lib.DirectionsSummary(n_segments=7, scale_exponent=-3, length_total=1.0, frame_axes=2, frame=(1, 2, 3), R=(2.0,) * 9)
    assert L.l3d_directions_counts(h, C.byref(n_d), C.byref(n_m), C.byref(n_h)) == 0 and (n_d.value, n_m.value, n_h.value) == (0, 0, 0)
    assert L.l3d_directions_get(h, None, None, None, None, C.byref(s)) == 0
    assert bytes(s) == M.pack_summary(M.empty_summary()) and list(s.R) == M.IDENTITY and list(s.frame) == [M.NONE] * 3 and s.frame_axes == 0
    assert all(getattr(s, f) == 0 for f in M.SUMMARY_KEYS[:14])
    path = str(tmp_path / "empty.obj")
    assert L.l3d_directions_save_obj(h, path.encode()) == 0 and open(path).read() == ""
    assert L.l3d_directions_save_obj(h, str(tmp_path / "no" / "such" / "dir.obj").encode()) == -11 and "cannot write" in _lib.last_error()
    L.l3d_directions_close(h)
    got = api.detect_directions(np.zeros((0, 6)), np.zeros(0, np.uint32), 1.0)
    Cs.same_result(got, M.detect(np.zeros((0, 6)), np.zeros(0, np.uint32), M.params(M.sin2_of(1.0))), "the empty model")
    assert np.array_equal(got["R"], np.eye(3))
    with pytest.raises(ValueError, match="one line index"):
        api.detect_directions(np.zeros((2, 6)), np.zeros(1, np.uint32), 1.0)


def test_the_python_writer_gives_the_models_text(tmp_path):
    segs, line, _ = Cs.sized_case(256)
    want = M.detect(segs, line, Cs.PAR)
    path = str(tmp_path / "py.obj")
    api.write_directions_obj(want, path)
    text = open(path).read()
    assert text == M.obj_text(want) and text.count("\nl ") + text.startswith("l ") == 4 and text.count("v ") == 8
    rows = [ln.split() for ln in text.splitlines()]
    ends = np.array([[float(x) for x in r[1:]] for r in rows if r[0] == "v"]).reshape(-1, 2, 3)
    P = want["directions"]
    assert np.array_equal(ends[:, 0], P["centroid"] + P["t_min"][:, None] * P["D_fit"])   # %.17g reads back exactly
    assert np.array_equal(ends[:, 1], P["centroid"] + P["t_max"][:, None] * P["D_fit"])
    assert [[int(x) for x in r[1:]] for r in rows if r[0] == "l"] == [[2 * k + 1, 2 * k + 2] for k in range(4)]


# ---- the command line, with the model in the library's place ----------------------------------------------------------
def model_detect_directions(segs, line, max_angle, min_length=0.0, min_segments=4, max_directions=16, max_tests=4096, frame_angle=5.0,
                            frame_search=16, slice_chunks=0, device=0, obj_path=None):
    p = api.directions_params(max_angle, min_length, min_segments, max_directions, max_tests, frame_angle, frame_search)
    return M.detect(segs, line, M.params(p.max_sin2, p.min_length, p.max_frame_cos2, p.min_segments, p.max_directions, p.max_tests,
                                         p.frame_search))


def test_command_line(tmp_path, capsys):
    """the excerpt's lines and two families of five parallel lines beside them, at right angles and askew to the axes"""
    lines = io.read_3d_lines_txt(os.path.join(GOLDEN, "ref_lines3d_excerpt.txt"))
    ex_segs, _ = api.flatten_lines(lines)
    size = M.extent(ex_segs)
    o = ex_segs.reshape(-1, 3).max(0) + size
    u, v = np.array([2.0, 1.0, 2.0]) / 3 * size, np.array([2.0, -2.0, -1.0]) / 3 * size * 0.5

    def one(a, b):
        return dict(segments=np.concatenate([a, b]).reshape(1, 6), residuals=np.zeros((0, 2), np.uint32), coords2D=np.zeros((0, 4), np.float32))
    more = [one(o + k * v, o + k * v + u) for k in range(5)] + [one(o + k * u, o + k * u + v) for k in range(5)]
    src = str(tmp_path / "model.txt")
    with open(src, "w") as f:
        f.write(io.format_3d_lines_txt(lines + more))
    seen = {}

    def spy(*args, **kw):
        seen.update(kw)
        return model_detect_directions(*args, **kw)
    out, upright = str(tmp_path / "directions.obj"), str(tmp_path / "upright.txt")
    argv = [src, out, "-a", "0.5", "-l", repr(size), "-s", "5", "-p", "9", "-f", "2", "--out", upright]
    assert directions.main(argv, detect_directions=spy) == 0
    res = json.loads(capsys.readouterr().out)
    assert (seen["max_angle"], seen["min_length"], seen["min_segments"], seen["max_directions"], seen["frame_angle"]) == (0.5, size, 5, 9, 2.0)
    segs, line = api.flatten_lines(io.read_3d_lines_txt(src))
    want = M.detect(segs, line, M.params(M.sin2_of(0.5), size, M.sin2_of(2.0), 5, 9))
    for k in M.SUMMARY_KEYS:
        assert res[k] == want["summary"][k], k
    n0 = len(line) - 10
    members = want["members"]
    assert res["n_directions"] >= 2 and res["frame_axes"] >= 2 and res["frame"][:2] == [0, 1]
    assert members["segment"][members["direction"] == 0].tolist() == list(range(n0, n0 + 5))
    assert members["segment"][members["direction"] == 1].tolist() == list(range(n0 + 5, n0 + 10))
    assert res["max_angle"] == 0.5 and res["frame_angle"] == 2.0 and res["input"] == src and res["output"] == out and res["out"] == upright
    text = open(out).read()
    assert text == M.obj_text(want)
    rows = [ln.split() for ln in text.splitlines()]
    assert len([r for r in rows if r[0] == "v"]) == 2 * res["n_directions"] and len([r for r in rows if r[0] == "l"]) == res["n_directions"]
    # the upright model: the input under R, in the text form; its first family runs along x, its second along y
    moved, _ = api.flatten_lines(io.read_3d_lines_txt(upright))
    R = want["R"]
    sim = api.similarity_from_matrix(np.concatenate([R, np.zeros((3, 1))], 1))
    wanted = api.transform_segments(segs, sim)
    assert moved.shape == segs.shape and np.allclose(moved, wanted, rtol=0, atol=1e-5 * size)   # (six digits in the text file)
    e = wanted[n0:, 3:] - wanted[n0:, :3]
    assert (np.abs(e[:5, 1:]).max() < 1e-4 * size) and (np.abs(e[5:, [0, 2]]).max() < 1e-4 * size)
    # a .bin input, the defaults
    assert directions.main([os.path.join(GOLDEN, "ref_lines3d_excerpt.bin"), out, "-a", "3"], detect_directions=spy) == 0
    res = json.loads(capsys.readouterr().out)
    assert seen["min_length"] == 0.0 and seen["min_segments"] == 4 and seen["max_directions"] == 16 and seen["frame_angle"] == 5.0
    assert res["out"] is None and res["n_segments"] > 3 and len(res["R"]) == 9 and len(res["frame"]) == 3
    # -a is required; both files; the extensions; a missing file; an angle outside [0, 90]
    for argv in ([src, out], [src, "-a", "1"]):
        with pytest.raises(SystemExit):
            directions.main(argv, detect_directions=model_detect_directions)
        assert "usage" in capsys.readouterr().err
    assert directions.main([str(tmp_path / "model.obj"), out, "-a", "1"], detect_directions=model_detect_directions) == 1
    assert ".txt or .bin" in capsys.readouterr().err
    assert directions.main([src, str(tmp_path / "directions.txt"), "-a", "1"], detect_directions=model_detect_directions) == 1
    assert "written as .obj" in capsys.readouterr().err
    assert directions.main([src, out, "-a", "1", "--out", str(tmp_path / "upright.bin")], detect_directions=model_detect_directions) == 1
    assert "written as .txt" in capsys.readouterr().err
    assert directions.main([str(tmp_path / "none.txt"), out, "-a", "1"], detect_directions=model_detect_directions) == 1
    assert "no such file" in capsys.readouterr().err
    assert directions.main([src, out, "-a", "120"], detect_directions=model_detect_directions) == 1
    assert "max_angle" in capsys.readouterr().err
