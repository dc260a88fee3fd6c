"""The numpy model of DESIGN §24 (tests/wireframe_model.py) on its own: the scalar and array forms of stage 1 agree, the
hand-built cases come out as the contract states them, and the reference's published model gives a wireframe within the
stated bounds; stage 2 of the library (l3d_wireframe.h), compiled into a stand-alone program, returns the model's bytes;
the library exports the new entries and checks their arguments without a device; the command line.  CPU only."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib, api, io, wireframe
from tests import wireframe_cases as Cs
from tests import wireframe_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_scalar_and_array_forms_of_stage_1_are_identical():
    accepted = 0
    for k, n in enumerate([90, 150, 0, 1, 64]):
        segs, line = Cs.model_case(21 + k, n, box=4.0)
        for par in Cs.PARAM_SETS:
            a = M.junctions_scalar(segs, line, **par)
            b = M.junctions(segs, line, chunk=32, **par)
            assert a.dtype == b.dtype == M.RECORD_DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes(), (k, par)
            if len(a):
                key = a["a"].astype(np.int64) << 32 | a["b"]
                assert (np.diff(key) > 0).all() and (a["a"] < a["b"]).all()     # ascending (a, b), no pair twice
                assert (line[a["a"]] != line[a["b"]]).all()
            if par is Cs.DEFAULTS:
                accepted += len(a)
    assert accepted >= 200                                  # the cases exercise the acceptance, not only the rejection


def test_hand_built_cases():
    for name, segs, line, par, expected in Cs.hand_cases():
        for form in (M.junctions_scalar, M.junctions):
            Cs.check_expected(f"{name} ({form.__name__})", M.wireframe(segs, line, form=form, **par), expected)


def test_the_graph_of_a_generated_model_is_consistent():
    segs, line = Cs.model_case(5, 400, box=5.0)
    w = M.wireframe(segs, line, **Cs.DEFAULTS)
    J, V, E, s = w["junctions"], w["vertices"], w["edges"], w["summary"]
    total = 0.0
    for v in segs:
        e = v[3:] - v[:3]
        total += float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))
    assert s["length_total"] == total and s["n_segments"] == 400 and s["n_point_segments"] >= 1
    assert s["n_L"] >= 50 and s["n_T"] >= 10 and s["n_X"] >= 5 and (V["n_junctions"] >= 3).sum() >= 5
    assert int(V["degree"].sum()) == 2 * len(E) and (E["v0"] != E["v1"]).all() and (np.diff(E["segment"].astype(np.int64)) >= 0).all()
    assert (line[E["segment"]] == E["line"]).all()
    # junction vertices come first, numbered by their smallest junction; the free ends follow
    nv = s["n_junction_vertices"]
    assert (V["n_junctions"][:nv] >= 1).all() and (V["n_junctions"][nv:] == 0).all() and V["n_junctions"].sum() == len(J)
    first = [int(np.flatnonzero(J["vertex"] == v)[0]) for v in range(nv)]
    assert first == sorted(first)
    assert s["max_spread"] == V["spread"].max() and s["max_gap"] == J["gap"].max() <= Cs.DEFAULTS["max_distance"]
    # a component is what the edges connect
    assert len(np.unique(V["component"])) == s["n_components"] and (V["component"][E["v0"]] == V["component"][E["v1"]]).all()
    assert np.bincount(V["component"][E["v0"]]).max() == s["largest_component"]
    # every live segment is covered from its first stop to its last: at least one edge unless both ends share a vertex
    live = ((segs[:, 3:] - segs[:, :3]) ** 2).sum(1) > 0
    assert set(np.unique(E["segment"])) <= set(np.flatnonzero(live)) and len(np.unique(E["segment"])) >= live.sum() - 2


# ---- the reference's published model of its testdata ------------------------------------------------------------------
def test_reference_model_is_a_wireframe():
    """the counts the contract-order model gives are recorded in DESIGN §24; the asserts are the issue's bounds"""
    d = np.load(os.path.join(GOLDEN, "ref_c0_models.npz"))
    segs, line = d["optimized_segs"], d["optimized_line"]
    md = 0.001 * M.extent(segs)
    w = M.wireframe(segs, line, md, md, M.min_sin2_of(10.0))
    s, J = w["summary"], w["junctions"]
    in_a_junction = len(np.unique(np.concatenate([J["a"], J["b"]])))
    print("summary:", s, "\nsegments in a junction:", in_a_junction, "\nvertices by degree:",
          dict(zip(*(x.tolist() for x in np.unique(w["vertices"]["degree"], return_counts=True)))))
    assert s["n_segments"] == 2503
    assert s["n_junctions"] >= 500 and in_a_junction >= 500
    assert s["n_L"] >= 3 * s["n_T"] and s["n_X"] <= 0.01 * s["n_junctions"]


# ---- stage 2 of the library against the model -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wf") / "wireframe_graph")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "cpp", "wireframe_graph.cpp"),
                           "-o", exe])
    return exe


def run_graph_program(exe, tmp_path, segs, line, rec, max_distance, max_extension):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "graph.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<2I2d", len(segs), len(rec), max_distance, max_extension))
        f.write(np.ascontiguousarray(segs, np.float64).tobytes()); f.write(np.ascontiguousarray(line, np.uint32).tobytes())
        f.write(np.ascontiguousarray(rec, M.RECORD_DTYPE).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(dst, "rb").read()
    nj, nv, ne = struct.unpack_from("<3Q", raw, 0)
    pos = 24
    got = {}
    for name, dtype, count in (("junctions", M.JUNCTION_DTYPE, nj), ("vertices", M.VERTEX_DTYPE, nv), ("edges", M.EDGE_DTYPE, ne)):
        got[name] = np.frombuffer(raw, dtype, count, pos); pos += dtype.itemsize * count
    got["summary"] = dict(zip(M.SUMMARY_KEYS, struct.unpack_from("<12Q3d", raw, pos)))
    assert pos + 120 == len(raw)
    return got


def test_stage_2_of_the_library_returns_the_models_bytes(graph_program, tmp_path):
    cases = [(name, segs, line, par) for name, segs, line, par, _ in Cs.hand_cases()]
    cases += [(f"generated {n}", *Cs.model_case(300 + n, n, box=5.0), par) for n, par in zip((400, 700, 120, 1), Cs.PARAM_SETS)]
    chained = 0
    for name, segs, line, par in cases:
        rec = M.junctions(segs, line, **par)
        want = M.graph(segs, line, rec, par["max_distance"], par["max_extension"])
        got = run_graph_program(graph_program, tmp_path, segs, line, rec, par["max_distance"], par["max_extension"])
        Cs.same_result(got, want, name)
        chained += int((want["vertices"]["n_junctions"] >= 3).sum())
    assert chained >= 20


# ---- the library's side, as far as it goes without a device -----------------------------------------------------------
ENTRIES = ("l3d_wireframe_segments", "l3d_wireframe_lines", "l3d_wireframe_counts", "l3d_wireframe_get", "l3d_wireframe_save_obj",
           "l3d_wireframe_close")
COUNTERS = ("wf_count_launches", "wf_write_launches", "wf_slices", "wf_junctions", "wf_skipped_blocks", "wf_kernel_ns")


def test_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    L = _lib.load()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    for name in ("l3d_wireframe_params", "l3d_wf_junction", "l3d_wf_vertex", "l3d_wf_edge", "l3d_wireframe_summary"):
        assert "typedef struct " + name in hdr
    for name in COUNTERS:
        assert L.l3d_debug_counter(name.encode()) != L.l3d_debug_counter(b"no such counter")
    facade = open(os.path.join(ROOT, "include", "line3dpp", "line3D.h")).read()
    assert re.search(r"\bwireframe\s*\(", facade)


def test_struct_layouts():
    assert C.sizeof(_lib.WireframeParams) == 32 and C.sizeof(_lib.WireframeSummary) == 120
    assert _lib.WF_JUNCTION_DTYPE == M.JUNCTION_DTYPE and _lib.WF_VERTEX_DTYPE == M.VERTEX_DTYPE and _lib.WF_EDGE_DTYPE == M.EDGE_DTYPE
    assert (M.JUNCTION_DTYPE.itemsize, M.VERTEX_DTYPE.itemsize, M.EDGE_DTYPE.itemsize, M.RECORD_DTYPE.itemsize) == (72, 48, 16, 32)
    assert tuple(f for f, _ in _lib.WireframeSummary._fields_) == M.SUMMARY_KEYS
    assert [f for f, _ in _lib.WireframeParams._fields_] == ["max_distance", "max_extension", "min_sin2", "slice_chunks", "reserved"]
    assert (_lib.WF_L, _lib.WF_T, _lib.WF_X) == (M.KIND_L, M.KIND_T, M.KIND_X) and (_lib.WF_AT_P1, _lib.WF_AT_P2, _lib.WF_INTERIOR) == (0, 1, 2)


def test_wireframe_params_follow_compare_params():
    p = api.wireframe_params(0.25, 0.5, 10.0, 3)
    assert (p.max_distance, p.max_extension, p.min_sin2, p.slice_chunks, p.reserved) == (0.25, 0.5, M.min_sin2_of(10.0), 3, 0)
    p = api.wireframe_params(0.25)
    assert p.max_extension == 0.25 and p.min_sin2 == M.min_sin2_of(10.0) and p.slice_chunks == 0
    assert api.wireframe_params(1.0, 0.0).max_extension == 0.0          # (0 is a value, not "none")
    assert api.wireframe_params(1.0, min_angle=0.0).min_sin2 == 0.0 and api.wireframe_params(1.0, min_angle=90.0).min_sin2 == 1.0
    for bad in (-1.0, 90.5, float("nan")):
        with pytest.raises(ValueError, match="min_angle"):
            api.wireframe_params(1.0, None, bad)


FILL = 0x5A5A5A5A5A5A5A5A


def call(par, segs=None, line=None, n=None, null=()):
    """l3d_wireframe_segments with a handle slot filled with a pattern, which every refused call must leave as it was"""
    L = _lib.load()
    base_segs, base_line = Cs.model_case(1, 4)
    segs = base_segs if segs is None else segs; line = base_line if line is None else line
    slot = C.c_void_p(FILL)
    rc = L.l3d_wireframe_segments(0, len(line) if n is None else n, None if "segs" in null else _lib.ptr(segs),
                                  None if "line" in null else _lib.ptr(line), C.byref(par) if par is not None else None,
                                  None if "out" in null else C.byref(slot))
    assert rc != 0 and slot.value == FILL
    return rc, _lib.last_error()


def test_argument_checks_need_no_device():
    """the checks come before any device work: they answer on a machine without a GPU as well"""
    ok = (0.5, 0.5, 0.03, 0, 0)
    for k, name, bad in ((0, "max_distance", (-1.0, float("inf"), float("nan"))), (1, "max_extension", (-1.0, float("inf"), float("nan"))),
                         (2, "min_sin2", (-0.1, 1.1, float("nan"))), (4, "reserved", (1, 0xFFFFFFFF))):
        for v in bad:
            vals = list(ok); vals[k] = v
            rc, msg = call(_lib.WireframeParams(*vals))
            assert rc == -1 and name in msg, (name, v, rc, msg)
    rc, msg = call(None)
    assert rc == -1 and "null" in msg
    good = _lib.WireframeParams(*ok)
    base = Cs.model_case(1, 4)[0]
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
    assert L.l3d_wireframe_lines(None, C.byref(good), C.byref(slot)) == -1 and "null" in _lib.last_error() and slot.value == FILL
    assert L.l3d_wireframe_counts(None, None, None, None) == -1 and L.l3d_wireframe_get(None, None, None, None, None) == -1
    assert L.l3d_wireframe_save_obj(None, b"x.obj") == -1
    L.l3d_wireframe_close(None)                              # (as free(NULL))


def test_empty_model_needs_no_device(tmp_path):
    L = _lib.load()
    good = _lib.WireframeParams(0.5, 0.5, 0.03, 0, 0)
    h = C.c_void_p()
    assert L.l3d_wireframe_segments(0, 0, None, None, C.byref(good), C.byref(h)) == 0 and h.value
    nj = C.c_uint64(7); nv = C.c_uint64(7); ne = C.c_uint64(7)
    s = _lib.WireframeSummary(n_segments=7, length_total=1.0, max_spread=2.0)
    assert L.l3d_wireframe_counts(h, C.byref(nj), C.byref(nv), C.byref(ne)) == 0 and (nj.value, nv.value, ne.value) == (0, 0, 0)
    assert L.l3d_wireframe_get(h, None, None, None, C.byref(s)) == 0 and all(getattr(s, f) == 0 for f in M.SUMMARY_KEYS)
    path = str(tmp_path / "empty.obj")
    assert L.l3d_wireframe_save_obj(h, path.encode()) == 0 and open(path).read() == ""
    assert L.l3d_wireframe_save_obj(h, str(tmp_path / "no" / "such" / "dir.obj").encode()) == -11 and "cannot write" in _lib.last_error()
    L.l3d_wireframe_close(h)
    w = api.build_wireframe(np.zeros((0, 6)), np.zeros(0, np.uint32), 0.5)
    Cs.same_result(w, M.wireframe(np.zeros((0, 6)), np.zeros(0, np.uint32), 0.5, 0.5, 0.03), "the empty model")
    with pytest.raises(ValueError, match="one line index"):
        api.build_wireframe(np.zeros((2, 6)), np.zeros(1, np.uint32), 0.5)


# ---- the command line, with the model in the library's place ----------------------------------------------------------
def model_build_wireframe(segs, line, max_distance, max_extension=None, min_angle=10.0, slice_chunks=0, device=0, obj_path=None):
    p = api.wireframe_params(max_distance, max_extension, min_angle, slice_chunks)
    return M.wireframe(segs, line, p.max_distance, p.max_extension, p.min_sin2)


def test_command_line(tmp_path, capsys):
    """the excerpt's lines and three more that meet its first segment: at an end, on its interior, across it"""
    lines = io.read_3d_lines_txt(os.path.join(GOLDEN, "ref_lines3d_excerpt.txt"))
    s0 = np.asarray(lines[0]["segments"], np.float64).reshape(-1)[:6]
    p1, p2 = s0[:3], s0[3:6]
    d = p2 - p1
    side = np.cross(d, [0.3, 0.5, 0.8]); side *= np.linalg.norm(d) / np.linalg.norm(side)
    mid = p1 + 0.5 * d

    def one(a, b):
        return dict(segments=np.concatenate([a, b]).reshape(1, 6), residuals=np.zeros((0, 2), np.uint32), coords2D=np.zeros((0, 4), np.float32))
    more = [one(p1, p1 + side), one(mid, mid + side), one(p1 + 0.25 * d - side, p1 + 0.25 * d + side)]
    src = str(tmp_path / "model.txt")
    with open(src, "w") as f:
        f.write(io.format_3d_lines_txt(lines + more))
    seen = {}

    def spy(*args, **kw):
        seen.update(kw)
        return model_build_wireframe(*args, **kw)
    out = str(tmp_path / "wire.obj")
    md = 1e-3 * float(np.linalg.norm(d))                  # (the text file keeps six digits of every coordinate)
    assert wireframe.main([src, out, "-d", repr(md), "-x", repr(2 * md), "-a", "20"], build_wireframe=spy) == 0
    res = json.loads(capsys.readouterr().out)
    assert seen["max_distance"] == md and seen["max_extension"] == 2 * md and seen["min_angle"] == 20.0
    segs, line = api.flatten_lines(io.read_3d_lines_txt(src))
    want = M.wireframe(segs, line, md, 2 * md, M.min_sin2_of(20.0))
    for k in M.SUMMARY_KEYS:
        assert res[k] == want["summary"][k], k
    assert res["n_L"] >= 1 and res["n_T"] >= 1 and res["n_X"] >= 1 and res["n_junction_vertices"] >= 3
    J = want["junctions"]
    n0 = len(line) - 3                                      # the three added segments, each with the excerpt's first one
    assert {(int(j["a"]), int(j["b"]), int(j["kind"])) for j in J} >= {(0, n0, M.KIND_L), (0, n0 + 1, M.KIND_T), (0, n0 + 2, M.KIND_X)}
    assert res["max_distance"] == md and res["max_extension"] == 2 * md and res["input"] == src and res["output"] == out
    assert open(out).read() == M.obj_text(want)
    v = [ln.split() for ln in open(out) if ln.startswith("v ")]
    e = [ln.split() for ln in open(out) if ln.startswith("l ")]
    assert len(v) == res["n_vertices"] and len(e) == res["n_edges"] and len(v) + len(e) == len(open(out).readlines())
    assert np.array_equal(np.array([[float(x) for x in r[1:]] for r in v]), want["vertices"]["P"])          # %.17g reads back exactly
    assert np.array_equal(np.array([[int(x) - 1 for x in r[1:]] for r in e]), np.stack([want["edges"]["v0"], want["edges"]["v1"]], 1))
    # -x defaults to -d; a .bin input
    assert wireframe.main([os.path.join(GOLDEN, "ref_lines3d_excerpt.bin"), out, "-d", "0.5"], build_wireframe=spy) == 0
    res = json.loads(capsys.readouterr().out)
    assert seen["max_extension"] is None and res["max_extension"] == 0.5 and res["min_angle"] == 10.0 and res["n_segments"] > 3
    # -d is required; both files; the extensions; a missing file; an angle outside [0, 90]
    for argv in ([src, out], [src, "-d", "1"]):
        with pytest.raises(SystemExit):
            wireframe.main(argv, build_wireframe=model_build_wireframe)
        assert "usage" in capsys.readouterr().err
    assert wireframe.main([str(tmp_path / "model.obj"), out, "-d", "1"], build_wireframe=model_build_wireframe) == 1
    assert ".txt or .bin" in capsys.readouterr().err
    assert wireframe.main([src, str(tmp_path / "wire.txt"), "-d", "1"], build_wireframe=model_build_wireframe) == 1
    assert "written as .obj" in capsys.readouterr().err
    assert wireframe.main([str(tmp_path / "none.txt"), out, "-d", "1"], build_wireframe=model_build_wireframe) == 1
    assert "no such file" in capsys.readouterr().err
    assert wireframe.main([src, out, "-d", "1", "-a", "120"], build_wireframe=model_build_wireframe) == 1
    assert "min_angle" in capsys.readouterr().err
