"""The junctions of a 3D line model and its wireframe graph on the MI355X (k_wireframe.hip, l3d_wireframe.hip)
against the numpy model of tests/wireframe_model.py with tolerance 0 on every output byte -- every operation of the
contract is an exactly rounded fp64 one, as in §18 and §19: tile, chunk and slice edges with the launches they take and
the workgroups the triangular walk skips, every slicing of one case, a model without a junction, a quiet tile next to a
busy one, the diagonal of the triangular walk, the hand-built cases, a case at size, the reference's published model, a
list whose 32-bit total wraps, the context form on the golden scene, the C++ facade and the OBJ file."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from line3dpp_amd.api import Line3D
from tests import wireframe_cases as Cs
from tests import wireframe_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PAR = Cs.DEFAULTS
FILL = 0x5A5A5A5A5A5A5A5A
COUNTERS = ("wf_count_launches", "wf_write_launches", "wf_slices", "wf_junctions", "wf_skipped_blocks")


def counters():
    L = _lib.load()
    return {k: L.l3d_debug_counter(k.encode()) for k in COUNTERS}


def run(segs, line, par=PAR, slice_chunks=0, expect=0, obj_path=None):
    """the stateless entry with the squared sine itself, as the model takes it -> the dict of a wireframe; a refused call
    must leave the handle's slot as it was"""
    L = _lib.load()
    segs = np.ascontiguousarray(segs, np.float64).reshape(-1, 6); line = np.ascontiguousarray(line, np.uint32)
    n = len(segs)
    p = _lib.WireframeParams(par["max_distance"], par["max_extension"], par["min_sin2"], slice_chunks, 0)
    slot = C.c_void_p(FILL)
    rc = L.l3d_wireframe_segments(0, n, _lib.ptr(segs) if n else None, _lib.ptr(line) if n else None, C.byref(p), C.byref(slot))
    assert rc == expect, _lib.last_error()
    if rc:
        assert slot.value == FILL
        return None
    return api.take_wireframe(slot, obj_path)


# ---- tile, chunk and slice edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,slice_chunks", Cs.EDGE_SHAPES)
def test_tile_chunk_and_slice_edges(n, slice_chunks):
    segs, line = Cs.model_case(1000 + n, n)
    want = M.wireframe(segs, line, **PAR)
    before = counters()
    got = run(segs, line, slice_chunks=slice_chunks)
    after = counters()
    Cs.same_result(got, want, f"({n}, {slice_chunks})")
    if not n:
        assert after == before                                        # nothing ran
        return
    nj = want["summary"]["n_junctions"]
    if n > 1:
        assert nj >= n // 2 and want["summary"]["n_T"] >= 1 and want["summary"]["n_X"] >= 1
    assert after["wf_count_launches"] == before["wf_count_launches"] + 1
    assert after["wf_write_launches"] == before["wf_write_launches"] + (nj > 0)
    assert after["wf_slices"] == Cs.slices_of(n, slice_chunks) and after["wf_junctions"] == nj
    assert after["wf_skipped_blocks"] == Cs.skipped_blocks(n, slice_chunks) == {257: 2, 513: 2, 256: 0, 1: 1, 63: 0}[n]


def test_no_output_depends_on_the_slicing():
    segs, line = Cs.model_case(42, Cs.SLICING_N)
    results = []
    for sc, n_slices, skipped in zip(Cs.SLICINGS, (3, 2, 1, 3, 1), (3, 1, 0, 3, 0)):
        got = run(segs, line, slice_chunks=sc)
        assert counters()["wf_slices"] == n_slices and counters()["wf_skipped_blocks"] == skipped == Cs.skipped_blocks(Cs.SLICING_N, sc), sc
        results.append(got)
    for got in results[1:]:
        Cs.same_result(got, results[0], "two slicings")
    want = M.wireframe(segs, line, **PAR)
    assert want["summary"]["n_junctions"] >= 500 and (want["vertices"]["n_junctions"] >= 3).sum() >= 10
    Cs.same_result(results[0], want, "every slicing")


def test_a_model_without_a_junction_skips_the_write_pass():
    segs, line = Cs.no_junction_case()
    before = counters()
    got = run(segs, line, slice_chunks=1)
    after = counters()
    assert after["wf_count_launches"] == before["wf_count_launches"] + 1 and after["wf_slices"] == 3
    assert after["wf_write_launches"] == before["wf_write_launches"] and after["wf_junctions"] == 0
    Cs.same_result(got, M.wireframe(segs, line, **PAR), "no junction")
    s = got["summary"]
    assert s["n_vertices"] == s["n_free_ends"] == 1200 and s["n_edges"] == s["n_components"] == 600 and s["largest_component"] == 1


def test_a_quiet_tile_next_to_a_busy_one():
    segs, line = Cs.quiet_tile_case()
    want = M.wireframe(segs, line, **PAR)
    assert want["summary"]["n_junctions"] == 22 and want["summary"]["n_L"] == 22 and (want["junctions"]["a"] >= 256).all()
    for sc in (0, Cs.ALL_CHUNKS):
        Cs.same_result(run(segs, line, slice_chunks=sc), want, f"quiet tile, slice_chunks={sc}")
    # the same with the busy tile first
    segs, line = segs[::-1].copy(), line[::-1].copy()
    want = M.wireframe(segs, line, **PAR)
    assert (want["junctions"]["b"] < 256).all()
    Cs.same_result(run(segs, line), want, "busy tile first")


def test_the_triangular_exit_does_not_eat_the_diagonal():
    """the only junction pairs the last query of the first tile with the first reference of the next chunk"""
    segs, line = Cs.diagonal_case()
    want = M.wireframe(segs, line, **Cs.HAND_PAR)
    assert [(int(j["a"]), int(j["b"])) for j in want["junctions"]] == [(255, 256)]
    for sc in (1, 2):
        got = run(segs, line, Cs.HAND_PAR, slice_chunks=sc)
        assert counters()["wf_junctions"] == 1 and counters()["wf_skipped_blocks"] == Cs.skipped_blocks(512, sc) == (1 if sc == 1 else 0)
        Cs.same_result(got, want, f"the diagonal, slice_chunks={sc}")


def test_hand_built_cases():
    for name, segs, line, par, expected in Cs.hand_cases():
        got = run(segs, line, par)
        Cs.check_expected(name, got, expected)
        Cs.same_result(got, M.wireframe(segs, line, form=M.junctions_scalar, **par), name)


# ---- at size ----------------------------------------------------------------------------------------------------------
def test_at_size():
    segs, line = Cs.large_case()
    assert len(segs) == 5000
    want = M.wireframe(segs, line, **PAR)
    s = want["summary"]
    print("at size:", s)
    assert (want["vertices"]["n_junctions"] >= 3).sum() >= 50 and s["n_X"] >= 1
    before = counters()
    got = run(segs, line)
    assert counters()["wf_slices"] == 20 and counters()["wf_write_launches"] == before["wf_write_launches"] + 1
    assert counters()["wf_skipped_blocks"] == Cs.skipped_blocks(5000, 0) == 190      # of 400: the lower triangle
    Cs.same_result(got, want, "5 000 segments, default slicing")
    Cs.same_result(run(segs, line, slice_chunks=7), want, "5 000 segments, 7 chunks per slice")


def test_reference_model(tmp_path):
    """the reference's published model of its testdata: the counts DESIGN §24 records, byte for byte from the GPU"""
    d = np.load(os.path.join(GOLDEN, "ref_c0_models.npz"))
    segs, line = d["optimized_segs"], d["optimized_line"]
    md = 0.001 * M.extent(segs)
    want = M.wireframe(segs, line, md, md, M.min_sin2_of(10.0))
    path = str(tmp_path / "ref.obj")
    got = api.build_wireframe(segs, line, md, obj_path=path)
    Cs.same_result(got, want, "ref_c0_models, optimised")
    s, V = got["summary"], got["vertices"]
    assert (s["n_junctions"], s["n_L"], s["n_T"], s["n_X"]) == (798, 646, 150, 2)
    assert (s["n_vertices"], s["n_junction_vertices"], s["n_free_ends"], s["n_edges"], s["n_components"], s["largest_component"]) == \
        (4402, 340, 4062, 2617, 1861, 49)
    assert dict(zip(*(x.tolist() for x in np.unique(V["degree"], return_counts=True)))) == \
        {1: 4062, 2: 105, 3: 109, 4: 58, 5: 36, 6: 15, 7: 8, 8: 5, 9: 3, 10: 1}
    assert s["max_spread"] == 0.009848941771128784 and len(np.unique(np.concatenate([got["junctions"]["a"], got["junctions"]["b"]]))) == 775
    assert s["n_junctions"] >= 500 and s["n_L"] >= 3 * s["n_T"] and s["n_X"] <= 0.01 * s["n_junctions"]
    # the OBJ file read back equals the arrays; the Python writer gives the same bytes
    text = open(path).read()
    assert text == M.obj_text(want)
    rows = [ln.split() for ln in text.splitlines()]
    assert np.array_equal(np.array([[float(x) for x in r[1:]] for r in rows if r[0] == "v"]), V["P"])
    assert np.array_equal(np.array([[int(x) - 1 for x in r[1:]] for r in rows if r[0] == "l"]),
                          np.stack([got["edges"]["v0"], got["edges"]["v1"]], 1))
    api.write_wireframe_obj(got, str(tmp_path / "py.obj"))
    assert open(str(tmp_path / "py.obj")).read() == text


def test_wrapper_takes_degrees_and_raises():
    segs, line = Cs.model_case(77, 400)
    want = M.wireframe(segs, line, 0.02, 0.04, M.min_sin2_of(20.0))
    Cs.same_result(api.build_wireframe(segs, line, 0.02, 0.04, 20.0, slice_chunks=1), want, "api.build_wireframe")
    with pytest.raises(ValueError):
        api.build_wireframe(segs, line, 0.02, min_angle=91.0)
    with pytest.raises(RuntimeError, match="max_distance"):
        api.build_wireframe(segs, line, -1.0)
    with pytest.raises(ValueError, match="one line index"):
        api.build_wireframe(segs, line[:-1], 0.02)


# ---- limits and argument checks ---------------------------------------------------------------------------------------
def test_a_total_that_wraps_in_32_bits_is_the_limit_error():
    """305 x 305 segments through the origin, every pair a junction: 93 025 x 93 024 / 2 = 2^32 + 31 811 504.  The 32-bit
    scan wraps to 31 811 504, below 2^28, which alone would pass for a short list; k_wf_check sees the descent."""
    segs, line = Cs.wrap_case()
    n = len(segs)
    assert n == 93025 and (n * (n - 1) // 2) % (1 << 32) == 31811504 < 1 << 28
    few = np.array([0, 1, 304, 305, 93024])
    sub = M.junctions(segs[few], line[few], 0.0, 0.0, 0.0)
    assert len(sub) == 10 and (sub["sa"] == 0.5).all() and (sub["sb"] == 0.5).all() and (sub["gap2"] == 0.0).all()
    before = counters()
    assert run(segs, line, dict(max_distance=0.0, max_extension=0.0, min_sin2=0.0), expect=-9) is None
    assert "2^28" in _lib.last_error()
    after = counters()
    assert after["wf_count_launches"] == before["wf_count_launches"] + 1
    assert after["wf_write_launches"] == before["wf_write_launches"]


def test_argument_errors_leave_the_handle_untouched():
    segs, line = Cs.model_case(1, 40)
    before = counters()
    for bad in (dict(max_distance=-1.0), dict(max_extension=float("inf")), dict(min_sin2=float("nan"))):
        assert run(segs, line, dict(PAR, **bad), expect=-1) is None
        assert list(bad)[0] in _lib.last_error()
    bad = segs.copy(); bad[7, 1] = np.nan
    assert run(bad, line, expect=-1) is None and "segment 7" in _lib.last_error()
    edge = segs.copy(); edge[39, 5] = 2.0 ** 100                    # the bound itself is allowed
    assert counters() == before                                     # nothing ran so far
    Cs.same_result(run(edge, line), M.wireframe(edge, line, **PAR), "a coordinate of 2^100")


# ---- the context form on the golden scene -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    from tests.golden.make_golden import golden_scene
    sc = golden_scene()
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages() and g.reconstruct3Dlines(3)
    yield dict(sc=sc, g=g)
    g.close()


def test_context_form_on_the_golden_scene(golden, tmp_path):
    g = golden["g"]
    L = _lib.load()
    before = g.get3Dlines()
    segs, line = api.flatten_lines(before)
    # the smallest of {1, 2, 5} x 10^-k x extent at which the scene's 83 lines have at least three junctions
    ext = M.extent(segs)
    for md in (f * 10.0 ** -k * ext for k in (3, 2, 1) for f in (1, 2, 5)):
        want = M.wireframe(segs, line, md, md, M.min_sin2_of(10.0))
        if want["summary"]["n_junctions"] >= 3:
            break
    print("golden scene: max_distance", md / ext, "x extent:", want["summary"])
    assert want["summary"]["n_junctions"] >= 3
    name_before = g.outputFilename()
    free = api.build_wireframe(segs, line, md)
    Cs.same_result(free, want, "stateless / model")
    mine = g.wireframe(md, obj_path=str(tmp_path / "golden.obj"))
    assert mine is not None
    Cs.same_result(mine, free, "context / stateless")
    assert open(str(tmp_path / "golden.obj")).read() == M.obj_text(want)
    assert g.setTimingLevel(2)
    try:
        assert g.wireframe(md) is not None and 0 < L.l3d_debug_counter(b"wf_kernel_ns") < 10 ** 9
    finally:
        g.setTimingLevel(1)
    # the context is untouched: its lines, its file name, and what a comparison and a merge make of them afterwards
    after = g.get3Dlines()
    a_segs, a_line = api.flatten_lines(after)
    assert a_segs.tobytes() == segs.tobytes() and a_line.tobytes() == line.tobytes() and len(after) == len(before)
    for A, B in zip(after, before):
        assert A["collinear3Dsegments"].tobytes() == B["collinear3Dsegments"].tobytes() and np.array_equal(A["residuals"], B["residuals"])
    assert g.outputFilename() == name_before
    cmp_ = g.compareLines(before, md)
    assert cmp_ is not None and cmp_[2]["n_matched"] == cmp_[2]["n_segments"] == len(segs)
    merged = g.mergeLines(5e-3 * M.extent(segs))
    stateless = api.merge_segments(segs, line, 5e-3 * M.extent(segs))[4]
    assert merged == stateless and merged["n_segments_in"] == len(segs)
    assert g.reconstruct3Dlines(3)


def test_context_errors(golden):
    g = golden["g"]
    L = _lib.load()
    slot = C.c_void_p(FILL)
    for par, word in ((_lib.WireframeParams(1e-3, -1.0, 0.03, 0, 0), "max_extension"), (_lib.WireframeParams(1e-3, 1e-3, 0.03, 0, 1), "reserved")):
        assert L.l3d_wireframe_lines(g.h, C.byref(par), C.byref(slot)) == -1 and word in _lib.last_error() and slot.value == FILL
    assert L.l3d_wireframe_lines(g.h, None, C.byref(slot)) == -1 and slot.value == FILL
    good = _lib.WireframeParams(1e-3, 1e-3, 0.03, 0, 0)
    assert L.l3d_wireframe_lines(g.h, C.byref(good), None) == -1 and "null" in _lib.last_error()
    assert g.wireframe(1e-3, min_angle=120.0) is None and g.last_status == -1        # printed, None
    assert g.wireframe(-1.0) is None and g.last_status == -1


def test_context_form_before_reconstruct3Dlines_returns_the_state_error():
    from line3dpp_amd.scene import make_scene
    sc = make_scene(4, 60, n_neighbors=2, seed=2)
    g = Line3D()
    g.add_scene(sc)
    assert g.wireframe(0.1) is None and g.last_status == -7
    assert "no 3D lines" in _lib.last_error()
    assert g.matchBegin()
    assert g.wireframe(0.1) is None and g.last_status == -7 and "split call" in _lib.last_error()
    g.matchAbort()
    g.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_wireframe(tmp_path):
    from line3dpp_amd.scene import make_scene
    exe = str(tmp_path / "wireframe_smoke")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "wireframe_smoke.cpp"), "-o", exe, "-L" + lib_dir,
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
    assert run_.stdout.count("[L3D++] ERROR: wireframe") == 2       # the call before the reconstruction, a bad angle
    raw = open(out_path, "rb").read()
    md, mx, min_sin2 = struct.unpack_from("<3d", raw, 0)
    n, nj, nv, ne = struct.unpack_from("<4Q", raw, 24)
    pos = 56
    segs = np.frombuffer(raw, np.float64, 6 * n, pos).reshape(n, 6); pos += 48 * n
    line = np.frombuffer(raw, np.uint32, n, pos); pos += 4 * n
    got = {}
    for name, dtype, count in (("junctions", M.JUNCTION_DTYPE, nj), ("vertices", M.VERTEX_DTYPE, nv), ("edges", M.EDGE_DTYPE, ne)):
        got[name] = np.frombuffer(raw, dtype, count, pos); pos += dtype.itemsize * count
    got["summary"] = dict(zip(M.SUMMARY_KEYS, struct.unpack_from("<12Q3d", raw, pos))); pos += 120
    assert pos == len(raw) and n > 10
    # (the facade's squared sine comes from the C library's sin, the model is given that very number)
    assert abs(min_sin2 - M.min_sin2_of(10.0)) < 1e-15 and mx == md
    Cs.same_result(got, M.wireframe(segs, line, md, mx, min_sin2), "the facade / the model")
    assert got["summary"]["n_junctions"] >= 1
