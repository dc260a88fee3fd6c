"""The planes of a 3D line model on the MI355X (k_planes.hip, l3d_planes.hip) against the numpy model of
tests/planes_model.py with tolerance 0 on every output byte, the scores of every hypothesis included -- every operation of
the contract is an exactly rounded fp64 one and the weights are integers: segment counts at the chunk and slice edges under
four slicings, hypothesis counts at the tile edge, inliers in the last partial chunk only, a tile of dead hypotheses beside
a live one in both orders, one model under five slicings, a model without a junction, the hand-built cases, a case at
size, the limit of 2^24 hypotheses, the argument errors, the context form on the golden scene, the C++ facade and the OBJ
file."""
import ctypes as C
import functools
import os
import struct
import subprocess
import time

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from line3dpp_amd.api import Line3D
from tests import planes_cases as Cs
from tests import planes_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A5A5A5A5A5A5A5A
COUNTERS = ("pl_score_launches", "pl_slices", "pl_hypotheses")
HAND = M.params(0.25, min_sin2=0.25)


def counters():
    L = _lib.load()
    return {k: L.l3d_debug_counter(k.encode()) for k in COUNTERS}


def run(segs, line, par, slice_chunks=0, expect=0, obj_path=None):
    """the stateless entry with the squared sine itself, as the model takes it -> the dict of the planes; a refused call
    must leave the handle's slot as it was"""
    L = _lib.load()
    segs = np.ascontiguousarray(segs, np.float64).reshape(-1, 6); line = np.ascontiguousarray(line, np.uint32)
    n = len(segs)
    p = _lib.PlanesParams(par["max_distance"], par["junction_distance"], par["junction_extension"], par["min_sin2"], par["min_length"],
                          par["min_segments"], par["max_planes"], par["max_tests"], slice_chunks, (0, 0))
    slot = C.c_void_p(FILL)
    rc = L.l3d_plane_segments(0, n, _lib.ptr(segs) if n else None, _lib.ptr(line) if n else None, C.byref(p), C.byref(slot))
    assert rc == expect, _lib.last_error()
    if rc:
        assert slot.value == FILL
        return None
    return api.take_planes(slot, obj_path)


@functools.lru_cache(maxsize=None)
def sized(n):
    """a generated case and what the model makes of it, computed once"""
    segs, line, planted = Cs.sized_case(n)
    want = M.detect(segs, line, Cs.PAR)
    assert Cs.admitted(want, planted) is None
    return segs, line, want


# ---- chunk, slice and tile edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_chunks", Cs.EDGE_SLICE_CHUNKS)
@pytest.mark.parametrize("n", Cs.EDGE_N)
def test_chunk_and_slice_edges(n, slice_chunks):
    segs, line, want = sized(n)
    before = counters()
    got = run(segs, line, Cs.PAR, slice_chunks)
    after = counters()
    Cs.same_result(got, want, f"({n}, {slice_chunks})")
    n_h = want["summary"]["n_hypotheses"]
    assert after["pl_hypotheses"] == n_h and (n_h >= 40 or n == 1)
    assert after["pl_score_launches"] == before["pl_score_launches"] + (n_h > 0)
    if n_h:
        assert after["pl_slices"] == Cs.slices_of(n, slice_chunks) == {63: [1] * 4, 256: [1] * 4, 257: [2, 2, 1, 1], 513: [3, 3, 2, 1]}[n][slice_chunks]
        assert want["summary"]["n_planes"] >= 1 and (want["scores"]["count"] >= 8).sum() >= 8


@pytest.mark.parametrize("teeth", (255, 256, 257))
def test_hypotheses_at_the_tile_edge(teeth):
    """a comb of `teeth` teeth has exactly that many junctions: one lane short of a tile, a full tile, one lane into the next"""
    g = Cs.segs(Cs.comb(teeth)); line = np.arange(len(g), dtype=np.uint32)
    want = M.detect(g, line, HAND)
    s = want["summary"]
    assert s["n_hypotheses"] == teeth and s["n_planes"] == 2 and want["planes"]["n_segments"].tolist() == [(teeth + 1) // 2 + 1, teeth // 2 + 1]
    for sc in (0, Cs.ALL_CHUNKS):
        got = run(g, line, HAND, sc)
        assert counters()["pl_hypotheses"] == teeth and counters()["pl_slices"] == (1 if sc or teeth < 256 else 2)
        Cs.same_result(got, want, f"{teeth} teeth, slice_chunks={sc}")


def test_inliers_in_the_last_partial_chunk_only():
    """segments 0 and 1 span z = 0; 2..255 and 256..511 lie far above it; the only other members are the last three of 515"""
    geo = [(0, 0, 0, 8, 0, 0), (0, 0, 0, 0, 8, 0)]
    geo += [(0, 10 * i, 100, 5, 10 * i, 100) for i in range(510)]
    geo += [(20, 0, 0, 28, 0, 0), (20, 3, 0, 28, 3, 0), (20, 6, 0, 28, 6, 0)]
    g = Cs.segs(geo); line = np.arange(len(g), dtype=np.uint32)
    assert len(g) == 515
    want = M.detect(g, line, HAND)
    assert want["summary"]["n_hypotheses"] == 1 and want["scores"]["count"].tolist() == [5]
    assert want["members"]["segment"].tolist() == [0, 1, 512, 513, 514]
    for sc in (0, 1, 2, 3):
        got = run(g, line, HAND, sc)
        assert counters()["pl_slices"] == Cs.slices_of(515, sc)
        Cs.same_result(got, want, f"the last chunk, slice_chunks={sc}")


def test_a_tile_of_dead_hypotheses_beside_a_live_one():
    fan, comb = Cs.dead_fan(256), Cs.comb(256)
    for name, geo, dead_first in (("dead first", fan + comb, True), ("live first", comb + fan, False)):
        g = Cs.segs(geo); line = np.arange(len(g), dtype=np.uint32)
        want = M.detect(g, line, HAND)
        s = want["summary"]
        assert s["n_hypotheses"] == 512 and s["n_dead"] == 256 and s["n_planes"] == 2
        dead = want["scores"]["count"] == 0
        assert dead[:256].all() == dead_first and dead[256:].all() != dead_first and dead.sum() == 256
        assert (want["scores"]["weight"][dead] == 0).all() and (want["scores"]["count"][~dead] == 129).all()
        for sc in (0, Cs.ALL_CHUNKS):
            Cs.same_result(run(g, line, HAND, sc), want, f"{name}, slice_chunks={sc}")


def test_no_output_depends_on_the_slicing():
    segs, line, want = sized(Cs.SLICING_N)
    results = []
    for sc, n_slices in zip(Cs.SLICINGS, (3, 2, 1, 3, 1)):
        results.append(run(segs, line, Cs.PAR, sc))
        assert counters()["pl_slices"] == n_slices, sc
    for got in results[1:]:
        Cs.same_result(got, results[0], "two slicings")
    assert want["summary"]["n_hypotheses"] >= 200 and want["summary"]["n_planes"] == 2
    Cs.same_result(results[0], want, "every slicing")


def test_a_model_without_a_junction_makes_no_score_launch():
    g = Cs.segs([(0, 10 * i, 0, 5, 10 * i, 0) for i in range(600)]); line = np.arange(600, dtype=np.uint32)
    before = counters()
    got = run(g, line, HAND, 1)
    after = counters()
    assert after["pl_score_launches"] == before["pl_score_launches"] and after["pl_hypotheses"] == 0
    Cs.same_result(got, M.detect(g, line, HAND), "no junction")
    s = got["summary"]
    assert s["n_segments"] == 600 and s["n_planes"] == 0 and s["length_total"] == 3000.0 and s["scale_exponent"] == 40


def test_hand_built_cases():
    for name, segs, line, par, expected in Cs.hand_cases():
        got = run(segs, line, par)
        Cs.check_expected(name, got, expected)
        Cs.same_result(got, M.detect(segs, line, par, "scalar"), name)


# ---- at size ----------------------------------------------------------------------------------------------------------
def test_at_size(tmp_path):
    segs, line, planted = Cs.large_case()
    assert len(segs) == 5000
    t0 = time.perf_counter()
    want = M.detect(segs, line, Cs.PAR)
    t_model = time.perf_counter() - t0
    assert Cs.admitted(want, planted) is None
    s = want["summary"]
    assert s["n_planes"] == 6 and s["n_hypotheses"] >= 2400
    path = str(tmp_path / "planes.obj")
    t0 = time.perf_counter()
    got = run(segs, line, Cs.PAR, obj_path=path)
    t_lib = time.perf_counter() - t0
    print("at size:", s, f"\nnumpy model {t_model:.3f} s, library call {t_lib:.4f} s (wall)")
    assert counters()["pl_slices"] == 20 and counters()["pl_hypotheses"] == s["n_hypotheses"]
    Cs.same_result(got, want, "5 000 segments, default slicing")
    Cs.same_result(run(segs, line, Cs.PAR, 7), want, "5 000 segments, 7 chunks per slice")
    # the OBJ file read back equals the arrays; the Python writer gives the same bytes
    text = open(path).read()
    assert text == M.obj_text(want)
    rows = [ln.split() for ln in text.splitlines()]
    assert np.array_equal(np.array([[float(x) for x in r[1:]] for r in rows if r[0] == "v"]).reshape(-1, 4, 3), got["planes"]["corners"])
    assert [[int(x) for x in r[1:]] for r in rows if r[0] == "f"] == [[4 * k + 1, 4 * k + 2, 4 * k + 3, 4 * k + 4] for k in range(6)]
    api.write_planes_obj(got, str(tmp_path / "py.obj"))
    assert open(str(tmp_path / "py.obj")).read() == text


def test_wrapper_takes_degrees_and_raises():
    segs, line, _ = Cs.sized_case(513)
    want = M.detect(segs, line, M.params(0.04, 0.05, 0.06, M.min_sin2_of(20.0), 30.0, 6, 5, 100))
    assert want["summary"]["n_planes"] >= 1
    Cs.same_result(api.detect_planes(segs, line, 0.04, 0.05, 0.06, 20.0, 30.0, 6, 5, 100, slice_chunks=1), want, "api.detect_planes")
    with pytest.raises(ValueError):
        api.detect_planes(segs, line, 0.02, min_angle=91.0)
    with pytest.raises(RuntimeError, match="max_distance"):
        api.detect_planes(segs, line, -1.0, 0.1, 0.1)
    with pytest.raises(ValueError, match="one line index"):
        api.detect_planes(segs, line[:-1], 0.02)


# ---- limits and argument checks ---------------------------------------------------------------------------------------
def test_more_than_2_24_hypotheses_is_the_limit_error():
    """5 794 segments through the origin, every pair a junction: 5 794 x 5 793 / 2 = 2^24 + 5 105"""
    i, j = np.meshgrid(np.arange(77.0), np.arange(77.0), indexing="ij")
    p = np.stack([i.ravel(), j.ravel(), np.ones(77 * 77)], 1)[:5794]
    segs = np.ascontiguousarray(np.concatenate([-p, p], 1)); line = np.arange(5794, dtype=np.uint32)
    assert 5794 * 5793 // 2 == (1 << 24) + 5105 and 5793 * 5792 // 2 <= 1 << 24
    par = M.params(0.0, 0.0, 0.0, 0.0)
    few = np.array([0, 1, 76, 77, 5793])
    assert M.detect(segs[few], line[few], dict(par, min_segments=1))["summary"]["n_hypotheses"] == 10
    before = counters()
    assert run(segs, line, par, expect=-9) is None
    assert "2^24" in _lib.last_error() and "junction_distance" in _lib.last_error()
    assert counters()["pl_score_launches"] == before["pl_score_launches"]


def test_argument_errors_leave_the_handle_untouched():
    segs, line, want = sized(63)
    before = counters()
    for bad in (dict(max_distance=-1.0), dict(junction_extension=float("inf")), dict(min_sin2=float("nan")), dict(min_segments=0)):
        assert run(segs, line, dict(Cs.PAR, **bad), expect=-1) is None
        assert list(bad)[0] in _lib.last_error()
    bad = segs.copy(); bad[7, 1] = np.nan
    assert run(bad, line, Cs.PAR, expect=-1) is None and "segment 7" in _lib.last_error()
    assert counters() == before                                     # nothing ran so far
    edge = segs.copy(); edge[62, 5] = 2.0 ** 100                    # the bound itself is allowed
    Cs.same_result(run(edge, line, Cs.PAR), M.detect(edge, line, Cs.PAR), "a coordinate of 2^100")


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
    # the smallest of {1, 2, 5} x 10^-k x extent at which the scene's lines lie in at least one plane of four segments
    ext = M.extent(segs)
    for md in (f * 10.0 ** -k * ext for k in (3, 2, 1) for f in (1, 2, 5)):
        want = M.detect(segs, line, M.params(md, 2 * md))
        if want["summary"]["n_planes"] >= 1:
            break
    print("golden scene: max_distance", md / ext, "x extent:", want["summary"])
    assert want["summary"]["n_planes"] >= 1
    name_before = g.outputFilename()
    free = api.detect_planes(segs, line, md, 2 * md)
    Cs.same_result(free, want, "stateless / model")
    mine = g.detectPlanes(md, 2 * md, obj_path=str(tmp_path / "golden.obj"))
    assert mine is not None
    Cs.same_result(mine, free, "context / stateless")
    assert open(str(tmp_path / "golden.obj")).read() == M.obj_text(want)
    assert g.setTimingLevel(2)
    try:
        assert g.detectPlanes(md, 2 * md) is not None
        kernel_ns, junction_ns = L.l3d_debug_counter(b"pl_kernel_ns"), L.l3d_debug_counter(b"pl_junction_ns")
        print("golden scene: pl_kernel_ns", kernel_ns, "pl_junction_ns", junction_ns)
        assert 0 < kernel_ns < 10 ** 9 and 0 < junction_ns < 10 ** 9
    finally:
        g.setTimingLevel(1)
    # the context is untouched: its lines, its file name, and what a wireframe makes of them afterwards
    after = g.get3Dlines()
    a_segs, a_line = api.flatten_lines(after)
    assert a_segs.tobytes() == segs.tobytes() and a_line.tobytes() == line.tobytes() and len(after) == len(before)
    for A, B in zip(after, before):
        assert A["collinear3Dsegments"].tobytes() == B["collinear3Dsegments"].tobytes() and np.array_equal(A["residuals"], B["residuals"])
    assert g.outputFilename() == name_before
    w_ctx, w_free = g.wireframe(md), api.build_wireframe(segs, line, md)
    assert w_ctx is not None and w_ctx["junctions"].tobytes() == w_free["junctions"].tobytes() and w_ctx["summary"] == w_free["summary"]
    assert g.reconstruct3Dlines(3)


def test_context_errors(golden):
    g = golden["g"]
    L = _lib.load()
    slot = C.c_void_p(FILL)
    ok = [1e-3, 1e-3, 1e-3, 0.03, 0.0, 4, 64, 4096, 0, (0, 0)]
    for k, v, word in ((2, -1.0, "junction_extension"), (9, (0, 1), "reserved"), (6, 0, "max_planes")):
        vals = list(ok); vals[k] = v
        par = _lib.PlanesParams(*vals)
        assert L.l3d_plane_lines(g.h, C.byref(par), C.byref(slot)) == -1 and word in _lib.last_error() and slot.value == FILL
    assert L.l3d_plane_lines(g.h, None, C.byref(slot)) == -1 and slot.value == FILL
    good = _lib.PlanesParams(*ok)
    assert L.l3d_plane_lines(g.h, C.byref(good), None) == -1 and "null" in _lib.last_error()
    assert g.detectPlanes(1e-3, min_angle=120.0) is None and g.last_status == -1        # printed, None
    assert g.detectPlanes(-1.0) is None and g.last_status == -1


def test_context_form_before_reconstruct3Dlines_returns_the_state_error():
    from line3dpp_amd.scene import make_scene
    sc = make_scene(4, 60, n_neighbors=2, seed=2)
    g = Line3D()
    g.add_scene(sc)
    assert g.detectPlanes(0.1) is None and g.last_status == -7
    assert "no 3D lines" in _lib.last_error()
    assert g.matchBegin()
    assert g.detectPlanes(0.1) is None and g.last_status == -7 and "split call" in _lib.last_error()
    g.matchAbort()
    g.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_detect_planes(tmp_path):
    from line3dpp_amd.scene import make_scene
    exe = str(tmp_path / "planes_smoke")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "planes_smoke.cpp"), "-o", exe, "-L" + lib_dir,
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
    assert run_.stdout.count("[L3D++] ERROR: detectPlanes") == 2    # the call before the reconstruction, a bad angle
    raw = open(out_path, "rb").read()
    par = _lib.PlanesParams.from_buffer_copy(raw[:64])
    n, n_p, n_m, n_h = struct.unpack_from("<4Q", raw, 64)
    pos = 96
    segs = np.frombuffer(raw, np.float64, 6 * n, pos).reshape(n, 6); pos += 48 * n
    line = np.frombuffer(raw, np.uint32, n, pos); pos += 4 * n
    got = {}
    for name, dtype, count in (("planes", M.PLANE_DTYPE, n_p), ("members", M.MEMBER_DTYPE, n_m), ("seg_planes", np.dtype("<u4"), n),
                               ("scores", M.SCORE_DTYPE, n_h)):
        got[name] = np.frombuffer(raw, dtype, count, pos); pos += dtype.itemsize * count
    got["summary"] = dict(zip(M.SUMMARY_KEYS, struct.unpack_from(M.SUMMARY_FORMAT, raw, pos))); pos += 136
    assert pos == len(raw) and n > 10
    # (the facade's squared sine comes from the C library's sin, the model is given that very number)
    assert abs(par.min_sin2 - M.min_sin2_of(10.0)) < 1e-15 and par.junction_distance == 2 * par.max_distance == 2 * par.junction_extension
    want = M.detect(segs, line, M.params(par.max_distance, par.junction_distance, par.junction_extension, par.min_sin2, par.min_length,
                                         par.min_segments, par.max_planes, par.max_tests))
    Cs.same_result(got, want, "the facade / the model")
    assert got["summary"]["n_hypotheses"] >= 1
