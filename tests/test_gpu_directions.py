"""The directions of a 3D line model on the MI355X (k_directions.hip, l3d_directions.hip) against the numpy
model of tests/directions_model.py with tolerance 0 on every output byte, the scores of every hypothesis included -- every
operation of the contract is an exactly rounded fp64 one and the weights are integers: segment counts at the chunk, tile
and slice edges under four slicings, a family of parallel segments at the tile edge, inliers in the last partial chunk
only, a tile of point segments beside a live one in both orders, one model under five slicings, the relation symmetric at
its threshold, the hand-built cases, a case at size with the OBJ file, the argument errors, the context form on the golden
scene and the C++ facade."""
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
from tests import directions_cases as Cs
from tests import directions_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A5A5A5A5A5A5A5A
COUNTERS = ("dir_score_launches", "dir_slices", "dir_hypotheses")
EXACT = M.params(0.0, min_segments=3)                          # exactly parallel segments only


def counters():
    L = _lib.load()
    return {k: L.l3d_debug_counter(k.encode()) for k in COUNTERS}


def run(segs, line, par, slice_chunks=0, expect=0, obj_path=None):
    """the stateless entry with the squared sines themselves, as the model takes them -> the dict of the directions; a
    refused call must leave the handle's slot as it was"""
    L = _lib.load()
    segs = np.ascontiguousarray(segs, np.float64).reshape(-1, 6); line = np.ascontiguousarray(line, np.uint32)
    n = len(segs)
    p = _lib.DirectionsParams(par["max_sin2"], par["min_length"], par["max_frame_cos2"], par["min_segments"], par["max_directions"],
                              par["max_tests"], slice_chunks, par["frame_search"], (0,) * 5)
    slot = C.c_void_p(FILL)
    rc = L.l3d_direction_segments(0, n, _lib.ptr(segs) if n else None, _lib.ptr(line) if n else None, C.byref(p), C.byref(slot))
    assert rc == expect, _lib.last_error()
    if rc:
        assert slot.value == FILL
        return None
    return api.take_directions(slot, obj_path)


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
    assert after["dir_hypotheses"] == n and after["dir_score_launches"] == before["dir_score_launches"] + 1
    assert after["dir_slices"] == Cs.slices_of(n, slice_chunks) == {1: [1] * 4, 63: [1] * 4, 256: [1] * 4, 257: [2, 2, 1, 1], 513: [3, 3, 2, 1]}[n][slice_chunks]
    if n > 1:
        assert want["summary"]["n_directions"] == 4 and (want["scores"]["count"] >= 8).sum() >= 32


@pytest.mark.parametrize("k", (255, 256, 257))
def test_a_family_at_the_tile_edge(k):
    """k exactly parallel segments, alternately reversed, with three along x behind them: the family ends one lane short of
    the first tile of hypotheses and the first chunk of segments, fills them, and reaches one into the next"""
    g = Cs.segs(Cs.parallel_family(k, 3)); line = np.arange(len(g), dtype=np.uint32)
    want = M.detect(g, line, EXACT)
    assert want["scores"]["count"].tolist() == [k] * k + [3] * 3 and want["directions"]["n_segments"].tolist() == [k, 3]
    assert want["summary"]["n_dropped"] == k + 1 and want["summary"]["frame_axes"] == 1
    for sc in (0, Cs.ALL_CHUNKS):
        got = run(g, line, EXACT, sc)
        assert counters()["dir_hypotheses"] == k + 3 and counters()["dir_slices"] == (1 if sc or k + 3 <= 256 else 2)
        Cs.same_result(got, want, f"a family of {k}, slice_chunks={sc}")


def test_inliers_in_the_last_partial_chunk_only():
    """segment 0 runs along (3, 4, 12); 1..511 along x; the only other segments along it are the last three of 515"""
    geo = [(0, 0, 0, 3, 4, 12)] + [(0, i, 50, 5, i, 50) for i in range(511)]
    geo += [(20, 0, 0, 23, 4, 12), (26, 4, 12, 23, 0, 0), (30, 0, 0, 36, 8, 24)]
    g = Cs.segs(geo); line = np.arange(len(g), dtype=np.uint32)
    assert len(g) == 515
    want = M.detect(g, line, EXACT)
    assert want["scores"]["count"][0] == 4 and want["scores"]["count"][1:512].tolist() == [511] * 511
    assert want["members"]["segment"][want["members"]["direction"] == 1].tolist() == [0, 512, 513, 514]
    for sc in (0, 1, 2, 3):
        got = run(g, line, EXACT, sc)
        assert counters()["dir_slices"] == Cs.slices_of(515, sc)
        Cs.same_result(got, want, f"the last chunk, slice_chunks={sc}")


def test_a_tile_of_point_segments_beside_a_live_one():
    live = Cs.parallel_family(250, 6)
    points = [(i, 7, 7, i, 7, 7) for i in range(256)]
    for name, geo, points_first in (("points first", points + live, True), ("live first", live + points, False)):
        g = Cs.segs(geo); line = np.arange(len(g), dtype=np.uint32)
        want = M.detect(g, line, EXACT)
        s = want["summary"]
        assert s["n_segments"] == 512 and s["n_point_segments"] == 256 and s["n_directions"] == 2
        dead = want["scores"]["count"] == 0
        assert dead[:256].all() == points_first and dead[256:].all() != points_first and dead.sum() == 256
        assert (want["scores"]["weight"][dead] == 0).all() and sorted(set(want["scores"]["count"][~dead].tolist())) == [6, 250]
        assert not want["seg_directions"][dead].any() and want["seg_directions"][~dead].all()
        for sc in (0, Cs.ALL_CHUNKS):
            Cs.same_result(run(g, line, EXACT, sc), want, f"{name}, slice_chunks={sc}")


def test_no_output_depends_on_the_slicing():
    segs, line, want = sized(Cs.SLICING_N)
    results = []
    for sc, n_slices in zip(Cs.SLICINGS, (3, 2, 1, 3, 1)):
        results.append(run(segs, line, Cs.PAR, sc))
        assert counters()["dir_slices"] == n_slices, sc
    for got in results[1:]:
        Cs.same_result(got, results[0], "two slicings")
    assert want["summary"]["n_directions"] == 4 and want["summary"]["frame_axes"] == 3
    Cs.same_result(results[0], want, "every slicing")


def test_the_relation_is_symmetric_at_its_threshold():
    """For a pair of segments, max_sin2 is set to the model's x2 of the pair: each must be the other's inlier on the device,
    whichever is the hypothesis, and neither at the next value below.  With max_sin2 = 0 every live hypothesis counts
    itself."""
    segs, line, _ = Cs.sized_case(63)
    live = np.flatnonzero(M.weights(segs)["live"])
    D = [[float(x) for x in d] for d in M.units_scalar(segs)]
    rng = np.random.default_rng(5)
    pairs = [(int(a), int(b)) for a, b in rng.choice(live, (24, 2)) if a != b]
    assert len(pairs) >= 20
    for a, b in pairs:
        x2 = M.sin2(D[a], D[b])
        assert x2 == M.sin2(D[b], D[a]) and 0.0 < x2 <= 1.0
        two = segs[[a, b]]
        at = run(two, [0, 1], M.params(x2, min_segments=1))
        below = run(two, [0, 1], M.params(float(np.nextafter(x2, 0.0)), min_segments=1))
        assert at["scores"]["count"].tolist() == [2, 2] and below["scores"]["count"].tolist() == [1, 1], (a, b, x2)
        assert at["scores"]["weight"][0] == at["scores"]["weight"][1] == below["scores"]["weight"].sum()
    alone = dict(EXACT, min_segments=1, max_directions=64)
    got = run(segs, line, alone)
    Cs.same_result(got, M.detect(segs, line, alone), "max_sin2 = 0")
    is_live = np.zeros(len(segs), bool); is_live[live] = True
    assert (got["scores"]["count"][is_live] >= 1).all() and not got["scores"]["count"][~is_live].any()
    # and over a whole model: the number of hypotheses that count s equals the number s counts
    segs, line, want = sized(513)
    got = run(segs, line, Cs.PAR)
    ok = M.relation(M.units(segs), M.weights(segs), Cs.PAR["max_sin2"])
    assert np.array_equal(ok, ok.T) and got["scores"]["count"].tolist() == ok.sum(1).tolist() == ok.sum(0).tolist()


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
    assert s["n_directions"] == 4 and s["frame_axes"] == 3
    path = str(tmp_path / "directions.obj")
    t0 = time.perf_counter()
    got = run(segs, line, Cs.PAR, obj_path=path)
    t_lib = time.perf_counter() - t0
    print("at size:", s, f"\nnumpy model {t_model:.3f} s, library call {t_lib:.4f} s (wall)")
    assert counters()["dir_slices"] == 20 and counters()["dir_hypotheses"] == 5000
    Cs.same_result(got, want, "5 000 segments, default slicing")
    Cs.same_result(run(segs, line, Cs.PAR, 7), want, "5 000 segments, 7 chunks per slice")
    # the OBJ file read back equals the arrays; the Python writer gives the same bytes
    text = open(path).read()
    assert text == M.obj_text(want)
    rows = [ln.split() for ln in text.splitlines()]
    ends = np.array([[float(x) for x in r[1:]] for r in rows if r[0] == "v"]).reshape(-1, 2, 3)
    P = got["directions"]
    assert np.array_equal(ends[:, 0], P["centroid"] + P["t_min"][:, None] * P["D_fit"])
    assert np.array_equal(ends[:, 1], P["centroid"] + P["t_max"][:, None] * P["D_fit"])
    assert [[int(x) for x in r[1:]] for r in rows if r[0] == "l"] == [[2 * k + 1, 2 * k + 2] for k in range(4)]
    api.write_directions_obj(got, str(tmp_path / "py.obj"))
    assert open(str(tmp_path / "py.obj")).read() == text


def test_wrapper_takes_degrees_and_raises():
    segs, line, _ = Cs.sized_case(513)
    want = M.detect(segs, line, M.params(M.sin2_of(2.0), 30.0, M.sin2_of(3.0), 6, 5, 100, 4))
    assert want["summary"]["n_directions"] >= 4
    Cs.same_result(api.detect_directions(segs, line, 2.0, 30.0, 6, 5, 100, 3.0, 4, slice_chunks=1), want, "api.detect_directions")
    with pytest.raises(ValueError):
        api.detect_directions(segs, line, 91.0)
    with pytest.raises(RuntimeError, match="min_length"):
        api.detect_directions(segs, line, 1.0, min_length=-1.0)
    with pytest.raises(ValueError, match="one line index"):
        api.detect_directions(segs, line[:-1], 1.0)


def test_argument_errors_leave_the_handle_untouched():
    segs, line, want = sized(63)
    before = counters()
    for bad in (dict(max_sin2=-1.0), dict(max_frame_cos2=float("nan")), dict(min_length=float("inf")), dict(min_segments=0),
                dict(max_directions=0), dict(max_tests=0), dict(frame_search=65)):
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
    # the smallest of these angles at which the scene's lines run in at least one direction of four segments
    for angle in (1.0, 2.0, 5.0, 10.0, 20.0, 45.0):
        want = M.detect(segs, line, M.params(M.sin2_of(angle)))
        if want["summary"]["n_directions"] >= 1:
            break
    print("golden scene: max_angle", angle, "degrees:", want["summary"])
    assert want["summary"]["n_directions"] >= 1
    name_before = g.outputFilename()
    free = api.detect_directions(segs, line, angle)
    Cs.same_result(free, want, "stateless / model")
    mine = g.detectDirections(angle, obj_path=str(tmp_path / "golden.obj"))
    assert mine is not None
    Cs.same_result(mine, free, "context / stateless")
    assert open(str(tmp_path / "golden.obj")).read() == M.obj_text(want)
    assert g.setTimingLevel(2)
    try:
        assert g.detectDirections(angle) is not None
        kernel_ns = L.l3d_debug_counter(b"dir_kernel_ns")
        print("golden scene: dir_kernel_ns", kernel_ns)
        assert 0 < kernel_ns < 10 ** 9
    finally:
        g.setTimingLevel(1)
    # the context is untouched: its lines, its file name, and what the plane detection makes of them afterwards
    after = g.get3Dlines()
    a_segs, a_line = api.flatten_lines(after)
    assert a_segs.tobytes() == segs.tobytes() and a_line.tobytes() == line.tobytes() and len(after) == len(before)
    for A, B in zip(after, before):
        assert A["collinear3Dsegments"].tobytes() == B["collinear3Dsegments"].tobytes() and np.array_equal(A["residuals"], B["residuals"])
    assert g.outputFilename() == name_before
    md = 1e-2 * M.extent(segs)
    p_ctx, p_free = g.detectPlanes(md, 2 * md), api.detect_planes(segs, line, md, 2 * md)
    assert p_ctx is not None and p_ctx["summary"] == p_free["summary"]
    for k in ("planes", "members", "seg_planes", "scores"):
        assert p_ctx[k].tobytes() == p_free[k].tobytes(), k
    assert g.reconstruct3Dlines(3)


def test_context_errors(golden):
    g = golden["g"]
    L = _lib.load()
    slot = C.c_void_p(FILL)
    ok = [0.01, 0.0, 0.01, 4, 16, 4096, 0, 16, (0,) * 5]
    for k, v, word in ((0, 1.5, "max_sin2"), (8, (0, 0, 0, 0, 1), "reserved"), (4, 0, "max_directions"), (7, 0, "frame_search")):
        vals = list(ok); vals[k] = v
        par = _lib.DirectionsParams(*vals)
        assert L.l3d_direction_lines(g.h, C.byref(par), C.byref(slot)) == -1 and word in _lib.last_error() and slot.value == FILL
    assert L.l3d_direction_lines(g.h, None, C.byref(slot)) == -1 and slot.value == FILL
    good = _lib.DirectionsParams(*ok)
    assert L.l3d_direction_lines(g.h, C.byref(good), None) == -1 and "null" in _lib.last_error()
    assert g.detectDirections(120.0) is None and g.last_status == -1               # printed, None
    assert g.detectDirections(1.0, min_length=-1.0) is None and g.last_status == -1


def test_context_form_before_reconstruct3Dlines_returns_the_state_error():
    from line3dpp_amd.scene import make_scene
    sc = make_scene(4, 60, n_neighbors=2, seed=2)
    g = Line3D()
    g.add_scene(sc)
    assert g.detectDirections(1.0) is None and g.last_status == -7
    assert "no 3D lines" in _lib.last_error()
    assert g.matchBegin()
    assert g.detectDirections(1.0) is None and g.last_status == -7 and "split call" in _lib.last_error()
    g.matchAbort()
    g.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_detect_directions(tmp_path):
    from line3dpp_amd.scene import make_scene
    exe = str(tmp_path / "directions_smoke")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "directions_smoke.cpp"), "-o", exe, "-L" + lib_dir,
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
    assert run_.stdout.count("[L3D++] ERROR: detectDirections") == 2    # the call before the reconstruction, a bad angle
    raw = open(out_path, "rb").read()
    par = _lib.DirectionsParams.from_buffer_copy(raw[:64])
    n, n_d, n_m, n_h = struct.unpack_from("<4Q", raw, 64)
    pos = 96
    segs = np.frombuffer(raw, np.float64, 6 * n, pos).reshape(n, 6); pos += 48 * n
    line = np.frombuffer(raw, np.uint32, n, pos); pos += 4 * n
    got = {}
    for name, dtype, count in (("directions", M.DIRECTION_DTYPE, n_d), ("members", M.MEMBER_DTYPE, n_m), ("seg_directions", np.dtype("<u4"), n),
                               ("scores", M.SCORE_DTYPE, n_h)):
        got[name] = np.frombuffer(raw, dtype, count, pos); pos += dtype.itemsize * count
    v = struct.unpack_from(M.SUMMARY_FORMAT, raw, pos); pos += 200
    got["summary"] = dict(zip(M.SUMMARY_KEYS[:15], v[:15]), frame=list(v[15:18]), R=list(v[18:27]))
    got["R"] = np.array(got["summary"]["R"]).reshape(3, 3)
    assert pos == len(raw) and n > 10 and n_h == n
    # (the facade's squared sines come from the C library's sin, the model is given those very numbers)
    assert abs(par.max_sin2 - M.sin2_of(15.0)) < 1e-15 and abs(par.max_frame_cos2 - M.sin2_of(20.0)) < 1e-15
    want = M.detect(segs, line, M.params(par.max_sin2, par.min_length, par.max_frame_cos2, par.min_segments, par.max_directions,
                                         par.max_tests, par.frame_search))
    Cs.same_result(got, want, "the facade / the model")
    assert got["summary"]["n_directions"] >= 1
