"""Two 3D line models compared on the MI355X (k_compare.hip, l3d_compare.hip) against the numpy model of
tests/compare_model.py with tolerance 0 on every field: tile, chunk and slice edges, every slicing of one case, hand-built
ties and thresholds, both directions, a model against itself, a case at size, the argument checks, the context form on
the golden scene against the stateless call, the model and the reference's own lines, and the C++ facade."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from line3dpp_amd.api import Line3D
from tests import compare_cases as Cs
from tests import compare_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR = Cs.DEFAULTS
FILL = 0x5A5A5A5A


def counters():
    L = _lib.load()
    return {k: L.l3d_debug_counter(k.encode()) for k in ("compare_launches", "compare_merge_launches", "compare_slices")}


def run(q, ql, r, rl, par=PAR, exclude_same_line=False, slice_chunks=0, want_q=True, want_r=True):
    """the stateless entry with the squared cosine itself, as the model takes it -> (matches_q, matches_r, summary_q,
    summary_r); a direction that is not asked for gives None"""
    L = _lib.load()
    q = np.ascontiguousarray(q, np.float64).reshape(-1, 6); r = np.ascontiguousarray(r, np.float64).reshape(-1, 6)
    ql = np.ascontiguousarray(ql, np.uint32); rl = np.ascontiguousarray(rl, np.uint32)
    out_q = np.full((len(q) + 1) * 6, FILL, np.uint32).view(_lib.LINE_MATCH_DTYPE)
    out_r = np.full((len(r) + 1) * 6, FILL, np.uint32).view(_lib.LINE_MATCH_DTYPE)
    sq = _lib.CompareSummary(); sr = _lib.CompareSummary()
    p = _lib.CompareParams(par["max_distance"], par["min_cos2"], par["min_overlap"], int(exclude_same_line), slice_chunks)
    rc = L.l3d_compare_segments(0, len(q), _lib.ptr(q) if len(q) else None, _lib.ptr(ql) if len(q) else None, len(r),
                                _lib.ptr(r) if len(r) else None, _lib.ptr(rl) if len(r) else None, C.byref(p),
                                _lib.ptr(out_q) if want_q else None, _lib.ptr(out_r) if want_r else None, C.byref(sq), C.byref(sr))
    assert rc == 0, _lib.last_error()
    for out in (out_q, out_r):
        assert (out[-1:].view(np.uint32) == FILL).all()            # nothing written past the last segment
    return (out_q[:-1] if want_q else None, out_r[:-1] if want_r else None, api.summary_dict(sq) if want_q else None,
            api.summary_dict(sr) if want_r else None)


def check_against_model(got, q, ql, r, rl, what, par=PAR, exclude_same_line=False):
    want = M.compare_both(q, ql, r, rl, exclude_same_line=exclude_same_line, **par)
    Cs.same_matches(got[0], want[0], what + ": Q in R")
    Cs.same_matches(got[1], want[1], what + ": R in Q")
    Cs.same_summary(got[2], want[2], what + ": Q in R")
    Cs.same_summary(got[3], want[3], what + ": R in Q")
    return want


# ---- tile, chunk and slice edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q,n_r,slice_chunks", Cs.EDGE_SHAPES)
def test_tile_chunk_and_slice_edges(n_q, n_r, slice_chunks):
    # (a single query is laid along a reference, so that the case is not an empty one)
    q, ql, r, rl = Cs.model_case(1000 * n_q + n_r, n_q, n_r, on_reference=1.0 if min(n_q, n_r) == 1 else 0.6)
    before = counters()
    got = run(q, ql, r, rl, slice_chunks=slice_chunks)
    after = counters()
    want = check_against_model(got, q, ql, r, rl, f"({n_q}, {n_r}, {slice_chunks})")
    if n_q > 1 and n_r > 1:
        assert (want[0]["segment"] >= 0).sum() >= max(n_q // 10, 1)
    if not n_q or not n_r:
        assert after == before                                     # nothing ran
        for m in got[:2]:
            assert (m["segment"] == -1).all() and (m["line"] == M.NONE).all() and not m["n_accepted"].any()
        return
    assert after["compare_launches"] == before["compare_launches"] + 2
    # which form ran: the slices of a direction are ceil(chunks of its references / slice_chunks); 0: one chunk per slice
    def slices(n_refs):
        chunks = -(-n_refs // Cs.CHUNK)
        return -(-chunks // min(slice_chunks or 1, chunks))
    merged = sum(slices(n) > 1 for n in (n_r, n_q))
    assert after["compare_merge_launches"] == before["compare_merge_launches"] + merged
    assert after["compare_slices"] == slices(n_q)                 # the last direction run: R in Q
    if (n_q, n_r, slice_chunks) == (256, 256, 1):
        assert merged == 0                                         # one workgroup per direction, direct write


def test_no_output_depends_on_the_slicing():
    n_q, n_r = Cs.SLICING_SHAPE
    q, ql, r, rl = Cs.model_case(42, n_q, n_r)
    results = []
    for sc, n_slices in zip(Cs.SLICINGS, (3, 2, 1, 3, 1)):
        before = counters()
        got = run(q, ql, r, rl, slice_chunks=sc, want_r=False)
        after = counters()
        assert after["compare_slices"] == n_slices, sc
        assert after["compare_merge_launches"] - before["compare_merge_launches"] == (n_slices > 1)
        results.append(got[0].tobytes())
    assert all(b == results[0] for b in results)
    Cs.same_matches(np.frombuffer(results[0], M.LINE_MATCH_DTYPE), M.compare(q, ql, r, rl, **PAR), "every slicing")


# ---- ties and thresholds ----------------------------------------------------------------------------------------------
def test_tie_across_a_slice_and_the_merge():
    q, ql, r, rl, expected = Cs.tie_across_slices()
    par = dict(PAR, max_distance=5.0)
    before = counters()
    got = run(q, ql, r, rl, par, slice_chunks=1, want_r=False)
    after = counters()
    assert after["compare_slices"] == 3 and after["compare_merge_launches"] == before["compare_merge_launches"] + 1
    Cs.check_expected("tie across slices", got[0], expected)
    Cs.same_matches(got[0], M.compare_scalar(q, ql, r, rl, **par), "tie across slices")


def test_hand_built_thresholds():
    for name, q, ql, r, rl, par, expected in Cs.hand_cases():
        excl = par["exclude_same_line"]
        thr = {k: v for k, v in par.items() if k != "exclude_same_line"}
        got = run(q, ql, r, rl, thr, exclude_same_line=excl)
        Cs.check_expected(name, got[0], expected)
        Cs.same_matches(got[0], M.compare_scalar(q, ql, r, rl, **par), name)
        Cs.same_matches(got[1], M.compare_scalar(r, rl, q, ql, **par), name + " (reverse)")


# ---- both directions --------------------------------------------------------------------------------------------------
def test_one_call_returns_both_directions():
    q, ql, r, rl = Cs.model_case(7, 300, 520)
    both = run(q, ql, r, rl)
    forth = run(q, ql, r, rl, want_r=False)
    back = run(r, rl, q, ql, want_r=False)
    assert forth[1] is None and forth[3] is None
    Cs.same_matches(both[0], forth[0], "Q in R alone"); Cs.same_summary(both[2], forth[2], "Q in R alone")
    Cs.same_matches(both[1], back[0], "R in Q by swapped sides"); Cs.same_summary(both[3], back[2], "R in Q by swapped sides")
    only_r = run(q, ql, r, rl, want_q=False)
    Cs.same_matches(only_r[1], both[1], "R in Q alone")
    assert (both[0]["segment"] >= 0).sum() > 30 and (both[1]["segment"] >= 0).sum() > 10


def test_wrapper_takes_degrees():
    q, ql, r, rl = Cs.model_case(77, 300, 600)
    want = M.compare_both(q, ql, r, rl, 0.02, M.min_cos2_of(20.0), 0.25)
    got = api.compare_segments(q, ql, r, rl, 0.02, 20.0, 0.25)
    check = (Cs.same_matches, Cs.same_matches, Cs.same_summary, Cs.same_summary)
    for k in range(4):
        check[k](got[k], want[k], "api.compare_segments")
    with pytest.raises(ValueError):
        api.compare_segments(q, ql, r, rl, 0.02, max_angle=91.0)
    with pytest.raises(RuntimeError, match="max_distance"):
        api.compare_segments(q, ql, r, rl, -1.0)


# ---- a model against itself -------------------------------------------------------------------------------------------
def test_a_model_against_itself():
    _, _, r, rl = Cs.model_case(3, 0, 700)
    r[500] = r[17]; rl[500] = rl[17] + 1
    got = run(r, rl, r, rl, slice_chunks=1)
    check_against_model(got, r, rl, r, rl, "itself")
    live = np.flatnonzero((r[:, :3] != r[:, 3:]).any(1))
    m = got[0]
    assert (m["distance"][live] == 0.0).all() and (m["overlap"][live] == 1.0).all()
    own = m["segment"][live] == live
    assert own.sum() == len(live) - 1 and m["segment"][500] == 17
    # pairs of the same line left out: no record names its own line
    got = run(r, rl, r, rl, exclude_same_line=True)
    want = check_against_model(got, r, rl, r, rl, "itself, same line excluded", exclude_same_line=True)
    hit = got[0]["segment"] >= 0
    assert hit.sum() >= 20 and (got[0]["line"][hit] != rl[hit]).all() and (got[0]["segment"][hit] != np.flatnonzero(hit)).all()
    assert got[0]["segment"][500] == 17 and got[0]["segment"][17] == 500
    assert want[2]["n_matched"] == hit.sum()


# ---- at size ----------------------------------------------------------------------------------------------------------
def test_at_size_under_the_default_slicing_and_one_chunk_per_slice():
    q, ql, r, rl = Cs.large_case()
    assert len(q) == 5000 and len(r) == 3000
    want = M.compare_both(q, ql, r, rl, **PAR)
    matched = int((want[0]["segment"] >= 0).sum()); ambiguous = int((want[0]["n_accepted"] > 1).sum())
    print(f"at size: {matched} of 5000 queries matched, {ambiguous} ambiguous; back: {want[3]['n_matched']} of 3000")
    assert 1000 <= matched <= 4000 and ambiguous >= 100
    before = counters()
    got = run(q, ql, r, rl)
    assert counters()["compare_slices"] == 20                     # R in Q: the 20 chunks of Q, one per slice
    fine = run(q, ql, r, rl, slice_chunks=1)
    assert counters()["compare_merge_launches"] == before["compare_merge_launches"] + 4
    for k in range(2):
        Cs.same_matches(got[k], want[k], f"direction {k}, default slicing")
        Cs.same_matches(fine[k], want[k], f"direction {k}, one chunk per slice")
        Cs.same_summary(got[2 + k], want[2 + k], f"direction {k}")


# ---- argument checks --------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched():
    L = _lib.load()
    q, ql, r, rl = Cs.model_case(1, 40, 30)
    out_q = np.full(40 * 6, FILL, np.uint32); out_r = np.full(30 * 6, FILL, np.uint32)
    s_q = np.full(14, FILL, np.uint32); s_r = np.full(14, FILL, np.uint32)
    p = _lib.ptr
    S = C.POINTER(_lib.CompareSummary)

    def call(par, q=q, ql=ql, r=r, rl=rl, n_q=40, n_r=30, null=()):
        a = dict(q=p(q), ql=p(ql), r=p(r), rl=p(rl))
        for k in null:
            a[k] = None
        rc = L.l3d_compare_segments(0, n_q, a["q"], a["ql"], n_r, a["r"], a["rl"], C.byref(par) if par is not None else None,
                                    p(out_q), p(out_r), C.cast(p(s_q), S), C.cast(p(s_r), S))
        assert all((x == FILL).all() for x in (out_q, out_r, s_q, s_r))
        return rc, _lib.last_error()

    good = (PAR["max_distance"], PAR["min_cos2"], PAR["min_overlap"], 0, 0)
    for k, name, bad in ((0, "max_distance", (-1.0, float("inf"), float("nan"))), (1, "min_cos2", (-0.1, 1.1, float("nan"))),
                         (2, "min_overlap", (-0.1, 1.1, float("nan"))), (3, "exclude_same_line", (2,))):
        for v in bad:
            vals = list(good); vals[k] = v
            rc, msg = call(_lib.CompareParams(*vals))
            assert rc == -1 and name in msg
    assert call(None)[0] == -1
    par = _lib.CompareParams(*good)
    bad_q = q.copy(); bad_q[7, 1] = np.nan
    rc, msg = call(par, q=bad_q)
    assert rc == -1 and "query" in msg and "segment 7" in msg
    bad_r = r.copy(); bad_r[29, 5] = -2.0 ** 101
    rc, msg = call(par, r=bad_r)
    assert rc == -1 and "reference" in msg and "segment 29" in msg
    edge = r.copy(); edge[29, 5] = 2.0 ** 100                     # the bound itself is allowed
    rc = L.l3d_compare_segments(0, 40, p(q), p(ql), 30, p(edge), p(rl), C.byref(par), None, None, None, None)
    assert rc == 0
    for k in ("q", "ql", "r", "rl"):
        rc, msg = call(par, null=(k,))
        assert rc == -1 and "null" in msg
    rc, msg = call(par, n_r=1 << 30)
    assert rc == -9 and "2^30" in msg and "reference" in msg


# ---- the context form on the golden scene -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    from tests.golden.make_golden import golden_scene
    sc = golden_scene()
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages() and g.reconstruct3Dlines(3)
    lines = g.get3Dlines()
    segs, line = api.flatten_lines(lines)
    yield dict(sc=sc, g=g, lines=lines, segs=segs, line=line, extent=M.extent(segs))
    g.close()


def test_context_equals_the_stateless_call_and_the_model(golden):
    G = golden
    g, segs, line = G["g"], G["segs"], G["line"]
    assert len(segs) > 50
    md = 1e-3 * G["extent"]
    ctx = g.compareLines(G["lines"], md)
    assert ctx is not None
    free = api.compare_segments(segs, line, segs, line, md)
    want = M.compare_both(segs, line, segs, line, md, M.min_cos2_of(10.0), 0.5)
    check = (Cs.same_matches, Cs.same_matches, Cs.same_summary, Cs.same_summary)
    for k in range(4):
        check[k](ctx[k], free[k], f"context / stateless [{k}]")
        check[k](ctx[k], want[k], f"context / model [{k}]")
    # every live segment is matched at distance 0
    live = (segs[:, :3] != segs[:, 3:]).any(1)
    assert live.sum() > 50 and (ctx[0]["segment"][live] >= 0).all() and (ctx[0]["distance"][live] == 0.0).all()
    # another Line3D as `other`: itself
    again = g.compareLines(g, md, slice_chunks=1)
    Cs.same_matches(again[0], ctx[0], "Line3D as other")


def test_context_kernel_time_at_timing_level_2(golden):
    g = golden["g"]
    L = _lib.load()
    assert g.setTimingLevel(2)
    try:
        assert g.compareLines(golden["lines"], 1e-3 * golden["extent"]) is not None
        assert 0 < L.l3d_debug_counter(b"compare_kernel_ns") < 10 ** 9
    finally:
        g.setTimingLevel(1)


def test_context_against_the_reference_own_lines(golden):
    """the lines oracle/_ref reconstructs from the same scene: every segment of either side has its counterpart within
    1e-4 of the extent, the bound tests/test_gpu_parity.py asserts on those end points"""
    from oracle import oracle as O
    assert O.have_reference(), "oracle/_ref is missing: no downgrade of the checker on the GPU box"
    G = golden
    r = O.Oracle(threads=1, reference=True)
    r.add_scene(G["sc"]); r.match_images(); r.reconstruct(3)
    rl = r.lines()
    rs, rline = api.flatten_lines(rl)
    assert len(rs) == len(G["segs"])
    res = G["g"].compareLines(rl, 1e-4 * G["extent"])
    assert res is not None
    mine, theirs, s_mine, s_theirs = res
    print("context in reference:", s_mine, "\nreference in context:", s_theirs, "\nworst distance / extent:",
          max(mine["distance"].max(), theirs["distance"].max()) / G["extent"])
    assert s_mine["n_matched"] == s_mine["n_segments"] == len(G["segs"])
    assert s_theirs["n_matched"] == s_theirs["n_segments"] == len(rs)
    Cs.same_matches(mine, M.compare(G["segs"], G["line"], rs, rline, 1e-4 * G["extent"], M.min_cos2_of(10.0), 0.5), "context / model")


def test_context_errors(golden):
    G = golden
    g = G["g"]
    L = _lib.load()
    n = len(G["segs"])
    out_m = np.full(n * 6, FILL, np.uint32); out_o = np.full(n * 6, FILL, np.uint32)
    p = _lib.ptr
    par = _lib.CompareParams(1e-3, 0.9, 0.5, 0, 0)

    def call(par=par, segs=G["segs"], line=G["line"]):
        rc = L.l3d_compare_lines(g.h, n, p(segs), p(line) if line is not None else None, C.byref(par) if par is not None else None,
                                 p(out_m), p(out_o), None, None)
        assert (out_m == FILL).all() and (out_o == FILL).all()
        return rc, _lib.last_error()

    assert call(par=None)[0] == -1 and call(line=None)[0] == -1
    rc, msg = call(par=_lib.CompareParams(1e-3, 0.9, 1.5, 0, 0))
    assert rc == -1 and "min_overlap" in msg
    bad = G["segs"].copy(); bad[3, 2] = np.inf
    rc, msg = call(segs=bad)
    assert rc == -1 and "other" in msg and "segment 3" in msg
    assert g.compareLines(G["lines"], 1e-3, max_angle=120.0) is None and g.last_status == -1     # printed, None
    assert g.compareLines(G["lines"], -1.0) is None and g.last_status == -1
    none = g.compareLines([], 1e-3)                               # an empty model: nothing matched, zero summaries
    assert len(none[0]) == n and (none[0]["segment"] == -1).all() and len(none[1]) == 0 and none[2]["n_segments"] == 0


def test_context_form_before_reconstruct3Dlines_returns_the_state_error():
    from line3dpp_amd.scene import make_scene
    sc = make_scene(4, 60, n_neighbors=2, seed=2)
    g = Line3D()
    g.add_scene(sc)
    other = [dict(segments=np.array([[0, 0, 0, 1, 0, 0.0]]))]
    assert g.compareLines(other, 0.1) is None and g.last_status == -7
    assert "no 3D lines" in _lib.last_error() or "has not run" in _lib.last_error()
    assert g.matchBegin()
    par = _lib.CompareParams(0.1, 0.9, 0.5, 0, 0)
    segs, line = api.flatten_lines(other)
    out = np.full(6, FILL, np.uint32)
    assert _lib.load().l3d_compare_lines(g.h, 1, _lib.ptr(segs), _lib.ptr(line), C.byref(par), None, _lib.ptr(out), None, None) == -7
    assert "split call" in _lib.last_error() and (out == FILL).all()
    g.matchAbort()
    g.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_compare_lines(tmp_path):
    from line3dpp_amd.scene import make_scene
    exe = str(tmp_path / "compare_smoke")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "compare_smoke.cpp"), "-o", exe, "-L" + lib_dir,
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
    assert run_.stdout.count("[L3D++] ERROR:") == 2 and "compareLines" in run_.stdout   # the call before the reconstruction, a bad angle
    raw = open(out_path, "rb").read()
    md, min_cos2, min_overlap, n_q, n_r = struct.unpack_from("<3d2I", raw, 0)
    pos = 32
    parts = []
    for n in (n_q, n_r):
        parts.append(np.frombuffer(raw, np.float64, 6 * n, pos).reshape(n, 6)); pos += 48 * n
        parts.append(np.frombuffer(raw, np.uint32, n, pos)); pos += 4 * n
    mine = np.frombuffer(raw, _lib.LINE_MATCH_DTYPE, n_q, pos); pos += 24 * n_q
    theirs = np.frombuffer(raw, _lib.LINE_MATCH_DTYPE, n_r, pos); pos += 24 * n_r
    assert pos == len(raw) and n_q > 10 and n_r > 10
    # (the facade's squared cosine comes from the C library's cos, the model is given that very number)
    assert abs(min_cos2 - M.min_cos2_of(10.0)) < 1e-15
    want = M.compare_both(*parts, md, min_cos2, min_overlap)
    Cs.same_matches(mine, want[0], "the facade's records / the model")
    Cs.same_matches(theirs, want[1], "the facade's records / the model (other side)")
    matched = int((mine["segment"] >= 0).sum())
    assert 0 < matched < n_q                                      # the moved lines are out of reach, the others are not
