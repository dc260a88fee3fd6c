"""Near-duplicate 3D lines merged on the MI355X (k_merge.hip, l3d_merge.hip) against the numpy model of
tests/merge_model.py with tolerance 0 on every output byte -- every operation of the contract is an exactly rounded fp64
one, as in §18: tile, chunk and slice edges with the launches they take, every slicing of one case, a model without a
pair, a quiet tile next to a busy one, the hand-built cases, a case at size, the reference's published model, a list
whose 32-bit total wraps, the argument checks, the context form on the golden scene and the C++ facade."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib, api, io
from line3dpp_amd.api import Line3D
from tests import merge_cases as Cs
from tests import merge_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PAR = Cs.DEFAULTS
FILL = 0x5A5A5A5A
COUNTERS = ("merge_count_launches", "merge_write_launches", "merge_slices", "merge_pairs")


def counters():
    L = _lib.load()
    return {k: L.l3d_debug_counter(k.encode()) for k in COUNTERS}


def run(segs, line, par=PAR, slice_chunks=0, expect=0):
    """the stateless entry with the squared cosine itself, as the model takes it -> (segs_out, line_out, line_map,
    line_info, summary); every buffer has one element more than the call is told, which must keep its pattern"""
    L = _lib.load()
    segs = np.ascontiguousarray(segs, np.float64).reshape(-1, 6); line = np.ascontiguousarray(line, np.uint32)
    n = len(segs)
    line_map = np.full(n + 1, FILL, np.uint32); out = np.full(12 * (n + 1), FILL, np.uint32).view(np.float64).reshape(-1, 6)
    out_line = np.full(n + 1, FILL, np.uint32); info = np.full(4 * (n + 1), FILL, np.uint32).view(_lib.MERGE_LINE_INFO_DTYPE)
    n_segs = C.c_uint32(FILL); n_lines = C.c_uint32(FILL); s = _lib.MergeSummary()
    p = _lib.MergeParams(par["max_distance"], par["min_cos2"], par["min_overlap"], slice_chunks, 0)
    rc = L.l3d_merge_segments(0, n, _lib.ptr(segs) if n else None, _lib.ptr(line) if n else None, C.byref(p), _lib.ptr(line_map), n,
                              _lib.ptr(out), _lib.ptr(out_line), C.byref(n_segs), n, _lib.ptr(info), C.byref(n_lines), C.byref(s))
    assert rc == expect, _lib.last_error()
    if rc:
        assert all((x.view(np.uint32) == FILL).all() for x in (line_map, out, out_line, info)) and n_segs.value == n_lines.value == FILL
        return None
    ns, nl = n_segs.value, n_lines.value
    assert ns <= n and nl <= n
    for buf, used in ((line_map, n), (out, ns), (out_line, ns), (info, nl)):
        assert (buf[used:].view(np.uint32) == FILL).all()            # nothing written past the end
    return out[:ns], out_line[:ns], line_map[:n], info[:nl], api.merge_summary_dict(s)


def slices_of(n, slice_chunks):
    chunks = -(-n // Cs.CHUNK)
    return -(-chunks // min(slice_chunks or 1, chunks)) if n else 0


# ---- tile, chunk and slice edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,slice_chunks", Cs.EDGE_SHAPES)
def test_tile_chunk_and_slice_edges(n, slice_chunks):
    segs, line = Cs.model_case(1000 + n, n)
    want = M.merge(segs, line, **PAR)
    before = counters()
    got = run(segs, line, slice_chunks=slice_chunks)
    after = counters()
    Cs.same_result(got, want, f"({n}, {slice_chunks})")
    if not n:
        assert after == before                                        # nothing ran
        return
    if n > 1:
        assert want[4]["n_pairs"] >= n // 10 and want[4]["n_merged_components"] >= 1
    assert after["merge_count_launches"] == before["merge_count_launches"] + 1
    assert after["merge_write_launches"] == before["merge_write_launches"] + (want[4]["n_pairs"] > 0)
    assert after["merge_slices"] == slices_of(n, slice_chunks) and after["merge_pairs"] == want[4]["n_pairs"]


def test_no_output_depends_on_the_slicing():
    segs, line = Cs.model_case(42, Cs.SLICING_N)
    results = []
    for sc, n_slices in zip(Cs.SLICINGS, (3, 2, 1, 3, 1)):
        got = run(segs, line, slice_chunks=sc)
        assert counters()["merge_slices"] == n_slices, sc
        results.append(got)
    for got in results[1:]:
        Cs.same_result(got, results[0], "two slicings")
    want = M.merge(segs, line, **PAR)
    assert want[4]["n_merged_components"] >= 50 and want[4]["largest_component"] >= 4
    Cs.same_result(results[0], want, "every slicing")


def test_a_model_without_a_pair_skips_the_write_pass():
    segs, line = Cs.no_pair_case()
    before = counters()
    got = run(segs, line, slice_chunks=1)
    after = counters()
    assert after["merge_count_launches"] == before["merge_count_launches"] + 1 and after["merge_slices"] == 3
    assert after["merge_write_launches"] == before["merge_write_launches"] and after["merge_pairs"] == 0
    Cs.same_result(got, M.merge(segs, line, **PAR), "no pair")
    assert np.array_equal(got[0], segs) and np.array_equal(got[2], np.arange(len(segs))) and (got[3]["n_members"] == 1).all()


def test_a_quiet_tile_next_to_a_busy_one():
    segs, line = Cs.quiet_tile_case()
    want = M.merge(segs, line, **PAR)
    assert want[4]["n_pairs"] == 44 and want[4]["n_merged_components"] == 22 and (want[2][:256] == np.arange(256)).all()
    for sc in (0, Cs.ALL_CHUNKS):
        Cs.same_result(run(segs, line, slice_chunks=sc), want, f"quiet tile, slice_chunks={sc}")
    # the same with the busy tile first
    segs, line = segs[::-1].copy(), line[::-1].copy()
    Cs.same_result(run(segs, line), M.merge(segs, line, **PAR), "busy tile first")


def test_hand_built_cases():
    for name, segs, line, expected in Cs.hand_cases():
        got = run(segs, line, Cs.HAND_PAR)
        Cs.check_expected(name, got, expected)
        Cs.same_result(got, M.merge(segs, line, form=M.pairs_scalar, **Cs.HAND_PAR), name)


# ---- at size ----------------------------------------------------------------------------------------------------------
def test_at_size():
    segs, line = Cs.large_case()
    assert len(segs) == 5000
    want = M.merge(segs, line, **PAR)
    s = want[4]
    print("at size:", s)
    assert s["n_merged_components"] >= 50 and (want[3]["n_members"] >= 4).sum() >= 1
    before = counters()
    got = run(segs, line)
    assert counters()["merge_slices"] == 20 and counters()["merge_write_launches"] == before["merge_write_launches"] + 1
    Cs.same_result(got, want, "5 000 segments, default slicing")
    Cs.same_result(run(segs, line, slice_chunks=7), want, "5 000 segments, 7 chunks per slice")


def test_reference_model():
    """the reference's published model of its testdata: the counts DESIGN §19 records, byte for byte from the GPU"""
    d = np.load(os.path.join(GOLDEN, "ref_c0_models.npz"))
    segs, line = d["optimized_segs"], d["optimized_line"]
    md = 0.001 * M.extent(segs)
    want = M.merge(segs, line, md, M.min_cos2_of(10.0), 0.5)
    got = api.merge_segments(segs, line, md)
    Cs.same_result(got, want, "ref_c0_models, optimised")
    s = got[4]
    assert (s["n_pairs"], s["n_lines_in"], s["n_lines_out"], s["n_merged_components"], s["largest_component"]) == (688, 2490, 2086, 334, 6)
    assert s["n_lines_out"] <= 0.9 * s["n_lines_in"]
    # the duplicates that are left, counted by the comparison stage on the GPU (the bound of tests/test_merge_host.py)
    dup_before = api.compare_segments(segs, line, segs, line, md, exclude_same_line=True)[2]["n_matched"]
    dup_after = api.compare_segments(got[0], got[1], got[0], got[1], md, exclude_same_line=True)[2]["n_matched"]
    found = api.compare_segments(segs, line, got[0], got[1], 2 * md)[2]
    assert (dup_before, dup_after) == (641, 11) and dup_after <= 0.1 * dup_before
    assert found["n_matched"] == found["n_segments"] == len(segs)


def test_wrapper_takes_degrees_and_raises():
    segs, line = Cs.model_case(77, 400)
    want = M.merge(segs, line, 0.02, M.min_cos2_of(20.0), 0.25)
    Cs.same_result(api.merge_segments(segs, line, 0.02, 20.0, 0.25, slice_chunks=1), want, "api.merge_segments")
    with pytest.raises(ValueError):
        api.merge_segments(segs, line, 0.02, max_angle=91.0)
    with pytest.raises(RuntimeError, match="max_distance"):
        api.merge_segments(segs, line, -1.0)
    with pytest.raises(ValueError, match="one line index"):
        api.merge_segments(segs, line[:-1], 0.02)


# ---- limits and argument checks ---------------------------------------------------------------------------------------
def test_a_total_that_wraps_in_32_bits_is_the_limit_error():
    """65 537 copies of one segment, each on a line of its own: 65 537 x 65 536 = 2^32 + 65 536 accepted pairs.  The
    32-bit scan wraps to 65 536, which alone would pass for a short list; k_merge_check sees the descent."""
    n = 65537
    segs = np.tile(np.array([[0.0, 0, 0, 1, 0, 0]]), (n, 1)); line = np.arange(n, dtype=np.uint32)
    before = counters()
    assert run(segs, line, expect=-9) is None
    assert "2^28" in _lib.last_error()
    after = counters()
    assert after["merge_count_launches"] == before["merge_count_launches"] + 1
    assert after["merge_write_launches"] == before["merge_write_launches"]


def test_argument_errors_leave_the_outputs_untouched():
    segs, line = Cs.model_case(1, 40)
    before = counters()
    for bad in (dict(max_distance=-1.0), dict(min_cos2=1.5), dict(min_overlap=float("nan"))):
        assert run(segs, line, dict(PAR, **bad), expect=-1) is None
        assert list(bad)[0] in _lib.last_error()
    bad = segs.copy(); bad[7, 1] = np.nan
    assert run(bad, line, expect=-1) is None and "segment 7" in _lib.last_error()
    edge = segs.copy(); edge[39, 5] = 2.0 ** 100                    # the bound itself is allowed
    assert counters() == before                                     # nothing ran so far
    Cs.same_result(run(edge, line), M.merge(edge, line, **PAR), "a coordinate of 2^100")


# ---- the context form on the golden scene -----------------------------------------------------------------------------
# the smallest of {1, 2, 5} x 10^-k x extent at which the model merges at least three components of the golden scene's 83
# lines: 5e-3 (4 pairs, 3 components of 2 lines, 80 lines left; 2e-3 and everything below: no pair at all)
GOLDEN_MD, GOLDEN_COMPONENTS, GOLDEN_LINES_OUT = 5e-3, 3, 80


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
    g, sc = golden["g"], golden["sc"]
    before = g.get3Dlines()
    segs, line = api.flatten_lines(before)
    ext = M.extent(segs)
    md = GOLDEN_MD * ext
    cos2 = M.min_cos2_of(10.0)
    assert M.merge(segs, line, 2e-3 * ext, cos2, 0.5)[4]["n_merged_components"] < 3
    want = M.merge_from_pairs(segs, line, M.pairs(segs, line, md, cos2, 0.5))
    assert want[4]["n_merged_components"] == GOLDEN_COMPONENTS and want[4]["n_lines_out"] == GOLDEN_LINES_OUT
    name_before = g.outputFilename()
    assert "MERGED" not in name_before
    free = api.merge_segments(segs, line, md)
    Cs.same_result(free, want[:5], "stateless / model")
    summary = g.mergeLines(md)
    assert summary is not None
    Cs.same_summary(summary, want[4], "context / model")
    after = g.get3Dlines()
    a_segs, a_line = api.flatten_lines(after)
    assert a_segs.tobytes() == free[0].tobytes() and a_line.tobytes() == free[1].tobytes()
    detail = want[5]
    fused = 0
    for k, L in enumerate(after):
        members = detail["member_lines"][k]
        assert np.array_equal(L["residuals"], np.concatenate([before[i]["residuals"] for i in members])), k
        assert L["reference_view"] == before[detail["leader_line"][k]]["reference_view"], k
        if len(members) == 1:                                       # an untouched line keeps every field
            B = before[members[0]]
            assert L["collinear3Dsegments"].tobytes() == B["collinear3Dsegments"].tobytes() and L["cluster_line"].tobytes() == B["cluster_line"].tobytes()
            continue
        fused += 1
        c = L["collinear3Dsegments"]
        e = c["P2"] - c["P1"]
        length = np.sqrt((e * e).sum(1))
        assert (c["valid"] == 1).all() and np.allclose(c["length"], length, rtol=1e-6) and np.allclose(c["dir"], e / length[:, None], atol=1e-12)
        assert np.array_equal(L["cluster_line"]["P1"], c["P1"][0]) and np.array_equal(L["cluster_line"]["P2"], c["P2"][-1])
        assert L["cluster_line"]["valid"] == 1
    assert fused == GOLDEN_COMPONENTS
    # saved files carry the token
    name = g.outputFilename()
    assert name == name_before.replace("vis_", "MERGED_%g__vis_" % md)
    # the stages after reconstruction see the merged model
    n_out = GOLDEN_LINES_OUT
    assert g.save3DLinesAsTXT(str(tmp_path))
    saved = io.read_3d_lines_txt(str(tmp_path / (name + ".txt")))
    assert len(saved) == n_out and sum(len(L["segments"]) for L in saved) == len(a_segs)
    cams = [v.cam for v in sc.views]
    rec = g.projectLines(cams)
    assert rec is not None and sum(len(r) for r in rec) > 0 and max(int(r["line"].max()) for r in rec if len(r)) < n_out
    assoc = g.associateSegments()
    assert assoc is not None and len(assoc[1]) == n_out and len(assoc[2]) == n_out and assoc[1].sum() > 0
    cmp_ = g.compareLines(after, md)
    assert cmp_ is not None and cmp_[2]["n_lines"] == n_out and cmp_[2]["n_segments"] == len(a_segs)
    # a second merge finds less to do and keeps the token; a new reconstruction drops it and brings the lines back
    again = g.mergeLines(md)
    assert again is not None and again["n_lines_in"] == n_out
    assert g.reconstruct3Dlines(3)
    assert g.outputFilename() == name_before and len(g.get3Dlines()) == len(before)


def test_context_kernel_time_at_timing_level_2(golden):
    g = golden["g"]
    L = _lib.load()
    assert g.setTimingLevel(2)
    try:
        assert g.mergeLines(1e-6) is not None                       # (nothing is near enough: the lines stay)
        assert 0 < L.l3d_debug_counter(b"merge_kernel_ns") < 10 ** 9
    finally:
        g.setTimingLevel(1)
        assert g.reconstruct3Dlines(3)


def test_context_errors(golden):
    g = golden["g"]
    L = _lib.load()
    n_lines = len(g.get3Dlines())
    s = np.full(20, FILL, np.uint32)
    S = C.POINTER(_lib.MergeSummary)
    for par, word in ((_lib.MergeParams(1e-3, 0.9, 1.5, 0, 0), "min_overlap"), (_lib.MergeParams(1e-3, 0.9, 0.5, 0, 1), "reserved")):
        assert L.l3d_merge_lines(g.h, C.byref(par), C.cast(_lib.ptr(s), S)) == -1 and word in _lib.last_error()
    assert L.l3d_merge_lines(g.h, None, C.cast(_lib.ptr(s), S)) == -1 and (s == FILL).all()
    assert g.mergeLines(1e-3, max_angle=120.0) is None and g.last_status == -1      # printed, None
    assert g.mergeLines(-1.0) is None and g.last_status == -1
    assert len(g.get3Dlines()) == n_lines and "MERGED" not in g.outputFilename()     # the model is as it was


def test_context_form_before_reconstruct3Dlines_returns_the_state_error():
    from line3dpp_amd.scene import make_scene
    sc = make_scene(4, 60, n_neighbors=2, seed=2)
    g = Line3D()
    g.add_scene(sc)
    assert g.mergeLines(0.1) is None and g.last_status == -7
    assert "no 3D lines" in _lib.last_error()
    assert g.matchBegin()
    assert g.mergeLines(0.1) is None and g.last_status == -7 and "split call" in _lib.last_error()
    g.matchAbort()
    g.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_merge_lines(tmp_path):
    from line3dpp_amd.scene import make_scene
    exe = str(tmp_path / "merge_smoke")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "merge_smoke.cpp"), "-o", exe, "-L" + lib_dir,
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
    assert run_.stdout.count("[L3D++] ERROR: mergeLines") == 2      # the call before the reconstruction, a bad angle
    raw = open(out_path, "rb").read()
    md, min_cos2, min_overlap, n_in, n_out = struct.unpack_from("<3d2I", raw, 0)
    pos = 32
    parts = []
    for n in (n_in, n_out):
        parts.append(np.frombuffer(raw, np.float64, 6 * n, pos).reshape(n, 6)); pos += 48 * n
        parts.append(np.frombuffer(raw, np.uint32, n, pos)); pos += 4 * n
    summary = dict(zip(M.SUMMARY_KEYS, struct.unpack_from("<7Q3d", raw, pos))); pos += 80
    assert pos == len(raw) and n_in > 10
    # (the facade's squared cosine comes from the C library's cos, the model is given that very number)
    assert abs(min_cos2 - M.min_cos2_of(10.0)) < 1e-15
    want = M.merge(parts[0], parts[1], md, min_cos2, min_overlap)
    assert parts[2].tobytes() == want[0].tobytes() and parts[3].tobytes() == want[1].tobytes()
    Cs.same_summary(summary, want[4], "the facade's summary / the model")
    assert summary["n_merged_components"] >= 1 and n_out < n_in      # at 1.5 units a few of the scene's lines join
