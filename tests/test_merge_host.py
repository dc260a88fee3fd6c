"""The numpy model of DESIGN §19 (tests/merge_model.py) on its own: the scalar and array forms of stage 1 agree, the
hand-built cases come out as the contract states them, and on the reference's published model the merge removes the
near-duplicate lines within the stated bounds; the library exports the new entries and checks their arguments without a
device; the command line.  CPU only."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from line3dpp_amd import _lib, api, io, merge
from tests import compare_model as CM
from tests import merge_cases as Cs
from tests import merge_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_scalar_and_array_forms_of_stage_1_are_identical():
    accepted = 0
    for k, n in enumerate([90, 150, 0, 1, 64]):
        segs, line = Cs.model_case(21 + k, n, box=4.0, chains=0.05)
        for par in Cs.PARAM_SETS:
            a = M.pairs_scalar(segs, line, **par)
            b = M.pairs(segs, line, chunk=32, **par)
            assert a.dtype == b.dtype == np.uint32 and a.shape == b.shape and a.tobytes() == b.tobytes(), (k, par)
            if len(a):
                key = a[:, 0].astype(np.uint64) << np.uint64(32) | a[:, 1]
                assert (np.diff(key.astype(np.int64)) > 0).all()            # ascending (q, r), no pair twice
                assert (line[a[:, 0]] != line[a[:, 1]]).all()
            if par is Cs.DEFAULTS:
                accepted += len(a)
    assert accepted >= 40                                   # the cases exercise the acceptance, not only the rejection


def test_hand_built_cases():
    for name, segs, line, expected in Cs.hand_cases():
        for form in (M.pairs_scalar, M.pairs):
            Cs.check_expected(f"{name} ({form.__name__})", M.merge(segs, line, form=form, **Cs.HAND_PAR), expected)


def test_the_chain_joins_lines_that_are_not_near_each_other():
    name, segs, line, _ = Cs.hand_cases()[0]
    p = M.pairs(segs, line, **Cs.HAND_PAR)
    assert [tuple(x) for x in p] == [(0, 1), (1, 0), (1, 2), (2, 1)]        # never (0, 2) or (2, 0)
    # offset pieces of a staircase: each step is within reach of the next one only; max_offset shows how far it went
    stairs = Cs.segs([(4 * k, 3 * k, 0, 4 * k + 10, 3 * k, 0) for k in range(4)])
    got = M.merge(stairs, np.arange(4, dtype=np.uint32), **Cs.HAND_PAR)
    assert got[4]["n_lines_out"] == 1 and got[4]["largest_component"] == 4 and len(M.pairs(stairs, np.arange(4), **Cs.HAND_PAR)) == 6
    assert got[4]["max_offset"] > 2.9 and got[3]["max_offset"][0] == got[4]["max_offset"]


def test_summary_adds_in_index_order_and_numbers_by_label():
    segs, line = Cs.model_case(5, 300, box=5.0, chains=0.05)
    so, lo, lm, info, s = M.merge(segs, line, **Cs.DEFAULTS)
    total = 0.0
    for v in segs:
        e = v[3:] - v[:3]
        total += float(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]))
    assert s["length_in"] == total and s["n_segments_in"] == 300 and s["n_lines_in"] == len(np.unique(line))
    assert s["n_merged_components"] >= 10 and s["n_lines_out"] < s["n_lines_in"] and s["n_segments_out"] <= 300
    assert (np.diff(info["label"].astype(np.int64)) > 0).all() and info["n_members"].sum() == s["n_lines_in"]
    assert (np.diff(lo.astype(np.int64)) >= 0).all() and len(np.unique(lo)) == s["n_lines_out"]
    for k in np.flatnonzero(info["n_members"] == 1):       # an untouched line keeps its segments, in input order
        assert np.array_equal(so[lo == k], segs[line == info["label"][k]])
    assert (info["label"][lm] <= line).all()                # a segment's output line carries the smallest index of its component


# ---- the reference's published model of its testdata ------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_model():
    d = np.load(os.path.join(GOLDEN, "ref_c0_models.npz"))
    segs, line = d["optimized_segs"], d["optimized_line"]
    md = 0.001 * M.extent(segs)
    return segs, line, md, M.merge(segs, line, md, M.min_cos2_of(10.0), 0.5)


def test_reference_model_loses_its_near_duplicates(reference_model):
    """the counts the contract-order model gives are recorded in DESIGN §19; the asserts are the issue's bounds"""
    segs, line, md, (so, lo, lm, info, s) = reference_model
    cos2 = M.min_cos2_of(10.0)
    hist = {int(k): int(v) for k, v in zip(*np.unique(info["n_members"], return_counts=True))}
    before = int((CM.compare(segs, line, segs, line, md, cos2, 0.5, exclude_same_line=True)["segment"] >= 0).sum())
    after = int((CM.compare(so, lo, so, lo, md, cos2, 0.5, exclude_same_line=True)["segment"] >= 0).sum())
    found = CM.compare(segs, line, so, lo, 2 * md, cos2, 0.5)
    print("summary:", s, "\ncomponents by lines:", hist, "\nsegments with a counterpart before / after:", before, after,
          "\noriginals re-found:", int((found["segment"] >= 0).sum()), "of", len(segs))
    assert s["n_lines_in"] == 2490 and s["n_segments_in"] == 2503
    assert s["n_lines_out"] <= 0.9 * s["n_lines_in"]
    assert after <= 0.1 * before
    assert (found["segment"] >= 0).all()


# ---- the library's side, as far as it goes without a device -----------------------------------------------------------
def test_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    L = _lib.load()
    for name in ("l3d_merge_segments", "l3d_merge_lines"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    for name in ("l3d_merge_params", "l3d_merge_line_info", "l3d_merge_summary"):
        assert "typedef struct " + name in hdr
    for name in ("merge_count_launches", "merge_write_launches", "merge_slices", "merge_pairs", "merge_kernel_ns"):
        assert L.l3d_debug_counter(name.encode()) != L.l3d_debug_counter(b"no such counter")
    facade = open(os.path.join(ROOT, "include", "line3dpp", "line3D.h")).read()
    assert re.search(r"\bmergeLines\s*\(", facade)


def test_struct_layouts():
    assert C.sizeof(_lib.MergeParams) == 32 and C.sizeof(_lib.MergeSummary) == 80
    assert _lib.MERGE_LINE_INFO_DTYPE.itemsize == 16 and _lib.MERGE_LINE_INFO_DTYPE == M.LINE_INFO_DTYPE
    assert tuple(f for f, _ in _lib.MergeSummary._fields_) == M.SUMMARY_KEYS
    assert [f for f, _ in _lib.MergeParams._fields_] == ["max_distance", "min_cos2", "min_overlap", "slice_chunks", "reserved"]


def test_merge_params_follow_compare_params():
    p = api.merge_params(0.25, 10.0, 0.5, 3)
    assert (p.max_distance, p.min_cos2, p.min_overlap, p.slice_chunks, p.reserved) == (0.25, M.min_cos2_of(10.0), 0.5, 3, 0)
    assert api.merge_params(1.0).min_cos2 == api.compare_params(1.0).min_cos2 and api.merge_params(1.0).min_overlap == 0.5
    for bad in (-1.0, 90.5, float("nan")):
        with pytest.raises(ValueError, match="max_angle"):
            api.merge_params(1.0, bad)


FILL = 0x5A5A5A5A


class Call:
    """l3d_merge_segments on buffers filled with a pattern, which every refused call must leave as it was"""

    def __init__(self, n=4, seed=1):
        self.L = _lib.load()
        self.segs, self.line = Cs.model_case(seed, n)
        self.n = n
        self.out = dict(out_line_map=np.full(n, FILL, np.uint32), out_segs=np.full(12 * n, FILL, np.uint32),
                        out_seg_line=np.full(n, FILL, np.uint32), out_info=np.full(4 * n, FILL, np.uint32),
                        n_segs=np.full(1, FILL, np.uint32), n_lines=np.full(1, FILL, np.uint32), summary=np.full(20, FILL, np.uint32))

    def __call__(self, par, segs=None, line=None, n=None, seg_cap=None, line_cap=None, null=()):
        p = _lib.ptr
        a = dict(segs=p(self.segs if segs is None else segs), line=p(self.line if line is None else line))
        a.update({k: p(v) for k, v in self.out.items()})
        for k in null:
            a[k] = None
        U = C.POINTER(C.c_uint32)
        rc = self.L.l3d_merge_segments(0, self.n if n is None else n, a["segs"], a["line"], C.byref(par) if par is not None else None,
                                       a["out_line_map"], self.n if seg_cap is None else seg_cap, a["out_segs"], a["out_seg_line"],
                                       C.cast(a["n_segs"], U), self.n if line_cap is None else line_cap, a["out_info"],
                                       C.cast(a["n_lines"], U), C.cast(a["summary"], C.POINTER(_lib.MergeSummary)))
        assert all((x == FILL).all() for x in self.out.values())
        return rc, _lib.last_error()


def test_argument_checks_need_no_device():
    """the checks come before any device work: they answer on a machine without a GPU as well"""
    call = Call()
    ok = (0.5, 0.9, 0.5, 0, 0)
    for k, name, bad in ((0, "max_distance", (-1.0, float("inf"), float("nan"))), (1, "min_cos2", (-0.1, 1.1, float("nan"))),
                         (2, "min_overlap", (-0.1, 1.1, float("nan"))), (4, "reserved", (1, 0xFFFFFFFF))):
        for v in bad:
            vals = list(ok); vals[k] = v
            rc, msg = call(_lib.MergeParams(*vals))
            assert rc == -1 and name in msg, (name, v, rc, msg)
    rc, msg = call(None)
    assert rc == -1 and "null" in msg
    good = _lib.MergeParams(*ok)
    for bad_value in (np.inf, -np.inf, np.nan, 2.0 ** 101, -(2.0 ** 101)):
        bad = call.segs.copy(); bad[2, 4] = bad_value
        rc, msg = call(good, segs=bad)
        assert rc == -1 and "segment 2" in msg and "2^100" in msg, msg
    for n in (1 << 30, 0xFFFFFFFF):
        rc, msg = call(good, n=n, seg_cap=n, line_cap=n)
        assert rc == -9 and "2^30" in msg, msg
    for k in ("segs", "line", "out_line_map", "out_segs", "out_seg_line", "out_info", "n_segs", "n_lines"):
        rc, msg = call(good, null=(k,))
        assert rc == -1 and "null" in msg, k
    rc, msg = call(good, seg_cap=3)
    assert rc == -1 and "out_seg_cap" in msg
    rc, msg = call(good, line=np.array([9, 4, 9, 1], np.uint32), line_cap=2)       # three distinct lines
    assert rc == -1 and "out_line_cap" in msg
    rc, msg = call(good, line=np.arange(4, dtype=np.uint32), line_cap=3)
    assert rc == -1 and "out_line_cap" in msg
    # the context form checks its arguments first as well
    assert call.L.l3d_merge_lines(None, C.byref(good), None) == -1 and "null" in _lib.last_error()


def test_empty_model_needs_no_device():
    L = _lib.load()
    good = _lib.MergeParams(0.5, 0.9, 0.5, 0, 0)
    n_segs = C.c_uint32(7); n_lines = C.c_uint32(7)
    s = _lib.MergeSummary(n_segments_in=7, length_in=1.0, max_offset=2.0)
    assert L.l3d_merge_segments(0, 0, None, None, C.byref(good), None, 0, None, None, C.byref(n_segs), 0, None, C.byref(n_lines), C.byref(s)) == 0
    assert n_segs.value == 0 and n_lines.value == 0 and all(getattr(s, f) == 0 for f in M.SUMMARY_KEYS)
    so, lo, lm, info, summary = api.merge_segments(np.zeros((0, 6)), np.zeros(0, np.uint32), 0.5)
    assert so.shape == (0, 6) and len(lo) == len(lm) == len(info) == 0 and summary == M.merge(np.zeros((0, 6)), np.zeros(0, np.uint32), 0.5, 0.9, 0.5)[4]


# ---- the command line, with the model in the library's place ----------------------------------------------------------
def model_merge_segments(segs, line, max_distance, max_angle=10.0, min_overlap=0.5, slice_chunks=0, device=0):
    return M.merge(segs, line, max_distance, M.min_cos2_of(max_angle), min_overlap)


def test_command_line_round_trip_at_distance_zero(tmp_path, capsys):
    src = os.path.join(GOLDEN, "ref_lines3d_excerpt.txt")
    out = str(tmp_path / "same.txt")
    assert merge.main([src, out, "-d", "0"], merge_segments=model_merge_segments) == 0
    res = json.loads(capsys.readouterr().out)
    assert open(out).read() == open(src).read()
    assert res["n_pairs"] == 0 and res["n_lines_out"] == res["n_lines_in"] > 3 and res["n_segments_out"] == res["n_segments_in"]
    assert res["max_distance"] == 0.0 and res["input"] == src and res["output"] == out


def test_command_line(tmp_path, capsys):
    """two copies of the excerpt's lines in one file, the second set moved by a hair: every line finds its copy"""
    lines = io.read_3d_lines_txt(os.path.join(GOLDEN, "ref_lines3d_excerpt.txt"))
    moved = [dict(L, segments=L["segments"] + 1e-5) for L in lines]
    src = str(tmp_path / "twice.txt")
    with open(src, "w") as f:
        f.write(io.format_3d_lines_txt(lines + moved))
    seen = {}

    def spy(*args, **kw):
        seen.update(kw)
        return model_merge_segments(*args, **kw)
    out = str(tmp_path / "merged.txt")
    assert merge.main([src, out, "-d", "0.01", "-a", "20", "-o", "0.25"], merge_segments=spy) == 0
    res = json.loads(capsys.readouterr().out)
    assert seen["max_distance"] == 0.01 and seen["max_angle"] == 20.0 and seen["min_overlap"] == 0.25
    both = io.read_3d_lines_txt(src)
    segs, line = api.flatten_lines(both)
    so, lo, lm, info, s = M.merge(segs, line, 0.01, M.min_cos2_of(20.0), 0.25)
    for k in M.SUMMARY_KEYS:
        assert res[k] == s[k], k
    assert s["n_merged_components"] >= len(lines) // 2 and s["n_lines_out"] < s["n_lines_in"] == 2 * len(lines)
    got = io.read_3d_lines_txt(out)
    assert len(got) == s["n_lines_out"] and sum(len(L["segments"]) for L in got) == s["n_segments_out"]
    # residuals and their 2D coordinates: the members' lists one after another in ascending line index
    for k, L in enumerate(got):
        members = np.unique(line[lm == k])
        assert len(members) == info["n_members"][k]
        assert np.array_equal(L["residuals"], np.concatenate([both[i]["residuals"] for i in members]))
        assert np.array_equal(L["coords2D"], np.concatenate([both[i]["coords2D"] for i in members]))
    assert open(out).read() == io.format_3d_lines_txt(merge.merged_lines(both, so, lo, lm, line, info))
    # a .bin input: no 2D coordinates to carry, zeros in their place
    assert merge.main([os.path.join(GOLDEN, "ref_lines3d_excerpt.bin"), out, "-d", "0"], merge_segments=model_merge_segments) == 0
    capsys.readouterr()
    back = io.read_3d_lines_txt(out)
    binary = io.read_3d_lines_bin(os.path.join(GOLDEN, "ref_lines3d_excerpt.bin"))[0]
    assert len(back) == len(binary) and all(np.array_equal(a["residuals"], b["residuals"]) and not a["coords2D"].any() for a, b in zip(back, binary))
    # -d is required; both files; the extensions; a missing file; an angle outside [0, 90]
    for argv in ([src, out], [src, "-d", "1"]):
        with pytest.raises(SystemExit):
            merge.main(argv, merge_segments=model_merge_segments)
        assert "usage" in capsys.readouterr().err
    assert merge.main([str(tmp_path / "model.obj"), out, "-d", "1"], merge_segments=model_merge_segments) == 1
    assert ".txt or .bin" in capsys.readouterr().err
    assert merge.main([src, str(tmp_path / "model.bin"), "-d", "1"], merge_segments=model_merge_segments) == 1
    assert "written as .txt" in capsys.readouterr().err
    assert merge.main([str(tmp_path / "none.txt"), out, "-d", "1"], merge_segments=model_merge_segments) == 1
    assert "no such file" in capsys.readouterr().err
    assert merge.main([src, out, "-d", "1", "-a", "120"], merge_segments=lambda *x, **k: api.merge_params(k["max_distance"], k["max_angle"])) == 1
    assert "max_angle" in capsys.readouterr().err
