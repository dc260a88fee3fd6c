"""The numpy model of DESIGN §18 (tests/compare_model.py) on its own: its scalar and array forms agree byte for byte, the
hand-built threshold cases come out as the contract states them, the reference's two published models match each other;
the library exports the new entries and checks their arguments without a device; flatten_lines and the command line.
CPU only."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from line3dpp_amd import _lib, api, compare, io
from tests import compare_cases as Cs
from tests import compare_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_scalar_and_array_forms_agree_byte_for_byte():
    matched = ambiguous = 0
    for k, (n_q, n_r) in enumerate([(70, 90), (33, 300), (0, 5), (5, 0), (120, 40)]):
        q, ql, r, rl = Cs.model_case(11 + k, n_q, n_r)
        for par in Cs.PARAM_SETS:
            for excl in (False, True):
                a = M.compare_scalar(q, ql, r, rl, exclude_same_line=excl, **par)
                b = M.compare(q, ql, r, rl, exclude_same_line=excl, chunk=32, **par)
                Cs.same_matches(b, a, f"case {k}, {par}, exclude_same_line={excl}")
                if par is Cs.DEFAULTS and not excl:
                    matched += int((a["segment"] >= 0).sum()); ambiguous += int((a["n_accepted"] > 1).sum())
    assert matched >= 50 and ambiguous >= 3             # the cases exercise the choice, not only the rejection


def test_hand_built_threshold_cases():
    for name, q, ql, r, rl, par, expected in Cs.hand_cases():
        for form in (M.compare_scalar, M.compare):
            Cs.check_expected(f"{name} ({form.__name__})", form(q, ql, r, rl, **par), expected)
    q, ql, r, rl, expected = Cs.tie_across_slices()
    Cs.check_expected("tie across slices", M.compare(q, ql, r, rl, **Cs.DEFAULTS | dict(max_distance=5.0)), expected)


def test_a_model_against_itself():
    """every live segment gets distance 0, overlap 1, and itself or an identical segment of lower index"""
    _, _, r, rl = Cs.model_case(3, 0, 400)
    r[200] = r[17]                                       # an identical segment further up
    for form in (M.compare_scalar, M.compare):
        m = form(r, rl, r, rl, **Cs.DEFAULTS)
        live = np.flatnonzero((r[:, :3] != r[:, 3:]).any(1))
        assert 0 < len(live) < len(r)
        dead = np.setdiff1d(np.arange(len(r)), live)
        assert (m["segment"][dead] == -1).all() and (m["n_accepted"][dead] == 0).all()
        assert (m["distance"][live] == 0.0).all() and (m["overlap"][live] == 1.0).all()
        own = m["segment"][live] == live
        assert own.sum() == len(live) - 1 and m["segment"][200] == 17
        for i in live[~own]:
            assert m["segment"][i] < i and np.array_equal(r[m["segment"][i]], r[i])


def test_summary_adds_in_index_order():
    q, ql, r, rl = Cs.model_case(5, 300, 200)
    mq, mr, sq, sr = M.compare_both(q, ql, r, rl, **Cs.DEFAULTS)
    total = got = 0.0
    for i in range(len(q)):
        e = q[i, 3:] - q[i, :3]
        ln = float(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]))
        total += ln
        if mq["segment"][i] >= 0:
            got += ln
    assert sq["length_total"] == total and sq["length_matched"] == got
    assert sq["n_segments"] == 300 and 0 < sq["n_matched"] < 300 and sq["n_lines_matched"] <= sq["n_lines"]
    assert M.compare_both(q, ql, r[:0], rl[:0], **Cs.DEFAULTS)[2]["n_segments"] == 0      # an empty side: zero summaries


def test_min_cos2_of_the_default_angle():
    assert abs(M.min_cos2_of(10.0) - np.cos(np.pi / 18) ** 2) < 1e-15
    assert M.min_cos2_of(0.0) == 1.0 and M.min_cos2_of(90.0) < 1e-30
    p = api.compare_params(0.25, 10.0, 0.5, True, 3)
    assert (p.max_distance, p.min_cos2, p.min_overlap, p.exclude_same_line, p.slice_chunks) == (0.25, M.min_cos2_of(10.0), 0.5, 1, 3)
    for bad in (-1.0, 90.5, float("nan")):
        with pytest.raises(ValueError, match="max_angle"):
            api.compare_params(1.0, bad)


# ---- the reference's two published models of its testdata (tests/golden/make_ref_models.py) ---------------------------
def test_reference_models_match_each_other():
    """sanity on real data: the optimised and the plain result of one reconstruction are the same lines, and a quarter
    of the segments has a near-duplicate on another line"""
    d = np.load(os.path.join(GOLDEN, "ref_c0_models.npz"))
    a, al, b, bl = d["optimized_segs"], d["optimized_line"], d["plain_segs"], d["plain_line"]
    assert a.shape == (2503, 6) and b.shape == (2501, 6) and len(np.unique(al)) == 2490 and len(np.unique(bl)) == 2489
    ext = M.extent(a)
    assert 4.2 < ext < 4.3
    mq, mr, sq, sr = M.compare_both(a, al, b, bl, 0.002 * ext, M.min_cos2_of(10.0), 0.5)
    print("optimised in plain:", sq, "\nplain in optimised:", sr)
    assert sq["n_matched"] >= 0.99 * sq["n_segments"] and sr["n_matched"] >= 0.99 * sr["n_segments"]
    dup = M.compare(a, al, a, al, 0.001 * ext, M.min_cos2_of(10.0), 0.5, exclude_same_line=True)
    hit = dup["segment"] >= 0
    print("segments with a counterpart on another line:", int(hit.sum()), "on", len(np.unique(al[hit])), "lines")
    assert 500 <= hit.sum() < len(a)
    assert (dup["line"][hit] != al[hit]).all()


# ---- the library's side, as far as it goes without a device -----------------------------------------------------------
def test_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    L = _lib.load()
    for name in ("l3d_compare_segments", "l3d_compare_lines"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    for name in ("l3d_compare_params", "l3d_line_match", "l3d_compare_summary"):
        assert "typedef struct " + name in hdr
    for name in ("compare_launches", "compare_merge_launches", "compare_slices", "compare_kernel_ns"):
        assert L.l3d_debug_counter(name.encode()) != L.l3d_debug_counter(b"no such counter")


def test_struct_layouts():
    assert _lib.LINE_MATCH_DTYPE.itemsize == 24 and _lib.LINE_MATCH_DTYPE == M.LINE_MATCH_DTYPE
    assert C.sizeof(_lib.CompareParams) == 32 and C.sizeof(_lib.CompareSummary) == 56
    assert tuple(f for f, _ in _lib.CompareSummary._fields_) == M.SUMMARY_KEYS
    assert M.NONE == _lib.EMPTY


FILL = 0x5A5A5A5A


def test_argument_checks_need_no_device():
    """the checks come before any device work: they answer on a machine without a GPU as well"""
    L = _lib.load()
    q, ql, r, rl = Cs.model_case(1, 4, 3)
    out_q = np.full(4 * 6, FILL, np.uint32); out_r = np.full(3 * 6, FILL, np.uint32)
    s_q = np.full(14, FILL, np.uint32); s_r = np.full(14, FILL, np.uint32)
    p = _lib.ptr
    S = C.POINTER(_lib.CompareSummary)

    def untouched():
        return all((x == FILL).all() for x in (out_q, out_r, s_q, s_r))

    def call(par, q=q, ql=ql, r=r, rl=rl, n_q=4, n_r=3, null=()):
        a = dict(q=p(q), ql=p(ql), r=p(r), rl=p(rl))
        for k in null:
            a[k] = None
        rc = L.l3d_compare_segments(0, n_q, a["q"], a["ql"], n_r, a["r"], a["rl"], C.byref(par) if par is not None else None,
                                    p(out_q), p(out_r), C.cast(p(s_q), S), C.cast(p(s_r), S))
        assert untouched()
        return rc, _lib.last_error()

    ok = (0.5, 0.9, 0.5, 0, 0)
    for k, name, bad in ((0, "max_distance", (-1.0, float("inf"), float("nan"))), (1, "min_cos2", (-0.1, 1.1, float("nan"))),
                         (2, "min_overlap", (-0.1, 1.1, float("nan"))), (3, "exclude_same_line", (2, 0xFFFFFFFF))):
        for v in bad:
            vals = list(ok); vals[k] = v
            rc, msg = call(_lib.CompareParams(*vals))
            assert rc == -1 and name in msg, (name, v, rc, msg)
    rc, msg = call(None)
    assert rc == -1 and "null" in msg
    good = _lib.CompareParams(*ok)
    for bad_value in (np.inf, -np.inf, np.nan, 2.0 ** 101, -(2.0 ** 101)):
        bad_q = q.copy(); bad_q[2, 4] = bad_value
        rc, msg = call(good, q=bad_q)
        assert rc == -1 and "query" in msg and "segment 2" in msg, msg
        bad_r = r.copy(); bad_r[1, 0] = bad_value
        rc, msg = call(good, r=bad_r)
        assert rc == -1 and "reference" in msg and "segment 1" in msg, msg
    for side, kw in (("query", dict(n_q=1 << 30)), ("reference", dict(n_r=1 << 30)), ("query", dict(n_q=0xFFFFFFFF))):
        rc, msg = call(good, **kw)
        assert rc == -9 and "2^30" in msg and side in msg, msg
    for k in ("q", "ql", "r", "rl"):
        rc, msg = call(good, null=(k,))
        assert rc == -1 and "null" in msg
    # the context form checks its arguments first as well
    assert L.l3d_compare_lines(None, 3, p(r), p(rl), C.byref(good), p(out_q), p(out_r), None, None) == -1 and "null" in _lib.last_error()
    assert untouched()


def test_empty_forms_need_no_device():
    L = _lib.load()
    q, ql, r, rl = Cs.model_case(1, 4, 3)
    good = _lib.CompareParams(0.5, 0.9, 0.5, 0, 0)
    p = _lib.ptr
    for n_q, n_r in ((4, 0), (0, 3), (0, 0)):
        out_q = np.full(4 * 24, FILL & 0xFF, np.uint8).view(M.LINE_MATCH_DTYPE)
        out_r = out_q[:3].copy()
        s_q = _lib.CompareSummary(n_segments=7, length_total=1.0); s_r = _lib.CompareSummary(n_segments=7, length_total=1.0)
        rc = L.l3d_compare_segments(0, n_q, p(q) if n_q else None, p(ql) if n_q else None, n_r, p(r) if n_r else None,
                                    p(rl) if n_r else None, C.byref(good), p(out_q), p(out_r), C.byref(s_q), C.byref(s_r))
        assert rc == 0, _lib.last_error()
        assert out_q[:n_q].tobytes() == M.nothing(n_q).tobytes() and out_r[:n_r].tobytes() == M.nothing(n_r).tobytes()
        assert (out_q[n_q:].view(np.uint8) == FILL & 0xFF).all() and (out_r[n_r:].view(np.uint8) == FILL & 0xFF).all()
        for s in (s_q, s_r):
            assert all(getattr(s, f) == 0 for f in M.SUMMARY_KEYS)
    # both outputs left out: nothing to do, whatever the sizes
    assert L.l3d_compare_segments(0, 4, p(q), p(ql), 3, p(r), p(rl), C.byref(good), None, None, None, None) == 0
    mq, mr, sq, sr = api.compare_segments(q, ql, np.zeros((0, 6)), np.zeros(0, np.uint32), 0.5)
    assert len(mq) == 4 and len(mr) == 0 and (mq["segment"] == -1).all() and sq["n_segments"] == 0 and sr["n_matched"] == 0


# ---- flatten_lines ----------------------------------------------------------------------------------------------------
def test_flatten_lines_on_both_list_forms():
    txt = io.read_3d_lines_txt(os.path.join(GOLDEN, "ref_lines3d_excerpt.txt"))
    segs, line = api.flatten_lines(txt)
    n = sum(len(L["segments"]) for L in txt)
    assert segs.shape == (n, 6) and segs.dtype == np.float64 and segs.flags.c_contiguous and line.dtype == np.uint32 and n >= len(txt) > 3
    at = 0
    for i, L in enumerate(txt):
        k = len(L["segments"])
        assert np.array_equal(segs[at:at + k], L["segments"]) and (line[at:at + k] == i).all()
        at += k
    binary = io.read_3d_lines_bin(os.path.join(GOLDEN, "ref_lines3d_excerpt.bin"))[0]
    bs, bl = api.flatten_lines(binary)                   # [n, 9]: P1, P2, dir
    assert bs.shape[1] == 6 and len(bs) == sum(len(L["segments"]) for L in binary)
    assert np.array_equal(bs, np.concatenate([np.asarray(L["segments"])[:, :6] for L in binary]))
    # the dicts of Line3D.get3Dlines: structured segments with P1, P2
    got = []
    for L in txt:
        sg = np.zeros(len(L["segments"]), _lib.SEGMENT3D_DTYPE)
        sg["P1"] = L["segments"][:, :3]; sg["P2"] = L["segments"][:, 3:]
        got.append(dict(collinear3Dsegments=sg, residuals=None))
    gs, gl = api.flatten_lines(got)
    assert np.array_equal(gs, segs) and np.array_equal(gl, line)
    es, el = api.flatten_lines([])
    assert es.shape == (0, 6) and el.shape == (0,)
    es, el = api.flatten_lines([dict(segments=np.zeros((0, 6))), dict(segments=np.ones((2, 6)))])
    assert es.shape == (2, 6) and list(el) == [1, 1]


# ---- the command line, with the model in the library's place -----------------------------------------------------------
def model_compare_segments(q_segs, q_line, r_segs, r_line, max_distance, max_angle=10.0, min_overlap=0.5, exclude_same_line=False,
                           slice_chunks=0, device=0):
    return M.compare_both(q_segs, q_line, r_segs, r_line, max_distance, M.min_cos2_of(max_angle), min_overlap, exclude_same_line)


def test_command_line(tmp_path, capsys):
    a = os.path.join(GOLDEN, "ref_lines3d_excerpt.txt"); b = os.path.join(GOLDEN, "ref_lines3d_excerpt.bin")
    assert compare.main([a, b, "-d", "0.01"], compare_segments=model_compare_segments) == 0
    res = json.loads(capsys.readouterr().out)
    segs, line = compare.read_model(a)
    bsegs, bline = compare.read_model(b)
    mq, mr, sq, sr = M.compare_both(segs, line, bsegs, bline, 0.01, M.min_cos2_of(10.0), 0.5)
    assert res["max_distance"] == 0.01 and res["max_angle"] == 10.0 and res["min_overlap"] == 0.5
    for key, s, m in (("a_in_b", sq, mq), ("b_in_a", sr, mr)):
        for k in M.SUMMARY_KEYS:
            assert res[key][k] == s[k]
        d = m["distance"][m["segment"] >= 0]
        assert res[key]["n_matched"] > 0 and res[key]["distance_median"] == float(np.median(d)) and res[key]["distance_p90"] == float(np.percentile(d, 90))
    seen = {}

    def spy(*args, **kw):
        seen.update(kw)
        return model_compare_segments(*args, **kw)
    assert compare.main([a, "--duplicates", "-d", "0.5", "-a", "20", "-o", "0.25"], compare_segments=spy) == 0
    res = json.loads(capsys.readouterr().out)
    assert seen["exclude_same_line"] is True and seen["max_angle"] == 20.0 and seen["min_overlap"] == 0.25 and seen["max_distance"] == 0.5
    dup = M.compare(segs, line, segs, line, 0.5, M.min_cos2_of(20.0), 0.25, exclude_same_line=True)
    hit = dup["segment"] >= 0
    assert res["n_segments"] == len(segs) and res["n_lines"] == len(np.unique(line))
    assert res["n_duplicate_segments"] == int(hit.sum()) and res["n_duplicate_lines"] == len(np.unique(line[hit]))
    # -d is required; the number of files; the extension; a missing file; an angle outside [0, 90]
    for argv in ([a, b], [a, "-d", "1"], [a, b, "--duplicates", "-d", "1"]):
        with pytest.raises(SystemExit):
            compare.main(argv, compare_segments=model_compare_segments)
        assert "usage" in capsys.readouterr().err
    assert compare.main([a, str(tmp_path / "model.obj"), "-d", "1"], compare_segments=model_compare_segments) == 1
    assert ".txt or .bin" in capsys.readouterr().err
    assert compare.main([a, str(tmp_path / "none.txt"), "-d", "1"], compare_segments=model_compare_segments) == 1
    assert "no such file" in capsys.readouterr().err
    assert compare.main([a, b, "-d", "1", "-a", "120"], compare_segments=lambda *x, **k: api.compare_params(k["max_distance"], k["max_angle"])) == 1
    assert "max_angle" in capsys.readouterr().err
