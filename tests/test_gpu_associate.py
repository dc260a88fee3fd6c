"""The 2D segments assigned to the projected 3D lines they observe on the MI355X (k_associate.hip, l3d_associate.hip;
DESIGN §17) against the numpy model of tests/associate_model.py with tolerance 0 on every field: tile and chunk edges,
several cameras in one launch, hand-built ties and thresholds, a case past one grid, the argument checks, the context
form on the golden scene against the stateless chain and the model, and the C++ facade."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from line3dpp_amd.api import Line3D
from tests import associate_cases as Cs
from tests import associate_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The sanity property of the context form: the condition is that of tests/associate_cases.py, which the reference's own
# lines meet at 273 / 275 = 0.9927 and 0 (tests/test_associate_reference.py).  Measured on the MI355X, on the lines of the
# GPU pipeline: 273 / 275 = 0.9927 on their own line, 0 on another.
SANITY_MIN_OWN_SHARE = Cs.SANITY_MIN_OWN_SHARE

ANGLE = 10.0
PAR = Cs.DEFAULTS


def run(recs, segs, par=PAR):
    """the stateless entry with the squared cosine itself, as the model takes it"""
    L = _lib.load()
    n = len(recs)
    n_rec = np.array([len(r) for r in recs] + [0], np.uint32); n_seg = np.array([len(s) for s in segs] + [0], np.uint32)
    rec = np.concatenate(list(recs) + [np.zeros(1, M.RECORD_DTYPE)])
    seg = np.concatenate([np.asarray(s, np.float32).reshape(-1, 4) for s in segs] + [np.zeros((1, 4), np.float32)])
    out = np.full(len(seg) * 6, 0x5A5A5A5A, np.uint32).view(_lib.ASSOCIATION_DTYPE)
    p = _lib.AssociateParams(par["max_distance"], par["min_cos2"], par["min_overlap"])
    rc = L.l3d_associate_segments(0, n, _lib.ptr(n_rec), _lib.ptr(rec), _lib.ptr(n_seg), _lib.ptr(seg), C.byref(p), _lib.ptr(out))
    assert rc == 0, _lib.last_error()
    assert (out[-1:].view(np.uint32) == 0x5A5A5A5A).all()          # nothing written past the last segment
    return api.split_records(out, n_seg[:n])


# ---- tile and chunk edges, one camera ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seg,n_rec", Cs.EDGE_SHAPES)
def test_one_camera_at_the_tile_and_chunk_edges(n_seg, n_rec):
    # (a single segment is laid along a record, so that the case is not an empty one)
    rec, segs = Cs.camera_case(1000 * n_seg + n_rec, n_seg, n_rec, on_record=1.0 if n_seg == 1 else 0.6)
    want = M.associate(rec, segs, **PAR)
    got, = run([rec], [segs])
    Cs.same_associations(got, want, f"({n_seg}, {n_rec})")
    if n_seg and n_rec:
        assert (want["record"] >= 0).sum() >= max(n_seg // 10, 1)
    if n_rec == 0:
        assert (got["record"] == -1).all() and (got["line"] == M.NONE).all() and not got["n_accepted"].any()


def test_wrapper_takes_degrees():
    rec, segs = Cs.camera_case(77, 300, 600)
    want = M.associate(rec, segs, 3.0, M.min_cos2_of(20.0), 0.25)
    got, = api.associate_segments([rec], [segs], 3.0, 20.0, 0.25)
    Cs.same_associations(got, want, "api.associate_segments")
    assert api.associate_segments([], []) == []
    with pytest.raises(ValueError):
        api.associate_segments([rec], [segs], max_angle=91.0)


# ---- several cameras in one launch ------------------------------------------------------------------------------------
def test_cameras_share_a_launch():
    recs, segs = Cs.cameras(Cs.MULTI_SHAPES, seed=9)
    assert [(len(s), len(r)) for r, s in zip(recs, segs)] == Cs.MULTI_SHAPES
    L = _lib.load()
    before = L.l3d_debug_counter(b"associate_launches")
    got = run(recs, segs)
    assert L.l3d_debug_counter(b"associate_launches") == before + 1
    want = M.associate_cameras(recs, segs, **PAR)
    for k in range(len(recs)):
        Cs.same_associations(got[k], want[k], f"camera {k}")
        alone, = run(recs[k:k + 1], segs[k:k + 1])
        Cs.same_associations(alone, got[k], f"camera {k} alone")
    assert sum(int((w["record"] >= 0).sum()) for w in want) > 100


# ---- ties and thresholds ----------------------------------------------------------------------------------------------
def test_hand_built_ties_and_thresholds():
    for name, rec, segs, par, expected in Cs.hand_cases():
        got, = run([rec], [segs], par)
        Cs.check_expected(name, got, rec, expected)
        Cs.same_associations(got, M.associate_scalar(rec, segs, **par), name)


# ---- past one grid ----------------------------------------------------------------------------------------------------
def test_large_camera_beside_a_small_one():
    recs, segs = Cs.large_case()
    assert len(segs[0]) == 20000 and len(recs[0]) == 3000
    want = M.associate_cameras(recs, segs, **PAR)
    assigned = int((want[0]["record"] >= 0).sum()); ambiguous = int((want[0]["n_accepted"] > 1).sum())
    print(f"large case: {assigned} of 20000 segments assigned, {ambiguous} ambiguous")
    assert assigned >= 2000 and ambiguous >= 100
    got = run(recs, segs)
    for k in range(2):
        Cs.same_associations(got[k], want[k], f"camera {k}")


# ---- argument checks --------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched():
    L = _lib.load()
    rec, segs = Cs.camera_case(1, 40, 30)
    n_rec = np.array([30], np.uint32); n_seg = np.array([40], np.uint32)
    out = np.full(40 * 6, 0x5A5A5A5A, np.uint32)
    p = _lib.ptr

    def call(par, rec=rec, segs=segs, n_rec=n_rec, n_seg=n_seg, out_ok=True):
        rc = L.l3d_associate_segments(0, 1, p(n_rec), p(rec), p(n_seg), p(segs), C.byref(par), p(out) if out_ok else None)
        assert (out == 0x5A5A5A5A).all()
        return rc, _lib.last_error()

    good = (PAR["max_distance"], PAR["min_cos2"], PAR["min_overlap"])
    for k, name, bad in ((0, "max_distance", (-1.0, float("inf"), float("nan"))), (1, "min_cos2", (-0.1, 1.1, float("nan"))),
                         (2, "min_overlap", (-0.1, 1.1, float("nan")))):
        for v in bad:
            vals = list(good); vals[k] = v
            rc, msg = call(_lib.AssociateParams(*vals))
            assert rc == -1 and name in msg
    par = _lib.AssociateParams(*good)
    bad_rec = rec.copy(); bad_rec["x1"][7] = np.nan
    rc, msg = call(par, rec=bad_rec)
    assert rc == -1 and "camera 0" in msg and "record 7" in msg
    bad_seg = segs.copy(); bad_seg[39, 0] = -np.inf
    rc, msg = call(par, segs=bad_seg)
    assert rc == -1 and "camera 0" in msg and "segment 39" in msg
    assert call(par, out_ok=False)[0] == -1
    rc, msg = call(par, n_rec=np.array([0x80000000], np.uint32))
    assert rc == -9 and "2^31" in msg
    rc = L.l3d_associate_segments(0, 2, p(np.array([0, 0], np.uint32)), None, p(np.array([0xFFFFFFFF, 1], np.uint32)), p(segs), C.byref(par), p(out))
    assert rc == -9 and "2^32" in _lib.last_error() and (out == 0x5A5A5A5A).all()
    # the empty forms
    assert L.l3d_associate_segments(0, 0, None, None, None, None, C.byref(par), None) == 0
    assert L.l3d_associate_segments(0, 1, p(n_rec), p(rec), p(np.zeros(1, np.uint32)), None, C.byref(par), None) == 0
    assert (out == 0x5A5A5A5A).all()
    got, = run([rec[:0]], [segs])                               # no records: every segment gets nothing
    Cs.same_associations(got, M.nothing(40), "no records")


# ---- the context form on the golden scene -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    from tests.golden.make_golden import golden_scene
    sc = golden_scene()
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages() and g.reconstruct3Dlines(3)
    lines = g.get3Dlines()
    cam_ids = [v.cam for v in sc.views]
    res = g.associateSegments()
    assert res is not None
    yield dict(sc=sc, g=g, lines=lines, cam_ids=cam_ids, assoc=res[0], sup_s=res[1], sup_v=res[2])
    g.close()


def test_context_equals_the_stateless_chain_and_the_model(golden):
    G = golden
    g, sc = G["g"], G["sc"]
    assert sorted(G["assoc"]) == sorted(G["cam_ids"])
    cams = [g.viewCamera(c) for c in G["cam_ids"]]
    P1 = np.concatenate([L["collinear3Dsegments"]["P1"] for L in G["lines"]])
    P2 = np.concatenate([L["collinear3Dsegments"]["P2"] for L in G["lines"]])
    line = np.concatenate([[i] * len(L["collinear3Dsegments"]) for i, L in enumerate(G["lines"])]).astype(np.uint32)
    rec = api.project_segments(cams, P1, P2, line)
    segs = [np.array([g.getSegmentCoords2D(v.cam, s) for s in range(len(v.segs))], np.float32).reshape(-1, 4) for v in sc.views]
    for v, s in zip(sc.views, segs):
        assert np.array_equal(s, np.asarray(v.segs, np.float32).reshape(-1, 4))
    chain = api.associate_segments(rec, segs)
    model = M.associate_cameras(rec, segs, PAR["max_distance"], M.min_cos2_of(ANGLE), PAR["min_overlap"])
    for k, cam in enumerate(G["cam_ids"]):
        assert len(G["assoc"][cam]) == len(segs[k])
        Cs.same_associations(G["assoc"][cam], chain[k], f"view {cam}: context / stateless chain")
        Cs.same_associations(G["assoc"][cam], model[k], f"view {cam}: context / model")
    assert sum(int((a["record"] >= 0).sum()) for a in G["assoc"].values()) > 200


def test_context_small_budget_and_subsets(golden):
    G = golden
    g, ids = G["g"], G["cam_ids"]
    n_seg = max(len(a) for a in G["assoc"].values())
    g.set_projection_budget(40 * n_seg + 64)                     # one camera per group at most
    L = _lib.load()
    try:
        before = L.l3d_debug_counter(b"associate_launches")
        small = g.associateSegments()
        launches = L.l3d_debug_counter(b"associate_launches") - before
    finally:
        g.set_projection_budget(0)
    assert launches == len(ids)
    for cam in ids:
        Cs.same_associations(small[0][cam], G["assoc"][cam], f"view {cam}: small budget")
    assert np.array_equal(small[1], G["sup_s"]) and np.array_equal(small[2], G["sup_v"])
    pick = [ids[7], ids[4], ids[1]]                              # a subset, in reversed order
    sub, sup_s, sup_v = g.associateSegments(pick)
    assert sorted(sub) == sorted(pick)
    for cam in pick:
        Cs.same_associations(sub[cam], G["assoc"][cam], f"view {cam}: in a subset")
    assert sup_s.sum() == sum(int((sub[c]["record"] >= 0).sum()) for c in pick) and sup_v.max() <= 3


def test_context_support_counts(golden):
    G = golden
    n = len(G["lines"])
    assert len(G["sup_s"]) == n and len(G["sup_v"]) == n
    hit = [a["line"][a["record"] >= 0] for a in G["assoc"].values()]
    assert np.array_equal(G["sup_s"], np.bincount(np.concatenate(hit), minlength=n).astype(np.uint32))
    views = np.zeros(n, np.uint32)
    for h in hit:
        views[np.unique(h)] += 1
    assert np.array_equal(G["sup_v"], views)
    assert (G["sup_v"] <= G["sup_s"]).all() and G["sup_v"].max() >= 3


def test_context_sanity_of_the_residuals(golden):
    G = golden
    pairs, own, other, none, where = Cs.residual_ownership(G["lines"], G["assoc"])
    in_cluster = {(int(r["cam"]), int(r["seg"])) for L in G["lines"] for r in L["residuals"]}
    new = sum(int(a["record"][s] >= 0) for cam, a in G["assoc"].items() for s in range(len(a)) if (cam, s) not in in_cluster)
    print(f"{len(G['lines'])} lines, {pairs} (line, residual) pairs: {own} on their own line ({own / pairs:.4f}), {other} on another "
          f"{where}, {none} on none; {new} segments in no cluster are assigned "
          f"(CPU, reference's lines: {Cs.REFERENCE_OWN} / {Cs.REFERENCE_PAIRS}, {Cs.REFERENCE_OTHER})")
    assert own / pairs >= SANITY_MIN_OWN_SHARE
    assert other == 0


def test_context_errors(golden):
    G = golden
    g = G["g"]
    L = _lib.load()
    par = _lib.AssociateParams(PAR["max_distance"], PAR["min_cos2"], PAR["min_overlap"])
    ids = np.array(G["cam_ids"][:2], np.uint32)
    n_seg = sum(len(G["assoc"][int(c)]) for c in ids)
    off = np.full(3, 77, np.uint64); out = np.full(n_seg * 6, 0x5A5A5A5A, np.uint32)
    sup = np.full(len(G["lines"]), 77, np.uint32)
    p = _lib.ptr

    def call(ids=ids, par=par, near=1e-6, off_ok=True):
        rc = L.l3d_associate_view_segments(g.h, len(ids), p(ids), C.byref(par) if par is not None else None, near,
                                           p(off) if off_ok else None, p(out), p(sup), p(sup))
        assert (off == 77).all() and (out == 0x5A5A5A5A).all() and (sup == 77).all()
        return rc, _lib.last_error()

    rc, msg = call(ids=np.array([ids[0], 12345], np.uint32))
    assert rc == -1 and "unknown camera ID" in msg
    rc, msg = call(ids=np.array([ids[0], ids[0]], np.uint32))
    assert rc == -1 and "twice" in msg
    assert call(par=None)[0] == -1 and call(off_ok=False)[0] == -1
    rc, msg = call(par=_lib.AssociateParams(-1.0, 0.5, 0.5))
    assert rc == -1 and "max_distance" in msg
    rc, msg = call(near=0.0)
    assert rc == -1 and "near plane" in msg
    assert g.associateSegments([12345]) is None and g.last_status == -1         # printed, None
    assert g.associateSegments(max_angle=120.0) is None and g.last_status == -1
    none = g.associateSegments([])
    assert none[0] == {} and not none[1].any() and not none[2].any()


def test_context_form_before_reconstruct3Dlines_returns_the_state_error():
    from line3dpp_amd.scene import make_scene
    sc = make_scene(4, 60, n_neighbors=2, seed=2)
    g = Line3D()
    g.add_scene(sc)
    assert g.associateSegments() is None and g.last_status == -7
    assert "no 3D lines" in _lib.last_error()
    assert g.matchBegin()
    assert g.associateSegments() is None and g.last_status == -7
    assert "split call" in _lib.last_error()
    g.matchAbort()
    g.close()


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
def test_facade_associate_segments(tmp_path):
    from line3dpp_amd.scene import make_scene
    exe = str(tmp_path / "associate_smoke")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "associate_smoke.cpp"), "-o", exe, "-L" + lib_dir,
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
    assert run_.stdout.count("[L3D++] ERROR:") == 2 and "no 3D lines" in run_.stdout     # the call before the reconstruction, a bad angle
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages() and g.reconstruct3Dlines(3)
    cam_ids = [v.cam for v in sc.views]
    rec = dict(zip(cam_ids, g.projectLines(cam_ids)))
    segs = {v.cam: v.segs for v in sc.views}
    raw = open(out_path, "rb").read()
    nv, min_cos2 = struct.unpack_from("<Id", raw, 0)
    assert nv == sc.n_views and abs(min_cos2 - M.min_cos2_of(ANGLE)) < 1e-15
    pos = 12
    total = 0
    for _ in range(nv):
        cam, n = struct.unpack_from("<2I", raw, pos)
        pos += 8
        got = np.frombuffer(raw, _lib.ASSOCIATION_DTYPE, n, pos)
        pos += 24 * n
        # (the facade's squared cosine comes from the C library's cos, the model is given that very number)
        Cs.same_associations(got, M.associate(rec[cam], segs[cam], PAR["max_distance"], min_cos2, PAR["min_overlap"]),
                             f"view {cam}: the facade's records / the model")
        total += int((got["record"] >= 0).sum())
    assert pos == len(raw) and total > 50
    g.close()
