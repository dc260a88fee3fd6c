"""The numpy model of DESIGN §17 (tests/associate_model.py) on its own: its scalar and array forms agree bit for bit, the
hand-built threshold cases come out as the contract states them, and the library exports the new entries.  CPU only."""
import ctypes as C
import os
import re

import numpy as np

from line3dpp_amd import _lib
from tests import associate_cases as Cs
from tests import associate_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scalar_and_array_forms_agree_bit_for_bit():
    shapes = [(70, 90), (33, 600), (0, 5), (5, 0), (120, 40)]
    recs, segs = Cs.cameras(shapes, seed=5)
    assigned = ambiguous = 0
    for k, (rec, sg) in enumerate(zip(recs, segs)):
        for par in (Cs.DEFAULTS, dict(max_distance=5.0, min_cos2=M.min_cos2_of(25.0), min_overlap=0.25),
                    dict(max_distance=0.0, min_cos2=1.0, min_overlap=1.0), dict(max_distance=50.0, min_cos2=0.0, min_overlap=0.0)):
            a = M.associate_scalar(rec, sg, **par)
            b = M.associate(rec, sg, chunk=32, **par)
            Cs.same_associations(b, a, f"camera {k}, {par}")
            if par is Cs.DEFAULTS:
                assigned += int((a["record"] >= 0).sum()); ambiguous += int((a["n_accepted"] > 1).sum())
    assert assigned >= 50 and ambiguous >= 3            # the cases exercise the choice, not only the rejection


def test_hand_built_threshold_cases():
    for name, rec, segs, par, expected in Cs.hand_cases():
        for form in (M.associate_scalar, M.associate):
            Cs.check_expected(f"{name} ({form.__name__})", form(rec, segs, **par), rec, expected)


def test_min_cos2_of_the_default_angle():
    assert abs(M.min_cos2_of(10.0) - np.cos(np.pi / 18) ** 2) < 1e-15
    assert M.min_cos2_of(0.0) == 1.0 and M.min_cos2_of(90.0) < 1e-30


def test_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    L = _lib.load()
    for name in ("l3d_associate_segments", "l3d_associate_view_segments"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    assert "typedef struct l3d_association" in hdr and "typedef struct l3d_associate_params" in hdr


def test_association_layout():
    assert _lib.ASSOCIATION_DTYPE.itemsize == 24
    assert _lib.ASSOCIATION_DTYPE == M.ASSOCIATION_DTYPE and _lib.PROJECTED_SEGMENT_DTYPE == M.RECORD_DTYPE
    assert C.sizeof(_lib.AssociateParams) == 24
    assert M.SEGMENT_MASK == _lib.PROJ_SEGMENT_MASK and M.NONE == _lib.EMPTY


def test_argument_checks_need_no_device():
    """the checks come before any device work: they answer on a machine without a GPU as well"""
    L = _lib.load()
    rec, segs = Cs.camera_case(1, 4, 3)
    n_rec = np.array([3], np.uint32); n_seg = np.array([4], np.uint32)
    out = np.full(4 * 6, 0x5A5A5A5A, np.uint32)
    p = _lib.ptr

    def call(par, rec=rec, segs=segs, n_rec=n_rec, n_seg=n_seg):
        rc = L.l3d_associate_segments(0, 1, p(n_rec), p(rec), p(n_seg), p(segs), C.byref(par) if par is not None else None, p(out))
        assert (out == 0x5A5A5A5A).all()
        return rc, _lib.last_error()

    ok = (2.5, 0.9, 0.5)
    for k, name, bad in ((0, "max_distance", (-1.0, float("inf"), float("nan"))), (1, "min_cos2", (-0.1, 1.1, float("nan"))),
                         (2, "min_overlap", (-0.1, 1.1, float("nan")))):
        for v in bad:
            vals = list(ok); vals[k] = v
            rc, msg = call(_lib.AssociateParams(*vals))
            assert rc == -1 and name in msg, (name, v, rc, msg)
    assert call(None)[0] == -1
    good = _lib.AssociateParams(*ok)
    bad_rec = rec.copy(); bad_rec["y2"][2] = np.inf
    rc, msg = call(good, rec=bad_rec)
    assert rc == -1 and "camera 0" in msg and "record 2" in msg
    bad_seg = segs.copy(); bad_seg[1, 3] = np.nan
    rc, msg = call(good, segs=bad_seg)
    assert rc == -1 and "camera 0" in msg and "segment 1" in msg
    rc, msg = call(good, n_rec=np.array([0x80000000], np.uint32))
    assert rc == -9 and "2^31" in msg
    rc = L.l3d_associate_segments(0, 2, p(np.array([0, 0], np.uint32)), None, p(np.array([0xFFFFFFFF, 1], np.uint32)), p(segs), C.byref(good), p(out))
    assert rc == -9 and "2^32" in _lib.last_error() and (out == 0x5A5A5A5A).all()
    for args in ((None, p(rec), p(n_seg), p(segs), p(out)), (p(n_rec), None, p(n_seg), p(segs), p(out)), (p(n_rec), p(rec), None, p(segs), p(out)),
                 (p(n_rec), p(rec), p(n_seg), None, p(out)), (p(n_rec), p(rec), p(n_seg), p(segs), None)):
        rc = L.l3d_associate_segments(0, 1, args[0], args[1], args[2], args[3], C.byref(good), args[4])
        assert rc == -1 and "null" in _lib.last_error()
    # the empty forms: nothing to do, nothing touched, no device needed
    assert L.l3d_associate_segments(0, 0, None, None, None, None, C.byref(good), None) == 0
    assert L.l3d_associate_segments(0, 1, p(n_rec), p(rec), p(np.zeros(1, np.uint32)), None, C.byref(good), None) == 0
    assert (out == 0x5A5A5A5A).all()
