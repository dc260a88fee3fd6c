"""CPU side of the culling cases (tests/cull_cases.py): every case reaches the condition it is named for, the
library's own make_cull (l3d_cull_forms: host only) agrees with the model (tests/cull_model.py) on every pair of every case
and along the epipole sweep, and the soundness claim of tests/test_culling_math.py holds on these geometries: at an overlap
threshold of 1e-6 every match the oracle accepts lies in intersecting model bands, without exception."""
import numpy as np
import pytest

from tests import cull_cases as CC
from tests import cull_model as CM

NAMES = list(CC.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_condition(name):
    info = CC.condition(name)
    print(name, info)
    sc = CC.scene(name)
    assert all(max(v.width, v.height) >= 800 for v in sc.views), "the oracle refuses smaller images"
    assert len(CC.pair_list(sc)) >= 1


def _assert_forms_equal(lib, mod, where):
    assert (lib is None) == (mod is None), where
    if mod is not None:
        for a, b, k in zip(lib, mod, ("As", "Bs", "At", "Bt")):
            # (the same formulas in another order of evaluation: norms, the cross products' signs)
            assert np.allclose(a, b, rtol=1e-11, atol=1e-11 * np.abs(b).max()), (where, k, a, b)


@pytest.mark.parametrize("name", NAMES)
def test_library_forms_match_the_model(name):
    from line3dpp_amd import api
    sc = CC.scene(name)
    V = CC.views_of(sc)
    for s, t in CC.pair_list(sc):
        F = CM._fundamental(V[s], V[t])
        size = (V[s].width, V[s].height, V[t].width, V[t].height)
        _assert_forms_equal(api.cull_forms(F, *size), CM.forms(F, *size), (name, s, t))


@pytest.mark.parametrize("swap", [False, True], ids=["target_side_limit", "source_side_limit"])
def test_library_forms_match_the_model_along_the_sweep(swap):
    """129 positions of the moving camera and the two the bisection found: one decision, one set of forms -- except within a
    relative 1e-9 of the flip, where the rounding of the two evaluations may decide; at most two positions lie there"""
    from line3dpp_amd import api
    lo, hi = CC.sweep_flip(swap)
    sliver = flips = 0
    last = None
    for s in sorted(list(np.linspace(0.0, 1.0, 129)) + [lo, hi]):
        a, b = CC.sweep_cameras(s, swap)
        F = CM._fundamental(CC._Cam(*a), CC._Cam(*b))
        size = (CC.SWEEP_W, CC.SWEEP_H, CC.SWEEP_W, CC.SWEEP_H)
        mod, reason, d = CM.forms_ex(F, *size)
        near = [abs(d[k] / CM.OK_MIN - 1.0) for k in ("min_Bt", "min_Bs") if k in d]
        if near and min(near) <= 1e-9:
            sliver += 1
            continue
        _assert_forms_equal(api.cull_forms(F, *size), mod, (swap, s, reason))
        flips += last is not None and last != (mod is not None)
        last = mod is not None
    assert sliver <= 2 and flips == 1, (sliver, flips)
    assert CM.forms_ex(*_sweep_args(lo, swap))[0] is not None and CM.forms_ex(*_sweep_args(hi, swap))[0] is None and 0 < hi - lo < 1e-6


def _sweep_args(s, swap):
    a, b = CC.sweep_cameras(s, swap)
    return CM._fundamental(CC._Cam(*a), CC._Cam(*b)), CC.SWEEP_W, CC.SWEEP_H, CC.SWEEP_W, CC.SWEEP_H


def test_refusal_rules_agree_on_matrices_that_are_no_fundamental_matrix():
    """the rules before the denominators: zero, non-finite, rank-1 and rank-3 matrices, and an epipole at the image centre"""
    from line3dpp_amd import api
    rng = np.random.default_rng(3)
    u, v = rng.normal(size=3), rng.normal(size=3)
    c = np.array([800.0, 600.0, 1.0])
    skew = lambda x: np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0.0]])
    want = {"F_zero_or_not_finite": [np.zeros((3, 3)), np.full((3, 3), np.nan), np.diag([1.0, np.inf, 0.0])],
            "no_epipole": [np.outer([1.0, 2.0, 3.0], [0.0, 0.0, 1.0]), np.outer([1.0, 0, 0], [0, 0, 1e-200])],
            # (a rank-1 matrix in general position: its columns' cross products are rounding noise, which the rank rule meets)
            "rank": [np.eye(3), rng.normal(size=(3, 3)), np.outer(u, v)],
            "epipole_at_centre": [skew(c)]}
    for reason, mats in want.items():
        for F in mats:
            fm, why, _ = CM.forms_ex(F, 1600, 1200, 1600, 1200)
            assert fm is None and why == reason, (reason, why, F)
            assert api.cull_forms(F, 1600, 1200, 1600, 1200) is None, (reason, F)


@pytest.mark.parametrize("name", NAMES)
def test_accepted_matches_lie_in_intersecting_model_bands(name):
    sc = CC.scene(name)
    matches = CC.oracle_pairs(name, 0)
    checked = touched = culled = 0
    for (s, t), m in zip(CC.pair_list(sc), matches):
        mp = CC.model_pair(sc, s, t)
        if not mp["enabled"]:
            continue
        culled += 1
        r, q = m["src_seg"].astype(np.int64), m["tgt_seg"].astype(np.int64)
        inter = CM.intersect(mp["src"][0], mp["src"][1], mp["tgt"][0], mp["tgt"][1], r, q)
        assert inter.all(), (name, s, t, int((~inter).sum()), m[~inter][:3])
        checked += len(m)
        touched += int(((mp["src"][2][r] == 0) | (mp["tgt"][2][q] == 0)).sum())
    print(name, dict(culled_pairs=culled, accepted=checked, touch_an_unbounded_band=touched))
    if name == "outside_segments":
        assert touched >= 20, touched
    if culled:
        assert checked >= 100, checked
