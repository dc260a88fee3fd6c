"""CPU side of the seam-level tests: the oracle's scoring of caller-supplied lists (Oracle.score_lists) pinned on
the scores scoringCPU recorded, the properties the GPU tier test relies on (checked on the generator and the oracle
alone), and the argument checks the seam entries make on the host before they touch a device."""
import ctypes as C

import numpy as np
import pytest

from line3dpp_amd import _lib
from line3dpp_amd._lib import CLEDGE_DTYPE, SLOT_DTYPE, ptr
from line3dpp_amd.scene import make_scene
from tests import seam_cases as S

L3D_ERR_ARG = -1


@pytest.mark.parametrize("n_views,n_segs,nn,seed", [(8, 300, 4, 95), (6, 300, 4, 1)])
def test_score_lists_reproduces_the_recorded_scores(n_views, n_segs, nn, seed):
    """The lists Oracle(record_scored=True) recorded, in sortMatches order, through Oracle.score_lists with the
    regularisers taken from the context's views: score3D bit for bit.  The second context stands in the frame the first
    one scored in (begin_match translates; a finished match_images has translated back)."""
    from oracle.oracle import Oracle
    sc = make_scene(n_views, n_segs, n_neighbors=nn, seed=seed)
    o = Oracle(record_scored=True, threads=4); o.add_scene(sc); o.match_images()
    f = Oracle(threads=4); f.add_scene(sc); f.begin_match()
    total = positive = 0
    for v in sc.views:
        m4, ranges, want = S.recorded_lists(v, o)
        k = f.view_info(v.cam)["k"]
        assert k == o.view_info(v.cam)["k"]
        got, _, regs = f.score_lists(v.cam, m4, ranges, None, k, 200.0, return_regs=True)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"view {v.cam}"
        # fed back as an input, the regularisers it used give the same scores again
        again, _ = f.score_lists(v.cam, m4, ranges, regs, k, 200.0)
        assert np.array_equal(again.view(np.uint32), want.view(np.uint32))
        total += len(want); positive += int((want > 0).sum())
    f.end_match()
    assert total > 5000 and positive > 100


def test_score_tier_case_decides_both_ways_in_every_class():
    """What makes a pass of the GPU tier test mean something, from the oracle's result alone: in every length class
    from 64 up between 10 % and 90 % of the hypotheses score above 0 and the replace branch ran."""
    c = S.score_tier_case()
    want, replaced, _ = c.reference()
    assert len(want) == LISTS_TOTAL and not np.isnan(want).any()
    assert c.ranges2[0].tolist() == [-1, -1] and c.ranges2[-1].tolist() == [-1, -1]
    assert sorted(c.lengths[c.lengths > 0].tolist()) == sorted(S.SCORE_LENGTHS * S.LISTS_PER_LENGTH)
    for L in S.SCORE_LENGTHS:
        if L < 64:
            continue
        m = c.length_of == L
        frac = float((want[m] > 0).mean())
        assert 0.10 <= frac <= 0.90, (L, frac)
        assert int(replaced[c.lengths == L].sum()) > 0, L
    # the hypotheses of a zero-length 2D segment with equal depths have no 3D length: they neither score nor support
    for L in S.ZERO_LENGTH_LISTS:
        s = int(np.nonzero(c.lengths == L)[0][0])
        a, b = c.ranges2[s]
        z = c.matches4[a:b + 1, 2] == c.matches4[a:b + 1, 3]
        assert z.sum() > L // 4 and not want[a:b + 1][z].any() and want[a:b + 1][~z].any()
    # the k = 0 call: exact duplicates across cameras score (both exponents NaN: the angular term alone), the rest do not
    n = S.score_nan_case()
    w, _, _ = n.reference()
    assert not np.isnan(w).any() and (w > 0).any() and (w == 0).any()
    for s, L in enumerate(n.lengths):
        a, b = n.ranges2[s]
        m = n.matches4[a:b + 1]
        dup = np.array([((m[:, 2] == r[2]) & (m[:, 3] == r[3]) & (m[:, 1] != r[1])).any() for r in m])
        assert np.array_equal(w[a:b + 1] > 0, dup), L


LISTS_TOTAL = sum(S.SCORE_LENGTHS) * S.LISTS_PER_LENGTH


@pytest.mark.parametrize("sigma_a", [0.5, 80.0])
def test_score_tier_case_decides_both_ways_at_other_sigma_a(sigma_a):
    """The tier lists and the k = 0 lists scored at sigma_a = 0.5 (an angular threshold of 0.59 degrees) and at sigma_a = 80
    (x_hi == 0: every direction passes) still decide both ways in every length class from 64 up, as at the default."""
    c = S.score_tier_case(sigma_a=sigma_a)
    assert c.two_sigA_sqr == 2.0 * sigma_a * sigma_a and c is not S.score_tier_case()
    want, _, _ = c.reference()
    default, _, _ = S.score_tier_case().reference()
    assert not np.isnan(want).any()
    for L in S.SCORE_LENGTHS:
        if L >= 64:
            frac = float((want[c.length_of == L] > 0).mean())
            print(f"sigma_a {sigma_a}: length {L}: {frac:.3f} positive")
            assert 0.10 <= frac <= 0.90, (L, frac)
    # the narrow angle takes supporters away; the wide one changes nothing the default's 8.3 degrees had not accepted already
    changed = int(((want > 0) != (default > 0)).sum())
    print(f"sigma_a {sigma_a}: {changed} decisions differ from sigma_a = 10")
    assert (changed > 100) if sigma_a < 1 else ((want > 0) >= (default > 0)).all()
    w, _, _ = S.score_nan_case(sigma_a=sigma_a).reference()
    assert not np.isnan(w).any() and (w > 0).sum() > 100 and (w == 0).sum() > 1000


@pytest.mark.parametrize("sigma_a", [10.0, 1.0])
@pytest.mark.parametrize("tier", S.THRESHOLD_TIERS)
def test_threshold_couples_flip_where_they_were_forced_to(tier, sigma_a):
    """What makes a pass of the GPU threshold test mean something, from the generator and the oracle alone: every anchor's
    score is ONE decision (nothing but its supporter within ten window radii), and the oracle flips exactly at the forced
    step -- y_thr + n ulp scores for n = 1, 2, 3 and not for n = -3 ... 0, the angular couples score up to the step before
    s* and not from s* on -- with at least ANCHORS_PER_STEP anchors at every n of the y1 and of the y2 set, and at least 6
    accepted and 6 rejected angular anchors inside kDirSlack of the flip and as many between one and two kDirSlack."""
    c = S.score_threshold_case(tier, sigma_a)
    want, _, _ = c.reference()
    mk, dp1, cam = c.marks, c.matches4[:, 2], c.matches4[:, 1]
    assert (c.lengths == tier).all() and len(want) == tier * len(c.lengths) and not np.isnan(want).any()
    A = mk["role"] == "A"
    # isolation, in the kernel's own float operations
    reg1 = S.kernel_reg(dp1, c.k, c.reg_tgt2[:, 0])
    radius = np.sqrt(np.float32(0.72) * reg1) * np.float32(1.0001)
    closest = np.inf
    for i in np.nonzero(mk["couple"] >= 0)[0]:
        if mk["kind"][i] == "fill":
            continue
        others = (c.list_of == c.list_of[i]) & (mk["couple"] != mk["couple"][i])
        closest = min(closest, float(np.abs(dp1[others] - dp1[i]).min() / radius[i]))
        mate = (c.list_of == c.list_of[i]) & (mk["couple"] == mk["couple"][i]) & (mk["role"] != mk["role"][i]) & (mk["role"] != "")
        assert mate.sum() == 1 and cam[mate][0] != cam[i]
        if mk["kind"][i] == "y1fill" and mk["role"][i] == "A":     # the walk from A to B steps over A's own camera
            own = (c.list_of == c.list_of[i]) & (mk["kind"] == "fill") & (mk["couple"] == mk["couple"][i])
            assert own.sum() == 6 and (cam[own] == cam[i]).all()
            assert ((dp1[own] > dp1[i]) & (dp1[own] < dp1[mate][0])).all()
    print(f"tier {tier}, sigma_a {sigma_a}: the nearest stranger of a couple member is {closest:.1f} window radii away")
    assert closest >= 10.0
    assert not want[mk["kind"] == "pad"].any()
    for s in range(len(c.lengths)):                                 # the ends of the sorted walk and the rank tie
        m = c.list_of == s
        assert mk["couple"][m][dp1[m].argmin()] >= 0 and mk["kind"][m][dp1[m].argmax()] == "top"
    for kind in ("y2", "angular"):
        i = np.nonzero(A & (mk["kind"] == kind))[0]
        assert all(dp1[(mk["couple"] == mk["couple"][j]) & (mk["role"] == "B")][0] == dp1[j] for j in i)
    # the oracle flips at the forced step
    for kind in ("y1", "y2", "y1fill", "top"):
        m = A & (mk["kind"] == kind)
        if sigma_a < 5 and kind != "top":
            assert not m.any()
            continue
        assert np.array_equal(want[m] > 0, mk["n"][m] > 0), kind
        counts = {n: int((m & (mk["n"] == n)).sum()) for n in S.Y_STEPS}
        print(f"  {kind}: anchors per n {counts}")
        if kind in ("y1", "y2"):
            assert min(counts.values()) >= S.ANCHORS_PER_STEP
        elif kind == "y1fill":
            assert min(counts.values()) >= 1
    assert (want[A & (mk["kind"] == "top")] > 0).any() or sigma_a < 5
    m = A & (mk["kind"] == "angular")
    assert sorted(mk["n"][m].tolist()) == list(S.ANGULAR_STEPS)
    assert np.array_equal(want[m] > 0, mk["n"][m] < 0)
    for band in (1, 2):
        acc = int((m & (mk["band"] == band) & (want > 0)).sum()); rej = int((m & (mk["band"] == band) & (want == 0)).sum())
        print(f"  angular, band {band} ({'inside kDirSlack' if band == 1 else 'between one and two kDirSlack'}): {acc} accepted, {rej} rejected")
        assert acc >= 6 and rej >= 6


# ---- host-side argument checks: nothing below launches a kernel or needs a device ---------------------------------------
def _score_raw(c, m4=None, ranges=None):
    L = _lib.load()
    m4 = np.ascontiguousarray(c.matches4 if m4 is None else m4, np.float32)
    ranges = np.ascontiguousarray(c.ranges2 if ranges is None else ranges, np.int32)
    segs = np.ascontiguousarray(c.segs, np.float32)
    A = np.ascontiguousarray(c.RtKinv, np.float64); Cc = np.zeros(3)
    out = np.full(len(m4), -7.0, np.float32)
    rc = L.l3d_score_matches(0, ptr(segs), len(segs), ptr(m4), ptr(ranges), ptr(c.reg_tgt2), len(m4), ptr(A), ptr(Cc),
                             C.c_float(S.TWO_SIGA_SQR), C.c_float(float(c.k)), ptr(out))
    return rc, _lib.last_error(), out


@pytest.mark.parametrize("what,value", [
    ("segment of the next list", None), ("segment beyond M", 1.0e6), ("negative segment", -1.0), ("NaN segment", np.nan),
    ("fractional segment", 0.5), ("infinite segment", np.inf),
    ("negative camera", -1.0), ("NaN camera", np.nan), ("fractional camera", 2.5), ("infinite camera", np.inf),
])
def test_score_matches_rejects_what_the_entry_kernel_would_misread(what, value):
    """l3d_score_matches reads the view's segment array at matches4[i].x on the device: a match whose source segment is
    not the segment whose range holds it (so also anything at or beyond M, negative, NaN or fractional) and a target
    camera that is no id are turned away on the host with L3D_ERR_ARG, the message names the first such match, and
    `scores` stays as it was."""
    c = S.score_single_case() if "next list" not in what else S.score_nan_case()
    m4 = c.matches4.copy()
    first_bad, other_bad = 17, 40
    col = 1 if "camera" in what else 0
    if value is None:
        a, b = c.ranges2[1]
        first_bad, other_bad = int(a) + 5, int(b)
        m4[first_bad, 0] = 2.0; m4[other_bad, 0] = 0.0       # valid segments of the view, not the ones of this range
    else:
        m4[first_bad, col] = m4[first_bad, col] + value if "fractional" in what else value
        m4[other_bad, col] = value
    rc, msg, out = _score_raw(c, m4=m4)
    assert rc == L3D_ERR_ARG
    assert f"match {first_bad} " in msg and ("camera" in msg) == (col == 1), msg
    assert (out == -7.0).all()


def test_score_matches_accepts_the_unmodified_lists_up_to_the_device():
    """the same arrays without the damage pass the host checks: the call gets as far as the device (or, without one, fails
    there and not on an argument)"""
    rc, msg, _ = _score_raw(S.score_single_case())
    assert rc != L3D_ERR_ARG, msg


def test_diffuse_affinity_rejects_a_pattern_without_its_transpose():
    """The reference's own diffusion has no defined result for an edge (i, j) without (j, i) -- it reads P[-1] when that
    leaves a row empty, and otherwise returns more entries than it was given -- so the seam entry turns it away."""
    L = _lib.load()
    rng = np.random.default_rng(5)
    e = S.symmetric_edges(rng, 60, S.random_pairs(rng, 0, 59, 200))
    drop = 123
    gone = e[drop]
    e = np.ascontiguousarray(np.delete(e, drop))
    first = int(np.nonzero((e["i"] == gone["j"]) & (e["j"] == gone["i"]))[0][0])
    out = np.zeros(len(e), CLEDGE_DTYPE); out["w"] = -7.0
    rc = L.l3d_diffuse_affinity(0, ptr(e), len(e), 60, 10, ptr(out))
    assert rc == L3D_ERR_ARG
    msg = _lib.last_error()
    assert f"edge {first} " in msg and f"({int(gone['j'])}, {int(gone['i'])})" in msg, msg
    assert (out["w"] == -7.0).all()


def test_match_lines_needs_a_positive_knn():
    L = _lib.load()
    v = make_scene(3, 5, n_neighbors=2, seed=2).views[0]
    segs = np.ascontiguousarray(v.segs, np.float32)
    I = np.eye(3); z = np.zeros(3)
    out = np.zeros((len(segs), 1), SLOT_DTYPE); out["tgt_seg"] = 12345
    n = C.c_uint64(99)
    rc = L.l3d_match_lines(0, ptr(segs), len(segs), ptr(segs), len(segs), ptr(I), ptr(I), ptr(I), ptr(z), ptr(z), v.width,
                           v.height, C.c_float(0.25), 0, ptr(out), C.byref(n))
    assert rc == L3D_ERR_ARG and "kNN" in _lib.last_error()
    assert (out["tgt_seg"] == 12345).all() and n.value == 99
