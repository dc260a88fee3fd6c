"""The four seam entries of the C-ABI (include/l3dpp_hip.h section (2)) on the GPU, at the sizes where their own device
code and host set-up change path: l3d_score_matches in every tier of k_support / k_score_all (k_views.hip),
l3d_match_lines at the sizes its set-up branches on, l3d_diffuse_affinity and l3d_find_collinear_segments at their
launch-grid edges.  Checkers: the CPU oracle's restatement and, for the diffusion, the reference's own code run on the host."""
import ctypes as C

import numpy as np
import pytest

from line3dpp_amd import _lib
from line3dpp_amd._lib import SLOT_DTYPE, ptr
from line3dpp_amd.scene import make_scene
from tests import helpers as H
from tests import seam_cases as S

pytestmark = pytest.mark.gpu

L3D_ERR_ARG, L3D_ERR_LIMIT = -1, -9
TIER_COUNTERS = {"wave": b"seam_support_wave_lists", "group_staged": b"seam_support_group_staged_lists",
                 "sort_only": b"seam_support_sort_only_lists", "all_pairs": b"seam_support_all_pairs_lists"}
UNSTAGED_COUNTER = b"seam_score_unstaged_lists"


def _counters():
    L = _lib.load()
    out = {k: L.l3d_debug_counter(n) for k, n in TIER_COUNTERS.items()}
    out["unstaged"] = L.l3d_debug_counter(UNSTAGED_COUNTER)
    assert all(v != 2**64 - 1 for v in out.values()), "l3d_debug_counter does not know a seam counter"
    return out


def _score_and_compare(case):
    """l3d_score_matches on the case's arrays against Oracle.score_lists on the same arrays: the > 0 pattern identical,
    every positive score within REL_TOL -- every match is in one of the two comparisons.  Returns (got, want)."""
    from line3dpp_amd.api import score_matches
    want, _, centre = case.reference()
    before = _counters()
    got = score_matches(case.segs, case.matches4, case.ranges2, case.reg_tgt2, case.RtKinv, centre, case.two_sigA_sqr, case.k)
    after = _counters()
    assert got.shape == want.shape and not np.isnan(got).any()
    flipped = np.nonzero((got > 0) != (want > 0))[0]
    assert not len(flipped), (f"{len(flipped)} matches scored on one side only, first {flipped[:5]} in lists of "
                              f"{case.length_of[flipped[:5]]}: got {got[flipped[:5]]}, want {want[flipped[:5]]}")
    nz = want > 0
    err = np.abs(got[nz].astype(np.float64) - want[nz]) / want[nz]
    print(f"lists {sorted(set(case.lengths.tolist()))}: {int(nz.sum())} of {len(want)} positive, max rel {err.max() if nz.any() else 0.0:.3g}")
    worst = np.nonzero(nz)[0][np.argsort(-err)[:5]] if nz.any() else []
    assert not nz.any() or err.max() <= H.REL_TOL, (worst, case.length_of[worst], got[worst], want[worst])
    assert not got[~nz].any()
    # the increments the call's own list lengths ask for
    expect = {k: 0 for k in before}
    for L in case.lengths:
        if L:
            expect[S.support_tier(int(L))] += 1
            expect["unstaged"] += int(L > 192)
    assert {k: after[k] - before[k] for k in before} == expect
    return got, want


def test_score_matches_in_every_tier_of_its_kernels():
    """Lists of 1 ... 2500 hypotheses, two per length, around every limit of k_support (192 / 768 / 1864) and k_score_all
    (192): all four support paths and both scoring paths run in this one call (the debug counters say so), and every
    score agrees with scoringCPU's loops on the same lists.  tests/test_seam_host.py shows on the CPU that these lists
    decide both ways in every length class."""
    case = S.score_tier_case()
    got, want = _score_and_compare(case)
    assert len(got) == sum(S.SCORE_LENGTHS) * S.LISTS_PER_LENGTH
    for L in S.SCORE_LENGTHS:
        if L >= 64:
            frac = float((want[case.length_of == L] > 0).mean())
            assert 0.10 <= frac <= 0.90, (L, frac)


def test_score_matches_with_zero_regularisers_drops_the_nan_terms():
    """k = 0 and reg_tgt2 = 0: -d^2 / reg is NaN for equal depths and -inf otherwise, in every tier; the fmin chain
    drops the NaN as the reference's does (exact duplicates score through the angular term alone)"""
    got, want = _score_and_compare(S.score_nan_case())
    assert (want > 0).sum() > 100 and (want == 0).sum() > 1000


@pytest.mark.parametrize("sigma_a", [0.5, 80.0])
def test_score_matches_in_every_tier_at_other_sigma_a(sigma_a):
    """The tier lists and the k = 0 lists again at sigma_a = 0.5 (angular thresholds at 0.59 degrees: many pairs inside the
    fp32 slack) and at sigma_a = 80 (the x_hi == 0 form of the thresholds: every direction passes).
    tests/test_seam_host.py shows that both still decide both ways in every length class."""
    got, want = _score_and_compare(S.score_tier_case(sigma_a=sigma_a))
    assert len(got) == sum(S.SCORE_LENGTHS) * S.LISTS_PER_LENGTH
    got, want = _score_and_compare(S.score_nan_case(sigma_a=sigma_a))
    assert (want > 0).sum() > 100 and (want == 0).sum() > 1000


@pytest.mark.parametrize("sigma_a", [10.0, 1.0])
@pytest.mark.parametrize("tier", S.THRESHOLD_TIERS)
def test_score_matches_at_the_thresholds_of_the_similarity(tier, sigma_a):
    """Lists of couples forced to within a few float steps of the thresholds of `similarityForScoring(i, j) > 0.5`
    (tests/seam_cases.py: score_threshold_case), in every tier of k_support: -d^2 / reg at y_thr - 3 ... + 3 ulp in either
    depth, and the direction at every float step of dp2 from 24 below to 24 above the step at which the oracle's angular
    decision flips, half of them inside kDirSlack of the threshold (the fp64 redo of the staged tiers) and half beyond it
    (the fp32 decision).  Every anchor's score is one decision and one similarity: a `>=` for a `>`, a slack that is too
    small or a window that loses its last neighbour flips one of them.  tests/test_seam_host.py shows from the oracle alone
    that the couples flip exactly where they were forced to.  k_lists, k_cand_exact and k_edges of the main path cannot be
    fed hand-built hypotheses: their behaviour at the thresholds rests on the host pin of the function they share with
    these kernels (tests/cpp/sim_scoring.cpp)."""
    case = S.score_threshold_case(tier, sigma_a)
    got, want = _score_and_compare(case)
    anchors = case.marks["role"] == "A"
    assert (want[anchors] > 0).sum() >= 24 and (want[anchors] == 0).sum() >= 24


def test_score_matches_single_list_single_segment():
    got, want = _score_and_compare(S.score_single_case())
    assert (want > 0).sum() > 10


# ---- l3d_match_lines ----------------------------------------------------------------------------------------------------
def _pair_scene(Ms, Mt, seed):
    """two ring views cut to Ms and Mt segments (as test_phase_a_views_of_different_size_and_overlap_threshold cuts them)"""
    sc = make_scene(2, max(Ms, Mt), n_neighbors=2, seed=seed)
    sc.views[0].segs = sc.views[0].segs[:Ms].copy()
    sc.views[1].segs = sc.views[1].segs[:Mt].copy()
    return sc


def _match_through_the_seam(sc, src, tgt, kNN, epi=0.25):
    from line3dpp_amd.api import match_lines
    from oracle.oracle import Oracle
    o = Oracle(threads=8); o.add_scene(sc)
    o.begin_match(kNN=kNN, epi_overlap=epi)
    F = o.fundamental(src, tgt)
    by_cam = {v.cam: v for v in sc.views}
    vs, vt = by_cam[src], by_cam[tgt]
    A0 = vs.R.T @ np.linalg.inv(vs.K); A1 = vt.R.T @ np.linalg.inv(vt.K)
    slots, n = match_lines(vs.segs, vt.segs, F, A0, A1, o.view_info(src)["C"], o.view_info(tgt)["C"], vs.width, vs.height,
                           epi, kNN)
    om, _ = o.match_pair(src, tgt)
    o.end_match()
    r = H.compare_pair(slots, om)
    assert n == len(om) and not r["missing"] and not r["extra"], (n, len(om), r["missing"][:3], r["extra"][:3])
    assert r["order_mismatch"] == 0
    assert r["max_rel"] < 1e-5      # RtKinv passed in comes from numpy's inverse, not the cofactor formula
    return len(om)


@pytest.mark.parametrize("Ms,Mt,kNN,min_matches", [
    (1, 1, 1, 0), (63, 350, 6, 50), (65, 64, 3, 20), (129, 1, 2, 0),
    (350, 4096, 6, 1000),       # sorted target copies (kSortedCopyMinSegs)
    (100, 16385, 4, 300),       # sort keys in global memory (beyond kCullLdsSegs)
    (100, 65600, 4, 300),       # 32-bit target indices (from 65 536 targets)
])
def test_match_lines_at_the_sizes_its_setup_branches_on(Ms, Mt, kNN, min_matches):
    assert _match_through_the_seam(_pair_scene(Ms, Mt, seed=23 + Ms), 0, 1, kNN) >= min_matches


def test_match_lines_streams_the_targets_when_culling_is_refused():
    """two cameras on one optical axis: the epipole lies inside the image, make_cull refuses, the targets are streamed"""
    from tests.test_gpu_parity import _forward_motion_scene
    assert _match_through_the_seam(_forward_motion_scene(n_segs=300), 0, 1, 5) > 200


def test_match_lines_replays_rows_of_equal_overlaps():
    """every segment twice in its view (as test_equal_overlaps_follow_the_reference_heap_order builds them): nearly every
    row has equal overlaps and goes through k_match_tied_rows behind the seam; same slots in the same order"""
    sc = make_scene(2, 300, n_neighbors=2, seed=41)
    for v in sc.views:
        v.segs[1::2] = v.segs[0::2]
    assert _match_through_the_seam(sc, 0, 1, 3) > 300


def test_match_lines_limits_leave_the_output_alone():
    L = _lib.load()
    sc = _pair_scene(3, 40, seed=5)
    a = np.ascontiguousarray(sc.views[0].segs, np.float32); b = np.ascontiguousarray(sc.views[1].segs, np.float32)
    I = np.eye(3); z = np.zeros(3); o = np.ones(3)
    for kNN, rc_want, word in ((400, L3D_ERR_LIMIT, "kNN too large"), (0, L3D_ERR_ARG, "kNN > 0")):
        out = np.zeros((len(a), max(kNN, 1)), SLOT_DTYPE); out["tgt_seg"] = 12345
        n = C.c_uint64(99)
        rc = L.l3d_match_lines(0, ptr(a), len(a), ptr(b), len(b), ptr(I), ptr(I), ptr(I), ptr(z), ptr(o), 3072, 2304,
                               C.c_float(0.25), kNN, ptr(out), C.byref(n))
        assert rc == rc_want and word in _lib.last_error(), (kNN, rc, _lib.last_error())
        assert (out["tgt_seg"] == 12345).all() and n.value == 99


# ---- l3d_diffuse_affinity -----------------------------------------------------------------------------------------------
def _covering_pairs(rng, first, last, n_pairs):
    """n_pairs unique pairs on the rows [first, last] that leave none of them empty: the chain first-...-last and random
    ones on top"""
    chain = [(i, i + 1) for i in range(first, last)]
    assert n_pairs >= len(chain)
    extra = [p for p in S.random_pairs(rng, first, last, min(n_pairs + len(chain), (last - first + 1) * (last - first) // 2))
             if p[1] != p[0] + 1]
    return chain + extra[:n_pairs - len(chain)]


def _check_diffusion(e, n_rows, iterations=10, own_code=True):
    """own_code: the checker is the reference's own code run on the host (10 iterations; patterns without empty rows only:
    K_sparseMat_row_normalization reads data[-1] for an empty row); otherwise the restatement"""
    from line3dpp_amd.api import diffuse_affinity
    from oracle import oracle as O
    if own_code:
        assert iterations == 10 and O.have_cuda_path(), "oracle/_ref/libl3d_ref_cuda.so is missing"
        assert (np.bincount(e["i"], minlength=n_rows) > 0).all()
        want = O.rdd_reference(e, n_rows)
    else:
        want = O.Oracle.rdd(e, n_rows, iterations)
    got = diffuse_affinity(e, n_rows, iterations)
    assert len(got) == len(e) == len(want)
    assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["j"], want["j"])
    assert (want["w"] > 0).all()
    err = np.abs(got["w"].astype(np.float64) - want["w"]) / want["w"]
    assert err.max() <= H.REL_TOL, (int(err.argmax()), got[err.argmax()], want[err.argmax()])
    return got, want


@pytest.mark.parametrize("n_rows,n_pairs", [(2, 1), (30, 127), (30, 128), (30, 129)])
def test_diffusion_at_the_edges_of_the_entry_grid(n_rows, n_pairs):
    """n_edges = 2, 254, 256, 258 around one 256-thread block; the reference's own code and the restatement agree bit for
    bit on the same input (one checker stands for the other at other iteration counts)"""
    from oracle import oracle as O
    rng = np.random.default_rng(100 + n_pairs)
    e = S.symmetric_edges(rng, n_rows, _covering_pairs(rng, 0, n_rows - 1, n_pairs))
    assert len(e) == 2 * n_pairs
    _, want = _check_diffusion(e, n_rows)
    restated = O.Oracle.rdd(e, n_rows, 10)
    assert np.array_equal(restated, want), "the restatement and the reference's own code differ"


@pytest.mark.parametrize("n_rows", [255, 256, 257])
def test_diffusion_at_the_edges_of_the_row_grid_with_empty_rows(n_rows):
    """n_rows + 1 row pointers around one 256-thread block; the first and the last three rows are empty (the restatement
    checks: the reference's own row normalisation reads outside its array for an empty row)"""
    rng = np.random.default_rng(n_rows)
    e = S.symmetric_edges(rng, n_rows, _covering_pairs(rng, 3, n_rows - 4, 600))
    _check_diffusion(e, n_rows, own_code=False)


def test_diffusion_of_a_hub_row_against_rows_of_degree_one():
    """row 0 has 5000 entries, every other row one: the lockstep walk of (row of P) x (column of W) stops at the shorter"""
    rng = np.random.default_rng(7)
    e = S.symmetric_edges(rng, 5001, [(0, j) for j in range(1, 5001)])
    got, _ = _check_diffusion(e, 5001)
    assert len(np.unique(got["w"])) > 100


def test_diffusion_clamps_tiny_rows_and_products():
    """the entries of rows 0-4 (and their transposes) weigh 1e-20: their row sums clamp to 1e-12 and so do the products"""
    rng = np.random.default_rng(8)
    e = S.symmetric_edges(rng, 40, _covering_pairs(rng, 0, 39, 200))
    e["w"][(e["i"] < 5) | (e["j"] < 5)] = 1e-20
    got, want = _check_diffusion(e, 40)
    assert (want["w"] == np.float32(1e-12)).sum() > 10 and (want["w"] > np.float32(1e-12)).sum() > 10


@pytest.mark.parametrize("iterations", [0, 1, 2, 11])
def test_diffusion_at_other_iteration_counts(iterations):
    """the P / P' swap parity follows the count"""
    rng = np.random.default_rng(9)
    e = S.symmetric_edges(rng, 80, _covering_pairs(rng, 0, 79, 400))
    _check_diffusion(e, 80, iterations=iterations, own_code=False)


@pytest.mark.parametrize("order", ["random", "reverse", "sorted"])
def test_diffusion_takes_the_edges_in_any_order(order):
    rng = np.random.default_rng(10)
    pairs = _covering_pairs(rng, 0, 299, 1500)
    _check_diffusion(S.symmetric_edges(np.random.default_rng(11), 300, pairs, order=order), 300)


# ---- l3d_find_collinear_segments ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 4097, 8193])
def test_collinear_segments_at_the_grid_and_scan_edges(M):
    """split synthetic views around one wave, and beyond 4096 and 8192 segments, where the scan of the list lengths has
    two and three tiles; against View::findCollinCPU of the oracle"""
    from line3dpp_amd.api import find_collinear_segments
    from oracle.oracle import Oracle
    sc = H.split_scene(make_scene(2, M, n_neighbors=2, seed=90 + M % 7, max_views=1))
    v = sc.views[0]
    assert len(v.segs) == M
    o = Oracle(threads=8); o.add_scene(sc)
    o.find_collinear(v.cam, 6.0)
    ooff, oidx = o.collinear(v.cam, M)
    off, idx = find_collinear_segments(v.segs, 6.0)
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    assert len(idx) > 0 or M < 63


def test_collinear_segments_sizing_protocol():
    L = _lib.load()
    v = H.split_scene(make_scene(2, 300, n_neighbors=2, seed=91, max_views=1)).views[0]
    a = np.ascontiguousarray(v.segs, np.float32)
    M = len(a)

    def call(t, idx, cap):
        off = np.full(M + 1, 777, np.uint32); n = C.c_uint64(777)
        rc = L.l3d_find_collinear_segments(0, ptr(a), M, C.c_float(t), ptr(off), ptr(idx), cap, C.byref(n))
        assert rc == 0, _lib.last_error()
        return off, n.value

    off0, n0 = call(6.0, None, 0)                                  # idx = NULL: the count and the offsets
    assert n0 > 0 and off0[0] == 0 and off0[M] == n0 and (np.diff(off0.astype(np.int64)) >= 0).all()
    small = np.full(n0, 0xABCDEF, np.uint32)
    off1, n1 = call(6.0, small, n0 - 1)                            # cap below *n: idx stays as it was
    assert n1 == n0 and np.array_equal(off1, off0) and (small == 0xABCDEF).all()
    full = np.full(n0 + 3, 0xABCDEF, np.uint32)
    off2, n2 = call(6.0, full, n0 + 3)
    assert n2 == n0 and np.array_equal(off2, off0) and (full[n0:] == 0xABCDEF).all() and (full[:n0] < M).all()
    for t in (1e-12, 0.0, -1.0):                                   # at or below L3D_EPS: empty lists
        off3, n3 = call(t, full, n0 + 3)
        assert n3 == 0 and not off3.any()
