"""Inputs of the seam-level tests (tests/test_seam_host.py on the CPU, tests/test_gpu_seam.py on the GPU): hypothesis
lists for l3d_score_matches at every list length at which k_support / k_score_all (k_views.hip) change their path, and
the sparse patterns l3d_diffuse_affinity is tried on.  Everything here is numpy and the CPU oracle: no GPU."""
import functools

import numpy as np

from line3dpp_amd.scene import make_scene

# k_views.hip: one wave staged up to 192, four waves staged up to 768, sort-only up to 1864, all pairs beyond; k_score_all
# stages up to 192.  Every limit, its two neighbours, and the ends.
SCORE_LENGTHS = (1, 2, 63, 64, 65, 191, 192, 193, 767, 768, 769, 1863, 1864, 1865, 2500)
LISTS_PER_LENGTH = 2
N_TARGET_CAMS = 40
TWO_SIGA_SQR = 200.0           # 2 * sigma_a^2 at the default sigma_a = 10 degrees
K_VIEW = np.float32(1.04e-3)   # View::k() of a 2.5 px regulariser at the focal length of make_scene
ZERO_LENGTH_LISTS = (768, 1864)  # the lists of the two zero-length 2D segments: the staged flag and sim_decide's


def support_tier(L):
    """the path of k_support for a list of L entries (the table of k_views.hip), None for an empty list"""
    if L == 0:
        return None
    return "wave" if L <= 192 else "group_staged" if L <= 768 else "sort_only" if L <= 1864 else "all_pairs"


class ScoreCase:
    """one call of l3d_score_matches / Oracle.score_lists: the view and the marshalled arrays"""

    def __init__(self, view, segs, lengths, matches4, ranges2, reg_tgt2, k):
        self.view, self.segs, self.lengths = view, segs, np.asarray(lengths)
        self.matches4, self.ranges2, self.reg_tgt2, self.k = matches4, ranges2, reg_tgt2, np.float32(k)
        self.RtKinv = view.R.T @ np.linalg.inv(view.K)
        self.list_of = np.repeat(np.arange(len(lengths)), lengths)     # the list (= segment) of every match
        self.length_of = self.lengths[self.list_of]

    def oracle(self, threads=8):
        from oracle.oracle import Oracle
        v = self.view
        o = Oracle(threads=threads)
        assert o.add_view(0, self.segs, v.K, v.R, v.t, v.width, v.height, v.median_depth, [1]) == 0
        return o

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """(scores, replace-branch count of every list, camera centre as the oracle holds it); computed once"""
        o = self.oracle()
        rep = np.zeros(len(self.lengths), np.uint64)
        scores, total = o.score_lists(0, self.matches4, self.ranges2, self.reg_tgt2, self.k, TWO_SIGA_SQR,
                                      replaced_per_seg=rep)
        assert total == int(rep.sum())
        scores.setflags(write=False); rep.setflags(write=False)
        return scores, rep, o.view_info(0)["C"]


def _one_list(rng, L, k, half_zero_length):
    """(target camera, dp1, dp2) of one list, grouped by camera.  A few true depth pairs, each seen by several cameras
    with jitter of 0.25 / 0.6 / 1.2 sqrt(reg) (similarities on both sides of 0.5) and several hypotheses per camera (the
    replace branch); exact (dp1, dp2) duplicates across cameras and duplicates of dp1 alone (rank-sort ties); clutter
    over the depth range."""
    n_cl = L if L <= 2 else L // 2
    T = 1 + min(3, L // 32)
    D1 = rng.uniform(15.0, 35.0, T); D2 = D1 + rng.uniform(-3.0, 3.0, T)
    per_cl = max(n_cl // T, 1)
    cams_of = [rng.permutation(N_TARGET_CAMS)[:min(30, max(2 if L <= 2 else 3, per_cl // 3))] for _ in range(T)]
    which = rng.integers(0, T, n_cl) if L > 2 else np.zeros(n_cl, np.int64)
    cam = np.array([cams_of[w][i % len(cams_of[w])] if L <= 2 else rng.choice(cams_of[w]) for i, w in enumerate(which)],
                   np.int64).reshape(-1)
    js = rng.choice([0.25, 0.6, 1.2], n_cl) if L > 2 else np.full(n_cl, 0.1)
    sig1 = np.sqrt(2.0) * D1[which] * float(k); sig2 = np.sqrt(2.0) * D2[which] * float(k)
    dp1 = D1[which] + rng.normal(0, 1, n_cl) * js * sig1
    dp2 = D2[which] + rng.normal(0, 1, n_cl) * js * sig2
    n_clu = L - n_cl
    cdp1 = rng.uniform(12.0, 40.0, n_clu)
    cam = np.concatenate([cam, rng.integers(0, N_TARGET_CAMS, n_clu)])
    dp1 = np.concatenate([dp1, cdp1]); dp2 = np.concatenate([dp2, cdp1 + rng.uniform(-4.0, 4.0, n_clu)])
    if L > 2:
        # duplicates: about a tenth of the list copies (dp1, dp2) of a cluster entry into another camera; a twentieth
        # copies dp1 alone
        for frac, both in ((0.10, True), (0.05, False)):
            for _ in range(max(1, int(L * frac))):
                src = rng.integers(0, n_cl); dst = rng.integers(0, L)
                if dst == src:
                    continue
                dp1[dst] = dp1[src]
                if both:
                    dp2[dst] = dp2[src]
                    if cam[dst] == cam[src]:
                        cam[dst] = (cam[src] + 1 + rng.integers(0, N_TARGET_CAMS - 1)) % N_TARGET_CAMS
    if half_zero_length:
        z = rng.random(L) < 0.5
        dp2[z] = dp1[z]          # on a zero-length 2D segment: a 3D segment of length 0
    order = rng.permutation(L)
    order = order[np.argsort(cam[order], kind="stable")]          # grouped by target camera (sortMatches)
    return cam[order], dp1[order].astype(np.float32), dp2[order].astype(np.float32)


def _assemble(view, segs, lengths, zero_len_segments, seed, k, zero_regs):
    rng = np.random.default_rng(seed)
    kt = (rng.uniform(0.8, 1.3, N_TARGET_CAMS) * float(K_VIEW)).astype(np.float32)   # View::k() of the target cameras
    rows, regs, ranges = [], [], []
    n = 0
    for s, L in enumerate(lengths):
        if L == 0:
            ranges.append((-1, -1))
            continue
        cam, dp1, dp2 = _one_list(rng, int(L), K_VIEW, s in zero_len_segments)
        rows.append(np.stack([np.full(L, s, np.float32), (1 + cam).astype(np.float32), dp1, dp2], 1))
        # stands in for View::regularizerFrom3Dpoint: distance to the target camera ~ depth, times that camera's k
        regs.append(np.stack([dp1 * kt[cam], dp2 * kt[cam]], 1).astype(np.float32))
        ranges.append((n, n + L - 1)); n += L
    m4 = np.concatenate(rows).astype(np.float32)
    rg = np.concatenate(regs).astype(np.float32)
    if zero_regs:
        rg[:] = 0
    return ScoreCase(view, segs, lengths, m4, np.array(ranges, np.int32), rg, k)


@functools.lru_cache(maxsize=None)
def score_tier_case(seed=7):
    """One view; per segment one list; every length of SCORE_LENGTHS LISTS_PER_LENGTH times in shuffled segment order,
    empty lists as the first, the last and one more segment; the segments of the lists ZERO_LENGTH_LISTS are zero-length."""
    rng = np.random.default_rng(seed)
    inner = np.array(list(SCORE_LENGTHS) * LISTS_PER_LENGTH + [0])
    lengths = np.concatenate([[0], inner[rng.permutation(len(inner))], [0]]).astype(np.int64)
    view = make_scene(3, len(lengths), n_neighbors=2, seed=seed).views[0]
    segs = view.segs.copy()
    zl = {int(np.nonzero(lengths == L)[0][0]) for L in ZERO_LENGTH_LISTS}
    for s in zl:
        segs[s, 2:] = segs[s, :2]
    return _assemble(view, segs, lengths, zl, seed + 1, K_VIEW, False)


@functools.lru_cache(maxsize=None)
def score_nan_case(seed=11):
    """k = 0 and all-zero reg_tgt2: both regularisers are 0, -d^2 / reg is NaN for equal depths and -inf otherwise; one
    list in every tier of k_support"""
    lengths = np.array([3, 65, 193, 769, 1865], np.int64)
    view = make_scene(3, len(lengths), n_neighbors=2, seed=seed).views[0]
    return _assemble(view, view.segs.copy(), lengths, set(), seed + 1, 0.0, True)


@functools.lru_cache(maxsize=None)
def score_single_case(seed=13):
    """M = 1: one segment, one list"""
    lengths = np.array([65], np.int64)
    view = make_scene(3, 1, n_neighbors=2, seed=seed).views[0]
    return _assemble(view, view.segs.copy(), lengths, set(), seed + 1, K_VIEW, False)


def recorded_lists(view, oracle):
    """The lists Oracle(record_scored=True) recorded for `view` after match_images, marshalled as Line3D::scoringGPU
    would (sortMatches: stable by target camera), with the recorded score3D.  -> (matches4, ranges2, want)"""
    m, off = oracle.scored(view.cam)
    rows, ranges, want = [], [], []
    n = 0
    for s in range(len(view.segs)):
        seg = m[off[s]:off[s + 1]]
        seg = seg[np.argsort(seg["tgt_cam"], kind="stable")]
        ranges.append((n, n + len(seg) - 1) if len(seg) else (-1, -1))
        n += len(seg)
        rows.append(np.stack([np.full(len(seg), s, np.float32), seg["tgt_cam"].astype(np.float32), seg["d_p1"], seg["d_p2"]], 1))
        want.append(seg["score3D"])
    return (np.concatenate(rows).astype(np.float32), np.array(ranges, np.int32), np.concatenate(want).astype(np.float32))


# ---- sparse patterns for l3d_diffuse_affinity --------------------------------------------------------------------
def symmetric_edges(rng, n_rows, pairs, order="random", lo=0.5, hi=1.0):
    """CLEdges (i, j, w) and (j, i, w') of the unordered `pairs` (unique, i != j); order: random | reverse | sorted"""
    from oracle.oracle import CLEDGE_DTYPE
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    e = np.zeros(2 * len(pairs), CLEDGE_DTYPE)
    e["i"] = np.concatenate([pairs[:, 0], pairs[:, 1]]); e["j"] = np.concatenate([pairs[:, 1], pairs[:, 0]])
    e["w"] = rng.uniform(lo, hi, len(e)).astype(np.float32)
    o = np.lexsort((e["j"], e["i"]))
    if order == "reverse":
        o = o[::-1]
    elif order == "random":
        o = rng.permutation(len(e))
    return np.ascontiguousarray(e[o])


def random_pairs(rng, first_row, last_row, n_pairs):
    """n_pairs unique unordered pairs (i < j) of rows in [first_row, last_row]"""
    n = last_row - first_row + 1
    assert n_pairs <= n * (n - 1) // 2
    seen = set()
    while len(seen) < n_pairs:
        i, j = rng.integers(first_row, last_row + 1, 2)
        if i != j:
            seen.add((int(min(i, j)), int(max(i, j))))
    return sorted(seen)
