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

    def __init__(self, view, segs, lengths, matches4, ranges2, reg_tgt2, k, two_sigA_sqr=None, marks=None):
        self.view, self.segs, self.lengths = view, segs, np.asarray(lengths)
        self.matches4, self.ranges2, self.reg_tgt2, self.k = matches4, ranges2, reg_tgt2, np.float32(k)
        self.two_sigA_sqr = float(TWO_SIGA_SQR if two_sigA_sqr is None else two_sigA_sqr)
        self.marks = marks                                             # score_threshold_case: what every match is there for
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
        scores, total = o.score_lists(0, self.matches4, self.ranges2, self.reg_tgt2, self.k, self.two_sigA_sqr,
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


def two_sigA_sqr_of(sigma_a):
    """Line3D::matchImages: 2 sigma_a^2 in float (line3D.cc:396-397)"""
    s = np.float32(sigma_a)
    return float(np.float32(2.0) * s * s)


def _assemble(view, segs, lengths, zero_len_segments, seed, k, zero_regs, two_sigA_sqr=None):
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
    return ScoreCase(view, segs, lengths, m4, np.array(ranges, np.int32), rg, k, two_sigA_sqr)


@functools.lru_cache(maxsize=None)
def score_tier_case(seed=7, sigma_a=None):
    """One view; per segment one list; every length of SCORE_LENGTHS LISTS_PER_LENGTH times in shuffled segment order,
    empty lists as the first, the last and one more segment; the segments of the lists ZERO_LENGTH_LISTS are zero-length.
    sigma_a: the same lists scored at 2 sigma_a^2 instead of TWO_SIGA_SQR."""
    rng = np.random.default_rng(seed)
    inner = np.array(list(SCORE_LENGTHS) * LISTS_PER_LENGTH + [0])
    lengths = np.concatenate([[0], inner[rng.permutation(len(inner))], [0]]).astype(np.int64)
    view = make_scene(3, len(lengths), n_neighbors=2, seed=seed).views[0]
    segs = view.segs.copy()
    zl = {int(np.nonzero(lengths == L)[0][0]) for L in ZERO_LENGTH_LISTS}
    for s in zl:
        segs[s, 2:] = segs[s, :2]
    return _assemble(view, segs, lengths, zl, seed + 1, K_VIEW, False, None if sigma_a is None else two_sigA_sqr_of(sigma_a))


@functools.lru_cache(maxsize=None)
def score_nan_case(seed=11, sigma_a=None):
    """k = 0 and all-zero reg_tgt2: both regularisers are 0, -d^2 / reg is NaN for equal depths and -inf otherwise; one
    list in every tier of k_support"""
    lengths = np.array([3, 65, 193, 769, 1865], np.int64)
    view = make_scene(3, len(lengths), n_neighbors=2, seed=seed).views[0]
    return _assemble(view, view.segs.copy(), lengths, set(), seed + 1, 0.0, True,
                     None if sigma_a is None else two_sigA_sqr_of(sigma_a))


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


# ---- threshold lists for l3d_score_matches ---------------------------------------------------------------------------
# Every list is made of COUPLES: an anchor A and one supporter B of another camera, at least ten window radii (of
# k_support's depth window) from every other couple, so that score(A) > 0 is one decision of similarityForScoring and its
# value one similarity.  Three kinds, each forced to within a few float steps of the value at which the decision flips:
#   y1, y2   B differs from A in one depth only; that depth and A's free target regulariser are stepped float by float until
#            -d^2 / reg, in the float operations of the kernels, is y_thr + n ulp for n = -3 ... 3
#   angular  the regulariser of the second depth is large (that term passes), B differs in dp2 by s* + t float steps,
#            t = -24 ... 24, s* the step at which the ORACLE's decision flips (bisection)
# The expected scores come from the oracle alone; `marks` only says what every match is there for.
THRESHOLD_TIERS = (64, 192, 768, 1864, 2500)   # k_support: wave, staged limit, four-wave staged, sort-only, all pairs
Y_STEPS = tuple(range(-3, 4))
ANCHORS_PER_STEP = 4
ANGULAR_STEPS = tuple(range(-24, 25))
DIR_SLACK = 2e-6                               # kDirSlack, l3d_dev.h
PAD_CAM, TOP_DEPTH = 39, 3000.0
MARK_DTYPE = np.dtype([("kind", "U8"), ("role", "U1"), ("n", "i4"), ("band", "i4"), ("couple", "i4")])


def _ford(x):
    """floats as a line of integers (monotone; -0 and +0 share 0)"""
    i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def fstep(x, n):
    """the float n steps above x (below for negative n)"""
    o = _ford(x) + np.asarray(n, np.int64)
    u = np.where(o < 0, 0x80000000 | (-o), o).astype(np.uint32)
    return u.view(np.float32)


@functools.lru_cache(maxsize=None)
def y_threshold():
    """the largest float y for which expf(y) > 0.5 fails, by bisection with the libm the oracle links (sim_thresholds)"""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.expf.restype = ctypes.c_float; libm.expf.argtypes = [ctypes.c_float]
    lo, hi = int(_ford(np.float32(-2.0))), 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if libm.expf(float(fstep(np.float32(0.0), mid))) > 0.5:
            hi = mid
        else:
            lo = mid
    return np.float32(fstep(np.float32(0.0), lo))


def kernel_reg(dp, k, rt):
    """the spatial regulariser as k_seam_entries and scoringCPU form it, in float operations"""
    dp, k, rt = np.asarray(dp, np.float32), np.float32(k), np.asarray(rt, np.float32)
    sig = dp * k
    return np.float32(0.5) * (np.float32(2.0) * sig * sig + np.float32(2.0) * rt * rt)


def _force_y(a, rt_nominal, k, n, up):
    """(b, rt): the other couple member's depth and the anchor's target regulariser with -(a - b)^2 / reg == y_thr + n ulp"""
    yt = fstep(y_threshold(), n)
    # a step of b moves d = a - b by an ulp of the DEPTH, thousands of ulps of y: the regulariser does the fine work
    rt = fstep(np.float32(rt_nominal), np.arange(-30000, 30001))[None, :]
    reg = kernel_reg(a, k, rt)
    d0 = np.sqrt(-np.float64(yt) * np.float64(kernel_reg(a, k, rt_nominal)))
    b = fstep(np.float32(np.float64(a) + (d0 if up else -d0)), np.arange(-2, 3))[:, None]
    d = np.float32(a) - b
    y = -d * d / reg
    hit = np.argwhere(y == yt)
    assert len(hit), "no (depth, regulariser) pair reaches the step"
    j, r = hit[len(hit) // 2]
    return np.float32(b[j, 0]), np.float32(rt[0, r])


def _unit_dirs(view, seg, dp1, dp2):
    """plain float64 unprojection of (dp1, dp2) on segment `seg`: unit directions [n, 3] (for the bands only)"""
    A = view.R.T @ np.linalg.inv(view.K)
    C = -view.R.T @ view.t
    r = [A @ np.array([seg[2 * i], seg[2 * i + 1], 1.0]) for i in range(2)]
    r = [x / np.linalg.norm(x) for x in r]
    P1 = C + np.asarray(dp1, np.float64)[:, None] * r[0]; P2 = C + np.asarray(dp2, np.float64)[:, None] * r[1]
    v = P2 - P1
    return v / np.linalg.norm(v, axis=1, keepdims=True)


class _Lists:
    """rows of one call: (list, camera, dp1, dp2, rt1, rt2, mark)"""

    def __init__(self):
        self.rows, self.n_couples = [], 0

    def add(self, lst, cam, dp1, dp2, rt1, rt2, kind, role="", n=0, band=0, couple=-1):
        self.rows.append((lst, cam, np.float32(dp1), np.float32(dp2), np.float32(rt1), np.float32(rt2), (kind, role, n, band, couple)))

    def couple(self):
        self.n_couples += 1
        return self.n_couples - 1


def _y_couple(B, lst, which, D, n, k, kt, cams, kind=None, fill=0):
    """one couple of the y1 (which = 0) or y2 set at anchor depth D; fill: hypotheses of A's camera between A and B"""
    a = [np.float32(D), np.float32(D * 1.02)]
    rt = [np.float32(a[0] * kt), np.float32(a[1] * kt)]
    b = list(a)
    b[which], rt[which] = _force_y(a[which], rt[which], k, n, up=True)
    c = B.couple()
    kind = kind or ("y1", "y2")[which]
    B.add(lst, cams[0], a[0], a[1], rt[0], rt[1], kind, "A", n, 0, c)
    # B's own target regulariser is 1.5 times the nominal one: its decision about A is far from the threshold (y = -0.55)
    B.add(lst, cams[1], b[0], b[1], 1.5 * a[0] * kt, 1.5 * a[1] * kt, kind, "B", n, 0, c)
    for f in range(fill):
        w = (f + 1.0) / (fill + 1.0)
        d = [np.float32(a[i] + w * (np.float64(b[i]) - a[i])) for i in range(2)]
        B.add(lst, cams[0], d[0], d[1], d[0] * kt, d[1] * kt, "fill", "", n, 0, c)


def _angular_couples(view, seg, depths, k, kt, two_sigA_sqr):
    """for anchors (D, D) on segment `seg`: the number of float steps of dp2 at which the ORACLE stops accepting the
    couple (first rejected step), by bisection on its scores alone"""
    from oracle.oracle import Oracle
    o = Oracle(threads=1)
    segs = np.ascontiguousarray(seg, np.float32).reshape(1, 4)
    assert o.add_view(0, segs, view.K, view.R, view.t, view.width, view.height, view.median_depth, [1]) == 0
    D = np.asarray(depths, np.float32)
    n = len(D)
    rt = np.stack([D * np.float32(kt), D * np.float32(0.2)], 1).astype(np.float32)

    def accepted(steps):
        m4 = np.zeros((2 * n, 4), np.float32)
        m4[:, 1] = np.repeat([1.0, 2.0], n)                       # grouped by camera: the anchors, then the supporters
        m4[:n, 2] = D; m4[:n, 3] = D; m4[n:, 2] = D; m4[n:, 3] = fstep(D, steps)
        s, _ = o.score_lists(0, m4, np.array([[0, 2 * n - 1]], np.int32), np.concatenate([rt, rt]), k, two_sigA_sqr)
        return s[:n] > 0

    lo, hi = np.zeros(n, np.int64), np.full(n, 1 << 20, np.int64)
    assert accepted(lo).all() and not accepted(hi).any()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        ok = accepted(mid)
        lo, hi = np.where(ok, mid, lo), np.where(ok, hi, mid)
    return hi, rt


def _segment(view, phi, angle):
    """a segment through the image centre that subtends phi radians"""
    f = float(view.K[0, 0]); cx, cy = float(view.K[0, 2]), float(view.K[1, 2])
    h = 0.5 * phi * f
    return np.array([cx - h * np.cos(angle), cy - h * np.sin(angle), cx + h * np.cos(angle), cy + h * np.sin(angle)], np.float32)


@functools.lru_cache(maxsize=None)
def _threshold_couples(sigma_a, seed=17):
    """the couples of score_threshold_case, the same in every tier: (view, segs, rows, k)"""
    rng = np.random.default_rng(seed)
    tsq = two_sigA_sqr_of(sigma_a)
    with_y = sigma_a >= 5.0          # below, moving one depth by a window radius turns the direction past the angular threshold
    n_lists = 5 if with_y else 2
    view = make_scene(3, n_lists, n_neighbors=2, seed=seed).views[0]
    k, kt = K_VIEW, np.float32(0.5) * K_VIEW
    # window radius of k_support / depth = sqrt(0.72 (k^2 + kt^2)) 1.0001 < 1.0e-3: depths 1.25 % apart are 12 radii apart
    assert np.sqrt(0.72 * (float(k) ** 2 + float(kt) ** 2)) * 1.0001 * 10 < 0.0125
    grid = np.float32(16.2) * np.float32(1.0125) ** np.arange(50)
    assert grid[-1] < 31.0           # one binade: a float step of a depth is 2^-19 everywhere
    B = _Lists()
    segs = np.zeros((n_lists, 4), np.float32)
    # the angular lists: segment length chosen so that a float step of dp2 moves the dot product by 1.5e-7 ... 3e-7
    theta = np.sqrt(np.log(2.0) * tsq) / 180.0 * np.pi
    phi = np.sin(theta) * 2.0 ** -19 / 16.2 / 2.9e-7
    ang_lists = (0, 1)
    for lst in ang_lists:
        segs[lst] = _segment(view, phi, rng.uniform(0, np.pi))
        ts = ANGULAR_STEPS[lst::2]
        D = grid[rng.permutation(49)[:len(ts)]]
        first_rejected, rt = _angular_couples(view, segs[lst], D, k, kt, tsq)
        for j, t in enumerate(ts):
            s = int(first_rejected[j]) + t
            # band: distance of the float64 dot product from where it is between the last accepted and first rejected step
            steps = np.array([first_rejected[j] - 1, first_rejected[j], s])
            dirs = _unit_dirs(view, segs[lst], np.full(4, D[j]), np.concatenate([[D[j]], fstep(np.full(3, D[j]), steps)]))
            x = dirs[1:] @ dirs[0]
            dist = abs(x[2] - 0.5 * (x[0] + x[1]))
            band = 1 if dist <= DIR_SLACK else 2 if dist <= 2 * DIR_SLACK else 0
            c = B.couple()
            B.add(lst, 1 + j % 5, D[j], D[j], rt[j, 0], rt[j, 1], "angular", "A", t, band, c)
            B.add(lst, 7 + j % 3, D[j], fstep(D[j], s), rt[j, 0], rt[j, 1], "angular", "B", t, band, c)
    if with_y:
        for which, lst in ((0, 2), (1, 3)):
            segs[lst] = _segment(view, 0.08, rng.uniform(0, np.pi))
            ns = [n for n in Y_STEPS for _ in range(ANCHORS_PER_STEP)]
            for j, n in enumerate(rng.permutation(ns)):
                _y_couple(B, lst, which, grid[j], int(n), k, kt, (1 + j % 5, 7 + j % 3))
        segs[4] = _segment(view, 0.08, rng.uniform(0, np.pi))
        for j, n in enumerate(Y_STEPS):                          # the walk has to step over A's own camera
            _y_couple(B, 4, 0, grid[3 * j], n, k, kt, (1 + j % 5, 7 + j % 3), kind="y1fill", fill=6)
    # in every list one more couple far above: it owns the largest dp1 (the first couple of the grid owns the smallest)
    for lst in range(n_lists):
        _y_couple(B, lst, 0, TOP_DEPTH * (1.0 + 0.01 * lst), (1, 0, -1, 2, 3)[lst], k, kt, (3, 8), kind="top")
    return view, segs, B.rows, k, tsq


@functools.lru_cache(maxsize=None)
def score_threshold_case(tier, sigma_a=10.0):
    """The couples of _threshold_couples(sigma_a) in lists of `tier` hypotheses each: padded with hypotheses of ONE
    camera in a depth band far from every couple (they support nobody and nobody supports them).  sigma_a = 10: two
    angular lists, the y1 list, the y2 list and a y1 list with the gaps filled; sigma_a = 1: the two angular lists."""
    view, segs, rows, k, tsq = _threshold_couples(float(sigma_a))
    rng = np.random.default_rng(1000 + tier)
    n_lists = len(segs)
    m4, rg, marks, ranges = [], [], [], []
    n = 0
    for lst in range(n_lists):
        mine = [r for r in rows if r[0] == lst]
        assert len(mine) <= tier, (lst, len(mine))
        pad = tier - len(mine)
        pd1 = rng.uniform(300.0, 600.0, pad).astype(np.float32)
        pd2 = (pd1 * rng.uniform(0.98, 1.02, pad)).astype(np.float32)
        mine += [(lst, PAD_CAM, pd1[i], pd2[i], pd1[i] * k, pd2[i] * k, ("pad", "", 0, 0, -1)) for i in range(pad)]
        order = rng.permutation(len(mine))
        order = order[np.argsort([mine[i][1] for i in order], kind="stable")]       # grouped by target camera (sortMatches)
        for i in order:
            _, cam, dp1, dp2, rt1, rt2, mark = mine[i]
            m4.append((lst, cam, dp1, dp2)); rg.append((rt1, rt2)); marks.append(mark)
        ranges.append((n, n + tier - 1)); n += tier
    return ScoreCase(view, segs, np.full(n_lists, tier, np.int64), np.array(m4, np.float32), np.array(ranges, np.int32),
                     np.array(rg, np.float32), k, tsq, np.array(marks, MARK_DTYPE))
