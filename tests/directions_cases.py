"""Cases of the direction detection, shared by tests/test_directions_host.py and tests/test_gpu_directions.py:
generated models with planted families of parallel segments (seeded numpy.random.default_rng) and hand-built cases from
small integer coordinates -- Pythagorean directions, whose lengths and unit vectors are exact -- in which the quantities
the tests pin are exact."""
import numpy as np

from tests import directions_model as M

TILE, CHUNK = 256, 256                     # kCmpTile, kCmpChunk: k_dir_score walks k_compare's tiling
MAX_ANGLE = 1.0                            # degrees, of the generated cases
# min_segments = 8: a clutter direction lies within 1 degree of a given one, either way round, with probability
# 1 - cos(1 degree) = 1.5e-4; among 5 000 clutter segments a hypothesis expects 0.76 such neighbours and has seven or more
# of them with probability 1e-6, which leaves 0.006 for any of 5 000 hypotheses
PAR = M.params(M.sin2_of(MAX_ANGLE), min_segments=8)
ALL_CHUNKS = 0xFFFFFFFF
EDGE_N = (1, 63, 256, 257, 513)
EDGE_SLICE_CHUNKS = (0, 1, 2, 3)
SLICING_N = 768
SLICINGS = [1, 2, 3, 0, ALL_CHUNKS]        # -> 3, 2, 1, 3, 1 slices
OBLIQUE = (2.0, 2.0, 1.0)                  # in the planted frame, / 3: 48 and 71 degrees from the axes
HAND_SIN2 = 0.2                            # between sin^2 of 20.6 and of 36.9 degrees, the steps of the Pythagorean fan


def slices_of(n, slice_chunks):
    chunks = -(-n // CHUNK)
    return -(-chunks // min(slice_chunks or 1, chunks)) if n else 0


def segs(geometry):
    return np.asarray(geometry, np.float64).reshape(-1, 6)


# ---- generated: planted families and clutter ----------------------------------------------------------------------------
def planted_case(seed, per_family, n, box=30.0, points=0.02):
    """Four families of `per_family` segments each: three along the axes of a random orthonormal frame and one along
    OBLIQUE in it, every segment's direction turned away from its family's by less than MAX_ANGLE / 4 and reversed with
    probability one half, lengths 0.5 .. 3, anywhere in a box.  The other n - 4 per_family segments are clutter with
    uniformly random directions, about 2 % of them points.  The order of the segments is shuffled.
    -> (segs [n, 6], line [n] uint32, planted: 4 arrays of segment indices, the orthogonal families first)"""
    rng = np.random.default_rng(seed)
    assert n >= 4 * per_family
    rows, label = [], []
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    families = [q[:, 0], q[:, 1], q[:, 2], q @ (np.array(OBLIQUE) / 3.0)] if per_family else []
    for f, d in enumerate(families):
        for _ in range(per_family):
            u = np.cross(d, rng.normal(size=3)); u /= np.linalg.norm(u)
            turned = d + np.tan(np.radians(rng.uniform(0.0, MAX_ANGLE / 4))) * u
            turned *= rng.choice([-1.0, 1.0]) / np.linalg.norm(turned)
            a = rng.uniform(0, box, 3)
            rows.append(np.concatenate([a, a + rng.uniform(0.5, 3.0) * turned])); label.append(f)
    n_clutter = n - len(rows)
    a = rng.uniform(0, box, (n_clutter, 3))
    d = rng.normal(size=(n_clutter, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    b = a + rng.uniform(0.5, 3.0, n_clutter)[:, None] * d
    point = rng.random(n_clutter) < points
    b[point] = a[point]
    rows += list(np.concatenate([a, b], 1)); label += [-1] * n_clutter
    order = rng.permutation(n)
    out = np.ascontiguousarray(np.array(rows).reshape(-1, 6)[order])
    label = np.array(label)[order]
    line = (np.arange(n, dtype=np.uint64) * 3 + 5).astype(np.uint32)
    return out, line, [np.flatnonzero(label == f) for f in range(len(families))]


def sized_case(n):
    """a planted case of exactly n segments: clutter alone below 63 segments, else four families of n // 7, 40 at most"""
    return planted_case(700 + n, min(40, n // 7) if n >= 63 else 0, n)


def large_case():
    """5 000 segments: four families of 60 in 4 760 clutter segments"""
    return planted_case(2032, 60, 5000)


def admitted(result, planted):
    """the issue's admission rule -> a message for the first condition the result misses, else None"""
    P, Mb, s = result["directions"], result["members"], result["summary"]
    if len(P) > len(planted) + 1:
        return f"{len(P)} directions for {len(planted)} planted"
    of_direction = [set(Mb["segment"][Mb["direction"] == p].tolist()) for p in range(len(P))]
    found = []
    for i, want in enumerate(planted):
        hits = [len(m & set(want.tolist())) for m in of_direction]
        best = max(hits, default=0)
        if best * 10 < 9 * len(want):
            return f"planted family {i}: {best} of {len(want)} segments are members of one direction"
        found.append(hits.index(best))
    if planted and (s["frame_axes"] != 3 or sorted(s["frame"]) != sorted(found[:3])):
        return f"the frame rests on {s['frame']}, the orthogonal families are directions {found[:3]}"
    return None


# ---- hand-built ---------------------------------------------------------------------------------------------------------
def cube(side=1):
    """the 12 edges of a cube, x edges first, then y, then z"""
    s = side
    geo = [(0, y, z, s, y, z) for y in (0, s) for z in (0, s)]
    geo += [(x, 0, z, x, s, z) for x in (0, s) for z in (0, s)]
    geo += [(x, y, 0, x, y, s) for x in (0, s) for y in (0, s)]
    return geo


def fan(s_length, c_length):
    """Segments in the plane z = 0 along (1, 0), (24, 7) / 25, (4, 3) / 5 and (3, 4) / 5: at 0, 16.3, 36.9 and 53.1 degrees,
    neighbours 16.3 or 20.6 degrees apart (squared sines 0.0784 and 0.1239) and the next but one 36.9 (0.36).  F0, F1 along
    x and X0, X1 along (24, 7), 25 long each; S along (4, 3), s_length long; C along (3, 4), c_length long (multiples of 5).
    At HAND_SIN2 the direction of X0 has F, X and S for members (100 + s_length), that of C only S and C."""
    s, c = s_length // 5, c_length // 5
    return [(0, 0, 0, 25, 0, 0), (0, 1, 0, 25, 1, 0), (0, 2, 0, 24, 9, 0), (0, 3, 0, 24, 10, 0), (0, 4, 0, 4 * s, 4 + 3 * s, 0),
            (0, 5, 0, 3 * c, 5 + 4 * c, 0)]


def parallel_family(k, others=0):
    """k segments along (3, 4, 12) / 13, alternately reversed, each 13 long, and `others` along x"""
    geo = [((i, 0, 0, i + 3, 4, 12) if i % 2 == 0 else (i + 3, 4, 12, i, 0, 0)) for i in range(k)]
    return geo + [(0, 10 + i, 0, 5, 10 + i, 0) for i in range(others)]


def hand_cases():
    """-> list of (name, segs, line, par, expected): expected = summary entries (every key of it is compared) plus
    counts (per hypothesis), direction_hypotheses, direction_sizes, direction_members (per direction), seg_directions"""
    out = []

    def add(name, geometry, par, line=None, **expected):
        g = segs(geometry)
        out.append((name, g, np.asarray(range(len(g)) if line is None else line, np.uint32), par, expected))

    one_degree = M.params(M.sin2_of(1.0))
    add("the 12 edges of a cube", cube(), one_degree, n_candidates=12, counts=[4] * 12, n_directions=3, n_tested=3, n_dropped=9,
        n_rejected=0, n_memberships=12, seg_directions=[1] * 12, n_segments_in_directions=12, n_segments_in_several=0, truncated=0,
        length_total=12.0, length_in_directions=12.0, scale_exponent=48, direction_hypotheses=[0, 4, 8], direction_sizes=[4, 4, 4],
        direction_members=[[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]], frame_axes=3, frame=[0, 1, 2],
        R=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    add("max_tests reached", cube(), dict(one_degree, max_tests=2), n_directions=2, n_tested=2, truncated=1, n_dropped=6, frame_axes=2,
        frame=[0, 1, M.NONE])
    add("max_directions reached", cube(), dict(one_degree, max_directions=2), n_directions=2, n_tested=2, truncated=0, n_memberships=8,
        n_dropped=3)
    add("point segments are counted and never members", [(0.5, 0.5, 0, 0.5, 0.5, 0)] + cube() + [(0, 0, 0, 0, 0, 0)], one_degree,
        n_segments=14, n_point_segments=2, n_candidates=12, counts=[0] + [4] * 12 + [0], n_directions=3,
        seg_directions=[0] + [1] * 12 + [0], length_total=12.0, direction_hypotheses=[1, 5, 9])
    # (1, 0, 0) against (3, 4, 0) / 5: X = (0, 0, 0.8), x2 = 0.8 * 0.8, whichever of the two is the hypothesis
    pair = [(0, 0, 0, 1, 0, 0), (0, 1, 0, 3, 5, 0)]
    x2 = M.sin2([1.0, 0.0, 0.0], [3.0 / 5.0, 4.0 / 5.0, 0.0])
    assert x2 == 0.8 * 0.8 == M.sin2([3.0 / 5.0, 4.0 / 5.0, 0.0], [1.0, 0.0, 0.0])
    add("a squared sine of exactly max_sin2 is an inlier", pair, M.params(x2, min_segments=2), counts=[2, 2], n_directions=1,
        direction_sizes=[2], direction_hypotheses=[0], n_dropped=1)                       # (equal members, equal weights: the first)
    add("... and the next value below it admits neither", pair, M.params(float(np.nextafter(x2, 0.0)), min_segments=2), counts=[1, 1],
        n_directions=0, n_candidates=0, frame_axes=0, frame=[M.NONE] * 3, R=list(M.IDENTITY))
    add("anti-parallel members", parallel_family(6, 2), M.params(0.0, min_segments=3), counts=[6] * 6 + [2] * 2, n_directions=1,
        direction_sizes=[6], direction_members=[[0, 1, 2, 3, 4, 5]], n_candidates=6, n_dropped=5, frame_axes=1, frame=[0, M.NONE, M.NONE])
    # C's direction shares S (15) with X0's and has C (10) to itself: 2 x 15 > 25, rejected
    add("a tilted copy is rejected", fan(15, 10), M.params(HAND_SIN2, min_segments=2), counts=[4, 4, 5, 5, 4, 2], n_candidates=6,
        n_directions=1, n_tested=2, n_dropped=4, n_rejected=1, direction_hypotheses=[2], direction_members=[[0, 1, 2, 3, 4]],
        seg_directions=[1, 1, 1, 1, 1, 0])
    # with S and C 10 long each it shares 10 of 20: 2 common == weight, accepted, and S belongs to two directions
    add("2 common == weight is accepted: a segment in two directions", fan(10, 10), M.params(HAND_SIN2, min_segments=2),
        counts=[4, 4, 5, 5, 4, 2], n_directions=2, n_tested=2, n_dropped=4, n_rejected=0, direction_hypotheses=[2, 5],
        direction_members=[[0, 1, 2, 3, 4], [4, 5]], seg_directions=[1, 1, 1, 1, 2, 1], n_segments_in_several=1, n_memberships=7,
        frame_axes=1, frame=[0, M.NONE, M.NONE])
    xy = [(0, i, 0, 2, i, 0) for i in range(4)] + [(5, 0, i, 5, 1, i) for i in range(4)]
    add("a frame of a pair", xy, one_degree, n_directions=2, frame_axes=2, frame=[0, 1, M.NONE], direction_sizes=[4, 4],
        R=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    # along z: |x_0| = |x_1| = 0, the first of equals: y from (1, 0, 0), z = x × y = (0, 1, 0)
    add("a frame of one axis: the first of equal components", [(i, 0, 0, i, 0, 3) for i in range(4)], one_degree, n_directions=1, frame_axes=1,
        frame=[0, M.NONE, M.NONE], R=[0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    # along (3, 4, 0) / 5 the smallest component is z, which the Jacobi leaves at exactly 0: y = (0, 0, 1)
    add("a frame of one axis: the smallest component", [(i, 0, 0, i + 3, 4, 0) for i in range(4)], one_degree, n_directions=1, frame_axes=1,
        frame=[0, M.NONE, M.NONE], R_y=[0.0, 0.0, 1.0])
    add("no direction", [(0, 0, 0, 1, 0, 0), (0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 1)], one_degree, counts=[1, 1, 1], n_candidates=0,
        n_directions=0, frame_axes=0, frame=[M.NONE] * 3, R=list(M.IDENTITY), length_total=3.0)
    return out


def check_expected(name, got, expected):
    P, Mb, s = got["directions"], got["members"], got["summary"]
    for k, want in expected.items():
        if k in M.SUMMARY_KEYS:
            assert s[k] == want, f"{name}: {k} = {s[k]!r}, expected {want!r}"
    assert s["n_directions"] == len(P) and s["n_memberships"] == len(Mb) == int(got["seg_directions"].sum()), name
    assert s["n_segments"] == len(got["scores"]) and s["n_tested"] == s["n_directions"] + s["n_rejected"], name
    assert np.array_equal(np.asarray(got["R"]), np.array(s["R"]).reshape(3, 3)), name
    if "R_y" in expected:
        assert s["R"][3:6] == expected["R_y"], f"{name}: R {s['R']}"
    if "counts" in expected:
        assert got["scores"]["count"].tolist() == expected["counts"], f"{name}: counts {got['scores']['count'].tolist()}"
    if "direction_sizes" in expected:
        assert P["n_segments"].tolist() == expected["direction_sizes"], f"{name}: sizes {P['n_segments'].tolist()}"
    if "direction_hypotheses" in expected:
        assert P["hypothesis"].tolist() == expected["direction_hypotheses"], f"{name}: hypotheses {P['hypothesis'].tolist()}"
    if "direction_members" in expected:
        assert [Mb["segment"][Mb["direction"] == p].tolist() for p in range(len(P))] == expected["direction_members"], f"{name}: members {Mb}"
    if "seg_directions" in expected:
        assert got["seg_directions"].tolist() == expected["seg_directions"], f"{name}: seg_directions {got['seg_directions'].tolist()}"


def same_result(got, want, what):
    """every output byte: directions, members, the per-segment counts, the scores of every hypothesis and the summary"""
    for name in ("directions", "members", "seg_directions", "scores"):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name}: {a.dtype}{a.shape} != {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(1))
            raise AssertionError(f"{what}: {name} differs in {len(bad)} rows, first {bad[0]}: {a[bad[0]]} != {b[bad[0]]}")
    same_summary(got["summary"], want["summary"], what)
    assert np.asarray(got["R"], np.float64).tobytes() == np.asarray(want["R"], np.float64).tobytes(), f"{what}: R"


def same_summary(got, want, what):
    """(the packing turns a NaN or a sign of zero into bytes, so neither passes for its counterpart)"""
    assert set(got) == set(M.SUMMARY_KEYS), what
    for k in M.SUMMARY_KEYS:
        assert M.pack_summary(dict(want, **{k: got[k]})) == M.pack_summary(want), f"{what}: summary {k}: {got[k]!r} != {want[k]!r}"
