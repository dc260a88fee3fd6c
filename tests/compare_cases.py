"""Cases of the comparison of two 3D line models, shared by tests/test_compare_host.py and
tests/test_gpu_compare.py: generated models (seeded numpy.random.default_rng) and hand-built threshold cases from small
integer coordinates, in which every quantity of the contract is exact."""
import numpy as np

from tests import compare_model as M

TILE, CHUNK = 256, 256                     # kCmpTile, kCmpChunk of k_compare.hip
DEFAULTS = dict(max_distance=0.01, min_cos2=M.min_cos2_of(10.0), min_overlap=0.5)
# the threshold sets of the model's own test: the defaults, a loose set, nothing but exact copies, everything
PARAM_SETS = [DEFAULTS, dict(max_distance=0.05, min_cos2=M.min_cos2_of(25.0), min_overlap=0.25),
              dict(max_distance=0.0, min_cos2=1.0, min_overlap=1.0), dict(max_distance=1e3, min_cos2=0.0, min_overlap=0.0)]

# (n_Q, n_R, slice_chunks) at the tile, chunk and slice edges; ALL_CHUNKS: one slice that holds every chunk
ALL_CHUNKS = 0xFFFFFFFF
EDGE_SHAPES = [(257, 513, 1), (1, 1025, 2), (513, 1, 0), (256, 256, 1), (0, 40, 0), (40, 0, 0), (1, 1, 0), (63, 511, 1)]
SLICING_SHAPE = (255, 768)
SLICINGS = [1, 2, 3, 0, ALL_CHUNKS]


def model_case(seed, n_q, n_r, box=10.0, on_reference=0.6, twins=0.1):
    """references like the segments of a reconstruction in a box -- a share of them `twins`, near copies of an earlier
    one on a line of their own, a few of them points -- and queries of which a share `on_reference` lies along a
    reference, up to two max_distance off it, the rest anywhere; a few are points.
    -> (q_segs [n_q, 6], q_line, r_segs [n_r, 6], r_line)"""
    rng = np.random.default_rng(seed)
    md = DEFAULTS["max_distance"]

    def unit(n):
        v = rng.normal(size=(n, 3))
        return v / np.maximum(np.linalg.norm(v, axis=1), 1e-12)[:, None]

    a = rng.uniform(0, box, (n_r, 3))
    b = a + rng.uniform(0.3, 3.0, n_r)[:, None] * unit(n_r)
    for i in np.flatnonzero(rng.random(n_r) < twins):
        if i:
            j = rng.integers(0, i)
            a[i] = a[j] + rng.uniform(-0.2, 0.2, 3) * md; b[i] = b[j] + rng.uniform(-0.2, 0.2, 3) * md
    point = rng.random(n_r) < 0.02
    b[point] = a[point]
    r_line = rng.integers(0, max(n_r // 3, 1), n_r).astype(np.uint32)
    p = rng.uniform(0, box, (n_q, 3))
    s = p + rng.uniform(0.1, 2.0, n_q)[:, None] * unit(n_q)
    if n_r and n_q:
        on = np.flatnonzero(rng.random(n_q) < on_reference)
        j = rng.integers(0, n_r, len(on))
        d = b[j] - a[j]
        t1 = rng.uniform(-0.3, 0.7, len(on)); t2 = t1 + rng.uniform(0.2, 0.6, len(on))
        p[on] = a[j] + t1[:, None] * d + rng.uniform(0, 1.2 * md, len(on))[:, None] * unit(len(on))
        s[on] = a[j] + t2[:, None] * d + rng.uniform(0, 1.2 * md, len(on))[:, None] * unit(len(on))
    swap = rng.random(n_q) < 0.5
    p[swap], s[swap] = s[swap].copy(), p[swap].copy()
    point = rng.random(n_q) < 0.01
    s[point] = p[point]
    q_line = rng.integers(0, max(n_r // 3, 1), n_q).astype(np.uint32)
    return (np.ascontiguousarray(np.concatenate([p, s], 1)), q_line, np.ascontiguousarray(np.concatenate([a, b], 1)), r_line)


def large_case():
    """5 000 queries against 3 000 references: past one tile and one chunk in both directions"""
    return model_case(2025, 5000, 3000)


def segs(geometry):
    return np.asarray(geometry, np.float64).reshape(-1, 6)


def hand_cases():
    """-> list of (name, q_segs, q_line, r_segs, r_line, params (with exclude_same_line), expected): expected = one tuple
    per query, (segment, line, n_accepted, distance, overlap), or None where nothing is assigned.  Small integers: every
    product, sum and quotient of the contract is exact (or, where a case is to be rejected, far from its threshold)."""
    out = []
    base = dict(max_distance=5.0, min_cos2=M.min_cos2_of(10.0), min_overlap=0.5, exclude_same_line=False)
    x10 = segs([(0, 0, 0, 10, 0, 0)])
    one = np.array([100], np.uint32)

    def add(name, q, r, par, expected, q_line=None, r_line=None):
        q = segs(q); r = segs(r)
        out.append((name, q, np.arange(len(q), dtype=np.uint32) if q_line is None else np.asarray(q_line, np.uint32), r,
                    np.arange(len(r), dtype=np.uint32) + 100 if r_line is None else np.asarray(r_line, np.uint32), par, expected))

    # d = (10, 0, 0), w = (2, 3, 4): c = (0, -40, 30), m = 2500, L2 = 100, D2 = 25 = 5^2
    add("D2 exactly max_distance^2", [(2, 3, 4, 8, 3, 4)], x10, base, [(0, 100, 1, 5.0, 1.0)])
    add("D2 one step beyond (34 > 25)", [(2, 3, 4, 8, 3, 5)], x10, base, [None])
    add("max_distance one ulp below 5", [(2, 3, 4, 8, 3, 4)], x10, dict(base, max_distance=float(np.nextafter(5.0, 0.0))), [None])
    # t = 0.5 and 1.5: ov = 0.5, hi - lo = 1
    add("frac exactly 0.5", [(5, 1, 0, 15, 1, 0)], x10, base, [(0, 100, 1, 1.0, 0.5)])
    add("frac one step below (0.5 / 1.1)", [(5, 1, 0, 16, 1, 0)], x10, base, [None])
    # dot^2 = 144 = 0.5 * (16 * 18)
    wide = dict(base, min_cos2=0.5)
    add("angle exactly at min_cos2", [(0, 0, 0, 3, 3, 0)], [(0, 0, 0, 4, 0, 0)], wide, [(0, 100, 1, 3.0, 1.0)])
    add("angle one step beyond (144 < 200)", [(0, 0, 0, 3, 4, 0)], [(0, 0, 0, 4, 0, 0)], wide, [None])
    add("reversed queries, reversed references", [(1, 0, 2, 6, 0, 2), (6, 0, 2, 1, 0, 2), (1, 30, 2, 6, 30, 2), (6, 30, 2, 1, 30, 2)],
        [(0, 0, 0, 10, 0, 0), (10, 30, 0, 0, 30, 0)], base,
        [(0, 100, 1, 2.0, 1.0), (0, 100, 1, 2.0, 1.0), (1, 101, 1, 2.0, 1.0), (1, 101, 1, 2.0, 1.0)])
    add("a query that is a point gets nothing", [(5, 0, 0, 5, 0, 0)], x10, base, [None])
    add("a reference that is a point matches nothing", [(1, 1, 1, 2, 1, 1)], [(1, 1, 1, 1, 1, 1), (0, 1, 1, 4, 1, 1)], base,
        [(1, 101, 1, 0.0, 1.0)])
    add("identical references on two lines: the lower index", [(1, 0, 1, 9, 0, 1)], [(0, 40, 0, 10, 40, 0), (0, 0, 0, 10, 0, 0), (0, 0, 0, 10, 0, 0)],
        base, [(1, 7, 2, 1.0, 1.0)], r_line=[5, 7, 9])
    add("the same line is excluded", [(1, 0, 1, 9, 0, 1)], [(0, 0, 0, 10, 0, 0), (0, 0, 0, 10, 0, 0)], dict(base, exclude_same_line=True),
        [(1, 9, 1, 1.0, 1.0)], q_line=[7], r_line=[7, 9])
    return out


def tie_across_slices():
    """the same geometry at references 3 and 600, every other reference far away: with one chunk per slice the tie
    crosses a slice and the merge; index 3 wins and n_accepted = 2"""
    geo = [(0, 5000 + 10 * i, 0, 100, 5000 + 10 * i, 0) for i in range(700)]
    geo[3] = (0, 0, 0, 100, 0, 0); geo[600] = (0, 0, 0, 100, 0, 0)
    lines = np.arange(700, dtype=np.uint32) + 100
    lines[3] = 7; lines[600] = 9
    return segs([(10, 1, 0, 60, 1, 0)]), np.array([0], np.uint32), segs(geo), lines, [(3, 7, 2, 1.0, 1.0)]


def check_expected(name, got, expected):
    assert len(got) == len(expected), name
    for s, e in enumerate(expected):
        g = got[s]
        have = (int(g["segment"]), int(g["line"]), int(g["n_accepted"]), float(g["distance"]), float(g["overlap"]))
        want = (-1, M.NONE, 0, 0.0, 0.0) if e is None else e
        assert have == want, f"{name}: query {s}: {have} != {want}"


def same_matches(got, want, what):
    assert got.dtype == M.LINE_MATCH_DTYPE and len(got) == len(want), f"{what}: {len(got)} results for {len(want)} queries"
    assert got.tobytes() == want.tobytes() or _first_difference(got, want, what)


def _first_difference(got, want, what):
    for name in M.LINE_MATCH_DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = a.view("u%d" % a.dtype.itemsize), b.view("u%d" % b.dtype.itemsize)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{what}: {name} differs in {len(bad)} queries, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
    raise AssertionError(f"{what}: the records differ outside their fields")


def same_summary(got, want, what):
    assert set(got) == set(M.SUMMARY_KEYS), what
    for k in M.SUMMARY_KEYS:
        a, b = got[k], want[k]
        if k.startswith("length"):
            a, b = np.float64(a).view(np.uint64), np.float64(b).view(np.uint64)
        assert a == b, f"{what}: summary {k}: {got[k]!r} != {want[k]!r}"
