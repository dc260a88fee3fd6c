"""Cases of the plane detection, shared by tests/test_planes_host.py and tests/test_gpu_planes.py: generated
models with planted planes (seeded numpy.random.default_rng) and hand-built cases from small integer coordinates and
binary fractions, in which the quantities the tests pin are exact."""
import numpy as np

from tests import planes_model as M

TILE, CHUNK = 256, 256                     # kCmpTile, kCmpChunk: k_pl_score walks k_compare's tiling
MD = 0.05                                  # max_distance of the generated cases
PAR = M.params(MD, min_segments=8)     # (four clutter segments lie in one plane by chance often enough)
ALL_CHUNKS = 0xFFFFFFFF
EDGE_N = (1, 63, 256, 257, 513)
EDGE_SLICE_CHUNKS = (0, 1, 2, 3)
SLICING_N = 768
SLICINGS = [1, 2, 3, 0, ALL_CHUNKS]        # -> 3, 2, 1, 3, 1 slices
UP = float(np.nextafter(0.5, 1.0))


def slices_of(n, slice_chunks):
    chunks = -(-n // CHUNK)
    return -(-chunks // min(slice_chunks or 1, chunks)) if n else 0


def segs(geometry):
    return np.asarray(geometry, np.float64).reshape(-1, 6)


# ---- generated: planted planes and clutter ------------------------------------------------------------------------------
def planted_case(seed, k, lines_per_family, n, box=30.0, size=6.0, noise=MD / 8, points=0.02):
    """k planes, each a grid of two families of `lines_per_family` lines, a segment each on a line of its own, across a
    size x size rectangle on a random plane in a box; every end point is moved by less than `noise` (< MD / 4) along each
    axis of the plane's frame.  The other n - 2 k lines_per_family segments are clutter, about 2 % of them points.  The
    order of the segments is shuffled.  -> (segs [n, 6], line [n] uint32, planted: k arrays of segment indices)"""
    rng = np.random.default_rng(seed)
    assert noise < MD / 4 and n >= 2 * k * lines_per_family
    rows, label = [], []
    for p in range(k):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        U, V, N = q[:, 0], q[:, 1], q[:, 2]
        centre = rng.uniform(0.3 * box, 0.7 * box, 3)
        at = (np.arange(lines_per_family) + 0.5) / lines_per_family * size - size / 2      # where a family's lines lie
        for along, across in ((U, V), (V, U)):
            for t in at:
                ends = []
                for s in (-size / 2, size / 2):
                    d = rng.uniform(-noise, noise, 3)
                    ends.append(centre + (s + d[0]) * along + (t + d[1]) * across + d[2] * N)
                rows.append(np.concatenate(ends)); label.append(p)
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
    return out, line, [np.flatnonzero(label == p) for p in range(k)]


def sized_case(n):
    """a planted case of exactly n segments: one plane below 64 segments, else two"""
    if n < 8:
        return planted_case(500 + n, 0, 0, n)
    k = 1 if n < 64 else 2
    return planted_case(500 + n, k, max(2, min(10, n // (8 * k))), n, box=12.0)


def large_case():
    """about 5 000 segments: six planes of 2 x 20 lines in 4 760 clutter segments"""
    return planted_case(2031, 6, 20, 5000)


def admitted(result, planted):
    """the issue's admission rule -> a message for the first condition the result misses, else None"""
    P, Mb = result["planes"], result["members"]
    if len(P) > len(planted) + 1:
        return f"{len(P)} planes for {len(planted)} planted"
    of_plane = [set(Mb["segment"][Mb["plane"] == p].tolist()) for p in range(len(P))]
    for i, want in enumerate(planted):
        best = max((len(m & set(want.tolist())) for m in of_plane), default=0)
        if best * 10 < 9 * len(want):
            return f"planted plane {i}: {best} of {len(want)} segments are members of one plane"
    return None


# ---- hand-built ---------------------------------------------------------------------------------------------------------
def cube(side=1):
    """the 12 edges of a cube, x edges first, then y, then z"""
    s = side
    geo = [(0, y, z, s, y, z) for y in (0, s) for z in (0, s)]
    geo += [(x, 0, z, x, s, z) for x in (0, s) for z in (0, s)]
    geo += [(x, y, 0, x, y, s) for x in (0, s) for y in (0, s)]
    return geo


def comb(teeth, origin=(100.0, 50.0, 50.0)):
    """a spine along x and `teeth` teeth standing on it one unit apart, alternately along y and along z, each on a line of
    its own: exactly `teeth` junctions, spine with tooth, in two planes (the y teeth with the spine, the z teeth with it)"""
    ox, oy, oz = origin
    geo = [(ox - 1, oy, oz, ox + teeth, oy, oz)]
    for t in range(teeth):
        geo.append((ox + t, oy, oz, ox + t, oy + 4, oz) if t % 2 == 0 else (ox + t, oy, oz, ox + t, oy, oz + 4))
    return geo


def dead_fan(n=256):
    """n + 1 segments from the origin whose n junctions are all dead: a = s (1, -1, 0) with s = 2^-300 and b_k =
    y_k (1, 1, -2) with y_k = (1 + k / 1024) 2^-239.  A C = 12 s^2 y^2 rounds to 2^-1074, so den > 0 and the pair is a
    junction with sa = sb = 0; every component of ea x eb is 2 s y, whose square lies below 2^-1075 and rounds to 0."""
    s = 2.0 ** -300
    geo = [(0, 0, 0, s, -s, 0)]
    for k in range(n):
        y = (1 + k / 1024) * 2.0 ** -239
        geo.append((0, 0, 0, y, y, -2 * y))
    return geo


def tilted_geometry():
    """The plane z = 0 holds S0 along x and S1..S6 along y at x = 0..5, and Ty along y below the origin.  Tx leaves the
    origin along (40, 0, 9) / 8 (length 5.125) and U1 stands on its end along y (length 5): with Ty they span the plane
    through the y axis whose normal is (9, 0, -40) / 41, at 9 x / 41 from the point (x, y, 0)."""
    geo = [(0, 0, 0, 5, 0, 0)] + [(x, 0, 0, x, 8, 0) for x in range(6)]
    geo += [(0, -2.125, 0, 0, 0, 0), (0, 0, 0, 5, 0, 1.125), (5, 0, 1.125, 5, 5, 1.125)]
    return geo


def three_planes_geometry():
    """three rectangles that share the segment along z: in y = 0, in x = 0 and in x = y"""
    geo = [(0, 0, 0, 0, 0, 8)]
    for x, y in ((8, 0), (0, 8), (8, 8)):
        geo += [(0, 0, 0, x, y, 0), (x, y, 0, x, y, 8), (0, 0, 8, x, y, 8)]
    return geo


def hand_cases():
    """-> list of (name, segs, line, par, expected): expected = summary counts (every key of it is compared) plus
    counts (per hypothesis), plane_hypotheses, plane_members (per plane), seg_planes where given"""
    out = []

    def add(name, geometry, par, line=None, **expected):
        g = segs(geometry)
        out.append((name, g, np.asarray(range(len(g)) if line is None else line, np.uint32), par, expected))

    # a corner of the cube gives three hypotheses, a face has four corners: the first is accepted, three are dropped
    cube_par = M.params(0.25, min_sin2=0.25)
    add("the 12 edges of a cube", cube(), cube_par, n_hypotheses=24, n_dead=0, n_candidates=24, counts=[4] * 24, n_planes=6,
        n_tested=6, n_dropped=18, n_rejected=0, n_memberships=24, seg_planes=[2] * 12, n_segments_in_planes=12,
        n_segments_in_several=12, truncated=0, length_total=12.0, length_in_planes=12.0, scale_exponent=48, max_rms=0.0,
        plane_sizes=[4] * 6, ascending_hypotheses=True)
    add("max_tests reached", cube(), dict(cube_par, max_tests=3), n_planes=3, n_tested=3, truncated=1, n_rejected=0)
    add("max_planes reached", cube(), dict(cube_par, max_planes=2), n_planes=2, n_tested=2, truncated=0, n_memberships=8)
    add("point segments are counted and never members", cube() + [(0.5, 0.5, 0, 0.5, 0.5, 0), (0, 0, 0, 0, 0, 0)], cube_par,
        n_segments=14, n_point_segments=2, n_hypotheses=24, counts=[4] * 24, n_planes=6, seg_planes=[2] * 12 + [0, 0], length_total=12.0)
    # the tilted plane shares Ty, S1, S2, S3 (26.125) with z = 0 and has Tx and U1 (10.125) to itself: rejected, once for
    # each of the three junctions that span it (S1 with Tx, Ty with Tx, Tx with U1)
    add("a tilted copy is rejected", tilted_geometry(), M.params(0.5, junction_distance=0.125, min_sin2=0.03), n_planes=1, n_rejected=3,
        plane_sizes=[8], plane_members=[[0, 1, 2, 3, 4, 5, 6, 7]])
    # at max_distance 1 / 8 it shares Ty and S1 (10.125) and has 10.125 to itself: 2 common == weight, accepted
    add("2 common == weight is accepted", tilted_geometry(), M.params(0.125, min_sin2=0.03), n_planes=2, n_rejected=0,
        plane_sizes=[8, 4], plane_members=[[0, 1, 2, 3, 4, 5, 6, 7], [1, 7, 8, 9]], seg_planes=[1, 2, 1, 1, 1, 1, 1, 2, 1, 1])
    square = [(0, 0, 0, 8, 0, 0), (8, 0, 0, 8, 8, 0), (8, 8, 0, 0, 8, 0), (0, 8, 0, 0, 0, 0)]
    thr = M.params(0.5, junction_distance=0.25, min_sin2=0.25)
    add("an end point at exactly max_distance is an inlier", square + [(2, 2, 0.5, 6, 2, -0.5)], thr, n_planes=1, plane_sizes=[5],
        counts=[5] * 4)
    add("... and the next one beyond it is not", square + [(2, 2, UP, 6, 2, -0.5)], thr, n_planes=1, plane_sizes=[4], counts=[4] * 4)
    add("a segment in three planes", three_planes_geometry(), M.params(0.25, min_sin2=0.25), n_planes=3, plane_sizes=[4, 4, 4],
        seg_planes=[3] + [1] * 9, n_segments_in_several=1, n_rejected=0)
    add("a dead hypothesis", dead_fan(1), M.params(0.25, min_segments=1), n_hypotheses=1, n_dead=1, n_candidates=0, n_planes=0, counts=[0])
    add("no junction", [(0, 10 * i, 0, 5, 10 * i, 0) for i in range(6)], M.params(0.25), n_hypotheses=0, n_planes=0, n_segments=6,
        length_total=30.0)
    return out


def check_expected(name, got, expected):
    P, Mb, s = got["planes"], got["members"], got["summary"]
    for k, want in expected.items():
        if k in M.SUMMARY_KEYS:
            assert s[k] == want, f"{name}: {k} = {s[k]!r}, expected {want!r}"
    assert s["n_planes"] == len(P) and s["n_memberships"] == len(Mb) == int(got["seg_planes"].sum()), name
    assert s["n_hypotheses"] == len(got["scores"]) and s["n_tested"] == s["n_planes"] + s["n_rejected"], name
    if "counts" in expected:
        assert got["scores"]["count"].tolist() == expected["counts"], f"{name}: counts {got['scores']['count'].tolist()}"
    if "plane_sizes" in expected:
        assert P["n_segments"].tolist() == expected["plane_sizes"], f"{name}: sizes {P['n_segments'].tolist()}"
    if expected.get("ascending_hypotheses"):
        assert (np.diff(P["hypothesis"].astype(np.int64)) > 0).all(), name
    if "plane_members" in expected:
        assert [Mb["segment"][Mb["plane"] == p].tolist() for p in range(len(P))] == expected["plane_members"], f"{name}: members {Mb}"
    if "seg_planes" in expected:
        assert got["seg_planes"].tolist() == expected["seg_planes"], f"{name}: seg_planes {got['seg_planes'].tolist()}"


def same_result(got, want, what):
    """every output byte: planes, members, the per-segment counts, the scores of every hypothesis and the summary"""
    for name in ("planes", "members", "seg_planes", "scores"):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name}: {a.dtype}{a.shape} != {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(1))
            raise AssertionError(f"{what}: {name} differs in {len(bad)} rows, first {bad[0]}: {a[bad[0]]} != {b[bad[0]]}")
    same_summary(got["summary"], want["summary"], what)


def same_summary(got, want, what):
    assert set(got) == set(M.SUMMARY_KEYS), what
    for k in M.SUMMARY_KEYS:
        a, b = got[k], want[k]
        if isinstance(b, float):
            a, b = np.float64(a).view(np.uint64), np.float64(b).view(np.uint64)
        assert a == b, f"{what}: summary {k}: {got[k]!r} != {want[k]!r}"
