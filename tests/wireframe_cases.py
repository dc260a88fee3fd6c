"""Cases of the wireframe stage, shared by tests/test_wireframe_host.py and tests/test_gpu_wireframe.py:
generated models (seeded numpy.random.default_rng) and hand-built cases from small integer coordinates (and binary
fractions), in which every quantity of the contract is exact."""
import numpy as np

from tests import wireframe_model as M

TILE, CHUNK = 256, 256                     # kCmpTile, kCmpChunk: k_wireframe.hip walks k_compare's tiling
DEFAULTS = dict(max_distance=0.05, max_extension=0.05, min_sin2=M.min_sin2_of(10.0))
PARAM_SETS = [DEFAULTS, dict(max_distance=0.05, max_extension=0.0, min_sin2=M.min_sin2_of(10.0)),
              dict(max_distance=0.02, max_extension=0.1, min_sin2=M.min_sin2_of(45.0)),
              dict(max_distance=0.05, max_extension=0.05, min_sin2=0.0)]
ALL_CHUNKS = 0xFFFFFFFF

# (n, slice_chunks) at the tile, chunk and slice edges
EDGE_SHAPES = [(257, 1), (513, 2), (256, 1), (1, 0), (0, 0), (63, 1)]
SLICING_N = 768
SLICINGS = [1, 2, 3, 0, ALL_CHUNKS]        # -> 3, 2, 1, 3, 1 slices


def slices_of(n, slice_chunks):
    chunks = -(-n // CHUNK)
    return -(-chunks // min(slice_chunks or 1, chunks)) if n else 0


def skipped_blocks(n, slice_chunks):
    """the workgroups (tile, slice) of the count pass whose slice ends at or below the tile's first query, one by one"""
    if not n:
        return 0
    chunks = -(-n // CHUNK)
    per_slice = min(slice_chunks or 1, chunks) * CHUNK
    n_slices = -(-n // per_slice)
    return sum(min((s + 1) * per_slice, n) - 1 <= q0 for q0 in range(0, n, TILE) for s in range(n_slices))


def model_case(seed, n, box=10.0, corners=0.45, tees=0.12, crosses=0.05, same_line=0.1):
    """segments like those of a reconstruction of a built scene in a box.  A share `corners` start at an end of an earlier
    segment, a share `tees` start on the interior of one and a share `crosses` pass through the interior of one, each
    within a fraction of max_distance; about 2 % are points.  Line indices are sparse (multiples of 3, plus 5); a share
    `same_line` of the attached ones stays on the line of the segment it meets, where the pair must not count.
    -> (segs [n, 6], line [n] uint32)"""
    rng = np.random.default_rng(seed)
    md = DEFAULTS["max_distance"]

    def unit():
        v = rng.normal(size=3)
        return v / max(np.linalg.norm(v), 1e-12)

    a = rng.uniform(0, box, (n, 3))
    b = a + rng.uniform(0.5, 3.0, n)[:, None] * np.array([unit() for _ in range(n)]).reshape(n, 3)
    line = (np.arange(n, dtype=np.uint64) * 3 + 5).astype(np.uint32)
    kind = rng.random(n)
    for i in range(1, n):
        j = int(rng.integers(0, i))
        d = b[j] - a[j]
        noise = rng.uniform(-0.2, 0.2, 3) * md
        length = rng.uniform(0.5, 3.0)
        if kind[i] < corners:
            a[i] = (a[j] if rng.random() < 0.5 else b[j]) + noise
            b[i] = a[i] + length * unit()
        elif kind[i] < corners + tees:
            a[i] = a[j] + rng.uniform(0.2, 0.8) * d + noise
            b[i] = a[i] + length * unit()
        elif kind[i] < corners + tees + crosses:
            m, u = a[j] + rng.uniform(0.2, 0.8) * d + noise, unit()
            a[i] = m - 0.4 * length * u; b[i] = m + 0.6 * length * u
        else:
            continue
        if rng.random() < same_line:
            line[i] = line[j]
    swap = rng.random(n) < 0.3
    a[swap], b[swap] = b[swap].copy(), a[swap].copy()
    point = rng.random(n) < 0.02
    b[point] = a[point]
    return np.ascontiguousarray(np.concatenate([a, b], 1)), line


def large_case():
    """5 000 segments: past one tile and one chunk (the tests assert at least 50 vertices of three or more junctions and
    an X on the model)"""
    return model_case(2027, 5000, box=30.0)


def segs(geometry):
    return np.asarray(geometry, np.float64).reshape(-1, 6)


def no_junction_case(n=600):
    """parallel segments ten units apart, each on a line of its own: nothing meets"""
    return segs([(0, 10 * i, 0, 5, 10 * i, 0) for i in range(n)]), np.arange(n, dtype=np.uint32)


def quiet_tile_case():
    """two tiles: segments 0..255 meet nothing, 256..299 are 22 corners of two -- the write pass of the first tile finds its
    256 counts all zero next to a tile that has junctions"""
    geo = [(0, 10 * i, 0, 5, 10 * i, 0) for i in range(256)]
    for k in range(22):
        geo += [(100, 10 * k, 7, 105, 10 * k, 7), (100, 10 * k, 7, 100, 10 * k, 12)]
    return segs(geo), np.arange(len(geo), dtype=np.uint32)


def diagonal_case():
    """512 parallel segments but for one corner: segment 255, the last query of the first tile, meets segment 256, the first
    reference of the next chunk, and nothing else meets"""
    geo = [(0, 10 * i, 0, 5, 10 * i, 0) for i in range(512)]
    geo[256] = (5, 2550, 0, 5, 2550, 4)
    return segs(geo), np.arange(512, dtype=np.uint32)


def wrap_case():
    """305 x 305 segments from -(i, j, 1) to +(i, j, 1) on distinct lines: every pair meets at the origin, exactly"""
    i, j = np.meshgrid(np.arange(305.0), np.arange(305.0), indexing="ij")
    p = np.stack([i.ravel(), j.ravel(), np.ones(305 * 305)], 1)
    return np.ascontiguousarray(np.concatenate([-p, p], 1)), np.arange(305 * 305, dtype=np.uint32)


HAND_PAR = dict(max_distance=1.0, max_extension=1.0, min_sin2=0.25)
UP = float(np.nextafter(1.0, 2.0))


def cube(side=10):
    """the 12 edges of a cube, x edges first, then y, then z"""
    s = side
    geo = [(0, y, z, s, y, z) for y in (0, s) for z in (0, s)]
    geo += [(x, 0, z, x, s, z) for x in (0, s) for z in (0, s)]
    geo += [(x, y, 0, x, y, s) for x in (0, s) for y in (0, s)]
    return geo


def hand_cases():
    """-> list of (name, segs, line, par, expected): expected = dict of summary counts (every key of it is compared) plus
    kinds / classes (per junction), n_junctions / degree (per vertex), edges (v0, v1, segment) and positions where given"""
    out = []

    def add(name, geometry, line=None, par=None, **expected):
        g = segs(geometry)
        out.append((name, g, np.asarray(range(len(g)) if line is None else line, np.uint32), dict(HAND_PAR, **(par or {})), expected))

    add("the 12 edges of a cube", cube(), n_junctions=24, n_L=24, n_T=0, n_X=0, n_vertices=8, n_junction_vertices=8, n_free_ends=0,
        n_edges=12, n_components=1, largest_component=12, vertex_junctions=[3] * 8, degree=[3] * 8, max_gap=0.0, max_spread=0.0,
        length_total=120.0)
    # the stem stands on the middle of the bar: one junction vertex, three free ends, the bar in two edges
    add("a T junction", [(0, 0, 0, 10, 0, 0), (5, 0, 0, 5, 8, 0)], n_junctions=1, n_T=1, kinds=[2], classes=[(2, 0)], n_vertices=4,
        n_free_ends=3, n_edges=3, n_components=1, degree=[3, 1, 1, 1], edges=[(1, 0, 0), (0, 2, 0), (0, 3, 1)],
        positions=[(5, 0, 0), (0, 0, 0), (10, 0, 0), (5, 8, 0)])
    add("an X crossing", [(0, 0, 0, 10, 0, 0), (5, -5, 0, 5, 5, 0)], n_junctions=1, n_X=1, kinds=[4], classes=[(2, 2)], n_vertices=5,
        n_free_ends=4, n_edges=4, degree=[4, 1, 1, 1, 1], n_components=1)
    add("three lines through one interior point", [(0, 0, 0, 10, 0, 0), (5, -5, 0, 5, 5, 0), (5, 0, -5, 5, 0, 5)], n_junctions=3, n_X=3,
        n_junction_vertices=1, vertex_junctions=[3, 0, 0, 0, 0, 0, 0], degree=[6, 1, 1, 1, 1, 1, 1], n_edges=6, n_components=1)
    # ta = 4 and 5 on the long segment; the two that cross it are parallel and meet each other nowhere
    add("two interior attachments exactly max_distance apart join", [(0, 0, 0, 16, 0, 0), (4, -4, 0, 4, 4, 0), (5, -4, 0, 5, 4, 0)],
        n_junctions=2, n_X=2, n_junction_vertices=1, positions=[(4.5, 0, 0)], max_spread=0.5, n_edges=6, degree=[6, 1, 1, 1, 1, 1, 1])
    x = float(np.nextafter(5.0, 6.0))
    add("... and one ulp further they do not", [(0, 0, 0, 16, 0, 0), (4, -4, 0, 4, 4, 0), (x, -4, 0, x, 4, 0)],
        n_junctions=2, n_X=2, n_junction_vertices=2, max_spread=0.0, n_edges=7)
    add("a gap of exactly max_distance", [(0, 0, 0, 10, 0, 0), (5, -5, 1, 5, 5, 1)], n_junctions=1, n_X=1, max_gap=1.0, positions=[(5, 0, 0.5)])
    add("... and the next gap beyond it", [(0, 0, 0, 10, 0, 0), (5, -5, UP, 5, 5, UP)], n_junctions=0, n_vertices=4, n_edges=2, n_components=2)
    # sa = 9 / 8: the meeting point lies max_extension beyond P2 of the first, in the middle of the second
    add("an extension of exactly max_extension", [(0, 0, 0, 8, 0, 0), (9, -4, 0, 9, 4, 0)], n_junctions=1, n_T=1, classes=[(1, 2)],
        n_vertices=4, n_free_ends=3, n_edges=3, positions=[(9, 0, 0)])
    x = float(np.nextafter(9.0, 10.0))
    add("... and the next one beyond it", [(0, 0, 0, 8, 0, 0), (x, -4, 0, x, 4, 0)], n_junctions=0, n_edges=2)
    add("parallel and anti-parallel segments", [(0, 0, 0, 10, 0, 0), (0, 0, 0, 10, 0, 0), (10, 0, 0, 0, 0, 0), (3, 0, 0, 20, 0, 0)],
        n_junctions=0, n_vertices=8, n_edges=4, n_components=4)
    add("skew lines further apart than max_distance", [(0, 0, 0, 10, 0, 0), (5, -5, 2, 5, 5, 2)], n_junctions=0, n_edges=2)
    add("two segments of one line", [(0, 0, 0, 10, 0, 0), (5, -5, 0, 5, 5, 0)], line=[3, 3], n_junctions=0, n_edges=2, n_components=2)
    # (8, 0, 0) against (4, 4, 0): A C = 2048, den = 1024: sin^2 = 1 / 2 exactly
    add("min_sin2 at equality", [(0, 0, 0, 8, 0, 0), (0, 0, 0, 4, 4, 0)], par=dict(min_sin2=0.5), n_junctions=1, n_L=1, classes=[(0, 0)])
    add("... and just above it", [(0, 0, 0, 8, 0, 0), (0, 0, 0, 4, 4, 0)], par=dict(min_sin2=float(np.nextafter(0.5, 1.0))), n_junctions=0)
    # L = 1.5 <= 2 max_extension: every point of it is within reach of both ends.  t = 0.75: t * 2 == L, P1; t = 1: P2
    add("a short segment takes the nearer end", [(0, 0, 0, 1.5, 0, 0), (0.75, -4, 0, 0.75, 4, 0), (1, -4, 0, 1, 4, 0)],
        n_junctions=2, n_T=2, classes=[(0, 2), (1, 2)], n_junction_vertices=2, n_free_ends=4, n_edges=5)
    add("a point segment is counted and otherwise absent", [(0, 0, 0, 10, 0, 0), (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 10, 0)],
        n_segments=3, n_point_segments=1, n_junctions=1, n_L=1, pairs=[(0, 2)], n_vertices=3, n_edges=2, length_total=20.0)
    add("sparse line indices", [(0, 0, 0, 10, 0, 0), (0, 0, 0, 0, 10, 0), (0, 0, 0, 0, 0, 10)], line=[7, 1_000_000, 4_000_000_000],
        n_junctions=3, n_L=3, n_junction_vertices=1, n_vertices=4, edge_lines=[7, 1_000_000, 4_000_000_000])
    add("the empty model", [], n_segments=0, n_junctions=0, n_vertices=0, n_edges=0, n_components=0, largest_component=0, length_total=0.0)
    return out


def check_expected(name, got, expected):
    """got = the dict of a wireframe"""
    J, V, E, s = got["junctions"], got["vertices"], got["edges"], got["summary"]
    for k, want in expected.items():
        if k in M.SUMMARY_KEYS:
            assert s[k] == want, f"{name}: {k} = {s[k]!r}, expected {want!r}"
    assert s["n_junctions"] == len(J) and s["n_vertices"] == len(V) and s["n_edges"] == len(E), name
    assert s["n_L"] + s["n_T"] + s["n_X"] == len(J) and s["n_junction_vertices"] + s["n_free_ends"] == len(V), name
    assert int(V["degree"].sum()) == 2 * len(E), name
    if "kinds" in expected:
        assert list(J["kind"]) == expected["kinds"], f"{name}: kinds {list(J['kind'])}"
    if "classes" in expected:
        assert [(int(j["class_a"]), int(j["class_b"])) for j in J] == expected["classes"], f"{name}: classes {J[['class_a', 'class_b']]}"
    if "pairs" in expected:
        assert [(int(j["a"]), int(j["b"])) for j in J] == expected["pairs"], name
    if "vertex_junctions" in expected:
        assert list(V["n_junctions"]) == expected["vertex_junctions"], f"{name}: {list(V['n_junctions'])}"
    if "degree" in expected:
        assert list(V["degree"]) == expected["degree"], f"{name}: degrees {list(V['degree'])}"
    if "edges" in expected:
        assert [(int(e["v0"]), int(e["v1"]), int(e["segment"])) for e in E] == expected["edges"], f"{name}: edges {E}"
    if "edge_lines" in expected:
        assert list(E["line"]) == expected["edge_lines"], name
    for k, p in enumerate(expected.get("positions", [])):
        assert tuple(V["P"][k]) == tuple(float(x) for x in p), f"{name}: vertex {k} at {V['P'][k]}"


def same_result(got, want, what):
    """every output byte: junctions, vertices, edges and the summary"""
    for name in ("junctions", "vertices", "edges"):
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
