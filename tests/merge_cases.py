"""Cases of the merging of near-duplicate 3D lines, shared by tests/test_merge_host.py and
tests/test_gpu_merge.py: generated models (seeded numpy.random.default_rng) and hand-built cases from small integer
coordinates, in which every quantity of the contract is exact."""
import numpy as np

from tests import compare_cases as Cs
from tests import merge_model as M

TILE, CHUNK = Cs.TILE, Cs.CHUNK            # kCmpTile, kCmpChunk: k_merge.hip walks k_compare's tiling
DEFAULTS = Cs.DEFAULTS
PARAM_SETS = Cs.PARAM_SETS                 # §18's four threshold sets
ALL_CHUNKS = Cs.ALL_CHUNKS

# (n, slice_chunks) at the tile, chunk and slice edges
EDGE_SHAPES = [(257, 1), (513, 2), (256, 1), (1, 0), (0, 0), (63, 1)]
SLICING_N = 768
SLICINGS = [1, 2, 3, 0, ALL_CHUNKS]        # -> 3, 2, 1, 3, 1 slices


def model_case(seed, n, box=10.0, twins=0.12, inside=0.06, chains=0.0, same_line=0.3):
    """segments like those of a reconstruction in a box.  A share `twins` are near copies of an earlier segment, within
    max_distance of it; a share `inside` are short pieces lying along an earlier, longer one (accepted one way only); a
    share `chains` continue an earlier one along its own line, shifted by 0.4 of its length (A~B~C without A~C); about 2 %
    are points.  Line indices are sparse (multiples of 3, plus 5); a share `same_line` of the copies stays on the line of
    its original, where the pair must not count.  -> (segs [n, 6], line [n] uint32)"""
    rng = np.random.default_rng(seed)
    md = DEFAULTS["max_distance"]

    def unit(k):
        v = rng.normal(size=(k, 3))
        return v / np.maximum(np.linalg.norm(v, axis=1), 1e-12)[:, None]

    a = rng.uniform(0, box, (n, 3))
    b = a + rng.uniform(0.3, 3.0, n)[:, None] * unit(n)
    line = (np.arange(n, dtype=np.uint64) * 3 + 5).astype(np.uint32)
    kind = rng.random(n)
    for i in range(1, n):
        j = int(rng.integers(0, i))
        d = b[j] - a[j]
        if kind[i] < twins:
            a[i] = a[j] + rng.uniform(-0.2, 0.2, 3) * md; b[i] = b[j] + rng.uniform(-0.2, 0.2, 3) * md
        elif kind[i] < twins + inside:
            t = rng.uniform(0.1, 0.5)
            a[i] = a[j] + t * d + rng.uniform(-0.2, 0.2, 3) * md; b[i] = a[j] + (t + 0.3) * d + rng.uniform(-0.2, 0.2, 3) * md
        elif kind[i] < twins + inside + chains:
            a[i] = a[j] + 0.4 * d; b[i] = b[j] + 0.4 * d
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
    """5 000 segments: past one tile and one chunk, with components of every small size (the tests assert at least 50
    merged components and one of four lines or more)"""
    return model_case(2026, 5000, box=30.0, twins=0.06, inside=0.03, chains=0.03)


def no_pair_case(n=600):
    """parallel segments ten units apart, each on a line of its own: no pair is accepted"""
    geo = [(0, 10 * i, 0, 5, 10 * i, 0) for i in range(n)]
    return segs(geo), np.arange(n, dtype=np.uint32)


def quiet_tile_case():
    """two tiles of queries: segments 0..255 far from everything, 256..299 in pairs of copies -- the write pass of the
    first tile finds its 256 counts all zero next to a tile that has pairs"""
    geo = [(0, 10 * i, 0, 5, 10 * i, 0) for i in range(256)]
    for k in range(22):
        geo += [(100, 10 * k, 7, 105, 10 * k, 7)] * 2
    return segs(geo), np.arange(len(geo), dtype=np.uint32)


def segs(geometry):
    return np.asarray(geometry, np.float64).reshape(-1, 6)


HAND_PAR = dict(max_distance=5.0, min_cos2=M.min_cos2_of(10.0), min_overlap=0.5)


def hand_cases():
    """-> list of (name, segs, line, expected): expected = dict(n_pairs, line_map, labels, n_members, max_offset, segs_out,
    line_out), every entry exact under HAND_PAR.  Small integers (and quarters): every product, sum and quotient of the
    contract is exact."""
    out = []

    def add(name, geometry, line, **expected):
        out.append((name, segs(geometry), np.asarray(line, np.uint32), expected))

    # A in B and B in C overlap by 0.6, A in C and C in A by 0.2: a chain.  c = (9, 0, 0), u = (1, 0, 0)
    add("a chain A~B~C without A~C is one component of three", [(0, 0, 0, 10, 0, 0), (4, 0, 0, 14, 0, 0), (8, 0, 0, 18, 0, 0)], [1, 2, 3],
        n_pairs=4, line_map=[0, 0, 0], labels=[1], n_members=[3], max_offset=[0.0], segs_out=[(0, 0, 0, 18, 0, 0)], line_out=[0])
    # the short one lies in the long one (overlap 1), the long one in the short one by a third only.  W = 40, c = (15, 1, 0);
    # offsets: sqrt(226 - 225) = 1 and sqrt(34 - 25) = 3
    add("an acceptance in one direction merges", [(0, 0, 0, 30, 0, 0), (10, 4, 0, 20, 4, 0)], [3, 9],
        n_pairs=1, line_map=[0, 0], labels=[3], n_members=[2], max_offset=[3.0], segs_out=[(0, 1, 0, 30, 1, 0)], line_out=[0])
    add("two segments of one line are never paired", [(0, 0, 0, 10, 0, 0), (0, 0, 0, 10, 0, 0)], [5, 5],
        n_pairs=0, line_map=[0, 0], labels=[5], n_members=[1], max_offset=[0.0],
        segs_out=[(0, 0, 0, 10, 0, 0), (0, 0, 0, 10, 0, 0)], line_out=[0, 0])
    add("sparse line indices are numbered by ascending label", [(0, 0, 0, 10, 0, 0), (0, 100, 0, 10, 100, 0), (0, 0, 0, 10, 0, 0)],
        [4_000_000_000, 7, 1_000_000], n_pairs=2, line_map=[1, 0, 1], labels=[7, 1_000_000], n_members=[1, 2], max_offset=[0.0, 0.0],
        segs_out=[(0, 100, 0, 10, 100, 0), (0, 0, 0, 10, 0, 0)], line_out=[0, 1])
    # c = (5, 1, 0); the reversed member counts with s = -1: dsum = (20, 0, 0)
    add("a reversed member", [(0, 0, 0, 10, 0, 0), (10, 2, 0, 0, 2, 0)], [1, 2],
        n_pairs=2, line_map=[0, 0], labels=[1], n_members=[2], max_offset=[1.0], segs_out=[(0, 1, 0, 10, 1, 0)], line_out=[0])
    # equal lengths: segment 0 leads and the fused segment runs its way, from x = 10 down to 0
    add("a leader tie goes to the smaller index", [(10, 0, 0, 0, 0, 0), (0, 2, 0, 10, 2, 0)], [1, 2],
        n_pairs=2, line_map=[0, 0], labels=[1], n_members=[2], max_offset=[1.0], segs_out=[(10, 1, 0, 0, 1, 0)], line_out=[0])
    # W = 40, c = (15, 0.25, 0); intervals [-15, -5] twice, [-5, 5], [15, 25]: the third touches and joins, the fourth does not
    add("touching intervals join, a gap stays two segments",
        [(0, 0, 0, 10, 0, 0), (0, 1, 0, 10, 1, 0), (10, 0, 0, 20, 0, 0), (30, 0, 0, 40, 0, 0)], [2, 3, 2, 3],
        n_pairs=2, line_map=[0, 0, 0, 0], labels=[2], n_members=[2], max_offset=[0.75],
        segs_out=[(0, 0.25, 0, 20, 0.25, 0), (30, 0.25, 0, 40, 0.25, 0)], line_out=[0, 0])
    add("a point segment leaves a fused line and stays in an untouched one",
        [(0, 0, 0, 10, 0, 0), (0, 0, 0, 10, 0, 0), (5, 0, 0, 5, 0, 0), (0, 50, 0, 10, 50, 0), (3, 50, 0, 3, 50, 0)], [1, 2, 1, 9, 9],
        n_pairs=2, line_map=[0, 0, 0, 1, 1], labels=[1, 9], n_members=[2, 1], max_offset=[0.0, 0.0],
        segs_out=[(0, 0, 0, 10, 0, 0), (0, 50, 0, 10, 50, 0), (3, 50, 0, 3, 50, 0)], line_out=[0, 1, 1])
    add("the empty model", [], [], n_pairs=0, line_map=[], labels=[], n_members=[], max_offset=[], segs_out=[], line_out=[])
    return out


def check_expected(name, got, expected):
    """got = (segs_out, line_out, line_map, line_info, summary)"""
    segs_out, line_out, line_map, info, summary = got
    assert summary["n_pairs"] == expected["n_pairs"], f"{name}: {summary['n_pairs']} pairs"
    assert list(line_map) == expected["line_map"], f"{name}: line_map {list(line_map)}"
    assert list(info["label"]) == expected["labels"] and list(info["n_members"]) == expected["n_members"], f"{name}: {info}"
    assert list(info["max_offset"]) == expected["max_offset"], f"{name}: max_offset {list(info['max_offset'])}"
    assert list(line_out) == expected["line_out"], f"{name}: line_out {list(line_out)}"
    assert np.array_equal(segs_out, segs(expected["segs_out"])), f"{name}: segments {segs_out}"
    assert summary["n_lines_out"] == len(expected["labels"]) and summary["n_segments_out"] == len(expected["line_out"]), name
    assert summary["n_merged_components"] == sum(m >= 2 for m in expected["n_members"]), name
    assert summary["largest_component"] == max(expected["n_members"], default=0), name


def same_result(got, want, what):
    """every output byte: segments, lines, the map, the line records and the summary"""
    names = ("segs_out", "line_out", "line_map", "line_info")
    for k, name in enumerate(names):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name}: {a.dtype}{a.shape} != {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(1))
            raise AssertionError(f"{what}: {name} differs in {len(bad)} rows, first {bad[0]}: {a[bad[0]]} != {b[bad[0]]}")
    same_summary(got[4], want[4], what)


def same_summary(got, want, what):
    assert set(got) == set(M.SUMMARY_KEYS), what
    for k in M.SUMMARY_KEYS:
        a, b = got[k], want[k]
        if isinstance(b, float):
            a, b = np.float64(a).view(np.uint64), np.float64(b).view(np.uint64)
        assert a == b, f"{what}: summary {k}: {got[k]!r} != {want[k]!r}"
