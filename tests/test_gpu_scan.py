"""The single-launch scan (k_scan.hip: decoupled look-back, ticket counter, a work space the last tile leaves zeroed) on
its own, through the test hook l3d_selftest_scan, on the MI355X.  The reference is exact integer arithmetic: np.cumsum in
uint64 with a leading 0 (for 8-byte elements on each 32-bit half), tolerance 0.  Every hook call runs its scans back to back
on ONE work space without a host synchronisation between them, so each scan but the first also checks that its
predecessor left the work space zeroed; the hook counts the non-zero words left at the end and the guard words behind the
work space that changed."""
import numpy as np
import pytest

from tests.scan_cases import TILE, WINDOW, selftest_scan

pytestmark = pytest.mark.gpu

N_MAX = 200 * TILE                        # 819 200: the smallest length with a fourth look-back window (tile 193 and up)
# within a block, around one tile, around the tile whose look-back fills all 64 lanes (index 64), the first tile that may
# need a second window (65), three and four windows
LENGTHS = [0, 1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8192, WINDOW * TILE - 1, WINDOW * TILE, WINDOW * TILE + 1,
           65 * TILE + 1, 129 * TILE + 5, N_MAX]
LIMIT = 2**32 - 1


def scaled_to(rng, n, total):
    """n random counts whose sum is exactly `total`"""
    w = rng.integers(0, 10000, n).astype(np.uint64)
    v = w * np.uint64(total) // w.sum()                 # (w * total < 2^64)
    v[:total - int(v.sum())] += np.uint64(1)            # the remainder of the roundings is below n
    assert int(v.sum()) == total and v.max() < 2**32
    return v


def one_per_tile(rng, where):
    v = np.zeros(N_MAX, np.uint64)
    at = {"first": 0, "last": TILE - 1}.get(where)
    idx = np.arange(0, N_MAX, TILE) + (rng.integers(0, TILE, N_MAX // TILE) if at is None else at)
    v[idx] = rng.integers(1, 1000, len(idx))
    return v


def halves(name, rng):
    """the 32-bit half (or the 4-byte input) of a case, as uint64 [N_MAX]"""
    if name == "zeros":                                 # every aggregate is 0 and must still read as "aggregate"
        return np.zeros(N_MAX, np.uint64)
    if name == "ones":
        return np.ones(N_MAX, np.uint64)
    if name.startswith("flags"):                        # as the compactions feed it
        return (rng.random(N_MAX) < float(name[5:])).astype(np.uint64)
    if name.startswith("one_per_tile_"):
        return one_per_tile(rng, name[13:])
    assert name == "limit"
    return scaled_to(rng, N_MAX, LIMIT)


# 8-byte cases: (low half, high half); "limit|flags0.01": the low total is 2^32 - 1 beside a small high one -- a carry out
# of the low half would show in the high one
CASES4 = ["zeros", "ones", "flags0.01", "flags0.5", "flags0.99", "one_per_tile_first", "one_per_tile_last", "one_per_tile_random", "limit"]
CASES8 = [c + "|" + c for c in CASES4[:-1]] + ["limit|flags0.01", "limit|limit", "zeros|one_per_tile_random"]
_cache = {}


def case(elem, name):
    """-> (input, reference: exclusive scan with the total at [N_MAX]); computed once, shared, read-only"""
    if (elem, name) not in _cache:
        rng = np.random.default_rng(20261020 + len(name))
        if elem == 4:
            lo = halves(name, rng)
            data, ref = lo.astype(np.uint32), np.concatenate([[0], np.cumsum(lo, dtype=np.uint64)]).astype(np.uint64)
            assert ref[-1] < 2**32                       # the scan's contract, on the input
            ref = ref.astype(np.uint32)
        else:
            lo, hi = (halves(h, rng) for h in name.split("|"))
            rl, rh = (np.concatenate([[0], np.cumsum(h, dtype=np.uint64)]).astype(np.uint64) for h in (lo, hi))
            assert rl[-1] < 2**32 and rh[-1] < 2**32     # the halves never carry: the scan's contract, on the input
            data, ref = lo | (hi << np.uint64(32)), rl | (rh << np.uint64(32))
        data.setflags(write=False); ref.setflags(write=False)
        _cache[(elem, name)] = (data, ref)
    return _cache[(elem, name)]


def check(data, ref, lengths, in_place, pass_total):
    rc, regions, totals, dirty, guard = selftest_scan(data, lengths, in_place, pass_total)
    what = f"in place {in_place}, total pointer {pass_total}"
    assert rc == 0, what
    for k, n in enumerate(lengths):
        out = regions[k]
        bad = np.flatnonzero(out != ref[:n + 1])
        assert len(bad) == 0, (f"{what}, call {k}, n = {n}: {len(bad)} of {n + 1} outputs differ, first at {bad[0]} "
                               f"(tile {bad[0] // TILE}): {out[bad[0]]:#x} != {ref[bad[0]]:#x}")
        if pass_total:
            assert totals[k] == out[n], f"{what}, call {k}, n = {n}: stored total"
    assert dirty == 0, f"{what}: {dirty} words of the work space are not zero after the last scan"
    assert guard == 0, f"{what}: {guard} guard words behind the work space changed"


@pytest.mark.parametrize("elem,name", [(4, c) for c in CASES4] + [(8, c) for c in CASES8])
def test_scan_equals_the_exact_sums_at_every_length(elem, name):
    data, ref = case(elem, name)
    if "limit" in name:
        assert int(ref[-1]) & 0xFFFFFFFF == LIMIT and (name != "limit|limit" or int(ref[-1]) >> 32 == LIMIT)
        assert name != "limit|flags0.01" or 0 < int(ref[-1]) >> 32 < 20000
    for in_place in (False, True):
        for pass_total in (True, False):
            check(data, ref, LENGTHS, in_place, pass_total)


@pytest.mark.parametrize("elem,name", [(4, "flags0.5"), (4, "zeros"), (4, "limit"), (8, "limit|limit"), (8, "zeros|one_per_tile_random"),
                                       (8, "flags0.5|flags0.5")])
def test_scan_sequences_on_one_work_space(elem, name):
    """a small scan right after a large one reads the state the large one had to zero; the same length twenty times"""
    data, ref = case(elem, name)
    for lengths in ([N_MAX, 1, 65 * TILE + 1, 0, 4097, N_MAX], [65 * TILE + 1] * 20, [4097] * 20):
        for in_place in (False, True):
            for pass_total in (True, False):
                check(data, ref, lengths, in_place, pass_total)
