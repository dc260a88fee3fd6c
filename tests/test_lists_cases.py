"""The host model of the hypothesis-list lengths (tests/lists_cases.py) on hand-made slot arrays: the GPU tests of
tests/test_gpu_lists.py assert their shape conditions through it, so it is checked here against counts made by hand."""
import numpy as np

from line3dpp_amd._lib import EMPTY, SLOT_DTYPE
from tests import lists_cases as LC

A, AI = LC.SLOT_ALIVE, LC.SLOT_ALIVE | LC.SLOT_INV_ALIVE


def _slots(entries):
    """[(target segment or None, flags)] -> (slot records, alive stream)"""
    s = np.zeros(len(entries), SLOT_DTYPE)
    s["tgt_seg"] = [EMPTY if t is None else t for t, _ in entries]
    s["flags"] = [f for _, f in entries]
    alive = np.array([t is not None and (f & LC.SLOT_ALIVE) != 0 for t, f in entries], bool)
    return s, alive


def test_three_views_uniform_rows_with_dead_slots():
    """views 0 (2 segments), 1 (3), 2 (2); pairs (0,1), (0,2), (1,2) with rows of 2 slots.  View 2 has no outgoing pair
    (all its hypotheses are inverse), view 0 no incoming one (all fresh); dead slots: empty, rejected by the source's
    orientation filter (flags 0), alive but rejected by the target's (kSlotAlive only: fresh, never inverse)."""
    entries = [
        # pair (0,1): row 0, row 1
        (2, AI), (0, A), (1, 0), (None, 0),
        # pair (0,2): row 0, row 1
        (1, AI), (None, 0), (1, AI), (0, AI),
        # pair (1,2): rows 0, 1, 2
        (0, AI), (1, A), (None, 0), (None, 0), (1, 0), (1, AI),
    ]
    slots, alive = _slots(entries)
    m = LC.list_lengths([(0, 1), (0, 2), (1, 2)], [0, 4, 8], {0: 2, 1: 3, 2: 2}, slots, alive, 2)
    assert m["seg_base"] == {0: 0, 1: 2, 2: 5} and m["cams"] == [0, 1, 2]
    #                         view 0    view 1       view 2
    assert m["n_fresh"].tolist() == [3, 2, 2, 0, 1, 0, 0]
    assert m["n_inv"].tolist() == [0, 0, 0, 0, 1, 2, 3]
    assert m["L"].tolist() == [3, 2, 2, 0, 2, 2, 3]
    assert int(m["L"].sum()) == int(alive.sum()) + 6          # every alive slot once, every inverse-alive one twice


def test_inverse_matches_only_go_to_later_views():
    """a pair whose target is the EARLIER view (asymmetric neighbour lists) hands nothing over, whatever its flags say;
    sparse cam ids are ordered by value"""
    slots, alive = _slots([(0, AI), (1, AI)])
    m = LC.list_lengths([(7, 3)], [0], {3: 2, 7: 1}, slots, alive, 2)
    assert m["seg_base"] == {3: 0, 7: 2}
    assert m["n_fresh"].tolist() == [0, 0, 2] and m["n_inv"].tolist() == [0, 0, 0]


def test_ragged_rows_of_the_keep_all_mode():
    """kNN <= 0: the slot buffer holds the matches back to back and every slot names its row; rows and pairs without a
    match take no room"""
    rows = LC.ragged_slot_rows([[2, 0, 1], [0, 0, 0], [3, 0]])
    assert rows.tolist() == [0, 0, 2, 0, 0, 0]
    slots, alive = _slots([(1, AI), (0, A), (1, AI),       # pair (0,1): row 0 has two matches, row 2 one
                           (0, AI), (1, 0), (2, AI)])      # pair (1,2): row 0 has three, one of them rejected; row 1 none
    m = LC.list_lengths([(0, 1), (0, 2), (1, 2)], [0, 3, 3], {0: 3, 1: 2, 2: 3}, slots, alive, 0, rows)
    assert m["n_fresh"].tolist() == [2, 0, 1, 2, 0, 0, 0, 0]
    assert m["n_inv"].tolist() == [0, 0, 0, 0, 2, 1, 0, 1]
    assert m["L"].tolist() == [2, 0, 1, 2, 2, 1, 0, 1]


def test_tier_counts_at_the_capacities():
    L = [0, 1, 2, 128, 129, 256, 257, 512, 513, 1024, 1025, 65535]
    assert LC.tier_counts(L, 128) == dict(tier1=4, tier2=2, tier4=2, huge=4)
    assert LC.tier_counts(L, 256) == dict(tier1=6, tier2=2, tier4=2, huge=2)
    assert sum(LC.tier_counts(L, 128).values()) == len(L)


def test_pass_base_from_estimate_and_measurement():
    # first call: 1.5 n_slots / G, truncated: 96 is still narrow, 97 wide
    assert LC.pass_base(6400, 100) == 128 and LC.pass_base(6466, 100) == 128 and LC.pass_base(6467, 100) == 256
    # later calls: the measured mean of the call before, whatever the slots say
    assert LC.pass_base(10**6, 100, entries_before=9699) == 128 and LC.pass_base(10, 100, entries_before=9700) == 256


def test_drop_segments_and_hub_neighbours():
    sc = LC.hub_scene(6, 20, 2, 3)
    hub = 5
    assert all(hub in v.neighbors for v in sc.views if v.cam != hub)
    assert [v for v in sc.views if v.cam == hub][0].neighbors == [0, 1, 2, 3, 4]
    assert all(set(v.neighbors) <= set(range(6)) for v in sc.views)
    assert sum(1 for s, t in sc.pair_tests()[1] if t == hub) == 5
    cut = LC.drop_segments(sc, {1: [0, 19], 4: [7]})
    assert [len(v.segs) for v in cut.views] == [20, 18, 20, 20, 19, 20] and len(sc.views[1].segs) == 20
    assert np.array_equal(cut.views[1].segs, sc.views[1].segs[1:19])
