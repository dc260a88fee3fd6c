"""Phase A (k_cull_prepare -> k_order_items -> k_match_pairs -> k_match_tied_rows) at the places where a launch changes
its form: the four launch tiers on both sides of their item-count edges (partial launches of one pair list, the second
with first > 0), the hand-over between the tile and the row form, an ordered launch that mixes tiny pairs with views
beyond 4 096 segments, kNN on both sides of what the LDS tables hold in every tier, and tied rows on both sides of the
1 024 entries k_match_tied_rows keeps in LDS.

Every test asks the host model (tests/match_cases.py) which form a launch takes and reads the library's launch counters
(l3d_debug_counter) before and after it: the predicted form is the one that ran.  The shape conditions of the scenes
are asserted on the CPU in tests/test_match_cases.py.  Results: the slots of every directed pair against the CPU
oracle's match_pair -- identical sets, overlap and depths bit for bit, rows in the reference's heap order
(helpers.compare_pair_fast) -- and runs of the library on the same input byte for byte.  The one exception (pairs of
views of 4 200 segments, compared with the library's brute-force path) is named in its test."""
import functools

import numpy as np
import pytest

from line3dpp_amd._lib import EMPTY, SLOT_DTYPE
from tests import helpers as H
from tests import match_cases as MC

pytestmark = pytest.mark.gpu


def _ctx(sc):
    from line3dpp_amd.api import Line3D
    g = Line3D()
    g.add_scene(sc)
    return g


@functools.lru_cache(maxsize=None)
def _oracle_pairs(scene_fn, args, kNN, epi, skip_targets_above=None):
    """the oracle's matches of every directed pair of a scene (by its builder), computed once and shared, never modified;
    None for the pairs whose target view has more than skip_targets_above segments"""
    from oracle.oracle import Oracle
    sc = scene_fn(*args)
    M = {v.cam: len(v.segs) for v in sc.views}
    o = Oracle(threads=16)
    o.add_scene(sc)
    o.begin_match(kNN=kNN, epi_overlap=epi)
    out = [None if skip_targets_above and M[t] > skip_targets_above else o.match_pair(s, t)[0] for s, t in MC.pair_list(sc)]
    o.end_match()
    return out


def _all_slots(g):
    """the slot buffer of the context as one host array (waits for the context's stream)"""
    import torch
    from line3dpp_amd import dist
    assert g.L.l3d_synchronize(g.h) == 0
    ptr, n = g.slot_buffer()
    return dist.device_tensor(ptr, n * SLOT_DTYPE.itemsize, torch.device("cuda", 0)).cpu().numpy().view(SLOT_DTYPE)


def _assert_pairs_equal_oracle(sc, g, slots, kNN, oracle, min_matches=1):
    pairs, off = g.pairs()
    assert [tuple(int(x) for x in p) for p in pairs] == MC.pair_list(sc)
    M = {v.cam: len(v.segs) for v in sc.views}
    total = 0
    for pi, (s, _) in enumerate(pairs):
        if oracle[pi] is None:
            continue
        a = int(off[pi])
        r = H.compare_pair_fast(slots[a:a + M[int(s)] * kNN].reshape(M[int(s)], kNN), oracle[pi])
        assert r["set_diff"] == 0 and r["inexact_fields"] == 0 and r["order_rows"] == r["tie_rows"] == 0, (pi, r)
        total += r["n_cpu"]
    assert total >= min_matches, total
    return total


def _launch(g, first, count, total_items, items, rows=MC.ROWS, replay=False):
    """one l3d_match_pairs; the form the model predicts for its item count is the form the counters saw"""
    before = MC.read_counters()
    assert g.matchPairs(first, count), (g.last_status, first, count)
    dc = MC.counters_since(before)
    want = dict.fromkeys(MC.COUNTERS, 0)
    t = MC.tier(items, rows)
    if not replay:
        want[MC.TIER_COUNTERS[t]] = 1
        want["match_order_launches"] = int(t == "row2_cached")
    assert dc == want, (first, count, items, t, dc)
    return t


# ---- item-count edges by partial launches ---------------------------------------------------------------------------------
def test_partial_launches_on_both_sides_of_every_item_count_edge():
    """One pair list of 17 438 row-form items (5 701 pairs of three or four items), launched as [0, c) + [c, P) for the
    seven splits of match_cases.partial_splits: a launch of exactly 3 584, 3 585, 16 384 and 16 385 items -- a prefix or, where
    no prefix sum has that value, the remainder of the list, which is how the launches with first > 0 come to sit on the
    edges of the ordering tier (3 585 and 16 384) -- and one first launch per row tier whose item count is no multiple of
    8.  Every split runs on one context that is begun again and again (pair list and work list kept) and on a fresh one."""
    sc = MC.partial_scene()
    items = MC.pair_items(sc)
    P, total = len(items), int(items.sum())
    oracle = _oracle_pairs(MC.partial_scene, (), 10, 0.25)
    kept = _ctx(sc)
    first_snap, tiers_seen, ordered_with_first = None, [], 0
    for label, (c, _) in MC.partial_splits(items).items():
        n = MC.split_items(items, c)
        for g in (kept, _ctx(sc)):
            assert g.matchBegin(kNN=10)
            assert len(g.pairs()[0]) == P
            t0 = _launch(g, 0, c, total, n[0])
            t1 = _launch(g, c, P - c, total, n[1])
            tiers_seen += [t0, t1]
            ordered_with_first += t1 == "row2_cached"
            tm = g.timings()
            assert P // 4 <= tm["culled_pairs"] < P                      # (the forward-motion pair streams unculled)
            snap = _all_slots(g)
            if first_snap is None:
                first_snap = snap.copy()
                n_matches = _assert_pairs_equal_oracle(sc, g, first_snap, 10, oracle, min_matches=10**4)
            assert snap.tobytes() == first_snap.tobytes(), label
            assert g.matchAbort()
        print(f"split {label}: [0, {c}) {n[0]} items {t0}, [{c}, {P}) {n[1]} items {t1}")
    print(f"launches per tier: { {t: tiers_seen.count(t) for t in MC.TIERS} }, ordered with first > 0: {ordered_with_first}, "
          f"{n_matches} matches")
    assert set(tiers_seen) == set(MC.TIERS[1:]) and ordered_with_first >= 2


# ---- the tile / row hand-over by itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_neighbor", [False, True])
def test_tile_row_hand_over_at_2048_estimated_items(extra_neighbor, monkeypatch):
    """2 048 estimated row-form items: the tile form; one more neighbour of one view, 2 049: the row form -- chosen by the
    library itself, and both equal the oracle"""
    monkeypatch.delenv("L3D_MATCH_TILE", raising=False)
    sc = MC.handover_scene(extra_neighbor)
    rows = MC.call_rows(sc)
    assert MC.est_items(sc) == MC.TILE_MAX_EST_ITEMS + int(extra_neighbor) and rows == (MC.ROWS if extra_neighbor else MC.TILE_ROWS)
    items = MC.pair_items(sc)
    g = _ctx(sc)
    assert g.matchBegin(kNN=10)
    t = _launch(g, 0, len(items), int(items.sum()), int(items.sum()), rows)
    assert t == ("row2_cached" if extra_neighbor else "tile")
    n = _assert_pairs_equal_oracle(sc, g, _all_slots(g), 10, _oracle_pairs(MC.handover_scene, (extra_neighbor,), 10, 0.25), 10**4)
    print(f"{sc.name}: est {MC.est_items(sc)}, {int(items.sum())} items, {t}, {n} matches")
    assert g.matchAbort()


# ---- an ordered launch with mixed pairs -----------------------------------------------------------------------------------
def test_ordered_launch_mixes_tiny_pairs_with_views_beyond_4096_segments():
    """The second launch (first > 0, 9 003 items) holds 2 900 pairs of 64 .. 130 segments and the three pairs of the views of
    4 200 segments: k_order_items takes chunk bands for those and target bands for the rest, its LDS and cost_max are set by
    the large views.  The three large pairs are compared with the library's brute-force path (every target through the
    exact test, set_brute_force) -- the oracle needs too long for them --, every other pair with the oracle."""
    sc = MC.mixed_scene()
    items = MC.pair_items(sc)
    P, total, c = len(items), int(items.sum()), MC.mixed_split(items)
    n = MC.split_items(items, c)
    g = _ctx(sc)
    assert g.matchBegin(kNN=10)
    assert _launch(g, 0, c, total, n[0]) == "row2_cached" and _launch(g, c, P - c, total, n[1]) == "row2_cached"
    slots = _all_slots(g)
    oracle = _oracle_pairs(MC.mixed_scene, (), 10, 0.25, 4096)
    assert [pi for pi, o in enumerate(oracle) if o is None] == [P - 3, P - 2, P - 1]
    n_small = _assert_pairs_equal_oracle(sc, g, slots, 10, oracle, 10**4)
    b = _ctx(sc)
    b.set_brute_force(1)
    assert b.matchBegin(kNN=10) and b.matchPairs(P - 3, 3)
    n_big = 0
    for pi in range(P - 3, P):
        mine, brute = g.pair_slots(pi), b.pair_slots(pi)
        assert mine.tobytes() == brute.tobytes(), pi
        n_big += int((mine["tgt_seg"] != EMPTY).sum())
    assert n_big > 1000
    print(f"{sc.name}: [0, {c}) {n[0]} items, [{c}, {P}) {n[1]} items, both ordered; {n_small} + {n_big} matches")
    assert g.matchAbort() and b.matchAbort()


# ---- kNN around the table limits, context path ----------------------------------------------------------------------------
def _knn_call(sc, scene_key, kNN, rows, expect_tier, epi=MC.KNN_EPI):
    items = MC.pair_items(sc, rows)
    total = int(items.sum())
    replay = MC.replays(total, kNN, rows)
    g = _ctx(sc)
    before = MC.read_counters()
    assert g.matchBegin(kNN=kNN, epipolar_overlap=epi), (g.last_status, kNN)
    assert MC.counters_since(before)["knn_replay_calls"] == int(replay), (kNN, total, replay)
    assert MC.tier(total, rows) == expect_tier
    _launch(g, 0, len(items), total, total, rows, replay=replay)
    oracle = _oracle_pairs(*scene_key, kNN, epi)
    pairs, _ = g.pairs()
    n, longest = 0, 0
    for pi in range(len(pairs)):
        sl = g.pair_slots(pi)
        r = H.compare_pair_fast(sl, oracle[pi])
        assert r["set_diff"] == 0 and r["inexact_fields"] == 0 and r["order_rows"] == r["tie_rows"] == 0, (kNN, pi, r)
        n += r["n_cpu"]
        longest = max(longest, int((sl["tgt_seg"] != EMPTY).sum(1).max()))
    print(f"{sc.name} kNN={kNN}: {total} items, {expect_tier}, replay {replay}, {n} matches, longest row {longest}")
    assert g.matchAbort()
    return replay, longest


@pytest.mark.parametrize("kNN", [312, 313, 408, 409, 416, 417, 422, 423])
@pytest.mark.parametrize("padded", [False, True])
def test_knn_at_the_table_limits_of_the_row_form(kNN, padded, monkeypatch):
    """The last K whose top-K tables fit 160 KiB of LDS and the first that does not, re-derived from the LDS layout documented
    in k_match.hip (struct Lds / carve: rings, per row two words, two indices and K x (overlap, index)), not asked of the
    library: 312 | 313 with 32-bit indices and two waves (the width the launch-time check used to assume), 408 | 409 with 16-bit
    indices, two waves and the row cache, 416 | 417 with two waves, 422 | 423 with one wave per item.  Every call succeeds and
    equals the oracle at that kNN; a call replays every row exactly when some launch it can make does not hold K -- from
    417 on for the three large views alone (78 items, forced into the row form), from 409 on with the 100 tiny views around
    them (4 078 items: in the row form by itself, row-cache tier).  Rows longer than 423 and rows shorter than 312 exist, so
    that full and unfilled tables are compared."""
    if padded:
        monkeypatch.delenv("L3D_MATCH_TILE", raising=False)
    else:
        monkeypatch.setenv("L3D_MATCH_TILE", "0")
    sc = MC.knn_scene(padded)
    replay, longest = _knn_call(sc, (MC.knn_scene, (padded,)), kNN, MC.ROWS, "row2_cached" if padded else "row2")
    assert longest == kNN                                                # some row fills its table
    assert replay == (kNN > (408 if padded else 416))
    assert not (kNN == 312 and replay) and not (kNN == 423 and not replay)


@pytest.mark.parametrize("kNN", [1250, 1251, 1667, 1668])
def test_knn_at_the_table_limits_of_the_tile_form(kNN, monkeypatch):
    """the tile form (16 rows per item: FIFO, one wave's rings, K x (overlap, index) for 16 rows) holds K = 1 250 with 32-bit
    and 1 667 with 16-bit indices.  One pair of views of 4 200 segments at an overlap threshold of 1e-4, in the tile form by
    itself (268 items): five rows accept more than 1 668 targets, 38 more than 1 251, so that tables filled to the limit
    and unfilled ones are compared."""
    monkeypatch.delenv("L3D_MATCH_TILE", raising=False)
    sc = MC.knn_tile_scene()
    replay, longest = _knn_call(sc, (MC.knn_tile_scene, ()), kNN, MC.TILE_ROWS, "tile", MC.KNN_TILE_EPI)
    assert longest == kNN and replay == (kNN == 1668)


# ---- tied rows beyond the LDS heap ----------------------------------------------------------------------------------------
def _pair_arguments(o):
    F = o.fundamental(0, 1)
    i0, i1 = o.view_info(0), o.view_info(1)
    return F, i0["C"], i1["C"]


@pytest.mark.parametrize("row_length", [None, 1025, 1024])
def test_tied_rows_on_both_sides_of_the_lds_heap(row_length):
    """Every segment twice in its view and an overlap threshold of 1e-4: nearly every row is replayed by k_match_tied_rows,
    which keeps the accepted (overlap, target) entries of a row in LDS up to 1 024 and in global scratch beyond.  Rows 32 / 33
    accept 1 068 targets as generated, exactly 1 025 / 1 024 with the first 43 / 44 of them dropped; four more rows lie
    above 1 024 and 2 590 below.  The context path with kNN = 10 (tied rows) and with kNN = 2000 (k_queue_all_rows: every
    row replayed, rows of more than 1 024 entries kept whole), and the seam entry l3d_match_lines with kNN = 10: same slots
    in the same order as the oracle."""
    from line3dpp_amd.api import match_lines
    from oracle.oracle import Oracle
    sc = MC.tie_scene(row_length)
    vs, vt = sc.views
    for kNN in (10, 2000):
        g = _ctx(sc)
        before = MC.read_counters()
        assert g.matchBegin(kNN=kNN, epipolar_overlap=MC.TIE_EPI) and g.matchPairs(0, 1)
        assert MC.counters_since(before)["knn_replay_calls"] == int(kNN == 2000)
        sl = g.pair_slots(0)
        om = _oracle_pairs(MC.tie_scene, (row_length,), kNN, MC.TIE_EPI)[0]
        r = H.compare_pair_fast(sl, om)
        assert r["set_diff"] == 0 and r["inexact_fields"] == 0 and r["order_rows"] == r["tie_rows"] == 0, (kNN, r)
        filled = (sl["tgt_seg"] != EMPTY).sum(1)
        want = row_length or 1068
        assert filled[MC.TIE_ROW] == filled[MC.TIE_ROW + 1] == min(kNN, want)
        assert g.matchFinish()
        tied = g.timings()["tied_rows"]
        assert tied == len(vs.segs) if kNN == 2000 else tied > 500, tied      # (rows 32 / 33 hold equal overlaps in any case)
        print(f"{sc.name} kNN={kNN}: row {MC.TIE_ROW} accepts {want}, {r['n_cpu']} matches, {tied} rows replayed")
    # the seam entry: F and the camera centres of the oracle's (translated) views; RtKinv from numpy's inverse, so the depths
    # agree to the seam's 1e-5 (test_seam_level_match_lines) while sets, order and overlaps are the oracle's
    o = Oracle(threads=16)
    o.add_scene(sc)
    o.begin_match(kNN=10, epi_overlap=MC.TIE_EPI)
    F, C0, C1 = _pair_arguments(o)
    om, _ = o.match_pair(0, 1)
    o.end_match()
    slots, n = match_lines(vs.segs, vt.segs, F, vs.R.T @ np.linalg.inv(vs.K), vt.R.T @ np.linalg.inv(vt.K), C0, C1, vs.width, vs.height,
                           MC.TIE_EPI, 10)
    assert n == len(om)
    valid = slots["tgt_seg"] != EMPTY
    rows = np.repeat(np.arange(len(vs.segs)), 10).reshape(-1, 10)[valid]
    assert np.array_equal(rows, om["src_seg"]) and np.array_equal(slots["tgt_seg"][valid], om["tgt_seg"])
    assert np.array_equal(slots["overlap"][valid], om["overlap"])
    for f in ("d_p1", "d_p2", "d_q1", "d_q2"):
        assert np.all(H.rel_close(slots[f][valid], om[f], 1e-5)), f
