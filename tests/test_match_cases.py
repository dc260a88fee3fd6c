"""CPU checks behind tests/test_gpu_match_forms.py (no device needed):

  * the host model of phase A's launch forms (tests/match_cases.py) against the library's own plan
    (l3d_match_plan, l3d_match_tile_rows) on both sides of every edge;
  * the PLAN INVARIANT: whenever l3d_match_begin decides "no replay" for a call, every launch l3d_match_pairs can make of it
    fits the LDS and passes the launch-time check;
  * the shape conditions of every GPU scene, on the model and the CPU oracle, so that a drift of the scene generator fails
    here instead of silently losing the coverage.
"""
import functools

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import match_cases as MC
from tests.test_culling_math import _cull_forms, _fundamental

EDGE_TOTALS = (2049, 3584, 3585, 16384, 16385, 40000)
LAUNCH_SIZES = (1, 7, 8) + EDGE_TOTALS
WIDTHS = ((1000, True), (70000, False))          # (largest target view, 16-bit indices)


@functools.lru_cache(maxsize=None)
def _oracle_rows(scene_fn, args, kNN, epi):
    """accepted matches per source row of every pair of a scene, by the CPU oracle: {(src, tgt): counts}"""
    sc = scene_fn(*args)
    o = Oracle(threads=16)
    o.add_scene(sc)
    o.begin_match(kNN=kNN, epi_overlap=epi)
    out = {}
    for s, t in MC.pair_list(sc):
        out[(s, t)] = np.diff(o.match_pair(s, t)[1].astype(np.int64))
    o.end_match()
    return out


# ---- the model against the library ---------------------------------------------------------------------------------------
def test_k_limits_of_the_documented_lds_layout():
    """the last K whose tables fit 160 KiB, per tier and index width"""
    assert [MC.max_k(t, True) for t in MC.TIERS] == [1667, 416, 408, 422]
    assert [MC.max_k(t, False) for t in MC.TIERS] == [1250, 312, 305, 316]


def test_tile_rows_follow_the_estimate(monkeypatch):
    from line3dpp_amd import _lib
    L = _lib.load()
    monkeypatch.delenv("L3D_MATCH_TILE", raising=False)
    for est in (1, 2047, 2048, 2049, 5000, 1 << 33):
        assert L.l3d_match_tile_rows(est) == (MC.TILE_ROWS if est <= MC.TILE_MAX_EST_ITEMS else 0), est
    monkeypatch.setenv("L3D_MATCH_TILE", "0")
    assert L.l3d_match_tile_rows(10) == 0
    monkeypatch.setenv("L3D_MATCH_TILE", "16")
    assert L.l3d_match_tile_rows(5000) == 16


def test_model_equals_the_plan_hook_on_both_sides_of_every_edge():
    items = sorted({max(1, e + d) for e in MC.ITEM_EDGES + (8, 40000) for d in (-1, 0, 1)})
    seen = set()
    for rows in (MC.ROWS, MC.TILE_ROWS):
        ks = (1, 10, 305, 306, 312, 313, 316, 317, 408, 409, 416, 417, 422, 423) if rows == MC.ROWS else (10, 1250, 1251, 1667, 1668)
        for max_target, ix16 in WIDTHS:
            for total in items:
                for n in [x for x in items if x <= total]:
                    for K in ks:
                        p = MC.plan(total, n, K, max_target, 16 if rows == MC.TILE_ROWS else 0)
                        t = MC.tier(n, rows)
                        assert p["tier"] == t and p["ix16"] == ix16, (rows, total, n, K, p)
                        assert p["lds"] == MC.lds_bytes(t, K, ix16), (rows, total, n, K, ix16, p)
                        assert p["accepted"] == (K <= MC.max_k(t, ix16)), (rows, total, n, K, ix16, p)
                        assert p["replay"] == MC.replays(total, K, rows, ix16), (rows, total, n, K, ix16, p)
                        assert (p["waves"], p["row_cache"]) == ((2, t == "row2_cached") if t.startswith("row2") else (1, False))
                        seen.add((t, p["replay"], p["accepted"]))
    assert {t for t, _, _ in seen} == set(MC.TIERS)
    assert {(r, a) for _, r, a in seen} >= {(False, True), (True, False), (True, True)}


@pytest.mark.parametrize("rows", [MC.ROWS, MC.TILE_ROWS])
def test_plan_invariant_no_replay_means_every_launch_fits(rows):
    """If l3d_match_begin decides against the replay, then whatever range of the pair list l3d_match_pairs is given, the
    launch asks for at most 160 KiB of LDS and the launch-time check accepts it."""
    ks = range(300, 431) if rows == MC.ROWS else range(1240, 1681)
    bad, no_replay = [], 0
    for max_target, _ in WIDTHS:
        for total in EDGE_TOTALS:
            for n in [x for x in LAUNCH_SIZES if x <= total]:
                for K in ks:
                    p = MC.plan(total, n, K, max_target, 16 if rows == MC.TILE_ROWS else 0)
                    if not p["replay"]:
                        no_replay += 1
                        if p["lds"] > MC.LDS_LIMIT or not p["accepted"]:
                            bad.append((total, n, K, max_target, p))
    assert no_replay > 1000
    assert not bad, (len(bad), bad[:5])


# ---- shape conditions of the GPU scenes --------------------------------------------------------------------------------------
def test_partial_scene_reaches_every_edge():
    sc = MC.partial_scene()
    items = MC.pair_items(sc)
    assert MC.est_items(sc) > MC.TILE_MAX_EST_ITEMS and MC.call_rows(sc) == MC.ROWS        # in the row form by itself
    assert items.sum() > MC.ORDER_MAX_ITEMS + 1 and set(items.tolist()) == {3, 4}
    sp = MC.partial_splits(items)
    assert set(sp) == {"3584", "3585", "16384", "16385", "odd row2", "odd row2_cached", "odd row1"}, sp
    ordered_second = 0
    for label, (c, which) in sp.items():
        n = MC.split_items(items, c)
        if label.isdigit():
            assert n[which] == int(label)
        else:
            assert n[0] % 8 and MC.tier(n[0]) == label[4:]
        ordered_second += MC.tier(n[1]) == "row2_cached"
    assert ordered_second >= 2                      # launches with first > 0 in the ordering tier
    assert {MC.tier(x) for _, (c, _) in sp.items() for x in MC.split_items(items, c)} == set(MC.TIERS[1:])


def test_partial_scene_culls_streams_and_matches():
    sc = MC.partial_scene()
    views = {v.cam: v for v in sc.views}
    pl = MC.pair_list(sc)
    refused = [p for p in pl if _cull_forms(_fundamental(views[p[0]], views[p[1]]), views[p[0]].width, views[p[0]].height,
                                            views[p[1]].width, views[p[1]].height) is None]
    assert refused == [(0, MC.PARTIAL_VIEWS)], refused          # the forward-motion pair streams unculled
    assert len(pl) - len(refused) >= len(pl) // 4
    rows = _oracle_rows(MC.partial_scene, (), 10, 0.25)
    assert sum(int(c.sum()) for c in rows.values()) >= 10**4


def test_handover_scenes_sit_on_the_edge():
    a, b = MC.handover_scene(False), MC.handover_scene(True)
    assert (MC.est_items(a), MC.est_items(b)) == (MC.TILE_MAX_EST_ITEMS, MC.TILE_MAX_EST_ITEMS + 1)
    assert (MC.call_rows(a), MC.call_rows(b)) == (MC.TILE_ROWS, MC.ROWS)
    assert len(MC.pair_list(b)) == len(MC.pair_list(a)) + 1
    assert MC.tier(MC.pair_items(b).sum()) == "row2_cached" and MC.pair_items(a).sum() == 6 * len(MC.pair_list(a))


def test_mixed_scene_orders_a_launch_with_large_and_tiny_pairs():
    sc = MC.mixed_scene()
    items = MC.pair_items(sc)
    c = MC.mixed_split(items)
    n = MC.split_items(items, c)
    assert MC.tier(n[0]) == MC.tier(n[1]) == "row2_cached" and n[1] % 8
    M = {v.cam: len(v.segs) for v in sc.views}
    tail = MC.pair_list(sc)[c:]
    big = [p for p in tail if M[p[1]] > 4096]
    assert len(big) == 3 and big == MC.pair_list(sc)[-3:]       # chunk bands in k_order_items, cost_max from these
    assert sum(1 for p in tail if M[p[1]] <= 130) > 2000        # ... while most items of the launch are tiny
    assert items[-1] == MC.items_per_pair(MC.MIXED_BIG_SEGS, MC.ROWS) == 71


def test_knn_scenes_have_full_and_unfilled_tables():
    for padded in (False, True):
        sc = MC.knn_scene(padded)
        assert (MC.call_rows(sc) == MC.ROWS) == padded
        assert MC.tier(MC.pair_items(sc, MC.ROWS).sum()) == ("row2_cached" if padded else "row2")
    rows = _oracle_rows(MC.knn_scene, (False,), 0, MC.KNN_EPI)
    assert len(rows) == 3
    for pair, c in rows.items():
        assert (c > 423).sum() >= 4 and (c < 312).sum() >= 100 and ((c >= 312) & (c <= 423)).sum() >= 4, (pair, np.sort(c)[-20:])


def test_knn_tile_scene_has_full_and_unfilled_tables():
    sc = MC.knn_tile_scene()
    assert MC.call_rows(sc) == MC.TILE_ROWS and MC.pair_list(sc) == [(0, 1)] and MC.pair_items(sc).sum() == 268
    c = _oracle_rows(MC.knn_tile_scene, (), 0, MC.KNN_TILE_EPI)[(0, 1)]
    assert (c > 1668).sum() >= 4 and ((c > 1251) & (c < 1667)).sum() >= 10 and (c < 1250).sum() >= 1000, np.sort(c)[-40:]


def test_tie_scenes_cross_the_lds_heap():
    want = {None: 1068, 1025: 1025, 1024: 1024}
    for length, n in want.items():
        c = _oracle_rows(MC.tie_scene, (length,), 0, MC.TIE_EPI)[(0, 1)]
        assert c[MC.TIE_ROW] == c[MC.TIE_ROW + 1] == n, (length, c[MC.TIE_ROW])
        assert (c > MC.TIE_LDS_HEAP).sum() >= 4 and (c < MC.TIE_LDS_HEAP).sum() > 2000
