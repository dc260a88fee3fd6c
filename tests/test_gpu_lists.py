"""Phase B's list pass (k_lists.hip, l3d_phase_b.hip) at the places where a list changes its path: the hand-over between
the kernel tiers at both staging widths, passes that are repeated (a left-out tier, record pools, the scratch of
k_lists_huge), the chain beyond the sweeps enqueued blindly, staging rounds of the incoming pairs, keep-all rows in the
upper tiers, the global-memory walk of k_edges, the sharded pass.

Every test first checks the host model of the list lengths (tests/lists_cases.py) against the library -- sum(L) ==
l3d_timings.list_entries, sum(n_inv) == list_inverse, lists per tier == the l3d_debug_counter differences -- and then
asserts its SHAPE CONDITIONS on the model, so that a drift of the scene generator fails loudly instead of losing the
coverage.  Results are compared with the CPU oracle (restatement) through helpers.compare_matches / full_result_diff at
helpers.REL_TOL, sets and order identical; runs of the library on the same input are compared byte for byte.

The scenes and kNN values were found with a search that ran phase A and the model only; the histograms they gave are in
the docstrings."""
import functools

import numpy as np
import pytest

from line3dpp_amd.scene import make_scene
from tests import helpers as H
from tests import lists_cases as LC

pytestmark = pytest.mark.gpu


def _ctx(sc):
    from line3dpp_amd.api import Line3D
    g = Line3D()
    g.add_scene(sc)
    return g


@functools.lru_cache(maxsize=None)
def _oracle(scene_fn, kNN, epi):
    """the oracle's full result of a scene (by its builder), computed once and shared, never modified"""
    from oracle.oracle import Oracle
    o = Oracle(threads=16)
    o.add_scene(scene_fn())
    o.match_images(kNN=kNN, epi_overlap=epi)
    o.compute_affinity()
    return o


def _call(g, sc, kNN, epi, entries_before=0):
    """one matchImages + computeAffinity on `g`; the model of its lists checked against the library's own counts.
    Returns dict(model, tm, dc (counter differences), base, tiers (predicted), snap (bytes of the result))."""
    before = LC.read_counters()
    assert g.matchImages(kNN=kNN, epipolar_overlap=epi), g.last_status
    dc = LC.counters_since(before)
    tm = g.timings()
    m = LC.model_of_context(g, sc, kNN)
    assert int(m["L"].sum()) == tm["list_entries"], "model: total list length"
    assert int(m["n_inv"].sum()) == tm["list_inverse"], "model: inverse hypotheses"
    base = LC.pass_base(m["n_slots"], m["G"], entries_before)
    tiers = LC.tier_counts(m["L"], base)
    print(f"{sc.name} kNN={kNN}: BASE {base}, lists per tier {tiers}, counters {dc}, retries {tm['pool_retries']}, "
          f"chain sweeps {tm['chain_sweeps']} + {tm['chain_extra_rounds']} rounds")
    assert (dc["lists_wide_passes"], dc["lists_narrow_passes"]) == ((1, 0) if base == 256 else (0, 1)), (base, dc)
    assert (dc["lists_tier2_lists"], dc["lists_tier4_lists"], dc["lists_huge_lists"]) == \
        (tiers["tier2"], tiers["tier4"], tiers["huge"]), (tiers, dc)
    assert g.computeAffinity()
    return dict(model=m, tm=tm, dc=dc, base=base, tiers=tiers, snap=_snapshot(g, sc))


def _snapshot(g, sc):
    """the bytes of everything the call produced: matches, best hypotheses, view medians, affinity"""
    out = []
    for v in sc.views:
        m, off = g.matches(v.cam)
        out += [m.tobytes(), off.tobytes(), g.view_info(v.cam)["median_depth"].tobytes()]
    out += [x.tobytes() for x in g.best()]
    e, l2g, msdl = g.affinity()
    out += [e.tobytes(), l2g.tobytes(), np.float32(msdl).tobytes()]
    return out


def _assert_equals_oracle(g, o, sc):
    """identical sets in identical order, values within REL_TOL"""
    r = H.full_result_diff(g, o, sc)
    assert r["ok"], r
    assert r["surviving"] > 0 and r["best"] > 0 and r["affinity_entries"] > 0, r
    for v in sc.views:
        gm, goff = g.matches(v.cam); om, ooff = o.matches(v.cam)
        c = H.compare_matches(gm, om)
        assert not c["missing"] and not c["extra"] and c["max_rel"] <= H.REL_TOL, (v.cam, c)
        assert np.array_equal(goff, ooff)
    s2, _, bm = g.best(); cs, _, _, obm = o.best()
    assert np.array_equal(np.stack([s2["cam"], s2["seg"]], 1), cs), "best hypotheses: order"
    assert np.array_equal(bm["tgt_cam"], obm["tgt_cam"]) and np.array_equal(bm["tgt_seg"], obm["tgt_seg"])
    ge, gl, _ = g.affinity(); oe, ol = o.affinity()
    assert np.array_equal(ge["i"], oe["i"]) and np.array_equal(ge["j"], oe["j"]), "affinity edges: order"
    assert np.array_equal(np.stack([gl["cam"], gl["seg"]], 1), ol)


def _has(L, *lengths):
    return {int(x): int((L == x).sum()) for x in lengths}


def _incoming_pairs(sc, cam):
    return sum(1 for s, t in sc.pair_tests()[1] if t == cam and s < t)


# ---- the scenes ------------------------------------------------------------------------------------------------------
# 34 views x 300 segments on a quarter arc, ring neighbours +-2, view 33 a neighbour of every view.  The hub's 300 lists
# are all-inverse and spread over 0 .. 1593; the segments dropped below are source rows of views 0-3 that hand a match
# to exactly one of eight chosen hub segments, which brings those eight lists to 128, 129, 256, 257, 512, 513, 1024 and
# 1025 (a hub list loses one entry per source row that named it).
HUB34_DROP = {0: [2, 5, 11, 24, 25, 28, 31, 33, 39, 41, 43, 52, 53, 63, 71, 73, 81, 84, 95, 109, 112, 114, 117, 128, 130, 131,
                  134, 136, 138, 153, 169, 198, 242, 278],
              1: [3, 20, 24, 29, 35, 39, 97, 125, 155, 190, 230],
              2: [87, 110, 126, 136, 139, 157, 193, 237, 252, 256],
              3: [63, 89]}
HUB34_KNN, HUB_EPI = 100, 0.05


def hub34_scene():
    return LC.drop_segments(LC.hub_scene(34, 300, 4, 1, real_fraction=0.9), HUB34_DROP)


def hub18_scene():
    return LC.hub_scene(18, 300, 4, 1, real_fraction=0.9)


def hub258_scene():
    return LC.hub_scene(258, 64, 4, 1, real_fraction=0.9)


def keepall_scene():
    return make_scene(8, 400, n_neighbors=7, seed=1, real_fraction=0.9)


def switch_scene():
    return make_scene(12, 200, n_neighbors=6, seed=5, real_fraction=0.5)


def dense18_scene():
    return make_scene(18, 300, n_neighbors=16, seed=71, real_fraction=0.5)


def chain_scene():
    return make_scene(200, 100, n_neighbors=2, seed=1, real_fraction=1.0, noise_px=0.0)


def mixed_scene():
    return LC.mixed_scene([300, 1, 64, 2, 65, 300, 64, 1, 65, 2, 300, 64], 6, 3, real_fraction=0.9)


@functools.lru_cache(maxsize=None)
def _hub34_runs():
    """The hub34 scene on a fresh context (first call: BASE from the estimate 1.5 n_slots / G = 423 -> 256) and on a
    context whose first call had kNN = 1 (mean list length 4.9 -> the next pass runs with BASE = 128, and with the
    four-wave tier and k_lists_huge left out of its first launch sequence)."""
    sc = hub34_scene()
    wide_g = _ctx(sc)
    wide = _call(wide_g, sc, HUB34_KNN, HUB_EPI)
    g = _ctx(sc)
    call1 = _call(g, sc, 1, HUB_EPI)
    call2 = _call(g, sc, HUB34_KNN, HUB_EPI, entries_before=call1["tm"]["list_entries"])
    _assert_equals_oracle(g, _oracle(hub34_scene, HUB34_KNN, HUB_EPI), sc)
    call3 = _call(g, sc, 1, HUB_EPI, entries_before=call2["tm"]["list_entries"])
    _assert_equals_oracle(g, _oracle(hub34_scene, 1, HUB_EPI), sc)
    return dict(sc=sc, wide_g=wide_g, wide=wide, call1=call1, call2=call2, call3=call3)


# ---- a. tier edges, both widths ---------------------------------------------------------------------------------------
def test_tier_edges_at_the_wide_staging():
    """BASE = 256 (fresh context, kNN = 100): lists of exactly CAP and CAP + 1 at the three hand-overs 256 / 512 / 1024,
    and of 0, 1 and 2.  hub34, 10143 lists, total length 603100 (296260 inverse), longest 1593; lists of length
    0: 20, 1: 24, 2: 34, 128: 16, 129: 15, 256: 1, 257: 1, 512: 1, 513: 1, 1024: 1, 1025: 1; per tier at BASE 256:
    9933 / 106 / 83 / 21 (one wave / two / four / k_lists_huge)."""
    R = _hub34_runs()
    w = R["wide"]
    assert w["base"] == 256 and w["dc"]["lists_wide_passes"] == 1
    have = _has(w["model"]["L"], 0, 1, 2, 256, 257, 512, 513, 1024, 1025)
    assert all(n >= 1 for n in have.values()), have
    assert min(w["tiers"].values()) >= 1, w["tiers"]
    assert w["dc"]["lists_tier_repeats"] == 0 and w["tm"]["pool_retries"] == 0
    _assert_equals_oracle(R["wide_g"], _oracle(hub34_scene, HUB34_KNN, HUB_EPI), R["sc"])


def test_tier_edges_at_the_narrow_staging():
    """BASE = 128 (the context's previous call measured a mean list length of 4.9): the same lists, now with CAP and
    CAP + 1 at 128 / 256 / 512; per tier at BASE 128: 9662 / 271 / 106 / 104.  Same result as at the wide staging, byte
    for byte (the oracle comparison of this call is in _hub34_runs)."""
    R = _hub34_runs()
    n = R["call2"]
    assert n["base"] == 128 and n["dc"]["lists_narrow_passes"] == 1
    have = _has(n["model"]["L"], 0, 1, 2, 128, 129, 256, 257, 512, 513)
    assert all(c >= 1 for c in have.values()), have
    assert min(n["tiers"].values()) >= 1, n["tiers"]
    assert n["snap"] == R["wide"]["snap"]


# ---- b. hub views: staging rounds of the incoming pairs ---------------------------------------------------------------
def test_hub_view_with_17_incoming_pairs():
    """18 views, kNN = 16 (estimate 64 -> BASE 128): the one-wave tier stages 16 incoming pairs per round, the hub has 17.
    Hub lists per tier 148 / 85 / 59 / 8, the longest has 694 entries, all of them inverse: its rounds take the early-out
    of a list that is too long for the tier.  5400 lists, total length 259899."""
    sc = hub18_scene()
    hub = max(v.cam for v in sc.views)
    assert _incoming_pairs(sc, hub) == 17
    g = _ctx(sc)
    r = _call(g, sc, 16, HUB_EPI)
    assert r["base"] == 128
    m = r["model"]
    h0 = m["seg_base"][hub]
    hub_tiers = LC.tier_counts(m["L"][h0:], 128)
    assert hub_tiers["tier2"] >= 1 and hub_tiers["tier4"] >= 1, hub_tiers
    assert m["n_fresh"][h0:].max() == 0 and m["n_inv"][h0:].max() > 128
    _assert_equals_oracle(g, _oracle(hub18_scene, 16, HUB_EPI), sc)


def test_hub_view_with_33_incoming_pairs():
    """34 views: the two- and four-wave tiers (and the one-wave tier at BASE = 256) stage 32 incoming pairs per round,
    the hub has 33.  At both widths hub lists reach tiers 2 and 4, and the longest (1593 inverse entries) is too long
    for every staged tier."""
    R = _hub34_runs()
    sc = R["sc"]
    hub = max(v.cam for v in sc.views)
    assert _incoming_pairs(sc, hub) == 33
    for run, base in ((R["wide"], 256), (R["call2"], 128)):
        m = run["model"]
        h0 = m["seg_base"][hub]
        assert run["base"] == base
        hub_tiers = LC.tier_counts(m["L"][h0:], base)
        assert hub_tiers["tier2"] >= 1 and hub_tiers["tier4"] >= 1 and hub_tiers["huge"] >= 1, hub_tiers
        assert m["n_fresh"][h0:].max() == 0 and m["n_inv"][h0:].max() > 4 * base


def test_hub_view_with_257_incoming_pairs_through_the_huge_kernel():
    """258 views of 64 segments, kNN = 10 (estimate 44 -> BASE 128): k_lists_huge stages 256 incoming pairs per round,
    the hub has 257.  16512 lists, total length 203536; 42 lists for k_lists_huge, the hub's longest with 3250 entries."""
    sc = hub258_scene()
    hub = max(v.cam for v in sc.views)
    assert _incoming_pairs(sc, hub) == 257
    g = _ctx(sc)
    r = _call(g, sc, 10, HUB_EPI)
    m = r["model"]
    h0 = m["seg_base"][hub]
    assert r["base"] == 128 and LC.tier_counts(m["L"][h0:], 128)["huge"] >= 1 and m["n_inv"][h0:].max() > 512
    _assert_equals_oracle(g, _oracle(hub258_scene, 10, HUB_EPI), sc)


# ---- c. keep-all rows in the upper tiers ------------------------------------------------------------------------------
def test_keep_all_rows_in_the_upper_tiers():
    """kNN = 0 (ragged rows: the fresh slots of a segment are found through the rows' starts) on 8 views x 400 segments,
    every view a neighbour of every other: 3200 lists, total length 341254, longest 512; BASE 128 (estimate 83), per tier
    2323 / 739 / 138 / 0.  Lists of tiers 2 and 4 hold fresh AND inverse hypotheses."""
    sc = keepall_scene()
    g = _ctx(sc)
    r = _call(g, sc, 0, HUB_EPI)
    m = r["model"]
    assert r["base"] == 128 and r["tiers"]["tier2"] >= 1 and r["tiers"]["tier4"] >= 1, r["tiers"]
    L = m["L"]
    for lo, hi in ((128, 256), (256, 512)):
        mixed = (L > lo) & (L <= hi) & (m["n_fresh"] > 0) & (m["n_inv"] > 0)
        assert mixed.any(), f"no list of ({lo}, {hi}] with fresh and inverse hypotheses"
    _assert_equals_oracle(g, _oracle(keepall_scene, 0, HUB_EPI), sc)


# ---- d. more than kEdgeLds candidates per segment ---------------------------------------------------------------------
def test_edges_of_segments_with_more_than_512_candidates():
    """k_edges keeps (ij, sim) of a segment's candidates in LDS up to 512 of them and walks global memory beyond: 24
    segments of hub34 do, at either width (the results are those compared in the tier tests)."""
    R = _hub34_runs()
    assert R["wide"]["dc"]["edges_global_segments"] >= 1 and R["call2"]["dc"]["edges_global_segments"] >= 1
    assert R["call1"]["dc"]["edges_global_segments"] == 0       # (kNN = 1: 20293 candidates over 10143 lists)


# ---- e. both widths on one context ------------------------------------------------------------------------------------
def test_width_switch_between_two_calls_of_one_context():
    """12 views x 200 segments, 6 neighbours, kNN = 30: the first call estimates a mean list length of
    1.5 x 216000 slots / 2400 segments = 135 (BASE 256), measures 22.8, and the second call runs with BASE 128."""
    sc = switch_scene()
    g = _ctx(sc)
    first = _call(g, sc, 30, 0.25)
    second = _call(g, sc, 30, 0.25, entries_before=first["tm"]["list_entries"])
    assert (first["base"], second["base"]) == (256, 128)
    assert first["snap"] == second["snap"]
    _assert_equals_oracle(g, _oracle(switch_scene, 30, 0.25), sc)


# ---- f. a pass repeated with the tiers it had left out ----------------------------------------------------------------
def test_pass_repeated_with_the_tiers_left_out():
    """One context, three calls on hub34.  kNN = 1: no list beyond one wave's staging (longest 123), so the next pass
    is launched without the four-wave tier and k_lists_huge; kNN = 100 then hands 106 and 104 lists to them and is
    repeated; kNN = 1 again gives the first call's bytes."""
    R = _hub34_runs()
    c1, c2, c3 = R["call1"], R["call2"], R["call3"]
    assert (c1["dc"]["lists_tier2_lists"], c1["dc"]["lists_tier4_lists"], c1["dc"]["lists_huge_lists"]) == (0, 0, 0)
    assert c2["dc"]["lists_tier4_lists"] >= 1 and c2["dc"]["lists_huge_lists"] >= 1
    assert c2["dc"]["lists_tier_repeats"] >= 1 and c2["tm"]["pool_retries"] >= c2["dc"]["lists_tier_repeats"]
    assert c2["snap"] == R["wide"]["snap"], "the repeated pass against the same call on a fresh context"
    assert c3["snap"] == c1["snap"] and c3["dc"]["lists_tier_repeats"] == 0


# ---- g. pools and scratch regrown at small size -----------------------------------------------------------------------
def test_pools_and_huge_scratch_regrow_at_small_size(monkeypatch):
    """L3D_POOL_SCALE = 0.02 on hub34 (2862900 slots): candidate pools of 111 records (56783 candidates over 256 pools,
    thousands from one long list), edge pools of 55, and a k_lists_huge scratch of 3578 entries for 21 lists of more than
    1024: the pass is repeated for the candidates, for the edges and for the scratch."""
    R = _hub34_runs()
    sc = R["sc"]
    monkeypatch.setenv("L3D_POOL_SCALE", "0.02")
    g = _ctx(sc)
    r = _call(g, sc, HUB34_KNN, HUB_EPI)
    assert r["tm"]["pool_retries"] >= 1 and r["dc"]["lists_huge_scratch_regrows"] >= 1
    assert r["dc"]["lists_cand_pool_regrows"] + r["dc"]["lists_edge_pool_regrows"] >= 1
    assert r["snap"] == R["wide"]["snap"]


def test_edge_pools_regrow_while_the_candidate_pools_hold(monkeypatch):
    """The k_edges branch of the overflow flag.  18 views x 300 segments, 16 neighbours, kNN = 30: 1296000 slots, 48719
    candidates, 23199 edges, 16398 headers, spread evenly (no list beyond 418).  L3D_POOL_SCALE = 0.15 gives per pool 379
    candidate records (mean need 190), 189 edges (mean 91) and 94 headers (mean 64): the fullest header pool overflows,
    the candidate pools do not."""
    sc = dense18_scene()
    plain = _call(_ctx(sc), sc, 30, 0.1)
    monkeypatch.setenv("L3D_POOL_SCALE", "0.15")
    g = _ctx(sc)
    r = _call(g, sc, 30, 0.1)
    assert r["dc"]["lists_edge_pool_regrows"] >= 1 and r["dc"]["lists_cand_pool_regrows"] == 0
    assert r["tm"]["pool_retries"] == r["dc"]["lists_edge_pool_regrows"]
    assert r["snap"] == plain["snap"]
    _assert_equals_oracle(g, _oracle(dense18_scene, 30, 0.1), sc)


# ---- h. a chain deeper than the sweeps enqueued -----------------------------------------------------------------------
def test_chain_deeper_than_the_enqueued_sweeps():
    """A ring of 200 views x 100 segments with TWO neighbours, every segment the noise-free image of a 3D line: a view
    but the first has fresh hypotheses towards one view only, so their supporters are all inverse and a hypothesis turns
    positive one view after its supporter's source did.  A fresh context enqueues 9 sweeps; the chain needs about 13, so
    the first call takes the extra round (tail_run(c, false)), the second enqueues 16."""
    sc = chain_scene()
    g = _ctx(sc)
    first = _call(g, sc, 10, 0.25)
    assert first["tm"]["chain_extra_rounds"] >= 1
    _assert_equals_oracle(g, _oracle(chain_scene, 10, 0.25), sc)
    second = _call(g, sc, 10, 0.25, entries_before=first["tm"]["list_entries"])
    assert second["tm"]["chain_sweeps"] > LC.CHAIN_SWEEPS_FRESH and second["tm"]["chain_extra_rounds"] == 0
    assert second["snap"] == first["snap"]


# ---- i. views of mixed size -------------------------------------------------------------------------------------------
def test_views_of_1_2_64_65_and_300_segments_in_one_scene():
    """the one-wave tier's grid is (largest view, views): its workgroups return early for the short views.  1228 lists,
    total length 17235, 138 of them empty."""
    sc = mixed_scene()
    assert sorted({len(v.segs) for v in sc.views}) == [1, 2, 64, 65, 300]
    g = _ctx(sc)
    r = _call(g, sc, 10, 0.25)
    assert r["tiers"]["tier1"] == r["model"]["G"] == 1228
    _assert_equals_oracle(g, _oracle(mixed_scene, 10, 0.25), sc)


# ---- j. the sharded list pass on long lists ---------------------------------------------------------------------------
def test_sharded_list_pass_on_the_long_list_scene():
    """hub34 through the one-GPU emulation of the list pass sharded by views, two ranks: the second rank's views hold
    the hub and with it every list beyond 513"""
    R = _hub34_runs()
    sc = R["sc"]
    for g in H.sharded_list_pass(sc, 2, kNN=HUB34_KNN, epipolar_overlap=HUB_EPI):
        assert g.computeAffinity()
        assert _snapshot(g, sc) == R["wide"]["snap"]
