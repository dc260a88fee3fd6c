"""Phase B's tail on the MI355X record by record (k_chain_sweep / k_chain_sweep_list, k_hyp_scores, k_hyp_filter,
k_seg_filter, k_seg_write, k_median_all), through the read-only hook l3d_debug_tail_records (Line3D.tail_records()).

Every test runs matchImages, reads the records the converged pass left behind, and checks EVERY stage against the host
model of tests/tail_cases.py, each stage fed with the records the hook returned for the stage before: bit for bit, except
the 3D end points of the best hypotheses (100 x the fp64 to long-double difference of the model; measured over these
scenes: end points 1.5e-13, direction 2.9e-14, length 1.6e-13 before the factor).  Then the accessors -- matches(),
best(), view_info()["median_depth"], timings() -- are checked against the same records.  Each test asserts from the
records that its branch was reached; tests/test_tail_cases.py shows the same with the CPU oracle."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import tail_cases as TC

pytestmark = pytest.mark.gpu


def _ctx(sc):
    from line3dpp_amd.api import Line3D
    g = Line3D()
    g.add_scene(sc)
    return g


def _check_accessors(g, sc, rec, w):
    """what the library hands out, against the records: matches per view, best hypotheses, medians, counts"""
    cams = [v.cam for v in sc.views]
    so, sb = rec["surv_off"].astype(np.int64), rec["seg_base"].astype(np.int64)
    for vi, cam in enumerate(cams):
        m, off = g.matches(cam)
        a, b = so[sb[vi]], so[sb[vi + 1]]
        assert m.tobytes() == w["surv"][a:b].tobytes(), ("matches", cam)
        assert np.array_equal(off, so[sb[vi]:sb[vi + 1] + 1] - a), ("match offsets", cam)
        assert g.view_info(cam)["median_depth"].tobytes() == rec["medians"][vi].tobytes(), ("median", cam)
    s2, s3, bm = g.best()
    assert bm.tobytes() == w["best"].tobytes(), "best(): the Match records"
    assert np.array_equal(s2["cam"], w["best"]["src_cam"]) and np.array_equal(s2["seg"], w["best"]["src_seg"])
    model, tol, diff = TC.hyprec_tolerances(sc, g.translation(), w["best"])
    if len(bm):
        err = dict(P=max(np.abs(s3["P1"] - model["P1"]).max(), np.abs(s3["P2"] - model["P2"]).max()),
                   dir=np.abs(s3["dir"] - model["dir"]).max(), length=np.abs(s3["length"].astype(np.float64) - model["length"]).max())
        print(f"{sc.name}: HypRec fp64 vs long double {diff}, tolerance {tol}, kernel vs fp64 model {err}")
        assert np.all(s3["valid"] == 1) and model["length"].min() > 1e-6
        assert err["P"] <= tol["P"] and err["dir"] <= tol["dir"] and err["length"] <= tol["length"], (err, tol)
    tm = g.timings()
    assert (tm["list_headers"], tm["support_words"]) == (rec["n_headers"], rec["n_edges"])


def _run(sc, kNN=TC.KNN, g=None):
    """matchImages on a fresh context (or on `g`), every stage and every accessor checked -> (g, rec, write-out model)"""
    g = g or _ctx(sc)
    assert g.matchImages(kNN=kNN, epipolar_overlap=TC.EPI), g.last_status
    rec = g.tail_records()
    assert rec is not None
    w = TC.check_stages(rec, g.pairs()[0], [v.cam for v in sc.views])
    _check_accessors(g, sc, rec, w)
    return g, rec, w


def _same_results(a, b):
    """two passes reached the same records (as sets per segment) and the same outputs"""
    assert TC.records_by_segment(a) == TC.records_by_segment(b)
    for k in ("max_score_bits", "kept_cnt", "best_pack", "off64s", "surv_off", "hyp_off", "hyp_of_seg", "surv_sg", "surv_tg",
              "depths", "medians"):
        x, y = (a[k].max(1), b[k].max(1)) if k == "max_score_bits" else (a[k], b[k])
        assert x.tobytes() == y.tobytes(), k


@functools.lru_cache(maxsize=None)
def _medians_run():
    sc = TC.medians_scene()
    return (sc,) + _run(sc)


@functools.lru_cache(maxsize=None)
def _accumulation_run():
    sc = TC.accumulation_scene()
    return (sc,) + _run(sc)


# ---- accumulation -------------------------------------------------------------------------------------------------------
def test_score_accumulation_over_edge_counts_and_cameras():
    """k_hyp_scores reads four edges per round trip, clamped to the last one.  Noise-free hub scene, 10 views x 150, every view a
    neighbour of every other, the 80 longest segments of a view doubled: headers with 1, 2, 3, 4, 5 and 8 edges (419,
    1413, 448, 998, 207 and 37 of them); consecutive supporters of one camera with the later one larger (replace) and
    smaller (keep); inverse supporters that do not exist.  (A camera that RETURNS after another one cannot occur in the
    records: every camera shares exactly one pair with the view, and the hypotheses of a pair are contiguous in
    canonical order -- asserted here; the model's rule for it is checked on hand-written records.)"""
    sc, g, rec, w = _accumulation_run()
    st = TC.record_stats(rec)
    print(st)
    assert {1, 2, 3, 4, 5, 8} <= set(st["edge_cnts"]), st
    assert st["later_larger"] >= 1 and st["later_smaller"] >= 1 and st["dead_inverse_supporters"] >= 1, st
    assert st["camera_returns"] == 0, st


# ---- view maximum -------------------------------------------------------------------------------------------------------
def test_view_maximum_of_a_single_positive_header_and_of_none():
    sc = TC.view_max_scene()
    g, rec, w = _run(sc)
    fc = TC.filter_counts(rec)
    print(fc)
    assert (fc["n_pos"] == 1).any() and (fc["n_pos"] == 0).any(), fc["n_pos"]
    view = TC.header_view(rec)
    for v in np.nonzero(fc["n_pos"] == 0)[0]:      # limit 0: nothing kept, nothing written, median L3D_EPS
        assert not rec["max_score_bits"][v].any() and not (rec["headers"]["state"][view == v] & TC.HYP_KEEP).any()
        assert fc["n_best"][v] == 0 and rec["medians"][v] == TC.L3D_EPS
    for v in np.nonzero(fc["n_pos"] == 1)[0]:      # the one positive header is the maximum and is kept
        h = rec["headers"][(view == v) & (rec["headers"]["score3D"] > 0)]
        assert rec["max_score_bits"][v].max() == h["score3D"].view(np.uint32)[0] and h["state"][0] & TC.HYP_KEEP


def test_view_maximum_of_three_views_in_one_wave():
    """the vote of k_hyp_scores runs once per distinct view among a wave's positive headers: the medians scene holds
    the tiny views (3 to 6 segments) of lists_cases.mixed_scene beside views of 300 and 1300"""
    sc, g, rec, w = _medians_run()
    st = TC.record_stats(rec)
    print(st)
    assert st["views_in_one_wave"] >= 3, st


# ---- best hypothesis and gates ------------------------------------------------------------------------------------------
def test_ties_for_best_go_to_the_smaller_canonical_index():
    sc = TC.ties_scene()
    g, rec, w = _run(sc)
    fc = TC.filter_counts(rec)
    print(fc)
    assert fc["ties"] >= 20, fc
    Hd = rec["headers"]
    best_s = (rec["best_pack"] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    best_canon = 0xFFFFFFFF - (rec["best_pack"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    at_best = ((Hd["state"] & TC.HYP_KEEP) != 0) & (Hd["score3D"] == best_s[Hd["g"]])
    for seg in np.unique(Hd["g"][at_best]):
        assert best_canon[seg] == Hd["canon"][at_best & (Hd["g"] == seg)].min(), seg
    d = [rec["depths"][rec["hyp_off"][rec["seg_base"][v]]:rec["hyp_off"][rec["seg_base"][v + 1]]].ravel() for v in range(rec["V"])]
    assert any(len(x) and (x == rec["medians"][v]).sum() >= 2 for v, x in enumerate(d)), "a median value that occurs twice"


def test_gated_segments_write_nothing():
    sc = TC.gate_scene()
    g, rec, w = _run(sc)
    fc = TC.filter_counts(rec)
    print(fc)
    assert fc["gated"] >= 10 and fc["passed"] >= 10, fc
    gated = (rec["kept_cnt"] > 0) & ~w["gate_ok"]
    assert np.all(rec["hyp_of_seg"][gated] == -1)
    assert np.all(rec["surv_off"][1:][gated] == rec["surv_off"][:-1][gated]) and np.all(rec["hyp_off"][1:][gated] == rec["hyp_off"][:-1][gated])


# ---- write-out grid -----------------------------------------------------------------------------------------------------
def test_write_out_grid_decided_by_the_segments_and_by_the_headers(monkeypatch):
    """k_seg_write launches max(G + 1, pools x hcap) threads.  12600 segments, mostly clutter, kNN = 1: with the default
    pools (stride 256) the header term decides; with L3D_POOL_SCALE = 0.01 the pools start at a stride of 16 and the
    segments (and the write of the end offsets, thread G) lie beyond the last header slot."""
    sc = TC.grid_scene()
    g, rec, w = _run(sc, kNN=1)
    assert rec["G"] + 1 < rec["pools"] * rec["hcap"], (rec["G"], rec["hcap"])
    monkeypatch.setenv("L3D_POOL_SCALE", "0.01")
    g2, rec2, w2 = _run(sc, kNN=1)
    assert rec2["G"] + 1 > rec2["pools"] * rec2["hcap"], (rec2["G"], rec2["hcap"])
    assert rec2["n_hyps"] >= 10 and rec2["hyp_off"][-1] == rec2["n_hyps"] and rec2["surv_off"][-1] == rec2["n_surv"]
    _same_results(rec, rec2)


def test_pass_repeated_after_a_pool_regrow_and_second_call(monkeypatch):
    """L3D_POOL_SCALE = 0.02 on the accumulation scene: header pools of 16 overflow, the library repeats the pass with
    larger ones (its own retry path); and a second matchImages on one context: the same records as a fresh context"""
    sc, g, rec, w = _accumulation_run()
    monkeypatch.setenv("L3D_POOL_SCALE", "0.02")
    g2, rec2, w2 = _run(sc)
    assert g2.timings()["pool_retries"] >= 1 and rec2["hcap"] != rec["hcap"]
    _same_results(rec, rec2)
    monkeypatch.delenv("L3D_POOL_SCALE")
    g3, rec3, w3 = _run(sc, g=g2)
    _same_results(rec, rec3)


def test_tail_started_over_after_a_chain_deeper_than_the_sweeps():
    """tests/test_gpu_lists.py's chain scene: the first call needs more sweeps than it enqueued and runs the tail again
    from the chain's state (fresh == false): changed[], the maxima, counts and best packs are zeroed and rebuilt"""
    from tests.test_gpu_lists import chain_scene
    sc = chain_scene()
    g, rec, w = _run(sc)
    assert g.timings()["chain_extra_rounds"] >= 1
    assert TC.model_exists(rec)["rounds"] > 9


# ---- medians ------------------------------------------------------------------------------------------------------------
def test_medians_at_the_strides_of_the_select_and_at_its_top_digit():
    """k_median_all: 1024 threads stride over n = 2 x (best hypotheses) depths -- n of 0, 2, 1024, 1026 and more than 2048
    (one, two and three rounds), n / 2 even and odd; near and far structure in one view, so that the top radix digit
    (sign and upper exponent bits) of the depths differs inside a view"""
    sc, g, rec, w = _medians_run()
    fc = TC.filter_counts(rec)
    print(fc)
    n_best = fc["n_best"].tolist()
    assert {0, 1, 512, 513} <= set(n_best) and max(n_best) > 1024, n_best
    for v in (n_best.index(512), n_best.index(513), int(np.argmax(n_best))):
        d = rec["depths"][rec["hyp_off"][rec["seg_base"][v]]:rec["hyp_off"][rec["seg_base"][v + 1]]].ravel()
        assert d.max() / d.min() >= 16 and len(set((d.view(np.uint32) >> 24).tolist())) >= 2, (v, d.min(), d.max())


# ---- keep-all mode and the sharded pass -----------------------------------------------------------------------------------
def test_keep_all_mode():
    sc = TC.keep_all_scene()
    g, rec, w = _run(sc, kNN=0)
    fc = TC.filter_counts(rec)
    assert fc["passed"] >= 50 and fc["gated"] >= 10, fc


def test_sharded_list_pass_reaches_the_same_records():
    sc, g, rec, w = _accumulation_run()
    for g2 in H.sharded_list_pass(sc, 2, kNN=TC.KNN, epipolar_overlap=TC.EPI):
        rec2 = g2.tail_records()
        w2 = TC.check_stages(rec2, g2.pairs()[0], [v.cam for v in sc.views])
        _check_accessors(g2, sc, rec2, w2)
        _same_results(rec, rec2)


def test_hook_needs_matches():
    sc = TC.keep_all_scene()
    g = _ctx(sc)
    assert g.tail_records() is None and g.last_status == -7      # L3D_ERR_STATE
