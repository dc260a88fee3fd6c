"""The host model of phase B's tail (tests/tail_cases.py) on records written by hand, against values worked out by hand;
and the scenes of tests/test_gpu_tail.py through the CPU oracle: each really holds what its GPU test names."""
import functools

import numpy as np

from tests import tail_cases as TC

f32 = np.float32
CAMS = [0, 1, 2, 3]
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
SEG_BASE = [0, 2, 4, 6, 8]


def _hand_records():
    """Four views of two segments.  Slots: 10 (A), 11 (B), 12 (R), 16 (S) fresh in view 0; 20 (C), 21 (X) fresh in view 1;
    30 (D) fresh in view 2; F is the inverse copy of slot 10 in view 1, G that of slot 21 in view 3."""
    return TC.make_records(SEG_BASE, [
        # segment 0 (view 0): A and B support each other, equal scores: a tie for best
        dict(g=0, ref=10, canon=0, pair=0, tgt_seg=0, dp=(4.0, 5.0), edges=[(11, 0.9, False, 2)]),
        dict(g=0, ref=11, canon=1, pair=1, tgt_seg=1, dp=(6.0, 7.0), edges=[(10, 0.9, False, 1)]),
        # segment 1 (view 0): R's camera 2 comes back after camera 3 with a larger similarity; S scores exactly 0.75
        dict(g=1, ref=12, canon=0, pair=0, tgt_seg=1, dp=(9.0, 1.0), edges=[(13, 0.6, False, 2), (14, 0.7, False, 3), (15, 0.9, False, 2)]),
        dict(g=1, ref=16, canon=1, pair=1, tgt_seg=0, dp=(2.0, 2.0), edges=[(12, 0.75, False, 1)]),
        # segment 2 (view 1): F exists because slot 10 is positive; C's only supporter is inverse, its source is A (link 1)
        dict(g=2, ref=10, canon=0, pair=0, inv=True, tgt_seg=0, dp=(3.0, 8.0), edges=[(20, 0.8, False, 2)]),
        dict(g=2, ref=20, canon=1, pair=3, tgt_seg=0, dp=(1.0, 1.5), edges=[(10, 0.8, True, 0)]),
        # segment 3 (view 1): X's only supporter is an inverse hypothesis of a slot without a header: never positive
        dict(g=3, ref=21, canon=0, pair=4, tgt_seg=0, edges=[(99, 0.9, True, 0)]),
        # segment 4 (view 2): D hangs on C (link 2) and scores exactly 0.75: kept, but the segment is gated
        dict(g=4, ref=30, canon=2, pair=5, tgt_seg=1, dp=(5.0, 5.0), edges=[(20, 0.75, True, 1)]),
        # segment 6 (view 3): G is the inverse copy of X, which is not positive: it does not exist
        dict(g=6, ref=21, canon=0, pair=4, inv=True, tgt_seg=1, edges=[(31, 0.9, False, 2)]),
    ])


def test_hand_written_records_stage_by_stage():
    rec = _hand_records()
    w = TC.run_model(rec, PAIRS, CAMS)
    H = rec["headers"]
    # exists: a two-link chain A -> C -> D needs three rounds; X never turns positive, G does not exist
    assert w["chain_rounds"] == 3
    assert rec["hdr_positive"].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 0]
    assert rec["edge_positive"].tolist() == [1, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0]
    assert (H["state"] & 1).tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 0]
    # score: in float32, in edge order; camera 2 comes back and its 0.9 replaces its 0.6
    r = f32(f32(f32(f32(0.6) + f32(0.7)) - f32(0.6)) + f32(0.9))
    expect = [f32(0.9), f32(0.9), r, f32(0.75), f32(0.8), f32(0.8), f32(0), f32(0.75), f32(0)]
    assert H["score3D"].view(np.uint32).tolist() == np.array(expect, f32).view(np.uint32).tolist()
    assert r != f32(f32(f32(0.6) + f32(0.7)) + f32(0.9)), "the rule of a camera that is merely the last one gives another value"
    # view max, keep (S: 0.75 > 0.1f * r; X: score 0)
    assert rec["max_score_bits"].max(1).view(f32).tolist() == [r, f32(0.8), f32(0.75), f32(0)]
    assert ((H["state"] & 2) != 0).tolist() == [True, True, True, True, True, True, False, True, False]
    # best: the first strict maximum; on a tie the smaller canonical index
    assert rec["kept_cnt"].tolist() == [2, 2, 2, 0, 1, 0, 0, 0]
    pack = lambda s, canon: (int(f32(s).view(np.uint32)) << 32) | (0xFFFFFFFF - canon)
    assert rec["best_pack"].tolist() == [pack(0.9, 0), pack(r, 0), pack(0.8, 0), 0, pack(0.75, 2), 0, 0, 0]
    # gate: 0.75 is not > 0.75 -- segment 4 keeps a header and writes nothing
    assert rec["surv_off"].tolist() == [0, 2, 4, 6, 6, 6, 6, 6, 6] and rec["hyp_off"].tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 3]
    assert (rec["n_surv"], rec["n_hyps"]) == (6, 3)
    assert rec["hyp_of_seg"].tolist() == [0, 1, 2, -1, -1, -1, -1, -1]
    # write-out: canonical order; an inverse match points back at its source view
    assert rec["surv_sg"].tolist() == [0, 0, 1, 1, 2, 2] and rec["surv_tg"].tolist() == [2, 5, 3, 4, 0, 4]
    assert w["surv"]["tgt_cam"].tolist() == [1, 2, 1, 2, 0, 2] and w["surv"]["src_cam"].tolist() == [0, 0, 0, 0, 1, 1]
    assert rec["depths"].tolist() == [[4.0, 5.0], [9.0, 1.0], [3.0, 8.0]]
    # median: sorted (1, 4, 5, 9)[2]; sorted (3, 8)[1]; no best hypothesis: L3D_EPS
    assert rec["medians"].tolist() == [5.0, 8.0, TC.L3D_EPS, TC.L3D_EPS]


def test_keep_limit_is_strict_and_in_float32():
    """0.1f * 8 == 0.8f exactly: a score of 0.8f is not above the limit; the next float is"""
    up = np.nextafter(f32(0.8), f32(1))
    rec = TC.make_records([0, 3], [
        dict(g=0, ref=1, canon=0, edges=[(2, 1.0, False, 1), (3, 1.0, False, 2), (4, 1.0, False, 3), (5, 1.0, False, 4),
                                         (6, 1.0, False, 5), (7, 1.0, False, 6), (8, 1.0, False, 7), (9, 1.0, False, 8)]),
        dict(g=1, ref=10, canon=0, edges=[(11, 0.8, False, 1)]),
        dict(g=2, ref=12, canon=0, edges=[(13, up, False, 1)])])
    TC.run_model(rec, [(0, 1)], [0, 1])
    assert rec["headers"]["score3D"].tolist() == [8.0, f32(0.8), up]
    assert ((rec["headers"]["state"] & 2) != 0).tolist() == [True, False, True]
    assert rec["hyp_of_seg"].tolist() == [0, -1, 1]


def test_same_camera_keeps_the_larger_and_records_by_segment_ignore_the_pools():
    assert TC.accumulate([0.9, 0.6], [1, 1]) == f32(0.9)
    assert TC.accumulate([0.6, 0.9], [1, 1]) == f32(f32(f32(0.6) - f32(0.6)) + f32(0.9))
    a = _hand_records(); TC.run_model(a, PAIRS, CAMS)
    b = _hand_records()
    b["edge_index"] = b["edge_index"] + 1000           # the same edges elsewhere in the pools
    b["headers"]["edge_begin"] += 1000
    b["hdr_pool"][:] = 3
    TC.run_model(b, PAIRS, CAMS)
    assert TC.records_by_segment(a) == TC.records_by_segment(b)
    assert a["surv_tg"].tolist() == b["surv_tg"].tolist() and a["medians"].tolist() == b["medians"].tolist()


# ---- the GPU scenes hold what their tests name (CPU oracle) -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _counts(scene_fn, kNN):
    from oracle.oracle import Oracle
    sc = scene_fn()
    o = Oracle(record_scored=True, threads=8)
    o.add_scene(sc)
    o.match_images(kNN=kNN, epi_overlap=TC.EPI)
    c = TC.oracle_counts(o, sc)
    for v in sc.views:      # the restatement of filterMatches in oracle_counts against the oracle's own median
        assert c["views"][v.cam]["median"] == o.view_info(v.cam)["median_depth"], v.cam
    print(sc.name, {k: v for k, v in c.items() if k != "views"},
          [(cam, v["n_pos"], v["n_best"]) for cam, v in c["views"].items()])
    return c, sc


def test_scenes_of_the_accumulation_gate_and_tie_tests():
    c, _ = _counts(TC.accumulation_scene, TC.KNN)
    assert min(v["n_pos"] for v in c["views"].values()) >= 100 and c["passed"] >= 500
    c, _ = _counts(TC.gate_scene, TC.KNN)
    assert c["gated"] >= 10 and c["passed"] >= 10, c        # 68 and 209
    c, _ = _counts(TC.ties_scene, TC.KNN)
    assert c["ties"] >= 20 and c["gated"] >= 10, c          # 58 ties among 58 passed, 28 gated
    assert max(v["median_dups"] for v in c["views"].values()) >= 2, "a view whose median value occurs twice"
    assert sum(v["n_pos"] == 0 for v in c["views"].values()) >= 1


def test_scene_of_the_view_maximum_test():
    c, sc = _counts(TC.view_max_scene, TC.KNN)
    n_pos = [c["views"][v.cam]["n_pos"] for v in sc.views]
    assert n_pos.count(1) >= 1 and n_pos.count(0) >= 1, n_pos    # [4, 0, 4, 2, 2, 6, 1, 3, 3, 3, 5, 2]
    assert sorted({len(v.segs) for v in sc.views}) == [3, 4, 5, 6, 300]


def test_scene_of_the_median_tests():
    c, sc = _counts(TC.medians_scene, TC.KNN)
    n_best = [c["views"][v.cam]["n_best"] for v in sc.views]
    # [512, 514, 514, 513, 4, 3, 1169, 1168, 1168, 2, 1, 3, 1, 2, 2, 0, 1, 2, 1, 1, 1]
    assert {0, 1, 512, 513} <= set(n_best) and max(n_best) > 1024, n_best
    assert n_best[0] == 512 and n_best[3] == 513               # n / 2 even and odd, n = 1024 and 1026
    for cam in (0, 3, 6):
        assert c["views"][cam]["depth_span"] >= 16, c["views"][cam]
    assert c["ties"] >= 20


def test_scenes_of_the_grid_and_keep_all_tests():
    sc = TC.grid_scene()
    assert sum(len(v.segs) for v in sc.views) == 12600          # G + 1 > 256 x 16 and < 256 x 256
    c, _ = _counts(TC.keep_all_scene, 0)
    assert c["passed"] >= 50 and c["gated"] >= 10, c            # 107 and 21
