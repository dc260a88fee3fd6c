"""The numpy model of the affinity fill (tests/affinity_cases.py) on records written by hand, against values worked out by
hand; and on the scenes of tests/test_gpu_affinity.py through the CPU oracle: the model reproduces the oracle's edges,
order and row ids, its weights stay within the stated distance of the oracle's expf, and each scene really holds the
branches its GPU test names."""
import math

import numpy as np
import pytest

from line3dpp_amd._lib import HYP_REC_DTYPE
from tests import affinity_cases as AC

f32, f64 = np.float32, np.float64


# ---- hand-written records -------------------------------------------------------------------------------------------------
def _hand_lists():
    """Two views of three segments.  Segment 2 has no hypothesis; hypotheses 0..4 belong to segments 0, 1, 3, 4, 5.
    Candidates: 0 (0->3)  1 (0->4)  2 (1->3)  3 (1->2)  4 (3->0)  5 (3->1)  6 (4->0)  7 (5->1)"""
    hyps = np.zeros(5, HYP_REC_DTYPE)
    hyps["m"]["src_cam"] = [7, 7, 9, 9, 9]; hyps["m"]["src_seg"] = [0, 1, 0, 1, 2]; hyps["view"] = [0, 0, 1, 1, 1]
    rec = dict(N=8, H=5, G=6, V=2, n_cand=8, hyps=hyps, hyp_of_seg=np.array([0, 1, -1, 2, 3, 4], np.int32),
               surv_off=np.array([0, 2, 4, 4, 6, 7, 8], np.uint32), surv_sg=np.array([0, 0, 1, 1, 3, 3, 4, 5], np.uint32),
               surv_tg=np.array([3, 4, 3, 2, 0, 1, 0, 1], np.uint32), seg_base=np.array([0, 3, 6]), cams=np.array([7, 9]),
               view_k=np.ones(2, f32), medians=np.ones(2, f32), msdl_dev=np.zeros(1, f32), two_sigA_sqr=f32(200))
    return rec


def _edges(w):
    return list(zip(w["edges"]["i"].tolist(), w["edges"]["j"].tolist(), w["edges"]["w"].tolist()))


def test_stages_on_hand_written_similarities():
    rec = _hand_lists()
    ca, cb = AC.model_candidates(rec)
    assert ca.tolist() == [0, 0, 1, 1, 2, 2, 3, 4] and cb.tolist() == [2, 3, 2, -1, 0, 1, 0, 1]
    assert AC.reverse_index(rec).tolist() == [4, 6, 5, -1, 0, 2, 1, -1]
    # pair (0, 3): the earlier direction fails, the later passes -- the later one claims it (the reverse exists and fails);
    # pair (0, 4): the earlier passes, the later fails; pair (1, 3): exactly 0.5 and NaN -- neither passes;
    # candidate 7: its target's hypothesis 1 comes earlier, the target's list holds no reverse; hypothesis 1 is touched
    # first (and only) as a target
    simv = np.array([0.25, 0.75, 0.5, 0.0, 0.75, np.nan, 0.25, 0.9], f32)
    w = AC.run_stages(rec, simv)
    assert w["flag"].tolist() == [0, 1, 0, 0, 1, 0, 0, 1]
    assert w["epos"].tolist() == [0, 0, 1, 1, 1, 2, 2, 2] and w["epos_total"] == 3
    assert w["first_touch"].tolist() == [0, 5, 2, 1, 4]
    assert w["touch_flag"].tolist() == [1, 1, 1, 0, 1, 1] + [0] * 11
    assert w["touch_rank"][:6].tolist() == [0, 1, 2, 3, 3, 4] and w["touch_total"] == 5
    assert _edges(w) == [(0, 1, 0.75), (1, 0, 0.75), (2, 0, 0.75), (0, 2, 0.75), (3, 4, f32(0.9)), (4, 3, f32(0.9))]
    assert list(zip(w["l2g"]["cam"].tolist(), w["l2g"]["seg"].tolist())) == [(7, 0), (9, 1), (9, 0), (9, 2), (7, 1)]
    se, rows = AC.model_sequential(rec, simv)
    assert se.tobytes() == w["edges"].tobytes() and AC.l2g_of_segments(rec, rows).tobytes() == w["l2g"].tobytes()
    c = AC.class_counts(rec, simv)
    assert (c["back_rev_fail"], c["back_rev_absent"], c["fwd_rev_present"], c["rows_as_id2"]) == (1, 1, 1, 2)
    # both directions of (1, 3) pass: the earlier claims the pair, the later emits nothing
    simv[[2, 5]] = 0.8
    w = AC.run_stages(rec, simv)
    assert w["flag"].tolist() == [0, 1, 1, 0, 1, 0, 0, 1] and w["touch_total"] == 5 and w["epos_total"] == 4
    se, rows = AC.model_sequential(rec, simv)
    assert se.tobytes() == w["edges"].tobytes() and AC.l2g_of_segments(rec, rows).tobytes() == w["l2g"].tobytes()
    # nothing passes: no edge, no row
    w = AC.run_stages(rec, np.full(8, 0.5, f32))
    assert not w["flag"].any() and w["epos_total"] == 0 and w["touch_total"] == 0 and len(w["edges"]) == 0 and len(w["l2g"]) == 0
    assert np.all(w["first_touch"] == AC.EMPTY)


def _line(p, d, length=1.0, dp=(2.0, 2.0), view=0):
    h = np.zeros(1, HYP_REC_DTYPE)
    d = np.asarray(d, f64)
    h["P1"] = p; h["dir"] = d; h["P2"] = np.asarray(p, f64) + d * length; h["length"] = length
    h["m"]["d_p1"], h["m"]["d_p2"] = dp; h["view"] = view
    return h


def _sim(h1, h2, k=(0.5, 0.5), med=(10.0, 10.0), msdl=0.0, sigma_a=10.0):
    rec = dict(hyps=np.concatenate([h1, h2]), view_k=np.array(k, f32), medians=np.array(med, f32),
               msdl_dev=np.array([msdl], f32), two_sigA_sqr=f32(2 * sigma_a * sigma_a))
    s = AC.model_sim(rec, [0, 1], [1, 0])
    assert s[0].tobytes() == s[1].tobytes(), "sim(h1, h2) == sim(h2, h1) bit for bit"
    s64 = AC.model_sim_fp64(rec, [0], [1])[0]
    return s[0], s64


def test_similarity_on_hand_written_hypotheses():
    ex = lambda y: f32(math.exp(f64(f32(y))))
    x = [1.0, 0.0, 0.0]
    base = _line([0, 0, 0], x)
    # parallel at distance 1, sigma = depth * k = 1, reg = 2: y = -1/2
    s, s64 = _sim(base, _line([0, 1, 0], x))
    assert s == ex(-0.5) and abs(s64 - math.exp(-0.5)) < 1e-15
    # identical lines: every term is 0, the similarity exactly 1; opposite directions fold 180 to 0
    assert _sim(base, _line([0, 0, 0], x))[0] == 1.0
    assert _sim(base, _line([1, 0, 0], [-1.0, 0, 0]))[0] == 1.0
    # the depth above the cutoff: sigma = cutoff * k (view median 1, then the scene's median 0.5)
    assert _sim(base, _line([0, 1, 0], x), med=(1.0, 1.0))[0] == ex(-1.0 / 0.5)
    assert _sim(base, _line([0, 1, 0], x), med=(1.0, 1.0), msdl=0.5)[0] == ex(-1.0 / 0.125)
    assert _sim(base, _line([0, 1, 0], x), med=(1.0, 1.0), msdl=1e-13)[0] == ex(-1.0 / 0.5)      # at most L3D_EPS: not used
    # an angle of exactly 90 degrees is not folded; 120 folds to 60 (through a point of the first line: distances of the
    # second line's points dominate, so the regulariser is made wide)
    wide = dict(k=(1e3, 1e3))
    assert _sim(base, _line([0, 0, 0], [0.0, 1.0, 0.0]), **wide)[0] == ex(-f32(90) * f32(90) / f32(200))
    a = math.radians(120)
    s, s64 = _sim(base, _line([0, 0, 0], [math.cos(a), math.sin(a), 0.0]), **wide)
    ang = f32(180) - f32(math.acos(f64(f32(math.cos(a)))) / math.pi * 180.0)
    assert s == ex(-ang * ang / f32(200)) and abs(s64 / math.exp(-18.0) - 1) < 1e-3
    # k = 0: a regulariser of 0; distance 0 gives NaN in all four position terms, which fminf skips -- the angle decides;
    # a distance above 0 gives -inf and a similarity of 0
    assert _sim(base, _line([0, 0, 0], x), k=(0.0, 0.0))[0] == 1.0
    assert _sim(base, _line([0, 1, 0], x), k=(0.0, 0.0))[0] == 0.0
    # a hypothesis shorter than L3D_EPS
    assert _sim(base, _line([0, 0, 0], x, length=1e-13))[0] == 0.0


# ---- the scenes through the CPU oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AC.CASES))
def test_model_reproduces_the_oracle(name):
    """records_from_oracle, then every stage: the oracle's edge ids, order and rows; weights within 2 ulp of the oracle's
    expf and differing in at most 1 % of the edges (measured: at most 1 ulp; 1 of 2217 edges on c0_six, 2 of 2137 on
    c0_six_n128x, 1 of 5420 on c0_eight, 1 of 332 on unequal_views, none elsewhere -- the kernel
    defines a weight as (float)exp((double)y), two correctly rounded steps, the reference calls expf; each lies within
    about half an ulp of the true value, so they differ by one ulp at the most, where the value is near a rounding
    boundary); the sequential restatement gives the staged model's bytes; every class count is the one written beside
    the scene."""
    r = AC.oracle_run(name)
    rec, w = r["rec"], r["w"]
    assert r["same_ids"], "edge ids and order"
    assert np.array_equal(r["l2g"].reshape(-1, 2), np.stack([w["l2g"]["cam"], w["l2g"]["seg"]], 1)), "rows"
    print(f"{name}: {len(r['edges']) // 2} edges, {r['n_diff']} weights differ from the oracle's, largest distance {r['max_ulp']} ulp")
    assert r["max_ulp"] <= 2 and r["n_diff"] <= max(1, len(r["edges"]) // 200)
    se, rows = AC.model_sequential(rec, w["simv"])
    assert se.tobytes() == w["edges"].tobytes() and AC.l2g_of_segments(rec, rows).tobytes() == w["l2g"].tobytes()
    c = AC.class_counts(rec)
    print(c)
    assert set(AC.CASES[name].expect) == set(c), "every count is written beside the scene"
    assert c == AC.CASES[name].expect
    ca, cb = w["cand_a"], w["cand_b"]
    e = np.nonzero(AC.eligible(ca, cb))[0]
    if len(e):
        ref = AC.model_sim_fp64(rec, ca[e], cb[e])
        big = ref > 1e-30
        rel = np.abs(w["simv"][e][big].astype(f64) - ref[big]) / ref[big]
        print(f"{name}: float path against fp64 throughout: largest relative error {rel.max():.3g} (contract 1e-4)")


def test_launch_edges_and_scan_tiles_of_the_scenes():
    n = {k: c.expect["N"] for k, c in AC.CASES.items()}
    assert n["c0_six_n128x"] % 128 == 0 and n["c0_six_n128x1"] % 128 == 1 and n["c0_six_n128x"] % 256 != 0
    assert n["c0_six"] > 4096 and 2 * n["c0_six"] > 2 * 4096 and n["tiny"] < 128
    assert sorted(len(v.segs) for v in AC.CASES["unequal_views"].scene().views) == [255, 256, 257, 513]


def test_model_library_functions_against_200_bits():
    """the model's float32(exp(float64(y))) and float32(acos(x) / pi * 180) on c0_six's own arguments against a 200-bit
    evaluation rounded once to 24 bits: no difference, so a difference between kernel and model is the kernel's"""
    import mpmath
    r = AC.oracle_run("c0_six")
    rec, w = r["rec"], r["w"]
    e = np.nonzero(AC.eligible(w["cand_a"], w["cand_b"]))[0]
    _, d = AC.model_sim(rec, w["cand_a"][e], w["cand_b"][e], details=True)
    mpmath.mp.prec = 200
    r24 = lambda v: float(mpmath.mpf(v, prec=24, rounding="n"))
    y = d["y"][np.isfinite(d["y"]) & (d["y"] > -80)]          # (float32 results in the normal range)
    got = AC._libm(math.exp, y.astype(f64)).astype(f32)
    want = np.array([r24(mpmath.exp(mpmath.mpf(float(v)))) for v in y], f32)
    assert len(y) > 1000 and got.tobytes() == want.tobytes()
    x = d["acos_arg"]
    got = (AC._libm(math.acos, x.astype(f64)) / math.pi * 180.0).astype(f32)
    want = np.array([r24(mpmath.acos(mpmath.mpf(float(v))) / mpmath.pi * 180) for v in x], f32)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["c0_six", "unequal_views"])
def test_collinear_model_reproduces_the_oracle(name):
    r = AC.oracle_run(name)
    o, sc = AC.CASES[name].oracle(collinearity=2.0)
    m = AC.model_collinear(r["rec"], sc, 2.0)
    sb = r["rec"]["seg_base"]
    for i, v in enumerate(sc.views):
        off, idx = o.collinear(v.cam, len(v.segs))
        a, b = sb[i], sb[i + 1]
        assert np.array_equal(off, m["coll_off"][a:b + 1] - m["coll_off"][a]), ("list lengths", v.cam)
        assert np.array_equal(idx, m["coll_idx"][m["coll_off"][a]:m["coll_off"][b]]), ("lists", v.cam)
    oe, ol = o.affinity()
    assert len(oe) > len(r["edges"]), "the collinear links add edges"
    assert np.array_equal(oe["i"], m["edges"]["i"]) and np.array_equal(oe["j"], m["edges"]["j"])
    assert np.array_equal(ol, np.stack([m["l2g"]["cam"], m["l2g"]["seg"]], 1))
    d = AC.ulp_distance(oe["w"], m["edges"]["w"])
    print(f"{name}: {len(m['coll_idx'])} collinear entries, {len(m['child_seg'])} child and {len(m['own_seg'])} own candidates, "
          f"{len(oe) // 2} edges, {(d > 0).sum() // 2} weights differ, largest {d.max()} ulp")
    assert d.max() <= 2 and (d > 0).sum() // 2 <= max(1, len(oe) // 200)
