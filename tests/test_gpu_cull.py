"""The epipolar-band culling of phase A (make_cull -> k_cull_prepare, whose tables k_order_items and the walk of k_match_pairs
trust) on the hand-built geometry of tests/cull_cases.py, stage by stage.

Every case runs bounded kNN in the tile form and keep-all (kNN = 0), class_edges in the row form as well.  After
l3d_match_pairs the tables of every pair are read back as they lie on the device (Line3D.cull_state) and held against the
host model (tests/cull_model.py), every stage of which is fed the DUMPED output of the stage before it:

  * culled or refused as the model decides, and as timings()["culled_pairs"] counts;
  * a band is exactly (-inf, +inf) where the model says unbounded and nowhere else; every bounded band within one fp32 ulp
    of the model's (the fp64 evaluation errs by about 1e-12 at denominators >= 0.05, far below half an ulp: rounding can
    move a value to its neighbour at most) -- the count of bands that differ at all is printed;
  * every match the oracle accepts at an overlap threshold of 1e-6 has intersecting DUMPED bands;
  * src_perm without its padding is a permutation of the rows, tgt_perm of the targets;
  * the padded layout: classes ascending, each from a multiple of R, padding = kEmpty with the band (+inf, -inf), the
    region tile_src_cap(Ms, R) long, padding behind the last class; the unpadded layout: classes ascending;
  * inside a class the band starts do not decrease -- exactly with 64-bit keys, up to one quantisation step with 32-bit
    keys (and by element where the start is the same for all: unbounded rows, an empty or zero-width span);
  * chunk_band[c] is exactly the hull of the 64 dumped target bands of chunk c;
  * the slots equal the brute-force path's (np.array_equal) and the oracle's (helpers.compare_pair: nothing missing, nothing
    extra, bit for bit, no row in another order)."""
import numpy as np
import pytest

from line3dpp_amd._lib import EMPTY
from tests import cull_cases as CC
from tests import cull_model as CM
from tests import helpers as H

pytestmark = pytest.mark.gpu

L3D_ERR_STATE = -7
FORMS = {"tile": (CC.KNN, "16", 16), "row": (CC.KNN, "0", 64), "keep": (0, None, 0)}   # kNN, L3D_MATCH_TILE, layout rows
BAND_STATS = dict(bands=0, differ=0)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in ("L3D_MATCH_TILE", "L3D_KEEPALL_TWO_PASS", "L3D_KEEPALL_NO_CULL", "L3D_KEEPALL_CAP", "L3D_NO_FASTMATH"):
        monkeypatch.delenv(k, raising=False)


def _run(name, form, monkeypatch, brute=False):
    """one matchBegin + matchPairs of a case -> (slots per pair, cull_state per pair or None, culled_pairs)"""
    from line3dpp_amd.api import Line3D
    kNN, tile, _ = FORMS[form]
    if tile is not None:
        monkeypatch.setenv("L3D_MATCH_TILE", tile)
    sc = CC.scene(name)
    g = Line3D()
    g.add_scene(sc)
    if brute:
        g.set_brute_force(1)
    assert g.matchBegin(kNN=kNN, epipolar_overlap=CC.EPI), g.last_status
    pairs, _ = g.pairs()
    assert [tuple(int(x) for x in p) for p in pairs] == CC.pair_list(sc)
    assert g.cull_state(0) is None and g.last_status == L3D_ERR_STATE, "no launch yet"
    assert g.matchPairs(0, len(pairs)), g.last_status
    states = None if brute else [g.cull_state(p) for p in range(len(pairs))]
    if not brute:
        assert all(s is not None for s in states), g.last_status
    culled = g.timings()["culled_pairs"]
    slots = [g.pair_slots(p) for p in range(len(pairs))]
    g.matchAbort()
    assert g.cull_state(0) is None and g.last_status == L3D_ERR_STATE, "the call is closed"
    g.close()
    monkeypatch.delenv("L3D_MATCH_TILE", raising=False)
    return slots, states, culled


def _ulp_apart(a, b):
    """fp32 values at most one ulp apart (or equal)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a == b) | (np.nextafter(a, b) == b)


def _assert_bands(where, lo, hi, mlo, mhi, mcls):
    unb = mcls == 0
    assert np.array_equal(np.isneginf(lo) & np.isposinf(hi), unb), (where, "class-0 bands", int(unb.sum()))
    assert np.isfinite(lo[~unb]).all() and np.isfinite(hi[~unb]).all(), where
    ok = _ulp_apart(lo[~unb], mlo[~unb]) & _ulp_apart(hi[~unb], mhi[~unb])
    assert ok.all(), (where, "bounded bands beyond one ulp", int((~ok).sum()), lo[~unb][~ok][:3], mlo[~unb][~ok][:3])
    BAND_STATS["bands"] += 2 * int((~unb).sum())
    BAND_STATS["differ"] += int((lo[~unb] != mlo[~unb]).sum() + (hi[~unb] != mhi[~unb]).sum())


def _assert_order(where, cls, start, elem, step, exact):
    """positions in walk order: classes ascending; inside a class the starts do not decrease by more than `step` (exact: not
    at all, equal starts by element); step == 0 with 32-bit keys: every start quantises to 0, the element decides"""
    assert (np.diff(cls) >= 0).all(), (where, "classes ascend")
    worst = 0.0
    for k in np.unique(cls):
        m = cls == k
        s, e = start[m].astype(np.float64), elem[m].astype(np.int64)
        if len(s) < 2:
            continue
        if k == 0 or (step == 0.0 and not exact):
            assert (np.diff(e) > 0).all(), (where, k, "equal keys order by element")
            continue
        back = np.maximum.accumulate(s)[:-1] - s[1:]
        if exact:
            assert (back <= 0).all(), (where, k, float(back.max()))
            tie = np.diff(s) == 0
            assert (np.diff(e)[tie] > 0).all(), (where, k, "equal starts order by element")
        else:
            assert (back <= step).all(), (where, k, float(back.max()), step)
            worst = max(worst, float(back.max()) / step)
    return worst


def _check_pair(name, form, sc, pi, s, t, st, oracle0):
    V = CC.views_of(sc)
    where = (name, form, s, t)
    R = FORMS[form][2]
    own = CC.model_pair(sc, s, t)
    if name not in CC.DECISION_FREE:
        assert bool(st["enabled"]) == own["enabled"], (where, own["reason"], own["detail"])
    assert st["layout_rows"] == R and (st["Ms"], st["Mt"]) == (len(V[s].segs), len(V[t].segs))
    if not st["enabled"]:
        assert st["src_len"] == 0 and st["n_chunks"] == 0 and not st["src_perm"].size and not st["tgt_perm"].size
        return None
    Ms, Mt = st["Ms"], st["Mt"]
    fm = tuple(st[k] for k in ("As", "Bs", "At", "Bt"))
    if name not in CC.DECISION_FREE:   # (the library forms F from the views it has translated to the scene's centre: another rounding)
        for a, b in zip(fm, own["forms"]):
            assert np.allclose(a, b, rtol=1e-8, atol=1e-8 * np.abs(b).max()), (where, a, b)
    # ---- permutations ----
    sp, tp = st["src_perm"], st["tgt_perm"]
    rows = sp != EMPTY
    assert np.array_equal(np.sort(sp[rows]), np.arange(Ms)), (where, "src_perm")
    assert np.array_equal(np.sort(tp), np.arange(Mt)), (where, "tgt_perm")
    slo = np.zeros(Ms, np.float32); shi = np.zeros(Ms, np.float32)
    slo[sp[rows]], shi[sp[rows]] = st["src_band"][rows, 0], st["src_band"][rows, 1]
    tlo = np.zeros(Mt, np.float32); thi = np.zeros(Mt, np.float32)
    tlo[tp], thi[tp] = st["tgt_band"][:, 0], st["tgt_band"][:, 1]
    # ---- bands: the model on the dumped forms; the target side on the dumped source span ----
    mslo, mshi, mscls = CM.src_bands(fm, V[s].segs)
    _assert_bands(where + ("src",), slo, shi, mslo, mshi, mscls)
    span = CM.src_span(slo, shi)
    mtlo, mthi, mtcls = CM.tgt_bands(fm, V[t].segs, span)
    _assert_bands(where + ("tgt",), tlo, thi, mtlo, mthi, mtcls)
    # ---- soundness on the device's own tables ----
    m = oracle0[pi]
    r, q = m["src_seg"].astype(np.int64), m["tgt_seg"].astype(np.int64)
    inter = CM.intersect(slo, shi, tlo, thi, r, q)
    assert inter.all(), (where, "accepted matches outside the dumped bands", int((~inter).sum()), m[~inter][:3])
    # ---- layout ----
    cls_row = CM.src_classes(slo, shi, Ms, R, V[t].width, V[t].height)
    if R:
        assert st["src_len"] == CM.tile_src_cap(Ms, R) == len(sp)
        want = CM.position_class(np.bincount(cls_row, minlength=CM.TILE_CLASSES), Ms, R)
        got = np.full(len(sp), -1, np.int64)
        got[rows] = cls_row[sp[rows]]
        assert np.array_equal(got, want), (where, "layout", np.nonzero(got != want)[0][:5])
        pad = st["src_band"][~rows]
        assert np.isposinf(pad[:, 0]).all() and np.isneginf(pad[:, 1]).all(), (where, "padding bands")
    else:
        assert st["src_len"] == Ms == len(sp) and rows.all()
    # ---- order inside a class ----
    exact = CM.big_keys(Ms, Mt)
    b = np.isfinite(slo)
    sstep = CM.quant_step(slo[b].min(), slo[b].max(), Ms) if b.any() else 0.0
    worst = _assert_order(where + ("src",), cls_row[sp[rows]], st["src_band"][rows, 0], sp[rows], sstep, exact)
    tstep = CM.quant_step(span[0], span[1], Mt) if span is not None else 0.0
    tstart = st["tgt_band"][:, 0] if (exact or span is None) else np.clip(st["tgt_band"][:, 0], span[0], span[1])
    worst = max(worst, _assert_order(where + ("tgt",), mtcls[tp], tstart, tp, tstep, exact))
    # ---- chunk bands ----
    assert st["n_chunks"] == -(-Mt // 64)
    hull = CM.chunk_hulls(st["tgt_band"][:, 0], st["tgt_band"][:, 1])
    assert np.array_equal(hull.view(np.uint32), st["chunk_band"].view(np.uint32)), (where, "chunk bands")
    return dict(unbounded=(int((mscls == 0).sum()), int((mtcls == 0).sum())), widened=int((mtcls == 1).sum()),
                touch=int(((mscls[r] == 0) | (mtcls[q] == 0)).sum()), order_worst_steps=round(worst, 3))


def _compare_oracle(where, slots, om):
    if len(om) > 80_000:           # (the same comparison without per-match Python work)
        r = H.compare_pair_fast(slots, om)
        assert r["set_diff"] == 0 and r["inexact_fields"] == 0 and r["order_rows"] == 0 and r["n_gpu"] == r["n_cpu"], (where, r)
    else:
        r = H.compare_pair(slots, om)
        assert not r["missing"] and not r["extra"] and r["bit_exact"] and r["order_mismatch"] == 0, \
            (where, len(r["missing"]), len(r["extra"]), r["bit_exact"], r["order_mismatch"])
    return r["n_cpu"]


def _case(name, forms, monkeypatch):
    sc = CC.scene(name)
    pairs = CC.pair_list(sc)
    oracle0 = CC.oracle_pairs(name, 0)
    brute = {}
    out = {}
    for form in forms:
        kNN = FORMS[form][0]
        slots, states, culled = _run(name, form, monkeypatch)
        infos = [_check_pair(name, form, sc, pi, s, t, states[pi], oracle0) for pi, (s, t) in enumerate(pairs)]
        assert culled == sum(int(st["enabled"]) for st in states), (name, form, culled)
        if kNN not in brute:
            brute[kNN] = _run(name, form, monkeypatch, brute=True)[0]
        oracle = CC.oracle_pairs(name, kNN)
        n = 0
        for pi in range(len(pairs)):
            assert np.array_equal(slots[pi], brute[kNN][pi]), (name, form, pi, "culled != brute force")
            n += _compare_oracle((name, form, pi), slots[pi], oracle[pi])
        out[form] = slots
        print(name, form, dict(culled=culled, pairs=len(pairs), matches=n, tables=infos), "bands so far", BAND_STATS)
    return out


PLAIN = [n for n in CC.CASES if n not in ("class_edges", "slow_arithmetic") and not n.startswith("big_keys")]


@pytest.mark.parametrize("name", PLAIN)
def test_tables_and_results(name, monkeypatch):
    _case(name, ("tile", "keep"), monkeypatch)


def test_class_edges_in_every_layout(monkeypatch):
    """Ms / R one below and at 24, 48 and 192 items (R = 16) and 24 and 48 items (R = 64), band widths on both sides of every
    cut, unbounded rows, no class a whole number of items: the padded region against tile_src_cap at its worst case"""
    CC.condition("class_edges")
    _case("class_edges", ("tile", "row", "keep"), monkeypatch)


@pytest.mark.parametrize("name", [n for n in CC.CASES if n.startswith("big_keys")])
def test_key_paths(name, monkeypatch):
    """64-bit keys in global scratch (a view of 16 385 segments, on either side) and 32-bit keys with (4 096) and without
    (4 097) the band cache; as the source view, the large one also takes the unpadded layout's 4 096 and 8 192 steps"""
    _case(name, ("tile", "keep"), monkeypatch)


def test_slow_arithmetic_gives_the_same_slots(monkeypatch):
    """one coordinate of 2e7 in every view: no pair has kPairFastMath, and the slots are those of the scene without the far
    segments (last in their views: the indices agree) -- and the oracle's"""
    CC.condition("slow_arithmetic")
    slow = _case("slow_arithmetic", ("tile", "keep"), monkeypatch)
    base = CC.scene("mixed_cameras")
    for form in ("tile", "keep"):
        fast = _run("mixed_cameras", form, monkeypatch)[0]
        for pi, (s, t) in enumerate(CC.pair_list(base)):
            a, b = slow[form][pi], fast[pi]
            Ms, Mt = len(CC.views_of(base)[s].segs), len(CC.views_of(base)[t].segs)
            assert a.shape == (Ms + 1, b.shape[1]) and np.array_equal(a[:Ms], b), (form, pi)
            assert (a[Ms]["tgt_seg"] == EMPTY).all() and not (a["tgt_seg"] == Mt).any(), "the far segment matches nothing"


def test_whole_pipeline_on_outside_segments():
    """matchImages + computeAffinity on segments far outside their images, against the reference's own code (the bands reach
    phase B through the match lists only: once is enough)"""
    import os
    from line3dpp_amd.api import Line3D
    from oracle import oracle as O
    assert O.have_reference()
    sc = CC.scene("outside_segments")
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages() and g.computeAffinity()
    assert g.timings()["culled_pairs"] == 3
    o = O.Oracle(threads=min(16, len(os.sched_getaffinity(0))), reference=True)
    o.add_scene(sc)
    o.match_images(); o.compute_affinity()
    r = H.full_result_diff(g, o, sc)
    print("outside_segments", r)
    assert r["ok"] and r["set_diff"] == 0 and r["inexact_phase_a_fields"] == 0 and r["order_rows"] == r["tie_rows"], r
    assert r["best_set_diff"] == 0 and r["affinity_set_diff"] == 0 and r["best_choice_diff"] == 0, r
    assert r["surviving"] > 100 and r["best"] > 50 and r["affinity_entries"] > 20, r
