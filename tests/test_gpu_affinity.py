"""The affinity fill on the MI355X stage by stage (k_aff_sim, k_aff_flag, the two scans, k_aff_touch, k_aff_mark,
k_aff_emit; k_collin, k_aff_coll_count, k_aff_coll_sim and the host pass), through the read-only hook
l3d_debug_affinity_records (Line3D.affinity_records()) and the numpy model of tests/affinity_cases.py.

Every integer stage, the edges and the row table are compared at tolerance 0, each stage against the model fed with the
GPU's OWN similarities, so that an ulp in a similarity cannot cascade.  The similarities are compared with model_sim:
at most one float32 ulp, in at most one value per 100 000 candidates (rounded up to one per scene) -- the last bit of the
device's double exp and acos before the cast to float is the only freedom.  The arms no scene reaches (a reverse that
exists and fails, 0.5 itself, NaN, inf) are reached with similarities written through the exchange pointer of
l3d_affinity_shard_begin.  The arm "a later hypothesis's passing candidate whose target's list holds no reverse" is
reached by the scene c0_eight (13 candidates with the library's own similarities, more with hand-set ones);
tests/test_affinity_cases.py shows on the CPU which branches every scene holds."""
import functools

import numpy as np
import pytest

from tests import affinity_cases as AC
from tests import helpers as H

pytestmark = pytest.mark.gpu
f32 = np.float32
STAGES = ("simv", "cand_a", "cand_b", "flag", "epos", "first_touch", "touch_flag", "touch_rank", "edges", "l2g")


def _ctx(sc):
    from line3dpp_amd.api import Line3D
    g = Line3D()
    g.add_scene(sc)
    return g


def _records(g, sc):
    rec = g.affinity_records()
    assert rec is not None, g.last_status
    return AC.with_scene(rec, sc)


def _check_simv(rec, what):
    """simv against model_sim -> number of values that differ (printed; at most 1 ulp, at most one per 100 000 candidates)"""
    m = AC.model_simv(rec, *AC.model_candidates(rec))
    d = AC.ulp_distance(rec["simv"], m)
    n_diff, cap = int((d > 0).sum()), max(1, -(-len(m) // 100000))
    print(f"{what}: {len(m)} similarities, {n_diff} differ from the model, largest distance {int(d.max()) if len(d) else 0} ulp (cap {cap})")
    assert (d.max() if len(d) else 0) <= 1 and n_diff <= cap, (what, n_diff, int(d.max()))
    return n_diff


def _check_parallel(g, rec, what, simv=None):
    """mode 0: every stage against the model fed with the GPU's own similarities (or `simv`, which the GPU must then
    hold bit for bit), the sequential restatement, and the accessors against the hook's arrays"""
    assert rec["mode"] == 0 and not rec["diffused"]
    if simv is not None:
        assert rec["simv"].tobytes() == simv.tobytes(), (what, "the similarities written")
    w = AC.run_stages(rec, rec["simv"])
    AC.check_stages(rec, w, what)
    assert rec["n_edges"] == 2 * rec["epos_total"] and rec["n_rows"] == rec["touch_total"], what
    se, rows = AC.model_sequential(rec, rec["simv"])
    assert se.tobytes() == rec["edges"].tobytes() and AC.l2g_of_segments(rec, rows).tobytes() == rec["l2g"].tobytes(), (what, "sequential rule")
    e, l2g, msdl = g.affinity()
    assert e.tobytes() == rec["edges"].tobytes() and l2g.tobytes() == rec["l2g"].tobytes(), (what, "affinity()")
    assert (len(e), len(l2g)) == (rec["n_edges"], rec["n_rows"])
    assert msdl == rec["med_scene_depth_lines"] and (not rec["n_cand"] or msdl == rec["msdl_dev"][0])
    return w


def _snapshot(g, sc):
    rec = _records(g, sc)
    e, l2g, msdl = g.affinity()
    out = {k: rec[k].tobytes() for k in STAGES}
    out.update(affinity=e.tobytes() + l2g.tobytes() + np.float32(msdl).tobytes(), totals=(rec["epos_total"], rec["touch_total"]),
               sizes=(rec["N"], rec["H"], rec["n_edges"], rec["n_rows"]))
    return out


@functools.lru_cache(maxsize=None)
def _run(name):
    """CASES[name] on a fresh context: matchImages, computeAffinity, the hook's records.  Shared; nobody writes to it."""
    case = AC.CASES[name]
    sc = case.scene()
    g = _ctx(sc)
    assert g.matchImages(**case.params) and g.computeAffinity(), g.last_status
    return g, sc, _records(g, sc)


# ---- a. stage by stage on every scene ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AC.CASES))
def test_stages_on_every_scene(name):
    g, sc, rec = _run(name)
    exp = AC.CASES[name].expect
    assert (rec["N"], rec["H"]) == (exp["N"], exp["H"]), "the scene drifted: N and H are what the launch edges rest on"
    print(f"{name}: N = {rec['N']} (N % 128 = {rec['N'] % 128}, N % 256 = {rec['N'] % 256}), H = {rec['H']}")
    _check_parallel(g, rec, name)
    _check_simv(rec, name)
    # the weights against the oracle's expf: no further than the model's own distance on the oracle's records
    r = AC.oracle_run(name)
    assert r["same_ids"]
    assert np.array_equal(rec["edges"]["i"], r["edges"]["i"]) and np.array_equal(rec["edges"]["j"], r["edges"]["j"]), "ids and order"
    assert np.array_equal(np.stack([rec["l2g"]["cam"], rec["l2g"]["seg"]], 1), r["l2g"].reshape(-1, 2))
    d = AC.ulp_distance(rec["edges"]["w"], r["edges"]["w"])[0::2]
    n_diff, worst = int((d > 0).sum()), int(d.max()) if len(d) else 0
    print(f"{name}: {len(d)} weights, {n_diff} differ from the oracle's (model: {r['n_diff']}), largest {worst} ulp (model: {r['max_ulp']})")
    assert n_diff <= r["n_diff"] and worst <= r["max_ulp"]


# ---- b. hand-set similarities through the exchange pointer ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sharded(name, world):
    sc = AC.CASES[name].scene()
    ctxs, counts = H.sharded_tail(sc, world, **AC.CASES[name].params)
    return sc, ctxs, counts


def _begin(ctxs):
    import torch
    from line3dpp_amd import dist
    world = len(ctxs)
    parts = [g.affinityShardBegin(r, world) for r, g in enumerate(ctxs)]
    assert all(p is not None and p[1] == 4 and p[2] == parts[0][2] for p in parts), "every rank derives the same parts"
    n_all = sum(n for _, n in parts[0][2])
    dev = torch.device("cuda", 0)
    return parts[0][2], [dist.device_tensor(p[0], 4 * n_all, dev) for p in parts]


def _upload(sims, pattern, cand_a, cand_b):
    """writes the whole similarity array of every context.  A value above 0.5 on a candidate with a segment without a
    hypothesis would make k_aff_touch index first_touch[-1]: the library never produces one, and neither does this."""
    import torch
    assert pattern.dtype == f32 and len(pattern) == len(cand_a)
    with np.errstate(invalid="ignore"):
        hot = pattern > AC.MIN_AFFINITY
    assert not (hot & ~AC.eligible(cand_a, cand_b)).any(), "a passing value on a candidate that is not eligible"
    src = torch.from_numpy(pattern.view(np.uint8).copy())
    for s in sims:
        assert s.numel() == src.numel()
        s.copy_(src)
    torch.cuda.synchronize()


def _patterns(rec):
    ca, cb = AC.model_candidates(rec)
    n, el = len(ca), AC.eligible(ca, cb)
    ei = np.nonzero(el)[0]
    rev = AC.reverse_index(rec)
    mutual = el & (rev >= 0)
    out = {}
    p = np.zeros(n, f32); p[el] = 1.0; out["all_one"] = p
    out["all_half"] = np.full(n, 0.5, f32)
    p = np.zeros(n, f32); p[el] = np.nextafter(f32(0.5), f32(1)); out["just_above_half"] = p
    p = np.zeros(n, f32); p[mutual & (ca < cb)] = 0.25; p[mutual & (ca > cb)] = 0.75; out["later_direction_passes"] = p
    p = np.zeros(n, f32); p[mutual & (ca < cb)] = 0.75; p[mutual & (ca > cb)] = 0.25; out["earlier_direction_passes"] = p
    p = np.zeros(n, f32); p[ei] = np.inf; p[ei[::3]] = np.nan; out["nan_and_inf"] = p
    for nm, c in (("one_first", ei[0]), ("one_last", ei[-1]), ("one_near_4096", ei[np.argmin(np.abs(ei - 4096))])):
        p = np.zeros(n, f32); p[c] = 0.75; out[nm] = p
    for seed in (1, 2):
        p = np.zeros(n, f32); p[el] = np.where(np.random.default_rng(seed).random(int(el.sum())) < 0.5, 0.75, 0.25); out[f"bernoulli_{seed}"] = p
    return out


PATTERNS = ("all_one", "all_half", "just_above_half", "later_direction_passes", "earlier_direction_passes", "nan_and_inf",
            "one_first", "one_last", "one_near_4096", "bernoulli_1", "bernoulli_2")


def _close(ctxs):
    """a test that fails between begin and finish must not leave the shared contexts with an open fill"""
    for g in ctxs:
        g.affinityShardAbort()


# every pattern on c0_six; on c0_eight, whose lists hold later-hypothesis candidates without a reverse, the two that
# let many of them pass
HAND_SET = [("c0_six", p) for p in PATTERNS] + [("c0_eight", "all_one"), ("c0_eight", "bernoulli_1")]


@pytest.mark.parametrize("name,pattern", HAND_SET)
def test_hand_set_similarities(name, pattern):
    """two contexts behind a sharded tail; between begin and finish the test writes the whole similarity array of both"""
    sc, ctxs, _ = _sharded(name, 2)
    _, _, single = _run(name)
    try:
        parts, sims = _begin(ctxs)
        pat = _patterns(single)[pattern]
        _upload(sims, pat, single["cand_a"], single["cand_b"])
        assert all(g.affinityShardFinish() for g in ctxs)
    finally:
        _close(ctxs)
    for g in ctxs:
        rec = _records(g, sc)
        assert rec["cand_a"].tobytes() == single["cand_a"].tobytes() and rec["cand_b"].tobytes() == single["cand_b"].tobytes()
        _check_parallel(g, rec, pattern, simv=pat)
    c = AC.class_counts(rec, pat)
    print(pattern, {k: c[k] for k in ("pass", "back_rev_pass", "back_rev_fail", "back_rev_absent", "fwd_rev_present", "fwd_rev_absent",
                                      "edges", "rows", "rows_as_id1", "rows_as_id2")})
    if name == "c0_eight":
        assert c["back_rev_absent"] > 13, "the loop over the target's list ends without a hit, f stays 1"
    if pattern == "all_half":
        assert rec["n_edges"] == 0 and rec["n_rows"] == 0 and len(ctxs[0].affinity()[0]) == 0
    if pattern == "just_above_half":
        assert c["pass"] == int(AC.eligible(single["cand_a"], single["cand_b"]).sum()) and c["edges"] > 0
    if pattern == "later_direction_passes":
        assert c["back_rev_fail"] > 0 and c["back_rev_fail"] == c["edges"], "the arm no scene reaches: the reverse exists and fails"
    if pattern == "earlier_direction_passes":
        assert c["back_rev_fail"] == 0 and c["fwd_rev_present"] == c["edges"] > 0
    if pattern == "nan_and_inf":
        assert np.isinf(rec["edges"]["w"]).all() and c["edges"] > 0 and c["back_rev_fail"] > 0
    if pattern.startswith("one_"):
        assert (rec["n_edges"], rec["n_rows"]) == (2, 2)
    if pattern.startswith("bernoulli"):
        assert c["back_rev_fail"] > 0 and c["back_rev_pass"] > 0 and c["fwd_rev_absent"] > 0


# ---- c. shard windows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_shard_windows(world):
    sc, ctxs, counts = _sharded("c0_six", world)
    _, _, single = _run("c0_six")
    try:
        _shard_windows(world, sc, ctxs, counts, single)
    finally:
        _close(ctxs)


def _shard_windows(world, sc, ctxs, counts, single):
    import torch
    parts, sims = _begin(ctxs)
    assert [n for _, n in parts] == [n for n, _ in counts] and sum(n for _, n in parts) == single["N"]
    for r, g in enumerate(ctxs):
        rec = g.affinity_records()
        lo, hi = parts[r][0], parts[r][0] + parts[r][1]
        print(f"world {world} rank {r}: window [{lo}, {hi}), lo % 128 = {lo % 128}, hi % 128 = {hi % 128}")
        assert rec["mode"] == 2 and (rec["n_edges"], rec["n_rows"]) == (0, 0) and "flag" not in rec
        assert rec["simv"][lo:hi].tobytes() == single["simv"][lo:hi].tobytes(), "this rank's window, bit for bit"
        assert rec["cand_a"].tobytes() == single["cand_a"].tobytes() and rec["cand_b"].tobytes() == single["cand_b"].tobytes()
    for r, (f, n) in enumerate(parts):
        for q in range(world):
            if q != r and n:
                sims[q][4 * f:4 * (f + n)].copy_(sims[r][4 * f:4 * (f + n)])
    torch.cuda.synchronize()
    assert all(g.affinityShardFinish() for g in ctxs)
    want = _snapshot(*_run("c0_six")[:2])
    for g in ctxs:
        assert _snapshot(g, sc) == want


# ---- d. leftover state ------------------------------------------------------------------------------------------------------
def test_repeated_calls_leave_nothing_behind():
    sc = AC.CASES["c0_six"].scene()
    fresh = {}
    for k in (10, 1):
        f = _ctx(sc)
        assert f.matchImages(kNN=k) and f.computeAffinity()
        fresh[k] = _snapshot(f, sc)
    assert fresh[1]["sizes"][0] < fresh[10]["sizes"][0], "N shrinks while the buffers keep their size"
    assert fresh[10] == _snapshot(*_run("c0_six")[:2])
    g = _ctx(sc)
    for k in (10, 1, 10):
        assert g.matchImages(kNN=k) and g.computeAffinity()
        assert _snapshot(g, sc) == fresh[k], k
    assert g.computeAffinity() and g.computeAffinity()
    assert _snapshot(g, sc) == fresh[10]
    _check_parallel(g, _records(g, sc), "repeated")


# ---- e. degenerate sizes ----------------------------------------------------------------------------------------------------
def test_no_candidates_at_all():
    """two views and no third to support a hypothesis: N == 0 and H == 0; the step succeeds and reports zeros"""
    sc = AC._ring(2, 64, n_neighbors=2, seed=5)
    g = _ctx(sc)
    assert g.matchImages() and g.computeAffinity()
    rec = _records(g, sc)
    assert (rec["N"], rec["H"], rec["n_cand"], rec["mode"], rec["n_edges"], rec["n_rows"], rec["epos_total"], rec["touch_total"]) == \
        (0, 0, 0, 0, 0, 0, 0, 0)
    assert all(len(rec[k]) == 0 for k in STAGES) and len(rec["surv_off"]) == rec["G"] + 1 and not rec["surv_off"].any()
    e, l2g, _ = g.affinity()
    assert len(e) == 0 and len(l2g) == 0


# ---- f. the collinear path --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c0_six", "unequal_views"])
def test_collinear_path(name):
    case = AC.CASES[name]
    sc = case.scene()
    g = _ctx(sc)
    assert g.matchImages(**case.params) and g.reconstruct3Dlines(3, False, 2.0), g.last_status
    rec = _records(g, sc)
    assert rec["mode"] == 1 and not rec["diffused"] and "flag" not in rec
    _check_simv(rec, name)
    m = AC.model_collinear(rec, sc, 2.0, simv=rec["simv"])
    for k in ("coll_off", "coll_idx", "child_off", "child_seg", "own_off", "own_seg"):
        assert rec[k].tobytes() == m[k].tobytes(), k
    assert (rec["n_coll"], rec["n_child"], rec["n_own"]) == (len(m["coll_idx"]), len(m["child_seg"]), len(m["own_seg"]))
    n_diff = 0
    for k in ("child_sim", "own_sim"):
        d = AC.ulp_distance(rec[k], m[k])
        assert d.max() <= 1, k
        n_diff += int((d > 0).sum())
    print(f"{name}: {rec['n_coll']} collinear entries, {rec['n_child']} child and {rec['n_own']} own candidates, {n_diff} of their similarities differ from the model")
    assert n_diff <= 1
    # the host pass, fed with the GPU's own three streams
    se, rows = AC.model_sequential(rec, rec["simv"], tuple(rec[k] for k in ("child_off", "child_seg", "child_sim", "own_off", "own_seg", "own_sim")))
    assert se.tobytes() == rec["edges"].tobytes() and AC.l2g_of_segments(rec, rows).tobytes() == rec["l2g"].tobytes()
    e, l2g, _ = g.affinity()
    assert e.tobytes() == rec["edges"].tobytes() and l2g.tobytes() == rec["l2g"].tobytes()
    o, _ = case.oracle(collinearity=2.0)
    oe, ol = o.affinity()
    assert np.array_equal(e["i"], oe["i"]) and np.array_equal(e["j"], oe["j"]) and np.array_equal(np.stack([l2g["cam"], l2g["seg"]], 1), ol)
    assert len(oe) > len(AC.oracle_run(name)["edges"])


def test_sharded_fill_refuses_collinear_links():
    sc, ctxs, _ = _sharded("unequal_views", 2)
    g = ctxs[0]
    assert g.reconstruct3Dlines(3, False, 2.0) and g.affinity_records()["mode"] == 1
    assert g.affinityShardBegin(0, 2) is None and g.last_status == -9          # L3D_ERR_LIMIT
    assert g.affinity_records()["mode"] == 1, "a refused begin leaves the records of the last fill"


# ---- g. the hook's own contract ---------------------------------------------------------------------------------------------
def test_hook_contract():
    sc = AC.CASES["tiny"].scene()
    g = _ctx(sc)
    assert g.affinity_records() is None and g.last_status == -7                # L3D_ERR_STATE: no matches
    assert g.matchImages()
    assert g.affinity_records() is None and g.last_status == -7                # matches, no affinity step on them
    assert g.computeAffinity()
    rec = _records(g, sc)
    assert rec["mode"] == 0 and rec["edges"] is not None
    assert g.matchImages()
    assert g.affinity_records() is None and g.last_status == -7                # new matches: the old buffers are stale
    assert g.reconstruct3Dlines(3, True)
    rec2 = _records(g, sc)
    assert rec2["mode"] == 0 and rec2["diffused"] == 1 and rec2["edges"] is None, "the diffused matrix is not the fill's output"
    for k in STAGES[:-2] + ("l2g",):
        assert rec2[k].tobytes() == rec[k].tobytes(), k
    assert g.computeAffinity()
    rec3 = _records(g, sc)
    assert not rec3["diffused"] and rec3["edges"].tobytes() == rec["edges"].tobytes()
