"""The keep-all mode (kNN <= 0: MODE 1 of k_match_pairs -> scan -> k_keep_pair_info -> k_keep_assemble, driven by
keep_all_single_pass) at the places where it changes form: rows of one block minus one to plus one and of two blocks and
more, a long row at every kind of start, row offsets on both sides of the staged row table, empty rows and empty pairs at
the boundaries, the pair table's reduction edges, the scratch and the output capacity on both sides of a repeat, and later
calls on one context.

Every case is a named scene of tests/keep_cases.py; tests/test_keep_cases.py asserts on the CPU that it meets its condition.
At tolerance 0: the ragged slot buffer against the CPU oracle's matches of every pair in row order; row_start, the pair
table, row_pair, blk_row and slot_row (l3d_debug_keep_rows) against the numpy model; the flags against the two-pass form,
where k_orient_all decides them; hyp_p and inv_tgt against the flags; the two halves of the keep_all_repeats counter
against the model's host decisions; two runs byte for byte."""
import time

import numpy as np
import pytest

from line3dpp_amd._lib import EMPTY, SLOT_DTYPE
from tests import helpers as H
from tests import keep_cases as KC
from tests import match_cases as MC

pytestmark = pytest.mark.gpu

FIELDS = ("tgt_seg", "overlap", "d_p1", "d_p2", "d_q1", "d_q2")
L3D_ERR_STATE = -7
ENV = ("L3D_KEEPALL_TWO_PASS", "L3D_KEEPALL_NO_CULL", "L3D_KEEPALL_CAP")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _ctx(name):
    from line3dpp_amd.api import Line3D
    g = Line3D()
    g.add_scene(KC.scene(name))
    return g


def _counter():
    from line3dpp_amd import _lib
    v = int(_lib.load().l3d_debug_counter(b"keep_all_repeats"))
    assert v != 2**64 - 1
    return v


def _all_slots(g):
    """the slot buffer of the context as one host array (waits for the context's stream)"""
    import torch
    from line3dpp_amd import dist
    assert g.L.l3d_synchronize(g.h) == 0
    ptr, n = g.slot_buffer()
    if not n:
        return np.zeros(0, SLOT_DTYPE)
    return dist.device_tensor(ptr, n * SLOT_DTYPE.itemsize, torch.device("cuda", 0)).cpu().numpy().view(SLOT_DTYPE)


def _call(g, epi):
    """one keep-all call; returns what it added to the two halves of the keep_all_repeats counter"""
    before = _counter()
    assert g.matchBegin(kNN=0, epipolar_overlap=epi), g.last_status
    assert g.matchPairs(0, len(g.pairs()[0])), g.last_status
    d = _counter() - before
    return d & 0xFFFF, d >> 16


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_call(g, name, epi, plan, delta):
    """everything a single-pass call left behind, against the oracle and the model; returns (slots, rows)"""
    lay = KC.layout(name, epi)
    oracle = KC.oracle_pairs(name, epi)
    assert delta == KC.counter_delta(plan), (name, delta, plan)
    pairs, off = g.pairs()
    assert [tuple(int(x) for x in p) for p in pairs] == MC.pair_list(KC.scene(name))
    slots = _all_slots(g)
    assert len(slots) == lay.total == g.slot_buffer()[1]
    assert np.array_equal(off.astype(np.int64), lay.pair_table[:, 0])
    # the ragged buffer = the oracle's matches of every pair, concatenated in row order
    want = np.concatenate([m for m, _ in oracle])
    assert np.array_equal(np.concatenate([np.repeat(np.arange(len(o) - 1), np.diff(o.astype(np.int64))) for _, o in oracle]), want["src_seg"])
    for f in FIELDS:
        assert np.array_equal(_bits(slots[f]), _bits(want[f])), (name, f, int(np.count_nonzero(_bits(slots[f]) != _bits(want[f]))))
    inner = np.ones(lay.total, bool)
    inner[lay.row_start[:-1][lay.all > 0]] = False                           # (not the first slot of a row)
    assert np.all(np.diff(slots["tgt_seg"].astype(np.int64))[inner[1:]] > 0), "targets ascend inside every row"
    assert not slots["score3D"].any()
    # the layout against the model
    rows = g.keep_rows()
    assert rows is not None, g.last_status
    assert (rows["n_rows"], rows["n_pairs"], rows["n_blocks"], rows["n_slots"]) == (lay.n_rows, len(lay.counts), lay.n_blocks, lay.total)
    assert rows["keep_cap"] == plan["keep_cap"]
    assert np.array_equal(rows["row_start"], lay.row_start) and np.array_equal(rows["row_pair"], lay.row_pair)
    assert np.array_equal(rows["blk_row"], lay.blk_row), np.nonzero(rows["blk_row"] != lay.blk_row)[0][:5]
    info = rows["pair_info"].astype(np.int64)
    assert np.array_equal(np.stack([info[:, 0], info[:, 1], info[:, 2] | (info[:, 3] << 32)], 1), lay.pair_table)
    assert np.array_equal(rows["slot_row"], lay.slot_row), np.nonzero(rows["slot_row"] != lay.slot_row)[0][:5]
    # flags and the streams of phase B
    alive, rejected = H._assert_slot_liveness(g, min_alive=1)
    flags = slots["flags"]
    assert not (flags & ~np.uint32(3)).any() and not ((flags & 2) != 0)[(flags & 1) == 0].any()
    assert np.array_equal(rows["inv_tgt"], np.where((flags & 2) != 0, slots["tgt_seg"], np.uint32(EMPTY)))
    return slots, rows


def _two_pass_ragged(name, epi, monkeypatch):
    """the two-pass form of the same call (count pass, rows padded to the pair's longest, streamed fill, flags by k_orient_all
    in phase B): its slots with a target, in buffer order = the ragged order"""
    monkeypatch.setenv("L3D_KEEPALL_TWO_PASS", "1")
    g = _ctx(name)
    assert _call(g, epi) == (0, 0)
    assert g.keep_rows() is None and g.last_status == L3D_ERR_STATE, "the two-pass form is not ragged"          # (L3D_ERR_STATE)
    assert g.matchFinish(), g.last_status
    padded = _all_slots(g)
    monkeypatch.delenv("L3D_KEEPALL_TWO_PASS")
    lay = KC.layout(name, epi)
    assert len(padded) == sum(len(c) * max(int(c.max(initial=0)), 1) for c in lay.counts)
    return g, padded[padded["tgt_seg"] != EMPTY]


# ---- every case: buffer, layout, flags, counters, two runs -------------------------------------------------------------------
@pytest.mark.parametrize("name", KC.GPU_CASES)
def test_ragged_rows_layout_flags_and_counters(name, monkeypatch):
    t0 = time.perf_counter()
    epi = KC.epi(name)
    plan = KC.host_plan(KC.layout(name))
    g = _ctx(name)
    slots, rows = _assert_call(g, name, epi, plan, _call(g, epi))
    g2 = _ctx(name)
    assert _call(g2, epi) == KC.counter_delta(plan)
    again, rows2 = _all_slots(g2), g2.keep_rows()
    assert again.tobytes() == slots.tobytes(), "two runs of the case differ"
    assert all(np.array_equal(rows[k], rows2[k]) for k in ("row_start", "row_pair", "blk_row", "pair_info", "slot_row", "inv_tgt"))
    _, two = _two_pass_ragged(name, epi, monkeypatch)
    assert len(two) == len(slots)
    for f in FIELDS + ("flags",):
        assert np.array_equal(_bits(two[f]), _bits(slots[f])), (name, f)
    lay = KC.layout(name)
    print(f"{name}: {lay.total} slots in {lay.n_rows} rows of {len(lay.counts)} pairs, longest {lay.longest}, {lay.n_blocks} blocks, "
          f"{int(lay.slot_in_memory.sum())} slots placed in memory, guess {plan['guess']}, counters {KC.counter_delta(plan)}, "
          f"keep_cap {rows['keep_cap']}, {time.perf_counter() - t0:.2f} s")


# ---- the padded form of the accessor -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "dense_row_1025", "empty_pairs"])
def test_padded_accessor_hands_out_the_ragged_rows(name):
    g = _ctx(name)
    _call(g, KC.epi(name))
    slots = _all_slots(g)
    lay = KC.layout(name)
    for pi, c in enumerate(lay.counts):
        if name == "empty_pairs" and pi not in (0, 2, 3):                    # (an empty pair, a pair, an empty pair)
            continue
        sl = g.pair_slots(pi)
        K = max(int(c.max(initial=0)), 1)
        assert sl.shape == (len(c), K)
        valid = np.arange(K)[None, :] < c[:, None]
        first = int(lay.pair_table[pi, 0])
        assert sl[valid].tobytes() == slots[first:first + int(c.sum())].tobytes()
        pad = sl[~valid]
        assert np.all(pad["tgt_seg"] == EMPTY) and not any(_bits(pad[f]).any() for f in SLOT_DTYPE.names if f != "tgt_seg")


# ---- scratch and capacity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap_minus_longest", [0, -1])
def test_scratch_of_exactly_the_longest_row_and_one_less(cap_minus_longest, monkeypatch):
    """L3D_KEEPALL_CAP equal to the longest row must not repeat the pass; one less must, and leaves the model's keep_cap.
    Either way the total lies beyond the capacity: the second assembly runs (both repeats in one call for one less)."""
    lay = KC.layout("dense")
    cap = lay.longest + cap_minus_longest
    monkeypatch.setenv("L3D_KEEPALL_CAP", str(cap))
    plan = KC.host_plan(lay, env_cap=cap)
    assert KC.counter_delta(plan) == (int(cap_minus_longest < 0), 1)
    g = _ctx("dense")
    _assert_call(g, "dense", KC.DENSE_EPI, plan, _call(g, KC.DENSE_EPI))


# ---- later calls on one context ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq", KC.SEQUENCES, ids=lambda s: "-".join("dense" if e == KC.DENSE_EPI else "sparse" for e in s))
def test_later_calls_on_one_context_equal_fresh_contexts(seq):
    """the dense scene at 1e-4 and at 0.9 on ONE context: the scratch, the block marks, keep_cap and the last total of the
    earlier calls are there when a call starts; every call equals a fresh context's, the counters follow the model"""
    g = _ctx("dense")
    fresh = {}
    for k, (e, plan) in enumerate(zip(seq, KC.sequence_plans(seq))):
        slots, rows = _assert_call(g, "dense", e, plan, _call(g, e))
        if e not in fresh:
            f = _ctx("dense")
            _call(f, e)
            fresh[e] = _all_slots(f).copy()
        assert slots.tobytes() == fresh[e].tobytes(), (k, e)
        assert g.matchAbort()
        assert g.keep_rows() is None and g.last_status == L3D_ERR_STATE


# ---- downstream ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse", "sparse_ring3", "empty_pairs", "pair_info"])
def test_final_result_against_the_oracle(name):
    """matchFinish and computeAffinity on the ragged rows against the oracle.  At their strict thresholds the sparse scenes
    and empty_pairs leave no hypothesis that a third view supports: by the oracle they end with empty results, and so must
    the library; pair_info ends with 323 surviving matches and 109 best hypotheses."""
    from oracle.oracle import Oracle
    sc, epi = KC.scene(name), KC.epi(name)
    g = _ctx(name)
    assert _call(g, epi) == KC.counter_delta(KC.host_plan(KC.layout(name)))
    assert g.matchFinish() and g.computeAffinity(), g.last_status
    o = Oracle(threads=1)
    o.add_scene(sc)
    o.match_images(kNN=0, epi_overlap=epi)
    o.compute_affinity()
    r = H.full_result_diff(g, o, sc)
    print(name, r)
    assert r["ok"] and r["order_rows"] == 0 and (r["surviving"], r["best"]) == ((323, 109) if name == "pair_info" else (0, 0)), r


@pytest.mark.parametrize("name", ["dense_row_1025", "pair_info"])
def test_final_result_equals_the_two_pass_form(name, monkeypatch):
    """matches() and affinity() of the single pass and of the two-pass form, byte for byte (the dense scene's two views
    support no hypothesis: both end empty; pair_info keeps 323 matches)"""
    sc, epi = KC.scene(name), KC.epi(name)
    g1 = _ctx(name)
    _call(g1, epi)
    assert g1.matchFinish() and g1.computeAffinity(), g1.last_status
    g0, _ = _two_pass_ragged(name, epi, monkeypatch)
    assert g0.computeAffinity(), g0.last_status
    n = 0
    for v in sc.views:
        m0, o0 = g0.matches(v.cam); m1, o1 = g1.matches(v.cam)
        assert np.array_equal(o0, o1) and m0.tobytes() == m1.tobytes(), v.cam
        n += len(m1)
    e0, l0, w0 = g0.affinity(); e1, l1, w1 = g1.affinity()
    assert e0.tobytes() == e1.tobytes() and l0.tobytes() == l1.tobytes() and np.float32(w0).tobytes() == np.float32(w1).tobytes()
    print(f"{name}: {n} surviving matches, {len(e1)} affinity entries")
    assert n == (323 if name == "pair_info" else 0)
