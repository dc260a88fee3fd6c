"""Host model of phase B's hypothesis lists (k_lists.hip) and the scenes of tests/test_gpu_lists.py.

The list of a 2D segment holds its FRESH hypotheses -- the alive slots of its rows in the outgoing pairs of its view -- and
its INVERSE ones: the slots of pairs from earlier views (src < tgt, line3D.cc:1680) that name the segment as target and
passed the target view's orientation filter (kSlotInvAlive, the stream k_pair_csr sorts).  Its length L = n_inv + n_fresh
decides which kernel tier takes it: one wave up to BASE, two waves up to 2 BASE, four up to 4 BASE, k_lists_huge beyond
(ListCfg<WPL, BASE>::CAP = BASE * WPL), with BASE = 256 when the pass' mean list length lies above 96 and 128 otherwise.
"""
import copy

import numpy as np

from line3dpp_amd._lib import EMPTY
from line3dpp_amd.scene import Scene, make_scene

SLOT_ALIVE, SLOT_INV_ALIVE = 1, 2          # l3d_dev.h: kSlotAlive, kSlotInvAlive
WIDE_MEAN_LIST = 96                        # l3d_kernels.h: kWideMeanList
EDGE_LDS = 512                             # k_lists.hip: kEdgeLds
CHAIN_SWEEPS_FRESH = 9                     # sweeps a fresh context enqueues (l3d_phase_b.hip: max(4, 6 + 3))


def list_lengths(pairs, slot_off, view_sizes, slots, alive, kNN, slot_rows=None):
    """n_inv, n_fresh and L for every 2D segment, from what phase A left.
    pairs [P, 2]: (source cam, target cam) of the directed pairs in pair order; slot_off [P]: first slot of each pair;
    view_sizes {cam: segments}; slots [n]: the slot buffer (fields tgt_seg, flags); alive [n] bool: the fresh-hypothesis
    stream (NaN = not alive); kNN > 0: uniform rows of kNN slots; kNN <= 0: ragged rows, slot_rows [n] names each slot's
    source row.  Segments are numbered view by view in ascending cam order (seg_base[cam] + segment)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    cams = sorted(view_sizes)
    seg_base, G = {}, 0
    for c in cams:
        seg_base[c] = G
        G += int(view_sizes[c])
    n = len(slots)
    alive = np.asarray(alive, bool)
    assert alive.shape == (n,)
    off = [int(x) for x in slot_off] + [n]
    n_inv = np.zeros(G, np.int64); n_fresh = np.zeros(G, np.int64)
    for p, (s, t) in enumerate(pairs):
        a, b = off[p], off[p + 1]
        if b <= a:
            continue
        row = (np.arange(b - a) // kNN) if kNN > 0 else np.asarray(slot_rows[a:b], np.int64)
        assert row.max() < view_sizes[int(s)]
        np.add.at(n_fresh, seg_base[int(s)] + row[alive[a:b]], 1)
        if t > s:                                   # inverse matches go to views processed later only
            sl = slots[a:b]
            inv = ((sl["flags"] & SLOT_INV_ALIVE) != 0) & (sl["tgt_seg"] != EMPTY)
            assert not (inv & ~alive[a:b]).any(), "an inverse hypothesis of a slot that is not alive"
            tg = sl["tgt_seg"][inv].astype(np.int64)
            assert not len(tg) or tg.max() < view_sizes[int(t)]
            np.add.at(n_inv, seg_base[int(t)] + tg, 1)
    return dict(n_inv=n_inv, n_fresh=n_fresh, L=n_inv + n_fresh, seg_base=seg_base, cams=cams)


def tier_counts(L, base):
    """lists per tier of a pass with that BASE: what flags[7], flags[4] and flags[5] of k_lists count"""
    L = np.asarray(L)
    return dict(tier1=int((L <= base).sum()), tier2=int(((L > base) & (L <= 2 * base)).sum()),
                tier4=int(((L > 2 * base) & (L <= 4 * base)).sum()), huge=int((L > 4 * base).sum()))


def pass_base(n_slots, G, entries_before=0):
    """BASE of a list pass: from the measured mean list length of the context's previous call, on a first call from the
    estimate 1.5 n_slots / G (l3d_phase_b.hip: lists_run; both are truncated to integers before the comparison)"""
    mean = entries_before // max(G, 1) if entries_before else int(1.5 * n_slots / max(G, 1))
    return 256 if mean > WIDE_MEAN_LIST else 128


def ragged_slot_rows(row_counts):
    """slot_rows of the keep-all layout: pairs in pair order, rows in order, a row's matches back to back;
    row_counts: per pair the number of matches of every source row"""
    out = [np.repeat(np.arange(len(c), dtype=np.int64), np.asarray(c, np.int64)) for c in row_counts]
    return np.concatenate(out) if out else np.zeros(0, np.int64)


LIST_COUNTERS = ("lists_tier2_lists", "lists_tier4_lists", "lists_huge_lists", "lists_wide_passes", "lists_narrow_passes",
                 "lists_tier_repeats", "lists_huge_scratch_regrows", "edges_global_segments", "lists_cand_pool_regrows",
                 "lists_edge_pool_regrows")


def read_counters():
    """the process-wide list-pass counters of l3d_debug_counter (tests take differences)"""
    from line3dpp_amd import _lib
    L = _lib.load()
    out = {k: int(L.l3d_debug_counter(k.encode())) for k in LIST_COUNTERS}
    assert all(v != 2**64 - 1 for v in out.values()), "l3d_debug_counter does not know a list-pass counter"
    return out


def counters_since(before):
    now = read_counters()
    return {k: now[k] - before[k] for k in now}


def model_of_context(g, scene, kNN):
    """list_lengths from what the last matchImages of context `g` left on the device (slot buffer, fresh-hypothesis
    stream, pair list); adds n_slots and G"""
    import torch
    from line3dpp_amd import dist
    from line3dpp_amd._lib import SLOT_DTYPE
    pairs, slot_off = g.pairs()
    hyp = g.fresh_hyp()
    assert hyp is not None
    ptr, n = g.slot_buffer()
    slots = dist.device_tensor(ptr, n * 32, torch.device("cuda", 0)).cpu().numpy().view(SLOT_DTYPE) if n else np.zeros(0, SLOT_DTYPE)
    rows = None
    if kNN <= 0:
        rows = ragged_slot_rows([(g.pair_slots(pi)["tgt_seg"] != EMPTY).sum(1) for pi in range(len(pairs))])
        assert len(rows) == n
    m = list_lengths(pairs, slot_off, {v.cam: len(v.segs) for v in scene.views}, slots, ~np.isnan(hyp[:, 0]), kNN, rows)
    m["n_slots"] = int(n); m["G"] = len(m["L"])
    return m


def drop_segments(sc, drop):
    """a copy of the scene without the segments drop = {cam: [segment indices]}"""
    out = copy_scene(sc)
    for v in out.views:
        if v.cam in drop:
            keep = np.ones(len(v.segs), bool)
            keep[np.asarray(sorted(drop[v.cam]), np.int64)] = False
            v.segs = v.segs[keep].copy()
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------
def hub_scene(n_views, n_segs, n_neighbors, seed, real_fraction=0.5, arc=4):
    """The first n_views views of a ring of arc * n_views (an arc of 1 / arc of the circle: every view sees the facades the
    others see), neighbours restricted to those views, and the view with the highest cam id made a neighbour of every
    other view: that view has n_views - 1 incoming pairs"""
    sc = make_scene(arc * n_views, n_segs, n_neighbors=n_neighbors, seed=seed, real_fraction=real_fraction, max_views=n_views)
    hub = max(v.cam for v in sc.views)
    have = {v.cam for v in sc.views}
    for v in sc.views:
        if v.cam != hub:
            v.neighbors = sorted((set(v.neighbors) & have) | {hub})
        else:
            v.neighbors = sorted(have - {hub})
    sc.name = f"hub{n_views}x{n_segs}"
    return sc


def mixed_scene(sizes, n_neighbors, seed, real_fraction=0.5):
    """one ring whose views are cut to the given segment counts (the longest segments of each view stay)"""
    sc = make_scene(len(sizes), max(sizes), n_neighbors=n_neighbors, seed=seed, real_fraction=real_fraction)
    for v, m in zip(sc.views, sizes):
        v.segs = v.segs[:m].copy()
    sc.name = "mixed" + "_".join(str(m) for m in sizes)
    return sc


def copy_scene(sc):
    out = Scene([copy.copy(v) for v in sc.views], sc.name)
    return out
