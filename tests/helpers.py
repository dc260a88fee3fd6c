"""Comparison helpers shared by the parity tests: HIP path (line3dpp_amd.Line3D) vs CPU oracle."""
import numpy as np

from line3dpp_amd._lib import EMPTY

REL_TOL = 1e-4   # north_star: results within 1e-4 relative of the reference CPU path


def rel_close(a, b, tol=REL_TOL):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b) <= tol * np.maximum(np.abs(a), np.abs(b)) + 1e-30


def slots_to_dict(slots):
    """(src_seg, tgt_seg) -> (overlap, dp1, dp2, dq1, dq2) for the valid slots of one pair; also row order"""
    out = {}
    rows = {}
    Ms, K = slots.shape
    for r in range(Ms):
        row = slots[r]
        valid = row["tgt_seg"] != EMPTY
        # valid slots must be a prefix
        nv = int(valid.sum())
        assert valid[:nv].all(), f"row {r}: valid slots are not a prefix"
        rows[r] = [int(x) for x in row["tgt_seg"][:nv]]
        for s in row[:nv]:
            out[(r, int(s["tgt_seg"]))] = (s["overlap"], s["d_p1"], s["d_p2"], s["d_q1"], s["d_q2"])
    return out, rows


def oracle_pair_to_dict(matches):
    out = {}
    rows = {}
    for m in matches:
        out[(int(m["src_seg"]), int(m["tgt_seg"]))] = (m["overlap"], m["d_p1"], m["d_p2"], m["d_q1"], m["d_q2"])
        rows.setdefault(int(m["src_seg"]), []).append(int(m["tgt_seg"]))
    return out, rows


def compare_pair(slots, omatches):
    """returns dict(n_gpu, n_cpu, missing, extra, max_rel, bit_exact, order_mismatch)"""
    g, grows = slots_to_dict(slots)
    o, orows = oracle_pair_to_dict(omatches)
    missing = [k for k in o if k not in g]
    extra = [k for k in g if k not in o]
    max_rel = 0.0
    bit_exact = True
    for k in o:
        if k in g:
            a = np.array(g[k], np.float64); b = np.array(o[k], np.float64)
            if not np.array_equal(np.array(g[k], np.float32), np.array(o[k], np.float32)):
                bit_exact = False
            max_rel = max(max_rel, float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30))))
    order_mismatch = sum(1 for r in orows if r in grows and grows[r] != orows[r])
    return dict(n_gpu=len(g), n_cpu=len(o), missing=missing, extra=extra, max_rel=max_rel, bit_exact=bit_exact,
                order_mismatch=order_mismatch)


def matches_to_dict(m):
    return {(int(x["src_seg"]), int(x["tgt_cam"]), int(x["tgt_seg"])): x for x in m}


def compare_matches(gm, om):
    g = matches_to_dict(gm); o = matches_to_dict(om)
    missing = [k for k in o if k not in g]
    extra = [k for k in g if k not in o]
    max_rel = 0.0
    for k in o:
        if k in g:
            for f in ("overlap", "score3D", "d_p1", "d_p2", "d_q1", "d_q2"):
                a, b = float(g[k][f]), float(o[k][f])
                max_rel = max(max_rel, abs(a - b) / max(abs(b), 1e-30))
    return dict(n_gpu=len(g), n_cpu=len(o), missing=missing, extra=extra, max_rel=max_rel)


def affinity_map(edges, l2g, key=lambda r: (int(r[0]), int(r[1]))):
    """{unordered (Segment2D, Segment2D) -> w}; also checks the (i,j),(j,i) pairing of A_"""
    out = {}
    assert len(edges) % 2 == 0
    for k in range(0, len(edges), 2):
        e1, e2 = edges[k], edges[k + 1]
        assert e1["i"] == e2["j"] and e1["j"] == e2["i"] and e1["w"] == e2["w"]
        a = key(l2g[e1["i"]]); b = key(l2g[e1["j"]])
        kk = (a, b) if a < b else (b, a)
        assert kk not in out, "duplicate unordered pair in A_"
        out[kk] = float(e1["w"])
    return out


def split_scene(sc, frac=0.5):
    """Breaks the first `frac` of every view's segments into two collinear halves with a gap (same segment count):
    the fragmented lines View::findCollinearSegments is meant for."""
    for v in sc.views:
        s = v.segs.astype(np.float64); n = int(len(s) * frac)
        a = s[:n, :2]; b = s[:n, 2:]
        h1 = np.concatenate([a, a + 0.45 * (b - a)], 1); h2 = np.concatenate([a + 0.55 * (b - a), b], 1)
        v.segs = np.concatenate([h1, h2, s[n:len(s) - n]], 0).astype(np.float32)
    return sc


# ---- vectorised whole-scene comparison (BASELINE-size scenes: millions of matches, no Python loops per match) ----
def _match_keys(m):
    return (m["src_seg"].astype(np.uint64) << np.uint64(40)) | (m["tgt_cam"].astype(np.uint64) << np.uint64(20)) | \
        m["tgt_seg"].astype(np.uint64)


def _max_rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-30)))


def _aff_table(edges, l2g_keys):
    """sorted [(lo key, hi key)] array + weights of the unordered pairs of A_ (edges come as (i,j),(j,i) pairs)"""
    e = edges[0::2]
    a = l2g_keys[e["i"]]; b = l2g_keys[e["j"]]
    lo = np.minimum(a, b); hi = np.maximum(a, b)
    order = np.lexsort((hi, lo))
    return lo[order], hi[order], e["w"][order]


def full_result_diff(g, o, scene):
    """HIP context `g` (line3dpp_amd.Line3D after matchImages + computeAffinity) against oracle `o` (oracle.Oracle
    after match_images + compute_affinity), every view of `scene`, vectorised.  Surviving match lists are compared as
    sets AND in order (a list is a per-segment private container in the reference, so its order is deterministic even
    with OpenMP); best hypotheses and A_ are compared as maps (their global order is scheduling-dependent when the
    oracle runs multi-threaded).  Returns a dict of counts / maxima; `ok` summarises the north_star bar (identical
    sets, values within REL_TOL)."""
    r = dict(surviving=0, set_diff=0, order_rows=0, tie_rows=0, inexact_phase_a_fields=0, max_rel_score3D=0.0,
             views=len(scene.views))
    for v in scene.views:
        gm, goff = g.matches(v.cam); om, ooff = o.matches(v.cam)
        gk, ok_ = _match_keys(gm), _match_keys(om)
        r["surviving"] += len(om)
        same_order = len(gk) == len(ok_) and np.array_equal(gk, ok_)
        if not same_order:
            gs, os_ = np.sort(gk), np.sort(ok_)
            if len(gs) != len(os_) or not np.array_equal(gs, os_):
                r["set_diff"] += len(np.setxor1d(gk, ok_))
                common = np.intersect1d(gk, ok_)
                gm = gm[np.isin(gk, common)]; om = om[np.isin(ok_, common)]
                gk, ok_ = _match_keys(gm), _match_keys(om)
            else:
                # same set, different order inside some lists: which segments, and is every one of them an exact
                # overlap tie (the only order freedom: libstdc++ priority_queue pop order of equal keys)?
                segs = np.unique(gm["src_seg"][gk != ok_])
                r["order_rows"] += len(segs)
                for s in segs:
                    a = gm[goff[s]:goff[s + 1]]; b = om[ooff[s]:ooff[s + 1]]
                    d = np.nonzero(_match_keys(a) != _match_keys(b))[0]
                    if np.array_equal(a["overlap"][d], b["overlap"][d]):
                        r["tie_rows"] += 1
            gm = gm[np.argsort(gk, kind="stable")]; om = om[np.argsort(ok_, kind="stable")]
        for f in ("overlap", "d_p1", "d_p2", "d_q1", "d_q2"):
            r["inexact_phase_a_fields"] += int(np.count_nonzero(gm[f] != om[f]))
        r["max_rel_score3D"] = max(r["max_rel_score3D"], _max_rel(gm["score3D"], om["score3D"]))
        gi, oi = g.view_info(v.cam), o.view_info(v.cam)
        r["k_mismatch"] = r.get("k_mismatch", 0) + int(gi["k"] != oi["k"])
        r["max_rel_median_depth"] = max(r.get("max_rel_median_depth", 0.0), _max_rel(gi["median_depth"], oi["median_depth"]))
    # best hypotheses (estimated_position3D_) as a map (cam, seg) -> (P1, P2, dir, best match)
    s2, s3, bm = g.best(); cs, geo, _, obm = o.best()
    gkey = (s2["cam"].astype(np.uint64) << np.uint64(32)) | s2["seg"].astype(np.uint64)
    okey = (cs[:, 0].astype(np.uint64) << np.uint64(32)) | cs[:, 1].astype(np.uint64)
    r["best"] = len(okey)
    r["best_set_diff"] = len(np.setxor1d(gkey, okey))
    if r["best_set_diff"] == 0:
        gi_, oi_ = np.argsort(gkey), np.argsort(okey)
        gg = np.concatenate([s3["P1"], s3["P2"], s3["dir"]], 1)[gi_]
        og = geo[oi_]
        # per 3-vector: |difference| relative to the vector's length (a coordinate near zero has no relative scale)
        err = 0.0
        for c in (0, 3, 6):
            den = np.maximum(np.linalg.norm(og[:, c:c + 3], axis=1), 1e-30)
            err = max(err, float(np.max(np.linalg.norm(gg[:, c:c + 3] - og[:, c:c + 3], axis=1) / den))) if len(og) else err
        r["max_rel_endpoints"] = err
        r["best_choice_diff"] = int(np.count_nonzero((bm["tgt_cam"][gi_] != obm["tgt_cam"][oi_]) |
                                                     (bm["tgt_seg"][gi_] != obm["tgt_seg"][oi_])))
    # A_ as a map {unordered (Segment2D, Segment2D) -> w}
    ge, gl, gms = g.affinity(); oe, ol = o.affinity()
    glk = (gl["cam"].astype(np.uint64) << np.uint64(32)) | gl["seg"].astype(np.uint64)
    olk = (ol[:, 0].astype(np.uint64) << np.uint64(32)) | ol[:, 1].astype(np.uint64)
    ga, gb, gw = _aff_table(ge, glk); oa, ob, ow = _aff_table(oe, olk)
    r["affinity_entries"] = len(oe)
    same = len(ga) == len(oa) and np.array_equal(ga, oa) and np.array_equal(gb, ob)
    r["affinity_set_diff"] = 0 if same else int(len(set(zip(ga.tolist(), gb.tolist())) ^ set(zip(oa.tolist(), ob.tolist()))))
    r["max_rel_affinity"] = _max_rel(gw, ow) if same else None
    r["max_rel_med_scene_depth"] = _max_rel(gms, o.med_scene_depth_lines())
    r["ok"] = bool(r["set_diff"] == 0 and r["best_set_diff"] == 0 and r["affinity_set_diff"] == 0 and
                   r["inexact_phase_a_fields"] == 0 and r.get("best_choice_diff", 1) == 0 and r["k_mismatch"] == 0 and
                   r["order_rows"] == r["tie_rows"] and
                   max(r["max_rel_score3D"], r.get("max_rel_endpoints", 1.0), r["max_rel_affinity"] or 0.0,
                       r["max_rel_median_depth"], r["max_rel_med_scene_depth"]) <= REL_TOL)
    return r


def ring_slice(scene, first, count):
    """`count` consecutive views of a ring scene starting at view `first`, neighbours restricted to the slice: the
    views in the middle of the slice keep their full neighbour set, i.e. the configured neighbour count x size."""
    import copy
    keep = {scene.views[(first + i) % scene.n_views].cam for i in range(count)}
    out = copy.copy(scene)
    out.views = []
    for i in range(count):
        w = copy.copy(scene.views[(first + i) % scene.n_views])
        w.neighbors = [n for n in w.neighbors if n in keep] or \
            [scene.views[(first + (i + 1) % count) % scene.n_views].cam]   # never empty (line3D.cc:154 rejects the view)
        out.views.append(w)
    out.views.sort(key=lambda v: v.cam)
    out.name = f"{scene.name}[{first}:{first + count}]"
    return out


def compare_pair_fast(slots, omatches):
    """compare_pair without per-match Python work: phase-A slots [Ms, K] of one directed pair against the oracle's
    matches of that pair.  Returns dict(n_gpu, n_cpu, set_diff, inexact_fields, order_rows, tie_rows)."""
    Ms, K = slots.shape
    valid = slots["tgt_seg"] != EMPTY
    nv = valid.sum(1)
    assert np.array_equal(valid, np.arange(K)[None, :] < nv[:, None]), "valid slots are not a prefix of their row"
    rows = np.repeat(np.arange(Ms, dtype=np.uint64), K).reshape(Ms, K)[valid]
    gs = slots[valid]
    gk = (rows << np.uint64(32)) | gs["tgt_seg"].astype(np.uint64)
    ok_ = (omatches["src_seg"].astype(np.uint64) << np.uint64(32)) | omatches["tgt_seg"].astype(np.uint64)
    r = dict(n_gpu=len(gk), n_cpu=len(ok_), set_diff=0, inexact_fields=0, order_rows=0, tie_rows=0)
    if len(gk) == len(ok_) and np.array_equal(gk, ok_):
        go, oo = gs, omatches
    else:
        gi, oi = np.argsort(gk, kind="stable"), np.argsort(ok_, kind="stable")
        if len(gk) != len(ok_) or not np.array_equal(gk[gi], ok_[oi]):
            r["set_diff"] = len(np.setxor1d(gk, ok_))
            return r
        # same set: rows whose order differs, and whether each of them is an exact-overlap tie
        bad = np.unique(rows[gk != ok_])
        r["order_rows"] = len(bad)
        for s in bad:
            a = gs[rows == s]; b = omatches[omatches["src_seg"] == s]
            d = np.nonzero(a["tgt_seg"] != b["tgt_seg"])[0]
            r["tie_rows"] += int(np.array_equal(a["overlap"][d], b["overlap"][d]))
        go, oo = gs[gi], omatches[oi]
    for f in ("overlap", "d_p1", "d_p2", "d_q1", "d_q2"):
        r["inexact_fields"] += int(np.count_nonzero(go[f] != oo[f]))
    return r


def gap_scene(world, n_segs, seed=0):
    """A multi-rank topology whose dependency sets have a HOLE: a 12-view ring on the cams of the first and the last rank
    (cams 0-5 and 6 (world - 1) .. 6 world - 1) and a self-contained 6-view ring on the cams of every rank in between.  The
    last rank depends on rank 0 alone; the ranks between depend on nobody.  The segment counts (n_segs on the last rank's
    views, 0.72 n_segs on rank 0's, 0.87 n_segs on the middle rings) give every rank the same matching cost, so that
    l3d_plan_shards cuts at the rings (rank 0's views hand out 15 pairs, the last rank's 9, a 6-view ring's 12)."""
    from line3dpp_amd.scene import Scene, make_scene
    hi = 6 * (world - 1)
    a, m = int(0.72 * n_segs), int(0.87 * n_segs)
    ren = {i: (i if i < 6 else hi + i - 6) for i in range(12)}
    views = []
    for v in make_scene(12, n_segs, n_neighbors=4, seed=seed).views:
        if v.cam < 6:
            v.segs = v.segs[:a].copy()
        v.cam = ren[v.cam]
        v.neighbors = [ren[int(x)] for x in v.neighbors]
        views.append(v)
    for r in range(1, world - 1):
        for v in make_scene(6, m, n_neighbors=4, seed=seed + r).views:
            v.cam += 6 * r
            v.neighbors = [int(x) + 6 * r for x in v.neighbors]
            views.append(v)
    views.sort(key=lambda v: v.cam)
    return Scene(views, f"gap{world}")


def sharded_list_pass(sc, world, **match_kw):
    """Phase B's list pass sharded by views (l3d_lists_shard, line3dpp_amd/dist.py) without a process group: `world`
    contexts on one GPU; every context holds all slots (as after the slot exchange), runs the list pass for ITS views into
    ITS pools, the pool slabs are copied where the all-gather would put them, and every context finishes on the complete
    records (repeating the step while the ranks report enlarged pools).  Returns the contexts after l3d_match_finish."""
    import torch
    from line3dpp_amd import dist
    from line3dpp_amd.api import Line3D
    dev = torch.device("cuda", 0)
    ctxs = []
    for _ in range(world):
        g = Line3D()
        g.add_scene(sc)
        assert g.matchBegin(**match_kw) and g.matchPairs(0, len(g.pairs()[0]))
        ctxs.append(g)
    for attempt in range(8):
        slabs = []
        for r, g in enumerate(ctxs):
            sl = g.listsShard(r, world)
            assert sl is not None and len(sl) == 4
            slabs.append(sl)
        for k in range(4):
            sizes = {sl[k][1] for sl in slabs}
            assert len(sizes) == 1, "equal slab sizes on every rank"
            sb = sizes.pop()
            fulls = [dist.device_tensor(sl[k][2], sb * world, dev) for sl in slabs]
            for r in range(world):
                assert slabs[r][k][0] == slabs[r][k][2] + r * sb
                for q in range(world):
                    if q != r:
                        fulls[q][r * sb:(r + 1) * sb].copy_(fulls[r][r * sb:(r + 1) * sb])
        torch.cuda.synchronize()
        rcs = [g.L.l3d_match_finish(g.h) for g in ctxs]
        assert len(set(rcs)) == 1, "every rank takes the same decision (all of them see all pool counters)"
        if rcs[0] == 0:
            return ctxs
        assert rcs[0] == -10, rcs               # L3D_ERR_RETRY: pools enlarged on every rank alike, repeat the step
    raise AssertionError("the pools never became large enough")


def sharded_tail(sc, world, **match_kw):
    """matchImages sharded over `world` contexts on one GPU up to l3d_tail_shard_commit, without a process group (the
    sequence of tests/test_gpu_parity.py's sharded-tail emulation): pairs matched by the planned halo shards, slot indices
    copied where the exchange would put them, the list pass and the tail per rank's views, the tail's parts copied, commit.
    Returns (contexts, [(surviving matches, best hypotheses) per rank]); l3d_affinity_shard_begin may follow."""
    import torch
    from line3dpp_amd import dist
    from line3dpp_amd.api import Line3D
    dev = torch.device("cuda", 0)
    ctxs = []
    for _ in range(world):
        g = Line3D()
        g.add_scene(sc)
        assert g.matchBegin(**match_kw)
        ctxs.append(g)
    pairs, slot_off = ctxs[0].pairs()
    plan = dist.plan_halo(pairs, ctxs[0]._M, world)
    vb, pb, runs, needs = plan["view_bounds"], plan["pair_bounds"], plan["runs"], plan["needs"]
    bufs = []
    for r, g in enumerate(ctxs):
        assert g.shardOptions(min(needs[r] + [r]), False)
        assert g.matchPairs(int(pb[r]), int(pb[r + 1] - pb[r]))
        for _, f, n in runs[r]:
            assert g.packSlotIndices(f, n)
        ptr, n_slots = g.slot_index_buffer()
        bufs.append(dist.device_tensor(ptr, n_slots * 4, dev))
    off = [int(o) for o in slot_off] + [int(n_slots)]
    for r in range(world):
        for q, f, n in runs[r]:
            bufs[q][4 * off[f]:4 * off[f + n]].copy_(bufs[r][4 * off[f]:4 * off[f + n]])
    torch.cuda.synchronize()
    for q, g in enumerate(ctxs):
        for r in range(world):
            for qq, f, n in runs[r]:
                if qq == q:
                    assert g.expandSlotIndices(f, n)
    for attempt in range(8):
        slabs = []
        for r, g in enumerate(ctxs):
            sl = g.listsShardViews(r, world, int(vb[r]), int(vb[r + 1]))
            assert sl is not None and len(sl) == 4
            slabs.append(sl)
        for k in range(4):
            sb = slabs[0][k][1]
            fulls = [dist.device_tensor(sl[k][2], sb * world, dev) for sl in slabs]
            for r in range(world):
                for q in range(world):
                    if q != r and (k == 3 or r in needs[q]):      # records: only to the ranks whose chain walks them
                        fulls[q][r * sb:(r + 1) * sb].copy_(fulls[r][r * sb:(r + 1) * sb])
        torch.cuda.synchronize()
        res = [g.tailShardCount() for g in ctxs]
        assert len({rc for rc, _, _ in res}) == 1, "every rank takes the same decision (all of them see all pool counters)"
        if res[0][0] == 0:
            break
        assert res[0][0] == -10, res                 # L3D_ERR_RETRY: pools enlarged on every rank alike
    else:
        raise AssertionError("the pools never became large enough")
    counts = [(n, h) for _, n, h in res]
    layouts = [g.tailShardLayout(world, counts, [int(v) for v in vb]) for g in ctxs]
    assert all(l is not None and len(l) == 9 for l in layouts)
    for k in range(9):
        elt, parts = layouts[0][k][1], layouts[0][k][2]
        assert all(l[k][1] == elt and l[k][2] == parts for l in layouts), "every rank derives the same layout"
        total = max(f + n for f, n in parts) * elt
        fulls = [dist.device_tensor(l[k][0], total, dev) for l in layouts]
        for r, (f, n) in enumerate(parts):
            for q in range(world):
                if q != r and n:
                    fulls[q][f * elt:(f + n) * elt].copy_(fulls[r][f * elt:(f + n) * elt])
    torch.cuda.synchronize()
    assert [g.tailShardCommit() for g in ctxs] == [0] * world
    return ctxs, counts


def _assert_slot_liveness(g, present_pairs=None, min_alive=1):
    """The list pass decides whether a fresh hypothesis is alive from the stream hyp_p (NaN = not alive, k_lists.hip), not
    from the slot's kSlotAlive flag: every producer of slots (the match epilogue, k_orient_all, k_keep_assemble, the halo
    expansion) must write both alike.  Over every slot of the present pairs (all of them when present_pairs is None): a slot
    with a target is alive in hyp_p exactly when its flags say so, and then hyp_p holds its (d_p1, d_p2) bit for bit; a slot
    without a target is not alive (the uniform-row sweep of the list pass reads it too).  Returns (alive, rejected)."""
    import torch
    from line3dpp_amd import dist
    from line3dpp_amd._lib import SLOT_DTYPE
    hyp = g.fresh_hyp()                              # (returns when the context's stream is done)
    assert hyp is not None
    ptr, n = g.slot_buffer()
    assert hyp.shape == (n, 2) and n > 0
    slots = dist.device_tensor(ptr, n * 32, torch.device("cuda", 0)).cpu().numpy().view(SLOT_DTYPE)
    mask = np.ones(n, bool)
    if present_pairs is not None:
        off = [int(o) for o in g.pairs()[1]] + [n]
        mask[:] = False
        for p in present_pairs:
            mask[off[p]:off[p + 1]] = True
    present = mask & (slots["tgt_seg"] != EMPTY)
    flag_alive = (slots["flags"] & 1) != 0
    hyp_alive = ~np.isnan(hyp[:, 0])
    bad = np.nonzero(present & (flag_alive != hyp_alive))[0]
    assert not len(bad), f"{len(bad)} present slots whose hyp_p disagrees with kSlotAlive, first {bad[:5]}"
    bad = np.nonzero(mask & ~present & hyp_alive)[0]
    assert not len(bad), f"{len(bad)} slots without a target that hyp_p calls alive, first {bad[:5]}"
    alive = present & flag_alive
    bits = hyp.view(np.uint32)
    assert np.array_equal(bits[alive, 0], slots["d_p1"].view(np.uint32)[alive])
    assert np.array_equal(bits[alive, 1], slots["d_p2"].view(np.uint32)[alive])
    assert int(alive.sum()) >= min_alive
    return int(alive.sum()), int((present & ~flag_alive).sum())
