"""Host model of phase B's tail (k_chain_sweep, k_hyp_scores, k_hyp_filter, k_seg_filter, k_seg_write, k_median_all) and
the scenes of tests/test_gpu_tail.py.

The tail works on the records the list pass left behind -- headers (HypHdr) and edges (EdgeRec), l3d_lists.h -- and the
model restates what the reference does with the hypotheses those records stand for, stage by stage, from its rule lists:
scoringCPU's accumulation (line3D.cc:1255-1274), storeInverseMatches (:1672-1699: an inverse hypothesis exists iff its
source scored > 0) and filterMatches (:1586-1668).  Every stage takes the PREVIOUS stage's records as the test hook
l3d_debug_tail_records handed them out (`rec`, Line3D.tail_records()), so that a disagreement names its stage.

Every comparison is bit equality except the end points, direction and length of the best hypotheses' 3D segments
(HypRec), which the kernel computes in fp64 from the view's rays: those are modelled in fp64 and in long double, and the
tolerance is 100 x the largest difference between the two models over the cases of the test (unproject_best)."""
import numpy as np

from line3dpp_amd._lib import EDGE_REC_DTYPE, HYP_HDR_DTYPE, MATCH_DTYPE
from line3dpp_amd.scene import Scene, make_scene

HYP_INV = 1 << 31            # l3d_lists.h: kHypInv (pair_flags)
EDGE_INV = 1 << 16           # kEdgeInv (j_cam)
HYP_EXISTS, HYP_KEEP = 1, 2  # HypHdr::state
REPLICAS = 16                # k_lists.hip: kMaxReplicas
MIN_BEST_SCORE_PERC = np.float32(0.10)   # commons.h:61
MIN_BEST_SCORE_3D = np.float32(0.75)     # commons.h:60
L3D_EPS = np.float32(1e-12)              # commons.h:97: the median of a view without best hypotheses
# Largest |fp64 - long double| of the unprojection model over the scenes of tests/test_gpu_tail.py (the tests recompute
# it for their own records and print it): end points 1.5e-13 (scene units; the medians scene, coordinates up to 500),
# direction 2.9e-14, length before its rounding to float 1.6e-13.  The tolerance is 100 x that; the kernel's largest
# distances from the fp64 model on the MI355X were 1.1e-13, 3.2e-14 and, for the float length, below half a float ulp.
HYPREC_TOL_FACTOR = 100.0


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def edge_positions(rec):
    """first edge of every header as a position in rec["edges"] (HypHdr::edge_begin counts pool * ecap + k)"""
    pos = np.searchsorted(rec["edge_index"], rec["headers"]["edge_begin"])
    n = rec["headers"]["edge_cnt"].astype(np.int64)
    assert len(rec["edge_index"]) == 0 or np.all(np.diff(rec["edge_index"].astype(np.int64)) > 0)
    assert np.all(n >= 1), "a header has at least one edge"
    assert np.all(rec["edge_index"][pos] == rec["headers"]["edge_begin"]) and np.all(pos + n <= len(rec["edges"]))
    # the edges of one header are contiguous inside its pool
    assert np.all(rec["edge_index"][pos + n - 1] == rec["headers"]["edge_begin"] + n - 1)
    return pos.astype(np.int64)


def header_view(rec):
    return (np.searchsorted(rec["seg_base"], rec["headers"]["g"], side="right") - 1).astype(np.int64)


# ---- stage 1: which hypotheses exist (the chain) -----------------------------------------------------------------------
def model_exists(rec):
    """Least fixed point.  A FRESH header is positive (score > 0) iff one of its supporters exists: a fresh supporter
    always does, an inverse one iff ITS source (the fresh hypothesis of the same slot) is positive.  An inverse header
    exists iff positive[ref].  Returns slot-level lookups: hdr_positive = positive[ref] per header, edge_positive =
    positive[ref_j] per edge, exists per header."""
    H, E = rec["headers"], rec["edges"]
    e0 = edge_positions(rec)
    fresh = (H["pair_flags"] & HYP_INV) == 0
    fresh_idx = np.nonzero(fresh)[0]
    order = np.argsort(H["ref"][fresh_idx], kind="stable")
    refs = H["ref"][fresh_idx][order]
    assert np.all(np.diff(refs.astype(np.int64)) > 0), "one fresh header per slot"

    def owner(slot):   # the fresh header of a slot, -1 if it has none (its bit is never set then)
        p = np.searchsorted(refs, slot)
        p = np.minimum(p, max(len(refs) - 1, 0))
        hit = (refs[p] == slot) if len(refs) else np.zeros(len(slot), bool)
        return np.where(hit, fresh_idx[order][p] if len(refs) else 0, -1)

    own_e = owner(E["ref_j"])
    einv = (E["j_cam"] & EDGE_INV) != 0
    hdr_of_edge = np.repeat(np.arange(len(H)), H["edge_cnt"].astype(np.int64))
    eidx = np.concatenate([np.arange(a, a + n) for a, n in zip(e0, H["edge_cnt"])]) if len(H) else np.zeros(0, np.int64)
    pos = np.zeros(len(H), bool)
    rounds = 0
    while True:
        src_pos = np.where(own_e >= 0, pos[np.maximum(own_e, 0)], False)
        ok = ~einv | src_pos
        new = np.zeros(len(H), bool)
        np.logical_or.at(new, hdr_of_edge, ok[eidx])
        new &= fresh
        if np.array_equal(new, pos):
            break
        assert not (pos & ~new).any(), "monotone"
        pos = new
        rounds += 1
    own_h = owner(H["ref"])
    hdr_positive = np.where(own_h >= 0, pos[np.maximum(own_h, 0)], False)
    edge_positive = np.where(own_e >= 0, pos[np.maximum(own_e, 0)], False)
    return dict(hdr_positive=hdr_positive.astype(np.uint8), edge_positive=edge_positive.astype(np.uint8),
                exists=fresh | hdr_positive, rounds=rounds)


# ---- stage 2: score3D ---------------------------------------------------------------------------------------------------
def accumulate(sims, cams):
    """scoringCPU's rule (line3D.cc:1255-1274) in float32, in list order: the first supporter of a camera adds its
    similarity; a later one of the same camera replaces it (subtract, add) iff it is larger"""
    score = np.float32(0.0)
    per_cam = {}
    for s, c in zip(sims, cams):
        s = np.float32(s); c = int(c)
        if c in per_cam:
            if s > per_cam[c]:
                score = np.float32(score - per_cam[c])
                score = np.float32(score + s)
                per_cam[c] = s
        else:
            score = np.float32(score + s)
            per_cam[c] = s
    return score


def model_scores(rec):
    """score3D of every header from the existing supporters (inverse ones: positive[ref_j] as the hook returned it),
    0 and state 0 for a header that does not exist"""
    H, E = rec["headers"], rec["edges"]
    e0 = edge_positions(rec)
    exists = ((H["pair_flags"] & HYP_INV) == 0) | (rec["hdr_positive"] != 0)
    ok = ((E["j_cam"] & EDGE_INV) == 0) | (rec["edge_positive"] != 0)
    out = np.zeros(len(H), np.float32)
    for i in np.nonzero(exists)[0]:
        sl = slice(e0[i], e0[i] + int(H["edge_cnt"][i]))
        m = ok[sl]
        out[i] = accumulate(E["sim"][sl][m], E["tv_j"][sl][m])
    return dict(score=out, exists=exists)


# ---- stages 3-6: view maximum, keep, best, gate and offsets --------------------------------------------------------------
def model_view_max(rec):
    """filterMatches :1592-1600: the largest score of the view, 0 without a positive one"""
    V = len(rec["seg_base"]) - 1
    s = rec["headers"]["score3D"]
    out = np.zeros(V, np.float32)
    m = s > 0
    np.maximum.at(out, header_view(rec)[m], s[m])
    return out


def model_keep(rec):
    """:1621 with score_lim = 0.1f * max_score in float32; the maximum as the kernel's replicas hold it"""
    H = rec["headers"]
    mx = rec["max_score_bits"].max(1).view(np.float32) if rec["max_score_bits"].size else np.zeros(0, np.float32)
    lim = (MIN_BEST_SCORE_PERC * mx[header_view(rec)]).astype(np.float32)
    s = H["score3D"]
    return ((H["state"] & HYP_EXISTS) != 0) & (s > 0) & (s > lim)


def canonical_order(rec):
    """positions of the headers by (segment, canonical index)"""
    H = rec["headers"]
    return np.lexsort((H["canon"], H["g"]))


def model_best(rec):
    """:1613-1627: per segment the kept headers counted and the FIRST strict maximum among them in canonical order,
    packed as k_hyp_filter packs it (score bits << 32 | ~canon); 0 for a segment that keeps nothing"""
    H = rec["headers"]
    G = int(rec["G"])
    kept = (H["state"] & HYP_KEEP) != 0
    cnt = np.zeros(G, np.uint32)
    pack = np.zeros(G, np.uint64)
    best_hdr = np.full(G, -1, np.int64)
    best_s = np.zeros(G, np.float32)
    for i in canonical_order(rec):
        if not kept[i]:
            continue
        g = int(H["g"][i])
        cnt[g] += 1
        if H["score3D"][i] > best_s[g]:      # best_match.score3D_ starts at 0
            best_s[g] = H["score3D"][i]; best_hdr[g] = i
            pack[g] = (np.uint64(_bits(H["score3D"][i])) << np.uint64(32)) | np.uint64(0xFFFFFFFF - int(H["canon"][i]))
    return dict(kept_cnt=cnt, best_pack=pack, best_hdr=best_hdr)


def model_gate(rec):
    """:1635: the segment keeps its matches and a best hypothesis iff the best score > 0.75; exclusive scan of (surviving
    matches | best hypotheses << 32) over G + 1 places"""
    best_s = (rec["best_pack"] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    ok = best_s > MIN_BEST_SCORE_3D
    n_surv = np.where(ok, rec["kept_cnt"], 0).astype(np.uint64)
    so = np.concatenate([[0], np.cumsum(n_surv)]).astype(np.uint64)
    ho = np.concatenate([[0], np.cumsum(ok.astype(np.uint64))]).astype(np.uint64)
    return dict(ok=ok, off64s=so | (ho << np.uint64(32)), surv_off=so.astype(np.uint32), hyp_off=ho.astype(np.uint32),
                n_surv=int(so[-1]), n_hyps=int(ho[-1]))


# ---- stage 7: write-out -------------------------------------------------------------------------------------------------
def model_write(rec, pairs, cams):
    """The surviving Match records in canonical order, surv_sg / surv_tg, hyp_of_seg, the best hypotheses' Match and
    depths.  pairs [P, 2]: (source cam, target cam) per directed pair; cams: the cam ids in view order."""
    H = rec["headers"]
    G = int(rec["G"])
    cams = np.asarray(cams, np.int64)
    view_of_cam = {int(c): i for i, c in enumerate(cams)}
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    off = rec["off64s"]
    ho = (off >> np.uint64(32)).astype(np.int64)
    ok = ho[1:] != ho[:-1]
    hview = header_view(rec)
    inv = (H["pair_flags"] & HYP_INV) != 0
    pr = (H["pair_flags"] & 0x7FFFFFFF).astype(np.int64)
    tgt_cam = np.where(inv, pairs[pr, 0], pairs[pr, 1]) if len(H) else np.zeros(0, np.int64)
    tgt_view = np.array([view_of_cam[int(c)] for c in tgt_cam], np.int64)
    sel = [i for i in canonical_order(rec) if (H["state"][i] & HYP_KEEP) and ok[H["g"][i]]]
    sel = np.asarray(sel, np.int64)
    m = np.zeros(len(sel), MATCH_DTYPE)
    h = H[sel]
    m["src_cam"] = cams[hview[sel]]; m["src_seg"] = h["g"] - rec["seg_base"][hview[sel]]
    m["tgt_cam"] = tgt_cam[sel]; m["tgt_seg"] = h["tgt_seg"]
    m["overlap"] = h["overlap"]; m["score3D"] = h["score3D"]
    m["d_p1"] = h["dp1"]; m["d_p2"] = h["dp2"]; m["d_q1"] = h["oq1"]; m["d_q2"] = h["oq2"]
    best_canon = 0xFFFFFFFF - (rec["best_pack"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    is_best = best_canon[h["g"]] == h["canon"]
    hyp_of_seg = np.where(ok, ho[:-1], -1).astype(np.int32)
    assert int(is_best.sum()) == int(ok.sum()), "one best header per surviving segment"
    return dict(surv=m, surv_sg=h["g"].astype(np.uint32), surv_tg=(rec["seg_base"][tgt_view[sel]] + h["tgt_seg"]).astype(np.uint32),
                hyp_of_seg=hyp_of_seg, best=m[is_best], best_view=hview[sel][is_best],
                depths=np.stack([h["dp1"][is_best], h["dp2"][is_best]], 1).astype(np.float32).reshape(-1, 2))


def unproject_best(scene, translation, best, dtype):
    """View::unprojectSegment (view.cc:356-371) + Segment3D for the best hypotheses, in `dtype` (float64 / longdouble):
    C + normalized(R^T K^-1 (x, y, 1)) * depth, in the translated frame (C_ += t, line3D.cc:436 with t = -translation)"""
    by_cam = {v.cam: v for v in scene.views}
    n = len(best)
    P1 = np.zeros((n, 3), dtype); P2 = np.zeros((n, 3), dtype); d = np.zeros((n, 3), dtype); ln = np.zeros(n, dtype)
    cache = {}
    for i, b in enumerate(best):
        cam = int(b["src_cam"])
        if cam not in cache:
            v = by_cam[cam]
            K = v.K.astype(dtype); R = v.R.astype(dtype); t = v.t.astype(dtype)
            fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
            Kinv = np.array([[1 / fx, -sk / (fx * fy), (sk * cy - cx * fy) / (fx * fy)], [0, 1 / fy, -cy / fy], [0, 0, 1]], dtype)
            cache[cam] = (R.T @ Kinv, R.T @ (-t) - np.asarray(translation, dtype), v.segs)
        RtKinv, C, segs = cache[cam]
        s = segs[int(b["src_seg"])].astype(dtype)
        r1 = RtKinv @ np.array([s[0], s[1], 1], dtype); r1 = r1 / np.sqrt((r1 * r1).sum())
        r2 = RtKinv @ np.array([s[2], s[3], 1], dtype); r2 = r2 / np.sqrt((r2 * r2).sum())
        a = C + r1 * dtype(b["d_p1"]); c = C + r2 * dtype(b["d_p2"])
        P1[i] = a; P2[i] = c
        ln[i] = np.sqrt(((a - c) ** 2).sum())
        d[i] = (c - a) / ln[i]
    return dict(P1=P1, P2=P2, dir=d, length=ln)


def hyprec_tolerances(scene, translation, best):
    """(fp64 model, tolerances): 100 x the largest fp64 to long-double difference of end points, direction and length;
    the length is a float in the record, so half a float ulp of the largest length is added to its tolerance"""
    a = unproject_best(scene, translation, best, np.float64)
    b = unproject_best(scene, translation, best, np.longdouble)
    diff = {k: float(np.abs(a[k].astype(np.longdouble) - b[k]).max()) if len(best) else 0.0 for k in a}
    tol = dict(P=HYPREC_TOL_FACTOR * max(diff["P1"], diff["P2"]), dir=HYPREC_TOL_FACTOR * diff["dir"],
               length=HYPREC_TOL_FACTOR * diff["length"] + (float(np.spacing(np.float32(a["length"].max()))) / 2 if len(best) else 0.0))
    return a, tol, diff


# ---- stage 8: medians ---------------------------------------------------------------------------------------------------
def model_medians(rec):
    """:1657-1663: sorted(depths of the view's best hypotheses)[n / 2], L3D_EPS without any"""
    V = len(rec["seg_base"]) - 1
    out = np.zeros(V, np.float32)
    for v in range(V):
        d = rec["depths"][rec["hyp_off"][rec["seg_base"][v]]:rec["hyp_off"][rec["seg_base"][v + 1]]].ravel()
        out[v] = np.sort(d)[len(d) // 2] if len(d) else L3D_EPS
    return out


# ---- the whole comparison -----------------------------------------------------------------------------------------------
def check_stages(rec, pairs, cams):
    """every stage of the tail against the model, each fed with the records the hook returned for the stage before;
    returns the write-out model (for the comparison with the accessors)"""
    H = rec["headers"]
    ex = model_exists(rec)
    assert np.array_equal(ex["hdr_positive"], rec["hdr_positive"]), "exists: positive[ref] of the headers"
    assert np.array_equal(ex["edge_positive"], rec["edge_positive"]), "exists: positive[ref_j] of the edges"
    sc = model_scores(rec)
    assert np.array_equal((H["state"] & HYP_EXISTS) != 0, sc["exists"]), "score: state bit 0"
    bad = np.nonzero(_bits(sc["score"]) != _bits(H["score3D"]))[0]
    assert not len(bad), ("score: score3D bits", len(bad), H[bad[:4]], sc["score"][bad[:4]])
    vm = model_view_max(rec)
    assert np.array_equal(_bits(vm), rec["max_score_bits"].max(1)), "view max"
    assert np.array_equal(model_keep(rec), (H["state"] & HYP_KEEP) != 0), "keep: state bit 1"
    b = model_best(rec)
    assert np.array_equal(b["kept_cnt"], rec["kept_cnt"]), "best: kept_cnt"
    assert np.array_equal(b["best_pack"], rec["best_pack"]), "best: best_pack"
    g = model_gate(rec)
    assert np.array_equal(g["off64s"], rec["off64s"]), "gate: off64s"
    assert np.array_equal(g["surv_off"], rec["surv_off"]) and np.array_equal(g["hyp_off"], rec["hyp_off"]), "gate: offsets"
    assert (g["n_surv"], g["n_hyps"]) == (rec["n_surv"], rec["n_hyps"]), "gate: totals"
    w = model_write(rec, pairs, cams)
    assert np.array_equal(w["surv_sg"], rec["surv_sg"]) and np.array_equal(w["surv_tg"], rec["surv_tg"]), "write-out: surv_sg / surv_tg"
    assert np.array_equal(w["hyp_of_seg"], rec["hyp_of_seg"]), "write-out: hyp_of_seg"
    assert np.array_equal(_bits(w["depths"]), _bits(rec["depths"])), "write-out: depths"
    assert np.array_equal(_bits(model_medians(rec)), _bits(rec["medians"])), "median"
    w["gate_ok"] = g["ok"]; w["best_hdr"] = b["best_hdr"]
    return w


def records_by_segment(rec):
    """the records as a set per segment, free of where the pools put them: per segment the headers in canonical order
    (edge_begin and padding left out), each with its edges, as bytes"""
    H = rec["headers"]
    e0 = edge_positions(rec)
    fields = [f for f in HYP_HDR_DTYPE.names if f not in ("edge_begin", "pad")]
    out = {}
    for i in canonical_order(rec):
        key = int(H["g"][i])
        part = b"".join(H[f][i].tobytes() for f in fields) + rec["edges"][e0[i]:e0[i] + int(H["edge_cnt"][i])].tobytes()
        out[key] = out.get(key, b"") + part + bytes([rec["hdr_positive"][i]])
    return out


# ---- hand-written records -----------------------------------------------------------------------------------------------
def make_records(seg_base, headers):
    """Records as the hook returns them, from a list of headers dict(g, ref, canon, inv (bool), pair, dp (2), tgt_seg,
    overlap, oq (2), edges = [(ref_j, sim, inverse, camera)]); one pool, edges back to back.  The outputs of the
    kernels (positive bits, scores, states, ...) are left zero: the caller fills them from the model stage by stage."""
    H = np.zeros(len(headers), HYP_HDR_DTYPE)
    E = []
    for i, h in enumerate(headers):
        H[i]["g"] = h["g"]; H[i]["ref"] = h["ref"]; H[i]["canon"] = h["canon"]
        H[i]["pair_flags"] = h.get("pair", 0) | (HYP_INV if h.get("inv") else 0)
        H[i]["dp1"], H[i]["dp2"] = h.get("dp", (1.0, 1.0))
        H[i]["tgt_seg"] = h.get("tgt_seg", 0); H[i]["overlap"] = h.get("overlap", 0.5)
        H[i]["oq1"], H[i]["oq2"] = h.get("oq", (1.0, 1.0))
        H[i]["edge_begin"] = len(E); H[i]["edge_cnt"] = len(h["edges"])
        for j, (ref_j, sim, inv, cam) in enumerate(h["edges"]):
            E.append((ref_j, sim, j | (EDGE_INV if inv else 0), cam))
    E = np.array(E, EDGE_REC_DTYPE) if E else np.zeros(0, EDGE_REC_DTYPE)
    seg_base = np.asarray(seg_base, np.uint32)
    G, V = int(seg_base[-1]), len(seg_base) - 1
    return dict(G=G, V=V, pools=1, ecap=max(len(E), 1), hcap=max(len(H), 1), scap=1, seg_base=seg_base, headers=H, edges=E,
                edge_index=np.arange(len(E), dtype=np.uint32), hdr_pool=np.zeros(len(H), np.uint32),
                hdr_index=np.arange(len(H), dtype=np.uint32))


def run_model(rec, pairs, cams):
    """the model alone, stage by stage on its own outputs: fills `rec` as the kernels would and returns the write-out"""
    ex = model_exists(rec)
    rec["hdr_positive"], rec["edge_positive"] = ex["hdr_positive"], ex["edge_positive"]
    sc = model_scores(rec)
    rec["headers"]["score3D"] = sc["score"]; rec["headers"]["state"] = np.where(sc["exists"], HYP_EXISTS, 0)
    vm = model_view_max(rec)
    rec["max_score_bits"] = np.zeros((rec["V"], REPLICAS), np.uint32); rec["max_score_bits"][:, 0] = _bits(vm)
    rec["headers"]["state"] |= np.where(model_keep(rec), HYP_KEEP, 0).astype(np.uint32)
    b = model_best(rec)
    rec["kept_cnt"], rec["best_pack"] = b["kept_cnt"], b["best_pack"]
    g = model_gate(rec)
    for k in ("off64s", "surv_off", "hyp_off", "n_surv", "n_hyps"):
        rec[k] = g[k]
    w = model_write(rec, pairs, cams)
    rec["surv_sg"], rec["surv_tg"], rec["hyp_of_seg"], rec["depths"] = w["surv_sg"], w["surv_tg"], w["hyp_of_seg"], w["depths"]
    rec["medians"] = model_medians(rec)
    w["chain_rounds"] = ex["rounds"]
    return w


# ---- scenes -------------------------------------------------------------------------------------------------------------
def two_depth_scene(n_views, n_segs, seed, far_scale=12.0, far_dist=400.0):
    """One near and one far structure in the same views: the box of make_scene around the origin and a copy of it, scaled
    by far_scale, far_dist behind it as the cameras look (they stand on a short arc at radius 25 and look at the origin).
    Every view holds noise-free images of both, half of its segments each where enough are visible, so that the depths of
    its best hypotheses lie around 20 and around far_dist: more than a factor 16 apart."""
    from line3dpp_amd.scene import FOCAL, HEIGHT, MIN_LEN, WIDTH, ViewData, _clip_segments, _lookat, _scene_lines
    rng = np.random.default_rng(seed)
    P, Q, N = _scene_lines(rng, 6 * n_segs)
    c = -far_dist * np.array([np.cos(np.pi / 4), np.sin(np.pi / 4), 0.0])
    P = np.concatenate([P, P * far_scale + c]); Q = np.concatenate([Q, Q * far_scale + c]); N = np.concatenate([N, N])
    far = np.arange(len(P)) >= len(P) // 2
    K = np.array([[FOCAL, 0, WIDTH / 2], [0, FOCAL, HEIGHT / 2], [0, 0, 1.0]])
    views = []
    for i in range(n_views):
        phi = np.pi / 4 + np.deg2rad(24.0) * (i / max(n_views - 1, 1) - 0.5)
        Cc = np.array([25.0 * np.cos(phi), 25.0 * np.sin(phi), rng.uniform(-2, 2)])
        R = _lookat(Cc, np.zeros(3))
        t = -R @ Cc
        Xp = (R @ P.T).T + t; Xq = (R @ Q.T).T + t
        ok = (Xp[:, 2] > 1.0) & (Xq[:, 2] > 1.0) & (((Cc[None, :] - P) * N).sum(1) > 0.5)
        idx = np.nonzero(ok)[0]
        xp = (K @ Xp[idx].T).T; xq = (K @ Xq[idx].T).T
        inside, pc, qc = _clip_segments(xp[:, :2] / xp[:, 2:3], xq[:, :2] / xq[:, 2:3], WIDTH, HEIGHT)
        inside &= np.hypot(*(pc - qc).T) >= MIN_LEN
        idx, seg = idx[inside], np.concatenate([pc, qc], 1)[inside]
        pick = np.concatenate([np.nonzero(far[idx])[0][:n_segs // 2], np.nonzero(~far[idx])[0][:n_segs - n_segs // 2]])
        seg = seg[np.sort(pick)]
        length = np.hypot(seg[:, 0] - seg[:, 2], seg[:, 1] - seg[:, 3])
        seg = seg[np.argsort(-length, kind="stable")].astype(np.float32)
        nb = sorted({j for j in (i - 2, i - 1, i + 1, i + 2) if 0 <= j < n_views})
        views.append(ViewData(i, seg, K.copy(), R, t, WIDTH, HEIGHT, 25.0, nb))
    return Scene(views, f"twodepth{n_views}x{n_segs}")


def merge_scenes(parts, name):
    """several scenes under distinct cam ids (the k-th scene's cams shifted behind those before it), no pairs between them"""
    views, base = [], 0
    for sc in parts:
        for v in sc.views:
            v.cam += base
            v.neighbors = [int(x) + base for x in v.neighbors]
            views.append(v)
        base = max(v.cam for v in views) + 1
    return Scene(views, name)


# ---- what a scene holds, from the CPU oracle ----------------------------------------------------------------------------
def oracle_counts(o, scene):
    """From the lists Oracle(record_scored=True) recorded right after scoring: filterMatches restated per view ->
    per view dict(n_pos (hypotheses with score > 0), n_best, n_depths, median_dups (how often the median value occurs
    among the depths), depth_span (largest / smallest depth of the best hypotheses), even_half (n_depths / 2 even)) and
    the totals ties (segments whose best score is attained by two or more kept hypotheses), gated (segments with kept
    hypotheses whose best is <= 0.75), passed (segments above it), exact_075 (best == 0.75)."""
    out = dict(views={}, ties=0, gated=0, passed=0, exact_075=0)
    for v in scene.views:
        s, off = o.scored(v.cam)
        sc = s["score3D"]
        mx = np.float32(sc.max()) if len(sc) and sc.max() > 0 else np.float32(0)
        lim = np.float32(MIN_BEST_SCORE_PERC * mx)
        kept = (sc > 0) & (sc > lim)
        depths = []
        for i in range(len(off) - 1):
            k = kept[off[i]:off[i + 1]]
            if not k.any():
                continue
            ss = sc[off[i]:off[i + 1]][k]
            b = int(np.argmax(ss))          # first maximum
            if ss[b] > MIN_BEST_SCORE_3D:
                out["passed"] += 1
                out["ties"] += int((ss == ss[b]).sum() >= 2)
                r = s[off[i]:off[i + 1]][k][b]
                depths += [r["d_p1"], r["d_p2"]]
            else:
                out["gated"] += 1
                out["exact_075"] += int(ss[b] == MIN_BEST_SCORE_3D)
        d = np.sort(np.asarray(depths, np.float32))
        med = d[len(d) // 2] if len(d) else L3D_EPS
        out["views"][v.cam] = dict(n_pos=int((sc > 0).sum()), n_best=len(d) // 2, n_depths=len(d),
                                   median_dups=int((d == med).sum()), depth_span=float(d[-1] / d[0]) if len(d) else 0.0,
                                   even_half=(len(d) // 2) % 2 == 0, median=np.float32(med))
    return out


# ---- what the records of a pass hold ------------------------------------------------------------------------------------
def record_stats(rec):
    """Counts that show which branches of the tail a pass reached, from the hook's records: edge_cnt values present;
    headers with two consecutive existing supporters of one camera, the later one larger / smaller (replace / keep);
    headers in whose existing supporters a camera returns after another one; inverse supporters that do not exist; the
    largest number of distinct views among the positive headers of one wave of k_hyp_scores (64 consecutive headers
    of a pool)."""
    H, E = rec["headers"], rec["edges"]
    e0 = edge_positions(rec)
    ok = ((E["j_cam"] & EDGE_INV) == 0) | (rec["edge_positive"] != 0)
    exists = (H["state"] & HYP_EXISTS) != 0
    larger = smaller = returns = 0
    for i in np.nonzero(exists & (H["edge_cnt"] >= 2))[0]:
        sl = slice(e0[i], e0[i] + int(H["edge_cnt"][i]))
        cams, sims = E["tv_j"][sl][ok[sl]], E["sim"][sl][ok[sl]]
        same = cams[1:] == cams[:-1]
        larger += int((same & (sims[1:] > sims[:-1])).any())
        smaller += int((same & (sims[1:] < sims[:-1])).any())
        runs = cams[np.concatenate([[True], ~same])] if len(cams) else cams
        returns += int(len(set(runs.tolist())) < len(runs))
    view = header_view(rec)
    wave = rec["hdr_pool"].astype(np.int64) * (1 << 20) + rec["hdr_index"] // 64
    views_in_wave = 0
    pos = H["score3D"] > 0
    for w in np.unique(wave[pos]):
        views_in_wave = max(views_in_wave, len(set(view[pos & (wave == w)].tolist())))
    return dict(edge_cnts=sorted(set(H["edge_cnt"].tolist())), later_larger=larger, later_smaller=smaller, camera_returns=returns,
                dead_inverse_supporters=int((((E["j_cam"] & EDGE_INV) != 0) & (rec["edge_positive"] == 0)).sum()),
                views_in_one_wave=views_in_wave, headers=len(H), edges=len(E))


def filter_counts(rec):
    """ties for best, gated and passed segments, per-view positive headers and best hypotheses, from the records"""
    H = rec["headers"]
    kept = (H["state"] & HYP_KEEP) != 0
    best_s = (rec["best_pack"] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    at_best = kept & (H["score3D"] == best_s[H["g"]])
    n_at_best = np.bincount(H["g"][at_best], minlength=rec["G"])
    has_kept = rec["kept_cnt"] > 0
    ok = best_s > MIN_BEST_SCORE_3D
    V = len(rec["seg_base"]) - 1
    view = header_view(rec)
    n_best = np.array([int(rec["hyp_off"][rec["seg_base"][v + 1]]) - int(rec["hyp_off"][rec["seg_base"][v]]) for v in range(V)])
    return dict(ties=int((ok & (n_at_best >= 2)).sum()), gated=int((has_kept & ~ok).sum()), passed=int(ok.sum()),
                n_pos=np.bincount(view[H["score3D"] > 0], minlength=V), n_best=n_best)


# ---- the scenes of tests/test_gpu_tail.py (tests/test_tail_cases.py shows with the CPU oracle what each holds) ------------
KNN, EPI = 10, 0.25


def accumulation_scene(n_neighbors=12, noise_px=0.0, doubled=80):
    """lists_cases.hub_scene (10 views x 150 segments on a quarter arc, the last view a neighbour of all) with every view
    a neighbour of every other, noise-free images, and the `doubled` longest segments of every view present twice: a
    hypothesis has supporters in up to nine cameras, and several in one camera where 3D lines overlap or a target is
    doubled -- headers of 1 to 8 edges"""
    sc = make_scene(40, 150, n_neighbors=n_neighbors, seed=1, real_fraction=0.9, noise_px=noise_px, max_views=10)
    hub = max(v.cam for v in sc.views)
    have = {v.cam for v in sc.views}
    for v in sc.views:
        v.neighbors = sorted((set(v.neighbors) & have) | {hub}) if v.cam != hub else sorted(have - {hub})
        v.segs[1:doubled:2] = v.segs[0:doubled - 1:2]
    sc.name = "accumulation"
    return sc


def gate_scene():
    from tests import lists_cases as LC
    return LC.hub_scene(10, 150, 4, 1, real_fraction=0.9)


def view_max_scene():
    from tests import lists_cases as LC
    return LC.mixed_scene([300, 3, 4, 5, 6, 300, 3, 4, 5, 6, 6, 5], 6, 1, real_fraction=0.9)


def ties_scene():
    """every segment occurs twice in its view (tests/test_gpu_parity.py: test_equal_overlaps_follow_the_reference_heap_
    order), on the hub scene: the two copies of a target give a segment two hypotheses of equal score"""
    sc = gate_scene()
    for v in sc.views:
        v.segs[1::2] = v.segs[0::2]
    sc.name = "ties"
    return sc


MEDIAN_CUTS = [1300, 536, 546, 1300, 4, 3]


def medians_scene():
    """Three scenes without pairs between them.  Cams 0-5: two_depth_scene cut to MEDIAN_CUTS -- the views of cams 0 and 3
    keep exactly 512 and 513 best hypotheses (a best hypothesis needs its supporters in the neighbouring views, which
    the cut views 1 and 2 bound).  Cams 6-8: three full views of 1300, more than 1024 best hypotheses each.  Cams 9-20:
    the tiny views of lists_cases.mixed_scene, among them views with one best hypothesis and with none."""
    from tests import lists_cases as LC
    b = two_depth_scene(6, 1300, 7)
    for v, m in zip(b.views, MEDIAN_CUTS):
        v.segs = v.segs[:m].copy()
    return merge_scenes([b, two_depth_scene(3, 1300, 9), LC.mixed_scene([300, 3, 4, 5, 6, 300, 3, 4, 5, 6, 6, 5], 6, 3, real_fraction=0.9)],
                        "medians")


def grid_scene():
    """many cluttered segments, few headers: two views of 6000 clutter segments beside a ring of 6 views x 100"""
    ring = make_scene(6, 100, n_neighbors=4, seed=11, real_fraction=0.9)
    clutter = make_scene(2, 6000, n_neighbors=2, seed=12, real_fraction=0.02)
    return merge_scenes([ring, clutter], "grid")


def keep_all_scene():
    from tests import lists_cases as LC
    return LC.hub_scene(6, 100, 4, 1, real_fraction=0.9)
