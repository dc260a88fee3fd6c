"""The affinity fill (k_affinity.hip, l3d_affinity_host.hip) restated in numpy, one function per stage, and the scenes its
tests run (tests/test_affinity_cases.py on the CPU oracle, tests/test_gpu_affinity.py on the GPU).

Every function takes a `rec` dict as Line3D.affinity_records() returns it (plus `seg_base` and `cams`, see with_scene), so
that a disagreement names its stage.  records_from_oracle builds the same dict from the CPU oracle alone.

    model_candidates   cand_a / cand_b from hyp_of_seg
    model_sim          the similarity with every operation typed as k_aff_sim types it
    model_sim_fp64     the same quantity in fp64 throughout (reporting only)
    model_flag, model_epos, model_first_touch, model_touch_rank, model_emit     the parallel stages
    model_sequential   the reference's rule (line3D.cc:1852-2023) restated on its own: must give model_emit's bytes
    model_collinear    findCollinCPU per view, the child and own streams, the host pass (l3d_affinity_host.hip)
"""
import copy
import functools
import math

import numpy as np

from line3dpp_amd._lib import CLEDGE_DTYPE, HYP_REC_DTYPE, SEGMENT2D_DTYPE

f32, f64, u32, i32 = np.float32, np.float64, np.uint32, np.int32
L3D_EPS = 1e-12
MIN_AFFINITY = f32(0.5)
EMPTY = 0xFFFFFFFF
TERMS = ("angle", "d11", "d12", "d21", "d22")


# ---- the similarity -------------------------------------------------------------------------------------------------------
def _libm(fn, x):
    """the C library's double function element by element (numpy's vector forms differ between CPUs in the last bit)"""
    return np.array([fn(v) for v in np.asarray(x, f64).tolist()], f64).reshape(np.shape(x))


def _dist_p2l(P1, d, P):
    """Segment3D::distance_Point2Line (segment3D.h:69-73) in Eigen's order: the outer product dir dir^T first, its rows
    summed left to right; fp64, the norm (x^2 + (y^2 + z^2)) cast to float"""
    v = P - P1
    h = [P1[:, r] + (((d[:, r] * v[:, 0]) * d[:, 0] + (d[:, r] * v[:, 1]) * d[:, 1]) + (d[:, r] * v[:, 2]) * d[:, 2]) for r in range(3)]
    e = [h[r] - P[:, r] for r in range(3)]
    return np.sqrt(e[0] * e[0] + (e[1] * e[1] + e[2] * e[2])).astype(f32)


def model_sim(rec, ha, hb, details=False):
    """sim_affinity (k_affinity.hip) for the hypothesis pairs (ha[i], hb[i]), operation by operation in the kernel's types.
    details: also the intermediate values class_counts reads."""
    ha, hb = np.asarray(ha, np.int64), np.asarray(hb, np.int64)
    hy = rec["hyps"]
    h1, h2 = hy[ha], hy[hb]
    k, med = rec["view_k"].astype(f32), rec["medians"].astype(f32)
    msdl, two_sig = f32(rec["msdl_dev"][0]), f32(rec["two_sigA_sqr"])
    with np.errstate(all="ignore"):
        a, b = h1["dir"], h2["dir"]
        dot = (a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])).astype(f32)
        clamped = np.fmax(np.fmin(dot, f32(1)), f32(-1))
        ang0 = (_libm(math.acos, clamped.astype(f64)) / math.pi * 180.0).astype(f32)
        folded = ang0 > f32(90)
        ang = np.where(folded, f32(180) - ang0, ang0).astype(f32)
        y_a = ((-ang) * ang / two_sig).astype(f32)
        k1, k2 = k[h1["view"]], k[h2["view"]]
        md1, md2 = med[h1["view"]], med[h2["view"]]
        if f64(msdl) > L3D_EPS:
            c1, c2 = np.fmin(md1, msdl), np.fmin(md2, msdl)
        else:
            c1, c2 = md1, md2
        d = [_dist_p2l(h2["P1"], h2["dir"], h1["P1"]), _dist_p2l(h2["P1"], h2["dir"], h1["P2"]),
             _dist_p2l(h1["P1"], h1["dir"], h2["P1"]), _dist_p2l(h1["P1"], h1["dir"], h2["P2"])]
        dp = [h1["m"]["d_p1"], h1["m"]["d_p2"], h2["m"]["d_p1"], h2["m"]["d_p2"]]
        cut, kk = [c1, c1, c2, c2], [k1, k1, k2, k2]
        over = [dp[i] > cut[i] for i in range(4)]
        ys = [y_a]
        for i in range(4):
            sig = np.where(over[i], cut[i] * kk[i], dp[i] * kk[i]).astype(f32)
            reg = (f32(2) * sig * sig).astype(f32)
            ys.append(((-d[i]) * d[i] / reg).astype(f32))
        y = np.fmin(ys[0], np.fmin(np.fmin(ys[1], ys[2]), np.fmin(ys[3], ys[4])))
        sim = _libm(math.exp, y.astype(f64)).astype(f32)
    short = (h1["length"].astype(f64) < L3D_EPS) | (h2["length"].astype(f64) < L3D_EPS)
    sim = np.where(short, f32(0), sim).astype(f32)
    if not details:
        return sim
    ys = np.stack(ys, 1)
    return sim, dict(short=short, dot=dot, clamped=np.abs(dot) > f32(1), folded=folded, over=np.stack(over, 1),
                     capped=np.stack([md1 > c1, md2 > c2], 1), ys=ys, y=y, acos_arg=clamped)


def model_sim_fp64(rec, ha, hb):
    """the same quantity with no float rounding anywhere: what the float path approximates"""
    ha, hb = np.asarray(ha, np.int64), np.asarray(hb, np.int64)
    hy = rec["hyps"]
    h1, h2 = hy[ha], hy[hb]
    k, med = rec["view_k"].astype(f64), rec["medians"].astype(f64)
    msdl, two_sig = f64(rec["msdl_dev"][0]), f64(rec["two_sigA_sqr"])

    def dist(s, P):
        v = P - s["P1"]
        foot = s["P1"] + (s["dir"] * v).sum(1)[:, None] * s["dir"]
        return np.linalg.norm(foot - P, axis=1)
    with np.errstate(all="ignore"):
        ang = np.degrees(np.arccos(np.clip((h1["dir"] * h2["dir"]).sum(1), -1, 1)))
        ang = np.where(ang > 90, 180 - ang, ang)
        ys = [-ang * ang / two_sig]
        for (s, o, P) in ((h1, h2, "P1"), (h1, h2, "P2"), (h2, h1, "P1"), (h2, h1, "P2")):
            cut = med[s["view"]]
            if msdl > L3D_EPS:
                cut = np.minimum(cut, msdl)
            dpv = s["m"]["d_p1" if P == "P1" else "d_p2"].astype(f64)
            sig = np.minimum(dpv, cut) * k[s["view"]]
            dd = dist(o, s[P])
            ys.append(-dd * dd / (2 * sig * sig))
        out = np.exp(np.fmin.reduce(ys))
    short = (h1["length"].astype(f64) < L3D_EPS) | (h2["length"].astype(f64) < L3D_EPS)
    return np.where(short, 0.0, out)


# ---- the stages -----------------------------------------------------------------------------------------------------------
def model_candidates(rec):
    hs = rec["hyp_of_seg"].astype(i32)
    return hs[rec["surv_sg"]], hs[rec["surv_tg"]]


def eligible(cand_a, cand_b):
    """a candidate whose two segments both have a hypothesis: the only ones that may carry a value above 0.5"""
    return (cand_a >= 0) & (cand_b >= 0)


def model_simv(rec, cand_a, cand_b):
    """k_aff_sim: 0 for a candidate with a segment without a hypothesis"""
    sim = np.zeros(len(cand_a), f32)
    e = np.nonzero(eligible(cand_a, cand_b))[0]
    if len(e):
        sim[e] = model_sim(rec, cand_a[e], cand_b[e])
    return sim


def reverse_index(rec):
    """for every candidate (sg -> tg) the first candidate (tg -> sg) in tg's list, or -1"""
    sg, tg = rec["surv_sg"].astype(np.int64), rec["surv_tg"].astype(np.int64)
    G = int(rec["G"])
    key = sg * (G + 1) + tg
    uk, first = np.unique(key, return_index=True)      # first occurrence of every (source, target)
    want = tg * (G + 1) + sg
    pos = np.searchsorted(uk, want)
    pos_c = np.minimum(pos, max(len(uk) - 1, 0))
    found = (uk[pos_c] == want) if len(uk) else np.zeros(len(want), bool)
    return np.where(found, first[pos_c] if len(uk) else 0, -1).astype(np.int64)


def model_flag(rec, simv, cand_a, cand_b):
    """k_aff_flag: a passing candidate emits unless its target's hypothesis comes earlier, the target's list holds the
    reverse match and that one passes too"""
    with np.errstate(invalid="ignore"):
        ok = simv > MIN_AFFINITY
    rev = reverse_index(rec)
    rev_ok = np.zeros(len(simv), bool)
    has = rev >= 0
    rev_ok[has] = ok[rev[has]]
    return (ok & ~((cand_b < cand_a) & rev_ok)).astype(u32)


def model_epos(flag):
    c = np.cumsum(flag, dtype=np.uint64)
    return (c - flag).astype(u32), int(c[-1]) if len(c) else 0


def model_first_touch(flag, epos, cand_a, cand_b, H):
    ft = np.full(H, EMPTY, np.int64)
    f = np.nonzero(flag)[0]
    np.minimum.at(ft, cand_a[f], 2 * epos[f].astype(np.int64))
    np.minimum.at(ft, cand_b[f], 2 * epos[f].astype(np.int64) + 1)
    return ft.astype(u32)


def model_touch_rank(first_touch, n_cand):
    tf = np.zeros(2 * n_cand + 1, u32)
    tf[first_touch[first_touch != EMPTY]] = 1
    c = np.cumsum(tf[:2 * n_cand], dtype=np.uint64)
    return tf, (c - tf[:2 * n_cand]).astype(u32), int(c[-1]) if len(c) else 0


def model_emit(rec, flag, epos, cand_a, cand_b, simv, first_touch, touch_rank, n_rows):
    f = np.nonzero(flag)[0]
    k = epos[f].astype(np.int64)
    ha, hb = cand_a[f], cand_b[f]
    id1, id2 = touch_rank[first_touch[ha]].astype(i32), touch_rank[first_touch[hb]].astype(i32)
    edges = np.zeros(2 * len(f), CLEDGE_DTYPE)
    edges["i"][2 * k] = id1; edges["j"][2 * k] = id2; edges["w"][2 * k] = simv[f]
    edges["i"][2 * k + 1] = id2; edges["j"][2 * k + 1] = id1; edges["w"][2 * k + 1] = simv[f]
    l2g = np.zeros(n_rows, SEGMENT2D_DTYPE)
    m = rec["hyps"]["m"]
    for h, idx, par in ((ha, id1, 0), (hb, id2, 1)):
        w = first_touch[h] == 2 * k + par
        l2g["cam"][idx[w]] = m["src_cam"][h[w]]; l2g["seg"][idx[w]] = m["src_seg"][h[w]]
    return edges, l2g


def run_stages(rec, simv=None):
    """every stage of the parallel path from the inputs (simv = None: the model's own similarities) -> dict"""
    ca, cb = model_candidates(rec)
    if simv is None:
        simv = model_simv(rec, ca, cb)
    n, H = len(ca), int(rec["H"])
    if not (n and H):
        return dict(cand_a=ca[:0], cand_b=cb[:0], simv=np.zeros(0, f32), flag=np.zeros(0, u32), epos=np.zeros(0, u32),
                    epos_total=0, first_touch=np.zeros(0, u32), touch_flag=np.zeros(0, u32), touch_rank=np.zeros(0, u32),
                    touch_total=0, edges=np.zeros(0, CLEDGE_DTYPE), l2g=np.zeros(0, SEGMENT2D_DTYPE))
    flag = model_flag(rec, simv, ca, cb)
    epos, e_tot = model_epos(flag)
    ft = model_first_touch(flag, epos, ca, cb, H)
    tf, tr, t_tot = model_touch_rank(ft, n)
    edges, l2g = model_emit(rec, flag, epos, ca, cb, simv, ft, tr, t_tot)
    return dict(cand_a=ca, cand_b=cb, simv=simv, flag=flag, epos=epos, epos_total=e_tot, first_touch=ft, touch_flag=tf,
                touch_rank=tr, touch_total=t_tot, edges=edges, l2g=l2g)


INT_STAGES = ("cand_a", "cand_b", "flag", "epos", "epos_total", "first_touch", "touch_flag", "touch_rank", "touch_total")


def check_stages(rec, w, what=""):
    """the hook's arrays (mode 0) against the model's `w`, tolerance 0; simv is compared by the caller"""
    for k in INT_STAGES:
        a, b = rec[k], w[k]
        assert (a == b) if np.isscalar(b) else (a.tobytes() == np.asarray(b, a.dtype).tobytes()), (what, k)
    assert rec["n_edges"] == len(w["edges"]) and rec["n_rows"] == len(w["l2g"]), (what, "counts")
    assert rec["edges"].tobytes() == w["edges"].tobytes(), (what, "edges")
    assert rec["l2g"].tobytes() == w["l2g"].tobytes(), (what, "l2g")


def seg_of_hyp(rec):
    out = np.full(int(rec["H"]), -1, np.int64)
    g = np.nonzero(rec["hyp_of_seg"] >= 0)[0]
    out[rec["hyp_of_seg"][g]] = g
    return out


def model_sequential(rec, simv, coll=None):
    """computingAffinityMatrix as the reference walks it: hypotheses ascending, each one's surviving matches in list
    order; the first passing candidate of an unordered segment pair claims it (`used`), a failing one claims nothing; row
    ids in first-touch order.  coll = (child_off, child_seg, child_sim, own_off, own_seg, own_sim): the links to collinear
    segments (line3D.cc:1904-1974).  -> (edges, l2g) with l2g as global segments"""
    so, tg = rec["surv_off"], rec["surv_tg"]
    used, local, rows, out = set(), {}, [], []

    def unused(a, b):
        key = (a, b) if a < b else (b, a)
        if key in used:
            return False
        used.add(key)
        return True

    def get_id(g):
        if g not in local:
            local[g] = len(rows); rows.append(g)
        return local[g]

    def push(i, j, w):
        out.append((i, j, w)); out.append((j, i, w))
    for h, a in enumerate(seg_of_hyp(rec).tolist()):
        if a < 0:
            continue
        id1, found = -1, False
        for p in range(int(so[a]), int(so[a + 1])):
            b = int(tg[p])
            if simv[p] > MIN_AFFINITY and unused(a, b):
                if id1 < 0:
                    id1 = get_id(a)
                push(id1, get_id(b), simv[p])
                found = True
                if coll is not None:
                    for q in range(int(coll[0][p]), int(coll[0][p + 1])):
                        x = int(coll[1][q])
                        if coll[2][q] > MIN_AFFINITY and unused(a, x):
                            push(id1, get_id(x), coll[2][q])
        if coll is not None and found and id1 >= 0:
            for q in range(int(coll[3][h]), int(coll[3][h + 1])):
                x = int(coll[4][q])
                if coll[5][q] > MIN_AFFINITY and unused(a, x):
                    push(id1, get_id(x), coll[5][q])
    return np.array(out, CLEDGE_DTYPE) if out else np.zeros(0, CLEDGE_DTYPE), np.array(rows, np.int64)


def l2g_of_segments(rec, segs):
    """global segments -> (cam, seg) records"""
    sb = np.asarray(rec["seg_base"], np.int64)
    vi = np.searchsorted(sb, segs, side="right") - 1
    out = np.zeros(len(segs), SEGMENT2D_DTYPE)
    out["cam"] = np.asarray(rec["cams"], np.int64)[vi] if len(segs) else 0
    out["seg"] = segs - sb[vi]
    return out


# ---- the collinear path ---------------------------------------------------------------------------------------------------
def collinear_lists(segs, t):
    """View::findCollinCPU (view.cc:213-258) on one view's float segments -> CSR (off [M + 1], idx ascending)"""
    s = np.asarray(segs, f32).astype(f64)
    M = len(s)
    x0, y0, x1, y1 = (s[:, i] for i in range(4))
    line = np.stack([y0 - y1, x1 - x0, x0 * y1 - y0 * x1], 1)          # cross((x0, y0, 1), (x1, y1, 1))
    den = np.sqrt((line[:, 0] * line[:, 0] + line[:, 1] * line[:, 1]).astype(f32)).astype(f64)

    def on_seg(ax, ay, bx, by, px, py):                                # View::pointOnSegment, view.cc:292-298
        return ((ax - px) * (bx - px) + (ay - py) * (by - py)) < L3D_EPS

    def d_line(li, px, py):                                            # distance_point2line_2D of line li[r], point [c]
        with np.errstate(all="ignore"):
            return np.abs(((line[li, 0, None] * px + line[li, 1, None] * py) + line[li, 2, None]) / den[li, None]).astype(f32)
    r = np.arange(M)
    R = lambda a: a[:, None]
    Cc = lambda a: a[None, :]
    overlap = on_seg(R(x0), R(y0), R(x1), R(y1), Cc(x0), Cc(y0)) | on_seg(R(x0), R(y0), R(x1), R(y1), Cc(x1), Cc(y1)) | \
        on_seg(Cc(x0), Cc(y0), Cc(x1), Cc(y1), R(x0), R(y0)) | on_seg(Cc(x0), Cc(y0), Cc(x1), Cc(y1), R(x1), R(y1))
    d1 = np.fmax(d_line(r, Cc(x0), Cc(y0)), d_line(r, Cc(x1), Cc(y1)))                  # [r, c]: line r, points of c
    with np.errstate(all="ignore"):                                   # [r, c]: line c, points of r
      d2 = np.fmax(np.abs(((line[None, :, 0] * R(x0) + line[None, :, 1] * R(y0)) + line[None, :, 2]) / den[None, :]).astype(f32),
                   np.abs(((line[None, :, 0] * R(x1) + line[None, :, 1] * R(y1)) + line[None, :, 2]) / den[None, :]).astype(f32))
    with np.errstate(invalid="ignore"):
        hit = ~overlap & (np.fmax(d1, d2) < f32(t)) & (R(r) != Cc(r))
    off = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(u32)
    return off, np.nonzero(hit)[1].astype(u32)


def model_collinear(rec, scene, t, simv=None):
    """the collinear path: per-view lists (CSR over global segments), the child stream (collinear segments of a passing
    primary's target) and the own stream (those of a hypothesis's own segment) with their similarities, and the host
    pass -> dict(coll_off, coll_idx, child_*, own_*, edges, l2g)"""
    sb = np.asarray(rec["seg_base"], np.int64)
    offs, idxs = [np.zeros(1, np.int64)], []
    for v in scene.views:
        o, ix = collinear_lists(v.segs, t)
        offs.append(o[1:].astype(np.int64) + offs[-1][-1]); idxs.append(ix)
    coll_off = np.concatenate(offs).astype(u32); coll_idx = np.concatenate(idxs).astype(u32)
    ca, cb = model_candidates(rec)
    if simv is None:
        simv = model_simv(rec, ca, cb)
    hs = rec["hyp_of_seg"].astype(i32)
    hy = rec["hyps"]

    def stream(ha, g, take):
        """per item: the global segments collinear to segment g[i] and sim(ha[i], their hypotheses)"""
        base = sb[np.searchsorted(sb, g, side="right") - 1]
        cnt = np.where(take, coll_off[g + 1].astype(np.int64) - coll_off[g], 0)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(u32)
        item = np.repeat(np.arange(len(g)), cnt)
        within = np.arange(int(off[-1])) - off[item].astype(np.int64)
        seg = (base[item] + coll_idx[coll_off[g[item]].astype(np.int64) + within]).astype(u32)
        a, b = ha[item], hs[seg]
        sim = np.zeros(len(seg), f32)
        e = np.nonzero(eligible(a, b))[0]
        if len(e):
            sim[e] = model_sim(rec, a[e], b[e])
        return off, seg, sim
    with np.errstate(invalid="ignore"):
        passing = simv > MIN_AFFINITY
    child = stream(ca, rec["surv_tg"].astype(np.int64), passing)
    own_g = sb[hy["view"]] + hy["m"]["src_seg"].astype(np.int64)
    own = stream(np.arange(int(rec["H"]), dtype=i32), own_g, np.ones(int(rec["H"]), bool))
    edges, rows = model_sequential(rec, simv, child + own)
    return dict(coll_off=coll_off, coll_idx=coll_idx, child_off=child[0], child_seg=child[1], child_sim=child[2],
                own_off=own[0], own_seg=own[1], own_sim=own[2], edges=edges, l2g=l2g_of_segments(rec, rows), simv=simv)


# ---- records from the CPU oracle ------------------------------------------------------------------------------------------
def with_scene(rec, scene):
    """adds what the hook leaves to the caller: seg_base (first global segment of every view) and the views' camera ids"""
    rec["cams"] = np.array([v.cam for v in scene.views], np.int64)
    assert np.all(np.diff(rec["cams"]) > 0), "views in camera order"
    rec["seg_base"] = np.concatenate([[0], np.cumsum([len(v.segs) for v in scene.views])]).astype(np.int64)
    return rec


def records_from_oracle(o, scene, sigma_angle=10.0):
    """the `rec` dict of Line3D.affinity_records() from the CPU oracle after match_images and compute_affinity"""
    rec = with_scene({}, scene)
    cams, sb = rec["cams"], rec["seg_base"]
    vi_of = {int(c): i for i, c in enumerate(cams)}
    G, V = int(sb[-1]), len(cams)
    camseg, geo, length, m = o.best()
    key = camseg[:, 0].astype(np.int64) * (G + 1) + camseg[:, 1]
    assert np.all(np.diff(key) > 0), "best hypotheses in (camera, segment) order"
    H = len(m)
    hyps = np.zeros(H, HYP_REC_DTYPE)
    hyps["P1"], hyps["P2"], hyps["dir"] = geo[:, 0:3], geo[:, 3:6], geo[:, 6:9]
    hyps["length"] = length; hyps["valid"] = 1; hyps["m"] = m
    hyps["view"] = [vi_of[int(c)] for c in camseg[:, 0]]
    hs = np.full(G, -1, i32)
    hs[sb[hyps["view"]] + camseg[:, 1].astype(np.int64)] = np.arange(H)
    so, sg, tg = [np.zeros(1, np.int64)], [], []
    for i, v in enumerate(scene.views):
        mm, off = o.matches(v.cam)
        so.append(off[1:].astype(np.int64) + so[-1][-1])
        sg.append(sb[i] + mm["src_seg"].astype(np.int64))
        tg.append(sb[[vi_of[int(c)] for c in mm["tgt_cam"]]] + mm["tgt_seg"].astype(np.int64) if len(mm) else np.zeros(0, np.int64))
    info = [o.view_info(v.cam) for v in scene.views]
    sa = f32(min(abs(f32(sigma_angle)), f32(90)))
    N = int(so[-1][-1])
    rec.update(N=N, H=H, G=G, V=V, n_cand=N if N and H else 0, mode=0, diffused=0, two_sigA_sqr=f32(f32(2) * sa * sa),
               med_scene_depth_lines=o.med_scene_depth_lines(), msdl_dev=np.array([o.med_scene_depth_lines()], f32),
               view_k=np.array([x["k"] for x in info], f32), medians=np.array([x["median_depth"] for x in info], f32),
               hyps=hyps, surv_off=np.concatenate(so).astype(u32), surv_sg=np.concatenate(sg).astype(u32),
               surv_tg=np.concatenate(tg).astype(u32), hyp_of_seg=hs)
    return rec


# ---- what a scene holds ---------------------------------------------------------------------------------------------------
def class_counts(rec, simv=None):
    """how often every branch of the fill is taken by the records (simv = None: the model's similarities)"""
    ca, cb = model_candidates(rec)
    n, H = len(ca), int(rec["H"])
    c = dict(N=n, H=H, no_source_hyp=int((ca < 0).sum()), no_target_hyp=int((cb < 0).sum()))
    e = np.nonzero(eligible(ca, cb))[0]
    sim, d = model_sim(rec, ca[e], cb[e], details=True) if len(e) else (np.zeros(0, f32), None)
    if simv is None:
        simv = np.zeros(n, f32); simv[e] = sim
    if d is not None:
        live = ~d["short"]
        with np.errstate(invalid="ignore"):
            arg = np.where(np.isnan(d["ys"]), np.inf, d["ys"]).argmin(1)
        c.update(short=int(d["short"].sum()), folded=int(d["folded"].sum()), clamped=int(d["clamped"].sum()),
                 capped=int(d["capped"].any(1).sum()), **{f"dp_over_{t}": int(d["over"][:, i].sum()) for i, t in enumerate(TERMS[1:])},
                 **{f"min_is_{t}": int(((arg == i) & live).sum()) for i, t in enumerate(TERMS)})
    else:
        c.update(short=0, folded=0, clamped=0, capped=0, **{f"dp_over_{t}": 0 for t in TERMS[1:]}, **{f"min_is_{t}": 0 for t in TERMS})
    with np.errstate(invalid="ignore"):
        ok = simv > MIN_AFFINITY
        c["near_half_below"] = int(((simv <= MIN_AFFINITY) & (simv > f32(0.499))).sum())
        c["near_half_above"] = int((ok & (simv < f32(0.501))).sum())
    c["pass"] = int(ok.sum())
    if n and H:
        rev = reverse_index(rec)
        rev_ok = np.zeros(n, bool); rev_ok[rev >= 0] = ok[rev[rev >= 0]]
        back, fwd = ok & (cb < ca), ok & (cb > ca)
        c.update(back_rev_pass=int((back & (rev >= 0) & rev_ok).sum()), back_rev_fail=int((back & (rev >= 0) & ~rev_ok).sum()),
                 back_rev_absent=int((back & (rev < 0)).sum()), fwd_rev_present=int((fwd & (rev >= 0)).sum()),
                 fwd_rev_absent=int((fwd & (rev < 0)).sum()))
        w = run_stages(rec, simv)
        ft = w["first_touch"][w["first_touch"] != EMPTY]
        c.update(edges=w["epos_total"], rows=w["touch_total"], rows_as_id1=int((ft % 2 == 0).sum()), rows_as_id2=int((ft % 2 == 1).sum()))
    else:
        c.update(back_rev_pass=0, back_rev_fail=0, back_rev_absent=0, fwd_rev_present=0, fwd_rev_absent=0, edges=0, rows=0,
                 rows_as_id1=0, rows_as_id2=0)
    return c


def ulp_distance(a, b):
    """distance of two float32 arrays in units in the last place (NaN: equal bits count as 0)"""
    def key(x):
        i = np.asarray(x, f32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---- the scenes -----------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, build, expect=None, **params):
        self.name, self._build, self.expect, self.params = name, build, expect or {}, params

    def scene(self):
        return self._build()

    def gpu_params(self):
        return dict(self.params)

    def oracle_params(self):
        p = self.params
        return dict(sigma_p=p.get("sigma_position", 2.5), sigma_a=p.get("sigma_angle", 10.0), kNN=p.get("kNN", 10))

    def oracle(self, collinearity=None):
        """the CPU oracle after match_images and compute_affinity -> (oracle, scene)"""
        from oracle import oracle as O
        sc = self.scene()
        o = O.Oracle(threads=1)
        o.add_scene(sc)
        o.match_images(**self.oracle_params())
        if collinearity is not None:
            o.set_collinearity(collinearity)
        o.compute_affinity()
        return o, sc

    def oracle_records(self):
        o, sc = self.oracle()
        return o, sc, records_from_oracle(o, sc, self.params.get("sigma_angle", 10.0))


def cut_views(name, n_views, cuts=None):
    """the first n_views views of the C0 scene, neighbours restricted to them; cuts: {view index: segments kept}"""
    from line3dpp_amd.scene import make_config
    sc = make_config("C0")
    keep = {v.cam for v in sc.views[:n_views]}
    out = copy.copy(sc)
    out.views = []
    for i, v in enumerate(sc.views[:n_views]):
        w = copy.copy(v)
        w.neighbors = [n for n in v.neighbors if n in keep]
        assert w.neighbors, "a view without neighbours is rejected (line3D.cc:154)"
        if cuts and i in cuts:
            w.segs = v.segs[:cuts[i]].copy()
        out.views.append(w)
    out.name = name
    return out


def _ring(*a, **k):
    from line3dpp_amd.scene import make_scene
    return make_scene(*a, **k)


# Cuts of the sixth view's segment count (596 in the fixture) that put N on the launch edges of k_aff_sim (128 lanes a
# block; k_aff_flag / _touch / _emit run 256): found by a search with the CPU oracle, N % 128 == 0 and N % 128 == 1.
CUT_N_MULTIPLE_OF_128 = 529      # N = 5504 = 43 x 128
CUT_N_ONE_PAST_128 = 301        # N = 5249 = 41 x 128 + 1

# The scenes.  `expect`: what class_counts measures on the CPU oracle's records, every count of it (tests/test_affinity_cases.py
# asserts the whole dict; tests/test_gpu_affinity.py asserts N and H on the GPU so that a drift shows).  Classes that are
# 0 in every scene:
#   clamped         no pair of unit directions in these records has a float dot product above 1
#   back_rev_fail   the similarity is exactly symmetric in its two hypotheses (y_p1 and y_p2 trade places), so a reverse
#                   candidate that exists passes whenever its forward one does; reached only by the hand-set similarities
#                   of tests/test_gpu_affinity.py
#   no_source_hyp, short    the tail writes surviving matches only for segments with a best hypothesis of positive length
# back_rev_absent (a passing candidate whose target's hypothesis comes earlier and whose target's list does not hold the
# reverse: the loop of k_aff_flag ends without a hit) is 0 up to seven views of the fixture and 13 on c0_eight.
CASES = {c.name: c for c in (
    # N = 5679 crosses one 4096-element scan tile in epos and two in touch_rank (2N = 11358)
    Case("c0_six", lambda: cut_views("c0_six", 6),
         expect=dict(N=5679, H=1666, no_source_hyp=0, no_target_hyp=306, short=0, folded=613, clamped=0,
                     capped=3580, dp_over_d11=2944, dp_over_d12=2874, dp_over_d21=2975, dp_over_d22=2909,
                     min_is_angle=14, min_is_d11=1404, min_is_d12=1322, min_is_d21=1368, min_is_d22=1265,
                     near_half_below=3, near_half_above=4, back_rev_pass=2170, back_rev_fail=0, back_rev_absent=0,
                     fwd_rev_present=2170, fwd_rev_absent=47, edges=2217, rows=1553, rows_as_id1=434,
                     rows_as_id2=1119, **{"pass": 4387})),
    Case("c0_six_n128x", lambda: cut_views("c0_six_n128x", 6, {5: CUT_N_MULTIPLE_OF_128}),
         expect=dict(N=5504, H=1628, no_source_hyp=0, no_target_hyp=307, short=0, folded=603, clamped=0,
                     capped=3492, dp_over_d11=2872, dp_over_d12=2822, dp_over_d21=2898, dp_over_d22=2854,
                     min_is_angle=14, min_is_d11=1353, min_is_d12=1287, min_is_d21=1314, min_is_d22=1229,
                     near_half_below=3, near_half_above=2, back_rev_pass=2089, back_rev_fail=0, back_rev_absent=0,
                     fwd_rev_present=2089, fwd_rev_absent=48, edges=2137, rows=1511, rows_as_id1=426,
                     rows_as_id2=1085, **{"pass": 4226})),
    Case("c0_six_n128x1", lambda: cut_views("c0_six_n128x1", 6, {5: CUT_N_ONE_PAST_128}),
         expect=dict(N=5249, H=1548, no_source_hyp=0, no_target_hyp=282, short=0, folded=575, clamped=0,
                     capped=3366, dp_over_d11=2770, dp_over_d12=2739, dp_over_d21=2797, dp_over_d22=2773,
                     min_is_angle=12, min_is_d11=1289, min_is_d12=1233, min_is_d21=1252, min_is_d22=1181,
                     near_half_below=3, near_half_above=2, back_rev_pass=1995, back_rev_fail=0, back_rev_absent=0,
                     fwd_rev_present=1995, fwd_rev_absent=48, edges=2043, rows=1440, rows_as_id1=405,
                     rows_as_id2=1035, **{"pass": 4038})),
    # the first eight views: the smallest slice of the fixture in which a later hypothesis's passing candidate finds no
    # reverse in its target's list (back_rev_absent = 13; 0 with six and seven views, 75 with nine)
    Case("c0_eight", lambda: cut_views("c0_eight", 8),
         expect=dict(N=18917, H=4088, no_source_hyp=0, no_target_hyp=705, short=0, folded=4790, clamped=0,
                     capped=10065, dp_over_d11=10609, dp_over_d12=10622, dp_over_d21=10362, dp_over_d22=10349,
                     min_is_angle=16, min_is_d11=4549, min_is_d12=4622, min_is_d21=4507, min_is_d22=4518,
                     near_half_below=3, near_half_above=9, back_rev_pass=5270, back_rev_fail=0, back_rev_absent=13,
                     fwd_rev_present=5270, fwd_rev_absent=137, edges=5420, rows=3629, rows_as_id1=1348,
                     rows_as_id2=2281, **{"pass": 10690})),
    # one partial block everywhere
    Case("tiny", lambda: _ring(8, 300, n_neighbors=4, seed=1, noise_px=2.0),
         expect=dict(N=69, H=34, no_source_hyp=0, no_target_hyp=19, short=0, folded=4, clamped=0, capped=34,
                     dp_over_d11=22, dp_over_d12=25, dp_over_d21=22, dp_over_d22=25, min_is_angle=0, min_is_d11=13,
                     min_is_d12=12, min_is_d21=13, min_is_d22=12, near_half_below=0, near_half_above=0,
                     back_rev_pass=24, back_rev_fail=0, back_rev_absent=0, fwd_rev_present=24, fwd_rev_absent=0,
                     edges=24, rows=24, rows_as_id1=8, rows_as_id2=16, **{"pass": 48})),
    # N, H > 0 and every target without a hypothesis: no edge, no row
    Case("no_edges", lambda: _ring(7, 129, n_neighbors=2, seed=3),
         expect=dict(N=10, H=5, no_source_hyp=0, no_target_hyp=10, short=0, folded=0, clamped=0, capped=0,
                     dp_over_d11=0, dp_over_d12=0, dp_over_d21=0, dp_over_d22=0, min_is_angle=0, min_is_d11=0,
                     min_is_d12=0, min_is_d21=0, min_is_d22=0, near_half_below=0, near_half_above=0, back_rev_pass=0,
                     back_rev_fail=0, back_rev_absent=0, fwd_rev_present=0, fwd_rev_absent=0, edges=0, rows=0,
                     rows_as_id1=0, rows_as_id2=0, **{"pass": 0})),
    # fixed-sigma mode: k = sigma_p / med_scene_depth for every view
    Case("fixed_sigma", lambda: _ring(6, 200, n_neighbors=4, seed=17), sigma_position=-0.05,
         expect=dict(N=156, H=68, no_source_hyp=0, no_target_hyp=43, short=0, folded=2, clamped=0, capped=77,
                     dp_over_d11=65, dp_over_d12=63, dp_over_d21=69, dp_over_d22=67, min_is_angle=0, min_is_d11=26,
                     min_is_d12=31, min_is_d21=24, min_is_d22=32, near_half_below=0, near_half_above=0,
                     back_rev_pass=50, back_rev_fail=0, back_rev_absent=0, fwd_rev_present=50, fwd_rev_absent=0,
                     edges=50, rows=54, rows_as_id1=19, rows_as_id2=35, **{"pass": 100})),
    # a narrow angular term: it is the smallest of the five for 20 candidates
    Case("narrow_angle", lambda: _ring(8, 300, n_neighbors=4, seed=1), sigma_angle=2.0, kNN=2,
         expect=dict(N=310, H=155, no_source_hyp=0, no_target_hyp=18, short=0, folded=0, clamped=0, capped=240,
                     dp_over_d11=167, dp_over_d12=167, dp_over_d21=167, dp_over_d22=167, min_is_angle=20,
                     min_is_d11=68, min_is_d12=68, min_is_d21=68, min_is_d22=68, near_half_below=0,
                     near_half_above=0, back_rev_pass=144, back_rev_fail=0, back_rev_absent=0, fwd_rev_present=144,
                     fwd_rev_absent=0, edges=144, rows=147, rows_as_id1=50, rows_as_id2=97, **{"pass": 288})),
    # k_collin's grid is (max_M / 256, V): views of 256, 513, 257 and 255 segments
    Case("unequal_views", lambda: cut_views("unequal_views", 4, {0: 256, 1: 513, 2: 257, 3: 255}),
         expect=dict(N=756, H=289, no_source_hyp=0, no_target_hyp=69, short=0, folded=35, clamped=0, capped=372,
                     dp_over_d11=365, dp_over_d12=360, dp_over_d21=368, dp_over_d22=362, min_is_angle=0,
                     min_is_d11=168, min_is_d12=180, min_is_d21=163, min_is_d22=176, near_half_below=0,
                     near_half_above=0, back_rev_pass=315, back_rev_fail=0, back_rev_absent=0, fwd_rev_present=315,
                     fwd_rev_absent=17, edges=332, rows=273, rows_as_id1=84, rows_as_id2=189, **{"pass": 647})),
)}


# ---- shared, computed once per process -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """CASES[name] through the CPU oracle and the model on its records -> dict(o, scene, rec, w, edges, l2g, n_diff,
    max_ulp): the oracle's A_ and how far the model's weights are from the oracle's expf (count, largest ulp distance).
    Nobody writes to what this returns."""
    case = CASES[name]
    o, sc, rec = case.oracle_records()
    w = run_stages(rec)
    oe, ol = o.affinity()
    same = len(oe) == len(w["edges"]) and np.array_equal(oe["i"], w["edges"]["i"]) and np.array_equal(oe["j"], w["edges"]["j"])
    d = ulp_distance(oe["w"], w["edges"]["w"])[0::2] if same else None
    return dict(o=o, scene=sc, rec=rec, w=w, edges=oe, l2g=ol, same_ids=same,
                n_diff=int((d > 0).sum()) if same else None, max_ulp=int(d.max()) if same and len(d) else 0)
