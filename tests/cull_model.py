"""Host model of the epipolar-band culling of phase A (make_cull in l3d_api.hip, k_cull_prepare in k_match.hip):
a restatement of the rules in numpy fp64, not of the kernels' loops.

  * forms(F, ws, hs, wt, ht): the four linear forms As, Bs, At, Bt of tau = (A.x) / (B.x) and every rule by which a pair is
    refused (REFUSALS names them);
  * src_bands / tgt_bands: a segment's tau band, its class (0 unbounded, 1 widened by the direction term, 2 plain), the pad
    0.01 + 1e-6 |tau| and the fp32 store;
  * src_classes: the width class of a source row in the three layouts -- padded with R = 16 (tile form) or 64 (row form), and
    the unpadded keep-all layout with its steps at 4 096 and 8 192 segments;
  * layout: the padded region -- classes ascending, each from a multiple of R, tile_src_cap(Ms, R) positions;
  * chunk_hulls: the band of every 64 consecutive targets;
  * key_bits / quant_step: the resolution of the 32-bit sort keys.

Every stage takes the PREVIOUS stage's output as its input, so a test can feed it what the device dumped
(Line3D.cull_state): the dumped bands feed the classes, the classes the layout, the permuted bands the chunk hulls.  One
fp32 ulp in a band then shows as a band difference and cannot turn into a class or layout mismatch."""
import numpy as np

MIN_DEN = 0.05                 # kCullMinDen: B.x of a usable end point (B.centre == 1)
OK_MARGIN, OK_MIN = 0.05, 0.1  # make_cull: B.x >= 0.1 at the corners of the image enlarged by 5 % on every side
TILE_CLASSES, TILE_MIN_ITEMS = 5, 24
LDS_SEGS = 16384               # kCullLdsSegs: larger views sort 64-bit keys in global scratch
BAND_CACHE_SEGS = 4096         # kCullBandCacheSegs
SORT_BLOCK = 512               # at least one key per thread
EMPTY = 0xFFFFFFFF
REFUSALS = ("F_zero_or_not_finite", "no_epipole", "rank", "epipole_at_centre", "st", "ss", "target_denominator",
            "source_denominator", "not_finite")


# ---- moved from tests/test_culling_math.py (which imports them) ------------------------------------------------------------
def _fundamental(s, t):                       # Line3D::getFundamentalMatrix, line3D.cc:874-892
    R = t.R @ s.R.T
    tt = t.t - R @ s.t
    T = np.array([[0, -tt[2], tt[1]], [tt[2], 0, -tt[0]], [-tt[1], tt[0], 0]])
    return np.linalg.inv(t.K.T) @ (T @ R) @ np.linalg.inv(s.K)


def _cull_forms(F, ws, hs, wt, ht):
    """As, Bs, At, Bt of make_cull, or None where the host refuses to cull the pair"""
    cols = [F[:, j] for j in range(3)]
    e, best = None, 0.0
    for a, b in ((0, 1), (0, 2), (1, 2)):
        x = np.cross(cols[a], cols[b]); n = np.linalg.norm(x)
        if n > best:
            best, e = n, x / n
    c = np.array([0.5 * wt, 0.5 * ht, 1.0])
    m = np.array([e[0] - c[0] * e[2], e[1] - c[1] * e[2]])
    if np.linalg.norm(m) < 1e-12:
        return None
    m /= np.linalg.norm(m)
    n = np.array([-m[1], m[0], 0.0])
    At, Bt = np.cross(e, c), np.cross(n, e)
    st = Bt @ c
    At, Bt = At / st, Bt / st
    As, Bs = -(F.T @ c), F.T @ n
    ss = Bs @ np.array([0.5 * ws, 0.5 * hs, 1.0])
    As, Bs = As / ss, Bs / ss

    def ok(B, w, h):                          # one sign, with margin, over the (slightly enlarged) image
        return all(B[0] * x + B[1] * y + B[2] >= 0.1 for x in (-0.05 * w, 1.05 * w) for y in (-0.05 * h, 1.05 * h))
    return (As, Bs, At, Bt) if ok(Bt, wt, ht) and ok(Bs, ws, hs) else None


def _bands(forms, S, T):
    As, Bs, At, Bt = forms

    def tau(A, B, x, y):
        return (A[0] * x + A[1] * y + A[2]) / (B[0] * x + B[1] * y + B[2])
    S = S.astype(np.float64); T = T.astype(np.float64)
    s1, s2 = tau(As, Bs, S[:, 0], S[:, 1]), tau(As, Bs, S[:, 2], S[:, 3])
    slo, shi = np.minimum(s1, s2), np.maximum(s1, s2)
    t1, t2 = tau(At, Bt, T[:, 0], T[:, 1]), tau(At, Bt, T[:, 2], T[:, 3])
    tlo, thi = np.minimum(t1, t2), np.maximum(t1, t2)
    # widening: the pencil line parallel to the target segment (tau of its direction), when it can lie in a wedge
    dx, dy = T[:, 2] - T[:, 0], T[:, 3] - T[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        td = (At[0] * dx + At[1] * dy) / (Bt[0] * dx + Bt[1] * dy)
    inside = (td >= slo.min() - 1.0) & (td <= shi.max() + 1.0)
    tlo = np.where(inside, np.minimum(tlo, td), tlo); thi = np.where(inside, np.maximum(thi, td), thi)
    pad = lambda v: 0.01 + 1e-6 * np.abs(v)
    return slo - pad(slo), shi + pad(shi), tlo - pad(tlo), thi + pad(thi)


# ---- the forms and the refusal rules ---------------------------------------------------------------------------------------
def corner_min(B, w, h):
    """smallest B.x over the corners of the image enlarged by 5 % on every side"""
    return min(B[0] * x + B[1] * y + B[2] for x in (-OK_MARGIN * w, (1 + OK_MARGIN) * w) for y in (-OK_MARGIN * h, (1 + OK_MARGIN) * h))


def forms_ex(F, ws, hs, wt, ht):
    """(forms or None, reason or None, detail): detail holds the corner minima of Bt and Bs once they exist, so that a case
    can say how far from the flip it stands and which side decides it"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    detail = {}
    fn = np.abs(F).max()
    if not (fn > 0.0) or not np.isfinite(fn):
        return None, "F_zero_or_not_finite", detail
    cols = [F[:, j] for j in range(3)]
    e, best = None, 0.0
    for a, b in ((0, 1), (0, 2), (1, 2)):
        x = np.cross(cols[a], cols[b]); n = np.linalg.norm(x)
        if n > best:
            best, e = n, x
    if not (best > 1e-30 * fn * fn):
        return None, "no_epipole", detail
    e = e / best
    for j in range(3):                         # rank 2: every line F p passes through e
        if abs(e @ cols[j]) > 1e-10 * np.linalg.norm(cols[j]) + 1e-300:
            return None, "rank", detail
    c = np.array([0.5 * wt, 0.5 * ht, 1.0])
    m = np.array([e[0] - c[0] * e[2], e[1] - c[1] * e[2]])
    ml = np.hypot(m[0], m[1])
    if not (ml > 1e-12 * np.abs(e).sum()):
        return None, "epipole_at_centre", detail
    m = m / ml
    n = np.array([-m[1], m[0], 0.0])
    At, Bt = np.cross(e, c), np.cross(n, e)
    st = Bt @ c
    if not (abs(st) > 1e-300):
        return None, "st", detail
    At, Bt = At / st, Bt / st
    As, Bs = -(F.T @ c), F.T @ n
    ss = Bs @ np.array([0.5 * ws, 0.5 * hs, 1.0])
    if not (abs(ss) > 1e-300):
        return None, "ss", detail
    As, Bs = As / ss, Bs / ss
    detail["min_Bt"], detail["min_Bs"] = corner_min(Bt, wt, ht), corner_min(Bs, ws, hs)
    if not (detail["min_Bt"] >= OK_MIN):
        return None, "target_denominator", detail
    if not (detail["min_Bs"] >= OK_MIN):
        return None, "source_denominator", detail
    if not all(np.isfinite(v).all() for v in (As, Bs, At, Bt)):
        return None, "not_finite", detail
    return (As, Bs, At, Bt), None, detail


def forms(F, ws, hs, wt, ht):
    return forms_ex(F, ws, hs, wt, ht)[0]


def pair_forms(s, t):
    """forms_ex of the directed pair of two views (scene.ViewData)"""
    return forms_ex(_fundamental(s, t), s.width, s.height, t.width, t.height)


# ---- bands -------------------------------------------------------------------------------------------------------------------
def _den(B, x, y):
    return B[0] * x + B[1] * y + B[2]


def _store(lo, hi, cls):
    """make_band: NaN, an inverted or an overflowing interval is never culled (class 0: (-inf, +inf)); else the interval
    padded by 0.01 + 1e-6 |tau| and rounded to fp32"""
    with np.errstate(invalid="ignore", over="ignore"):
        bad = ~(lo <= hi) | ~(np.abs(lo) < 1e30) | ~(np.abs(hi) < 1e30) | (cls == 0)
        lo32 = (lo - (0.01 + 1e-6 * np.abs(lo))).astype(np.float32)
        hi32 = (hi + (0.01 + 1e-6 * np.abs(hi))).astype(np.float32)
    return (np.where(bad, np.float32(-np.inf), lo32).astype(np.float32), np.where(bad, np.float32(np.inf), hi32).astype(np.float32),
            np.where(bad, 0, cls).astype(np.int64))


def src_bands(fm, S):
    """(lo32, hi32, cls) of the source rows S [M, 4]: the wedge of the epipolar lines of the two end points"""
    As, Bs = fm[0], fm[1]
    S = np.asarray(S, np.float32).astype(np.float64)
    d1, d2 = _den(Bs, S[:, 0], S[:, 1]), _den(Bs, S[:, 2], S[:, 3])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t1, t2 = _den(As, S[:, 0], S[:, 1]) / d1, _den(As, S[:, 2], S[:, 3]) / d2
        usable = (d1 > MIN_DEN) & (d2 > MIN_DEN)
        return _store(np.fmin(t1, t2), np.fmax(t1, t2), np.where(usable, 2, 0))


def src_span(src_lo32, src_hi32):
    """the span of all bounded source wedges, as the target side reduces it from the (stored) bands: (lo, hi) or None"""
    b = np.isfinite(src_lo32)
    return (np.float32(src_lo32[b].min()), np.float32(src_hi32[b].max())) if b.any() else None


def tgt_bands(fm, T, span):
    """(lo32, hi32, cls) of the targets T [M, 4]; span: src_span of the stored source bands.  The band is widened to the
    tau of the segment's own direction where that lies within 1 of the span -- only then can a wedge contain the direction."""
    At, Bt = fm[2], fm[3]
    T = np.asarray(T, np.float32).astype(np.float64)
    d1, d2 = _den(Bt, T[:, 0], T[:, 1]), _den(Bt, T[:, 2], T[:, 3])
    dx, dy = T[:, 2] - T[:, 0], T[:, 3] - T[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t1, t2 = _den(At, T[:, 0], T[:, 1]) / d1, _den(At, T[:, 2], T[:, 3]) / d2
        lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
        td = (At[0] * dx + At[1] * dy) / (Bt[0] * dx + Bt[1] * dy)
        usable = (d1 > MIN_DEN) & (d2 > MIN_DEN) & ~np.isnan(td)      # (td NaN: a zero-length segment)
        widen = np.zeros(len(T), bool) if span is None else (td >= float(span[0]) - 1.0) & (td <= float(span[1]) + 1.0)
        lo, hi = np.where(widen, np.fmin(lo, td), lo), np.where(widen, np.fmax(hi, td), hi)
        return _store(lo, hi, np.where(usable, np.where(widen, 1, 2), 0))


def intersect(slo, shi, tlo, thi, r, q):
    """the bands of source rows r and targets q meet"""
    return (tlo[q] <= shi[r]) & (thi[q] >= slo[r])


# ---- width classes and the layout ----------------------------------------------------------------------------------------------
def tile_classes(Ms, R):
    return 2 if Ms // R < TILE_MIN_ITEMS else TILE_CLASSES


def tile_src_cap(Ms, R):
    return ((Ms + tile_classes(Ms, R) * (R - 1) + R - 1) // R) * R


def class_cuts(Ms, R, wt, ht):
    """the fp32 width cuts of the layout with R rows per item (0: the unpadded keep-all layout), widest first"""
    ref = np.float32(np.float32(0.5) * np.float32(wt) + np.float32(0.5) * np.float32(ht))
    inf = np.float32(np.inf)
    if R:
        items = Ms // R
        c16 = ref * np.float32(1 / 16) if items >= TILE_MIN_ITEMS else inf
        c32 = ref * np.float32(1 / 32) if items >= 192 else c16
        c64 = ref * np.float32(1 / 64) if items >= 48 else c16
        return c16, c32, c64
    two = Ms >= 8192
    w1 = ref * np.float32(1 / 32 if two else 1 / 16) if Ms >= 4096 else inf
    return (ref * np.float32(1 / 8) if two else inf), w1


def src_classes(lo32, hi32, Ms, R, wt, ht):
    """the width class of every source row from its STORED band: 0 unbounded; padded layout 1 (beyond 1/16 of (w + h) / 2) ..
    4 (narrow); unpadded layout 1 (beyond 1/8, from 8 192 segments), 2 (beyond 1/16, 1/32 from 8 192 segments), 3"""
    lo32, hi32 = np.asarray(lo32, np.float32), np.asarray(hi32, np.float32)
    unb = np.isneginf(lo32)
    with np.errstate(invalid="ignore"):
        w = (hi32 - lo32).astype(np.float32)
        if R:
            c16, c32, c64 = class_cuts(Ms, R, wt, ht)
            cls = np.where(w > c16, 1, np.where(w > c32, 2, np.where(w > c64, 3, 4)))
        else:
            w2, w1 = class_cuts(Ms, 0, wt, ht)
            cls = np.where(w > w1, np.where(w > w2, 1, 2), 3)
    return np.where(unb, 0, cls).astype(np.int64)


def layout(counts, Ms, R):
    """the padded region from the rows per class: (cap, base [6]) -- class k holds the positions base[k] .. base[k] +
    counts[k], everything else is padding"""
    counts = np.asarray(counts, np.int64)
    assert len(counts) == TILE_CLASSES and counts.sum() == Ms
    base = np.concatenate([[0], np.cumsum(-(-counts // R) * R)])
    cap = tile_src_cap(Ms, R)
    assert base[-1] <= cap, "tile_src_cap reserves c (R - 1) positions of padding"
    return cap, base


def position_class(counts, Ms, R):
    """class at every position of the padded region, -1: padding"""
    cap, base = layout(counts, Ms, R)
    out = np.full(cap, -1, np.int64)
    for k in range(TILE_CLASSES):
        out[base[k]:base[k] + counts[k]] = k
    return out


def chunk_hulls(tlo32, thi32):
    """[ceil(M / 64), 2]: the hull of every 64 consecutive target bands in walk order"""
    M = len(tlo32)
    n = -(-M // 64)
    lo = np.full(n * 64, np.inf, np.float32); hi = np.full(n * 64, -np.inf, np.float32)
    lo[:M], hi[:M] = tlo32, thi32
    return np.stack([lo.reshape(n, 64).min(1), hi.reshape(n, 64).max(1)], 1)


# ---- sort keys ---------------------------------------------------------------------------------------------------------------
def big_keys(Ms, Mt):
    """the pair sorts 64-bit keys (class | exact band start | element) in global scratch: one of its views is beyond the LDS"""
    return max(Ms, Mt) > LDS_SEGS


def key_bits(n):
    """element bits of a side's 32-bit key: log2 of the side's padded sort size"""
    n2 = SORT_BLOCK
    while n2 < n:
        n2 <<= 1
    return n2.bit_length() - 1


def quant_step(span_lo, span_hi, n):
    """one step of the band start's quantisation in a 32-bit key: class (3 bits) | start over [span_lo, span_hi] in
    29 - bits bits | element (bits).  0 for an empty or zero-width span (everything quantises to 0: element order)."""
    w = float(span_hi) - float(span_lo)
    return w / ((1 << (29 - key_bits(n))) - 1) if w > 0 and np.isfinite(w) else 0.0


def band_cache(n_largest):
    """the launch keeps a side's bands in LDS: decided from the largest view of the launch's culled pairs"""
    n2 = SORT_BLOCK
    while n2 < n_largest:
        n2 <<= 1
    return n2 <= BAND_CACHE_SEGS
