"""Cases of the association of 2D segments with projected 3D lines, shared by tests/test_associate_host.py
and tests/test_gpu_associate.py: generated cameras (seeded numpy.random.default_rng) and hand-built threshold cases from
integer coordinates, in which every quantity of the contract is exact."""
import numpy as np

from tests import associate_model as M

TILE, CHUNK = 256, 512                     # kAssocTile, kAssocChunk of k_associate.hip
DEFAULTS = dict(max_distance=2.5, min_cos2=M.min_cos2_of(10.0), min_overlap=0.5)

# tile and chunk edges, one camera: (M, R)
EDGE_SHAPES = [(257, 513), (1, 1025), (513, 1), (256, 512), (0, 40), (40, 0), (63, 511), (64, 1), (65, 512), (255, 513), (1, 1)]
# several cameras in one launch, in this order
MULTI_SHAPES = [(0, 40), (300, 0), (1, 1), (257, 513), (64, 512), (5, 1100), (0, 0)]


def camera_case(seed, n_seg, n_rec, width=1000, height=800, on_record=0.6, twins=0.1):
    """records like projected 3D segments in a width x height image -- a share of them `twins`, near copies of an earlier
    record, a few shorter than a pixel -- and 2D segments of which a share `on_record` lies along a record, half a pixel
    to two pixels off it, the rest anywhere; a few are points"""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n_rec, M.RECORD_DTYPE)
    if n_rec:
        a = rng.uniform([0, 0], [width, height], (n_rec, 2))
        ang = rng.uniform(0, 2 * np.pi, n_rec)
        length = rng.uniform(20, 300, n_rec)
        length[rng.random(n_rec) < 0.02] = 0.7
        b = a + length[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        for i in np.flatnonzero(rng.random(n_rec) < twins):
            if i:
                j = rng.integers(0, i)
                a[i] = a[j] + rng.uniform(-0.4, 0.4, 2); b[i] = b[j] + rng.uniform(-0.4, 0.4, 2)
        rec["x1"], rec["y1"], rec["x2"], rec["y2"] = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
        rec["inv_depth1"] = rng.uniform(0.1, 1, n_rec); rec["inv_depth2"] = rng.uniform(0.1, 1, n_rec)
        rec["line"] = rng.integers(0, max(n_rec // 3, 1), n_rec)
        rec["segment"] = np.arange(n_rec, dtype=np.uint32) | (rng.integers(0, 4, n_rec).astype(np.uint32) << np.uint32(30))
    segs = np.zeros((n_seg, 4), np.float32)
    if n_seg:
        p = rng.uniform([0, 0], [width, height], (n_seg, 2))
        ang = rng.uniform(0, 2 * np.pi, n_seg)
        q = p + rng.uniform(5, 200, n_seg)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        if n_rec:
            on = np.flatnonzero(rng.random(n_seg) < on_record)
            j = rng.integers(0, n_rec, len(on))
            a = np.stack([rec["x1"][j], rec["y1"][j]], 1).astype(np.float64)
            d = np.stack([rec["x2"][j], rec["y2"][j]], 1).astype(np.float64) - a
            nrm = np.stack([-d[:, 1], d[:, 0]], 1) / np.maximum(np.hypot(d[:, 0], d[:, 1]), 1e-9)[:, None]
            t1 = rng.uniform(-0.3, 0.7, len(on)); t2 = t1 + rng.uniform(0.2, 0.6, len(on))
            p[on] = a + t1[:, None] * d + rng.uniform(-2.0, 2.0, len(on))[:, None] * nrm
            q[on] = a + t2[:, None] * d + rng.uniform(-2.0, 2.0, len(on))[:, None] * nrm
        swap = rng.random(n_seg) < 0.5
        p[swap], q[swap] = q[swap].copy(), p[swap].copy()
        q[rng.random(n_seg) < 0.01] = np.nan                      # (marked: made a point below)
        segs[:, 0:2] = p; segs[:, 2:4] = q
        point = np.isnan(segs[:, 2])
        segs[point, 2:4] = segs[point, 0:2]
    return rec, segs


def cameras(shapes, seed):
    both = [camera_case(seed + 31 * k, m, r) for k, (m, r) in enumerate(shapes)]
    return [b[0] for b in both], [b[1] for b in both]


def large_case():
    """past one grid of tiles' worth of chunks: 20 000 segments against 3 000 records, and a second, small camera"""
    return cameras([(20000, 3000), (100, 100)], seed=2024)


def records(geometry, lines=None):
    rec = np.zeros(len(geometry), M.RECORD_DTYPE)
    g = np.asarray(geometry, np.float32).reshape(-1, 4)
    rec["x1"], rec["y1"], rec["x2"], rec["y2"] = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    rec["inv_depth1"] = 0.5; rec["inv_depth2"] = 0.25
    rec["line"] = np.arange(len(g)) + 100 if lines is None else lines
    rec["segment"] = np.arange(len(g), dtype=np.uint32) | np.uint32(0x80000000)
    return rec


def hand_cases():
    """-> list of (name, records, segments float32 [M, 4], params, expected): expected = one tuple per segment, (record,
    line, n_accepted, distance, overlap) or None where nothing is assigned"""
    out = []
    base = dict(DEFAULTS)
    # the same geometry at indices 3 and 600, other lines far away: the tie crosses a chunk, the smaller index wins
    geo = [(0, 5000 + 10 * i, 100, 5000 + 10 * i) for i in range(700)]
    geo[3] = (0, 0, 100, 0); geo[600] = (0, 0, 100, 0)
    lines = np.arange(700) + 100
    lines[3] = 7; lines[600] = 9
    out.append(("tie across a chunk", records(geo, lines), [(10, 1, 60, 1)], base, [(3, 7, 2, 1.0, 1.0)]))
    long = records([(0, 0, 100, 0)])
    above = float(np.nextafter(np.float32(2.5), np.float32(np.inf)))
    out.append(("distance exactly max_distance", long, [(20, 1, 80, 2.5)], base, [(0, 100, 1, 2.5, 1.0)]))
    out.append(("distance one step beyond", long, [(20, 1, 80, above)], base, [None]))
    out.append(("overlap exactly min_overlap", long, [(50, 1, 150, 1)], base, [(0, 100, 1, 1.0, 0.5)]))
    out.append(("overlap one step below", long, [(50, 1, 151, 1)], base, [None]))
    wide = dict(max_distance=5.0, min_cos2=0.5, min_overlap=0.5)
    out.append(("angle exactly at min_cos2", records([(0, 0, 4, 0)]), [(0, 0, 3, 3)], wide, [(0, 100, 1, 3.0, 1.0)]))
    out.append(("angle one step beyond", records([(0, 0, 4, 0)]), [(0, 0, 3, 4)], wide, [None]))
    out.append(("a record of exactly one pixel is used", records([(0, 0, 1, 0)]), [(0, 0, 1, 0)], base, [(0, 100, 1, 0.0, 1.0)]))
    out.append(("a record of 0.9 pixels is ignored", records([(0, 0, 0.9, 0)]), [(0, 0, 0.9, 0)], base, [None]))
    out.append(("a point gets nothing", long, [(5, 0, 5, 0)], base, [None]))
    out.append(("reversed segment, reversed record", records([(0, 0, 100, 0), (100, 300, 0, 300)]),
                [(10, 1, 60, 2), (60, 2, 10, 1), (10, 301, 60, 302), (60, 302, 10, 301)], base,
                [(0, 100, 1, 2.0, 1.0), (0, 100, 1, 2.0, 1.0), (1, 101, 1, 2.0, 1.0), (1, 101, 1, 2.0, 1.0)]))
    return [(n, r, np.asarray(s, np.float32).reshape(-1, 4), p, e) for n, r, s, p, e in out]


# The sanity property of the context form on the golden scene: of the (line, residual) pairs of the reconstruction, the
# share assigned to their own line, and none to another.  On the lines the reference's own code reconstructs the model
# gives 273 of 275 and 0 (tests/test_associate_reference.py recomputes that on the CPU).
SANITY_MIN_OWN_SHARE = 0.95
REFERENCE_PAIRS, REFERENCE_OWN, REFERENCE_OTHER = 275, 273, 0


def residual_ownership(lines, assoc_of_cam):
    """lines: get3Dlines() (line i = index in the records' `line`); assoc_of_cam[camID] = the associations of the view's
    segments -> (pairs, assigned to their own line, to another line, to none, the pairs on another line)"""
    pairs = own = none = 0
    other = []
    for i, L in enumerate(lines):
        for res in L["residuals"]:
            cam, seg = (int(res["cam"]), int(res["seg"])) if getattr(res, "dtype", None) is not None and res.dtype.names else (int(res[0]), int(res[1]))
            pairs += 1
            a = assoc_of_cam[cam][seg]
            if a["record"] < 0:
                none += 1
            elif int(a["line"]) == i:
                own += 1
            else:
                other.append((i, cam, seg, int(a["line"]), float(a["distance"])))
    return pairs, own, len(other), none, other


def check_expected(name, got, rec, expected):
    assert len(got) == len(expected), name
    for s, e in enumerate(expected):
        g = got[s]
        if e is None:
            assert (g["record"], g["line"], g["segment"], g["distance"], g["overlap"], g["n_accepted"]) == (-1, M.NONE, M.NONE, 0.0, 0.0, 0), \
                f"{name}: segment {s} should get nothing, got {g}"
        else:
            want = (e[0], e[1], int(rec["segment"][e[0]]) & M.SEGMENT_MASK, np.float32(e[3]), np.float32(e[4]), e[2])
            assert (g["record"], g["line"], g["segment"], g["distance"], g["overlap"], g["n_accepted"]) == want, \
                f"{name}: segment {s}: {g} != {want}"


def same_associations(got, want, what):
    assert got.dtype == M.ASSOCIATION_DTYPE and len(got) == len(want), f"{what}: {len(got)} results for {len(want)} segments"
    for name in M.ASSOCIATION_DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{what}: {name} differs in {len(bad)} segments, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
