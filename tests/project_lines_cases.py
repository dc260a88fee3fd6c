"""Inputs shared by the tests of the projection stages: the cameras and 3D segments that take every branch of
stage 1, the records that take every branch of stage 2, and the sanity property of the context forms."""
import functools

import numpy as np

from tests import project_lines_model as M


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def stage1_cameras():
    """four cameras; the first looks down +z from the origin with a plain K, so that pixels of hand-made segments are
    exact; the third has skew, K[8] != 1 and width != height"""
    cams = [dict(K=np.array([[100.0, 0, 64], [0, 100.0, 48], [0, 0, 1]]), R=np.eye(3), t=np.zeros(3), width=129, height=97)]
    cams.append(dict(K=np.array([[310.5, 0, 99.25], [0, 305.25, 37.5], [0, 0, 1]]), R=rot(0.1, -0.2, 0.05),
                     t=np.array([0.3, -0.1, 0.5]), width=200, height=75))
    cams.append(dict(K=np.array([[250.0, 1.75, 48.5], [0, 260.0, 30.25], [0, 0, 1]]) * 1.25, R=rot(-0.3, 0.4, 1.0),
                     t=np.array([-0.2, 0.4, 1.0]), width=97, height=61))
    cams.append(dict(K=np.array([[80.0, 0, 32], [0, 80.0, 32], [0, 0, 1]]), R=rot(3.0, 0.1, -0.4), t=np.array([0.1, 0.2, 6.0]),
                     width=64, height=64))
    return cams


def unproject0(x, y, z):
    """the point of camera 0 (K = [100 0 64; 0 100 48], R = I, t = 0) at pixel (x, y) and depth z"""
    return [(x - 64.0) / 100.0 * z, (y - 48.0) / 100.0 * z, z]


def stage1_segments():
    """197 segments (not a multiple of 64): hand-made ones for every branch in camera 0 (129 x 97: x in [0, 128],
    y in [0, 96]), the rest random around the cameras -> (P1 [197, 3], P2 [197, 3], line_of_segment [197])"""
    px = []      # (x1, y1, z1, x2, y2, z2) in pixels / depth of camera 0
    px.append((10, 10, 2, 100, 80, 3))            # fully inside
    px.append((-20, 30, 2, 50, 40, 2))            # across the left edge
    px.append((100, 30, 2, 150, 50, 2.5))         # right
    px.append((40, -15, 2, 60, 20, 2))            # top
    px.append((40, 80, 2, 45, 120, 2))            # bottom
    px.append((-10, 12, 2, 12, -8, 2))            # across the top-left corner region (cuts two edges)
    px.append((120, 90, 2, 140, 110, 2))          # across the bottom-right corner
    px.append((-30, 10, 2, -5, 60, 2))            # outside, left
    px.append((140, 10, 2, 160, 60, 2))           # outside, right
    px.append((10, -30, 2, 60, -5, 2))            # outside, above
    px.append((10, 100, 2, 60, 130, 2))           # outside, below
    px.append((0, 10, 2, 0, 50, 2))               # parallel to the left edge ON it (zero direction, q == 0)
    px.append((1, 10, 2, 1, 50, 2))               # one pixel inside
    px.append((-1, 10, 2, -1, 50, 2))             # one pixel outside
    px.append((10, 96, 2, 90, 96, 2))             # on the bottom edge
    px.append((10, 95, 2, 90, 95, 2))
    px.append((10, 97, 2, 90, 97, 2))
    px.append((128, 20, 2, 60, 40, 2))            # an end point exactly on the right border
    px.append((30, 0, 2, 50, 70, 4))              # ... on the top border
    px.append((50, 50, 2, 50, 50, 2))             # zero length, inside
    px.append((-50, 50, 2, -50, 50, 2))           # zero length, outside
    px.append((-40, -40, 2, 200, 160, 2))         # through the whole image: both ends clipped
    P1 = [unproject0(*p[:3]) for p in px]
    P2 = [unproject0(*p[3:]) for p in px]
    # behind camera 0, and across its near plane from either end
    P1 += [[0.1, 0.1, -1.0], [0.1, 0.0, -0.5], [0.2, 0.1, 2.0], [0.0, 0.0, 1e-7]]
    P2 += [[0.3, -0.2, -3.0], [0.2, 0.1, 2.0], [-0.1, 0.3, -1.5], [0.1, 0.1, 1.0]]
    rng = np.random.default_rng(20261018)
    n = 197 - len(P1)
    c = rng.uniform(-1.5, 1.5, (n, 3)) + [0, 0, 2.0]
    d = rng.normal(size=(n, 3)) * rng.uniform(0.05, 2.0, (n, 1))
    P1 = np.concatenate([np.array(P1, np.float64), c - d])
    P2 = np.concatenate([np.array(P2, np.float64), c + d])
    line = (np.arange(197) * 7 // 3).astype(np.uint32)
    assert len(P1) == 197
    return P1, P2, line


def rec(x1, y1, x2, y2, z1, z2, line, segment=0):
    return (x1, y1, x2, y2, z1, z2, line, segment)


def stage2_records(width, height, seed):
    """records for a width x height image: every kind of line of the contract, then 300 random ones"""
    w1, h1 = width - 1, height - 1
    r = [
        rec(3, 5, 40, 5, 0.5, 0.25, 0), rec(40, 7, 3, 7, 0.5, 0.25, 1),                    # horizontal, both directions
        rec(6, 10, 6, 50, 0.3, 0.6, 2), rec(8, 50, 8, 10, 0.3, 0.6, 3),                    # vertical
        rec(10, 10, 40, 40, 0.4, 0.4, 4), rec(45, 40, 15, 10, 0.4, 0.2, 5),                # exactly 45 degrees: x-major
        rec(50, 12, 20, 42, 0.4, 0.2, 6),                                                  # -45 degrees
        rec(2.25, 20.5, 60.75, 27.25, 0.7, 0.1, 7), rec(60.5, 30.25, 2.5, 24.75, 0.7, 0.1, 8),   # shallow
        rec(70.5, 2.25, 76.25, 58.5, 0.2, 0.9, 9), rec(80.25, 58.75, 74.5, 1.5, 0.2, 0.9, 10),   # steep
        rec(1.5, 1.25, w1 - 0.5, h1 - 1.75, 0.05, 0.95, 11),                               # longer than 128 steps at width 200
        rec(12, 55, 30, 57, 1.0, 1.0, 12),                                                 # integer end points: both drawn
        rec(20.25, 33.25, 20.75, 33.5, 1.0, 1.0, 13),                                      # sub-pixel: nothing drawn
        rec(33.5, 44.5, 33.5, 44.5, 1.0, 1.0, 14),                                         # zero length
        rec(5, 45, 60, 52, 0.5, 0.5, 15), rec(30, 38, 36, 59, 0.8, 0.8, 16),               # crossing, 16 is nearer
        rec(62, 3, 90, 3, 0.5, 0.5, 18), rec(70, 3, 96, 3, 0.5, 0.5, 17),                  # overlapping at equal depth: 17
        rec(2, 0, w1 - 2, 0, 0.6, 0.6, 19), rec(w1, 3, w1, h1 - 3, 0.6, 0.6, 20),          # along the borders
        rec(2, h1, w1 - 2, h1 - 0.25, 0.6, 0.6, 21), rec(0, 4, 0.4, h1 - 4, 0.6, 0.6, 22),
    ]
    rng = np.random.default_rng(seed)
    for k in range(300):
        c = rng.uniform([0, 0], [w1, h1])
        d = rng.normal(size=2) * rng.choice([0.4, 3.0, 12.0, 40.0])
        a, b = np.clip(c - d, 0, [w1, h1]), np.clip(c + d, 0, [w1, h1])
        z = rng.choice([0.125, 0.25, 0.5, 1.0], 2) if k % 3 == 0 else rng.uniform(0.05, 2.0, 2)
        r.append(rec(a[0], a[1], b[0], b[1], z[0], z[1], 23 + k % 41, k))
    return np.array(r, M.RECORD_DTYPE)


def stage2_multi_camera():
    """three cameras of different sizes with records and a fourth without -> (cameras, one record array per camera)"""
    sizes = [(200, 75), (97, 61), (33, 130)]
    cams = [dict(K=np.eye(3), R=np.eye(3), t=np.zeros(3), width=w, height=h) for w, h in sizes]
    recs = [stage2_records(200, 75, 5), stage2_records(97, 61, 6), stage2_records(97, 61, 7)[23:]]
    recs[2]["x1"] *= 0.3; recs[2]["x2"] *= 0.3; recs[2]["y1"] *= 2.1; recs[2]["y2"] *= 2.1
    recs.append(recs[0][:0])                                       # a camera without records
    cams.append(dict(cams[1]))
    return cams, recs


# ---- the large cases: past one scan tile (4096 elements) and past one grid (2048 blocks of 256 lanes) -------------------
STAGE1_LARGE_EMPTY = (0, 33, 69)


@functools.lru_cache(maxsize=None)
def stage1_large():
    """70 cameras x 4001 segments = 280 070 visibility flags: 69 scan tiles of 4096, so the compaction reads offsets of
    tiles whose look-back needs a second window of 64 predecessors (tile index 65 and up); 4001 is no multiple of 256 or
    4096, so cameras begin inside blocks and tiles.  The cameras cycle through the four of stage1_cameras() with t
    perturbed by N(0, 0.05); cameras 0, 33 and 69 look away from the scene and see nothing (an empty camera at the front,
    in the middle and at the end of a group).  Segments: the random recipe of stage1_segments(), seed 20261019.
    The model gives (tests assert the conditions, not the figures): STAGE1_LARGE_FIGURES below.
    -> (cameras, P1 [4001, 3], P2 [4001, 3], line_of_segment [4001]); shared between tests, not to be modified"""
    rng = np.random.default_rng(20261019)
    n = 4001
    c = rng.uniform(-1.5, 1.5, (n, 3)) + [0, 0, 2.0]
    d = rng.normal(size=(n, 3)) * rng.uniform(0.05, 2.0, (n, 1))
    P1, P2 = c - d, c + d
    line = (np.arange(n) * 7 // 3).astype(np.uint32)
    base = stage1_cameras()
    cams = []
    for k in range(70):
        cam = dict(base[k % 4])
        cam["t"] = np.asarray(cam["t"], np.float64) + rng.normal(0.0, 0.05, 3)
        if k in STAGE1_LARGE_EMPTY:
            cam["R"] = rot(np.pi, 0, 0) @ np.asarray(cam["R"], np.float64)
            cam["t"] = np.array([0.0, 0.0, -10.0])
        cams.append(cam)
    for a in (P1, P2, line):
        a.setflags(write=False)
    return cams, P1, P2, line


# what tests/project_lines_model_vec.py gives for stage1_large() (CPU): visible share of the 280 070 (camera, segment)
# pairs, fewest and most records of a camera that is not empty, records with each clip flag
STAGE1_LARGE_FIGURES = dict(visible_share=0.5521, min_records=762, max_records=3812, clipped_near=10414, clipped_rect=120249)


def stage2_large_records(width, height, n, seed):
    """n records for a width x height image: centres uniform in the image, half-lengths N(0, 1)^2 * one of 0.4 / 3 / 40 /
    300 pixels, clipped to the image and rounded to float32; every third record has inverse depths from {1/8, 1/4, 1/2, 1}
    so that equal depths meet; line ids k % 997.  Records 0, n/2 - 1 .. n/2 + 1 and n - 1 are shorter than a pixel and lie
    between integer coordinates (no step: a record without steps first, last and in a run of three); records 10 and 11
    cross at (x, y) = (0.4 w, 0.5 h) at the same depth, nearer than every random record."""
    w1, h1 = width - 1, height - 1
    rng = np.random.default_rng(seed)
    r = []
    for k in range(n):
        c = rng.uniform([0, 0], [w1, h1])
        d = rng.normal(size=2) * rng.choice([0.4, 3.0, 40.0, 300.0])
        a, b = np.clip(c - d, 0, [w1, h1]), np.clip(c + d, 0, [w1, h1])
        z = rng.choice([0.125, 0.25, 0.5, 1.0], 2) if k % 3 == 0 else rng.uniform(0.05, 2.0, 2)
        r.append(rec(a[0], a[1], b[0], b[1], z[0], z[1], k % 997, k))
    for k in (0, n // 2 - 1, n // 2, n // 2 + 1, n - 1):
        x, y = float(int(0.3 * w1)) + 0.25, float(int(0.7 * h1)) + 0.25
        r[k] = rec(x, y, x + 0.5, y + 0.25, 1.0, 1.0, k % 997, k)
    cx, cy = float(int(0.4 * width)), float(int(0.5 * height))
    r[10] = rec(cx - 0.25 * cy, cy, cx + 0.25 * cy, cy, 4.0, 4.0, 10, 10)
    r[11] = rec(cx, 0.5 * cy, cx, 1.5 * cy, 4.0, 4.0, 11, 11)
    return np.array(r, M.RECORD_DTYPE)


@functools.lru_cache(maxsize=None)
def stage2_large(seed=7):
    """Three cameras in one call: 33 x 130 WITHOUT records (a leading empty camera: two cameras share rec0 = 0), 1100 x 500
    with 6000 records of stage2_large_records (550 000 pixels: the per-pixel kernels stride past their 2048 x 256 lanes;
    two scan tiles of records; more than 524 288 major-axis steps: the work-item loop strides), 97 x 61 with
    stage2_records(97, 61, seed).  The model gives: STAGE2_LARGE_FIGURES below.
    -> (cameras, one record array per camera); shared between tests, not to be modified"""
    sizes = [(33, 130), (1100, 500), (97, 61)]
    cams = [dict(K=np.eye(3), R=np.eye(3), t=np.zeros(3), width=w, height=h) for w, h in sizes]
    recs = [np.zeros(0, M.RECORD_DTYPE), stage2_large_records(1100, 500, 6000, seed), stage2_records(97, 61, seed)]
    for a in recs:
        a.setflags(write=False)
    return cams, recs


# what the model gives for the 1100 x 500 camera of stage2_large(7) (CPU): major-axis steps, records without steps, the
# longest run of them, the longest record, pixels where the winner ties in depth with another line (thickness 1)
STAGE2_LARGE_FIGURES = dict(steps=854157, zero_step_records=384, longest_zero_run=4, longest_record=1100, tie_pixels=353)


# The sanity property of the context forms on the golden scene, taken on the CPU first
# (tests/test_project_reference.py recomputes both figures): the numpy model on the final lines the reference's own code
# (oracle/_ref) reconstructs from the scene sees the line of every one of the 275 (line, residual) pairs in the
# residual's camera (100 %; the condition is 95 %), and the residual segments' end points lie at a median of 0.15255 px
# from the projected infinite line.  The bound on the GPU pipeline's lines is twice that: its lines agree with the
# reference's to 1e-4 of the scene extent, not exactly.
SANITY_CPU_MEDIAN_PX = 0.15255
SANITY_MIN_VISIBLE = 0.95
SANITY_MAX_MEDIAN_PX = 2 * SANITY_CPU_MEDIAN_PX


def residual_sanity(lines, records_per_cam, cam_ids, segs_of_cam):
    """The sanity property of the context forms.  lines: get3Dlines() (line i = index in the records' `line`);
    records_per_cam[k]: the records of camera cam_ids[k]; segs_of_cam[cam]: the view's 2D segments [M, 4].
    -> (fraction of (line, residual (camID, segID)) pairs whose line is visible in camID, median distance in pixels of
    the residual segments' end points from the projected infinite line)"""
    first = {}
    for k, cam in enumerate(cam_ids):
        for r in records_per_cam[k]:
            first.setdefault((cam, int(r["line"])), r)
    seen, total, dist = 0, 0, []
    for i, L in enumerate(lines):
        for res in L["residuals"]:
            cam, seg = (int(res["cam"]), int(res["seg"])) if getattr(res, "dtype", None) is not None and res.dtype.names else (int(res[0]), int(res[1]))
            total += 1
            r = first.get((cam, i))
            if r is None:
                continue
            seen += 1
            a = np.array([r["x1"], r["y1"]], np.float64); b = np.array([r["x2"], r["y2"]], np.float64)
            d = b - a
            nrm = np.hypot(*d)
            if nrm == 0:
                continue
            s = np.asarray(segs_of_cam[cam], np.float64)[seg]
            for p in (s[:2], s[2:]):
                dist.append(abs(d[0] * (p[1] - a[1]) - d[1] * (p[0] - a[0])) / nrm)
    return seen / max(total, 1), float(np.median(dist)) if dist else float("nan")
