"""Host model of the launch forms of phase A's bounded-kNN kernel (DESIGN §5.1, table "launch tiers") and the scenes of
tests/test_gpu_match_forms.py.  A restatement of the design, not of the library's code: tests/test_match_cases.py holds
it against the library's own plan (l3d_match_plan, l3d_match_tile_rows) on the CPU.

  * a call is in the TILE form (16 rows per work item) when its estimated row-form items -- half the sum over the views
    of (visual neighbours x ceil(segments / 64)), rounded up -- are at most 2 048, else in the ROW form (64 rows);
  * a pair with Ms source rows has ceil((Ms + c (R - 1)) / R) work items of R rows: its rows are laid out in c width
    classes, each padded to a multiple of R; c = 2 while Ms / R < 24, else 5;
  * a row-form LAUNCH of n items (any range of the pair list) has two waves per item up to 16 384 items -- with the source
    rows cached in LDS and the items ordered by k_order_items from 3 585 on -- and one wave per item beyond;
  * the LDS of a work item: candidate rings (per wave 256 + 128 entries of 4 B; 128 + 128 with one wave), per row the
    K-th-best overlap and a claim word (4 B each), count and worst position (one index each) and the top-K table (K
    overlaps of 4 B, K indices); an index has 2 B while every target view of the launch has fewer than 65 536 segments,
    else 4 B; the row cache adds 52 B per row, the tile form's FIFO 128 x 20 B.  160 KiB is the limit.
"""
import copy
import functools

import numpy as np

from line3dpp_amd.scene import Scene, make_scene

ROWS, TILE_ROWS = 64, 16
TILE_MAX_EST_ITEMS = 2048
ORDER_MIN_ITEMS, ORDER_MAX_ITEMS = 3584, 16384       # the ordering tier is (ORDER_MIN_ITEMS, ORDER_MAX_ITEMS]
ITEM_EDGES = (TILE_MAX_EST_ITEMS + 1, ORDER_MIN_ITEMS, ORDER_MIN_ITEMS + 1, ORDER_MAX_ITEMS, ORDER_MAX_ITEMS + 1)
LDS_LIMIT = 160 * 1024
TIERS = ("tile", "row2", "row2_cached", "row1")      # numbered as l3d_match_plan_info.tier
TIER_COUNTERS = {"tile": "match_tile_launches", "row2": "match_row2_launches", "row2_cached": "match_row2_cached_launches",
                 "row1": "match_row1_launches"}
COUNTERS = tuple(TIER_COUNTERS.values()) + ("match_ix32_launches", "match_order_launches", "knn_replay_calls")


# ---- the model ---------------------------------------------------------------------------------------------------------
def pair_list(scene):
    """the directed pairs of a call in pair order: [(source cam, target cam)]"""
    return scene.pair_tests()[1]


def est_items(scene):
    cams = {v.cam for v in scene.views}
    total = sum(len(set(v.neighbors) & (cams - {v.cam})) * -(-len(v.segs) // ROWS) for v in scene.views)
    return (total + 1) // 2


def call_rows(scene):
    """rows per work item of the scene's bounded-kNN call"""
    e = est_items(scene)
    return TILE_ROWS if 0 < e <= TILE_MAX_EST_ITEMS else ROWS


def items_per_pair(Ms, rows):
    classes = 2 if Ms // rows < 24 else 5
    return -(-(Ms + classes * (rows - 1)) // rows)


def pair_items(scene, rows=None):
    """work items of every pair of the call, in pair order"""
    rows = rows or call_rows(scene)
    M = {v.cam: len(v.segs) for v in scene.views}
    return np.array([items_per_pair(M[s], rows) for s, _ in pair_list(scene)], np.int64)


def tier(n_items, rows=ROWS):
    if rows == TILE_ROWS:
        return "tile"
    return "row2" if n_items <= ORDER_MIN_ITEMS else "row2_cached" if n_items <= ORDER_MAX_ITEMS else "row1"


def lds_bytes(tier_name, K, ix16=True):
    ib = 2 if ix16 else 4
    rows = TILE_ROWS if tier_name == "tile" else ROWS
    waves = 2 if tier_name in ("row2", "row2_cached") else 1
    rings = waves * ((256 if waves == 2 else 128) + 128) * 4
    extra = 128 * 20 if tier_name == "tile" else rows * 52 if tier_name == "row2_cached" else 0
    return extra + rings + rows * (4 + 4 + ib + ib) + rows * K * (4 + ib)


def max_k(tier_name, ix16=True):
    """the largest K whose tables fit the LDS in that tier"""
    K = (LDS_LIMIT - lds_bytes(tier_name, 0, ix16)) // ((TILE_ROWS if tier_name == "tile" else ROWS) * (6 if ix16 else 8))
    assert lds_bytes(tier_name, K, ix16) <= LDS_LIMIT < lds_bytes(tier_name, K + 1, ix16)
    return K


def reachable_tiers(total_items, rows=ROWS):
    """tiers a launch of at most total_items items can take"""
    if rows == TILE_ROWS:
        return ["tile"]
    return [t for t, lo in (("row2", 1), ("row2_cached", ORDER_MIN_ITEMS + 1), ("row1", ORDER_MAX_ITEMS + 1)) if total_items >= lo]


def replays(total_items, K, rows=ROWS, ix16=True):
    """l3d_match_begin sends every row through the exact replay when SOME launch of the call could not hold its tables"""
    return any(K > max_k(t, ix16) for t in reachable_tiers(total_items, rows))


def splits_for(items, targets):
    """{target item count: (c, which)}: a split of the pair list into [0, c) and [c, P) whose first (which = 0) or second
    (which = 1) launch has exactly that many items.  Prefix sums move in steps of a pair's three or four items, so two
    neighbouring counts are never both prefixes: the remainder of the list supplies the other."""
    cum = np.concatenate([[0], np.cumsum(items)])
    total = int(cum[-1])
    out = {}
    for n in targets:
        hit = np.nonzero(cum == n)[0]
        if len(hit) and 0 < hit[0] < len(items):
            out[n] = (int(hit[0]), 0)
            continue
        hit = np.nonzero(total - cum == n)[0]
        if len(hit) and 0 < hit[0] < len(items):
            out[n] = (int(hit[0]), 1)
    return out


PARTIAL_TARGETS = (ORDER_MIN_ITEMS, ORDER_MIN_ITEMS + 1, ORDER_MAX_ITEMS, ORDER_MAX_ITEMS + 1)


def partial_splits(items):
    """the splits of the partial-launch test: {label: (c, which)} -- one per edge of PARTIAL_TARGETS (a launch of exactly
    that many items) and, per row tier, one whose first launch has an item count that is no multiple of 8"""
    out = {str(n): cw for n, cw in splits_for(items, PARTIAL_TARGETS).items()}
    cum = np.cumsum(items)
    for name in TIERS[1:]:
        hit = [c for c in range(1, len(items)) if tier(int(cum[c - 1])) == name and cum[c - 1] % 8 and cum[c - 1] not in PARTIAL_TARGETS]
        if hit:
            out["odd " + name] = (hit[len(hit) // 2], 0)
    return out


def split_items(items, c):
    """items of the two launches [0, c) and [c, P)"""
    return int(np.sum(items[:c])), int(np.sum(items[c:]))


def mixed_split(items, second=9001):
    """first pair of the second launch of the mixed scene: the shortest tail of the list with at least `second` items"""
    tail = np.cumsum(items[::-1])
    return len(items) - 1 - int(np.nonzero(tail >= second)[0][0])


# ---- counters ------------------------------------------------------------------------------------------------------------
def read_counters():
    from line3dpp_amd import _lib
    L = _lib.load()
    out = {k: int(L.l3d_debug_counter(k.encode())) for k in COUNTERS}
    assert all(v != 2**64 - 1 for v in out.values()), "l3d_debug_counter does not know a match counter"
    return out


def counters_since(before):
    now = read_counters()
    return {k: now[k] - before[k] for k in COUNTERS}


def plan(total_items, launch_items, K, max_target=1000, tile_rows=0):
    """the library's own plan of a launch (l3d_match_plan; host only)"""
    import ctypes as C
    from line3dpp_amd import _lib
    info = _lib.MatchPlanInfo()
    rc = _lib.load().l3d_match_plan(int(total_items), int(launch_items), int(K), int(max_target), int(tile_rows), C.byref(info))
    assert rc == 0, (rc, _lib.last_error())
    return dict(tier=TIERS[info.tier], lds=int(info.lds_bytes), replay=bool(info.replay), accepted=bool(info.launch_accepted),
                ix16=bool(info.ix16), waves=int(info.waves), row_cache=bool(info.row_cache))


# ---- the scenes ----------------------------------------------------------------------------------------------------------
def _with_views(scene, views, name):
    out = Scene(sorted(views, key=lambda v: v.cam), name)
    return out


def _forward_view(cam, seed, n_views, n_segs, of_cam=0):
    """view `of_cam` of the ring moved three units along its optical axis: the epipoles of the pair lie inside both images,
    the geometry the epipolar-band culling refuses (the pair streams unculled)"""
    v = copy.copy(make_scene(n_views, n_segs, n_neighbors=2, seed=seed, radius=22.0, max_views=of_cam + 1).views[of_cam])
    v.cam = cam
    v.neighbors = [of_cam]
    return v


# (a) more than 16 385 row-form items from many small pairs: 190 ring views with 60 neighbours each, 64 segments (three
# items per pair) except the views of PARTIAL_BIG (130 segments: four), which move the prefix sums of the item counts
# through every residue; view 190 sits in front of view 0
PARTIAL_VIEWS, PARTIAL_NEIGHBORS, PARTIAL_SEED = 190, 60, 7
PARTIAL_BIG = (6, 19, 40, 47, 60, 65, 72, 76, 126, 157)


@functools.lru_cache(maxsize=None)
def partial_scene():
    sc = make_scene(PARTIAL_VIEWS, 130, n_neighbors=PARTIAL_NEIGHBORS, seed=PARTIAL_SEED, real_fraction=0.9)
    views = []
    for v in sc.views:
        v.segs = v.segs[:130 if v.cam in PARTIAL_BIG else 64].copy()
        views.append(v)
    f = _forward_view(PARTIAL_VIEWS, PARTIAL_SEED, PARTIAL_VIEWS, 130)
    f.segs = f.segs[:64].copy()
    views[0].neighbors = sorted(views[0].neighbors + [f.cam])
    return _with_views(sc, views + [f], "partial190")


# (b) the hand-over between the tile and the row form: 128 ring views x 64 segments x 32 neighbours = 2 048 estimated items;
# one more (one-sided) neighbour of view 0 makes it 2 049
@functools.lru_cache(maxsize=None)
def handover_scene(extra_neighbor):
    sc = make_scene(128, 64, n_neighbors=32, seed=11, real_fraction=0.9)
    if extra_neighbor:
        sc.views[0].neighbors = sorted(sc.views[0].neighbors + [64])
        sc.name += "+1"
    return sc


# (c) the scene of (a) plus three views of 4 200 segments that neighbour each other: their pairs come last in the list
MIXED_BIG_SEGS = 4200


@functools.lru_cache(maxsize=None)
def mixed_scene():
    base = partial_scene()
    big = make_scene(3, MIXED_BIG_SEGS, n_neighbors=2, seed=19).views
    views = [copy.copy(v) for v in base.views]
    for v in big:
        v.cam += 200
        v.neighbors = [int(n) + 200 for n in v.neighbors]
    return _with_views(base, views + list(big), "partial190+3x4200")


# (d) kNN at the table limits: three views of 1 500 segments that neighbour each other (78 row-form items: the two-wave
# tier under L3D_MATCH_TILE=0), alone and with 100 views of two segments and 40 neighbours each around them, which bring
# the call into the row form by itself (2 072 estimated items) and its launch of 4 078 items into the row-cache tier
KNN_SEGS, KNN_EPI = 1500, 0.005


@functools.lru_cache(maxsize=None)
def knn_scene(padded):
    big = make_scene(3, KNN_SEGS, n_neighbors=2, seed=29).views
    if not padded:
        return Scene(list(big), "knn3")
    small = make_scene(100, 2, n_neighbors=40, seed=31).views
    for v in small:
        v.cam += 10
        v.neighbors = [int(n) + 10 for n in v.neighbors]
    return Scene(list(big) + list(small), "knn3+100x2")


# ... and for the tile form two views of 4 200 segments at an overlap threshold of 1e-4: one pair of 268 tile items, rows
# that accept more than 1 668 targets
KNN_TILE_SEGS, KNN_TILE_EPI = 4200, 1e-4


@functools.lru_cache(maxsize=None)
def knn_tile_scene():
    return make_scene(2, KNN_TILE_SEGS, n_neighbors=2, seed=47, real_fraction=0.9)


def doubled(scene):
    """every segment twice in its view, as the tie tests of test_gpu_parity.py do it: nearly every row sees equal overlaps"""
    for v in scene.views:
        v.segs[1::2] = v.segs[0::2][:len(v.segs[1::2])]
    return scene


def drop_targets(scene, cam, segments):
    """the scene without the given segments of view `cam`"""
    out = Scene([copy.copy(v) for v in scene.views], scene.name + f"-{len(segments)}")
    for v in out.views:
        if v.cam == cam:
            v.segs = np.delete(v.segs, np.asarray(sorted(segments), np.int64), axis=0)
    return out


# (e) tied rows beyond the 1 024 entries k_match_tied_rows keeps in LDS: two views of 2 600 doubled segments at an overlap
# threshold of 1e-4.  Rows 32 and 33 of view 0 (one doubled segment) accept 1 068 targets of view 1; without the first 43 /
# 44 of them (TIE_DROP, ascending) they accept exactly 1 025 / 1 024.
TIE_SEGS, TIE_EPI, TIE_ROW = 2600, 1e-4, 32
TIE_DROP = (2, 3, 6, 7, 12, 13, 14, 15, 20, 21, 30, 31, 36, 37, 44, 45, 46, 47, 48, 49, 54, 55, 58, 59, 60, 61, 74, 75, 82, 83, 88, 89,
            108, 109, 118, 119, 124, 125, 134, 135, 138, 139, 148, 149)
TIE_LDS_HEAP = 1024


@functools.lru_cache(maxsize=None)
def tie_scene(row_length=None):
    """row_length None: as generated (rows 32 / 33 accept 1 068 targets); 1025 / 1024: with that many"""
    sc = doubled(make_scene(2, TIE_SEGS, n_neighbors=2, seed=43))
    if row_length is None:
        return sc
    return drop_targets(sc, 1, TIE_DROP[:1068 - row_length])
