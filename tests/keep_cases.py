"""Host model of the keep-all mode's ragged slot buffer (kNN <= 0) and the scenes of tests/test_gpu_keep.py.
A restatement of the contract in numpy (cumulative sums, searchsorted, unique), not of the kernels' loops:

  * the accepted matches of source row r of pair p lie in the slots [row_start[row_off[p] + r], row_start[row_off[p] + r + 1]) of
    ONE buffer, pairs in pair order, rows in row order, a row's matches in ascending target order;
  * per pair the table {first slot, longest row, number of slots}; per row its pair (row_pair); per block of BLOCK = 1 024
    slots the row that holds the block's first slot (blk_row) -- an empty row holds no slot;
  * the assembly runs one workgroup per block: it stages STAGED_ROWS = 2 048 row starts from blk_row on, a slot whose row
    lies fewer than STAGED_ROWS - 1 rows behind blk_row is placed from the staged starts, any other by a search in memory;
    a slot's rank in its row is counted in three parts -- the row's records before the block, inside it, behind it;
  * the host (host_plan): the scratch keeps `keep_cap` records per row (96 on a context's first call, or L3D_KEEPALL_CAP); a
    longer row repeats the pass with keep_cap = (longest + longest / 8 + 31) & ~31, which the context keeps; the outputs are
    sized before the pass to guess = max(last total + last total / 8 + 65 536, 16 x rows) slots, and the assembly runs a
    second time when the total is beyond what they hold -- at least `guess`, at most 1.5 x guess.

tests/test_keep_cases.py holds the model against a sequential restatement and asserts, on the CPU oracle's counts, that
every scene meets the condition it is named for."""
import copy
import functools

import numpy as np

from line3dpp_amd.scene import Scene, make_scene
from tests import match_cases as MC

BLOCK = 1024
STAGED_ROWS = 2048
DEFAULT_CAP = 96
GUESS_FLOOR = 1 << 16
DENSE_EPI, SPARSE_EPI = 1e-4, 0.9


# ---- the model -----------------------------------------------------------------------------------------------------------
class Layout:
    """the ragged buffer of one call, from the accepted matches per source row of every pair, in pair order"""

    def __init__(self, counts):
        self.counts = [np.asarray(c, np.int64) for c in counts]
        P = len(self.counts)
        Ms = np.array([len(c) for c in self.counts], np.int64)
        self.row_off = np.concatenate([[0], np.cumsum(Ms)])
        self.all = np.concatenate(self.counts) if P else np.zeros(0, np.int64)
        self.n_rows = int(self.row_off[-1])
        self.row_start = np.concatenate([[0], np.cumsum(self.all)])
        self.total = int(self.row_start[-1])
        self.pair_table = np.array([[self.row_start[self.row_off[p]], c.max(initial=0), c.sum()] for p, c in enumerate(self.counts)],
                                   np.int64).reshape(P, 3)
        self.longest = int(self.pair_table[:, 1].max(initial=0))
        self.row_pair = np.repeat(np.arange(P), Ms)
        self.n_blocks = -(-self.total // BLOCK)
        ends = self.row_start[1:]
        # the row that holds a slot: the first row that ends behind it
        self.blk_row = np.searchsorted(ends, np.arange(self.n_blocks) * BLOCK, side="right")
        slot = np.arange(self.total)
        self.slot_grow = np.searchsorted(ends, slot, side="right")                 # row among all rows of the call
        self.slot_row = self.slot_grow - self.row_off[self.row_pair[self.slot_grow]]   # row inside its pair
        self.slot_block = slot // BLOCK
        self.slot_offset = self.slot_grow - self.blk_row[self.slot_block]
        self.slot_in_memory = self.slot_offset >= STAGED_ROWS - 1

    def rank_parts(self):
        """per (row, block) that share a slot: arrays row, block, and the row's records before / inside / behind the block"""
        key, inside = np.unique(self.slot_grow * max(self.n_blocks, 1) + self.slot_block, return_counts=True)
        row, block = key // max(self.n_blocks, 1), key % max(self.n_blocks, 1)
        before = np.maximum(block * BLOCK - self.row_start[row], 0)
        return dict(row=row, block=block, before=before, inside=inside, after=self.all[row] - before - inside)

    def rows_per_block(self):
        """rows between the row of a block's first slot and the row of its last one, inclusive"""
        last = np.minimum((np.arange(self.n_blocks) + 1) * BLOCK, self.total) - 1
        return self.slot_grow[last] - self.blk_row + 1


def host_plan(layout, keep_cap=0, last_total=0, env_cap=None):
    """what the host decides for a call with this layout on a context that holds keep_cap (0: its first keep-all call, which
    reads L3D_KEEPALL_CAP = env_cap) and whose previous keep-all call had last_total slots.  second_assembly: True / False
    where the contract decides it, None between guess and 1.5 x guess (the allocator's choice)."""
    first_cap = keep_cap or (env_cap if env_cap and env_cap > 0 else DEFAULT_CAP)
    longest, total = layout.longest, layout.total
    repeat = longest > first_cap
    next_cap = ((longest + longest // 8 + 31) & ~31) if repeat else first_cap
    guess = min(max(last_total + last_total // 8 + GUESS_FLOOR, 16 * layout.n_rows), 2**32 - 1)
    second = True if total > guess + guess // 2 else False if total <= guess else None
    return dict(first_cap=first_cap, repeat=repeat, keep_cap=next_cap, guess=guess, second_assembly=second,
                last_total=total)


def counter_delta(plan):
    """what the call adds to l3d_debug_counter("keep_all_repeats"): (low half: passes repeated, high half: second assemblies)"""
    assert plan["second_assembly"] is not None, "the case leaves the second assembly to the allocator"
    return int(plan["repeat"]), int(plan["second_assembly"])


# ---- tools -----------------------------------------------------------------------------------------------------------------
def rows_summing_to(counts, rows, amount):
    """rows among `rows` whose counts sum to exactly `amount` (a subset-sum table over the sums up to `amount`), or None"""
    reach = {0: ()}
    for r in rows:
        c = int(counts[r])
        if amount in reach:
            break
        if c == 0 or c > amount:
            continue
        for s, sel in list(reach.items()):
            if s + c <= amount and s + c not in reach:
                reach[s + c] = sel + (int(r),)
    return reach.get(amount)


def rows_shifting(counts, rows, residue):
    """rows among `rows` whose counts sum to `residue` modulo BLOCK"""
    for k in range(4):
        sel = rows_summing_to(counts, rows, residue % BLOCK + k * BLOCK)
        if sel is not None:
            return sel
    raise AssertionError(f"no rows among {len(rows)} sum to {residue} mod {BLOCK}")


def _named(scene, name):
    return Scene([copy.copy(v) for v in scene.views], name)


def without(scene, cam, segments, name):
    out = MC.drop_targets(scene, cam, list(segments))
    out.name = name
    return out


def _swapped(scene, cam, a, b):
    for v in scene.views:
        if v.cam == cam:
            v.segs = v.segs.copy()
            v.segs[[a, b]] = v.segs[[b, a]]
    return scene


@functools.lru_cache(maxsize=None)
def oracle_pairs(name, epi=None):
    """((matches, CSR offsets per source row), ...) of every pair of a case's scene, by the CPU oracle at kNN = 0: computed
    once per process and never modified"""
    from oracle.oracle import Oracle
    sc = scene(name)
    o = Oracle(threads=16)
    o.add_scene(sc)
    o.begin_match(kNN=0, epi_overlap=CASES[name][1] if epi is None else epi)
    out = tuple(o.match_pair(s, t) for s, t in MC.pair_list(sc))
    o.end_match()
    for m, off in out:
        m.setflags(write=False); off.setflags(write=False)
    return out


def counts_of(name, epi=None):
    return [np.diff(off.astype(np.int64)) for _, off in oracle_pairs(name, epi)]


@functools.lru_cache(maxsize=None)
def layout(name, epi=None):
    return Layout(counts_of(name, epi))


# ---- the scenes ------------------------------------------------------------------------------------------------------------
# dense: two views of 2 600 segments at an overlap threshold of 1e-4 -- one pair of 287 712 matches, 110.7 per row, the longest
# row (row 64) 1 185, five rows beyond a block, three empty rows (388, 688, 1 798)
def _dense():
    return make_scene(2, 2600, n_neighbors=2, seed=43)


def _dense_long_row():
    c = counts_of("dense")[0]
    r = int(np.argmax(c))
    m, off = oracle_pairs("dense")[0]
    return c, r, np.asarray(m["tgt_seg"][off[r]:off[r + 1]], np.int64)


def _dense_row(length):
    """the longest row cut to `length` matches: without its first targets"""
    c, r, tg = _dense_long_row()
    return without(_dense(), 1, tg[:int(c[r]) - length], f"dense_row_{length}")


def _dense_row_doubled():
    """every accepted target of the longest row twice in the target view: a row of two blocks and more"""
    c, r, tg = _dense_long_row()
    sc = _named(_dense(), "dense_row_doubled")
    sc.views[1].segs = np.concatenate([sc.views[1].segs, sc.views[1].segs[tg]], 0)
    return sc


def _dense_moved(long_start, block_row_start, total, name, long_end=None):
    """the dense scene without some source rows, chosen so that the longest row starts at long_start modulo BLOCK (or ends
    at long_end), the row behind the first empty row starts at block_row_start, and the total is `total`: each None or a
    residue modulo BLOCK"""
    c, r, _ = _dense_long_row()
    start = np.concatenate([[0], np.cumsum(c)])
    gone = []
    if long_end is not None:
        long_start = long_end - int(c[r])
    if long_start is not None:
        gone += rows_shifting(c, range(r), int(start[r]) - long_start)
    e = int(np.nonzero(c == 0)[0][0])                   # the first empty row; e + 1 holds matches
    assert e > r + 1 and c[e + 1] > 0
    if block_row_start is not None:
        gone += rows_shifting(c, range(r + 1, e), int(start[e + 1]) - int(c[gone].sum()) - block_row_start)
    if total is not None:
        gone += rows_shifting(c, range(e + 2, len(c)), int(start[-1]) - int(c[gone].sum()) - total)
    return without(_dense(), 0, gone, name)


# sparse: two views of 3 000 segments at 0.9 -- one pair of 555 matches in 484 of its 3 000 rows, all in one block
def _sparse():
    return make_scene(2, 3000, n_neighbors=2, seed=5)


def _sparse_ring3():
    """three such views, pairs (0,1) (0,2) (1,2): the second block starts in the middle of the call's 9 000 rows"""
    return make_scene(3, 3000, n_neighbors=2, seed=5)


def _sparse_offsets():
    """without empty source rows, so that three rows with matches lie exactly 2 046, 2 047 and 2 048 rows behind the first
    row with matches"""
    c = counts_of("sparse")[0]
    nz = np.nonzero(c)[0]
    first = int(nz[0])
    k = int(np.searchsorted(nz, first + STAGED_ROWS))
    a, b, d = (int(x) for x in nz[k:k + 3])
    empty_before = [r for r in range(first + 1, a) if c[r] == 0]
    gone = empty_before[:(a - first) - (STAGED_ROWS - 2)] + list(range(a + 1, b)) + list(range(b + 1, d))
    return without(_sparse(), 0, gone, "sparse_offsets")


def _sparse_control():
    sc = _named(_sparse(), "sparse_control")
    for v in sc.views:
        v.segs = v.segs[:1000].copy()
    return sc


# empty_pairs: seven views in a ring, pairs (0,1) (0,6) (1,2) (2,3) (3,4) (4,5) (5,6); without the source rows that match in
# the first, a middle and the last pair
EMPTY_PAIRS = ((0, 1), (2, 3), (5, 6))
EMPTY_PAIRS_EPI = 0.5


def _ring7():
    return make_scene(7, 400, n_neighbors=2, seed=17)


def _empty_pairs():
    sc = _ring7()
    pl = MC.pair_list(sc)
    c = counts_of("ring7")
    for s, t in EMPTY_PAIRS:
        sc = without(sc, s, np.nonzero(c[pl.index((s, t))])[0], "empty_pairs")
    return sc


# pair_info: source views of 1 100, 257, 256, 65, 63 and 1 segments; the longest row of pair (0,1) moved to its last row, of
# pair (1,2) to row 255 of 257, of pair (2,3) to row 255 of 256
PAIR_INFO_SIZES = (1100, 257, 256, 65, 63, 1, 300)
PAIR_INFO_EPI = 0.05
PAIR_INFO_MOVES = ((0, 1, 1099), (1, 2, 255), (2, 3, 255))


def _pair_info_raw():
    sc = make_scene(7, 1100, n_neighbors=2, seed=3)
    for v, n in zip(sc.views, PAIR_INFO_SIZES):
        v.segs = v.segs[:n].copy()
    return sc


def _pair_info():
    sc = _named(_pair_info_raw(), "pair_info")
    pl = MC.pair_list(sc)
    c = counts_of("pair_info_raw")
    for s, t, to in PAIR_INFO_MOVES:
        _swapped(sc, s, int(np.argmax(c[pl.index((s, t))])), to)
    return sc


# name: (builder, overlap threshold, the condition it reaches)
CASES = {
    "dense": (_dense, DENSE_EPI, "rows beyond a block; total beyond 1.5 x guess; longest row beyond the default scratch"),
    "dense_row_1023": (lambda: _dense_row(1023), DENSE_EPI, "a row of 1 023 matches"),
    "dense_row_1024": (lambda: _dense_row(1024), DENSE_EPI, "a row of 1 024 matches"),
    "dense_row_1025": (lambda: _dense_row(1025), DENSE_EPI, "a row of 1 025 matches"),
    "dense_row_doubled": (_dense_row_doubled, DENSE_EPI, "a row of 2 049 or more: two block boundaries, three rank parts"),
    "dense_aligned": (lambda: _dense_moved(0, 0, 0, "dense_aligned"), DENSE_EPI,
                      "a long row starts on a block boundary; empty row before a block's first row; total a multiple of 1 024"),
    "dense_after": (lambda: _dense_moved(1, None, 1, "dense_after"), DENSE_EPI,
                    "a long row starts one slot behind a boundary; total a multiple of 1 024 plus 1"),
    "dense_end": (lambda: _dense_moved(None, None, None, "dense_end", long_end=0), DENSE_EPI, "a long row ends on a block boundary"),
    "sparse": (_sparse, SPARSE_EPI, "one block over nearly 3 000 rows; empty rows at the end; total below the guess"),
    "sparse_offsets": (_sparse_offsets, SPARSE_EPI, "row offsets 2 046, 2 047, 2 048 and beyond 2 900 in one block"),
    "sparse_control": (_sparse_control, SPARSE_EPI, "fewer than 2 047 rows per block"),
    "sparse_ring3": (_sparse_ring3, SPARSE_EPI, "a block behind the first whose rows go beyond the staged table"),
    "ring7": (_ring7, EMPTY_PAIRS_EPI, "(base of empty_pairs)"),
    "empty_pairs": (_empty_pairs, EMPTY_PAIRS_EPI, "pairs without a slot: the first, a middle one, the last"),
    "pair_info_raw": (_pair_info_raw, PAIR_INFO_EPI, "(base of pair_info)"),
    "pair_info": (_pair_info, PAIR_INFO_EPI, "Ms of 1, 63, 65, 256, 257, 1 100; longest row last and at row 255"),
}
GPU_CASES = tuple(n for n in CASES if n not in ("ring7", "pair_info_raw"))
DENSE_CASES = tuple(n for n in GPU_CASES if n.startswith("dense"))


@functools.lru_cache(maxsize=None)
def scene(name):
    sc = CASES[name][0]()
    sc.name = name
    return sc


def epi(name):
    return CASES[name][1]


# (h) calls on one context: the dense scene at both thresholds, in two orders
SEQUENCES = ((DENSE_EPI, SPARSE_EPI, DENSE_EPI), (SPARSE_EPI, DENSE_EPI))


def sequence_plans(seq, name="dense"):
    """host_plan of every call of a sequence on one context"""
    cap, last, out = 0, 0, []
    for e in seq:
        p = host_plan(layout(name, e), keep_cap=cap, last_total=last)
        cap, last = p["keep_cap"], p["last_total"]
        out.append(p)
    return out
