"""CPU checks behind tests/test_gpu_keep.py (no device needed): the numpy model of the keep-all mode's ragged slot buffer
(tests/keep_cases.py) against a sequential restatement -- a plain loop over the rows -- and, on the CPU oracle's counts, the
condition every scene is named for (conditions a to h of DESIGN §21).  A condition that a scene no longer meets, after a
drift of the scene generator for instance, fails here instead of silently losing the coverage on the GPU."""
import numpy as np
import pytest

from tests import keep_cases as KC
from tests import match_cases as MC

B = KC.BLOCK


def _long_rows(lay):
    """(row, start, length) of the rows beyond a block"""
    return [(int(r), int(lay.row_start[r]), int(lay.all[r])) for r in np.nonzero(lay.all > B)[0]]


# ---- the model against a plain loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KC.GPU_CASES)
def test_model_equals_a_sequential_restatement(name):
    lay = KC.layout(name)
    counts = KC.counts_of(name)
    row_start, slot_grow, slot_row, row_pair, table = [0], [], [], [], []
    for p, c in enumerate(counts):
        first, longest, n = row_start[-1], 0, 0
        for r, k in enumerate(c):
            k = int(k)
            slot_grow += [len(row_pair)] * k
            slot_row += [r] * k
            row_pair.append(p)
            row_start.append(row_start[-1] + k)
            longest = max(longest, k); n += k
        table.append([first, longest, n])
    total = row_start[-1]
    assert lay.total == total == len(slot_grow) and lay.n_rows == len(row_pair)
    assert lay.row_start.tolist() == row_start and lay.row_pair.tolist() == row_pair
    assert lay.pair_table.tolist() == table
    assert lay.slot_grow.tolist() == slot_grow and lay.slot_row.tolist() == slot_row
    blk_row = [slot_grow[b] for b in range(0, total, B)]
    assert lay.blk_row.tolist() == blk_row and lay.n_blocks == len(blk_row)
    assert lay.slot_offset.tolist() == [g - blk_row[i // B] for i, g in enumerate(slot_grow)]
    parts = {}
    for i, g in enumerate(slot_grow):
        parts[(g, i // B)] = parts.get((g, i // B), 0) + 1
    rp = lay.rank_parts()
    assert len(rp["row"]) == len(parts)
    seen = {}                                           # records of a row in the blocks walked so far
    for (r, b), got in zip(sorted(parts), zip(*(rp[k].tolist() for k in ("row", "block", "before", "inside", "after")))):
        assert got == (r, b, seen.get(r, 0), parts[(r, b)], int(lay.all[r]) - seen.get(r, 0) - parts[(r, b)])
        seen[r] = seen.get(r, 0) + parts[(r, b)]


def test_host_plan_arithmetic():
    lay = KC.Layout([np.array([0, 97, 3])])
    p = KC.host_plan(lay)
    assert p == dict(first_cap=96, repeat=True, keep_cap=(97 + 12 + 31) & ~31, guess=65536, second_assembly=False, last_total=100)
    assert KC.host_plan(lay, env_cap=97)["repeat"] is False and KC.host_plan(lay, keep_cap=128, env_cap=2)["first_cap"] == 128
    big = KC.Layout([np.full(5000, 20)])
    assert KC.host_plan(big)["guess"] == 80000 and KC.host_plan(big)["second_assembly"] is None       # 80 000 < 100 000 <= 120 000
    assert KC.host_plan(big, last_total=100000)["guess"] == 100000 + 12500 + 65536
    assert KC.host_plan(KC.Layout([np.full(5000, 25)]))["second_assembly"] is True


# ---- the raw scenes ------------------------------------------------------------------------------------------------------------
def test_the_two_raw_scenes_have_the_measured_shape():
    d = KC.layout("dense")
    assert MC.pair_list(KC.scene("dense")) == [(0, 1)] and d.n_rows == 2600
    assert d.total == 287712 and d.longest == 1185 and int((d.all > B).sum()) == 5 and int((d.all == 0).sum()) == 3
    assert abs(d.all.mean() - 110.66) < 0.01
    s = KC.layout("sparse")
    assert s.n_rows == 3000 and s.total == 555 and int((s.all == 0).sum()) == 2516 and s.longest == 3 and s.n_blocks == 1
    print(f"dense: {d.total} matches, longest {d.longest}, rows beyond a block {_long_rows(d)}; sparse: {s.total} matches in "
          f"{int((s.all > 0).sum())} of {s.n_rows} rows, block 0 spans {int(s.rows_per_block()[0])} rows")


# ---- conditions a to h -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_a_rows_of_one_block_minus_one_to_plus_one(n):
    lay = KC.layout(f"dense_row_{n}")
    rows = np.nonzero(lay.all == n)[0]
    assert len(rows) >= 1
    print(f"(a) dense_row_{n}: row {int(rows[0])} has {n} matches, starts at slot {int(lay.row_start[rows[0]])}; total {lay.total}")


def test_a_row_across_two_block_boundaries_with_three_rank_parts():
    lay = KC.layout("dense_row_doubled")
    assert lay.longest >= 2 * B + 1
    rp = lay.rank_parts()
    hit = np.nonzero((rp["before"] > 0) & (rp["inside"] == B) & (rp["after"] > 0) & (lay.all[rp["row"]] >= 2 * B + 1))[0]
    assert len(hit) >= 1
    r = int(rp["row"][hit[0]])
    assert int((rp["row"] == r).sum()) >= 3
    print(f"(a) dense_row_doubled: row {r} has {int(lay.all[r])} matches from slot {int(lay.row_start[r])}; in block "
          f"{int(rp['block'][hit[0]])} its rank parts are {int(rp['before'][hit[0]])} / {B} / {int(rp['after'][hit[0]])}")


def test_b_a_long_row_at_every_kind_of_start():
    for name, what, test in (("dense_aligned", "starts on a boundary", lambda s, n: s % B == 0),
                             ("dense_after", "starts one slot behind a boundary", lambda s, n: s % B == 1),
                             ("dense_end", "ends on a boundary", lambda s, n: (s + n) % B == 0)):
        lay = KC.layout(name)
        hit = [x for x in _long_rows(lay) if test(x[1], x[2])]
        assert hit, (name, _long_rows(lay))
        print(f"(b) {name}: row {hit[0][0]} of {hit[0][2]} matches {what}: slots [{hit[0][1]}, {hit[0][1] + hit[0][2]})")


def test_c_row_offsets_across_the_staged_table():
    lay = KC.layout("sparse_offsets")
    assert lay.n_blocks == 1
    offs = set(lay.slot_offset.tolist())
    S = KC.STAGED_ROWS
    assert {S - 2, S - 1, S} <= offs and max(offs) > 2900
    for o, mem in ((S - 2, False), (S - 1, True), (S, True)):
        assert set(lay.slot_in_memory[lay.slot_offset == o].tolist()) == {mem}
    raw = KC.layout("sparse")
    assert int(raw.rows_per_block()[0]) >= S - 1 and raw.slot_in_memory.any()
    ctl = KC.layout("sparse_control")
    assert ctl.total > 0 and int(ctl.rows_per_block().max()) < S - 1 and not ctl.slot_in_memory.any()
    print(f"(c) sparse_offsets: block 0 from row {int(lay.blk_row[0])}, offsets {S - 2}, {S - 1}, {S} present, largest "
          f"{max(offs)}, {int(lay.slot_in_memory.sum())} of {lay.total} slots found in memory; sparse: "
          f"{int(raw.slot_in_memory.sum())} of {raw.total}; sparse_control: {ctl.total} slots, "
          f"{int(ctl.rows_per_block().max())} rows in its block, none in memory")
    r3 = KC.layout("sparse_ring3")
    later = np.unique(r3.slot_block[r3.slot_in_memory])
    assert r3.n_blocks >= 2 and later.max() >= 1 and int(r3.blk_row[later.max()]) > 0
    print(f"(c) sparse_ring3: {r3.total} slots in {r3.n_blocks} blocks of {r3.rows_per_block().tolist()} rows, slots found in "
          f"memory in blocks {later.tolist()}, block {int(later.max())} from row {int(r3.blk_row[later.max()])}")
    for name in KC.DENSE_CASES:                         # (the dense scenes never leave the staged table)
        assert not KC.layout(name).slot_in_memory.any()


def test_d_empty_rows_and_pairs_at_the_boundaries():
    lay = KC.layout("dense_aligned")
    hit = [b for b in range(1, lay.n_blocks) if lay.row_start[lay.blk_row[b]] == b * B and lay.all[lay.blk_row[b] - 1] == 0]
    assert hit
    print(f"(d) dense_aligned: block {hit[0]} starts with row {int(lay.blk_row[hit[0]])}, behind an empty row; total {lay.total} = "
          f"{lay.total // B} x {B}")
    assert lay.total % B == 0 and lay.total > 0
    aft = KC.layout("dense_after")
    assert aft.total % B == 1 and aft.n_blocks == aft.total // B + 1
    print(f"(d) dense_after: total {aft.total} = {aft.total // B} x {B} + 1")
    sp = KC.layout("sparse")
    tail = sp.n_rows - 1 - int(np.nonzero(sp.all)[0][-1])
    assert tail >= 1 and sp.all[0] == 0
    print(f"(d) sparse: {tail} empty rows at the end of the buffer, {int(np.nonzero(sp.all)[0][0])} before its first slot")
    ep = KC.layout("empty_pairs")
    pl = MC.pair_list(KC.scene("empty_pairs"))
    empty = [pl[p] for p in np.nonzero(ep.pair_table[:, 2] == 0)[0]]
    assert tuple(empty) == KC.EMPTY_PAIRS and pl[0] == empty[0] and pl[-1] == empty[-1] and 0 < pl.index(empty[1]) < len(pl) - 1
    assert ep.total > 500
    print(f"(d) empty_pairs: slots per pair {dict(zip(pl, ep.pair_table[:, 2].tolist()))}")


def test_e_pair_info_reduction_edges():
    lay = KC.layout("pair_info")
    pl = MC.pair_list(KC.scene("pair_info"))
    Ms = [len(c) for c in lay.counts]
    assert {1, 63, 65, 256, 257} <= set(Ms) and max(Ms) > B
    for s, t, to in KC.PAIR_INFO_MOVES:
        c = lay.counts[pl.index((s, t))]
        assert int(np.argmax(c)) == to and int((c == c.max()).sum()) == 1, (s, t, np.nonzero(c == c.max())[0])
        assert to % 256 == 255 or to == len(c) - 1
    assert all(n > 0 for n in lay.pair_table[:, 2])
    print(f"(e) pair_info: Ms {Ms}, longest rows {lay.pair_table[:, 1].tolist()} at "
          f"{[int(np.argmax(c)) for c in lay.counts]}, slots {lay.pair_table[:, 2].tolist()}")


def test_f_g_capacity_and_scratch_decisions():
    d, s = KC.layout("dense"), KC.layout("sparse")
    ps = KC.host_plan(s)
    assert KC.counter_delta(ps) == (0, 0)
    pd = KC.host_plan(d)
    assert pd["first_cap"] == 96 and KC.counter_delta(pd) == (1, 1) and pd["keep_cap"] == 1344
    at = KC.host_plan(d, env_cap=d.longest)
    assert KC.counter_delta(at) == (0, 1) and at["keep_cap"] == d.longest
    below = KC.host_plan(d, env_cap=d.longest - 1)
    assert KC.counter_delta(below) == (1, 1) and below["keep_cap"] == 1344
    print(f"(f) sparse: total {s.total} <= guess {ps['guess']}: no second assembly; dense: total {d.total} > 1.5 x {pd['guess']}: one")
    print(f"(g) dense: L3D_KEEPALL_CAP {d.longest}: no repeat; {d.longest - 1}: repeat, keep_cap {below['keep_cap']}; default 96: repeat")
    for name in KC.GPU_CASES:                           # every case's counters are decided by the contract
        KC.counter_delta(KC.host_plan(KC.layout(name)))


def test_h_later_calls_on_one_context():
    a, b = (KC.sequence_plans(seq) for seq in KC.SEQUENCES)
    assert [KC.counter_delta(p) for p in a] == [(1, 1), (0, 0), (0, 1)]
    assert [KC.counter_delta(p) for p in b] == [(0, 0), (1, 1)]
    assert [p["first_cap"] for p in a] == [96, 1344, 1344] and [p["first_cap"] for p in b] == [96, 96]
    assert a[1]["guess"] == 287712 + 287712 // 8 + 65536 and a[2]["guess"] == 400 + 50 + 65536 == b[1]["guess"]
    print(f"(h) dense, sparse, dense: guesses {[p['guess'] for p in a]}, totals {[p['last_total'] for p in a]}, counters "
          f"{[KC.counter_delta(p) for p in a]}; sparse, dense: guesses {[p['guess'] for p in b]}, counters {[KC.counter_delta(p) for p in b]}")
