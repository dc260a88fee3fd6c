"""The triangulation cases and their high-precision reference, on the CPU (tests/triangulate_cases.py):
the stored inputs are the generator's, bit for bit; the stored truth is mpmath's again, within one ulp; and every case is
what tests/test_gpu_triangulate.py takes it for -- its yardstick sharp enough to say something, its special points
special -- judged on the references alone."""
import numpy as np
import pytest

from tests import triangulate_cases as TC
from tests import triangulate_model as TM


@pytest.fixture(scope="module")
def stored():
    return TC.load()


def test_the_fixture_holds_every_case_and_nothing_else(stored):
    assert sorted(stored) == sorted(TC.BUILDERS) and set(TC.ACCURACY) <= set(stored)
    assert sum(len(c["off"]) - 1 for c in stored.values()) == 5 * 64 + 513 + 2 * 128
    assert max(len(c["cam"]) for c in stored.values()) <= 5300


@pytest.mark.parametrize("name", list(TC.BUILDERS))
def test_the_stored_inputs_are_the_generators_bit_for_bit(stored, name):
    made, kept = TC.build(name), stored[name]
    assert sorted(kept) == sorted(list(made) + ["truth"])
    for k, v in made.items():
        v = np.asarray(v)
        assert v.dtype == kept[k].dtype and v.shape == kept[k].shape, k
        assert v.tobytes() == kept[k].tobytes(), k                              # NaN payloads and signed zeros included


@pytest.mark.parametrize("name", list(TC.BUILDERS))
def test_the_stored_truth_is_mpmaths_within_one_ulp(stored, name):
    pytest.importorskip("mpmath")
    c = stored[name]
    T = TC.truth(*TC.matrices(c))
    assert np.array_equal(np.isnan(T), np.isnan(c["truth"]))
    inf = np.isinf(T)
    assert np.array_equal(T[inf], c["truth"][inf])
    ok = np.isfinite(T)
    ulps = np.abs(T[ok] - c["truth"][ok]) / np.spacing(np.abs(c["truth"][ok]))
    print(f"{name}: {int(ok.sum())} finite components, largest distance {ulps.max():.3g} ulp")
    assert ulps.max() <= 1


def _parts(name, c):
    """the sets of points the GPU test judges together"""
    if name == "lds_edge":
        return {"first half": list(range(64)), "all": None}
    if name == "contract":
        return {"ordinary": TC.ordinary(), "one camera": [TC.ONE_CAMERA]}
    return {"all": None}


@pytest.mark.parametrize("name", TC.ACCURACY)
def test_the_yardstick_of_every_accuracy_case_says_something(stored, name):
    c = stored[name]
    for part, points in _parts(name, c).items():
        e_svd, e_eigh, bound = TC.yardsticks(c, points)
        print(f"{name}, {part}: e_svd {e_svd:.3g}, e_eigh {e_eigh:.3g}, bound {bound:.3g}")
        assert min(e_svd, e_eigh) <= TC.YARDSTICK_MAX
        assert bound >= 4 * TC.EPS
    # the two host solvers agree on which points are valid, and the judged points are the valid finite ones
    M, counts = TC.matrices(c)
    (Xs, vs), (Xe, ve) = TM.solve_svd(M, counts), TM.solve_eigh(M, counts)
    assert np.array_equal(vs, ve)
    finite = vs & np.isfinite(Xs).all(axis=1)
    if name == "contract":
        assert np.array_equal(TC.judged(c) & vs, finite)
    else:
        assert np.array_equal(TC.judged(c), finite) and np.array_equal(vs, counts > 2)


def test_shifts_move_the_cameras_and_points_only(stored):
    o = stored["origin"]
    for name in ("shift_1e3", "shift_1e5", "scaled_P"):
        c = stored[name]
        assert np.array_equal(c["off"], o["off"]) and np.array_equal(c["cam"], o["cam"]) and c["extent"] == o["extent"]
    for name, s in (("shift_1e3", 1e3), ("shift_1e5", 1e5)):
        moved = stored[name]["truth"] - s * TC.SHIFT
        assert np.abs(moved - o["truth"]).max() <= 1e-4 * o["extent"]           # the same scene, somewhere else
        assert np.abs(stored[name]["xy"] - o["xy"]).max() <= 1e-6               # pixels
    assert np.array_equal(stored["scaled_P"]["xy"], o["xy"])
    ratio = stored["scaled_P"]["P"] / o["P"]
    assert np.array_equal(ratio, np.broadcast_to(np.array([2.0 ** -4, 2.0 ** 4, 1.0] * 4)[:, None, None], ratio.shape))


def test_edges_has_its_short_lists_at_the_block_boundary(stored):
    c = stored["edges"]
    counts = np.diff(c["off"].astype(np.int64))
    assert len(counts) == 513 == TC.EDGE_PREFIXES[-1] and int(c["cam"].max()) == 39
    assert np.nonzero(counts <= 2)[0].tolist() == list(TC.EDGE_TWO_OBSERVATIONS) and counts.min() == 2
    assert 3 <= counts[counts > 2].min() and counts.max() <= 9
    for n in TC.EDGE_PREFIXES:
        off, cam, xy = TC.prefix(c, n)
        assert len(off) == n + 1 and off[0] == 0 and len(cam) == len(xy) == off[-1]


def test_lds_edge_reads_the_last_staged_camera_and_the_first_unstaged_one(stored):
    c = stored["lds_edge"]
    assert len(c["P"]) == TC.LDS_CAMERAS + 1 and 96 * TC.LDS_CAMERAS <= 32 * 1024 < 96 * (TC.LDS_CAMERAS + 1)
    off = c["off"].astype(np.int64)
    for i in range(128):
        mine = c["cam"][off[i]:off[i + 1]].tolist()
        assert 3 <= len(mine) <= 12 and len(set(mine)) == len(mine)
        assert TC.LDS_CAMERAS - 1 in mine and (TC.LDS_CAMERAS in mine) == (i >= 64)
    assert {len(c["cam"][off[i]:off[i + 1]]) for i in range(128)} >= {3, 12}


def test_long_list_has_one_long_one_empty_and_the_rest_three(stored):
    c = stored["long_list"]
    counts = np.diff(c["off"].astype(np.int64))
    assert counts.tolist() == [TC.LONG_OBSERVATIONS, 0] + [3] * 62 and len(c["P"]) == 300
    seen = c["cam"][:TC.LONG_OBSERVATIONS]
    assert len(np.unique(seen)) == 300                                           # with repetition: every camera, many times
    assert len(np.unique(c["xy"][:TC.LONG_OBSERVATIONS], axis=0)) == TC.LONG_OBSERVATIONS      # each with its own noise
    rev = TC.select(c, list(range(63, -1, -1)))
    assert np.diff(rev[0].astype(np.int64)).tolist() == counts[::-1].tolist()
    assert np.array_equal(rev[1][-TC.LONG_OBSERVATIONS:], seen)


def test_the_contract_batchs_special_points_are_special(stored):
    c = stored["contract"]
    M, counts = TC.matrices(c)
    (Xs, vs), (Xe, ve) = TM.solve_svd(M, counts), TM.solve_eigh(M, counts)
    T = c["truth"]
    assert len(counts) == TC.CONTRACT_POINTS and len(c["P"]) == TC.CONTRACT_CAMERAS < TC.LDS_CAMERAS
    # at infinity: decoupled exactly; the two host solvers take opposite signs
    m = M[TC.AT_INFINITY]
    assert not m[:3, 3].any() and not m[3, :3].any() and m[3, 3] == TC.INFINITY_M33
    assert c["cam"][c["off"][TC.AT_INFINITY]:c["off"][TC.AT_INFINITY + 1]].tolist() == list(range(TC.CAM_INFINITY, TC.CAM_INFINITY + 6))
    for X in (T, Xs, Xe):
        assert np.isinf(X[TC.AT_INFINITY]).all() and len(set(np.sign(X[TC.AT_INFINITY]))) == 1
    assert vs[TC.AT_INFINITY] and ve[TC.AT_INFINITY]
    # one camera, three observations: its centre, by the truth and by both solvers
    lo, hi = int(c["off"][TC.ONE_CAMERA]), int(c["off"][TC.ONE_CAMERA + 1])
    assert c["cam"][lo:hi].tolist() == [TC.CAM_ONE] * 3 and len(np.unique(c["xy"][lo:hi], axis=0)) == 3
    for X in (T, Xs, Xe):
        assert np.abs(X[TC.ONE_CAMERA] - c["centre"]).max() <= 1e-6 * c["extent"]
    assert vs[TC.ONE_CAMERA]
    # diagonal on entry, the smallest entry at index 2 and at index 3
    for i, diagonal in ((TC.DIAGONAL_2, [4, 4, 0, 8]), (TC.DIAGONAL_3, [4, 4, 8, 0])):
        assert np.array_equal(M[i], np.diag(np.array(diagonal, np.float64))) and not vs[i] and not ve[i]
    # non-finite inputs: M is not finite, the model says invalid
    for i in (TC.NAN_PIXEL, TC.INF_PIXEL, TC.NAN_P):
        assert counts[i] > 2 and not np.isfinite(M[i]).all() and not vs[i] and np.isnan(T[i]).all()
    lo = int(c["off"][TC.NAN_PIXEL])
    assert np.isnan(c["xy"][lo + 1, 1]) and np.isinf(c["xy"][int(c["off"][TC.INF_PIXEL]), 0])
    assert TC.CAM_NAN in c["cam"][c["off"][TC.NAN_P]:c["off"][TC.NAN_P + 1]] and np.isnan(c["P"][TC.CAM_NAN]).sum() == 1
    assert (c["cam"] == TC.CAM_NAN).sum() == 1
    # the camera whose P the test poisons is observed by nobody and finite here
    assert TC.CAM_UNUSED not in c["cam"] and np.isfinite(c["P"][TC.CAM_UNUSED]).all()
    # the special points share waves with ordinary ones, and everything else is ordinary
    assert {i // 64 for i in TC.SPECIAL} == {0, 1}
    o = TC.ordinary()
    assert len(o) == TC.CONTRACT_POINTS - len(TC.SPECIAL) and vs[o].all() and int(c["cam"][np.concatenate(
        [np.arange(c["off"][i], c["off"][i + 1]) for i in o]).astype(np.int64)].max()) < 12
    assert (~vs).sum() == 5
