"""l3d_triangulate_points (k_triangulate.hip, l3d_triangulate.hip) on the MI355X against a high-precision eigenvector, at
its launch, staging and contract edges.

The inputs and their truth come from tests/golden/triangulate_truth.npz (tests/triangulate_cases.py; mpmath is not needed
here, tests/test_triangulate_cases.py holds the fixture to its generator on the CPU).  Per case, over its valid finite points:
    e_dev <= max(4 min(e_svd, e_eigh), 4 eps max(1, max|T| / extent))
with every e the largest distance to the truth as a fraction of the case's extent: the device may be no worse than four
times the better of numpy's SVD and eigh, each measured against the truth of the same M.  `valid` must be the model's, and
X zero where it is false.  Wherever the same point is computed twice -- in another prefix, behind another staging of the
projection matrices, in another order, beside other lanes -- its X and valid must be the same bits."""
import gc

import numpy as np
import pytest

from line3dpp_amd import _lib, api
from line3dpp_amd._lib import ptr
from tests import triangulate_cases as TC
from tests import triangulate_model as TM
from tests.test_gpu_blocks import live

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return TC.load()


def _same(a, b):
    """(X, valid) pairs equal bit for bit: NaNs, infinities and signed zeros included"""
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def _model_valid(c, points=None):
    M, counts = TC.matrices(c, points)
    return TM.solve_svd(M, counts)[1]


def _judge(name, c, X, valid, points=None):
    """print the row of DESIGN §22's table and hold the device to the bound; X, valid: of `points` in their order"""
    e_svd, e_eigh, bound = TC.yardsticks(c, points)
    e_dev = TC.error(X, c, points)
    n = len(c["off"]) - 1 if points is None else len(points)
    print(f"{name}: {n} points, {int(TC.judged(c, points).sum())} judged; e_svd {e_svd:.3g}, e_eigh {e_eigh:.3g}, "
          f"e_dev {e_dev:.3g}: {e_dev / bound:.3g} of the bound {bound:.3g}")
    assert min(e_svd, e_eigh) <= TC.YARDSTICK_MAX
    assert np.array_equal(valid, _model_valid(c, points))
    assert not X[~valid].any()
    assert e_dev <= bound


# ---- accuracy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["origin", "shift_1e3", "shift_1e5", "scaled_P"])
def test_against_the_high_precision_eigenvector(cases, name):
    c = cases[name]
    X, valid = api.triangulate_points(c["P"], c["off"], c["cam"], c["xy"])
    assert valid.all()
    _judge(name, c, X, valid)


def test_a_point_is_the_same_bits_in_every_prefix_that_holds_it(cases):
    """1, 255, 256, 257 and 513 points: one lane, a block short of one lane, a full block, a block and one lane, two
    blocks and one lane; lists of two observations in the last lanes of block 0, the first of block 1 and alone in block 2"""
    c = cases["edges"]
    whole = api.triangulate_points(c["P"], c["off"], c["cam"], c["xy"])
    _judge("edges", c, *whole)
    assert np.nonzero(~whole[1])[0].tolist() == list(TC.EDGE_TWO_OBSERVATIONS)
    for n in TC.EDGE_PREFIXES:
        part = api.triangulate_points(c["P"], *TC.prefix(c, n))
        assert part[0].shape == (n, 3) and _same(part, (whole[0][:n], whole[1][:n])), n


def test_the_last_staged_camera_and_the_first_unstaged_one(cases):
    """341 cameras are staged in LDS, 342 are read through the cache; every point observes camera 340, the last one
    staged, and the second half camera 341.  The source array of the 341-camera run holds NaN where camera 341 would be."""
    c = cases["lds_edge"]
    first = list(range(64))
    poisoned = c["P"].copy()
    poisoned[TC.LDS_CAMERAS] = np.nan
    staged_P = poisoned[:TC.LDS_CAMERAS]
    assert np.shares_memory(np.ascontiguousarray(staged_P), poisoned)              # no copy: the NaNs lie right behind
    staged = api.triangulate_points(staged_P, *TC.prefix(c, 64))
    cached = api.triangulate_points(c["P"], c["off"], c["cam"], c["xy"])
    _judge("lds_edge, 341 cameras in LDS", c, *staged, points=first)
    _judge("lds_edge, 342 cameras through the cache", c, *cached)
    assert staged[1].all() and cached[1].all()
    assert _same(staged, (cached[0][:64], cached[1][:64]))


def test_a_long_list_beside_short_ones_in_either_order(cases):
    """lane 0 walks 5 000 observations while its wave's other lanes walk three or none; reversed, it is lane 63"""
    c = cases["long_list"]
    forward = api.triangulate_points(c["P"], c["off"], c["cam"], c["xy"])
    _judge("long_list", c, *forward)
    assert forward[1].tolist() == [True, False] + [True] * 62
    order = list(range(63, -1, -1))
    backward = api.triangulate_points(c["P"], *TC.select(c, order))
    assert _same(backward, (forward[0][order], forward[1][order]))


# ---- the contract ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contract(cases):
    """the batch of 128 on the device, the same batch with a NaN in the projection matrix nobody observes, and its ordinary
    points alone"""
    c = cases["contract"]
    batch = api.triangulate_points(c["P"], c["off"], c["cam"], c["xy"])
    poisoned = c["P"].copy()
    poisoned[TC.CAM_UNUSED, 2, 1] = np.nan
    harmless = api.triangulate_points(poisoned, c["off"], c["cam"], c["xy"])
    alone = api.triangulate_points(c["P"], *TC.select(c, TC.ordinary()))
    return c, batch, harmless, alone


def test_ordinary_points_do_not_notice_the_special_ones_in_their_waves(contract):
    c, batch, _, alone = contract
    o = TC.ordinary()
    assert alone[1].all() and _same(alone, (batch[0][o], batch[1][o]))
    _judge("contract, ordinary points", c, *alone, points=o)


def test_valid_is_the_models_on_the_whole_batch(contract):
    c, (X, valid), _, _ = contract
    assert np.array_equal(valid, _model_valid(c))
    assert (~valid).sum() == 5 and not X[~valid].any()


def test_a_point_at_infinity_is_valid_and_infinite_with_one_sign(contract):
    _, (X, valid), _, _ = contract
    x = X[TC.AT_INFINITY]
    print("at infinity:", x)
    assert valid[TC.AT_INFINITY] and np.isinf(x).all() and (x[0] == x[1] == x[2])


def test_three_observations_by_one_camera_give_its_centre(contract):
    """M's null vector is the camera's centre; its next eigenvalue, 5.3, comes from the noise alone, beside a largest of
    6.7e7: eps |M| / lambda_2 = 2.8e-9, so a backward-stable fp64 solver owes this point about 1e-9 and no more.

    The rotations alone missed the bound here (e_svd 1.04e-11, e_eigh 5.22e-9, e_dev 1.09e-10 = 2.62 of the bound 4.17e-11);
    with the kernel's correction of the vector from its residual e_dev is 1.78e-16."""
    c, (X, valid), _, _ = contract
    i = [TC.ONE_CAMERA]
    to_centre = [float(np.linalg.norm(x - c["centre"]) / c["extent"]) for x in (c["truth"][i[0]], X[i[0]])]
    print(f"one camera: to the centre, of the extent: truth {to_centre[0]:.3g}, device {to_centre[1]:.3g}")
    assert valid[i[0]] and max(to_centre) <= 1e-6
    _judge("contract, one camera", c, X[i], valid[i], points=i)


@pytest.mark.parametrize("point", ["DIAGONAL_2", "DIAGONAL_3"])
def test_a_diagonal_matrix_runs_no_sweep_and_is_invalid(contract, point):
    """smallest entry at index 2: X holds 0 / 0; at index 3: X = 0, whose norm is not above L3D_EPS"""
    _, (X, valid), _, _ = contract
    i = getattr(TC, point)
    assert not valid[i] and X[i].tobytes() == np.zeros(3).tobytes()


@pytest.mark.parametrize("point", ["NAN_PIXEL", "INF_PIXEL", "NAN_P"])
def test_a_non_finite_input_is_invalid_and_zero(contract, point):
    c, (X, valid), _, _ = contract
    i = getattr(TC, point)
    assert not _model_valid(c)[i]
    assert not valid[i] and X[i].tobytes() == np.zeros(3).tobytes()


def test_a_nan_in_a_staged_matrix_nobody_observes_changes_nothing(contract):
    _, batch, harmless, _ = contract
    assert _same(batch, harmless)


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_outputs_and_the_blocks_alone(cases):
    L = _lib.load()
    c = cases["origin"]
    n = len(c["off"]) - 1
    P, off, cam, xy = (np.ascontiguousarray(c[k]) for k in TC.FIELDS)
    X, valid = np.full((n, 3), -777.25), np.full(n, 0xAB, np.uint8)
    X0, valid0 = X.tobytes(), valid.tobytes()
    shifted = off.copy()
    shifted[0] = 1
    gc.collect()
    base = live()

    def refused(message, **swap):
        a = {**dict(P=P, off=off, cam=cam, xy=xy, X=X, valid=valid), **swap}
        rc = L.l3d_triangulate_points(0, len(P), ptr(a["P"]), n, ptr(a["off"]), ptr(a["cam"]), ptr(a["xy"]), ptr(a["X"]), ptr(a["valid"]))
        assert rc == -1 and _lib.last_error() == message, (rc, _lib.last_error())
        assert X.tobytes() == X0 and valid.tobytes() == valid0
        gc.collect()
        assert live() == base

    refused("obs_offsets[0] is not 0", off=shifted)
    assert off[-1] > 0
    refused("null argument", cam=None)
    refused("null argument", xy=None)
    refused("null argument", P=None)
    refused("null argument", X=None)
    refused("null argument", valid=None)
    refused("null argument", off=None)
    with pytest.raises(ValueError, match="do not describe the same observations"):
        api.triangulate_points(P, off, cam, xy[:-1])
    with pytest.raises(ValueError, match="do not describe the same observations"):
        api.triangulate_points(P, off, cam[:-1], xy[:-1])
    gc.collect()
    assert live() == base
    # and the same arguments unrefused: the sentinels go
    assert L.l3d_triangulate_points(0, len(P), ptr(P), n, ptr(off), ptr(cam), ptr(xy), ptr(X), ptr(valid)) == 0
    assert _same((X, valid.astype(bool)), api.triangulate_points(P, off, cam, xy))
    gc.collect()
    assert live() == base
