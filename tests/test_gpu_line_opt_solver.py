"""The bundling solver on its own (l3d_line_opt_solve: k_lineopt.hip through the function the pipeline's stage calls) on the
MI355X, at its lane tiers, past one chunk of the wave tier, at every stopping rule and at the edges of its grid.  Most of
the weight is on checks without a tolerance (a batch against its singletons, the 16-lane tier against the wave tier, the
lines that must come back untouched); the iteration itself is compared with the restated rule set of
tests/line_opt_model.py (lm_solve), exactly in status and iteration count for every line that is no close call
(tests/line_opt_cases.py; tests/test_line_opt_cases.py holds their number down on the CPU)."""
import numpy as np
import pytest

from line3dpp_amd import _lib, api
from tests import line_opt_cases as Cs
from tests import line_opt_model as M

pytestmark = pytest.mark.gpu

# Largest relative difference between the model's own fp64 and long double runs over the compared lines (Cs.iteration_batches():
# the counts batch and two grid batches, close calls left out), in x (max-norm over max(1, |x|_inf)) and in cost1 (over
# max(1, cost1)).  Recompute on any CPU with an 80-bit long double:
#     python -c "from tests import line_opt_cases as Cs; print(Cs.model_rounding())"
# T = 100 x that: the factor covers what the two model runs do not differ in (the kernel sums in a tree, the device's exp /
# acos / sqrt may differ from numpy's by an ulp).  Neither number comes from the kernel's output;
# tests/test_line_opt_cases.py measures again and holds the constant to it.
MODEL_ROUNDING = 4.232e-8
T = 100 * MODEL_ROUNDING
L3D_ERR_ARG = -1

BATCHES = sorted(Cs.all_batches())


def solve(b, max_iter=Cs.MAX_ITER, narrow_max=16):
    return api.line_opt_solve(b.x0, b.res_off, b.obs, b.obs_cam, b.cams, max_iter, narrow_max)


def bits(res, i):
    """line i of a result as bytes: (x, cost0, cost1, iters, status)"""
    return b"".join(np.ascontiguousarray(a[i]).tobytes() for a in res)


def assert_same_lines(res_a, idx_a, res_b, idx_b, what):
    for i, j in zip(idx_a, idx_b):
        assert bits(res_a, i) == bits(res_b, j), (what, i, j, [a[i] for a in res_a], [a[j] for a in res_b])


# ---- 1. a batch equals its singletons ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BATCHES)
def test_a_batch_equals_its_singletons(name):
    """The tier and the lane mapping of a line do not depend on its neighbours, so a line solved in a batch and alone must
    agree in every bit: a shuffle that crosses a 16-lane group, a wrong slot of the work order, a grid edge or a group
    that stops early and disturbs its wave would show here.  The same for the batch in another input order."""
    b = Cs.all_batches()[name]
    n = len(b)
    whole = solve(b)
    for i in range(n):
        assert_same_lines(whole, [i], solve(b.take([i])), [0], f"{name}: line {i} alone")
    perm = np.random.default_rng(7).permutation(n)
    assert_same_lines(whole, perm, solve(b.take(perm)), range(n), f"{name}: shuffled")
    by_count = np.argsort(-b.counts(), kind="stable")
    assert_same_lines(whole, by_count, solve(b.take(by_count)), range(n), f"{name}: sorted")


def test_counts_batch_equals_its_singletons_in_the_wave_tier():
    b = Cs.counts_batch()
    whole = solve(b, narrow_max=0)
    for i in range(len(b)):
        assert_same_lines(whole, [i], solve(b.take([i]), narrow_max=0), [0], f"line {i} alone, wave tier")


# ---- 2. the narrow tier equals the wave tier ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", BATCHES)
def test_the_narrow_tier_equals_the_wave_tier(name):
    """A line with at most 16 residuals gives the same bits from a 16-lane group (narrow_max = 16) and from a whole wave
    (narrow_max = 0).  In the wave, lanes 16 .. 63 have no residual and hold exact zeros; the first two xor stages (32, 16)
    add 0.0 to the sums of lanes 0 .. 15, which changes no bit, and the other four stages (8, 4, 2, 1) are the 16-lane
    group's tree.  Everything after the sums is the same code on the same numbers, and the library is built with
    -ffp-contract=off, so the two instantiations cannot differ by a fused multiply-add."""
    b = Cs.all_batches()[name]
    narrow, wide = solve(b, narrow_max=16), solve(b, narrow_max=0)
    # (the lines with more than 16 residuals take a wave in both calls, with other neighbours: they must agree as well)
    assert_same_lines(narrow, range(len(b)), wide, range(len(b)), f"{name}: 16 lanes against a wave")


def test_the_tier_comparison_sees_short_lines():
    assert sum(int((b.counts() <= 16).sum()) for b in Cs.all_batches().values()) > 100


# ---- 3. special lines ------------------------------------------------------------------------------------------------

def test_lines_that_must_come_back_untouched():
    """a start that cannot be evaluated keeps its parameters (status other, no iteration); a line without residuals has
    cost 0 and gradient 0.  Both sit inside waves of ordinary narrow lines (test_a_batch_equals_its_singletons covers
    their neighbours)"""
    b = Cs.special_batch()
    for narrow_max in (16, 0):
        x, c0, c1, iters, status = solve(b, narrow_max=narrow_max)
        for key in ("omega_0", "omega_5e-13"):
            i = Cs.SPECIAL[key]
            assert x[i].tobytes() == b.x0[i].tobytes() and iters[i] == 0 and status[i] == M.OTHER, (key, x[i], iters[i], status[i])
        i = Cs.SPECIAL["zero"]
        assert x[i].tobytes() == b.x0[i].tobytes() and c0[i] == 0.0 and c1[i] == 0.0 and iters[i] == 0 and status[i] == M.GRADIENT
        i = Cs.SPECIAL["exact"]
        m = Cs.model_runs("special")[i]
        if i not in Cs.close_calls("special"):
            assert (iters[i], status[i]) == (m[3], m[4])


@pytest.mark.parametrize("name", ["special", "counts"])
def test_max_iter_zero_returns_the_start(name):
    b = Cs.all_batches()[name]
    x, c0, c1, iters, status = solve(b, max_iter=0)
    assert x.tobytes() == b.x0.tobytes() and c1.tobytes() == c0.tobytes() and not iters.any()
    assert list(status) == [r[4] for r in Cs.model_runs(name, 0)]


@pytest.mark.parametrize("max_iter", [1, 2, 3])
@pytest.mark.parametrize("name", ["special", "counts"])
def test_iteration_limit(name, max_iter):
    b = Cs.all_batches()[name]
    x, c0, c1, iters, status = solve(b, max_iter=max_iter)
    model = Cs.model_runs(name, max_iter)
    excused = set(Cs.close_calls(name, max_iter))
    assert len(excused) <= Cs.cap(len(b))
    assert np.all(iters <= max_iter)
    hit = 0
    for i, m in enumerate(model):
        if i not in excused:
            assert (status[i] == M.MAX_ITER) == (m[4] == M.MAX_ITER) and status[i] == m[4] and iters[i] == m[3], (i, status[i], iters[i], m)
            hit += m[4] == M.MAX_ITER
    assert hit > 0


# ---- 4. sums past one chunk ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("narrow_max", [16, 0])
def test_start_cost_at_every_count(narrow_max):
    """the wave tier's loop over 64-residual chunks takes 2, 3 and 4 trips here (65, 129, 152, 200 residuals): the start
    cost against the model's, at the bound of the evaluator test"""
    b = Cs.counts_batch()
    x, c0, c1, iters, status = solve(b, max_iter=0, narrow_max=narrow_max)
    for i in range(len(b)):
        want = M.cost(*b.line(i))
        print(f"{int(b.counts()[i])} residuals: cost0 {c0[i]!r} model {want!r}")
        assert abs(c0[i] - want) <= 1e-11 * max(1.0, want), (int(b.counts()[i]), c0[i], want)


# ---- 5. the iteration, 6. the reported cost ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(Cs.iteration_batches()) + sorted(Cs.status_batches()))
def test_the_iteration_follows_the_rules(name):
    """status and iteration count are the fp64 model's for every line that is no close call, and the cost within T; in
    the batches T was measured on (Cs.iteration_batches()) the parameters within T as well.  (The other batches hold
    a line of 2 residuals that the model itself moves by 3e-6 between fp64 and long double over its 130 iterations.)"""
    b = Cs.all_batches()[name]
    x, c0, c1, iters, status = solve(b)
    model = Cs.model_runs(name)
    excused = Cs.close_calls(name)
    print(f"{name}: {len(b)} lines, close calls {excused}")
    assert len(excused) <= Cs.cap(len(b))
    worst_x = worst_c = 0.0
    for i, (mx, mc0, mc1, mit, mst, _) in enumerate(model):
        if i in excused:
            assert c1[i] <= c0[i] * (1 + 1e-9) + 1e-12
            assert abs(c1[i] - mc1) <= 1e-3 * max(mc1, M.TINY), (i, c1[i], mc1)
            continue
        assert (status[i], iters[i]) == (mst, mit), (i, int(b.counts()[i]), status[i], iters[i], mst, mit)
        dx = np.abs(x[i] - mx).max() / max(1.0, np.abs(mx).max())
        dc = abs(c1[i] - mc1) / max(1.0, mc1)
        worst_x, worst_c = max(worst_x, dx), max(worst_c, dc)
        assert dc <= T, (i, int(b.counts()[i]), dc, T)
        assert dx <= T or name not in Cs.iteration_batches(), (i, int(b.counts()[i]), dx, T)
    print(f"{name}: against the fp64 model: x {worst_x:.3g}, cost1 {worst_c:.3g} (T = {T:.3g})")


@pytest.mark.parametrize("name", BATCHES)
def test_the_reported_cost_is_the_cost(name):
    b = Cs.all_batches()[name]
    x, c0, c1, iters, status = solve(b)
    solved = 0
    for i in range(len(b)):
        if status[i] == M.OTHER and iters[i] == 0:
            continue                                   # a start that cannot be evaluated has no cost
        want = M.cost(x[i], *b.line(i)[1:])
        assert abs(c1[i] - want) <= 1e-11 * max(1.0, want), (i, c1[i], want)
        assert c1[i] <= c0[i]
        solved += 1
    assert solved >= len(b) - 2


# ---- 7. the entry ------------------------------------------------------------------------------------------------------

def test_the_entry_refuses_bad_arguments_and_writes_nothing():
    L = _lib.load()
    b = Cs.grid_batch(1, 1)
    n = len(b)
    x0, off, obs, cam, cams = (np.ascontiguousarray(a) for a in (b.x0, b.res_off, b.obs, b.obs_cam, b.cams))

    def call(n_lines=n, x0=x0, off=off, obs=obs, cam=cam, n_cams=len(cams), cams=cams, narrow_max=16, null_out=None):
        out = [np.full((n, 4), -7.0), np.full((n, 2), -7.0), np.full(n, 77, np.uint32), np.full(n, 77, np.uint32)]
        keep = [a.copy() for a in out]
        p = [_lib.ptr(a) for a in out]
        if null_out is not None:
            p[null_out] = None
        rc = L.l3d_line_opt_solve(0, n_lines, _lib.ptr(x0), _lib.ptr(off), _lib.ptr(obs), _lib.ptr(cam), n_cams, _lib.ptr(cams),
                                  50, narrow_max, *p)
        return rc, all(np.array_equal(a, k) for a, k in zip(out, keep))

    assert call()[0] == 0 and not call()[1]
    assert call(n_lines=0) == (0, True)
    assert L.l3d_line_opt_solve(0, 0, None, None, None, None, 0, None, 50, 16, None, None, None, None) == 0
    for kw in (dict(x0=None), dict(off=None), dict(obs=None), dict(cam=None), dict(cams=None), dict(null_out=0),
               dict(null_out=1), dict(null_out=2), dict(null_out=3)):
        assert call(**kw) == (L3D_ERR_ARG, True), kw
    down = off.copy(); down[1], down[2] = down[2], down[1]
    assert down[2] < down[1] and call(off=down) == (L3D_ERR_ARG, True)
    late = off.copy(); late[0] = 1
    assert call(off=late) == (L3D_ERR_ARG, True)
    bad = cam.copy(); bad[-1] = len(cams)
    assert call(cam=bad) == (L3D_ERR_ARG, True)
    assert call(n_cams=int(cam.max())) == (L3D_ERR_ARG, True)
    assert call(narrow_max=17) == (L3D_ERR_ARG, True)
    assert call(narrow_max=16)[0] == 0 and call(narrow_max=0)[0] == 0
