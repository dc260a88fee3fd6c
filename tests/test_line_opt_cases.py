"""The model of the bundling solver (tests/line_opt_model.py: jacobian, lm_solve) and the case lines of
tests/line_opt_cases.py, on the CPU: the model's derivatives are right, its restated rule set finds optima, the cases
reach every stopping rule, and few enough of them are close calls for the GPU tests (tests/test_gpu_line_opt_solver.py) to
pin status and iteration count of nearly every line."""
import numpy as np
import pytest

from tests import line_opt_cases as Cs
from tests import line_opt_model as M

two_precisions = pytest.mark.skipif(not Cs.HAVE_LONG_DOUBLE, reason="np.longdouble is no wider than float64 on this platform")


def _every_line():
    """(batch name, index) of every case line"""
    return [(name, i) for name, b in Cs.all_batches().items() for i in range(len(b))]


def test_long_double_is_wider():
    assert Cs.HAVE_LONG_DOUBLE == (np.finfo(np.longdouble).eps < 1e-18)


def test_jacobian_matches_central_differences():
    """(a) on 300 generated residuals, at the 1e-6 relative of the evaluator test of tests/test_gpu_line_opt.py"""
    n = n_fold = n_out = 0
    for seed in range(30):
        x0, cams, obs, obs_cam = Cs.line_problem(1000 + seed, 10)
        for o, ci in zip(obs, obs_cam):
            c = cams[ci]
            ok, r = M.residual(x0, c, o)
            assert ok
            Jn = np.zeros((2, 4))
            for j in range(4):
                e = np.zeros(4); e[j] = 1e-6 * max(1.0, abs(x0[j]))
                Jn[:, j] = (M.residual(x0 + e, c, o)[1] - M.residual(x0 - e, c, o)[1]) / (2 * e[j])
            J = M.jacobian(x0, c, o)
            assert np.abs(J - Jn).max() <= 1e-6 * max(1.0, np.abs(Jn).max()), (seed, J, Jn)
            l, m = M.plucker(x0)
            q = c[0:9].reshape(3, 3) @ (m - np.cross(c[9:12], l))
            n_fold += (c[13] * q[0] * o[4] + c[12] * q[1] * o[5]) < 0
            n_out += r @ r > 4.0
            n += 1
    assert n == 300 and n_fold > 20 and n_out > 20, (n, n_fold, n_out)


def test_jacobian_rule_at_unit_dotp():
    """|dotp| = 1: the weight is 1 and its derivative 0 -> the Jacobian of the unweighted distances"""
    cam = M.camera(np.eye(3), np.zeros(3), np.eye(3))
    x = np.array([2.0, 0.0, 0.0, 1.0])
    for nx in (-1.0, 1.0):
        o = np.array([0.25, -3.0, 0.75, 4.0, nx, 0.0])
        Jn = np.zeros((2, 4))
        for j in range(4):
            e = np.zeros(4); e[j] = 1e-6
            Jn[:, j] = (M.residual(x + e, cam, o, False)[1] - M.residual(x - e, cam, o, False)[1]) / 2e-6
        J = M.jacobian(x, cam, o)
        assert np.all(np.isfinite(J)) and np.abs(J - Jn).max() <= 1e-6 * max(1.0, np.abs(Jn).max())


def test_model_never_ends_above_its_start():
    """(b)"""
    for name, i in _every_line():
        x, c0, c1, iters, status, _ = Cs.model_runs(name)[i]
        if status == M.OTHER and iters == 0:
            assert np.array_equal(x, Cs.all_batches()[name].x0[i])
            continue
        assert c1 <= c0, (name, i, c0, c1)
        assert c1 == pytest.approx(M.cost(x, *Cs.all_batches()[name].line(i)[1:]), rel=1e-11, abs=1e-11)


def test_model_reaches_scipys_optimum():
    """(c) the restated rule set finds optima: the thresholds of test_bundled_lines_reach_the_robust_optimum.  Lines with
    at least 3 observations: below that the problem is under-determined, the optimum is cost 0 and a relative gap says
    nothing"""
    lines = [(name, i) for name, i in _every_line()
             if name != "special" and Cs.all_batches()[name].counts()[i] >= 3]
    lines = lines[::max(1, len(lines) // 40)][:40]
    gaps = []
    for name, i in lines:
        x0, cams, obs = Cs.all_batches()[name].line(i)
        f1 = Cs.model_runs(name)[i][2]
        xs, fs, conv = M.minimise(x0, cams, obs)
        gaps.append((f1 - fs) / max(fs, 1e-300))
    gaps = np.array(gaps)
    print(f"{len(gaps)} lines against scipy: relative cost gap median {np.median(gaps):.3g} max {gaps.max():.3g}, "
          f"within 1e-9: {np.mean(gaps <= 1e-9):.3f}")
    assert len(gaps) == 40 and np.mean(gaps <= 1e-9) >= 0.75 and gaps.max() <= 1e-3


def test_cases_reach_every_stopping_rule():
    """(d)"""
    seen = {r[4] for name, _ in _every_line() for r in [Cs.model_runs(name)[_]]}
    for k in (1, 2, 3):
        runs = Cs.model_runs("special", k)
        assert all(r[3] <= k for r in runs)
        seen |= {r[4] for r in runs}
        assert any(r[4] == M.MAX_ITER for r in runs)
    assert seen >= {M.GRADIENT, M.FUNCTION, M.PARAMETER, M.MAX_ITER, M.OTHER}, seen
    sp = Cs.special_batch()
    runs = Cs.model_runs("special")
    for key in ("omega_0", "omega_5e-13"):
        x, c0, c1, iters, status, _ = runs[Cs.SPECIAL[key]]
        assert status == M.OTHER and iters == 0 and np.array_equal(x, sp.x0[Cs.SPECIAL[key]])
    x, c0, c1, iters, status, _ = runs[Cs.SPECIAL["zero"]]
    assert status == M.GRADIENT and iters == 0 and c0 == c1 == 0.0 and np.array_equal(x, sp.x0[Cs.SPECIAL["zero"]])
    rejected = {}
    for name, b in Cs.all_batches().items():
        for i in range(len(b)):
            trace = []
            run = M.lm_solve(*b.line(i), Cs.MAX_ITER, trace=trace)
            assert len(trace) == run[3] == Cs.model_runs(name)[i][3]
            rejected[name] = rejected.get(name, 0) + ("rejected" in trace)
    print("lines with a rejected step:", {k: v for k, v in rejected.items() if v})
    assert sum(rejected[name] for name in Cs.iteration_batches()) >= 1      # among the lines the GPU run is held to


@two_precisions
def test_few_close_calls():
    """(e) the cap: in every batch of the GPU tests, and at every max_iter they compare statuses at, the close-call lines
    -- the only ones excused from exact status and iteration count on the GPU -- are at most 5 % of the lines and never
    more than 3"""
    total = 0
    for name, b in Cs.all_batches().items():
        cc = Cs.close_calls(name)
        print(name, len(b), "lines, close calls:", cc)
        assert len(cc) <= Cs.cap(len(b)), (name, cc)
        total += len(cc)
    for k in (1, 2, 3):
        assert len(Cs.close_calls("special", k)) <= Cs.cap(len(Cs.special_batch()))
    measured = Cs.model_rounding()
    print("close calls in all batches:", total, "; fp64 against long double on the compared lines:", measured)
    from tests.test_gpu_line_opt_solver import MODEL_ROUNDING
    assert 0.5 * MODEL_ROUNDING <= measured <= 1.01 * MODEL_ROUNDING, (measured, MODEL_ROUNDING)
