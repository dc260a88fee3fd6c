"""Line bundling (use_CERES), host side: the parametrisation and write-back of LineOptimizer::optimize
(optimization.cc:31-95, 209-295) as the library computes them (l3d_line_to_cayley / l3d_cayley_to_segment) against the
independent numpy model of tests/line_opt_model.py; and the C++ driver of the facade's bundled path builds and links."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from line3dpp_amd import _lib
from tests import line_opt_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _to_cayley(P1, P2):
    L = _lib.load()
    x = np.zeros(4)
    rc = L.l3d_line_to_cayley(_lib.ptr(np.asarray(P1, np.float64)), _lib.ptr(np.asarray(P2, np.float64)), _lib.ptr(x))
    assert rc in (0, 1)
    return x, rc == 1


def _write_back(x, P1, P2):
    L = _lib.load()
    a = np.zeros(3); b = np.zeros(3)
    rc = L.l3d_cayley_to_segment(_lib.ptr(np.asarray(x, np.float64)), _lib.ptr(np.asarray(P1, np.float64)),
                                 _lib.ptr(np.asarray(P2, np.float64)), _lib.ptr(a), _lib.ptr(b))
    assert rc in (0, 1)
    return a, b, rc == 1


def _close(a, b, rel):
    return np.abs(a - b).max() <= rel * max(1.0, np.abs(b).max())


def _same_infinite_line(P1, P2, Q1, Q2, rel):
    d1, o1 = M.infinite_line(P1, P2)
    d2, o2 = M.infinite_line(Q1, Q2)
    scale = max(1.0, np.abs(np.concatenate([P1, P2])).max())
    return np.abs(d1 - d2).max() <= rel and np.abs(o1 - o2).max() <= rel * scale


def test_cayley_of_random_lines_matches_model_and_round_trips():
    rng = np.random.default_rng(11)
    n = 0
    for _ in range(500):
        P1 = rng.normal(0, 5, 3); P2 = P1 + rng.normal(0, 2, 3)
        x, const = _to_cayley(P1, P2)
        xm, cm = M.to_cayley(P1, P2)
        assert const == cm
        if const:
            continue
        assert _close(x, xm, 1e-12), (x, xm)
        # the write-back of the unchanged parameters re-expresses the same infinite line
        Q1, Q2, kept = _write_back(x, P1, P2)
        assert kept and _same_infinite_line(P1, P2, Q1, Q2, 1e-12)
        R1, R2, kept_m = M.write_back(xm, P1, P2)
        assert kept_m and _close(Q1, R1, 1e-12) and _close(Q2, R2, 1e-12)
        n += 1
    assert n > 450


def test_line_through_origin_takes_the_full_pivot_lu_kernel():
    n_free = 0
    for P1, P2 in [((1.0, 2.0, 3.0), (-1.0, -2.0, -3.0)), ((0.3, -0.2, 0.1), (-0.3, 0.2, -0.1)),
                   ((2.0, 0.0, 0.0), (-2.0, 0.0, 0.0)), ((0.0, 1.0, 1.0), (0.0, -1.0, -1.0))]:
        x, const = _to_cayley(P1, P2)
        xm, cm = M.to_cayley(P1, P2)
        assert const == cm
        if const:
            assert np.array_equal(x, [-1.0, 0.0, 0.0, 0.0])
        else:
            assert abs(x[0]) < M.EPS and _close(x, xm, 1e-12), (P1, x, xm)      # omega = |m| = 0
            n_free += 1
        # omega below L3D_EPS: the write-back keeps the old end points
        Q1, Q2, kept = _write_back(x, P1, P2)
        assert kept and np.array_equal(Q1, P1) and np.array_equal(Q2, P2)
    assert n_free >= 2
    # the kernel vectors are not orthonormal, the model's (Eigen's) choice: e.g. l = (1, 2, 3) / |.|, pivot z
    l = np.array([1.0, 2.0, 3.0]) / np.linalg.norm([1.0, 2.0, 3.0])
    x, _ = _to_cayley(-l, l)
    assert np.all(np.isfinite(x)) and not np.allclose(x[1:], 0)


def test_symmetric_line_is_held_constant():
    # e.g. l = (-1, 0, 0), m = (0, -1, 0): Q = diag(-1, -1, 1), Q + I singular -> NaN in the Cayley form
    for P1, P2 in [((0.5, 0.0, 1.0), (-0.5, 0.0, 1.0)), ((0.0, 0.5, -1.0), (0.0, -0.5, -1.0)),
                   ((-1.0, 0.0, 0.5), (-1.0, 0.0, -0.5))]:
        xm, cm = M.to_cayley(P1, P2)
        x, const = _to_cayley(P1, P2)
        assert cm and const and np.array_equal(x, [-1.0, 0.0, 0.0, 0.0])
        Q1, Q2, kept = _write_back(x, P1, P2)
        assert kept and np.array_equal(Q1, P1) and np.array_equal(Q2, P2)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_write_back_branches(axis):
    """the three intersection branches (largest |l| component), against the model, for moved parameters"""
    rng = np.random.default_rng(20 + axis)
    for _ in range(50):
        d = rng.normal(0, 0.2, 3); d[axis] = 1.0 if rng.random() < 0.5 else -1.0
        P1 = rng.normal(0, 4, 3); P2 = P1 + 3.0 * d
        x, const = _to_cayley(P1, P2)
        assert not const
        y = x + rng.normal(0, 1e-3, 4) * np.array([abs(x[0]), 1, 1, 1])
        l, _ = M.plucker(y)
        assert np.argmax(np.abs(l)) == axis
        Q1, Q2, kept = _write_back(y, P1, P2)
        R1, R2, kept_m = M.write_back(y, P1, P2)
        assert kept and kept_m and _close(Q1, R1, 1e-12) and _close(Q2, R2, 1e-12)
        # the new mid point lies in the plane of the old one along that axis, the new line is the line of y
        assert abs(0.5 * (Q1 + Q2)[axis] - 0.5 * (P1 + P2)[axis]) <= 1e-12 * max(1.0, np.abs(P1 + P2).max())
        ln, mn = M.plucker(y)
        assert np.abs(np.cross(0.5 * (Q1 + Q2), ln) - mn).max() <= 1e-11 * max(1.0, np.abs(Q1).max())


def test_write_back_drops_degenerate_cluster():
    P = np.array([1.0, 2.0, 3.0])
    _, _, kept = _write_back(np.array([-1.0, 0, 0, 0]), P, P)
    assert not kept


def test_cpp_line_opt_driver_builds_and_links(tmp_path):
    """tests/cpp/line_opt_driver.cpp: reconstruct3Dlines(3, false, -1, true, 50) through the C++ facade (run on the
    GPU box by tests/test_gpu_line_opt.py)"""
    exe = str(tmp_path / "line_opt_driver")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "line_opt_driver.cpp"), "-o", exe, "-L" + lib_dir,
                           "-ll3dpp_hip", "-Wl,-rpath," + lib_dir])
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libl3dpp_hip" in out and "not found" not in out
