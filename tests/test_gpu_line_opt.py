"""Line bundling on the MI355X (reconstruct3Dlines(use_CERES=True); k_lineopt.hip), checked against the independent numpy
model of tests/line_opt_model.py (the reference's LineReprojectionError, HuberLoss(2), parametrisation and write-back) and
scipy's minimiser of the same robust cost."""
import hashlib
import lzma
import os
import subprocess
import struct

import numpy as np
import pytest

from line3dpp_amd import _lib
from line3dpp_amd.api import Line3D
from line3dpp_amd.scene import make_config
from tests import line_opt_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_full", "kNN_10__OPTIMIZED__vis_3.bin.xz")
# get3Dlines() of reconstruct3Dlines(3) on the parent commit of the bundling stage (before it existed): digest below
PARENT_DIGEST = {
    "golden": "3a3e7596bc851518c08e3a2998317b8866d6757f0f56cd675c502787d6b035d7",
    "C0": "06a9ee7ee50252f639ccc4a3e9c5e18173ea87c8a81560315a72b137a582aac6",
}


def lines_digest(lines):
    h = hashlib.sha256()
    h.update(np.uint64(len(lines)).tobytes())
    for L in lines:
        for k in ("collinear3Dsegments", "residuals"):
            a = np.ascontiguousarray(L[k]); h.update(np.uint64(len(a)).tobytes()); h.update(a.tobytes())
        h.update(np.ascontiguousarray(L["cluster_line"]).tobytes()); h.update(np.uint32(L["reference_view"]).tobytes())
    return h.hexdigest()


def _scene(name):
    if name == "golden":
        from tests.golden.make_golden import PARAMS, golden_scene
        return golden_scene(), dict(sigma_position=PARAMS["sigma_p"], sigma_angle=PARAMS["sigma_a"], kNN=PARAMS["kNN"],
                                    epipolar_overlap=PARAMS["epi_overlap"])
    return make_config(name), {}


def _run(sc, kw, **rk):
    g = Line3D()
    g.add_scene(sc)
    assert g.matchImages(**kw)
    assert g.reconstruct3Dlines(3, **rk)
    return g


def _key(L):
    return frozenset(map(tuple, np.stack([L["residuals"]["cam"], L["residuals"]["seg"]], 1).tolist()))


def _cams(sc):
    """camera rows of the model, original frame (C = -R^T t)"""
    out = {}
    for v in sc.views:
        R = np.asarray(v.R, np.float64); t = np.asarray(v.t, np.float64)
        out[v.cam] = M.camera(R, -R.T @ t, v.K)
    return out


def _problem(sc, cams, L):
    segs = {v.cam: v.segs for v in sc.views}
    c = [cams[int(r["cam"])] for r in L["residuals"]]
    o = [M.observation(segs[int(r["cam"])][int(r["seg"])]) for r in L["residuals"]]
    return c, o


def _extent(lines):
    pts = np.concatenate([np.stack([L["cluster_line"]["P1"], L["cluster_line"]["P2"]]) for L in lines], 0)
    return float(np.linalg.norm(np.percentile(pts, 95, axis=0) - np.percentile(pts, 5, axis=0)))


# ---- 3. the evaluator -----------------------------------------------------------------------------------------------

def _eval(x, cams, obs):
    L = _lib.load()
    n = len(obs)
    cost = np.zeros(1); r = np.zeros(2 * n); J = np.zeros(8 * n); ok = np.zeros(n, np.int32)
    rc = L.l3d_line_opt_eval(0, n, _lib.ptr(np.asarray(x, np.float64)), _lib.ptr(np.ascontiguousarray(obs, np.float64)),
                             _lib.ptr(np.ascontiguousarray(cams, np.float64)), _lib.ptr(cost), _lib.ptr(r), _lib.ptr(J),
                             _lib.ptr(ok))
    assert rc == 0, _lib.last_error()
    return float(cost[0]), r.reshape(n, 2), J.reshape(n, 2, 4), ok.astype(bool)


def _central(x, cam, obs, h=1e-6, angle_weight=True):
    J = np.zeros((2, 4))
    for j in range(4):
        e = np.zeros(4); e[j] = h * max(1.0, abs(x[j]))
        a = M.residual(x + e, cam, obs, angle_weight)[1]; b = M.residual(x - e, cam, obs, angle_weight)[1]
        J[:, j] = (a - b) / (2 * e[j])
    return J


def test_evaluator_matches_model_on_all_branches():
    rng = np.random.default_rng(3)
    sc = make_config("C0")
    cams_by = _cams(sc)
    cam_ids = sorted(cams_by)
    xs, cams, obs = [], [], []
    # real geometry: lines in front of the cameras, observations near and far from the projection (Huber in and out),
    # segment directions either way round (angle folded or not)
    for k in range(300):
        c = cams_by[cam_ids[k % len(cam_ids)]]
        R = c[0:9].reshape(3, 3); C = c[9:12]
        P1 = C + R.T @ np.array([rng.normal(0, 1), rng.normal(0, 1), rng.uniform(4, 10)])
        P2 = P1 + R.T @ np.array([rng.normal(0, 1), rng.normal(0, 1), rng.normal(0, 0.3)])
        x, const = M.to_cayley(P1, P2)
        if const:
            continue
        K = np.array([[c[12], 0, c[14]], [0, c[13], c[15]], [0, 0, 1]])
        p = [K @ (R @ (P - C)) for P in (P1, P2)]
        p = [q[:2] / q[2] for q in p]
        noise = rng.normal(0, 0.5 if k % 2 else 20.0, 4)
        seg = np.concatenate([p[0], p[1]]) + noise
        if k % 3 == 0:
            seg = np.concatenate([seg[2:], seg[:2]])
        xs.append(x); cams.append(c); obs.append(M.observation(seg))
    n_in = n_out = n_fold = 0
    for x, c, o in zip(xs, cams, obs):
        cost, r, J, ok = _eval(x, [c], [o])
        okm, rm = M.residual(x, c, o)
        assert ok[0] and okm
        scale = max(1.0, np.abs(rm).max())
        assert np.abs(r[0] - rm).max() <= 1e-12 * scale * 10, (r[0], rm)
        s = rm @ rm
        assert abs(cost - 0.5 * M.huber(s)) <= 1e-11 * max(1.0, cost)
        n_in += s <= 4.0; n_out += s > 4.0
        l, m = M.plucker(x)
        Jn = _central(x, c, o)
        assert np.abs(J[0] - Jn).max() <= 1e-6 * max(1.0, np.abs(Jn).max()), (J[0], Jn)
        # folded angle: the image line's normal points away from the segment's
        R = c[0:9].reshape(3, 3); q = R @ (m - np.cross(c[9:12], l))
        n_fold += (c[13] * q[0] * o[4] + c[12] * q[1] * o[5]) < 0
    assert n_in > 20 and n_out > 20 and n_fold > 20, (n_in, n_out, n_fold)


def test_evaluator_rule_at_unit_dotp_and_failures():
    # R = I, C = 0, fx = fy = 1, px = py = 0; x = (omega, 0, 0, 1): l = (0, 0, 1)... m = (-omega, 0, 0) -> image line
    # (-omega, 0, 0): its normal is exactly +-(1, 0), dotp exactly +-1 against a segment normal (+-1, 0)
    cam = M.camera(np.eye(3), np.zeros(3), np.eye(3))
    x = np.array([2.0, 0.0, 0.0, 1.0])
    for nx in (-1.0, 1.0):                   # dotp = +1 (angle 0) and -1 (angle pi, folded to 0)
        o = np.array([0.25, -3.0, 0.75, 4.0, nx, 0.0])
        cost, r, J, ok = _eval(x, [cam], [o])
        okm, rm = M.residual(x, cam, o)
        assert ok[0] and okm and np.array_equal(r[0], rm) and np.allclose(rm, [-0.25, -0.75])
        # the stated rule: weight 1, its derivative 0 -> the Jacobian of the unweighted distances
        Jd = _central(x, cam, o, angle_weight=False)
        assert np.all(np.isfinite(J[0])) and np.abs(J[0] - Jd).max() <= 1e-6 * max(1.0, np.abs(Jd).max()), (J[0], Jd)
    # failures: |omega| < 1e-12; projected line of zero length (x = (omega, 1, 0, 0): m = (0, 0, omega), q = (0, 0, omega))
    o = np.array([0.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    for xf in (np.array([0.0, 0.1, 0.2, 0.3]), np.array([5e-13, 0.1, 0.2, 0.3]), np.array([1.0, 1.0, 0.0, 0.0])):
        cost, r, J, ok = _eval(xf, [cam], [o])
        okm, _ = M.residual(xf, cam, o)
        assert not ok[0] and not okm and np.all(r == 0)


# ---- 4. optimum, 5. no change when off -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["golden", "C0"])
def test_bundled_lines_reach_the_robust_optimum(name):
    sc, kw = _scene(name)
    off = _run(sc, kw).get3Dlines()
    g = _run(sc, kw, use_CERES=True, max_iter_CERES=250)
    st = g.lineOptStats()
    on = g.get3Dlines()
    print(name, st)
    assert st["lines_bundled"] + st["lines_constant"] >= len(on) > 0
    assert (st["stop_gradient"] + st["stop_function"] + st["stop_parameter"] + st["stop_max_iter"] + st["stop_other"]
            == st["lines_bundled"])
    assert 0 < st["max_iterations"] <= 250 and st["cost_after"] <= st["cost_before"]
    cams = _cams(sc)
    start = {_key(L): L for L in off}
    extent = _extent(off)
    step = max(1, len(on) // 60)
    gaps, dist = [], []
    for i, L in enumerate(on):
        k = _key(L)
        if k not in start:
            continue
        c, o = _problem(sc, cams, L)
        cl0, cl1 = start[k]["cluster_line"], L["cluster_line"]
        x0, const = M.to_cayley(cl0["P1"], cl0["P2"])
        x1, _ = M.to_cayley(cl1["P1"], cl1["P2"])
        if const:
            continue
        f0, f1 = M.cost(x0, c, o), M.cost(x1, c, o)
        assert f1 <= f0 * (1 + 1e-9) + 1e-12, (i, f0, f1)      # never worse than the start
        if i % step:
            continue
        xs, fs, conv = M.minimise(x0, c, o)
        gap = (f1 - fs) / max(fs, 1e-300)
        gaps.append(gap)
        if conv and gap <= 1e-9:
            ls, ms = M.plucker(xs)
            Ps = np.cross(ls, ms) / (ls @ ls)                  # the point of the scipy line closest to the origin
            d1, o1 = M.infinite_line(cl1["P1"], cl1["P2"])
            d2 = ls / np.linalg.norm(ls)
            d2 = d2 if d2[np.argmax(np.abs(d2))] > 0 else -d2
            dist.append(max(np.abs(d1 - d2).max(), np.abs(o1 - Ps).max() / extent))
    gaps, dist = np.array(gaps), np.array(dist)
    print(f"{name}: {len(gaps)} lines against scipy: relative cost gap median {np.median(gaps):.3g} p90 "
          f"{np.percentile(gaps, 90):.3g} max {gaps.max():.3g}, within 1e-9: {np.mean(gaps <= 1e-9):.3f}; "
          f"line distance (scipy converged, gap <= 1e-9) max {dist.max() if len(dist) else 0:.3g} over {len(dist)}")
    # The per-line stop follows the reference solver's function tolerance (|cost change| <= 1e-6 cost), so a line may
    # stop slightly above the optimum: most lines are at scipy's optimum to 1e-9, all within 1e-3.
    assert len(gaps) >= min(40, len(on)) and np.mean(gaps <= 1e-9) >= 0.75 and gaps.max() <= 1e-3
    assert len(dist) >= 10 and dist.max() <= 1e-6


@pytest.mark.parametrize("name", ["golden", "C0"])
def test_off_is_byte_identical_to_the_parent(name):
    sc, kw = _scene(name)
    g = _run(sc, kw)
    assert lines_digest(g.get3Dlines()) == PARENT_DIGEST[name]
    assert g.lineOptStats()["lines_bundled"] == 0


def test_max_iter_zero_re_expresses_the_same_lines():
    sc, kw = _scene("C0")
    off = _run(sc, kw).get3Dlines()
    g = _run(sc, kw, use_CERES=True, max_iter_CERES=0)
    on = g.get3Dlines()
    st = g.lineOptStats()
    assert st["max_iterations"] == 0 and st["lines_dropped"] == 0
    assert [_key(L) for L in on] == [_key(L) for L in off]
    extent = _extent(off)
    worst = 0.0
    for a, b in zip(on, off):
        assert len(a["collinear3Dsegments"]) == len(b["collinear3Dsegments"])
        for s, t in zip(a["collinear3Dsegments"], b["collinear3Dsegments"]):
            p = np.concatenate([s["P1"], s["P2"]]); q = np.concatenate([t["P1"], t["P2"]])
            worst = max(worst, min(np.abs(p - q).max(), np.abs(p - np.concatenate([q[3:], q[:3]])).max()) / extent)
    assert worst <= 1e-9, worst


# ---- 6. writers, 7. the reference's bundled fixture ------------------------------------------------------------------

def test_bundled_writers_and_reference_fixture(tmp_path):
    from line3dpp_amd.io import read_3d_lines_bin
    sc, kw = _scene("C0")
    off = _run(sc, kw).get3Dlines()
    g = _run(sc, kw, use_CERES=True)
    name = "Line3D++__W_FULL__N_10__sigmaP_2.5__sigmaA_10__epiOverlap_0.25__kNN_10__OPTIMIZED__vis_3"
    assert g.outputFilename() == name
    assert g.save3DLinesAsTXT(tmp_path) and g.save3DLinesAsBIN(tmp_path)
    assert sorted(p.name for p in tmp_path.iterdir()) == [name + ".bin", name + ".txt"]
    on = g.get3Dlines()
    binl, version = read_3d_lines_bin(tmp_path / (name + ".bin"))
    assert version == 10 and len(binl) == len(on)
    for a, b in zip(binl, on):
        assert np.array_equal(a["cluster_line"][:6], np.concatenate([b["cluster_line"]["P1"], b["cluster_line"]["P2"]]))
    # the reference's bundled result: match lines by residual set; report end point distances, assert coverage only
    fx = tmp_path / "fixture.bin"
    with lzma.open(FIXTURE) as src:
        fx.write_bytes(src.read())
    ref, _ = read_3d_lines_bin(fx)
    # the fixture's segment ids -> the scene's (tests/golden/make_real_scene.py keeps the fixture's segments only)
    d = np.load(os.path.join(ROOT, "tests", "golden", "real_scene_c0.npz"))
    ids = {}
    for i, cam in enumerate(d["cam"]):
        for k, s in enumerate(d["orig_seg"][d["seg_off"][i]:d["seg_off"][i + 1]]):
            ids[(int(cam), int(s))] = (int(cam), k)
    rk = {}
    for L in ref:
        res = [ids.get(tuple(r)) for r in L["residuals"].tolist()]
        if None not in res:
            rk[frozenset(res)] = L
    extent = _extent(off)

    def dists(lines):
        d = []
        for L in lines:
            R = rk.get(_key(L))
            if R is None:
                continue
            p = np.concatenate([L["cluster_line"]["P1"], L["cluster_line"]["P2"]]); q = R["cluster_line"][:6]
            d.append(min(np.abs(p - q).max(), np.abs(p - np.concatenate([q[3:], q[:3]])).max()) / extent)
        return np.array(d)

    d_on, d_off = dists(on), dists(off)
    coverage = len(set(rk) & {_key(L) for L in on}) / len(rk)
    print(f"fixture coverage {coverage:.3f} ({len(rk)} lines); cluster line end points / extent {extent:.3g}: bundled "
          f"median {np.median(d_on):.3g} p90 {np.percentile(d_on, 90):.3g}; un-bundled median {np.median(d_off):.3g} "
          f"p90 {np.percentile(d_off, 90):.3g}")
    # measured on the MI355X: 0.389 (the other fixture lines have residual sets that differ by a segment or more)
    assert coverage > 0.3


# ---- 8. the facade ---------------------------------------------------------------------------------------------------

def test_facade_bundles_lines(tmp_path):
    exe = str(tmp_path / "line_opt_driver")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "line_opt_driver.cpp"), "-o", exe, "-L" + lib_dir,
                           "-ll3dpp_hip", "-Wl,-rpath," + lib_dir])
    sc = make_config("C0")
    path = str(tmp_path / "scene.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", sc.n_views))
        for v in sc.views:
            f.write(struct.pack("<5I", v.cam, len(v.segs), v.width, v.height, len(v.neighbors)))
            f.write(np.ascontiguousarray(v.K, np.float64).tobytes()); f.write(np.ascontiguousarray(v.R, np.float64).tobytes())
            f.write(np.ascontiguousarray(v.t, np.float64).tobytes()); f.write(struct.pack("<f", v.median_depth))
            f.write(np.asarray(v.neighbors, np.uint32).tobytes()); f.write(np.ascontiguousarray(v.segs, np.float32).tobytes())
    out = subprocess.check_output([exe, path], timeout=600).decode()
    assert "#unoptimizable_lines = " in out
    kv = dict(x.split("=") for x in [l for l in out.splitlines() if l.startswith("RESULT")][0].split()[1:])
    assert int(kv["common"]) > 0.9 * int(kv["lines_on"]) > 1000
    assert int(kv["moved"]) > 0.9 * int(kv["common"])
