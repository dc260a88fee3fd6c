"""CPU tests of the host side: C-ABI exports, scene generator, pair list, sharding, loud failure
without a GPU.  No compute call is made here (there is no GPU in the CPU container)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from line3dpp_amd import _lib, dist
from line3dpp_amd.scene import CONFIGS, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cabi_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "l3dpp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(l3d_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 25
    L = _lib.load()
    for name in sorted(declared):
        assert hasattr(L, name), f"{name} declared in include/l3dpp_hip.h but not exported"
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert b"gfx950" in L.l3d_build_info()


def test_pod_layouts_match_reference():
    # commons.h:186-203 Match = 4 x u32 + 6 x f32; clustering.h:47-51 CLEdge = 2 x int + float
    assert _lib.MATCH_DTYPE.itemsize == 40 and _lib.CLEDGE_DTYPE.itemsize == 12
    assert _lib.SEGMENT2D_DTYPE.itemsize == 8 and _lib.SLOT_DTYPE.itemsize == 32
    assert [n for n in _lib.MATCH_DTYPE.names] == ["src_cam", "src_seg", "tgt_cam", "tgt_seg", "overlap", "score3D",
                                                  "d_p1", "d_p2", "d_q1", "d_q2"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box without a GPU")
def test_fails_loudly_without_gpu():
    from line3dpp_amd.api import Line3D
    with pytest.raises(RuntimeError, match="no usable HIP device"):
        Line3D()


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_scene_generator_is_deterministic_and_well_formed():
    a = make_scene(6, 200, n_neighbors=4, seed=9)
    b = make_scene(6, 200, n_neighbors=4, seed=9)
    for va, vb in zip(a.views, b.views):
        assert np.array_equal(va.segs, vb.segs) and np.array_equal(va.R, vb.R)
        assert va.segs.shape == (200, 4) and va.segs.dtype == np.float32
        length = np.hypot(va.segs[:, 0] - va.segs[:, 2], va.segs[:, 1] - va.segs[:, 3])
        assert np.all(np.diff(length) <= 1e-3), "sorted by length, longest first (line3D.cc:323-360)"
        assert length.min() >= 19.0
        assert va.segs[:, [0, 2]].min() >= 0 and va.segs[:, [0, 2]].max() <= va.width - 1
        assert np.allclose(va.R @ va.R.T, np.eye(3), atol=1e-12)
        assert len(va.neighbors) == 4 and va.cam not in va.neighbors


def test_pair_counts_match_survey():
    # C1 320 directed pairs / 1.28e9 tests
    views = CONFIGS["C1"]["n_views"]; M = CONFIGS["C1"]["n_segs"]
    sc = make_scene(views, 8, n_neighbors=CONFIGS["C1"]["n_neighbors"], seed=1)
    tests, pairs = sc.pair_tests()
    assert len(pairs) == 320
    assert len(pairs) * M * M == 1_280_000_000
    # direction rule (line3D.cc:704-741): every unordered neighbour pair exactly once, src = first visitor
    assert len({tuple(sorted(p)) for p in pairs}) == len(pairs)
    assert all(s < t or s not in sc.views[t].neighbors for s, t in pairs)


def test_pair_ranges_cover_and_balance():
    rng = np.random.default_rng(0)
    for world in (1, 2, 3, 8):
        costs = rng.integers(1, 100, 57)
        r = dist.pair_ranges(costs, world)
        assert len(r) == world and r[0][0] == 0 and sum(c for _, c in r) == 57
        for (f0, c0), (f1, c1) in zip(r, r[1:]):
            assert f0 + c0 == f1
        loads = [costs[f:f + c].sum() for f, c in r]
        assert max(loads) <= costs.sum() / world + costs.max()
    assert dist.pair_ranges([], 4) == [(0, 0)] * 4
    assert dist.pair_ranges([5], 4)[-1] == (0, 1) or sum(c for _, c in dist.pair_ranges([5], 4)) == 1


def test_slot_byte_ranges():
    ranges = [(0, 2), (2, 1), (3, 0)]
    off = [0, 100, 250]
    br = dist.slot_byte_ranges(ranges, off, 400)
    assert br == [(0, 250 * 32), (250 * 32, 400 * 32), (400 * 32, 400 * 32)]


def test_reference_txt_result_format_round_trip():
    """The TXT result format of Line3D::save3DLinesAsTXT (line3D.cc:2631-2688): an excerpt of the reference's own
    fixture testdata/Line3D++_ref/...kNN_10__vis_3.txt (first 40 lines, tests/golden/make_golden.py --txt-excerpt) is
    parsed and re-created byte for byte."""
    import os
    from line3dpp_amd.io import read_3d_lines_txt, format_3d_lines_txt
    path = os.path.join(os.path.dirname(__file__), "golden", "ref_lines3d_excerpt.txt")
    lines = read_3d_lines_txt(path)
    assert len(lines) == 40
    assert all(len(L["segments"]) >= 1 and len(L["residuals"]) >= 3 for L in lines)   # visibility_t = 3
    assert format_3d_lines_txt(lines) == open(path).read()
    # the first record of the fixture
    assert np.allclose(lines[0]["segments"][0], [4.71643, -1.30196, 1.86753, 4.80419, -1.30583, 1.8841])
    assert lines[0]["residuals"].tolist() == [[19, 273], [17, 313], [24, 301]]


def test_reference_obj_and_stl_formats():
    """saveResultAsOBJ / saveResultAsSTL formats (line3D.cc:2579-2628, 2465-2531): the OBJ text generated from the
    parsed TXT excerpt equals the `v` records of the reference's own .obj fixture for the same 3D segments (the full
    files are identical too, 165 115 bytes, checked when the excerpt was made); the STL text has the reference's
    record structure."""
    import os
    from line3dpp_amd.io import read_3d_lines_txt, format_obj, format_stl
    gd = os.path.join(os.path.dirname(__file__), "golden")
    lines = read_3d_lines_txt(os.path.join(gd, "ref_lines3d_excerpt.txt"))
    n_seg = sum(len(L["segments"]) for L in lines)
    obj = format_obj(lines).splitlines(keepends=True)
    assert "".join(obj[:2 * n_seg]) == open(os.path.join(gd, "ref_lines3d_excerpt.obj")).read()
    assert obj[2 * n_seg:] == [f"l {2 * k + 1} {2 * k + 2}\n" for k in range(n_seg)]
    stl = format_stl(lines).splitlines()
    assert stl[0] == "solid lineModel" and stl[-1] == "endsolid lineModel" and len(stl) == 2 + 7 * n_seg
    assert stl[1] == " facet normal 1.0e+000 0.0e+000 0.0e+000" and stl[3].startswith("   vertex 4.716430e+00 ")


def test_principal_direction_of_the_library_agrees_with_lapack():
    """get3DlineFromCluster's 3x3 scatter problem (line3D.cc:2196-2211): the library's closed-form solver
    (l3d_recon.hip: principal_direction, host code, reachable without a GPU through the test hook
    l3d_principal_direction) against numpy.linalg.eigh.  The checker's Eigen stand-in solves the same problem with Jacobi
    rotations (oracle/ref_shim, bounded against LAPACK in tests/test_shim_vs_lapack.py): two independent codes, both
    within 1e-12 of LAPACK, so the reconstruction tail is not compared with itself."""
    import ctypes as C
    from line3dpp_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(3)
    worst = 0.0
    for trial in range(500):
        n = int(rng.integers(3, 40))
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        pts = rng.normal(size=3)[:, None] * 5 + d[:, None] * rng.uniform(-3, 3, 2 * n)[None, :] + \
            rng.normal(scale=10.0 ** rng.uniform(-6, -0.5), size=(3, 2 * n))
        Cm = np.eye(2 * n) - np.full((2 * n, 2 * n), 1.0 / (2 * n))
        S = np.ascontiguousarray(pts @ Cm @ pts.T)
        out = np.zeros(3)
        assert L.l3d_principal_direction(S.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
        w, V = np.linalg.eigh(S)
        want = V[:, np.argmax(w)]
        assert abs(np.linalg.norm(out) - 1.0) <= 1e-14
        err = min(np.linalg.norm(out - want), np.linalg.norm(out + want))
        gap = (w[-1] - w[-2]) / w[-1]
        assert err <= 1e-12 / max(gap, 1e-3), (trial, err, gap)
        worst = max(worst, err)
        assert out[np.argmax(np.abs(out))] > 0          # sign convention: largest component positive
    assert worst <= 1e-9


def test_cpp_rccl_driver_builds_and_links(tmp_path):
    """tests/cpp/rccl_driver.cpp: the multi-GPU matchImages (halo form) as a C++ host drives it -- C-ABI + RCCL, one
    process per GPU, no Python.  No multi-GPU box here: compiled and linked against libl3dpp_hip.so and librccl.so (every
    C-ABI entry of the sequence resolves), run single-rank on the GPU box (tests/test_gpu_modes.py)."""
    import subprocess
    if not os.path.exists("/opt/rocm/lib/librccl.so"):
        pytest.skip("no RCCL in this image")
    exe = str(tmp_path / "rccl_driver")
    lib_dir = os.path.join(ROOT, "line3dpp_amd", "csrc")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "rccl_driver.cpp"), "-o", exe, "-L" + lib_dir, "-ll3dpp_hip",
                           "-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath," + lib_dir])
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "librccl" in out and "libl3dpp_hip" in out and "not found" not in out


def test_bench_multi_gpu_model_terms():
    """bench.py prints what the halo form is expected to take on 2 / 4 / 8 GPUs from a single-GPU run's phase times
    (no node has been available): the terms must follow the plan the ranks would use (l3d_plan_shards) and the direct
    record exchange (one slab per xGMI link), with the ring figure beside it"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    from line3dpp_amd.scene import CONFIGS
    cfg = CONFIGS["C2"]
    nv, nn = cfg["n_views"], cfg["n_neighbors"]
    pairs = sorted({(min(i, (i + d) % nv), max(i, (i + d) % nv)) for i in range(nv) for d in range(1, nn // 2 + 1)})
    M = {i: cfg["n_segs"] for i in range(nv)}
    phase = dict(begin=0.13, match=14.0, finish=9.4, affinity=0.27)
    out = b.multi_gpu_model(pairs, M, 10, phase, lists_ms=7.8, record_bytes=510e6)
    t1 = sum(phase.values())
    for n in ("2", "4", "8"):
        m = out[n]; t = m["terms_ms"]
        assert abs(t["gather_records_direct"] - 1e3 * 510e6 / int(n) / 153e9) < 1e-3
        assert abs(t["gather_records_if_ring"] - (int(n) - 1) * t["gather_records_direct"]) < 2e-3
        assert abs(m["total_ms"] - sum(v for k, v in t.items() if not k.endswith("_MB") and not k.endswith("_if_ring"))) < 1e-3
        assert 1.0 / int(n) <= m["largest_pair_share"] < 1.3 / int(n)          # the plan balances the matching cost
        assert abs(m["speedup_over_1_gpu"] - t1 / m["total_ms"]) < 0.02
    assert out["8"]["speedup_over_1_gpu"] > out["4"]["speedup_over_1_gpu"] > out["2"]["speedup_over_1_gpu"] > 1.0


def _bench_module():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b, root


def test_bench_gpus_n_starts_n_ranks_and_never_runs_fewer():
    """`python bench.py --gpus N` without WORLD_SIZE starts N ranks itself (torch.distributed.run on 127.0.0.1) -- round 4
    parsed --gpus and ignored it.  Checked through the launcher's self-test (gloo on the CPU, no GPU work): two ranks come
    up and the backend reports two.  Without a GPU the real run refuses loudly, and a WORLD_SIZE that contradicts --gpus
    is refused as well (never a silent N = 1 line)."""
    import json
    import subprocess
    import sys
    _, root = _bench_module()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--launcher-selftest"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-800:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["ranks"] == [0, 1] and line["ranks_reported_by_backend"] == 2 and line["backend"] == "gloo"
    import torch
    if not torch.cuda.is_available():
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                             timeout=300, env=env)
        assert out.returncode != 0 and "n_gpus" not in out.stdout and "MI355X" in (out.stderr + out.stdout)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                         timeout=300, env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert out.returncode != 0 and "WORLD_SIZE=1" in (out.stderr + out.stdout)


def test_weak_scaling_scene_is_n_rings_cut_at_the_rings():
    """bench.py's weak-scaling scene for N ranks: N rings of the configuration in one scene -- N times the pairs and pair
    tests, no pair between rings, and the cost-balanced cut into N view ranges (l3d_plan_shards) falls on the ring
    boundaries: every rank gets one GPU's work and no pair crosses a cut."""
    b, _ = _bench_module()
    import line3dpp_amd.scene as S
    from line3dpp_amd import dist
    old = dict(S.CONFIGS["C1"])
    S.CONFIGS["C1"] = dict(n_views=10, n_segs=40, n_neighbors=4)          # a small stand-in of the configuration's shape
    try:
        one = b.weak_scene("C1", 1)
        three = b.weak_scene("C1", 3)
    finally:
        S.CONFIGS["C1"] = old
    t1, p1 = one.pair_tests(); t3, p3 = three.pair_tests()
    assert three.n_views == 3 * one.n_views and t3 == 3 * t1 and len(p3) == 3 * len(p1)
    assert [v.cam for v in three.views] == list(range(30))
    assert all(int(s) // 10 == int(t) // 10 for s, t in p3)              # neighbours stay inside a ring
    assert np.array_equal(three.views[0].segs, one.views[0].segs)         # ring 0 is the configuration itself
    assert not np.array_equal(three.views[10].segs, one.views[0].segs)    # the other rings are their own instances
    M = {v.cam: len(v.segs) for v in three.views}
    plan = dist.plan_halo(p3, M, 3)
    assert [int(x) for x in plan["view_bounds"]] == [0, 10, 20, 30] and not any(plan["runs"])


def test_multi_gpu_model_prices_the_sharded_tail_and_the_weak_reading():
    b, _ = _bench_module()
    from line3dpp_amd.scene import CONFIGS
    cfg = CONFIGS["C1"]
    nv, nn = cfg["n_views"], cfg["n_neighbors"]
    pairs = sorted({(min(i, (i + d) % nv), max(i, (i + d) % nv)) for i in range(nv) for d in range(1, nn // 2 + 1)})
    M = {i: cfg["n_segs"] for i in range(nv)}
    phase = dict(begin=0.03, match=0.74, finish=0.59, affinity=0.05)          # round 4's C1 phases
    out = b.multi_gpu_model(pairs, M, 10, phase, lists_ms=0.42, record_bytes=35.7e6, tail_bytes=8e6, sim_bytes=0.5e6)
    s8, w8 = out["8"]["strong"], out["8"]["weak"]
    assert "tail_own_views" in s8["terms_ms"] and "tail_chain_replicated" in s8["terms_ms"] and "tail_replicated" not in s8["terms_ms"]
    assert abs(s8["terms_ms"]["tail_own_views"] - 0.55 * 0.17 / 8) < 1e-3
    # (a 1.4 ms call on 8 GPUs is bound by its host synchronisation points -- 0.22 ms of 0.56 -- whatever is sharded)
    assert 2.3 < s8["speedup_over_1_gpu"] < 4.0
    assert abs(w8["total_ms"] - sum(w8["terms_ms"].values())) < 1e-3 and 0.3 < w8["efficiency"] < 1.0
    assert abs(w8["throughput_over_1_gpu"] - 8 * w8["efficiency"]) < 0.05
    assert out["2"]["weak"]["efficiency"] > w8["efficiency"]


def test_bench_dump_outputs_stays_within_its_limit_and_samples_reproducibly(tmp_path):
    """bench.py --dump-outputs: float64 .npy files, at most 64 MB in all; an output too large keeps the same seeded sample
    of its rows from run to run, and says which rows"""
    b, _ = _bench_module()
    from line3dpp_amd._lib import SEGMENT3D_DTYPE
    s3 = np.zeros(3, SEGMENT3D_DTYPE); s3["P1"] = [[1, 2, 3]] * 3; s3["valid"] = 4294967295
    cols = b._columns(s3)
    assert cols.shape == (3, 11) and cols.dtype == np.float64 and cols[0, 0] == 1 and cols[0, 10] == 4294967295
    assert b._columns(np.zeros(0, SEGMENT3D_DTYPE)).shape == (0, 11)
    big = np.arange(9_000_000, dtype=np.float64).reshape(-1, 9)          # 72 MB
    arrays = {"matches": big, "affinity_median_depth": np.array([2.5])}
    r1, r2 = b.write_outputs(arrays, str(tmp_path / "a")), b.write_outputs(arrays, str(tmp_path / "b"))
    assert r1["sampled"] == ["matches"] and r1["bytes"] == r2["bytes"]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["affinity_median_depth.npy", "matches.npy", "matches_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    rows = np.load(tmp_path / "a" / "matches_rows.npy").astype(np.int64)
    m = np.load(tmp_path / "a" / "matches.npy")
    assert m.dtype == np.float64 and len(rows) > 0.8 * len(big) and np.all(np.diff(rows) > 0)
    assert np.array_equal(m, big[rows]) and np.array_equal(m, np.load(tmp_path / "b" / "matches.npy"))
    small = b.write_outputs({"x": np.ones((4, 3))}, str(tmp_path / "c"))
    assert small["sampled"] == [] and os.listdir(tmp_path / "c") == ["x.npy"]
