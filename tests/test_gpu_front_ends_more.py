"""The Pix4D, OpenMVG and mavmap front ends on the MI355X.

1. l3d_triangulate_points (k_triangulate.hip) against the numpy model of tests/triangulate_model.py.  `valid` must be
   identical.  The position bound is not a constant: per case the yardstick is how far two correct fp64 host solvers lie
   apart on the same input -- the largest distance over the case's points between the model's SVD and numpy.linalg.eigh on
   the same M, as a fraction of the case's extent.  The device must stay within 4 times that of the SVD model, with a floor
   of 1e-12 of the extent (machine epsilon times the dataset's largest ratio of singular values of M, 6.6e3, is 1.5e-12).
   Four times, because fused multiply-adds and another rotation order move the rounding by a small factor.
2. The three programs as child processes on the rendered dataset (tests/front_end_dataset_more.py): the four files are
   byte-identical to the same dataset pushed by hand through the reader and the library's API, a run with two images per
   chunk gives the same bytes, and every Pix4D view's median_depth is within one float32 ulp of the model's.
3. The numbers of 3D lines are those the reference's own line3D.cc (oracle/_ref) reconstructs on the CPU from what each
   program hands to addImage with the segments of tests/lsd_model.py (REFERENCE_LINES below).

CHILD_TIMEOUT_S and what follows a child that runs into it are those of tests/test_gpu_front_end.py."""
import os

import numpy as np
import pytest

from line3dpp_amd import _lib, io
from line3dpp_amd.scene import _lookat
from tests import front_end_dataset as D
from tests import front_end_dataset_more as DM
from tests import triangulate_model as TM
from tests.test_gpu_front_end import SUFFIXES, _child, _files, _lines

pytestmark = pytest.mark.gpu

PROGRAMS = ("openmvg", "pix4d", "mavmap")
# (3D lines, 3D segments) the reference's line3D.cc reconstructs on the CPU at visibility_t 3 and 4
REFERENCE_LINES = {
    "openmvg": {3: (96, 96), 4: (94, 94)},
    "pix4d": {3: (96, 96), 4: (94, 94)},
    "mavmap": {3: (96, 96), 4: (93, 93)},              # median_depth = -1 reaches addImage, and the reference reconstructs
    "mavmap_metric": {3: (96, 96), 4: (93, 93)},       # -p -0.1 -z 25
}
MAVMAP_METRIC = ["-p", "-0.1", "-z", str(DM.MAVMAP_DISTANCE)]


# ---- 1. the triangulation kernel ---------------------------------------------------------------------------------------
def _dataset_case(noise):
    sc, X, _ = D.make()
    seen = [[v.cam for v in sc.views if i in set(v.worldpoints)] for i in range(len(X))]
    Ps = np.array([v.K @ np.column_stack([v.R, v.t]) for v in sc.views])
    return (Ps,) + TM.observations(Ps, X, seen, noise, np.random.default_rng(11)) + (X,)


def _ring_case(n_points=20000, n_cams=300, seed=12):
    """points in the scene's box, each seen by 3 to 200 of 300 cameras on make_scene's ring (radius 25, heights within
    +-2, looking at a point near the centre), pixels with Gaussian noise of 0.5 px"""
    rng = np.random.default_rng(seed)
    K = np.array([[D.FOCAL, 0, D.WIDTH / 2], [0, D.FOCAL, D.HEIGHT / 2], [0, 0, 1.0]])
    Ps = []
    for j in range(n_cams):
        phi = 2 * np.pi * j / n_cams
        C = np.array([25.0 * np.cos(phi), 25.0 * np.sin(phi), rng.uniform(-2, 2)])
        R = _lookat(C, rng.normal(0, 0.5, 3))
        Ps.append(K @ np.column_stack([R, -R @ C]))
    X = rng.uniform(-D.HALF, D.HALF, (n_points, 3))
    seen = [np.sort(rng.choice(n_cams, size=rng.integers(3, 201), replace=False)) for _ in range(n_points)]
    return (np.array(Ps),) + TM.observations(Ps, X, seen, 0.5, rng) + (X,)


def _special_case():
    """the dataset's cameras; points with 0, 1 and 2 observations, a point at the origin (invalid by the rule: norm(X) is
    not above L3D_EPS), and three ordinary points for the extent"""
    sc, _, _ = D.make()
    Ps = np.array([v.K @ np.column_stack([v.R, v.t]) for v in sc.views])
    X = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [4.0, -3.0, 1.0], [-6.0, 5.0, -2.0], [9.0, 9.0, 3.0]])
    seen = [[], [2], [0, 5], [0, 1, 2, 3, 4, 5, 6], [0, 1, 2], [1, 3, 4, 6], [0, 1, 2, 3, 4, 5, 6]]
    return (Ps,) + TM.observations(Ps, X, seen) + (X,)


CASES = {"dataset_exact": lambda: _dataset_case(0.0), "dataset_noise": lambda: _dataset_case(0.5), "ring_20000": _ring_case,
         "special": _special_case}
MADE_INVALID = {"special": 4}


@pytest.mark.parametrize("case", list(CASES))
def test_triangulate_points_against_the_model(case):
    from line3dpp_amd.api import triangulate_points
    Ps, off, cam, xy, X = CASES[case]()
    counts = np.diff(off.astype(np.int64))
    M = TM.normal_matrices(Ps, off, cam, xy)
    Xs, vs = TM.solve_svd(M, counts)
    Xe, ve = TM.solve_eigh(M, counts)
    Xd, vd = triangulate_points(Ps, off, cam, xy)
    extent = np.ptp(X, axis=0).max()
    both = vs & ve
    yard = np.linalg.norm(Xs[both] - Xe[both], axis=1).max() / extent
    bound = max(4 * yard, 1e-12)
    dist = np.linalg.norm(Xd[vs & vd] - Xs[vs & vd], axis=1).max() / extent
    truth = np.linalg.norm(Xs[vs] - X[vs], axis=1).max() / extent
    print(f"{case}: {len(X)} points, {int(vs.sum())} valid in the model, {int(vd.sum())} on the device; extent {extent:.4g}; "
          f"svd to eigh {yard:.3g}, device to svd {dist:.3g} of the extent: {dist / bound:.3g} of the bound {bound:.3g}, "
          f"{dist / yard:.3g} of the yardstick; model to the true points {truth:.3g}")
    assert np.array_equal(vd, vs), np.nonzero(vd != vs)[0][:10]
    assert np.array_equal(ve, vs)
    assert (~vs).sum() - MADE_INVALID.get(case, 0) <= 0.05 * len(X)           # otherwise a badly chosen input
    assert not Xd[~vd].any()
    assert dist <= bound
    if case.startswith("dataset"):
        assert int((vs & vd).sum()) >= 570
    if case == "special":
        assert vs.tolist() == [False, False, False, False, True, True, True]


def test_triangulate_points_arguments():
    from line3dpp_amd.api import triangulate_points
    L = _lib.load()
    Ps, off, cam, xy, _ = _special_case()
    bad = cam.copy()
    bad[5] = len(Ps)                                                          # one camera index out of range
    with pytest.raises(RuntimeError, match=r"\[-1\].*camera >= n_cameras"):
        triangulate_points(Ps, off, bad, xy)
    X, valid = triangulate_points(Ps, np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros((0, 2)))
    assert X.shape == (0, 3) and valid.shape == (0,)                          # no points: L3D_OK
    assert L.l3d_triangulate_points(0, 0, None, 0, None, None, None, None, None) == 0
    P = np.ascontiguousarray(Ps)
    out, flags = np.zeros((len(off) - 1, 3)), np.zeros(len(off) - 1, np.uint8)
    down = off.copy(); down[3] = 0                                            # offsets that decrease
    assert L.l3d_triangulate_points(0, len(P), _lib.ptr(P), len(off) - 1, _lib.ptr(down), _lib.ptr(cam), _lib.ptr(xy),
                                    _lib.ptr(out), _lib.ptr(flags)) == -1
    # the projection matrices beyond the LDS staging (more than 341 cameras) go through the cache: same bits
    many = np.concatenate([P, np.tile(P[:1], (400, 1, 1))])
    a, b = triangulate_points(P, off, cam, xy), triangulate_points(many, off, cam, xy)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 2. the programs -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    folder = tmp_path_factory.mktemp("front_end_dataset_more")
    DM.write(folder)
    return folder


@pytest.fixture(scope="module")
def programs(data, tmp_path_factory):
    """one child process per program, one after another: program -> (result folder, stdout)"""
    out = {}
    for p in PROGRAMS:
        folder = tmp_path_factory.mktemp("out_" + p)
        out[p] = (folder, _child(p, DM.argv(data, p, folder)))
    return out


def _entries(data, program):
    if program == "openmvg":
        es = io.read_openmvg(str(data / "sfm_data.json"), str(data / "images"))
        return [(e["id"], e["path"], e) for e in es]
    if program == "pix4d":
        es = io.read_pix4d(str(data / "pix4d"), DM.PIX4D_PREFIX)
        return [(e["id"], str(data / "images" / e["name"]), e) for e in es]
    es = io.read_mavmap(str(data / "image-data.txt"), 10)
    return [(e["id"], str(data / "images" / (e["name"] + ".png")), dict(e, median_depth=-1.0)) for e in es]


def _longhand(data, program, out):
    """the dataset through the reader and the library's API, step by step, without front_end"""
    from line3dpp_amd.api import Line3D
    from line3dpp_amd.lsd import read_image_gray, undistort_images
    views = _entries(data, program)
    assert [cam for cam, _, _ in views] == list(range(D.N_VIEWS))
    os.makedirs(out)
    images = [read_image_gray(path) for _, path, _ in views]
    assert all(im.shape == (D.HEIGHT, D.WIDTH) for im in images)
    und = [io.front_end_undistortion(program, e, D.WIDTH, D.HEIGHT) for _, _, e in views]
    todo = [i for i, u in enumerate(und) if u is not None]
    assert len(todo) == {"openmvg": len(D.DISTORTION), "pix4d": D.N_VIEWS, "mavmap": 0}[program]
    if todo:
        done = undistort_images([images[i] for i in todo], [und[i][0] for i in todo], [und[i][1] for i in todo], [und[i][2] for i in todo])
        for i, im in zip(todo, done):
            assert im.shape == images[i].shape and np.array_equal(im, images[i]) == (not und[i][1].any())
            images[i] = im
    g = Line3D(str(out), True, -1, 3000, program != "mavmap", True)
    for (cam, _, e), im in zip(views, images):
        g.addImage(cam, im, e["K"], e["R"], e["t"], float(e["median_depth"]), e["worldpoints"])
    assert g.numImages() == D.N_VIEWS
    assert g.matchImages(2.5, 10.0, 10, 0.25, 10, -1.0)
    assert g.reconstruct3Dlines(3, False, -1.0, False)
    name = g.outputFilename()
    assert g.saveResultAsSTL(str(out)) and g.saveResultAsOBJ(str(out)) and g.save3DLinesAsTXT(str(out)) and g.save3DLinesAsBIN(str(out))
    g.close()
    return name


@pytest.mark.parametrize("program", PROGRAMS)
def test_program_leaves_the_four_files_and_they_are_the_longhand_pipelines(data, programs, tmp_path, program):
    folder, stdout = programs[program]
    got = _files(folder)
    name = _longhand(data, program, tmp_path / "longhand")
    assert sorted(got) == sorted(name + s for s in SUFFIXES)
    assert "seconds per stage: read " in stdout
    print(program, stdout[stdout.index("seconds per stage"):].strip())
    want = _files(tmp_path / "longhand")
    for n in got:
        assert got[n] == want[n], f"{program}: {n} differs from the step-by-step pipeline's"


@pytest.mark.parametrize("program", PROGRAMS)
def test_chunking_does_not_change_the_result(data, programs, tmp_path, program):
    from line3dpp_amd import front_end
    budget = 2 * D.WIDTH * D.HEIGHT                                         # two images per chunk, one in the last
    _child(program, DM.argv(data, program, tmp_path / "out"), env={front_end.CHUNK_ENV: str(budget)})
    assert _files(tmp_path / "out") == _files(programs[program][0])


def test_pix4d_median_depths_are_the_model_s(data):
    dev = io.read_pix4d(str(data / "pix4d"), DM.PIX4D_PREFIX)
    model = io.read_pix4d(str(data / "pix4d"), DM.PIX4D_PREFIX, triangulate=TM.triangulate_points)
    assert [e["id"] for e in dev] == [e["id"] for e in model] == list(range(D.N_VIEWS))
    assert [e["worldpoints"] for e in dev] == [e["worldpoints"] for e in model]
    ulps = [abs(float(a["median_depth"]) - float(b["median_depth"])) / float(np.spacing(b["median_depth"])) for a, b in zip(dev, model)]
    print(f"Pix4D median_depth: {sum(u == 0 for u in ulps)} of {len(ulps)} views equal to the model's, float32 ulps {ulps}")
    assert max(ulps) <= 1


def test_a_missing_device_ends_pix4d_before_line3d_is_constructed(data, tmp_path, capsys):
    from line3dpp_amd import front_end
    from tests.test_front_end_programs import Recorder
    rec = Recorder()
    read = io.read_pix4d
    try:
        io.read_pix4d = lambda folder, prefix, **kw: read(folder, prefix, device=4096)
        rc = front_end.main(["pix4d"] + DM.argv(data, "pix4d", tmp_path / "out"), line3d_factory=rec, undistort=rec.undistort)
    finally:
        io.read_pix4d = read
    assert rc == 1 and rec.constructed == 0 and "l3d_triangulate_points failed" in capsys.readouterr().err


# ---- 3. line counts ------------------------------------------------------------------------------------------------------------
def _count(folder):
    lines = _lines(folder)
    return len(lines), sum(len(L["segments"]) for L in lines)


@pytest.mark.parametrize("program", ("openmvg", "pix4d"))
def test_line_counts_are_the_reference_s(data, programs, tmp_path, program):
    from line3dpp_amd import front_end
    got3 = _count(programs[program][0])
    g, _ = front_end.PROGRAMS[program](DM.argv(data, program, tmp_path / "v4") + ["-v", "4"])
    g.close()
    got4 = _count(tmp_path / "v4")
    print(f"{program}: visibility 3: {got3}, visibility 4: {got4} (3D lines, 3D segments)")
    assert got3 == REFERENCE_LINES[program][3] and got4 == REFERENCE_LINES[program][4]


def test_mavmap_line_counts_are_the_reference_s(data, programs, tmp_path):
    """default flags: median_depth = const_reg_depth = -1 reaches addImage; and one metric run"""
    from line3dpp_amd import front_end
    got = {("mavmap", 3): _count(programs["mavmap"][0])}
    for key, extra in (("mavmap", []), ("mavmap_metric", MAVMAP_METRIC)):
        for v in (3, 4):
            if (key, v) in got:
                continue
            out = tmp_path / f"{key}_{v}"
            g, _ = front_end.run_mavmap(DM.argv(data, "mavmap", out) + extra + ["-v", str(v)])
            g.close()
            got[(key, v)] = _count(out)
    print("mavmap (3D lines, 3D segments):", got)
    for (key, v), count in got.items():
        assert count == REFERENCE_LINES[key][v], (key, v, count)
