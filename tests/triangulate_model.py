"""Independent numpy model of l3d_triangulate_points (the checker of tests/test_front_ends_more.py and
tests/test_gpu_front_ends_more.py), written from main_pix4d.cpp's linearHomTriangulation (:34-69) and the loop that calls
it (:354-372): per observation the rows (0, -1, y) P_c and (1, 0, -x) P_c, M = A^T A, v = the right singular vector of M
for its smallest singular value (numpy.linalg.svd, LAPACK), X = v[0:3] / v[3]; valid = more than two observations and
norm(X) > L3D_EPS, a NaN is invalid, an infinite X valid; X = 0 where not valid.

`normal_matrices` and `solve_eigh` give the second fp64 host solver (numpy.linalg.eigh on the same M) whose distance to
the SVD is the yardstick of the GPU test: how far two correct solvers lie apart on the same input."""
import numpy as np

L3D_EPS = 1e-12


def normal_matrices(P, obs_offsets, obs_camera, obs_xy):
    """-> M [n, 4, 4]: A^T A per point, summed in observation order"""
    P = np.asarray(P, np.float64).reshape(-1, 3, 4)
    off = np.asarray(obs_offsets, np.int64)
    cam = np.asarray(obs_camera, np.int64)
    xy = np.asarray(obs_xy, np.float64).reshape(-1, 2)
    n = len(off) - 1
    M = np.zeros((n, 4, 4))
    if len(cam):
        Pc = P[cam]
        r1 = xy[:, 1:2] * Pc[:, 2] - Pc[:, 1]
        r2 = Pc[:, 0] - xy[:, 0:1] * Pc[:, 2]
        outer = r1[:, :, None] * r1[:, None, :] + r2[:, :, None] * r2[:, None, :]
        point = np.repeat(np.arange(n), np.diff(off))
        np.add.at(M, point, outer)
    return M


def _finish(v, counts):
    with np.errstate(divide="ignore", invalid="ignore"):
        X = v[:, :3] / v[:, 3:4]
        valid = (counts > 2) & (np.sqrt((X * X).sum(1)) > L3D_EPS)          # a NaN compares false
    X[~valid] = 0.0
    return X, valid


def solve_svd(M, counts):
    """the contract: the last right singular vector of every M"""
    v = np.zeros((len(M), 4))
    for i, m in enumerate(M):
        if counts[i] > 2 and np.isfinite(m).all():
            v[i] = np.linalg.svd(m)[2][3]
        else:
            v[i] = np.nan
    return _finish(v, counts)


def solve_eigh(M, counts):
    """the same vector from the symmetric eigensolver: the eigenvector of the eigenvalue of smallest magnitude"""
    v = np.full((len(M), 4), np.nan)
    ok = (counts > 2) & np.isfinite(M).all(axis=(1, 2))
    if ok.any():
        w, V = np.linalg.eigh(M[ok])
        k = np.abs(w).argmin(axis=1)
        v[ok] = V[np.arange(len(k)), :, k]
    return _finish(v, counts)


def triangulate_points(P, obs_offsets, obs_camera, obs_xy):
    """the model: -> (X [n, 3], valid [n] bool), the interface of line3dpp_amd.api.triangulate_points without a device"""
    counts = np.diff(np.asarray(obs_offsets, np.int64))
    return solve_svd(normal_matrices(P, obs_offsets, obs_camera, obs_xy), counts)


def project(P, X):
    """exact observations: pixel of X [n, 3] in the camera P [3, 4]"""
    x = np.column_stack([X, np.ones(len(X))]) @ np.asarray(P, np.float64).T
    return x[:, :2] / x[:, 2:3]


def observations(Ps, X, seen, noise=0.0, rng=None):
    """CSR observations of the points X: seen[i] = the cameras that observe point i, in order; Gaussian pixel noise"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in seen])]).astype(np.uint64)
    cam = np.array([c for s in seen for c in s], np.uint32)
    point = np.repeat(np.arange(len(X)), [len(s) for s in seen])
    Ps = np.asarray(Ps, np.float64).reshape(-1, 3, 4)
    x = np.einsum("nij,nj->ni", Ps[cam], np.column_stack([X, np.ones(len(X))])[point]) if len(cam) else np.zeros((0, 3))
    with np.errstate(divide="ignore", invalid="ignore"):          # a point in a camera's principal plane
        xy = x[:, :2] / x[:, 2:3]
    if noise:
        xy = xy + rng.normal(0.0, noise, xy.shape)
    return off, cam, xy
