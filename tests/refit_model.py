"""The contract of DESIGN §28 (the 3D lines refit against cameras and their 2D segments) restated in numpy from the text:
the frame about the model's centre, the observation list and its CSR per line, eligibility, carriers and start parameters,
the write-back, the span of a 2D segment along a carrier, the sweep into pieces and the assembly of the output model.  The
projection comes from tests/project_lines_model_vec.py, the association from tests/associate_model.py, the
parametrisation, the write-back and the Levenberg-Marquardt solver from tests/line_opt_model.py.  Python floats and numpy's
element-wise float64 operations round every operation on its own, as the library does when built with
-ffp-contract=off; dot products are written out left to right.

`refit` runs a whole call.  Every stage can be handed the library's own result of the stage before (`associations`,
`solve`), so that tests/test_gpu_refit.py pins the stages one by one."""
import math

import numpy as np

from tests import associate_model as AM
from tests import line_opt_model as LO
from tests import pose_model as PO
from tests import project_lines_model_vec as PV

LINE_DTYPE = np.dtype([("status", "<u4"), ("n_observations", "<u4"), ("n_views", "<u4"), ("solver_status", "<u4"),
                       ("iterations", "<u4"), ("n_pieces", "<u4"), ("cost0", "<f8"), ("cost1", "<f8"), ("x0", "<f8", 4),
                       ("x", "<f8", 4), ("P1", "<f8", 3), ("P2", "<f8", 3)])
OBSERVATION_DTYPE = np.dtype([("camera", "<u4"), ("segment", "<u4"), ("line", "<u4"), ("valid", "<u4"), ("s_lo", "<f8"),
                              ("s_hi", "<f8")])
STATUS = ("REFIT", "TOO_FEW_VIEWS", "CONSTANT", "FAILED", "NO_EXTENT", "EMPTY")
REFIT, TOO_FEW_VIEWS, CONSTANT, FAILED, NO_EXTENT, EMPTY = range(6)
LO_OTHER = 5
DEFAULTS = dict(max_distance=2.5, min_cos2=AM.min_cos2_of(10.0), min_overlap=0.5, near_plane=1e-6, min_length=0.0, visibility=3,
                max_iterations=50, use_ambiguous=False)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def lo_camera(cam, c):
    """the 16 numbers of LoCam about the centre c: R, C = Q - c with Q_i = -((R_0i t0 + R_1i t1) + R_2i t2), fx, fy, px, py"""
    K, R, t = PO.floats(cam["K"]), PO.floats(cam["R"]), PO.floats(cam["t"])
    C = [-((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]) - c[i] for i in range(3)]
    return np.array(list(R) + C + [K[0], K[4], K[2], K[5]], np.float64)


def observation(seg4):
    """stage 4: (p1x, p1y, p2x, p2y, nx, ny) of a float32 segment, the unit normal (-dy, dx) of its direction"""
    p1x, p1y, p2x, p2y = (float(v) for v in np.asarray(seg4, np.float32))
    dx, dy = p2x - p1x, p2y - p1y
    n = math.sqrt(dx * dx + dy * dy)
    if n > 0.0:
        dx, dy = dx / n, dy / n
    return np.array([p1x, p1y, p2x, p2y, -dy, dx])


def span_point(cam16, x, y, M, u):
    """stage 8 for one end point -> (valid, s)"""
    R, C = [float(v) for v in cam16[:9]], [float(v) for v in cam16[9:12]]
    fx, fy, px, py = (float(v) for v in cam16[12:16])
    xn = (x - px) / fx
    yn = (y - py) / fy
    v = [(R[i] * xn + R[3 + i] * yn) + R[6 + i] for i in range(3)]
    w = [M[i] - C[i] for i in range(3)]
    a, b, cc, d, e = dot3(u, u), dot3(u, v), dot3(v, v), dot3(u, w), dot3(v, w)
    den = a * cc - b * b
    if not den > 1e-12 * (a * cc):
        return False, 0.0
    return True, (b * e - cc * d) / den


def span(cam16, seg4, M, u):
    """-> (s_lo, s_hi, valid) of a float32 segment (x1, y1, x2, y2)"""
    p = [float(v) for v in np.asarray(seg4, np.float32)]
    M, u = [float(v) for v in M], [float(v) for v in u]
    with np.errstate(all="ignore"):
        ok1, s1 = span_point(cam16, p[0], p[1], M, u)
        ok2, s2 = span_point(cam16, p[2], p[3], M, u)
    if not (ok1 and ok2 and math.isfinite(s1) and math.isfinite(s2)):
        return 0.0, 0.0, 0
    return (s1, s2, 1) if s1 < s2 else (s2, s1, 1)


def sweep(s_lo, s_hi, camera, visibility, min_length, u_norm):
    """stage 9 -> [(s_start, s_end)] of the kept pieces, ascending"""
    events = sorted([(float(s_lo[i]), 0, i) for i in range(len(s_lo))] + [(float(s_hi[i]), 1, i) for i in range(len(s_lo))])
    open_of, count, start, out = {}, 0, 0.0, []
    for s, closing, i in events:
        cam = int(camera[i])
        if not closing:
            open_of[cam] = open_of.get(cam, 0) + 1
            if open_of[cam] == 1:
                count += 1
                if count == visibility:
                    start = s
        else:
            open_of[cam] -= 1
            if open_of[cam] == 0:
                count -= 1
                if count == visibility - 1 and s > start and (s - start) * u_norm >= min_length:
                    out.append((start, s))
    return out


def associations(segs, line, cams, segs_per_cam, par):
    """stage 2: what l3d_project_segments + l3d_associate_segments return, one array per camera"""
    model = np.asarray(segs, np.float64).reshape(-1, 6)
    out = []
    for cam, s2 in zip(cams, segs_per_cam):
        s2 = np.asarray(s2, np.float32).reshape(-1, 4)
        if not len(s2) or not len(model):
            out.append(AM.nothing(len(s2)))
            continue
        rec = PV.project_camera(cam, model[:, :3], model[:, 3:], line, par["near_plane"])
        out.append(AM.associate(rec, s2, par["max_distance"], par["min_cos2"], par["min_overlap"]))
    return out


def numpy_solve(x0, res_off, obs, obs_cam, cams16, max_iter):
    """the solver of tests/line_opt_model.py line by line -> (x, cost0, cost1, iters, status)"""
    n = len(x0)
    x = np.zeros((n, 4)); c0 = np.zeros(n); c1 = np.zeros(n); it = np.zeros(n, np.uint32); st = np.zeros(n, np.uint32)
    for i in range(n):
        r = slice(int(res_off[i]), int(res_off[i + 1]))
        x[i], c0[i], c1[i], it[i], st[i], _ = LO.lm_solve(x0[i], cams16[obs_cam[r]], obs[r], max_iter)
    return x, c0, c1, it, st


def prepare(segs, line, cams, segs_per_cam, assoc, par, to_cayley=LO.to_cayley):
    """stages 1, 3 and 5 from the associations -> a dict: c, n_lines, lines (LINE_DTYPE with status EMPTY / TOO_FEW_VIEWS /
    CONSTANT set, FAILED for the lines to solve), observations (CSR order over all lines), obs_off, and the solver's
    tables: solved (line indices), x0, res_off, obs [n, 6], obs_cam, cams16, carriers (centred, as given)"""
    model = np.asarray(segs, np.float64).reshape(-1, 6)
    line = np.asarray(line, np.uint32).reshape(-1)
    c, diag = PO.bounding_box(model)
    assert diag > 0.0
    n_lines = int(line.max()) + 1
    seg2d = [np.asarray(s, np.float32).reshape(-1, 4) for s in segs_per_cam]
    # the observation list in flat (camera, segment) order
    flat = [(k, i) for k, a in enumerate(assoc) for i in range(len(a))
            if a["record"][i] >= 0 and (a["n_accepted"][i] == 1 or par["use_ambiguous"])]
    by_line = [[] for _ in range(n_lines)]
    for k, i in flat:
        by_line[int(assoc[k]["line"][i])].append((k, i))          # (stable: ascending flat index)
    lines = np.zeros(n_lines, LINE_DTYPE)
    obs_rec = np.zeros(len(flat), OBSERVATION_DTYPE)
    obs_off = np.zeros(n_lines + 1, np.uint32)
    need = max(2, par["visibility"])
    solved, x0, res_off, obs, obs_cam, carriers = [], [], [0], [], [], []
    at = 0
    for l in range(n_lines):
        mine = np.flatnonzero(line == l)
        for k, i in by_line[l]:
            obs_rec[at] = (k, i, l, 0, 0.0, 0.0)
            at += 1
        obs_off[l + 1] = at
        L = lines[l]
        L["n_observations"] = len(by_line[l]); L["n_views"] = len({k for k, _ in by_line[l]})
        if not len(mine):
            L["status"] = EMPTY
            continue
        L["P1"] = model[mine[0], :3]; L["P2"] = model[mine[-1], 3:]
        L["status"] = TOO_FEW_VIEWS
        if L["n_views"] < need:
            continue
        P1 = np.array([float(L["P1"][k]) - c[k] for k in range(3)]); P2 = np.array([float(L["P2"][k]) - c[k] for k in range(3)])
        with np.errstate(all="ignore"):
            x, constant = to_cayley(P1, P2)
        L["x0"] = x
        if constant:
            L["status"] = CONSTANT; L["x"] = x
            continue
        L["status"] = FAILED
        solved.append(l); x0.append(x); carriers.append((P1, P2))
        for k, i in by_line[l]:
            obs.append(observation(seg2d[k][i])); obs_cam.append(k)
        res_off.append(len(obs))
    return dict(c=c, n_lines=n_lines, lines=lines, observations=obs_rec, obs_off=obs_off, solved=np.array(solved, np.uint32),
                x0=np.array(x0, np.float64).reshape(-1, 4), res_off=np.array(res_off, np.uint32),
                obs=np.array(obs, np.float64).reshape(-1, 6), obs_cam=np.array(obs_cam, np.uint32),
                cams16=np.array([lo_camera(cam, c) for cam in cams]).reshape(-1, 16), carriers=carriers, seg2d=seg2d)


def finish(segs, line, prep, solve, par, spans=None, write_back=LO.write_back):
    """stages 7, 9 and 10 (and 8 unless `spans` = (s_lo, s_hi, valid) over the solved lines' observations is given) from
    the solver's result -> the dict the library returns: segments, line, lines, observations"""
    model = np.asarray(segs, np.float64).reshape(-1, 6)
    line = np.asarray(line, np.uint32).reshape(-1)
    c, lines, obs_rec, obs_off = prep["c"], prep["lines"].copy(), prep["observations"].copy(), prep["obs_off"]
    x, cost0, cost1, iters, status = solve
    pieces = {}
    for s, l in enumerate(prep["solved"]):
        L = lines[l]
        L["x"] = x[s]; L["cost0"] = cost0[s]; L["cost1"] = cost1[s]; L["iterations"] = iters[s]; L["solver_status"] = status[s]
        if (status[s] == LO_OTHER and iters[s] == 0) or not (np.all(np.isfinite(x[s])) and math.isfinite(cost0[s]) and math.isfinite(cost1[s])):
            continue
        with np.errstate(all="ignore"):
            P1, P2, kept = write_back(x[s], *prep["carriers"][s])
        if not kept or not (np.all(np.isfinite(P1)) and np.all(np.isfinite(P2))):
            continue
        P1 = [float(v) for v in P1]; P2 = [float(v) for v in P2]
        M = [P1[k] * 0.5 + P2[k] * 0.5 for k in range(3)]
        u = [(P1[k] - P2[k]) * 0.5 for k in range(3)]
        L["P1"] = [P1[k] + c[k] for k in range(3)]; L["P2"] = [P2[k] + c[k] for k in range(3)]
        r0, r1 = int(prep["res_off"][s]), int(prep["res_off"][s + 1])
        lo, hi, cam = [], [], []
        for r in range(r0, r1):
            ob = obs_rec[int(obs_off[l]) + (r - r0)]
            k = int(ob["camera"])
            if spans is None:
                s_lo, s_hi, valid = span(prep["cams16"][k], prep["seg2d"][k][int(ob["segment"])], M, u)
            else:
                s_lo, s_hi, valid = float(spans[0][r]), float(spans[1][r]), int(spans[2][r])
            ob["s_lo"], ob["s_hi"], ob["valid"] = s_lo, s_hi, valid
            if valid:
                lo.append(s_lo); hi.append(s_hi); cam.append(k)
        cut = sweep(lo, hi, cam, par["visibility"], par["min_length"], math.sqrt(dot3(u, u)))
        L["status"] = REFIT if cut else NO_EXTENT
        pieces[int(l)] = [[(M[k] + a * u[k]) + c[k] for k in range(3)] + [(M[k] + b * u[k]) + c[k] for k in range(3)] for a, b in cut]
    out_segs, out_line = [], []
    for l in range(prep["n_lines"]):
        rows = pieces[l] if lines[l]["status"] == REFIT else [model[i] for i in np.flatnonzero(line == l)]
        out_segs.extend(rows); out_line.extend([l] * len(rows))
        lines[l]["n_pieces"] = len(rows)
    return dict(segments=np.array(out_segs, np.float64).reshape(-1, 6), line=np.array(out_line, np.uint32), lines=lines,
                observations=obs_rec)


def refit(segs, line, cams, segs_per_cam, assoc=None, solver=numpy_solve, to_cayley=LO.to_cayley, write_back=LO.write_back, **kw):
    """what one call of the library returns (a non-empty model, at least one camera with a segment)"""
    par = dict(DEFAULTS, **kw)
    if assoc is None:
        assoc = associations(segs, line, cams, segs_per_cam, par)
    prep = prepare(segs, line, cams, segs_per_cam, assoc, par, to_cayley)
    solve = solver(prep["x0"], prep["res_off"], prep["obs"], prep["obs_cam"], prep["cams16"], par["max_iterations"])
    out = finish(segs, line, prep, solve, par, write_back=write_back)
    out["associations"] = assoc
    out["prep"] = prep
    out["solve"] = solve
    return out
