"""The dataset of tests/front_end_dataset.py in three more formats: an OpenMVG sfm_data.json, a Pix4D project
(calibrated camera parameters and tie points) and a mavmap image-data log, for tests/test_front_ends_more.py and
tests/test_gpu_front_ends_more.py.  Doubles are written with 17 significant digits, so the files carry the scene's
cameras exactly; the Pix4D observations are the exact projections of the worldpoints (no noise); the mavmap angles come
from the scene's rotations.  Nothing here is taken from a real project of any of the three packages: the layouts are what
the reference's mains parse."""
import numpy as np

from tests import front_end_dataset as D

PIX4D_PREFIX = "scene"
MAVMAP_DISTANCE = 25.0           # scene.make_scene: the ring's radius = the cameras' distance to the structure's centre


def g17(x):
    return "%.17g" % float(x)


def feature_name(i):
    return f"tp{i:05d}"


def rpy(Rwc):
    """(roll, pitch, yaw) with Rwc = Rz(yaw) Ry(pitch) Rx(roll); away from pitch = +-90 degrees"""
    return (np.arctan2(Rwc[2, 1], Rwc[2, 2]), -np.arcsin(Rwc[2, 0]), np.arctan2(Rwc[1, 0], Rwc[0, 0]))


def pix4d_feature_order(sc):
    """worldpoint index of feature id k: Pix4D features are numbered in order of first appearance in the tie-point file"""
    order, seen = [], set()
    for v in sc.views:
        for i in v.worldpoints:
            if i not in seen:
                seen.add(i); order.append(i)
    return order


def write_openmvg(path, sc, X):
    """one intrinsic group per distinct distortion; cereal writes a polymorphic_name once, so only the first group of a
    model carries it"""
    k1 = {v.cam: D.DISTORTION.get(v.cam, 0.0) for v in sc.views}
    groups = sorted(set(k1.values()), key=lambda k: (k != 0.0, k))            # group 0: no distortion
    group_of = {k: g for g, k in enumerate(groups)}
    views = ",\n".join(
        '{"key": %d, "value": {"polymorphic_id": 1073741824, "ptr_wrapper": {"id": %d, "data": {"local_path": "", '
        '"filename": "view_%d.png", "width": %d, "height": %d, "id_view": %d, "id_intrinsic": %d, "id_pose": %d}}}}'
        % (v.cam, 2147483649 + v.cam, v.cam, D.WIDTH, D.HEIGHT, v.cam, group_of[k1[v.cam]], v.cam) for v in sc.views)
    intr, named = [], set()
    for g, k in enumerate(groups):
        model = "pinhole_radial_k1" if k else "pinhole"
        name = "" if model in named else '"polymorphic_name": "%s", ' % model
        named.add(model)
        disto = ', "disto_k1": [%s]' % g17(k) if k else ""
        intr.append('{"key": %d, "value": {"polymorphic_id": 2147483649, %s"ptr_wrapper": {"id": %d, "data": {"width": %d, '
                    '"height": %d, "focal_length": %s, "principal_point": [%s, %s]%s}}}}'
                    % (g, name, 2147483700 + g, D.WIDTH, D.HEIGHT, g17(D.FOCAL), g17(D.WIDTH / 2), g17(D.HEIGHT / 2), disto))
    extr = ",\n".join('{"key": %d, "value": {"rotation": [%s], "center": [%s]}}'
                      % (v.cam, ", ".join("[" + ", ".join(g17(x) for x in row) + "]" for row in v.R),
                         ", ".join(g17(x) for x in -v.R.T @ v.t)) for v in sc.views)
    seen = {v.cam: set(v.worldpoints) for v in sc.views}
    struct = ",\n".join('{"key": %d, "value": {"X": [%s], "observations": [%s]}}'
                        % (i, ", ".join(g17(x) for x in X[i]),
                           ", ".join('{"key": %d, "value": {"id_feat": %d, "x": [1.0, 1.0]}}' % (c, i)
                                     for c in sorted(seen) if i in seen[c])) for i in range(len(X)))
    path.write_text('{"sfm_data_version": "0.3", "root_path": "",\n"views": [\n%s],\n"intrinsics": [\n%s],\n"extrinsics": [\n%s],\n'
                    '"structure": [\n%s],\n"control_points": []}\n' % (views, ",\n".join(intr), extr, struct))


def projections(sc, X):
    """{camera: [n, 2] exact pixels of its worldpoints}"""
    out = {}
    for v in sc.views:
        x = (v.K @ ((v.R @ X[v.worldpoints].T).T + v.t).T).T
        out[v.cam] = x[:, :2] / x[:, 2:3]
    return out


def write_pix4d(folder, sc, X):
    rows = ["fileName imageWidth imageHeight", "camera matrix K [3x3]", "radial distortion [3x1]", "tangential distortion [2x1]",
            "camera position t [3x1]", "camera rotation R [3x3]", ""]
    for v in sc.views:
        rows.append(f"view_{v.cam}.png {D.WIDTH} {D.HEIGHT}")
        rows += [" ".join(g17(x) for x in row) for row in v.K]
        rows.append(" ".join(g17(x) for x in (D.DISTORTION.get(v.cam, 0.0), 0.0, 0.0)))
        rows.append("0 0")
        rows.append(" ".join(g17(x) for x in -v.R.T @ v.t))
        rows += [" ".join(g17(x) for x in row) for row in v.R]
    (folder / f"{PIX4D_PREFIX}_calibrated_camera_parameters.txt").write_text("\n".join(rows) + "\n")
    px = projections(sc, X)
    rows = []
    for v in sc.views:
        rows.append(f"view_{v.cam}")
        rows += [f"{feature_name(i)} {g17(p[0])} {g17(p[1])} 1.5" for i, p in zip(v.worldpoints, px[v.cam])]
    (folder / f"{PIX4D_PREFIX}_tp_pix4d.txt").write_text("\n".join(rows) + "\n")


def write_mavmap(path, sc):
    rows = ["# image-data: NAME, ROLL, PITCH, YAW, LAT, LON, ALT, H, TX, TY, TZ, CAMERA, MODEL, FX, FY, CX, CY,"]
    for v in sc.views:
        r, p, y = rpy(v.R.T)
        C = -v.R.T @ v.t
        tok = [f"view_{v.cam}", g17(r), g17(p), g17(y), "47.0", "8.5", "400.0", "10.0", g17(C[0]), g17(C[1]), g17(C[2]), "1",
               "PINHOLE", g17(v.K[0, 0]), g17(v.K[1, 1]), g17(v.K[0, 2]), g17(v.K[1, 2])]
        rows.append(" ".join(t + "," for t in tok))
    path.write_text("\n".join(rows) + "\n")


def write(folder):
    """front_end_dataset.write(folder) (images, .nvm, COLMAP, bundler) and beside it folder/sfm_data.json,
    folder/pix4d/scene_{calibrated_camera_parameters,tp_pix4d}.txt and folder/image-data.txt -> (scene, worldpoints)"""
    sc = D.write(folder)
    _, X, _ = D.make()
    write_openmvg(folder / "sfm_data.json", sc, X)
    (folder / "pix4d").mkdir()
    write_pix4d(folder / "pix4d", sc, X)
    write_mavmap(folder / "image-data.txt", sc)
    return sc, X


def argv(data, program, out):
    return {"openmvg": ["-i", str(data / "images"), "-j", str(data / "sfm_data.json"), "-o", str(out)],
            "pix4d": ["-i", str(data / "images"), "-b", str(data / "pix4d"), "-f", PIX4D_PREFIX, "-o", str(out)],
            "mavmap": ["-i", str(data / "images"), "-b", str(data / "image-data.txt"), "-t", "png", "-o", str(out)]}[program]
