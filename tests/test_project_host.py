"""CPU tests of the projection stages: the numpy model's own properties, the layout of the two new structs
and the new symbols of the built library, and the array forms of the model (tests/project_lines_model_vec.py) against
its loops, byte for byte.  No device call is made here."""
import ctypes as C

import numpy as np

from line3dpp_amd import _lib
from tests import project_lines_cases as Cs
from tests import project_lines_model as M
from tests import project_lines_model_vec as V

NEW_SYMBOLS = ["l3d_project_segments", "l3d_render_line_maps", "l3d_draw_line_maps", "l3d_view_camera", "l3d_project_lines",
               "l3d_get_projected_lines", "l3d_render_lines", "l3d_draw_lines", "l3d_set_projection_budget"]


def test_library_exports_the_projection_entries():
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by the built library"
        assert name in _lib.EXPORTS


def test_struct_sizes():
    assert C.sizeof(_lib.ProjectedSegment) == 32 and _lib.PROJECTED_SEGMENT_DTYPE.itemsize == 32
    assert M.RECORD_DTYPE == _lib.PROJECTED_SEGMENT_DTYPE
    # l3d_camera { double K[9], R[9], t[3]; uint32_t width, height; } = 21 doubles and two 32-bit words
    assert C.sizeof(_lib.Camera) == 21 * 8 + 2 * 4 == 176


def test_stage1_model_properties():
    cams = Cs.stage1_cameras()
    P1, P2, line = Cs.stage1_segments()
    n_vis = n_rect = n_near = 0
    for cam in cams:
        xmax, ymax = cam["width"] - 1, cam["height"] - 1
        for s in range(len(P1)):
            r = M.project_segment(cam, P1[s], P2[s])
            if r is None:
                continue
            n_vis += 1
            x1, y1, x2, y2, iz1, iz2, flags, t0, t1, (ux1, uy1, ux2, uy2) = r
            assert 0.0 <= t0 < t1 <= 1.0
            n_rect += bool(flags & M.CLIPPED_RECT); n_near += bool(flags & M.CLIPPED_NEAR)
            assert bool(flags & M.CLIPPED_RECT) == (t0 > 0 or t1 < 1)
            # the clipped end points lie inside the rectangle (to the rounding of a + t d: 1e-9 pixels is generous) ...
            scale = max(1.0, abs(ux1), abs(uy1), abs(ux2), abs(uy2))
            for x, y in ((x1, y1), (x2, y2)):
                assert -1e-9 * scale <= x <= xmax + 1e-9 * scale and -1e-9 * scale <= y <= ymax + 1e-9 * scale
                # ... and on the unclipped projected line
                d = np.hypot(ux2 - ux1, uy2 - uy1)
                if d > 0:
                    assert abs((ux2 - ux1) * (y - uy1) - (uy2 - uy1) * (x - ux1)) / d <= 1e-9 * scale
            assert iz1 > 0 and iz2 > 0
    assert n_vis > 150 and n_rect > 50 and n_near > 5      # the cases do reach the branches


def test_stage1_model_drops_a_projection_that_is_not_finite():
    cam = dict(Cs.stage1_cameras()[0])
    P1, P2, line = Cs.stage1_segments()
    assert M.project_segment(cam, P1[0], P2[0]) is not None
    cam["K"] = np.array(cam["K"], np.float64).copy(); cam["K"][2] = 0.0            # q.z = 0: x and y are NaN or infinite
    assert all(M.project_segment(cam, P1[s], P2[s]) is None for s in range(len(P1)))
    # 1 / near is finite in double and infinite in float32: segments clipped at such a near plane go (unless the rectangle
    # clips the same end, which interpolates a finite inverse depth), the others stay
    cam = Cs.stage1_cameras()[0]
    usual, tiny = (M.project_segments([cam], P1, P2, line, near=near)[0] for near in (1e-6, 1e-45))
    clipped = (usual["segment"] & M.CLIPPED_NEAR) != 0
    assert 0 < len(usual) - len(tiny) <= clipped.sum()
    assert set(tiny["segment"] & M.SEGMENT_MASK) >= set(usual["segment"][~clipped] & M.SEGMENT_MASK)
    assert all(np.isfinite(tiny[k]).all() for k in ("x1", "y1", "x2", "y2", "inv_depth1", "inv_depth2"))


def test_stage1_hand_made_cases_in_camera_0():
    cam = Cs.stage1_cameras()[0]
    P1, P2, line = Cs.stage1_segments()
    rec = M.project_segments([cam], P1, P2, line)[0]
    by_seg = {int(r["segment"]) & M.SEGMENT_MASK: r for r in rec}
    flags = {s: int(r["segment"]) & ~M.SEGMENT_MASK for s, r in by_seg.items()}
    assert flags[0] == 0 and np.allclose([by_seg[0][k] for k in ("x1", "y1", "x2", "y2")], [10, 10, 100, 80], atol=1e-4)
    assert abs(by_seg[0]["inv_depth1"] - 0.5) < 1e-6 and abs(by_seg[0]["inv_depth2"] - 1 / 3) < 1e-6
    for s in (1, 2, 3, 4, 5, 6, 21):
        assert flags[s] == M.CLIPPED_RECT, s
    for s in (7, 8, 9, 10, 13, 16, 20, 22):                  # outside, one pixel outside, behind the camera
        assert s not in by_seg, s
    for s in (11, 12, 14, 15, 19):                           # on the border, one pixel inside, zero length inside
        assert flags[s] == 0, s
    assert flags[17] == 0 and flags[18] == 0                 # an end point exactly on the border stays unclipped
    assert flags[23] & M.CLIPPED_NEAR and flags[24] & M.CLIPPED_NEAR and flags[25] & M.CLIPPED_NEAR
    assert line[5] == by_seg[5]["line"]
    assert list(np.array(sorted(by_seg))) == [int(r["segment"]) & M.SEGMENT_MASK for r in rec]   # ascending order


def brute_force_maps(records, width, height, thickness):
    """the rule of stage 2 asked per pixel: which records draw (x, y), and which key is the largest"""
    half = (thickness - 1) // 2
    line_id = np.full((height, width), -1, np.int32)
    inv_depth = np.zeros((height, width), np.float32)
    ends = []
    for r in records:
        x1, y1, x2, y2, z1, z2 = (np.float64(r[k]) for k in ("x1", "y1", "x2", "y2", "inv_depth1", "inv_depth2"))
        if x1 == x2 and y1 == y2:
            continue
        xm = abs(x2 - x1) >= abs(y2 - y1)
        e1, e2 = ((x1, y1, z1), (x2, y2, z2)) if xm else ((y1, x1, z1), (y2, x2, z2))
        ends.append((xm, e1, e2, int(r["line"])) if e1[0] <= e2[0] else (xm, e2, e1, int(r["line"])))
    for y in range(height):
        for x in range(width):
            best = 0
            for xm, a, b, line in ends:
                m, n = (x, y) if xm else (y, x)
                if not (np.ceil(a[0]) <= m <= np.floor(b[0])):
                    continue
                s = (np.float64(m) - a[0]) / (b[0] - a[0])
                if abs(n - int(np.floor(a[1] + s * (b[1] - a[1]) + 0.5))) > half:
                    continue
                best = max(best, M.pixel_key(np.float32(a[2] + s * (b[2] - a[2])), line))
            if best:
                line_id[y, x] = 0xFFFFFFFF - (best & 0xFFFFFFFF)
                inv_depth[y, x] = np.array([best >> 32], np.uint32).view(np.float32)[0]
    return line_id, inv_depth


def test_stage2_model_equals_a_dense_brute_force():
    rec = Cs.stage2_records(40, 29, seed=3)[[0, 2, 4, 6, 7, 9, 15, 16, 17, 18, 19, 22, 23, 24, 25, 26]].copy()
    for k in ("x1", "x2"):
        rec[k] = np.minimum(rec[k] * 0.4, 39)
    for k in ("y1", "y2"):
        rec[k] = np.minimum(rec[k] * 0.45, 28)
    for thickness in (1, 3):
        got = M.render_line_maps(rec, 40, 29, thickness)
        want = brute_force_maps(rec, 40, 29, thickness)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (got[0] >= 0).sum() > 60


def test_stage2_model_rules():
    R = lambda *a: np.array([Cs.rec(*a)], M.RECORD_DTYPE)   # noqa: E731
    ids, iz = M.render_line_maps(R(2, 3, 6, 3, 0.5, 0.25, 7), 10, 8)
    assert list(np.argwhere(ids == 7)[:, 1]) == [2, 3, 4, 5, 6] and set(np.argwhere(ids == 7)[:, 0]) == {3}   # both ends drawn
    assert iz[3, 2] == np.float32(0.5) and iz[3, 6] == np.float32(0.25) and iz[3, 4] == np.float32(0.375)
    assert (M.render_line_maps(R(2.25, 3, 2.75, 3.2, 1, 1, 7), 10, 8)[0] == -1).all()            # no integer m in range
    ids = M.render_line_maps(R(1, 1, 5, 5, 1, 1, 2), 10, 8)[0]                                    # 45 degrees: x-major
    assert [tuple(p) for p in np.argwhere(ids == 2)] == [(k, k) for k in range(1, 6)]
    ids = M.render_line_maps(R(1, 0, 8, 0, 1, 1, 2), 10, 8, 3)[0]                                 # thickness 3 on the border
    assert set(np.argwhere(ids == 2)[:, 0]) == {0, 1}
    two = np.concatenate([R(0, 2, 9, 2, 0.5, 0.5, 4), R(4, 0, 4, 7, 0.75, 0.75, 9)])
    assert M.render_line_maps(two, 10, 8)[0][2, 4] == 9 and M.render_line_maps(two[::-1], 10, 8)[0][2, 4] == 9   # nearer
    same = np.concatenate([R(0, 2, 9, 2, 0.5, 0.5, 4), R(3, 2, 6, 2, 0.5, 0.5, 1)])
    assert list(M.render_line_maps(same, 10, 8)[0][2]) == [4, 4, 4, 1, 1, 1, 1, 4, 4, 4]          # equal depth: smaller index


def test_palette_and_blend():
    # h = 1 * 0x9E3779B1: bytes 0x9E, 0x37, 0x79 -> 64 + 158 * 3 / 4, 64 + 55 * 3 / 4, 64 + 121 * 3 / 4
    assert M.palette(0) == (182, 105, 154)
    assert M.palette(1) == tuple(64 + ((0x3C6EF362 >> s) & 255) * 3 // 4 for s in (24, 16, 8))
    assert all(64 <= c <= 255 for k in range(2000) for c in M.palette(k))
    img = np.array([[10, 200], [30, 40]], np.uint8)
    ids = np.array([[-1, 0], [1, -1]], np.int32)
    out = M.draw_line_map(img, ids, 255)
    assert out[0, 0].tolist() == [10, 10, 10] and out[0, 1].tolist() == [182, 105, 154] and out[1, 1].tolist() == [40, 40, 40]
    out = M.draw_line_map(img, ids, 128, colors=[(255, 0, 0), (0, 255, 7)])
    assert out[0, 1].tolist() == [(128 * 255 + 127 * 200 + 127) // 255, (127 * 200 + 127) // 255, (127 * 200 + 127) // 255]
    assert out[1, 0].tolist() == [(127 * 30 + 127) // 255, (128 * 255 + 127 * 30 + 127) // 255, (128 * 7 + 127 * 30 + 127) // 255]
    rgb = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    assert np.array_equal(M.draw_line_map(rgb, np.full((2, 2), -1, np.int32)), rgb)
    assert M.draw_line_map(rgb, ids, 0).tolist() == rgb.tolist()                                  # alpha 0 changes nothing


# ---- the vectorised model (tests/project_lines_model_vec.py) is the loop model, byte for byte ---------------------------
def same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def same_planes(records, width, height, thickness, what):
    want = M.render_line_maps(records, width, height, thickness)
    got = V.render_line_maps(records, width, height, thickness)
    same_bytes(got[0], want[0], f"{what}: line ids")
    same_bytes(got[1], want[1], f"{what}: inverse depths")
    return want


def test_vectorised_stage1_equals_the_loop_model_on_the_existing_cases():
    cams = Cs.stage1_cameras()
    P1, P2, line = Cs.stage1_segments()
    flat = dict(cams[0]); flat["K"] = np.array(cams[0]["K"], np.float64).copy(); flat["K"][2] = 0.0
    for what, cam_list, near in (("the four cameras", cams, 1e-6), ("near = 0.75", cams[:1], 0.75), ("flat K", [flat, cams[1]], 1e-6),
                                 ("near = 1e-45", cams[:1], 1e-45)):
        want = M.project_segments(cam_list, P1, P2, line, near=near)
        got = V.project_segments(cam_list, P1, P2, line, near=near)
        for c in range(len(cam_list)):
            same_bytes(got[c], want[c], f"{what}, camera {c}")
    assert len(V.project_segments([flat], P1, P2, line)[0]) == 0
    assert len(V.project_segments(cams, P1[:0], P2[:0], line[:0])[2]) == 0


def test_vectorised_stage1_equals_the_loop_model_on_a_sample_of_the_large_case():
    cams, P1, P2, line = Cs.stage1_large()
    pick = np.arange(5, 4001, 11)                      # 364 segments
    assert len(pick) >= 300
    seen = 0
    for c in (5, 6, 7, 33, 34):                        # one of each of the four kinds and an empty one
        want = M.project_segments([cams[c]], P1[pick], P2[pick], line[pick])[0]
        same_bytes(V.project_segments([cams[c]], P1[pick], P2[pick], line[pick])[0], want, f"camera {c}")
        seen += len(want)
        # the sample's records are the sampled records of the whole camera: rows of the array form do not see each other
        whole = V.project_camera(cams[c], P1, P2, line)
        part = whole[np.isin(whole["segment"] & M.SEGMENT_MASK, pick)].copy()
        part["segment"] = (part["segment"] & ~np.uint32(M.SEGMENT_MASK)) | np.searchsorted(pick, part["segment"] & M.SEGMENT_MASK).astype(np.uint32)
        same_bytes(part, want, f"camera {c}: sample of the whole")
    assert seen > 500


def test_vectorised_stage2_equals_the_loop_model_on_the_existing_cases():
    for width, height in ((200, 75), (97, 61)):
        rec = Cs.stage2_records(width, height, seed=width)
        for thickness in (1, 3):
            want = same_planes(rec, width, height, thickness, f"{width} x {height}, thickness {thickness}")
            assert (want[0] >= 0).sum() > 1500
    cams, recs = Cs.stage2_multi_camera()
    for k in range(4):
        want = same_planes(recs[k], cams[k]["width"], cams[k]["height"], 3, f"camera {k} of four")
    assert (want[0] == -1).all() and not want[1].any()                               # the camera without records
    rec = Cs.stage2_records(40, 29, seed=3)                                          # coordinates outside the image
    same_planes(rec, 40, 29, 3, "records of a larger image")


def test_vectorised_stage2_equals_the_loop_model_on_the_large_recipe():
    crop = Cs.stage2_large_records(200, 75, 400, seed=7)
    for thickness in (1, 3):
        want = same_planes(crop, 200, 75, thickness, f"200 x 75 by the large recipe, thickness {thickness}")
        assert (want[0] >= 0).sum() > 3000
    assert want[0][37, 80] == 10                                                     # the hand-made tie: the smaller id
    cams, recs = Cs.stage2_large()
    sample = recs[1][3::20]                                                          # 300 of the 6000 records at 1100 x 500
    assert len(sample) == 300
    for thickness in (1, 3):
        want = same_planes(sample, 1100, 500, thickness, f"sample at 1100 x 500, thickness {thickness}")
    assert (want[0] >= 0).sum() > 20000
    count, _ = V.raster_steps(sample, 1100, 500)
    assert count.sum() == sum(len(M.record_pixels(r, 1100, 500)) for r in sample) and (count == 0).sum() > 5 and count.max() > 500


def test_vectorised_stage3_equals_the_loop_model():
    rng = np.random.default_rng(11)
    ids = [M.render_line_maps(Cs.stage2_records(97, 61, 8), 97, 61, 3)[0], M.render_line_maps(Cs.stage2_records(200, 75, 9), 200, 75, 1)[0],
           V.render_line_maps(Cs.stage2_large_records(200, 75, 400, 7), 200, 75, 3)[0]]
    imgs = [rng.integers(0, 256, (61, 128), np.uint8)[:, :97], rng.integers(0, 256, (75, 211, 3), np.uint8)[:, :200],
            rng.integers(0, 256, (75, 200), np.uint8)]
    table = rng.integers(0, 256, (40, 3), np.uint8)
    for alpha in (255, 128, 0):
        for colors in (None, table):
            for k in range(3):
                same_bytes(V.draw_line_map(imgs[k], ids[k], alpha, colors), M.draw_line_map(imgs[k], ids[k], alpha, colors),
                           f"image {k}, alpha {alpha}, colors {'table' if colors is not None else 'palette'}")
    assert (ids[2] >= 40).any() and (ids[2] >= 0).any() and (ids[2] < 40).any()
