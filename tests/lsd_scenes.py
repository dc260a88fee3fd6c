"""Synthetic 8-bit test images for the line-segment detection tests: anti-aliased polygons and lines with noise."""
import numpy as np


def polygons(w, h, seed=0, n_poly=4, noise=3.0, rgb=False):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w, 3) if rgb else (h, w), 90.0)
    for _ in range(n_poly):
        cx, cy = rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h
        a = rng.uniform(0, np.pi)
        r1, r2 = rng.uniform(0.1, 0.3) * w, rng.uniform(0.05, 0.25) * h
        u = (xx - cx) * np.cos(a) + (yy - cy) * np.sin(a)
        v = -(xx - cx) * np.sin(a) + (yy - cy) * np.cos(a)
        cover = np.clip(np.minimum(r1 - np.abs(u), r2 - np.abs(v)) + 0.5, 0, 1)
        amp = rng.uniform(-80, 80, 3 if rgb else 1)
        img += cover[..., None] * amp if rgb else cover * amp[0]
    for _ in range(3):                                  # thin anti-aliased lines
        x0, y0, x1, y1 = rng.uniform(0, 1, 4) * [w, h, w, h]
        d = np.hypot(x1 - x0, y1 - y0) + 1e-9
        dist = np.abs((xx - x0) * (y1 - y0) - (yy - y0) * (x1 - x0)) / d
        t = ((xx - x0) * (x1 - x0) + (yy - y0) * (y1 - y0)) / (d * d)
        cover = np.clip(1.5 - dist, 0, 1) * ((t >= 0) & (t <= 1))
        amp = rng.uniform(60, 120)
        img += cover[..., None] * amp if rgb else cover * amp
    img += rng.normal(0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def edge_at_border(w, h):
    """the strongest edge in the last row and the last column"""
    img = np.full((h, w), 60, np.uint8)
    img[-1, :] = 220
    img[:, -1] = 220
    img[h // 3:h // 2, w // 4:3 * w // 4] = 120
    return img


def tiles(w, h, step, sq):
    """identical bright squares on a grid: many segments of exactly equal length (the tie order of the length heap)"""
    img = np.full((h, w), 70, np.uint8)
    for y in range(step // 2, h - sq, step):
        for x in range(step // 2, w - sq, step):
            img[y:y + sq, x:x + sq] = 200
    return img


def bars(w, h):
    """bright bars 14 px high from row 16, 8 to 40 px long in steps of 1, 30 px apart from column 22: segment lengths on
    both sides of the length filter's threshold (0.005 x the diagonal); the canvas sets the threshold, not the bars"""
    img = np.full((h, w), 70, np.uint8)
    x = 22
    for length in range(8, 41):
        img[16:30, x:x + length] = 200
        x += length + 30
    assert x < w and h >= 48
    return img


def rings(w, h):
    """128 + 100 sin(r / 3) around the centre: curved regions that refine re-grows and reduce_region_radius shrinks"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r = np.hypot(xx - (w - 1) / 2, yy - (h - 1) / 2)
    return np.clip(np.rint(128 + 100 * np.sin(r / 3)), 0, 255).astype(np.uint8)


def noise(w, h, seed):
    """uniform 8-bit noise"""
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# ---- the cases of tests/test_lsd_cases.py (CPU: the model reaches what each case is for) and
# tests/test_gpu_lsd_stages.py (GPU against the model) ---------------------------------------------------------------
# stage comparison at small and awkward sizes: (w, h, seed) of uniform noise.  2x2 is the image without a defined gradient.
TINY = [(2, 2, 2), (9, 2, 0), (2, 9, 0), (3, 3, 0), (7, 5, 0), (6, 6, 2), (257, 3, 0), (3, 257, 0)]


def tiny_batch():
    return [noise(w, h, s) for (w, h, s) in TINY] + [polygons(64, 48, 0), polygons(65, 49, 1)]


MIXED_WIDTH = 250


def mixed_batch():
    """max_image_width = 250: downscaled, RGB not downscaled, portrait downscaled, RGB downscaled, 3x3, flat"""
    return [polygons(400, 300, 8), polygons(200, 150, 7, rgb=True), polygons(233, 301, 9),
            polygons(301, 233, 10, rgb=True), noise(3, 3, 0), np.full((120, 160), 128, np.uint8)]


SYNTH_WALK = [(64, 48, 0), (65, 49, 1), (97, 131, 2), (160, 120, 3), (241, 179, 4), (320, 240, 5)]


def walk_cases():
    """name -> (image, max_image_width): the raw list and the statistics of the walk"""
    c = {"rings": (rings(160, 120), -1), "noise": (noise(128, 96, 1), -1), "tiles160": (tiles(160, 120, 24, 12), -1),
         "tiles320": (tiles(320, 240, 40, 20), 200), "polygons_noisy": (polygons(160, 120, 3, noise=12.0), -1)}
    for (w, h, seed) in SYNTH_WALK:
        c[f"synth{w}x{h}"] = (polygons(w, h, seed), -1)
    return c


TILES = ["tiles160", "tiles320"]
# the length filter: threshold 16.0018 px with and without the downscale; and a canvas whose threshold, 16.250183 px, is
# the float32 length of one raw segment exactly (`>` keeps it out, `>=` would let it in)
BARS = {"bars": (3200, 48, -1), "bars_down": (3200, 48, 1600), "bars_on_threshold": (3244, 198, -1)}


def all_cases():
    c = walk_cases()
    for name, (w, h, mw) in BARS.items():
        c[name] = (bars(w, h), mw)
    return c
