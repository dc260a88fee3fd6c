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
