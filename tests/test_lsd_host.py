"""CPU checks of the line-segment detection stage's definitions: fastAtan2, the Gaussian kernel and its
border rule, the resize coordinate map, the tie order of the host cap and the cache file name.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

from line3dpp_amd import io
from tests import lsd_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fast_atan2_axes_and_quadrants():
    f = lambda y, x: float(M.fast_atan2(np.float32(y), np.float32(x)))
    assert f(0, 1) == 0.0 and f(0, 0) == 0.0
    assert abs(f(1, 0) - 90.0) < 1e-4 and abs(f(0, -1) - 180.0) < 1e-4 and abs(f(-1, 0) - 270.0) < 1e-4
    for k in range(-179, 180, 7):                     # every quadrant, within the polynomial's error
        a = math.radians(k + 0.3)
        ref = math.degrees(math.atan2(math.sin(a), math.cos(a))) % 360.0
        got = f(3 * math.sin(a), 3 * math.cos(a))
        assert 0.0 <= got < 360.0
        assert abs(got - ref) < 0.02, (k, got, ref)
    # the quadrant fix-ups are 180 - a and 360 - a on the first-octant value, in float
    a = M.fast_atan2(np.float32(0.25), np.float32(1.0))
    assert M.fast_atan2(np.float32(0.25), np.float32(-1.0)) == np.float32(180.0) - a
    assert M.fast_atan2(np.float32(-0.25), np.float32(1.0)) == np.float32(360.0) - a
    assert M.fast_atan2(np.float32(1.0), np.float32(0.25)) == np.float32(90.0) - a


def test_gaussian_kernel_and_reflect101():
    k = M.gauss_kernel()
    assert len(k) == 7 and abs(k.sum() - 1.0) < 1e-15
    assert all(k[i] == k[6 - i] for i in range(3))
    assert abs(k[3] - 1 / sum(math.exp(-x * x / (2 * 0.75 ** 2)) for x in range(-3, 4))) < 1e-15
    # ksize of lsd_opencv.cpp: 1 + 2 ceil(sigma sqrt(2 * 3 ln 10)) with sigma = 0.6 / 0.8
    assert 1 + 2 * math.ceil(0.75 * math.sqrt(6 * math.log(10.0))) == 7
    assert [M.reflect101(i, 5) for i in range(-3, 8)] == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    # a constant image stays constant up to rounding; a step is smoothed symmetrically
    img = np.full((9, 11), 77, np.uint8)
    assert np.allclose(M.blur(img), 77.0, rtol=0, atol=1e-12)


def test_resize_coordinate_map():
    assert M.resize_size(640, 0.8) == 512 and M.resize_size(63, 0.8) == 50 and M.resize_size(65, 0.8) == 52
    sx, fx = M.resize_map(8, 10, 0.8)                 # fx = (d + 0.5) * 1.25 - 0.5
    assert sx[0] == 0 and fx[0] == np.float32(0.125)
    assert sx[1] == 1 and fx[1] == np.float32(0.375)
    assert sx[7] == 8 and fx[7] == np.float32(0.875)
    sx, fx = M.resize_map(3, 3, 1.0)                  # identity: weights 0, index clamped at the border
    assert list(sx) == [0, 1, 2] and not fx.any()
    # the 8U downscale: weights in 1/2048, rounding shift by 22; a constant stays constant
    g = np.full((30, 40), 201, np.uint8)
    small, upx, upy = M.downscale(g, 20)
    assert small.shape == (15, 20) and (small == 201).all() and upx == np.float32(2.0) and upy == np.float32(2.0)


def test_host_cap_pops_ties_like_std_priority_queue(tmp_path):
    src = tmp_path / "pq.cpp"
    src.write_text(r'''
#include <cstdio>
#include <queue>
#include <vector>
struct S { float len; int id; };
struct Less { bool operator()(const S& a, const S& b) const { return a.len < b.len; } };
int main() {
    unsigned x = 12345;
    for (int t = 0; t < 200; ++t) {
        std::priority_queue<S, std::vector<S>, Less> q;
        int n = 1 + t % 37;
        for (int i = 0; i < n; ++i) { x = x * 1103515245u + 12345u; q.push({float((x >> 16) % 5), i}); }
        std::printf("%d", n);
        while (!q.empty()) { std::printf(" %d", q.top().id); q.pop(); }
        std::printf("\n");
    }
}
''')
    exe = str(tmp_path / "pq")
    subprocess.check_call(["g++", "-std=c++17", "-O2", str(src), "-o", exe])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    x = 12345
    for t, line in enumerate(lines):
        n = 1 + t % 37
        lens = []
        for _ in range(n):
            x = (x * 1103515245 + 12345) & 0xFFFFFFFF
            lens.append(float((x >> 16) % 5))
        want = [int(v) for v in line.split()[1:]]
        assert M.pq_order(lens) == want, t


def test_model_cap_and_filter():
    raw = np.array([[0, 0, 3, 4], [0, 0, 0, 1], [1, 1, 1, 11], [2, 2, 5, 6]], np.float32)   # lengths 5, 1, 10, 5
    out = M.finish(raw, 100, 100, np.float32(1), np.float32(1), max_segments=2)
    assert out.shape == (2, 4) and out[0].tolist() == [1, 1, 1, 11]
    # the length filter uses the ORIGINAL diagonal: 0.005 * sqrt(2) * 200 = 1.41 drops the unit segment
    out = M.finish(raw, 200, 200, np.float32(1), np.float32(1))
    assert len(out) == 3


def test_cache_file_name():
    assert io.segment_cache_name(4, 2457, 1843) == "segments_L3D++_4_2457x1843_3000.bin"
    import ctypes as C
    from line3dpp_amd import _lib
    buf = C.create_string_buffer(128)
    assert _lib.load().l3d_segment_cache_name(4, 1536, 1152, 3000, buf, 128) == 0
    assert buf.value.decode() == "segments_L3D++_4_1536x1152_3000.bin"


@pytest.mark.parametrize("shape", [(48, 64), (61, 77)])
def test_model_flat_image_has_no_segments(shape):
    assert len(M.detect(np.full(shape, 128, np.uint8))) == 0
