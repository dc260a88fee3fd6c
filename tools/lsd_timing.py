"""Wall time of detect_line_segments (k_lsd.hip) on the committed full-size test images, for a batch of 1, of both
images and of both repeated four times.  Per-stage kernel times: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lsd_timing.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from line3dpp_amd.lsd import detect_line_segments, read_image_gray  # noqa: E402


def main():
    gold = os.path.join(ROOT, "tests", "golden", "lsd")
    imgs = [read_image_gray(os.path.join(gold, n)) for n in ("img000055.jpg", "img000056.jpg")]
    detect_line_segments(imgs[:1])                       # first call of the process: runtime set-up
    for batch in (imgs[:1], imgs, imgs * 4):
        t = time.perf_counter()
        segs = detect_line_segments(batch)
        print(f"batch of {len(batch)}: {time.perf_counter() - t:.3f} s, {sum(len(s) for s in segs)} segments")


if __name__ == "__main__":
    main()
