"""python -m line3dpp_amd.compare A B -d max_distance [-a degrees] [-o overlap]
   python -m line3dpp_amd.compare A --duplicates -d max_distance [-a degrees] [-o overlap]

Compares two 3D line models -- result files as saveResultAsTXT / save3DLinesAsBIN write them, .txt or .bin
by their extension -- in both directions on the GPU and prints one JSON object: both summaries and, per direction, the
median and the 90th percentile of the distance over the matched segments.  --duplicates takes one file and compares it
with itself, pairs of the same line left out: the segments and lines that have a counterpart on another line.  -d is in
the model's units and has no default; the models must be in one frame."""
import argparse
import json
import os
import sys

import numpy as np

from . import io


class CompareError(Exception):
    pass


def read_model(path):
    """a .txt or .bin result file -> (segs [n, 6] float64, line [n] uint32)"""
    from .api import flatten_lines
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".txt", ".bin"):
        raise CompareError(f"{path}: a result file ends in .txt or .bin")
    if not os.path.exists(path):
        raise CompareError(f"{path}: no such file")
    lines = io.read_3d_lines_txt(path) if ext == ".txt" else io.read_3d_lines_bin(path)[0]
    return flatten_lines(lines)


def _arguments(argv):
    p = argparse.ArgumentParser(prog="python -m line3dpp_amd.compare", description="compare two 3D line models")
    p.add_argument("files", nargs="+", metavar="FILE", help="two result files (.txt or .bin); one with --duplicates")
    p.add_argument("-d", "--max-distance", type=float, required=True, help="largest distance, in the model's units")
    p.add_argument("-a", "--max-angle", type=float, default=10.0, help="largest angle in degrees [0, 90] (10)")
    p.add_argument("-o", "--min-overlap", type=float, default=0.5, help="smallest overlap share [0, 1] (0.5)")
    p.add_argument("--duplicates", action="store_true", help="one file against itself, pairs of the same line left out")
    p.add_argument("--device", type=int, default=0)
    a = p.parse_args(argv)
    if len(a.files) != (1 if a.duplicates else 2):
        p.error("--duplicates takes one file" if a.duplicates else "two files are compared")
    return a


def _direction(summary, matches):
    out = {k: (float(v) if isinstance(v, float) else int(v)) for k, v in summary.items()}
    d = matches["distance"][matches["segment"] >= 0]
    out["distance_median"] = float(np.median(d)) if len(d) else None
    out["distance_p90"] = float(np.percentile(d, 90)) if len(d) else None
    return out


def run(argv, compare_segments=None):
    """the program up to its result: -> the dict it prints.  compare_segments: api.compare_segments, or a stand-in with
    its signature (the tests put the numpy model there)"""
    a = _arguments(argv)
    if compare_segments is None:
        from .api import compare_segments
    par = dict(max_distance=a.max_distance, max_angle=a.max_angle, min_overlap=a.min_overlap, device=a.device)
    if a.duplicates:
        segs, line = read_model(a.files[0])
        m, _, s, _ = compare_segments(segs, line, segs, line, exclude_same_line=True, **par)
        hit = m["segment"] >= 0
        return dict(file=a.files[0], max_distance=a.max_distance, max_angle=a.max_angle, min_overlap=a.min_overlap,
                    n_segments=int(len(line)), n_lines=int(len(np.unique(line))), n_duplicate_segments=int(hit.sum()),
                    n_duplicate_lines=int(len(np.unique(line[hit]))))
    qs, ql = read_model(a.files[0])
    rs, rl = read_model(a.files[1])
    mq, mr, sq, sr = compare_segments(qs, ql, rs, rl, exclude_same_line=False, **par)
    return dict(a=a.files[0], b=a.files[1], max_distance=a.max_distance, max_angle=a.max_angle, min_overlap=a.min_overlap,
                a_in_b=_direction(sq, mq), b_in_a=_direction(sr, mr))


def main(argv=None, compare_segments=None):
    """the program: -> exit status"""
    try:
        print(json.dumps(run(list(sys.argv[1:] if argv is None else argv), compare_segments)))
    except (CompareError, ValueError, RuntimeError) as e:
        print(e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
