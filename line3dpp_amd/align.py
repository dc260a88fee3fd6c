"""python -m line3dpp_amd.align A B -d max_distance [-s start_distance] [-a degrees] [-o overlap] [--init FILE]
                                [--no-scale] [--out OUT.txt]

Aligns the 3D line model A to the model B: the result files of two reconstructions of one scene, .txt or
.bin by their extension, whose frames differ by a similarity transform -- another SfM tool's gauge, a surveyed ground
truth.  Iterated closest lines on the GPU from the start --init gives (FILE: a 3x4 or 4x4 matrix as text; default
identity), the gate halving from -s down to -d.  Prints one JSON object: the similarity (scale, quaternion w x y z,
translation), its 4x4 matrix, the summary of the alignment, and the comparison of both directions after it as
line3dpp_amd.compare prints it.  --out writes A under the transform, in the text form of save3DLinesAsTXT.  -d and -s
are in B's units; -d has no default."""
import argparse
import json
import sys

import numpy as np

from . import io
from .compare import CompareError
from .merge import read_lines


def _arguments(argv):
    p = argparse.ArgumentParser(prog="python -m line3dpp_amd.align", description="align one 3D line model to another")
    p.add_argument("a", metavar="A", help="the model that is moved (.txt or .bin)")
    p.add_argument("b", metavar="B", help="the model that stays (.txt or .bin)")
    p.add_argument("-d", "--max-distance", type=float, required=True, help="largest distance of a match, in B's units")
    p.add_argument("-s", "--start-distance", type=float, default=0.0, help="the gate of the first iteration (0: max-distance)")
    p.add_argument("-a", "--max-angle", type=float, default=10.0, help="largest angle in degrees [0, 90] (10)")
    p.add_argument("-o", "--min-overlap", type=float, default=0.5, help="smallest overlap share [0, 1] (0.5)")
    p.add_argument("--init", metavar="FILE", help="the start: a 3x4 or 4x4 matrix as text")
    p.add_argument("--no-scale", action="store_true", help="keep the scale of the start")
    p.add_argument("--out", metavar="OUT.txt", help="write A under the transform")
    p.add_argument("--device", type=int, default=0)
    return p.parse_args(argv)


def read_matrix(path):
    try:
        M = np.loadtxt(path, dtype=np.float64)
    except (OSError, ValueError) as e:
        raise CompareError(f"{path}: {e}")
    if M.shape not in ((3, 4), (4, 4)):
        raise CompareError(f"{path}: a start is a 3x4 or 4x4 matrix")
    return M


def direction_summary(segs, line, matches):
    """one direction of the comparison after alignment: the fields of l3d_compare_summary from the records, the lengths
    added in ascending index order, with the median and the 90th percentile of the distance"""
    e = segs[:, 3:6] - segs[:, 0:3]
    length = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
    hit = matches["segment"] >= 0
    total = np.cumsum(length); got = np.cumsum(length[hit])
    d = matches["distance"][hit]
    return dict(n_segments=int(len(segs)), n_matched=int(hit.sum()), n_ambiguous=int((matches["n_accepted"] > 1).sum()),
                n_lines=int(len(np.unique(line))), n_lines_matched=int(len(np.unique(line[hit]))),
                length_total=float(total[-1]) if len(total) else 0.0, length_matched=float(got[-1]) if len(got) else 0.0,
                distance_median=float(np.median(d)) if len(d) else None, distance_p90=float(np.percentile(d, 90)) if len(d) else None)


def run(argv, align_segments=None):
    """the program up to its result: -> the dict it prints.  align_segments: api.align_segments, or a stand-in with its
    signature (the tests put the numpy model there)"""
    a = _arguments(argv)
    from .api import flatten_lines
    if align_segments is None:
        from .api import align_segments
    if a.out and not a.out.lower().endswith(".txt"):
        raise CompareError(f"{a.out}: the moved model is written as .txt")
    lines = read_lines(a.a)
    qs, ql = flatten_lines(lines)
    rs, rl = flatten_lines(read_lines(a.b))
    initial = read_matrix(a.init) if a.init else None
    res = align_segments(qs, ql, rs, rl, max_distance=a.max_distance, start_distance=a.start_distance, initial=initial,
                         estimate_scale=not a.no_scale, max_angle=a.max_angle, min_overlap=a.min_overlap, device=a.device)
    if a.out:
        moved, at = [], 0
        for L in lines:
            n = len(L["segments"])
            moved.append(dict(L, segments=res["segments"][at:at + n]))
            at += n
        with open(a.out, "w") as f:
            f.write(io.format_3d_lines_txt(moved))
    sim, summary = res["similarity"], res["summary"]
    return dict(a=a.a, b=a.b, out=a.out, max_distance=a.max_distance, start_distance=a.start_distance, max_angle=a.max_angle,
                min_overlap=a.min_overlap, estimate_scale=not a.no_scale,
                similarity=dict(scale=float(sim["scale"]), q=[float(v) for v in sim["q"]], t=[float(v) for v in sim["t"]]),
                matrix=[[float(v) for v in row] for row in np.asarray(res["matrix"])],
                summary=dict(status=summary["status"], iterations=int(summary["iterations"]), n_matched=int(summary["n_matched"]),
                             rms=float(summary["rms"]), last_step=float(summary["last_step"]), diag=float(summary["diag"]),
                             center=[float(v) for v in summary["center"]]),
                a_in_b=direction_summary(res["segments"], ql, res["matches_q"]), b_in_a=direction_summary(rs, rl, res["matches_r"]))


def main(argv=None, align_segments=None):
    """the program: -> exit status"""
    try:
        print(json.dumps(run(list(sys.argv[1:] if argv is None else argv), align_segments)))
    except (CompareError, ValueError, RuntimeError, OSError) as e:
        print(e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
