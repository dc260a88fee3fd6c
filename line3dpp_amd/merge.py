"""python -m line3dpp_amd.merge IN OUT.txt -d max_distance [-a degrees] [-o overlap]

Merges the near-duplicate lines of a 3D line model: IN is a result file as save3DLinesAsTXT /
save3DLinesAsBIN write it, .txt or .bin by its extension; lines joined by accepted pairs of segments (the pair test of
line3dpp_amd.compare, between different lines) become one line, and the merged model is written to OUT.txt in the text
form of save3DLinesAsTXT.  A fused line carries the residuals of its members, with their 2D coordinates where IN has
them (a .bin file has none: zeros), concatenated in ascending line index.  Prints the summary as one JSON object.  -d is
in the model's units and has no default."""
import argparse
import json
import os
import sys

import numpy as np

from . import io
from .compare import CompareError


def read_lines(path):
    """a .txt or .bin result file -> the list of lines, each with segments [n, 6], residuals [m, 2], coords2D [m, 4]"""
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".txt", ".bin"):
        raise CompareError(f"{path}: a result file ends in .txt or .bin")
    if not os.path.exists(path):
        raise CompareError(f"{path}: no such file")
    if ext == ".txt":
        return io.read_3d_lines_txt(path)
    return [dict(segments=np.asarray(L["segments"], np.float64).reshape(-1, 9)[:, :6], residuals=L["residuals"],
                 coords2D=np.zeros((len(L["residuals"]), 4), np.float32)) for L in io.read_3d_lines_bin(path)[0]]


def merged_lines(lines, segs_out, line_out, line_map, line, line_info):
    """the list of lines of the merged model: an untouched line as it was, a fused one with the fused segments and its
    members' residuals and coords2D in ascending line index"""
    out = []
    for k, info in enumerate(line_info):
        if info["n_members"] == 1:
            out.append(lines[int(info["label"])])
            continue
        members = np.unique(line[line_map == k])
        out.append(dict(segments=segs_out[line_out == k],
                        residuals=np.concatenate([np.asarray(lines[i]["residuals"], np.uint32).reshape(-1, 2) for i in members]),
                        coords2D=np.concatenate([np.asarray(lines[i]["coords2D"], np.float32).reshape(-1, 4) for i in members])))
    return out


def _arguments(argv):
    p = argparse.ArgumentParser(prog="python -m line3dpp_amd.merge", description="merge the near-duplicate lines of a 3D line model")
    p.add_argument("input", metavar="IN", help="a result file (.txt or .bin)")
    p.add_argument("output", metavar="OUT.txt", help="the merged model, as save3DLinesAsTXT writes one")
    p.add_argument("-d", "--max-distance", type=float, required=True, help="largest distance, in the model's units")
    p.add_argument("-a", "--max-angle", type=float, default=10.0, help="largest angle in degrees [0, 90] (10)")
    p.add_argument("-o", "--min-overlap", type=float, default=0.5, help="smallest overlap share [0, 1] (0.5)")
    p.add_argument("--device", type=int, default=0)
    return p.parse_args(argv)


def run(argv, merge_segments=None):
    """the program up to its result: writes OUT.txt -> the dict it prints.  merge_segments: api.merge_segments, or a
    stand-in with its signature (the tests put the numpy model there)"""
    a = _arguments(argv)
    from .api import flatten_lines
    if merge_segments is None:
        from .api import merge_segments
    if not a.output.lower().endswith(".txt"):
        raise CompareError(f"{a.output}: the merged model is written as .txt")
    lines = read_lines(a.input)
    segs, line = flatten_lines(lines)
    segs_out, line_out, line_map, line_info, summary = merge_segments(segs, line, max_distance=a.max_distance, max_angle=a.max_angle,
                                                                      min_overlap=a.min_overlap, device=a.device)
    with open(a.output, "w") as f:
        f.write(io.format_3d_lines_txt(merged_lines(lines, segs_out, line_out, line_map, line, line_info)))
    res = dict(input=a.input, output=a.output, max_distance=a.max_distance, max_angle=a.max_angle, min_overlap=a.min_overlap)
    res.update({k: (float(v) if isinstance(v, float) else int(v)) for k, v in summary.items()})
    return res


def main(argv=None, merge_segments=None):
    """the program: -> exit status"""
    try:
        print(json.dumps(run(list(sys.argv[1:] if argv is None else argv), merge_segments)))
    except (CompareError, ValueError, RuntimeError, OSError) as e:
        print(e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
