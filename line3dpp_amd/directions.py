"""python -m line3dpp_amd.directions IN OUT.obj -a degrees [-l min_length] [-s min_segments] [-p max_directions]
                                              [-f frame_degrees] [--out UPRIGHT.txt]

Finds the directions that the lines of a 3D line model run in: IN is a result file as save3DLinesAsTXT /
save3DLinesAsBIN write it, .txt or .bin by its extension.  The direction of every segment is a hypothesis; a segment
belongs to it when the angle between them is at most `degrees`, either way round.  The directions with at least
min_segments members of at least min_length in all are kept, best-supported first, and written to OUT.obj as one line
each ("v x y z" for both ends, "l i j").  The frame is the rotation that turns the heaviest directions that are orthogonal
within frame_degrees into the coordinate axes; --out writes the model under it, in the text form of save3DLinesAsTXT.
Prints the summary as one JSON object.  -a has no default."""
import argparse
import json
import sys

import numpy as np

from . import io
from .compare import CompareError
from .merge import read_lines


def _arguments(argv):
    p = argparse.ArgumentParser(prog="python -m line3dpp_amd.directions", description="the directions the lines of a 3D line model run in")
    p.add_argument("input", metavar="IN", help="a result file (.txt or .bin)")
    p.add_argument("output", metavar="OUT.obj", help="the directions: a line each")
    p.add_argument("-a", "--max-angle", type=float, required=True, help="largest angle between a member and its direction in degrees [0, 90]")
    p.add_argument("-l", "--min-length", type=float, default=0.0, help="least summed length of a direction's members (0)")
    p.add_argument("-s", "--min-segments", type=int, default=4, help="least number of members (4)")
    p.add_argument("-p", "--max-directions", type=int, default=16, help="(16)")
    p.add_argument("-f", "--frame-angle", type=float, default=5.0, help="how far from 90 degrees two axes of the frame may be, in degrees (5)")
    p.add_argument("--out", metavar="UPRIGHT.txt", help="write the model under the frame's rotation")
    p.add_argument("--device", type=int, default=0)
    return p.parse_args(argv)


def run(argv, detect_directions=None):
    """the program up to its result: writes OUT.obj (and --out) -> the dict it prints.  detect_directions:
    api.detect_directions, or a stand-in with its signature (the tests put the numpy model there)"""
    a = _arguments(argv)
    from .api import flatten_lines, similarity_from_matrix, transform_segments, write_directions_obj
    if detect_directions is None:
        from .api import detect_directions
    if not a.output.lower().endswith(".obj"):
        raise CompareError(f"{a.output}: the directions are written as .obj")
    if a.out and not a.out.lower().endswith(".txt"):
        raise CompareError(f"{a.out}: the upright model is written as .txt")
    lines = read_lines(a.input)
    segs, line = flatten_lines(lines)
    dr = detect_directions(segs, line, max_angle=a.max_angle, min_length=a.min_length, min_segments=a.min_segments,
                           max_directions=a.max_directions, frame_angle=a.frame_angle, device=a.device)
    write_directions_obj(dr, a.output)
    if a.out:
        M = np.zeros((3, 4)); M[:, :3] = np.asarray(dr["R"], np.float64).reshape(3, 3)
        moved_segs = transform_segments(segs, similarity_from_matrix(M))
        moved, at = [], 0
        for L in lines:
            n = len(L["segments"])
            moved.append(dict(L, segments=moved_segs[at:at + n]))
            at += n
        with open(a.out, "w") as f:
            f.write(io.format_3d_lines_txt(moved))
    res = dict(input=a.input, output=a.output, out=a.out, max_angle=a.max_angle, min_length=a.min_length, min_segments=a.min_segments,
               max_directions=a.max_directions, frame_angle=a.frame_angle)
    for k, v in dr["summary"].items():
        res[k] = [float(x) if isinstance(x, float) else int(x) for x in v] if isinstance(v, (list, tuple)) else \
            float(v) if isinstance(v, float) else int(v)
    return res


def main(argv=None, detect_directions=None):
    """the program: -> exit status"""
    try:
        print(json.dumps(run(list(sys.argv[1:] if argv is None else argv), detect_directions)))
    except (CompareError, ValueError, RuntimeError, OSError) as e:
        print(e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
