"""python -m line3dpp_amd.wireframe IN OUT.obj -d max_distance [-x max_extension] [-a degrees]

Finds where the lines of a 3D line model meet: IN is a result file as save3DLinesAsTXT / save3DLinesAsBIN
write it, .txt or .bin by its extension; two segments of different lines whose carriers come within max_distance of each
other, at an angle of at least `degrees`, at a point on both or at most max_extension beyond an end, form a junction.  The
junctions and the ends that meet nothing are the vertices, the pieces of the segments between them the edges of the
wireframe, which is written to OUT.obj ("v x y z" per vertex, "l i j" per edge).  Prints the summary as one JSON object.
-d is in the model's units and has no default; -x defaults to it."""
import argparse
import json
import sys

from .compare import CompareError
from .merge import read_lines


def _arguments(argv):
    p = argparse.ArgumentParser(prog="python -m line3dpp_amd.wireframe", description="the junctions and the wireframe graph of a 3D line model")
    p.add_argument("input", metavar="IN", help="a result file (.txt or .bin)")
    p.add_argument("output", metavar="OUT.obj", help="the wireframe: vertices and edges")
    p.add_argument("-d", "--max-distance", type=float, required=True, help="largest gap between two lines that meet, in the model's units")
    p.add_argument("-x", "--max-extension", type=float, default=None, help="how far beyond a segment's end they may meet (max-distance)")
    p.add_argument("-a", "--min-angle", type=float, default=10.0, help="smallest angle in degrees [0, 90] (10)")
    p.add_argument("--device", type=int, default=0)
    return p.parse_args(argv)


def run(argv, build_wireframe=None):
    """the program up to its result: writes OUT.obj -> the dict it prints.  build_wireframe: api.build_wireframe, or a
    stand-in with its signature (the tests put the numpy model there)"""
    a = _arguments(argv)
    from .api import flatten_lines, write_wireframe_obj
    if build_wireframe is None:
        from .api import build_wireframe
    if not a.output.lower().endswith(".obj"):
        raise CompareError(f"{a.output}: the wireframe is written as .obj")
    segs, line = flatten_lines(read_lines(a.input))
    wf = build_wireframe(segs, line, max_distance=a.max_distance, max_extension=a.max_extension, min_angle=a.min_angle, device=a.device)
    write_wireframe_obj(wf, a.output)
    res = dict(input=a.input, output=a.output, max_distance=a.max_distance,
               max_extension=a.max_distance if a.max_extension is None else a.max_extension, min_angle=a.min_angle)
    res.update({k: (float(v) if isinstance(v, float) else int(v)) for k, v in wf["summary"].items()})
    return res


def main(argv=None, build_wireframe=None):
    """the program: -> exit status"""
    try:
        print(json.dumps(run(list(sys.argv[1:] if argv is None else argv), build_wireframe)))
    except (CompareError, ValueError, RuntimeError, OSError) as e:
        print(e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
