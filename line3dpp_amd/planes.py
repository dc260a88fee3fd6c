"""python -m line3dpp_amd.planes IN OUT.obj -d max_distance [-j junction_distance] [-x extension] [-a degrees]
                                          [-l min_length] [-s min_segments] [-p max_planes]

Finds the planes that the lines of a 3D line model lie in: IN is a result file as save3DLinesAsTXT /
save3DLinesAsBIN write it, .txt or .bin by its extension.  Two segments of different lines that meet (within
junction_distance, at an angle of at least `degrees`, at most `extension` beyond an end) span a plane; a segment belongs to
it when both its end points lie within max_distance of it.  The planes with at least min_segments members of at least
min_length in all are kept, best-supported first, and written to OUT.obj as one rectangle each ("v x y z" per corner, "f i
j k l" per plane).  Prints the summary as one JSON object.  -d is in the model's units and has no default; -j and -x
default to it."""
import argparse
import json
import sys

from .compare import CompareError
from .merge import read_lines


def _arguments(argv):
    p = argparse.ArgumentParser(prog="python -m line3dpp_amd.planes", description="the planes the lines of a 3D line model lie in")
    p.add_argument("input", metavar="IN", help="a result file (.txt or .bin)")
    p.add_argument("output", metavar="OUT.obj", help="the planes: a rectangle each")
    p.add_argument("-d", "--max-distance", type=float, required=True, help="largest distance of a member's end points from its plane, in the model's units")
    p.add_argument("-j", "--junction-distance", type=float, default=None, help="largest gap between two lines that span a plane (max-distance)")
    p.add_argument("-x", "--junction-extension", type=float, default=None, help="how far beyond a segment's end they may meet (max-distance)")
    p.add_argument("-a", "--min-angle", type=float, default=10.0, help="smallest angle between them in degrees [0, 90] (10)")
    p.add_argument("-l", "--min-length", type=float, default=0.0, help="least summed length of a plane's members (0)")
    p.add_argument("-s", "--min-segments", type=int, default=4, help="least number of members (4)")
    p.add_argument("-p", "--max-planes", type=int, default=64, help="(64)")
    p.add_argument("--device", type=int, default=0)
    return p.parse_args(argv)


def run(argv, detect_planes=None):
    """the program up to its result: writes OUT.obj -> the dict it prints.  detect_planes: api.detect_planes, or a stand-in
    with its signature (the tests put the numpy model there)"""
    a = _arguments(argv)
    from .api import flatten_lines, write_planes_obj
    if detect_planes is None:
        from .api import detect_planes
    if not a.output.lower().endswith(".obj"):
        raise CompareError(f"{a.output}: the planes are written as .obj")
    segs, line = flatten_lines(read_lines(a.input))
    pl = detect_planes(segs, line, max_distance=a.max_distance, junction_distance=a.junction_distance,
                       junction_extension=a.junction_extension, min_angle=a.min_angle, min_length=a.min_length,
                       min_segments=a.min_segments, max_planes=a.max_planes, device=a.device)
    write_planes_obj(pl, a.output)
    res = dict(input=a.input, output=a.output, max_distance=a.max_distance,
               junction_distance=a.max_distance if a.junction_distance is None else a.junction_distance,
               junction_extension=a.max_distance if a.junction_extension is None else a.junction_extension, min_angle=a.min_angle,
               min_length=a.min_length, min_segments=a.min_segments, max_planes=a.max_planes)
    res.update({k: (float(v) if isinstance(v, float) else int(v)) for k, v in pl["summary"].items()})
    return res


def main(argv=None, detect_planes=None):
    """the program: -> exit status"""
    try:
        print(json.dumps(run(list(sys.argv[1:] if argv is None else argv), detect_planes)))
    except (CompareError, ValueError, RuntimeError, OSError) as e:
        print(e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
