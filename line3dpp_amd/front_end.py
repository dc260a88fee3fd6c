"""Run a dataset end to end: the reference's six front ends main_vsfm.cpp, main_colmap.cpp, main_bundler.cpp,
main_pix4d.cpp, main_openmvg.cpp and main_mavmap.cpp.

    python -m line3dpp_amd.front_end vsfm    -m result.nvm [-i image_folder] [flags]
    python -m line3dpp_amd.front_end colmap  -i image_folder [-m sfm_folder] [flags]
    python -m line3dpp_amd.front_end bundler -i image_folder [-b bundle.rd.out] [-f image_list] [-t extension] [flags]
    python -m line3dpp_amd.front_end pix4d   -i image_folder -b params_folder -f project_prefix [flags]
    python -m line3dpp_amd.front_end openmvg -i image_folder -j sfm_data.json [flags]
    python -m line3dpp_amd.front_end mavmap  -i image_folder -b image-data.txt -t extension [-f image_prefix] [flags]

Each program takes the flags of its reference main (FLAGS below: short and long name, required or not, default), reads
the SfM result with the readers of io.py, looks its images up as that main does, and drives `Line3D` through the
reference's call sequence: undistortImage where a camera has distortion, addImage, matchImages, reconstruct3Dlines,
get3Dlines, then the STL, OBJ, TXT and BIN writers into the output folder.  `run_vsfm`, `run_colmap`, `run_bundler`,
`run_pix4d`, `run_openmvg` and `run_mavmap` are the same programs as functions; they return the `Line3D` object and the
wall-clock seconds per stage.  Pix4D gives no 3D points: its program triangulates every tie point on the GPU
(api.triangulate_points) while it reads the project, before `Line3D` is constructed.

What differs from the reference:
- images go through the library in chunks: a chunk is read on the host, the images that need it are undistorted in ONE
  `undistort_images` call (those of a COLMAP camera model beyond five coefficients in ONE `undistort_images_model`
  call) and the chunk is added with ONE `Line3D.addImages` call, so that line-segment detection runs as
  one batch per chunk (the reference does all three image by image, one image per OpenMP thread).  A chunk is bounded by
  CHUNK_BYTES of decoded pixels; the result does not depend on the chunking;
- `-g / --use_cuda` is accepted and ignored: the library has no CPU path;
- `-c / --use_ceres` defaults to 0, as in a reference build without Ceres.
"""
import os
import sys
import time

import numpy as np

from . import io

PREFIX = "[L3D++] "

# decoded pixels held per chunk, in bytes (README, switch table).  The detection arena on the device is about 80 B per
# pixel, so the default keeps a chunk of 8-bit grey images near 20 GB of device memory.
CHUNK_BYTES = 256 << 20
CHUNK_ENV = "L3D_FRONT_END_CHUNK_BYTES"

STAGES = ("read", "undistort", "add", "match", "reconstruct", "save")

_NOT_HERE_G = " (accepted and ignored: this library has no CPU path)"
_NOT_HERE_C = " (default 0, as in a reference build without Ceres; 1 bundles the 3D lines on the GPU)"

# (short, long, type, required, default, help): the numeric flags the six mains share (main_vsfm.cpp:53-92, commons.h:40-88)
_COMMON = [
    ("w", "max_image_width", int, False, -1, "scale image down to fixed max width for line segment detection"),
    ("n", "num_matching_neighbors", int, False, 10, "number of neighbors for matching"),
    ("a", "sigma_a", float, False, 10.0, "angle regularizer"),
    ("p", "sigma_p", float, False, 2.5, "position regularizer (if negative: fixed sigma_p in world-coordinates)"),
    ("e", "min_epipolar_overlap", float, False, 0.25, "minimum epipolar overlap for matching"),
    ("k", "knn_matches", int, False, 10, "number of matches to be kept (<= 0 --> use all that fulfill overlap)"),
    ("y", "num_segments_per_image", int, False, 3000, "maximum number of 2D segments per image (longest)"),
    ("v", "visibility_t", int, False, 3, "minimum number of cameras to see a valid 3D line"),
    ("d", "diffusion", bool, False, False, "perform Replicator Dynamics Diffusion before clustering"),
    ("l", "load_and_store_flag", bool, False, True, "load/store segments (recommended for big images)"),
    ("r", "collinearity_t", float, False, -1.0, "threshold for collinearity"),
    ("g", "use_cuda", bool, False, True, "use the GPU" + _NOT_HERE_G),
    ("c", "use_ceres", bool, False, False, "optimize the 3D lines" + _NOT_HERE_C),
    ("z", "const_reg_depth", float, False, -1.0, "use a constant regularization depth (only when sigma_p is metric!)"),
]

FLAGS = {
    "vsfm": [   # main_vsfm.cpp:44-92
        ("i", "input_folder", str, False, "", "folder containing the images (if not specified, path in .nvm file is expected to be correct)"),
        ("m", "nvm_file", str, True, ".", "full path to the VisualSfM result file (.nvm)"),
        ("o", "output_folder", str, False, "", "folder where result and temporary files are stored (if not specified --> input_folder+'/Line3D++/')"),
    ] + _COMMON,
    "colmap": [  # main_colmap.cpp:41-89
        ("i", "input_folder", str, True, "", "folder containing the images"),
        ("m", "sfm_folder", str, False, "", "full path to the colmap result files (cameras.txt, images.txt, and points3D.txt), if not specified --> input_folder"),
        ("o", "output_folder", str, False, "", "folder where result and temporary files are stored (if not specified --> sfm_folder+'/Line3D++/')"),
    ] + _COMMON,
    "bundler": [  # main_bundler.cpp:42-96
        ("i", "image_folder", str, True, ".", "folder containing the images (be carefull with the path if an image list is used!)"),
        ("b", "bundle_file", str, False, "", "full path to the bundle.*.out file (if not specified -> image_folder/../bundle.rd.out)"),
        ("f", "img_list", str, False, "", "full path to an optional image list (e.g. for the Dubrovnik6K dataset)"),
        ("t", "image_extension", str, False, "", "image extension (case sensitive), if not specified: jpg, png or bmp expected"),
        ("o", "output_folder", str, False, "", "folder where result and temporary files are stored (if not specified --> input_folder+'/Line3D++/')"),
    ] + _COMMON,
    "pix4d": [  # main_pix4d.cpp:84-136
        ("i", "input_folder", str, True, ".", "folder containing the images"),
        ("b", "params_folder", str, True, "", "folder containing the project files <project_prefix>_calibrated_camera_parameters.txt and <project_prefix>_tp_pix4d.txt"),
        ("f", "project_prefix", str, True, "", "project name and output file prefix"),
        ("o", "output_folder", str, False, "", "folder where result and temporary files are stored (if not specified --> image_folder+'/Line3D++/')"),
    ] + _COMMON,
    "openmvg": [  # main_openmvg.cpp:45-94
        ("i", "input_folder", str, True, ".", "folder containing the original images"),
        ("j", "sfm_json_file", str, True, ".", "full path to the OpenMVG result file (sfm_data.json)"),
        ("o", "output_folder", str, False, "", "folder where result and temporary files are stored (if not specified --> input_folder+'/Line3D++/')"),
    ] + _COMMON,
    "mavmap": [  # main_mavmap.cpp:43-98
        ("i", "input_folder", str, True, ".", "folder containing the images"),
        ("b", "mavmap_output", str, True, "", "full path to the mavmap output (image-data-*.txt)"),
        ("t", "image_extension", str, False, "", "image extension (case sensitive); mavmap needs it: without it the file looked for ends in a bare '.'"),
        ("f", "image_prefix", str, False, "", "optional image prefix"),
        ("o", "output_folder", str, False, "", "folder where result and temporary files are stored (if not specified --> input_folder+'/Line3D++/')"),
    ] + _COMMON,
}

BUNDLER_EXTENSIONS = (".jpg", ".JPG", ".png", ".PNG", ".jpeg", ".JPEG", ".bmp", ".BMP")   # main_bundler.cpp:301-308


class FrontEndError(Exception):
    """what ends a program with a non-zero status: a wrong command line, or an error the reference's main ends on"""

    def __init__(self, message, status=1):
        super().__init__(message)
        self.status = int(status)


class UsageError(FrontEndError):
    """a command line the program cannot read: the usage text follows the message"""


def usage(program):
    rows = [f"usage: python -m line3dpp_amd.front_end {program} <flags>", ""]
    for short, name, typ, required, default, text in FLAGS[program]:
        kind = {str: "string", int: "int", float: "float", bool: "0|1"}[typ]
        default = int(default) if typ is bool else default
        rows.append(f"  -{short}, --{name} <{kind}>  {'(required) ' if required else ''}{text}"
                    + ("" if required else f" [default: {default!r}]"))
    return "\n".join(rows)


def _value(typ, text, key):
    try:
        if typ is str:
            return text
        if typ is int:
            return int(text)
        if typ is float:
            return np.float32(float(text))              # TCLAP::ValueArg<float>
        if text in ("0", "1"):                          # what the stream extraction of a bool accepts
            return text == "1"
    except ValueError:
        pass
    raise UsageError(f"argument {key}: cannot read '{text}' as {'0 or 1' if typ is bool else typ.__name__}")


def parse_args(program, argv):
    """-> dict long name -> value; flags come as `-f value` or `--name value` (a value may start with '-')"""
    table = FLAGS[program]
    values = {name: (np.float32(default) if typ is float else default) for _, name, typ, _, default, _ in table}
    keys = {}
    for short, name, typ, _, _, _ in table:
        keys["-" + short] = keys["--" + name] = (name, typ)
    argv = list(argv)
    seen = set()
    for i in range(0, len(argv), 2):
        key = argv[i]
        if key not in keys:
            raise UsageError(f"unknown argument {key}")
        if i + 1 >= len(argv):
            raise UsageError(f"argument {key}: value missing")
        name, typ = keys[key]
        if name in seen:
            raise UsageError(f"argument {key}: given more than once")
        seen.add(name)
        values[name] = _value(typ, argv[i + 1], key)
    for short, name, _, required, _, _ in table:
        if required and name not in seen:
            raise UsageError(f"required argument missing: -{short} / --{name}")
    return values


def _settings(a, output_folder):
    """the values as the mains normalise them (main_vsfm.cpp:100-133)"""
    return dict(
        output_folder=output_folder,
        load_segments=bool(a["load_and_store_flag"]),
        max_img_width=int(a["max_image_width"]),
        max_line_segments=int(a["num_segments_per_image"]) & 0xFFFFFFFF,         # unsigned int there
        use_gpu=bool(a["use_cuda"]),
        use_ceres=bool(a["use_ceres"]),
        neighbors=max(int(a["num_matching_neighbors"]), 2),
        epipolar_overlap=float(min(abs(np.float32(a["min_epipolar_overlap"])), np.float32(0.99))),
        sigma_a=float(abs(np.float32(a["sigma_a"]))),
        sigma_p=float(a["sigma_p"]),
        kNN=int(a["knn_matches"]),
        visibility_t=int(a["visibility_t"]) & 0xFFFFFFFF,
        diffusion=bool(a["diffusion"]),
        collinearity_t=float(a["collinearity_t"]),
        const_reg_depth=float(a["const_reg_depth"]),
    )


def undistort_images(images, Ks, radials, tangentials):
    """the default `undistort`: lsd.undistort_images, one batch.  An image that could not be read arrives empty; OpenCV
    refuses it inside the reference's undistortImage, here it is reported and handed on empty, and addImage refuses it."""
    from . import lsd
    out = list(images)
    real = [i for i, im in enumerate(images) if im.size]
    if len(real) < len(out):
        print(f"{PREFIX}ERROR: undistortImage: {len(out) - len(real)} empty image(s)")
    if real:
        done = lsd.undistort_images([images[i] for i in real], [Ks[i] for i in real], [radials[i] for i in real],
                                    [tangentials[i] for i in real])
        for i, im in zip(real, done):
            out[i] = im
    return out


def undistort_images_model(images, models, Ks, params):
    """the default `undistort_model`: lsd.undistort_images_model, one batch; empty images as undistort_images treats them"""
    from . import lsd
    out = list(images)
    real = [i for i, im in enumerate(images) if im.size]
    if len(real) < len(out):
        print(f"{PREFIX}ERROR: undistortImage: {len(out) - len(real)} empty image(s)")
    if real:
        done = lsd.undistort_images_model([images[i] for i in real], [models[i] for i in real], [Ks[i] for i in real],
                                          [params[i] for i in real])
        for i, im in zip(real, done):
            out[i] = im
    return out


def _chunk_bytes():
    return int(os.environ.get(CHUNK_ENV, CHUNK_BYTES))


def run_views(kind, views, s, line3d_factory=None, read_image=None, undistort=None, neighbors_by_worldpoints=True,
              undistort_model=None):
    """The shared core.  `views`: what a main's image loop visits, in its order, as (camera id, image path, entry of the
    io reader); `s`: _settings; `neighbors_by_worldpoints`: what the main constructs Line3D with (main_mavmap.cpp:150-151
    hands over neighbour lists, the others worldpoint lists).  -> (Line3D object, seconds per stage)"""
    if line3d_factory is None:
        from .api import Line3D as line3d_factory
    if read_image is None:
        from .lsd import read_image_gray

        def read_image(path):
            try:
                return read_image_gray(path)
            except (OSError, ValueError, SyntaxError):         # no such file, or PIL cannot decode it
                return None
    if undistort is None:
        undistort = undistort_images
    if undistort_model is None:
        undistort_model = undistort_images_model
    times = dict.fromkeys(STAGES, 0.0)

    def timed(stage, fn, *args):
        t0 = time.perf_counter()
        out = fn(*args)
        times[stage] += time.perf_counter() - t0
        return out

    os.makedirs(s["output_folder"], exist_ok=True)
    line3d = line3d_factory(s["output_folder"], s["load_segments"], s["max_img_width"], s["max_line_segments"],
                            neighbors_by_worldpoints, s["use_gpu"])
    budget = _chunk_bytes()
    chunk, held = [], 0

    def flush():
        todo = [v for v in chunk if v["undistortion"] is not None]
        if todo:
            done = timed("undistort", undistort, [v["image"] for v in todo], *zip(*[v["undistortion"] for v in todo]))
            for v, im in zip(todo, done):
                v["image"] = im
        todo = [v for v in chunk if v["camera_model"] is not None]      # COLMAP's models beyond five coefficients
        if todo:
            done = timed("undistort", undistort_model, [v["image"] for v in todo], *zip(*[v["camera_model"] for v in todo]))
            for v, im in zip(todo, done):
                v["image"] = im
        add = [v for v in chunk if v["add"]]
        if add:
            timed("add", line3d.addImages, [v["id"] for v in add], [v["image"] for v in add], [v["K"] for v in add],
                  [v["entry"]["R"] for v in add], [v["entry"]["t"] for v in add],
                  [float(v["entry"]["median_depth"]) for v in add], [v["entry"]["worldpoints"] for v in add])
        chunk.clear()

    for cam_id, path, entry in views:
        image = timed("read", read_image, path)
        if image is None:
            print(f"{PREFIX}WARNING: image '{path}' could not be read!")
            image = np.zeros((0, 0), np.uint8)                 # cv::imread's empty Mat: 0 x 0 from here on, as there
        rows, cols = image.shape[:2]
        model = io.front_end_camera_model(kind, entry, cols, rows)
        und = io.front_end_undistortion(kind, entry, cols, rows) if model is None else None
        K = entry["K"] if "K" in entry else io.nvm_intrinsics(entry["focal"], cols, rows)   # .nvm, bundler: from the image size
        if chunk and held + image.nbytes > budget:
            flush()
            held = 0
        chunk.append(dict(id=cam_id, image=image, entry=entry, K=K, undistortion=und, camera_model=model,
                          add=kind == "mavmap" or bool(entry["worldpoints"])))
        held += image.nbytes
    flush()

    ok = timed("match", line3d.matchImages, s["sigma_p"], s["sigma_a"], s["neighbors"], s["epipolar_overlap"], s["kNN"],
               s["const_reg_depth"])
    if ok is False:
        raise FrontEndError("matchImages failed", 4)
    ok = timed("reconstruct", line3d.reconstruct3Dlines, s["visibility_t"], s["diffusion"], s["collinearity_t"], s["use_ceres"])
    if ok is False:
        raise FrontEndError("reconstruct3Dlines failed", 4)
    line3d.get3Dlines()
    for save in (line3d.saveResultAsSTL, line3d.saveResultAsOBJ, line3d.save3DLinesAsTXT, line3d.save3DLinesAsBIN):
        # (the library's writers take max_image_width, which createOutputFilename reads from the object in the reference)
        if timed("save", save, s["output_folder"], s["max_img_width"]) is False:
            raise FrontEndError(f"{save.__name__} failed", 4)
    return line3d, times


def _read(reader, path, status=1):
    try:
        return reader(path)
    except ValueError as e:
        raise FrontEndError(str(e), status) from None


def _start(program, argv):
    a = parse_args(program, argv)
    if not a["use_cuda"]:
        print(f"{PREFIX}-g 0 is ignored: this library has no CPU path, everything runs on the GPU")
    return a


def run_vsfm(argv, **pieces):
    """main_vsfm.cpp; `pieces`: line3d_factory, read_image, undistort of run_views"""
    a = _start("vsfm", argv)
    nvm, folder = a["nvm_file"], a["input_folder"]
    if not os.path.exists(nvm):
        raise FrontEndError(f"NVM file {nvm} does not exist!")
    full_path = len(folder) == 0                       # :110-116: the .nvm's entries, relative to the folder of the .nvm
    if full_path:
        folder = nvm[:nvm.rfind("/")] if "/" in nvm else ""
    s = _settings(a, a["output_folder"] or folder + "/Line3D++/")
    cams = _read(io.read_nvm, nvm)
    views = [(i, folder + "/" + (c["filename"] if full_path else c["filename"][c["filename"].rfind("/") + 1:]), c)
             for i, c in enumerate(cams) if c["worldpoints"]]                                         # :252-270
    return run_views("nvm", views, s, **pieces)


def run_colmap(argv, **pieces):
    """main_colmap.cpp"""
    a = _start("colmap", argv)
    folder = a["input_folder"]
    sfm = a["sfm_folder"] or folder
    if not os.path.exists(sfm):
        raise FrontEndError(f'colmap result folder "{sfm}" does not exist!')
    s = _settings(a, a["output_folder"] or sfm + "/Line3D++/")
    # COLMAP's binary model (its default output) is read where there is no cameras.txt and all three .bin files exist
    binary = not os.path.exists(sfm + "/cameras.txt") and all(
        os.path.exists(sfm + "/" + n) for n in ("cameras.bin", "images.bin", "points3D.bin"))
    if not binary and not all(os.path.exists(sfm + "/" + n) for n in ("cameras.txt", "images.txt", "points3D.txt")):
        raise FrontEndError(f'at least one of the colmap result files does not exist in sfm folder: "{sfm}"', 2)
    try:
        images = io.read_colmap(sfm)
    except ValueError as e:                                                                           # :221-226
        if not str(e).endswith("unknown!"):                    # a binary file that is truncated or over-long
            raise FrontEndError(str(e), 2) from None
        raise FrontEndError(f"{e}\nplease specify its parameters in l3d_io.hip (kColmapModels) in order to proceed...", 3) from None
    # :353-410: every image of a known camera is read, and undistorted if its camera has distortion; only one with
    # worldpoints is added
    return run_views("colmap", [(im["id"], folder + "/" + im["name"], im) for im in images], s, **pieces)


def run_bundler(argv, **pieces):
    """main_bundler.cpp"""
    a = _start("bundler", argv)
    folder, ext = a["image_folder"], a["image_extension"]
    if ext and not ext.startswith("."):
        ext = "." + ext
    bundle = a["bundle_file"] or folder + "/../bundle.rd.out"
    s = _settings(a, a["output_folder"] or folder + "/Line3D++/")
    if not os.path.exists(bundle):
        raise FrontEndError(f"bundle file '{bundle}' does not exist!")
    cams = _read(io.read_bundler, bundle)
    listed = {}
    if a["img_list"]:                                  # :255-276: first token per line, line index = camera id
        try:
            with open(a["img_list"]) as f:
                lines = f.read().split("\n")
        except OSError:
            lines = []                                 # a list that cannot be opened is an empty list there
        for k, line in enumerate(lines[:-1] if lines and lines[-1] == "" else lines):
            tok = line.split()
            if tok:
                listed[k] = tok[0]
    views = []
    for i, c in enumerate(cams):                       # :282-335
        path = None
        if i in listed:
            path = folder + "/" + listed[i]
        else:
            for e in ([ext] if ext else BUNDLER_EXTENSIONS):
                if os.path.exists(f"{folder}/{i:08d}{e}"):
                    path = f"{folder}/{i:08d}{e}"
                    break
        if path is not None and c["worldpoints"]:
            views.append((i, path, c))
    return run_views("bundler", views, s, **pieces)


def run_pix4d(argv, **pieces):
    """main_pix4d.cpp"""
    a = _start("pix4d", argv)
    folder = a["input_folder"]
    s = _settings(a, a["output_folder"] or folder + "/Line3D++/")
    file1, file2 = io.pix4d_files(a["params_folder"], a["project_prefix"])
    if not os.path.exists(file1) or not os.path.exists(file2):                                        # :171-175
        raise FrontEndError(f"pix4d file '{file1}' or '\n{file2}' does not exist!")
    try:
        cams = io.read_pix4d(a["params_folder"], a["project_prefix"])
    except (ValueError, RuntimeError) as e:            # RuntimeError: the library's, e.g. no usable device for the triangulation
        raise FrontEndError(str(e)) from None
    return run_views("pix4d", [(c["id"], folder + "/" + c["name"], c) for c in cams], s, **pieces)     # :378-419


def run_openmvg(argv, **pieces):
    """main_openmvg.cpp"""
    a = _start("openmvg", argv)
    folder, json_file = a["input_folder"], a["sfm_json_file"]
    s = _settings(a, a["output_folder"] or folder + "/Line3D++/")
    if not os.path.exists(json_file):                                                                 # :119-125
        raise FrontEndError(f"OpenMVG json file {json_file} does not exist!")
    views = _read(lambda path: io.read_openmvg(path, folder), json_file)
    return run_views("openmvg", [(v["id"], v["path"], v) for v in views], s, **pieces)                # :369-410


def run_mavmap(argv, **pieces):
    """main_mavmap.cpp"""
    a = _start("mavmap", argv)
    folder, ext = a["input_folder"], a["image_extension"]
    if not ext.startswith("."):                        # :125-126: the empty extension gets its dot as well, so the probe
        ext = "." + ext                                # of :263-274 is never reached
    s = _settings(a, a["output_folder"] or folder + "/Line3D++/")
    if np.float32(s["sigma_p"]) < io.L3D_EPS and np.float32(s["const_reg_depth"]) < io.L3D_EPS:       # :130-135
        print("sigma_p cannot be negative (i.e. in world coordiantes) when no valid regularization depth (--const_reg_depth) is given!")
        print("reverting to: sigma_p = 2.5px")
        s["sigma_p"] = 2.5
    if not os.path.exists(a["mavmap_output"]):                                                        # :137-143
        raise FrontEndError(f"mavmap file '{a['mavmap_output']}' does not exist!")
    cams = _read(lambda path: io.read_mavmap(path, s["neighbors"]), a["mavmap_output"])
    views = []
    for c in cams:                                     # :256-327: a camera without an image file keeps its position
        path = folder + "/" + a["image_prefix"] + c["name"] + ext
        if os.path.exists(path):
            views.append((c["id"], path, dict(c, median_depth=s["const_reg_depth"])))
    return run_views("mavmap", views, s, neighbors_by_worldpoints=False, **pieces)


PROGRAMS = {"vsfm": run_vsfm, "colmap": run_colmap, "bundler": run_bundler, "pix4d": run_pix4d, "openmvg": run_openmvg,
            "mavmap": run_mavmap}


def main(argv=None, **pieces):
    """the program: -> exit status"""
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in PROGRAMS:
        print("usage: python -m line3dpp_amd.front_end {" + "|".join(PROGRAMS) + "} <flags>\n\n"
              + "\n\n".join(usage(p) for p in PROGRAMS), file=sys.stderr)
        return 1
    try:
        _, times = PROGRAMS[argv[0]](argv[1:], **pieces)
    except FrontEndError as e:
        print(e, file=sys.stderr)
        if isinstance(e, UsageError):
            print("\n" + usage(argv[0]), file=sys.stderr)
        return e.status
    print(f"{PREFIX}seconds per stage: " + ", ".join(f"{k} {times[k]:.3f}" for k in STAGES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
