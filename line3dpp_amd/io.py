"""Reader/formatter of the reference's TXT result format (Line3D::save3DLinesAsTXT, line3D.cc:2631-2688):
one text line per 3D line --  n_segments (P1.x P1.y P1.z P2.x P2.y P2.z)*  n_residuals (camID segID x1 y1 x2 y2)*
with the C++ stream defaults (6 significant digits).  The library writes the format itself
(l3d_save_3d_lines_txt); this module parses it (e.g. testdata/Line3D++_ref/*.txt of the reference) and
re-creates the text for diffing."""
import ctypes as C
import os

import numpy as np

from . import _lib


def read_3d_lines_txt(path):
    """-> list of dicts: segments [n,6] float64 (P1, P2), residuals [m,2] uint32 (camID, segID), coords2D [m,4] float32"""
    out = []
    with open(path) as f:
        for raw in f:
            tok = raw.split()
            if not tok:
                continue
            n = int(tok[0]); p = 1
            segs = np.array(tok[p:p + 6 * n], np.float64).reshape(n, 6); p += 6 * n
            m = int(tok[p]); p += 1
            rec = np.array(tok[p:p + 6 * m], np.float64).reshape(m, 6); p += 6 * m
            if p != len(tok):
                raise ValueError(f"{path}: trailing tokens in a 3D-line record")
            out.append(dict(segments=segs, residuals=rec[:, :2].astype(np.uint32), coords2D=rec[:, 2:].astype(np.float32)))
    return out


def _g(x):
    return "%g" % x          # == operator<<(std::ostream&, double/float) with the default precision of 6


def format_3d_lines_txt(lines):
    """inverse of read_3d_lines_txt: the exact text Line3D::save3DLinesAsTXT writes for these lines"""
    rows = []
    for L in lines:
        if len(L["segments"]) == 0:
            continue
        t = [str(len(L["segments"]))]
        for s in L["segments"]:
            t += [_g(v) for v in s]
        t.append(str(len(L["residuals"])))
        for (cam, seg), co in zip(L["residuals"], L["coords2D"]):
            t += [str(int(cam)), str(int(seg))] + [_g(np.float32(v)) for v in co]
        rows.append(" ".join(t) + " \n")
    return "".join(rows)


def format_obj(lines):
    """the text Line3D::saveResultAsOBJ (line3D.cc:2579-2628) writes: two `v` records per 3D segment, then one `l`
    record per segment"""
    v, n = [], 0
    for L in lines:
        for s in L["segments"]:
            v.append("v " + " ".join(_g(x) for x in s[:3]) + "\n")
            v.append("v " + " ".join(_g(x) for x in s[3:]) + "\n")
            n += 1
    return "".join(v) + "".join(f"l {2 * k + 1} {2 * k + 2}\n" for k in range(n))


def format_stl(lines):
    """the text Line3D::saveResultAsSTL (line3D.cc:2465-2531) writes (degenerate triangles P1-P2-P1, printf %e)"""
    t = ["solid lineModel\n"]
    for L in lines:
        for s in L["segments"]:
            a = ["%e" % x for x in s]
            t += [" facet normal 1.0e+000 0.0e+000 0.0e+000\n", "  outer loop\n",
                  "   vertex %s %s %s\n" % tuple(a[:3]), "   vertex %s %s %s\n" % tuple(a[3:]),
                  "   vertex %s %s %s\n" % tuple(a[:3]), "  endloop\n", " endfacet\n"]
    t.append("endsolid lineModel\n")
    return "".join(t)


# ---- BIN result format (Line3D::save3DLinesAsBIN, line3D.cc:2690-2711) ------------------------------------------
# boost::archive::binary_oarchive of std::vector<FinalLine3D> (serialization.h:38-45), little endian, as written by
# the Boost version behind the reference's fixtures (archive library version 10).  Layout, verified byte for byte
# against testdata/Line3D++_ref/*vis_3.bin (tests/test_bin_format.py):
#   u64 22, "serialization::archive", u16 library version, sizeof(int, long, float, double) as 4 bytes, u32 1 (endian)
#   every class writes a 5-byte header (u8 tracking = 0, u32 version = 0) at its FIRST occurrence in the archive only
#   collections: u64 count, u32 item_version
#   vector<FinalLine3D>   = [hdr] count item_version FinalLine3D*
#   FinalLine3D           = [hdr] list<Segment3D> LineCluster3D                       (segment3D.h:165-178)
#   list<Segment3D>       = [hdr] count item_version Segment3D*
#   Segment3D             = [hdr] f32 length_, u8 valid_, 9 x f64 (P1, P2, dir)       (segment3D.h:99-115)
#   LineCluster3D         = [hdr] Segment3D list<Segment2D> u32 reference_view_        (segment3D.h:152-160)
#   list<Segment2D>       = [hdr] count item_version Segment2D*
#   Segment2D             = [hdr] u32 camID_, u32 segID_                               (commons.h:123-130)
_BIN_SIG = b"serialization::archive"
_CLASS_HDR = b"\x00" * 5


class _Reader:
    def __init__(self, buf):
        self.b, self.p, self.seen = buf, 0, set()

    def take(self, fmt):
        import struct
        try:
            v = struct.unpack_from("<" + fmt, self.b, self.p)
        except struct.error as e:
            raise ValueError(f"truncated archive at byte {self.p}: {e}") from None
        self.p += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def hdr(self, cls):
        if cls not in self.seen:
            self.seen.add(cls)
            if self.b[self.p:self.p + 5] != _CLASS_HDR:
                raise ValueError(f"unexpected class header for {cls} at byte {self.p}")
            self.p += 5

    def seg3d(self):
        self.hdr("Segment3D")
        length, valid = self.take("fB")
        geo = np.array(self.take("9d"))
        return length, valid, geo


def read_3d_lines_bin(path):
    """-> (lines, library_version); lines = list of dicts: segments [n,9] float64 (P1, P2, dir), seg_length [n] float32,
    seg_valid [n] uint8, cluster_line [9] float64, cluster_length, cluster_valid, residuals [m,2] uint32 (camID, segID),
    reference_view"""
    r = _Reader(open(path, "rb").read())
    if r.take("Q") != len(_BIN_SIG) or r.b[r.p:r.p + len(_BIN_SIG)] != _BIN_SIG:
        raise ValueError(f"{path}: not a boost binary archive")
    r.p += len(_BIN_SIG)
    lib_version = r.take("H")
    if bytes(r.b[r.p:r.p + 8]) != bytes([4, 8, 4, 8, 1, 0, 0, 0]):
        raise ValueError(f"{path}: written on a platform with other type sizes / endianness")
    r.p += 8
    r.hdr("vector<FinalLine3D>")
    n, _ = r.take("QI")
    lines = []
    for _ in range(n):
        r.hdr("FinalLine3D")
        r.hdr("list<Segment3D>")
        ns, _ = r.take("QI")
        segs = [r.seg3d() for _ in range(ns)]
        r.hdr("LineCluster3D")
        cl_len, cl_valid, cl_geo = r.seg3d()
        r.hdr("list<Segment2D>")
        nr, _ = r.take("QI")
        res = np.zeros((nr, 2), np.uint32)
        for k in range(nr):
            r.hdr("Segment2D")
            res[k] = r.take("II")
        ref_view = r.take("I")
        lines.append(dict(segments=np.array([s[2] for s in segs]).reshape(-1, 9),
                          seg_length=np.array([s[0] for s in segs], np.float32),
                          seg_valid=np.array([s[1] for s in segs], np.uint8),
                          cluster_line=cl_geo, cluster_length=np.float32(cl_len), cluster_valid=int(cl_valid),
                          residuals=res, reference_view=int(ref_view)))
    if r.p != len(r.b):
        raise ValueError(f"{path}: {len(r.b) - r.p} trailing bytes")
    return lines, lib_version


def format_3d_lines_bin(lines, lib_version=10):
    """inverse of read_3d_lines_bin: the exact bytes Line3D::save3DLinesAsBIN writes for these lines"""
    import struct
    out = [struct.pack("<Q", len(_BIN_SIG)), _BIN_SIG, struct.pack("<H", lib_version), bytes([4, 8, 4, 8, 1, 0, 0, 0])]
    seen = set()

    def hdr(cls):
        if cls not in seen:
            seen.add(cls)
            out.append(_CLASS_HDR)

    def seg3d(length, valid, geo):
        hdr("Segment3D")
        out.append(struct.pack("<fB9d", float(length), int(valid), *[float(x) for x in geo]))
    hdr("vector<FinalLine3D>")
    out.append(struct.pack("<QI", len(lines), 0))
    for L in lines:
        hdr("FinalLine3D")
        hdr("list<Segment3D>")
        out.append(struct.pack("<QI", len(L["segments"]), 0))
        for g, ln, va in zip(L["segments"], L["seg_length"], L["seg_valid"]):
            seg3d(ln, va, g)
        hdr("LineCluster3D")
        seg3d(L["cluster_length"], L["cluster_valid"], L["cluster_line"])
        hdr("list<Segment2D>")
        out.append(struct.pack("<QI", len(L["residuals"]), 0))
        for cam, seg in L["residuals"]:
            hdr("Segment2D")
            out.append(struct.pack("<II", int(cam), int(seg)))
        out.append(struct.pack("<I", int(L["reference_view"])))
    return b"".join(out)


# ---- input side: the segment cache, VisualSfM .nvm files, COLMAP results and bundler files ---------
# One reader per format: the library's (line3dpp_amd/csrc/l3d_io.hip, declared in include/l3dpp_hip.h), which follows
# main_vsfm.cpp, main_colmap.cpp and main_bundler.cpp line by line.  What is here hands its records over as dicts; an
# error of the library is a ValueError with its message.  tests/sfm_readers_model.py restates the formats in Python as
# the model the library is checked against.
def _check(rc):
    if rc != 0:
        raise ValueError(_lib.last_error())


def _text(raw):
    return raw.decode("utf-8", "surrogateescape")


def _pose(rec):
    """R, t, C of an l3d_nvm_camera or l3d_sfm_image"""
    return dict(R=np.array(rec.R).reshape(3, 3), t=np.array(rec.t), C=np.array(rec.C))


def _points(get, handle, index, rec):
    """the worldpoint list of record `index` through l3d_nvm_get_worldpoints / l3d_sfm_get_worldpoints, and its median
    depth (None where it sees no point)"""
    ids = np.zeros(rec.n_worldpoints, np.uint32)
    _check(get(handle, index, _lib.ptr(ids), len(ids)))
    return dict(worldpoints=ids.tolist(), median_depth=np.float32(rec.median_depth) if len(ids) else None)


def segment_cache_name(camID, width, height, max_segments=3000):
    """the file name of the cache Line3D::detectLineSegments keeps per image (line3D.cc:295-309)"""
    name = C.create_string_buffer(80)
    _check(_lib.load().l3d_segment_cache_name(int(camID), int(width), int(height), int(max_segments), name, len(name)))
    return _text(name.value)


def read_segment_cache(path):
    """-> [n,4] float32 segments of a cache file written by the reference or by l3d_write_segment_cache"""
    L, path, n = _lib.load(), os.fsencode(path), C.c_uint32(0)
    _check(L.l3d_read_segment_cache(path, None, 0, C.byref(n)))
    segs = np.zeros((n.value, 4), np.float32)
    _check(L.l3d_read_segment_cache(path, _lib.ptr(segs), len(segs), C.byref(n)))
    return segs


def format_segment_cache(segs):
    """the bytes of the cache file l3d_write_segment_cache writes for [n,4] segments"""
    import tempfile
    segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 4)
    with tempfile.TemporaryDirectory() as folder:
        path = os.path.join(folder, "segments.bin")
        _check(_lib.load().l3d_write_segment_cache(os.fsencode(path), _lib.ptr(segs), len(segs)))
        with open(path, "rb") as f:
            return f.read()


def rotation_from_q(qw, qx, qy, qz):
    """Line3D::rotationFromQ (l3d_rotation_from_q), which the COLMAP reader applies to a pose's quaternion"""
    R = np.zeros(9)
    _check(_lib.load().l3d_rotation_from_q(float(qw), float(qx), float(qy), float(qz), _lib.ptr(R)))
    return R.reshape(3, 3)


def _mv3(M, v):
    """M v for a 3x3 M in the evaluation order of the reference's fixed-size Eigen product (and of the C-ABI readers):
    (M[i,0] v[0] + M[i,1] v[1]) + M[i,2] v[2] -- numpy's matmul may sum in another order or fuse the multiplies"""
    M = np.asarray(M, np.float64); v = np.asarray(v, np.float64)
    return (M[:, 0] * v[0] + M[:, 1] * v[1]) + M[:, 2] * v[2]


def read_nvm(path):
    """VisualSfM .nvm as main_vsfm.cpp:144-250 reads it (l3d_nvm_open) -> list of cameras in file order (the reference
    uses the index as camID): dict(filename, focal, R, t, C, distortion, worldpoints = ids of the 3D points it sees,
    median_depth = sorted distances to them [n/2] as float32, main_vsfm.cpp:300-303; None for a camera without points,
    which the reference skips)"""
    L, h = _lib.load(), C.c_void_p()
    _check(L.l3d_nvm_open(os.fsencode(path), C.byref(h)))
    try:
        cams = []
        for i in range(L.l3d_nvm_num_cameras(h)):
            c = _lib.NvmCamera()
            _check(L.l3d_nvm_get_camera(h, i, C.byref(c)))
            cams.append(dict(filename=_text(c.filename), focal=np.float32(c.focal), **_pose(c),
                             distortion=np.float32(c.distortion), **_points(L.l3d_nvm_get_worldpoints, h, i, c)))
        return cams
    finally:
        L.l3d_nvm_close(h)


def nvm_intrinsics(focal, width, height):
    """K as main_vsfm.cpp:272-282 builds it: principal point at the image centre (float arithmetic there)"""
    K = np.zeros(9)
    _lib.load().l3d_nvm_intrinsics(float(focal), int(width), int(height), _lib.ptr(K))
    return K.reshape(3, 3)


def _read_sfm(open_, path, entry):
    """[entry(handle, index, l3d_sfm_image) of every image of the l3d_sfm handle that `open_` gives for `path`]"""
    L, h = _lib.load(), C.c_void_p()
    _check(open_(os.fsencode(path), C.byref(h)))
    try:
        out = []
        for i in range(L.l3d_sfm_num_images(h)):
            im = _lib.SfmImage()
            _check(L.l3d_sfm_get_image(h, i, C.byref(im)))
            out.append(entry(h, i, im))
        return out
    finally:
        L.l3d_sfm_close(h)


# COLMAP's binary model ids, in order, with the length of each model's parameter list (what `model` and `params` of
# read_colmap can be; the library's own table is kColmapModels in l3d_io.hip)
COLMAP_MODEL_IDS = (("SIMPLE_PINHOLE", 3), ("PINHOLE", 4), ("SIMPLE_RADIAL", 4), ("RADIAL", 5), ("OPENCV", 8),
                    ("OPENCV_FISHEYE", 8), ("FULL_OPENCV", 12), ("FOV", 5), ("SIMPLE_RADIAL_FISHEYE", 4),
                    ("RADIAL_FISHEYE", 5), ("THIN_PRISM_FISHEYE", 12))
# (index of the first distortion parameter in the list, their number) of the models l3d_undistort_images_model takes
_COLMAP_DISTORTION = {"FULL_OPENCV": (4, 8), "OPENCV_FISHEYE": (4, 4), "SIMPLE_RADIAL_FISHEYE": (3, 1),
                      "RADIAL_FISHEYE": (3, 2), "FOV": (4, 1)}


def read_colmap(folder):
    """cameras.txt / images.txt / points3D.txt as main_colmap.cpp:136-348 reads them or, where there is no cameras.txt and
    cameras.bin, images.bin and points3D.bin all exist, COLMAP's binary form of the same (l3d_sfm_open_colmap)
    -> list of images in file order: dict(id, camera, name, width, height, K, R, t, C, radial (k1, k2, k3), tangential
    (p1, p2), model (COLMAP's name), params (the model's parameter list), worldpoints, median_depth or None).  An image
    whose camera is unknown is dropped; points3D.txt lines that do not parse as "id X Y Z" are ignored; a worldpoint
    without an entry there sits at the origin (the reference's map default).  A binary file that is truncated, over-long
    or states a count that cannot fit: ValueError with its name."""
    L = _lib.load()

    def entry(h, i, im):
        params, n = (C.c_double * max(k for _, k in COLMAP_MODEL_IDS))(), C.c_uint32(0)
        model = L.l3d_sfm_get_camera_params(h, i, params, len(params), C.byref(n))
        if model is None:
            raise ValueError(_lib.last_error())
        return dict(id=im.id, camera=im.camera, name=_text(im.name), width=im.width, height=im.height,
                    K=np.array(im.K).reshape(3, 3), **_pose(im), radial=np.array(im.radial), tangential=np.array(im.tangential),
                    model=_text(model), params=list(params[:n.value]), **_points(L.l3d_sfm_get_worldpoints, h, i, im))
    return _read_sfm(L.l3d_sfm_open_colmap, folder, entry)


def read_bundler(path):
    """bundle.rd.out as main_bundler.cpp:147-252 reads it (l3d_sfm_open_bundler) -> list of cameras (index = camID):
    dict(id, focal, radial (d1, d2, 0), R, t (second and third row / entry negated), C, worldpoints, median_depth or
    None)"""
    L = _lib.load()
    return _read_sfm(L.l3d_sfm_open_bundler, path, lambda h, i, im: dict(
        id=im.id, focal=np.float32(im.focal), radial=np.array(im.radial), **_pose(im),
        **_points(L.l3d_sfm_get_worldpoints, h, i, im)))


L3D_EPS = 1e-12     # commons.h:95


# ---- mavmap logs, OpenMVG sfm_data.json and Pix4D projects (main_mavmap.cpp, main_openmvg.cpp, main_pix4d.cpp) -----------
def _getlines(path):
    """std::getline's view of a file: no extra empty line behind a final newline"""
    with open(path) as f:
        lines = f.read().split("\n")
    return lines[:-1] if lines and lines[-1] == "" else lines


_NUMBER = None


def _stream_double(text):
    """what `stream >> double` leaves for a token: its longest numeric prefix, 0 when there is none"""
    global _NUMBER
    if _NUMBER is None:
        import re
        _NUMBER = re.compile(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?")
    m = _NUMBER.match(text)
    return float(m.group(0)) if m else 0.0


def _row(line, n):
    tok = line.split()
    return [_stream_double(tok[k]) if k < len(tok) else 0.0 for k in range(n)]


def _mm3(A, B):
    """A B for a 3x3 A in the evaluation order of _mv3, column by column of B"""
    B = np.asarray(B, np.float64)
    return np.stack([_mv3(A, B[:, j]) for j in range(B.shape[1])], axis=1)


def rotation_from_rpy(roll, pitch, yaw):
    """Line3D::rotationFromRPY, line3D.cc:2714-2727: Rz(yaw) Ry(pitch) Rx(roll), each factor as
    Eigen::AngleAxisd(angle, unit axis).toRotationMatrix() fills it (the axis' own diagonal entry is (1 - c) + c)"""
    def axis(k, angle):
        s, c = np.sin(angle), np.cos(angle)
        i, j = (k + 1) % 3, (k + 2) % 3
        R = np.zeros((3, 3))
        R[k, k] = (1.0 - c) + c
        R[i, i] = R[j, j] = c
        R[i, j], R[j, i] = -s, s
        return R
    return _mm3(_mm3(axis(2, float(yaw)), axis(1, float(pitch))), axis(0, float(roll)))


def mavmap_neighbors(i, n_cams, neighbors):
    """main_mavmap.cpp:311-321: up to neighbors / 2 previous positions, nearest first, then following ones until the list
    holds `neighbors`"""
    out = []
    k = i - 1
    while k >= 0 and len(out) < neighbors // 2:
        out.append(k); k -= 1
    k = i + 1
    while k < n_cams and len(out) < neighbors:
        out.append(k); k += 1
    return out


def read_mavmap(path, neighbors=10):
    """image-data-*.txt as main_mavmap.cpp:153-250 reads it -> list of cameras in file order (position = camera id, also
    of a camera whose image the program does not find): dict(id, name, K, R, t, C, radial, tangential, worldpoints = the
    NEIGHBOUR list of :311-321 for `neighbors`, median_depth None: the program hands over const_reg_depth).
    Leading lines that start with '#' are skipped (:159-163); the list ends at the first line shorter than 28 characters
    (:173).  17 whitespace-separated tokens per line, and every token that is used loses its last character, the comma
    -- the last token, cy, as well (:188-245).  A camera model other than PINHOLE: ValueError (:188-192).  The pose is
    the inverse of [R t; 0 1] with R = rotationFromRPY(roll, pitch, yaw) (:206-226), here R^T and -R^T t."""
    lines = _getlines(path)
    pos, line = 0, ""
    while pos < len(lines):
        line = lines[pos]; pos += 1
        if line[:1] != "#":
            break
    cams = []
    while len(line) >= 28:
        tok = line.split()
        tok = [tok[k][:-1] if k < len(tok) else "" for k in range(17)]
        if tok[12] != "PINHOLE":
            raise ValueError("only PINHOLE camera model supported...")
        roll, pitch, yaw = (_stream_double(tok[k]) for k in (1, 2, 3))
        t = np.array([_stream_double(tok[k]) for k in (8, 9, 10)])
        fx, fy, cx, cy = (_stream_double(tok[k]) for k in (13, 14, 15, 16))
        R = rotation_from_rpy(roll, pitch, yaw).T.copy()
        cams.append(dict(id=len(cams), name=tok[0], K=np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]), R=R,
                         t=_mv3(R, -1.0 * t), C=t, radial=np.zeros(3), tangential=np.zeros(2), median_depth=None))
        if pos >= len(lines):
            break
        line = lines[pos]; pos += 1
    for c in cams:
        c["worldpoints"] = mavmap_neighbors(c["id"], len(cams), neighbors)
    return cams


def read_openmvg(json_file, input_folder):
    """sfm_data.json as main_openmvg.cpp:135-410 reads it -> list of the views its image loop adds, in the order of
    `views`: dict(id = id_view, name, path = input_folder/name, K, R, t, C, radial, tangential, worldpoints = the keys of
    the structure points that observe the view, in file order, median_depth = sorted float32 distances [n // 2]).
    A view whose file does not exist is warned about and not visited, and its pose maps to no view (:169-187).  The camera
    model of an intrinsic is its polymorphic_name when it has one, otherwise that of the element before it (:205-211);
    an unknown model is warned about and has no distortion (:247-250).  t = -R C (:310).  A view is added when it has
    worldpoints, its file exists and its intrinsic id is known (:374-375).  Empty views, intrinsics, extrinsics or
    structure: ValueError with the reference's message (:145-149, :199-203, :282-286, :330-334)."""
    import json
    import os
    import sys
    with open(json_file) as f:
        d = json.load(f)
    views = d.get("views") or []
    if not views:
        raise ValueError("No aligned cameras in json file!")
    found, pose2view = [], {}
    for v in views:
        data = v["value"]["ptr_wrapper"]["data"]
        name, view_id = data["filename"], int(data["id_view"])
        path = input_folder + "/" + name
        if os.path.exists(path):
            found.append(dict(id=view_id, name=name, path=path, intrinsic=int(data["id_intrinsic"])))
            pose2view[int(data["id_pose"])] = view_id
        else:
            found.append(None)
            print(f"WARNING: image '{name}' not found (ID={view_id})", file=sys.stderr)
    intrinsics = d.get("intrinsics") or []
    if not intrinsics:
        raise ValueError("No intrinsics in json file!")
    cams, model = {}, ""
    for e in intrinsics:
        data = e["value"]["ptr_wrapper"]["data"]
        model = e["value"].get("polymorphic_name", model)
        group = int(e["key"])
        radial, tangential = np.zeros(3), np.zeros(2)
        if model == "pinhole_radial_k3":
            radial[:] = [float(x) for x in data["disto_k3"][:3]]
        elif model == "pinhole_radial_k1":
            radial[0] = float(data["disto_k1"][0])
        elif model == "pinhole_brown_t2":
            radial[:] = [float(x) for x in data["disto_t2"][:3]]
            tangential[:] = [float(x) for x in data["disto_t2"][3:5]]
        elif model != "pinhole":
            print(f"WARNING: camera model '{model}' for group {group} unknown! No distortion assumed...", file=sys.stderr)
        f_, pp = float(data["focal_length"]), data["principal_point"]
        cams[group] = dict(K=np.array([[f_, 0.0, float(pp[0])], [0.0, f_, float(pp[1])], [0.0, 0.0, 1.0]]), radial=radial,
                           tangential=tangential)
    extrinsics = d.get("extrinsics") or []
    if not extrinsics:
        raise ValueError("No extrinsics in json file!")
    poses = {}
    for e in extrinsics:
        pose = int(e["key"])
        if pose in pose2view:
            R = np.array(e["value"]["rotation"], np.float64).reshape(3, 3)
            Cc = np.array(e["value"]["center"], np.float64).reshape(3)
            poses[pose2view[pose]] = dict(R=R, t=_mv3(-R, Cc), C=Cc)
        else:
            print(f"WARNING: pose with ID {pose} does not map to an image!", file=sys.stderr)
    structure = d.get("structure") or []
    if not structure:
        raise ValueError("No worldpoints in json file!")
    wps, depths = {}, {}
    for e in structure:
        X = np.array(e["value"]["X"], np.float64).reshape(3)
        for o in e["value"]["observations"]:
            view = int(o["key"])
            if view in poses:
                wps.setdefault(view, []).append(int(e["key"]))
                depths.setdefault(view, []).append(np.float32(np.linalg.norm(poses[view]["C"] - X)))
    out = []
    for v in found:
        if v is not None and v["id"] in wps and v["intrinsic"] in cams:
            dd = sorted(depths[v["id"]])
            out.append(dict(id=v["id"], name=v["name"], path=v["path"], **cams[v["intrinsic"]], **poses[v["id"]],
                            worldpoints=list(wps[v["id"]]), median_depth=dd[len(dd) // 2]))
    return out


def pix4d_files(params_folder, project_prefix):
    """main_pix4d.cpp:163-168: the camera file and the tie-point file of a project"""
    prefix = params_folder + "/" + project_prefix
    if prefix[-1:] != "_":
        prefix += "_"
    return prefix + "calibrated_camera_parameters.txt", prefix + "tp_pix4d.txt"


def read_pix4d(params_folder, project_prefix, device=0, triangulate=None):
    """<prefix>_calibrated_camera_parameters.txt and <prefix>_tp_pix4d.txt as main_pix4d.cpp:162-420 reads them -> list of
    the cameras its image loop adds, in file order: dict(id = position in the camera file, name, K, R, t, C, radial,
    tangential, worldpoints = the feature ids of the camera's key, one per tie-point line, invalid ones included,
    median_depth).
    Camera file (:186-279): header lines up to the first line shorter than 2 characters; then blocks of `name width
    height`, 3 rows of K, radial (3), tangential (2), the camera centre, 3 rows of R, until a line shorter than 5
    characters; t = -R C, P = K [R | t]; the key of a camera is its name up to the last dot.
    Tie-point file (:282-349): `id rest...` per line; an id shorter than 2 characters ends the file, one that starts with
    '-' is skipped; a line of one token names the key image of the lines that follow (an unknown key maps to position 0,
    as std::map::operator[] gives it, and counts as a camera in the printed total); any other line is `id px py scale`.
    Every feature is triangulated from its observations (:354-372; `triangulate`, by default api.triangulate_points on
    `device`): valid with more than two observations and norm(X) > L3D_EPS.  A camera is added when its key has features
    and more than two of them are valid (:386-405); median_depth = sorted float32 distances to the valid ones [n // 2]."""
    file1, file2 = pix4d_files(params_folder, project_prefix)
    lines = _getlines(file1)
    pos = 0
    while pos < len(lines):
        pos += 1
        if len(lines[pos - 1]) < 2:
            break
    take = lambda: lines[pos] if pos < len(lines) else ""
    cams, img2pos, pos2img = [], {}, {}
    while pos < len(lines):
        line = lines[pos]; pos += 1
        if len(line) < 5:
            break
        name = (line.split() + [""])[0]
        raw = name[:name.rfind(".")] if "." in name else name
        img2pos[raw] = len(cams); pos2img[len(cams)] = raw
        rows = []
        for n in (3, 3, 3, 3, 2, 3, 3, 3, 3):                     # K, radial, tangential, centre, R
            rows.append(_row(take(), n)); pos += 1
        K, R = np.array(rows[0:3]), np.array(rows[6:9])
        t = _mv3(-R, np.array(rows[5]))
        cams.append(dict(id=len(cams), name=name, K=K, R=R, t=t, C=_mv3(R.T, -1.0 * t), radial=np.array(rows[3]),
                         tangential=np.array(rows[4]), P=_mm3(K, np.column_stack([R, t]))))
    per_cam, feat_id, obs = {}, {}, []
    key, key_pos = "", 0
    for line in _getlines(file2):
        tok = line.split()
        fid, rest = (tok + ["", ""])[:2]
        if len(fid) < 2:
            break
        if fid[0] == "-":
            continue
        if rest == "":
            key = fid
            key_pos = img2pos.setdefault(key, 0)
            continue
        if fid not in feat_id:
            feat_id[fid] = len(obs)
            obs.append([])
        per_cam.setdefault(key, []).append(feat_id[fid])
        obs[feat_id[fid]].append((key_pos, _stream_double(tok[1]), _stream_double(tok[2]) if len(tok) > 2 else 0.0))
    print(f"Pix4D: #cameras = {len(img2pos)}")
    print(f"Pix4D: #points  = {len(obs)}")
    print("triangulating...")
    X, valid = np.zeros((len(obs), 3)), np.zeros(len(obs), bool)
    if obs and cams:
        if triangulate is None:
            from .api import triangulate_points
            triangulate = lambda *a: triangulate_points(*a, device=device)
        off = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.uint64)
        flat = [o for f in obs for o in f]
        X, valid = triangulate(np.array([c["P"] for c in cams]), off, np.array([o[0] for o in flat], np.uint32),
                               np.array([o[1:] for o in flat], np.float64).reshape(-1, 2))
    out = []
    for c in cams:
        feats = per_cam.get(pos2img[c["id"]])
        if feats is None:
            continue
        depths = sorted(np.float32(np.linalg.norm(X[f] - c["C"])) for f in feats if valid[f])
        if len(depths) > 2:
            out.append(dict(c, worldpoints=list(feats), median_depth=depths[len(depths) // 2]))
    return out


def front_end_undistortion(kind, entry, cols, rows):
    """(K, radial, tangential) as the reference's front end hands them to Line3D::undistortImage for the image of `entry`
    (cols x rows pixels), or None when it does not call it.  kind / entry: "nvm" and an element of read_nvm
    (main_vsfm.cpp:283-297: radial (-d, 0, 0), K from the image size), "bundler" and an element of read_bundler
    (main_bundler.cpp:352-368: radial (d1, d2, 0), K from the image size), "colmap" and an element of read_colmap
    (main_colmap.cpp:377-389: the camera's five coefficients and K).  Each calls it only when a coefficient exceeds
    L3D_EPS in magnitude; main_vsfm and main_bundler skip a camera without worldpoints before that, main_colmap does
    not.  "openmvg" and an element of read_openmvg: as colmap; "pix4d" and an element of read_pix4d: always (an entry of
    another reader: ValueError, as for an unknown kind); "mavmap": never."""
    zero2 = np.zeros(2)
    if kind == "nvm":
        d = np.float32(entry["distortion"])
        if not entry["worldpoints"] or not abs(float(d)) > L3D_EPS:
            return None
        return nvm_intrinsics(entry["focal"], cols, rows), np.array([float(-d), 0.0, 0.0]), zero2
    if kind == "bundler":
        d1, d2 = float(entry["radial"][0]), float(entry["radial"][1])
        if not entry["worldpoints"] or not (abs(d1) > L3D_EPS or abs(d2) > L3D_EPS):
            return None
        return nvm_intrinsics(entry["focal"], cols, rows), np.array([d1, d2, 0.0]), zero2
    if kind == "colmap":
        radial = np.array(entry["radial"], np.float64)
        tangential = np.array(entry["tangential"], np.float64)
        if not any(abs(float(v)) > L3D_EPS for v in (*radial, *tangential)):
            return None
        return np.array(entry["K"], np.float64), radial, tangential
    if kind == "openmvg":        # main_openmvg.cpp:253-257, :384-393: like colmap's, the intrinsic group's coefficients and K
        return front_end_undistortion("colmap", entry, cols, rows)
    if kind == "pix4d":          # main_pix4d.cpp:410-413: every added view, whatever its coefficients
        # This kind never answers None, so another reader's entry would be undistorted unasked: it is refused.  Only
        # read_pix4d's entries carry the projection matrix the triangulation used.
        if "P" not in entry:
            raise ValueError('front end "pix4d" takes an element of read_pix4d')
        return np.array(entry["K"], np.float64), np.array(entry["radial"], np.float64), np.array(entry["tangential"], np.float64)
    if kind == "mavmap":         # main_mavmap.cpp:293-326: never
        return None
    raise ValueError(f"unknown front end {kind!r}: nvm, bundler, colmap, openmvg, pix4d or mavmap")


def front_end_camera_model(kind, entry, cols, rows):
    """(model, K, params) for lsd.undistort_images_model when the image of `entry` has to be undistorted by its camera
    model, else None (front_end_undistortion then says what happens to it).  Only "colmap" has such
    cameras: the fisheye family always (with zero coefficients the image is still equidistant, not pinhole), FOV when
    |omega| exceeds L3D_EPS, FULL_OPENCV when k4, k5 or k6 exceeds L3D_EPS in magnitude (with zeros it is the reference's
    five coefficients).  params: the model's distortion parameters in COLMAP's order."""
    if kind != "colmap" or entry.get("model") not in _COLMAP_DISTORTION:
        return None
    model = entry["model"]
    first, n = _COLMAP_DISTORTION[model]
    params = [float(v) for v in entry["params"][first:first + n]]
    if model == "FOV" and not abs(params[0]) > L3D_EPS:
        return None
    if model == "FULL_OPENCV" and not any(abs(v) > L3D_EPS for v in params[5:8]):
        return None
    return model, np.array(entry["K"], np.float64), params
