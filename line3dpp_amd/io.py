"""Reader/formatter of the reference's TXT result format (Line3D::save3DLinesAsTXT, line3D.cc:2631-2688):
one text line per 3D line --  n_segments (P1.x P1.y P1.z P2.x P2.y P2.z)*  n_residuals (camID segID x1 y1 x2 y2)*
with the C++ stream defaults (6 significant digits).  The library writes the format itself
(l3d_save_3d_lines_txt); this module parses it (e.g. testdata/Line3D++_ref/*.txt of the reference) and
re-creates the text for diffing."""
import numpy as np


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


# ---- input side: the segment cache and VisualSfM .nvm files ---------------------------------------
# Segment cache = what Line3D::detectLineSegments stores / loads per image when `load_segments` is set
# (line3D.cc:295-309, 362-366): "<data folder>/segments_L3D++_<camID>_<width>x<height>_<max segments>.bin", a
# boost::archive::binary_oarchive of L3DPP::DataArray<float4> (dataArray.h:352-374): width_, height_, real_width_
# (u32), pitchCPU_, strideCPU_, pitchGPU_, strideGPU_ (u64), then real_width_ * height_ float4 elements, each through
# serialize(float4) (dataArray.h:62-69: the class header of float4 appears once, before the first element).
# width_ = number of segments, height_ = 1; the host row is padded to a multiple of 32 bytes (dataArray.h:111-122), so
# an odd number of segments carries one padding element.
def segment_cache_name(camID, width, height, max_segments=3000):
    return f"segments_L3D++_{camID}_{width}x{height}_{max_segments}.bin"


def _data_array_geometry(n):
    pitch = n * 16
    real = n + (0 if pitch % 32 == 0 else (32 - pitch % 32) // 16)
    return real, real * 16, real           # real_width_, pitchCPU_, strideCPU_


def format_segment_cache(segs, lib_version=10):
    """the bytes serializeToFile(name, DataArray<float4>(n, 1, false, segments)) writes for [n,4] float32 (x1,y1,x2,y2)"""
    import struct
    segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 4)
    n = len(segs)
    real, pitch, stride = _data_array_geometry(n)
    data = np.zeros((real, 4), np.float32)
    data[:n] = segs
    return b"".join([struct.pack("<Q", len(_BIN_SIG)), _BIN_SIG, struct.pack("<H", lib_version), bytes([4, 8, 4, 8, 1, 0, 0, 0]),
                     _CLASS_HDR, struct.pack("<IIIQQQQ", n, 1, real, pitch, stride, 0, 0),
                     _CLASS_HDR if real else b"", data.tobytes()])


def read_segment_cache(path):
    """-> [n,4] float32 segments of a cache file written by the reference (or by format_segment_cache)"""
    r = _Reader(open(path, "rb").read())
    if r.take("Q") != len(_BIN_SIG) or r.b[r.p:r.p + len(_BIN_SIG)] != _BIN_SIG:
        raise ValueError(f"{path}: not a boost binary archive")
    r.p += len(_BIN_SIG)
    r.take("H")
    if bytes(r.b[r.p:r.p + 8]) != bytes([4, 8, 4, 8, 1, 0, 0, 0]):
        raise ValueError(f"{path}: written on a platform with other type sizes / endianness")
    r.p += 8
    r.hdr("DataArray<float4>")
    width, height, real, pitch, stride, _, _ = r.take("IIIQQQQ")
    if height != 1 or real < width or pitch != real * 16 or stride != real:
        raise ValueError(f"{path}: not a one-row DataArray<float4> (width {width}, height {height}, real width {real})")
    if real:
        r.hdr("float4")
    if r.p + real * 16 > len(r.b):
        raise ValueError(f"{path}: truncated ({len(r.b) - r.p} of {real * 16} element bytes)")
    data = np.frombuffer(r.b, np.float32, real * 4, r.p).reshape(real, 4)
    r.p += real * 16
    if r.p != len(r.b):
        raise ValueError(f"{path}: {len(r.b) - r.p} trailing bytes")
    return data[:width].copy()


# VisualSfM .nvm as main_vsfm.cpp:144-250 reads it: two ignored lines, the number of cameras, one line per camera
# (file name, focal length, quaternion w x y z, camera centre, radial distortion, 0), an ignored line, the number of 3D
# points, one line per point (position, colour, number of measurements, then per measurement camera index, feature
# index, x, y).
def nvm_rotation(qw, qx, qy, qz):
    """main_vsfm.cpp:188-199"""
    return np.array([[1.0 - 2.0 * qy * qy - 2.0 * qz * qz, 2.0 * qx * qy - 2.0 * qz * qw, 2.0 * qx * qz + 2.0 * qy * qw],
                     [2.0 * qx * qy + 2.0 * qz * qw, 1.0 - 2.0 * qx * qx - 2.0 * qz * qz, 2.0 * qy * qz - 2.0 * qx * qw],
                     [2.0 * qx * qz - 2.0 * qy * qw, 2.0 * qy * qz + 2.0 * qx * qw, 1.0 - 2.0 * qx * qx - 2.0 * qy * qy]])


def _mv3(M, v):
    """M v for a 3x3 M in the evaluation order of the reference's fixed-size Eigen product (and of the C-ABI readers):
    (M[i,0] v[0] + M[i,1] v[1]) + M[i,2] v[2] -- numpy's matmul may sum in another order or fuse the multiplies"""
    M = np.asarray(M, np.float64); v = np.asarray(v, np.float64)
    return (M[:, 0] * v[0] + M[:, 1] * v[1]) + M[:, 2] * v[2]


def read_nvm(path):
    """-> list of cameras in file order (the reference uses the index as camID): dict(filename, focal, R, t, C,
    distortion, worldpoints = ids of the 3D points it sees, median_depth = sorted distances to them [n/2] as float32,
    main_vsfm.cpp:300-303; None for a camera without points, which the reference skips)"""
    with open(path) as f:
        lines = f.read().split("\n")
    pos = 2
    n_cams = int(lines[pos].split()[0]); pos += 1
    if n_cams == 0:
        raise ValueError("No aligned cameras in NVM file!")          # main_vsfm.cpp:157-161
    cams = []
    for i in range(n_cams):
        tok = lines[pos].split(); pos += 1
        focal, qw, qx, qy, qz, cx, cy, cz, dist = (float(x) for x in tok[1:10])
        R = nvm_rotation(qw, qx, qy, qz)
        Cc = np.array([cx, cy, cz])
        cams.append(dict(filename=tok[0], focal=np.float32(focal), R=R, t=_mv3(-R, Cc), C=Cc, distortion=np.float32(dist),   # t = -R*C, :207
                         worldpoints=[], _depths=[]))
    pos += 1
    n_pts = int(lines[pos].split()[0]); pos += 1
    for i in range(n_pts):
        if pos >= len(lines):
            break                      # the file ends early: the stream parser of main_vsfm.cpp sees no further measurements
        tok = lines[pos].split(); pos += 1
        if len(tok) < 7:
            continue
        p = np.array([float(tok[0]), float(tok[1]), float(tok[2])])
        nv = int(tok[6])
        for j in range(nv):
            cam = int(tok[7 + 4 * j])
            if cam >= n_cams:
                raise ValueError("malformed measurement in NVM file")
            cams[cam]["worldpoints"].append(i)
            cams[cam]["_depths"].append(np.float32(np.linalg.norm(p - cams[cam]["C"])))
    for c in cams:
        d = sorted(c.pop("_depths"))
        c["median_depth"] = d[len(d) // 2] if d else None
    return cams


def nvm_intrinsics(focal, width, height):
    """K as main_vsfm.cpp:272-282 builds it: principal point at the image centre (float arithmetic there)"""
    return np.array([[np.float32(focal), 0.0, np.float32(width) / np.float32(2.0)],
                     [0.0, np.float32(focal), np.float32(height) / np.float32(2.0)], [0.0, 0.0, 1.0]], np.float64)


# ---- COLMAP text results and bundler files (the Python twin of l3d_sfm_open_colmap / l3d_sfm_open_bundler) --------------
def rotation_from_q(qw, qx, qy, qz):
    """Line3D::rotationFromQ, line3D.cc:2730-2754"""
    n = qw * qw + qx * qx + qy * qy + qz * qz
    s = 0.0 if abs(n) < 1e-12 else 2.0 / n
    wx, wy, wz = s * qw * qx, s * qw * qy, s * qw * qz
    xx, xy, xz = s * qx * qx, s * qx * qy, s * qx * qz
    yy, yz, zz = s * qy * qy, s * qy * qz, s * qz * qz
    return np.array([[1.0 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1.0 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1.0 - (xx + yy)]])


_COLMAP_MODELS = {  # parameter order of cameras.txt -> (fx, fy, cx, cy, k1, k2, p1, p2, k3), main_colmap.cpp:177-219
    "SIMPLE_PINHOLE": lambda p: (p[0], p[0], p[1], p[2], 0, 0, 0, 0, 0),
    "PINHOLE": lambda p: (p[0], p[1], p[2], p[3], 0, 0, 0, 0, 0),
    "SIMPLE_RADIAL": lambda p: (p[0], p[0], p[1], p[2], p[3], 0, 0, 0, 0),
    "RADIAL": lambda p: (p[0], p[0], p[1], p[2], p[3], p[4], 0, 0, 0),
    "OPENCV": lambda p: (p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], 0),
    "FULL_OPENCV": lambda p: (p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]),
    # beyond the reference: undistorted by camera model, the five coefficients are zero
    "OPENCV_FISHEYE": lambda p: (p[0], p[1], p[2], p[3], 0, 0, 0, 0, 0),
    "FOV": lambda p: (p[0], p[1], p[2], p[3], 0, 0, 0, 0, 0),
    "SIMPLE_RADIAL_FISHEYE": lambda p: (p[0], p[0], p[1], p[2], 0, 0, 0, 0, 0),
    "RADIAL_FISHEYE": lambda p: (p[0], p[0], p[1], p[2], 0, 0, 0, 0, 0),
}
# COLMAP's binary model ids, in order, with the length of each model's parameter list
COLMAP_MODEL_IDS = (("SIMPLE_PINHOLE", 3), ("PINHOLE", 4), ("SIMPLE_RADIAL", 4), ("RADIAL", 5), ("OPENCV", 8),
                    ("OPENCV_FISHEYE", 8), ("FULL_OPENCV", 12), ("FOV", 5), ("SIMPLE_RADIAL_FISHEYE", 4),
                    ("RADIAL_FISHEYE", 5), ("THIN_PRISM_FISHEYE", 12))
_COLMAP_N_PARAMS = dict(COLMAP_MODEL_IDS)
# (index of the first distortion parameter in the list, their number) of the models l3d_undistort_images_model takes
_COLMAP_DISTORTION = {"FULL_OPENCV": (4, 8), "OPENCV_FISHEYE": (4, 4), "SIMPLE_RADIAL_FISHEYE": (3, 1),
                      "RADIAL_FISHEYE": (3, 2), "FOV": (4, 1)}


def _median_depth(C, pts):
    d = sorted(np.float32(np.linalg.norm(C - p)) for p in pts)
    return d[len(d) // 2] if d else None


def _colmap_camera(model, p, width, height):
    """the camera record of both parsers: p = the parameter list (padded with zeros behind its end)"""
    p = [float(x) for x in p]
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (float(x) for x in _COLMAP_MODELS[model](p + [0.0] * 12))
    n = _COLMAP_N_PARAMS[model]
    return dict(width=width, height=height, K=np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]),
                radial=np.array([k1, k2, k3]), tangential=np.array([p1, p2]), model=model, params=(p + [0.0] * n)[:n])


def _colmap_text(folder):
    """cameras.txt / images.txt / points3D.txt -> (cams, image records, points): an image record is (head, ids) with head =
    dict(id, camera, name, R, t, C) or None (an image line of an unknown camera, or one that does not parse) and ids =
    the POINT3D_IDs of its line of 2D points"""
    import os
    def getlines(path):      # std::getline's view of a file: no extra empty line behind a final newline
        text = open(path).read()
        lines = text.split("\n")
        return lines[:-1] if lines and lines[-1] == "" else lines
    cams = {}
    for line in getlines(os.path.join(folder, "cameras.txt")):
        if line[:1] == "#":
            continue
        tok = line.split()
        # (a blank line is NOT skipped: the reference and l3d_sfm_open_colmap parse it and fail on its empty model name)
        model = tok[1] if len(tok) > 1 else ""
        if model not in _COLMAP_MODELS:
            raise ValueError(f"camera model {model} unknown!")
        cams[int(tok[0])] = _colmap_camera(model, [float(x) for x in tok[4:]], int(tok[2]), int(tok[3]))
    records = []
    first = True
    for line in open(os.path.join(folder, "images.txt")).read().split("\n"):
        if line[:1] == "#":
            continue
        tok = line.split()
        if first:
            head = None
            if len(tok) >= 9 and int(tok[8]) in cams:
                R = rotation_from_q(*(float(x) for x in tok[1:5]))
                t = np.array([float(x) for x in tok[5:8]])
                head = dict(id=int(tok[0]), camera=int(tok[8]), name=tok[9] if len(tok) > 9 else "", R=R, t=t, C=R.T @ (-1.0 * t))
            records.append([head, None])
            first = False
        else:
            if records[-1][0] is not None:
                records[-1][1] = [int(tok[k]) for k in range(2, len(tok), 3)]
            first = True
    points = []
    for line in open(os.path.join(folder, "points3D.txt")).read().split("\n"):
        tok = line.split()
        try:
            points.append((int(tok[0]), float(tok[1]), float(tok[2]), float(tok[3])))
        except (ValueError, IndexError):
            continue
    return cams, records, points


class _Cursor:
    """a COLMAP binary file in memory, read little-endian with a cursor that never passes its end"""

    def __init__(self, folder, name):
        import os
        self.name = name
        with open(os.path.join(folder, name), "rb") as f:
            self.buf = f.read()
        self.pos = 0

    def left(self):
        return len(self.buf) - self.pos

    def get(self, fmt):
        import struct
        n = struct.calcsize("<" + fmt)
        if self.left() < n:
            raise ValueError(f"{self.name}: the file ends inside a record (truncated?)")
        v = struct.unpack_from("<" + fmt, self.buf, self.pos)
        self.pos += n
        return v

    def count(self, what, least):
        """a u64 count of records of at least `least` bytes each, checked against what is left before anything is made"""
        n, = self.get("Q")
        if n > self.left() // least:
            raise ValueError(f"{self.name}: {n} {what} cannot fit in the {self.left()} bytes that follow")
        return n

    def finish(self):
        if self.left():
            raise ValueError(f"{self.name}: {self.left()} bytes behind the last record")


def _atoi(n):
    """POINT3D_ID of images.bin as l3d_sfm_open_colmap's atoi sees the same number in decimal: strtol saturates at
    LONG_MAX and the int keeps its low 32 bits, so 2^64 - 1 ("no point") is -1"""
    n = min(n, 2 ** 63 - 1) & 0xFFFFFFFF
    return n - 2 ** 32 if n >= 2 ** 31 else n


def _colmap_binary(folder):
    """cameras.bin / images.bin / points3D.bin (COLMAP's binary model) -> the records of _colmap_text"""
    f = _Cursor(folder, "cameras.bin")
    cams = {}
    for _ in range(f.count("cameras", 48)):
        cid, model_id, width, height = f.get("IiQQ")
        known = 0 <= model_id < len(COLMAP_MODEL_IDS) and COLMAP_MODEL_IDS[model_id][0] in _COLMAP_MODELS
        if not known:
            raise ValueError(f"camera model {COLMAP_MODEL_IDS[model_id][0] if 0 <= model_id < len(COLMAP_MODEL_IDS) else model_id} unknown!")
        if width >= 2 ** 32 or height >= 2 ** 32:
            raise ValueError(f"{f.name}: image size of camera {cid} beyond 32 bits")
        model, n = COLMAP_MODEL_IDS[model_id]
        cams[cid] = _colmap_camera(model, list(f.get(f"{n}d")), width, height)
    f.finish()
    f = _Cursor(folder, "images.bin")
    records = []
    for _ in range(f.count("images", 73)):
        iid, qw, qx, qy, qz, tx, ty, tz, cid = f.get("I7dI")
        end = f.buf.find(b"\0", f.pos)
        if end < 0:
            raise ValueError(f"{f.name}: the file ends inside a record (truncated?)")
        name = f.buf[f.pos:end].decode("utf-8", "surrogateescape")
        f.pos = end + 1
        m = f.count("2D points", 24)
        ids = [_atoi(f.get("2dQ")[2]) for _ in range(m)]
        head = None
        if cid in cams:
            R = rotation_from_q(qw, qx, qy, qz)
            t = np.array([tx, ty, tz])
            head = dict(id=iid, camera=cid, name=name, R=R, t=t, C=R.T @ (-1.0 * t))
        records.append([head, ids])
    f.finish()
    f = _Cursor(folder, "points3D.bin")
    points = []
    for _ in range(f.count("3D points", 51)):
        pid, X, Y, Z, _r, _g, _b, _err = f.get("Q3d3Bd")
        track = f.count("track elements", 8)
        f.pos += 8 * track
        if pid < 2 ** 32:                    # (the text reader of the C-ABI takes the id as a uint32_t)
            points.append((pid, X, Y, Z))
    f.finish()
    return cams, records, points


def read_colmap(folder):
    """cameras.txt / images.txt / points3D.txt as main_colmap.cpp:136-348 reads them or, where there is no cameras.txt and
    cameras.bin, images.bin and points3D.bin all exist, COLMAP's binary form of the same -> list of images
    in file order: dict(id, camera, name, width, height, K, R, t, C, radial (k1, k2, k3), tangential (p1, p2), model
    (COLMAP's name), params (the model's parameter list), worldpoints, median_depth or None).  An image whose camera is
    unknown is dropped; points3D.txt lines that do not parse as "id X Y Z" are ignored; a worldpoint without an entry
    there sits at the origin (the reference's map default).  A binary file that is truncated, over-long or states a
    count that cannot fit: ValueError with its name."""
    import os
    binary = not os.path.exists(os.path.join(folder, "cameras.txt")) and all(
        os.path.exists(os.path.join(folder, n)) for n in ("cameras.bin", "images.bin", "points3D.bin"))
    cams, records, points = (_colmap_binary if binary else _colmap_text)(folder)
    imgs, by_id, wps = [], {}, {}
    for head, ids in records:
        if head is None:
            continue
        cur = dict(head, worldpoints=[], **cams[head["camera"]])
        by_id[cur["id"]] = cur
        imgs.append(cur)
        if ids is not None:
            lst = []
            for wp in ids:
                if wp >= 0:
                    lst.append(wp); wps[wp] = np.zeros(3)
            cur["worldpoints"] = lst
    # a repeated IMAGE_ID: the reference's maps are keyed by the id, so BOTH entries of the image sequence see the last pose
    # and the last worldpoint list (l3d_sfm_open_colmap does the same fix-up)
    imgs = [im if by_id[im["id"]] is im else dict(by_id[im["id"]]) for im in imgs]
    for pid, X, Y, Z in points:
        if pid in wps:
            wps[pid] = np.array([X, Y, Z])
    for im in imgs:
        im["median_depth"] = _median_depth(im["C"], [wps[w] for w in im["worldpoints"]])
    return imgs


def read_bundler(path):
    """bundle.rd.out as main_bundler.cpp:147-252 reads it -> list of cameras (index = camID): dict(id, focal, radial
    (d1, d2, 0), R, t (second and third row / entry negated), C, worldpoints, median_depth or None)"""
    lines = open(path).read().split("\n")
    n_cams, n_pts = (int(x) for x in lines[1].split()[:2])
    if n_cams == 0 or n_pts == 0:
        raise ValueError("No cameras and/or points in bundle file!")
    pos, cams = 2, []
    for i in range(n_cams):
        f, d1, d2 = (float(x) for x in lines[pos].split()[:3])
        R = np.array([[float(x) for x in lines[pos + 1 + j].split()[:3]] for j in range(3)])
        R[1] *= -1.0; R[2] *= -1.0
        t = np.array([float(x) for x in lines[pos + 4].split()[:3]])
        t[1] *= -1.0; t[2] *= -1.0
        cams.append(dict(id=i, focal=np.float32(f), radial=np.array([np.float32(d1), np.float32(d2), 0.0]), R=R, t=t,
                         C=R.T @ (-1.0 * t), worldpoints=[], _pts=[]))
        pos += 5
    for i in range(n_pts):
        if pos + 2 >= len(lines):
            break
        p = np.array([float(x) for x in lines[pos].split()[:3]])
        tok = lines[pos + 2].split()
        for j in range(int(tok[0])):
            cam = int(tok[1 + 4 * j])
            if cam >= n_cams:
                raise ValueError("malformed view list in bundle file")
            cams[cam]["worldpoints"].append(i); cams[cam]["_pts"].append(p)
        pos += 3
    for c in cams:
        c["median_depth"] = _median_depth(c["C"], c.pop("_pts"))
    return cams


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
