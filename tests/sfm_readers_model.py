"""Independent Python model of the library's readers of its input formats (line3dpp_amd/csrc/l3d_io.hip behind
l3d_nvm_*, l3d_sfm_open_colmap, l3d_sfm_open_bundler and the segment cache, which line3dpp_amd/io.py wraps): VisualSfM
.nvm, COLMAP's text and binary models, bundler files and the boost archive of the segment cache, each written from the
main of the reference that reads it (main_vsfm.cpp, main_colmap.cpp, main_bundler.cpp) and from the documented layouts.
tests/test_input_formats.py, tests/test_colmap_binary.py and tests/test_io_wraps_the_library.py hold the library against
it.

It shares no code with the package.  Rotations, translations, coefficients, names, ids and worldpoint lists equal the
library's bit for bit.  Two values are computed with numpy's own summation order instead of the reference's fixed-size
Eigen products, and the tests give them the only two tolerances of this pair: the camera centre
C = R^T (-t) as `R.T @ (-1.0 * t)`, within 1e-12 absolute, and the depth |X - C| with numpy.linalg.norm, so the float32
median depth within 2e-7 relative (the last bits of C, and one float32 rounding).

Unlike the library's stream parsers the model raises Python's own errors on malformed text (int("abc"), a missing file:
OSError)."""
import numpy as np

# the boost binary archive (layout: line3dpp_amd/io.py, BIN result format)
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


# ---- the segment cache and VisualSfM .nvm files (l3d_*_segment_cache, l3d_nvm_*) -----------------------------------
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


# ---- COLMAP text and binary results and bundler files (l3d_sfm_open_colmap / l3d_sfm_open_bundler) ------------------
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
