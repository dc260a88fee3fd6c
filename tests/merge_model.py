"""The contract of DESIGN §19 (near-duplicate 3D lines merged) restated in numpy.  Stage 1, the accepted pairs, in a
scalar form over compare_model.pair and in an array form chunked over the queries (tests/test_merge_host.py shows the two
identical); stages 2 and 3, the components and the fusion, as plain loops over Python floats.  All arithmetic is fp64 in
the order of the text: Python floats and numpy's element-wise float64 operations round every operation on its own, as the
library does when built with -ffp-contract=off; dot products are written out left to right and sums over members run one
after another in ascending index order."""
import math

import numpy as np

from tests import compare_model as CM

LINE_INFO_DTYPE = np.dtype([("n_members", "<u4"), ("label", "<u4"), ("max_offset", "<f8")])
SUMMARY_KEYS = ("n_segments_in", "n_segments_out", "n_lines_in", "n_lines_out", "n_pairs", "n_merged_components",
                "largest_component", "length_in", "length_out", "max_offset")
min_cos2_of = CM.min_cos2_of
extent = CM.extent


# ---- stage 1 ----------------------------------------------------------------------------------------------------------
def pairs_scalar(segs, line, max_distance, min_cos2, min_overlap):
    """the accepted ordered pairs, pair by pair -> [k, 2] uint32 (q, r), ascending"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    out = []
    for q in range(len(segs)):
        for r in range(len(segs)):
            if CM.pair(segs[q], line[q], segs[r], line[r], float(max_distance), float(min_cos2), float(min_overlap), True)[0]:
                out.append((q, r))
    return np.array(out, np.uint32).reshape(-1, 2)


def pairs(segs, line, max_distance, min_cos2, min_overlap, chunk=512):
    """the array form of pairs_scalar: all references against `chunk` queries at a time"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6); line = np.asarray(line, np.uint32).reshape(-1)
    if not len(segs):
        return np.zeros((0, 2), np.uint32)
    md2 = np.float64(max_distance) * np.float64(max_distance)
    min_cos2 = np.float64(min_cos2); min_overlap = np.float64(min_overlap)
    bx, by, bz = segs[None, :, 0], segs[None, :, 1], segs[None, :, 2]
    dx, dy, dz = segs[None, :, 3] - bx, segs[None, :, 4] - by, segs[None, :, 5] - bz
    L2 = dx * dx + dy * dy + dz * dz
    used = L2 > 0.0
    L2s = np.where(used, L2, 1.0)
    out = []
    for s0 in range(0, len(segs), chunk):
        sg = segs[s0:s0 + chunk]
        px, py, pz, sx, sy, sz = (sg[:, k:k + 1] for k in range(6))
        ex, ey, ez = sx - px, sy - py, sz - pz
        E2 = ex * ex + ey * ey + ez * ez
        ok = used & (E2 > 0.0) & (line[s0:s0 + chunk, None] != line[None, :])
        dot = dx * ex + dy * ey + dz * ez
        ok &= dot * dot >= min_cos2 * (L2 * E2)
        wx, wy, wz = px - bx, py - by, pz - bz
        ux, uy, uz = sx - bx, sy - by, sz - bz
        c1x, c1y, c1z = dy * wz - dz * wy, dz * wx - dx * wz, dx * wy - dy * wx
        c2x, c2y, c2z = dy * uz - dz * uy, dz * ux - dx * uz, dx * uy - dy * ux
        m1 = c1x * c1x + c1y * c1y + c1z * c1z
        m2 = c2x * c2x + c2y * c2y + c2z * c2z
        ok &= np.maximum(m1, m2) / L2s <= md2
        t1 = (dx * wx + dy * wy + dz * wz) / L2s
        t2 = (dx * ux + dy * uy + dz * uz) / L2s
        lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
        ov = np.minimum(hi, 1.0) - np.maximum(lo, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = ov / (hi - lo)
        ok &= (ov > 0.0) & (frac >= min_overlap)
        q, r = np.nonzero(ok)                              # row-major: ascending (q, r)
        out.append(np.stack([q + s0, r], 1).astype(np.uint32))
    return np.concatenate(out)


# ---- stage 2 ----------------------------------------------------------------------------------------------------------
def components(line, pair_list):
    """-> (labels: the ascending labels of the output lines, label_of: dict input line index -> label)"""
    ids = sorted(set(int(v) for v in line))
    parent = {i: i for i in ids}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for q, r in pair_list:
        a, b = find(int(line[q])), find(int(line[r]))
        if a != b:
            parent[max(a, b)] = min(a, b)                  # the smaller index is the root: a root is its component's label
    label_of = {i: find(i) for i in ids}
    return sorted(set(label_of.values())), label_of


# ---- stage 3 ----------------------------------------------------------------------------------------------------------
def _length(v):
    ex, ey, ez = float(v[3]) - float(v[0]), float(v[4]) - float(v[1]), float(v[5]) - float(v[2])
    return math.sqrt(ex * ex + ey * ey + ez * ez), (ex, ey, ez)


def fuse(segs, members):
    """one component of two or more lines; members = its live segments in ascending index -> (segments [k, 6],
    max_offset, leader: the index of the leading segment)"""
    e, ln = [], []
    for i in members:                                       # 1.
        length, vec = _length(segs[i])
        e.append(vec); ln.append(length)
    lead = 0
    for k in range(len(members)):
        if ln[k] > ln[lead]:
            lead = k                                        # (the first of equal lengths stays)
    dsx = dsy = dsz = 0.0                                   # 2.
    for ex, ey, ez in e:
        s = -1.0 if ex * e[lead][0] + ey * e[lead][1] + ez * e[lead][2] < 0.0 else 1.0
        dsx += s * ex; dsy += s * ey; dsz += s * ez
    dn = math.sqrt(dsx * dsx + dsy * dsy + dsz * dsz)
    ux, uy, uz = dsx / dn, dsy / dn, dsz / dn
    W = csx = csy = csz = 0.0                               # 3.
    for k, i in enumerate(members):
        v = [float(x) for x in segs[i]]
        mx, my, mz = (v[0] + v[3]) * 0.5, (v[1] + v[4]) * 0.5, (v[2] + v[5]) * 0.5
        W += ln[k]
        csx += ln[k] * mx; csy += ln[k] * my; csz += ln[k] * mz
    cx, cy, cz = csx / W, csy / W, csz / W
    iv = []
    max_offset = 0.0
    for i in members:                                       # 4. and 7.
        v = [float(x) for x in segs[i]]
        t = []
        for end in (0, 3):
            wx, wy, wz = v[end] - cx, v[end + 1] - cy, v[end + 2] - cz
            tt = wx * ux + wy * uy + wz * uz
            off2 = (wx * wx + wy * wy + wz * wz) - tt * tt
            off = math.sqrt(off2) if off2 > 0.0 else 0.0
            max_offset = max(max_offset, off)
            t.append(tt)
        iv.append((min(t), max(t), i))
    iv.sort(key=lambda x: (x[0], x[2]))                     # 5.
    runs = []
    cur_lo, cur_hi = iv[0][0], iv[0][1]
    for lo, hi, _ in iv[1:]:
        if lo <= cur_hi:
            cur_hi = max(cur_hi, hi)
        else:
            runs.append((cur_lo, cur_hi)); cur_lo, cur_hi = lo, hi
    runs.append((cur_lo, cur_hi))
    out = [(cx + lo * ux, cy + lo * uy, cz + lo * uz, cx + hi * ux, cy + hi * uy, cz + hi * uz) for lo, hi in runs]   # 6.
    return np.array(out, np.float64).reshape(-1, 6), max_offset, members[lead]


def merge_from_pairs(segs, line, pair_list):
    """stages 2 and 3 -> (segs_out [m, 6], line_out [m], line_map [n], line_info, summary, detail); detail: per output
    line the ascending member lines and the line of the leader"""
    segs = np.ascontiguousarray(segs, np.float64).reshape(-1, 6); line = np.asarray(line, np.uint32).reshape(-1)
    n = len(segs)
    labels, label_of = components(line, pair_list)
    number = {lab: k for k, lab in enumerate(labels)}
    line_map = np.array([number[label_of[int(v)]] for v in line], np.uint32).reshape(-1)
    member_lines = [[] for _ in labels]
    for i in sorted(label_of):
        member_lines[number[label_of[i]]].append(i)
    info = np.zeros(len(labels), LINE_INFO_DTYPE)
    segs_of = [[] for _ in labels]                          # the input segments of every output line, ascending
    for i in range(n):
        segs_of[line_map[i]].append(i)
    out, out_line, leaders = [], [], []
    for k, lab in enumerate(labels):
        info[k]["n_members"] = len(member_lines[k]); info[k]["label"] = lab
        if len(member_lines[k]) == 1:
            got = segs[segs_of[k]]
            leaders.append(lab)
        else:
            live = []
            for i in segs_of[k]:
                ex, ey, ez = _length(segs[i])[1]
                if ex * ex + ey * ey + ez * ez > 0.0:       # E2 > 0: a point segment is dropped
                    live.append(i)
            got, info[k]["max_offset"], lead = fuse(segs, live)
            leaders.append(int(line[lead]))
        out.append(got); out_line += [k] * len(got)
    segs_out = np.concatenate(out).reshape(-1, 6) if out else np.zeros((0, 6))
    length_in = length_out = 0.0
    for v in segs:
        length_in += _length(v)[0]
    for v in segs_out:
        length_out += _length(v)[0]
    summary = dict(n_segments_in=n, n_segments_out=len(segs_out), n_lines_in=len(label_of), n_lines_out=len(labels),
                   n_pairs=len(pair_list), n_merged_components=int((info["n_members"] >= 2).sum()),
                   largest_component=int(info["n_members"].max()) if len(info) else 0, length_in=length_in, length_out=length_out,
                   max_offset=float(info["max_offset"].max()) if len(info) else 0.0)
    return (np.ascontiguousarray(segs_out), np.array(out_line, np.uint32).reshape(-1), line_map, info, summary,
            dict(member_lines=member_lines, leader_line=leaders))


def merge(segs, line, max_distance, min_cos2, min_overlap, form=pairs):
    """what one call of the library returns: (segs_out, line_out, line_map, line_info, summary)"""
    p = form(segs, line, max_distance, min_cos2, min_overlap)
    return merge_from_pairs(segs, line, p)[:5]
