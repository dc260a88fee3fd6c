"""The contract of DESIGN §24 (where 3D lines meet: junctions and the wireframe graph) restated in numpy, from its text.
Stage 1, the junctions, in a scalar form over Python floats and in an array form chunked over the first segments
(tests/test_wireframe_host.py shows the two identical); stage 2, the graph, as plain loops over Python floats.  All
arithmetic is fp64 in the order of the text: Python floats and numpy's element-wise float64 operations round every
operation on its own, as the library does when built with -ffp-contract=off; dot products are written out left to right
and sums over members run one after another in ascending index order."""
import math

import numpy as np

RECORD_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("sa", "<f8"), ("sb", "<f8"), ("gap2", "<f8")])
JUNCTION_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("kind", "<u4"), ("class_a", "<u4"), ("class_b", "<u4"), ("vertex", "<u4"),
                           ("sa", "<f8"), ("sb", "<f8"), ("gap", "<f8"), ("J", "<f8", 3)])
VERTEX_DTYPE = np.dtype([("P", "<f8", 3), ("spread", "<f8"), ("n_junctions", "<u4"), ("kinds", "<u4"), ("degree", "<u4"),
                         ("component", "<u4")])
EDGE_DTYPE = np.dtype([("v0", "<u4"), ("v1", "<u4"), ("segment", "<u4"), ("line", "<u4")])
SUMMARY_KEYS = ("n_segments", "n_point_segments", "n_junctions", "n_L", "n_T", "n_X", "n_vertices", "n_junction_vertices",
                "n_free_ends", "n_edges", "n_components", "largest_component", "length_total", "max_gap", "max_spread")
KIND_L, KIND_T, KIND_X = 1, 2, 4
AT_P1, AT_P2, INTERIOR = 0, 1, 2
assert RECORD_DTYPE.itemsize == 32 and JUNCTION_DTYPE.itemsize == 72 and VERTEX_DTYPE.itemsize == 48 and EDGE_DTYPE.itemsize == 16


def min_sin2_of(degrees):
    """sin^2 of an angle in degrees, as api.wireframe_params computes it"""
    s = float(np.sin(np.radians(np.float64(degrees))))
    return s * s


def extent(segs):
    """the diagonal of the bounding box of a model's end points"""
    p = np.asarray(segs, np.float64).reshape(-1, 3)
    return float(np.sqrt(((p.max(0) - p.min(0)) ** 2).sum())) if len(p) else 0.0


# ---- stage 1 ----------------------------------------------------------------------------------------------------------
def pair(va, vb, max_distance, max_extension, min_sin2):
    """the test of one ordered pair of live segments of different lines, va in the first role -> (sa, sb, gap2) or None"""
    p1a = [float(x) for x in va[:3]]; p1b = [float(x) for x in vb[:3]]
    ea = [float(va[3 + c]) - p1a[c] for c in range(3)]
    eb = [float(vb[3 + c]) - p1b[c] for c in range(3)]
    w = [p1a[c] - p1b[c] for c in range(3)]

    def dot(x, y):
        return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
    A, B, C, D, E = dot(ea, ea), dot(ea, eb), dot(eb, eb), dot(ea, w), dot(eb, w)
    den = A * C - B * B
    if not (den > 0.0 and den >= min_sin2 * (A * C)):
        return None
    sa = (B * E - C * D) / den
    sb = (A * E - B * D) / den
    La, Lb = math.sqrt(A), math.sqrt(C)
    ta, tb = sa * La, sb * Lb
    if not (ta >= -max_extension and ta <= La + max_extension and tb >= -max_extension and tb <= Lb + max_extension):
        return None
    g = [(p1a[c] + sa * ea[c]) - (p1b[c] + sb * eb[c]) for c in range(3)]
    gap2 = dot(g, g)
    if not gap2 <= max_distance * max_distance:
        return None
    return sa, sb, gap2


def _live(v):
    e = [float(v[3 + c]) - float(v[c]) for c in range(3)]
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] > 0.0


def junctions_scalar(segs, line, max_distance, max_extension, min_sin2):
    """the junction records, pair by pair -> RECORD_DTYPE array in ascending (a, b) order"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6)
    md, mx, ms = float(max_distance), float(max_extension), float(min_sin2)
    live = [_live(v) for v in segs]
    out = []
    for a in range(len(segs)):
        for b in range(a + 1, len(segs)):
            if not (live[a] and live[b]) or int(line[a]) == int(line[b]):
                continue
            got = pair(segs[a], segs[b], md, mx, ms)
            if got is not None:
                out.append((a, b) + got)
    return np.array(out, RECORD_DTYPE).reshape(-1)


def junctions(segs, line, max_distance, max_extension, min_sin2, chunk=256):
    """the array form of junctions_scalar: `chunk` first segments against all second ones at a time"""
    segs = np.asarray(segs, np.float64).reshape(-1, 6); line = np.asarray(line, np.uint32).reshape(-1)
    n = len(segs)
    if not n:
        return np.zeros(0, RECORD_DTYPE)
    md2 = np.float64(max_distance) * np.float64(max_distance)
    mx = np.float64(max_extension); ms = np.float64(min_sin2)
    P1 = [segs[:, c] for c in range(3)]
    e = [segs[:, 3 + c] - segs[:, c] for c in range(3)]
    E2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    L = np.sqrt(E2)
    index = np.arange(n)
    out = []
    with np.errstate(all="ignore"):
        for a0 in range(0, n, chunk):
            a1 = min(n, a0 + chunk)
            b0 = a0 + 1                                     # (nothing below the chunk's first segment can follow it)
            pa = [P1[c][a0:a1, None] for c in range(3)]; ea = [e[c][a0:a1, None] for c in range(3)]
            pb = [P1[c][None, b0:] for c in range(3)]; eb = [e[c][None, b0:] for c in range(3)]
            A = E2[a0:a1, None]; C = E2[None, b0:]
            La = L[a0:a1, None]; Lb = L[None, b0:]
            ok = (index[a0:a1, None] < index[None, b0:]) & (A > 0.0) & (C > 0.0) & (line[a0:a1, None] != line[None, b0:])
            w = [pa[c] - pb[c] for c in range(3)]
            B = (ea[0] * eb[0] + ea[1] * eb[1]) + ea[2] * eb[2]
            D = (ea[0] * w[0] + ea[1] * w[1]) + ea[2] * w[2]
            E = (eb[0] * w[0] + eb[1] * w[1]) + eb[2] * w[2]
            AC = A * C
            den = AC - B * B
            ok &= (den > 0.0) & (den >= ms * AC)
            dens = np.where(den > 0.0, den, 1.0)
            sa = (B * E - C * D) / dens
            sb = (A * E - B * D) / dens
            ta = sa * La; tb = sb * Lb
            ok &= (ta >= -mx) & (ta <= La + mx) & (tb >= -mx) & (tb <= Lb + mx)
            g = [(pa[c] + sa * ea[c]) - (pb[c] + sb * eb[c]) for c in range(3)]
            gap2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
            ok &= gap2 <= md2
            ia, ib = np.nonzero(ok)                         # row-major: ascending (a, b)
            rec = np.zeros(len(ia), RECORD_DTYPE)
            rec["a"] = ia + a0; rec["b"] = ib + b0
            rec["sa"] = sa[ia, ib]; rec["sb"] = sb[ia, ib]; rec["gap2"] = gap2[ia, ib]
            out.append(rec)
    return np.concatenate(out)


# ---- stage 2 ----------------------------------------------------------------------------------------------------------
class _Sets:
    """union-find; the smaller index becomes the root, so a root is the smallest member of its set"""

    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        while self.parent[x] != x:
            self.parent[x] = self.parent[self.parent[x]]
            x = self.parent[x]
        return x

    def join(self, x, y):
        a, b = self.find(x), self.find(y)
        if a != b:
            self.parent[max(a, b)] = min(a, b)


def end_class(t, L, max_extension):
    at1, at2 = t <= max_extension, t >= L - max_extension
    if at1 and at2:
        return AT_P1 if t * 2.0 <= L else AT_P2
    return AT_P1 if at1 else AT_P2 if at2 else INTERIOR


def graph(segs, line, records, max_distance, max_extension):
    """stage 2 on the junction records of stage 1 -> dict(junctions, vertices, edges, summary)"""
    segs = np.ascontiguousarray(segs, np.float64).reshape(-1, 6); line = np.asarray(line, np.uint32).reshape(-1)
    md, mx = float(max_distance), float(max_extension)
    n, nj = len(segs), len(records)
    S = [[float(x) for x in v] for v in segs]
    length, live = [], []
    length_total = 0.0
    for v in S:
        e = [v[3 + c] - v[c] for c in range(3)]
        E2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        length.append(math.sqrt(E2)); live.append(E2 > 0.0)
        length_total += length[-1]
    J = np.zeros(nj, JUNCTION_DTYPE)
    sets = _Sets(nj)
    at_end = {}                                             # (segment, end) -> the junctions there, ascending
    inner = [[] for _ in range(n)]                          # per segment: (t, junction) of its interior attachments
    count = {KIND_L: 0, KIND_T: 0, KIND_X: 0}
    max_gap = 0.0
    for k, r in enumerate(records):
        a, b, sa, sb = int(r["a"]), int(r["b"]), float(r["sa"]), float(r["sb"])
        pos = []
        for c in range(3):                                  # 1.
            pa = S[a][c] + sa * (S[a][3 + c] - S[a][c])
            pb = S[b][c] + sb * (S[b][3 + c] - S[b][c])
            pos.append((pa + pb) * 0.5)
        gap = math.sqrt(float(r["gap2"]))
        max_gap = max(max_gap, gap)
        cls = []
        for seg, s in ((a, sa), (b, sb)):                   # 2.
            t = s * length[seg]
            c = end_class(t, length[seg], mx)
            cls.append(c)
            if c == INTERIOR:
                inner[seg].append((t, k))
            else:
                at_end.setdefault((seg, c), []).append(k)
        ends = (cls[0] != INTERIOR) + (cls[1] != INTERIOR)  # 3.
        kind = KIND_L if ends == 2 else KIND_T if ends == 1 else KIND_X
        count[kind] += 1
        J[k] = (a, b, kind, cls[0], cls[1], 0, sa, sb, gap, pos)
    for members in at_end.values():                         # 4. the same end of the same segment
        for k in members[1:]:
            sets.join(members[0], k)
    for seg in range(n):                                    # 4. neighbours in the sweep along a segment's interior
        inner[seg].sort()
        for (t0, k0), (t1, k1) in zip(inner[seg], inner[seg][1:]):
            if t1 - t0 <= md:
                sets.join(k0, k1)
    roots = [k for k in range(nj) if sets.find(k) == k]     # 5. ascending: numbered by the smallest member
    number = {r: i for i, r in enumerate(roots)}
    V = [dict(sum=[0.0, 0.0, 0.0], n=0, kinds=0, spread=0.0, P=None) for _ in roots]
    for k in range(nj):
        v = number[sets.find(k)]
        J[k]["vertex"] = v
        for c in range(3):
            V[v]["sum"][c] += float(J[k]["J"][c])
        V[v]["n"] += 1; V[v]["kinds"] |= int(J[k]["kind"])
    for v in V:
        v["P"] = [v["sum"][c] / float(v["n"]) for c in range(3)]
    for k in range(nj):
        v = V[int(J[k]["vertex"])]
        d = [float(J[k]["J"][c]) - v["P"][c] for c in range(3)]
        v["spread"] = max(v["spread"], math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    n_junction_vertices = len(V)
    max_spread = max([v["spread"] for v in V], default=0.0)
    end_vertex = {}                                         # 6.
    for i in range(n):
        if not live[i]:
            continue
        for end in (0, 1):
            if (i, end) in at_end:
                end_vertex[(i, end)] = int(J[at_end[(i, end)][0]]["vertex"])
            else:
                end_vertex[(i, end)] = len(V)
                V.append(dict(P=S[i][3 * end:3 * end + 3], n=0, kinds=0, spread=0.0))
    degree = [0] * len(V)
    edges = []
    for i in range(n):                                      # 7.
        if not live[i]:
            continue
        first_t = {}
        for t, k in inner[i]:                               # (sorted: the first t of a vertex is its smallest)
            first_t.setdefault(int(J[k]["vertex"]), t)
        stops = [end_vertex[(i, 0)]] + [v for t, v in sorted((t, v) for v, t in first_t.items())] + [end_vertex[(i, 1)]]
        for v0, v1 in zip(stops, stops[1:]):
            if v0 != v1:
                edges.append((v0, v1, i, int(line[i])))
                degree[v0] += 1; degree[v1] += 1
    comp = _Sets(len(V))                                    # 8.
    for v0, v1, _, _ in edges:
        comp.join(v0, v1)
    comp_roots = [v for v in range(len(V)) if comp.find(v) == v]
    comp_number = {r: i for i, r in enumerate(comp_roots)}
    edges_of = [0] * len(comp_roots)
    for v0, _, _, _ in edges:
        edges_of[comp_number[comp.find(v0)]] += 1
    vertices = np.zeros(len(V), VERTEX_DTYPE)
    for i, v in enumerate(V):
        vertices[i] = (v["P"], v["spread"], v["n"], v["kinds"], degree[i], comp_number[comp.find(i)])
    summary = dict(n_segments=n, n_point_segments=n - sum(live), n_junctions=nj, n_L=count[KIND_L], n_T=count[KIND_T],
                   n_X=count[KIND_X], n_vertices=len(V), n_junction_vertices=n_junction_vertices,
                   n_free_ends=len(V) - n_junction_vertices, n_edges=len(edges), n_components=len(comp_roots),
                   largest_component=max(edges_of, default=0), length_total=length_total, max_gap=max_gap, max_spread=max_spread)
    return dict(junctions=J, vertices=vertices, edges=np.array(edges, EDGE_DTYPE).reshape(-1), summary=summary)


def wireframe(segs, line, max_distance, max_extension, min_sin2, form=junctions):
    """what one call of the library returns"""
    rec = form(segs, line, max_distance, max_extension, min_sin2)
    return graph(segs, line, rec, max_distance, max_extension)


def obj_text(w):
    """the OBJ file of a wireframe: vertices at %.17g, then the edges as 1-based lines"""
    out = ["v %.17g %.17g %.17g\n" % tuple(float(x) for x in v["P"]) for v in w["vertices"]]
    out += ["l %d %d\n" % (int(e["v0"]) + 1, int(e["v1"]) + 1) for e in w["edges"]]
    return "".join(out)
