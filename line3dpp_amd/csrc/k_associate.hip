// k_associate.hip -- the 2D segments of a camera assigned to the projected 3D lines they observe (host
// side: l3d_associate.hip).  No counterpart in the reference.  The arithmetic is the contract of §17, fp64 in the order
// written there (the library is built with -ffp-contract=off), so that tests/associate_model.py follows it operation
// for operation.
//   k_associate    the unit of work is a TILE of kAssocTile = 256 consecutive 2D segments of one camera: one workgroup of
//                  four waves, one lane per segment.  All cameras of a group share the launch; a workgroup finds its
//                  camera by a binary search in the exclusive prefix of tiles per camera (uniform: scalar loads).  The
//                  camera's records pass through LDS in chunks of kAssocChunk = 512 (16 KiB), loaded coalesced by the
//                  whole workgroup; every lane walks the chunk with broadcast reads (all lanes read the same address: no
//                  bank conflict) and keeps (bits(D2), r, frac) of its best and its count in registers -- no atomics and
//                  no cross-lane traffic, and the ascending walk makes the smaller index win equal distances.  The tests
//                  are ordered cheapest first (a record shorter than a pixel is skipped by the whole workgroup; the angle
//                  test needs no division, the distance one, the overlap three); a pair is accepted iff all hold, so the
//                  order changes nothing.  Lanes beyond the camera's last segment take part in every barrier and write
//                  nothing.
#include "l3d_kernels.h"

namespace l3d {
namespace {

static_assert(kAssocChunk % kAssocTile == 0, "the workgroup loads a chunk in whole rounds");

__global__ __launch_bounds__(kAssocTile) void k_associate(AssocArgs a) {
    __shared__ float4 s_rec[kAssocChunk][2];       // ProjRecord: (x1, y1, x2, y2), (iz1, iz2, line, segment)
    // the camera of this tile: the last one whose first tile is <= blockIdx.x (cameras without segments own no tile and
    // share their successor's first tile: they are passed over)
    uint32_t lo = 0, hi = a.n_cams;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.cams[mid].tile0 <= blockIdx.x) lo = mid; else hi = mid;
    }
    const AssocCam cam = a.cams[lo];
    const uint32_t s = (blockIdx.x - cam.tile0) * kAssocTile + threadIdx.x;     // segment of this lane in its camera
    const bool in_range = s < cam.n_seg;
    double px = 0.0, py = 0.0, qx = 0.0, qy = 0.0;
    if (in_range) {
        const float4 v = a.segs[(size_t)cam.seg0 + s];
        px = (double)v.x; py = (double)v.y; qx = (double)v.z; qy = (double)v.w;
    }
    const double ex = qx - px, ey = qy - py;
    const double E2 = ex * ex + ey * ey;
    const bool live = in_range && E2 > 0.0;
    unsigned long long best_bits = ~0ull;
    uint32_t best_r = 0xFFFFFFFFu, n_acc = 0;
    double best_frac = 0.0;
    const float4* rec = (const float4*)(a.rec + cam.rec0);
    for (uint32_t r0 = 0; r0 < cam.n_rec; r0 += kAssocChunk) {
        const uint32_t n = min(kAssocChunk, cam.n_rec - r0);
        __syncthreads();                                                         // the previous chunk has been read
        for (uint32_t i = threadIdx.x; i < 2 * n; i += kAssocTile) (&s_rec[0][0])[i] = rec[2 * (size_t)r0 + i];
        __syncthreads();
        for (uint32_t k = 0; k < n; ++k) {
            const float4 rv = s_rec[k][0];
            // 1. record vector and length
            const double ax = (double)rv.x, ay = (double)rv.y;
            const double dx = (double)rv.z - ax, dy = (double)rv.w - ay;
            const double L2 = dx * dx + dy * dy;
            if (L2 < 1.0) continue;                                              // (uniform)
            if (!live) continue;
            // 4. angle
            const double dot = dx * ex + dy * ey;
            if (!(dot * dot >= a.min_cos2 * (L2 * E2))) continue;
            // 3. distance
            const double c1 = dx * (py - ay) - dy * (px - ax);
            const double c2 = dx * (qy - ay) - dy * (qx - ax);
            const double m1 = c1 * c1, m2 = c2 * c2;
            const double D2 = (m1 > m2 ? m1 : m2) / L2;
            if (!(D2 <= a.max_d2)) continue;
            // 5. overlap
            const double t1 = (dx * (px - ax) + dy * (py - ay)) / L2;
            const double t2 = (dx * (qx - ax) + dy * (qy - ay)) / L2;
            const double tlo = t1 < t2 ? t1 : t2, thi = t1 < t2 ? t2 : t1;
            const double ov = (thi < 1.0 ? thi : 1.0) - (tlo > 0.0 ? tlo : 0.0);
            if (!(ov > 0.0)) continue;
            const double frac = ov / (thi - tlo);
            if (!(frac >= a.min_overlap)) continue;
            ++n_acc;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(D2);
            if (bits < best_bits) { best_bits = bits; best_r = r0 + k; best_frac = frac; }
        }
    }
    if (!in_range) return;
    AssocOut o{-1, 0xFFFFFFFFu, 0xFFFFFFFFu, 0.0f, 0.0f, 0u};
    if (n_acc) {
        const ProjRecord w = a.rec[(size_t)cam.rec0 + best_r];
        o.record = (int32_t)best_r; o.line = w.line; o.segment = w.segment & kAssocSegmentMask;
        o.d2 = (float)__longlong_as_double((long long)best_bits); o.overlap = (float)best_frac; o.n_accepted = n_acc;
    }
    a.out[(size_t)cam.seg0 + s] = o;
}

}  // namespace

hipError_t launch_associate(const AssocArgs& a, uint32_t n_tiles, hipStream_t st) {
    if (!a.n_cams || !n_tiles) return hipSuccess;
    hipLaunchKernelGGL(k_associate, dim3(n_tiles), dim3(kAssocTile), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d
