// k_project.hip -- the reconstructed 3D lines projected into cameras: 2D segments, line-id and
// inverse-depth planes, overlays.  No counterpart in the reference; the arithmetic is the contract of §16, fp64 in the
// order written there (the library is built with -ffp-contract=off), so that tests/project_lines_model.py follows it
// operation for operation.
//   k_project_lines    one lane per (camera, segment), the block's camera in LDS: R P + t, near plane, K, Liang-Barsky
//                      against [0, w-1] x [0, h-1]; writes the float32 record and a visibility flag.  The flags are
//                      scanned by k_scan.hip's single-launch scan; k_project_compact moves the visible records to
//                      their places: (camera, segment) order, i.e. a stable compaction per camera.
//   k_raster_count     major-axis steps of every record (0 for a record that draws nothing), scanned likewise
//   k_raster_lines     the unit of work is ONE major-axis step: segments are a few to a few thousand pixels long, a lane
//                      or a wave per segment would idle most lanes.  A lane finds the record of its step by binary
//                      search in the scanned step counts (consecutive lanes land on the same few cache lines), computes
//                      the pixel and its inverse depth and sends the 64-bit key (bits(iz) << 32 | ~line) to the key
//                      plane with a no-return atomic max: the nearest line wins, of equal depths the smaller index, in
//                      any order of arrival.  Contention is what the scene gives it -- one atomic per drawn pixel, more
//                      than one on the same word only where lines cross or overlap; there is nothing to pre-reduce per
//                      wave (cdna_hip_programming Guideline 12 is about sums into few destinations).
//   k_map_decode       key plane -> line_id (int32, -1) and inv_depth (float, 0)
//   k_overlay          line_id + source image -> packed RGB, integer blend
// All cameras of a group share each launch: grid.y is the camera for the per-pixel kernels, a flat index elsewhere.
#include <algorithm>

#include "l3d_kernels.h"

namespace l3d {
namespace {

constexpr uint32_t kProjBlock = 256;

__global__ __launch_bounds__(kProjBlock) void k_project_lines(ProjArgs a) {
    __shared__ ProjCam s_cam;
    {
        const double* src = (const double*)(a.cams + blockIdx.y);
        double* dst = (double*)&s_cam;
        for (uint32_t i = threadIdx.x; i < sizeof(ProjCam) / 8; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n_seg) return;
    const ProjCam& c = s_cam;
    const size_t at = (size_t)blockIdx.y * a.n_seg + s;
    const double* P = a.P + 6 * (size_t)s;
    // 1. X = R P + t
    d3 X1 = mul33(c.R, d3{P[0], P[1], P[2]}) + d3{c.t[0], c.t[1], c.t[2]};
    d3 X2 = mul33(c.R, d3{P[3], P[4], P[5]}) + d3{c.t[0], c.t[1], c.t[2]};
    uint32_t flags = 0;
    bool visible = true;
    // 2. near plane
    const double nz = a.near_plane;
    const bool b1 = X1.z < nz, b2 = X2.z < nz;
    if (b1 && b2) visible = false;
    else if (b1) {
        const double t = (nz - X1.z) / (X2.z - X1.z);
        X1.x = X1.x + t * (X2.x - X1.x); X1.y = X1.y + t * (X2.y - X1.y); X1.z = nz;
        flags |= kProjNear;
    } else if (b2) {
        const double t = (nz - X2.z) / (X1.z - X2.z);
        X2.x = X2.x + t * (X1.x - X2.x); X2.y = X2.y + t * (X1.y - X2.y); X2.z = nz;
        flags |= kProjNear;
    }
    ProjRecord r{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0u, 0u};
    if (visible) {
        // 3. pixels and inverse depths
        d3 q = mul33(c.K, d3{X1.x / X1.z, X1.y / X1.z, 1.0});
        const double x1 = q.x / q.z, y1 = q.y / q.z, iz1 = 1.0 / X1.z;
        q = mul33(c.K, d3{X2.x / X2.z, X2.y / X2.z, 1.0});
        const double x2 = q.x / q.z, y2 = q.y / q.z, iz2 = 1.0 / X2.z;
        // 4. Liang-Barsky, edges left, right, top, bottom: p t <= q
        const double dx = x2 - x1, dy = y2 - y1;
        const double p[4] = {-dx, dx, -dy, dy};
        const double qq[4] = {x1, c.xmax - x1, y1, c.ymax - y1};
        double t0 = 0.0, t1 = 1.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (p[e] == 0.0) {
                if (qq[e] < 0.0) visible = false;
            } else {
                const double t = qq[e] / p[e];
                if (p[e] < 0.0) t0 = t > t0 ? t : t0;
                else t1 = t < t1 ? t : t1;
            }
        }
        if (!(t0 < t1)) visible = false;
        double ox1 = x1, oy1 = y1, oz1 = iz1, ox2 = x2, oy2 = y2, oz2 = iz2;
        if (t0 > 0.0) { ox1 = x1 + t0 * dx; oy1 = y1 + t0 * dy; oz1 = iz1 + t0 * (iz2 - iz1); flags |= kProjRect; }
        if (t1 < 1.0) { ox2 = x1 + t1 * dx; oy2 = y1 + t1 * dy; oz2 = iz1 + t1 * (iz2 - iz1); flags |= kProjRect; }
        r = ProjRecord{(float)ox1, (float)oy1, (float)ox2, (float)oy2, (float)oz1, (float)oz2, a.line[s], s | flags};
        // 5. a record that is not finite in float32 (a degenerate K, an overflow) is not visible: NaN passes every
        // comparison above, and stage 2 reads finite records only
        if (!(isfinite(r.x1) && isfinite(r.y1) && isfinite(r.x2) && isfinite(r.y2) && isfinite(r.iz1) && isfinite(r.iz2))) visible = false;
    }
    a.vis[at] = visible ? 1u : 0u;
    if (visible) a.rec[at] = r;
}

__global__ __launch_bounds__(kProjBlock) void k_project_compact(ProjArgs a) {
    const size_t n = (size_t)a.n_cams * a.n_seg;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = a.vis[i];
    if (a.vis[i + 1] != at) a.out[at] = a.rec[i];
    // bounds[c] = first visible record of camera c, bounds[n_cams] = their number
    if (i % a.n_seg == 0) a.bounds[i / a.n_seg] = at;
    if (i == n - 1) a.bounds[a.n_cams] = a.vis[n];
}

// the two ends of a record along its major axis, a = the end with the smaller major coordinate
struct RasterSeg { double am, an, aiz, bm, bn, biz; bool xmajor, draws; };
__device__ __forceinline__ RasterSeg raster_seg(const ProjRecord& r) {
    const double x1 = r.x1, y1 = r.y1, x2 = r.x2, y2 = r.y2, z1 = r.iz1, z2 = r.iz2;
    const double dx = x2 - x1, dy = y2 - y1;
    RasterSeg s;
    s.xmajor = fabs(dx) >= fabs(dy);
    s.draws = !(dx == 0.0 && dy == 0.0);
    const double m1 = s.xmajor ? x1 : y1, n1 = s.xmajor ? y1 : x1, m2 = s.xmajor ? x2 : y2, n2 = s.xmajor ? y2 : x2;
    const bool first = m1 <= m2;
    s.am = first ? m1 : m2; s.an = first ? n1 : n2; s.aiz = first ? z1 : z2;
    s.bm = first ? m2 : m1; s.bn = first ? n2 : n1; s.biz = first ? z2 : z1;
    return s;
}
// the integer major coordinates of a record inside the image: [m0, m0 + count)
__device__ __forceinline__ uint32_t raster_range(const RasterSeg& s, const MapCam& c, double& m0) {
    if (!s.draws) return 0;
    const double size = (double)(s.xmajor ? c.width : c.height);
    m0 = fmax(ceil(s.am), 0.0);
    const double m1 = fmin(floor(s.bm), size - 1.0);
    if (!(m0 <= m1)) return 0;
    return (uint32_t)(m1 - m0) + 1u;
}
// the camera of record r: the last one whose first record is <= r
__device__ __forceinline__ uint32_t cam_of_record(const MapCam* cams, uint32_t n_cams, uint32_t r) {
    uint32_t lo = 0, hi = n_cams;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cams[mid].rec0 <= r) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kProjBlock) void k_raster_count(MapArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rec) return;
    const MapCam c = a.cams[cam_of_record(a.cams, a.n_cams, r)];
    double m0;
    a.steps[r] = raster_range(raster_seg(a.rec[r]), c, m0);
}

__global__ __launch_bounds__(kProjBlock) void k_raster_lines(MapArgs a) {
    const uint32_t total = a.steps[a.n_rec];
    const int half = (int)(a.thickness >> 1);
    for (uint64_t it = blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t item = (uint32_t)it;
        // the record whose steps hold this item: the last r with steps[r] <= item (records without steps share their
        // successor's offset and are passed over)
        uint32_t lo = 0, hi = a.n_rec;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.steps[mid] <= item) lo = mid; else hi = mid;
        }
        const ProjRecord rec = a.rec[lo];
        const MapCam c = a.cams[cam_of_record(a.cams, a.n_cams, lo)];
        const RasterSeg s = raster_seg(rec);
        double m0;
        const uint32_t count = raster_range(s, c, m0);
        const uint32_t k = item - a.steps[lo];
        if (k >= count) continue;                       // (cannot happen: the counts came from the same arithmetic)
        const double m = m0 + (double)k;
        const double t = (m - s.am) / (s.bm - s.am);
        const double nd = floor(s.an + t * (s.bn - s.an) + 0.5);
        const float iz = (float)(s.aiz + t * (s.biz - s.aiz));
        const double nsize = (double)(s.xmajor ? c.height : c.width);
        if (!(nd >= -1073741824.0 && nd <= 1073741824.0)) continue;
        const int n0 = (int)nd, mi = (int)m;
        const unsigned long long key = ((unsigned long long)__float_as_uint(iz) << 32) | (0xFFFFFFFFu - rec.line);
        for (int o = -half; o <= half; ++o) {
            const int n = n0 + o;
            if (n < 0 || (double)n > nsize - 1.0) continue;
            const uint32_t x = s.xmajor ? (uint32_t)mi : (uint32_t)n, y = s.xmajor ? (uint32_t)n : (uint32_t)mi;
            // (the result is not used: a no-return global_atomic_umax_x2)
            (void)__hip_atomic_fetch_max(&a.keys[c.pix0 + (uint64_t)y * c.width + x], key, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ __launch_bounds__(kProjBlock) void k_map_decode(MapArgs a) {
    const MapCam c = a.cams[blockIdx.y];
    const uint64_t n = (uint64_t)c.width * c.height;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = a.keys[c.pix0 + i];
        a.line_id[c.pix0 + i] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
        a.inv_depth[c.pix0 + i] = key ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
    }
}

__global__ __launch_bounds__(kProjBlock) void k_overlay(MapArgs a) {
    const MapCam c = a.cams[blockIdx.y];
    const uint64_t n = (uint64_t)c.width * c.height;
    const uint32_t al = a.alpha;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t y = (uint32_t)(i / c.width), x = (uint32_t)(i - (uint64_t)y * c.width);
        const uint8_t* src = a.img + c.img_off + (uint64_t)y * c.img_stride + (uint64_t)x * c.img_channels;
        uint32_t px[3];
        if (c.img_channels == 3) { px[0] = src[0]; px[1] = src[1]; px[2] = src[2]; }
        else { px[0] = src[0]; px[1] = px[0]; px[2] = px[0]; }
        const int32_t id = a.line_id[c.pix0 + i];
        if (id >= 0) {
            uint32_t col[3];
            if (a.colors && (uint32_t)id < a.n_lines) {
                col[0] = a.colors[3 * (size_t)id]; col[1] = a.colors[3 * (size_t)id + 1]; col[2] = a.colors[3 * (size_t)id + 2];
            } else {
                const uint32_t h = ((uint32_t)id + 1u) * 0x9E3779B1u;
                col[0] = 64u + ((h >> 24) & 255u) * 3u / 4u;
                col[1] = 64u + ((h >> 16) & 255u) * 3u / 4u;
                col[2] = 64u + ((h >> 8) & 255u) * 3u / 4u;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) px[k] = (al * col[k] + (255u - al) * px[k] + 127u) / 255u;
        }
        uint8_t* dst = a.rgb + c.rgb_off + 3 * i;
        dst[0] = (uint8_t)px[0]; dst[1] = (uint8_t)px[1]; dst[2] = (uint8_t)px[2];
    }
}

// blocks of a per-pixel kernel along x: enough for the largest camera, capped (the kernels stride)
uint32_t pixel_blocks(uint32_t max_pix) { return std::min(2048u, std::max(1u, (max_pix + kProjBlock - 1) / kProjBlock)); }

}  // namespace

hipError_t launch_project_lines(const ProjArgs& a, hipStream_t st) {
    if (!a.n_cams || !a.n_seg) return hipSuccess;
    hipLaunchKernelGGL(k_project_lines, dim3((a.n_seg + kProjBlock - 1) / kProjBlock, a.n_cams), dim3(kProjBlock), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_project_compact(const ProjArgs& a, hipStream_t st) {
    const size_t n = (size_t)a.n_cams * a.n_seg;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_project_compact, dim3((uint32_t)((n + kProjBlock - 1) / kProjBlock)), dim3(kProjBlock), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_raster_count(const MapArgs& a, hipStream_t st) {
    if (!a.n_rec) return hipSuccess;
    hipLaunchKernelGGL(k_raster_count, dim3((a.n_rec + kProjBlock - 1) / kProjBlock), dim3(kProjBlock), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_raster_lines(const MapArgs& a, uint32_t blocks, hipStream_t st) {
    if (!a.n_rec || !blocks) return hipSuccess;
    hipLaunchKernelGGL(k_raster_lines, dim3(blocks), dim3(kProjBlock), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_map_decode(const MapArgs& a, hipStream_t st) {
    if (!a.n_cams || !a.n_pix) return hipSuccess;
    hipLaunchKernelGGL(k_map_decode, dim3(pixel_blocks(a.max_pix), a.n_cams), dim3(kProjBlock), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_overlay(const MapArgs& a, hipStream_t st) {
    if (!a.n_cams || !a.n_pix) return hipSuccess;
    hipLaunchKernelGGL(k_overlay, dim3(pixel_blocks(a.max_pix), a.n_cams), dim3(kProjBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d
