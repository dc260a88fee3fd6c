// k_pose.hip -- the device side of the refinement of camera poses against the 3D line model (host side:
// l3d_pose.hip).  No counterpart in the reference.  The arithmetic is the contract of §27, fp64 in the order written there
// (the library is built with -ffp-contract=off), so that tests/pose_model.py follows it operation for operation.  No
// atomics, no inline assembly.
//   k_pose_bounds   one lane per camera: rec0 / n_rec of the association's camera table from the bounds the compaction of
//                   stage 1 (k_project.hip) left on the device, so that the records never pass through the host.
//   k_pose_normal   a tile of kAssocTile = 256 consecutive 2D segments of one camera per workgroup of four waves, one lane
//                   per segment; the camera is found through the tile table as in k_associate, its K^-T entries, R and t
//                   are uniform (scalar loads).  A matched lane reads the two end points of its 3D segment from the model
//                   in fp64 and forms its term of kPoseTerms = 29 doubles in registers -- H (21), b (6), cost, count:
//                   term(P) + term(Q) --, every other lane holds 29 times +0.0.  The tile's sum is the tree of
//                   k_align_normal: inside a wave v[i] = v[i] + v[i + stride] for stride 32 .. 1 by __shfl_down, the four
//                   wave sums through LDS as (W0 + W1) + (W2 + W3).  The host adds a camera's tiles in ascending order.
#include "l3d_kernels.h"

namespace l3d {
namespace {

__global__ __launch_bounds__(64) void k_pose_bounds(AssocCam* cams, uint32_t n_cams, const uint32_t* bounds) {
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_cams) return;
    const uint32_t b0 = bounds[c];
    cams[c].rec0 = b0;
    cams[c].n_rec = bounds[c + 1] - b0;
}

// K^-T v for an upper-triangular K with K22 = 1: M = (m00, m10, m11, m20, m21)
__device__ __forceinline__ void pose_line(const double* M, const double* v, double* l) {
    l[0] = M[0] * v[0];
    l[1] = M[1] * v[0] + M[2] * v[1];
    l[2] = (M[3] * v[0] + M[4] * v[1]) + v[2];
}

// The term of one 2D end point (x, y): image line lam of norm nu, columns dl with B_i = (lam0 dl_i0 + lam1 dl_i1) / nu^3.
// kFirst: v = term, else v = v + term.
template <bool kFirst>
__device__ __forceinline__ void pose_point(double x, double y, const double* lam, double nu, const double (*dl)[3], const double* B, double* v) {
    const double u = (lam[0] * x + lam[1] * y) + lam[2];
    const double r = u / nu;
    double J[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) J[i] = ((dl[i][0] * x + dl[i][1] * y) + dl[i][2]) / nu - u * B[i];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++k) {
            const double h = J[i] * J[j];
            v[k] = kFirst ? h : v[k] + h;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double b = J[i] * r;
        v[21 + i] = kFirst ? b : v[21 + i] + b;
    }
    const double cost = r * r;
    v[27] = kFirst ? cost : v[27] + cost;
}

__global__ __launch_bounds__(kAssocTile) void k_pose_normal(PoseNormalArgs a) {
    __shared__ double s_w[4][kPoseTerms];
    // the camera of this tile, as in k_associate: the last one whose first tile is <= blockIdx.x
    uint32_t lo = 0, hi = a.n_cams;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.cams[mid].tile0 <= blockIdx.x) lo = mid; else hi = mid;
    }
    const AssocCam cam = a.cams[lo];
    const PoseCam& pc = a.pose[lo];
    const uint32_t s = (blockIdx.x - cam.tile0) * kAssocTile + threadIdx.x;      // segment of this lane in its camera
    double v[kPoseTerms];
#pragma unroll
    for (uint32_t k = 0; k < kPoseTerms; ++k) v[k] = 0.0;
    if (s < cam.n_seg) {
        const AssocOut o = a.assoc[(size_t)cam.seg0 + s];
        if (o.record >= 0 && o.segment < a.n_model) {
            const float4 sg = a.segs[(size_t)cam.seg0 + s];
            const double* X = a.model + 6 * (size_t)o.segment;
            const d3 t{pc.t[0], pc.t[1], pc.t[2]};
            const d3 Y1 = mul33(pc.R, d3{X[0], X[1], X[2]}) + t;
            const d3 Y2 = mul33(pc.R, d3{X[3], X[4], X[5]}) + t;
            const d3 Nc = cross(Y1, Y2), Dc = Y2 - Y1;
            const double N[3] = {Nc.x, Nc.y, Nc.z}, D[3] = {Dc.x, Dc.y, Dc.z};
            double lam[3];
            pose_line(pc.M, N, lam);
            const double nu = sqrt(lam[0] * lam[0] + lam[1] * lam[1]);
            if (nu > 0.0 && isfinite(nu)) {
                // the columns: e_i x N (rotation), e_i x D (translation)
                const double dN[6][3] = {{0.0, -N[2], N[1]}, {N[2], 0.0, -N[0]}, {-N[1], N[0], 0.0},
                                         {0.0, -D[2], D[1]}, {D[2], 0.0, -D[0]}, {-D[1], D[0], 0.0}};
                const double nu3 = (nu * nu) * nu;
                double dl[6][3], B[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    pose_line(pc.M, dN[i], dl[i]);
                    B[i] = (lam[0] * dl[i][0] + lam[1] * dl[i][1]) / nu3;
                }
                pose_point<true>((double)sg.x, (double)sg.y, lam, nu, dl, B, v);
                pose_point<false>((double)sg.z, (double)sg.w, lam, nu, dl, B, v);
                v[28] = 1.0;
            }
        }
    }
    // inside the wave: stride 32, 16, 8, 4, 2, 1 (a lane whose partner lies past the wave gets its own value back; only
    // the lanes below the stride are read afterwards)
#pragma unroll
    for (uint32_t stride = 32; stride >= 1; stride >>= 1)
#pragma unroll
        for (uint32_t k = 0; k < kPoseTerms; ++k) v[k] = v[k] + __shfl_down(v[k], stride);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0)
#pragma unroll
        for (uint32_t k = 0; k < kPoseTerms; ++k) s_w[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < kPoseTerms) {
        const uint32_t k = threadIdx.x;
        a.tiles[(size_t)blockIdx.x * kPoseTerms + k] = (s_w[0][k] + s_w[1][k]) + (s_w[2][k] + s_w[3][k]);
    }
}

}  // namespace

hipError_t launch_pose_bounds(AssocCam* cams, uint32_t n_cams, const uint32_t* bounds, hipStream_t st) {
    if (!n_cams) return hipSuccess;
    hipLaunchKernelGGL(k_pose_bounds, dim3((n_cams + 63) / 64), dim3(64), 0, st, cams, n_cams, bounds);
    return hipGetLastError();
}

hipError_t launch_pose_normal(const PoseNormalArgs& a, uint32_t n_tiles, hipStream_t st) {
    if (!a.n_cams || !n_tiles) return hipSuccess;
    hipLaunchKernelGGL(k_pose_normal, dim3(n_tiles), dim3(kAssocTile), 0, st, a);
    return hipGetLastError();
}

}  // namespace l3d
