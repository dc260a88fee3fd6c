// l3d_refit.h -- the 3D lines refit against cameras and their 2D segments, shared by the host stage
// (l3d_refit.hip) and the kernels (k_refit.hip): the records of the two new kernels, the span of a 2D end point along a
// carrier as one function for the device and the host hook, and the sweep of stage 9.
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/l3dpp_hip.h"
#include "l3d_kernels.h"
#include "l3d_lineopt.h"

namespace l3d {

// the span of one observation along its line's carrier M' + s u
struct RefitSpan { double lo, hi; uint32_t valid, pad; };
static_assert(sizeof(RefitSpan) == 24 && sizeof(LoObs) == 56 && sizeof(LoCam) == 128 && sizeof(LoOut) == 56, "refit record layout");

// Stage 8 for one end point (x, y) of a camera (R, C = Q', fx, fy, px, py): the parameter s at which the carrier M + s u
// comes closest to the ray of the pixel; project2DsegmentOnto3Dline (line3D.cc:2221-2266) without normalising the ray.
// fp64 in the order DESIGN §28 writes it.  false: the ray and the carrier are parallel, or the carrier is a point.
__host__ __device__ inline bool refit_point(const LoCam& cam, double x, double y, const double M[3], const double u[3], double& s) {
    const double xn = (x - cam.px) / cam.fx;
    const double yn = (y - cam.py) / cam.fy;
    double v[3], w[3];
    for (int i = 0; i < 3; ++i) {
        v[i] = (cam.R[i] * xn + cam.R[3 + i] * yn) + cam.R[6 + i];
        w[i] = M[i] - cam.C[i];
    }
    const double a = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    const double b = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
    const double cc = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double d = (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2];
    const double e = (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2];
    const double den = a * cc - b * b;
    s = 0.0;
    if (!(den > 1e-12 * (a * cc))) return false;
    s = (b * e - cc * d) / den;
    return true;
}

// ... for a 2D segment: [min(s1, s2), max(s1, s2)], valid iff both end points are and both s are finite
__host__ __device__ inline RefitSpan refit_span(const LoCam& cam, double x1, double y1, double x2, double y2, const double M[3],
                                                const double u[3]) {
    double s1, s2;
    const bool ok1 = refit_point(cam, x1, y1, M, u, s1), ok2 = refit_point(cam, x2, y2, M, u, s2);
    RefitSpan r{0.0, 0.0, 0u, 0u};
    const double big = 1.7976931348623157e308;     // |s| <= big: finite (a NaN compares false)
    if (ok1 && ok2 && fabs(s1) <= big && fabs(s2) <= big) {
        r.lo = s1 < s2 ? s1 : s2;
        r.hi = s1 < s2 ? s2 : s1;
        r.valid = 1u;
    }
    return r;
}

// Stage 9: the sweep of the final segments with the visibility as a parameter.  Events in ascending s, at equal s the
// openings before the closings, then in observation order; the count is over the distinct cameras with an open span; a
// piece opens where the count reaches `visibility` and closes where it falls below; kept iff s_end > s_start and
// (s_end - s_start) * u_norm >= min_length.  cam_open: one zeroed counter per camera, zero again on return.
inline void refit_sweep(uint32_t n, const double* lo, const double* hi, const uint32_t* cam, uint32_t visibility, double min_length,
                        double u_norm, std::vector<uint32_t>& cam_open, std::vector<double>& pieces) {
    struct Event { double s; uint32_t closing, obs; };
    std::vector<Event> ev;
    ev.reserve(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) { ev.push_back(Event{lo[i], 0u, i}); ev.push_back(Event{hi[i], 1u, i}); }
    std::sort(ev.begin(), ev.end(), [](const Event& a, const Event& b) {
        if (a.s != b.s) return a.s < b.s;
        if (a.closing != b.closing) return a.closing < b.closing;
        return a.obs < b.obs;
    });
    uint32_t count = 0;
    double start = 0.0;
    for (const Event& e : ev) {
        uint32_t& open = cam_open[cam[e.obs]];
        if (!e.closing) {
            if (open++ == 0 && ++count == visibility) start = e.s;
        } else if (--open == 0 && count-- == visibility) {
            if (e.s > start && (e.s - start) * u_norm >= min_length) { pieces.push_back(start); pieces.push_back(e.s); }
        }
    }
}

// launchers (k_refit.hip)
struct RefitCompactArgs {
    const AssocOut* assoc;     // [n_seg] the association's records of every 2D segment, camera after camera
    uint32_t n_seg, use_ambiguous;
    uint32_t* flag;            // [n_seg + 1] k_refit_flag: 1 for an observation; then its exclusive scan, in place
    uint32_t* obs_seg;         // [n_seg] k_refit_compact: the flat 2D segment of observation j
    uint32_t* obs_line;        // [n_seg] ... and its line
};
hipError_t launch_refit_flag(const RefitCompactArgs& a, hipStream_t st);
hipError_t launch_refit_compact(const RefitCompactArgs& a, hipStream_t st);
struct RefitObsArgs {
    uint32_t n_obs;            // observations of the solved lines, in CSR order
    const uint32_t* perm;      // [n_obs] the observation (its rank in the compaction) at CSR position r
    const uint32_t* obs_seg;   // the compaction's
    const float4* segs;        // [2D segments of the call]
    const uint32_t* seg_begin; uint32_t n_cams;
    LoObs* obs;                // [n_obs] k_refit_obs
    const LoCam* cams;         // [n_cams]
    const uint32_t* res_off;   // [n_lines + 1] CSR of the solved lines
    uint32_t n_lines;
    const double* carrier;     // [n_lines x 6] M', u of the written-back carriers
    RefitSpan* spans;          // [n_obs] k_refit_spans
};
hipError_t launch_refit_obs(const RefitObsArgs& a, hipStream_t st);
hipError_t launch_refit_spans(const RefitObsArgs& a, hipStream_t st);

// ---- host (l3d_refit.hip): stages 1 to 3, shared with the joint bundle of DESIGN §29 (l3d_bundle.hip) ----
struct ProjWork;               // l3d_ctx.h
struct RefitJob {
    uint32_t n_model; const double* segs; const uint32_t* line;
    uint32_t n_cams; const l3d_camera* cams; const uint32_t* n_seg; const float* const* seg;
};
// What the stages leave behind.  On the device (offsets into w.d, kept until the caller overwrites them): the model as
// given at o_P, its line indices at o_line, every camera's float4 segments at o_segs, their first indices [n_cams + 1]
// at o_begin, the flat 2D segment of every observation at o_oseg; the caller's own tables go at keep_end and behind, up
// to `bound` = up256(keep_end) + tail_bytes, which w.h and w.d hold.
struct RefitObserved {
    std::vector<uint32_t> seg_begin;             // [n_cams + 1]
    uint32_t S = 0, n_obs = 0;                   // 2D segments, observations
    size_t o_P = 0, o_line = 0, o_segs = 0, o_begin = 0, o_oseg = 0, keep_end = 0, bound = 0;
    std::vector<l3d_association> assoc;          // [S] as they are handed out
    uint64_t n_ambiguous_left_out = 0;
    std::vector<uint32_t> oseg, oline;           // [n_obs] in flat order: the flat 2D segment, the line
    std::vector<uint32_t> obs_off, csr;          // [n_lines + 1]; [n_obs] the observation at a CSR position
};
// Arguments already checked; model, cameras and 2D segments non-empty.  `who` opens the messages ("refit", "bundle");
// ms_assoc / ms_list (may be null): the time of the launches of stage 2 and of stage 3.
int refit_observe(ProjWork& w, hipStream_t st, const RefitJob& J, double max_distance, double min_cos2, double min_overlap, double near_plane,
                  uint32_t use_ambiguous, uint32_t n_lines, size_t tail_bytes, const char* who, float* ms_assoc, float* ms_list,
                  RefitObserved& O);

// the near plane, the cameras' sides and entries as stage 1 checks them, and the form of K that LoCam can hold
int check_refit_cameras(uint32_t n_cams, const l3d_camera* cams, double near_plane);
// midpoint c and diagonal of the bounding box of the n > 0 segments' end points (§23's)
void refit_bounding_box(size_t n, const double* segs, double c[3], double& diag);
// LoCam of a camera about the centre c
LoCam refit_lo_camera(const l3d_camera& cam, const double c[3]);
// The model's side of a call: the lines' segments in input order (a stable counting sort by line index)
struct ModelLines {
    uint32_t n_lines = 0;
    std::vector<uint32_t> off, seg;              // [n_lines + 1], [n_model]: line l's segments are seg[off[l] .. off[l + 1])
    void build(uint32_t n, const uint32_t* line) {
        for (uint32_t i = 0; i < n; ++i) n_lines = std::max(n_lines, line[i] + 1);
        off.assign((size_t)n_lines + 1, 0); seg.resize(n);
        for (uint32_t i = 0; i < n; ++i) ++off[line[i] + 1];
        for (uint32_t l = 0; l < n_lines; ++l) off[l + 1] += off[l];
        std::vector<uint32_t> at(off.begin(), off.end() - 1);
        for (uint32_t i = 0; i < n; ++i) seg[at[line[i]]++] = i;
    }
};

// the checks of the entries of §28 and §29 behind their parameters (messages and order as §28 lists them)
int refit_check_job(const RefitJob& J, double near_plane, double c[3], ModelLines& ml, uint64_t& n_seg);

}  // namespace l3d
