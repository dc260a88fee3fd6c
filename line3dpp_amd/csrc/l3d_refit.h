// l3d_refit.h -- the 3D lines refit against cameras and their 2D segments, shared by the host stage
// (l3d_refit.hip) and the kernels (k_refit.hip): the records of the two new kernels, the span of a 2D end point along a
// carrier as one function for the device and the host hook, and the sweep of stage 9.  Behind them the host pieces that
// the joint bundle of §29 runs too: the observation list, the lines cut anew, the skeleton of a result.
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

// ---- host (l3d_refit.hip): what the refit shares with the joint bundle of DESIGN §29 (l3d_bundle.hip) ----
struct ProjWork; struct KernelTimer;             // l3d_ctx.h
// a call's model, its cameras and every camera's 2D segments (of §27's entries too)
struct RefitJob {
    uint32_t n_model; const double* segs; const uint32_t* line;
    uint32_t n_cams; const l3d_camera* cams; const uint32_t* n_seg; const float* const* seg;
};
// What stages 1 to 3 leave behind.  On the device (offsets into w.d, kept until the caller overwrites them): the model as
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
// Stages 1 to 3.  Arguments already checked; model, cameras and 2D segments non-empty.  `who` opens the messages ("refit",
// "bundle"); ms_assoc / ms_list (may be null): the time of the launches of stage 2 and of stage 3.
int refit_observe(ProjWork& w, hipStream_t st, const RefitJob& J, double max_distance, double min_cos2, double min_overlap, double near_plane,
                  uint32_t use_ambiguous, uint32_t n_lines, size_t tail_bytes, const char* who, float* ms_assoc, float* ms_list,
                  RefitObserved& O);
// The observation records in CSR order, {camera, segment in its camera, line, 0, 0, 0}, and the list cut into cells --
// (line, camera) pairs: within a line the observations come in ascending flat index, so a camera's are neighbours.  A
// line's views are its cells.
struct RefitCells { std::vector<uint32_t> cell_off, cell_line, cell_cam, line_cell_off; };   // [n_cells + 1], [n_cells] x 2, [n_lines + 1]
void refit_list_observations(const RefitObserved& O, uint32_t n_lines, std::vector<l3d_refit_observation>& obs, RefitCells& cells);

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

// Stages 8 and 9 for the lines of `cuts`, in their order.  The caller has enqueued the uploads of the carriers (and of the
// LoCams, where they are new) that oa names; here k_refit_spans runs under the caller's timer, the spans come down to
// `down` (oa.n_obs of them, the pinned place of oa.spans) and, after one synchronisation, every line's observations take
// their valid / s_lo / s_hi, refit_sweep cuts the line and its pieces (M + s u) + c are appended.  A line without a
// carrier is unusable: its observations keep valid = 0, s_lo = s_hi = 0 and it gets no sweep.
struct RefitPieces {                             // of the lines cut anew: line l's n[l] pieces are xyz[6 * off[l] ..], 6 doubles each
    std::vector<double> xyz;
    std::vector<uint32_t> off, n;                // [n_lines] (0, 0 for a line that was not cut or kept no piece)
    explicit RefitPieces(uint32_t n_lines) : off(n_lines, 0), n(n_lines, 0) {}
};
struct RefitCut {
    uint32_t line, obs0, span0, n;               // its n observations are obs[obs0 ..], their spans down[span0 ..]
    const double* carrier;                       // M, u about the centre; null: unusable
};
int refit_cut_lines(hipStream_t st, KernelTimer& timer, const RefitObsArgs& oa, RefitSpan* down, const std::vector<RefitCut>& cuts,
                    uint32_t n_cams, uint32_t visibility, double min_length, const double c[3], const char* who,
                    std::vector<l3d_refit_observation>& obs, RefitPieces& pieces);

// What the results of §28 and §29 share: the output model, the observations and the associations, and per line -- under
// the same names in l3d_refit_line and l3d_bundle_line -- status, n_observations, n_views, n_pieces, P1, P2
struct RefitModel {
    std::vector<double> segs;                    // the output model
    std::vector<uint32_t> seg_line;
    std::vector<uint32_t> seg_off;               // [n_lines + 1] where a line's segments begin in it
    std::vector<l3d_refit_observation> obs;      // line after line
    std::vector<uint32_t> obs_off;               // [n_lines + 1]
    std::vector<l3d_association> assoc;
};
template <class Line, class Summary> struct LinesResult : RefitModel {
    std::vector<Line> lines;
    Summary sum{};
};

// every line as given: `empty` without a segment, else `given` with its carrier
template <class Line, class Summary>
void lines_as_given(const RefitJob& J, const ModelLines& ml, uint32_t empty, uint32_t given, LinesResult<Line, Summary>& R) {
    R.lines.assign(ml.n_lines, Line{});
    for (uint32_t l = 0; l < ml.n_lines; ++l) {
        Line& L = R.lines[l];
        if (ml.off[l] == ml.off[l + 1]) { L.status = empty; continue; }
        L.status = given;
        const double* a = J.segs + 6 * (size_t)ml.seg[ml.off[l]];
        const double* b = J.segs + 6 * (size_t)ml.seg[ml.off[l + 1] - 1] + 3;
        for (int k = 0; k < 3; ++k) { L.P1[k] = a[k]; L.P2[k] = b[k]; }
    }
    R.obs_off.assign((size_t)ml.n_lines + 1, 0);
}

// Stage 10: the output model and the summary's counts from the lines' statuses: the pieces of a line that was cut `anew`,
// every other line's segments as given in input order
template <class Line, class Summary>
void assemble(const RefitJob& J, const ModelLines& ml, const RefitPieces& pieces, uint32_t anew, LinesResult<Line, Summary>& R) {
    R.segs.clear(); R.seg_line.clear();
    R.seg_off.assign((size_t)ml.n_lines + 1, 0);
    R.sum.n_lines = ml.n_lines;
    R.sum.n_segments_before = J.n_model;
    for (uint32_t l = 0; l < ml.n_lines; ++l) {
        Line& L = R.lines[l];
        if (L.status == anew) {
            const auto first = pieces.xyz.begin() + 6 * (size_t)pieces.off[l];
            R.segs.insert(R.segs.end(), first, first + 6 * (size_t)pieces.n[l]);
            R.seg_line.insert(R.seg_line.end(), pieces.n[l], l);
        } else {
            for (uint32_t k = ml.off[l]; k < ml.off[l + 1]; ++k) {
                R.segs.insert(R.segs.end(), J.segs + 6 * (size_t)ml.seg[k], J.segs + 6 * (size_t)ml.seg[k] + 6);
                R.seg_line.push_back(l);
            }
        }
        R.seg_off[l + 1] = (uint32_t)R.seg_line.size();
        L.n_pieces = R.seg_off[l + 1] - R.seg_off[l];
        ++R.sum.n_status[L.status];
    }
    R.sum.n_segments_after = R.seg_line.size();
}

// the lines of a result that were cut anew, with their carriers: what context_take_lines (l3d_ctx.h) puts into a context
struct NewLine { uint32_t line; const double *P1, *P2; };
template <class Line> std::vector<NewLine> lines_cut_anew(const std::vector<Line>& lines, uint32_t anew) {
    std::vector<NewLine> out;
    for (uint32_t l = 0; l < lines.size(); ++l)
        if (lines[l].status == anew) out.push_back(NewLine{l, lines[l].P1, lines[l].P2});
    return out;
}

}  // namespace l3d
