// l3d_pose.hip -- host side of the refinement of camera poses against the 3D line model (kernels: k_pose.hip
// and, unchanged, k_project.hip's stage 1, k_scan.hip and k_associate.hip): the stateless l3d_refine_cameras and
// l3d_refine_view_cameras on the context's lines and the added views' own cameras and segments, on the context's stream
// and the work space of the projection stages.
//
// The model is uploaded once (about its centre for the iterations, as given for the delivery pass), every camera's 2D
// segments once.  Cameras are taken in GROUPS under the budget of the projection stages; every camera is refined from its
// own records and segments alone, so the grouping changes nothing but the number of launches.  Per iteration the active
// cameras' tables go up, stage 1 projects the model into them, k_pose_bounds hands the compaction's bounds to the
// association's camera table on the device, launch_associate runs once per gate in force, k_pose_normal sums the normal
// equations per tile of 256 segments; 29 doubles per tile come down, the host adds a camera's tiles in ascending order,
// solves the 6 x 6 system by the Cholesky factorisation the alignment uses and updates the pose.  The records and the
// associations never leave the device but for the delivery pass' associations.  Everything the host computes is fp64 in
// the order DESIGN §27 writes it, so that tests/pose_model.py reproduces a whole run bit for bit.
#include <atomic>

#include "l3d_ctx.h"
#include "l3d_pose.h"
#include "l3d_refit.h"

namespace l3d {
// test hooks (l3d_debug_counter): iterations run (summed over the cameras) and launches of k_pose_normal so far, and the
// kernel time of the last timed call (context at timing level 2)
std::atomic<uint64_t> g_pose_iterations{0}, g_pose_normal_launches{0}, g_pose_kernel_ns{0};
}  // namespace l3d

using namespace l3d;

namespace {

constexpr uint32_t kPoseMaxGroup = 4096;        // cameras per group at most
static_assert(sizeof(l3d_pose_params) == 72 && sizeof(l3d_pose_summary) == 88 && sizeof(l3d_pose_iteration) == 392, "pose structs");
static_assert(sizeof(AssocOut) == sizeof(l3d_association), "association layout");

int check_params(const l3d_pose_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_thresholds(p->max_distance, p->min_cos2, p->min_overlap)) return rc;
    if (!(p->start_distance == 0.0 || (std::isfinite(p->start_distance) && p->start_distance >= p->max_distance)))
        return fail(L3D_ERR_ARG, "start_distance must be 0, or finite and not below max_distance");
    if (!(p->stall_tolerance > 0.0) || !std::isfinite(p->stall_tolerance)) return fail(L3D_ERR_ARG, "stall_tolerance must be finite and greater than 0");
    if (!(p->step_tolerance > 0.0) || !std::isfinite(p->step_tolerance)) return fail(L3D_ERR_ARG, "step_tolerance must be finite and greater than 0");
    if (p->max_iterations < 1 || p->max_iterations > 256) return fail(L3D_ERR_ARG, "max_iterations must lie in [1, 256]");
    if (p->min_matches < 6) return fail(L3D_ERR_ARG, "min_matches must be at least 6");
    if (p->reserved[0] || p->reserved[1]) return fail(L3D_ERR_ARG, "reserved must be 0");
    return L3D_OK;
}

// one camera's state: the delta (q, tau) on the input pose and t'_in = t_in + R_in c (l3d_pose.h), the gate and how far
// it has come
struct CamState : PoseDelta {
    double gate = 0.0, last_step = 0.0;
    uint32_t status = L3D_POSE_TOO_FEW, iterations = 0;
    bool done = true;
};

// H delta = -b from the 29 sums (n = 6), by the alignment's Cholesky.  false: a pivot that is not finite and > 0
bool solve_normal(const double* s, double delta[6]) {
    static const int kRow[6] = {0, 6, 11, 15, 18, 20};   // where row i of the upper triangle begins
    double H[36] = {}, rhs[6], work[kCholeskyWork];
    for (int i = 0; i < 6; ++i) {
        for (int j = i; j < 6; ++j) H[i * 6 + j] = s[kRow[i] + (j - i)];
        rhs[i] = -s[21 + i];
    }
    return cholesky_solve(6, H, rhs, delta, work);
}

double step_of(const double delta[6], double diag) {
    double s = 0.0;
    for (int i = 0; i < 3; ++i) {
        s = std::max(s, std::fabs(delta[i]));
        s = std::max(s, std::fabs(delta[3 + i]) / diag);
    }
    return s;
}

using Job = RefitJob;
struct Outputs { l3d_camera* cams; l3d_pose_summary* summaries; l3d_association* assoc; l3d_pose_iteration* trace; };

// the offsets of a group's tables behind the model, and where the host's part and the whole end
struct GroupLayout { size_t pcam, acam, ncam, pose, segs, tiles, assoc, bounds, host_end, vis, rec, out, end; };
GroupLayout group_layout(size_t model_end, uint32_t g, uint64_t n_seg, uint64_t n_tiles, uint32_t n_model) {
    Layout lay;
    lay.at = model_end;
    GroupLayout L;
    const size_t n = (size_t)g * n_model;
    L.pcam = lay.take(sizeof(ProjCam) * g); L.acam = lay.take(sizeof(AssocCam) * g); L.ncam = lay.take(sizeof(AssocCam) * g);
    L.pose = lay.take(sizeof(PoseCam) * g);
    L.segs = lay.take(16 * (size_t)n_seg); L.tiles = lay.take(8 * kPoseTerms * (size_t)n_tiles); L.assoc = lay.take(24 * (size_t)n_seg);
    L.bounds = lay.take(4 * ((size_t)g + 1)); L.host_end = lay.at;
    L.vis = lay.take(4 * (n + 1)); L.rec = lay.take(32 * n); L.out = lay.take(32 * n); L.end = lay.at;
    return L;
}

// Arguments already checked, model and cameras non-empty, (c, diag) the box of the model.  Outputs are written only after
// everything has run.  kernel_ms (may be null): the time of every launch of the call, summed.
int refine_core(ProjWork& w, hipStream_t st, const Job& J, const l3d_pose_params& p, const double c[3], double diag, const Outputs& o,
                float* kernel_ms) {
    const uint32_t n_model = J.n_model;
    // the groups: cameras while their records, segments and sums fit the budget (one at least)
    struct Group { uint32_t c0, c1; uint64_t n_seg, n_tiles; };
    std::vector<Group> groups;
    for (uint32_t c0 = 0; c0 < J.n_cams;) {
        Group G{c0, c0, 0, 0};
        uint64_t bytes = 0;
        while (G.c1 < J.n_cams && G.c1 - c0 < kPoseMaxGroup) {
            const uint64_t tiles = ((uint64_t)J.n_seg[G.c1] + kAssocTile - 1) / kAssocTile;
            const uint64_t b = 68 * (uint64_t)n_model + 40 * (uint64_t)J.n_seg[G.c1] + 8 * kPoseTerms * tiles;
            if (G.c1 > c0 && (bytes + b > projection_budget(w) || (uint64_t)(G.c1 - c0 + 1) * n_model >= ((uint64_t)1 << 31) ||
                              G.n_tiles + tiles >= ((uint64_t)1 << 31)))
                break;
            bytes += b; G.n_seg += J.n_seg[G.c1]; G.n_tiles += tiles;
            ++G.c1;
        }
        groups.push_back(G);
        c0 = G.c1;
    }
    Layout lay;
    const size_t o_Pc = lay.take(48 * (size_t)n_model), o_P = lay.take(48 * (size_t)n_model), o_line = lay.take(4 * (size_t)n_model);
    const size_t model_end = lay.at;
    size_t host_bytes = model_end, total = model_end, scan_words = 0;
    for (const Group& G : groups) {
        const GroupLayout L = group_layout(model_end, G.c1 - G.c0, G.n_seg, G.n_tiles, n_model);
        host_bytes = std::max(host_bytes, L.host_end); total = std::max(total, L.end);
        scan_words = std::max(scan_words, scan_ws_words((size_t)(G.c1 - G.c0) * n_model, 4));
    }
    if (w.h.reserve(host_bytes) != hipSuccess || w.d.reserve(total) != hipSuccess || w.scan_ws.reserve_zeroed(scan_words, st) != hipSuccess)
        return fail(L3D_ERR_HIP, "pose refinement: allocation failed");
    char* h = w.h.p; char* d = w.d.p;
    KernelTimer timer(kernel_ms);
    if (!timer.ok()) return fail(L3D_ERR_HIP, "pose refinement: no event");
    // the model about its centre, the model as given, the line indices: one upload
    {
        double* Pc = (double*)(h + o_Pc);
        for (size_t i = 0; i < 6 * (size_t)n_model; ++i) Pc[i] = J.segs[i] - c[i % 3];
        std::memcpy(h + o_P, J.segs, 48 * (size_t)n_model);
        std::memcpy(h + o_line, J.line, 4 * (size_t)n_model);
    }
    hipError_t e = hipMemcpyAsync(d, h, model_end, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("pose refinement: ") + hipGetErrorString(e));

    std::vector<CamState> state(J.n_cams);
    std::vector<l3d_camera> out_cams(J.n_cams);
    std::vector<l3d_pose_summary> summaries(J.n_cams);
    std::vector<l3d_pose_iteration> trace(o.trace ? (size_t)J.n_cams * p.max_iterations : 0);
    uint64_t n_seg_total = 0;
    for (uint32_t k = 0; k < J.n_cams; ++k) n_seg_total += J.n_seg[k];
    std::vector<l3d_association> assoc(o.assoc ? (size_t)n_seg_total : 0);
    for (uint32_t k = 0; k < J.n_cams; ++k) {
        CamState& s = state[k];
        const d3 rc = mul33(J.cams[k].R, d3{c[0], c[1], c[2]});
        s.tin[0] = J.cams[k].t[0] + rc.x; s.tin[1] = J.cams[k].t[1] + rc.y; s.tin[2] = J.cams[k].t[2] + rc.z;
        s.gate = p.start_distance > p.max_distance ? p.start_distance : p.max_distance;
        s.done = J.n_seg[k] == 0;                   // a camera without segments: TOO_FEW, as given, no iteration
    }

    uint64_t seg_at = 0;
    std::vector<uint32_t> act;                      // the cameras of a pass, in the order of their tables
    std::vector<double> sums;                       // [cameras of the pass x kPoseTerms]
    for (const Group& G : groups) {
        const uint32_t g = G.c1 - G.c0;
        const GroupLayout L = group_layout(model_end, g, G.n_seg, G.n_tiles, n_model);
        std::vector<uint32_t> seg0(g);              // where a camera's segments begin among the group's
        {
            uint64_t at = 0;
            for (uint32_t k = 0; k < g; ++k) {
                seg0[k] = (uint32_t)at;
                if (J.n_seg[G.c0 + k]) std::memcpy(h + L.segs + 16 * (size_t)at, J.seg[G.c0 + k], 16 * (size_t)J.n_seg[G.c0 + k]);
                at += J.n_seg[G.c0 + k];
            }
        }
        if (G.n_seg) {
            e = hipMemcpyAsync(d + L.segs, h + L.segs, 16 * (size_t)G.n_seg, hipMemcpyHostToDevice, st);
            if (e != hipSuccess) break;
        }
        // steps 2-4 for the cameras in `act`, sorted so that equal gates are neighbours; final: the delivery pass, in the
        // frame of the model as given with the cameras as they are handed out, and the associations come down too
        auto pass = [&](bool final) -> hipError_t {
            const uint32_t a = (uint32_t)act.size();
            ProjCam* pcam = (ProjCam*)(h + L.pcam); AssocCam* acam = (AssocCam*)(h + L.acam); AssocCam* ncam = (AssocCam*)(h + L.ncam);
            PoseCam* pose = (PoseCam*)(h + L.pose);
            uint32_t n_tiles = 0;
            std::vector<std::pair<uint32_t, uint32_t>> runs;     // [first, last) of the cameras that share a gate
            for (uint32_t i = 0; i < a; ++i) {
                const uint32_t k = act[i];
                const l3d_camera& in = J.cams[k];
                const CamState& s = state[k];
                ProjCam pc;
                std::memcpy(pc.K, in.K, 72);
                if (final) {
                    const l3d_camera now = pose_camera_now(in, s, c);
                    std::memcpy(pc.R, now.R, 72); std::memcpy(pc.t, now.t, 24);
                } else {
                    pose_about_centre(in, s, pc.R, pc.t);
                }
                pc.xmax = (double)(in.width - 1); pc.ymax = (double)(in.height - 1);
                pcam[i] = pc;
                PoseCam po;
                pose_inverse_transpose(in.K, po.M);
                std::memcpy(po.R, pc.R, 72); std::memcpy(po.t, pc.t, 24);
                pose[i] = po;
                const double gate = final ? p.max_distance : s.gate;
                if (runs.empty() || (final ? p.max_distance : state[act[runs.back().first]].gate) != gate) runs.push_back({i, i});
                runs.back().second = i + 1;
                const uint32_t tiles = (J.n_seg[k] + kAssocTile - 1) / kAssocTile;
                ncam[i] = AssocCam{n_tiles, seg0[k - G.c0], J.n_seg[k], 0u, 0u};
                acam[i] = ncam[i];
                acam[i].tile0 = n_tiles - ncam[runs.back().first].tile0;      // the association's launches are per run
                n_tiles += tiles;
            }
            ProjArgs pa{(const ProjCam*)(d + L.pcam), a, n_model, (const double*)(d + (final ? o_P : o_Pc)), (const uint32_t*)(d + o_line),
                        p.near_plane, (ProjRecord*)(d + L.rec), (uint32_t*)(d + L.vis), (ProjRecord*)(d + L.out), (uint32_t*)(d + L.bounds)};
            PoseNormalArgs na{(const AssocCam*)(d + L.ncam), a, (const PoseCam*)(d + L.pose), (const float4*)(d + L.segs),
                              (const AssocOut*)(d + L.assoc), (const double*)(d + (final ? o_P : o_Pc)), n_model, (double*)(d + L.tiles)};
            hipError_t e_ = hipMemcpyAsync(d + L.pcam, h + L.pcam, L.segs - L.pcam, hipMemcpyHostToDevice, st);
            if (e_ == hipSuccess) e_ = timer.start(st);
            if (e_ == hipSuccess) e_ = launch_project_stage1(w, pa, st);
            if (e_ == hipSuccess) e_ = launch_pose_bounds((AssocCam*)(d + L.acam), a, pa.bounds, st);
            for (const auto& r : runs) {
                if (e_ != hipSuccess) break;
                const double gate = final ? p.max_distance : state[act[r.first]].gate;
                const uint32_t t1 = r.second < a ? ncam[r.second].tile0 : n_tiles;
                AssocArgs aa{(const AssocCam*)(d + L.acam) + r.first, r.second - r.first, (const float4*)(d + L.segs), (const ProjRecord*)(d + L.out),
                             (AssocOut*)(d + L.assoc), gate * gate, p.min_cos2, p.min_overlap};
                e_ = launch_associate(aa, t1 - ncam[r.first].tile0, st);
            }
            if (e_ == hipSuccess) e_ = launch_pose_normal(na, n_tiles, st);
            if (e_ == hipSuccess) e_ = timer.stop(st);
            if (e_ == hipSuccess) e_ = hipMemcpyAsync(h + L.tiles, d + L.tiles, 8 * kPoseTerms * (size_t)n_tiles, hipMemcpyDeviceToHost, st);
            if (e_ == hipSuccess && final && o.assoc) e_ = hipMemcpyAsync(h + L.assoc, d + L.assoc, 24 * (size_t)G.n_seg, hipMemcpyDeviceToHost, st);
            if (e_ == hipSuccess) e_ = hipStreamSynchronize(st);
            if (e_ != hipSuccess) return e_;
            timer.add();
            g_pose_normal_launches.fetch_add(1, std::memory_order_relaxed);
            const double* tiles = (const double*)(h + L.tiles);
            sums.assign((size_t)a * kPoseTerms, 0.0);
            for (uint32_t i = 0; i < a; ++i) {
                const uint32_t t1 = i + 1 < a ? ncam[i + 1].tile0 : n_tiles;
                double* s = sums.data() + (size_t)i * kPoseTerms;
                for (uint32_t t = ncam[i].tile0; t < t1; ++t)
                    for (uint32_t k = 0; k < kPoseTerms; ++k) s[k] = s[k] + tiles[(size_t)t * kPoseTerms + k];
            }
            return hipSuccess;
        };

        for (uint32_t it = 0; it < p.max_iterations; ++it) {
            act.clear();
            for (uint32_t k = G.c0; k < G.c1; ++k)
                if (!state[k].done) act.push_back(k);
            if (act.empty()) break;
            // equal gates side by side (wider first), the cameras of a gate in ascending order
            std::stable_sort(act.begin(), act.end(), [&](uint32_t x, uint32_t y) { return state[x].gate > state[y].gate; });
            if ((e = pass(false)) != hipSuccess) break;
            for (uint32_t i = 0; i < act.size(); ++i) {
                const uint32_t k = act[i];
                CamState& s = state[k];
                const double* sm = sums.data() + (size_t)i * kPoseTerms;
                g_pose_iterations.fetch_add(1, std::memory_order_relaxed);
                l3d_pose_iteration tr{};
                tr.gate = s.gate;
                std::memcpy(tr.sums, sm, sizeof(tr.sums));
                tr.n_matched = (uint64_t)sm[28];
                s.iterations = it + 1;
                double delta[6];
                bool solved = false;
                if (tr.n_matched < p.min_matches) { s.status = L3D_POSE_TOO_FEW; s.done = true; }
                else if (!solve_normal(sm, delta)) { s.status = L3D_POSE_DEGENERATE; s.done = true; }
                else solved = true;
                if (solved) {
                    pose_update(s, delta);
                    s.last_step = step_of(delta, diag);
                    std::memcpy(tr.delta, delta, sizeof(delta));
                    if (s.gate == p.max_distance && s.last_step <= p.step_tolerance) { s.status = L3D_POSE_CONVERGED; s.done = true; }
                    else if (it + 1 == p.max_iterations) { s.status = L3D_POSE_MAX_ITERATIONS; s.done = true; }
                    else if (s.last_step <= p.stall_tolerance) {
                        const double half = s.gate * 0.5;
                        s.gate = half > p.max_distance ? half : p.max_distance;
                    }
                }
                if (o.trace) {
                    const l3d_camera now = pose_camera_now(J.cams[k], s, c);
                    std::memcpy(tr.R, now.R, 72); std::memcpy(tr.t, now.t, 24);
                    trace[(size_t)k * p.max_iterations + it] = tr;
                }
            }
        }
        if (e != hipSuccess) break;
        // the delivery pass: every camera of the group that has segments, at max_distance
        act.clear();
        for (uint32_t k = G.c0; k < G.c1; ++k)
            if (J.n_seg[k]) act.push_back(k);
        if (!act.empty() && (e = pass(true)) != hipSuccess) break;
        for (uint32_t k = G.c0; k < G.c1; ++k) {
            out_cams[k] = pose_camera_now(J.cams[k], state[k], c);
            l3d_pose_summary sm{};
            sm.status = state[k].status; sm.iterations = state[k].iterations; sm.last_step = state[k].last_step;
            for (int i = 0; i < 4; ++i) sm.q[i] = state[k].q[i];
            for (int i = 0; i < 3; ++i) sm.t[i] = state[k].tau[i];
            summaries[k] = sm;
        }
        for (uint32_t i = 0; i < act.size(); ++i) {
            const double* s = sums.data() + (size_t)i * kPoseTerms;
            l3d_pose_summary& sm = summaries[act[i]];
            sm.n_matched = (uint64_t)s[28];
            sm.rms = sm.n_matched ? std::sqrt(s[27] / (2.0 * s[28])) : 0.0;
        }
        if (o.assoc) {
            const AssocOut* res = (const AssocOut*)(h + L.assoc);
            for (size_t i = 0; i < (size_t)G.n_seg; ++i) {
                const AssocOut& r = res[i];
                assoc[seg_at + i] = l3d_association{r.record, r.line, r.segment, std::sqrt(r.d2), r.overlap, r.n_accepted};
            }
        }
        seg_at += G.n_seg;
    }
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("pose refinement: ") + hipGetErrorString(e));

    std::memcpy(o.cams, out_cams.data(), sizeof(l3d_camera) * J.n_cams);
    std::memcpy(o.summaries, summaries.data(), sizeof(l3d_pose_summary) * J.n_cams);
    if (o.assoc && n_seg_total) std::memcpy(o.assoc, assoc.data(), sizeof(l3d_association) * (size_t)n_seg_total);
    if (o.trace)
        for (uint32_t k = 0; k < J.n_cams; ++k)
            if (state[k].iterations)
                std::memcpy(o.trace + (size_t)k * p.max_iterations, trace.data() + (size_t)k * p.max_iterations,
                            sizeof(l3d_pose_iteration) * state[k].iterations);
    return L3D_OK;
}

// What both entries check and decide once the parameters, the model's arrays and the cameras' pointers are known to be
// sound.  done: the call is answered (an error, or nothing to refine against)
int prepare(const Job& J, const l3d_pose_params& p, const Outputs& o, double c[3], double& diag, bool& done) {
    done = true;
    if (J.n_cams && (!o.cams || !o.summaries)) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_pose_cameras(J.n_cams, J.cams, p.near_plane, false)) return rc;
    uint64_t n_seg = 0;
    if (int rc = check_camera_segments(J.n_cams, J.n_seg, J.seg, n_seg)) return rc;
    c[0] = c[1] = c[2] = 0.0; diag = 0.0;
    if (J.n_model) {
        bounding_box(J.n_model, J.segs, c, diag);
        if (!(diag > 0.0)) return fail(L3D_ERR_ARG, "the model's bounding box is a point");
    }
    if (!J.n_cams) return L3D_OK;
    if (J.n_model && n_seg) { done = false; return L3D_OK; }
    // an empty model, or no camera with a segment: nothing to iterate on
    for (uint32_t k = 0; k < J.n_cams; ++k) {
        o.cams[k] = J.cams[k];
        l3d_pose_summary sm{};
        sm.status = L3D_POSE_TOO_FEW; sm.q[0] = 1.0;
        o.summaries[k] = sm;
    }
    if (o.assoc)
        for (uint64_t i = 0; i < n_seg; ++i) o.assoc[i] = no_association();
    return L3D_OK;
}

}  // namespace

extern "C" {

int l3d_refine_cameras(int device, uint32_t n_segments, const double* segs6, const uint32_t* line, uint32_t n_cams,
                       const l3d_camera* cams, const uint32_t* n_segments_per_cam, const float* segs4,
                       const l3d_pose_params* params, l3d_camera* out_cams, l3d_pose_summary* summaries,
                       l3d_association* out_assoc, l3d_pose_iteration* trace) {
    if (int rc = check_params(params)) return rc;
    if (int rc = check_model(nullptr, n_segments, segs6, line)) return rc;
    std::vector<const float*> seg;
    if (int rc = camera_segments(n_cams, cams, n_segments_per_cam, segs4, seg)) return rc;
    const Job J{n_segments, segs6, line, n_cams, cams, n_segments_per_cam, seg.data()};
    const Outputs o{out_cams, summaries, out_assoc, trace};
    double c[3], diag; bool done;
    if (int rc = prepare(J, *params, o, c, diag, done)) return rc;
    if (done) return L3D_OK;
    if (int rc = set_device(device)) return rc;
    ProjWork w;
    return refine_core(w, 0, J, *params, c, diag, o, nullptr);
}

int l3d_refine_view_cameras(l3d_ctx* c, uint32_t n_views, const uint32_t* camIDs, const l3d_pose_params* params,
                            l3d_camera* out_cams, l3d_pose_summary* summaries, uint64_t* offsets, l3d_association* out_assoc,
                            l3d_pose_iteration* trace) {
    if (!c || !offsets || (n_views && !camIDs)) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_params(params)) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (int rc = lines_ready(c, "cameras are refined", "refine cameras against")) return rc;
    ContextViews V; Job J;
    if (int rc = context_job(c, n_views, camIDs, nullptr, V, J)) return rc;
    const Outputs o{out_cams, summaries, out_assoc, trace};
    double ctr[3], diag; bool done;
    if (int rc = prepare(J, *params, o, ctr, diag, done)) return rc;
    if (!done) {
        if (int rc = set_device(c->device)) return rc;
        float ms = 0.0f;
        const bool timed = c->timing_level >= 2;
        if (int rc = refine_core(c->proj, c->stream, J, *params, ctr, diag, o, timed ? &ms : nullptr)) return rc;
        if (timed) g_pose_kernel_ns.store((uint64_t)((double)ms * 1e6), std::memory_order_relaxed);
    }
    offsets[0] = 0;
    for (uint32_t k = 0; k < n_views; ++k) offsets[k + 1] = offsets[k] + V.m[k];
    return L3D_OK;
}

}  // extern "C"
