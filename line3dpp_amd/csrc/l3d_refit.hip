// l3d_refit.hip -- host side of the refit of the 3D lines against cameras and their 2D segments (kernels:
// k_refit.hip and, unchanged, k_project.hip's stage 1, k_scan.hip, k_associate.hip and k_lineopt.hip): the stateless
// l3d_refit_segments with its handle, l3d_refit_view_lines on the context's lines and the added views' own segments, which
// puts the refit model in the context's place, and the host-only hooks l3d_refit_span and l3d_refit_sweep.
//
// The model as given and every camera's 2D segments go up once.  Cameras are taken in GROUPS under the budget of the
// projection stages: stage 1 projects the model into a group's cameras, k_pose_bounds hands the compaction's bounds to the
// association's camera table on the device and launch_associate fills the group's share of the associations, which stay
// on the device for all cameras.  k_refit_flag, k_scan and k_refit_compact list the observations in flat (camera, segment)
// order; their lines come down (4 bytes each) with the associations the handle hands out, from which the host reads off
// every observation's camera and segment.  The host
// sorts them by line (stable counting sort), decides which lines are eligible, forms carriers and start parameters and
// sends the CSR and the permutation back up; k_refit_obs writes the solver's observations, k_lineopt solves every line in
// one launch in the work order of the line bundling (lo_work_order), the host writes the carriers back, k_refit_spans
// projects the observations onto them and the host sweeps the spans into pieces.  Everything the host computes is fp64 in
// the order DESIGN §28 writes it, so that tests/refit_model.py reproduces a call from the associations on.
#include <atomic>
#include <new>
#include <numeric>

#include "l3d_ctx.h"
#include "l3d_refit.h"

namespace l3d {
// test hooks (l3d_debug_counter): observations of the last call, lines handed to the solver so far, and the kernel time of
// the last timed call (context at timing level 2) with its split: projection + association, flag + scan + compaction,
// k_refit_obs, k_lineopt, k_refit_spans
std::atomic<uint64_t> g_refit_observations{0}, g_refit_lines_solved{0}, g_refit_kernel_ns{0}, g_refit_part_ns[5];
}  // namespace l3d

using namespace l3d;

struct l3d_refit { LinesResult<l3d_refit_line, l3d_refit_summary> r; };
using RefitResult = decltype(l3d_refit::r);

namespace {

constexpr uint32_t kRefitMaxGroup = 4096;        // cameras per group at most
static_assert(sizeof(l3d_refit_params) == 64 && sizeof(l3d_refit_line) == 152 && sizeof(l3d_refit_observation) == 32 &&
              sizeof(l3d_refit_summary) == 104, "refit structs");
static_assert(sizeof(AssocOut) == sizeof(l3d_association), "association layout");

int check_params(const l3d_refit_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_thresholds(p->max_distance, p->min_cos2, p->min_overlap)) return rc;
    if (!(p->min_length >= 0.0) || !std::isfinite(p->min_length)) return fail(L3D_ERR_ARG, "min_length must be finite and not negative");
    if (p->visibility < 1) return fail(L3D_ERR_ARG, "visibility must be at least 1");
    if (p->max_iterations > 1000) return fail(L3D_ERR_ARG, "max_iterations must lie in [0, 1000]");
    if (p->use_ambiguous > 1) return fail(L3D_ERR_ARG, "use_ambiguous must be 0 or 1");
    if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return fail(L3D_ERR_ARG, "reserved must be 0");
    return L3D_OK;
}

using Job = RefitJob;

}  // namespace

namespace l3d {

// LoCam of a camera about the centre c: R, C = Q - c with Q_i = -((R_0i t0 + R_1i t1) + R_2i t2), and K's four entries
LoCam refit_lo_camera(const l3d_camera& cam, const double c[3]) {
    LoCam lc;
    for (int k = 0; k < 9; ++k) lc.R[k] = cam.R[k];
    for (int i = 0; i < 3; ++i) lc.C[i] = -((cam.R[i] * cam.t[0] + cam.R[3 + i] * cam.t[1]) + cam.R[6 + i] * cam.t[2]) - c[i];
    lc.fx = cam.K[0]; lc.fy = cam.K[4]; lc.px = cam.K[2]; lc.py = cam.K[5];
    return lc;
}

// What the entries of §28 and §29 check once the parameters, the model's arrays and the cameras' pointers are known to be
// sound; c: the centre of the model's box (0 for an empty model), ml: its lines, n_seg: the 2D segments in all
int refit_check_job(const RefitJob& J, double near_plane, double c[3], ModelLines& ml, uint64_t& n_seg) {
    for (uint32_t i = 0; i < J.n_model; ++i)
        if (J.line[i] >= 0x80000000u) return fail(L3D_ERR_LIMIT, "segment " + std::to_string(i) + " has a line index of 2^31 or more");
    if (int rc = check_pose_cameras(J.n_cams, J.cams, near_plane, true)) return rc;
    if (int rc = check_camera_segments(J.n_cams, J.n_seg, J.seg, n_seg)) return rc;
    c[0] = c[1] = c[2] = 0.0;
    if (J.n_model) {
        double diag;
        bounding_box(J.n_model, J.segs, c, diag);
        if (!(diag > 0.0)) return fail(L3D_ERR_ARG, "the model's bounding box is a point");
    }
    ml.build(J.n_model, J.line);
    return L3D_OK;
}

// Stages 1 to 3 of §28, which the joint bundle of §29 runs on the same function: the upload, projection and association
// group by group, the observation list and its CSR per line.  See l3d_refit.h.
int refit_observe(ProjWork& w, hipStream_t st, const RefitJob& J, double max_distance, double min_cos2, double min_overlap, double near_plane,
                  uint32_t use_ambiguous, uint32_t n_lines, size_t tail_bytes, const char* who, float* ms_assoc, float* ms_list,
                  RefitObserved& O) {
    const std::string tag = std::string(who) + ": ";
    const uint32_t n_model = J.n_model, n_cams = J.n_cams;
    std::vector<uint32_t>& seg_begin = O.seg_begin;
    seg_begin.assign((size_t)n_cams + 1, 0);
    for (uint32_t k = 0; k < n_cams; ++k) seg_begin[k + 1] = seg_begin[k] + J.n_seg[k];
    const uint32_t S = seg_begin[n_cams];
    O.S = S;
    // the groups: cameras with segments while their records fit the budget (one at least)
    struct Group { uint32_t c0, c1, g; uint64_t n_tiles; };
    std::vector<Group> groups;
    for (uint32_t c0 = 0; c0 < n_cams;) {
        Group G{c0, c0, 0, 0};
        uint64_t bytes = 0;
        while (G.c1 < n_cams && G.g < kRefitMaxGroup) {
            const bool has = J.n_seg[G.c1] != 0;
            const uint64_t tiles = ((uint64_t)J.n_seg[G.c1] + kAssocTile - 1) / kAssocTile;
            const uint64_t b = has ? 68 * (uint64_t)n_model + 40 * (uint64_t)J.n_seg[G.c1] : 0;
            if (G.g && has && (bytes + b > projection_budget(w) || (uint64_t)(G.g + 1) * n_model >= ((uint64_t)1 << 31) ||
                               G.n_tiles + tiles >= ((uint64_t)1 << 31)))
                break;
            bytes += b; G.n_tiles += tiles; G.g += has ? 1 : 0;
            ++G.c1;
        }
        groups.push_back(G);
        c0 = G.c1;
    }
    uint32_t g_max = 0;
    for (const Group& G : groups) g_max = std::max(g_max, G.g);
    // what stays for the whole call; behind it a group's tables and records, and later, in their place, the caller's
    Layout lay;
    const size_t o_P = lay.take(48 * (size_t)n_model), o_line = lay.take(4 * (size_t)n_model), o_segs = lay.take(16 * (size_t)S);
    const size_t o_begin = lay.take(4 * ((size_t)n_cams + 1)), up_end = lay.at;
    const size_t o_assoc = lay.take(24 * (size_t)S), o_oseg = lay.take(4 * (size_t)S), o_oline = lay.take(4 * (size_t)S);
    const size_t o_flag = lay.take(4 * ((size_t)S + 1)), keep_end = lay.at;
    const size_t n_rec = (size_t)g_max * n_model;
    const size_t o_pcam = lay.take(sizeof(ProjCam) * g_max), o_acam = lay.take(sizeof(AssocCam) * g_max), grp_up_end = lay.at;
    const size_t o_bounds = lay.take(4 * ((size_t)g_max + 1)), o_vis = lay.take(4 * (n_rec + 1)), o_rec = lay.take(32 * n_rec),
                 o_out = lay.take(32 * n_rec);
    const size_t grp_end = lay.at;
    const size_t sol_bound = up256(keep_end) + tail_bytes;
    O.o_P = o_P; O.o_line = o_line; O.o_segs = o_segs; O.o_begin = o_begin; O.o_oseg = o_oseg; O.keep_end = keep_end; O.bound = sol_bound;
    if (w.h.reserve(std::max(std::max(grp_up_end, keep_end), sol_bound)) != hipSuccess || w.d.reserve(std::max(grp_end, sol_bound)) != hipSuccess ||
        w.scan_ws.reserve_zeroed(std::max(scan_ws_words(n_rec, 4), scan_ws_words(S, 4)), st) != hipSuccess)
        return fail(L3D_ERR_HIP, tag + "allocation failed");
    char* h = w.h.p; char* d = w.d.p;
    KernelTimer t_assoc(ms_assoc), t_list(ms_list);
    if (!t_assoc.ok() || !t_list.ok()) return fail(L3D_ERR_HIP, tag + "no event");
    auto hip_fail = [&tag](hipError_t e) { return fail(L3D_ERR_HIP, tag + hipGetErrorString(e)); };

    // the model as given, its line indices, every camera's segments and where they begin: one upload
    std::memcpy(h + o_P, J.segs, 48 * (size_t)n_model);
    std::memcpy(h + o_line, J.line, 4 * (size_t)n_model);
    for (uint32_t k = 0; k < n_cams; ++k)
        if (J.n_seg[k]) std::memcpy(h + o_segs + 16 * (size_t)seg_begin[k], J.seg[k], 16 * (size_t)J.n_seg[k]);
    std::memcpy(h + o_begin, seg_begin.data(), 4 * ((size_t)n_cams + 1));
    hipError_t e = hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return hip_fail(e);

    // stage 2: projection and association, group by group, in the frame of the model as given
    for (const Group& G : groups) {
        if (!G.g) continue;
        ProjCam* pcam = (ProjCam*)(h + o_pcam); AssocCam* acam = (AssocCam*)(h + o_acam);
        uint32_t i = 0, n_tiles = 0;
        for (uint32_t k = G.c0; k < G.c1; ++k) {
            if (!J.n_seg[k]) continue;
            const l3d_camera& in = J.cams[k];
            ProjCam pc;
            std::memcpy(pc.K, in.K, 72); std::memcpy(pc.R, in.R, 72); std::memcpy(pc.t, in.t, 24);
            pc.xmax = (double)(in.width - 1); pc.ymax = (double)(in.height - 1);
            pcam[i] = pc;
            acam[i] = AssocCam{n_tiles, seg_begin[k], J.n_seg[k], 0u, 0u};
            n_tiles += (J.n_seg[k] + kAssocTile - 1) / kAssocTile;
            ++i;
        }
        ProjArgs pa{(const ProjCam*)(d + o_pcam), G.g, n_model, (const double*)(d + o_P), (const uint32_t*)(d + o_line), near_plane,
                    (ProjRecord*)(d + o_rec), (uint32_t*)(d + o_vis), (ProjRecord*)(d + o_out), (uint32_t*)(d + o_bounds)};
        AssocArgs aa{(const AssocCam*)(d + o_acam), G.g, (const float4*)(d + o_segs), (const ProjRecord*)(d + o_out), (AssocOut*)(d + o_assoc),
                     max_distance * max_distance, min_cos2, min_overlap};
        e = hipMemcpyAsync(d + o_pcam, h + o_pcam, grp_up_end - o_pcam, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = t_assoc.start(st);
        if (e == hipSuccess) e = launch_project_stage1(w, pa, st);
        if (e == hipSuccess) e = launch_pose_bounds((AssocCam*)(d + o_acam), G.g, pa.bounds, st);
        if (e == hipSuccess) e = launch_associate(aa, n_tiles, st);
        if (e == hipSuccess) e = t_assoc.stop(st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);       // (the next group reuses the tables)
        if (e != hipSuccess) return hip_fail(e);
        t_assoc.add();
    }
    // stage 3: the observation list
    const RefitCompactArgs ca{(const AssocOut*)(d + o_assoc), S, use_ambiguous, (uint32_t*)(d + o_flag), (uint32_t*)(d + o_oseg),
                              (uint32_t*)(d + o_oline)};
    uint32_t n_obs = 0;
    e = t_list.start(st);
    if (e == hipSuccess) e = launch_refit_flag(ca, st);
    if (e == hipSuccess) e = launch_scan(ca.flag, S, ca.flag, w.scan_ws.p, nullptr, st);
    if (e == hipSuccess) e = launch_refit_compact(ca, st);
    if (e == hipSuccess) e = t_list.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(h + o_flag, d + o_flag + 4 * (size_t)S, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h + o_assoc, d + o_assoc, 24 * (size_t)S, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e);
    t_list.add();
    std::memcpy(&n_obs, h + o_flag, 4);
    if (n_obs > S) return fail(L3D_ERR_HIP, tag + "the observation count is out of range");
    if (n_obs) {
        e = hipMemcpyAsync(h + o_oline, d + o_oline, 4 * (size_t)n_obs, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(e);
    }
    O.n_obs = n_obs;
    O.assoc.resize(S);
    // the associations as they are handed out; from them the flat 2D segment of every observation, which the device keeps
    // to itself: the list is in flat order, so its j-th entry is the j-th segment that the rule of stage 3 accepts
    std::vector<uint32_t>& oseg = O.oseg;
    oseg.clear(); oseg.reserve(n_obs);
    O.n_ambiguous_left_out = 0;
    {
        const AssocOut* res = (const AssocOut*)(h + o_assoc);
        for (uint32_t i = 0; i < S; ++i) {
            const AssocOut& r = res[i];
            O.assoc[i] = l3d_association{r.record, r.line, r.segment, std::sqrt(r.d2), r.overlap, r.n_accepted};
            if (r.record >= 0 && r.n_accepted > 1 && !use_ambiguous) ++O.n_ambiguous_left_out;
            if (r.record >= 0 && (r.n_accepted == 1 || use_ambiguous)) oseg.push_back(i);
        }
    }
    // the CSR per line (stable counting sort: a line's observations in ascending flat 2D segment)
    O.oline.assign((const uint32_t*)(h + o_oline), (const uint32_t*)(h + o_oline) + n_obs);
    const std::vector<uint32_t>& oline = O.oline;
    if (oseg.size() != n_obs) return fail(L3D_ERR_HIP, tag + "the observation list does not match the associations");
    for (uint32_t j = 0; j < n_obs; ++j)
        if (oline[j] >= n_lines || oline[j] != O.assoc[oseg[j]].line) return fail(L3D_ERR_HIP, tag + "an observation is out of range");
    std::vector<uint32_t>& obs_off = O.obs_off;
    obs_off.assign((size_t)n_lines + 1, 0);
    for (uint32_t j = 0; j < n_obs; ++j) ++obs_off[oline[j] + 1];
    for (uint32_t l = 0; l < n_lines; ++l) obs_off[l + 1] += obs_off[l];
    O.csr.resize(n_obs);                         // the observation (its rank in the compaction) at a CSR position
    {
        std::vector<uint32_t> at(obs_off.begin(), obs_off.end() - 1);
        for (uint32_t j = 0; j < n_obs; ++j) O.csr[at[oline[j]]++] = j;
    }
    return L3D_OK;
}

void refit_list_observations(const RefitObserved& O, uint32_t n_lines, std::vector<l3d_refit_observation>& obs, RefitCells& cells) {
    obs.resize(O.n_obs);
    cells = RefitCells{};
    cells.cell_off.reserve((size_t)O.n_obs + 1); cells.cell_line.reserve(O.n_obs); cells.cell_cam.reserve(O.n_obs);
    cells.line_cell_off.assign((size_t)n_lines + 1, 0);
    for (uint32_t l = 0; l < n_lines; ++l) {
        uint32_t last_cam = 0xFFFFFFFFu;
        for (uint32_t r = O.obs_off[l]; r < O.obs_off[l + 1]; ++r) {
            const uint32_t flat = O.oseg[O.csr[r]];
            const uint32_t cam = (uint32_t)(std::upper_bound(O.seg_begin.begin(), O.seg_begin.end(), flat) - O.seg_begin.begin()) - 1;
            if (cam != last_cam) {
                cells.cell_off.push_back(r);
                cells.cell_line.push_back(l); cells.cell_cam.push_back(cam);
                last_cam = cam;
            }
            obs[r] = l3d_refit_observation{cam, flat - O.seg_begin[cam], l, 0u, 0.0, 0.0};
        }
        cells.line_cell_off[l + 1] = (uint32_t)cells.cell_line.size();
    }
    cells.cell_off.push_back(O.n_obs);
}

int refit_cut_lines(hipStream_t st, KernelTimer& timer, const RefitObsArgs& oa, RefitSpan* down, const std::vector<RefitCut>& cuts,
                    uint32_t n_cams, uint32_t visibility, double min_length, const double c[3], const char* who,
                    std::vector<l3d_refit_observation>& obs, RefitPieces& pieces) {
    // stage 8: spans
    hipError_t e = timer.start(st);
    if (e == hipSuccess) e = launch_refit_spans(oa, st);
    if (e == hipSuccess) e = timer.stop(st);
    if (e == hipSuccess) e = hipMemcpyAsync(down, oa.spans, sizeof(RefitSpan) * oa.n_obs, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    timer.add();
    // stage 9: extents
    std::vector<uint32_t> cam_open(n_cams, 0), cams_v;
    std::vector<double> lo_v, hi_v, cut;
    for (const RefitCut& k : cuts) {
        if (!k.carrier) continue;
        lo_v.clear(); hi_v.clear(); cams_v.clear(); cut.clear();
        for (uint32_t i = 0; i < k.n; ++i) {
            l3d_refit_observation& ob = obs[k.obs0 + i];
            const RefitSpan& sp = down[k.span0 + i];
            ob.valid = sp.valid; ob.s_lo = sp.valid ? sp.lo : 0.0; ob.s_hi = sp.valid ? sp.hi : 0.0;
            if (ob.valid) { lo_v.push_back(sp.lo); hi_v.push_back(sp.hi); cams_v.push_back(ob.camera); }
        }
        const double* M = k.carrier; const double* u = M + 3;
        const double u_norm = std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
        refit_sweep((uint32_t)lo_v.size(), lo_v.data(), hi_v.data(), cams_v.data(), visibility, min_length, u_norm, cam_open, cut);
        pieces.off[k.line] = (uint32_t)(pieces.xyz.size() / 6); pieces.n[k.line] = (uint32_t)(cut.size() / 2);
        for (size_t j = 0; j < cut.size(); ++j)
            for (int i = 0; i < 3; ++i) pieces.xyz.push_back((M[i] + cut[j] * u[i]) + c[i]);
    }
    return L3D_OK;
}

}  // namespace l3d

namespace {

bool finite4(const double* x) { return std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]) && std::isfinite(x[3]); }

// Arguments already checked, model, cameras and 2D segments non-empty, c the centre of the model's box.  R is complete on
// L3D_OK.  kernel_ms (may be null): [5] the time of the launches, by part.
int refit_core(ProjWork& w, hipStream_t st, const Job& J, const l3d_refit_params& p, const double c[3], const ModelLines& ml, RefitResult& R,
               float* kernel_ms) {
    const uint32_t n_cams = J.n_cams, n_lines = ml.n_lines;
    uint64_t S64 = 0;
    for (uint32_t k = 0; k < n_cams; ++k) S64 += J.n_seg[k];
    // the solve's tables at their largest: every line that has a segment solved, every 2D segment an observation
    const size_t nl_max = std::min<size_t>(n_lines, J.n_model);
    const size_t tail = sizeof(LoCam) * n_cams + (32 + 4 + 4 + 48 + sizeof(LoOut)) * nl_max +
                        (4 + sizeof(RefitSpan) + sizeof(LoObs)) * (size_t)S64 + 4 + 9 * 256;
    float* const ms = kernel_ms;
    RefitObserved O;
    if (int rc = refit_observe(w, st, J, p.max_distance, p.min_cos2, p.min_overlap, p.near_plane, p.use_ambiguous, n_lines, tail, "refit",
                               ms ? ms + 0 : nullptr, ms ? ms + 1 : nullptr, O))
        return rc;
    KernelTimer t_obs(ms ? ms + 2 : nullptr), t_solve(ms ? ms + 3 : nullptr), t_spans(ms ? ms + 4 : nullptr);
    if (!t_obs.ok() || !t_solve.ok() || !t_spans.ok()) return fail(L3D_ERR_HIP, "refit: no event");
    auto hip_fail = [](hipError_t e) { return fail(L3D_ERR_HIP, std::string("refit: ") + hipGetErrorString(e)); };
    char* h = w.h.p; char* d = w.d.p;
    hipError_t e = hipSuccess;
    const std::vector<uint32_t>& csr = O.csr;
    const size_t o_segs = O.o_segs, o_begin = O.o_begin, o_oseg = O.o_oseg, keep_end = O.keep_end, sol_bound = O.bound;
    const uint32_t n_obs = O.n_obs;
    g_refit_observations.store(n_obs, std::memory_order_relaxed);
    R.assoc = std::move(O.assoc);
    R.sum.n_ambiguous_left_out = O.n_ambiguous_left_out;
    R.sum.n_observations = n_obs;
    lines_as_given(J, ml, L3D_REFIT_EMPTY, L3D_REFIT_TOO_FEW_VIEWS, R);
    R.obs_off = O.obs_off;
    const std::vector<uint32_t>& obs_off = R.obs_off;
    RefitCells cells;
    refit_list_observations(O, n_lines, R.obs, cells);
    const uint32_t need = std::max<uint32_t>(2u, p.visibility);
    std::vector<uint32_t> sol;                   // the lines handed to the solver, ascending
    std::vector<uint32_t> res_off(1, 0u), perm;
    std::vector<double> x0, carrier0;            // [4 x solved], [6 x solved] the centred carriers as given
    for (uint32_t l = 0; l < n_lines; ++l) {
        l3d_refit_line& L = R.lines[l];
        L.n_observations = obs_off[l + 1] - obs_off[l];
        L.n_views = cells.line_cell_off[l + 1] - cells.line_cell_off[l];
        if (L.status == L3D_REFIT_EMPTY || L.n_views < need) continue;
        double q[6];
        for (int k = 0; k < 3; ++k) { q[k] = L.P1[k] - c[k]; q[3 + k] = L.P2[k] - c[k]; }
        if (line_to_cayley(d3{q[0], q[1], q[2]}, d3{q[3], q[4], q[5]}, L.x0)) {
            L.status = L3D_REFIT_CONSTANT;
            std::memcpy(L.x, L.x0, 32);
            continue;
        }
        L.status = L3D_REFIT_FAILED;             // (until the solve and the sweep say otherwise)
        sol.push_back(l);
        x0.insert(x0.end(), L.x0, L.x0 + 4);
        carrier0.insert(carrier0.end(), q, q + 6);
        perm.insert(perm.end(), csr.begin() + obs_off[l], csr.begin() + obs_off[l + 1]);
        res_off.push_back((uint32_t)perm.size());
    }
    const uint32_t ns = (uint32_t)sol.size(), no = (uint32_t)perm.size();
    RefitPieces pieces(n_lines);
    if (ns) {
        // stages 4 and 6: the solver's tables in the place of the group's
        std::vector<uint32_t> order(ns);
        std::iota(order.begin(), order.end(), 0u);
        const uint32_t n_wide = lo_work_order(res_off.data(), order, kLoNarrow);
        Layout sl;
        sl.at = keep_end;
        const size_t o_cam = sl.take(sizeof(LoCam) * n_cams), o_x0 = sl.take(32 * (size_t)ns), o_off = sl.take(4 * ((size_t)ns + 1)),
                     o_ord = sl.take(4 * (size_t)ns), o_perm = sl.take(4 * (size_t)no), sol_up_end = sl.at;
        const size_t o_car = sl.take(48 * (size_t)ns), o_res = sl.take(sizeof(LoOut) * ns), o_span = sl.take(sizeof(RefitSpan) * no),
                     sol_host_end = sl.at;
        const size_t o_obs = sl.take(sizeof(LoObs) * no), sol_end = sl.at;
        if (sol_end > sol_bound || sol_host_end > sol_bound) return fail(L3D_ERR_HIP, "refit: the solve's tables exceed their bound");
        LoCam* lc = (LoCam*)(h + o_cam);
        for (uint32_t k = 0; k < n_cams; ++k) lc[k] = refit_lo_camera(J.cams[k], c);
        std::memcpy(h + o_x0, x0.data(), 32 * (size_t)ns);
        std::memcpy(h + o_off, res_off.data(), 4 * ((size_t)ns + 1));
        std::memcpy(h + o_ord, order.data(), 4 * (size_t)ns);
        std::memcpy(h + o_perm, perm.data(), 4 * (size_t)no);
        RefitObsArgs oa{no, (const uint32_t*)(d + o_perm), (const uint32_t*)(d + o_oseg), (const float4*)(d + o_segs),
                        (const uint32_t*)(d + o_begin), n_cams, (LoObs*)(d + o_obs), (const LoCam*)(d + o_cam),
                        (const uint32_t*)(d + o_off), ns, (const double*)(d + o_car), (RefitSpan*)(d + o_span)};
        LoArgs la{oa.cams, oa.obs, (const double*)(d + o_x0), oa.res_off, (const uint32_t*)(d + o_ord), n_wide, ns - n_wide,
                  p.max_iterations, (LoOut*)(d + o_res)};
        e = hipMemcpyAsync(d + o_cam, h + o_cam, sol_up_end - o_cam, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = t_obs.start(st);
        if (e == hipSuccess) e = launch_refit_obs(oa, st);
        if (e == hipSuccess) e = t_obs.stop(st);
        if (e == hipSuccess) e = t_solve.start(st);
        if (e == hipSuccess) e = launch_lineopt(la, st);
        if (e == hipSuccess) e = t_solve.stop(st);
        if (e == hipSuccess) e = hipMemcpyAsync(h + o_res, d + o_res, sizeof(LoOut) * ns, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(e);
        t_obs.add(); t_solve.add();
        g_refit_lines_solved.fetch_add(ns, std::memory_order_relaxed);
        // stage 7: write-back
        const LoOut* res = (const LoOut*)(h + o_res);
        double* car = (double*)(h + o_car);
        std::vector<RefitCut> cuts(ns);              // (a line stays without a carrier where the solve failed)
        for (uint32_t s = 0; s < ns; ++s) {
            l3d_refit_line& L = R.lines[sol[s]];
            const LoOut& o = res[s];
            cuts[s] = RefitCut{sol[s], obs_off[sol[s]], res_off[s], res_off[s + 1] - res_off[s], nullptr};
            std::memcpy(L.x, o.x, 32);
            L.cost0 = o.cost0; L.cost1 = o.cost1; L.iterations = o.iters; L.solver_status = o.status;
            for (int k = 0; k < 6; ++k) car[6 * (size_t)s + k] = 0.0;
            if ((o.status == LO_OTHER && o.iters == 0) || !finite4(o.x) || !std::isfinite(o.cost0) || !std::isfinite(o.cost1)) continue;
            const double* q = &carrier0[6 * (size_t)s];
            d3 P1, P2;
            if (!cayley_to_segment(o.x, d3{q[0], q[1], q[2]}, d3{q[3], q[4], q[5]}, P1, P2)) continue;
            const double a[3] = {P1.x, P1.y, P1.z}, b[3] = {P2.x, P2.y, P2.z};
            if (!(std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]) && std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2])))
                continue;
            cuts[s].carrier = car + 6 * (size_t)s;
            for (int k = 0; k < 3; ++k) {
                car[6 * (size_t)s + k] = a[k] * 0.5 + b[k] * 0.5;
                car[6 * (size_t)s + 3 + k] = (a[k] - b[k]) * 0.5;
                L.P1[k] = a[k] + c[k]; L.P2[k] = b[k] + c[k];
            }
        }
        // stages 8 and 9: the lines cut anew on the carriers written back
        e = hipMemcpyAsync(d + o_car, h + o_car, 48 * (size_t)ns, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return hip_fail(e);
        if (int rc = refit_cut_lines(st, t_spans, oa, (RefitSpan*)(h + o_span), cuts, n_cams, p.visibility, p.min_length, c, "refit", R.obs, pieces))
            return rc;
        for (const RefitCut& k : cuts)
            if (k.carrier) R.lines[k.line].status = pieces.n[k.line] ? L3D_REFIT_REFIT : L3D_REFIT_NO_EXTENT;
    }
    assemble(J, ml, pieces, L3D_REFIT_REFIT, R);
    for (const l3d_refit_line& L : R.lines)
        if (L.status == L3D_REFIT_REFIT) { R.sum.cost0 += L.cost0; R.sum.cost1 += L.cost1; }
    return L3D_OK;
}

// What both entries check and decide once the parameters, the model's arrays and the cameras' pointers are known to be
// sound.  done: the call is answered (an error, or every line as given)
int prepare(const Job& J, const l3d_refit_params& p, double c[3], ModelLines& ml, RefitResult& R, bool& done) {
    done = true;
    uint64_t n_seg = 0;
    if (int rc = refit_check_job(J, p.near_plane, c, ml, n_seg)) return rc;
    if (J.n_model && J.n_cams && n_seg) { done = false; return L3D_OK; }
    // an empty model, no camera or no 2D segment: every line as given
    lines_as_given(J, ml, L3D_REFIT_EMPTY, L3D_REFIT_TOO_FEW_VIEWS, R);
    R.assoc.assign((size_t)n_seg, no_association());
    assemble(J, ml, RefitPieces(ml.n_lines), L3D_REFIT_REFIT, R);
    return L3D_OK;
}

void store_kernel_time(const float ms[5]) {
    double all = 0.0;
    for (int k = 0; k < 5; ++k) { g_refit_part_ns[k].store((uint64_t)((double)ms[k] * 1e6), std::memory_order_relaxed); all += (double)ms[k]; }
    g_refit_kernel_ns.store((uint64_t)(all * 1e6), std::memory_order_relaxed);
}

}  // namespace

extern "C" {

int l3d_refit_segments(int device, uint32_t n_segments, const double* segs6, const uint32_t* line, uint32_t n_cams,
                       const l3d_camera* cams, const uint32_t* n_segments_per_cam, const float* segs4,
                       const l3d_refit_params* params, l3d_refit** out) try {
    if (int rc = check_params(params)) return rc;
    if (!out) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_model(nullptr, n_segments, segs6, line)) return rc;
    std::vector<const float*> seg;
    if (int rc = camera_segments(n_cams, cams, n_segments_per_cam, segs4, seg)) return rc;
    const Job J{n_segments, segs6, line, n_cams, cams, n_segments_per_cam, seg.data()};
    auto rf = std::make_unique<l3d_refit>();
    double c[3]; bool done; ModelLines ml;
    if (int rc = prepare(J, *params, c, ml, rf->r, done)) return rc;
    if (!done) {
        if (int rc = set_device(device)) return rc;
        ProjWork w;
        if (int rc = refit_core(w, 0, J, *params, c, ml, rf->r, nullptr)) return rc;
    }
    *out = rf.release();
    return L3D_OK;
} catch (const std::bad_alloc&) {
    return fail(L3D_ERR_LIMIT, "refit: out of host memory");
}

int l3d_refit_view_lines(l3d_ctx* c, uint32_t n_views, const uint32_t* camIDs, const l3d_camera* cams_in,
                         const l3d_refit_params* params, l3d_refit_summary* summary, l3d_refit** out) try {
    if (!c || (n_views && !camIDs)) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_params(params)) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (int rc = lines_ready(c, "lines are refit", "refit")) return rc;
    ContextViews V; Job J;
    if (int rc = context_job(c, n_views, camIDs, cams_in, V, J)) return rc;
    auto rf = std::make_unique<l3d_refit>();
    RefitResult& R = rf->r;
    double ctr[3]; bool done; ModelLines ml;
    if (int rc = prepare(J, *params, ctr, ml, R, done)) return rc;
    if (!done) {
        if (int rc = set_device(c->device)) return rc;
        float ms[5] = {};
        const bool timed = c->timing_level >= 2;
        if (int rc = refit_core(c->proj, c->stream, J, *params, ctr, ml, R, timed ? ms : nullptr)) return rc;
        if (timed) store_kernel_time(ms);
    }
    // the refit model takes the place of lines3D_: the REFIT lines change, every other line is untouched
    if (context_take_lines(c, camIDs, R, lines_cut_anew(R.lines, L3D_REFIT_REFIT))) {   // (else the model is what it was, bit for bit, and so is its name)
        c->lines_refit = true;
        c->refit_distance = params->max_distance;
    }
    if (summary) *summary = R.sum;
    if (out) *out = rf.release();
    return L3D_OK;
} catch (const std::bad_alloc&) {
    return fail(L3D_ERR_LIMIT, "refit: out of host memory");
}

int l3d_refit_counts(const l3d_refit* rf, uint64_t* n_segments, uint64_t* n_lines, uint64_t* n_observations, uint64_t* n_associations) {
    if (!rf) return fail(L3D_ERR_ARG, "null argument");
    if (n_segments) *n_segments = rf->r.seg_line.size();
    if (n_lines) *n_lines = rf->r.lines.size();
    if (n_observations) *n_observations = rf->r.obs.size();
    if (n_associations) *n_associations = rf->r.assoc.size();
    return L3D_OK;
}

int l3d_refit_get(const l3d_refit* rf, double* segs6, uint32_t* seg_line, l3d_refit_line* lines, l3d_refit_observation* observations,
                  l3d_association* associations, l3d_refit_summary* summary) {
    if (!rf) return fail(L3D_ERR_ARG, "null argument");
    const RefitResult& r = rf->r;
    if (segs6 && !r.segs.empty()) std::memcpy(segs6, r.segs.data(), 8 * r.segs.size());
    if (seg_line && !r.seg_line.empty()) std::memcpy(seg_line, r.seg_line.data(), 4 * r.seg_line.size());
    if (lines && !r.lines.empty()) std::memcpy(lines, r.lines.data(), sizeof(l3d_refit_line) * r.lines.size());
    if (observations && !r.obs.empty()) std::memcpy(observations, r.obs.data(), sizeof(l3d_refit_observation) * r.obs.size());
    if (associations && !r.assoc.empty()) std::memcpy(associations, r.assoc.data(), sizeof(l3d_association) * r.assoc.size());
    if (summary) *summary = r.sum;
    return L3D_OK;
}

void l3d_refit_close(l3d_refit* rf) { delete rf; }

int l3d_refit_span(const l3d_camera* cam, const float seg4[4], const double M[3], const double u[3], const double Q[3],
                   double* s_lo, double* s_hi) {
    if (!cam || !seg4 || !M || !u || !Q || !s_lo || !s_hi) return -1;
    LoCam lc;
    for (int k = 0; k < 9; ++k) lc.R[k] = cam->R[k];
    for (int k = 0; k < 3; ++k) lc.C[k] = Q[k];
    lc.fx = cam->K[0]; lc.fy = cam->K[4]; lc.px = cam->K[2]; lc.py = cam->K[5];
    const RefitSpan s = refit_span(lc, (double)seg4[0], (double)seg4[1], (double)seg4[2], (double)seg4[3], M, u);
    *s_lo = s.lo; *s_hi = s.hi;
    return s.valid ? 1 : 0;
}

int l3d_refit_sweep(uint32_t n, const double* s_lo, const double* s_hi, const uint32_t* camera, uint32_t visibility,
                    double min_length, double u_norm, double* pieces, uint32_t* n_pieces) {
    if (!n_pieces || (n && (!s_lo || !s_hi || !camera || !pieces))) return fail(L3D_ERR_ARG, "null argument");
    if (visibility < 1) return fail(L3D_ERR_ARG, "visibility must be at least 1");
    if (!(min_length >= 0.0) || !std::isfinite(min_length)) return fail(L3D_ERR_ARG, "min_length must be finite and not negative");
    if (!(u_norm >= 0.0) || !std::isfinite(u_norm)) return fail(L3D_ERR_ARG, "u_norm must be finite and not negative");
    // the cameras renumbered densely, in order of first appearance
    std::map<uint32_t, uint32_t> dense;
    std::vector<uint32_t> cam(n);
    for (uint32_t i = 0; i < n; ++i) cam[i] = dense.emplace(camera[i], (uint32_t)dense.size()).first->second;
    std::vector<uint32_t> cam_open(dense.size(), 0);
    std::vector<double> cut;
    refit_sweep(n, s_lo, s_hi, cam.data(), visibility, min_length, u_norm, cam_open, cut);
    if (!cut.empty()) std::memcpy(pieces, cut.data(), 8 * cut.size());
    *n_pieces = (uint32_t)(cut.size() / 2);
    return L3D_OK;
}

}  // extern "C"
