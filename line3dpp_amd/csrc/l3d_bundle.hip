// l3d_bundle.hip -- host side of the joint bundle of cameras and 3D lines (kernels: k_bundle.hip and,
// unchanged, k_project.hip's stage 1, k_scan.hip, k_associate.hip and k_refit.hip): the stateless l3d_bundle_segments with
// its handle, l3d_bundle_view_lines on the context's lines and the added views' own segments, and the host-only hook
// l3d_bundle_solve.
//
// Stages 1 to 3 are §28's, on §28's function (refit_observe): one association, the observation list sorted by line.  The
// host cuts the list into cells -- (line, camera) pairs --, decides which lines are eligible and which cameras are free,
// builds the second CSR and the slot table and sends everything up once.  Per iteration of Levenberg-Marquardt:
// k_bundle_cells (after an accepted step only), k_bundle_lines and k_bundle_reduce at the damping in force, the blocks of
// the reduced camera system come down (synchronisation 1), the host assembles and solves it (l3d_bundle_solve), the step
// and the trial poses go up, k_bundle_update and k_bundle_cost run, the cost tiles and the trial carriers come down
// (synchronisation 2) and the host accepts or rejects.  Then §28's stages 8 to 10 on the new carriers and cameras.
// Everything the host computes is fp64 in the order DESIGN §29 writes it, so that tests/bundle_model.py reproduces a call
// from the associations on.
#include <atomic>
#include <new>

#include "l3d_bundle.h"
#include "l3d_ctx.h"
#include "l3d_pose.h"

namespace l3d {
// test hooks (l3d_debug_counter): iterations run and steps rejected so far, the kernel time of the last timed call
std::atomic<uint64_t> g_bundle_iterations{0}, g_bundle_rejected_steps{0}, g_bundle_kernel_ns{0};
}  // namespace l3d

using namespace l3d;

namespace {

struct BundleResult : LinesResult<l3d_bundle_line, l3d_bundle_summary> {
    std::vector<l3d_camera> cams;
    std::vector<l3d_bundle_iteration> trace;
    std::vector<double> system, rhs;             // of the captured iteration: [n x n] (upper triangle set), [n]
};

}  // namespace

struct l3d_bundle { BundleResult r; };

namespace {

static_assert(sizeof(l3d_bundle_params) == 104 && sizeof(l3d_bundle_line) == 64 && sizeof(l3d_bundle_iteration) == 56 &&
              sizeof(l3d_bundle_summary) == 144, "bundle structs");
using Job = RefitJob;

int check_params(const l3d_bundle_params* p) {
    if (!p) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_thresholds(p->max_distance, p->min_cos2, p->min_overlap)) return rc;
    if (!(p->min_length >= 0.0) || !std::isfinite(p->min_length)) return fail(L3D_ERR_ARG, "min_length must be finite and not negative");
    if (p->visibility < 1) return fail(L3D_ERR_ARG, "visibility must be at least 1");
    if (p->max_iterations > 256) return fail(L3D_ERR_ARG, "max_iterations must lie in [0, 256]");
    if (p->use_ambiguous > 1) return fail(L3D_ERR_ARG, "use_ambiguous must be 0 or 1");
    if (!(p->min_damping > 0.0) || !std::isfinite(p->min_damping)) return fail(L3D_ERR_ARG, "min_damping must be finite and greater than 0");
    if (!(p->max_damping >= p->min_damping) || !std::isfinite(p->max_damping))
        return fail(L3D_ERR_ARG, "max_damping must be finite and not below min_damping");
    if (!(p->initial_damping >= p->min_damping && p->initial_damping <= p->max_damping))
        return fail(L3D_ERR_ARG, "initial_damping must lie in [min_damping, max_damping]");
    if (!(p->function_tolerance >= 0.0) || !std::isfinite(p->function_tolerance))
        return fail(L3D_ERR_ARG, "function_tolerance must be finite and not negative");
    if (p->capture_iteration > 256) return fail(L3D_ERR_ARG, "capture_iteration must lie in [0, 256]");
    if (p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3]) return fail(L3D_ERR_ARG, "reserved must be 0");
    return L3D_OK;
}

// S delta = -g for the symmetric S of n rows whose upper triangle S[i * n + j], i <= j, is read, by cholesky_solve
// (l3d_model.h) on heap storage.  false: a pivot that is not finite and > 0, delta untouched.
bool dense_solve(size_t n, const double* S, const double* g, double* delta) {
    std::vector<double> work(n * (n + 1)), rhs(n);
    for (size_t i = 0; i < n; ++i) rhs[i] = -g[i];
    return cholesky_solve(n, S, rhs.data(), delta, work.data());
}

// where the stage's tables lie behind `base`, for given counts
struct Plan {
    size_t locam, perm, obs_off, cell_off, cell_line, cell_cam, line_cell_off, eligible, is_eligible, cam_cell_off, cam_cells, slot,
        free_cam, cam_free, line_ok, delta_l, AB0, AB1, cams0, up_end;
    size_t cams1, delta_c, blocks, rhs, tiles, carrier, spans, host_end;
    size_t obs, cells, W, factor, end;
};
Plan plan(size_t base, size_t n_cams, size_t n_lines, size_t n_obs, size_t n_cells, size_t n_elig, size_t n_free) {
    Layout s;
    s.at = base;
    Plan P;
    P.locam = s.take(sizeof(LoCam) * n_cams); P.perm = s.take(4 * n_obs); P.obs_off = s.take(4 * (n_lines + 1));
    P.cell_off = s.take(4 * (n_cells + 1)); P.cell_line = s.take(4 * n_cells); P.cell_cam = s.take(4 * n_cells);
    P.line_cell_off = s.take(4 * (n_lines + 1)); P.eligible = s.take(4 * n_elig); P.is_eligible = s.take(4 * n_lines);
    P.cam_cell_off = s.take(4 * (n_cams + 1)); P.cam_cells = s.take(4 * n_cells); P.slot = s.take(4 * n_lines * n_cams);
    P.free_cam = s.take(4 * n_free); P.cam_free = s.take(4 * n_cams); P.line_ok = s.take(4 * n_lines); P.delta_l = s.take(32 * n_lines);
    P.AB0 = s.take(48 * n_lines); P.AB1 = s.take(48 * n_lines); P.cams0 = s.take(sizeof(PoseCam) * n_cams); P.up_end = s.at;
    P.cams1 = s.take(sizeof(PoseCam) * n_cams); P.delta_c = s.take(48 * n_free); P.blocks = s.take(288 * n_free * n_free);
    P.rhs = s.take(48 * n_free); P.tiles = s.take(8 * ((n_obs + kBundleBlock - 1) / kBundleBlock)); P.carrier = s.take(48 * n_lines);
    P.spans = s.take(sizeof(RefitSpan) * n_obs); P.host_end = s.at;
    P.obs = s.take(sizeof(LoObs) * n_obs); P.cells = s.take(8 * kBundleCell * n_cells); P.W = s.take(192 * n_cells);
    P.factor = s.take(sizeof(BundleFactor) * n_lines); P.end = s.at;
    return P;
}

bool finite6(const double* x) {
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(x[k])) return false;
    return true;
}

// Arguments already checked, model, cameras and 2D segments non-empty, c the centre of the model's box.  R is complete on
// L3D_OK.  kernel_ms (may be null): the time of the launches, summed.
int bundle_core(ProjWork& w, hipStream_t st, const Job& J, const uint8_t* fixed, const l3d_bundle_params& p, const double c[3],
                const ModelLines& ml, BundleResult& R, float* kernel_ms) {
    const uint32_t n_cams = J.n_cams, n_lines = ml.n_lines;
    uint64_t S64 = 0;
    uint32_t not_fixed = 0;
    for (uint32_t k = 0; k < n_cams; ++k) { S64 += J.n_seg[k]; not_fixed += (fixed && fixed[k]) ? 0 : 1; }
    const size_t tail = plan(0, n_cams, n_lines, S64, S64, n_lines, not_fixed).end + 256;
    float ms[3] = {0.0f, 0.0f, 0.0f};
    RefitObserved O;
    if (int rc = refit_observe(w, st, J, p.max_distance, p.min_cos2, p.min_overlap, p.near_plane, p.use_ambiguous, n_lines, tail, "bundle",
                               kernel_ms ? ms + 0 : nullptr, kernel_ms ? ms + 1 : nullptr, O))
        return rc;
    KernelTimer timer(kernel_ms ? ms + 2 : nullptr);
    if (!timer.ok()) return fail(L3D_ERR_HIP, "bundle: no event");
    auto hip_fail = [](hipError_t e) { return fail(L3D_ERR_HIP, std::string("bundle: ") + hipGetErrorString(e)); };
    const uint32_t n_obs = O.n_obs;
    R.assoc = std::move(O.assoc);
    R.sum.n_ambiguous_left_out = O.n_ambiguous_left_out;
    R.sum.n_observations = n_obs;
    lines_as_given(J, ml, L3D_BUNDLE_EMPTY, L3D_BUNDLE_HELD, R);
    R.obs_off = O.obs_off;
    const std::vector<uint32_t>& obs_off = R.obs_off;
    RefitCells cells;
    refit_list_observations(O, n_lines, R.obs, cells);
    const std::vector<uint32_t>&cell_off = cells.cell_off, &cell_line = cells.cell_line, &cell_cam = cells.cell_cam,
                               &line_cell_off = cells.line_cell_off;
    const uint32_t n_cells = (uint32_t)cell_line.size();
    R.sum.n_cells = n_cells;
    // eligible lines, carriers about the centre
    const uint32_t need = std::max<uint32_t>(2u, p.visibility);
    std::vector<uint32_t> eligible, is_eligible(n_lines, 0);
    std::vector<double> AB(6 * (size_t)n_lines, 0.0);
    for (uint32_t l = 0; l < n_lines; ++l) {
        l3d_bundle_line& L = R.lines[l];
        L.n_observations = obs_off[l + 1] - obs_off[l];
        L.n_views = line_cell_off[l + 1] - line_cell_off[l];
        if (L.status == L3D_BUNDLE_EMPTY) continue;
        double* q = &AB[6 * (size_t)l];
        for (int k = 0; k < 3; ++k) { q[k] = L.P1[k] - c[k]; q[3 + k] = L.P2[k] - c[k]; }
        const double u[3] = {q[3] - q[0], q[4] - q[1], q[5] - q[2]};
        const double uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
        if (L.n_views < need || !(uu > 0.0) || !std::isfinite(uu)) continue;
        is_eligible[l] = 1; eligible.push_back(l);
    }
    const uint32_t n_elig = (uint32_t)eligible.size();
    R.sum.n_eligible_lines = n_elig;
    // the second CSR (stable counting sort of the cells by camera), the slot table, the free cameras
    std::vector<uint32_t> cam_cell_off((size_t)n_cams + 1, 0), cam_cells(n_cells);
    for (uint32_t i = 0; i < n_cells; ++i) ++cam_cell_off[cell_cam[i] + 1];
    for (uint32_t k = 0; k < n_cams; ++k) cam_cell_off[k + 1] += cam_cell_off[k];
    {
        std::vector<uint32_t> at(cam_cell_off.begin(), cam_cell_off.end() - 1);
        for (uint32_t i = 0; i < n_cells; ++i) cam_cells[at[cell_cam[i]]++] = i;
    }
    std::vector<int32_t> slot((size_t)n_lines * n_cams, -1), cam_free(n_cams, -1);
    for (uint32_t i = 0; i < n_cells; ++i) slot[(size_t)cell_line[i] * n_cams + cell_cam[i]] = (int32_t)i;
    std::vector<uint32_t> free_cam;
    for (uint32_t k = 0; k < n_cams; ++k)
        if (!(fixed && fixed[k]) && cam_cell_off[k + 1] > cam_cell_off[k]) { cam_free[k] = (int32_t)free_cam.size(); free_cam.push_back(k); }
    const uint32_t F = (uint32_t)free_cam.size();
    R.sum.n_free_cameras = F;
    // the cameras' states and their poses about the centre
    std::vector<PoseDelta> state(n_cams), trial_state;
    std::vector<PoseCam> pose(n_cams), pose_trial(n_cams);
    for (uint32_t k = 0; k < n_cams; ++k) {
        const d3 rc = mul33(J.cams[k].R, d3{c[0], c[1], c[2]});
        state[k].tin[0] = J.cams[k].t[0] + rc.x; state[k].tin[1] = J.cams[k].t[1] + rc.y; state[k].tin[2] = J.cams[k].t[2] + rc.z;
        pose_inverse_transpose(J.cams[k].K, pose[k].M);
        pose_about_centre(J.cams[k], state[k], pose[k].R, pose[k].t);
    }
    R.cams.assign(J.cams, J.cams + n_cams);

    const Plan P = plan(O.keep_end, n_cams, n_lines, n_obs, n_cells, n_elig, F);
    if (P.end > O.bound) return fail(L3D_ERR_HIP, "bundle: the tables exceed their bound");
    char* h = w.h.p; char* d = w.d.p;
    auto put = [h](size_t at, const void* src, size_t bytes) { if (bytes) std::memcpy(h + at, src, bytes); };
    std::memset(h + P.locam, 0, P.up_end - P.locam);
    put(P.perm, O.csr.data(), 4 * (size_t)n_obs); put(P.obs_off, obs_off.data(), 4 * ((size_t)n_lines + 1));
    put(P.cell_off, cell_off.data(), 4 * ((size_t)n_cells + 1)); put(P.cell_line, cell_line.data(), 4 * (size_t)n_cells);
    put(P.cell_cam, cell_cam.data(), 4 * (size_t)n_cells); put(P.line_cell_off, line_cell_off.data(), 4 * ((size_t)n_lines + 1));
    put(P.eligible, eligible.data(), 4 * (size_t)n_elig); put(P.is_eligible, is_eligible.data(), 4 * (size_t)n_lines);
    put(P.cam_cell_off, cam_cell_off.data(), 4 * ((size_t)n_cams + 1)); put(P.cam_cells, cam_cells.data(), 4 * (size_t)n_cells);
    put(P.slot, slot.data(), 4 * slot.size()); put(P.free_cam, free_cam.data(), 4 * (size_t)F); put(P.cam_free, cam_free.data(), 4 * (size_t)n_cams);
    put(P.AB0, AB.data(), 48 * (size_t)n_lines); put(P.AB1, AB.data(), 48 * (size_t)n_lines);
    put(P.cams0, pose.data(), sizeof(PoseCam) * n_cams);
    const size_t o_AB[2] = {P.AB0, P.AB1}, o_cams[2] = {P.cams0, P.cams1};
    int cur = 0;
    double mu = p.initial_damping;
    auto args = [&]() {
        BundleArgs a{};
        a.n_cams = n_cams; a.n_lines = n_lines; a.n_obs = n_obs; a.n_cells = n_cells; a.n_eligible = n_elig; a.n_free = F;
        a.cams = (const PoseCam*)(d + o_cams[cur]); a.cams_trial = (const PoseCam*)(d + o_cams[cur ^ 1]);
        a.obs = (const LoObs*)(d + P.obs); a.obs_off = (const uint32_t*)(d + P.obs_off);
        a.cell_off = (const uint32_t*)(d + P.cell_off); a.cell_line = (const uint32_t*)(d + P.cell_line);
        a.cell_cam = (const uint32_t*)(d + P.cell_cam); a.line_cell_off = (const uint32_t*)(d + P.line_cell_off);
        a.eligible = (const uint32_t*)(d + P.eligible); a.is_eligible = (const uint32_t*)(d + P.is_eligible);
        a.cam_cell_off = (const uint32_t*)(d + P.cam_cell_off); a.cam_cells = (const uint32_t*)(d + P.cam_cells);
        a.slot = (const int32_t*)(d + P.slot); a.free_cam = (const uint32_t*)(d + P.free_cam); a.cam_free = (const int32_t*)(d + P.cam_free);
        a.AB = (const double*)(d + o_AB[cur]); a.AB_trial = (double*)(d + o_AB[cur ^ 1]);
        a.mu = mu;
        a.cells = (double*)(d + P.cells); a.line_ok = (uint32_t*)(d + P.line_ok); a.factor = (BundleFactor*)(d + P.factor);
        a.W = (double*)(d + P.W); a.blocks = (double*)(d + P.blocks); a.rhs = (double*)(d + P.rhs);
        a.delta_c = (const double*)(d + P.delta_c); a.delta_l = (double*)(d + P.delta_l); a.tiles = (double*)(d + P.tiles);
        return a;
    };
    const uint32_t n_tiles = (n_obs + kBundleBlock - 1) / kBundleBlock;
    auto host_cost = [&]() {
        const double* t = (const double*)(h + P.tiles);
        double s = 0.0;
        for (uint32_t i = 0; i < n_tiles; ++i) s = s + t[i];
        return s;
    };
    RefitObsArgs oa{n_obs, (const uint32_t*)(d + P.perm), (const uint32_t*)(d + O.o_oseg), (const float4*)(d + O.o_segs),
                    (const uint32_t*)(d + O.o_begin), n_cams, (LoObs*)(d + P.obs), (const LoCam*)(d + P.locam),
                    (const uint32_t*)(d + P.obs_off), n_lines, (const double*)(d + P.carrier), (RefitSpan*)(d + P.spans)};
    // the tables go up; the solver's observations; the cost of the input (the "trial" of the state in force)
    hipError_t e = hipMemcpyAsync(d + P.locam, h + P.locam, P.up_end - P.locam, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = timer.start(st);
    if (e == hipSuccess) e = launch_refit_obs(oa, st);
    {
        BundleArgs a = args();
        a.cams_trial = a.cams; a.AB_trial = (double*)(d + o_AB[cur]);
        if (e == hipSuccess) e = launch_bundle_cost(a, st);
    }
    if (e == hipSuccess) e = timer.stop(st);
    if (e == hipSuccess && n_tiles) e = hipMemcpyAsync(h + P.tiles, d + P.tiles, 8 * (size_t)n_tiles, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e);
    timer.add();
    double cost = host_cost();
    R.sum.cost0 = cost;
    R.sum.status = (n_elig || F) ? L3D_BUNDLE_MAX_ITERATIONS : L3D_BUNDLE_NO_VARIABLES;
    bool linearise = true;
    const size_t n = 6 * (size_t)F;
    std::vector<double> Ssys(n * n), g(n), delta(n), AB_trial;
    for (uint32_t it = 0; it < p.max_iterations && (n_elig || F); ++it) {
        l3d_bundle_iteration T{};
        T.damping = mu; T.cost = cost;
        ++R.sum.iterations;
        g_bundle_iterations.fetch_add(1, std::memory_order_relaxed);
        const BundleArgs a = args();
        e = timer.start(st);
        if (e == hipSuccess && linearise) e = launch_bundle_cells(a, st);
        if (e == hipSuccess) e = launch_bundle_lines(a, st);
        if (e == hipSuccess) e = launch_bundle_reduce(a, st);
        if (e == hipSuccess) e = timer.stop(st);
        if (e == hipSuccess && F) e = hipMemcpyAsync(h + P.blocks, d + P.blocks, 288 * (size_t)F * F, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && F) e = hipMemcpyAsync(h + P.rhs, d + P.rhs, 48 * (size_t)F, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h + P.line_ok, d + P.line_ok, 4 * (size_t)n_lines, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);       // synchronisation 1
        if (e != hipSuccess) return hip_fail(e);
        timer.add();
        linearise = false;
        {
            const uint32_t* ok = (const uint32_t*)(h + P.line_ok);
            for (uint32_t l : eligible) T.n_held_for_step += ok[l] ? 0u : 1u;
        }
        // the reduced system over the free cameras, ascending
        bool solved = true;
        if (F) {
            const double* blocks = (const double*)(h + P.blocks);
            std::fill(Ssys.begin(), Ssys.end(), 0.0);
            for (uint32_t fa = 0; fa < F; ++fa)
                for (uint32_t fb = fa; fb < F; ++fb) {
                    const double* B = blocks + 36 * ((size_t)fa * F + fb);
                    for (int i = 0; i < 6; ++i)
                        for (int j = 0; j < 6; ++j) {
                            const size_t row = 6 * (size_t)fa + i, col = 6 * (size_t)fb + j;
                            if (row <= col) Ssys[row * n + col] = B[6 * i + j];
                        }
                }
            std::memcpy(g.data(), h + P.rhs, 8 * n);
            if (p.capture_iteration == it + 1) { R.system = Ssys; R.rhs = g; R.sum.captured = 1; }
            solved = dense_solve(n, Ssys.data(), g.data(), delta.data());
        } else if (p.capture_iteration == it + 1) {
            R.system.clear(); R.rhs.clear(); R.sum.captured = 1;
        }
        T.solved = solved ? 1u : 0u;
        bool accept = false;
        if (solved) {
            trial_state = state;
            pose_trial = pose;
            for (uint32_t f = 0; f < F; ++f) {
                const uint32_t k = free_cam[f];
                pose_update(trial_state[k], &delta[6 * (size_t)f]);
                pose_about_centre(J.cams[k], trial_state[k], pose_trial[k].R, pose_trial[k].t);
                for (int i = 0; i < 6; ++i) T.step_cameras = std::max(T.step_cameras, std::fabs(delta[6 * (size_t)f + i]));
            }
            put(o_cams[cur ^ 1], pose_trial.data(), sizeof(PoseCam) * n_cams);
            put(P.delta_c, delta.data(), 8 * n);
            e = hipMemcpyAsync(d + o_cams[cur ^ 1], h + o_cams[cur ^ 1], sizeof(PoseCam) * n_cams, hipMemcpyHostToDevice, st);
            if (e == hipSuccess && F) e = hipMemcpyAsync(d + P.delta_c, h + P.delta_c, 8 * n, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = timer.start(st);
            if (e == hipSuccess) e = launch_bundle_update(a, st);
            if (e == hipSuccess) e = launch_bundle_cost(a, st);
            if (e == hipSuccess) e = timer.stop(st);
            if (e == hipSuccess && n_tiles) e = hipMemcpyAsync(h + P.tiles, d + P.tiles, 8 * (size_t)n_tiles, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(h + P.delta_l, d + P.delta_l, 32 * (size_t)n_lines, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(h + o_AB[cur ^ 1], d + o_AB[cur ^ 1], 48 * (size_t)n_lines, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);   // synchronisation 2
            if (e != hipSuccess) return hip_fail(e);
            timer.add();
            const double* dl = (const double*)(h + P.delta_l);
            for (uint32_t l : eligible)
                for (int i = 0; i < 4; ++i) T.step_lines = std::max(T.step_lines, std::fabs(dl[4 * (size_t)l + i]));
            T.cost_trial = host_cost();
            accept = T.cost_trial < cost;
        }
        T.accepted = accept ? 1u : 0u;
        R.trace.push_back(T);
        if (accept) {
            ++R.sum.accepted_steps;
            state = trial_state; pose = pose_trial;
            AB.assign((const double*)(h + o_AB[cur ^ 1]), (const double*)(h + o_AB[cur ^ 1]) + 6 * (size_t)n_lines);
            cur ^= 1;
            linearise = true;
            mu = std::max(mu / 10.0, p.min_damping);
            const bool converged = (cost - T.cost_trial) <= p.function_tolerance * cost;
            cost = T.cost_trial;
            if (converged) { R.sum.status = L3D_BUNDLE_CONVERGED; break; }
        } else {
            ++R.sum.rejected_steps;
            g_bundle_rejected_steps.fetch_add(1, std::memory_order_relaxed);
            mu = mu * 10.0;
            if (mu > p.max_damping) { R.sum.status = L3D_BUNDLE_STALLED; break; }
        }
    }
    R.sum.cost1 = cost; R.sum.damping = mu;
    // the cameras by §27's rule; the carriers back in the model's frame
    std::vector<LoCam> locam(n_cams);
    for (uint32_t k = 0; k < n_cams; ++k) { R.cams[k] = pose_camera_now(J.cams[k], state[k], c); locam[k] = refit_lo_camera(R.cams[k], c); }
    std::vector<double> carrier(6 * (size_t)n_lines, 0.0);
    for (uint32_t l = 0; l < n_lines; ++l) {
        const double* q = &AB[6 * (size_t)l];
        for (int k = 0; k < 3; ++k) {
            carrier[6 * (size_t)l + k] = q[k] * 0.5 + q[3 + k] * 0.5;
            carrier[6 * (size_t)l + 3 + k] = (q[k] - q[3 + k]) * 0.5;
        }
        if (is_eligible[l] && R.sum.accepted_steps)
            for (int k = 0; k < 3; ++k) { R.lines[l].P1[k] = q[k] + c[k]; R.lines[l].P2[k] = q[3 + k] + c[k]; }
    }
    RefitPieces pieces(n_lines);
    if (n_elig) {
        // §28's stages 8 and 9 on the new carriers and cameras
        std::vector<RefitCut> cuts;
        for (uint32_t l : eligible) {
            R.lines[l].status = L3D_BUNDLE_NO_EXTENT;
            cuts.push_back(RefitCut{l, obs_off[l], obs_off[l], obs_off[l + 1] - obs_off[l], finite6(&AB[6 * (size_t)l]) ? &carrier[6 * (size_t)l] : nullptr});
        }
        put(P.locam, locam.data(), sizeof(LoCam) * n_cams); put(P.carrier, carrier.data(), 48 * (size_t)n_lines);
        e = hipMemcpyAsync(d + P.locam, h + P.locam, sizeof(LoCam) * n_cams, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d + P.carrier, h + P.carrier, 48 * (size_t)n_lines, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return hip_fail(e);
        if (int rc = refit_cut_lines(st, timer, oa, (RefitSpan*)(h + P.spans), cuts, n_cams, p.visibility, p.min_length, c, "bundle", R.obs, pieces))
            return rc;
        for (uint32_t l : eligible)
            if (pieces.n[l]) R.lines[l].status = L3D_BUNDLE_BUNDLED;
    }
    assemble(J, ml, pieces, L3D_BUNDLE_BUNDLED, R);
    if (kernel_ms) *kernel_ms = ms[0] + ms[1] + ms[2];
    return L3D_OK;
}

// What both entries check and decide once the parameters, the model's arrays and the cameras' pointers are known to be
// sound.  done: the call is answered (an error, or everything as given)
int prepare(const Job& J, const uint8_t* fixed, const l3d_bundle_params& p, double c[3], ModelLines& ml, BundleResult& R, bool& done) {
    done = true;
    uint64_t n_seg = 0;
    if (int rc = refit_check_job(J, p.near_plane, c, ml, n_seg)) return rc;
    uint32_t not_fixed = 0;
    for (uint32_t k = 0; k < J.n_cams; ++k) {
        if (fixed && fixed[k] > 1) return fail(L3D_ERR_ARG, "camera " + std::to_string(k) + ": fixed must be 0 or 1");
        not_fixed += (fixed && fixed[k]) ? 0 : 1;
    }
    if (not_fixed > kBundleMaxFree) return fail(L3D_ERR_LIMIT, "more than 512 free cameras: the reduced system is dense");
    if ((uint64_t)ml.n_lines * J.n_cams >= ((uint64_t)1 << 28)) return fail(L3D_ERR_LIMIT, "lines x cameras reach 2^28: the slot table is dense");
    if (J.n_model && J.n_cams && n_seg) { done = false; return L3D_OK; }
    // an empty model, no camera or no 2D segment: everything as given
    lines_as_given(J, ml, L3D_BUNDLE_EMPTY, L3D_BUNDLE_HELD, R);
    R.assoc.assign((size_t)n_seg, no_association());
    R.cams.assign(J.cams, J.cams + J.n_cams);
    R.sum.status = L3D_BUNDLE_NO_VARIABLES;
    assemble(J, ml, RefitPieces(ml.n_lines), L3D_BUNDLE_BUNDLED, R);
    return L3D_OK;
}

}  // namespace

extern "C" {

int l3d_bundle_segments(int device, uint32_t n_segments, const double* segs6, const uint32_t* line, uint32_t n_cams,
                        const l3d_camera* cams, const uint8_t* fixed, const uint32_t* n_segments_per_cam, const float* segs4,
                        const l3d_bundle_params* params, l3d_bundle** out) try {
    if (int rc = check_params(params)) return rc;
    if (!out) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_model(nullptr, n_segments, segs6, line)) return rc;
    std::vector<const float*> seg;
    if (int rc = camera_segments(n_cams, cams, n_segments_per_cam, segs4, seg)) return rc;
    const Job J{n_segments, segs6, line, n_cams, cams, n_segments_per_cam, seg.data()};
    auto bd = std::make_unique<l3d_bundle>();
    double c[3]; bool done; ModelLines ml;
    if (int rc = prepare(J, fixed, *params, c, ml, bd->r, done)) return rc;
    if (!done) {
        if (int rc = set_device(device)) return rc;
        ProjWork w;
        if (int rc = bundle_core(w, 0, J, fixed, *params, c, ml, bd->r, nullptr)) return rc;
    }
    *out = bd.release();
    return L3D_OK;
} catch (const std::bad_alloc&) {
    return fail(L3D_ERR_LIMIT, "bundle: out of host memory");
}

int l3d_bundle_view_lines(l3d_ctx* c, uint32_t n_views, const uint32_t* camIDs, const l3d_camera* cams_in, const uint8_t* fixed,
                          const l3d_bundle_params* params, l3d_bundle_summary* summary, l3d_bundle** out) try {
    if (!c || (n_views && !camIDs)) return fail(L3D_ERR_ARG, "null argument");
    if (int rc = check_params(params)) return rc;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (int rc = lines_ready(c, "lines are bundled", "bundle")) return rc;
    ContextViews V; Job J;
    if (int rc = context_job(c, n_views, camIDs, cams_in, V, J)) return rc;
    auto bd = std::make_unique<l3d_bundle>();
    BundleResult& R = bd->r;
    double ctr[3]; bool done; ModelLines ml;
    if (int rc = prepare(J, fixed, *params, ctr, ml, R, done)) return rc;
    if (!done) {
        if (int rc = set_device(c->device)) return rc;
        float ms = 0.0f;
        const bool timed = c->timing_level >= 2;
        if (int rc = bundle_core(c->proj, c->stream, J, fixed, *params, ctr, ml, R, timed ? &ms : nullptr)) return rc;
        if (timed) g_bundle_kernel_ns.store((uint64_t)((double)ms * 1e6), std::memory_order_relaxed);
    }
    // the bundled model takes the place of lines3D_: the BUNDLED lines change, every other line is untouched; the views'
    // cameras stay as they are
    if (context_take_lines(c, camIDs, R, lines_cut_anew(R.lines, L3D_BUNDLE_BUNDLED))) {   // (else the model is what it was, bit for bit, and so is its name)
        c->lines_bundled = true;
        c->bundle_distance = params->max_distance;
    }
    if (summary) *summary = R.sum;
    if (out) *out = bd.release();
    return L3D_OK;
} catch (const std::bad_alloc&) {
    return fail(L3D_ERR_LIMIT, "bundle: out of host memory");
}

int l3d_bundle_counts(const l3d_bundle* bd, uint64_t* n_segments, uint64_t* n_lines, uint64_t* n_observations, uint64_t* n_associations,
                      uint64_t* n_cameras, uint64_t* n_iterations, uint64_t* n_system) {
    if (!bd) return fail(L3D_ERR_ARG, "null argument");
    if (n_segments) *n_segments = bd->r.seg_line.size();
    if (n_lines) *n_lines = bd->r.lines.size();
    if (n_observations) *n_observations = bd->r.obs.size();
    if (n_associations) *n_associations = bd->r.assoc.size();
    if (n_cameras) *n_cameras = bd->r.cams.size();
    if (n_iterations) *n_iterations = bd->r.trace.size();
    if (n_system) *n_system = bd->r.rhs.size();
    return L3D_OK;
}

int l3d_bundle_get(const l3d_bundle* bd, double* segs6, uint32_t* seg_line, l3d_bundle_line* lines, l3d_refit_observation* observations,
                   l3d_association* associations, l3d_camera* cams, l3d_bundle_iteration* trace, double* system, double* rhs,
                   l3d_bundle_summary* summary) {
    if (!bd) return fail(L3D_ERR_ARG, "null argument");
    const BundleResult& r = bd->r;
    if (segs6 && !r.segs.empty()) std::memcpy(segs6, r.segs.data(), 8 * r.segs.size());
    if (seg_line && !r.seg_line.empty()) std::memcpy(seg_line, r.seg_line.data(), 4 * r.seg_line.size());
    if (lines && !r.lines.empty()) std::memcpy(lines, r.lines.data(), sizeof(l3d_bundle_line) * r.lines.size());
    if (observations && !r.obs.empty()) std::memcpy(observations, r.obs.data(), sizeof(l3d_refit_observation) * r.obs.size());
    if (associations && !r.assoc.empty()) std::memcpy(associations, r.assoc.data(), sizeof(l3d_association) * r.assoc.size());
    if (cams && !r.cams.empty()) std::memcpy(cams, r.cams.data(), sizeof(l3d_camera) * r.cams.size());
    if (trace && !r.trace.empty()) std::memcpy(trace, r.trace.data(), sizeof(l3d_bundle_iteration) * r.trace.size());
    if (system && !r.system.empty()) std::memcpy(system, r.system.data(), 8 * r.system.size());
    if (rhs && !r.rhs.empty()) std::memcpy(rhs, r.rhs.data(), 8 * r.rhs.size());
    if (summary) *summary = r.sum;
    return L3D_OK;
}

void l3d_bundle_close(l3d_bundle* bd) { delete bd; }

int l3d_bundle_solve(uint32_t n, const double* S, const double* g, double* delta) try {
    if (n && (!S || !g || !delta)) return -1;
    return dense_solve(n, S, g, delta) ? 1 : 0;
} catch (const std::bad_alloc&) {
    return -1;
}

}  // extern "C"
