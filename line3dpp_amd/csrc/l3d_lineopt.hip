// l3d_lineopt.hip -- host side of the line bundling stage (l3d_lineopt.h): Line3D::optimizeClusters ->
// LineOptimizer::optimize (optimization.cc:8-303) between the clustering and computeFinal3Dsegments of
// reconstruct3Dlines, in the translated frame.  Parametrisation (:31-95) and write-back (:209-295) are host work as in
// the reference; the per-line solves run in one launch of k_lineopt (k_lineopt.hip).
#include "l3d_ctx.h"
#include "l3d_lineopt.h"

#include <algorithm>
#include <numeric>

namespace l3d {

// Plücker form of the line through P1, P2 and its Cayley form (optimization.cc:31-95).  true = the line is held
// constant (a NaN anywhere: x = (-1, 0, 0, 0))
bool line_to_cayley(const d3& P1, const d3& P2, double x[4]) {
    const d3 l = normalized(P2 - P1);
    const d3 m = cross((P1 + P2) * 0.5, l);
    const double omega = norm(m);
    d3 e1, e2;
    if (omega < kEps) {
        // kernel of l^T as Eigen's FullPivLU::kernel() gives it: pivot = first largest |l_k|; with the columns
        // permuted (0 <-> k), the kernel vectors are -u_j / u_0 at row k and a 1 at the rows of the permuted columns 1, 2
        const double a[3] = {l.x, l.y, l.z};
        int k = 0;
        for (int j = 1; j < 3; ++j) if (std::fabs(a[j]) > std::fabs(a[k])) k = j;
        int q[3] = {0, 1, 2};
        std::swap(q[0], q[k]);
        double v[2][3] = {{0, 0, 0}, {0, 0, 0}};
        for (int c = 0; c < 2; ++c) {
            v[c][k] = -(a[q[c + 1]] / a[q[0]]);
            v[c][q[c + 1]] = 1.0;
        }
        e1 = d3{v[0][0], v[0][1], v[0][2]};
        e2 = d3{v[1][0], v[1][1], v[1][2]};
    } else {
        e1 = normalized(m);
        e2 = normalized(cross(l, m));
    }
    const M3 Q{{l.x, e1.x, e2.x, l.y, e1.y, e2.y, l.z, e1.z, e2.z}};
    M3 Qm = Q, Qp = Q;
    for (int i = 0; i < 3; ++i) { Qm.m[4 * i] -= 1.0; Qp.m[4 * i] += 1.0; }
    const M3 sx = m3_mul(Qm, m3_inv(Qp));
    x[0] = omega; x[1] = sx.m[7]; x[2] = sx.m[2]; x[3] = sx.m[3];
    if (std::isnan(x[1]) || std::isnan(x[2]) || std::isnan(x[3]) || std::isnan(x[0])) {
        x[0] = -1.0; x[1] = x[2] = x[3] = 0.0;
        return true;
    }
    return false;
}

// write-back of one line (optimization.cc:209-295): the new end points; false = the cluster is dropped
bool cayley_to_segment(const double x[4], const d3& P1_old, const d3& P2_old, d3& P1, d3& P2) {
    const double omega = x[0];
    P1 = P1_old; P2 = P2_old;
    if (!(omega < 0.0 || std::fabs(omega) < kEps)) {
        const double s[3] = {x[1], x[2], x[3]};
        const double nm = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
        const double sk[9] = {0, -s[2], s[1], s[2], 0, -s[0], -s[1], s[0], 0};
        double Q[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                Q[3 * i + j] = 1.0 / (1.0 + nm) * (((1.0 - nm) * (i == j ? 1.0 : 0.0) + 2.0 * sk[3 * i + j]) + (2.0 * s[i]) * s[j]);
        const d3 l{Q[0], Q[3], Q[6]};
        const d3 m{Q[1] * omega, Q[4] * omega, Q[7] * omega};
        if (std::fabs(l.x) > kEps || std::fabs(l.y) > kEps || std::fabs(l.z) > kEps) {
            const d3 Pm = (P1_old + P2_old) * 0.5;
            double x1, x2, x3;
            if (std::fabs(l.x) > std::fabs(l.y) && std::fabs(l.x) > std::fabs(l.z)) {
                x1 = Pm.x;
                x3 = (-m.y - x1 * l.z) / -l.x;
                x2 = (m.z - x1 * l.y) / -l.x;
            } else if (std::fabs(l.y) > std::fabs(l.x) && std::fabs(l.y) > std::fabs(l.z)) {
                x2 = Pm.y;
                x3 = (m.x - x2 * l.z) / -l.y;
                x1 = (m.z + x2 * l.x) / l.y;
            } else {
                x3 = Pm.z;
                x2 = (m.x + x3 * l.y) / l.z;
                x1 = (-m.y + x3 * l.x) / l.z;
            }
            const d3 P{x1, x2, x3};
            P1 = P + l; P2 = P - l;
        }
    }
    return norm(P1 - P2) > kEps;
}

namespace {
size_t up64(size_t b) { return (b + 63) & ~(size_t)63; }
}

// The work order of a launch of k_lineopt over the lines of `order` (indices into res_off, in the caller's order): a
// stable sort by residual count, longest first, so lines of equal count keep the caller's order; the first n_wide (the
// value returned), with more than narrow_max (<= kLoNarrow) residuals, take a wave each, the others a 16-lane group.
// Shared by the line bundling and the refit of §28 (l3d_refit.hip).
uint32_t lo_work_order(const uint32_t* res_off, std::vector<uint32_t>& order, uint32_t narrow_max) {
    auto cnt = [&](uint32_t i) { return res_off[i + 1] - res_off[i]; };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cnt(a) > cnt(b); });
    uint32_t n_wide = 0;
    while (n_wide < order.size() && cnt(order[n_wide]) > narrow_max) ++n_wide;
    return n_wide;
}

// The per-line solves of `order` (indices into x0 / res_off, in the caller's order): the work order (lo_work_order), then
// one packed upload, one launch of k_lineopt and one download through the caller's buffers.  `order` comes back sorted,
// *out points at the results by line index (inside hb; only the lines of `order` are written).  ev: an event pair
// recorded around the launch, or null.
int lo_solve_lines(PinnedBuf<char>& hb, DevBuf<char>& db, hipStream_t stream, hipEvent_t* ev, const std::vector<LoCam>& cams,
                   const std::vector<LoObs>& obs, const std::vector<double>& x0, const std::vector<uint32_t>& res_off,
                   std::vector<uint32_t>& order, uint32_t narrow_max, uint32_t max_iter, uint32_t* n_wide_out, const LoOut** out) {
    const size_t nl = x0.size() / 4;
    const uint32_t n_wide = lo_work_order(res_off.data(), order, narrow_max);
    *n_wide_out = n_wide;
    // one packed upload: cameras | observations | start parameters | CSR | order; then the results
    const size_t o_cam = 0, o_obs = up64(o_cam + cams.size() * sizeof(LoCam)), o_x = up64(o_obs + obs.size() * sizeof(LoObs));
    const size_t o_off = up64(o_x + x0.size() * 8), o_ord = up64(o_off + res_off.size() * 4);
    const size_t in_bytes = o_ord + std::max<size_t>(order.size(), 1) * 4, o_out = up64(in_bytes);
    const size_t total = o_out + nl * sizeof(LoOut);
    if (hb.reserve(total) != hipSuccess || db.reserve(total) != hipSuccess)
        return fail(L3D_ERR_HIP, "line bundling: allocation failed");
    char* h = hb.p;
    if (!cams.empty()) std::memcpy(h + o_cam, cams.data(), cams.size() * sizeof(LoCam));
    if (!obs.empty()) std::memcpy(h + o_obs, obs.data(), obs.size() * sizeof(LoObs));
    std::memcpy(h + o_x, x0.data(), x0.size() * 8);
    std::memcpy(h + o_off, res_off.data(), res_off.size() * 4);
    if (!order.empty()) std::memcpy(h + o_ord, order.data(), order.size() * 4);
    char* d = db.p;
    LoArgs a{(const LoCam*)(d + o_cam), (const LoObs*)(d + o_obs), (const double*)(d + o_x), (const uint32_t*)(d + o_off),
             (const uint32_t*)(d + o_ord), n_wide, (uint32_t)order.size() - n_wide, max_iter, (LoOut*)(d + o_out)};
    hipError_t e = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && ev) e = hipEventRecord(ev[0], stream);
    if (e == hipSuccess) e = launch_lineopt(a, stream);
    if (e == hipSuccess && ev) e = hipEventRecord(ev[1], stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h + o_out, d + o_out, nl * sizeof(LoOut), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(L3D_ERR_HIP, std::string("line bundling: ") + hipGetErrorString(e));
    *out = (const LoOut*)(h + o_out);
    return L3D_OK;
}

// LineOptimizer::optimize on `clusters` (clusters3D_, translated frame; views = views_): parameters, the solves
// (lo_solve_lines), write-back in the original order (dropped clusters leave the list)
int line_opt(::l3d_ctx* c, const std::map<uint32_t, const HostView*>& views, std::vector<ReconCluster>& clusters,
             uint32_t max_iter) {
    l3d_line_opt_summary& st = c->lo_stats;
    st = l3d_line_opt_summary{};
    const size_t nl = clusters.size();
    if (!nl) return L3D_OK;
    // cameras (cam_global2local, :98-135)
    std::map<uint32_t, uint32_t> cam_local;
    std::vector<LoCam> cams;
    for (const auto& kv : views) {
        const HostView& v = *kv.second;
        cam_local[kv.first] = (uint32_t)cams.size();
        LoCam lc;
        for (int k = 0; k < 9; ++k) lc.R[k] = v.R.m[k];
        lc.C[0] = v.C.x; lc.C[1] = v.C.y; lc.C[2] = v.C.z;
        lc.fx = v.K.m[0]; lc.fy = v.K.m[4]; lc.px = v.K.m[2]; lc.py = v.K.m[5];
        cams.push_back(lc);
    }
    // lines (:25-95) and residuals (:137-167)
    std::vector<double> x0(4 * nl);
    std::vector<uint32_t> res_off(nl + 1, 0), order;
    std::vector<LoObs> obs;
    for (size_t i = 0; i < nl; ++i) {
        const ReconCluster& cl = clusters[i];
        if (line_to_cayley(cl.seg.P1, cl.seg.P2, &x0[4 * i])) ++st.lines_constant;
        else order.push_back((uint32_t)i);
        for (const auto& r : cl.residuals) {
            const HostView& v = *views.at(r.first);
            const float* co = &v.segs[4 * (size_t)r.second];
            const double p1x = co[0], p1y = co[1], p2x = co[2], p2y = co[3];
            double dx = p2x - p1x, dy = p2y - p1y;
            const double n = std::sqrt(dx * dx + dy * dy);
            if (n > 0.0) { dx /= n; dy /= n; }
            obs.push_back(LoObs{p1x, p1y, p2x, p2y, -dy, dx, cam_local.at(r.first), 0});
        }
        res_off[i + 1] = (uint32_t)obs.size();
    }
    st.lines_bundled = (uint32_t)order.size();
    st.residuals = (uint32_t)obs.size();
    for (uint32_t i : order) st.max_residuals = std::max(st.max_residuals, res_off[i + 1] - res_off[i]);
    const bool timed = c->timing_level >= 2;
    if (timed && !c->lo_ev[0]) {
        if (hipEventCreate(&c->lo_ev[0]) != hipSuccess || hipEventCreate(&c->lo_ev[1]) != hipSuccess)
            return fail(L3D_ERR_HIP, "line bundling: hipEventCreate failed");
    }
    const LoOut* out = nullptr;
    if (int rc = lo_solve_lines(c->h_lopt, c->d_lopt, c->stream, timed ? c->lo_ev : nullptr, cams, obs, x0, res_off, order,
                                kLoNarrow, max_iter, &st.lines_wide, &out))
        return rc;
    if (timed) st.kernel_ms = ev_ms(c->lo_ev[0], c->lo_ev[1]);
    for (uint32_t i : order) {
        const LoOut& o = out[i];
        switch (o.status) {
            case LO_GRADIENT: ++st.stop_gradient; break;
            case LO_FUNCTION: ++st.stop_function; break;
            case LO_PARAMETER: ++st.stop_parameter; break;
            case LO_MAX_ITER: ++st.stop_max_iter; break;
            default: ++st.stop_other; break;
        }
        st.max_iterations = std::max(st.max_iterations, o.iters);
        if (std::isfinite(o.cost0) && std::isfinite(o.cost1)) { st.cost_before += o.cost0; st.cost_after += o.cost1; }
        for (int j = 0; j < 4; ++j) x0[4 * i + j] = o.x[j];
    }
    // write-back (:209-295)
    std::vector<ReconCluster> kept;
    kept.reserve(nl);
    for (size_t i = 0; i < nl; ++i) {
        d3 P1, P2;
        if (!cayley_to_segment(&x0[4 * i], clusters[i].seg.P1, clusters[i].seg.P2, P1, P2)) { ++st.lines_dropped; continue; }
        kept.push_back(std::move(clusters[i]));
        kept.back().seg = segment3d(P1, P2);
    }
    clusters.swap(kept);
    return L3D_OK;
}

}  // namespace l3d

extern "C" {

int l3d_line_opt_solve(int device, uint32_t n_lines, const double* x0, const uint32_t* res_off, const double* obs,
                       const uint32_t* obs_cam, uint32_t n_cams, const double* cams, uint32_t max_iter, uint32_t narrow_max,
                       double* x_out, double* cost01, uint32_t* iters, uint32_t* status) {
    if (!n_lines) return L3D_OK;
    if (!x0 || !res_off || !x_out || !cost01 || !iters || !status) return fail(L3D_ERR_ARG, "null argument");
    if (narrow_max > kLoNarrow) return fail(L3D_ERR_ARG, "narrow_max above 16");
    if (res_off[0] != 0) return fail(L3D_ERR_ARG, "res_off[0] is not 0");
    for (uint32_t i = 0; i < n_lines; ++i)
        if (res_off[i + 1] < res_off[i]) return fail(L3D_ERR_ARG, "res_off decreases");
    const uint32_t n_res = res_off[n_lines];
    if (n_res && (!obs || !obs_cam || !cams)) return fail(L3D_ERR_ARG, "null argument");
    for (uint32_t r = 0; r < n_res; ++r)
        if (obs_cam[r] >= n_cams) return fail(L3D_ERR_ARG, "observation of a camera >= n_cams");
    if (int rc = set_device(device)) return rc;
    std::vector<LoCam> hc(cams ? n_cams : 0);
    for (size_t i = 0; i < hc.size(); ++i) {
        const double* c = cams + 16 * i;
        for (int k = 0; k < 9; ++k) hc[i].R[k] = c[k];
        for (int k = 0; k < 3; ++k) hc[i].C[k] = c[9 + k];
        hc[i].fx = c[12]; hc[i].fy = c[13]; hc[i].px = c[14]; hc[i].py = c[15];
    }
    std::vector<LoObs> ho(n_res);
    for (uint32_t r = 0; r < n_res; ++r) {
        const double* o = obs + 6 * (size_t)r;
        ho[r] = LoObs{o[0], o[1], o[2], o[3], o[4], o[5], obs_cam[r], 0};
    }
    const std::vector<double> hx(x0, x0 + 4 * (size_t)n_lines);
    const std::vector<uint32_t> hoff(res_off, res_off + (size_t)n_lines + 1);
    std::vector<uint32_t> order(n_lines);
    std::iota(order.begin(), order.end(), 0u);
    PinnedBuf<char> hb; DevBuf<char> db;
    uint32_t n_wide = 0;
    const LoOut* out = nullptr;
    if (int rc = lo_solve_lines(hb, db, 0, nullptr, hc, ho, hx, hoff, order, narrow_max, max_iter, &n_wide, &out)) return rc;
    for (uint32_t i = 0; i < n_lines; ++i) {
        for (int j = 0; j < 4; ++j) x_out[4 * (size_t)i + j] = out[i].x[j];
        cost01[2 * (size_t)i] = out[i].cost0; cost01[2 * (size_t)i + 1] = out[i].cost1;
        iters[i] = out[i].iters; status[i] = out[i].status;
    }
    return L3D_OK;
}

int l3d_line_opt_stats(l3d_ctx* c, l3d_line_opt_summary* out) {
    if (!c || !out) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    *out = c->lo_stats;
    return L3D_OK;
}

int l3d_line_to_cayley(const double P1[3], const double P2[3], double x[4]) {
    if (!P1 || !P2 || !x) return -1;
    return line_to_cayley(d3{P1[0], P1[1], P1[2]}, d3{P2[0], P2[1], P2[2]}, x) ? 1 : 0;
}

int l3d_cayley_to_segment(const double x[4], const double P1_old[3], const double P2_old[3], double P1[3], double P2[3]) {
    if (!x || !P1_old || !P2_old || !P1 || !P2) return -1;
    d3 a, b;
    const bool keep = cayley_to_segment(x, d3{P1_old[0], P1_old[1], P1_old[2]}, d3{P2_old[0], P2_old[1], P2_old[2]}, a, b);
    P1[0] = a.x; P1[1] = a.y; P1[2] = a.z; P2[0] = b.x; P2[1] = b.y; P2[2] = b.z;
    return keep ? 1 : 0;
}

}  // extern "C"
