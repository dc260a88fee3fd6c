// l3d_access.hip -- accessors of the C-ABI: host copies of matches_, estimated_position3D_, A_ / local2global_ and the
// SparseMatrix COO form in the reference's own layouts (commons.h:186-203, segment3D.h:99-115, clustering.h:47-51,
// sparsematrix.cc:8-60), per-view k / median depth, timings.
#include "l3d_ctx.h"
#include "l3d_lsd.h"

using namespace l3d;

extern "C" {

int l3d_synchronize(l3d_ctx* c) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    L3D_HIP_CHECK(hipStreamSynchronize(c->stream));
    return L3D_OK;
}

int l3d_pair_tests(l3d_ctx* c, uint64_t* n) {
    if (!c || !n) return fail(L3D_ERR_ARG, "null argument");
    *n = c->pair_tests;
    return L3D_OK;
}

static int fetch_host_offsets(l3d_ctx* c) {
    if (c->host_offsets_valid) return L3D_OK;
    c->h_surv_off.assign((size_t)c->G + 1, 0);
    c->h_hyp_off.assign((size_t)c->G + 1, 0);
    L3D_HIP_CHECK(hipStreamSynchronize(c->stream));
    L3D_HIP_CHECK(hipMemcpy(c->h_surv_off.data(), c->d_surv_off.p, ((size_t)c->G + 1) * 4, hipMemcpyDeviceToHost));
    L3D_HIP_CHECK(hipMemcpy(c->h_hyp_off.data(), c->d_hyp_off.p, ((size_t)c->G + 1) * 4, hipMemcpyDeviceToHost));
    c->host_offsets_valid = true;
    return L3D_OK;
}

int l3d_get_matches(l3d_ctx* c, uint32_t camID, l3d_match* out, uint64_t cap, uint32_t* seg_offsets, uint64_t* n) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (c->state != l3d_ctx::MATCHED) return fail(L3D_ERR_STATE, "no matches yet");
    auto f = c->views.find(camID);
    if (f == c->views.end()) return fail(L3D_ERR_ARG, "unknown camera ID");
    HostView& v = *f->second;
    (void)hipSetDevice(c->device);
    int rc = fetch_host_offsets(c);
    if (rc) return rc;
    const uint32_t g0 = c->seg_base[v.index], g1 = c->seg_base[v.index + 1];
    const uint32_t base = c->h_surv_off[g0], cnt = c->h_surv_off[g1] - base;
    if (n) *n = cnt;
    if (seg_offsets) for (uint32_t s = 0; s <= v.M; ++s) seg_offsets[s] = c->h_surv_off[g0 + s] - base;
    if (out) {
        const uint64_t m = std::min<uint64_t>(cap, cnt);
        if (m) L3D_HIP_CHECK(hipMemcpy(out, c->d_surv.p + base, m * sizeof(l3d_match), hipMemcpyDeviceToHost));
    }
    return L3D_OK;
}

int l3d_get_pair_slots(l3d_ctx* c, uint32_t pi, l3d_slot* out, uint64_t cap, uint32_t* Ms, uint32_t* K) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (pi >= c->pairs.size() || !c->pair_done[pi]) return fail(L3D_ERR_STATE, "pair not matched");
    const PairDesc& pd = c->pairs[pi];
    if (Ms) *Ms = pd.Ms;
    if (K) *K = pd.K;
    (void)hipSetDevice(c->device);
    if (out) {
        const uint64_t m = std::min<uint64_t>(cap, (uint64_t)pd.Ms * pd.K);
        L3D_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (c->ragged) {
            // ragged rows on the device (keep-all mode, k_keep_assemble): handed out in the padded Ms x K form of this
            // interface -- a row's matches in ascending target order, then empty slots up to the pair's longest row
            std::vector<uint32_t> rs((size_t)pd.Ms + 1);
            L3D_HIP_CHECK(hipMemcpy(rs.data(), c->d_row_start.p + pd.row_off, rs.size() * 4, hipMemcpyDeviceToHost));
            std::vector<l3d_slot> rows(rs[pd.Ms] - rs[0]);
            if (!rows.empty()) L3D_HIP_CHECK(hipMemcpy(rows.data(), c->d_slots.p + rs[0], rows.size() * sizeof(l3d_slot), hipMemcpyDeviceToHost));
            l3d_slot empty{};
            empty.tgt_seg = kEmpty;
            for (uint64_t i = 0; i < m; ++i) {
                const uint32_t r = (uint32_t)(i / pd.K), j = (uint32_t)(i % pd.K);
                out[i] = j < rs[r + 1] - rs[r] ? rows[rs[r] - rs[0] + j] : empty;
            }
            return L3D_OK;
        }
        if (m) L3D_HIP_CHECK(hipMemcpy(out, c->d_slots.p + pd.slot_off, m * sizeof(l3d_slot), hipMemcpyDeviceToHost));
    }
    return L3D_OK;
}

// Test hook (include/l3dpp_hip.h): the layout of a keep-all call's ragged slot buffer as k_keep_pair_info and k_keep_assemble
// left it, copied out as it lies -- stream synchronisation and device-to-host copies only: no kernel, nothing written on the
// device.
int l3d_debug_keep_rows(l3d_ctx* c, int query_only, l3d_keep_rows* out) {
    if (!c || !out) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (c->state == l3d_ctx::IDLE || !c->ragged || c->pairs.empty() || !c->pair_done[0])
        return fail(L3D_ERR_STATE, "l3d_debug_keep_rows: the context's current matches are not ragged");
    const uint32_t R = c->n_rows_total, P = (uint32_t)c->pairs.size();
    const uint64_t S = c->n_slots;
    const uint32_t nb = (uint32_t)((S + kKeepBlock - 1) / kKeepBlock);
    out->n_rows = R; out->n_pairs = P; out->n_blocks = nb; out->keep_cap = c->keep_cap;
    out->tgt16 = c->tgt16; out->reserved = 0; out->n_slots = S;
    if (query_only) return L3D_OK;
    (void)hipSetDevice(c->device);
    L3D_HIP_CHECK(hipStreamSynchronize(c->stream));
    auto fetch = [](void* dst, const void* src, size_t bytes) -> hipError_t {
        return dst && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    };
    L3D_HIP_CHECK(fetch(out->row_start, c->d_row_start.p, ((size_t)R + 1) * 4));
    L3D_HIP_CHECK(fetch(out->row_pair, c->d_row_pair.p, (size_t)R * 4));
    L3D_HIP_CHECK(fetch(out->blk_row, c->d_blk_row.p, (size_t)nb * 4));
    L3D_HIP_CHECK(fetch(out->pair_info, c->d_keep_info.p, (size_t)P * sizeof(uint4)));
    L3D_HIP_CHECK(fetch(out->slot_row, c->d_slot_row.p, (size_t)S * 4));
    if (out->inv_tgt && S) {
        if (c->tgt16) {
            std::vector<uint16_t> t16(S);
            L3D_HIP_CHECK(fetch(t16.data(), c->d_inv_tgt.p, (size_t)S * 2));
            for (uint64_t i = 0; i < S; ++i) out->inv_tgt[i] = t16[i] == 0xFFFFu ? kEmpty : t16[i];
        } else L3D_HIP_CHECK(fetch(out->inv_tgt, c->d_inv_tgt.p, (size_t)S * 4));
    }
    return L3D_OK;
}

// Test hooks of the epipolar-band culling (include/l3dpp_hip.h): make_cull as l3d_match_begin calls it, and the
// tables k_cull_prepare wrote for a pair of the last launch -- copies only, no kernel.
int l3d_cull_forms(const double F[9], double ws, double hs, double wt, double ht, l3d_cull_forms_info* out) {
    if (!F || !out) return fail(L3D_ERR_ARG, "null argument");
    PairCull pc{};
    make_cull(F, ws, hs, wt, ht, pc);
    *out = l3d_cull_forms_info{};
    out->enabled = pc.enabled;
    if (pc.enabled) { std::memcpy(out->As, pc.As, 24); std::memcpy(out->Bs, pc.Bs, 24); std::memcpy(out->At, pc.At, 24); std::memcpy(out->Bt, pc.Bt, 24); }
    return L3D_OK;
}

int l3d_debug_cull(l3d_ctx* c, uint32_t pair, int query_only, l3d_cull_state* out) {
    if (!c || !out) return fail(L3D_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const auto& cl = c->cull_launch;
    if (c->state != l3d_ctx::BEGUN || !cl.valid || pair < cl.first || pair - cl.first >= cl.count || pair >= c->cull.size())
        return fail(L3D_ERR_STATE, "l3d_debug_cull: not a pair of the last launch of an open call");
    PairCull pc = c->cull[pair];
    if (!cl.culled) pc.enabled = 0;   // (brute-force hook, or no pair of the launch suited: k_cull_prepare did not run)
    const PairDesc& pd = c->pairs[pair];
    out->enabled = pc.enabled; out->layout_rows = cl.layout; out->Ms = pd.Ms; out->Mt = pd.Mt;
    out->src_len = pc.enabled ? (cl.layout ? tile_src_cap(pd.Ms, cl.layout) : pd.Ms) : 0u;
    out->n_chunks = pc.enabled ? (pd.Mt + 63) / 64 : 0u;
    std::memset(out->As, 0, 4 * 24);
    if (pc.enabled) { std::memcpy(out->As, pc.As, 24); std::memcpy(out->Bs, pc.Bs, 24); std::memcpy(out->At, pc.At, 24); std::memcpy(out->Bt, pc.Bt, 24); }
    if (query_only || !pc.enabled) return L3D_OK;
    (void)hipSetDevice(c->device);
    L3D_HIP_CHECK(hipStreamSynchronize(c->stream));
    auto fetch = [](void* dst, const void* src, size_t bytes) -> hipError_t {
        return dst && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    };
    L3D_HIP_CHECK(fetch(out->src_perm, c->d_src_perm.p + pc.s_off, (size_t)out->src_len * 4));
    L3D_HIP_CHECK(fetch(out->src_band, c->d_src_band.p + pc.s_off, (size_t)out->src_len * 8));
    L3D_HIP_CHECK(fetch(out->tgt_perm, c->d_tgt_perm.p + pc.t_off, (size_t)pd.Mt * 4));
    L3D_HIP_CHECK(fetch(out->tgt_band, c->d_tgt_band.p + pc.t_off, (size_t)pd.Mt * 8));
    L3D_HIP_CHECK(fetch(out->chunk_band, c->d_chunk_band.p + pc.c_off, (size_t)out->n_chunks * 8));
    return L3D_OK;
}

int l3d_num_best(l3d_ctx* c, uint32_t* n) {
    if (!c || !n) return fail(L3D_ERR_ARG, "null argument");
    *n = c->state == l3d_ctx::MATCHED ? c->n_hyps : 0;
    return L3D_OK;
}

int l3d_get_best(l3d_ctx* c, l3d_segment2d* seg2d, l3d_segment3d* seg3d, l3d_match* best) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (c->state != l3d_ctx::MATCHED) return fail(L3D_ERR_STATE, "no matches yet");
    (void)hipSetDevice(c->device);
    std::vector<HypRec> h(c->n_hyps);
    if (c->n_hyps) L3D_HIP_CHECK(hipMemcpy(h.data(), c->d_hyps.p, h.size() * sizeof(HypRec), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i) {
        if (seg2d) { seg2d[i].camID_ = h[i].m.src_cam; seg2d[i].segID_ = h[i].m.src_seg; }
        if (seg3d) {
            std::memcpy(seg3d[i].P1, h[i].P1, 24); std::memcpy(seg3d[i].P2, h[i].P2, 24);
            std::memcpy(seg3d[i].dir, h[i].dir, 24);
            seg3d[i].length_ = h[i].length; seg3d[i].valid_ = h[i].valid;
        }
        if (best) std::memcpy(&best[i], &h[i].m, sizeof(l3d_match));
    }
    return L3D_OK;
}

int l3d_view_info(l3d_ctx* c, uint32_t camID, float* k, float* median_depth) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    auto f = c->views.find(camID);
    if (f == c->views.end()) return fail(L3D_ERR_ARG, "unknown camera ID");
    if (k) *k = f->second->k;
    if (median_depth) *median_depth = f->second->median_depth;
    return L3D_OK;
}

int l3d_translation(l3d_ctx* c, double t[3]) {
    if (!c || !t) return fail(L3D_ERR_ARG, "null argument");
    t[0] = c->translation.x; t[1] = c->translation.y; t[2] = c->translation.z;
    return L3D_OK;
}

int l3d_num_affinity(l3d_ctx* c, uint32_t* n_edges, uint32_t* n_rows) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (!c->affinity_done) return fail(L3D_ERR_STATE, "l3d_compute_affinity has not run");
    if (n_edges) *n_edges = c->aff_n_edges;
    if (n_rows) *n_rows = c->aff_n_rows;
    return L3D_OK;
}

int l3d_get_affinity(l3d_ctx* c, l3d_cledge* edges, l3d_segment2d* l2g, float* msdl) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (!c->affinity_done) return fail(L3D_ERR_STATE, "l3d_compute_affinity has not run");
    { std::lock_guard<std::recursive_mutex> lk(c->mu); const int rc = ensure_affinity_host(c); if (rc) return rc; }
    if (edges && !c->edges.empty()) std::memcpy(edges, c->edges.data(), c->edges.size() * sizeof(l3d_cledge));
    if (l2g && !c->l2g.empty()) std::memcpy(l2g, c->l2g.data(), c->l2g.size() * sizeof(l3d_segment2d));
    if (msdl) *msdl = c->med_scene_depth_lines;
    return L3D_OK;
}

// SparseMatrix::SparseMatrix(entries, n, 1.0f, sort_by_row), sparsematrix.cc:8-60.  std::list::sort is
// stable, so equal keys keep A_'s order.
int l3d_get_sparse_matrix(l3d_ctx* c, int sort_by_row, l3d_float4* entries, int32_t* start_indices) {
    if (!c) return fail(L3D_ERR_ARG, "null argument");
    if (!c->affinity_done) return fail(L3D_ERR_STATE, "l3d_compute_affinity has not run");
    { std::lock_guard<std::recursive_mutex> lk(c->mu); const int rc = ensure_affinity_host(c); if (rc) return rc; }
    std::vector<l3d_cledge> e = c->edges;
    if (sort_by_row)
        std::stable_sort(e.begin(), e.end(), [](const l3d_cledge& a, const l3d_cledge& b) {
            return a.i_ < b.i_ || (a.i_ == b.i_ && a.j_ < b.j_); });   // sortCLEdgesByRow, clustering.h
    else
        std::stable_sort(e.begin(), e.end(), [](const l3d_cledge& a, const l3d_cledge& b) {
            return a.j_ < b.j_ || (a.j_ == b.j_ && a.i_ < b.i_); });   // sortCLEdgesByCol
    if (start_indices) for (size_t i = 0; i < c->l2g.size(); ++i) start_indices[i] = -1;
    int cur = -1;
    for (size_t pos = 0; pos < e.size(); ++pos) {
        if (entries) entries[pos] = l3d_float4{(float)e[pos].i_, (float)e[pos].j_, e[pos].w_, 0.0f};
        const int rc = sort_by_row ? e[pos].i_ : e[pos].j_;
        if (rc != cur) { if (start_indices) start_indices[rc] = (int)pos; cur = rc; }
    }
    return L3D_OK;
}

// test hook: process-wide counters that let a test see WHICH form of a kernel ran (the global-cursor form
// of k_pair_csr was selected by an environment variable that had been latched before the test set it)
unsigned long long l3d_debug_counter(const char* name) {
    if (name && std::string(name) == "csr_global_launches") return g_csr_global_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "knn_replay_calls") return g_knn_replay_calls.load(std::memory_order_relaxed);
    if (name && std::string(name) == "keep_all_repeats") return g_keep_all_repeats.load(std::memory_order_relaxed);
    if (name && std::string(name) == "lsd_images_detected") return g_lsd_images_detected.load(std::memory_order_relaxed);
    if (name && std::string(name) == "lsd_cache_loads") return g_lsd_cache_loads.load(std::memory_order_relaxed);
    if (name && std::string(name) == "associate_launches") return g_assoc_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "associate_kernel_ns") return g_assoc_kernel_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "compare_launches") return g_cmp_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "compare_merge_launches") return g_cmp_merge_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "compare_slices") return g_cmp_slices.load(std::memory_order_relaxed);
    if (name && std::string(name) == "compare_kernel_ns") return g_cmp_kernel_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "merge_count_launches") return g_mrg_count_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "merge_write_launches") return g_mrg_write_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "merge_slices") return g_mrg_slices.load(std::memory_order_relaxed);
    if (name && std::string(name) == "merge_pairs") return g_mrg_pairs.load(std::memory_order_relaxed);
    if (name && std::string(name) == "merge_kernel_ns") return g_mrg_kernel_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "align_iterations") return g_aln_iterations.load(std::memory_order_relaxed);
    if (name && std::string(name) == "align_normal_launches") return g_aln_normal_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "align_kernel_ns") return g_aln_kernel_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "pose_iterations") return g_pose_iterations.load(std::memory_order_relaxed);
    if (name && std::string(name) == "pose_normal_launches") return g_pose_normal_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "pose_kernel_ns") return g_pose_kernel_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "refit_observations") return g_refit_observations.load(std::memory_order_relaxed);
    if (name && std::string(name) == "refit_lines_solved") return g_refit_lines_solved.load(std::memory_order_relaxed);
    if (name && std::string(name) == "refit_kernel_ns") return g_refit_kernel_ns.load(std::memory_order_relaxed);
    {
        // the parts of refit_kernel_ns: projection + association, observation list, k_refit_obs, k_lineopt, k_refit_spans
        static const char* const kParts[5] = {"refit_associate_ns", "refit_list_ns", "refit_obs_ns", "refit_lineopt_ns", "refit_spans_ns"};
        for (int k = 0; k < 5; ++k)
            if (name && std::string(name) == kParts[k]) return g_refit_part_ns[k].load(std::memory_order_relaxed);
    }
    if (name && std::string(name) == "bundle_iterations") return g_bundle_iterations.load(std::memory_order_relaxed);
    if (name && std::string(name) == "bundle_rejected_steps") return g_bundle_rejected_steps.load(std::memory_order_relaxed);
    if (name && std::string(name) == "bundle_kernel_ns") return g_bundle_kernel_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "wf_count_launches") return g_wf_count_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "wf_write_launches") return g_wf_write_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "wf_slices") return g_wf_slices.load(std::memory_order_relaxed);
    if (name && std::string(name) == "wf_junctions") return g_wf_junctions.load(std::memory_order_relaxed);
    if (name && std::string(name) == "wf_skipped_blocks") return g_wf_skipped_blocks.load(std::memory_order_relaxed);
    if (name && std::string(name) == "wf_kernel_ns") return g_wf_kernel_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "wf_count_ns") return g_wf_count_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "pl_score_launches") return g_pl_score_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "pl_slices") return g_pl_slices.load(std::memory_order_relaxed);
    if (name && std::string(name) == "pl_hypotheses") return g_pl_hypotheses.load(std::memory_order_relaxed);
    if (name && std::string(name) == "pl_kernel_ns") return g_pl_kernel_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "pl_junction_ns") return g_pl_junction_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "dir_score_launches") return g_dir_score_launches.load(std::memory_order_relaxed);
    if (name && std::string(name) == "dir_slices") return g_dir_slices.load(std::memory_order_relaxed);
    if (name && std::string(name) == "dir_hypotheses") return g_dir_hypotheses.load(std::memory_order_relaxed);
    if (name && std::string(name) == "dir_kernel_ns") return g_dir_kernel_ns.load(std::memory_order_relaxed);
    if (name && std::string(name) == "live_device_blocks") return g_live_blocks[0].load(std::memory_order_relaxed);
    if (name && std::string(name) == "live_pinned_blocks") return g_live_blocks[1].load(std::memory_order_relaxed);
    static const char* const kSeamSupport[4] = {"seam_support_wave_lists", "seam_support_group_staged_lists",
                                                "seam_support_sort_only_lists", "seam_support_all_pairs_lists"};
    for (int i = 0; i < 4; ++i)
        if (name && std::string(name) == kSeamSupport[i]) return g_seam_support_lists[i].load(std::memory_order_relaxed);
    for (uint32_t i = 0; i < kLcCount; ++i)
        if (name && std::string(name) == kListCounterNames[i]) return g_list_counters[i].load(std::memory_order_relaxed);
    if (name && std::string(name) == "seam_score_unstaged_lists") return g_seam_score_unstaged_lists.load(std::memory_order_relaxed);
    static const char* const kMatchTiers[kMatchTierCount + 1] = {"match_tile_launches", "match_row2_launches", "match_row2_cached_launches",
                                                                 "match_row1_launches", "match_ix32_launches"};
    for (uint32_t i = 0; i <= kMatchTierCount; ++i)
        if (name && std::string(name) == kMatchTiers[i]) return g_match_tier_launches[i].load(std::memory_order_relaxed);
    if (name && std::string(name) == "match_order_launches") return g_match_order_launches.load(std::memory_order_relaxed);
    return ~0ull;
}

// test hook (host only): the form a bounded-kNN launch takes and what l3d_match_begin decides for its call, from the
// very functions run_match_kernel and match_begin_body call (k_match.hip)
int l3d_match_plan(uint64_t total_items, uint32_t launch_items, uint32_t kNN, uint32_t max_target_segments, uint32_t tile_rows,
                   l3d_match_plan_info* out) {
    if (!out || (tile_rows != 0 && tile_rows != 16) || !launch_items || launch_items > total_items || !kNN)
        return fail(L3D_ERR_ARG, "l3d_match_plan: tile_rows 0 or 16, 1 <= launch_items <= total_items, kNN >= 1");
    const MatchPlan p = match_launch_plan(0, false, launch_items, kNN, max_target_segments, tile_rows);
    out->tier = (uint32_t)p.tier; out->waves = p.waves; out->row_cache = p.row_cache ? 1u : 0u; out->ix16 = p.ix16 ? 1u : 0u;
    out->lds_bytes = p.lds;
    out->replay = match_knn_replay(false, kNN, max_target_segments, total_items, tile_rows) ? 1u : 0u;
    out->launch_accepted = p.fits() ? 1u : 0u;   // (run_match_kernel refuses the launch otherwise: L3D_ERR_LIMIT)
    return L3D_OK;
}

uint32_t l3d_match_tile_rows(uint64_t est_row_items) { return match_tile_rows(0, false, est_row_items); }

int l3d_set_timing_level(l3d_ctx* c, int level) {
    if (!c || level < 0 || level > 2) return fail(L3D_ERR_ARG, "l3d_set_timing_level: level 0, 1 or 2");
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    c->timing_level = level;
    return L3D_OK;
}

int l3d_get_timings(l3d_ctx* c, l3d_timings* t) {
    if (!c || !t) return fail(L3D_ERR_ARG, "null argument");
    *t = c->tm;   // (nothing here waits for the GPU: tied_rows arrives with the read-back of l3d_match_finish)
    return L3D_OK;
}

}  // extern "C"
