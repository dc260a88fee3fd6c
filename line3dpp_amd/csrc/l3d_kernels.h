// l3d_kernels.h -- launch prototypes shared by the .hip translation units of libl3dpp_hip.so
#pragma once
#include <atomic>

#include "l3d_dev.h"

struct l3d_cledge;

namespace l3d {

extern std::atomic<uint64_t> g_knn_replay_calls;      // l3d_api.hip
extern std::atomic<uint64_t> g_keep_all_repeats;      // l3d_api.hip
extern std::atomic<uint64_t> g_live_blocks[2];        // l3d_api.hip
extern std::atomic<uint64_t> g_csr_global_launches;   // k_lists.hip, test hook read through l3d_debug_counter
// l3d_phase_b.hip, test hooks: which forms of the list pass ran (names: kListCounterNames, same order)
enum ListCounter : uint32_t { kLcTier2Lists = 0, kLcTier4Lists, kLcHugeLists, kLcWidePasses, kLcNarrowPasses, kLcTierRepeats,
                              kLcHugeScratchRegrows, kLcEdgesGlobalSegments, kLcCandPoolRegrows, kLcEdgePoolRegrows, kLcCount };
extern std::atomic<uint64_t> g_list_counters[kLcCount];
extern const char* const kListCounterNames[kLcCount];
// l3d_seam.hip, test hooks: lists l3d_score_matches sent down each path of k_support / k_score_all (k_views.hip)
extern std::atomic<uint64_t> g_seam_support_lists[4];  // indexed by SupportTier - 1
extern std::atomic<uint64_t> g_seam_score_unstaged_lists;
enum SupportTier : uint32_t { kSupportNone = 0, kSupportWave, kSupportGroupStaged, kSupportSortOnly, kSupportAllPairs };
struct ListTier { SupportTier support; bool score_unstaged; };
ListTier list_tier(uint32_t L);   // k_views.hip, next to the limits it is derived from

constexpr int kMatchRows = 64;   // source rows per work item of k_match_pairs (one wave64): the ROW form (keep-all modes, brute-force
                                 // hook, the accelerator seam, L3D_MATCH_TILE=0)
// The TILE form of the bounded-kNN kernel (round 5): a work item is R = 16 or 32 source rows of ONE width class, a lane is
// a (row, target) pair -- 64 / R targets per step -- and the targets come out of an LDS FIFO of the records whose band
// meets the hull of the R rows (k_match.hip).  k_cull_prepare lays the rows of a pair out class by class, every class
// padded to a multiple of R (kEmpty rows), in a region of tile_src_cap(Ms, R) positions: the host's work list is that
// region cut into items of R positions, whatever the class sizes turn out to be on the device.
constexpr uint32_t kTileClasses = 5;   // unbounded band | width beyond 1/16, 1/32, 1/64 of the target image | narrow
// Width classes only pay where a class is cut into enough items: a view of 1000 segments (C3) has 16 items of 64 rows per
// pair, and splitting them into classes that each end in a partially filled item cost its match kernel 10 % (3.11 against
// 2.81 ms), while C1's 31 items gain.  Below 24 items per pair: the unbounded rows and ONE class of bounded rows.
constexpr uint32_t kTileMinItems = 24;
__host__ __device__ constexpr uint32_t tile_classes(uint32_t Ms, uint32_t R) { return Ms / R < kTileMinItems ? 2u : kTileClasses; }
__host__ __device__ constexpr uint32_t tile_src_cap(uint32_t Ms, uint32_t R) {
    return ((Ms + tile_classes(Ms, R) * (R - 1) + R - 1) / R) * R;
}
constexpr uint64_t kMatchTileMaxItems = 2048;     // launches of up to this many 64-row items take the tile form (C0: 1 430 items,
                                                  // kernel -7 %; C1's 10 560 and C3's 81 920 lose 20 % in it)
uint32_t match_tile_rows(int mode, bool brute, uint64_t est_row_items);   // 0: row form; 16: tile form (L3D_MATCH_TILE overrides)
uint32_t match_layout_rows(int mode, bool brute, uint32_t tile_rows); // rows per work item of the padded class layout: the tile form's R, 64 for the
                                                  // row form, 0 for the keep-all passes and the brute-force hook (legacy layout)
struct WorkItem {
    uint32_t pair;  // index into the pair array
    uint32_t src0;  // first source row (position in the pair's row order) of the work item
};

// Epipolar-band culling (k_match.hip): per directed pair, the pencil of epipolar lines in the target image
// is parametrised by tau = (A.x)/(B.x), the coordinate at which the pencil line through x crosses a fixed
// transversal through the image centre.  Source rows and target segments are ordered by tau so that a wave
// can skip whole 64-segment chunks of targets whose tau band cannot meet the bands of its rows.
struct PairCull {
    double As[3], Bs[3];   // tau of the epipolar line F*p of a source point p: (As.p)/(Bs.p), Bs.centre == 1
    double At[3], Bt[3];   // tau of a target point / direction q: (At.q)/(Bt.q), Bt.centre == 1
    uint64_t s_off;        // first entry of this pair in the source pools
    uint64_t t_off;        // first entry in the target pools
    uint32_t c_off;        // first chunk band
    uint32_t enabled;      // 0: geometry not suited (epipole in/near the image, degenerate F) -> plain streaming
    uint64_t k_off;        // views beyond the LDS sort capacity: this pair's sort keys in CullPools::big_keys (source
                           // side first, target side behind it); ~0 when both sides sort in LDS
    uint32_t w_item0;      // first work item (64 source rows each) of the pair, counted over all pairs of the context
    uint32_t sorted_copy;  // 1: k_cull_prepare also keeps the target's seg4 / SegD records in walk order (CullPools::tgt_s4 /
                           // tgt_sd) and the exact tests read those.  For views of a few thousand segments the per-view arrays
                           // stay in the L2s across the pairs of a view and gathers by original index hit; per-pair copies
                           // would only add traffic (C1: +30 % bytes for nothing).  From 4096 segments on the gathers miss
                           // (C4 read 132 x its segment records) and the copies pay.
};
constexpr uint32_t kSortedCopyMinSegs = 4096;
struct CullPools {
    const PairCull* cull;      // [n_pairs] or nullptr
    uint32_t* src_perm;        // [sum Ms] source row visited at sorted position i (tile form: [sum tile_src_cap], kEmpty = padding)
    float2* src_band;          // [sum Ms] its tau band (lo, hi)
    uint32_t* tgt_perm;        // [sum Mt] target segment at sorted position i
    float4* tgt_sf;            // [sum Mt] SegF records in sorted order
    float2* tgt_band;          // [sum Mt] their tau bands
    float2* chunk_band;        // [sum ceil(Mt/64)] tau band of each 64-record chunk
    uint64_t* big_keys;        // global sort scratch of the pairs whose views exceed kCullLdsSegs
    // longest-first order of the work items of a launch (nullptr: launch order = list order), see k_order_items
    uint32_t* item_bucket;     // [items of the launch] length class of each item
    uint32_t* item_order;      // [items of the launch] work item started by workgroup b
    uint32_t* order_done;      // workgroups of k_order_items that have filed their items (zero between launches)
    uint32_t w_base;           // PairCull::w_item0 of the first pair of the launch
    uint32_t cost_max;         // largest Mt of the launch
    // what the exact tests read of a target, in sorted order as well (the candidates of a wave are neighbours in that
    // order: gathers by original index miss the L2s on large views -- C4 read 132 x its segment records)
    float4* tgt_s4;            // [sum Mt] raw segments (x1,y1,x2,y2)
    SegD32* tgt_sd;            // [sum Mt] rays and plane normal in float (the depth decision's share of SegX, l3d_dev.h SegD32)
    uint32_t row_cache;        // set by launch_match_pairs: the work items stage their source rows' records in LDS
    uint32_t padded_rows;      // 0: src_perm / src_band hold Ms rows per pair (row form, legacy classes); R: the padded class layout
                               // of tile_src_cap(Ms, R) positions per pair (tile form: R = 16 / 32; row form with classes: 64)
};
constexpr uint32_t kOrderBuckets = 1024;
constexpr uint32_t kCullLdsSegs = 16384;   // LDS sort capacity of k_cull_prepare (larger views sort in global memory)
constexpr uint32_t kCullBandCacheSegs = 4096;   // ... sides of up to this many elements keep their bands in LDS (8 bytes each)
constexpr uint32_t kCullMaxSegs = 1u << 20; // 20 index bits in the sort keys beside class and band

// the orientation filter of phase B fused into whatever produces a slot (match epilogue, exchange expansion)
struct OrientFuse {
    uint32_t* inv_tgt;              // [n_slots] target segment of a slot that hands an inverse match to its target view
                                    // (kSlotInvAlive), kEmpty otherwise: the stream k_pair_csr sorts by target
    uint32_t tgt16;                 // 1: the stream holds 16-bit entries (0xFFFF: none) -- every view of the scene has fewer
                                    // than 65 535 segments: half the bytes the epilogue writes and k_pair_csr reads twice
    OrientThr thr;
    // rows in which the match kernel saw equal overlaps (the reference's heap order decides there): (pair, source row),
    // replayed by k_match_tied_rows
    uint32_t* tie_count;            // rows queued by this match launch
    uint2* tie_list;
    uint32_t tie_cap;
    uint32_t* tie_next;             // the counter the next match launch will use (zeroed by k_match_tied_rows)
    uint32_t* tie_total;            // rows replayed so far (diagnostics)
    // The compact hypothesis streams of phase B (round 6), written beside the slots by whatever produces a slot (nullptr: not
    // kept -- the accelerator seam): the list pass of phase B reads 8 bytes per slot where it read the 32-byte record for 8.
    float2* hyp_p;                  // [n_slots] (depth_p1, depth_p2) of an ALIVE slot (kSlotAlive), NaN otherwise: the fresh
                                    // hypotheses of the source segment
    float2* hyp_q;                  // [n_slots] (depth_q1, depth_q2): the depths of a slot's INVERSE hypothesis (read where
                                    // inv_tgt names a target); k_pair_csr carries them into the sorted order of its records
    // keep-all mode (kNN <= 0), single culled pass (round 6): the count pass leaves every accepted match of row r at
    // keep_rec[(row_off + r) * keep_cap + arrival index] as a whole 32-byte slot (flags 0: k_keep_assemble sets them and puts
    // the rows into ascending target order)
    Slot* keep_rec;                 // nullptr: counts only (the legacy two-pass form)
    uint32_t keep_cap;              // records kept per row (a longer row: the pass is repeated with a larger scratch)
    uint32_t* slot_row;             // [n_slots] source segment of a slot (ragged rows), written by k_keep_assemble
};

// ---- k_match.hip ----
size_t match_lds_bytes(int mode, uint32_t K, bool ix16 = false, uint32_t waves = 1, bool brute = false, uint32_t tile_rows = 0,
                       bool row_cache = false);
bool match_row_cache(int mode, bool brute, uint32_t nwork, uint32_t tile_rows);   // the source rows' records staged in LDS (k_match.hip)
constexpr uint32_t kMatchOrderMaxItems = 16384;   // launches up to this many work items: two waves per item
constexpr uint32_t kMatchOrderMinItems = 3584;    // ... and, from this many on (more waves than wave slots), longest-first order
uint32_t match_waves_per_group(int mode, bool brute, uint32_t nwork);   // waves that share one 64-row work item of k_match_pairs
// The form a launch of k_match_pairs takes, from the functions above: what run_match_kernel checks before it
// launches, what the replay decision of l3d_match_begin is taken from, and what l3d_match_plan shows to the tests.
constexpr size_t kMatchLdsLimit = 160 * 1024;     // LDS of a CU: the top-K tables of a work item must fit
enum MatchTier : uint32_t { kMatchTierTile = 0, kMatchTierRow2, kMatchTierRow2Cached, kMatchTierRow1, kMatchTierCount };
struct MatchPlan { MatchTier tier; uint32_t waves; bool row_cache; bool ix16; size_t lds; bool fits() const { return lds <= kMatchLdsLimit; } };
// nwork: items of the launch; K, max_Mt: largest kNN and largest target view of its pairs
MatchPlan match_launch_plan(int mode, bool brute, uint32_t nwork, uint32_t K, uint32_t max_Mt, uint32_t tile_rows);
// l3d_match_begin: true when some launch l3d_match_pairs can make of a call of total_items work items -- any range of its pair
// list, i.e. any item count up to total_items -- would not fit the LDS: every row of the call then takes the exact replay
bool match_knn_replay(bool brute, uint32_t K, uint32_t max_Mt, uint64_t total_items, uint32_t tile_rows);
// test hooks (l3d_debug_counter): launches of the staged bounded-kNN kernel per tier ([kMatchTierCount]: those with 32-bit
// table indices), launches of k_order_items
extern std::atomic<uint64_t> g_match_tier_launches[kMatchTierCount + 1];
extern std::atomic<uint64_t> g_match_order_launches;
hipError_t launch_cull_prepare(const ViewDev* views, const PairDesc* pairs, uint32_t first, uint32_t count,
                               uint32_t max_M, CullPools pools, uint32_t tile_rows, hipStream_t stream);
hipError_t launch_order_items(const PairDesc* pairs, uint32_t first, uint32_t count, uint32_t max_Mt, CullPools pools,
                              uint32_t nwork, hipStream_t stream);
hipError_t launch_match_pairs(int mode, bool brute, const ViewDev* views, const PairDesc* pairs,
                              const WorkItem* work, uint32_t nwork, uint32_t maxK, Slot* slots,
                              uint32_t* row_counts, float thr, CullPools pools, OrientFuse of, bool ix16,
                              uint32_t tile_rows, hipStream_t stream);
// rows flagged by the match kernel (equal overlaps): the reference's priority_queue order, replayed; scratch = one
// region of 2 * scratch_stride (stride >= max Mt) packed entries per workgroup of match_tied_grid(stride); cp: the culling pools of the
// match launch (cp.cull == nullptr: every target is visited)
uint32_t match_tied_grid(uint32_t scratch_stride);
// kNN beyond the LDS tables of k_match_pairs: every row of the pairs [first, first + count) is queued for
// k_match_tied_rows instead (list_base = PairDesc::row_off of pair `first`)
hipError_t launch_queue_all_rows(const PairDesc* pairs, uint32_t first, uint32_t count, uint32_t max_Ms, uint32_t list_base,
                                 OrientFuse of, hipStream_t stream);
hipError_t launch_match_tied_rows(const ViewDev* views, const PairDesc* pairs, Slot* slots, uint32_t maxK, float thr,
                                  OrientFuse of, CullPools cp, uint64_t* scratch, uint32_t scratch_stride,
                                  hipStream_t stream);
// compact exchange of slots between ranks: target indices out, full records back (bit-identical re-derivation)
hipError_t launch_pack_slot_idx(const Slot* slots, uint32_t* idx, uint64_t lo, uint64_t hi, hipStream_t stream);
hipError_t launch_expand_slot_idx(const ViewDev* views, const PairDesc* pairs, uint32_t first, uint32_t count,
                                  uint32_t max_row_slots, const uint32_t* idx, Slot* slots, OrientFuse of,
                                  hipStream_t stream);
// keep-all mode (kNN <= 0), after the count pass that kept its records (OrientFuse::keep_rec) and the scan of the row counts
// info[p] = {first slot, longest row, slots lo, slots hi}; row_pair[row] = its pair; blk_row[b] = the row that holds slot b * kKeepBlock
constexpr uint32_t kKeepBlock = 1024;
hipError_t launch_keep_pair_info(const PairDesc* pairs, uint32_t n_pairs, const uint32_t* row_counts, const uint32_t* row_start,
                                 uint4* info, uint32_t* row_pair, uint32_t* blk_row, uint32_t n_blk, uint32_t* longest, hipStream_t stream);   // *longest: the longest row of all
// (slot_cap: capacity of the output arrays -- the number of slots is read on the device, a pass with more writes nothing)
hipError_t launch_keep_assemble(const ViewDev* views, const PairDesc* pairs, uint32_t n_rows, uint64_t slot_cap, const uint32_t* row_start,
                                const uint32_t* row_pair, const uint32_t* blk_row, const uint32_t* longest, Slot* slots, OrientFuse of,
                                hipStream_t stream);
// per-segment invariants of all views
hipError_t launch_prep_views(const ViewDev* views, uint32_t n_views, uint32_t max_M, hipStream_t stream);

// ---- k_lists.hip: the sparse phase B (l3d_lists.h) ----
struct InvRec; struct ListPools; struct PairCsr;
constexpr uint32_t kWideMeanList = 96;      // a pass whose mean list length lies above stages 256 hypotheses per wave, else 128
constexpr uint32_t kFlagEdgesGlobal = 8;    // word of the pass' flag block: segments whose candidates k_edges walked in global memory
struct HugeScratchArgs { float* f32; uint32_t* u32; uint64_t* u64; uint32_t cap; uint32_t mean_list; uint32_t run_huge; uint32_t run_tier4; };   // [2 cap] [3 cap] [cap]; mean list length (estimate); which of the rarely needed tiers are launched
hipError_t launch_scan64(const unsigned long long* in, uint32_t n, unsigned long long* out, unsigned long long* tmp,
                         unsigned long long* total, hipStream_t st);
// the inverse hypotheses of every pair that hands matches to a later view, sorted by target segment (counting sort per
// pair, one workgroup each): poff = per-pair CSR offsets over the target's segments, refs = the slot indices in that order
hipError_t launch_pair_csr(const PairDesc* pairs, uint32_t n_pairs, uint32_t max_Mt, const PairCsr* pair_csr,
                           const uint32_t* inv_tgt, uint32_t tgt16, uint32_t* poff, uint32_t* refs,
                           uint32_t* dummy, uint32_t tgt_v0, uint32_t tgt_v1, uint64_t max_pair_slots,
                           const uint32_t* row_start, hipStream_t st);   // row_start: ragged rows (l3d_lists.h), else nullptr
hipError_t launch_seg_index(ListPools lp, uint32_t* seg_of_g, uint32_t G, uint32_t world, hipStream_t st);
struct ListView; struct OutPair; struct InPair;
hipError_t launch_lists(uint32_t v0, uint32_t nv, uint32_t max_M, const ViewDev* views, const PairDesc* pairs,
                        const ListView* lviews, const OutPair* opairs, const InPair* ipairs, const uint32_t* gseg_view,
                        const uint32_t* poff, const uint32_t* inv_refs, const float2* hyp_p, const float2* hyp_q,
                        const Slot* slots, uint32_t uniform_K,
                        SimConst sc, ListPools lp, uint32_t* seg_of_g, HugeScratchArgs hsa, hipStream_t st);
hipError_t launch_chain_sweep(ListPools lp, uint8_t* positive, uint32_t* changed, uint32_t sweep, uint32_t* undecided,
                              hipStream_t st);   // sweep 0: all headers of lp, files the undecided ones per pool; later sweeps: those lists
hipError_t launch_hyp_scores(ListPools lp, const uint8_t* positive, const uint32_t* gseg_view, Slot* slots,
                             const uint8_t* pair_present, uint32_t* max_score_bits, hipStream_t st);
hipError_t launch_hyp_filter(ListPools lp, uint32_t g0, uint32_t g1, const uint32_t* gseg_view, const uint32_t* max_score_bits,
                             uint32_t* kept_cnt, unsigned long long* best_pack, unsigned long long* cnt64,
                             hipStream_t st);
hipError_t launch_seg_write(uint32_t g0, uint32_t g1, unsigned long long base64, const ViewDev* views, const PairDesc* pairs, const uint32_t* seg_base,
                            const uint32_t* gseg_view, const unsigned long long* off64s,
                            const unsigned long long* best_pack, const uint32_t* seg_of_g, ListPools lp,
                            const Slot* slots, uint32_t* surv_off, uint32_t* hyp_off, Match* surv, uint32_t* surv_tg,
                            uint32_t* surv_sg, int32_t* hyp_of_seg, HypRec* hyps, float* depths, hipStream_t st);

// ---- k_rdd.hip ----
size_t rdd_workspace_bytes(uint32_t nnz, uint32_t n_rows);
hipError_t launch_rdd(const struct ::l3d_cledge* edges_in, uint32_t nnz, uint32_t n_rows, uint32_t iterations,
                      struct ::l3d_cledge* edges_out, void* workspace, size_t workspace_bytes, hipStream_t stream);

// ---- k_triangulate.hip: linear triangulation of tie points (l3d_triangulate_points) ----
struct TriArgs {
    const double* P;          // [n_cameras x 12] projection matrices, row-major 3x4
    uint32_t n_cameras;
    uint64_t n_points;
    const uint64_t* off;      // [n_points + 1] CSR over the observations
    const uint32_t* cam;      // [n_obs] camera of an observation, < n_cameras (the host checks)
    const double* xy;         // [n_obs x 2] its pixel
    double* X;                // [n_points x 3]
    uint8_t* valid;           // [n_points]
};
constexpr size_t kTriLdsBytes = 32 * 1024;   // projection matrices up to this size (341 cameras) are staged in LDS
hipError_t launch_triangulate(const TriArgs& t, hipStream_t st);

// ---- k_project.hip: the 3D lines projected into cameras (host side: l3d_project.hip) ----
struct ProjRecord { float x1, y1, x2, y2, iz1, iz2; uint32_t line, segment; };   // = l3d_projected_segment
constexpr uint32_t kProjNear = 0x80000000u, kProjRect = 0x40000000u;              // flag bits in ProjRecord::segment
struct ProjCam { double K[9], R[9], t[3], xmax, ymax; };   // xmax = width - 1, ymax = height - 1
struct ProjArgs {
    const ProjCam* cams;      // [n_cams]
    uint32_t n_cams, n_seg;
    const double* P;          // [n_seg x 6] P1, P2
    const uint32_t* line;     // [n_seg]
    double near_plane;
    ProjRecord* rec;          // [n_cams x n_seg] the record of (camera, segment), written where visible
    uint32_t* vis;            // [n_cams x n_seg + 1] 1 where visible; scanned in place by the caller
    ProjRecord* out;          // [n_cams x n_seg] the visible records, compacted in (camera, segment) order
    uint32_t* bounds;         // [n_cams + 1] first record of every camera in out; [n_cams] = the number of records
};
hipError_t launch_project_lines(const ProjArgs& a, hipStream_t st);     // fills rec and vis
hipError_t launch_project_compact(const ProjArgs& a, hipStream_t st);   // vis holds its exclusive scan: rec -> out
// a camera of a group of the map stages: its records, its pixels in the group's planes, its image
struct MapCam {
    uint32_t width, height;
    uint32_t rec0;            // first record of the camera in the group's record array
    uint32_t img_stride, img_channels, pad;
    uint64_t pix0;            // first pixel of the camera in the group's planes
    uint64_t img_off;         // first byte of its source image in the group's image block
    uint64_t rgb_off;         // first byte of its output image
};
struct MapArgs {
    const MapCam* cams; uint32_t n_cams;
    const ProjRecord* rec; uint32_t n_rec;
    uint32_t* steps;                    // [n_rec + 1] major-axis steps per record; scanned in place by the caller
    uint32_t thickness;
    unsigned long long* keys;           // [pixels of the group] zeroed by the caller
    uint64_t n_pix; uint32_t max_pix;   // pixels of the group / of its largest camera
    int32_t* line_id; float* inv_depth; // [pixels of the group]
    const uint8_t* img; uint8_t* rgb;   // overlay: source images, packed RGB out
    const uint8_t* colors; uint32_t n_lines, alpha;
};
hipError_t launch_raster_count(const MapArgs& a, hipStream_t st);
hipError_t launch_raster_lines(const MapArgs& a, uint32_t blocks, hipStream_t st);   // steps holds its exclusive scan
hipError_t launch_map_decode(const MapArgs& a, hipStream_t st);                      // keys -> line_id, inv_depth
hipError_t launch_overlay(const MapArgs& a, hipStream_t st);                         // line_id + img -> rgb

// ---- k_associate.hip: 2D segments assigned to the projected 3D lines they observe (host side: l3d_associate.hip) ----
constexpr uint32_t kAssocTile = 256;     // 2D segments of one camera per workgroup, one lane each
constexpr uint32_t kAssocChunk = 512;    // records per pass through LDS (16 KiB)
constexpr uint32_t kAssocSegmentMask = 0x3FFFFFFFu;   // = L3D_PROJ_SEGMENT_MASK
// a camera of a group: its tiles in the launch, its segments and records in the group's arrays
struct AssocCam { uint32_t tile0, seg0, n_seg, rec0, n_rec; };
// = l3d_association, but for d2: the squared distance, of which the host takes the root after the download
struct AssocOut { int32_t record; uint32_t line, segment; float d2, overlap; uint32_t n_accepted; };
struct AssocArgs {
    const AssocCam* cams; uint32_t n_cams;   // [n_cams] tile0 ascending: the exclusive prefix of tiles per camera
    const float4* segs;                      // [segments of the group] (x1, y1, x2, y2)
    const ProjRecord* rec;                   // [records of the group]
    AssocOut* out;                           // [segments of the group]
    double max_d2, min_cos2, min_overlap;    // max_distance * max_distance, the squared cosine, the overlap share
};
hipError_t launch_associate(const AssocArgs& a, uint32_t n_tiles, hipStream_t st);
extern std::atomic<uint64_t> g_assoc_launches, g_assoc_kernel_ns;   // l3d_associate.hip, test hooks read through l3d_debug_counter

// ---- k_compare.hip: two 3D line models compared segment by segment (host side: l3d_compare.hip) ----
constexpr uint32_t kCmpTile = 256;       // queries per workgroup, one lane each
constexpr uint32_t kCmpChunk = 256;      // references per pass through LDS (12 KiB of end points + 1 KiB of line indices)
// = l3d_line_match, but for d2: the squared distance, of which the host takes the root after the download
struct CmpOut { int32_t segment; uint32_t line, n_accepted; float overlap; double d2; };
// what one slice of the references found for one query: [query * n_slices + slice]
struct CmpPartial { unsigned long long bits; uint32_t index, n_accepted; double frac; double pad; };
static_assert(sizeof(CmpOut) == 24 && sizeof(CmpPartial) == 32, "comparison layout");
struct CmpArgs {
    const double* q; const uint32_t* q_line; uint32_t n_q;   // [n_q] x (P1, P2), their lines
    const double* r; const uint32_t* r_line; uint32_t n_r;   // the references
    uint32_t slice_chunks, n_slices;         // chunks of kCmpChunk references per slice; slices (grid.y)
    uint32_t exclude_same_line;
    double max_d2, min_cos2, min_overlap;    // max_distance * max_distance, the squared cosine, the overlap share
    CmpOut* out;                             // [n_q]
    CmpPartial* part;                        // [n_q * n_slices], used when n_slices > 1
};
// Steps 1-6 of DESIGN §18 for one pair, shared by k_compare.hip and k_merge.hip so that the two stages cannot drift apart.
// CmpQuery holds step 2, computed once per lane; cmp_pair runs the others on one reference r6 = (P1, P2) and calls
// accept(D2, frac), with the squared distance and the overlap share, iff the pair is accepted.  The tests are
// ordered cheapest first; a pair is accepted iff all hold, so the order changes nothing.
struct CmpQuery { double px, py, pz, sx, sy, sz, ex, ey, ez, E2; uint32_t line; bool live; };
__device__ __forceinline__ CmpQuery cmp_query(const double* v, uint32_t line, bool in_range) {
    CmpQuery q{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, false};
    if (in_range) { q.px = v[0]; q.py = v[1]; q.pz = v[2]; q.sx = v[3]; q.sy = v[4]; q.sz = v[5]; q.line = line; }
    q.ex = q.sx - q.px; q.ey = q.sy - q.py; q.ez = q.sz - q.pz;
    q.E2 = q.ex * q.ex + q.ey * q.ey + q.ez * q.ez;
    q.live = in_range && q.E2 > 0.0;
    return q;
}
template <class Accept>
__device__ __forceinline__ void cmp_pair(const CmpQuery& q, const double* r6, uint32_t r_line, bool exclude_same_line,
                                         double max_d2, double min_cos2, double min_overlap, Accept&& accept) {
    // 1. reference vector and length
    const double bx = r6[0], by = r6[1], bz = r6[2];
    const double dx = r6[3] - bx, dy = r6[4] - by, dz = r6[5] - bz;
    const double L2 = dx * dx + dy * dy + dz * dz;
    if (!(L2 > 0.0)) return;                                       // (uniform over the workgroup)
    // 2. the query
    if (!q.live) return;
    // 3. the same line
    if (exclude_same_line && r_line == q.line) return;
    // 4. angle
    const double dot = dx * q.ex + dy * q.ey + dz * q.ez;
    if (!(dot * dot >= min_cos2 * (L2 * q.E2))) return;
    // 5. distance
    const double wx = q.px - bx, wy = q.py - by, wz = q.pz - bz;
    const double ux = q.sx - bx, uy = q.sy - by, uz = q.sz - bz;
    const double c1x = dy * wz - dz * wy, c1y = dz * wx - dx * wz, c1z = dx * wy - dy * wx;
    const double c2x = dy * uz - dz * uy, c2y = dz * ux - dx * uz, c2z = dx * uy - dy * ux;
    const double m1 = c1x * c1x + c1y * c1y + c1z * c1z;
    const double m2 = c2x * c2x + c2y * c2y + c2z * c2z;
    const double D2 = (m1 > m2 ? m1 : m2) / L2;
    if (!(D2 <= max_d2)) return;
    // 6. overlap
    const double t1 = (dx * wx + dy * wy + dz * wz) / L2;
    const double t2 = (dx * ux + dy * uy + dz * uz) / L2;
    const double tlo = t1 < t2 ? t1 : t2, thi = t1 < t2 ? t2 : t1;
    const double ov = (thi < 1.0 ? thi : 1.0) - (tlo > 0.0 ? tlo : 0.0);
    if (!(ov > 0.0)) return;
    const double frac = ov / (thi - tlo);
    if (!(frac >= min_overlap)) return;
    accept(D2, frac);
}
// The references of a slice, for k_compare.hip and k_merge.hip alike: chunks [slice * slice_chunks, + slice_chunks) of
// kCmpChunk, cut at n_refs (never empty: the host derives n_slices from slice_chunks, slice_plan of l3d_model.h).
__device__ __forceinline__ void cmp_slice_range(uint32_t n_refs, uint32_t slice, uint32_t slice_chunks, uint32_t& r_begin, uint32_t& r_end) {
    const unsigned long long ref0 = (unsigned long long)slice * slice_chunks * kCmpChunk;
    const unsigned long long ref1 = ref0 + (unsigned long long)slice_chunks * kCmpChunk;
    r_begin = (uint32_t)(ref0 < n_refs ? ref0 : n_refs);
    r_end = (uint32_t)(ref1 < n_refs ? ref1 : n_refs);
}
// The n <= kCmpChunk references from r0 on staged into LDS, coalesced, by the whole workgroup: every lane calls it, the
// lanes beyond the last query too.
__device__ __forceinline__ void cmp_stage_chunk(double* s_p, uint32_t* s_line, const double* refs, const uint32_t* ref_line, uint32_t r0, uint32_t n) {
    __syncthreads();                                                             // the previous chunk has been read
    for (uint32_t i = threadIdx.x; i < 6 * n; i += kCmpTile) s_p[i] = refs[6 * (size_t)r0 + i];
    if (threadIdx.x < n) s_line[threadIdx.x] = ref_line[r0 + threadIdx.x];
    __syncthreads();
}
hipError_t launch_compare(const CmpArgs& a, hipStream_t st);         // tiles x slices; writes out (one slice) or part
hipError_t launch_compare_merge(const CmpArgs& a, hipStream_t st);   // part -> out
// l3d_compare.hip, test hooks read through l3d_debug_counter
extern std::atomic<uint64_t> g_cmp_launches, g_cmp_merge_launches, g_cmp_slices, g_cmp_kernel_ns;

// ---- k_merge.hip: the accepted pairs of one model against itself, as a list (host side: l3d_merge.hip) ----
// k_compare's tiling (kCmpTile queries x one slice of the references per workgroup, chunks of kCmpChunk through LDS).
struct MrgPair { uint32_t q, r; };
struct MrgArgs {
    const double* segs; const uint32_t* line; uint32_t n;    // [n] x (P1, P2), their lines: queries and references alike
    uint32_t slice_chunks, n_slices;
    double max_d2, min_cos2, min_overlap;
    uint32_t* counts;                        // [n * n_slices + 1]: k_merge_count's counts at [q * n_slices + slice], then
                                             // their exclusive scan in place (the total behind the last one)
    MrgPair* pairs; uint32_t n_pairs;        // [n_pairs = the total], written by k_merge_write
    uint32_t* wrapped;                       // k_merge_check: set to 1 where the 32-bit scan has wrapped
};
hipError_t launch_merge_count(const MrgArgs& a, hipStream_t st);
hipError_t launch_merge_write(const MrgArgs& a, hipStream_t st);
hipError_t launch_merge_check(const MrgArgs& a, hipStream_t st);
// l3d_merge.hip, test hooks read through l3d_debug_counter
extern std::atomic<uint64_t> g_mrg_count_launches, g_mrg_write_launches, g_mrg_slices, g_mrg_pairs, g_mrg_kernel_ns;

// ---- k_wireframe.hip: the junctions of one model, as a list (host side: l3d_wireframe.hip) ----
// k_merge's two walks over k_compare's tiling, over the pairs a < b only.
struct WfJunction { uint32_t a, b; double sa, sb, gap2; };   // = WfRecord of l3d_wireframe.h
static_assert(sizeof(WfJunction) == 32, "junction record layout");
struct WfArgs {
    const double* segs; const uint32_t* line; uint32_t n;    // [n] x (P1, P2), their lines: queries and references alike
    uint32_t slice_chunks, n_slices;
    double max_d2, max_extension, min_sin2;  // max_distance * max_distance, the reach beyond an end, the squared sine
    uint32_t* counts;                        // [n * n_slices + 1]: k_wf_count's counts at [q * n_slices + slice], then
                                             // their exclusive scan in place (the total behind the last one)
    WfJunction* out; uint32_t n_out;         // [n_out = the total], written by k_wf_write
    uint32_t* wrapped;                       // k_wf_check: set to 1 where the 32-bit scan has wrapped
};
hipError_t launch_wf_count(const WfArgs& a, hipStream_t st);
hipError_t launch_wf_write(const WfArgs& a, hipStream_t st);
hipError_t launch_wf_check(const WfArgs& a, hipStream_t st);
// l3d_wireframe.hip, test hooks read through l3d_debug_counter
extern std::atomic<uint64_t> g_wf_count_launches, g_wf_write_launches, g_wf_slices, g_wf_junctions, g_wf_skipped_blocks, g_wf_kernel_ns, g_wf_count_ns;

// ---- k_planes.hip: a plane per junction, and every plane scored against every segment (host side:
// l3d_planes.hip, the selection: l3d_planes.h) ----
struct PlHypothesis { double N[3], J[3]; uint32_t a, b, live, pad; };   // = PlHyp of l3d_planes.h
struct PlCell { unsigned long long weight; uint32_t count, zero; };      // = l3d_pl_score
static_assert(sizeof(PlHypothesis) == 64 && sizeof(PlCell) == 16, "plane record layout");
constexpr unsigned long long kPlLiveBit = 1ull << 63;   // of a segment's weight word: E2 > 0.  The weight itself is below 2^53
struct PlArgs {
    const double* segs; uint32_t n;          // [n] x (P1, P2)
    const unsigned long long* weight;        // [n] the integer weight, kPlLiveBit set for a live segment; 0: a point
    const WfJunction* junctions; uint32_t n_h;   // the hypotheses' junctions
    uint32_t slice_chunks, n_slices;
    double max_distance;
    PlHypothesis* hyp;                       // [n_h], written by k_pl_hypotheses
    PlCell* cells;                           // [n_h * n_slices] at [h * n_slices + slice], written by k_pl_score
    PlCell* scores;                          // [n_h], the cells of a hypothesis added, written by k_pl_merge
};
hipError_t launch_pl_hypotheses(const PlArgs& a, hipStream_t st);
hipError_t launch_pl_score(const PlArgs& a, hipStream_t st);
// k_pl_merge, for the planes and for the directions of §26 alike: scores[h] = the sum of cells[h * n_slices + slice]
hipError_t launch_pl_merge(const PlCell* cells, PlCell* scores, uint32_t n_h, uint32_t n_slices, hipStream_t st);
// l3d_planes.hip, test hooks read through l3d_debug_counter
extern std::atomic<uint64_t> g_pl_score_launches, g_pl_slices, g_pl_hypotheses, g_pl_kernel_ns, g_pl_junction_ns;

// ---- k_directions.hip: a unit direction per segment, and every direction scored against every segment (DESIGN §26;
// host side: l3d_directions.hip, the selection: l3d_directions.h).  The cells are §25's, added by k_pl_merge ----
struct DirUnit { double D[3]; unsigned long long w; };   // e / sqrt(E2), 0 for a point; the weight word (kPlLiveBit)
static_assert(sizeof(DirUnit) == 32, "direction record layout");
struct DirArgs {
    const double* segs; uint32_t n;          // [n] x (P1, P2): segments and hypotheses alike
    const unsigned long long* weight;        // [n] the weight words of §25
    uint32_t slice_chunks, n_slices;
    double max_sin2;
    DirUnit* units;                          // [n], written by k_dir_units
    PlCell* cells;                           // [n * n_slices] at [h * n_slices + slice], written by k_dir_score
    PlCell* scores;                          // [n], written by k_pl_merge
};
hipError_t launch_dir_units(const DirArgs& a, hipStream_t st);
hipError_t launch_dir_score(const DirArgs& a, hipStream_t st);
// l3d_directions.hip, test hooks read through l3d_debug_counter
extern std::atomic<uint64_t> g_dir_score_launches, g_dir_slices, g_dir_hypotheses, g_dir_kernel_ns;

// ---- k_align.hip: the similarity transform applied, and the normal equations of an alignment step (host
// side: l3d_align.hip) ----
constexpr uint32_t kAlnTerms = 37;       // H (28: the upper triangle of 7 x 7, row by row), b (7), cost, count
struct AlnTransformArgs {
    const double* in; double* out; uint32_t n;   // [n] x (P1, P2)
    double scale, q[4], t[3];                    // q of unit length
};
struct AlnNormalArgs {
    const double* q; uint32_t n_q;           // the transformed queries
    const double* r; uint32_t n_r;           // the references
    const CmpOut* match;                    // [n_q] the comparison's records: segment = the reference, -1: none
    double c[3];                             // the centre the update rotates and scales about
    double* tiles;                           // [ceil(n_q / kCmpTile) x kAlnTerms]
};
hipError_t launch_align_transform(const AlnTransformArgs& a, hipStream_t st);
hipError_t launch_align_normal(const AlnNormalArgs& a, hipStream_t st);
// l3d_align.hip, test hooks read through l3d_debug_counter
extern std::atomic<uint64_t> g_aln_iterations, g_aln_normal_launches, g_aln_kernel_ns;

// ---- k_pose.hip: the normal equations of a camera's pose against the 3D line model (host side:
// l3d_pose.hip).  The tiles are k_associate's: AssocCam, kAssocTile segments of one camera per workgroup. ----
constexpr uint32_t kPoseTerms = 29;      // H (21: the upper triangle of 6 x 6, row by row), b (6), cost, count
// a camera of a pass: the entries m00, m10, m11, m20, m21 of K^-T (the others are 0, 0, 0 and 1) and the pose in force
struct PoseCam { double M[5], R[9], t[3]; };
struct PoseNormalArgs {
    const AssocCam* cams; uint32_t n_cams;   // the table launch_associate was given
    const PoseCam* pose;                     // [n_cams]
    const float4* segs;                      // [segments of the group] (x1, y1, x2, y2)
    const AssocOut* assoc;                   // [segments of the group] the association's records
    const double* model; uint32_t n_model;   // the 3D segments (P1, P2) in the frame of `pose`
    double* tiles;                           // [tiles of the launch x kPoseTerms]
};
hipError_t launch_pose_normal(const PoseNormalArgs& a, uint32_t n_tiles, hipStream_t st);
// cams[c].rec0 / n_rec from the compaction's bounds[n_cams + 1], one lane per camera
hipError_t launch_pose_bounds(AssocCam* cams, uint32_t n_cams, const uint32_t* bounds, hipStream_t st);
// l3d_pose.hip, test hooks read through l3d_debug_counter
extern std::atomic<uint64_t> g_pose_iterations, g_pose_normal_launches, g_pose_kernel_ns;

// ---- k_refit.hip: the 3D lines refit against cameras and their 2D segments (host side: l3d_refit.hip; the
// kernels' arguments: l3d_refit.h).  l3d_refit.hip, test hooks read through l3d_debug_counter ----
extern std::atomic<uint64_t> g_refit_observations, g_refit_lines_solved, g_refit_kernel_ns, g_refit_part_ns[5];

// ---- k_bundle.hip: cameras and 3D lines bundled jointly (host side: l3d_bundle.hip; the kernels' arguments:
// l3d_bundle.h).  l3d_bundle.hip, test hooks read through l3d_debug_counter ----
extern std::atomic<uint64_t> g_bundle_iterations, g_bundle_rejected_steps, g_bundle_kernel_ns;

}  // namespace l3d
