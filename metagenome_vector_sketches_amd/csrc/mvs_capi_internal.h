// mvs_capi_internal.h -- what the translation units of the C ABI (mvs_capi*.hip) share: the context and sketch-set objects, the
// buffer / read-back helpers, the stages of the comparison that the streamed output and the block plans drive themselves, and
// the bodies that families of entry points share (consumers of kept cells, of dense dots, of units over sorted hash lists).
// Not installed.
#ifndef MVS_CAPI_INTERNAL_H
#define MVS_CAPI_INTERNAL_H

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <dlfcn.h>
#include <mutex>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <chrono>
#include <thread>
#include <vector>

#include <array>

#include "mvs_encode.h"
#include "mvs_internal.h"
#include "mvs_owned.h"

// the ABI's objects are declared outside the namespace (include/mvs_hip.h names them)
using mvs_capi::DevBuf;
using mvs_capi::Event;
using mvs_capi::PinnedBuf;
using mvs_capi::Stream;

// a balanced tile order of a filter launch (mvs::plan_tile_order), cached by launch geometry: the comparisons of a job repeat
// the same few shapes, so a list is built and uploaded once
struct mvs_tile_order {
    std::vector<long long> key;
    DevBuf d;                         // unsigned; empty: the static map serves this shape
    unsigned per = 0;
};

namespace mvs_capi {
// what the calls of one consumer of kept cells (clustering, linkage, dereplication) did on a context since that consumer's
// last *_create there: kernel times of the comparison and of the consumer's own work (timing enabled), cells with row != col
// consumed, row blocks, the most rounds a list needed
struct ConsumerStats {
    double compare_ms = 0.0, work_ms = 0.0;
    long long edges = 0, blocks = 0, rounds = 0;
    void reset() { *this = ConsumerStats(); }
};
// what the last call of one consumer of dense dots (top-k, containment, level counts, the Jaccard operator) did on a context:
// kernel times of the dots and of the consumer's own work summed over the row blocks (timing enabled), row blocks, rows per block
struct DotsStats {
    double dots_ms = 0.0, work_ms = 0.0;
    long long blocks = 0, block_rows = 0;
    void reset() { *this = DotsStats(); }
};
// what the last mvs_group_sums / mvs_permanova did on a context (mvs_ctx_groups_stats): kernel times summed over the row blocks
// (timing enabled), row blocks, rows per block, labellings
struct GroupsStats {
    double dots_ms = 0.0, quantise_ms = 0.0, sums_ms = 0.0;
    long long blocks = 0, block_rows = 0, slots = 0;
    void reset() { *this = GroupsStats(); }
};
// what the last mvs_label_sums / mvs_silhouette did on a context (mvs_ctx_label_stats): kernel times of the dots and of the
// segmented reduction summed over the row blocks, the time of the gather into label order (timing enabled), row blocks, rows
// per block
struct LabelStats {
    double dots_ms = 0.0, reduce_ms = 0.0, gather_ms = 0.0;
    long long blocks = 0, block_rows = 0;
    void reset() { *this = LabelStats(); }
};
// what the last mvs_core_jaccard / mvs_hdbscan did on a context (mvs_ctx_hdbscan_stats): kernel times of the core pass (top-k's
// dots and selection summed over the ranges, k_core_kth), of the comparison and the forest, the host time of the selection;
// top-k ranges, Boruvka rounds, links, fed cells
struct HdbscanStats {
    double core_dots_ms = 0.0, core_select_ms = 0.0, core_kth_ms = 0.0, compare_ms = 0.0, forest_ms = 0.0, host_ms = 0.0;
    long long ranges = 0, rounds = 0, links = 0, edges = 0;
    void reset() { *this = HdbscanStats(); }
};
// what the last mvs_pairwise_stream / mvs_cells_stream did on a context (mvs_ctx_stream_stats): comparison kernels summed over
// the row blocks (timing enabled), bytes, row blocks, pieces, the two-stage route -- and the route its row blocks took
// (mvs_ctx_stream_dense_stats): delivered out of the dense byte matrix, row passes queued with buffers sized from the blocks
// before, of those the ones whose sizes did not hold (done again), dense blocks with a q a byte cannot hold (that block and the
// rest became lists)
struct StreamStats {
    double kernel_ms = 0.0;
    long long bytes = 0, blocks = 0, pieces = 0, two_stage = 0;
    long long dense_blocks = 0, spec_blocks = 0, spec_redone = 0, list_fallbacks = 0;
    void reset() { *this = StreamStats(); }
};
// what the last mvs_hclust / mvs_hclust_weights / mvs_hclust_sums did on a context (mvs_ctx_hclust_stats): kernel times of the
// dots and of the fill summed over the row blocks, of the nearest pass, of the merge (pairs, column and row phase) and of the
// compactions summed over the rounds (timing enabled); rounds, rows scanned, bytes of the table those scans read, compactions
struct HclustStats {
    double dots_ms = 0.0, fill_ms = 0.0, nearest_ms = 0.0, merge_ms = 0.0, compact_ms = 0.0;
    long long rounds = 0, row_scans = 0, bytes_scanned = 0, compactions = 0;
    void reset() { *this = HclustStats(); }
};
// what the community calls did on a context since its last mvs_community_create (mvs_ctx_community_stats): kernel times of the
// comparison, of the graph's build (sort, unique, mirror, CSR), of the local moving and of the numbering + aggregation (timing
// enabled), the moving of level 0 alone with its rounds and the bytes one of its rounds reads; edges, levels, rounds, row
// blocks; vertices that started in the wave / workgroup / global path (summed over the levels) and hand-overs wave ->
// workgroup and workgroup -> global (summed over the rounds)
struct CommunityStats {
    double compare_ms = 0.0, build_ms = 0.0, move_ms = 0.0, aggregate_ms = 0.0, level0_move_ms = 0.0;
    long long edges = 0, levels = 0, rounds = 0, blocks = 0, level0_rounds = 0, level0_bytes = 0;
    long long paths[5] = {0, 0, 0, 0, 0};
    void reset() { *this = CommunityStats(); }
};
// what the t-SNE calls did on a context since its last mvs_tsne_create (mvs_ctx_tsne_stats): kernel times of top-k, of the
// calibration, of the graph's build (sort, sum by key, CSR, P), of the repulsion, the attraction and the update summed over the
// iterations (timing enabled); iterations run, directed entries of the graph, units of one repulsion, top-k row ranges
struct TsneStats {
    double topk_ms = 0.0, calibrate_ms = 0.0, graph_ms = 0.0, repulse_ms = 0.0, attract_ms = 0.0, update_ms = 0.0;
    long long iterations = 0, edges = 0, units = 0, blocks = 0;
    void reset() { *this = TsneStats(); }
};
// what the last sketching call of one kind did on a context (mvs_ctx_kmer_stats, mvs_ctx_aa_stats): time of the hashing passes
// and the scatter (timing enabled), bytes read, hashed k-mers, kept values before the unique compaction, units of work, hashing
// passes repeated because the staging list was too short; hashed k-mers and kept values per sample
struct SeqStats {
    double kernel_ms = 0.0;
    long long bases = 0, kmers = 0, kept = 0, units = 0, second_trips = 0;
    std::vector<long long> sample_kmers, sample_kept;
};
}  // namespace mvs_capi

struct mvs_ctx {
    mvs_ctx() = default;
    ~mvs_ctx();   // waits for `stream`; the members release what they own
    int device = 0;
    // the streams and events stand before every buffer, so that they are destroyed after the memory their work may use
    Stream own_stream;
    hipStream_t stream = nullptr;   // own_stream, or the caller's (mvs_ctx_set_stream)
    // event pairs: 0 projection kernel, 1 whole comparison (filter + re-check, or the exact kernel),
    // 2 the filter kernel alone, 3 the re-check kernel alone
    Event ev[8];
    // streamed output (mvs_pairwise_stream): the download side
    Stream dl_stream;
    Event dl_done[2];    // download into pinned buffer i has completed
    Event dl_block[2];   // the downloads out of CSR array set i have completed
    Event dl_ready[2];   // the arrays of the row block in set i are final on the compute stream
    Stream post_stream;  // dense row blocks -> CSR / encoded rows beside the next block's comparison
    Event cmp_done;      // the comparison launch of the block about to be post-processed is through
    Stream up_stream;    // host hash lists on their way to the device (below)
    Event up_done[2];    // DMA out of staging buffer i has completed
    Event pinned_ev;     // the upload out of `pinned` has completed
    std::vector<mvs_tile_order> tile_orders;
    mvs::Options opt;   // tuning switches: environment defaults read once at creation, then mvs_ctx_set_option
    // timing of the dominant kernels (optional)
    bool timing = false;
    bool ev_valid[5] = {false, false, false, false, false};   // [4]: exact kernel on the flagged tiles (ev[6]..ev[3])
    // reusable device scratch
    DevBuf scratch;
    DevBuf d_counter;                       // 8-byte slots for counters / max
    unsigned long long* counters() const { return d_counter.as<unsigned long long>(); }
    // grow-only device buffers of mvs_pairwise_rows (no hipMalloc/hipFree on the hot path)
    DevBuf pw_thr, pw_tmp, pw_sort, pw_out;
    DevBuf stage;                           // host sketches on their way to the limb planes
    // two-stage comparison: coarse plane + row statistics of the set `coarse_id` (generation `coarse_gen`),
    // per-call filter constants, candidate list
    DevBuf pw_coarse;
    DevBuf pw_coarse_fm;                    // fragment-major copy (streaming search filters), built on demand
    DevBuf st_tlist, st_tlist_n;            // dense row passes: active tiles per tile row of the block, their counts,
    DevBuf st_ends;                         // and every row's first / last kept column
    DevBuf pw_need;                         // block plans: rows whose limb planes are to be rebuilt (mvs_plan_wire)
    DevBuf pw_planes_fm;                    // fragment-major copy of the limb planes of set planes_fm_id
    unsigned long long planes_fm_id = 0, planes_fm_gen = 0;         // (generation planes_fm_gen), for the ping-pong exact kernel
    bool coarse_fm_valid = false;           // ... of the cached plane
    DevBuf pw_rows, pw_fmeta, pw_cand;
    // streamed output (mvs_pairwise_stream): packed kept cells raw / sorted, their CSR form, the download side
    DevBuf st_raw, st_sorted;
    DevBuf st_col[2], st_q[2];              // CSR arrays of two row blocks: one is downloaded while the next is built
    DevBuf st_rowptr, st_counts;
    DevBuf st_dense;                        // dense results: one byte per cell (mvs_internal.h)
    PinnedBuf rb_pinned;                                    // pinned landing zone of the small per-block read-backs (row index,
                                                            // record offsets, counters): a copy into pageable memory makes the
                                                            // runtime stage and block per copy -- 5 of them per row block
    size_t st_dense_zero = 0;   // the first st_dense_zero bytes of st_dense are zero once the work queued on `stream` is through:
                                // the tile-granular dense flow needs a cleared matrix, clears it again behind its last block --
                                // while the link still drains -- and so finds it clean the next time
    // rows encoded on the device (mvs_pairwise_stream_encoded): per-row sizes / offsets / directory, the records themselves
    DevBuf en_size, en_off, en_jac, en_first, en_par;
    DevBuf st_enc[2];
    PinnedBuf dl_pinned[2];                       // pinned host buffers, each allocated (and grown) when first needed:
                                                  // pinning costs ~0.3 ms per MiB, a one-piece result needs only one
    std::unique_ptr<void, void (*)(void*)> dl_hsa{nullptr, nullptr};   // option stream_copy = 1: agents + completion signals of
                                                                       // the DMA copies (mvs_capi_stream.hip owns the type)
    mvs_capi::StreamStats st;                     // what the last mvs_pairwise_stream did
    // tile-granular two-stage comparison: tile flags, flagged tiles per tile row, their row-major list (entry 0 = total),
    // the candidate list without the pairs of flagged tiles
    DevBuf pw_tflag, pw_trow, pw_tlist, pw_cand2;
    DevBuf pw_ttouch, pw_tnew;              // dense byte matrix: tiles the re-check's cells were scattered into, and the list of
                                            // those touched for the first time (to be cleared)
    long long last_flagged_tiles = 0, last_filter_tiles = 0;   // of the last two-stage comparison (mvs_ctx_pairwise_stats)
    DevBuf pw_chdr, pw_cent;                // candidate regions of the ping-pong filter: counts, entries
    unsigned long long coarse_id = 0, coarse_gen = 0;
    int coarse_mode = -1;                   // radix rule (option coarse_radix) the cached plane was built with
    // derived data built / refreshed since the context was created (mvs_ctx_derived_stats): whole builds of the coarse plane,
    // of its fragment-major copy and of the fragment-major limb planes, and the rows refresh_derived() re-derived in place
    long long dv_coarse_builds = 0, dv_coarse_rows = 0, dv_coarse_fm_builds = 0, dv_planes_fm_builds = 0, dv_planes_fm_rows = 0;
    unsigned long long few_rows_id = 0, few_rows_gen = 0;   // the set whose last comparison was a block of < 1024 rows done by the
                                                            // exact kernel because no coarse plane existed (pairwise_launch)
    unsigned long long filter_off_id = 0;   // (set, coefficient) for which the filter passed too many pairs
    double filter_off_coeff = 0.0;
    unsigned long long last_candidates = 0; // candidate pairs of the last two-stage comparison (0: exact kernel)
    unsigned long long h_start = 0;      // host copy of the starting cell count of an appending call
    // host hash lists on their way to the device: two pinned staging buffers + a copy stream, so that the host-side
    // copy into pinned memory, the DMA and the projection kernel of consecutive pieces overlap
    PinnedBuf up_pinned[2];
    // workgroups of k_project the device holds at a time, by [variant][statistics]: CUs x the occupancy of that instantiation,
    // asked for once (0: not yet) -- what mvs_project_plan balances a launch's last round against
    int cu_count = 0;
    int proj_slots[25][2] = {};
    // what the last projection launched (mvs_ctx_project_stats)
    long long pj_units = 0, pj_cut_samples = 0;
    int pj_slots = 0, pj_ny = 0;
    // pinned host staging for small metadata uploads (projection unit lists)
    PinnedBuf pinned;
    bool pinned_busy = false;
    // block plans (mvs_plan_*): state between begin / filter / finish, scratch of mvs_sketch_set_prepare_rows, events
    int plan_overlap = 0;                 // block plans: 1 = filter launches alternate between the stream and a side stream
    int report_spin = 0;                  // mvs_cells_report: microseconds to poll the stream before blocking on it (0: block at once)
                                          // (measured at the per-rank size of an 8-way split: filters 1.191 -> 1.164 ms, within
                                          // the box-to-box spread; off by default -- one more queue beside RCCL's for 2 %)
    struct PlanState* plan = nullptr;
    DevBuf plan_tmp;
    const void* rows_max_done = nullptr;   // state block whose widest row mvs_cells_sort_rows_ahead has already computed
    // what the last mvs_pairwise_topk / _contain / _levels did (mvs_ctx_topk_stats, mvs_ctx_contain_stats, mvs_ctx_levels_stats)
    mvs_capi::DotsStats tk, ct, lv;
    // what the last mvs_sketch_moments / mvs_pca_fit / mvs_pca_transform did (mvs_ctx_pca_stats): times with timing enabled
    double pc_gram_ms = 0.0, pc_eigen_ms = 0.0, pc_scores_ms = 0.0;
    long long pc_slabs = 0, pc_iters = 0;
    // what the last mvs_jaccard_apply / mvs_pcoa_fit / mvs_pcoa_transform did (mvs_ctx_pcoa_stats): kernel times summed over its
    // passes and row blocks, the solver's whole time (timing enabled)
    mvs_capi::DotsStats po;
    double po_eigen_ms = 0.0;
    long long po_passes = 0;
    // what the clustering, linkage and dereplication calls did since the last mvs_cluster_create / mvs_linkage_create /
    // mvs_derep_create on this context (mvs_ctx_cluster_stats, mvs_ctx_linkage_stats, mvs_ctx_derep_stats)
    mvs_capi::ConsumerStats cl, lk, dr;
    mvs_capi::GroupsStats gs;
    mvs_capi::HdbscanStats hd;
    mvs_capi::LabelStats ls;
    int labels_dots = 0;                  // mvs_label_sums / mvs_silhouette: dots of a row block from 0 = the matrix-core kernels, 1 = the
                                          // vector-ALU kernel (A/B, tests); same sums (option labels_dots)
    int labels_block_rows = 0;            // ... and > 0 = upper bound on the rows of a block (tests); 0 = by the device budget.  Host-side
                                          // blocking only (option labels_block_rows)
    mvs_capi::HclustStats hc;
    int hclust_dots = 0;                  // mvs_hclust: dots of a row block from 0 = the matrix-core kernels, 1 = the vector-ALU kernel (A/B,
                                          // tests); same table (option hclust_dots)
    int hclust_block_rows = 0;            // ... and > 0 = upper bound on the rows of a block of the fill (tests); 0 = by the device budget
                                          // (option hclust_block_rows)
    int hclust_compact = 1;               // the table's columns are compacted 0 = never, 1 = when at most half of them are alive, 2 = after
                                          // every round; same records (option hclust_compact)
    mvs_capi::CommunityStats cm;
    int community_path = 0;               // mvs_community_finish: a vertex starts in 0 = the path its degree names, 1 = the wave path, 2 = the
                                          // workgroup path, 3 = the global path (tests); same result (option community_path)
    mvs_capi::TsneStats ts;
    int tsne_slice_cols = 1024;           // mvs_tsne_gradient / _run / _kl: columns of a repulsion unit, 16 .. 1024 (tests force small inputs
                                          // through many slices); same sums (option tsne_slice_cols)
    int core_block_rows = 0;              // mvs_core_jaccard / mvs_hdbscan: > 0 = upper bound on the rows of a top-k range (tests); 0 = by
                                          // the cell buffer's budget.  Host-side blocking only (option core_block_rows)
    // mvs_intersect_cells: grow-only work space (unit counts, their scan, the scan's scratch, counters) and what the last call
    // did (mvs_ctx_intersect_stats)
    DevBuf ix_work;
    double ix_kernel_ms = 0.0;
    long long ix_units = 0, ix_cut = 0, ix_bytes = 0;
    // what the last mvs_gather did (mvs_ctx_gather_stats): survivors of phase 0, rounds run, batches (= read-backs of the
    // walk's state), bytes of the bit rows; kernel times of the three phases (timing enabled)
    long long ga_survivors = 0, ga_rounds = 0, ga_batches = 0, ga_row_bytes = 0, ga_round_bytes = 0;
    double ga_overlap_ms = 0.0, ga_mark_ms = 0.0, ga_rounds_ms = 0.0;
    // what the last mvs_hash_set_from_sequences (mvs_ctx_kmer_stats) and the last mvs_hash_set_from_residues (mvs_ctx_aa_stats) did
    mvs_capi::SeqStats km, aa;
    // what the last counted set build did (mvs_ctx_abund_stats): time of the sorts and of the run-sum passes (timing enabled),
    // values given, distinct values, values that passed the filter, units of the run-sum passes, samples sorted device-wide
    double ab_sort_ms = 0.0, ab_count_ms = 0.0;
    long long ab_values = 0, ab_distinct = 0, ab_passed = 0, ab_units = 0, ab_big = 0;
};

// hash lists resident on the device (mvs_capi_intersect.hip builds them; mvs_capi_gather.hip reads them too)
struct mvs_hash_set {
    mvs_ctx* ctx = nullptr;
    int64_t n = 0, total = 0;
    int was_sorted = 0;
    DevBuf hashes;    // unsigned long long, per sample strictly increasing
    DevBuf offsets;   // long long, n + 1
    DevBuf sizes;     // int32_t, n
    DevBuf abund;     // uint32_t aligned with hashes: the counted builds' abundances; empty for every other set
};

struct mvs_sketch_set {
    mvs_ctx* ctx = nullptr;
    const int8_t* planes = nullptr;
    DevBuf owned;
    int64_t n = 0, n_alloc = 0;
    int d = 0, d_pad = 0, limbs = 0;
    unsigned long long id = 0, gen = 0;   // identity of the plane contents (cache key of derived data)
    // mvs_sketch_set_attach_derived: the filter's inputs in caller buffers (block plans), NULL otherwise
    int8_t* ext_coarse_fm = nullptr;
    mvs::CoarseRow* ext_rows = nullptr;
    // rows rewritten (mvs_sketch_set_fill) since the context's derived data of this set was built: refreshed row by row on
    // the next comparison instead of rebuilding everything (a search appends a handful of query rows to a resident database)
    int64_t dirty_lo = 0, dirty_hi = 0;
};

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return mvs_capi::fail(MVS_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace mvs_capi {

extern std::atomic<unsigned long long> g_set_ids;

// sets the calling thread's error message (mvs_last_error) and returns `code`
int fail(int code, const char* fmt, ...);
inline bool mem_ok(int m) { return m == MVS_MEM_HOST || m == MVS_MEM_DEVICE; }

// rocprofv3 --marker-trace range around an entry point (option `markers`)
struct Range {
    bool on = false;
    Range(const mvs_ctx* c, const char* name);
    ~Range();
};

// The time of a stretch of kernels on the context's stream, for a statistic.  With timing off every method does nothing: a
// call site synchronises exactly where it did without the timer.
struct StageTimer {
    Event ev[2];   // around the stretch
    hipStream_t stream = nullptr;
    bool on = false;
    // the stretch begins here
    int begin(mvs_ctx* c) {
        on = c->timing;
        if (!on) return MVS_OK;
        stream = c->stream;
        for (Event& x : ev) HIP_TRY(x.create());
        HIP_TRY(hipEventRecord(ev[0], stream));
        return MVS_OK;
    }
    // ... and ends here (nothing waits)
    int mark_end() {
        if (on) HIP_TRY(hipEventRecord(ev[1], stream));
        return MVS_OK;
    }
    // waits for the end mark (at once where the caller has synchronised the stream since) and adds the stretch's time
    int add_to(double* ms) {
        if (!on) return MVS_OK;
        HIP_TRY(hipEventSynchronize(ev[1]));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        *ms += t;
        return MVS_OK;
    }
};

// the grow-only buffers of a context: `b` holds at least `bytes` afterwards.  A smaller block is freed -- once the work queued on
// the context's stream is through -- before the larger one is asked for; MVS_E_NOMEM leaves the buffer empty
int ensure_buf(mvs_ctx* c, DevBuf& b, size_t bytes);
struct ReadBack {
    void* dst;
    const void* src;
    size_t bytes;
};
int ensure_read_back(mvs_ctx* c, size_t total);
int read_back(mvs_ctx* c, hipStream_t st, std::initializer_list<ReadBack> items);
int ensure_scratch(mvs_ctx* c, size_t bytes);
int acquire_pinned(mvs_ctx* c, size_t bytes);
void parallel_copy(void* dst, const void* src, size_t bytes);
constexpr size_t kUploadPiece = 32u << 20;    // bytes per staging buffer (pinning memory costs ~0.3 ms per MiB: keep them small)
int ensure_upload_pipeline(mvs_ctx* c);
int check_kernel(const char* what);
void plan_state_free(mvs_ctx* c);      // mvs_capi_plan.hip

// ---- mvs_capi_kmer.hip: bytes -> hash set, for any hashing kernel of the k_kmer_hash frame ----
// The units of work (up to `unit` window positions of one sample, a window `window` bytes long), the upload, the staging list
// with its second trip at the exact size, the counts per sample, k_kmer_scatter and mvs_hash_set_create.  `launch` queues the
// hashing kernel (named `kernel` in messages) over the units; it hashes `per_window` k-mers per position.  The arguments are
// checked by the caller (check_sample_bytes: the offsets and the bytes of n samples); *st is reset and filled.
int check_sample_bytes(const uint8_t* bytes, const int64_t* offsets, int64_t n);
using HashLauncher = std::function<int(const uint8_t* d_bytes, long long total_bytes, const mvs::KmerUnit* d_units, long long n_units,
                                       unsigned long long* d_vals, int32_t* d_sample, unsigned long long cap, unsigned long long* d_counters,
                                       unsigned long long* d_sample_counts, unsigned long long* d_sample_valid)>;
int hash_set_from_bytes(mvs_ctx* c, const char* call, const char* kernel, const uint8_t* bytes, int mem_bytes, const int64_t* offsets,
                        int64_t n, int window, int per_window, int unit, uint64_t max_hash, SeqStats* st, const HashLauncher& launch,
                        mvs_hash_set** out);

// ---- mvs_capi_reads.hip: the counted set build (mvs_hash_set_create_counted, mvs_kmer_sketcher_finish) ----
// d_in (and d_w, or NULL: weight 1) hold the samples' values on the device, sample s at [off[s], off[s + 1]) with off[0] = 0,
// in any order.  -> a new set with abundances; histogram (host, n x 256, or NULL); distinct / passed per sample (or NULL).
int counted_build(mvs_ctx* c, const unsigned long long* d_in, const uint32_t* d_w, const std::vector<long long>& off, int64_t n,
                  uint32_t min_abundance, uint32_t max_abundance, int64_t* histogram, std::vector<long long>* distinct,
                  std::vector<long long>* passed, mvs_hash_set** out);

// ---- mvs_capi_sketch.hip ----
void note_rows_rewritten(mvs_sketch_set* s, int64_t lo, int64_t hi);

// ---- mvs_capi_compare.hip ----
int refresh_derived(mvs_ctx* c, const mvs_sketch_set* cs);
// the balanced order of the launch `segs` describes with the kernel arguments `a` (option plan_order; *d == NULL: use the static map)
int tile_order_for(mvs_ctx* c, const mvs::PairwiseArgs& a, const mvs::PlanSegs& segs, const unsigned** d, unsigned* per);
struct PackedOut {
    DevBuf* buf;               // grows as needed (ensure_buf)
    int64_t row0;              // rows are stored relative to this one
    int shift;                 // row field starts at this bit (16 bits of q, then the column)
    bool two_stage_only;       // do not fall back to the exact kernel: return kNeedExact and let the caller plan row blocks
};
constexpr int kNeedExact = 100;   // internal status of pairwise_launch (never leaves the library)

// Streamed output where the result is dense: the exact kernel writes one byte per cell (q or 0) into a row-major matrix
// instead of appending to a list; [sym_begin, sym_end) is the square the symmetric schedule works in -- larger than the
// launch's own rows when a caller walks a shard block by block and lets the mirror images land in later blocks' rows.
struct DenseOut {
    uint8_t* matrix;
    int64_t row0, ld;
    int64_t sym_begin, sym_end;
    unsigned int* flag;
};

// ---- the two-stage comparison, stage by stage ----
// What the filter stage leaves for the stages after it.  The stages are separate functions because the streamed output
// decides BETWEEN them how the kept cells leave the device (a list when they are few, the dense byte matrix when whole
// regions of the result are dense) and, for the matrix, launches the flagged tiles row block by row block.
struct TwoStage {
    mvs::PairwiseArgs a{};            // the filter launch's arguments: candidate list (pruned), tile grid, symmetric square
    bool tiles = false;               // the filter could flag tiles (tile-granular comparison)
    int n_tr = 0, n_tc = 0;           // its grid of 256 x 256 tiles
    unsigned long long n_cand = 0;    // listed candidates (an upper bound once the list has been pruned)
    int n_flagged = 0;                // flagged tiles
    std::vector<int> row_first;       // n_tr + 1 entries: where each tile row starts in the row-major list of flagged tiles
    const int* d_list = nullptr;      // that list on the device
    mvs::Options opt;                 // the options the filter stage ran with: the later stages use the same
    unsigned int* ext_flags = nullptr;   // in: tile flags live here (this launch's tile rows of a larger grid) instead of in
                                         // the context's own array -- the streamed pipeline keeps one array for the whole matrix
};

void fill_args(mvs_ctx* c, const mvs_sketch_set* s, const double* d_n2, int keep_mode, int64_t rb, int64_t re, int64_t cb,
               int64_t ce, bool symmetric, bool mirror_all, double keep_coeff, mvs::PairwiseArgs& a, const mvs::Options* o = nullptr);
// the running cell count starts at `start` (appending calls); kKeepCount: it stays what the device counter holds
constexpr unsigned long long kKeepCount = ~0ULL;
int set_cell_count(mvs_ctx* c, unsigned long long start);
int two_stage_filter(mvs_ctx* c, const mvs_sketch_set* s, const double* d_n2, double keep_coeff, int64_t capacity_hint,
                     bool hold_all, unsigned long long start, mvs::PairwiseArgs& a, TwoStage& ts, const mvs::Options* o = nullptr);
int two_stage_recheck(mvs_ctx* c, TwoStage& ts);
int two_stage_tiles(mvs_ctx* c, TwoStage& ts, int first, int count, bool timed);
bool two_stage_applies(mvs_ctx* c, const mvs_sketch_set* s, int64_t rb, int64_t re, int64_t cb, int64_t ce, double keep_coeff,
                       bool symmetric = true, const mvs::Options* o = nullptr);
int sort_on_device(mvs_ctx* c, mvs_cell* in, int64_t n, mvs_cell* out);
int pairwise_launch(mvs_ctx* c, const mvs_sketch_set* s, const double* d_n2, int keep_mode, int64_t rb, int64_t re,
                    int64_t cb, int64_t ce, bool symmetric, bool mirror_all, mvs_cell* raw, int64_t capacity,
                    unsigned long long start, unsigned long long* count, double keep_coeff = 0.05,
                    const PackedOut* po = nullptr, const DenseOut* dn = nullptr, const mvs::Options* o = nullptr);

// ---- mvs_capi_cluster.hip: what the consumers of kept cells share (clustering, linkage, dereplication) ----
// the threshold comparison of a set with itself at a Jaccard level, each row block's unsorted cells handed to
// consume(cells, n_cells, row_begin, row_end); the blocks arrive in ascending row order and tile [0, n)
using ConsumeCells = std::function<int(const mvs_cell*, int64_t, int64_t, int64_t)>;
int pairwise_feed(mvs_ctx* c, const mvs_sketch_set* s, const double* d_n2, double min_jaccard, double* compare_ms, long long* row_blocks,
                  const ConsumeCells& consume);
// *d_n2 := n norms on the device: norms_sq itself, or a copy of the host's in `staging` (queued on the context's stream)
int norms_on_device(mvs_ctx* c, const double* norms_sq, int mem_norms, int64_t n, DevBuf& staging, const double** d_n2);
// The argument checks of mvs_pairwise_cluster / _linkage / _derep, `noun` naming the consumer `k` (any of the three objects);
// an entry point's own checks follow them.
template <typename K>
int consumer_checks(const char* noun, const mvs_ctx* c, const mvs_sketch_set* s, const K* k, int mem_norms, double min_jaccard) {
    if (!c || !s || !k) return fail(MVS_E_INVALID, "NULL argument");
    if (!(min_jaccard > 0.0) || !(min_jaccard < 1.0)) return fail(MVS_E_INVALID, "min_jaccard = %g outside (0, 1)", min_jaccard);
    if (!mem_ok(mem_norms)) return fail(MVS_E_INVALID, "bad argument");
    if (k->ctx != c) return fail(MVS_E_INVALID, "the %s belongs to another context", noun);
    if (k->n != s->n) return fail(MVS_E_INVALID, "the %s holds %lld samples, the sketch set %lld", noun, (long long)k->n, (long long)s->n);
    return MVS_OK;
}
// ... and what follows the checks: nothing for an empty set, else the norms to the device and pairwise_feed under the marker
// range `entry`, with the comparison's time and row blocks added to `st`
int feed_consumer(const char* entry, mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double min_jaccard,
                  ConsumerStats& st, const ConsumeCells& consume);
// the body of mvs_ctx_cluster_stats / _linkage_stats / _derep_stats
int consumer_stats_out(const mvs_ctx* c, ConsumerStats mvs_ctx::*which, double* compare_ms, double* work_ms, int64_t* edges,
                       int64_t* row_blocks, int64_t* rounds);

// ---- mvs_capi_compare.hip: what the consumers of dense dots share (top-k, containment, level counts, the Jaccard operator,
// group sums, label sums, hclust's fill) ----
// the arguments of a dense-dots launch of set `s` over [r0, r1) x [cb, ce) into `out`
mvs::PairwiseArgs dots_args(const mvs_sketch_set* s, int64_t r0, int64_t r1, int64_t cb, int64_t ce, int32_t* out);
// Rows per block of such a consumer.  Its dots block (row_bytes per row) may take budget_bytes, which the caller derives from
// the device's free memory where its own allocations stand (a quarter of it, as mvs_pairwise_stream sizes its blocks).  A block
// has at least 1 row and at most 8192, at most cap_option where that is > 0 (the consumer's *_block_rows), at most max_rows.
int64_t dots_block_rows(size_t budget_bytes, size_t row_bytes, int cap_option, int64_t max_rows);
// the marker range of a consumer's dots launch, the refusal when the launcher rejects it, the kernel's name for check_kernel
struct DotsTexts {
    const char *marker, *rejected, *kernel;
};
// A consumer's walk over rows in blocks of R: the dense-dots kernel (option value `algo`) fills the R x (ce - cb) int32 block
// this object owns, then work(r0, r1, dots) queues the consumer's own launches over it.  With timing off nothing is recorded
// and nothing waits: a consumer synchronises where its `work` does.  With timing on run() waits once per block and adds the
// two stretches' times to *dots_ms and *work_ms.
struct DotsBlocks {
    mvs_ctx* c = nullptr;
    const mvs_sketch_set* s = nullptr;
    int64_t cb = 0, ce = 0, R = 0;
    int algo = 0;
    DotsTexts txt{};
    DevBuf dots;
    Event e[3];
    int init(mvs_ctx* ctx, const mvs_sketch_set* set, int64_t col_begin, int64_t col_end, int64_t block_rows, int dots_algo,
             const DotsTexts& texts) {
        c = ctx, s = set, cb = col_begin, ce = col_end, R = block_rows, algo = dots_algo, txt = texts;
        HIP_TRY(dots.alloc((size_t)R * (size_t)(ce - cb) * 4));
        if (c->timing)
            for (Event& x : e) HIP_TRY(x.create());
        return MVS_OK;
    }
    // rows [rb, re); work_ms and blocks may be NULL (a consumer that times its own stages, or keeps no count)
    template <typename Work>
    int run(int64_t rb, int64_t re, double* dots_ms, double* work_ms, long long* blocks, Work&& work) {
        int32_t* const d = dots.as<int32_t>();
        for (int64_t r0 = rb; r0 < re; r0 += R) {
            const int64_t r1 = std::min(r0 + R, re);
            if (c->timing) HIP_TRY(hipEventRecord(e[0], c->stream));
            {
                Range rd(c, txt.marker);
                int rc = mvs::launch_pairwise(c->stream, dots_args(s, r0, r1, cb, ce, d), 1, algo, c->opt);
                if (rc) return fail(rc, "%s", txt.rejected);
                rc = check_kernel(txt.kernel);
                if (rc) return rc;
            }
            if (c->timing) HIP_TRY(hipEventRecord(e[1], c->stream));
            if (const int rc = work(r0, r1, d)) return rc;
            if (c->timing) {
                HIP_TRY(hipEventRecord(e[2], c->stream));
                HIP_TRY(hipEventSynchronize(e[2]));
                float m0 = 0.f, m1 = 0.f;
                HIP_TRY(hipEventElapsedTime(&m0, e[0], e[1]));
                HIP_TRY(hipEventElapsedTime(&m1, e[1], e[2]));
                *dots_ms += m0;
                if (work_ms) *work_ms += m1;
            }
            if (blocks) ++*blocks;
        }
        return MVS_OK;
    }
};
// ---- what the consumers of units over two sorted hash lists share (mvs_intersect_cells, mvs_abund_overlap_cells, mvs_gather) ----
// The units of n_cells device cells over two sets, planned in the context's work space: c->ix_work is grown and carved into
// counters (256 bytes) | units per cell | their scan (n_cells + 1 entries each, rounded up to 256 bytes) | the scan's scratch,
// isect_plan<R> fills it -- d_result as it leaves it: zero for a cell in range, mark_bad: -1 for the others -- and the figures
// come back with ONE synchronisation of the stream.  `noun` names the caller in the messages.  ev (or NULL): two events that
// exist when timing is on, recorded around the planning launches then.  counters = false: only n_units is read back.
struct PlannedUnits {
    const long long* d_start = nullptr;               // where every cell's units start, n_cells + 1 entries; valid until ix_work grows
    long long n_units = 0;
    unsigned long long back[3] = {0, 0, 0};           // cells out of range, cells cut into several units, sum of 8 (|A| + |B|)
};
template <typename R>
int plan_units(mvs_ctx* c, const char* noun, const mvs_cell* d_cells, int64_t n_cells, const mvs_hash_set* hs_rows,
               const mvs_hash_set* hs_cols, int unit, R* d_result, bool mark_bad, Event* ev, bool counters, PlannedUnits& plan) {
    const size_t arr = (((size_t)n_cells + 1) * 8 + 255) & ~(size_t)255;
    size_t need = 0;
    int rc = mvs::isect_plan(c->stream, d_cells, n_cells, hs_rows->sizes.as<int32_t>(), hs_rows->n, hs_cols->sizes.as<int32_t>(),
                             hs_cols->n, unit, nullptr, nullptr, d_result, false, nullptr, nullptr, 0, &need);
    if (rc) return fail(rc, "%s: scan sizing failed", noun);
    rc = ensure_buf(c, c->ix_work, 256 + 2 * arr + need);
    if (rc) return rc;
    unsigned long long* d_counters = (unsigned long long*)c->ix_work.p;
    long long* d_units = (long long*)((char*)c->ix_work.p + 256);
    long long* d_start = (long long*)((char*)c->ix_work.p + 256 + arr);
    void* d_scan = (char*)c->ix_work.p + 256 + 2 * arr;
    const bool timed = ev && c->timing;
    if (timed) HIP_TRY(hipEventRecord(ev[0], c->stream));
    HIP_TRY(hipMemsetAsync(d_counters, 0, 32, c->stream));
    rc = mvs::isect_plan(c->stream, d_cells, n_cells, hs_rows->sizes.as<int32_t>(), hs_rows->n, hs_cols->sizes.as<int32_t>(), hs_cols->n,
                         unit, d_units, d_start, d_result, mark_bad, d_counters, d_scan, need, nullptr);
    if (rc) return fail(rc, "%s: planning the units failed", noun);
    rc = check_kernel("k_isect_count");
    if (rc) return rc;
    if (timed) HIP_TRY(hipEventRecord(ev[1], c->stream));
    plan.d_start = d_start;
    return read_back(c, c->stream, {{plan.back, d_counters, counters ? sizeof(plan.back) : 0}, {&plan.n_units, d_start + n_cells, 8}});
}

// The body of mvs_intersect_cells (R = int32_t) and mvs_abund_overlap_cells (R = mvs_abund_overlap): the checks, cells and results
// staged on the device where they are the host's, the plan, launch(d_cells, plan, d_out) -- the caller's units kernel --, the
// download, which leaves the entries of cells out of range what the caller had there, and the statistics of
// mvs_ctx_intersect_stats.
struct CellsTexts {
    const char *entry, *noun, *results, *out_name, *kernel;   // "mvs_intersect_cells", "intersect", "counts", "inter", "k_isect_units"
};
inline bool answered(int32_t r) { return r >= 0; }
inline bool answered(const mvs_abund_overlap& r) { return r.inter >= 0; }
template <typename R, typename Launch>
int cells_over_units(mvs_ctx* c, const CellsTexts& txt, const mvs_hash_set* hs_rows, const mvs_hash_set* hs_cols, const mvs_cell* cells,
                     int mem_cells, int64_t n_cells, R* out, int mem_out, Launch&& launch) {
    if (!c || !hs_rows) return fail(MVS_E_INVALID, "NULL argument");
    if (!hs_cols) hs_cols = hs_rows;
    if (!mem_ok(mem_cells) || !mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (n_cells < 0) return fail(MVS_E_INVALID, "n_cells = %lld is negative", (long long)n_cells);
    if (n_cells >= (1LL << 40)) return fail(MVS_E_RANGE, "n_cells too large");
    if (hs_rows->ctx != c || hs_cols->ctx != c) return fail(MVS_E_INVALID, "a hash set belongs to another context");
    c->ix_kernel_ms = 0.0;
    c->ix_units = c->ix_cut = c->ix_bytes = 0;
    if (n_cells == 0) return MVS_OK;
    if (!cells || !out) return fail(MVS_E_INVALID, "cells or %s is NULL", txt.out_name);
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, txt.entry);

    DevBuf dcells, dout;
    const mvs_cell* d_cells = cells;
    if (mem_cells == MVS_MEM_HOST) {
        if (dcells.alloc((size_t)n_cells * sizeof(mvs_cell)) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %lld cells failed", (long long)n_cells);
        HIP_TRY(hipMemcpyAsync(dcells.p, cells, (size_t)n_cells * sizeof(mvs_cell), hipMemcpyHostToDevice, c->stream));
        d_cells = (const mvs_cell*)dcells.p;
    }
    R* d_out = out;
    if (mem_out == MVS_MEM_HOST) {
        if (dout.alloc((size_t)n_cells * sizeof(R)) != hipSuccess)
            return fail(MVS_E_NOMEM, "hipMalloc of %lld %s failed", (long long)n_cells, txt.results);
        d_out = (R*)dout.p;
    }
    Event ev[4];                                      // around the plan, around the units
    if (c->timing)
        for (Event& x : ev) HIP_TRY(x.create());
    PlannedUnits plan;
    int rc = plan_units(c, txt.noun, d_cells, n_cells, hs_rows, hs_cols, c->opt.intersect_unit, d_out, mem_out == MVS_MEM_HOST, ev, true, plan);
    if (rc) return rc;
    if (c->timing) HIP_TRY(hipEventRecord(ev[2], c->stream));
    rc = launch(d_cells, plan, d_out);
    if (!rc) rc = check_kernel(txt.kernel);
    if (rc) return rc;
    if (c->timing) HIP_TRY(hipEventRecord(ev[3], c->stream));
    if (mem_out == MVS_MEM_HOST) {
        if (plan.back[0] == 0) {
            HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n_cells * sizeof(R), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        } else {
            // the entries of the cells out of range (count -1 on the device) stay what the caller had there
            std::vector<R> tmp((size_t)n_cells);
            HIP_TRY(hipMemcpyAsync(tmp.data(), d_out, (size_t)n_cells * sizeof(R), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (int64_t i = 0; i < n_cells; ++i)
                if (answered(tmp[(size_t)i])) out[i] = tmp[(size_t)i];
        }
    } else {
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (c->timing) {
        float a = 0.f, b = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&b, ev[2], ev[3]));
        c->ix_kernel_ms = (double)a + (double)b;
    }
    c->ix_units = plan.n_units;
    c->ix_cut = (long long)plan.back[1];
    c->ix_bytes = (long long)plan.back[2];
    if (plan.back[0] != 0)
        return fail(MVS_E_RANGE, "%llu cells name a sample outside the sets (%lld rows, %lld columns): they were not answered", plan.back[0],
                    (long long)hs_rows->n, (long long)hs_cols->n);
    return MVS_OK;
}

// the body of mvs_ctx_topk_stats / _contain_stats / _levels_stats
int dots_stats_out(const mvs_ctx* c, DotsStats mvs_ctx::*which, double* dots_ms, double* work_ms, int64_t* row_blocks, int64_t* block_rows);
// ---- mvs_capi_pca.hip: the eigensolver the ordinations share (mvs_pca_fit, mvs_pcoa_fit) ----
// Block subspace iteration with a Rayleigh-Ritz step for the leading eigenpairs of a symmetric operator of size d (the loop is
// described at the top of mvs_capi_pca.hip).  op(q, d_Q, d_Y): q is the orthonormal block on the host and d_Q the same on the
// device, both d x b row-major; the callable leaves the operator applied to it in d_Y, queued on the context's stream.
// -> theta (b Ritz values, descending), V (d x b row-major Ritz vectors), res (b residual norms) of the last iteration.
struct SubspaceResult {
    std::vector<double> theta, V, res;
    int iterations = 0, converged = 0;
    double ms = 0.0;   // the loop's time on the stream (timing enabled)
};
using SubspaceOp = std::function<int(const double* q, const double* d_Q, double* d_Y)>;
int subspace_iterate(mvs_ctx* c, int d, int b, int components, double tol, int max_iters, const SubspaceOp& op, SubspaceResult& out);
// column j of v (d x ld row-major) -> out[0 .. d): unit length, the entry of largest magnitude (the smaller index on ties) positive
void signed_unit_column(const double* v, int64_t d, int ld, int j, double* out);
// `count` results of a *_finish to the caller's buffer (NULL: not wanted), queued on the context's stream
template <typename T>
int give_out(mvs_ctx* c, T* dst, const void* d_src, int64_t count, int mem_out) {
    if (!dst || count <= 0) return MVS_OK;
    HIP_TRY(hipMemcpyAsync(dst, d_src, (size_t)count * sizeof(T), mem_out == MVS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           c->stream));
    return MVS_OK;
}
}  // namespace mvs_capi

#endif
