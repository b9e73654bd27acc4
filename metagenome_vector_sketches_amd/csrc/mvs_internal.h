// mvs_internal.h -- declarations shared by the translation units of libmvs_hip.so (not installed).
#ifndef MVS_INTERNAL_H
#define MVS_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/mvs_hip.h"

namespace mvs {

// One unit of projection work: a run of <= 65536 hashes of one sample (the layout of mvs_proj_unit, include/mvs_hip.h).
struct ProjUnit {
    int64_t begin;    // index of the unit's first hash in the CSR value array
    int32_t count;    // hashes in the unit
    int32_t sample;   // output row
    int32_t single;   // 1: the unit is the whole sample -> plain store, fused statistics; 0: combine with atomics
    int32_t flags;    // kProjTailGuard
};
constexpr int kProjUnitMax = 65536;
// the 512 hashes behind the unit's last full batch are not all inside the hash array: the main loop of k_project, whose
// look-ahead load is unclamped, leaves the unit's last group of four batches to the clamped leftover path
constexpr int kProjTailGuard = 1;

// ---- geometry of the pairwise kernel (mvs_pairwise.hip) ----
constexpr int kTile = 128;      // samples per workgroup tile edge (rows and cols)
constexpr int kBK = 128;        // bytes (= int8 k values) per staged k-slice
constexpr int kMaxLimbs = 4;
// limb code: 1..4 = signed base-256 limbs; kLimbsK3 = three planes (l0, l1, l0+l1) of signed base-128
// digits for the 3-pass Karatsuba product (|v| <= 8127)
constexpr int kLimbsK3 = MVS_LIMBS_K3;
inline __host__ __device__ int planes_of(int code) { return code & 0xff; }
inline __host__ __device__ bool is_k3(int code) { return code == kLimbsK3; }
inline bool limb_code_ok(int code) { return (code >= 1 && code <= kMaxLimbs) || code == kLimbsK3; }

// Tuning / diagnostic options of a context (mvs_ctx_set_option).  Initial values come from the MVS_*
// environment variables, read once by mvs_ctx_create; nothing below the C ABI reads the environment.
struct Options {
    int pairwise_filter = 1;        // 0 exact kernel on every cell; 1 two-stage for blocks >= 2^22 cells; 2 always two-stage
    int filter_variant = -1;        // -1 by block size; 0 128x128 ring; 1 256x256 ring; 8 256x256 ping-pong (7/9/10: its
                                    // variants); 3/5/6 other ring shapes / depths
    int exact_variant = 3;          // re-check kernel: 3 = tree reduction over a round of 64 pairs (default); 0 = 64 pairs per
                                    // round with a shuffle butterfly per pair, 1 quarter wave per pair, 2 = 16 per round
    int pairwise_variant = 8;       // exact kernel, two limbs: 8 = ping-pong 16x16x64 (7/9: its variants), 6 = 16x16x64 ring;
                                    // 0-5 = 32x32x32 tile / ring variants (the only ones for other limb codes)
    int pairwise_symmetric = 1;     // 0: compute every tile (no mirroring)
    int pairwise_debug = 0;         // profiling ablations; only honoured by a -DMVS_ABLATIONS build
    int sort = 0;                   // kept-cell sort: 0 by list length, 1 merge, 2 radix
    int project_variant = 0;        // projection kernel: 0 by dimension; 1 / 2 blocks per wave; 12 / 14 = 2 / 4 blocks per
                                    // wave sharing the first splitmix64 round; 24 = 14 with the deep carry-save tree and
                                    // the VALU epilogue
    int project_balance = 1;        // 1: units that would end behind the launch's ideal end are cut into pieces that fill the idle
                                    // workgroup slots (mvs_project_plan); 0: samples are cut at 65536 hashes only
    int markers = 0;                // 1: roctx ranges around the main entry points (rocprofv3 --marker-trace)
    int enable_k3 = 0;              // 1: mvs_sketch_set_create picks the three-plane Karatsuba code for |v| <= 8127
    int pairwise_map = 0;           // sub-patch an XCD takes in k_pairwise_pp: 0 = 4 rows x 8 cols, 1 = 8 x 4, 2 = 2 x 16
    int coarse_radix = 1;           // radix of the filter's coarse plane: 1 = smallest residual (default), 0 = ceil(max|v| / 127)
    int stream_dense = 1;           // mvs_pairwise_stream, dense results: 1 = dense byte matrix + count / scan / fill -- on a side
                                    // stream beside the next block's launch (exact kernel on whole row blocks; segmented filter),
                                    // on the context's stream where ONE filter pass feeds the matrix (short tile launches lose more
                                    // to the contention than the bubbles cost: 38.4 against 41.6 ms); 2 = always the context's
                                    // stream; 3 = always the side stream; 0 = packed list + sort
    int encode_stage_words = 64;    // device encoder: LDS words a chunk of unary codes may span before it falls back to atomics (tests)
    int stream_block_rows = 0;      // > 0: upper bound on the rows of a dense row block (tests); 0 = by the budget
    int recheck_mode = 1;           // re-check work split: 1 first round fixed + per-XCD counter, 2 counter only, 0 fixed stride, 3 eighths
    int recheck_blocks = 24;        // re-check grid in units of 256 workgroups (24: one round per wave at 100k samples)
    int cand_regions = 1;           // 1: filter waves leave up to 8 candidates in a region of their own (no atomic to wait for)
    int tile_dense_thr = 64;        // ping-pong filter: a wave with more candidates than this flags its 256 x 256 tile for the
                                    // exact kernel instead of listing them (0: list everything, give up on the block when the
                                    // list passes 1/128 of its cells -- the behaviour up to round 3)
    int stream_list_cells = 1 << 26;   // mvs_pairwise_stream, two-stage comparison: up to this many cells (candidates + cells
                                    // of flagged tiles, mirror images included) leave as ONE packed list; beyond it the dense
                                    // byte matrix takes the flagged tiles (tests lower it)
    int stream_pipeline = 1;        // mvs_pairwise_stream: 1 (default) = where the result looks dense (first tile row of the filter:
                                    // the probe, 1 % of a pass) the filter runs per SEGMENT of row blocks (5 passes), so the first
                                    // rows are final -- and on the link -- a millisecond after the call started (10 % dense 100k:
                                    // encoded rows 37.4 against 38.4 ms, CSR pieces 94.5 against 102.9 ms = 1.02 x the link);
                                    // 0 = always one filter pass over the whole row range first
    int pairwise_bdirect = 1;       // ping-pong kernels: 1 = the B operand's fragments come straight from the fragment-major plane into
                                    // registers (LDS carries the A operand only), 0 = both operands through LDS
    int fragment_major = 1;         // 1: the matrix-core kernels that copy 16 samples x 64 k values per instruction (ping-pong filter and
                                    // exact kernel, streaming search filter) read fragment-major copies of the coarse plane / limb planes
                                    // (PairwiseArgs::coarse_fm, planes_fm), built once per set; 0: the row-major planes (A/B, tests)
    int search_stream = 1;          // blocks of few rows x >= 4096 columns outside the symmetric schedule: 1 = the streaming
                                    // filter (rows resident in LDS, columns streamed into the matrix cores), 0 = the tile kernels
    int search_depth = 5;           // k_search_filter: register buffers of one k-slice x 64 columns per wave (3 .. 6); all but one
                                    // are in flight (10^6 x 2048: 256 queries 0.654 -> 0.622 ms, 512 queries 1.146 -> 1.034 from 3 to 5)
    int stream_trace = 0;           // 1: mvs_pairwise_stream prints the host-side time line of its row blocks to stderr
    int recode_rows_wg = 8;         // k_recode_rows: rows (= waves) per workgroup, 8 or 16
    int stream_copy = 0;            // streamed output, device -> host copies of the pieces: 0 = hipMemcpyAsync on the download stream (a blit
                                    // KERNEL on this stack: it holds CUs while the link drains it), 1 = hsa_amd_memory_async_copy (a DMA engine:
                                    // no CU involved; the copies' ordering then lives on the host threads of the streamed output)
    int stream_spec = 0;            // mvs_pairwise_stream_encoded, dense row blocks: 1 = a block's row passes (count, scan, fill, scan, encode)
                                    // are queued in one go with buffers sized from the blocks before it and ONE read-back at the end says
                                    // whether the sizes held (else the block is done again the careful way); 0 (default) = read the count
                                    // back before the fill and the record sizes before the encode (two host round trips per block).
                                    // Measured (10 % dense 100k): 33.5 against 33.0 ms -- the producer is not bound by its host round
                                    // trips but by the link's copy kernels on the CUs (profiles/r06_exp_dense_output.log)
    int stream_piece_mib = 32;      // mvs_pairwise_stream / mvs_cells_stream: MiB per pinned buffer = per device-to-host copy (a copy is a
                                    // blit kernel that fills the card while the link drains it: kernels that start beside one end with it)
    int plan_order = 1;             // block plans: 1 = filter launches of up to 2^20 tiles take the balanced tile order (PlanSegs::order),
                                    // 0 = the static super-patch map (A/B, tests)
    int plan_speculate = 0;         // block plans: second half of a plan sized from the previous plan's counts, no host round trip
    int plan_strip_wgs = 1 << 22;   // block plans: a rectangle whose padded grid holds more workgroups than this is cut into column
                                    // strips (a dispatch holds 2^32 work-items per dimension = 2^23 workgroups; tests lower it)
    int comm_timeout_s = 600;       // file transport: how long a rank waits for a peer's block before it gives up
    int topk_dots = 0;              // mvs_pairwise_topk: dots of a row block from 0 = the matrix-core kernels (launch_pairwise algo 0),
                                    // 1 = the vector-ALU kernel (A/B, tests); same selection, same result
    int topk_block_rows = 0;        // mvs_pairwise_topk: > 0 = upper bound on the rows of a block (tests); 0 = by the device budget
    int contain_dots = 0;           // mvs_pairwise_contain: dots of a row block from 0 = the matrix-core kernels, 1 = the vector-ALU
                                    // kernel (A/B, tests); same selection, same result
    int contain_block_rows = 0;     // mvs_pairwise_contain: > 0 = upper bound on the rows of a block (tests); 0 = by the device budget
    int levels_dots = 0;            // mvs_pairwise_levels: dots of a row block from 0 = the matrix-core kernels, 1 = the vector-ALU
                                    // kernel (A/B, tests); same counts
    int levels_block_rows = 0;      // mvs_pairwise_levels: > 0 = upper bound on the rows of a block (tests); 0 = by the device budget
    int pcoa_dots = 0;              // mvs_jaccard_apply / mvs_pcoa_*: dots of a row block from 0 = the matrix-core kernels, 1 = the vector-ALU
                                    // kernel (A/B, tests); same result
    int pcoa_block_rows = 0;        // mvs_jaccard_apply / mvs_pcoa_*: > 0 = upper bound on the rows of a block (tests); 0 = by the device budget
    int groups_dots = 0;            // mvs_group_sums / mvs_permanova: dots of a row block from 0 = the matrix-core kernels, 1 = the vector-ALU
                                    // kernel (A/B, tests); same sums
    int groups_block_rows = 0;      // mvs_group_sums / mvs_permanova: > 0 = upper bound on the rows of a block (tests); 0 = by the device budget
    int gram_slab_rows = 65536;     // mvs_sketch_moments / mvs_pca_fit: samples per slab of the transposed scratch copy, 64 .. 65536
                                    // (rounded down to a multiple of 64; tests lower it to force several slabs)
    int gram_variant = 0;           // k_gram_tiles: 0 = by shape (128 x 128 tiles for one or two limbs and d >= 128, else 64 x 64),
                                    // 1 = always 64 x 64 (A/B, tests); same result
    int cluster_cells = 0;          // mvs_pairwise_cluster: cells the staging buffer of a row block holds; 0 = a quarter of the free
                                    // device memory (never more than the block can produce); tests lower it
    int cluster_block_rows = 0;     // mvs_pairwise_cluster: > 0 = upper bound on the rows of a block (tests); 0 = by pairwise_block_cells
    int intersect_unit = 2048;      // mvs_intersect_cells: elements of a pair's shorter hash list that one unit of work (one wave) covers
    int gather_batch = 16;          // mvs_gather: rounds queued between two read-backs of the walk's state, 1 .. 1024
    int kmer_unit = 17408;          // mvs_hash_set_from_sequences: k-mer positions of one sample that one unit of work (one workgroup)
                                    // covers, 64 .. 32768 (the default is 256 threads x 68 positions: LDS reads 17 dwords apart)
    int kmer_capacity = 0;          // mvs_hash_set_from_sequences: > 0 = values the staging list of the first trip holds (tests force
                                    // the second trip with it); 0 = the expected number of kept values plus a margin
    int abund_unit = 4096;          // counted set build: sorted values that one unit of work (one wave) of the run-sum passes covers,
                                    // 64 .. 2^20; never changes a result (tests lower it to put borders everywhere)
    int abund_big_segment = 1 << 18;   // counted set build: a sample of more values than this is sorted by a device-wide radix sort
                                    // of its own, the others by the segmented sort (one workgroup per sample there); >= 64.  The
                                    // largest size at which the segmented sort still wins in bulk (2^26 values as samples
                                    // of 2^18: 9.1 against 26.4 ms; of 2^20: 34.7 against 11.9 ms)
    double pairwise_block_cells = 1099511627776.0;   // row-chunk bound of mvs_pairwise_rows (2^40 cells)
};

constexpr int kMaxTopk = 256;   // largest k of mvs_pairwise_topk
constexpr int kMaxLevels = 64;  // most levels of mvs_pairwise_levels (MVS_MAX_LEVELS)

constexpr int kCandRegion = 8;   // candidate entries a filter wave can leave in its own region (one 64-byte line)

constexpr unsigned long long kStampSlots = 400000ULL;   // workgroups the time-stamp buffer of an ablation build holds

struct PairwiseArgs {
    const int8_t* planes;   // [(row*limbs + limb) * d_pad + k]
    const int8_t* planes_fm;  // the same values fragment-major, or NULL: [((row / 16 * limbs + limb) * (d_pad / 64) + k / 64) * 1024 + lane * 16],
                              // lane = (k / 16 % 4) * 16 + row % 16 (see coarse_fm); read by the ping-pong exact kernel (two limbs)
    int64_t n;              // samples
    int64_t n_alloc;        // allocated (zero padded) rows
    int d;
    int d_pad;
    int limbs;              // limb code (see kLimbsK3)
    int64_t row_begin, row_end;   // row range of this call
    int64_t sym_begin, sym_end;   // symmetric schedule: the square whose lower triangle is skipped and produced by mirroring
                                  // (the call's own row range unless a caller walks a larger square block by block)
    int64_t col_begin, col_end;   // column range (dots) / [0,n) for the comparison
    // comparison outputs
    const double* norms_sq;       // n
    const int32_t* cand_thr;      // n_alloc (+ 1, launch_cand_thr's mark): conservative integer per-sample threshold part
    int keep_mode;
    double keep_coeff;            // 0.05 in the reference's keep test; j/(1+j) for a Jaccard > j search
    mvs_cell* cells;
    unsigned long long capacity;
    unsigned long long* counter;  // number of kept cells (may exceed capacity)
    // streamed output (mvs_pairwise_stream): when non-NULL a kept cell is ONE word in `packed` instead of an mvs_cell:
    // (row - pack_row0) << pack_shift | col << 16 | q (16 bits) -- sorts by (row, col) as an integer
    unsigned long long* packed;
    int64_t pack_row0;
    int pack_shift;
    // dense output (mvs_pairwise_stream where the two-limb exact kernel runs): one byte per cell, q or 0, row-major with
    // leading dimension dense_ld (a multiple of 128), row dense_row0 first; *dense_flag is set when a kept cell's q is
    // not in 1..255 (the byte cannot say so: the caller redoes that block through the packed list)
    uint8_t* dense;
    int64_t dense_row0, dense_ld;
    unsigned int* dense_flag;
    // dense outputs (dots mode)
    int32_t* dots;                // (row_end-row_begin) x (col_end-col_begin)
    int mirror_all;               // 1: every kept (row, col) is appended as (col, row) too (the transposed
                                  //    block belongs to another shard and is not computed there)
    int symmetric;                // 1: tiles strictly below the diagonal of the row range are skipped and
                                  //    produced by mirroring the kept cells of their transposes
    int debug_flags;              // profiling ablations (-DMVS_ABLATIONS builds only): 1 skip k-loop, 2 skip epilogue,
                                  // 4 filter epilogue: injected candidates instead of the accumulators' verdict
    int map_mode;                 // workgroup -> tile map: 0 = 4 x 8 sub-patch per XCD, 1 = 8 x 4, 2 = 2 x 16 (option pairwise_map),
                                  // 3 = 16 x 2 (set by the launchers for blocks less than 16 tile rows high)
    // two-stage comparison (coarse filter + exact re-check, see "filter" in mvs_pairwise.hip)
    const int8_t* coarse;         // [row * d_pad + k], c = round(v / radix[row]), |c| <= 127
    const int8_t* coarse_fm;      // the same values fragment-major, or NULL: [(row / 16 * (d_pad / 64) + k / 64) * 1024 + lane * 16],
                                  // lane = (k / 16 % 4) * 16 + row % 16 -- 1 KiB = one B fragment of v_mfma_i32_16x16x64_i8 for 16
                                  // rows and 64 k values, what a wave of the streaming search filter loads with ONE coalesced
                                  // instruction (from the row-major plane the same instruction touches 16 rows, 64 bytes each)
    const float4* fmeta;          // n_alloc: per-row filter constants {s, w, a, p}
    int2* cand;                   // candidate list: {row, col | mirror << 31}
    unsigned long long cand_capacity;
    unsigned long long* cand_counter;
    unsigned long long cand_limit;   // once the counter is beyond this the remaining filter tiles and the re-check
                                     // give up at once: the caller falls back to the exact kernel
    unsigned long long* stamps;      // ablation builds (pairwise_debug bit 8): kStampSlots x 8 words, per workgroup of
                                     //    k_pairwise_pp {XCC / HW id, start, end, k-loop end, epilogue phases} on the
                                     //    100 MHz realtime clock; the library dumps them to /tmp/mvs_stamps.bin
                                     //    (tools/exp/stamps.py reads that)
    int recheck_mode;                    // work split of k_exact_pairs_tree (see there)
    unsigned long long* recheck_queue;   // 8 zeroed counters, 64 bytes apart: the re-check hands its rounds out per XCD
    unsigned int* cand_hdr;          // per (workgroup, wave) region of the ping-pong filter: number of candidates the wave
    int2* cand_ent;                  //    left in its kCandRegion entries (0: none, or it went to the list itself)
    unsigned int* cand_stop;         // set by the wave that takes the counter past the limit; lives on its own cache
                                     // line (polling the counter itself queues behind its atomics)
    // Tile-granular two-stage comparison (ping-pong filter on 256 x 256 tiles).  A filter wave that finds more than
    // tile_dense_thr candidates in its 128 x 64 cells does not list them: it flags its tile, tile_flag[tr * tile_flag_ld +
    // tc] (tr, tc relative to row_begin / col_begin in units of 256), and the exact ping-pong kernel later computes the
    // flagged tiles -- and only those -- from tile_list (four 128 x 128 tiles each).  Candidates that other waves of a
    // flagged tile had already listed are dropped by k_cand_prune before the re-check, so no cell is produced twice.
    unsigned int* tile_flag;         // NULL: every candidate is listed (ring filters, option tile_dense_thr = 0)
    int tile_flag_ld;
    unsigned int tile_dense_thr;
    unsigned int* tile_flag_count;   // flagged tiles so far; beyond tile_flag_limit the filter raises cand_stop (the result
    unsigned int tile_flag_limit;    //    is dense nearly everywhere: the exact kernel alone is faster)
    const int* tile_list;            // k_pairwise_pp<0>: flagged filter tiles (row-major ids), NULL = the whole grid
    int tile_list_n;
    // Block plans (mvs_plan_*: a rank's share of the symmetric multi-rank schedule in ONE launch, PlanSegs below).
    // [row_begin, row_end) x [col_begin, col_end) is then the FRAME the tile flags, the flagged-tile list and the candidate
    // pruning index into; the tiles themselves come from the launch's segments.  plan = 1 also keeps `symmetric` together
    // with `mirror_all`: inside the square [sym_begin, sym_end)^2 the symmetric schedule rules (tiles below the diagonal
    // skipped, cells above it mirrored), every kept cell outside it is mirrored (its transposed block is nobody else's).
    int plan;
    unsigned long long cand_region_base;   // first candidate region of this launch (several filter launches share the arrays)
};

// The rectangles of one plan launch of k_pairwise_pp: a 1-D grid, segment s owning workgroups [wg_begin[s], wg_begin[s + 1])
// = n_spr x n_spc super-patches of 256 workgroups (map_tile inside each, so the XCD-aware placement of the single-block
// launch carries over: every segment starts on a multiple of 256 workgroups).  n = 0: the launch is one block on the 2-D grid.
constexpr int kPlanSegs = 16;
struct PlanSegs {
    int n;
    unsigned wg_begin[kPlanSegs + 1];
    int n_tr[kPlanSegs], n_tc[kPlanSegs], n_spc[kPlanSegs];
    long long i_begin[kPlanSegs], j_begin[kPlanSegs];
    // Balanced order (plan_tile_order; NULL: the static map above): the tiles the launch really computes, XCD label x
    // (blockIdx.x % 8) takes entries [x * order_per, (x + 1) * order_per) -- its share of every super-patch, in sub-patch
    // order, so that the XCDs still walk the same super-patch at the same time (panels shared through the memory-side cache)
    // but no XCD carries more tiles than another: a triangle's static sub-patches hold 32, 26, 10 or 0 tiles, and a launch
    // of a few rounds (1225 tiles of a rank's diagonal block, 820 of a 10k x 10k comparison) waited for its fullest XCD --
    // 174 tiles where 154 would do.  Entry = segment << 28 | tile row << 14 | tile column; ~0u = no tile.
    const unsigned* order;
    unsigned order_per;
};

// Which 256 x 256 tiles of the dense byte matrix can hold a kept cell (tile-granular comparison feeding the matrix): the
// tiles the filter flagged (the exact kernel wrote them whole), their mirror images, and the tiles the re-check's kept
// cells were scattered into.  The row -> CSR passes read only those; nothing else of the matrix is ever cleared or read.
struct DenseActive {
    const unsigned int* flags;   // [n_tr * n_tc] of the matrix's tile grid (rows relative to its first row); NULL: every tile
    const unsigned int* touch;   // same shape
    int n_tr, n_tc;
    int o;                       // tile column of the matrix's first row (row_begin / 256): mirror of (tr, tc) = (tc - o, tr + o)
    int sym;                     // the symmetric schedule was on: mirror images of flagged tiles exist
    long long row_rel0;          // first row of the launch, relative to the matrix's first row
};

// per-row statistics of the coarse plane: radix m, sum c^2, sum r^2 (r = v - m*c), and whether the row's sum
// of squares reaches 2^31 (its dots may wrap: the filter then passes every pair of that row on to the re-check)
struct CoarseRow {
    int32_t radix;
    int32_t c2;
    int32_t r2;
    int32_t big;
};

// d_sumsq / d_max_abs non-NULL: fused statistics of the samples that are one unit (d_sumsq zeroed by the caller); the rows
// of samples cut into several units are final only after the launch and get theirs from launch_stats
int launch_project(hipStream_t stream, const uint64_t* d_hashes, const ProjUnit* d_units, int64_t n_units,
                   int d, int32_t* d_out, int variant, unsigned long long* d_sumsq, unsigned long long* d_max_abs);
// workgroups of the k_project instantiation `variant` (with / without statistics) that one CU holds at a time; <= 0 on error
int project_blocks_per_cu(int variant, bool stats);
// 64-dim blocks per wave of a variant, and the workgroups one unit takes at dimension d
inline int project_ny(int variant, int d) { return ((d + 63) / 64 + 4 * (variant % 10) - 1) / (4 * (variant % 10)); }
int launch_sumsq(hipStream_t stream, const int32_t* d_sk, int64_t n, int d, int64_t* d_out);
int launch_saturate_i16(hipStream_t stream, const int32_t* d_in, int64_t n, int16_t* d_out);
int launch_stats(hipStream_t stream, const int32_t* d_sk, int64_t n, int d, int64_t* d_sumsq,
                 unsigned long long* d_max_abs);

int launch_max_abs(hipStream_t stream, const void* d_sk, int elem_bytes, int64_t n_elems,
                   unsigned long long* d_out);
int launch_limb_split(hipStream_t stream, const void* d_sk, int elem_bytes, int64_t n_rows, int d, int limbs,
                      int8_t* d_planes, int d_pad, int64_t row_offset);
int launch_cand_thr(hipStream_t stream, const double* d_norms_sq, int64_t n, int64_t n_alloc, int d,
                    double coeff, int32_t* d_thr);
// mode 0: comparison (kept cells), mode 1: dense dots.  algo 0: MFMA, 1: vector ALU.
int launch_pairwise(hipStream_t stream, const PairwiseArgs& a, int mode, int algo, const Options& opt);
// top-k selection over a block of dense dots (mvs_topk.hip): rows [row0, row0 + rows) x columns [c0, c0 + ld) -> k padded cells
// per row at (row - out_row0) * k of d_pad, their number in d_counts[row - out_row0]; then the padded lists -> consecutive cells
int launch_topk_select(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                       const double* d_norms_sq, int d, int k, int exclude_self, mvs_cell* d_pad, int* d_counts,
                       int64_t out_row0);
int launch_topk_compact(hipStream_t stream, const mvs_cell* d_pad, const int* d_counts, const int64_t* d_offs, int64_t rows,
                        int k, mvs_cell* d_out);
// containment selection over a block of dense dots (mvs_contain.hip; the rule is stated there and in include/mvs_hip.h):
// zz = slack * slack (one rounding, on the host), zsign = the sign of slack, dd = (double)d, pretest = 1 for slack >= 0.
// thr: the integer pre-test value of every sample; count: kept cells per row of the block; scan: offs[r] = *d_total + cells of
// the block's earlier rows, *d_total advances; fill: the rows' cells in (row, col) order at their offsets -- a row that does
// not fit `capacity` is left out
struct ContainRule {
    double c, zz, dd;
    int zsign, mode, pretest;
};
int launch_contain_thr(hipStream_t stream, const double* d_norms_sq, int64_t n, const ContainRule& ru, int* d_thr);
int launch_contain_count(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                         const double* d_norms_sq, const int* d_thr, const ContainRule& ru, int* d_counts);
int launch_contain_scan(hipStream_t stream, const int* d_counts, int64_t rows, long long* d_offs, unsigned long long* d_total);
int launch_contain_fill(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                        const double* d_norms_sq, const int* d_thr, const ContainRule& ru, const int* d_counts,
                        const long long* d_offs, mvs_cell* d_cells, int64_t capacity);
// neighbour counts at m Jaccard levels over a block of dense dots (mvs_levels.hip; the rule is stated there and in
// include/mvs_hip.h).  prep: d_thr[i] = every sample's part of the integer pre-test at the lowest level's coefficient, *d_flag = 1
// if a column of the range has a negative norm (the caller zeroes it first).  count: row r of the block -> d_deg[r * m + l]
// (NULL: not wanted), the rows' values added to d_total[l]; d_coef: m coefficients t / (1 + t)
int launch_levels_prep(hipStream_t stream, const double* d_norms_sq, int64_t n, int64_t col_begin, int64_t col_end, double coef0, int d,
                       int* d_thr, int* d_flag);
int launch_levels_count(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                        const double* d_norms_sq, const double* d_coef, int m, int d, const int* d_thr, const int* d_neg_flag,
                        int32_t* d_deg, unsigned long long* d_total);
// exact second moments over the sample axis and the device side of the PCA (mvs_gram.hip).  gram_limbs: limbs read and their
// radix for a limb code.  gram_slab: rows [row0, row_end) (at most 65536) are transposed into d_T (gram_scratch_bytes) and
// their products added to d_gram (d x d, zeroed by the caller before the first slab); variant: option gram_variant.  colsums: added to d_sums (d, zeroed).
// pca_matmul: Y = C Q (C d x d, Q and Y d x b row-major).  pca_ritz: V = Q S, W = Y S, R = W - V diag(theta), res[i] = ||R[:, i]||.
// pca_scores: rows [rb, re) of the planes against V (d x c row-major) minus off[c] -> d_scores ((re - rb) x c).
void gram_limbs(int code, int* L, int* W);
size_t gram_scratch_bytes(int d, int code, int64_t slab_rows);
int launch_gram_slab(hipStream_t stream, const int8_t* d_planes, int code, int d, int d_pad, int64_t row0, int64_t row_end, int8_t* d_T,
                     unsigned long long* d_gram, int variant);
int launch_gram_colsums(hipStream_t stream, const int8_t* d_planes, int code, int d, int d_pad, int64_t rb, int64_t re,
                        unsigned long long* d_sums);
int launch_pca_matmul(hipStream_t stream, const double* d_C, const double* d_Q, int d, int b, double* d_Y);
int launch_pca_ritz(hipStream_t stream, const double* d_Q, const double* d_Y, const double* d_S, const double* d_theta, int d, int b,
                    double* d_V, double* d_W, double* d_R, double* d_res);
int launch_pca_scores(hipStream_t stream, const int8_t* d_planes, int code, int d, int d_pad, int64_t rb, int64_t re, const double* d_V,
                      const double* d_off, int c, double* d_scores);
// the Jaccard kernel matrix of a block of dense dots times a thin block of vectors (mvs_kapply.hip; the rule is stated there and in
// include/mvs_hip.h): Y (rows x b) = k(rows x ld) Xp, Xp the ld x b operand zero-padded to apply_padded_cols(ld) rows of
// apply_padded_b(b) doubles
int64_t apply_padded_cols(int64_t cols);
int apply_padded_b(int b);
int launch_jaccard_apply(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                         const double* d_norms_sq, int d, double floor_, const double* d_Xp, int b, double* d_Y);
// within-group sums of quantised squared distances for many labellings at once (mvs_groups.hip; the rule is stated there and in
// include/mvs_hip.h).  quantise: a block of dense dots becomes uint32 weights in place.  transpose: labels (slots x m bytes) ->
// d_packed, m x group_label_quads(slots) dwords.  sums: the block's ORDERED-pair sums are added to d_acc (slots x groups);
// rows x ld must stay below 2^34 (MVS_E_INVALID otherwise) and the caller clears d_acc between blocks
int64_t group_label_quads(int64_t slots);
int launch_dist_quantise(hipStream_t stream, int32_t* d_cells, int64_t rows, int64_t ld, int64_t row0, int64_t c0, const double* d_norms_sq,
                         int d, double floor_);
int launch_labels_transpose(hipStream_t stream, const uint8_t* d_labels, int64_t slots, int64_t m, uint32_t* d_packed);
int launch_group_sums(hipStream_t stream, const uint32_t* d_w, int64_t rows, int64_t ld, int64_t f0, const uint32_t* d_packed, int64_t slots,
                      int groups, unsigned long long* d_acc);
// single-linkage clustering over device cell lists (mvs_cluster.hip): union-find rounds over parent[n] -- d_counters: [0] cells
// with row != col, [1] cells with an index outside [0, n), [2] cells whose endpoints still have different roots -- and the
// finish passes (cluster ids by ascending root, sizes, representatives)
int launch_cluster_init(hipStream_t stream, int32_t* d_parent, int32_t* d_degree, int64_t n);
int launch_cluster_hook(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, int32_t* d_parent, int32_t* d_degree, int64_t n,
                        bool first, unsigned long long* d_counters);
int launch_cluster_flatten(hipStream_t stream, int32_t* d_parent, int64_t n);
int launch_cluster_verify(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, const int32_t* d_parent, int64_t n,
                          unsigned long long* d_counters);
int cluster_finish(hipStream_t stream, const int32_t* d_parent, const double* d_norms_sq, int64_t n, int32_t* d_is_root, int32_t* d_ids,
                   int32_t* d_labels, int32_t* d_sizes, int32_t* d_rep, unsigned long long* d_best, void* d_scratch,
                   size_t scratch_bytes, size_t* scratch_needed);
// the single-linkage tree over device cell lists (mvs_linkage.hip): Boruvka rounds that turn the forest and a list into the
// maximum spanning forest of both.  One round = slots, select passes 0 (key; counts the crossing edges) / 1 (pair) / 2 (pick),
// hook, jump.  d_counters (8 words): [0] fed cells with row != col in range, [1] fed cells with an index outside [0, n),
// [2] edges between different components, [3] cells in forest_next, [4] internal faults (must stay 0), [5] links above a level
struct LinkState {
    int64_t n = 0;
    int d = 0;
    const double* norms_sq = nullptr;       // n doubles on the device
    const mvs_cell* forest = nullptr;       // n_forest cells, row < col
    int64_t n_forest = 0;
    mvs_cell* forest_next = nullptr;        // room for `capacity` cells
    int64_t capacity = 0;
    int32_t* comp = nullptr;                // n each
    int32_t* next = nullptr;
    unsigned long long* best_key = nullptr;
    unsigned long long* best_pair = nullptr;
    unsigned long long* best_idx = nullptr;
    unsigned long long* counters = nullptr;
};
int launch_link_identity(hipStream_t stream, int32_t* d_comp, int64_t n);
int launch_link_slots(hipStream_t stream, const LinkState& s);
int launch_link_select(hipStream_t stream, const LinkState& s, const mvs_cell* d_cells, int64_t n_cells, int pass, bool first);
int launch_link_hook(hipStream_t stream, const LinkState& s, const mvs_cell* d_cells);
int launch_link_jump(hipStream_t stream, const LinkState& s);
int link_sorted(hipStream_t stream, const LinkState& s, mvs_link* d_tmp, mvs_link* d_links, void* d_scratch, size_t scratch_bytes,
                size_t* scratch_needed);
int launch_link_cells(hipStream_t stream, const mvs_link* d_links, int64_t n_links, double level, mvs_cell* d_cells, int64_t capacity,
                      unsigned long long* d_counters);
// greedy dereplication over device cell lists in rank space (mvs_derep.hip): rows arrive block by block in ascending order.
// Per block: pre (cells against the rows before the block; counts the fed cells), then rounds of scan + decide until no row
// of the block is undecided, a last scan (members decided early may still find an earlier representative), link.
// d_counters (8 words): [0] fed cells with row != col in range, [1] fed cells naming a row outside the block or a column
// outside [0, n), [2] rows of the block still undecided after a decide, [3] representatives (finish), [4] entries of an order
// that is no permutation (finish)
constexpr int32_t kDerepUndecided = 0, kDerepRep = 1, kDerepMember = 2;
constexpr int32_t kDerepNone = 0x7fffffff;      // assign[r]: no representative linked to r has been seen
struct DerepState {
    int64_t n = 0;
    int32_t* state = nullptr;                 // n each
    int32_t* assign = nullptr;                // the earliest representative linked to the row so far
    int32_t* blocked = nullptr;               // the last round in which the row had an undecided earlier neighbour
    int2* link = nullptr;                     // (dot, q) of the cell (row, assign[row]); (0, -1) for a representative
    unsigned long long* counters = nullptr;
};
int launch_derep_init(hipStream_t stream, const DerepState& s);
int launch_derep_pre(hipStream_t stream, const DerepState& s, const mvs_cell* d_cells, int64_t n_cells, int64_t rb, int64_t re);
int launch_derep_scan(hipStream_t stream, const DerepState& s, const mvs_cell* d_cells, int64_t n_cells, int64_t rb, int64_t re,
                      int round);
int launch_derep_decide(hipStream_t stream, const DerepState& s, int64_t rb, int64_t re, int round);
int launch_derep_link(hipStream_t stream, const DerepState& s, const mvs_cell* d_cells, int64_t n_cells, int64_t rb, int64_t re);
// order == NULL: identity.  check: marks (n int32, zeroed) count how often each sample is named -> counters[4];
// scatter: rows -> the caller's samples (d_sizes zeroed by the caller), representatives -> counters[3]
int launch_derep_order_check(hipStream_t stream, const int32_t* d_order, int64_t n, int32_t* d_marks, unsigned long long* d_counters);
int launch_derep_scatter(hipStream_t stream, const DerepState& s, const int32_t* d_order, int32_t* d_rep_of, int32_t* d_link_dot,
                         int32_t* d_link_q, int32_t* d_sizes);
// row i of dst (n_rows rows of row_bytes bytes, a multiple of 16) = row d_rows[i] of src; rows outside [0, n_src) are counted in
// *d_bad and left alone
int launch_gather_rows(hipStream_t stream, const int8_t* d_src, int64_t n_src, const int32_t* d_rows, int64_t n_rows, int64_t row_bytes,
                       int8_t* d_dst, unsigned long long* d_bad);
// two-stage comparison for two base-256 limbs: coarse plane + row statistics from the limb planes,
// per-call filter constants, the one-pass filter
// that appends candidate pairs, and the exact re-check of the candidates that appends kept cells
int launch_coarse_build(hipStream_t stream, const int8_t* d_planes, int64_t n, int64_t n_alloc, int d_pad,
                        int8_t* d_coarse, CoarseRow* d_rows, int radix_mode);
// limb split + coarse build + fragment-major copy of a row range in one pass (k_recode_rows); false: no fused kernel for
// this geometry (the caller takes the three separate launches)
int launch_planes_from_wire(hipStream_t stream, const int8_t* d_lo_wire, const int8_t* d_coarse_fm, const CoarseRow* d_rows,
                            int64_t count, int d_pad, int8_t* d_planes, const unsigned char* d_need = nullptr, int64_t skip_first = 0,
                            int64_t skip_count = 0);
int launch_rows_needed(hipStream_t stream, const PairwiseArgs& a, int n_tr, int n_tc, int64_t f0, int64_t f1, int64_t n_rows,
                       unsigned char* d_need);
bool launch_recode_rows(hipStream_t stream, const void* d_sk, int elem_bytes, int64_t n_rows, int64_t count, int d, int d_pad,
                        int8_t* d_planes, int8_t* d_coarse_fm, CoarseRow* d_rows, int radix_mode, int rows_per_wg);
// fragment-major copy of the coarse plane (PairwiseArgs::coarse_fm) / of the limb planes (planes_fm): `limbs` planes per row
int launch_coarse_fm(hipStream_t stream, const int8_t* d_coarse, int64_t n_alloc, int d_pad, int8_t* d_fm, int limbs = 1);
// true when launch_pairwise / launch_exact_tiles run the kernel that reads planes_fm for this set
bool exact_reads_fm(const PairwiseArgs& a, const Options& opt);
int launch_filter_meta(hipStream_t stream, const CoarseRow* d_rows, const double* d_norms_sq, int64_t n,
                       int64_t n_alloc, int d, double coeff, float4* d_meta);
int launch_filter(hipStream_t stream, const PairwiseArgs& a, const Options& opt, const unsigned* order = nullptr, unsigned order_per = 0);
struct PlanSegs;
bool filter_order_geometry(const PairwiseArgs& a, const Options& opt, PairwiseArgs* b, PlanSegs* segs);
// block plans (mvs_plan_*): rectangles {row_begin, row_end, col_begin, col_end} -> the segments of one launch (returns its
// 1-D grid in workgroups, 0: empty, -1: too many rectangles / too large for one launch), and that launch of the ping-pong filter
long long plan_segments(const int64_t (*blocks)[4], int n, PlanSegs* segs);
int launch_filter_plan(hipStream_t stream, const PairwiseArgs& a, const PlanSegs& segs, long long workgroups);
// the balanced order of a plan launch (host): per XCD label the tiles it computes, order_per entries each (padded with ~0u);
// false when a coordinate does not fit an entry or the launch is too large for a list to pay (the static map is used then)
bool plan_tile_order(const PairwiseArgs& a, const PlanSegs& segs, std::vector<unsigned>* order, unsigned* per);
int launch_exact_pairs(hipStream_t stream, const PairwiseArgs& a, const Options& opt, long long n_hint = -1);
// candidate regions of the ping-pong filter: how many (workgroups x 8 waves) launch_filter's grid has for this block, 0 if
// the variant it would pick appends with atomics only; k_cand_gather moves the regions' contents into the candidate list
int64_t filter_region_count(const PairwiseArgs& a, const Options& opt);
int launch_cand_gather(hipStream_t stream, const PairwiseArgs& a, int64_t n_regions);
// tile-granular two-stage comparison: does launch_filter pick a kernel that can flag tiles for this block, and the tile
// grid (256 x 256) it works on; flags -> per-tile-row counts -> row-major list of flagged tile ids (d_list holds the total);
// candidates whose tile is flagged are dropped (d_out / d_out_count: the pruned list); the exact kernel on a run of the list
bool filter_flags_tiles(const PairwiseArgs& a, const Options& opt);
// true when launch_filter would take the streaming search filter for this block (few rows, many columns, no symmetry)
bool filter_streams_rows(const PairwiseArgs& a, const Options& opt);
// ... or another filter kernel that reads the fragment-major coarse plane (the ping-pong tile filter)
bool filter_streams(const PairwiseArgs& a, const Options& opt);
void filter_tile_grid(const PairwiseArgs& a, int* n_tr, int* n_tc);
int launch_tile_count(hipStream_t stream, const unsigned int* d_flags, int n_tr, int n_tc, int* d_row_count);
int launch_tile_list(hipStream_t stream, const unsigned int* d_flags, int n_tr, int n_tc, const int* d_row_count, int* d_list,
                     int cap = 0x7fffffff);
int launch_cand_prune(hipStream_t stream, const PairwiseArgs& a, unsigned long long n_cand, int2* d_out,
                      unsigned long long* d_out_count, long long n_hint = -1);
int launch_exact_tiles(hipStream_t stream, const PairwiseArgs& a, const int* d_list, int n_list, const Options& opt,
                       bool device_count = false);
// the cell count of a plan whose speculative second half ran on stale counts (k_plan_verdict)
constexpr unsigned long long kPlanStale = 1ULL << 62;
int launch_plan_verdict(hipStream_t stream, unsigned long long* d_counter, unsigned long long cand_capacity, const int* d_tile_total,
                        int tile_cap, bool tiles_skipped);
// exact hash-set intersections (mvs_intersect.hip).  Building a set: is every sample's list strictly increasing (*d_flag = 1
// if not), a segmented sort of up to 2^32 - 1 keys (offsets relative to d_in), distinct values per sample of sorted lists, and
// their compaction.  Intersecting: isect_plan<R> zeroes the result of every cell in range (R = int32_t: the count; R =
// mvs_abund_overlap: the whole record; mark_bad: the count of the others becomes -1), counts the units of every cell and scans
// them (d_units, d_unit_start: n_cells + 1 entries; d_counters: [0] cells out of range, [1] cells cut into several units, [2] sum
// of 8 (|A| + |B|)); d_scratch == NULL: *scratch_needed only.  launch_isect_units gives every unit to one wave, which decodes it
// and walks it with the code of mvs_intersect_dev.h, as the units kernels of mvs_overlap.hip and mvs_gather.hip do.
int launch_hs_check(hipStream_t stream, const unsigned long long* d_hashes, const long long* d_offsets, int64_t n,
                    unsigned int* d_flag);
int hs_sort_segments(hipStream_t stream, const unsigned long long* d_in, unsigned long long* d_out, unsigned int count,
                     unsigned int segments, const unsigned int* d_begin, const unsigned int* d_end, void* d_scratch,
                     size_t scratch_bytes, size_t* scratch_needed);
int launch_hs_count(hipStream_t stream, const unsigned long long* d_sorted, const long long* d_offsets, int64_t n, int32_t* d_sizes);
int launch_hs_compact(hipStream_t stream, const unsigned long long* d_sorted, const long long* d_offsets, const long long* d_new_offsets,
                      int64_t n, unsigned long long* d_out);
template <typename R>
int isect_plan(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, const int32_t* d_size_r, int64_t n_r,
               const int32_t* d_size_c, int64_t n_c, int unit, long long* d_units, long long* d_unit_start, R* d_inter,
               bool mark_bad, unsigned long long* d_counters, void* d_scratch, size_t scratch_bytes, size_t* scratch_needed);
int launch_isect_units(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, const long long* d_unit_start, long long n_units,
                       const unsigned long long* d_hash_r, const long long* d_off_r, const int32_t* d_size_r,
                       const unsigned long long* d_hash_c, const long long* d_off_c, const int32_t* d_size_c, int unit,
                       int32_t* d_inter);
// abundance-weighted overlaps (mvs_overlap.hip).  The plan is isect_plan<mvs_abund_overlap>; launch_overlap_units gives every unit
// to one wave as launch_isect_units does and adds the unit's count and five sums to the cell's record.  d_ab_r / d_ab_c: uint32
// abundances aligned with the hashes, or NULL = 1 for every value of that side.  launch_abund_totals: S, Q mod 2^32 summed,
// Q / 2^32 summed per sample (any output NULL).
int launch_overlap_units(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, const long long* d_unit_start, long long n_units,
                         const unsigned long long* d_hash_r, const long long* d_off_r, const int32_t* d_size_r, const uint32_t* d_ab_r,
                         const unsigned long long* d_hash_c, const long long* d_off_c, const int32_t* d_size_c, const uint32_t* d_ab_c,
                         int unit, mvs_abund_overlap* d_out);
int launch_abund_totals(hipStream_t stream, const uint32_t* d_abund, const long long* d_offsets, int64_t n, unsigned long long* d_sum,
                        unsigned long long* d_sumsq_lo, unsigned long long* d_sumsq_hi);
// FracMinHash values of DNA bytes (mvs_kmer.hip).  A unit is npos <= `unit` consecutive k-mer positions of one sample, the first
// at byte `byte0` of the buffer; launch_kmer_hash gives every unit to one workgroup (kmer_lds_bytes(unit, ksize) of LDS), which
// appends (value, sample) of the kept positions to a staging list of `cap` entries -- what does not fit is dropped but
// counted: d_counters[0] = kept values, d_sample_counts[s] / d_sample_valid[s] = kept values / valid positions of sample s
// (all zeroed by the caller).  launch_kmer_scatter moves n staged entries to d_out[d_offsets[sample] + ...] (d_cursors: one zeroed counter per
// sample), in arbitrary order inside a sample.
struct KmerUnit {
    long long byte0;
    int32_t sample, npos;
};
constexpr int kKmerUnitMax = 32768;
size_t kmer_lds_bytes(int unit, int ksize);
int launch_kmer_hash(hipStream_t stream, const uint8_t* d_bases, long long total_bytes, const KmerUnit* d_units, long long n_units,
                     int unit, int ksize, uint32_t seed, uint64_t max_hash, unsigned long long* d_vals, int32_t* d_sample,
                     unsigned long long cap, unsigned long long* d_counters, unsigned long long* d_sample_counts,
                     unsigned long long* d_sample_valid);
int launch_kmer_scatter(hipStream_t stream, const unsigned long long* d_vals, const int32_t* d_sample, long long n,
                        const long long* d_offsets, unsigned long long* d_cursors, unsigned long long* d_out);
// FracMinHash values of residues (mvs_protein.hip).  The units, the staging list and the counters are launch_kmer_hash's; a
// unit's positions are window starts (a window is ksize bytes, or 3 * ksize bases with translate, which hashes two k-mers per
// window: d_sample_valid counts hashed k-mers).  aa_fill_tables makes the look-up tables of the kernel's classification pass
// for an alphabet (0 protein, 1 dayhoff, 2 hp).  The planes of residues make a unit cost more LDS than k_kmer_hash's: a unit
// holds at most aa_unit_max positions, which keeps a workgroup under a third of a CU's 160 KiB.
struct AaTables {
    uint8_t byte_map[256];     // protein: byte -> encoded residue, 0 for a break; translate: byte -> T C A G = 0 1 2 3, 0x80 for a break
    uint8_t codon_fw[64];      // translate: 16x + 4y + z -> the encoded residue of codon xyz
    uint8_t codon_rv[64];      // ... of its reverse complement
};
constexpr int kAaUnitProtein = 18432, kAaUnitTranslate = 12032;
int aa_unit_max(bool translate);
size_t aa_lds_bytes(int unit, int ksize, bool translate);
int aa_fill_tables(bool translate, int alphabet, AaTables* out);
int launch_aa_hash(hipStream_t stream, const uint8_t* d_bytes, long long total_bytes, const KmerUnit* d_units, long long n_units, int unit,
                   bool translate, const AaTables& tables, int ksize, uint32_t seed, uint64_t max_hash, unsigned long long* d_vals,
                   int32_t* d_sample, unsigned long long cap, unsigned long long* d_counters, unsigned long long* d_sample_counts,
                   unsigned long long* d_sample_valid);
// the counted set build (mvs_abund.hip).  ab_sort_segments / ab_sort_whole: the segmented sort of hs_sort_segments, or a
// device-wide radix sort of ONE sample, with the weights travelling along where d_win is not NULL.  launch_ab_borders sets
// bit off[s] of the (zeroed) bit map for every sample that starts in front of `total`.  ab_count queues passes A, B, C and the
// two scans over the sorted values (d_scratch: ab_work_bytes(n_units)); ab_fill the offsets' tail, pass D and the sizes.
struct AbCarry {
    unsigned long long v, f;
};
struct AbArgs {
    const unsigned long long* keys;      // sorted inside every sample
    const uint32_t* weights;             // aligned with the keys, or NULL: 1 each
    const unsigned int* borders;         // bit map of the samples' first positions: (total + 31) / 32 + 1 words
    const long long* off;                // n + 1
    long long n, total, n_units;
    int unit;
    unsigned long long min_ab, max_ab;   // the filter (max_ab 0: no cap)
    AbCarry *summary, *tails;            // n_units each
    long long *head_counts, *pass_counts, *head_start, *pass_start;   // n_units + 1 each, the counts' last entry zero
    unsigned int* flags;                 // [0] != 0: an abundance reached 2^32 (zeroed by the caller)
    unsigned long long* hist;            // n x 256, zeroed by the caller, or NULL
};
int ab_sort_segments(hipStream_t stream, const unsigned long long* d_in, unsigned long long* d_out, const uint32_t* d_win,
                     uint32_t* d_wout, unsigned int count, unsigned int segments, const unsigned int* d_begin,
                     const unsigned int* d_end, void* d_scratch, size_t scratch_bytes, size_t* scratch_needed);
int ab_sort_whole(hipStream_t stream, const unsigned long long* d_in, unsigned long long* d_out, const uint32_t* d_win,
                  uint32_t* d_wout, unsigned int count, void* d_scratch, size_t scratch_bytes, size_t* scratch_needed);
size_t ab_work_bytes(long long n_units);
int launch_ab_borders(hipStream_t stream, const long long* d_off, long long n, long long total, unsigned int* d_borders);
int ab_count(hipStream_t stream, const AbArgs& a, void* d_scratch, size_t scratch_bytes);
int ab_fill(hipStream_t stream, const AbArgs& a, unsigned long long* d_out_vals, uint32_t* d_out_ab, long long* d_new_off,
            long long* d_distinct_off, int32_t* d_sizes);
// the greedy decomposition of a query (mvs_gather.hip).  The walk's state lives on the device: the best bid of a round
// ((count << 32) | (2^32 - 1 - survivor), 0 = none; consecutive rounds use alternating slots), the rows read so far, whether the
// walk has ended, records written, live positions of the query, rounds run.  launch_gather_init: alive = the query's positions,
// nobody retired, counts zero, a fresh state.  launch_gather_mark: the bit rows of the survivors (d_rows: n_cells x W words,
// zeroed by the caller) over the units isect_plan laid out for d_cells = (query, survivor's sample) with `unit`, a multiple of
// 64.  launch_gather_round: one round -- k_gather_count, k_gather_bid, k_gather_pick, all of which return at once when the walk
// has ended --; parity = the round's number mod 2, counted over everything queued since launch_gather_init.
struct GatherState {
    unsigned long long best[2];
    unsigned long long rows_read;   // live rows counted, summed over the rounds (x W x 8 = the bytes the round passes streamed)
    int32_t done, n_records, remaining, rounds;
};
int launch_gather_init(hipStream_t stream, unsigned long long* d_alive, int64_t W, int32_t q_size, int32_t* d_retired, int32_t* d_count,
                       int64_t ns, GatherState* d_state);
int launch_gather_mark(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, const long long* d_unit_start, long long n_units,
                       const unsigned long long* d_hash_q, const long long* d_off_q, const int32_t* d_size_q,
                       const unsigned long long* d_hash_d, const long long* d_off_d, const int32_t* d_size_d, int unit,
                       unsigned long long* d_rows, int64_t W);
int launch_gather_round(hipStream_t stream, const unsigned long long* d_rows, int64_t W, int64_t ns, unsigned long long* d_alive,
                        int32_t* d_retired, int32_t min_hashes, int32_t* d_count, const int32_t* d_surv_sample,
                        const int32_t* d_surv_orig, mvs_gather_match* d_rec, int64_t max_matches, GatherState* d_state, int parity);
// packed cells of the streamed output: radix sort on the (row, col) bits, then CSR arrays (row_ptr over `rows` rows,
// col, q as 8 bits -- *d_wide set if some q needs 16 -- or as 16 bits when d_q16 is given)
int sort_packed(hipStream_t stream, unsigned long long* d_in, unsigned long long* d_out, int64_t n, int begin_bit, int end_bit,
                void* d_scratch, size_t scratch_bytes, size_t* scratch_needed);
int launch_packed_csr(hipStream_t stream, const unsigned long long* d_keys, int64_t n, int shift, int64_t rows,
                      unsigned long long col_mask, long long* d_row_ptr, int32_t* d_col, uint8_t* d_q8, uint16_t* d_q16,
                      unsigned int* d_wide);
// the tile rows [tr0, tr0 + n_trows) the rows of a launch fall into and the tile columns of the matrix: sizes of the
// active-tile lists (d_list: n_trows x n_tc ints, d_list_n: n_trows ints) the row passes walk
void dense_tile_rows(const DenseActive& active, int64_t rows, int64_t n_cols, int* tr0, int* n_trows, int* n_tc);
int launch_dense_count(hipStream_t stream, const uint8_t* d_dense, int64_t ld, int64_t n_cols, int64_t rows, long long* d_counts,
                       int2* d_ends, const DenseActive& active, int* d_list, int* d_list_n);
int dense_row_ptr(hipStream_t stream, long long* d_counts, long long* d_row_ptr, int64_t rows, void* d_scratch, size_t scratch_bytes,
                  size_t* scratch_needed);
struct EncRow;
int launch_dense_fill(hipStream_t stream, const uint8_t* d_dense, int64_t ld, int64_t n_cols, int64_t rows, const long long* d_row_ptr,
                      int32_t* d_col, uint8_t* d_q, const DenseActive& active, const int* d_list, const int* d_list_n,
                      const int2* d_ends, unsigned long long* d_size, unsigned int* d_jac, unsigned int* d_first_col, EncRow* d_par,
                      long long capacity = 0x7fffffffffffffffLL);
// the re-check's kept cells (packed words, *d_n of them, rows relative to pack_row0 = the matrix's first row) into the dense
// byte matrix: mark the tiles they fall into (newly touched ones are listed in d_new, count in d_new[-1] .. i.e. d_new_count),
// clear those tiles, then write the bytes; *d_odd is set when a q is not in 1..255
int launch_packed_to_dense(hipStream_t stream, const unsigned long long* d_keys, const unsigned long long* d_n, int shift,
                           unsigned long long col_mask, uint8_t* d_dense, int64_t ld, int64_t matrix_rows, unsigned int* d_touch,
                           int n_tc, int* d_new, unsigned int* d_new_count, unsigned int* d_odd);
// true when launch_pairwise would run the kernel whose epilogue can write the dense byte matrix (two base-256 limbs on the
// ping-pong kernel)
bool exact_kernel_writes_dense(const PairwiseArgs& a, const Options& opt);
// kept cells of a block plan (storage coordinates) -> sample indices, own rows / other ranks' rows (mvs_cells_route);
// the cells of own rows out of the other ranks' send buffers (mvs_cells_collect)
int launch_cells_route(hipStream_t stream, const mvs_cell* d_raw, const unsigned long long* d_n_raw, unsigned long long raw_capacity,
                       long long block_pad, long long block_rows, long long n_total, int own_begin, int own_end, mvs_cell* d_own,
                       unsigned long long own_capacity, unsigned long long* d_own_count, unsigned long long* d_send,
                       unsigned long long foreign_capacity, long long status, long long max_abs);
int launch_cells_collect(hipStream_t stream, const unsigned long long* d_recv, int world, int rank, unsigned long long capacity,
                         int own_begin, int own_end, mvs_cell* d_own, unsigned long long own_capacity, unsigned long long* d_own_count);
// the shard's cells by row buckets (rows of <= 64 cells): state block as the route / collect kernels fill it
int launch_rows_max(hipStream_t stream, unsigned long long* d_state, int rows);
// up to 8 device ranges (4-byte aligned, sizes multiples of 4; NULL / empty ones are skipped) zeroed by ONE launch
int launch_zero_ranges(hipStream_t stream, void* const* ptrs, const size_t* bytes, int n);
// sort_cells_rows also leaves the widest row in d_state[1] (what launch_rows_max computes)
int sort_cells_rows(hipStream_t stream, const mvs_cell* d_in, mvs_cell* d_out, int64_t n, int row0, int rows,
                    const unsigned long long* d_state, void* d_scratch, size_t scratch_bytes, size_t* scratch_needed,
                    int64_t in_cap = -1, int64_t out_cap = -1);
// sort cells by (row, col); tmp buffers owned by the caller
int sort_cells(hipStream_t stream, mvs_cell* d_cells, mvs_cell* d_tmp, int64_t n, void* d_scratch,
               size_t scratch_bytes, size_t* scratch_needed, const Options& opt);

}  // namespace mvs

#endif
