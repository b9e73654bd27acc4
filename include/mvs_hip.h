/*
 * mvs_hip.h -- C ABI of libmvs_hip.so: the MI355X (gfx950) implementation of the reference's
 * random-projection sketching + all-vs-all sketch comparison hot path.
 *
 * The reference (RolandFaure/metagenome_vector_sketches) has no FFI seam on this path: the
 * functions below are what its two executables would bind if the hot loops were moved behind one.
 * Each entry point cites the reference code it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the call sites a maintainer would change.
 *
 * Conventions
 *   - plain C types only; the caller owns every buffer it passes in; the library never frees
 *     caller memory and never keeps a caller pointer after the call returns (except the non-owning
 *     views documented at mvs_sketch_set_from_planes);
 *   - every function returns MVS_OK (0) or an MVS_E_* code; mvs_last_error() gives the message of the
 *     last failure on the calling thread; no C++ exception crosses this boundary;
 *   - `mem` arguments say where a buffer lives: MVS_MEM_HOST (pageable or pinned host memory) or
 *     MVS_MEM_DEVICE (HBM of the context's device);
 *   - all work of a context is issued on ONE HIP stream (its own, or the one given to
 *     mvs_ctx_set_stream); calls with only device buffers are asynchronous on that stream unless
 *     stated otherwise; a context is thread-compatible, not thread-safe;
 *   - there is no CPU fallback: if no gfx950 device is usable every call fails with MVS_E_HIP.
 */
#ifndef MVS_HIP_H
#define MVS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_OK           0
#define MVS_E_INVALID    1   /* bad argument */
#define MVS_E_HIP        2   /* HIP runtime / device failure */
#define MVS_E_CAPACITY   3   /* output buffer too small; the needed size is reported */
#define MVS_E_NOMEM      4   /* host or device allocation failed */
#define MVS_E_RANGE      5   /* input outside the supported numeric range */
#define MVS_E_ABORTED    6   /* a caller's callback asked to stop */
#define MVS_E_INTERNAL   7   /* an invariant of the library's own results does not hold; nothing was rounded or guessed */

#define MVS_MEM_HOST     0
#define MVS_MEM_DEVICE   1

/* limb codes (the `limbs` arguments below): 1..4 = that many signed base-256 limb planes;
 * MVS_LIMBS_K3 = three planes (l0, l1, l0+l1) of signed base-128 digits, |v| <= 8127: the comparison then
 * needs 3 matrix-core passes per cell (Karatsuba) instead of the 4 of two base-256 limbs. */
#define MVS_LIMBS_K3     0x103

/* keep test variants */
#define MVS_KEEP_INT32   0   /* src/pairwise_comp_optimized.cpp:139-141  (int64 dot / d truncates) */
#define MVS_KEEP_INT16   1   /* src/pairwise_comp_optimized_16bits.cpp:211-218 (double(dot)/d)    */

typedef struct mvs_ctx mvs_ctx;
typedef struct mvs_sketch_set mvs_sketch_set;

/* One kept cell of the comparison matrix: what the reference appends to `all_results`
 * (src/pairwise_comp_optimized.cpp:974-980) plus the quantised Jaccard its writer derives from it
 * (:658-665). */
typedef struct {
    int32_t row;   /* global sample index of the row                              */
    int32_t col;   /* global sample index of the column                           */
    int32_t dot;   /* int32 dot product, wrapped mod 2^32 (MatrixXi product, :135) */
    int32_t q;     /* uint16_t(round(min(J,1)*255)), J = (dot/d)/(n2r+n2c-dot/d)   */
} mvs_cell;

/* ---- library / context ------------------------------------------------------------------------ */
const char* mvs_version(void);
const char* mvs_last_error(void);
int mvs_device_count(int* count);

int mvs_ctx_create(int device, mvs_ctx** ctx);
int mvs_ctx_destroy(mvs_ctx* ctx);
/* Issue all later work on `hip_stream`, a hipStream_t of the same device (e.g. the caller's framework
 * stream); NULL is HIP's default ("null") stream.  mvs_ctx_use_own_stream switches back to the
 * non-blocking stream the context created for itself (the initial state). */
int mvs_ctx_set_stream(mvs_ctx* ctx, void* hip_stream);
int mvs_ctx_use_own_stream(mvs_ctx* ctx);
int mvs_ctx_synchronize(mvs_ctx* ctx);
/* Optional kernel timing: when enabled, HIP events are recorded on the context's stream around the
 * dominant kernel of mvs_project_csr (which = 0) and around the comparison kernels of mvs_pairwise_rows /
 * _block / mvs_search_block (which = 1: the whole comparison -- filter + re-check, or the exact kernel;
 * which = 2: the filter kernel alone; which = 3: the re-check kernel with the list passes in front of it; which = 4:
 * the exact kernel on the tiles the filter flagged as dense; 2 and 3 are only recorded by a two-stage comparison, 4 only
 * when it flagged tiles).  mvs_ctx_kernel_ms returns the duration of the most recent such launch in ms. */
int mvs_ctx_set_timing(mvs_ctx* ctx, int enabled);
int mvs_ctx_kernel_ms(mvs_ctx* ctx, int which, float* ms);
/* Tuning / diagnostic options of a context, by name.  The library reads the environment exactly once per
 * context, in mvs_ctx_create: MVS_<NAME> (upper case) gives an option's initial value; afterwards only
 * mvs_ctx_set_option changes it, so two contexts (or two threads with a context each) never interfere.
 *   pairwise_filter       0 exact kernel on every cell; 1 (default) two-stage comparison for blocks of at least
 *                         2^22 cells and more than 16 rows of a two-limb set (fewer than 1024 rows: from the second
 *                         such block on the same set on, or if the set's coarse plane is already cached); 2 two-stage
 *                         whenever the set has two limbs (tests)
 *   filter_variant        kernel of the one-pass filter: -1 (default) by block size, 8 = ping-pong wave groups on
 *                         256 x 256 tiles (7/9/10 its variants), 0 = 128 x 128 ring, 1 = 256 x 256 ring, 3/5/6 other rings
 *   exact_variant         re-check kernel: 3 (default) tree reduction over rounds of 64 pairs, 0 one shuffle butterfly per
 *                         pair, 1 quarter wave per pair, 2 16 pairs per round
 *   pairwise_variant      exact kernel: 8 (default) ping-pong 16x16x64 MFMA for two limbs (7/9 its variants), 6 the ring
 *                         kernel on the same shape, 0-5 32x32x32 tile / ring variants.  With the default, a block of up
 *                         to 16 rows x at least 1024 columns of a two-limb set (a search with a few queries) goes to a
 *                         streaming vector-ALU kernel instead (rows in LDS, one wave per column, v_dot2_i32_i16)
 *   pairwise_symmetric    1 (default) skip tiles below the diagonal and mirror; 0 compute every tile
 *   pairwise_block_cells  row-chunk bound of mvs_pairwise_rows, in cells (default 2^40)
 *   sort                  kept-cell sort: 0 (default) by list length, 1 merge sort, 2 radix sort
 *   enable_k3             1: mvs_sketch_set_create codes sets with 127 < max|v| <= 8127 as MVS_LIMBS_K3
 *   project_variant       projection kernel: 0 (default) by dimension -- 24 = four 64-dim blocks per wave sharing the
 *                         first splitmix64 round, deep carry-save tree, VALU-only epilogue, when d is a multiple of 256
 *                         (>= 512), else 2 or 1 blocks per wave; 1 / 2 / 12 / 14 / 24 force a variant (14 = 24 with
 *                         the ripple every 32 hashes and the ds_bpermute epilogue)
 *   project_balance       1 (default): the projection cuts the units of work that would end behind the launch's ideal end
 *                         -- the last partial round of workgroups, a long sample late in the list, every sample of a launch
 *                         too small to fill the device -- into pieces that fill the idle workgroup slots
 *                         (mvs_project_plan); 0: samples are cut at 65536 hashes only
 *   stream_dense          mvs_pairwise_stream, dense results: 1 (default) one byte per cell in a matrix, a row block turned
 *                         into CSR / encoded rows on a side stream beside the next block's launch where the exact kernel
 *                         does whole row blocks, on the context's stream where the two-stage comparison feeds the matrix;
 *                         2 always the context's stream; 3 always the side stream; 0 packed 64-bit cells + sort
 *   tile_dense_thr        two-stage comparison on large blocks: a filter wave (128 x 64 cells) with more candidates than this
 *                         flags its 256 x 256 tile for the exact kernel instead of listing them (default 64; 0 = list
 *                         everything and give the whole block to the exact kernel once the list passes 1/128 of its cells)
 *   stream_list_cells, stream_pipeline
 *                         mvs_pairwise_stream with the two-stage comparison: up to stream_list_cells kept cells (bound from
 *                         the filter pass) leave as one sorted list, more through the dense byte matrix; stream_pipeline = 0
 *                         always filters the whole row range in one pass first (tests)
 *   fragment_major        1 (default): the matrix-core kernels that move 16 samples x 64 k values per instruction (ping-pong
 *                         filter and exact kernel, streaming search filter) read fragment-major copies of the coarse plane /
 *                         limb planes, built once per resident set (+1 x the planes' bytes); 0: the row-major planes
 *   pairwise_bdirect      1 (default): with those copies, the ping-pong kernels load the B operand's fragments straight into
 *                         registers and LDS carries the A operand only; 0: both operands through LDS
 *   search_stream         1 (default): blocks of up to 640 rows x at least 4096 columns outside the symmetric schedule (a
 *                         search) take the streaming filter (rows resident in LDS, columns streamed); 0: the tile kernels
 *   plan_order            1 (default) the launches of the ping-pong filter -- of a block plan, and the one-block launch of
 *                         mvs_pairwise_rows / _stream -- take a balanced tile order: every XCD the same number of tiles of every
 *                         16 x 16-tile super-patch; 0 the static super-patch map (a triangle's static sub-patches hold 32, 26, 10
 *                         or 0 tiles: launches of a few rounds waited for their fullest XCD)
 *   topk_dots, topk_block_rows
 *                         mvs_pairwise_topk: dots from the matrix cores (0, default) or the vector-ALU kernel (1); > 0 bounds
 *                         the rows of a block (0: by the device budget)
 *   contain_dots, contain_block_rows
 *                         mvs_pairwise_contain: dots from the matrix cores (0, default) or the vector-ALU kernel (1); > 0 bounds
 *                         the rows of a block (0: by the device budget)
 *   levels_dots, levels_block_rows
 *                         mvs_pairwise_levels: dots from the matrix cores (0, default) or the vector-ALU kernel (1); > 0 bounds
 *                         the rows of a block (0: by the device budget)
 *   pcoa_dots, pcoa_block_rows
 *                         mvs_jaccard_apply / mvs_pcoa_*: dots from the matrix cores (0, default) or the vector-ALU kernel (1); > 0
 *                         bounds the rows of a block (0: by the device budget)
 *   groups_dots, groups_block_rows
 *                         mvs_group_sums / mvs_permanova: dots from the matrix cores (0, default) or the vector-ALU kernel (1); > 0
 *                         bounds the rows of a block (0: by the device budget)
 *   labels_dots, labels_block_rows
 *                         mvs_label_sums / mvs_silhouette: dots from the matrix cores (0, default) or the vector-ALU kernel (1); > 0
 *                         bounds the rows of a block (0: by the device budget)
 *   hclust_dots, hclust_block_rows, hclust_compact
 *                         mvs_hclust: dots from the matrix cores (0, default) or the vector-ALU kernel (1); > 0 bounds the rows
 *                         of a block of the fill (0: by the device budget); the table's columns are compacted never (0), when
 *                         at most half are alive (1, default), after every round (2).  None changes a record
 *   community_path        mvs_community_finish: a vertex starts in the local-moving path its degree names (0, default), in the
 *                         wave (1), workgroup (2) or global (3) path (A/B, tests).  Never changes a result
 *   tsne_slice_cols       mvs_tsne_gradient / _run / _kl: columns of a repulsion unit, 16 .. 1024 (default 1024; tests).  Never
 *                         changes a result
 *   core_block_rows       mvs_core_jaccard / mvs_hdbscan: > 0 bounds the rows of a top-k range (0: by the cell buffer's budget)
 *   gram_slab_rows        mvs_sketch_moments / mvs_pca_fit: samples per slab of the transposed scratch copy, 64 .. 65536 (default
 *                         65536; rounded down to a multiple of 64)
 *   gram_variant          tile kernel of the moments: 0 (default) by shape -- 128 x 128 tiles for one or two limbs and d >= 128, else
 *                         64 x 64 --, 1 always 64 x 64 (A/B, tests)
 *   cluster_cells, cluster_block_rows
 *                         mvs_pairwise_cluster: cells the staging buffer of a row block holds (0, default: a quarter of the free
 *                         device memory) and an upper bound on the rows of a block (0: by pairwise_block_cells); a block that
 *                         overflows the buffer is halved and redone, so neither changes a result
 *   intersect_unit        mvs_intersect_cells: elements of a pair's SHORTER hash list that one unit of work (one wave) covers,
 *                         64 .. 2^30 (default 2048); a pair with a longer one is cut into several units
 *   gather_batch          mvs_gather: rounds of the walk queued between two read-backs of its state, 1 .. 1024 (default 16)
 *   kmer_unit             mvs_hash_set_from_sequences: k-mer positions of one sample that one unit of work (one workgroup)
 *                         covers, 64 .. 32768 (default 17408); a longer sample is cut into several units
 *   kmer_capacity         mvs_hash_set_from_sequences: > 0 = the values the staging list of the first hashing pass holds (tests
 *                         lower it to force the second pass); 0 (default) = the expected number of kept values plus a margin.
 *                         Both act per call of mvs_kmer_sketcher_add too
 *   abund_unit            counted set build (mvs_hash_set_create_counted, mvs_kmer_sketcher_finish): sorted values that one unit
 *                         of work (one wave) of the run-sum passes covers, 64 .. 2^20 (default 4096)
 *   abund_big_segment     counted set build: a sample of more values than this is sorted by a device-wide radix sort of its own,
 *                         the others by the segmented sort, 64 .. 2^30 (default 262144).  Neither has an environment default
 *   stream_block_rows, encode_stage_words, pairwise_map, coarse_radix, cand_regions, recheck_mode, recheck_blocks
 *                         test / experiment switches (DESIGN.md, appendix "switches"; encode_stage_words below 64 also keeps
 *                         every row on the device encoder's general loop)
 *   comm_timeout_s        file transport (mvs_comm_create_files / _rendezvous): seconds a rank waits for its peers
 *   markers               1: roctx ranges named after the entry points around mvs_project_csr / mvs_pairwise_rows /
 *                         mvs_pairwise_block (rocprofv3 --marker-trace); libroctx64 is bound at run time
 *   pairwise_debug        profiling aids, bit mask: 1 / 2 skip the k-loop / the epilogue (such runs produce garbage by
 *                         design), 8 per-workgroup time stamps of the comparison kernel dumped to /tmp/mvs_stamps.bin;
 *                         rejected unless the library was built with -DMVS_ABLATIONS (make -C csrc ablations)
 * Unknown names and out-of-range values return MVS_E_INVALID.  None of them changes a result. */
int mvs_ctx_set_option(mvs_ctx* ctx, const char* name, int64_t value);
int mvs_ctx_get_option(const mvs_ctx* ctx, const char* name, int64_t* value);

/* Diagnostics of the most recent comparison (mvs_pairwise_rows / _block / mvs_search_block): the number
 * of candidate pairs its coarse filter passed on to the exact re-check, 0 if the exact kernel ran on
 * every cell (see mvs_pairwise_rows). */
int mvs_ctx_pairwise_candidates(mvs_ctx* ctx, int64_t* candidates);
/* The same with the tile-granular part of the two-stage comparison: `flagged_tiles` of the `filter_tiles` 256 x 256 tiles the
 * filter pass worked on held so many candidates that the exact kernel computed them whole instead (dense regions of the
 * result; the reference's cost is flat in the density, src/pairwise_comp_optimized.cpp:135-147 -- this keeps ours from
 * falling off a cliff between "sparse" and "dense").  Any pointer may be NULL. */
int mvs_ctx_pairwise_stats(mvs_ctx* ctx, int64_t* candidates, int64_t* flagged_tiles, int64_t* filter_tiles);

/* ---- device memory and events for hosts above the ABI -------------------------------------------------
 * The host drivers are plain C++ above this header (no HIP runtime of their own): the buffers a multi-rank step keeps between
 * its calls (limb planes, coarse plane, statistics, kept cells -- INTEGRATION.md B5) and the ordering between the context
 * that compares and the context the communicator exchanges on come from here.  Replaces nothing of the reference by
 * itself: its tiles live in Eigen matrices on the host (src/pairwise_comp_optimized.cpp:33-54).
 * mvs_device_alloc : bytes of HBM on the context's device (zero != 0: cleared, on the context's stream).
 * mvs_device_free  : waits for the context's stream first.
 * mvs_device_zero  : asynchronous on the context's stream.
 * mvs_device_copy  : dst / src each MVS_MEM_HOST or MVS_MEM_DEVICE; device-to-device copies are asynchronous on the
 *                    context's stream, copies that touch host memory return when the host buffer may be reused / read.
 * Events order two contexts of one device without the host waiting: mvs_event_record puts the event on the context's
 * stream, mvs_ctx_wait_event makes everything queued LATER on a context's stream wait for it (an event that was never
 * recorded counts as complete).  timing != 0 at creation: mvs_event_elapsed_ms between two recorded events. */
typedef struct mvs_event mvs_event;
int mvs_device_alloc(mvs_ctx* ctx, size_t bytes, int zero, void** ptr);
int mvs_device_free(mvs_ctx* ctx, void* ptr);
int mvs_device_zero(mvs_ctx* ctx, void* ptr, size_t bytes);
int mvs_device_copy(mvs_ctx* ctx, void* dst, int mem_dst, const void* src, int mem_src, size_t bytes);
int mvs_event_create(mvs_ctx* ctx, int timing, mvs_event** event);
int mvs_event_record(mvs_ctx* ctx, mvs_event* event);
int mvs_ctx_wait_event(mvs_ctx* ctx, mvs_event* event);
int mvs_event_synchronize(mvs_event* event);
int mvs_event_elapsed_ms(mvs_event* begin, mvs_event* end, float* ms);
int mvs_event_destroy(mvs_event* event);

/* ---- projection ----------------------------------------------------------------------------------
 * Replaces transform_set_into_vector() (src/random_projection.cpp:9-26) called once per sample from
 * the OpenMP loop of sketch() (src/project_everything.cpp:289-298) and from standalone_projection
 * (src/standalone_projection.cpp:37).
 *
 * hashes  : concatenated per-sample hash lists (CSR values), `mem_hashes` says where they live.
 *           Precondition: hashes of one sample are unique (the reference holds them in an
 *           std::unordered_set); order is irrelevant.
 * offsets : n_samples+1 HOST int64, offsets[s]..offsets[s+1] is sample s; a sample may be empty.
 *           Each sample must hold < 2^31 hashes.
 * out     : n_samples x d int32, row-major by sample (the vectors.bin record layout,
 *           src/project_everything.cpp:349-353), `mem_out` says where.
 * out[s][k] = sum over hashes h of (1 - 2*bit_{k%64}(splitmix64(h + 64*(k/64)))), exact.
 */
int mvs_project_csr(mvs_ctx* ctx, const uint64_t* hashes, int mem_hashes, const int64_t* offsets,
                    int64_t n_samples, int d, int32_t* out, int mem_out);

/* mvs_project_csr plus the two statistics the next stages need, produced by the same kernel for every sample
 * that is one unit of work (the others -- longer than 65536 hashes, or cut by the planner below -- by one extra pass
 * over their rows alone): sumsq[s] = exact sum of squares of sketch s
 * (int64[n_samples], in the same memory space as `out`: device array for device sketches, host array for host
 * sketches) and *max_abs = largest |v| (host; decides the limb code).  Synchronous.
 * Host hash lists beyond 32 MiB travel through two pinned staging buffers: the host-side copy, the DMA and the
 * projection of the samples already complete overlap (measured: 1.07 x the bare PCIe time of the same bytes). */
int mvs_project_csr_stats(mvs_ctx* ctx, const uint64_t* hashes, int mem_hashes, const int64_t* offsets,
                          int64_t n_samples, int d, int32_t* out, int mem_out, int64_t* sumsq, int64_t* max_abs);

/* The units of work a projection launch consists of, without a device: how mvs_project_csr would lay out the samples of
 * `offsets` (n_samples + 1 entries) for a kernel variant that takes `ny` workgroups per unit on a device that holds
 * `slots` of its workgroups at a time (compute units x occupancy; the library asks the runtime).  A unit is a run of
 * at most 65536 hashes of one sample; `single` = 1: it is the whole sample (plain stores, statistics inside the
 * kernel), 0: its sample consists of several units that combine with int32 atomics.  The units of a sample tile it
 * in order; an empty sample has one unit of zero hashes.  balance != 0: units that would end behind the ideal end of
 * the launch (total work / slots) under in-order dispatch are cut into pieces that fill the slots which would idle.
 * Each piece is sized when its turn comes, from what still fits in front of the ideal end: a multiple of 2048 hashes,
 * at least 4096, so the pieces of a unit need not be equal; the last piece takes what is left of the unit (any
 * remainder of 2048 hashes or more; a smaller one is added to the piece before it).  A workgroup is taken to cost its
 * hashes + `overhead` hash-times (< 0: the library's constant).  The model is described where it is implemented
 * (csrc/mvs_capi_sketch.hip, "projection units").  balance == 0 or slots <= 0: samples are cut at 65536 hashes only.
 * flags bit 0: the 512 hashes behind the unit's last full batch of 512 are not all inside [0, offsets[n_samples]).
 * Writes at most `capacity` units and returns the number the plan has in *n_units (units may be NULL when capacity is 0).
 * Pure host code. */
typedef struct mvs_proj_unit {
    int64_t begin;   /* index of the unit's first hash */
    int32_t count;   /* hashes in the unit */
    int32_t sample;  /* output row */
    int32_t single;
    int32_t flags;
} mvs_proj_unit;
int mvs_project_plan(const int64_t* offsets, int64_t n_samples, int ny, int slots, int overhead, int balance,
                     mvs_proj_unit* units, int64_t capacity, int64_t* n_units);
/* What the context's most recent mvs_project_csr[_stats] launched: the units of its list, the samples among them that
 * consist of several units, and the `slots` and `ny` its plan was made with (slots = 0: no balancing -- option
 * project_balance 0, or the pipelined upload of a large host hash list).  Any pointer may be NULL. */
int mvs_ctx_project_stats(const mvs_ctx* ctx, int64_t* n_units, int64_t* cut_samples, int* slots, int* ny);

/* Sum of squares of each sketch (exact int64): the integer the norm of
 * src/project_everything.cpp:328-329 is derived from (norm = sqrt(sumsq / d)). */
int mvs_sketch_sumsq(mvs_ctx* ctx, const int32_t* sketches, int mem_in, int64_t n, int d,
                     int64_t* sumsq, int mem_out);

/* The vector_norms.txt round trip without the file, on the device: out[i] = strtod(text_i)^2 where text_i is the
 * "%g" (6 significant digits) rendering of sqrt(double(sumsq[i]) / d) -- i.e. exactly the squared norm that
 * src/pairwise_comp_optimized.cpp:893-901 parses from the line src/project_everything.cpp:328-330 writes (with this
 * build's norm definition).  Decimal rounding is done in exact arithmetic (ties included), so
 * the values are bit-identical to the ones read back from the file.  sumsq and out are device arrays of n entries;
 * asynchronous on the context's stream.  For a pipeline that sketches and compares in one process. */
int mvs_norms_sq_text(mvs_ctx* ctx, const int64_t* sumsq, int64_t n, int d, double* out);

/* Both statistics the stages after the projection need, in one pass over the sketches: the per-sketch sum
 * of squares (as mvs_sketch_sumsq) and the largest |v| of the whole array (as mvs_sketch_max_abs, which
 * decides the limb code).  Synchronous: *max_abs is valid on return. */
int mvs_sketch_stats(mvs_ctx* ctx, const int32_t* sketches, int mem_in, int64_t n, int d, int64_t* sumsq,
                     int mem_out, int64_t* max_abs);

/* Saturating int32 -> int16 store of the --int16 mode (src/project_everything.cpp:332-347). */
int mvs_sketch_saturate_i16(mvs_ctx* ctx, const int32_t* sketches, int mem_in, int64_t n_elems,
                            int16_t* out, int mem_out);

/* ---- pairwise comparison --------------------------------------------------------------------------
 * Replaces load_matrix_block() + compute_sparse_dot_products_optimized() + the tiling loop of
 * main() (src/pairwise_comp_optimized.cpp:33-54, :57-160, :949-982) and the per-cell arithmetic of
 * write_sparse_results_jaccard_wo_sort() (:658-665); for elem_bytes == 2 also
 * compute_sparse_dot_products_optimized_16() (src/pairwise_comp_optimized_16bits.cpp:96-244).
 *
 * The sketches are first re-coded into signed base-256 int8 "limb planes" kept in HBM (exact:
 * v == sum_a limb_a * 256^a mod 2^32); the comparison kernel multiplies limb planes on the int8
 * matrix cores with int32 accumulation and recombines them mod 2^32, so `dot` carries exactly the
 * bits of the reference's int32 Eigen product.
 */

/* Largest |v| over n*d sketch entries (elem_bytes 4: int32, 2: int16); synchronous. */
int mvs_sketch_max_abs(mvs_ctx* ctx, const void* sketches, int elem_bytes, int mem, int64_t n_elems,
                       int64_t* max_abs);
/* Limb code for entries up to max_abs: 1 (<=127), 2 (<=32639), 3, or 4.  (MVS_LIMBS_K3 is never chosen here: it
 * measures slower than 2 on MI355X; option enable_k3 makes mvs_sketch_set_create use it for 128..8127.) */
int mvs_limbs_for_max_abs(int64_t max_abs);
/* Geometry of the limb-plane buffer for n samples: rows are padded to n_alloc (multiple of 256,
 * plus one spare tile), the dimension to d_pad (multiple of 128); layout is
 * planes[(row * P + plane) * d_pad + k] with P = limbs & 0xff planes per row, zero filled outside n x d. */
int mvs_limb_geometry(int64_t n, int d, int limbs, int64_t* n_alloc, int* d_pad, size_t* bytes);
/* Re-code rows [0, n_rows) of `sketches` into rows [row_offset, row_offset + n_rows) of a
 * caller-owned DEVICE plane buffer that has been zero-filled (so several producers -- e.g. the
 * ranks of an all-gather -- can fill disjoint row ranges of one buffer). */
int mvs_limb_split(mvs_ctx* ctx, const void* sketches, int elem_bytes, int mem, int64_t n_rows, int d,
                   int limbs, int8_t* planes, int d_pad, int64_t row_offset);

/* A sketch set = limb planes of N samples resident in HBM.
 * mvs_sketch_set_create : allocates the planes, re-codes `sketches` (chooses the limb count itself).
 * mvs_sketch_set_from_planes : NON-owning view of a caller-owned device buffer filled by
 *   mvs_limb_split (and, across GPUs, by an all-gather of per-rank row blocks); the buffer must
 *   outlive the set and keep its contents while the set is compared (the library caches data derived
 *   from the planes per set: make a new view after rewriting the buffer). */
int mvs_sketch_set_create(mvs_ctx* ctx, const void* sketches, int elem_bytes, int mem, int64_t n, int d,
                          mvs_sketch_set** set);
int mvs_sketch_set_from_planes(mvs_ctx* ctx, const int8_t* planes, int64_t n, int64_t n_alloc, int d,
                               int d_pad, int limbs, mvs_sketch_set** set);
/* For databases streamed from disk in row chunks (load_matrix_block, src/pairwise_comp_optimized.cpp:33-54):
 * allocate zeroed planes for n samples with a given limb count, then fill row ranges. */
int mvs_sketch_set_alloc(mvs_ctx* ctx, int64_t n, int d, int limbs, mvs_sketch_set** set);
int mvs_sketch_set_fill(mvs_sketch_set* set, const void* sketches, int elem_bytes, int mem, int64_t row_offset,
                        int64_t n_rows);
/* mvs_sketch_set_fill that also reports the largest |v| of the rows it was given (same upload).  A loader can
 * then stream a database ONCE: allocate for two limbs, fill, and only if some chunk reports |v| beyond what the
 * set's limb count holds (mvs_limbs_for_max_abs) start over with more limbs. */
int mvs_sketch_set_fill_stats(mvs_sketch_set* set, const void* sketches, int elem_bytes, int mem,
                              int64_t row_offset, int64_t n_rows, int64_t* max_abs);
int mvs_sketch_set_info(const mvs_sketch_set* set, int64_t* n, int* d, int* limbs, int64_t* n_alloc,
                        int* d_pad);
/* The DEVICE plane buffer of a set the library allocated (mvs_sketch_set_alloc / _create), for collectives that fill
 * other ranks' row blocks in place (mvs_allgather_planes).  mvs_sketch_set_touch tells the library that the caller
 * has rewritten the planes (data derived from them is rebuilt on the next comparison). */
int mvs_sketch_set_planes(mvs_sketch_set* set, int8_t** planes);
int mvs_sketch_set_touch(mvs_sketch_set* set);
/* How often the context has derived data from a set's limb planes since it was created (cumulative, read-only): whole
 * builds of the coarse plane, of its fragment-major copy and of the fragment-major copy of the limb planes, and the rows
 * (widened to groups of 16) that were re-derived in place after mvs_sketch_set_fill rewrote a small part of a set.  Any
 * pointer may be NULL. */
int mvs_ctx_derived_stats(mvs_ctx* ctx, int64_t* coarse_builds, int64_t* coarse_rows_refreshed,
                          int64_t* coarse_fm_builds, int64_t* planes_fm_builds, int64_t* planes_fm_rows_refreshed);
int mvs_sketch_set_destroy(mvs_sketch_set* set);

/* All-vs-all for the row range [row_begin, row_end) against ALL n columns -- one shard of
 * src/pairwise_comp_optimized.cpp:938-982.
 *   norms_sq : n doubles, (parsed norm)^2 as built at :893-901 (`mem_norms` says where): squares, so >= 0,
 *              or nan / inf if the text said so (such a sample keeps nothing, as in the reference);
 *              negative values are outside the contract.
 *   keep_mode: MVS_KEEP_INT32 or MVS_KEEP_INT16.
 *   cells    : capacity entries (`mem_cells`); on success holds *n_cells kept cells sorted by
 *              (row, col) -- the per-row, ascending-column order the reference's writer relies on
 *              (:718-722).  If more than `capacity` cells are kept the call returns MVS_E_CAPACITY
 *              and *n_cells is the number needed (retry with a larger buffer or fewer rows).
 * Synchronous (returns after the count is known).
 * How the cells are found is the library's business and never changes the result: sets of two base-256
 * limbs are compared in two stages -- a one-pass int8 filter on a coarse plane with a proven error bound
 * drops the pairs that cannot pass the keep test, the exact int32 dot and the reference's keep test run on
 * the survivors (rows whose sum of squares reaches 2^31, whose dots may wrap, are re-checked against every
 * column) -- everything else goes through the exact kernel cell by cell (option pairwise_filter = 0 forces
 * that, = 2 forces the two stages on small blocks too; mvs_ctx_pairwise_candidates reports which one ran). */
int mvs_pairwise_rows(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms,
                      int keep_mode, int64_t row_begin, int64_t row_end, mvs_cell* cells,
                      int64_t capacity, int mem_cells, int64_t* n_cells);

/* The same comparison with the result STREAMED out in row blocks instead of returned in one caller-sized buffer -- what a
 * shard writer wants (src/pairwise_comp_optimized.cpp:974-990 keeps all of `all_results` in RAM and then groups it by row;
 * its writer, :718-736, needs per row only the ascending columns and q).  Rows [row_begin,row_end) against all columns;
 * the kept cells come back as CSR pieces of consecutive whole rows, in ascending row order, each piece exactly once:
 *     row r of a piece (row_begin <= r < row_end) holds cells row_ptr[r - row_begin] .. row_ptr[r - row_begin + 1] of
 *     col[] (ascending) and q[]; q16 replaces q (which is then NULL) in the one case where a value does not fit 8 bits
 *     (a negative Jaccard estimate from a norms file that does not belong to the vectors).
 * The arrays live in pinned host memory of the library and are valid only during the callback.  The callback runs on a
 * worker thread of the library, one call at a time, while the device computes and downloads the next pieces; a
 * non-zero return stops the comparison (MVS_E_ABORTED).  Empty rows are covered too (pieces with n_cells 0 occur).
 * Nothing is ever computed twice for lack of space: the two-stage comparison sizes its output from the candidate count
 * between its stages; where the exact kernel runs, the rows are cut into blocks whose worst case fits
 * `device_budget_bytes` of HBM (0: a quarter of what is free), each using the symmetric schedule inside its own square.
 * *n_cells (optional) receives the number of kept cells delivered.  Synchronous. */
typedef struct {
    int64_t row_begin, row_end;
    int64_t n_cells;
    const int64_t* row_ptr;
    const int32_t* col;
    const uint8_t* q;
    const uint16_t* q16;
} mvs_row_block;
typedef int (*mvs_row_block_cb)(void* user, const mvs_row_block* block);
int mvs_pairwise_stream(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, int keep_mode,
                        int64_t row_begin, int64_t row_end, size_t device_budget_bytes, mvs_row_block_cb cb, void* user,
                        int64_t* n_cells);

/* mvs_pairwise_stream with the rows already ENCODED on the device in this build's shard codec
 * (metagenome_vector_sketches_amd/csrc/host/mvs_codec.hpp; the reference's writer, src/pairwise_comp_optimized.cpp:718-736,
 * stores per row a compact_vector of the q values and, when the row holds more than one cell, a rice_sequence of the
 * column deltas -- through the `bits` library, which is absent from the reference tree, so the byte layout is this
 * build's own).  A piece covers rows [row_begin, row_end) and carries, for its n_rows rows that hold cells (ascending):
 * their ids, their first columns (what goes into neighbor_start.bin), the byte offset of each row's record inside
 * `bytes`, the size of its compact_vector (the "Jac space" statistic of :808) and the records themselves, back to back --
 * exactly the bytes the host writer appends to matrix.bin for the same rows (tests compare the files).  Same delivery
 * rules as mvs_pairwise_stream.  1.4 bytes per kept cell cross the link instead of 5, and no host thread touches a cell. */
typedef struct {
    int64_t row_begin, row_end;
    int64_t n_cells;
    int64_t n_rows;
    const uint32_t* rows;
    const uint32_t* first_col;
    const uint64_t* offset;
    const uint32_t* jac_bytes;
    const uint8_t* bytes;
    int64_t n_bytes;
} mvs_encoded_rows;
typedef int (*mvs_encoded_rows_cb)(void* user, const mvs_encoded_rows* piece);
int mvs_pairwise_stream_encoded(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, int keep_mode,
                                int64_t row_begin, int64_t row_end, size_t device_budget_bytes, mvs_encoded_rows_cb cb,
                                void* user, int64_t* n_cells);

/* What the most recent mvs_pairwise_stream of the context did: time of its comparison kernels summed over the row blocks
 * (0 unless mvs_ctx_set_timing is on), bytes handed to the callback, row blocks computed, pieces delivered, and whether
 * the two-stage comparison produced them as one list (1), through the dense byte matrix after one filter pass over all rows,
 * its flagged tiles computed row block by row block (2), through the matrix with the filter itself running row block by row
 * block (3: results that look dense from the first tile row on), or the exact kernel alone in row blocks (0).  Any pointer
 * may be NULL. */
int mvs_ctx_stream_stats(const mvs_ctx* ctx, double* kernel_ms, int64_t* bytes_out, int64_t* row_blocks, int64_t* pieces,
                         int* two_stage);

/* Which route the row blocks of the most recent stream call took (counters only): blocks delivered out of the dense byte
 * matrix (dense_blocks); of the encoded ones, those whose row passes were queued with buffers sized from the blocks before
 * them (spec_blocks, option stream_spec) and, among these, the ones whose sizes did not hold, so that the block was done
 * again with its own counts read back first (spec_redone); dense blocks that held a q a byte cannot store -- 0, or beyond
 * 255 -- after which that block and the rest of the rows went through packed lists (list_fallbacks).  Any pointer may be
 * NULL. */
int mvs_ctx_stream_dense_stats(const mvs_ctx* ctx, int64_t* dense_blocks, int64_t* spec_blocks, int64_t* spec_redone,
                               int64_t* list_fallbacks);

/* One rectangular block of the comparison -- rows [row_begin,row_end) x columns [col_begin,col_end) -- for
 * schedules that split a shard's work by column block (metagenome_vector_sketches_amd/parallel.py: with G
 * shards every unordered pair of row blocks is compared ONCE and the mirrored cells are exchanged).
 *   flags : MVS_BLOCK_SYMMETRIC  the column range contains the square of the row range: inside it tiles
 *                                strictly below the diagonal are skipped and produced by mirroring (this is
 *                                what mvs_pairwise_rows does on its own);
 *           MVS_BLOCK_MIRROR_ALL every kept (row, col) is also appended as (col, row) -- the transposed block
 *                                belongs to another shard, which then does not compute it.
 *   norms_sq, cells : DEVICE buffers.  Cells are APPENDED, unsorted, at index *n_cells (in/out);
 *   MVS_E_CAPACITY reports the needed total in *n_cells.  Order them with mvs_cells_sort.  Synchronous. */
#define MVS_BLOCK_SYMMETRIC   1
#define MVS_BLOCK_MIRROR_ALL  2
int mvs_pairwise_block(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int keep_mode,
                       int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, int flags,
                       mvs_cell* cells, int64_t capacity, int64_t* n_cells);
/* Query-by-sketch search, the exact brute-force counterpart of the reference's FAISS IndexFlatIP path
 * (src/jaccard.py:63-224: normalised inner products, then jaccard = ip*qn*nn / (nn^2 + qn^2 - ip*qn*nn) > j).
 * Rows [row_begin,row_end) of the set are the queries (their sketches appended after the database rows),
 * columns [col_begin,col_end) the database; a pair is reported iff its Jaccard estimate
 * (dot/d) / (n2_row + n2_col - dot/d) exceeds jaccard_min (0 < jaccard_min < 1).  Same kernel as the
 * comparison, with the keep coefficient 0.05 replaced by jaccard_min/(1+jaccard_min) and the floating keep
 * test.  norms_sq and cells are DEVICE buffers; cells come back sorted by (row, col), `dot` exact, `q` the
 * 8-bit quantised estimate.  Synchronous. */
int mvs_search_block(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, double jaccard_min,
                     int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, mvs_cell* cells,
                     int64_t capacity, int64_t* n_cells);

/* Exact k nearest neighbours: for every row of [row_begin, row_end), the k columns of [col_begin, col_end) whose Jaccard
 * estimate is highest -- the question `query_pc_mat --top` and read_pc_mat.py ask of a thresholded matrix
 * (src/pairwise_comp_optimized.cpp:135-147 keeps a cell only when dot/d > 0.05 (n2_i + n2_j)), answered for every row
 * whatever its neighbours' Jaccard.
 *   score : J = inter / (n2_row + n2_col - inter), inter = (double)dot / d, in fp64 in that order -- the writer's Jaccard
 *           before its clamp (:654-672); `dot` is the int32 dot, wrapped as mvs_pairwise_dots returns it.  The same for
 *           int32 and int16 DBs.
 *   order : J descending, equal J by the smaller column; a cell whose J is NaN is never selected, +-inf are ordinary values.
 *           MVS_TOPK_EXCLUDE_SELF in `flags` skips the cell col == row.
 *   k     : 1..256 (MVS_E_INVALID otherwise).
 *   cells : (row_end - row_begin) * k entries (`mem_cells`); on return *n_cells cells sorted by (row, col): per row its best
 *           min(k, eligible columns), in ASCENDING column order (what the shard writer needs, :718-722), with `dot` and
 *           `q` exactly as mvs_pairwise_rows reports them (q = the writer's quantised Jaccard, :658-665).
 *   norms_sq : n doubles (`mem_norms`), as for mvs_pairwise_rows.
 * Exact and deterministic: bit-identical to a brute-force evaluation of the rule above, whatever the device, the blocking or
 * the options.  Rows go in blocks whose dots fit a quarter of the free device memory (option topk_block_rows bounds them,
 * option topk_dots = 1 computes the dots on the vector ALUs instead of the matrix cores); no N x N buffer exists.  Synchronous.
 * mvs_ctx_topk_stats: what the last call did -- dots and selection kernel times summed over its row blocks (0 unless
 * mvs_ctx_set_timing is on), the number of row blocks and the rows per block.  Any pointer may be NULL. */
#define MVS_TOPK_EXCLUDE_SELF 1
int mvs_pairwise_topk(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, int k,
                      int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, int flags,
                      mvs_cell* cells, int mem_cells, int64_t* n_cells);
int mvs_ctx_topk_stats(const mvs_ctx* ctx, double* dots_ms, double* select_ms, int64_t* row_blocks, int64_t* block_rows);

/* Containment from sketches: the cells whose ESTIMATED CONTAINMENT of the row's sample in the column's sample exceeds a level.
 * Every call above scores a pair by its Jaccard estimate, which the size ratio of the two samples bounds (a sample wholly
 * contained in one 30 x its size has J <= 0.033, under every keep level here); dot / d estimates |A n B| and n2 estimates |A|,
 * so the containment |A n B| / |A| is in the same data.  The reference has nothing of the kind.
 *
 * The rule.  Row i, column j, i != j; P the int32 dot as mvs_pairwise_dots returns it (wrapped); c = min_containment,
 * 0 < c < 1; z = slack, any finite double.  Everything is fp64 and each line is ONE rounding:
 *     inter = (double)P / (double)d
 *     t     = c * n2[i]
 *     e     = inter - t                       (never fused with the product above)
 *     ok    = n2[i] > 0 && n2[i] < inf && n2[j] >= 0 && n2[j] < inf      (NaN fails)
 *     z == 0 : dir(i,j) = ok && e > 0
 *     z  > 0 : dir(i,j) = ok && e > 0 && (e*e)*(double)d > (z*z) * (n2[i]*n2[j])
 *     z  < 0 : dir(i,j) = ok && (e > 0 || (e*e)*(double)d < (z*z) * (n2[i]*n2[j]))
 * -- "the estimated containment of i in j exceeds c by more than z standard errors": the variance of inter is about
 * n2[i] n2[j] / d, and the test is written in squares so that no square root is taken.  z > 0 buys precision, z < 0 recall:
 * candidate lists for an exact step (mvs_intersect_cells).
 *   flags : MVS_CONTAIN_ROW  a cell is kept iff dir(i,j);
 *           MVS_CONTAIN_MAX  a cell is kept iff dir(i,j) || dir(j,i): max-containment, symmetric bit for bit, so its cells may
 *                            feed mvs_cluster_add_cells / mvs_linkage_add_cells.
 *   Cells with row == col are never reported.
 *   q     : Cq = inter / n2[i]; !(Cq > 0) -> 0; Cq > 1 -> 1; q = (int32)round(Cq * 255), halves away from zero.  In MAX mode
 *           the larger of the two directions' values, a direction whose row norm is not in (0, inf) counting 0.  0 <= q <= 255;
 *           0 occurs at z < 0.  dot = P.
 *   cells : `capacity` entries (`mem_cells`); on success *n_cells kept cells sorted by (row, col).  More than `capacity` kept:
 *           MVS_E_CAPACITY and *n_cells is the number needed (capacity 0 with cells NULL asks for the count alone).
 *   norms_sq : n doubles (`mem_norms`).
 *   min_containment outside (0, 1), a non-finite slack, unknown flags, ranges outside the set: MVS_E_INVALID.  An empty row or
 *   column range: MVS_OK with 0 cells.
 * Exact and deterministic: bit-identical to a brute-force evaluation of the rule above, whatever the device, the blocking or
 * the options.  Rows go in blocks sized as mvs_pairwise_topk sizes them (option contain_block_rows bounds them, option
 * contain_dots = 1 computes the dots on the vector ALUs); one dense-dots launch per block, no N x N buffer.  Synchronous.
 * mvs_ctx_contain_stats: what the last call did -- dots and selection kernel times summed over its row blocks (0 unless
 * mvs_ctx_set_timing is on), the number of row blocks and the rows per block.  Any pointer may be NULL. */
#define MVS_CONTAIN_ROW 0
#define MVS_CONTAIN_MAX 1
int mvs_pairwise_contain(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double min_containment,
                         double slack, int flags, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end,
                         mvs_cell* cells, int mem_cells, int64_t capacity, int64_t* n_cells);
int mvs_ctx_contain_stats(const mvs_ctx* ctx, double* dots_ms, double* select_ms, int64_t* row_blocks, int64_t* block_rows);

/* Neighbour counts at many Jaccard levels in one pass: how many samples every sample would be linked to at each of up to 64
 * levels -- what a level keeps, what it leaves isolated and where the neighbour counts collapse, before mvs_pairwise_cluster,
 * _linkage, _derep or mvs_search_block is run at one of them.  (The reference asks the same of its output:
 * src/interpret_pairwise_comp.py ends with a histogram of neighbours per sample.)
 *
 * The rule.  Levels t_0 < t_1 < ... < t_{m-1}, 1 <= m <= MVS_MAX_LEVELS, each 0 < t_l < 1; coef_l = t_l / (1.0 + t_l), computed
 * on the host in fp64.  Row i, column j, i != j by sample index; P the int32 dot as mvs_pairwise_dots returns it (wrapped).
 * Everything is fp64 and each line is ONE rounding; a NaN compares false:
 *     inter = (double)P / (double)d
 *     s     = n2[i] + n2[j]
 *     pass_l(i,j) = inter > coef_l * s
 *     deg[i][l]   = #{ j in [col_begin, col_end), j != i : pass_l(i,j) }
 *     total[l]    = sum over i in [row_begin, row_end) of deg[i][l]            (int64)
 * -- the link rule of mvs_pairwise_cluster / mvs_search_block, evaluated independently per level: over the full square,
 * deg[i][l] is the `degree` mvs_cluster_finish reports at min_jaccard = t_l, and total[l] is twice the number of linked pairs.
 * The contract is per level and holds for any norms (NaN, +-inf, 0, negative).
 *   levels   : n_levels doubles on the HOST.
 *   degrees  : (row_end - row_begin) x n_levels int32, row-major (`mem_degrees`); NULL when only the totals are wanted.
 *   totals   : n_levels int64 on the HOST; may be NULL.
 *   norms_sq : n doubles (`mem_norms`).
 *   n_levels outside 1 .. MVS_MAX_LEVELS, a level outside (0, 1) or NaN, levels that are not strictly ascending, computed
 *   coefficients that are not non-decreasing (two levels an ulp apart can round that way), ranges outside the set, levels or
 *   norms_sq NULL where needed: MVS_E_INVALID.  An empty row or column range: MVS_OK, nothing written to degrees, totals 0.
 * Exact and deterministic: equal to a brute-force evaluation of the rule above, whatever the device, the blocking or the
 * options.  Rows go in blocks sized as mvs_pairwise_contain sizes them (option levels_block_rows bounds them, option
 * levels_dots = 1 computes the dots on the vector ALUs); one dense-dots launch and one counting launch per block; device
 * memory besides the set is the dots block plus O(block rows x n_levels), never N x N.  Synchronous.
 * mvs_ctx_levels_stats: what the last call did -- dots and counting kernel times summed over its row blocks (0 unless
 * mvs_ctx_set_timing is on), the number of row blocks and the rows per block.  Any pointer may be NULL. */
#define MVS_MAX_LEVELS 64
int mvs_pairwise_levels(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, const double* levels,
                        int n_levels, int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, int32_t* degrees,
                        int mem_degrees, int64_t* totals);
int mvs_ctx_levels_stats(const mvs_ctx* ctx, double* dots_ms, double* count_ms, int64_t* row_blocks, int64_t* block_rows);

/* Single-linkage clustering of the samples at a Jaccard level, on the device: samples i != j are LINKED iff
 *   (double)dot / (double)d > (t / (1.0 + t)) * (n2[i] + n2[j])        (fp64, in that order; t = min_jaccard, 0 < t < 1)
 * -- "the Jaccard estimate of src/pairwise_comp_optimized.cpp:661-662 exceeds t", the rule and the kernels of mvs_search_block
 * (the floating keep test with the coefficient t/(1+t) in place of 0.05); `dot` is the wrapped int32 dot every path reports.
 * A sample whose norm is NaN or +inf is linked to nothing; every other double is held to the test as written, on every comparison
 * path: a negative norm lowers the threshold, and a sample whose norm is -inf is linked to every sample whose norm is neither NaN
 * nor +inf.  (The single-linkage tree and the greedy dereplication take their pairs from the same comparison.)  A CLUSTER is a
 * connected component of that graph.  The reference
 * has no clustering: it writes the thresholded matrix (:645-817) and leaves the grouping to its readers; here the kept cells
 * never leave the device and the answer is four int32 arrays:
 *   labels[i]          cluster of sample i; clusters are numbered 0 .. C-1 by ascending smallest member
 *   sizes[c]           members of cluster c
 *   representatives[c] the member with the largest norms_sq (the largest estimated hash set), equal values: the smaller index;
 *                      a NaN norm ranks below every number
 *   degree[i]          samples linked to i (self excluded)
 * Exact and deterministic: everything is a function of the edge set, so the arrays equal a brute force over all pairs bit
 * for bit, whatever the blocking, the options or the comparison path (mvs_cluster.hip states the argument).
 *
 * mvs_cluster_create    a forest of n singletons on the context's device (parent[i] = i, degree 0); resets the statistics
 *                       mvs_ctx_cluster_stats reports.
 * mvs_cluster_add_cells unions row ~ col of every cell of a DEVICE list (cells with row == col are ignored; dot and q are not
 *                       read) and adds 1 to degree[row] per cell with row != col -- so degree is the graph's only if every
 *                       ordered pair is fed exactly once; feeding a list twice changes degree and nothing else.  Any producer
 *                       may feed it (mvs_search_block, mvs_pairwise_block, a multi-rank step's own cells).  The list is
 *                       consumed when the call returns.  MVS_E_RANGE: a cell named a sample outside [0, n) (ignored).
 * mvs_pairwise_cluster  the one-call producer: compares `set` (n samples, the cluster's n) with itself at level min_jaccard,
 *                       row block by row block -- the launch mvs_pairwise_rows makes, with the other coefficient: every ordered
 *                       pair of linked samples arrives exactly once -- and feeds each block's unsorted list to add_cells.  No
 *                       sort, no download.  min_jaccard outside (0, 1), NaN included: MVS_E_INVALID.  Never fails because the
 *                       result is dense: the staging buffer holds option cluster_cells cells (default: a quarter of the free
 *                       device memory, at most 2^30 cells or what the block can produce); a block that reports more is halved
 *                       on a multiple of 256 rows and redone, a block of 256 rows grows the buffer instead.  Option
 *                       cluster_block_rows bounds the rows of a block (default: pairwise_block_cells / n).
 * mvs_cluster_finish    flattens the forest and writes the arrays (`mem_out` says where all four live; any pointer may be NULL;
 *                       representatives and sizes need room for n entries, *n_clusters of them are written).  norms_sq: n
 *                       doubles, read for the representatives.  More cells may be added afterwards and finish called again.
 * mvs_ctx_cluster_stats since the context's last mvs_cluster_create: time of the comparison kernels and of the union-find
 *                       kernels (hook + flatten + verify + finish; both 0 unless mvs_ctx_set_timing is on), cells with
 *                       row != col consumed, row blocks of mvs_pairwise_cluster, the most hook -> flatten -> verify rounds any
 *                       list needed.  Any pointer may be NULL.
 * All synchronous. */
typedef struct mvs_cluster mvs_cluster;
int mvs_cluster_create(mvs_ctx* ctx, int64_t n, mvs_cluster** cluster);
int mvs_cluster_add_cells(mvs_cluster* cluster, const mvs_cell* d_cells, int64_t n_cells);
int mvs_pairwise_cluster(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double min_jaccard,
                         mvs_cluster* cluster);
int mvs_cluster_finish(mvs_cluster* cluster, const double* norms_sq, int mem_norms, int32_t* labels, int32_t* degree,
                       int32_t* representatives, int32_t* sizes, int mem_out, int64_t* n_clusters);
int mvs_cluster_destroy(mvs_cluster* cluster);
int mvs_ctx_cluster_stats(const mvs_ctx* ctx, double* compare_ms, double* union_ms, int64_t* edges, int64_t* row_blocks,
                          int64_t* rounds);

/* ---- the single-linkage tree: maximum spanning forest of the kept cells -------------------------------------------------------
 * mvs_pairwise_cluster answers one level.  The maximum spanning forest of the thresholded Jaccard graph is the single-linkage
 * dendrogram: at most n - 1 links, and cutting it at any level >= the level it was built at gives exactly the connected
 * components of the graph cut at that level -- one comparison at the lowest level of interest instead of one per level.  The
 * reference has nothing of the kind.
 *
 * Graph.  For n samples, norms n2, dimension d and a level 0 < t < 1, the edge set is mvs_pairwise_cluster's: i != j linked iff
 *   (double)P / (double)d > (t / (1.0 + t)) * (n2[i] + n2[j]),  P the wrapped int32 dot.  A NaN or +inf norm links to nothing.
 * Weight.  The weight of an edge is mvs_pairwise_topk's score: inter = (double)P / d; J = inter / (n2[i] + n2[j] - inter), fp64
 *   in that order.  It is symmetric bit for bit.
 * Order.  Edges are totally ordered "best first" by (key(J) descending, lo ascending, hi ascending): lo = min(i, j),
 *   hi = max(i, j); key is the order-preserving map of mvs_pairwise_topk (-0.0 folded into +0.0, +-inf ordinary values); a
 *   cell whose J is NaN is ignored, as top-k ignores it.
 * Result.  The maximum spanning forest under that order -- unique, because the order is total -- as mvs_link records
 *   { a = lo, b = hi, dot, q, jaccard } (24 bytes), SORTED BEST FIRST: n - C links for C components.  dot and q are exactly what
 *   mvs_pairwise_rows / mvs_search_block report for that cell, jaccard is the fp64 J above, bit for bit.
 * Exactness.  The forest is a function of the edge set and the norms only: the blocking, the options, the comparison path, the
 *   order of cells and the number of times a cell is fed do not change it.  It equals a host Kruskal under the same order, bit
 *   for bit.  Parallel copies of a pair, (r, c) and (c, r), are one edge.  Feeding a list twice changes nothing (`degree` of
 *   mvs_cluster does not have this property).
 * Cut property.  For any level u the links with jaccard > u form a prefix of the output, and their components equal the
 *   components of {edges of the graph with J > u}.  That equals mvs_pairwise_cluster at u whenever the two forms of the test,
 *   J > u and the product-form keep test, agree on every pair -- always, except for a pair within a rounding error of the level.
 *
 * mvs_linkage_create    an empty forest over n samples of dimension d on the context's device; norms_sq (n doubles) is copied
 *                       to the device and decides every weight.  Resets the statistics mvs_ctx_linkage_stats reports.
 * mvs_linkage_set_core  switches the weight to the MUTUAL REACHABILITY of HDBSCAN* (section below): core (n doubles, `mem_core`) is
 *                       copied to the device, and from then on the weight of the edge (lo, hi) is m = min(J, core[lo], core[hi]),
 *                       the minimum taken in key order: J, unless a core value's key is strictly smaller -- then that value, lo's
 *                       before hi's.  An edge whose J or either core value is NaN is ignored (and counted with the fed cells, as
 *                       a NaN J is today).  The order stays (key(m) descending, lo, hi): total, so the forest is still unique,
 *                       equal to a host Kruskal under that order, and independent of blocking, cell order and repeats -- the
 *                       argument needs a fixed weight per edge, nothing more.  In this mode the field `jaccard` of mvs_link
 *                       holds m, bit for bit: finish sorts by it, mvs_linkage_cells(level) returns the prefix with m > level,
 *                       and J stays recomputable from dot and the norms.  Allowed only before the first cell is fed
 *                       (MVS_E_INVALID afterwards: a forest built under one weight says nothing about another); may be
 *                       called again until then.  Without it every result is bit for bit what it was.
 * mvs_linkage_add_cells replaces the forest F by the maximum spanning forest of F and the cells of a DEVICE list.  Unlike
 *                       mvs_cluster_add_cells it reads `dot`, so any producer that reports real dots may feed it
 *                       (mvs_pairwise_rows, mvs_pairwise_block, mvs_search_block, mvs_pairwise_topk).  Cells with row == col
 *                       and cells whose J is NaN are ignored.  MVS_E_RANGE: a cell named a sample outside [0, n) -- that cell is
 *                       ignored and every other cell is consumed (the rule of mvs_cluster_add_cells).
 * mvs_pairwise_linkage  the one-call producer: mvs_pairwise_cluster's loop with this consumer -- same launch, same staging
 *                       buffer, same halving and grow rule, same options cluster_cells / cluster_block_rows, same argument
 *                       checks and error codes.  norms_sq here feeds the keep test; pass the norms the linkage was created with.
 * mvs_linkage_finish    sorts the links best first and writes them (`mem_out` says where).  capacity too small: MVS_E_CAPACITY,
 *                       *n_links = the needed count.  May be called again after more cells.
 * mvs_linkage_cells     the links with jaccard > level as a DEVICE cell list (row = a, col = b, dot, q), best first: ready for
 *                       mvs_cluster_add_cells (labels, sizes and representatives at that level -- `degree` of a cluster fed
 *                       this way is the FOREST's degree, not the graph's) and for mvs_intersect_cells (the exact Jaccard of the
 *                       backbone).  MVS_E_CAPACITY reports the needed count in *n_cells; a NaN level is MVS_E_INVALID.
 * mvs_ctx_linkage_stats since the context's last mvs_linkage_create: time of the comparison kernels and of the forest kernels
 *                       (rounds + the sort of finish; both 0 unless mvs_ctx_set_timing is on), fed cells with row != col,
 *                       row blocks of mvs_pairwise_linkage, the most rounds any list needed.  Any pointer may be NULL.
 * All synchronous.  The kernels and the argument for their exactness are in mvs_linkage.hip. */
typedef struct mvs_link {
    int32_t a;         /* the smaller sample index */
    int32_t b;         /* the larger one */
    int32_t dot;
    int32_t q;
    double jaccard;    /* the weight: J, or the mutual reachability m once mvs_linkage_set_core was called */
} mvs_link;
typedef struct mvs_linkage mvs_linkage;
int mvs_linkage_create(mvs_ctx* ctx, int64_t n, int d, const double* norms_sq, int mem_norms, mvs_linkage** linkage);
int mvs_linkage_set_core(mvs_linkage* linkage, const double* core, int mem_core);
int mvs_linkage_add_cells(mvs_linkage* linkage, const mvs_cell* d_cells, int64_t n_cells);
int mvs_pairwise_linkage(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double min_jaccard,
                         mvs_linkage* linkage);
int mvs_linkage_finish(mvs_linkage* linkage, mvs_link* links, int64_t capacity, int mem_out, int64_t* n_links);
int mvs_linkage_cells(mvs_linkage* linkage, double level, mvs_cell* d_cells, int64_t capacity, int64_t* n_cells);
int mvs_linkage_destroy(mvs_linkage* linkage);
int mvs_ctx_linkage_stats(const mvs_ctx* ctx, double* compare_ms, double* forest_ms, int64_t* edges, int64_t* row_blocks,
                          int64_t* rounds);

/* ---- HDBSCAN* on the Jaccard estimates: clusters without a level to choose -----------------------------------------------------
 * Every grouping call above takes one Jaccard level, and single linkage chains: a path of overlapping samples is one cluster.
 * HDBSCAN* (Campello, Moulavi, Sander 2013; McInnes, Healy 2017) answers both.  It weighs a pair by its MUTUAL REACHABILITY
 * m(i, j) = min(core[i], core[j], J(i, j)), core[i] the similarity of i's K-th nearest neighbour -- a thin chain between two dense
 * groups then weighs only as much as its sparsest sample --, builds the single-linkage tree of that weight, and picks clusters
 * by their stability over ALL levels.  The reference has nothing of the kind.  Both expensive halves are the exact device paths
 * above (mvs_pairwise_topk, the forest of mvs_linkage_*); the selection is integer arithmetic on the host, so every output is a
 * function of the set, the norms and the parameters alone.
 *
 * Core.  core[i] = the K-th best score of row i under mvs_pairwise_topk's rule, every column eligible, MVS_TOPK_EXCLUDE_SELF
 *   set: the minimum in key order of the fp64 J of the K cells top-k returns for the row, J = inter / (n2[i] + n2[j] - inter),
 *   inter = (double)P / d, -0.0 folded into +0.0.  A row that gets fewer than K cells (its scores are NaN) has core = NaN.
 *   K = min_samples, 1 <= K <= 256 and K <= n - 1 (MVS_E_INVALID otherwise).
 * Levels.  lambda(x) = llrint(min(max(x, 0), 1) * 2^30): every level below is an int64, every stability an exact int64 sum.
 * Dendrogram.  The links with m > floor (fp64 compare), best first as mvs_linkage_finish returns them under
 *   mvs_linkage_set_core, are Kruskal merges: merge v has lambda_v = lambda(m), two children and a size.  A forest; samples no
 *   link touches are singleton roots.
 * Condensed tree, top-down from every root of size >= s = min_cluster_size (smaller roots are noise).  A cluster C is born at
 *   birth(C) (lambda(floor) for a root).  At a merge v inside C: both children >= s -- C ends, every sample under v leaves C at
 *   lambda_v, two clusters are born at lambda_v; exactly one child >= s -- the samples of the small child leave C at lambda_v, C
 *   continues into the large one; both < s -- every sample under v leaves at lambda_v, C ends as a leaf cluster.
 *   stability(C) = sum over all samples ever in C of (lambda_leave(p, C) - birth(C)); death(C) = the split's lambda, for a leaf
 *   the largest lambda_leave.
 * Selection by excess of mass, bottom-up.  A leaf has S^ = stability.  A cluster with children A, B is selected when
 *   stability(C) >= S^(A) + S^(B) (ties go to the parent): its descendants are deselected and S^(C) = stability(C); otherwise
 *   S^(C) = S^(A) + S^(B).  Roots are eligible: a root is a component at the floor, what mvs_pairwise_cluster reports there.
 *   With MVS_HDBSCAN_NO_ROOTS a root that has child clusters is never selected.
 * Output.
 *   clusters : one mvs_hdbscan_cluster per condensed cluster, sorted by (smallest member ascending, size descending): parent
 *              (index into this array, -1 for a root), size at birth, selected (0 / 1), representative (the member at birth with
 *              the largest core in key order, NaN below every number, ties to the smaller index; core == NULL: the smallest
 *              member), birth, death, stability.  Fewer than max(n, 2) of them (leaves are disjoint and hold >= 2 samples, the rest have
 *              two children); MVS_E_CAPACITY reports the count in *n_clusters.
 *   labels[i]     the rank among the SELECTED clusters (in array order) of the one whose subtree holds i, -1 for noise.
 *   strength[i]   (min(lambda_i, lmax(C)) - birth(C)) / (lmax(C) - birth(C)) for i's selected cluster C, lambda_i the level at
 *                 which i left its last cluster and lmax(C) the largest such level under C: one fp64 division of two exactly
 *                 converted integers; 1.0 when the denominator is 0, 0.0 for noise.
 *   lambda_out[i] lambda_i, -1 for a sample that was never in a cluster.
 *
 * mvs_core_jaccard    core[] of every sample of the set -> core_out (n doubles, `mem_out`).  Top-k runs over row ranges into a
 *                     bounded device cell buffer (option core_block_rows bounds a range); a kernel reduces each range's ragged
 *                     list to its rows' values (mvs_core.hip); no cell list crosses the link.
 * mvs_hdbscan_select  pure host, needs no device: n, the links best first (by (key(jaccard) descending, a, b): anything else,
 *                     a link outside [0, n), a == b, a NaN weight or a link that closes a cycle is MVS_E_INVALID), core (n
 *                     doubles or NULL), floor (not NaN), min_cluster_size >= 2, flags.  Any output pointer may be NULL.
 * mvs_hdbscan         core (K = min_samples), linkage with that core at `floor` (0 < floor < 1, as mvs_pairwise_linkage), finish,
 *                     select.  core_out, links (room for n - 1), n_links and the outputs of the selection are HOST buffers;
 *                     any may be NULL.  cluster_capacity as above.  The pairs that arrive are those of the comparison's keep
 *                     test at `floor` (the cut property's caveat above applies); the selection's m > floor only removes links.
 * mvs_ctx_hdbscan_stats  of the context's last mvs_core_jaccard / mvs_hdbscan: kernel times of top-k's dots and selection summed
 *                     over the ranges and of the reduction (0 unless mvs_ctx_set_timing is on), of the comparison and the
 *                     forest (mvs_ctx_linkage_stats), host time of the selection (always measured); top-k ranges, the most
 *                     Boruvka rounds a list needed, links, fed cells.  Any pointer may be NULL. */
#define MVS_HDBSCAN_NO_ROOTS 1
typedef struct mvs_hdbscan_cluster {
    int32_t parent;
    int32_t size;
    int32_t selected;
    int32_t representative;
    int64_t birth;
    int64_t death;
    int64_t stability;
} mvs_hdbscan_cluster;
int mvs_core_jaccard(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, int k, double* core_out,
                     int mem_out);
int mvs_hdbscan_select(int64_t n, const mvs_link* links, int64_t n_links, const double* core, double floor, int64_t min_cluster_size,
                       int flags, int32_t* labels, double* strength, int64_t* lambda_out, mvs_hdbscan_cluster* clusters,
                       int64_t cluster_capacity, int64_t* n_clusters);
int mvs_hdbscan(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, int min_samples, double floor,
                int64_t min_cluster_size, int flags, double* core_out, mvs_link* links, int64_t* n_links, int32_t* labels,
                double* strength, int64_t* lambda_out, mvs_hdbscan_cluster* clusters, int64_t cluster_capacity, int64_t* n_clusters);
int mvs_ctx_hdbscan_stats(const mvs_ctx* ctx, double* core_dots_ms, double* core_select_ms, double* core_kth_ms, double* compare_ms,
                          double* forest_ms, double* host_ms, int64_t* ranges, int64_t* rounds, int64_t* links, int64_t* edges);

/* ---- greedy dereplication: representatives with a radius guarantee -------------------------------------------------------------
 * Single linkage chains: a cluster's representative may have nothing in common with most of its members.  Dereplication wants
 * what greedy incremental clustering gives (the rule of dRep, galah, CD-HIT, linclust): the lexicographically first maximal
 * independent set of the threshold graph under a priority order.  The reference has nothing of the kind.
 *
 * Graph.  Exactly mvs_pairwise_cluster's: samples i != j are linked iff
 *   (double)P / (double)d > (t / (1.0 + t)) * (n2[i] + n2[j]),  P the wrapped int32 dot, 0 < t < 1.  A NaN or +inf norm links to
 *   nothing.
 * Order.  A permutation order[0..n) of the samples; order[0] goes first.  The default is norms_sq descending under the key of
 *   mvs_cluster_finish's representatives (NaN ranks below every number, -0.0 ties with +0.0), equal keys by the smaller index.
 * Result.  Walk the samples in that order.  A sample becomes a REPRESENTATIVE iff none of the samples linked to it that come
 *   earlier in the order is a representative; otherwise it is a MEMBER of the earliest-in-order representative linked to it.
 *   In the caller's index space:
 *   rep_of[i]               the sample's representative; i itself for a representative
 *   link_dot[i], link_q[i]  dot and q of the cell (i, rep_of[i]), exactly as mvs_pairwise_rows reports them; 0 and -1 for a
 *                           representative
 *   sizes[i]                samples assigned to i including itself; 0 for a member
 *   *n_reps                 the number of representatives
 * Properties.  No two representatives are linked.  Every member is linked to its representative.  The result is a function of
 *   (edge set, order) only: independent of the blocking, the options, the comparison path, the order of cells in a list and of
 *   duplicate or mirrored cells.  rep_of[i] lies in i's single-linkage cluster at the same level, hence n_reps >= n_clusters, with
 *   equality iff every cluster is a star around its best member.
 *
 * mvs_sketch_set_gather an owned set of n_rows rows, same d and limb code: row i is row rows[i] of src (rows may repeat; `rows`
 *                       lives where mem_rows says).  A row outside [0, src n): MVS_E_RANGE, no set is returned.
 * mvs_derep_create      n undecided samples on the context's device, greedy in ROW order (row 0 first: the caller has permuted
 *                       its samples into the order it wants, see mvs_dereplicate); resets the statistics
 *                       mvs_ctx_derep_stats reports.
 * mvs_derep_add_rows    decides rows [row_begin, row_end) from a DEVICE list that holds every cell (r, c), c < r, of those rows;
 *                       cells with c >= r are ignored (row c's own list brings (c, r)), copies of a cell change nothing.
 *                       row_begin must equal the number of rows decided so far, else MVS_E_INVALID: everything before a block is
 *                       final when the block arrives, which is why nothing is kept between blocks.  A cell naming a row outside
 *                       [row_begin, row_end) or a column outside [0, n): MVS_E_RANGE -- that cell is ignored and every other
 *                       cell is consumed (the rule of mvs_cluster_add_cells).  The list is consumed when the call returns.
 * mvs_pairwise_derep    the one-call producer: mvs_pairwise_cluster's loop with this consumer -- same launch, same staging
 *                       buffer, same halving and grow rule, same options cluster_cells / cluster_block_rows, same argument
 *                       checks and error codes.  The dereplication must not have decided any row yet.
 * mvs_derep_finish      writes the arrays (`mem_out` says where all four live; any pointer may be NULL).  order (n int32 where
 *                       mem_order says; NULL = identity) maps rows back to the caller's samples: row r is sample order[r].
 *                       Not a permutation of [0, n), or rows still undecided: MVS_E_INVALID.
 * mvs_ctx_derep_stats   since the context's last mvs_derep_create: time of the comparison kernels and of the greedy kernels
 *                       (both 0 unless mvs_ctx_set_timing is on), cells with row != col consumed, row blocks of
 *                       mvs_pairwise_derep, the most rounds any block needed.  Any pointer may be NULL.
 * mvs_dereplicate       the one call: builds the order (order: n HOST int32, or NULL = by norm as above; not a permutation of
 *                       [0, n): MVS_E_INVALID), gathers the set and the norms into that order unless it is the identity, then
 *                       mvs_derep_create, mvs_pairwise_derep and mvs_derep_finish with the order.
 * All synchronous.  The kernels and the argument for their exactness are in mvs_derep.hip. */
int mvs_sketch_set_gather(mvs_ctx* ctx, const mvs_sketch_set* src, const int32_t* rows, int mem_rows, int64_t n_rows,
                          mvs_sketch_set** out);
typedef struct mvs_derep mvs_derep;
int mvs_derep_create(mvs_ctx* ctx, int64_t n, mvs_derep** derep);
int mvs_derep_add_rows(mvs_derep* derep, const mvs_cell* d_cells, int64_t n_cells, int64_t row_begin, int64_t row_end);
int mvs_pairwise_derep(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double min_jaccard,
                       mvs_derep* derep);
int mvs_derep_finish(mvs_derep* derep, const int32_t* order, int mem_order, int32_t* rep_of, int32_t* link_dot, int32_t* link_q,
                     int32_t* sizes, int mem_out, int64_t* n_reps);
int mvs_derep_destroy(mvs_derep* derep);
int mvs_ctx_derep_stats(const mvs_ctx* ctx, double* compare_ms, double* greedy_ms, int64_t* edges, int64_t* row_blocks,
                        int64_t* rounds);
int mvs_dereplicate(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double min_jaccard,
                    const int32_t* order, int32_t* rep_of, int32_t* link_dot, int32_t* link_q, int32_t* sizes, int mem_out,
                    int64_t* n_reps);

/* ---- exact hash-set intersections for kept pairs --------------------------------------------------------------------------
 * Everything above reports the ESTIMATE of a pair: dot, q, the top-k lists and the clusters are exact with respect to the
 * reference's arithmetic, which estimates |A n B| from two +-1 random projections.  These calls compute the quantity itself
 * from the hash lists the sketches were made of, for the pairs a comparison kept ("filter on sketches, verify on sets").
 * They would replace nothing on the reference's hot path: the closest reference code is its offline error study on simulated
 * vectors (src/compute_error_of_random_projections.py, jaccard_exact() and the RMSE studies); nothing there says which kept
 * pairs of real data are above the level.
 *
 * For hash lists H(s) (set semantics: a value that occurs several times in a sample counts once) and cells (row, col):
 *     inter[i] = | H_rows(cells[i].row) n H_cols(cells[i].col) |        (int32, exact)
 * `dot` and `q` of a cell are not read; row == col on the same set gives the sample's size; an empty sample intersects to 0; a
 * cell that appears several times is answered every time.  Hash values are arbitrary 64-bit words (0 and 2^64 - 1 are
 * ordinary values; the implementation has no sentinel).  Exact and deterministic: equal to the size of the intersection of
 * the two sorted, de-duplicated lists whatever the blocking, the options or the order of the cells.  Derived quantities
 * (Jaccard = inter / (|A| + |B| - inter), containment = inter / |A|) are the caller's, in fp64.
 *
 * mvs_hash_set_create   a resident copy of the lists in HBM, per sample sorted and de-duplicated.  hashes / offsets as for
 *                       mvs_project_csr (offsets: n_samples + 1 HOST int64, non-decreasing -- MVS_E_INVALID otherwise; each
 *                       sample < 2^31 hashes, the total may pass 2^32: positions are 64-bit).  One pass checks "strictly
 *                       increasing inside every sample"; where that holds (the <hash_file>.csr cache, sorted inputs) the
 *                       data is used as uploaded, otherwise a segmented radix sort and a unique compaction run on the
 *                       device (which then holds input + sorted copy + result for the duration of the call).  Host lists
 *                       are uploaded with ONE plain copy of the whole list, not through the pinned staging pipeline of
 *                       mvs_project_csr_stats: a set is built once and then serves many calls.  Synchronous.
 * mvs_hash_set_info     samples, distinct hashes in total, whether the input was already sorted and unique.  Any pointer may be NULL.
 * mvs_hash_set_sizes    distinct hashes per sample: n_samples int32 (`mem_out` says where).  Synchronous.
 * mvs_intersect_cells   the contract above for n_cells cells (`mem_cells`) into inter (`mem_out`); hs_cols == NULL: columns
 *                       index hs_rows too.  With device cells and device inter nothing but counters crosses the link: the
 *                       lists of mvs_pairwise_rows, mvs_search_block and mvs_pairwise_topk with mem_cells = MVS_MEM_DEVICE
 *                       feed it as they stand.  A cell that names a sample outside its set: MVS_E_RANGE, nothing is written
 *                       for that cell, every other cell is answered (the rule of mvs_cluster_add_cells).  NULL buffers,
 *                       negative n_cells, sets of another context: MVS_E_INVALID.  Synchronous.
 *                       Work is laid out in units of option intersect_unit (default 2048) elements of a pair's shorter list
 *                       against the window of the longer one they can match, one wave per unit, in cell order (a list
 *                       sorted by row reuses the row's hashes from the caches); the option never changes a result.
 * mvs_ctx_intersect_stats  the context's last mvs_intersect_cells: time of its kernels (0 unless mvs_ctx_set_timing is on),
 *                       units launched, pairs cut into several units, and the bytes the contract implies: the sum of
 *                       8 (|A| + |B|) over the cells in range.  Any pointer may be NULL. */
typedef struct mvs_hash_set mvs_hash_set;
int mvs_hash_set_create(mvs_ctx* ctx, const uint64_t* hashes, int mem_hashes, const int64_t* offsets, int64_t n_samples,
                        mvs_hash_set** set);
int mvs_hash_set_info(const mvs_hash_set* set, int64_t* n_samples, int64_t* n_hashes, int* was_sorted);
int mvs_hash_set_sizes(const mvs_hash_set* set, int32_t* sizes, int mem_out);
int mvs_hash_set_destroy(mvs_hash_set* set);
int mvs_intersect_cells(mvs_ctx* ctx, const mvs_hash_set* hs_rows, const mvs_hash_set* hs_cols, const mvs_cell* cells,
                        int mem_cells, int64_t n_cells, int32_t* inter, int mem_out);
int mvs_ctx_intersect_stats(const mvs_ctx* ctx, double* kernel_ms, int64_t* units, int64_t* cut_pairs, int64_t* bytes);

/* ---- sketches from sequences: FracMinHash values of DNA bytes ------------------------------------------------------------------
 * Every path of this library starts from hash lists.  These calls make them from sequences, on the device, as a mvs_hash_set:
 * mvs_intersect_cells and mvs_gather take it as it is, mvs_project_csr takes its device pointer (mvs_hash_set_device).  The
 * reference has no hashing of sequences (only its unused extract_31mers hints at the need), so nothing of it is replaced.
 *
 * A SAMPLE is a byte string.  Its sketch for (ksize, seed, max_hash) is the ascending list of the distinct values h below.
 *   Bases and breaks: the bytes A C G T a c g t are bases, lower case counting as upper case; every other byte (N, IUPAC codes,
 *     '\n', 0, 255, ...) is a break.  No k-mer contains a break; a caller joins the records of one sample with one break byte,
 *     so that no k-mer spans two records.
 *   Per k-mer: for every position i such that bytes i .. i + ksize - 1 are all bases, fw = those bytes upper-cased, rc = the
 *     reverse complement (A<->T, C<->G), canon = the bytewise-lexicographically smaller of the two,
 *         h = the FIRST 64-bit word of MurmurHash3_x64_128(canon, ksize bytes, seed)       (Appleby, public domain)
 *     and h is kept iff h <= max_hash.  1 <= ksize <= 32 (a k-mer is then one 64-bit word of 2-bit codes, whose integer order is
 *     the string order); ksize > 32 is refused.
 *   max_hash(scaled) = (uint64)(2^64 / (double)scaled) for scaled >= 2 and 2^64 - 1 for scaled = 1 (keep everything): 1000 gives
 *     18446744073709552, 2000 gives 9223372036854776.
 * Exact and deterministic whatever the options, the units of work or where the bytes lie.  Not offered: ksize > 32,
 * abundances, sourmash .sig JSON, adding bases to a sample over several calls, several GPUs.  (Protein, dayhoff and hp
 * alphabets: "protein sketches" below.)
 *
 * mvs_kmer_max_hash     the formula above.  Pure host.  scaled < 1: MVS_E_INVALID.
 * mvs_kmer_hash         the per-k-mer rule for the ksize bytes at `kmer`: *h and *valid = 1, or *valid = 0 (and *h = 0) if one
 *                       of them is a break.  Pure host: the library's own statement of the contract.
 * mvs_hash_set_from_sequences
 *                       the sketches of n_samples samples -> a new hash set (destroy it with mvs_hash_set_destroy).  Sample s
 *                       is bytes [offsets[s], offsets[s + 1]) of `bases` (`mem_bases` says where they lie; offsets: n_samples
 *                       + 1 HOST int64, non-decreasing).  Samples may be empty or shorter than ksize: they get an empty list.
 *                       The byte count is 64-bit; a sample keeps fewer than 2^31 values (MVS_E_RANGE otherwise).  NULL
 *                       pointers, ksize outside 1 .. 32, decreasing offsets: MVS_E_INVALID, nothing is allocated.  Host
 *                       bytes go up in ONE plain copy, as for mvs_hash_set_create.  Synchronous.
 *                       How: the host cuts the samples into units of up to option kmer_unit positions, one workgroup each;
 *                       kept values are appended to a staging list sized for the expected number (positions x (max_hash + 1)
 *                       / 2^64, plus an eighth and 65536; option kmer_capacity > 0: exactly that many).  The counts are exact
 *                       even when the list is too short: the hashing pass then runs a second time with a list of exactly
 *                       the counted size -- nothing is ever truncated.  The values are moved to their samples' ranges and
 *                       mvs_hash_set_create's segmented sort and unique compaction finish the set.
 * mvs_hash_set_export   what a set (however it was made) holds: `hashes` (total values where `mem_out` says, per sample
 *                       strictly increasing) and `offsets` (n_samples + 1 HOST int64).  Either may be NULL.  Synchronous.
 * mvs_hash_set_device   the device address of the set's values, valid until the set is destroyed: with the exported offsets,
 *                       mvs_project_csr(..., MVS_MEM_DEVICE, offsets, ...) projects the set where it lies.
 * mvs_ctx_kmer_stats    the context's last mvs_hash_set_from_sequences: time of its hashing passes and of the move into sample
 *                       order (0 unless mvs_ctx_set_timing is on), bytes given, valid positions (k-mers), values kept before
 *                       the unique compaction, units of work, hashing passes repeated for a longer staging list.  Any
 *                       pointer may be NULL.
 * mvs_ctx_kmer_sample_stats
 *                       ... and per sample: valid positions and values kept before the unique compaction, n_samples int64
 *                       each on the host (n_samples must be the last call's: MVS_E_INVALID otherwise).  Either may be NULL. */
int mvs_kmer_max_hash(int64_t scaled, uint64_t* max_hash);
int mvs_kmer_hash(const char* kmer, int ksize, uint32_t seed, uint64_t* h, int* valid);
int mvs_hash_set_from_sequences(mvs_ctx* ctx, const uint8_t* bases, int mem_bases, const int64_t* offsets, int64_t n_samples,
                                int ksize, uint32_t seed, uint64_t max_hash, mvs_hash_set** set);
int mvs_hash_set_export(const mvs_hash_set* set, uint64_t* hashes, int mem_out, int64_t* offsets);
int mvs_hash_set_device(const mvs_hash_set* set, const uint64_t** d_hashes);
int mvs_ctx_kmer_stats(const mvs_ctx* ctx, double* kernel_ms, int64_t* bases, int64_t* kmers, int64_t* kept, int64_t* units,
                       int64_t* second_trips);
int mvs_ctx_kmer_sample_stats(const mvs_ctx* ctx, int64_t n_samples, int64_t* kmers, int64_t* kept);

/* ---- protein sketches: FracMinHash values of residues, from proteins or from DNA in six frames ----------------------------------
 * DNA k-mers at ksize 31 see nothing below roughly 80 % identity; relations at the level of a family show in protein k-mers, in
 * the amino acids themselves or in reduced alphabets.  These calls make such sketches, as a mvs_hash_set like the one above:
 * every consumer takes it unchanged.
 *
 * A SAMPLE is a byte string.  Its sketch for (input kind, alphabet, ksize, seed, max_hash) is the ascending list of the distinct
 * kept values h below.
 *   Residues: the 20 letters A C D E F G H I K L M N P Q R S T V W Y in either case (lower case counting as upper case) and
 *     '*', the stop, are residues; every other byte (X B Z J U O - '\n' 0 255 ...) is a break.  No k-mer contains a break; a
 *     caller joins the records of one sample with one '\n'.
 *   Alphabets: what the hash reads, one byte per residue.
 *     MVS_AA_PROTEIN  the upper-case letter;
 *     MVS_AA_DAYHOFF  C -> a;  A G P S T -> b;  D E N Q -> c;  H K R -> d;  I L M V -> e;  F W Y -> f;
 *     MVS_AA_HP       A F G I L M P V W Y -> h;  C D E H K N Q R S T -> p;
 *     '*' stays '*' in all three.
 *   Hash: h = the FIRST 64-bit word of MurmurHash3_x64_128(the ksize encoded bytes, seed), kept iff h <= max_hash
 *     (mvs_kmer_max_hash, unchanged).  There is no canonical form: a protein has one direction.  1 <= ksize <= 64 residues.
 *     Customary: seed 42, scaled 200, ksize 10 / 16 / 42 for protein / dayhoff / hp.
 *   MVS_SEQ_PROTEIN: the bytes are residues; every window of ksize residues gives one h.
 *   MVS_SEQ_TRANSLATE: the bytes are DNA, bases and breaks exactly as in "sketches from sequences".  The genetic code is the
 *     standard one: codon xyz with T, C, A, G = 0, 1, 2, 3 indexes
 *         FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG       at 16x + 4y + z.
 *     The sketch is the union over all six reading frames: for every maximal run of bases, the run and its reverse complement,
 *     each at offsets 0, 1 and 2, translated codon by codon (a trailing partial codon is dropped); every window of ksize
 *     residues gives one h.  Equivalently: every window of 3 * ksize bases gives two values, one of its codons read forward,
 *     one of the codons of its reverse complement.
 *   Statistics: `kmers` counts hashed k-mers (two per window with MVS_SEQ_TRANSLATE), `kept` the values <= max_hash, duplicates
 *     included.
 * An unknown residue or codon is a break here (sourmash hashes it as X); byte-compatibility with sourmash's signatures is not
 * claimed.  Not offered: translated read sets with abundances, other genetic codes, .sig JSON, several GPUs.
 *
 * mvs_translate_codon   the residue of the three bytes at `codon3`: *aa (an upper-case letter or '*') and *valid = 1, or *valid =
 *                       0 (and *aa = 0) if one of them is no base.  Pure host.
 * mvs_aa_hash           the hash of the ksize residues at `kmer` in `alphabet`: *h and *valid = 1, or *valid = 0 (and *h = 0) if
 *                       one of them is a break.  Pure host, and shares no code with the kernel.
 * mvs_hash_set_from_residues
 *                       the sketches of n_samples samples -> a new hash set.  Samples, offsets, `mem_bytes`, limits and
 *                       synchrony as for mvs_hash_set_from_sequences.  NULL pointers, an input kind or alphabet that is none
 *                       of the constants, ksize outside 1 .. 64, decreasing offsets: MVS_E_INVALID, nothing is allocated.
 *                       How: the frame of mvs_hash_set_from_sequences with its options kmer_unit and kmer_capacity (the
 *                       staging list expects two values per window with MVS_SEQ_TRANSLATE), and k_aa_hash as the hashing
 *                       pass.  Its planes of residues cost LDS, so a unit holds at most 18432 positions with
 *                       MVS_SEQ_PROTEIN and 12032 with MVS_SEQ_TRANSLATE whatever kmer_unit says.
 * mvs_ctx_aa_stats, mvs_ctx_aa_sample_stats
 *                       the context's last mvs_hash_set_from_residues, shaped like mvs_ctx_kmer_stats and
 *                       mvs_ctx_kmer_sample_stats (which keep what the last mvs_hash_set_from_sequences left). */
#define MVS_SEQ_PROTEIN   0
#define MVS_SEQ_TRANSLATE 1
#define MVS_AA_PROTEIN 0
#define MVS_AA_DAYHOFF 1
#define MVS_AA_HP      2
int mvs_translate_codon(const char* codon3, char* aa, int* valid);
int mvs_aa_hash(const char* kmer, int ksize, int alphabet, uint32_t seed, uint64_t* h, int* valid);
int mvs_hash_set_from_residues(mvs_ctx* ctx, const uint8_t* bytes, int mem_bytes, const int64_t* offsets, int64_t n_samples,
                               int input_kind, int alphabet, int ksize, uint32_t seed, uint64_t max_hash, mvs_hash_set** set);
int mvs_ctx_aa_stats(const mvs_ctx* ctx, double* kernel_ms, int64_t* bytes, int64_t* kmers, int64_t* kept, int64_t* units,
                     int64_t* second_trips);
int mvs_ctx_aa_sample_stats(const mvs_ctx* ctx, int64_t n_samples, int64_t* kmers, int64_t* kept);

/* ---- abundances: read sets, k-mer counts, a minimum count ----------------------------------------------------------------------
 * A metagenome sample is a read set, and in raw reads most distinct k-mers are sequencing errors seen once.  These calls count
 * how often every kept value occurs in a sample, whatever the number of calls the sample's bases arrive in, and build the set
 * from the values whose count passes a filter.  Bases, breaks, the canonical k-mer, the hash, max_hash and 1 <= ksize <= 32 are
 * exactly those of "sketches from sequences" above.
 *
 *   Pieces.  A PIECE is a byte string that belongs to a sample index.  No k-mer spans two pieces: the caller cuts at record
 *     borders.  The pieces of a sample may arrive in any number of calls, in any order, mixed with other samples' pieces.
 *   Abundance.  M(s) is the multiset of the kept values h <= max_hash over all valid positions of all pieces of sample s; the
 *     abundance a_s(h) is the multiplicity of h in M(s).
 *   Finish(min_abundance >= 1, max_abundance; 0 = no cap) returns a hash set: sample s holds, ascending, the h with
 *     min_abundance <= a_s(h), and a_s(h) <= max_abundance if max_abundance > 0.  The set carries a uint32 abundance per value,
 *     aligned with the values.  With min_abundance = 1 and max_abundance = 0 the values equal mvs_hash_set_from_sequences of
 *     the same samples bit for bit.
 *   Histogram (optional, a HOST int64[n_samples][256]): bin b counts the distinct h of sample s with min(a_s(h), 255) == b,
 *     BEFORE the filter.  Bin 0 is always 0.
 *   Weights.  The same rule applies to arbitrary hash lists with optional uint32 weights (mvs_hash_set_create_counted): the
 *     abundance of a value is the sum of the weights of its occurrences in the sample, 1 each without weights.  A sum >= 2^32
 *     is MVS_E_RANGE.  A value whose weights sum to 0 counts as absent: it is no distinct value, has no histogram bin and is
 *     never kept.  Values are arbitrary 64-bit words: 0 and 2^64 - 1 are ordinary values, there is no sentinel.
 *   Invariance.  Exact and deterministic: the result does not depend on the options, the units of work, the cutting into pieces
 *     and calls, the arrival order, or where the bytes lie.
 *
 * mvs_kmer_sketcher_create   a sketcher for n_samples samples (all empty).  ksize outside 1 .. 32, n_samples < 0: MVS_E_INVALID.
 * mvs_kmer_sketcher_add      n_pieces pieces: piece i is bytes [offsets[i], offsets[i + 1]) of `bases` (`mem_bases` says where
 *                       they lie; offsets: n_pieces + 1 HOST int64, non-decreasing) and belongs to sample samples[i] (HOST
 *                       int32).  n_pieces = 0, empty pieces and pieces shorter than ksize are fine.  The call runs the hashing
 *                       kernel of mvs_hash_set_from_sequences over the pieces -- a piece is laid out in units of option
 *                       kmer_unit exactly as a sample is there, options kmer_capacity and the second trip act per call -- and
 *                       appends the kept (value, sample) pairs to a staging list on the device that lives as long as the
 *                       sketcher and grows geometrically (by a device copy).  Synchronous: `bases` may be reused on return.
 *                       Refused, with nothing allocated and nothing appended: NULL where a pointer is needed, decreasing
 *                       offsets, a finished sketcher (MVS_E_INVALID); a sample index outside [0, n_samples) (MVS_E_RANGE).
 *                       NOT a clean refusal: a sample whose |M(s)| reaches 2^31 makes that add fail with MVS_E_RANGE after
 *                       its pairs were staged; the sketcher can then only be destroyed (every later add / finish:
 *                       MVS_E_INVALID).
 * mvs_kmer_sketcher_finish   the set described above (destroy it with mvs_hash_set_destroy; it outlives the sketcher) and, if
 *                       `histogram` is not NULL, the histogram.  The pairs are moved to their samples' ranges and handed to
 *                       the counted build below.  min_abundance = 0, 0 < max_abundance < min_abundance, NULL `set`: MVS_E_INVALID
 *                       and the sketcher stays as it was.  A second finish, or an add after it: MVS_E_INVALID.
 * mvs_kmer_sketcher_stats    per sample, n_samples HOST int64 each, any may be NULL: bytes given, valid positions, values kept
 *                       (= |M(s)|), and after finish the distinct values and those that passed the filter (0 before).
 * mvs_kmer_sketcher_info     what the sketcher's calls did so far, any pointer may be NULL: time of the hashing passes and of finish's
 *                       move into sample order (0 unless mvs_ctx_set_timing is on), pairs staged, pairs the list has room for (0
 *                       after finish), adds that hashed something, hashing passes repeated for more room, times the list grew.
 *                       The sketcher keeps these itself: mvs_ctx_kmer_stats stays what the last mvs_hash_set_from_sequences left.
 * mvs_kmer_sketcher_destroy  frees the staging list.  NULL is fine.
 * mvs_hash_set_create_counted
 *                       the counted build for hash lists: hashes / offsets as for mvs_hash_set_create (any order, duplicates
 *                       welcome), weights aligned with the hashes where `mem_weights` says, or NULL.  Refusals as for
 *                       mvs_hash_set_create plus the filter's.  How: a sort inside every sample -- samples of up to option
 *                       abund_big_segment values (default 262144, >= 64) in batches through the segmented radix sort, each
 *                       longer one by a device-wide radix sort of its own --, then four passes over units of option
 *                       abund_unit sorted values (default 4096, >= 64), one wave each, whose work depends neither on the
 *                       length of a sample nor on the length of a run of equal values: per-unit summaries, a segmented scan
 *                       of them, count + histogram, scan, fill.  Equal values on both sides of a sample border are two runs.
 *                       Neither option changes a result.  Synchronous.
 * mvs_hash_set_abundances    the abundances of a counted set, aligned with mvs_hash_set_export's values, where `mem_out` says.
 *                       MVS_E_INVALID for a set that carries none (made by mvs_hash_set_create / _from_sequences).  To
 *                       mvs_intersect_cells, mvs_gather, mvs_hash_set_export and mvs_hash_set_device a counted set is the
 *                       plain set it also is.  mvs_abund_overlap_cells ("abundance-weighted overlaps" below) reads them.
 * mvs_ctx_abund_stats   the context's last counted build: time of its sorts and of its run-sum passes (0 unless
 *                       mvs_ctx_set_timing is on), values given, distinct values, values that passed, units of the run-sum
 *                       passes, samples sorted device-wide.  Any pointer may be NULL. */
typedef struct mvs_kmer_sketcher mvs_kmer_sketcher;
int mvs_kmer_sketcher_create(mvs_ctx* ctx, int64_t n_samples, int ksize, uint32_t seed, uint64_t max_hash, mvs_kmer_sketcher** sketcher);
int mvs_kmer_sketcher_add(mvs_kmer_sketcher* sketcher, const uint8_t* bases, int mem_bases, const int64_t* offsets, const int32_t* samples,
                          int64_t n_pieces);
int mvs_kmer_sketcher_finish(mvs_kmer_sketcher* sketcher, uint32_t min_abundance, uint32_t max_abundance, int64_t* histogram,
                             mvs_hash_set** set);
int mvs_kmer_sketcher_stats(const mvs_kmer_sketcher* sketcher, int64_t* bases, int64_t* kmers, int64_t* kept, int64_t* distinct,
                            int64_t* passed);
int mvs_kmer_sketcher_info(const mvs_kmer_sketcher* sketcher, double* kernel_ms, int64_t* staged, int64_t* capacity, int64_t* adds,
                           int64_t* second_trips, int64_t* growths);
int mvs_kmer_sketcher_destroy(mvs_kmer_sketcher* sketcher);
int mvs_hash_set_create_counted(mvs_ctx* ctx, const uint64_t* hashes, int mem_hashes, const uint32_t* weights, int mem_weights,
                                const int64_t* offsets, int64_t n_samples, uint32_t min_abundance, uint32_t max_abundance,
                                int64_t* histogram, mvs_hash_set** set);
int mvs_hash_set_abundances(const mvs_hash_set* set, uint32_t* out, int mem_out);
int mvs_ctx_abund_stats(const mvs_ctx* ctx, double* sort_ms, double* count_ms, int64_t* values_in, int64_t* distinct, int64_t* passed,
                        int64_t* units, int64_t* big_segments);

/* ---- abundance-weighted overlaps for kept pairs -----------------------------------------------------------------------------
 * The measures people report for metagenomes weigh a shared k-mer by how often it was seen: Bray-Curtis, weighted Jaccard
 * (Ruzicka), the cosine of the abundance vectors with sourmash's angular similarity of it, abundance-weighted containment.
 * These calls compute their integer ingredients for a list of cells with the units of work, the searches and the exactness
 * of mvs_intersect_cells, and state the derived measures once, in host code.  The reference carries no abundances anywhere,
 * so nothing of it is replaced.
 *
 * For a hash set let a_s(h) be the abundance of value h in sample s: the carried uint32 of a counted set, and 1 FOR EVERY
 * VALUE OF A SET THAT CARRIES NONE -- a metagenome with counts against plain genome sketches is an ordinary call, and a call
 * on two plain sets reproduces mvs_intersect_cells in every field.  For a cell (row r of hs_rows, column c of hs_cols), with
 * M = H(r) n H(c):
 *     inter  = |M|
 *     w_row  = sum over M of a_r(h)                      w_col = sum over M of a_c(h)
 *     w_min  = sum over M of min(a_r(h), a_c(h))
 *     dot_lo = sum over M of (a_r(h) * a_c(h) mod 2^32)  dot_hi = sum over M of floor(a_r(h) * a_c(h) / 2^32)
 * The dot product of the two abundance vectors is dot_hi * 2^32 + dot_lo.  It is carried as two sums and not as one 64-bit
 * word so that NO FIELD CAN OVERFLOW: a sample holds fewer than 2^31 values and every term is below 2^32, so every sum is
 * below 2^63 -- a poly-A k-mer seen 10^7 times in both samples (one term of 10^14) stays an ordinary input, and so do 2^31 - 1
 * of them.  Exact and deterministic: integer sums do not depend on the unit size, the blocking, the order of the cells or of
 * the units.  Per-sample totals, with the same split:
 *     S(s) = sum of a_s(h)      Q_lo(s) = sum of (a_s(h)^2 mod 2^32)      Q_hi(s) = sum of floor(a_s(h)^2 / 2^32)
 * A cell with row == col on the same set yields w_row = w_col = w_min = S and dot = Q = Q_hi * 2^32 + Q_lo.
 *
 * mvs_abund_overlap_cells   the records of n_cells cells.  Arguments, refusals, hs_cols == NULL, repeated cells and device / host
 *                       memory exactly as for mvs_intersect_cells; `out` holds n_cells records where `mem_out` says.  A cell that
 *                       names a sample outside its set: MVS_E_RANGE, nothing is written for that cell, every other cell is
 *                       answered.  Synchronous.  Like mvs_gather it is also "the context's last mvs_intersect_cells" for
 *                       mvs_ctx_intersect_stats.  How: the plan, the units and the searches of mvs_intersect_cells (option
 *                       intersect_unit); the lane that finds its key knows the position on both sides, loads the two
 *                       abundances from global memory -- on a match only, no load at all for a side that carries none --,
 *                       and the wave adds its six sums to the cell's record with one 64-bit integer atomic per non-zero field.
 * mvs_hash_set_abundance_totals
 *                       S, Q_lo and Q_hi of every sample: n_samples uint64 each where `mem_out` says; any pointer may be NULL.
 *                       A set that carries no abundances: S = Q_lo = the sample's size, Q_hi = 0.  Synchronous.
 * mvs_abund_similarity  pure host, the library's own statement of the derived measures of one cell, from its record and the
 *                       totals of its row and column sample.  Every integer is converted to fp64 with round-to-nearest-even, a
 *                       128-bit value (D = dot, Q_row, Q_col) as a whole; then exactly these operations, 0 / 0 = NaN:
 *                         out[0] w_contain_row = w_row / S_row
 *                         out[1] w_contain_col = w_col / S_col
 *                         out[2] bray_curtis   = (S_row + S_col - 2 w_min) / (S_row + S_col)     the DISsimilarity; numerator and
 *                                                                                                 denominator formed as integers
 *                         out[3] ruzicka       = w_min / (S_row + S_col - w_min)                 denominator formed as an integer
 *                         out[4] cosine        = min(1, D / sqrt(Q_row * Q_col))                 one multiply, one sqrt, one divide
 *                         out[5] angular       = 1 - 2 acos(cosine) / pi                         sourmash's angular_similarity
 *                       size_row / size_col (the samples' numbers of values) enter no measure; they are checked with the
 *                       rest: a NULL pointer, a negative size or inter, inter above a size, w_min above S_row or S_col:
 *                       MVS_E_INVALID. */
typedef struct mvs_abund_overlap {
    int64_t inter;                                   /* never negative in an answered cell */
    uint64_t w_row, w_col, w_min, dot_lo, dot_hi;
} mvs_abund_overlap;                                 /* 48 bytes */
int mvs_abund_overlap_cells(mvs_ctx* ctx, const mvs_hash_set* hs_rows, const mvs_hash_set* hs_cols, const mvs_cell* cells,
                            int mem_cells, int64_t n_cells, mvs_abund_overlap* out, int mem_out);
int mvs_hash_set_abundance_totals(const mvs_hash_set* set, uint64_t* sum, uint64_t* sumsq_lo, uint64_t* sumsq_hi, int mem_out);
int mvs_abund_similarity(const mvs_abund_overlap* overlap, uint64_t sum_row, uint64_t sumsq_lo_row, uint64_t sumsq_hi_row,
                         int64_t size_row, uint64_t sum_col, uint64_t sumsq_lo_col, uint64_t sumsq_hi_col, int64_t size_col,
                         double out[6]);

/* ---- gather: the greedy decomposition of a query into samples of a hash set -------------------------------------------------
 * Everything above asks about a PAIR of samples.  This call answers the set question "which DB samples make up my sample, and
 * how much of it does each explain that the ones before it did not": the greedy minimum-set-cover walk (the rule of sourmash
 * `gather`).  The reference has no counterpart -- its search (src/jaccard.py) is pairwise --, so nothing of it is replaced.
 *
 * Q = H_query(query) (set semantics), H(c) the samples of hs_db, C the candidates (sample indices of hs_db; NULL: every sample;
 * duplicates are allowed and harmless), min_hashes >= 1, max_matches >= 0:
 *     R = Q;  orig[c] = |Q n H(c)|
 *     repeat:
 *         f[c] = |R n H(c)|  for c in C
 *         best = the c with the largest f[c]; ties go to the SMALLER sample index
 *         stop if C is empty, f[best] < min_hashes, or max_matches records are written
 *         R = R \ H(best)
 *         write (sample = best, intersect = orig[best], unique = f[best], remaining = |R|)
 * Exact and deterministic: equal to that walk on the sorted, de-duplicated lists whatever the options, the blocking, the order
 * or multiplicity of C, or whether the lists arrived sorted.  Hash values are arbitrary 64-bit words (0 and 2^64 - 1 are
 * ordinary values; no sentinel).  It follows that `unique` never rises from record to record, that the sum of `unique` plus the
 * last `remaining` is |Q|, that the first record has unique == intersect and that no sample is reported twice.  Derived
 * fractions (intersect / |Q|, intersect / |H|, unique / |Q|) are the caller's, in fp64.
 *
 * mvs_gather            the walk above.  candidates: n_candidates int32 where mem_candidates says (NULL: all of hs_db);
 *                       out: room for max_matches records where mem_out says; *n_matches: records written; *query_size: |Q|
 *                       (may be NULL; set whenever the query index is valid, max_matches == 0 included).  An empty query or an
 *                       empty candidate sample is ordinary: it matches nothing.  A query index or a candidate outside its set:
 *                       MVS_E_RANGE, nothing is written, *n_matches = 0.  min_hashes < 1, max_matches < 0, a NULL buffer that
 *                       is needed, a set of another context: MVS_E_INVALID.  Synchronous.
 *                       How: orig[] for all candidates comes from mvs_intersect_cells on the cells (query, c) -- which also
 *                       makes this the context's last mvs_intersect_cells --, and the candidates below min_hashes are retired
 *                       before anything is allocated for them (f only falls: they could never be written).  Every SURVIVOR gets
 *                       a bit row over the positions of Q's sorted list; a round is then one streaming pass over the live rows
 *                       (popcount(row & alive) per survivor, one 64-bit atomic max for the pick) and clears the winner's bits
 *                       from `alive`.  Rounds are queued option gather_batch at a time (default 16) with one small read-back
 *                       per batch and no host synchronisation in between; the option never changes a result.
 *                       Memory besides the sets: survivors x ceil(|Q| / 64) x 8 bytes of bit rows (10^6 hashes against 10^4
 *                       survivors: 1.25 GB) plus 16 bytes per candidate; where that does not fit the call returns MVS_E_NOMEM
 *                       and mvs_last_error names the byte count.
 * mvs_ctx_gather_stats  the context's last mvs_gather: survivors of the first phase, rounds run (the round that found nothing
 *                       included), batches (= read-backs), bytes of the bit rows, and the times of the three phases --
 *                       original overlaps, marking, rounds -- which are 0 unless mvs_ctx_set_timing is on.  Any pointer may
 *                       be NULL.
 * mvs_ctx_gather_round_bytes  what the rounds of that call streamed: live rows x ceil(|Q| / 64) x 8 bytes, summed over the
 *                       rounds (a measurement divides it by rounds_ms).  The kernels are in csrc/mvs_gather.hip. */
typedef struct {
    int32_t sample, intersect, unique, remaining;
} mvs_gather_match;
int mvs_gather(mvs_ctx* ctx, const mvs_hash_set* hs_query, int64_t query, const mvs_hash_set* hs_db, const int32_t* candidates,
               int mem_candidates, int64_t n_candidates, int32_t min_hashes, int64_t max_matches, mvs_gather_match* out, int mem_out,
               int64_t* n_matches, int32_t* query_size);
int mvs_ctx_gather_stats(const mvs_ctx* ctx, int64_t* survivors, int64_t* rounds, int64_t* batches, int64_t* row_bytes,
                         double* overlap_ms, double* mark_ms, double* rounds_ms);
int mvs_ctx_gather_round_bytes(const mvs_ctx* ctx, int64_t* bytes);

/* ---- block plans: one rank's share of the symmetric multi-rank schedule, compared in few launches ----------------
 * The reference shards by rows and lets every shard process compute its rows against ALL columns
 * (src/pairwise_comp_optimized.cpp:937-982); dot, keep test and quantised Jaccard are symmetric in (row, col), so with G
 * ranks every unordered pair of row blocks needs comparing only once (metagenome_vector_sketches_amd/parallel.py:
 * block_plan).  A rank's share -- its diagonal block under the symmetric schedule plus G/2 off-diagonal blocks whose kept
 * cells are mirrored -- is handed over as rectangles and runs as ONE two-stage comparison: the filter in as few launches
 * as the caller wants (one per group of rectangles whose columns have arrived: the blocks of a peer can be launched as soon
 * as that peer's rows have landed, while the rest of the exchange is still on the wire), then one re-check, one launch of
 * the exact kernel on the flagged tiles.  One host synchronisation, in mvs_plan_finish.
 *
 * STORAGE coordinates.  Plans work on a set whose rows are laid out in per-rank blocks of `block_rows_padded` rows
 * (mvs_shard_layout: the shard size ceil(N / G) of :938-940 rounded up to a multiple of 256, so that every block starts on
 * the tile grid and on the 16-row grid of the fragment-major planes; the rows behind a shard's last sample are zero
 * sketches with zero norms).  Kept cells come out in storage coordinates; mvs_cells_route turns them into sample indices
 * and drops anything that touches a padding row.
 *
 * mvs_sketch_set_attach_derived : the filter's inputs for this set -- the fragment-major coarse plane (n_alloc * d_pad
 *     bytes) and 16 bytes of statistics per row -- live in CALLER buffers from now on: the caller fills them for its own
 *     rows with mvs_sketch_set_prepare_rows and for the other ranks' rows by gathering those ranks' (mvs_allgather_rows on
 *     the coarse plane in units of 16 rows, mvs_allgather_bytes on the statistics), instead of every rank rebuilding them
 *     for all N rows from the gathered limb planes.  Two-limb sets only (others: the calls succeed and plans run the exact
 *     kernel block by block).
 * mvs_sketch_set_prepare_rows   : coarse plane + statistics of rows [row_first, row_first + row_count) from the limb planes
 *     (row_first and row_count multiples of 16).  Asynchronous.
 * mvs_plan_begin  : frame = the rank's own row block [frame_row_begin, frame_row_end) (multiples of 256) x all columns;
 *     the symmetric schedule applies inside the frame's square; MVS_PLAN_MIRROR_OUTSIDE mirrors every kept cell outside it.
 *     norms_sq and cells are DEVICE buffers (norms indexed by storage row); cells are appended from index 0, unsorted.
 * mvs_plan_filter : the filter over these rectangles (rows inside the frame; bounds on multiples of 256 or at the set's
 *     end) as one launch.  Asynchronous: the caller orders it behind the arrival of the columns it reads.
 * mvs_plan_finish : re-check + flagged tiles.  *d_count = DEVICE address of the running cell count (it may exceed the
 *     capacity: cells beyond it were dropped, compare after reading it back).  Synchronises once in the middle.
 *
 * Option plan_speculate = 1 (off by default; set it around mvs_plan_begin, where the decision is taken): a plan with the
 *     same frame, set geometry, keep mode and capacity as the previous plan of this context sizes its second half --
 *     candidate pruning, re-check, the launch on the flagged tiles -- from THAT plan's counts and mvs_plan_finish does not
 *     synchronise at all: the kernels read the real counts on the device, and a last kernel checks that the sizes held.  If
 *     they did not (more flagged tiles than twice the previous count + 64, a candidate list beyond its buffer), the cell
 *     count reads MVS_PLAN_STALE or more: discard the cells and run the same plan again -- it will not speculate.  The
 *     counts reach the host with the caller's next read-back (mvs_cells_report brings them along; mvs_plan_stats and the
 *     next mvs_plan_begin wait for them if nobody has).  A steady multi-rank step thus has ONE host synchronisation. */
#define MVS_PLAN_MIRROR_OUTSIDE 1
#define MVS_PLAN_STALE (1ULL << 62)
typedef struct {
    int64_t row_begin, row_end, col_begin, col_end;
} mvs_plan_block;
int mvs_shard_layout(int64_t n_total, int world, int64_t* block_rows, int64_t* block_rows_padded);
int mvs_sketch_set_attach_derived(mvs_sketch_set* set, int8_t* coarse_fm, void* row_stats);
int mvs_sketch_set_prepare_rows(mvs_ctx* ctx, mvs_sketch_set* set, int64_t row_first, int64_t row_count);
/* mvs_limb_split + mvs_sketch_set_prepare_rows in ONE pass over the sketches (k_recode_rows): rows [row_first, row_first +
 * n_rows) of the set's planes and derived data from `sketches` (DEVICE, n_rows x d, elem_bytes 4 or 2), the remaining rows up to
 * row_first + row_count as zero rows (their planes must be zero already).  WRITES the plane buffer the set was made from
 * (mvs_sketch_set_from_planes).  Two-limb sets of d_pad <= 4096 with derived data attached; anything else takes the separate
 * passes, same result.  Asynchronous. */
int mvs_sketch_set_recode_rows(mvs_ctx* ctx, mvs_sketch_set* set, const void* sketches, int elem_bytes, int64_t n_rows,
                               int64_t row_first, int64_t row_count);
/* The exchange without the high limb.  The coarse plane c, its radix m (in the row statistics) and the LOW limb of a row pin
 * the row's values (v is the one value congruent to the low limb mod 256 near m * c: the radix search only admits radices for
 * which that holds, csrc/mvs_pairwise.hip "The high limb on the wire"), so ranks exchange 2 bytes per entry -- coarse plane
 * and low limbs -- instead of 3 and rebuild the other ranks' limb planes here: rows [row_first, row_first + row_count)
 * (multiples of 16) of the set's plane buffer from lo_wire[row * d_pad + k] (DEVICE; indexed like the set's rows) and the
 * attached coarse plane / statistics of those rows.  Valid for rows whose radix is <= MVS_WIRE_RADIX_MAX, i.e. max|v| <=
 * MVS_WIRE_MAX_ABS: the caller checks the largest |v| of all ranks (it travels in the cells header) and falls back to
 * exchanging the limb planes otherwise.  Asynchronous. */
#define MVS_WIRE_RADIX_MAX 252
#define MVS_WIRE_MAX_ABS 32004
int mvs_sketch_set_planes_from_wire(mvs_ctx* ctx, mvs_sketch_set* set, const int8_t* lo_wire, int64_t row_first, int64_t row_count);
/* The sender's side of that exchange: the LOW limbs of rows [row_first, row_first + row_count) of a two-limb set's planes into
 * lo_wire[row * d_pad + k] (DEVICE, indexed like the set's rows) -- a rank calls it for its own row block before the all-gather
 * of the wire buffer.  Asynchronous. */
int mvs_sketch_set_wire_rows(mvs_ctx* ctx, const mvs_sketch_set* set, int8_t* lo_wire, int64_t row_first, int64_t row_count);
/* The same for a plan, ROW BY ROW AS NEEDED: after mvs_plan_wire, mvs_plan_finish rebuilds -- between gathering the candidates
 * and the re-check -- exactly the rows outside the frame that its second half reads (the columns of the candidates and of the
 * flagged tiles; lo_wire as above, valid until the plan has finished).  A plan whose filter leaves few candidates touches few
 * rows; the others' limb planes keep whatever an earlier step left there.  Plans with a filter only (others read every row of
 * their blocks: mvs_sketch_set_planes_from_wire before mvs_plan_filter). */
int mvs_plan_wire(mvs_ctx* ctx, const int8_t* lo_wire);
/* The caller announces that the row statistics (mvs_sketch_set_attach_derived) and squared norms of rows [row_begin, row_end) are
 * in place on the context's stream -- in a multi-rank step: the small exchange has been joined.  The plan derives the filter's
 * per-row constants of those rows in ONE launch (the part of the range inside the frame is skipped: derived at mvs_plan_begin),
 * and mvs_plan_filter no longer derives them block by block (eight 4-us launches per step of an 8-way split).  Optional: blocks
 * whose columns were never announced are handled as before.  Replaces nothing of the reference by itself -- part of the tile
 * loop's set-up (src/pairwise_comp_optimized.cpp:949-958: norms of the column tile). */
int mvs_plan_rows_ready(mvs_ctx* ctx, int64_t row_begin, int64_t row_end);
int mvs_plan_begin(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int keep_mode, int64_t frame_row_begin,
                   int64_t frame_row_end, int flags, mvs_cell* cells, int64_t capacity);
int mvs_plan_filter(mvs_ctx* ctx, const mvs_plan_block* blocks, int n_blocks);
int mvs_plan_finish(mvs_ctx* ctx, const uint64_t** d_count);
/* What the last plan did.  ms (timing enabled, else zeros): [0] the time during which a filter launch of the plan was running
 * (with option plan_overlap = 1 consecutive launches alternate between the context's stream and a side stream and overlap), [1] re-check (candidate gather,
 * pruning, k_exact_pairs), [2] exact kernel on the flagged tiles, [3] first filter launch .. end of the plan on the stream.
 * counts: [0] candidates, [1] flagged tiles, [2] 256 x 256 filter tiles computed, [3] filter launches, [4] bit 0: the plan ran
 * the exact kernel block by block (no filter), bit 1: it ran ahead of its read-backs (plan_speculate), bit 2: and its sizes
 * did not hold (MVS_PLAN_STALE), [5] d_pad.  Call after the stream has drained. */
int mvs_plan_stats(mvs_ctx* ctx, double ms[4], int64_t counts[6]);

/* Kept cells of a plan -> this rank's shard.  A cell of the plan is in storage coordinates and, under the symmetric
 * multi-rank schedule, about half of them are mirror images that belong to OTHER ranks' rows.
 * d_own_count (DEVICE) is the shard's state block of 16 + 4 * (own_end - own_begin + 1) bytes: u64 cells of own rows, u32 largest
 *     number of cells in one row (valid after mvs_cells_report), u32 unused, then one u32 per own row: its cells.
 * mvs_cells_route   : cells [0, min(*d_n_raw, raw_capacity)) -> sample indices (row = block * block_rows + offset for offset <
 *     block_rows; cells touching a padding row or a row >= n_total are dropped); those of rows [own_begin, own_end) are
 *     appended to own_out (state block zeroed by this call, then counted into), the others to `send` = a 64-byte header
 *     {foreign cells (may exceed the capacity), status, max_abs, *d_n_raw, raw_capacity, ...} followed by foreign_capacity
 *     cells.  status / max_abs travel in the header so that one exchange tells every rank how every other rank fared.
 * mvs_cells_collect : `recv` = world such buffers (after an all-gather of the send buffers): the cells of rows
 *     [own_begin, own_end) in the other ranks' buffers are appended to own_out.
 * mvs_cells_report  : read back -- out[0] = cells of own rows, then per rank {foreign cells, status, max_abs, raw cells,
 *     raw capacity} (5 * world values), then out[1 + 5 * world] = the largest number of cells in one own row.  Synchronous; the
 *     others are asynchronous.
 * mvs_cells_sort_rows : own_out -> (row, col) order by row buckets -- the rows' counts are in the state block: scan, scatter
 *     into the rows' segments, one wave per row orders its cells by column.  For shards whose rows hold at most 64 cells (what
 *     the report says); anything else: mvs_cells_sort. */
int mvs_cells_route(mvs_ctx* ctx, const mvs_cell* raw, const uint64_t* d_n_raw, int64_t raw_capacity, int64_t block_rows_padded,
                    int64_t block_rows, int64_t n_total, int64_t own_begin, int64_t own_end, mvs_cell* own_out,
                    int64_t own_capacity, uint64_t* d_own_count, void* send, int64_t foreign_capacity, int64_t status,
                    int64_t max_abs);
int mvs_cells_collect(mvs_ctx* ctx, const void* recv, int world, int rank, int64_t foreign_capacity, int64_t own_begin,
                      int64_t own_end, mvs_cell* own_out, int64_t own_capacity, uint64_t* d_own_count);
int mvs_cells_report(mvs_ctx* ctx, const void* recv, int world, int64_t foreign_capacity, int64_t own_rows, uint64_t* d_own_count,
                     int64_t* out);
int mvs_cells_sort_rows(mvs_ctx* ctx, const mvs_cell* cells_in, int64_t n, int64_t own_begin, int64_t own_end,
                        const uint64_t* d_own_count, mvs_cell* cells_out);
/* mvs_cells_sort_rows queued IN FRONT of mvs_cells_report's read-back: the number of cells is the one in the state block (at
 * most in_capacity of them are in cells_in), cells whose place lies beyond out_capacity are dropped.  For a caller that knows
 * from its previous step that no row holds more than 64 cells and that the buffers suffice; what the report then says -- cell
 * count, largest row -- tells it whether that held (if not: sort again with what the report says).  Asynchronous. */
int mvs_cells_sort_rows_ahead(mvs_ctx* ctx, const mvs_cell* cells_in, int64_t in_capacity, int64_t own_begin, int64_t own_end,
                              const uint64_t* d_own_count, mvs_cell* cells_out, int64_t out_capacity);
#define MVS_CELLS_HEADER_BYTES 64

/* A shard's kept cells -> the writer.  `cells` (DEVICE) holds n_cells cells ordered by (row, col) -- what a step leaves behind
 * (mvs_cells_sort_rows / mvs_cells_sort) --, rows [row_begin, row_end) of them are delivered exactly as mvs_pairwise_stream /
 * mvs_pairwise_stream_encoded deliver their result: CSR pieces of whole rows in ascending order, or the rows' finished shard
 * records, through the same callbacks under the same rules (pinned buffers of the library, a worker thread, a non-zero return
 * aborts).  A process that owns several shards (src/pairwise_comp_optimized.cpp:937-940: one row range each) compares the union
 * of their rows ONCE and calls this per shard folder with that shard's row range; cells outside the range are skipped.
 * The contract the kernels rely on (they index by these values, nothing checks them): the cells are ordered by (row, col) with
 * the columns strictly ascending inside a row, 0 <= col < 2^31 and 0 <= q <= 65535 (q is kept in 16 bits and truncated).
 * *n_delivered (optional): the cells handed over.  Synchronous.  Writer loop replaced: src/pairwise_comp_optimized.cpp:700-790. */
int mvs_cells_stream(mvs_ctx* ctx, const mvs_cell* cells, int64_t n_cells, int64_t row_begin, int64_t row_end,
                     mvs_row_block_cb cb, void* user, int64_t* n_delivered);
int mvs_cells_stream_encoded(mvs_ctx* ctx, const mvs_cell* cells, int64_t n_cells, int64_t row_begin, int64_t row_end,
                             mvs_encoded_rows_cb cb, void* user, int64_t* n_delivered);

/* Sort n cells by (row, col) from one DEVICE buffer into another (asynchronous on the context's stream). */
int mvs_cells_sort(mvs_ctx* ctx, const mvs_cell* cells_in, int64_t n, mvs_cell* cells_out);

/* Dense int32 dot products of rows [r0,r1) x cols [c0,c1) (row-major, leading dimension c1-c0):
 * the bare `block_i.transpose() * block_j` of src/pairwise_comp_optimized.cpp:135.  For validation
 * and small problems.  `algo` 0 = matrix-core path, 1 = plain vector-ALU path (independent check). */
int mvs_pairwise_dots(mvs_ctx* ctx, const mvs_sketch_set* set, int64_t r0, int64_t r1, int64_t c0,
                      int64_t c1, int32_t* out, int mem_out, int algo);

/* ---- ordination: exact moments over the sample axis, PCA -------------------------------------------------------
 * What the reference's src/clusters.py does with scikit-learn on a dense float copy of vectors.bin: a PCA of the samples whose
 * norm is at least 10, and the projection of a second, larger set (big_vectors.bin) onto its axes.  Here the part of a PCA that
 * matters is exact: the Gram matrix over the SAMPLE axis, bit for bit, from the resident limb planes.
 *
 * x[i][a] is the integer a set's limbs encode: sum_l limb_l * 256^l (MVS_LIMBS_K3: l0 + 128 * l1); 0 <= a < d.
 *
 * mvs_sketch_moments  n = row_end - row_begin >= 1:
 *                         col_sums[a]     = sum_i x[i][a]                 int64 [d]
 *                         gram[a * d + b] = sum_i x[i][a] * x[i][b]       int64 [d * d], the full symmetric matrix, row-major
 *                     over the rows of [row_begin, row_end) only; exact for every limb code, any d and any range: padding rows,
 *                     padding columns and rows outside the range contribute nothing.  Both outputs live where mem_out says.
 *                     With B the largest magnitude the limb code holds (127, 32 639, 2^23, 2^31; MVS_LIMBS_K3: 8 127), a call
 *                     with n * B^2 > 2^62 returns MVS_E_RANGE before any launch.  n < 1, a range outside the set, a NULL
 *                     output: MVS_E_INVALID.  Option gram_slab_rows bounds the scratch copy (slab rows x limbs x d bytes).
 * mvs_pca_fit         n >= 2, 1 <= components <= min(64, d), 0 <= tol < 1, max_iters >= 1 (else MVS_E_INVALID; the range rule
 *                     of the moments applies).  From the moments, on the host, each numerator formed exactly in 128-bit
 *                     integers, converted with one rounding and divided once:
 *                         mean[a] = (double)col_sums[a] / (double)n
 *                         C[a][b] = (double)(n * gram[a][b] - col_sums[a] * col_sums[b]) / ((double)n * (double)(n - 1))
 *                         total_variance = sum_a C[a][a]
 *                     The leading eigenpairs of C by block subspace iteration with a Rayleigh-Ritz step (block of
 *                     min(d, components + 8) columns; the d x d x block products and the residuals on the device, in fp64; the
 *                     block's orthonormalisation and the small symmetric eigenproblem, by cyclic Jacobi, on the host; no
 *                     library beyond what libmvs_hip.so links anyway).  It stops when max_i ||C v_i - lambda_i v_i||_2 <=
 *                     tol * lambda_1 over the components, or after max_iters iterations.  Not converging is not an error: the
 *                     call returns MVS_OK with converged = 0, the iterations used and every component's residual.  lambda comes
 *                     back descending; every axis has unit length and is signed so that its entry of largest magnitude (the
 *                     smaller index on ties) is positive.  Deterministic bit for bit from run to run: the start block is a
 *                     fixed function of (row, column) through splitmix64, nothing uses floating-point atomics, every reduction
 *                     order is fixed.  1e-10 and 300 are the defaults of the Python binding and of pca_sketches.
 * mvs_pca_info        any pointer may be NULL.
 * mvs_pca_get         HOST arrays, any may be NULL: mean[d], axes[components * d] (axis j at j * d), variances[components]
 *                     (lambda), residuals[components] (||C v - lambda v||_2 of the returned pair).
 * mvs_pca_transform   scores[(i - row_begin) * components + j] = sum_a (x[i][a] - mean[a]) * axes[j][a] in fp64, for the rows
 *                     of ANY set of the same d on the same context (the fitted one, or another DB); evaluated as
 *                     sum_a x V - sum_a mean V.  scores lives where mem_out says.  Another d: MVS_E_INVALID.
 * mvs_ctx_pca_stats   of the context's last mvs_sketch_moments / mvs_pca_fit (gram_ms, slabs), mvs_pca_fit (eigen_ms: the
 *                     solver from its first product to its last residual, iterations) and mvs_pca_transform (scores_ms); the
 *                     times are 0 unless mvs_ctx_set_timing is on.  Any pointer may be NULL.
 * All synchronous.  The kernels are in csrc/mvs_gram.hip. */
typedef struct mvs_pca mvs_pca;
int mvs_sketch_moments(mvs_ctx* ctx, const mvs_sketch_set* set, int64_t row_begin, int64_t row_end, int64_t* gram,
                       int64_t* col_sums, int mem_out);
int mvs_pca_fit(mvs_ctx* ctx, const mvs_sketch_set* set, int64_t row_begin, int64_t row_end, int components, double tol,
                int max_iters, mvs_pca** pca);
int mvs_pca_info(const mvs_pca* pca, int* d, int* components, int64_t* n, int* iterations, int* converged, double* total_variance);
int mvs_pca_get(const mvs_pca* pca, double* mean, double* axes, double* variances, double* residuals);
int mvs_pca_transform(mvs_ctx* ctx, const mvs_pca* pca, const mvs_sketch_set* set, int64_t row_begin, int64_t row_end,
                      double* scores, int mem_out);
int mvs_pca_destroy(mvs_pca* pca);
int mvs_ctx_pca_stats(const mvs_ctx* ctx, double* gram_ms, double* eigen_ms, double* scores_ms, int64_t* slabs, int64_t* iterations);

/* ---- principal coordinates of the Jaccard estimates, matrix-free --------------------------------------
 * Every other analysis here judges two samples by their Jaccard estimate; this is the ordination in that geometry: classical
 * PCoA of the distance sqrt(1 - k).  The n x n matrix it is defined on is never stored: the dense-dots kernels produce a block
 * of rows, one kernel turns the block into Jaccard values and multiplies them into a thin block of vectors in the same pass.
 *
 * The rule.  n2 = norms_sq, d the set's dimension, 0 <= floor < 1; row i, column j by sample index; P the int32 dot as
 * mvs_pairwise_dots returns it (wrapped).  Everything is fp64 and every line is ONE rounding; a NaN compares false:
 *     i == j : k(i,j) = 1.0
 *     i != j : inter = (double)P / (double)d
 *              s     = n2[i] + n2[j]
 *              den   = s - inter
 *              J     = inter / den
 *              k(i,j) = !(J > floor) ? 0.0 : (J > 1.0 ? 1.0 : J)
 * -- the score of mvs_pairwise_topk with the writer's clamp.  k is symmetric bit for bit (n2[i] + n2[j] commutes) and defined
 * for any norms: NaN, +-inf, 0, negative.
 *
 * mvs_jaccard_apply   Y[(i - row_begin) * b + c] = sum over j in [col_begin, col_end) of k(i,j) * X[(j - col_begin) * b + c]
 *                     X: (col_end - col_begin) x b doubles, row-major (`mem_x`); Y: (row_end - row_begin) x b (`mem_y`);
 *                     1 <= b <= 128.  fp64 on the matrix cores, no floating-point atomics; the order of every sum is a fixed
 *                     function of the column range and of b only, so Y is bit-identical from run to run AND for every row
 *                     blocking (option pcoa_block_rows, or the caller's own splitting of the row range).  Against the exact
 *                     sum every entry is within (C + 4) 2^-53 sum_j |k| |X|, C the number of columns.  Rows go in blocks sized as
 *                     mvs_pairwise_levels sizes them; per block one dense-dots launch (option pcoa_dots = 1: on the vector
 *                     ALUs) and one apply launch; device memory besides the set is the dots block plus O((rows + cols) x b),
 *                     never N x N.  An empty row range returns MVS_OK and writes nothing; an empty column range gives Y = 0.
 *                     MVS_E_INVALID: floor outside [0, 1) or NaN, b outside 1 .. 128, ranges outside the set, a NULL buffer
 *                     that is needed.
 * mvs_pcoa_fit        F = [row_begin, row_end), m = its size >= 2, 1 <= components <= min(64, m - 1), 0 <= tol < 1,
 *                     max_iters >= 1 (else MVS_E_INVALID).  K = k on F x F, H = I - 11^T / m, B = 1/2 H K H: classical PCoA,
 *                     -1/2 H (D o D) H with D o D = 1 - K, the constant removed by the centring.  One apply against a column of
 *                     ones gives
 *                         rowmean[i] = (sum_j k(i,j)) / m,  grand = (sum_i rowmean[i]) / m,  trace = 1/2 m (1 - grand)
 *                     (the host sums in index order).  The leading eigenpairs of B come from the solver of mvs_pca_fit: block
 *                     min(m, components + 8), the same splitmix64 start block, orthonormalisation, Jacobi and Ritz step; B Q is
 *                     formed as: centre Q's columns (host), mvs_jaccard_apply's passes (device), centre the result and halve it
 *                     (host).  It stops at max_i ||B v_i - lambda_i v_i||_2 <= tol * lambda_1 or after max_iters; not
 *                     converging is not an error (converged = 0, the iterations used and the residuals come back).  lambda
 *                     descends by value; vectors have unit length and are signed as the PCA axes are;
 *                     coordinates[i][c] = sqrt(max(lambda_c, 0)) * v[i][c].  Deterministic bit for bit.
 *                     An estimated kernel need not be positive semi-definite, and the iteration finds the eigenvalues of
 *                     largest MAGNITUDE: a returned pair is always a verified eigenpair -- its residual is returned -- but it
 *                     is the top pair by value only where the top of the spectrum dominates the negative end.  negative_ritz
 *                     counts the negative Ritz values of the final block.
 * mvs_pcoa_info       any pointer may be NULL.
 * mvs_pcoa_get        HOST arrays, any may be NULL: eigenvalues[components], vectors[m * components] and
 *                     coordinates[m * components] (row-major, sample i at i * components), row_means[m], residuals[components].
 * mvs_pcoa_transform  Gower's out-of-sample formula for rows [row_begin, row_end) of the SAME set handle (the fitted rows
 *                     where they were, new samples appended behind them; `norms_sq` covers the whole set):
 *                         score[x][c] = lambda_c > 0 ? (1/2 sum_{j in F} (k(x,j) - rowmean[j]) v[j][c]) / sqrt(lambda_c) : 0
 *                     one apply over rows x F, evaluated as sum k v - sum rowmean v.  A fitted row reproduces its coordinate up
 *                     to the pair's residual / sqrt(lambda).  Another set handle: MVS_E_INVALID.
 * mvs_ctx_pcoa_stats  of the context's last call of this section: dense-dots and apply kernel times summed over passes and row
 *                     blocks, the solver from its first product to its last residual (host work included), passes over K, row
 *                     blocks, rows per block; the times are 0 unless mvs_ctx_set_timing is on.  Any pointer may be NULL.
 * All synchronous.  The kernel is in csrc/mvs_kapply.hip. */
typedef struct mvs_pcoa mvs_pcoa;
int mvs_jaccard_apply(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double floor,
                      int64_t row_begin, int64_t row_end, int64_t col_begin, int64_t col_end, const double* X, int b, int mem_x,
                      double* Y, int mem_y);
int mvs_pcoa_fit(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, int64_t row_begin,
                 int64_t row_end, int components, double floor, double tol, int max_iters, mvs_pcoa** pcoa);
int mvs_pcoa_info(const mvs_pcoa* pcoa, int64_t* row_begin, int64_t* row_end, int* components, int* block, int* iterations,
                  int* converged, int* negative_ritz, double* floor, double* grand_mean, double* trace);
int mvs_pcoa_get(const mvs_pcoa* pcoa, double* eigenvalues, double* vectors, double* coordinates, double* row_means,
                 double* residuals);
int mvs_pcoa_transform(mvs_ctx* ctx, const mvs_pcoa* pcoa, const mvs_sketch_set* set, const double* norms_sq, int mem_norms,
                       int64_t row_begin, int64_t row_end, double* scores, int mem_out);
int mvs_pcoa_destroy(mvs_pcoa* pcoa);
int mvs_ctx_pcoa_stats(const mvs_ctx* ctx, double* dots_ms, double* apply_ms, double* eigen_ms, int64_t* passes,
                       int64_t* row_blocks, int64_t* block_rows);

/* ---- PERMANOVA on the Jaccard estimates, matrix-free ---------------------------------------------------
 * Do labelled groups of samples differ in the geometry of the section above, the distance sqrt(1 - k)?  PERMANOVA (Anderson
 * 2001; adonis2, scikit-bio's permanova) answers with a pseudo-F from within-group and total sums of squared distances and a
 * p-value from relabelling the samples.  The n x n matrix it is defined on is never stored: the dense-dots kernels produce a
 * block of rows, one kernel turns it into fixed-point squared distances, one folds those into per-group sums for MANY
 * labellings at once -- the matrix is produced once and the permutations ride along.
 *
 * The weight of a cell.  k(i,j) is the rule of "principal coordinates" above, word for word (unit diagonal, floor, any norms).
 * Then, fp64, ONE rounding per line:
 *     t      = 1.0 - k(i,j)
 *     w(i,j) = (uint32) rint(t * 1073741824.0)             2^30; 0 on the diagonal, 2^30 for k = 0
 * w is symmetric bit for bit because k is.  Every sum of w is an INTEGER: sums do not depend on order, blocking or atomics,
 * and two labellings that induce the same partition get EQUAL statistics -- what a permutation p-value needs, F_perm >= F_obs
 * must hold for a tie.  The resolution of d^2 is 2^-30 = 9.3e-10, far below the estimator's own error (about 1 / sqrt(d)).
 *
 * mvs_group_sums      F = [row_begin, row_end) of a resident set, m = |F|; labels: HOST bytes labels[s * m + (i - row_begin)],
 *                     `slots` labellings, every value < groups; 1 <= groups <= 255; 1 <= slots <= MVS_MAX_GROUP_SLOTS.
 *                         sizes[s * groups + g]  = #{i in F : labels[s][i] = g}
 *                         S[s][g]                = sum over unordered pairs {i, j} of F, i < j, labels[s][i] = labels[s][j] = g, of w(i,j)
 *                     S is returned as 128-bit integers, sums_hi[s * groups + g] * 2^64 + sums_lo[s * groups + g] (HOST uint64
 *                     arrays; sums_hi and sizes may be NULL).  Rows go in blocks sized as mvs_pairwise_levels sizes them
 *                     (options groups_block_rows, groups_dots as pcoa_*); per block one dense-dots launch, the quantising
 *                     kernel and the summing kernel.  Device memory besides the set: the dots block, slots x m bytes of labels
 *                     twice (as given and sample-major) and slots x groups accumulators -- never n x n.
 *                     No sum wraps: a block's partial per (slot, group) is at most block_rows * m * 2^30, so the block rows
 *                     are clamped to block_rows * m < 2^34 and the blocks are added on the host in 128 bits; m > 2^31 - 1 is
 *                     refused (MVS_E_INVALID).  The kernels sum over ORDERED pairs and the host halves: an odd ordered-pair
 *                     sum is a broken invariant and returns MVS_E_INTERNAL.  An empty row range: MVS_OK, zero sums and sizes.
 *                     MVS_E_INVALID: a label >= groups, groups outside 1 .. 255, slots outside 1 .. MVS_MAX_GROUP_SLOTS,
 *                     floor outside [0, 1) or NaN, a range outside the set, a NULL buffer that is needed.
 * mvs_permutation_labels  pure host.  out[(permutations + 1) * m]: slot 0 is `labels`; slot p >= 1 is a Fisher-Yates shuffle
 *                     of it.  With mix(x): x += 0x9e3779b97f4a7c15; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9;
 *                     x = (x ^ (x >> 27)) * 0x94d049bb133111eb; return x ^ (x >> 31)  (uint64 arithmetic, splitmix64):
 *                         state = mix(seed ^ mix(p))
 *                         for i = m - 1 down to 1:  r = mix(state) % (i + 1);  state += 0x9e3779b97f4a7c15;  swap(out[i], out[r])
 *                     (the bias of `%` is at most (i + 1) / 2^64 and accepted).  m >= 0, permutations >= 0.
 * mvs_permanova_stats pure host: from the sums and sizes of slots = permutations + 2 labellings -- slot 0 observed, slots
 *                     1 .. permutations relabelled, the LAST slot all zeros (its group 0 holds S_all) -- to the numbers.  All
 *                     fp64, each line one rounding:
 *                         term_g     = (double)S_g / (double)n_g            for n_g > 0   (128 bits -> double, to nearest even)
 *                         ss_within  = (sum of the term_g taken in ASCENDING order of value) * 2^-30
 *                         ss_total   = ((double)S_all / (double)m) * 2^-30
 *                         ss_between = ss_total - ss_within
 *                         F          = (ss_between / (G - 1)) / (ss_within / (m - G))     G = non-empty groups of slot 0
 *                         R2         = ss_between / ss_total
 *                         p_value    = (1 + #{p >= 1 : ss_within(p) <= ss_within(0)}) / (permutations + 1)
 *                     The ascending order makes equal multisets of (S_g, n_g) give equal doubles: swapping the ids of two
 *                     groups ties.  The p-value compares ss_within, equivalent to F_p >= F_0 because ss_total is shared,
 *                     which sidesteps ss_within = 0 (there F is +inf or NaN as IEEE gives it).  group_mean_d2[g] (NULL: not
 *                     wanted) = ((double)S_g / (double)(n_g (n_g - 1) / 2)) * 2^-30 of slot 0, 0 for n_g < 2; perm_f[p - 1]
 *                     (NULL: not wanted) is the F of slot p.  MVS_E_INVALID: G < 2 or G >= m, sizes of slot 0 that do not add
 *                     up to m, permutations < 0, groups outside 1 .. 255, a NULL buffer that is needed.
 * mvs_permanova       generates the labellings (mvs_permutation_labels), appends the all-zero slot, calls mvs_group_sums and
 *                     mvs_permanova_stats.  labels: m HOST bytes < groups; 0 <= permutations <= MVS_MAX_GROUP_SLOTS - 2 (0 gives
 *                     p_value = 1).  group_sizes[groups], group_mean_d2[groups], perm_f[permutations]: HOST, any may be NULL.
 *                     G < 2 or G >= m is refused before any launch.
 * mvs_ctx_groups_stats  of the context's last mvs_group_sums / mvs_permanova: kernel times of the dots, the quantising and the
 *                     summing summed over the row blocks (0 unless mvs_ctx_set_timing is on), row blocks, rows per block,
 *                     slots.  Any pointer may be NULL.
 * All synchronous.  The kernels are in csrc/mvs_groups.hip. */
#define MVS_MAX_GROUP_SLOTS 16384
typedef struct {
    double f, r2, p_value, ss_total, ss_within, ss_between;
    int64_t df_between, df_within, samples, groups, permutations;   /* groups: the non-empty ones, G */
} mvs_permanova_result;
int mvs_group_sums(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double floor, int64_t row_begin,
                   int64_t row_end, const uint8_t* labels, int64_t slots, int groups, uint64_t* sums_lo, uint64_t* sums_hi,
                   int64_t* sizes);
int mvs_permutation_labels(const uint8_t* labels, int64_t m, int64_t permutations, uint64_t seed, uint8_t* out);
int mvs_permanova_stats(const uint64_t* sums_lo, const uint64_t* sums_hi, const int64_t* sizes, int64_t permutations, int groups,
                        int64_t m, mvs_permanova_result* result, double* group_mean_d2, double* perm_f);
int mvs_permanova(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double floor, int64_t row_begin,
                  int64_t row_end, const uint8_t* labels, int groups, int64_t permutations, uint64_t seed,
                  mvs_permanova_result* result, int64_t* group_sizes, double* group_mean_d2, double* perm_f);
int mvs_ctx_groups_stats(const mvs_ctx* ctx, double* dots_ms, double* quantise_ms, double* sums_ms, int64_t* row_blocks,
                         int64_t* block_rows, int64_t* slots);

/* ---- Labelling quality: silhouette, nearest group, medoids and dispersion, matrix-free ---------------------
 * Five calls here write a labelling of a set (clusters at a level, a cut of the tree, representatives, HDBSCAN*, a user's
 * metadata).  These judge one: per sample the silhouette, the nearest other group and the squared distance to the own group's
 * centroid; per group the medoid, the mean silhouette and the dispersion (what betadisper reports).  All of it follows from
 * the per-sample sums of distances to every group, B[i][g] = sum over j in g of w(i,j); only the own group's and the nearest
 * other group's entry of a row are kept, so neither the n x n matrix nor the sample x group table is stored, and the number
 * of groups is not bounded.
 *
 * The weight of a cell.  k(i,j) is the rule of "principal coordinates" above, word for word (unit diagonal, floor, any norms).
 * Then, fp64, ONE rounding per line:
 *     t      = 1.0 - k(i,j)
 *     w(i,j) = (uint32) rint(t * 1073741824.0)             2^30; 0 on the diagonal, 2^30 for k = 0
 * -- the weight of "PERMANOVA" above.  1 - k is the Jaccard distance, so w is that distance in units of 2^-30; it is also d^2
 * in the geometry sqrt(1 - k) of the principal coordinates.  Every sum of w is an INTEGER.
 *
 * mvs_label_sums      F = [row_begin, row_end) of a resident set, m = |F|; labels: m HOST int32 in [-1, groups), labels[i -
 *                     row_begin] the group of sample i, -1 = unlabelled (noise, or not named); groups >= 1; ids may be sparse
 *                     (empty groups are allowed).  Per sample i of F with g = labels[i]:
 *                         own_sum[i]    = sum of w(i,j) over j in F with labels[j] = g                  (0 for g = -1)
 *                         B_ih          = sum of w(i,j) over j in F with labels[j] = h, for every non-empty group h != g
 *                         mean_ih       = (double)B_ih / (double)n_h                                    one IEEE division
 *                         near_group[i] = the h with the smallest (mean_ih, h): equal doubles go to the smaller id
 *                         near_sum[i]   = B_ih of that group
 *                     Without such a group near_group[i] = -1 and near_sum[i] = 0.  sizes[g] = #{i in F : labels[i] = g}
 *                     (NULL: not wanted).  Unlabelled samples are rows, never columns: they have a nearest group and belong
 *                     to nobody's sums.  own_sum, near_sum: HOST uint64 [m]; near_group: HOST int32 [m]; all three needed
 *                     unless the range is empty.  The host sorts F by label (stable, unlabelled last) and gathers the set and
 *                     the norms into that order (mvs_sketch_set_gather), so that a group is an interval of columns; rows go in
 *                     blocks sized as mvs_group_sums sizes them without the clamp (options labels_block_rows, labels_dots);
 *                     per block one dense-dots launch against the labelled columns and one kernel that takes the weight from
 *                     the dot in registers and reduces the row by segments.  O(m) bytes cross the link.  Device memory besides
 *                     the set: the gathered copy, one dots block, O(m) arrays.  No sum wraps: a row's sum is at most
 *                     m * 2^30 < 2^61 for m <= 2^31 - 1; a larger m is refused.  The results do not depend on the row
 *                     blocking, the dots kernel or the order of the labels.  An empty range: MVS_OK, zero sizes.
 *                     MVS_E_INVALID: a label outside [-1, groups), groups < 1, floor outside [0, 1) or NaN, a range outside
 *                     the set, a NULL buffer that is needed.
 * mvs_silhouette_stats  pure host: labels, sizes and the three arrays of mvs_label_sums -> the numbers.  fp64, each line one
 *                     rounding.  Per labelled sample, n_g the size of its group and n_near that of near_group[i]:
 *                         a           = ((double)own_sum / (double)(n_g - 1)) * 2^-30                   0 for n_g = 1
 *                         b           = ((double)near_sum / (double)n_near) * 2^-30
 *                         s           = (b - a) / max(a, b)           0 for n_g = 1 or max(a, b) = 0 (scikit-learn's convention)
 *                         centroid_d2 = ((double)own_sum / (double)n_g - ((double)W_g / (double)n_g) / (double)n_g) * 2^-30
 *                     W_g = (sum of own_sum over the group) / 2, exact in 128 bits (an odd sum: MVS_E_INTERNAL, as in
 *                     mvs_group_sums).  centroid_d2 is the squared distance to the group's centroid in the principal
 *                     coordinates; it may be negative because the estimated kernel is not Euclidean, and is reported as it is.
 *                     Per unlabelled sample s, a and centroid_d2 are NaN; b (and the nearest group) are given.  Per group g:
 *                         medoids[g]          = the member with the smallest (own_sum, index), as an index into F (-1: empty)
 *                         group_mean_s[g]     = (sum of s over the members in ascending index) / n_g            (NaN: empty)
 *                         group_dispersion[g] = (sum of centroid_d2 over the members in ascending index) / n_g  (NaN: empty)
 *                         group_within[g]     = ((double)W_g / (double)(n_g (n_g - 1) / 2)) * 2^-30, 0 for n_g < 2 -- the
 *                                               group_mean_d2 of mvs_permanova_stats
 *                     result: mean = (sum of s over the labelled samples in ascending index) / their number; negative = the
 *                     labelled samples with s < 0; samples = m; labelled; groups = the non-empty ones.  Every output array but
 *                     `result` may be NULL.  MVS_E_INVALID: fewer than 2 non-empty groups, sizes that are not those of the
 *                     labels, a near_group that is not another non-empty group, a label outside [-1, groups), a NULL input.
 * mvs_silhouette      mvs_label_sums, then mvs_silhouette_stats; group_sizes [groups] and nearest [m] (near_group) may be NULL
 *                     like the arrays of the statistic.  Fewer than 2 non-empty groups is refused before any launch.
 * mvs_ctx_label_stats of the context's last mvs_label_sums / mvs_silhouette: kernel times of the dots and of the reduction
 *                     summed over the row blocks, the time of the gather (all 0 unless mvs_ctx_set_timing is on), row blocks,
 *                     rows per block.  Any pointer may be NULL.
 * All synchronous.  The kernel is in csrc/mvs_labelsum.hip. */
typedef struct {
    double mean;                                   /* mean silhouette of the labelled samples */
    int64_t negative, samples, labelled, groups;   /* groups: the non-empty ones */
} mvs_silhouette_result;
int mvs_label_sums(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double floor, int64_t row_begin,
                   int64_t row_end, const int32_t* labels, int groups, uint64_t* own_sum, int32_t* near_group, uint64_t* near_sum,
                   int64_t* sizes);
int mvs_silhouette_stats(const int32_t* labels, int64_t m, int groups, const int64_t* sizes, const uint64_t* own_sum,
                         const int32_t* near_group, const uint64_t* near_sum, mvs_silhouette_result* result, double* s, double* a,
                         double* b, double* centroid_d2, double* group_mean_s, double* group_within, double* group_dispersion,
                         int64_t* medoids);
int mvs_silhouette(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double floor, int64_t row_begin,
                   int64_t row_end, const int32_t* labels, int groups, mvs_silhouette_result* result, int64_t* group_sizes,
                   int32_t* nearest, double* s, double* a, double* b, double* centroid_d2, double* group_mean_s, double* group_within,
                   double* group_dispersion, int64_t* medoids);
int mvs_ctx_label_stats(const mvs_ctx* ctx, double* dots_ms, double* reduce_ms, double* gather_ms, int64_t* row_blocks,
                        int64_t* block_rows);

/* ---- Average and complete linkage: the agglomerative tree of the Jaccard distances ---------------------------
 * Single linkage (mvs_pairwise_linkage) chains.  Average linkage (UPGMA) and complete linkage do not, but they need the
 * distance between GROUPS, a sum (or maximum) over all cross pairs: this is the one clustering here that keeps the m x m
 * table, 8 m^2 bytes on the device.  It keeps it in integers: with the weight w = rint((1 - k) * 2^30) of "Labelling quality"
 * above, a merge is an addition, an average is one rational number, and no order of rounds, blocks or lanes changes a merge.
 *
 * State.  Slots 0 .. m-1, each alive or dead, a live slot s with a size n_s >= 1; a symmetric table S[a][b] of uint64: for
 * MVS_HCLUST_AVERAGE the sum of w over the cross pairs of the clusters in slots a and b, for MVS_HCLUST_COMPLETE their maximum.
 * The diagonal is never read.  A slot's index is the smallest member of its cluster.
 *
 * A round.  Every live row r names its nearest live column c != r: the one with the smallest (value, key).
 *     average:   value = S[r][c] / n_c as an exact rational -- S1 / n1 < S2 / n2 iff S1 * n2 < S2 * n1, in 128 bits
 *     complete:  value = S[r][c]
 *     key(r, c) = splitmix64(((uint64)min(r, c) << 32) | max(r, c)), splitmix64(x): x += 0x9E3779B97F4A7C15;
 *                 x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; return x ^ x >> 31
 * Keys of distinct pairs are distinct, so the order is total; the key is symmetric, so the globally smallest pair is mutual
 * and every round merges at least one pair -- and a clique of equal distances halves per round instead of losing one slot
 * per round, as it would with "ties go to the smaller column".
 * All mutual pairs (a, b), a < b, nearest[a] = b and nearest[b] = a, merge in that round:
 *     first every live row r, the dying ones included:  S[r][a] = S[r][a] (+) S[r][b]          for every pair
 *     then every pair, over the live columns c:          S[a][c] = S[a][c] (+) S[b][c]
 *     then n_a += n_b and b dies
 * (+) is + for average and max for complete.  Rounds repeat until one slot lives: m - 1 merges.
 *
 * A merge record, mvs_hmerge: a < b the two slots, round (from 0), size = n_a + n_b, sum = S[a][b] before the merge, and
 *     average:   height = ((double)sum / ((double)n_a * (double)n_b)) * 2^-30     one IEEE division; the product is exact
 *     complete:  height = (double)sum * 2^-30
 * Records are in (round, a) ascending order.  Both linkages are reducible: a merge's exact value is never below that of its
 * children (the double heights follow wherever a sum is below 2^53).
 *
 * Bounds.  The total of the sizes is <= 2^17 = 131072 and every entry <= n_a * n_b * 2^30, so no sum reaches 2^63; anything
 * beyond: MVS_E_INVALID.  A table the device cannot hold: MVS_E_NOMEM, the message names the bytes asked for (8 m^2 for the
 * table, rows padded to an even length, plus one block of dots).
 *
 * mvs_hclust_sums     the engine.  sums: m x m uint64, row-major, HOST or DEVICE (mem), symmetric off the diagonal (checked;
 *                     the diagonal is ignored); sizes: m HOST int32 >= 1, NULL = all ones.  For a caller who starts from
 *                     groups already formed (representatives with their group sizes).  merges: m - 1 HOST records; rounds
 *                     (may be NULL): the rounds it took.  The caller's table is copied, not changed.
 * mvs_hclust_weights  w: m x m uint32 <= 2^30, row-major, HOST or DEVICE, symmetric off the diagonal; unit sizes.
 * mvs_hclust          F = [row_begin, row_end) of a resident set, m = |F|; slot i is sample row_begin + i.  Rows go in blocks
 *                     (options hclust_block_rows, hclust_dots): one dense-dots launch, then a kernel that writes the
 *                     table's rows with the weight of "Labelling quality".  The table stays on the device; the records
 *                     cross the link.  MVS_E_INVALID: floor outside [0, 1) or NaN, a range outside the set.
 * Per round: one workgroup per live row scans the live columns (16-byte loads; the exact comparison per lane, one reduction
 * through the wave and LDS); one workgroup finds the mutual pairs with a prefix scan over the live rows in ascending order --
 * which is the records' order --, writes records, sizes and the next list of live rows; the column phase and the row phase of
 * the merge are two launches.  Option hclust_compact: 1 (default) when at most half the columns of the layout are alive, the
 * columns of every live row are compacted in place (rows stay where they are: the table is never held twice), 2 after every
 * round, 0 never.  Neither option changes a record.  m = 1: MVS_OK, no merges.  MVS_E_INVALID: an unknown method, m < 1, an
 * asymmetric table, an entry or a size outside the bounds, a NULL that is needed.
 *
 * Pure host, no device (like mvs_hdbscan_select); merges: the m - 1 records of one of the calls above:
 * mvs_hclust_order      Z: double [m - 1][4], SciPy's linkage matrix.  The merges sorted by (height, round, a); a leaf has
 *                       its index as id, the t-th merge of the sorted order the id m + t; Z[t] = {the smaller id, the larger
 *                       id, height, size} of the clusters in slots a and b.
 * mvs_hclust_cut        labels: int32 [m] after the merges with height <= `height` (NaN: MVS_E_INVALID).
 * mvs_hclust_cut_count  labels after the first m - k merges of the sorted order: k clusters, 1 <= k <= m.
 *                       Labels are 0-based in ascending order of each cluster's smallest member.
 * mvs_ctx_hclust_stats  of the context's last call: kernel times of the dots and the fill summed over the row blocks, of the
 *                       nearest pass, the merge (pairs + both phases) and the compactions summed over the rounds (all 0
 *                       unless mvs_ctx_set_timing is on); rounds, row scans, bytes of the table the scans read, compactions.
 *                       Any pointer may be NULL.
 * All synchronous.  The kernels are in csrc/mvs_hclust.hip. */
#define MVS_HCLUST_AVERAGE 0
#define MVS_HCLUST_COMPLETE 1
#define MVS_HCLUST_MAX_TOTAL 131072
typedef struct {
    int32_t a, b, round, size;
    uint64_t sum;
    double height;
} mvs_hmerge;
int mvs_hclust_sums(mvs_ctx* ctx, const uint64_t* sums, int mem, const int32_t* sizes, int64_t m, int method, mvs_hmerge* merges,
                    int64_t* rounds);
int mvs_hclust_weights(mvs_ctx* ctx, const uint32_t* w, int mem, int64_t m, int method, mvs_hmerge* merges, int64_t* rounds);
int mvs_hclust(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double floor, int64_t row_begin,
               int64_t row_end, int method, mvs_hmerge* merges, int64_t* rounds);
int mvs_hclust_order(int64_t m, const mvs_hmerge* merges, double* Z);
int mvs_hclust_cut(int64_t m, const mvs_hmerge* merges, double height, int32_t* labels);
int mvs_hclust_cut_count(int64_t m, const mvs_hmerge* merges, int64_t k, int32_t* labels);
int mvs_ctx_hclust_stats(const mvs_ctx* ctx, double* dots_ms, double* fill_ms, double* nearest_ms, double* merge_ms, double* compact_ms,
                         int64_t* rounds, int64_t* row_scans, int64_t* bytes_scanned, int64_t* compactions);

/* ---- Communities: modularity clustering (Louvain) of the thresholded Jaccard graph --------------------------------------------
 * Single linkage chains, dereplication fixes a radius, HDBSCAN* calls everything noise that is no density peak, average linkage
 * needs the m x m table.  Modularity communities work on what the comparison produces anyway -- the kept cells above a floor --,
 * need memory proportional to the edges, have one knob (the resolution) and partition every sample.  The reference has nothing
 * of the kind.  Everything below is an integer: no order of summation, blocking, atomics or fed cells can change a result, and
 * tests/communities_model.py is the same rule in Python integers.
 *
 * Graph.  n samples.  A fed cell (row, col, dot) with row != col is the edge {lo, hi} of weight a = rint(k * 2^20), k the clamped
 *   estimate of "PERMANOVA" above: inter = (double)dot / d (dot * (1 / d) when d is a power of two); s = n2[row] + n2[col];
 *   den = s - inter; J = inter / den; k = !(J > floor) ? 0 : (J > 1 ? 1 : J) -- fp64, one rounding per operation, the operations
 *   of the distance w up to k.  An edge with a = 0 (a NaN estimate included) does not exist.  (r, c), (c, r) and repeated feeding
 *   are one edge; where copies disagree the larger weight wins.  A cell that names a sample outside [0, n) is ignored and
 *   reported as MVS_E_RANGE, the rule of mvs_cluster_add_cells.  20 fractional bits, not the 30 of w: 10^-6 in J, far below
 *   the estimator's error, and W (below) stays under 2^55 for a clique of 100 000 and for 10^6 samples of mean degree 1 000, so
 *   every product below fits a signed 128-bit integer.  W >= 2^55: mvs_community_finish fails with MVS_E_RANGE.
 * Resolution.  R = 2^12, g = rint(resolution * R), 2^-12 <= resolution <= 16.
 * Level l.  Vertices v with a self weight s_v (0 at level 0) and off-diagonal weights a_uv.  Strength k_v = s_v + sum_{u != v}
 *   a_vu; W = sum_v k_v, the same on every level.  A level starts with c(v) = v.
 * Round r = 0, 1, ... -- all reads are from the state at the start of the round:
 *   v is ACTIVE iff the lowest bit of splitmix64((l << 48) ^ (r << 32) ^ v) is 1 (splitmix64 as in "Average and complete
 *   linkage" above).  Half the vertices move per round: a synchronous sweep of all of them swaps neighbours forever.
 *   For an active v in community A and every OTHER community C that holds a neighbour of v:
 *       gain(C) = R W (k_vC - k_vA) - g k_v (tot(C) - tot(A) + k_v),   k_vC = sum_{u != v, c(u) = C} a_vu,  tot(C) = sum_{u in C} k_u
 *   The best C has the largest gain, ties go to the smaller C.  v moves to it iff that gain is > 0 and not (size(A) = 1 and
 *   size(C) = 1 and C > A).  All moves of a round are applied together.  Then
 *       Qnum = R W sum_C in(C) - g sum_C tot(C)^2,   in(C) = sum_{v in C} s_v + sum over ordered pairs u != v in C of a_uv;
 *   the modularity is Qnum / (R W^2).
 * End of a level.  After a round in which no vertex moved, after 3 consecutive rounds that did not raise Qnum above the best
 *   seen, or after max_rounds rounds.  The level's result is the best state seen (the earliest, among equals); the singleton
 *   state counts as seen first.
 * Aggregation.  The communities of the level's result are numbered in the order of their smallest member; if they are all
 *   singletons the algorithm ends (that level is still reported), and it ends after MVS_COMMUNITY_MAX_LEVELS levels.  Otherwise
 *   s'_C = in(C), a'_CD = the summed weights between C and D, and the next level starts from that graph.
 * Finish.  A sample's community is the composition of the levels.  Every community is then split into the connected components
 *   of its level-0 edges (the union-find of mvs_cluster_*): a split can only raise Qnum, and it removes Louvain's known defect
 *   of disconnected communities.  Final labels are numbered by smallest member; the final Qnum is that of the final labels.
 *
 * mvs_community_create    an empty graph over n samples.  norms_sq (n doubles, `mem_norms`), d and floor decide the weight of a
 *                         fed cell; norms_sq may be NULL for a graph that takes raw edges only.  floor outside [0, 1) or NaN:
 *                         MVS_E_INVALID.  Resets the statistics mvs_ctx_community_stats reports.
 * mvs_community_add_cells the cells of a DEVICE list (any producer's; q is not read).  The list is consumed when the call returns.
 * mvs_community_add_edges raw integer edges (lo[i], hi[i], a[i]), 1 <= a <= 2^20, HOST or DEVICE (`mem`): the entry of crafted
 *                         tests and of other producers.  lo == hi is ignored; an index outside [0, n) or a weight outside its
 *                         range is ignored and reported as MVS_E_RANGE (the rest is consumed).
 * mvs_pairwise_community  the one-call producer: the comparison of mvs_pairwise_cluster (its staging buffer, halving rule, options
 *                         cluster_cells / cluster_block_rows and argument checks on `floor`: outside (0, 1) is MVS_E_INVALID),
 *                         every block's list fed to add_cells.  The set's d must be the graph's.  The comparison runs at the
 *                         level floor * (1 - 2^-40), not at floor: its keep test, (double)dot / d > t / (1 + t) * s, and the
 *                         rule's J > floor are one inequality in algebra and differ in fp64 within a few doubles of the boundary
 *                         (at floor 0.1 and d = 384 the keep test drops pairs whose J exceeds the floor).  2^-40 is 2^12 times
 *                         that disagreement, so every pair with J > floor is kept and add_cells decides it: the edge set is the
 *                         graph rule's alone wherever s = n2[row] + n2[col] > 0.  (A pair with s < inter < 0 -- negative norms
 *                         and a negative dot -- has J > 0 and fails the keep test at every level: it is never fed.)  So
 *                         mvs_pairwise_cluster at level t and the communities at floor t may differ, in degree and in who is
 *                         linked, on pairs whose J is within an ulp of t.
 * mvs_community_finish    builds the graph if cells arrived since the last build (sort, one entry per edge, both directions
 *                         sorted into a CSR) and runs the rule.  May be called again with another resolution without feeding
 *                         again; more cells may be added in between.  `mem_out` says where labels (n int32), level_labels
 *                         (level_capacity x n int32, row l = every sample's community after level l), degree (n int32),
 *                         strength (n uint64, k_v of level 0), internal and total (room for n uint64 each, res->communities are
 *                         written: in(C) and tot(C) of the final communities) live.  level_communities, level_rounds (int64) and
 *                         level_qnum_hi / _lo are HOST arrays of level_capacity entries: a 128-bit value is hi * 2^64 + lo as in
 *                         mvs_group_sums, in two's complement (Qnum may be negative).  Any pointer may be NULL.  More than
 *                         level_capacity levels with a level array given: MVS_E_CAPACITY after everything else was written
 *                         (MVS_COMMUNITY_MAX_LEVELS always suffices).  res: edges, W, levels, the final communities, the
 *                         communities before the split, rounds of all levels, the final Qnum, g.  resolution outside
 *                         [2^-12, 16], NaN, max_rounds < 1: MVS_E_INVALID.
 * mvs_communities         create, mvs_pairwise_community, finish, destroy in one call.
 * mvs_community_modularity  pure host, no device (like mvs_hdbscan_select): Qnum of `labels` (any int32 values) on the graph of
 *                         the raw edges (the graph rule above: pairs once, the larger weight wins) at g_fixed = g.  Weights are
 *                         int64 here, 1 <= a < 2^55, so that a coarse graph can be checked too; W >= 2^55, an index outside
 *                         [0, n) or a weight outside its range: MVS_E_RANGE.
 * Local moving, the hot path: a sweep of the CSR per round.  A vertex's edge weights are summed by neighbour community in a hash
 * table, then the table is scanned for the best (gain, smaller C) with 128-bit gains.  Three paths, by the vertex's degree:
 *     wave       degree <= 256:    one wave, 128 slots in LDS
 *     workgroup  degree <= 16384:  256 lanes, 4096 slots in LDS
 *     global     beyond:           256 lanes, >= 2 x degree slots in device memory
 * A vertex that meets more neighbour communities than its table has slots is handed to the next path and done again from the
 * start: nothing is lost or counted twice; the global table cannot fill.  Option community_path: 0 (default) by degree, 1 / 2 / 3
 * = every vertex starts in the wave / workgroup / global path.  It never changes a result.
 * mvs_ctx_community_stats since the context's last mvs_community_create: kernel times of the comparison, the build, the local
 *                         moving and the numbering + aggregation, the moving of level 0 alone (all 0 unless mvs_ctx_set_timing
 *                         is on); edges, levels and rounds of the last finish resp. all finishes, row blocks, the rounds of level
 *                         0 and the bytes one of them reads (row_ptr, col, weight, the community gather); paths[5]: vertices
 *                         that started in the wave / workgroup / global path (summed over the levels) and the hand-overs wave ->
 *                         workgroup and workgroup -> global (summed over the rounds).  Any pointer may be NULL.
 * All synchronous.  The kernels are in csrc/mvs_community.hip. */
#define MVS_COMMUNITY_MAX_LEVELS 64
typedef struct mvs_community mvs_community;
typedef struct {
    int64_t n, edges, levels, communities, composed, rounds;
    uint64_t total_weight;          /* W */
    uint64_t qnum_hi, qnum_lo;      /* the final Qnum */
    int64_t g_fixed;
} mvs_community_result;
int mvs_community_create(mvs_ctx* ctx, int64_t n, int d, const double* norms_sq, int mem_norms, double floor, mvs_community** graph);
int mvs_community_add_cells(mvs_community* graph, const mvs_cell* d_cells, int64_t n_cells);
int mvs_community_add_edges(mvs_community* graph, const int32_t* lo, const int32_t* hi, const int32_t* a, int64_t n_edges, int mem);
int mvs_pairwise_community(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double floor,
                           mvs_community* graph);
int mvs_community_finish(mvs_community* graph, double resolution, int64_t max_rounds, int32_t* labels, int32_t* level_labels,
                         int64_t level_capacity, int32_t* degree, uint64_t* strength, uint64_t* internal, uint64_t* total, int mem_out,
                         int64_t* level_communities, int64_t* level_rounds, uint64_t* level_qnum_hi, uint64_t* level_qnum_lo,
                         mvs_community_result* res);
int mvs_community_destroy(mvs_community* graph);
int mvs_communities(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, double floor, double resolution,
                    int64_t max_rounds, int32_t* labels, int32_t* level_labels, int64_t level_capacity, int32_t* degree,
                    uint64_t* strength, uint64_t* internal, uint64_t* total, int mem_out, int64_t* level_communities,
                    int64_t* level_rounds, uint64_t* level_qnum_hi, uint64_t* level_qnum_lo, mvs_community_result* res);
int mvs_community_modularity(int64_t n, const int32_t* lo, const int32_t* hi, const int64_t* a, int64_t n_edges, const int32_t* labels,
                             int64_t g_fixed, uint64_t* qnum_hi, uint64_t* qnum_lo);
int mvs_ctx_community_stats(const mvs_ctx* ctx, double* compare_ms, double* build_ms, double* move_ms, double* aggregate_ms,
                            double* level0_move_ms, int64_t* edges, int64_t* levels, int64_t* rounds, int64_t* row_blocks,
                            int64_t* level0_rounds, int64_t* level0_bytes, int64_t* paths);

/* ---- t-SNE: the exact map of the Jaccard kNN graph ---------------------------------------------------------------------------
 * The two ordinations above are linear; at 10^5 .. 10^6 samples in hundreds of groups two leading axes show a blob.  What one
 * draws of such a collection is its neighbour graph: t-SNE on the K best Jaccard estimates of every sample.  Both expensive inputs
 * exist here exactly -- mvs_pairwise_topk's cells and the community graph's sort + sum-by-key --, and the gradient's all-pairs
 * repulsion is n^2 rational terms per iteration, which the device evaluates exactly: no Barnes-Hut tree, no FFT grid, no n x n
 * buffer.  A pair's term is a fixed sequence of IEEE fp64 operations, each rounded once and never fused (the precedent of
 * "PERMANOVA" and "Communities"), and is QUANTISED before it is added: every sum over more than one term is a sum of integers.
 * No tiling, atomic or order of lanes can change a coordinate, and tests/tsne_model.py -- the same rule in numpy -- equals the
 * device bit for bit over hundreds of iterations.  Two quantities pass through exp / log and are not bit-stable: beta, which the
 * stopping rule pins, and the KL divergence, which is reported once.
 *
 * Affinities.  Row i has the neighbours j_1 .. j_m of a cell list sorted by row (mvs_pairwise_topk's, MVS_TOPK_EXCLUDE_SELF):
 *   m <= 256; m < K where n - 1 < K.  Per cell, in fp64, one rounding per operation, top-k's order:
 *       inter = (double)dot / d;  s = n2[i] + n2[j];  den = s - inter;  J = inter / den;  J = !(J > 0) ? 0 : (J > 1 ? 1 : J)
 *       delta = 1.0 - J                                   (the squared distance of "principal coordinates")
 *   x_j = delta_j - min_j delta_j;  w_j = exp(-beta x_j);  p_j = w_j / sum w;  H = log(sum w) + beta (sum w x) / (sum w).
 *   beta: 0 if m <= perplexity or all delta of the row are equal (p is uniform); else bisection from beta = 1 with lo = 0 and no
 *   upper bound: stop when |H - log(perplexity)| <= 1e-5 or after 200 steps; H too large: lo = beta, beta = beta * 2 while no upper
 *   bound is known, else (beta + hi) / 2; H too small: hi = beta, beta = (lo + beta) / 2.  The two sums are wave reductions, so
 *   beta may differ from another implementation's in its last bits.  Everything after beta is exact:
 *       c_ij = rint(p_j * 2^30)                           (int, a cell's value)
 *       s_ij = c_ij + c_ji, summed by key; both directions (i, j) and (j, i) are stored with the same s
 *       S = the sum of all stored s;  P_ij = (double)s_ij / (double)S
 *   Raw edges (lo, hi, s >= 1) enter the same sum: each adds s to (lo, hi) and to (hi, lo); duplicates and reversed copies add
 *   up; lo == hi is ignored.
 * One evaluation at the state y (n x 2 doubles).  Per ordered pair i != j:
 *       dx = y_i0 - y_j0;  dy = y_i1 - y_j1;  r = dx * dx + dy * dy;  q = 1.0 / (1.0 + r);  u = q * q
 *   Row sums, int64:  Z_i = sum_j rint(q * 2^40);  Rx_i = sum_j rint((u * dx) * 2^40), Ry_i likewise  (|u dx| < 0.33: a row fits
 *   for n < 2^23).  Z = sum_i (Z_i >> 20) fits int64 for n <= 2^21: a larger n is MVS_E_INVALID.  Zd = (double)Z * 2^-20.
 *   Attraction over the stored entries of row i:  Ax_i = sum_j rint(((P_ij * q) * dx) * 2^40), Ay_i likewise.
 *       g_x = 4.0 * (e * ((double)Ax_i * 2^-40) - ((double)Rx_i * 2^-40) / Zd),   e the exaggeration;
 *   the quotient counts as 0.0 where Z = 0 (n = 1).
 * One iteration, per coordinate, all reads from the state before it:
 *       gain = ((g > 0) == (vel > 0)) ? gain * 0.8 : gain + 0.2;  gain < 0.01: gain = 0.01
 *       vel  = momentum * vel - learning_rate * (gain * g);   y = y + vel
 *   A new handle's state is y = 0, vel = 0, gain = 1.  Nothing is recentred while the optimiser runs.  The state must stay finite.
 * mvs_tsne, the whole path.  K = params->neighbours, or ceil(3 * perplexity) where that is 0; 1 <= perplexity <= K <= 256 (so the
 *   default K allows a perplexity of 85), else MVS_E_INVALID.  Initial y: MVS_TSNE_INIT_PCOA -- the two leading coordinates of
 *   mvs_pcoa_fit(rows [0, n), floor 0, tol 1e-10, 300 iterations), times 1e-4 / sd, sd the population standard deviation of
 *   coordinate 1 with mean and squares summed in index order (n >= 3, sd > 0, else MVS_E_INVALID) -- or MVS_TSNE_INIT_RANDOM:
 *   u = (splitmix64(splitmix64(seed) ^ (2 i + axis)) >> 11) * 2^-53, y = (2 u - 1) * 1e-4.  Schedule: min(iterations,
 *   exaggeration_iters) iterations at e = exaggeration, momentum 0.5, the rest at e = 1, momentum 0.8; learning_rate <= 0 means
 *   max(n / 12 / 4, 50).  Output: Y = y - mean per axis, mean = ((double)sum_i rint(y_i * 2^30) * 2^-30) / n, an integer sum.
 *   KL = sum over the stored entries with s > 0 of P log(P / (q / Zd)), summed on the device with fp64 atomics.
 *
 * mvs_tsne_create         an empty graph and a fresh state over 1 <= n <= 2^21 samples.  Resets mvs_ctx_tsne_stats.
 * mvs_tsne_add_edges      raw integer edges, HOST or DEVICE (`mem`).  An index outside [0, n) or s < 1: MVS_E_RANGE, and NOTHING of
 *                         the list is added.
 * mvs_tsne_add_neighbours calibrates a cell list (HOST or DEVICE; sorted by row, <= 256 cells per row, row != col, indices in
 *                         [0, n): else MVS_E_RANGE / MVS_E_INVALID and nothing is added).  norms_sq: n doubles.  beta_out (HOST, n
 *                         doubles, may be NULL) is written for the rows between the list's first and last row; c_out (HOST, n_cells
 *                         int32, may be NULL) receives c per cell.  perplexity outside [1, 256]: MVS_E_INVALID.
 * mvs_tsne_finish_graph   sort, sum by key, CSR, S and P.  More may be added afterwards; finish again then.
 * mvs_tsne_edges          the stored directed entries sorted by (row, col): HOST arrays of `capacity`, any may be NULL; *n_entries
 *                         and *S are always written; MVS_E_CAPACITY if an array is given and too small.
 * mvs_tsne_set_state / _get_state   y, velocity, gain: HOST, n x 2 doubles each, any may be NULL (left as it is / not wanted).
 * mvs_tsne_gradient       one evaluation, state untouched: grad (n x 2), z_rows (n int64), *z -- HOST, any may be NULL.
 * mvs_tsne_run            `iterations` iterations at one (exaggeration, momentum, learning_rate); the host reads nothing back
 *                         while they run.
 * mvs_tsne_kl             KL at the present state.
 * _edges, _gradient, _run and _kl before mvs_tsne_finish_graph (or after feeding more): MVS_E_INVALID.  Every refusal leaves the
 * handle as it was.
 * mvs_tsne                top-k over row ranges (option cluster_block_rows bounds their rows), each range calibrated on the
 *                         device, the graph, the initial state, the schedule, the centring.  Y (n x 2), Y0 (the initial state),
 *                         beta (n): HOST, any may be NULL.  graph_out: NULL, or receives the handle with the final state (the
 *                         caller destroys it).
 * mvs_ctx_tsne_stats      since the context's last mvs_tsne_create: kernel times of top-k, calibration, graph build, and of the
 *                         repulsion, attraction and update summed over the iterations (0 unless mvs_ctx_set_timing is on: with
 *                         it every iteration is waited for); iterations, stored entries, units of one repulsion, top-k ranges.
 * The repulsion, the hot path: a unit is 256 rows x one slice of columns (option tsne_slice_cols, 16 .. 1024, default 1024;
 * never changes a result).  A lane owns a row; the slice's y is staged in LDS and read as broadcasts.  The quantised terms are
 * integer-valued doubles <= 2^40, at most 1024 of them per unit, so a lane's fp64 partial sums are exact below 2^53: one
 * conversion to int64 and one 64-bit atomic per accumulator and unit.  All synchronous.  The kernels are in csrc/mvs_tsne.hip. */
#define MVS_TSNE_INIT_PCOA   0
#define MVS_TSNE_INIT_RANDOM 1
typedef struct mvs_tsne_graph mvs_tsne_graph;
typedef struct {
    double perplexity, exaggeration, learning_rate;
    int64_t neighbours, iterations, exaggeration_iters, init;
    uint64_t seed;
} mvs_tsne_params;
typedef struct {
    int64_t n, neighbours, entries, beta_zero_rows, iterations;
    uint64_t S;
    double learning_rate, kl;
} mvs_tsne_result;
int mvs_tsne_create(mvs_ctx* ctx, int64_t n, mvs_tsne_graph** graph);
int mvs_tsne_destroy(mvs_tsne_graph* graph);
int mvs_tsne_add_edges(mvs_tsne_graph* graph, const int32_t* lo, const int32_t* hi, const int32_t* s, int64_t n_edges, int mem);
int mvs_tsne_add_neighbours(mvs_tsne_graph* graph, const mvs_cell* cells, int64_t n_cells, int mem_cells, const double* norms_sq,
                            int mem_norms, int d, double perplexity, double* beta_out, int32_t* c_out);
int mvs_tsne_finish_graph(mvs_tsne_graph* graph);
int mvs_tsne_edges(mvs_tsne_graph* graph, int32_t* row, int32_t* col, int64_t* s, int64_t capacity, int64_t* n_entries, uint64_t* S);
int mvs_tsne_set_state(mvs_tsne_graph* graph, const double* y, const double* velocity, const double* gain);
int mvs_tsne_get_state(mvs_tsne_graph* graph, double* y, double* velocity, double* gain);
int mvs_tsne_gradient(mvs_tsne_graph* graph, double exaggeration, double* grad, int64_t* z_rows, int64_t* z);
int mvs_tsne_run(mvs_tsne_graph* graph, int64_t iterations, double exaggeration, double momentum, double learning_rate);
int mvs_tsne_kl(mvs_tsne_graph* graph, double* kl);
int mvs_tsne(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, const mvs_tsne_params* params, double* Y,
             double* Y0, double* beta, mvs_tsne_result* result, mvs_tsne_graph** graph_out);
int mvs_ctx_tsne_stats(const mvs_ctx* ctx, double* topk_ms, double* calibrate_ms, double* graph_ms, double* repulse_ms,
                       double* attract_ms, double* update_ms, int64_t* iterations, int64_t* entries, int64_t* units, int64_t* row_blocks);

/* ---- multi-GPU exchange ---------------------------------------------------------------------------
 * One process per GPU; shard k of src/pairwise_comp_optimized.cpp:938-940 is rank k.  Where the reference's shard
 * processes each re-read the whole vectors.bin (:953, :962), a rank here loads (or sketches) only its own rows,
 * re-codes them into ITS row block of the global plane buffer (mvs_limb_split with row_offset = rank *
 * rows_per_rank) and ONE all-gather over RCCL / xGMI gives every GPU all N columns.  Norms travel the same way.
 *
 * mvs_comm_unique_id  : rank 0 draws the 128-byte RCCL id; the caller hands it to the other ranks out of band
 *                       (a file, an environment variable, MPI, a torch.distributed store ...).
 * mvs_comm_create     : collective over all ranks (ncclCommInitRank on the context's device).  RCCL is bound at
 *                       run time (dlopen): if it is missing this call fails with MVS_E_HIP, nothing else does.
 * mvs_comm_create_callbacks : the same interface over caller-supplied collectives -- for ranks that share one
 *                       device (RCCL refuses that), for tests, or for an application's own transport.  The
 *                       callbacks receive DEVICE pointers and the context's stream and return 0 on success.
 * The collectives below are in place and asynchronous on the context's stream (the callback kind: as the
 * callback chooses); every rank must call them in the same order with the same sizes. */
#define MVS_COMM_ID_BYTES 128
typedef struct mvs_comm mvs_comm;
typedef struct {
    void* user;
    /* buf holds world * bytes_per_rank bytes on the device; block `rank` is filled in, the others are wanted */
    int (*allgather)(void* user, void* buf, size_t bytes_per_rank, int rank, int world, void* hip_stream);
    /* *value (host) becomes the maximum over the ranks */
    int (*allreduce_max_i64)(void* user, int64_t* value, int rank, int world);
} mvs_comm_callbacks;
int mvs_comm_unique_id(void* id /* MVS_COMM_ID_BYTES */);
int mvs_comm_create(mvs_ctx* ctx, const void* id, int rank, int world, mvs_comm** comm);
int mvs_comm_create_callbacks(mvs_ctx* ctx, const mvs_comm_callbacks* callbacks, int rank, int world, mvs_comm** comm);
/* File transport: ranks exchange their blocks through files named <path_prefix>_<sequence>_<rank> in a directory
 * all of them can reach.  For ranks that share one device (RCCL refuses that) and for one-GPU test boxes; every
 * rank passes the same prefix.  Collective: the call returns when all `world` ranks have met under the prefix and
 * agreed on a job nonce (option comm_timeout_s, default 600, bounds the wait); every block carries that nonce and its
 * sequence number, so files an earlier job left under the same prefix are never read as this job's data, and a rank
 * removes its own files when it fails and when the communicator is destroyed. */
int mvs_comm_create_files(mvs_ctx* ctx, const char* path_prefix, int rank, int world, mvs_comm** comm);
/* RCCL communicator for shard processes that share nothing but a directory (how the reference's shard processes
 * relate: one process per --shard_idx, src/pairwise_comp_optimized.cpp:937-940): the ranks meet through the file
 * transport's handshake above, rank 0's id (mvs_comm_unique_id) travels as one verified block, the meeting point is
 * removed again, then mvs_comm_create.  Replaces "rank 0 leaves the id in a file": a file a previous job left behind
 * can no longer be taken for this job's id. */
int mvs_comm_create_rendezvous(mvs_ctx* ctx, const char* path_prefix, int rank, int world, mvs_comm** comm);
/* Collective semantics of the file transport (mvs_comm_create_files / _rendezvous): creation is a blocking handshake --
 * every rank must be inside its create call at the same time (ranks created one after the other from ONE thread would
 * wait for each other until comm_timeout_s); destruction is local once the communicator has carried at least one exchange,
 * otherwise it waits up to 10 s for the peers so that nobody is left polling for this rank's handshake files. */
int mvs_comm_destroy(mvs_comm* comm);
int mvs_comm_info(const mvs_comm* comm, int* rank, int* world, int* is_rccl);
/* Which RCCL the library bound at run time: the path of the shared object its collectives come from (dladdr; in a process
 * that already carries a copy -- PyTorch ships one -- the loader hands back that copy) and ncclGetVersion's number
 * (e.g. 22105).  Binds the library if that has not happened yet; MVS_E_HIP when no librccl can be loaded.  A measurement
 * that claims "RCCL over xGMI" should say which RCCL. */
int mvs_comm_library(char* path, size_t path_len, int* version);
/* planes: the global plane buffer (mvs_limb_geometry of rows_per_rank * world rows); rank r has filled rows
 * [r * rows_per_rank, (r+1) * rows_per_rank).  After the call (on the stream) every block is present. */
int mvs_allgather_planes(mvs_ctx* ctx, mvs_comm* comm, int8_t* planes, int64_t rows_per_rank, int limbs, int d_pad);
/* The same for a sub-range of every rank's block: rows [row_first, row_first + row_count) of each block of
 * rows_per_rank rows (each rank has filled that sub-range of ITS block).  A rank can thus hand over the rows it has
 * finished while it is still producing the rest -- e.g. sketch the first half of its samples, start this exchange on
 * the communicator's stream, sketch the second half meanwhile (metagenome_vector_sketches_amd/parallel.py does). */
int mvs_allgather_rows(mvs_ctx* ctx, mvs_comm* comm, int8_t* planes, int64_t rows_per_rank, int64_t row_first,
                       int64_t row_count, int limbs, int d_pad);
/* values: DEVICE array of world * count_per_rank doubles (e.g. squared norms), block `rank` filled in */
int mvs_allgather_f64(mvs_ctx* ctx, mvs_comm* comm, double* values, int64_t count_per_rank);
/* any DEVICE buffer of world * bytes_per_rank bytes (e.g. kept cells that belong to other ranks' rows) */
int mvs_allgather_bytes(mvs_ctx* ctx, mvs_comm* comm, void* buf, int64_t bytes_per_rank);
/* *value (HOST) becomes the maximum over all ranks (largest |v| -> one limb code for everybody).  Synchronous. */
int mvs_allreduce_max_i64(mvs_ctx* ctx, mvs_comm* comm, int64_t* value);

/* src/pairwise_comp_optimized.cpp:903-906 and :938-940, for drivers that keep the reference CLI */
int64_t mvs_chunk_size(double max_memory_gb, int d);
void mvs_shard_rows(int64_t n, int num_shards, int shard_idx, int64_t* begin, int64_t* end);

#ifdef __cplusplus
}
#endif
#endif /* MVS_HIP_H */
