// mvs_gather.hip -- the kernels of mvs_gather: the greedy decomposition of a query's hash list into samples of a hash set
// (include/mvs_hip.h "gather").  The reference has nothing like it: its search (src/jaccard.py) judges pairs.
//
// The walk is sequential -- every round removes the winner's hashes from what is left of the query -- so the work is to make a
// round ONE streaming pass with no host round trip.  That is done on the POSITIONS of the query's sorted list:
//
//   k_gather_mark   once, for every surviving candidate s (those whose overlap with the whole query reaches min_hashes: the
//                   intersection kernel of mvs_intersect.hip counted it): a bit row over the query's positions, W = ceil(|Q| / 64)
//                   words, bit p set iff Q[p] is in H(s).  The units of work are those of mvs_intersect.hip and so is the walk
//                   (unit_of and walk_unit<true> of mvs_intersect_dev.h: every lane reaches the sink on every trip); a match sets a
//                   bit instead of adding one.  Where the query is the chunked side the 64 lanes cover 64 consecutive
//                   positions of a word that belongs to this unit alone (the unit size is a multiple of 64): the ballot is
//                   the word, lane 0 ORs it in with a plain load and store.  Where the candidate is the chunked side every
//                   lane finds its element's position in Q and sets the bit with an atomic OR.  Rows start zeroed.
//   k_gather_count  per round, one wave per (live survivor, slice of kGaSlice words): count[s] += sum of popcount(row[w] &
//                   alive[w]), the streaming read of the live rows.  Rows are cut into slices because the walk's tail has few
//                   live rows, each a megabyte long for a query of 10^7 hashes: one wave per row would leave the device idle.
//   k_gather_bid    per round, one thread per survivor: a live survivor below min_hashes is retired (counts only fall: it can
//                   never win again), the others bid with one 64-bit atomic max on (count << 32) | (2^32 - 1 - s): largest
//                   count, then smallest survivor index = smallest sample, since survivors are kept in ascending sample order.
//                   The bids of consecutive rounds go to alternating slots of the state, so that nobody resets a word that
//                   another workgroup of the same launch reads.
//   k_gather_pick   per round: no bid -> the walk is done; else every workgroup clears its part of the winner's bits from
//                   `alive`, and the first one writes the record, retires the winner, and ends the walk when max_matches
//                   records exist.
// Three launches per round.  Every kernel of a round returns at once when the walk is done, so the host queues rounds in
// batches and reads the state back once per batch.  Nothing spins, nothing is cooperative.  All arithmetic is on integers: the
// result is exact and does not depend on the order of anything.
#include "mvs_internal.h"
#include "mvs_intersect_dev.h"

namespace mvs {

namespace {

constexpr int kGaThreads = 256;
constexpr int kGaWaves = kGaThreads / 64;
constexpr int kGaSlice = 2048;                 // words of a row that one wave counts (16 KiB: 32 loads per lane)

// alive: ones for the positions [0, q_size); retired: nobody; counts: zero; state: nothing found yet
__global__ __launch_bounds__(kGaThreads) void k_gather_init(unsigned long long* __restrict__ alive, int64_t W, int32_t q_size,
                                                           int32_t* __restrict__ retired, int32_t* __restrict__ count, int64_t ns,
                                                           GatherState* __restrict__ st) {
    const int64_t stride = (int64_t)gridDim.x * kGaThreads;
    const int64_t i0 = (int64_t)blockIdx.x * kGaThreads + threadIdx.x;
    for (int64_t w = i0; w < W; w += stride) {
        const int64_t left = (int64_t)q_size - w * 64;                 // > 0
        alive[w] = left >= 64 ? ~0ULL : ((1ULL << left) - 1ULL);
    }
    for (int64_t s = i0; s < ns; s += stride) {
        retired[s] = 0;
        count[s] = 0;
    }
    if (i0 == 0) {
        st->best[0] = st->best[1] = 0;
        st->rows_read = 0;
        st->done = 0;
        st->n_records = 0;
        st->remaining = q_size;
        st->rounds = 0;
    }
}

// what the walk found for position x of the chunked list, which the value shares with position y of the other one if hit.  The
// query chunked: the lanes of a trip stand at 64 consecutive positions of it, lane 0 at a multiple of 64 -- the ballot is the word,
// which is this unit's alone.  Else y is the bit.
__device__ __forceinline__ void mark_hits(unsigned long long* __restrict__ row, bool q_chunked, bool hit, int32_t x, int32_t y, int lane) {
    if (q_chunked) {
        const unsigned long long m = __ballot(hit);
        if (lane == 0 && m) row[x >> 6] |= m;
    } else if (hit) {
        atomicOr(row + (y >> 6), 1ULL << (y & 63));
    }
}

// cells[i] = (query, sample of survivor i); the units are those isect_plan laid out with `unit` (a multiple of 64);
// rows: n_cells x W words, zero on entry
__global__ __launch_bounds__(kIxThreads) void k_gather_mark(const mvs_cell* __restrict__ cells, int64_t n_cells,
                                                            const long long* __restrict__ unit_start, long long n_units,
                                                            const unsigned long long* __restrict__ hash_q,
                                                            const long long* __restrict__ off_q, const int32_t* __restrict__ size_q,
                                                            const unsigned long long* __restrict__ hash_d,
                                                            const long long* __restrict__ off_d, const int32_t* __restrict__ size_d,
                                                            int unit, unsigned long long* __restrict__ rows, int64_t W) {
    __shared__ unsigned long long tiles[kIxWaves][kTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long* tile = tiles[wave];
    const long long n_waves = (long long)gridDim.x * kIxWaves;
    for (long long u = (long long)blockIdx.x * kIxWaves + wave; u < n_units; u += n_waves) {
        // the query is the row of every cell: where it is the shorter list it is the chunked side (a0 is a multiple of 64)
        const IxUnit n = unit_of(cells, n_cells, unit_start, u, hash_q, off_q, size_q, hash_d, off_d, size_d, unit, lane);
        unsigned long long* row = rows + n.cell * W;
        walk_unit<true>(n, tile, lane, [&](int32_t x, int32_t y, bool hit) { mark_hits(row, n.row_short, hit, x, y, lane); });
    }
}

// one wave per (survivor, slice of kGaSlice words of its row): the slice's part of |row & alive| is added to count[s] (zero on
// entry: k_gather_init, then k_gather_bid behind every read).  A row is cut so that a round with FEW live rows still fills the
// device: one wave per row would stream a megabyte-long row 512 bytes at a time.
__global__ __launch_bounds__(kGaThreads) void k_gather_count(const unsigned long long* __restrict__ rows, int64_t W, int64_t ns,
                                                            int64_t n_slices, const unsigned long long* __restrict__ alive,
                                                            const int32_t* __restrict__ retired, int32_t* __restrict__ count,
                                                            const GatherState* __restrict__ st) {
    if (st->done) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * kGaWaves;
    const int64_t items = ns * n_slices;
    for (int64_t i = (int64_t)blockIdx.x * kGaWaves + wave; i < items; i += n_waves) {
        const int64_t s = i / n_slices;
        if (retired[s]) continue;
        const int64_t w0 = (i - s * n_slices) * kGaSlice;
        const int64_t w1 = w0 + kGaSlice < W ? w0 + kGaSlice : W;
        const unsigned long long* row = rows + s * W;
        int sum = 0;
#pragma unroll 4
        for (int64_t w = w0 + lane; w < w1; w += 64) sum += __popcll(row[w] & alive[w]);
        sum = wave_sum(sum);
        if (lane == 0 && sum) atomicAdd(count + s, sum);
    }
}

// one thread per survivor: a live one below min_hashes is retired (counts only fall: it can never win again), the others bid
// for this round's slot of the state
__global__ __launch_bounds__(kGaThreads) void k_gather_bid(int64_t ns, int32_t* __restrict__ retired, int32_t min_hashes,
                                                          int32_t* __restrict__ count, GatherState* __restrict__ st, int parity) {
    if (st->done) return;
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kGaThreads;
    for (int64_t base = (int64_t)blockIdx.x * kGaThreads; base < ns; base += stride) {   // (every lane makes every trip)
        const int64_t s = base + threadIdx.x;
        const bool live = s < ns && !retired[s];
        if (live) {
            const int32_t f = count[s];
            count[s] = 0;
            if (f < min_hashes) retired[s] = 1;
            else atomicMax(&st->best[parity], ((unsigned long long)f << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)s));
        }
        const unsigned long long n_live = (unsigned long long)__popcll(__ballot(live));
        if (lane == 0 && n_live) atomicAdd(&st->rows_read, n_live);
    }
}

// every workgroup clears its part of the winner's bits from `alive`; the first one keeps the books.  The state words this launch
// reads (done, best[parity]) are written by nobody in it but for `done`, and a workgroup that sees the walk ended early only
// skips work nobody will read.
__global__ __launch_bounds__(kGaThreads) void k_gather_pick(const unsigned long long* __restrict__ rows, int64_t W,
                                                           unsigned long long* __restrict__ alive, int32_t* __restrict__ retired,
                                                           const int32_t* __restrict__ surv_sample,
                                                           const int32_t* __restrict__ surv_orig, mvs_gather_match* __restrict__ rec,
                                                           int64_t max_matches, GatherState* __restrict__ st, int parity) {
    const int done = st->done;
    const unsigned long long best = st->best[parity];
    __syncthreads();                                                   // everybody here has read the state before thread 0 writes it
    if (done) return;
    const bool keeper = blockIdx.x == 0 && threadIdx.x == 0;
    if (best == 0) {                                                   // nobody is left at min_hashes or above
        if (keeper) {
            st->rounds += 1;
            st->done = 1;
        }
        return;
    }
    const int64_t s = (int64_t)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFULL));
    const int32_t unique = (int32_t)(best >> 32);
    const unsigned long long* row = rows + s * W;
    const int64_t stride = (int64_t)gridDim.x * kGaThreads;
    for (int64_t w = (int64_t)blockIdx.x * kGaThreads + threadIdx.x; w < W; w += stride) alive[w] &= ~row[w];
    if (keeper) {
        const int32_t k = st->n_records;
        const int32_t remaining = st->remaining - unique;              // the bits being cleared were alive: exactly `unique` of them
        mvs_gather_match m;
        m.sample = surv_sample[s];
        m.intersect = surv_orig[s];
        m.unique = unique;
        m.remaining = remaining;
        rec[k] = m;
        retired[s] = 1;
        st->remaining = remaining;
        st->n_records = k + 1;
        st->rounds += 1;
        st->best[parity ^ 1] = 0;                                      // the next round's slot
        if ((int64_t)k + 1 >= max_matches) st->done = 1;
    }
}

}  // namespace

int launch_gather_init(hipStream_t stream, unsigned long long* d_alive, int64_t W, int32_t q_size, int32_t* d_retired, int32_t* d_count,
                       int64_t ns, GatherState* d_state) {
    hipLaunchKernelGGL(k_gather_init, dim3(ix_grid(std::max(W, ns), kGaThreads)), dim3(kGaThreads), 0, stream, d_alive, W, q_size,
                       d_retired, d_count, ns, d_state);
    return 0;
}

int launch_gather_mark(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, const long long* d_unit_start, long long n_units,
                       const unsigned long long* d_hash_q, const long long* d_off_q, const int32_t* d_size_q,
                       const unsigned long long* d_hash_d, const long long* d_off_d, const int32_t* d_size_d, int unit,
                       unsigned long long* d_rows, int64_t W) {
    if (n_units <= 0) return 0;
    hipLaunchKernelGGL(k_gather_mark, dim3(ix_grid(n_units, kIxWaves)), dim3(kIxThreads), 0, stream, d_cells, n_cells, d_unit_start,
                       n_units, d_hash_q, d_off_q, d_size_q, d_hash_d, d_off_d, d_size_d, unit, d_rows, W);
    return 0;
}

int launch_gather_round(hipStream_t stream, const unsigned long long* d_rows, int64_t W, int64_t ns, unsigned long long* d_alive,
                        int32_t* d_retired, int32_t min_hashes, int32_t* d_count, const int32_t* d_surv_sample,
                        const int32_t* d_surv_orig, mvs_gather_match* d_rec, int64_t max_matches, GatherState* d_state, int parity) {
    const int64_t n_slices = (W + kGaSlice - 1) / kGaSlice;
    hipLaunchKernelGGL(k_gather_count, dim3(ix_grid(ns * n_slices, kGaWaves)), dim3(kGaThreads), 0, stream, d_rows, W, ns, n_slices,
                       d_alive, d_retired, d_count, d_state);
    hipLaunchKernelGGL(k_gather_bid, dim3(ix_grid(ns, kGaThreads)), dim3(kGaThreads), 0, stream, ns, d_retired, min_hashes, d_count,
                       d_state, parity);
    hipLaunchKernelGGL(k_gather_pick, dim3(ix_grid(W, 4 * kGaThreads)), dim3(kGaThreads), 0, stream, d_rows, W, d_alive, d_retired,
                       d_surv_sample, d_surv_orig, d_rec, max_matches, d_state, parity);
    return 0;
}

}  // namespace mvs
