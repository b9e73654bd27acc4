// mvs_intersect.hip -- exact sorted-set intersections of hash lists for lists of cells (mvs_hash_set_*, mvs_intersect_cells).
//
// Everything else in this library answers questions about the ESTIMATE: dot, q, the top-k lists and the clusters are exact
// with respect to the reference's arithmetic, and that arithmetic estimates |A n B| from two +-1 random projections.  This
// unit computes the quantity itself for the pairs a comparison kept: inter = |H(row) n H(col)| over the samples' hash lists,
// as the offline study of the reference does on simulated vectors (src/compute_error_of_random_projections.py,
// jaccard_exact()).  Nothing on the reference's hot path is replaced.
//
// A hash set is resident in HBM as the concatenation of per-sample lists, each STRICTLY INCREASING (sorted, no duplicates),
// with int64 offsets and int32 sizes.  Hash values are arbitrary 64-bit words: there is no sentinel anywhere, every bound
// below comes from an index.
//
// Units of work.  A cell's cost is anything between 3 and 10^6 elements, so the cell is not the unit.  With A the shorter of
// the two lists and B the longer, a unit is (cell, chunk c of A): elements [c * U, min(|A|, (c + 1) * U)) of A against all of
// B (U = option intersect_unit).  k_isect_count writes ceil(|A| / U) per cell (0 for an empty list or a cell out of range),
// an exclusive scan of those numbers lays the units of all cells out in cell order -- so consecutive units share the row's
// list while it is in the L2 / Infinity Cache -- and k_isect_units gives every unit to ONE wave.  Steps 1 and 2 are unit_of and
// step 3 is walk_unit of mvs_intersect_dev.h, which k_overlap_units (mvs_overlap.hip) and k_gather_mark (mvs_gather.hip) call
// too; step 4 is this kernel's own:
//   1. the unit's cell: upper bound of the unit index in the scanned array, as a 64-ary search (each lane probes one of 64
//      splitters and a ballot picks the interval: 3 rounds for 2^18 entries instead of 18 dependent loads);
//   2. B's window for the chunk: lower bound of the chunk's first element, upper bound of its last, the same search;
//   3. the window is staged in LDS tile by tile (kTile elements per wave, coalesced loads); for each tile the wave advances
//      over the elements of A that cannot lie behind the tile's last element (upper bound in the chunk, found with the same
//      search), each lane takes one of them and binary-searches the tile in LDS on the full 64-bit key;
//      a window more than kSkew times longer than the chunk (3 hashes against 300 000) is not streamed through LDS: each lane
//      binary-searches the window in global memory for its element, |A| log |B| probes instead of |B| loads;
//   4. matches are counted per lane, summed over the wave, and lane 0 adds the sum to inter[cell] with one atomic.  The
//      lists hold no duplicates, so an element of A matches at most one of B and the chunks of a cell partition A: the sum
//      over a cell's units is |A n B|.  Integer addition commutes: the result does not depend on the order of the units,
//      the unit size or the order of the cells.
// inter[] is zeroed by k_isect_count, a launch of its own in front of k_isect_units, for every cell in range; a cell out of
// range is never written.
#include "mvs_internal.h"
#include "mvs_intersect_dev.h"   // unit geometry (kIxThreads, kTile, kSkew), unit_of, walk_unit, wave_sum, ix_grid

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace mvs {

namespace {

__device__ __forceinline__ void wave_add64(unsigned long long* counter, unsigned long long v) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(counter, v);
}

// what the planning launch leaves in a cell's result: the count (0, or -1 for a cell out of range), and for the weighted
// overlaps (mvs_overlap.hip) the five sums zeroed with it
__device__ __forceinline__ void set_result(int32_t& r, int v) { r = v; }
__device__ __forceinline__ void set_result(mvs_abund_overlap& r, int v) { r = mvs_abund_overlap{v, 0, 0, 0, 0, 0}; }

// counters: [0] cells out of range, [1] cells cut into several units, [2] sum of 8 * (|A| + |B|) over the cells in range
// units[i] for i < n_cells, units[n_cells] = 0 (the exclusive scan then ends with the number of units)
template <typename R>
__global__ __launch_bounds__(kIxThreads) void k_isect_count(const mvs_cell* __restrict__ cells, int64_t n_cells,
                                                            const int32_t* __restrict__ size_r, int64_t n_r,
                                                            const int32_t* __restrict__ size_c, int64_t n_c, int unit,
                                                            long long* __restrict__ units, R* __restrict__ inter,
                                                            int mark_bad, unsigned long long* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kIxThreads;
    const int64_t rounds = (n_cells + 1 + stride - 1) / stride;        // every lane makes every trip: whole-wave sums
    int64_t i = (int64_t)blockIdx.x * kIxThreads + threadIdx.x;
    for (int64_t t = 0; t < rounds; ++t, i += stride) {
        unsigned long long bad = 0, cut = 0, bytes = 0;
        if (i < n_cells) {
            const int32_t r = cells[i].row, c = cells[i].col;
            long long u = 0;
            if (r < 0 || c < 0 || r >= n_r || c >= n_c) {
                bad = 1;
                if (mark_bad) set_result(inter[i], -1);                // (host output: the caller's entry is left alone)
            } else {
                const int32_t la = size_r[r], lb = size_c[c];
                const int32_t m = la < lb ? la : lb;
                u = ((long long)m + unit - 1) / unit;
                cut = u > 1;
                bytes = 8ULL * ((unsigned long long)la + (unsigned long long)lb);
                set_result(inter[i], 0);
            }
            units[i] = u;
        } else if (i == n_cells) {
            units[i] = 0;
        }
        wave_add64(counters + 0, bad);
        wave_add64(counters + 1, cut);
        wave_add64(counters + 2, bytes);
    }
}

__global__ __launch_bounds__(kIxThreads) void k_isect_units(const mvs_cell* __restrict__ cells, int64_t n_cells,
                                                            const long long* __restrict__ unit_start, long long n_units,
                                                            const unsigned long long* __restrict__ hash_r,
                                                            const long long* __restrict__ off_r, const int32_t* __restrict__ size_r,
                                                            const unsigned long long* __restrict__ hash_c,
                                                            const long long* __restrict__ off_c, const int32_t* __restrict__ size_c,
                                                            int unit, int32_t* __restrict__ inter) {
    __shared__ unsigned long long tiles[kIxWaves][kTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long* tile = tiles[wave];
    const long long n_waves = (long long)gridDim.x * kIxWaves;
    for (long long u = (long long)blockIdx.x * kIxWaves + wave; u < n_units; u += n_waves) {
        const IxUnit n = unit_of(cells, n_cells, unit_start, u, hash_r, off_r, size_r, hash_c, off_c, size_c, unit, lane);
        int found = 0;
        walk_unit<false>(n, tile, lane, [&](int32_t, int32_t, bool) { found += 1; });
        found = wave_sum(found);
        if (lane == 0 && found) atomicAdd(inter + n.cell, found);
    }
}

// ---- building a set ----
// *flag = 1 if some sample's list is not strictly increasing; one workgroup per sample at a time
__global__ __launch_bounds__(kIxThreads) void k_hs_check(const unsigned long long* __restrict__ hashes,
                                                         const long long* __restrict__ offsets, int64_t n,
                                                         unsigned int* __restrict__ flag) {
    bool bad = false;
    for (int64_t s = blockIdx.x; s < n; s += gridDim.x) {
        const long long b = offsets[s], e = offsets[s + 1];
        for (long long i = b + threadIdx.x; i + 1 < e; i += kIxThreads) bad |= !(hashes[i] < hashes[i + 1]);
    }
    if (bad) atomicOr(flag, 1u);
}

// distinct values per sample of SORTED lists
__global__ __launch_bounds__(kIxThreads) void k_hs_count(const unsigned long long* __restrict__ sorted,
                                                         const long long* __restrict__ offsets, int64_t n,
                                                         int32_t* __restrict__ sizes) {
    __shared__ int part[kIxWaves];
    for (int64_t s = blockIdx.x; s < n; s += gridDim.x) {
        const long long b = offsets[s], e = offsets[s + 1];
        int mine = 0;
        for (long long i = b + threadIdx.x; i < e; i += kIxThreads) mine += (i == b || sorted[i] != sorted[i - 1]) ? 1 : 0;
        mine = wave_sum(mine);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            int total = 0;
            for (int w = 0; w < kIxWaves; ++w) total += part[w];
            sizes[s] = total;
        }
        __syncthreads();
    }
}

// the first occurrence of every value of sample s (sorted lists at offsets[]) -> out at new_offsets[s], in order
__global__ __launch_bounds__(kIxThreads) void k_hs_compact(const unsigned long long* __restrict__ sorted,
                                                           const long long* __restrict__ offsets,
                                                           const long long* __restrict__ new_offsets, int64_t n,
                                                           unsigned long long* __restrict__ out) {
    __shared__ int part[kIxWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t s = blockIdx.x; s < n; s += gridDim.x) {
        const long long b = offsets[s], e = offsets[s + 1];
        long long at = new_offsets[s];
        for (long long i0 = b; i0 < e; i0 += kIxThreads) {              // (uniform over the workgroup)
            const long long i = i0 + threadIdx.x;
            unsigned long long v = 0;
            bool head = false;
            if (i < e) {
                v = sorted[i];
                head = i == b || v != sorted[i - 1];
            }
            const unsigned long long mask = __ballot(head);
            if (lane == 0) part[wave] = __popcll(mask);
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < kIxWaves; ++w) {
                before += w < wave ? part[w] : 0;
                total += part[w];
            }
            if (head) out[at + before + __popcll(mask & ((1ULL << lane) - 1ULL))] = v;
            at += total;
            __syncthreads();
        }
    }
}

}  // namespace

int launch_hs_check(hipStream_t stream, const unsigned long long* d_hashes, const long long* d_offsets, int64_t n,
                    unsigned int* d_flag) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_hs_check, dim3(ix_grid(n, 1)), dim3(kIxThreads), 0, stream, d_hashes, d_offsets, n, d_flag);
    return 0;
}

// Sorts `count` keys that form `segments` lists (d_begin / d_end: unsigned offsets relative to d_in) into d_out.
// d_scratch == NULL: *scratch_needed only.
int hs_sort_segments(hipStream_t stream, const unsigned long long* d_in, unsigned long long* d_out, unsigned int count,
                     unsigned int segments, const unsigned int* d_begin, const unsigned int* d_end, void* d_scratch,
                     size_t scratch_bytes, size_t* scratch_needed) {
    size_t need = 0;
    hipError_t e = rocprim::segmented_radix_sort_keys(nullptr, need, d_in, d_out, count, segments, d_begin, d_end, 0, 64, stream);
    if (e != hipSuccess) return MVS_E_HIP;
    if (scratch_needed) *scratch_needed = need;
    if (d_scratch == nullptr) return 0;
    if (scratch_bytes < need) return MVS_E_CAPACITY;
    e = rocprim::segmented_radix_sort_keys(d_scratch, need, d_in, d_out, count, segments, d_begin, d_end, 0, 64, stream);
    return e == hipSuccess ? 0 : MVS_E_HIP;
}

int launch_hs_count(hipStream_t stream, const unsigned long long* d_sorted, const long long* d_offsets, int64_t n, int32_t* d_sizes) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_hs_count, dim3(ix_grid(n, 1)), dim3(kIxThreads), 0, stream, d_sorted, d_offsets, n, d_sizes);
    return 0;
}

int launch_hs_compact(hipStream_t stream, const unsigned long long* d_sorted, const long long* d_offsets, const long long* d_new_offsets,
                      int64_t n, unsigned long long* d_out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_hs_compact, dim3(ix_grid(n, 1)), dim3(kIxThreads), 0, stream, d_sorted, d_offsets, d_new_offsets, n, d_out);
    return 0;
}

// d_units / d_unit_start: n_cells + 1 entries each; scratch as rocprim's scan wants it (d_scratch == NULL: *scratch_needed only)
template <typename R>
int isect_plan(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, const int32_t* d_size_r, int64_t n_r,
               const int32_t* d_size_c, int64_t n_c, int unit, long long* d_units, long long* d_unit_start, R* d_inter,
               bool mark_bad, unsigned long long* d_counters, void* d_scratch, size_t scratch_bytes, size_t* scratch_needed) {
    size_t need = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, need, d_units, d_unit_start, 0LL, (size_t)n_cells + 1, rocprim::plus<long long>(), stream);
    if (e != hipSuccess) return MVS_E_HIP;
    if (scratch_needed) *scratch_needed = need;
    if (d_scratch == nullptr) return 0;
    if (scratch_bytes < need) return MVS_E_CAPACITY;
    hipLaunchKernelGGL(k_isect_count<R>, dim3(ix_grid(n_cells + 1, kIxThreads)), dim3(kIxThreads), 0, stream, d_cells, n_cells, d_size_r,
                       n_r, d_size_c, n_c, unit, d_units, d_inter, mark_bad ? 1 : 0, d_counters);
    e = rocprim::exclusive_scan(d_scratch, need, d_units, d_unit_start, 0LL, (size_t)n_cells + 1, rocprim::plus<long long>(), stream);
    return e == hipSuccess ? 0 : MVS_E_HIP;
}
// the two results a plan is made for: counts, and the records of the weighted overlaps (mvs_overlap.hip)
template int isect_plan<int32_t>(hipStream_t, const mvs_cell*, int64_t, const int32_t*, int64_t, const int32_t*, int64_t, int, long long*,
                                 long long*, int32_t*, bool, unsigned long long*, void*, size_t, size_t*);
template int isect_plan<mvs_abund_overlap>(hipStream_t, const mvs_cell*, int64_t, const int32_t*, int64_t, const int32_t*, int64_t, int,
                                           long long*, long long*, mvs_abund_overlap*, bool, unsigned long long*, void*, size_t, size_t*);

int launch_isect_units(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, const long long* d_unit_start, long long n_units,
                       const unsigned long long* d_hash_r, const long long* d_off_r, const int32_t* d_size_r,
                       const unsigned long long* d_hash_c, const long long* d_off_c, const int32_t* d_size_c, int unit,
                       int32_t* d_inter) {
    if (n_units <= 0) return 0;
    hipLaunchKernelGGL(k_isect_units, dim3(ix_grid(n_units, kIxWaves)), dim3(kIxThreads), 0, stream, d_cells, n_cells, d_unit_start,
                       n_units, d_hash_r, d_off_r, d_size_r, d_hash_c, d_off_c, d_size_c, unit, d_inter);
    return 0;
}

}  // namespace mvs
