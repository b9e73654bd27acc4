// mvs_overlap.hip -- abundance-weighted overlaps of hash lists for lists of cells (mvs_abund_overlap_cells) and the per-sample
// totals of the abundances (mvs_hash_set_abundance_totals); the contract is in include/mvs_hip.h, "abundance-weighted overlaps".
//
// The work is that of mvs_intersect.hip and is laid out the same way: isect_plan cuts every cell into units of `unit` elements
// of its shorter list A and zeroes the cell's record, and k_overlap_units gives every unit to one wave, which decodes it and walks
// it with unit_of and walk_unit of mvs_intersect_dev.h.  What is its own happens in the sink, where a lane has found its key: it
// hears the position on both sides and loads the two abundances from global memory.  B's abundances are NOT staged beside the
// tile: a load happens on a match only, at most one per element of the chunk, and a side that carries no abundances (template
// argument) costs no load at all: its abundance is the constant 1.
//
// A lane accumulates the count and five 64-bit sums; the sums of a wave are reduced once per unit and lane 0 adds each non-zero
// one to the cell's record with a 64-bit integer atomic.  The lists hold no duplicates, so a value of A matches at most one of
// B and the chunks of a cell partition A: the sums over a cell's units are the contract's.  No sum can overflow (fewer than 2^31
// terms below 2^32 each) and integer addition commutes: nothing depends on the unit size or on any order.
#include "mvs_internal.h"
#include "mvs_intersect_dev.h"   // unit geometry (kIxThreads), unit_of, walk_unit, wave_sum, ix_grid

namespace mvs {

namespace {

// what a lane (and after the reduction a wave) found: sums over the matches of the abundances on A's side, on B's side, of
// their minimum and of the two halves of their product
struct Sums {
    unsigned long long n = 0, wa = 0, wb = 0, wmin = 0, dlo = 0, dhi = 0;
    __device__ __forceinline__ void add(unsigned int a, unsigned int b) {
        const unsigned long long p = (unsigned long long)a * b;
        n += 1;
        wa += a;
        wb += b;
        wmin += a < b ? a : b;
        dlo += p & 0xffffffffULL;
        dhi += p >> 32;
    }
};

__device__ __forceinline__ void add_field(unsigned long long* field, unsigned long long v) {
    if (v) atomicAdd(field, v);
}

template <bool kAbundR, bool kAbundC>
__global__ __launch_bounds__(kIxThreads) void k_overlap_units(const mvs_cell* __restrict__ cells, int64_t n_cells,
                                                              const long long* __restrict__ unit_start, long long n_units,
                                                              const unsigned long long* __restrict__ hash_r,
                                                              const long long* __restrict__ off_r, const int32_t* __restrict__ size_r,
                                                              const uint32_t* __restrict__ ab_r,
                                                              const unsigned long long* __restrict__ hash_c,
                                                              const long long* __restrict__ off_c, const int32_t* __restrict__ size_c,
                                                              const uint32_t* __restrict__ ab_c, int unit,
                                                              mvs_abund_overlap* __restrict__ out) {
    __shared__ unsigned long long tiles[kIxWaves][kTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long* tile = tiles[wave];
    const long long n_waves = (long long)gridDim.x * kIxWaves;
    for (long long u = (long long)blockIdx.x * kIxWaves + wave; u < n_units; u += n_waves) {
        const IxUnit n = unit_of(cells, n_cells, unit_start, u, hash_r, off_r, size_r, hash_c, off_c, size_c, unit, lane);
        const bool row_short = n.row_short;
        // the abundances aligned with A and B; NULL: 1 throughout (known when the kernel is compiled if neither side carries any)
        const uint32_t* wr = kAbundR ? ab_r + (row_short ? n.at_a : n.at_b) : nullptr;
        const uint32_t* wc = kAbundC ? ab_c + (row_short ? n.at_b : n.at_a) : nullptr;
        const uint32_t* WA = row_short ? wr : wc;
        const uint32_t* WB = row_short ? wc : wr;
        Sums s;
        walk_unit<false>(n, tile, lane, [&](int32_t x, int32_t y, bool) { s.add(WA ? WA[x] : 1u, WB ? WB[y] : 1u); });
        s.n = wave_sum(s.n);
        if (s.n == 0) continue;                                        // (the same for every lane) no match: every sum is 0
        s.wa = wave_sum(s.wa);
        s.wb = wave_sum(s.wb);
        s.wmin = wave_sum(s.wmin);
        s.dlo = wave_sum(s.dlo);
        s.dhi = wave_sum(s.dhi);
        if (lane == 0) {
            mvs_abund_overlap* o = out + n.cell;
            atomicAdd((unsigned long long*)&o->inter, s.n);
            add_field((unsigned long long*)&o->w_row, row_short ? s.wa : s.wb);
            add_field((unsigned long long*)&o->w_col, row_short ? s.wb : s.wa);
            add_field((unsigned long long*)&o->w_min, s.wmin);
            add_field((unsigned long long*)&o->dot_lo, s.dlo);
            add_field((unsigned long long*)&o->dot_hi, s.dhi);
        }
    }
}

// S, Q_lo, Q_hi of every sample: one workgroup per sample at a time
__global__ __launch_bounds__(kIxThreads) void k_abund_totals(const uint32_t* __restrict__ abund, const long long* __restrict__ offsets,
                                                             int64_t n, unsigned long long* __restrict__ sum,
                                                             unsigned long long* __restrict__ sumsq_lo,
                                                             unsigned long long* __restrict__ sumsq_hi) {
    __shared__ unsigned long long part[kIxWaves][3];
    for (int64_t s = blockIdx.x; s < n; s += gridDim.x) {
        const long long b = offsets[s], e = offsets[s + 1];
        unsigned long long t = 0, lo = 0, hi = 0;
        for (long long i = b + threadIdx.x; i < e; i += kIxThreads) {
            const unsigned long long a = abund[i], q = a * a;
            t += a;
            lo += q & 0xffffffffULL;
            hi += q >> 32;
        }
        t = wave_sum(t);
        lo = wave_sum(lo);
        hi = wave_sum(hi);
        if ((threadIdx.x & 63) == 0) {
            part[threadIdx.x >> 6][0] = t;
            part[threadIdx.x >> 6][1] = lo;
            part[threadIdx.x >> 6][2] = hi;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long tot[3] = {0, 0, 0};
            for (int w = 0; w < kIxWaves; ++w)
                for (int k = 0; k < 3; ++k) tot[k] += part[w][k];
            if (sum) sum[s] = tot[0];
            if (sumsq_lo) sumsq_lo[s] = tot[1];
            if (sumsq_hi) sumsq_hi[s] = tot[2];
        }
        __syncthreads();
    }
}

}  // namespace

int launch_overlap_units(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, const long long* d_unit_start, long long n_units,
                         const unsigned long long* d_hash_r, const long long* d_off_r, const int32_t* d_size_r, const uint32_t* d_ab_r,
                         const unsigned long long* d_hash_c, const long long* d_off_c, const int32_t* d_size_c, const uint32_t* d_ab_c,
                         int unit, mvs_abund_overlap* d_out) {
    if (n_units <= 0) return 0;
    const dim3 grid(ix_grid(n_units, kIxWaves)), block(kIxThreads);
#define MVS_OVERLAP_LAUNCH(R, C)                                                                                              \
    hipLaunchKernelGGL((k_overlap_units<R, C>), grid, block, 0, stream, d_cells, n_cells, d_unit_start, n_units, d_hash_r, d_off_r, \
                       d_size_r, d_ab_r, d_hash_c, d_off_c, d_size_c, d_ab_c, unit, d_out)
    if (d_ab_r && d_ab_c) MVS_OVERLAP_LAUNCH(true, true);
    else if (d_ab_r) MVS_OVERLAP_LAUNCH(true, false);
    else if (d_ab_c) MVS_OVERLAP_LAUNCH(false, true);
    else MVS_OVERLAP_LAUNCH(false, false);
#undef MVS_OVERLAP_LAUNCH
    return 0;
}

int launch_abund_totals(hipStream_t stream, const uint32_t* d_abund, const long long* d_offsets, int64_t n, unsigned long long* d_sum,
                        unsigned long long* d_sumsq_lo, unsigned long long* d_sumsq_hi) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_abund_totals, dim3(ix_grid(n, 1)), dim3(kIxThreads), 0, stream, d_abund, d_offsets, n, d_sum, d_sumsq_lo,
                       d_sumsq_hi);
    return 0;
}

}  // namespace mvs
