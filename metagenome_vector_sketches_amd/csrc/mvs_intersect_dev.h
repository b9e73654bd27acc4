// mvs_intersect_dev.h -- device code that the units-of-work kernels over sorted hash lists share (mvs_intersect.hip: counting
// |A n B|; mvs_overlap.hip: summing abundances over it; mvs_gather.hip: marking the positions of Q that lie in H): the geometry
// of a unit, the wave-wide search, the decoding of a unit (unit_of) and the walk over its matches (walk_unit), the wave sum and
// the grid of a launch.  What a kernel adds is its sink -- what a lane does with a match -- and its ending.  DESIGN.md §12.
#ifndef MVS_INTERSECT_DEV_H
#define MVS_INTERSECT_DEV_H

#include "mvs_internal.h"

namespace mvs {
namespace {

constexpr int kIxThreads = 256;                // 4 waves: 4 units in flight per workgroup
constexpr int kIxWaves = kIxThreads / 64;
constexpr int kTile = 1024;                    // elements of B a wave stages in LDS at a time (8 KiB per wave)
constexpr int kSkew = 32;                      // window / chunk ratio from which the window is searched in place

// First index i in [lo, hi) with !(arr[i] < key) (upper == false) or !(arr[i] <= key) (upper == true); hi if there is none.
// arr is non-decreasing on [lo, hi).  The whole wave calls it with the same arguments and gets the same answer.
template <typename T, typename I>
__device__ __forceinline__ I wave_bound(const T* __restrict__ arr, I lo, I hi, T key, bool upper, int lane) {
    // invariant: the answer lies in [lo, hi] (hi included)
    while (hi - lo > 64) {
        const I n = hi - lo;
        const I step = (n + 63) / 64;                                  // >= 2
        const I pos = lo + (I)(lane + 1) * step - 1;                   // splitter of this lane
        bool below = false;
        if (pos < hi) {
            const T v = arr[pos];
            below = upper ? (v <= key) : (v < key);
        }
        const int k = __popcll(__ballot(below));                       // splitters 0 .. k-1 are below: a prefix
        const I nlo = lo + (I)k * step;
        const I nhi = lo + (I)(k + 1) * step - 1;                      // splitter k is not below (if it exists)
        lo = nlo < hi ? nlo : hi;
        hi = (k < 64 && nhi < hi) ? nhi : hi;
    }
    bool below = false;
    const I pos = lo + (I)lane;
    if (pos < hi) {
        const T v = arr[pos];
        below = upper ? (v <= key) : (v < key);
    }
    return lo + (I)__popcll(__ballot(below));
}

// a wave's tile in LDS is final (or free again): its lanes run in lockstep, the compiler orders LDS stores and loads
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the sum of v over the wave, in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// workgroups of a grid-stride launch over `items`, per_block of them to a workgroup
inline unsigned ix_grid(int64_t items, int per_block) {
    const int64_t blocks = (items + per_block - 1) / per_block;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, 1 << 20));
}

// One unit of work: chunk [a0, a1) of A, the shorter list of the cell's two, against B's window [w0, w1), which holds everything
// that can equal an element of the chunk.  The same in every lane of the wave that owns the unit.
struct IxUnit {
    int64_t cell;                          // index into cells[] (and into the results)
    int32_t row, col;                      // its samples
    bool row_short;                        // A is the row's list (also on a tie: the rule of k_isect_count), B the column's
    long long at_a, at_b;                  // where A / B starts in its set's arrays
    const unsigned long long *A, *B;
    int32_t a0, a1;                        // a0 < a1 <= |A|
    int32_t w0, w1;
};

// unit u of the units that isect_plan laid out (unit_start: the scanned units per cell, n_cells + 1 entries) with `unit`
// elements of A to a unit.  The whole wave calls it with the same arguments.
__device__ __forceinline__ IxUnit unit_of(const mvs_cell* __restrict__ cells, int64_t n_cells, const long long* __restrict__ unit_start,
                                          long long u, const unsigned long long* __restrict__ hash_r,
                                          const long long* __restrict__ off_r, const int32_t* __restrict__ size_r,
                                          const unsigned long long* __restrict__ hash_c, const long long* __restrict__ off_c,
                                          const int32_t* __restrict__ size_c, int unit, int lane) {
    IxUnit n;
    // the unit's cell: the last one whose first unit is <= u (cells without units share their successor's start)
    n.cell = wave_bound<long long, int64_t>(unit_start, 0, n_cells + 1, u, true, lane) - 1;
    n.row = cells[n.cell].row, n.col = cells[n.cell].col;
    const int32_t lr = size_r[n.row], lc = size_c[n.col];
    n.row_short = lr <= lc;
    // (each offset is loaded where its list is chosen: with both loaded ahead of the choice k_isect_units ran 1.2 % slower)
    n.at_a = n.row_short ? off_r[n.row] : off_c[n.col];
    n.at_b = n.row_short ? off_c[n.col] : off_r[n.row];
    n.A = (n.row_short ? hash_r : hash_c) + n.at_a;
    n.B = (n.row_short ? hash_c : hash_r) + n.at_b;
    const int32_t la = n.row_short ? lr : lc, lb = n.row_short ? lc : lr;
    const long long chunk = u - unit_start[n.cell];
    n.a0 = (int32_t)(chunk * unit);
    n.a1 = (int32_t)(((long long)n.a0 + unit < la) ? (long long)n.a0 + unit : la);
    n.w0 = wave_bound<unsigned long long, int32_t>(n.B, 0, lb, n.A[n.a0], false, lane);
    n.w1 = wave_bound<unsigned long long, int32_t>(n.B, n.w0, lb, n.A[n.a1 - 1], true, lane);
    return n;
}

// Every element of the chunk is looked up in the window, one element to a lane, and sink(x, y, hit) hears of it: x its position
// in A, y where B holds the same value if hit.  The window is staged in the wave's LDS tile (kTile elements) piece by piece; one
// more than kSkew times longer than the chunk (3 hashes against 300 000) is searched where it lies instead, |A| log |B| probes
// for |B| loads.
// kWhole = false: the sink is called for the matches only (hit is true), by the lanes that found them; a lane steps through its
// own positions p.
// kWhole = true: every lane calls the sink on every trip, so that a sink may ballot: the trips are groups of 64 positions on the
// grid of a0, p is a group's first one (the same in every lane: lane 0 stands there) and hit is false where x lies outside the
// trip's elements.  A group that straddles two tiles is visited by both, each with its own elements.
// (Both forms are measured: whole groups for everybody cost k_overlap_units 3.5 %, and a loop on p + lane < end for the first
// form is 0.5 % slower there -- profiles/README.md, "unit walk".)
template <bool kWhole, typename Sink>
__device__ __forceinline__ void walk_unit(const IxUnit& n, unsigned long long* tile, int lane, Sink&& sink) {
    const unsigned long long *A = n.A, *B = n.B;
    const int32_t a0 = n.a0, a1 = n.a1, w0 = n.w0, w1 = n.w1;
    if ((long long)(w1 - w0) > (long long)kSkew * (a1 - a0)) {
        // a long window for a few elements: search it where it lies
        for (int32_t p = kWhole ? a0 : a0 + lane; p < a1; p += 64) {
            const int32_t x = kWhole ? p + lane : p;
            bool hit = false;
            int32_t l = w0;
            if (!kWhole || x < a1) {
                const unsigned long long key = A[x];
                int32_t h = w1;
                while (l < h) {
                    const int32_t mid = l + ((h - l) >> 1);
                    if (B[mid] < key) l = mid + 1;
                    else h = mid;
                }
                hit = l < w1 && B[l] == key;
            }
            if (kWhole || hit) sink(x, l, hit);
        }
    } else {
        int32_t a = a0;                                                // elements of the chunk before a are settled
        for (int32_t t0 = w0; t0 < w1 && a < a1; t0 += kTile) {
            const int tn = (w1 - t0 < kTile) ? (w1 - t0) : kTile;
            for (int j = lane; j < tn; j += 64) tile[j] = B[t0 + j];
            wave_lds_sync();
            // the chunk's elements up to the tile's last one can only match inside this tile (B's earlier tiles are below the
            // elements from a on: those were not <= the previous tile's last element)
            const int32_t ae = wave_bound<unsigned long long, int32_t>(A, a, a1, tile[tn - 1], true, lane);
            for (int32_t p = kWhole ? a0 + ((a - a0) & ~63) : a + lane; p < ae; p += 64) {
                const int32_t x = kWhole ? p + lane : p;
                bool hit = false;
                int l = 0;
                if (!kWhole || (x >= a && x < ae)) {
                    const unsigned long long key = A[x];
                    int h = tn;
                    while (l < h) {
                        const int mid = (l + h) >> 1;
                        if (tile[mid] < key) l = mid + 1;
                        else h = mid;
                    }
                    hit = l < tn && tile[l] == key;
                }
                if (kWhole || hit) sink(x, t0 + l, hit);
            }
            a = ae;
            wave_lds_sync();                                           // the next tile overwrites what the lanes just read
        }
    }
}

}  // namespace
}  // namespace mvs

#endif
