// mvs_core.hip -- the core similarity of HDBSCAN* (mvs_core_jaccard): the K-th best Jaccard estimate of every sample, reduced on
// the device from the cell list mvs_pairwise_topk leaves there.
//
// Contract (include/mvs_hip.h "HDBSCAN*").  core[i] is the K-th best score of row i under mvs_pairwise_topk's rule with every
// column eligible but i itself: the minimum, by topk_key, of the fp64 J of the K cells top-k returns for the row.  J is
// recomputed from the cell's dot and the norms in the contract's order (inter = (double)P / d; J = inter / (n2[row] + n2[col] -
// inter)) -- the expression k_topk_select ranked the cell by -- and -0.0 is folded into +0.0.  A row with fewer than K cells
// (its scores are NaN) has core = NaN.  Which K cells top-k returns among equal scores depends on the column rule; their
// minimum does not: it is the K-th largest value of the row's multiset of scores.
//
// The list is ragged (a row has 0 .. K cells) and sorted by (row, col), so the cells of a row are neighbours.  k_core_kth gives
// every cell a lane and reduces inside the wave by segments: log2(64) steps of "take the value 2^s lanes up if it belongs to my
// row" leave in the first lane of every run of equal rows the minimum key and the number of cells of that run (a run is an
// interval: if lane i + 2^s has my row, so has every lane between; by induction lane i holds its run's [i, i + 2^(s+1)) part
// after step s).  The run's first lane then issues one 64-bit atomic min and one atomic add for its row -- a row whose cells
// straddle a wave or a grid-stride trip gets one pair per piece.  A minimum and a sum over a set are what they are whatever the
// interleaving.  key() is a bijection on the non-NaN doubles with -0.0 folded, so k_core_finish turns the minimum key back into
// the double; the count decides NaN.  No cell crosses the link.
#include "mvs_core.h"

namespace mvs {

namespace {

constexpr int kCoreThreads = 256;

// mvs_topk.hip's topk_key and its inverse
__device__ __forceinline__ unsigned long long core_key(double J) {
    if (J == 0.0) J = 0.0;                                          // -0.0 -> +0.0
    const unsigned long long u = (unsigned long long)__double_as_longlong(J);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double core_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// d_keys: all ones, d_counts: 0 on entry (rows entries each).  Every lane makes every trip: the shuffles are whole.
__global__ __launch_bounds__(kCoreThreads) void k_core_kth(const mvs_cell* __restrict__ cells, int64_t n_cells, int64_t row0, int64_t rows,
                                                         const double* __restrict__ norms_sq, int64_t n, int d,
                                                         unsigned long long* __restrict__ keys, int* __restrict__ counts) {
    const int64_t stride = (int64_t)gridDim.x * kCoreThreads;
    const int64_t trips = (n_cells + stride - 1) / stride;
    const int lane = (int)(threadIdx.x & 63);
    int64_t e = (int64_t)blockIdx.x * kCoreThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, e += stride) {
        int64_t seg = -1;                                           // the row's index in the range; -1: no cell, or one outside it
        unsigned long long key = ~0ULL;
        int cnt = 0;
        if (e < n_cells) {
            const mvs_cell c = cells[e];
            const int64_t r = (int64_t)c.row - row0;
            if (r >= 0 && r < rows && c.col >= 0 && c.col < n) {
                const double inter = (double)c.dot / (double)d;
                const double J = inter / (norms_sq[c.row] + norms_sq[c.col] - inter);
                if (J == J) {                                       // (top-k selects no NaN; one would not count)
                    seg = r;
                    key = core_key(J);
                    cnt = 1;
                }
            }
        }
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long okey = __shfl_down(key, (unsigned)off, 64);
            const int ocnt = __shfl_down(cnt, (unsigned)off, 64);
            const long long oseg = __shfl_down((long long)seg, (unsigned)off, 64);
            if (lane + off < 64 && oseg == seg) {
                key = okey < key ? okey : key;
                cnt += ocnt;
            }
        }
        const long long before = __shfl_up((long long)seg, 1u, 64);
        if (seg >= 0 && (lane == 0 || before != seg)) {
            atomicMin(keys + seg, key);
            atomicAdd(counts + seg, cnt);
        }
    }
}

__global__ __launch_bounds__(kCoreThreads) void k_core_finish(const unsigned long long* __restrict__ keys, const int* __restrict__ counts,
                                                            int64_t rows, int k, double* __restrict__ core) {
    for (int64_t i = (int64_t)blockIdx.x * kCoreThreads + threadIdx.x; i < rows; i += (int64_t)gridDim.x * kCoreThreads)
        core[i] = counts[i] >= k ? core_unkey(keys[i]) : __longlong_as_double(0x7ff8000000000000LL);
}

// one workgroup per CU of the largest part: the pass streams 16 bytes per cell once and is a small fraction of the selection
// that produced the list; a list of more than 65536 cells takes further grid-stride trips (300 rows at k = 256 do: tests)
unsigned core_grid(int64_t items) {
    const int64_t blocks = (items + kCoreThreads - 1) / kCoreThreads;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, 256));
}

}  // namespace

// d_core: the entry of row row0 (the caller passes core + row0)
int launch_core_kth(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, int64_t row0, int64_t rows, int k,
                    const double* d_norms_sq, int64_t n, int d, unsigned long long* d_keys, int* d_counts, double* d_core) {
    if (rows <= 0) return 0;
    if (n_cells < 0 || k < 1 || d <= 0 || row0 < 0 || row0 + rows > n) return MVS_E_INVALID;
    if (hipMemsetAsync(d_keys, 0xff, (size_t)rows * sizeof(unsigned long long), stream) != hipSuccess) return MVS_E_HIP;
    if (hipMemsetAsync(d_counts, 0, (size_t)rows * sizeof(int), stream) != hipSuccess) return MVS_E_HIP;
    if (n_cells > 0)
        hipLaunchKernelGGL(k_core_kth, dim3(core_grid(n_cells)), dim3(kCoreThreads), 0, stream, d_cells, n_cells, row0, rows, d_norms_sq, n, d,
                           d_keys, d_counts);
    hipLaunchKernelGGL(k_core_finish, dim3(core_grid(rows)), dim3(kCoreThreads), 0, stream, d_keys, d_counts, rows, k, d_core);
    return 0;
}

}  // namespace mvs
