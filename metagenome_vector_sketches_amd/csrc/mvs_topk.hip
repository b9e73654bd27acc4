// mvs_topk.hip -- exact k-nearest-neighbour selection over blocks of int32 dots (mvs_pairwise_topk).
//
// The comparison kernels answer "which cells pass the keep test"; this unit answers "which k columns of a row score best".
// The dots of a row block come from the existing dense-dots kernels (launch_pairwise mode 1: the int8 matrix cores for one,
// two-limb and K3 sets, the vector-ALU kernel otherwise) into a scratch block of R rows x C columns; k_topk_select then ranks
// every cell of a row and keeps the best k, k_topk_compact packs the rows' lists into the caller's cell array.
//
// Score and order (the contract of mvs_pairwise_topk, include/mvs_hip.h).  The score of a cell is the writer's Jaccard BEFORE
// its clamp, fp64, in quantize_cell's order: inter = (double)P / d; J = inter / (n2_row + n2_col - inter)
// (src/pairwise_comp_optimized.cpp:661-662).  Cells are ranked by J descending, equal J by the smaller column; a NaN J is never
// selected, +-inf are ordinary values.  A cell is ranked by the pair (key(J), col) with key() the order-preserving map of a
// double onto an unsigned 64-bit integer (sign bit set: all bits flipped; clear: the sign bit set).  -0.0 is folded into +0.0
// first, so that the two zeros -- equal as doubles -- tie and fall to the column rule.  key() of any non-NaN double is >= 1
// (-inf maps to 0x000fffffffffffff), so the pair (0, INT_MAX) is below every real cell: the sentinel of empty slots.
//
// Selection, and why it is exact.  A workgroup owns one row.  It walks the row's C columns in rounds of kRound, and every
// cell that beats the row's threshold tau goes into a candidate buffer in LDS (kCap entries).  When the buffer holds more than
// kCap - kRound entries it is flushed: sorted best first (bitonic, kCap entries), cut to its best min(count, k), and -- if k
// entries remain -- tau becomes the k-th of them.  Invariant: the buffer always contains the best min(k, seen) cells of the
// columns seen so far.  It holds at the start (empty, nothing seen).  A round keeps it: a cell that does not beat tau is
// worse than k cells already in the buffer, so it is not among the best k of the columns seen, now or later; every other cell
// is appended.  A flush keeps it: it discards only cells with k better ones in the buffer.  tau only ever rises (it is the
// k-th best of a set that only gains members), so the argument holds round after round.  Room: a round starts with at most
// kCap - kRound entries (more are flushed down to k <= 256 <= kCap - kRound) and appends at most kRound, so the buffer never
// overflows (kCap = 2048, kRound = 1024).  After the last round one more
// flush leaves the best min(k, eligible) cells; they are re-sorted by column and written with their dot and q.
// Nothing depends on the order in which a round's threads append (the buffer is a set until it is sorted, and the sort's
// order is total: columns are distinct), nor on how rows are blocked, so the result is bit-identical to a brute force.
#include "mvs_internal.h"
#include "mvs_pairwise_dev.h"

#include <climits>

namespace mvs {

namespace {

constexpr int kTopkThreads = 256;
constexpr int kTopkPer = 4;                          // columns per thread and round
constexpr int kRound = kTopkThreads * kTopkPer;      // columns per round
constexpr int kCap = 2048;                           // candidate buffer (entries)
static_assert(kMaxTopk <= kCap - kRound, "a flushed buffer must take a whole round");

__device__ __forceinline__ unsigned long long topk_key(double J) {
    if (J == 0.0) J = 0.0;                                          // -0.0 -> +0.0
    const unsigned long long u = (unsigned long long)__double_as_longlong(J);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// (ka, ca) ranks before (kb, cb)
__device__ __forceinline__ bool topk_better(unsigned long long ka, int ca, unsigned long long kb, int cb) {
    return ka > kb || (ka == kb && ca < cb);
}

// Bitonic sort of n (a power of two, <= kCap) LDS entries with the whole workgroup: best first (BY_COL = false) or by
// ascending column (BY_COL = true).  Every thread calls it; it ends with a barrier.
template <bool BY_COL>
__device__ __forceinline__ void topk_sort(unsigned long long* keys, int* cols, int n) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += kTopkThreads) {
                const int i = 2 * t - (t & (stride - 1));
                const int j = i + stride;
                const bool first_half = (i & size) == 0;            // this half-sequence runs best first / ascending
                const unsigned long long ki = keys[i], kj = keys[j];
                const int ci = cols[i], cj = cols[j];
                const bool j_first = BY_COL ? (cj < ci) : topk_better(kj, cj, ki, ci);
                if (j_first == first_half) {
                    keys[i] = kj;
                    keys[j] = ki;
                    cols[i] = cj;
                    cols[j] = ci;
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ void topk_flush(unsigned long long* keys, int* cols, int n, int k, int* cnt,
                                           unsigned long long* tau_key, int* tau_col) {
    for (int i = n + (int)threadIdx.x; i < kCap; i += kTopkThreads) {
        keys[i] = 0ull;
        cols[i] = INT_MAX;
    }
    __syncthreads();
    topk_sort<false>(keys, cols, kCap);
    if (threadIdx.x == 0) {
        *cnt = n < k ? n : k;
        if (n >= k) {
            *tau_key = keys[k - 1];
            *tau_col = cols[k - 1];
        }
    }
    __syncthreads();
}

// One workgroup per row of the block.  dots: rows x ld int32 (row r of the block is sample row0 + r, column j is sample
// c0 + j, ld = c1 - c0); out: k cells per row starting at row out_row0 of the call's padded list; counts: cells per row.
__global__ __launch_bounds__(kTopkThreads) void k_topk_select(const int32_t* __restrict__ dots, int64_t ld, int64_t row0,
                                                              int64_t c0, const double* __restrict__ norms_sq, int d, int k,
                                                              int exclude_self, mvs_cell* __restrict__ out,
                                                              int* __restrict__ counts, int64_t out_row0) {
    __shared__ unsigned long long keys[kCap];
    __shared__ int cols[kCap];
    __shared__ int cnt;
    __shared__ unsigned long long tau_key;
    __shared__ int tau_col;
    const int64_t r = blockIdx.x;
    const int64_t row = row0 + r;
    const int32_t* __restrict__ dp = dots + r * ld;
    const double n2r = norms_sq[row];
    const double dd = (double)d;
    if (threadIdx.x == 0) {
        cnt = 0;
        tau_key = 0ull;                                  // the sentinel: every real cell beats it
        tau_col = INT_MAX;
    }
    __syncthreads();
    for (int64_t base = 0; base < ld; base += kRound) {
        const unsigned long long tk = tau_key;
        const int tc = tau_col;
        int32_t P[kTopkPer];
#pragma unroll
        for (int u = 0; u < kTopkPer; ++u) {
            const int64_t j = base + u * kTopkThreads + threadIdx.x;
            P[u] = j < ld ? dp[j] : 0;
        }
#pragma unroll
        for (int u = 0; u < kTopkPer; ++u) {
            const int64_t j = base + u * kTopkThreads + threadIdx.x;
            if (j >= ld) continue;
            const int64_t col = c0 + j;
            if (exclude_self && col == row) continue;
            const double inter = (double)P[u] / dd;                        // :661
            const double J = inter / (n2r + norms_sq[col] - inter);        // :662
            if (!(J == J)) continue;
            const unsigned long long key = topk_key(J);
            if (topk_better(key, (int)col, tk, tc)) {
                const int pos = atomicAdd(&cnt, 1);
                keys[pos] = key;
                cols[pos] = (int)col;
            }
        }
        __syncthreads();
        const int n = cnt;
        __syncthreads();                                 // every thread has read cnt before anybody changes it
        if (n > kCap - kRound) topk_flush(keys, cols, n, k, &cnt, &tau_key, &tau_col);
    }
    const int n_all = cnt;
    __syncthreads();
    topk_flush(keys, cols, n_all, k, &cnt, &tau_key, &tau_col);
    const int m = cnt;                                   // min(k, eligible columns)
    int p = 1;
    while (p < m) p <<= 1;
    for (int i = m + (int)threadIdx.x; i < p; i += kTopkThreads) cols[i] = INT_MAX;
    __syncthreads();
    topk_sort<true>(keys, cols, p);                      // the winners by ascending column (:718-722)
    for (int i = threadIdx.x; i < m; i += kTopkThreads) {
        const int col = cols[i];
        const int32_t P = dp[col - c0];
        mvs_cell c;
        c.row = (int32_t)row;
        c.col = col;
        c.dot = P;
        c.q = quantize_cell(P, d, n2r, norms_sq[col]);
        out[(row - out_row0) * k + i] = c;
    }
    if (threadIdx.x == 0) counts[row - out_row0] = m;
}

// padded lists (k slots per row) -> consecutive cells; offs = exclusive scan of the rows' counts
__global__ __launch_bounds__(256) void k_topk_compact(const mvs_cell* __restrict__ pad, const int* __restrict__ counts,
                                                      const int64_t* __restrict__ offs, int64_t rows, int k,
                                                      mvs_cell* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * k) return;
    const int64_t r = i / k;
    const int j = (int)(i - r * k);
    if (j < counts[r]) out[offs[r] + j] = pad[i];
}

}  // namespace

int launch_topk_select(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                       const double* d_norms_sq, int d, int k, int exclude_self, mvs_cell* d_pad, int* d_counts,
                       int64_t out_row0) {
    if (rows <= 0) return 0;
    if (k < 1 || k > kMaxTopk || ld <= 0 || ld > INT_MAX || rows > INT_MAX) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_topk_select, dim3((unsigned)rows), dim3(kTopkThreads), 0, stream, d_dots, ld, row0, c0, d_norms_sq, d,
                       k, exclude_self, d_pad, d_counts, out_row0);
    return 0;
}

int launch_topk_compact(hipStream_t stream, const mvs_cell* d_pad, const int* d_counts, const int64_t* d_offs, int64_t rows,
                        int k, mvs_cell* d_out) {
    const int64_t n = rows * (int64_t)k;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_topk_compact, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_pad, d_counts, d_offs, rows, k,
                       d_out);
    return 0;
}

}  // namespace mvs
