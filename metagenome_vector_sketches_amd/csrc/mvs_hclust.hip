// mvs_hclust.hip -- average (UPGMA) and complete linkage on a resident m x m table of integer sums (include/mvs_hip.h "Average
// and complete linkage"; the rounds are driven from mvs_capi_hclust.hip).  Everything is integer: a table entry is the sum (or
// the maximum) of the fixed-point weights of mvs_weight_dev.h over the cross pairs of two clusters, a merge adds two columns
// and two rows, and the nearest column of a row is chosen by an exact comparison, so no order of blocks or lanes shows in a
// record.
//
// Layout.  Row s of the table belongs to slot s for good; the COLUMNS follow a layout (HclustState) that drops its dead columns
// at a compaction.  Rows are ld entries apart, ld even, so every row starts on 16 bytes and a lane loads two entries at once.
//
// k_hclust_fill      a block of int32 dots -> rows of the table: quantised_distance per cell, the function k_dist_quantise calls.
// k_hclust_nearest   one workgroup per live row, the hot pass: it reads the row's live layout once per round.  A lane takes two
//                    columns per trip (one 16-byte load of the table, 8 bytes each of col_n and col_slot, which every row shares
//                    and the cache holds) and keeps its best (sum, n, column); the key -- two 64-bit multiplies -- is taken
//                    only where two values are EQUAL.  For average the values compare as sum1 * n2 against sum2 * n1 in 128
//                    bits (two mul_hi); equal sizes, the whole first round, compare the sums alone.  Then six shuffle steps and
//                    one pass through LDS over the four waves.
// k_hclust_pairs     one workgroup.  It walks the live list, ascending in slot, 1024 rows per trip, and scans two flags: "a
//                    mutual pair's smaller slot" numbers the records and the pair list, "does not die" the next live list --
//                    the (round, a) order of the records by construction, no atomics.  The pair's thread writes the record, the
//                    new size and the two col_n entries: nobody else touches them.
// k_hclust_merge_cols / _rows   the two phases of the contract, two launches: one workgroup per live row (the dying ones
//                    included) runs over the pairs, then one workgroup per pair runs over the layout's columns, two per lane.
//                    Dead and padding columns are folded too: nobody reads them again.
// k_hclust_layout / _compact    one workgroup scans col_n for the live columns and rewrites the layout in place; then one
//                    workgroup per live row moves its entries in ascending chunks, read -- barrier -- write: a destination
//                    j never lies behind its source keep[j] >= j, so a chunk overwrites nothing a later chunk still reads.
#include "mvs_hclust.h"
#include "mvs_weight_dev.h"

#include <algorithm>
#include <climits>
#include <type_traits>

namespace mvs {

namespace {

constexpr int kRowThreads = 256;          // a workgroup of the per-row kernels
constexpr int kScanThreads = 1024;        // the single workgroup of the scans
constexpr uint32_t kNone = 0xffffffffu;

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

__device__ __forceinline__ unsigned long long pair_key(uint32_t r, uint32_t c) {
    const uint32_t lo = r < c ? r : c, hi = r < c ? c : r;
    return splitmix64(((unsigned long long)lo << 32) | hi);
}

// sign of s1 / n1 - s2 / n2, exact: the cross products in 128 bits
__device__ __forceinline__ int compare_means(unsigned long long s1, uint32_t n1, unsigned long long s2, uint32_t n2) {
    if (n1 == n2) return s1 < s2 ? -1 : (s1 > s2 ? 1 : 0);
    const unsigned long long l1 = s1 * n2, h1 = __umul64hi(s1, (unsigned long long)n2);
    const unsigned long long l2 = s2 * n1, h2 = __umul64hi(s2, (unsigned long long)n1);
    if (h1 != h2) return h1 < h2 ? -1 : 1;
    return l1 < l2 ? -1 : (l1 > l2 ? 1 : 0);
}

// a row's best column so far; the key is taken when a tie first asks for it
template <int METHOD>
struct Best {
    unsigned long long sum, key;
    uint32_t n, slot;
    bool keyed;
    __device__ __forceinline__ int compare(unsigned long long s, uint32_t m) const {
        if (METHOD == MVS_HCLUST_COMPLETE) return s < sum ? -1 : (s > sum ? 1 : 0);
        return compare_means(s, m, sum, n);
    }
    __device__ __forceinline__ void offer(uint32_t row, unsigned long long s, uint32_t m, uint32_t c) {
        if (slot == kNone) {
            sum = s, n = m, slot = c, keyed = false;
            return;
        }
        const int o = compare(s, m);
        if (o > 0) return;
        if (o < 0) {
            sum = s, n = m, slot = c, keyed = false;
            return;
        }
        if (!keyed) key = pair_key(row, slot), keyed = true;
        const unsigned long long k = pair_key(row, c);
        if (k < key) sum = s, n = m, slot = c, key = k;
    }
    // another lane's best, its key already taken
    __device__ __forceinline__ void merge(unsigned long long s, uint32_t m, uint32_t c, unsigned long long k) {
        if (c == kNone) return;
        if (slot != kNone) {
            const int o = compare(s, m);
            if (o > 0 || (o == 0 && key < k)) return;
        }
        sum = s, n = m, slot = c, key = k;
    }
};

template <int METHOD>
__global__ __launch_bounds__(kRowThreads) void k_hclust_nearest(const unsigned long long* __restrict__ table, int64_t ld,
                                                                const int32_t* __restrict__ col_slot, const uint32_t* __restrict__ col_n,
                                                                const int32_t* __restrict__ live, int64_t n_cols, int32_t* __restrict__ nearest) {
    __shared__ unsigned long long s_sum[kRowThreads / 64], s_key[kRowThreads / 64];
    __shared__ uint32_t s_n[kRowThreads / 64], s_slot[kRowThreads / 64];
    const uint32_t row = (uint32_t)live[blockIdx.x];
    const ulonglong2* __restrict__ cells = reinterpret_cast<const ulonglong2*>(table + (int64_t)row * ld);
    const uint2* __restrict__ sizes = reinterpret_cast<const uint2*>(col_n);
    const int2* __restrict__ slots = reinterpret_cast<const int2*>(col_slot);
    const int64_t duos = (n_cols + 1) >> 1;                      // (an odd layout's padding column has col_n = 0)
    Best<METHOD> best{0ULL, 0ULL, 0u, kNone, false};
    for (int64_t q = threadIdx.x; q < duos; q += kRowThreads) {
        const ulonglong2 v = cells[q];
        const uint2 m = sizes[q];
        const int2 c = slots[q];
        if (m.x != 0u && (uint32_t)c.x != row) best.offer(row, v.x, m.x, (uint32_t)c.x);
        if (m.y != 0u && (uint32_t)c.y != row) best.offer(row, v.y, m.y, (uint32_t)c.y);
    }
    if (best.slot != kNone && !best.keyed) best.key = pair_key(row, best.slot);
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long os = __shfl_xor(best.sum, off, 64), ok = __shfl_xor(best.key, off, 64);
        const uint32_t om = __shfl_xor(best.n, off, 64), oc = __shfl_xor(best.slot, off, 64);
        best.merge(os, om, oc, ok);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_sum[wave] = best.sum, s_key[wave] = best.key, s_n[wave] = best.n, s_slot[wave] = best.slot;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kRowThreads / 64; ++w) best.merge(s_sum[w], s_n[w], s_slot[w], s_key[w]);
        nearest[row] = (int32_t)best.slot;                       // (-1 only for the last live row, which is never asked)
    }
}

// exclusive prefix of v over the workgroup of kScanThreads, its total in *total; lds: kScanThreads / 64 ints
__device__ __forceinline__ int block_scan(int v, int* total, int* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, (unsigned)off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kScanThreads / 64; ++w) {
        const int t = lds[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + x - v;
}

template <int METHOD>
__global__ __launch_bounds__(kScanThreads) void k_hclust_pairs(HclustState st, const int32_t* __restrict__ live, int32_t* __restrict__ live_next,
                                                               int64_t n_live, int round, int64_t done) {
#pragma clang fp contract(off)
    __shared__ int lds[kScanThreads / 64];
    int n_pairs = 0, n_next = 0;
    for (int64_t i0 = 0; i0 < n_live; i0 += kScanThreads) {
        const int64_t i = i0 + threadIdx.x;
        const bool valid = i < n_live;
        int32_t a = -1, b = -1;
        bool mutual = false;
        if (valid) {
            a = live[i];
            b = st.nearest[a];
            mutual = b >= 0 && st.nearest[b] == a;
        }
        const bool leads = mutual && a < b, stays = valid && !(mutual && a > b);
        int total = 0;
        const int at = block_scan((leads ? 1 : 0) | (stays ? 1 << 16 : 0), &total, lds);   // (each count <= 1024 < 2^16)
        if (leads) {
            const int64_t p = n_pairs + (at & 0xffff);
            const int32_t na = st.size[a], nb = st.size[b];
            const int32_t ca = st.slot_col[a], cb = st.slot_col[b];
            const unsigned long long sum = st.table[(int64_t)a * st.ld + cb];
            double h;
            if (METHOD == MVS_HCLUST_COMPLETE) {
                h = (double)sum * 0x1p-30;
            } else {
                const double cross = (double)na * (double)nb;
                const double mean = (double)sum / cross;
                h = mean * 0x1p-30;
            }
            mvs_hmerge rec;
            rec.a = a, rec.b = b, rec.round = round, rec.size = na + nb, rec.sum = sum, rec.height = h;
            st.merges[done + p] = rec;
            st.pairs[2 * p] = a;
            st.pairs[2 * p + 1] = b;
            st.size[a] = na + nb;
            st.col_n[ca] = (uint32_t)(na + nb);
            st.col_n[cb] = 0u;
        }
        if (stays) live_next[n_next + (at >> 16)] = a;
        n_pairs += total & 0xffff;
        n_next += total >> 16;
    }
    if (threadIdx.x == 0) {
        st.counters[0] = n_pairs;
        st.counters[1] = n_next;
    }
}

template <int METHOD>
__device__ __forceinline__ unsigned long long fold(unsigned long long x, unsigned long long y) {
    return METHOD == MVS_HCLUST_COMPLETE ? (x > y ? x : y) : x + y;
}

template <int METHOD>
__global__ __launch_bounds__(kRowThreads) void k_hclust_merge_cols(unsigned long long* __restrict__ table, int64_t ld,
                                                                   const int32_t* __restrict__ slot_col, const int32_t* __restrict__ pairs,
                                                                   const int32_t* __restrict__ live, int64_t n_pairs) {
    unsigned long long* row = table + (int64_t)live[blockIdx.x] * ld;
    for (int64_t p = threadIdx.x; p < n_pairs; p += kRowThreads) {
        const int32_t ca = slot_col[pairs[2 * p]], cb = slot_col[pairs[2 * p + 1]];
        row[ca] = fold<METHOD>(row[ca], row[cb]);                // the pairs' columns are distinct, and no column b is written
    }
}

template <int METHOD>
__global__ __launch_bounds__(kRowThreads) void k_hclust_merge_rows(unsigned long long* __restrict__ table, int64_t ld,
                                                                   const int32_t* __restrict__ pairs, int64_t n_cols) {
    ulonglong2* into = reinterpret_cast<ulonglong2*>(table + (int64_t)pairs[2 * blockIdx.x] * ld);
    const ulonglong2* from = reinterpret_cast<const ulonglong2*>(table + (int64_t)pairs[2 * blockIdx.x + 1] * ld);
    const int64_t duos = (n_cols + 1) >> 1;
    for (int64_t q = threadIdx.x; q < duos; q += kRowThreads) {
        ulonglong2 x = into[q];
        const ulonglong2 y = from[q];
        x.x = fold<METHOD>(x.x, y.x);
        x.y = fold<METHOD>(x.y, y.y);
        into[q] = x;
    }
}

__global__ __launch_bounds__(kScanThreads) void k_hclust_layout(HclustState st, int64_t n_cols) {
    __shared__ int lds[kScanThreads / 64];
    int n_new = 0;
    for (int64_t j0 = 0; j0 < n_cols; j0 += kScanThreads) {
        const int64_t j = j0 + threadIdx.x;
        int32_t slot = -1;
        uint32_t n = 0u;
        if (j < n_cols) slot = st.col_slot[j], n = st.col_n[j];
        int total = 0;
        const int at = block_scan(n != 0u ? 1 : 0, &total, lds);     // (its barriers stand between these reads and the writes)
        if (n != 0u) {
            const int to = n_new + at;                               // to <= j: behind every column still to be read
            st.col_slot[to] = slot;
            st.col_n[to] = n;
            st.keep[to] = (int32_t)j;
            st.slot_col[slot] = to;
        }
        n_new += total;
    }
    __syncthreads();
    if (threadIdx.x == 0 && (n_new & 1)) st.col_n[n_new] = 0u;       // the padding column of an odd layout
}

__global__ __launch_bounds__(kRowThreads) void k_hclust_compact(unsigned long long* __restrict__ table, int64_t ld, const int32_t* __restrict__ keep,
                                                                const int32_t* __restrict__ live, int64_t n_cols_new) {
    unsigned long long* row = table + (int64_t)live[blockIdx.x] * ld;
    for (int64_t j0 = 0; j0 < n_cols_new; j0 += kRowThreads) {       // (the same trips for every thread: the barrier is whole)
        const int64_t j = j0 + threadIdx.x;
        unsigned long long v = 0ULL;
        if (j < n_cols_new) v = row[keep[j]];
        __syncthreads();
        if (j < n_cols_new) row[j] = v;
    }
}

__global__ __launch_bounds__(kRowThreads) void k_hclust_fill(const int32_t* __restrict__ dots, int64_t m, int64_t row0, int64_t c0,
                                                             const double* __restrict__ n2, double dd, double inv, int pow2, double floor_,
                                                             unsigned long long* __restrict__ rows_out, int64_t ld) {
#pragma clang fp contract(off)
    const int64_t q = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (2 * q >= ld) return;
    const int64_t row = row0 + r;
    const double n2r = n2[row];
    const int32_t* __restrict__ drow = dots + r * m;
    unsigned long long w[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int64_t j = 2 * q + u;
        w[u] = (j >= m || c0 + j == row) ? 0ULL : (unsigned long long)quantised_distance(drow[j], n2r, n2[c0 + j], dd, inv, pow2 != 0, floor_);
    }
    reinterpret_cast<ulonglong2*>(rows_out + r * ld)[q] = make_ulonglong2(w[0], w[1]);
}

__global__ __launch_bounds__(kRowThreads) void k_hclust_widen(const uint32_t* __restrict__ w, int64_t m, unsigned long long* __restrict__ table,
                                                              int64_t ld) {
    const int64_t j = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    const int64_t r = blockIdx.y + (int64_t)blockIdx.z * 32768;
    if (j >= ld || r >= m) return;
    table[r * ld + j] = j < m ? (unsigned long long)w[r * m + j] : 0ULL;
}

// one workgroup per row i, over the columns j > i (the layout is still the identity)
__global__ __launch_bounds__(kRowThreads) void k_hclust_check(const unsigned long long* __restrict__ table, int64_t ld, const int32_t* __restrict__ size,
                                                              int64_t m, int32_t* __restrict__ flags) {
    const int64_t i = blockIdx.x;
    const unsigned long long ni = (unsigned long long)size[i];
    int bad = 0;
    for (int64_t j = i + 1 + threadIdx.x; j < m; j += kRowThreads) {
        const unsigned long long v = table[i * ld + j];
        if (v != table[j * ld + i]) bad |= 1;
        if (v > ((ni * (unsigned long long)size[j]) << 30)) bad |= 2;   // (sizes total <= 2^17: the product is < 2^34)
    }
    if (bad) atomicOr(flags, bad);
}

template <typename F>
int by_method(int method, F&& f) {
    if (method == MVS_HCLUST_AVERAGE) return f(std::integral_constant<int, MVS_HCLUST_AVERAGE>()), 0;
    if (method == MVS_HCLUST_COMPLETE) return f(std::integral_constant<int, MVS_HCLUST_COMPLETE>()), 0;
    return MVS_E_INVALID;
}

}  // namespace

int launch_hclust_fill(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t m, int64_t row0, int64_t c0, const double* d_norms_sq,
                       int d, double floor_, unsigned long long* d_rows, int64_t ld) {
    if (rows <= 0) return 0;
    if (m <= 0 || ld < m || (ld & 1) || ld > INT_MAX || rows > 65535 || row0 < 0 || c0 < 0 || d <= 0 || !(floor_ >= 0.0) || !(floor_ < 1.0))
        return MVS_E_INVALID;
    const int pow2 = (d & (d - 1)) == 0;
    const int64_t duos = ld / 2;
    hipLaunchKernelGGL(k_hclust_fill, dim3((unsigned)((duos + kRowThreads - 1) / kRowThreads), (unsigned)rows), dim3(kRowThreads), 0, stream, d_dots, m,
                       row0, c0, d_norms_sq, (double)d, 1.0 / (double)d, pow2, floor_, d_rows, ld);
    return 0;
}

int launch_hclust_widen(hipStream_t stream, const uint32_t* d_w, int64_t m, unsigned long long* d_table, int64_t ld) {
    if (m <= 0 || ld < m || m > MVS_HCLUST_MAX_TOTAL) return MVS_E_INVALID;
    const unsigned ny = (unsigned)std::min<int64_t>(m, 32768), nz = (unsigned)((m + 32767) / 32768);
    hipLaunchKernelGGL(k_hclust_widen, dim3((unsigned)((ld + kRowThreads - 1) / kRowThreads), ny, nz), dim3(kRowThreads), 0, stream, d_w, m, d_table, ld);
    return 0;
}

int launch_hclust_check(hipStream_t stream, const HclustState& st, int64_t m) {
    if (m <= 1) return 0;
    if (m > MVS_HCLUST_MAX_TOTAL) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_hclust_check, dim3((unsigned)(m - 1)), dim3(kRowThreads), 0, stream, st.table, st.ld, st.size, m, st.counters + 2);
    return 0;
}

int launch_hclust_nearest(hipStream_t stream, const HclustState& st, int method, const int32_t* d_live, int64_t n_live, int64_t n_cols) {
    if (n_live <= 0) return 0;
    if (n_cols <= 0 || n_cols > st.ld || n_live > MVS_HCLUST_MAX_TOTAL) return MVS_E_INVALID;
    return by_method(method, [&](auto M) {
        hipLaunchKernelGGL(k_hclust_nearest<decltype(M)::value>, dim3((unsigned)n_live), dim3(kRowThreads), 0, stream, st.table, st.ld, st.col_slot,
                           st.col_n, d_live, n_cols, st.nearest);
    });
}

int launch_hclust_pairs(hipStream_t stream, const HclustState& st, int method, const int32_t* d_live, int32_t* d_live_next, int64_t n_live,
                        int round, int64_t done) {
    if (n_live <= 0 || n_live > MVS_HCLUST_MAX_TOTAL || done < 0) return MVS_E_INVALID;
    return by_method(method, [&](auto M) {
        hipLaunchKernelGGL(k_hclust_pairs<decltype(M)::value>, dim3(1), dim3(kScanThreads), 0, stream, st, d_live, d_live_next, n_live, round, done);
    });
}

int launch_hclust_merge_cols(hipStream_t stream, const HclustState& st, int method, const int32_t* d_live, int64_t n_live, int64_t n_pairs) {
    if (n_live <= 0 || n_pairs <= 0) return 0;
    if (n_live > MVS_HCLUST_MAX_TOTAL || 2 * n_pairs > n_live) return MVS_E_INVALID;
    return by_method(method, [&](auto M) {
        hipLaunchKernelGGL(k_hclust_merge_cols<decltype(M)::value>, dim3((unsigned)n_live), dim3(kRowThreads), 0, stream, st.table, st.ld, st.slot_col,
                           st.pairs, d_live, n_pairs);
    });
}

int launch_hclust_merge_rows(hipStream_t stream, const HclustState& st, int method, int64_t n_pairs, int64_t n_cols) {
    if (n_pairs <= 0) return 0;
    if (n_cols <= 0 || n_cols > st.ld || 2 * n_pairs > MVS_HCLUST_MAX_TOTAL) return MVS_E_INVALID;
    return by_method(method, [&](auto M) {
        hipLaunchKernelGGL(k_hclust_merge_rows<decltype(M)::value>, dim3((unsigned)n_pairs), dim3(kRowThreads), 0, stream, st.table, st.ld, st.pairs,
                           n_cols);
    });
}

int launch_hclust_layout(hipStream_t stream, const HclustState& st, int64_t n_cols) {
    if (n_cols <= 0 || n_cols > st.ld) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_hclust_layout, dim3(1), dim3(kScanThreads), 0, stream, st, n_cols);
    return 0;
}

int launch_hclust_compact(hipStream_t stream, const HclustState& st, const int32_t* d_live, int64_t n_live, int64_t n_cols_new) {
    if (n_live <= 0 || n_cols_new <= 0) return 0;
    if (n_cols_new > st.ld || n_live > MVS_HCLUST_MAX_TOTAL) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_hclust_compact, dim3((unsigned)n_live), dim3(kRowThreads), 0, stream, st.table, st.ld, st.keep, d_live, n_cols_new);
    return 0;
}

}  // namespace mvs
