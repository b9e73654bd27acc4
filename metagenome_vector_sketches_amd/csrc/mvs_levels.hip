// mvs_levels.hip -- neighbour counts at many Jaccard levels in one pass over a block of int32 dots (mvs_pairwise_levels).
//
// Every analysis path takes ONE Jaccard level from its caller; this unit answers "how many neighbours would every sample have
// at each of these levels" for up to 64 levels at once, so that a level can be chosen before a tool is run.  The dots of a row
// block come from the dense-dots kernels (launch_pairwise mode 1) into a scratch block of R rows x C columns, exactly as for
// top-k and containment; the kernel below REDUCES the block instead of selecting from it.
//
// The rule (the contract of mvs_pairwise_levels, include/mvs_hip.h).  Levels t_0 < ... < t_{m-1}, 1 <= m <= 64, 0 < t_l < 1;
// coef_l = t_l / (1.0 + t_l) computed on the host in fp64.  Row i, column j, i != j by sample index; P the wrapped int32 dot.
// Everything is fp64 and every line is ONE rounding; a NaN compares false:
//     inter = (double)P / (double)d
//     s     = n2[i] + n2[j]
//     pass_l(i,j) = inter > coef_l * s
//     deg[i][l]   = #{ j in [col_begin, col_end), j != i : pass_l(i,j) }
//     total[l]    = sum over the rows of deg[i][l]                       (int64)
// -- the link rule of mvs_pairwise_cluster / mvs_search_block (keep_cell in mvs_pairwise_dev.h with the floating keep test),
// evaluated independently per level.  It holds for any norms: NaN, +-inf, 0, negative.
//
// Contraction.  As in mvs_contain.hip: no line may be joined with another into a fused multiply-add, so every function that
// states a line carries #pragma clang fp contract(off), and the Makefile builds the unit with -ffp-contract=off.
//
// The prefix.  The host rejects coefficients that are not non-decreasing.  For a cell with s >= 0 (or s = -0.0) the products
// fl(coef_l * s) are then non-decreasing in l -- rounding a product with a non-negative factor is monotone; s = +inf gives inf
// throughout -- so pass_l is non-increasing and the passed levels are a PREFIX 0 .. L-1.  The cell is compared against level 0
// (most cells of a real DB fail it: L = 0, nothing more happens), then L is found with six more compares (steps 32, 16, ..., 1
// from L = 1).  A NaN s fails every compare and gets L = 0 the same way.  The exception is s < 0: the products DEcrease there,
// the passed levels are no prefix, and such a cell takes the slow path -- every level evaluated, one add per passed level into
// a direct counter array.  (s = -inf passes every level of every finite inter; it is on that path.)
//
// Counting.  One workgroup of four waves per row; thread t takes the four consecutive columns 4t .. 4t + 3 of a round of 1024
// columns with one 16-byte load.  Each wave owns a histogram of 65 bins in LDS; a cell adds 1 to bin L, bin 0 is never stored
// (it does not enter any degree).  At the row's end deg[i][l] = (sum of the bins above l over the waves) + direct[l], written
// with plain stores; the row's non-zero values go to total[] with 64-bit integer atomics (integer addition: the order is
// irrelevant).  (Summing the table's columns in a second kernel instead, one atomic per strip of rows and level, measured the
// same time at 100k x 100k: the row atomics are not what the kernel waits for.)
//
// Same-bin scheme: ballot aggregation.  A clique of identical samples puts all 64 lanes of a wave into the same bin every
// round; 64 LDS atomics on one address would serialise.  So the lanes never add for themselves: per column slot u the wave
// loops over the DISTINCT bins among its lanes -- the first pending lane's L is broadcast, a ballot finds the lanes that share
// it, that one lane adds the popcount, the group leaves the pending mask.  A clique costs one iteration and one LDS add per
// slot, whatever the lane count; the worst case (64 distinct bins) costs what 64 serialised atomics would.  A slot in which no
// lane passed level 0 costs one ballot.
//
// Integer pre-test (optional, changes no result).  The lowest level of a real question sits close to the noise of unrelated
// pairs (t = 0.05 at d = 2048 is 2.2 standard deviations of inter): a bound from the row's norm alone lets 1.6 % of the cells
// through, which is at least one lane of nearly every wave in every round, and the wave then pays the fp64 division for all
// four slots (measured at 100k x 100k, m = 16: 12.0 ms, against 8.3 ms with the bound below).  So the bound takes both
// norms, as the comparison's filter does: k_levels_prep leaves per sample an integer a[i] with 0 <= a[i] <= coef_0 * n2[i] * d
// in real arithmetic (fl(fl(coef_0 * n2[i]) * d) shrunk by 2^-40 of itself and by 1, floored, at least 0, at most 2^30 - 1;
// 0 for a norm that is negative, NaN or +inf), and a cell with P <= a[i] + a[j] is dropped before the division.  It is valid
// for a row with 0 <= n2[i] < inf when NO column of the call's range has a negative norm (k_levels_prep raises a flag; then
// the pre-test is off for the call).  Proof: s = fl(n2[i] + n2[j]) >= 0 and T = fl(coef_0 * s) carry two roundings, 2^-52 of
// relative error together, far inside the 2^-40 (the "- 1" per sample covers products that underflow), so
// a[i] + a[j] <= T * d; then P / d <= T in real arithmetic, T is a double, rounding is monotone, hence inter <= T: the cell
// fails level 0 and, s being >= 0, every level.  A column whose norm is NaN or +inf fails every level whatever P.  A row whose
// norm is NaN or +inf passes nothing at all (s is NaN or +inf for every column) and is answered without reading its dots.
#include "mvs_internal.h"

#include <climits>

namespace mvs {

namespace {

constexpr int kLevelsThreads = 256;
constexpr int kLevelsPer = 4;                                   // consecutive columns per thread and round
constexpr int kLevelsRound = kLevelsThreads * kLevelsPer;       // columns per round
constexpr int kLevelsWaves = kLevelsThreads / 64;
constexpr int kLevelsBins = kMaxLevels + 1;                     // bin L = levels passed, 0 .. 64

// pass_l of the rule; inter = (double)P / d and s = n2[i] + n2[j] computed by the caller
__device__ __forceinline__ bool level_pass(double inter, double coef, double s) {
#pragma clang fp contract(off)
    const double t = coef * s;
    return inter > t;
}

// a[i] of the pre-test for every sample (see the top of the file); *flag = 1 if a column of [cb, ce) has a negative norm (-inf
// included; NaN is not negative): the pre-test is off for the call
__global__ __launch_bounds__(256) void k_levels_prep(const double* __restrict__ n2, int64_t n, int64_t cb, int64_t ce, double coef0, double dd,
                                                     int* __restrict__ thr, int* __restrict__ flag) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = n2[i];
    int a = 0;
    if (v >= 0.0 && v < __builtin_inf()) {
        const double td = (coef0 * v) * dd;
        const double lo = floor(td * (1.0 - 0x1p-40) - 1.0);
        a = lo < 0.0 ? 0 : lo >= 1073741823.0 ? 1073741823 : (int)lo;
    }
    thr[i] = a;
    if (i >= cb && i < ce && v < 0.0) *flag = 1;
}

// One workgroup per row of the block.  dots: rows x ld int32 (row r of the block is sample row0 + r, column j is sample c0 + j).
// deg: the block's rows x m table (NULL: totals only).
__global__ __launch_bounds__(kLevelsThreads) void k_levels_count(const int32_t* __restrict__ dots, int64_t ld, int64_t row0, int64_t c0,
                                                                 const double* __restrict__ n2, const double* __restrict__ coef_g, int m,
                                                                 double dd, const int* __restrict__ thr, const int* __restrict__ neg_flag,
                                                                 int32_t* __restrict__ deg, unsigned long long* __restrict__ total) {
#pragma clang fp contract(off)
    __shared__ double coef[kMaxLevels];
    __shared__ int hist[kLevelsWaves][kLevelsBins];
    __shared__ int direct[kMaxLevels];
    __shared__ int bins[kLevelsBins];
    const int64_t r = blockIdx.x;
    const int64_t row = row0 + r;
    const double n2r = n2[row];
    const int tid = threadIdx.x;
    if (!(n2r < __builtin_inf())) {                              // NaN or +inf: s is NaN or +inf, nothing passes (uniform)
        if (deg && tid < m) deg[r * m + tid] = 0;
        return;
    }
    for (int i = tid; i < kLevelsWaves * kLevelsBins; i += kLevelsThreads) (&hist[0][0])[i] = 0;
    if (tid < kMaxLevels) {
        direct[tid] = 0;
        coef[tid] = tid < m ? coef_g[tid] : __builtin_inf();
    }
    __syncthreads();
    const double coef0 = coef[0];
    // the integer pre-test (see the top of the file): this row's part, and whether the row may use it
    const bool pre = n2r >= 0.0 && *neg_flag == 0;
    const int thr_r = thr[row];
    const int* __restrict__ tc = thr + c0;
    const int32_t* __restrict__ dp = dots + r * ld;
    const bool vec = (ld & 3) == 0;
    const bool vec_thr = vec && (c0 & 3) == 0;                   // the columns' parts: one 16-byte load where they are aligned too
    const int lane = tid & 63, wave = tid >> 6;
    int* __restrict__ myhist = hist[wave];
    for (int64_t base = 0; base < ld; base += kLevelsRound) {    // every lane walks every round: the ballots need whole waves
        const int64_t j = base + (int64_t)tid * kLevelsPer;
        int32_t P[kLevelsPer] = {0, 0, 0, 0}, A[kLevelsPer] = {0, 0, 0, 0};
        int nv = 0;
        if (j < ld) {
            if (vec) {                                           // ld % 4 == 0 and j % 4 == 0: j < ld implies j + 3 < ld
                const int4 v = *reinterpret_cast<const int4*>(dp + j);
                P[0] = v.x;
                P[1] = v.y;
                P[2] = v.z;
                P[3] = v.w;
                nv = kLevelsPer;
            } else {
                nv = (int)(ld - j < kLevelsPer ? ld - j : kLevelsPer);
#pragma unroll
                for (int u = 0; u < kLevelsPer; ++u)
                    if (u < nv) P[u] = dp[j + u];
            }
            if (pre) {
                if (vec_thr) {
                    const int4 v = *reinterpret_cast<const int4*>(tc + j);
                    A[0] = v.x;
                    A[1] = v.y;
                    A[2] = v.z;
                    A[3] = v.w;
                } else {
#pragma unroll
                    for (int u = 0; u < kLevelsPer; ++u)
                        if (u < nv) A[u] = tc[j + u];
                }
            }
        }
        int L[kLevelsPer];
#pragma unroll
        for (int u = 0; u < kLevelsPer; ++u) {
            L[u] = 0;
            const int64_t col = c0 + j + u;
            if (u >= nv || col == row) continue;
            if (pre && P[u] <= thr_r + A[u]) continue;
            const double inter = (double)P[u] / dd;
            const double s = n2r + n2[col];
            if (s < 0.0) {                                       // the slow path: no prefix, every level on its own
                for (int l = 0; l < m; ++l)
                    if (level_pass(inter, coef[l], s)) atomicAdd(&direct[l], 1);
                continue;
            }
            if (!level_pass(inter, coef0, s)) continue;
            int len = 1;                                         // levels 0 .. len - 1 pass
#pragma unroll
            for (int step = kMaxLevels / 2; step > 0; step >>= 1) {
                const int cand = len + step;
                if (cand <= m && level_pass(inter, coef[cand - 1], s)) len = cand;
            }
            L[u] = len;
        }
#pragma unroll
        for (int u = 0; u < kLevelsPer; ++u) {                   // ballot aggregation: one LDS add per distinct bin of the wave
            unsigned long long todo = __ballot(L[u] > 0);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const int Lb = __shfl(L[u], leader, 64);
                const unsigned long long same = __ballot(L[u] == Lb);
                if (lane == leader) atomicAdd(&myhist[Lb], __popcll(same));
                todo &= ~same;
            }
        }
    }
    __syncthreads();
    if (tid < kLevelsBins) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < kLevelsWaves; ++w) v += hist[w][tid];
        bins[tid] = v;
    }
    __syncthreads();
    if (tid < m) {
        int v = direct[tid];
        for (int b = tid + 1; b <= m; ++b) v += bins[b];
        if (deg) deg[r * m + tid] = v;
        if (v) atomicAdd(&total[tid], (unsigned long long)v);
    }
}

}  // namespace

int launch_levels_prep(hipStream_t stream, const double* d_norms_sq, int64_t n, int64_t col_begin, int64_t col_end, double coef0, int d,
                       int* d_thr, int* d_flag) {
    if (n <= 0) return 0;
    if (n > INT_MAX || d <= 0) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_levels_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_norms_sq, n, col_begin, col_end, coef0,
                       (double)d, d_thr, d_flag);
    return 0;
}

int launch_levels_count(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                        const double* d_norms_sq, const double* d_coef, int m, int d, const int* d_thr, const int* d_neg_flag,
                        int32_t* d_deg, unsigned long long* d_total) {
    if (rows <= 0) return 0;
    if (ld <= 0 || ld > INT_MAX || rows > INT_MAX || m < 1 || m > kMaxLevels || d <= 0) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_levels_count, dim3((unsigned)rows), dim3(kLevelsThreads), 0, stream, d_dots, ld, row0, c0, d_norms_sq, d_coef,
                       m, (double)d, d_thr, d_neg_flag, d_deg, d_total);
    return 0;
}

}  // namespace mvs
