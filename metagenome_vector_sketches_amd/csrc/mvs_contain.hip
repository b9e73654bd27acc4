// mvs_contain.hip -- containment from sketches: which cells of a block of int32 dots pass the containment rule
// (mvs_pairwise_contain).
//
// Every other comparison of this library scores a pair by its Jaccard estimate, which the size ratio of the two samples
// bounds: a sample wholly contained in one 30 times its size has J <= 0.033.  This unit keeps a cell when the ESTIMATED
// CONTAINMENT of the row's sample in the column's exceeds a level.  The dots of a row block come from the dense-dots kernels
// (launch_pairwise mode 1) into a scratch block of R rows x C columns, exactly as for top-k; the kernels below select.
//
// The rule (the contract of mvs_pairwise_contain, include/mvs_hip.h).  Row i, column j, i != j; P the wrapped int32 dot;
// c = min_containment, 0 < c < 1; z = slack, finite.  Everything is fp64 and every line is ONE rounding:
//     inter = (double)P / (double)d
//     t     = c * n2[i]
//     e     = inter - t                          // never fused with the product above
//     ok    = n2[i] > 0 && n2[i] < inf && n2[j] >= 0 && n2[j] < inf          // NaN fails
//     z == 0 : dir(i,j) = ok && e > 0
//     z  > 0 : dir(i,j) = ok && e > 0 && (e*e)*(double)d > (z*z) * (n2[i]*n2[j])
//     z  < 0 : dir(i,j) = ok && (e > 0 || (e*e)*(double)d < (z*z) * (n2[i]*n2[j]))
// "the estimated containment of i in j exceeds c by more than z standard errors" (the variance of inter is about
// n2[i] n2[j] / d), in squares so that no square root is taken.  MVS_CONTAIN_ROW keeps a cell iff dir(i,j), MVS_CONTAIN_MAX
// iff dir(i,j) || dir(j,i) (P is symmetric, so that mode is symmetric bit for bit).  q of a kept cell: Cq = inter / n2[i];
// !(Cq > 0) -> 0; Cq > 1 -> 1; q = (int32)round(Cq * 255) (C round: halves away from zero, as the writer's q); in MAX mode the
// larger of the two directions' values, a direction whose row norm is not in (0, inf) counting 0.  dot = P.
//
// Contraction.  hipcc contracts a - b * c into one fused multiply-add by default; a host restatement (numpy) rounds the
// product first.  The two differ exactly where it matters: c * n2[i] = 0.3 * 10.0 rounds to 3.0, e = 0 and the cell is not
// kept, while the fused form gives +1.1e-16 and keeps it.  Contraction is therefore switched off inside every function that
// states a line of the rule (#pragma clang fp contract(off) at the top of its body; the Makefile also builds this unit with
// -ffp-contract=off).  __dmul_rn / __dsub_rn do NOT do it: in this toolchain's headers they are the plain operators, parsed
// with contraction allowed, and the compiler fuses them like any other product and difference (the rounding case of
// tests/test_contain_gpu.py caught exactly that in MAX mode's second direction).
//
// Integer pre-test (z >= 0).  dir(i,j) needs e > 0, i.e. fl(P / d) > t.  thr[i] is an integer with thr[i] <= t * d in real
// arithmetic (t * d rounded, shrunk by 2^-40 of itself and by 1, floored, at least 0): for P <= thr[i] the real quotient P / d
// is <= t, t is a double, rounding is monotone, so fl(P / d) <= t and e <= 0; P <= 0 gives inter <= 0 <= t.  A row whose norm
// is not in (0, inf) has thr = INT_MAX.  A cell is evaluated in fp64 only if P > thr[row] (MAX mode: > the smaller of the two
// samples' values); everything the pre-test drops fails the rule, so the result is that of the rule alone.  z < 0 has no
// pre-test: a cell may pass there with e <= 0.
//
// Order.  The cells of a block come out sorted by (row, col) by construction.  k_contain_count: one workgroup per row walks
// the row in rounds of kContainRound columns -- thread t takes the four consecutive columns 4t .. 4t + 3 of the round with one
// 16-byte load -- and counts the kept cells.  k_contain_scan: one workgroup turns the block's counts into offsets behind the
// call's running total, which lives on the device and advances.  k_contain_fill walks the row again; a kept cell's slot is
// the row's offset + the cells kept in earlier rounds + those of lower threads of this round (ballots of the four column
// bits, popcounts below the lane, the waves' totals through LDS) + the lower bits of its own thread: the column order.  No
// atomic and no sort decides a position.  A row whose cells do not fit the caller's capacity is not written; the total goes
// on counting, so the call can report what it needs.
#include "mvs_internal.h"

#include <climits>

namespace mvs {

namespace {

constexpr int kContainThreads = 256;
constexpr int kContainPer = 4;                                  // consecutive columns per thread and round
constexpr int kContainRound = kContainThreads * kContainPer;    // columns per round
constexpr int kContainWaves = kContainThreads / 64;

__device__ __forceinline__ bool norm_pos_finite(double v) { return v > 0.0 && v < __builtin_inf(); }

// dir(i,j) of the rule; inter = (double)P / d computed by the caller
__device__ __forceinline__ bool contain_dir(double inter, double n2i, double n2j, const ContainRule& ru) {
#pragma clang fp contract(off)
    const bool ok = norm_pos_finite(n2i) && n2j >= 0.0 && n2j < __builtin_inf();
    const double t = ru.c * n2i;
    const double e = inter - t;                                  // not fused with the product above
    if (ru.zsign == 0) return ok && e > 0.0;
    const double lhs = (e * e) * ru.dd;
    const double rhs = ru.zz * (n2i * n2j);
    if (ru.zsign > 0) return ok && e > 0.0 && lhs > rhs;
    return ok && (e > 0.0 || lhs < rhs);
}

__device__ __forceinline__ int32_t contain_q_dir(double inter, double n2i) {
#pragma clang fp contract(off)
    if (!norm_pos_finite(n2i)) return 0;
    double cq = inter / n2i;
    if (!(cq > 0.0)) cq = 0.0;
    if (cq > 1.0) cq = 1.0;
    return (int32_t)round(cq * 255.0);
}

// the four columns j .. j + 3 of a row of dots (those below ld): one 16-byte load where the row is 16-byte aligned
__device__ __forceinline__ int load4(const int32_t* __restrict__ dp, int64_t j, int64_t ld, bool vec, int32_t P[kContainPer]) {
    if (vec) {                                                   // ld % 4 == 0 and j % 4 == 0: j < ld implies j + 3 < ld
        const int4 v = *reinterpret_cast<const int4*>(dp + j);
        P[0] = v.x;
        P[1] = v.y;
        P[2] = v.z;
        P[3] = v.w;
        return kContainPer;
    }
    const int nv = (int)(ld - j < kContainPer ? ld - j : kContainPer);
#pragma unroll
    for (int u = 0; u < kContainPer; ++u) P[u] = u < nv ? dp[j + u] : 0;
    return nv;
}

// bit u: the cell (row, col0 + u) is kept
__device__ __forceinline__ unsigned keep4(const int32_t P[kContainPer], int nv, int64_t col0, int64_t row, double n2r, int thr_r,
                                          const double* __restrict__ n2, const int* __restrict__ thr, const ContainRule& ru) {
    unsigned mask = 0;
#pragma unroll
    for (int u = 0; u < kContainPer; ++u) {
        const int64_t col = col0 + u;
        if (u >= nv || col == row) continue;
        if (ru.pretest) {
            int th = thr_r;
            if (ru.mode == MVS_CONTAIN_MAX) th = min(th, thr[col]);
            if (P[u] <= th) continue;
        }
        const double n2c = n2[col];
        const double inter = (double)P[u] / ru.dd;
        bool keep = contain_dir(inter, n2r, n2c, ru);
        if (!keep && ru.mode == MVS_CONTAIN_MAX) keep = contain_dir(inter, n2c, n2r, ru);
        if (keep) mask |= 1u << u;
    }
    return mask;
}

// thr[i] of the pre-test for every sample (see the top of the file)
__global__ __launch_bounds__(256) void k_contain_thr(const double* __restrict__ n2, int64_t n, ContainRule ru, int* __restrict__ thr) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = n2[i];
    int th = INT_MAX;
    if (norm_pos_finite(v)) {
        const double td = (ru.c * v) * ru.dd;
        const double lo = floor(td * (1.0 - 0x1p-40) - 1.0);     // (fused or not: below t * d either way)
        if (lo < 2147483647.0) th = lo < 0.0 ? 0 : (int)lo;
    }
    thr[i] = th;
}

// a row of ROW mode whose norm fails `ok` keeps nothing, whatever z
__device__ __forceinline__ bool row_is_dead(double n2r, const ContainRule& ru) {
    return ru.mode == MVS_CONTAIN_ROW && !norm_pos_finite(n2r);
}

// One workgroup per row of the block.  dots: rows x ld int32 (row r of the block is sample row0 + r, column j is sample c0 + j).
__global__ __launch_bounds__(kContainThreads) void k_contain_count(const int32_t* __restrict__ dots, int64_t ld, int64_t row0, int64_t c0,
                                                                   const double* __restrict__ n2, const int* __restrict__ thr,
                                                                   ContainRule ru, int* __restrict__ counts) {
    __shared__ int wsum[kContainWaves];
    const int64_t r = blockIdx.x;
    const int64_t row = row0 + r;
    const double n2r = n2[row];
    if (row_is_dead(n2r, ru)) {
        if (threadIdx.x == 0) counts[r] = 0;
        return;
    }
    const int32_t* __restrict__ dp = dots + r * ld;
    const int thr_r = ru.pretest ? thr[row] : 0;
    const bool vec = (ld & 3) == 0;
    int mine = 0;
    for (int64_t base = 0; base < ld; base += kContainRound) {
        const int64_t j = base + (int64_t)threadIdx.x * kContainPer;
        if (j >= ld) continue;
        int32_t P[kContainPer];
        const int nv = load4(dp, j, ld, vec, P);
        mine += __popc(keep4(P, nv, c0 + j, row, n2r, thr_r, n2, thr, ru));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kContainWaves; ++w) total += wsum[w];
        counts[r] = total;
    }
}

// offs[r] = *total + (cells of the block's rows before r); *total += the block's cells.  One workgroup.
__global__ __launch_bounds__(256) void k_contain_scan(const int* __restrict__ counts, int rows, long long* __restrict__ offs,
                                                      unsigned long long* __restrict__ total) {
    __shared__ long long part[256];
    const int per = (rows + 255) / 256;
    const int b = min(rows, (int)threadIdx.x * per), e = min(rows, b + per);
    long long s = 0;
    for (int i = b; i < e; ++i) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = (long long)*total;
        for (int t = 0; t < 256; ++t) {
            const long long v = part[t];
            part[t] = run;
            run += v;
        }
        *total = (unsigned long long)run;
    }
    __syncthreads();
    long long at = part[threadIdx.x];
    for (int i = b; i < e; ++i) {
        offs[i] = at;
        at += counts[i];
    }
}

__global__ __launch_bounds__(kContainThreads) void k_contain_fill(const int32_t* __restrict__ dots, int64_t ld, int64_t row0, int64_t c0,
                                                                  const double* __restrict__ n2, const int* __restrict__ thr,
                                                                  ContainRule ru, const int* __restrict__ counts,
                                                                  const long long* __restrict__ offs, mvs_cell* __restrict__ cells,
                                                                  long long capacity) {
    __shared__ int wtot[2][kContainWaves];
    const int64_t r = blockIdx.x;
    const int cnt = counts[r];
    if (cnt == 0) return;
    long long run = offs[r];                                     // the row's next free slot before this round (uniform)
    if (run + cnt > capacity) return;                            // no room: the call reports the total it needs
    const int64_t row = row0 + r;
    const double n2r = n2[row];
    const int32_t* __restrict__ dp = dots + r * ld;
    const int thr_r = ru.pretest ? thr[row] : 0;
    const bool vec = (ld & 3) == 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    int par = 0;
    for (int64_t base = 0; base < ld; base += kContainRound, par ^= 1) {
        const int64_t j = base + (int64_t)threadIdx.x * kContainPer;
        int32_t P[kContainPer] = {0, 0, 0, 0};
        unsigned mask = 0;
        if (j < ld) {
            const int nv = load4(dp, j, ld, vec, P);
            mask = keep4(P, nv, c0 + j, row, n2r, thr_r, n2, thr, ru);
        }
        int before = 0, wave_total = 0;                          // kept cells of lower lanes / of the whole wave, this round
#pragma unroll
        for (int u = 0; u < kContainPer; ++u) {
            const unsigned long long b = __ballot((mask >> u) & 1u);
            before += __popcll(b & below);
            wave_total += __popcll(b);
        }
        if (lane == 0) wtot[par][wave] = wave_total;
        __syncthreads();                                         // (the buffer of two rounds ago is free: see the top)
        int pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kContainWaves; ++w) {
            const int v = wtot[par][w];
            if (w < wave) pre += v;
            tot += v;
        }
        long long slot = run + pre + before;
#pragma unroll
        for (int u = 0; u < kContainPer; ++u) {
            if (!((mask >> u) & 1u)) continue;
            const int64_t col = c0 + j + u;
            const double inter = (double)P[u] / ru.dd;
            int32_t q = contain_q_dir(inter, n2r);
            if (ru.mode == MVS_CONTAIN_MAX) q = max(q, contain_q_dir(inter, n2[col]));
            mvs_cell c;
            c.row = (int32_t)row;
            c.col = (int32_t)col;
            c.dot = P[u];
            c.q = q;
            cells[slot++] = c;
        }
        run += tot;
    }
}

}  // namespace

int launch_contain_thr(hipStream_t stream, const double* d_norms_sq, int64_t n, const ContainRule& ru, int* d_thr) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_contain_thr, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_norms_sq, n, ru, d_thr);
    return 0;
}

int launch_contain_count(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                         const double* d_norms_sq, const int* d_thr, const ContainRule& ru, int* d_counts) {
    if (rows <= 0) return 0;
    if (ld <= 0 || ld > INT_MAX || rows > INT_MAX) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_contain_count, dim3((unsigned)rows), dim3(kContainThreads), 0, stream, d_dots, ld, row0, c0, d_norms_sq,
                       d_thr, ru, d_counts);
    return 0;
}

int launch_contain_scan(hipStream_t stream, const int* d_counts, int64_t rows, long long* d_offs, unsigned long long* d_total) {
    if (rows <= 0) return 0;
    if (rows > INT_MAX) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_contain_scan, dim3(1), dim3(256), 0, stream, d_counts, (int)rows, d_offs, d_total);
    return 0;
}

int launch_contain_fill(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                        const double* d_norms_sq, const int* d_thr, const ContainRule& ru, const int* d_counts,
                        const long long* d_offs, mvs_cell* d_cells, int64_t capacity) {
    if (rows <= 0) return 0;
    if (ld <= 0 || ld > INT_MAX || rows > INT_MAX) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_contain_fill, dim3((unsigned)rows), dim3(kContainThreads), 0, stream, d_dots, ld, row0, c0, d_norms_sq,
                       d_thr, ru, d_counts, d_offs, d_cells, (long long)capacity);
    return 0;
}

}  // namespace mvs
