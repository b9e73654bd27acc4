// mvs_tsne.hip -- the kernels of the exact t-SNE map of the Jaccard kNN graph (mvs_tsne_*).
//
// The rule is stated in include/mvs_hip.h "t-SNE" and DESIGN.md section 26; tests/tsne_model.py is the same rule in numpy.  A
// pair's term is a handful of IEEE fp64 operations, each rounded once (this unit is built with -ffp-contract=off, so no
// multiply and add are fused), then quantised: rint(x * 2^40).  Every sum over more than one term is therefore a sum of
// integers, and no tiling, atomic or order of lanes can change a coordinate.
//
// k_tsne_calibrate   one wave per row: the row's <= 256 squared distances in four registers per lane, the entropy's two sums by
//                    xor butterflies (every lane ends with the same bits, so the bisection's branches are uniform).
// k_tsne_repulse     the hot path, n^2 terms per iteration.  A unit is 256 rows x one slice of columns: a lane owns a row's y
//                    and three accumulators, the slice's y sits in LDS and every lane reads the same address (a broadcast).  The
//                    quantised terms are integer-valued doubles of magnitude <= 2^40; a unit adds at most 1024 of them, so a
//                    lane's partial sums stay below 2^53 and fp64 addition is exact: the emulated fp64 -> int64 conversion
//                    is paid three times per unit, not per pair, followed by one 64-bit integer atomic per accumulator.
//                    The pair (i, i) is computed like any other (q = 1, u dx = 0) and its 2^40 taken off Z_i once, exactly.
// k_tsne_attract     one wave per row of the CSR, int64 sums by butterfly; its lane 0 also folds Z_i >> 20 into Z.
// k_tsne_update      elementwise over the 2 n coordinates.
#include "mvs_tsne.h"

#include <climits>
#include <cmath>

namespace mvs {

namespace {

typedef unsigned long long u64;

constexpr int kTsThreads = 256;
constexpr double kTsScale = 1099511627776.0;          // 2^40
constexpr double kTsInv = 1.0 / 1099511627776.0;
constexpr double kTsZInv = 1.0 / 1048576.0;           // 2^-20
constexpr double kTsCScale = 1073741824.0;            // 2^30
constexpr int kTsMaxSteps = 200;
constexpr double kTsEntropyTol = 1e-5;

unsigned grid_for(int64_t items) {
    const int64_t blocks = (items + kTsThreads - 1) / kTsThreads;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, 1 << 16));
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) { return (long long)wave_sum((u64)v); }
// xor butterflies: a + b commutes bit for bit, so every lane ends with the same value
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_check_cells(const mvs_cell* __restrict__ cells, int64_t n_cells, int64_t n,
                                                                 u64* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kTsThreads;
    u64 bad = 0, down = 0, many = 0;
    for (int64_t i = (int64_t)blockIdx.x * kTsThreads + threadIdx.x; i < n_cells; i += stride) {
        const int32_t r = cells[i].row, c = cells[i].col;
        if (r < 0 || c < 0 || r >= n || c >= n || r == c) ++bad;
        if (i > 0 && cells[i - 1].row > r) ++down;
        if (i >= kTsneMaxNeighbours && cells[i - kTsneMaxNeighbours].row == r) ++many;
    }
    if (bad) atomicAdd(counters + 0, bad);
    if (down) atomicAdd(counters + 1, down);
    if (many) atomicAdd(counters + 2, many);
}

// the first cell of the (row-sorted) list whose row is >= want
__device__ __forceinline__ int64_t first_of_row(const mvs_cell* __restrict__ cells, int64_t n_cells, int64_t want) {
    int64_t lo = 0, hi = n_cells;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)cells[mid].row < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_calibrate(const mvs_cell* __restrict__ cells, int64_t n_cells, int64_t row0, int64_t rows,
                                                               const double* __restrict__ n2, double dd, double perplexity, double target,
                                                               double* __restrict__ beta_out, int32_t* __restrict__ c_out,
                                                               u64* __restrict__ keys, u64* __restrict__ vals, u64* __restrict__ counters) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t w = (int64_t)blockIdx.x * (kTsThreads / 64) + (threadIdx.x >> 6);
    if (w >= rows) return;                                              // whole waves leave together
    const int64_t row = row0 + w;
    const int64_t b = first_of_row(cells, n_cells, row), e = first_of_row(cells, n_cells, row + 1);
    const int m = (int)(e - b);                                         // <= 256: k_tsne_check_cells
    if (m == 0) {
        if (lane == 0) {
            beta_out[row] = 0.0;
            atomicAdd(counters + 3, 1ULL);
        }
        return;
    }
    constexpr int kPer = kTsneMaxNeighbours / 64;
    double x[kPer];
    int32_t col[kPer];
    const double n2r = n2[row];
    double lo_d = INFINITY, hi_d = -INFINITY;
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        const int k = lane + 64 * t;
        x[t] = 0.0;
        col[t] = 0;
        if (k < m) {
            const mvs_cell cell = cells[b + k];
            col[t] = cell.col;
            const double inter = (double)cell.dot / dd;
            const double s = n2r + n2[cell.col];
            const double den = s - inter;
            double J = inter / den;
            J = !(J > 0.0) ? 0.0 : (J > 1.0 ? 1.0 : J);
            x[t] = 1.0 - J;
            lo_d = fmin(lo_d, x[t]);
            hi_d = fmax(hi_d, x[t]);
        }
    }
    lo_d = wave_min(lo_d);
    hi_d = wave_max(hi_d);
#pragma unroll
    for (int t = 0; t < kPer; ++t) x[t] = x[t] - lo_d;
    double beta = 0.0;
    if ((double)m > perplexity && hi_d != lo_d) {
        beta = 1.0;
        double lo = 0.0, hi = 0.0;
        bool have_hi = false;
        for (int step = 0; step < kTsMaxSteps; ++step) {
            double sw = 0.0, sx = 0.0;
#pragma unroll
            for (int t = 0; t < kPer; ++t)
                if (lane + 64 * t < m) {
                    const double wt = exp(-beta * x[t]);
                    sw += wt;
                    sx += wt * x[t];
                }
            sw = wave_sum(sw);
            sx = wave_sum(sx);
            const double diff = (log(sw) + beta * sx / sw) - target;
            if (fabs(diff) <= kTsEntropyTol) break;
            if (diff > 0.0) {
                lo = beta;
                beta = have_hi ? (beta + hi) * 0.5 : beta * 2.0;
            } else {
                hi = beta;
                have_hi = true;
                beta = (lo + beta) * 0.5;
            }
        }
    }
    double wt[kPer];
    double sw = 0.0;
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        wt[t] = 0.0;
        if (lane + 64 * t < m) {
            wt[t] = exp(-beta * x[t]);
            sw += wt[t];
        }
    }
    sw = wave_sum(sw);
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
        const int k = lane + 64 * t;
        if (k < m) {
            const u64 c = (u64)llrint((wt[t] / sw) * kTsCScale);
            const int64_t at = b + k;
            if (c_out) c_out[at] = (int32_t)c;
            keys[2 * at] = ((u64)(uint32_t)row << 32) | (u64)(uint32_t)col[t];
            keys[2 * at + 1] = ((u64)(uint32_t)col[t] << 32) | (u64)(uint32_t)row;
            vals[2 * at] = c;
            vals[2 * at + 1] = c;
        }
    }
    if (lane == 0) {
        beta_out[row] = beta;
        if (beta == 0.0) atomicAdd(counters + 3, 1ULL);
    }
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_check_edges(const int32_t* __restrict__ elo, const int32_t* __restrict__ ehi,
                                                                 const int32_t* __restrict__ es, int64_t n_edges, int64_t n,
                                                                 u64* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kTsThreads;
    u64 bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kTsThreads + threadIdx.x; i < n_edges; i += stride) {
        const int32_t r = elo[i], c = ehi[i];
        if (r < 0 || c < 0 || r >= n || c >= n || es[i] < 1) ++bad;
    }
    if (bad) atomicAdd(counters + 0, bad);
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_edges(const int32_t* __restrict__ elo, const int32_t* __restrict__ ehi,
                                                           const int32_t* __restrict__ es, int64_t n_edges, u64* __restrict__ keys,
                                                           u64* __restrict__ vals, u64* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kTsThreads;
    u64 selfs = 0;
    for (int64_t i = (int64_t)blockIdx.x * kTsThreads + threadIdx.x; i < n_edges; i += stride) {
        const uint32_t r = (uint32_t)elo[i], c = (uint32_t)ehi[i];
        const bool self = r == c;
        if (self) ++selfs;
        keys[2 * i] = self ? ~0ULL : ((u64)r << 32) | c;
        keys[2 * i + 1] = self ? ~0ULL : ((u64)c << 32) | r;
        vals[2 * i] = self ? 0ULL : (u64)es[i];
        vals[2 * i + 1] = self ? 0ULL : (u64)es[i];
    }
    if (selfs) atomicAdd(counters + 1, selfs);
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_total(const u64* __restrict__ vals, int64_t m, u64* __restrict__ total) {
    const int64_t stride = (int64_t)gridDim.x * kTsThreads;
    u64 s = 0;
    for (int64_t i = (int64_t)blockIdx.x * kTsThreads + threadIdx.x; i < m; i += stride) s += vals[i];
    s = wave_sum(s);                                                    // (every lane of the wave is here)
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_p(const u64* __restrict__ vals, int64_t m, double S, double* __restrict__ p) {
    const int64_t stride = (int64_t)gridDim.x * kTsThreads;
    for (int64_t i = (int64_t)blockIdx.x * kTsThreads + threadIdx.x; i < m; i += stride) p[i] = (double)vals[i] / S;
}

// 1.0 / x for x >= 1 (or inf, NaN), correctly rounded: the division's own sequence -- v_rcp_f64, two Newton steps, the residual
// correction, v_div_fixup for inf and NaN -- without its two v_div_scale and the multiply by the numerator, which do nothing
// for a numerator of 1 and an x >= 1 away from the top of the exponent range.  Up there (x > 2^700, say) the quotient is below
// 2^-700 whichever way it is formed, and every term it enters quantises to 0 (tests: the state "huge").  The fused operations are the division's internals, not the contract's: the result is the IEEE quotient.
__device__ __forceinline__ double reciprocal_ge1(double x) {
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    const double r = fma(-x, y, 1.0);
    return __builtin_amdgcn_div_fixup(fma(r, y, y), x, 1.0);
}

// unit u: rows [256 (u % row_blocks), ...), columns [slice (u / row_blocks), ...)
__global__ __launch_bounds__(kTsThreads) void k_tsne_repulse(const double2* __restrict__ y, int n, int slice, int row_blocks,
                                                             long long* __restrict__ z_rows, long long* __restrict__ rep) {
    __shared__ double2 tile[kTsneMaxSlice];
    const int rb = (int)(blockIdx.x % (unsigned)row_blocks), sl = (int)(blockIdx.x / (unsigned)row_blocks);
    const int c0 = sl * slice;                                          // < n: the host launches ceil(n / slice) slices
    const int cnt = min(slice, n - c0);
    for (int k = (int)threadIdx.x; k < cnt; k += kTsThreads) tile[k] = y[c0 + k];
    __syncthreads();
    const int i = rb * kTsneRows + (int)threadIdx.x;
    if (i >= n) return;
    const double2 yi = y[i];
    double z = 0.0, rx = 0.0, ry = 0.0;
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) {
        const double2 yj = tile[k];
        const double dx = yi.x - yj.x;
        const double dy = yi.y - yj.y;
        const double r = dx * dx + dy * dy;
        const double q = reciprocal_ge1(1.0 + r);
        const double u = q * q;
        z += rint(q * kTsScale);
        rx += rint((u * dx) * kTsScale);
        ry += rint((u * dy) * kTsScale);
    }
    if (i >= c0 && i < c0 + cnt) z -= kTsScale;                         // the pair (i, i): q = 1, u dx = u dy = 0
    atomicAdd((u64*)(z_rows + i), (u64)(long long)z);
    atomicAdd((u64*)(rep + 2 * (int64_t)i), (u64)(long long)rx);
    atomicAdd((u64*)(rep + 2 * (int64_t)i + 1), (u64)(long long)ry);
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_attract(const double2* __restrict__ y, int64_t n, const long long* __restrict__ row_ptr,
                                                             const int32_t* __restrict__ col, const double* __restrict__ p,
                                                             const long long* __restrict__ z_rows, long long* __restrict__ att,
                                                             long long* __restrict__ z) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t row = (int64_t)blockIdx.x * (kTsThreads / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const double2 yi = y[row];
    long long ax = 0, ay = 0;
    if (row_ptr) {
        const int64_t b = row_ptr[row], e = row_ptr[row + 1];
        for (int64_t k = b + lane; k < e; k += 64) {
            const double2 yj = y[col[k]];
            const double dx = yi.x - yj.x;
            const double dy = yi.y - yj.y;
            const double r = dx * dx + dy * dy;
            const double q = 1.0 / (1.0 + r);
            const double t = p[k] * q;
            ax += (long long)rint((t * dx) * kTsScale);
            ay += (long long)rint((t * dy) * kTsScale);
        }
    }
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    if (lane == 0) {
        att[2 * row] = ax;
        att[2 * row + 1] = ay;
        const long long zi = z_rows[row] >> 20;
        if (zi) atomicAdd((u64*)z, (u64)zi);
    }
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_update(int64_t count, const long long* __restrict__ rep, const long long* __restrict__ att,
                                                            const long long* __restrict__ z, double exaggeration, double momentum,
                                                            double learning_rate, int advance, double* __restrict__ y,
                                                            double* __restrict__ vel, double* __restrict__ gain, double* __restrict__ grad) {
    const int64_t stride = (int64_t)gridDim.x * kTsThreads;
    const long long Z = *z;
    const double zd = (double)Z * kTsZInv;
    for (int64_t k = (int64_t)blockIdx.x * kTsThreads + threadIdx.x; k < count; k += stride) {
        const double a = exaggeration * ((double)att[k] * kTsInv);
        const double r = Z == 0 ? 0.0 : ((double)rep[k] * kTsInv) / zd;
        const double g = 4.0 * (a - r);
        if (grad) grad[k] = g;
        if (advance) {
            const double v = vel[k];
            double gn = gain[k];
            gn = ((g > 0.0) == (v > 0.0)) ? gn * 0.8 : gn + 0.2;
            if (gn < 0.01) gn = 0.01;
            const double step = learning_rate * (gn * g);
            const double nv = momentum * v - step;
            gain[k] = gn;
            vel[k] = nv;
            y[k] = y[k] + nv;
        }
    }
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_kl(const double2* __restrict__ y, int64_t m, const int32_t* __restrict__ src,
                                                        const int32_t* __restrict__ col, const double* __restrict__ p,
                                                        const long long* __restrict__ z, double* __restrict__ kl) {
    const int64_t stride = (int64_t)gridDim.x * kTsThreads;
    const int64_t trips = (m + stride - 1) / stride;                    // every lane makes every trip: the butterflies are whole
    const double zd = (double)*z * kTsZInv;
    double sum = 0.0;
    int64_t k = (int64_t)blockIdx.x * kTsThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, k += stride) {
        if (k < m && p[k] > 0.0) {
            const double2 yi = y[src[k]], yj = y[col[k]];
            const double dx = yi.x - yj.x;
            const double dy = yi.y - yj.y;
            const double r = dx * dx + dy * dy;
            const double q = 1.0 / (1.0 + r);
            sum += p[k] * log(p[k] / (q / zd));
        }
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && sum != 0.0) atomicAdd(kl, sum);
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_fill(double* __restrict__ x, int64_t count, double value) {
    const int64_t stride = (int64_t)gridDim.x * kTsThreads;
    for (int64_t k = (int64_t)blockIdx.x * kTsThreads + threadIdx.x; k < count; k += stride) x[k] = value;
}

}  // namespace

int launch_tsne_check_cells(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, int64_t n, unsigned long long* d_counters) {
    if (n_cells <= 0) return 0;
    hipLaunchKernelGGL(k_tsne_check_cells, dim3(grid_for(n_cells)), dim3(kTsThreads), 0, stream, d_cells, n_cells, n, d_counters);
    return 0;
}

int launch_tsne_calibrate(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, int64_t row0, int64_t rows, const double* d_norms_sq,
                          int d, double perplexity, double* d_beta, int32_t* d_c, unsigned long long* d_keys, unsigned long long* d_vals,
                          unsigned long long* d_counters) {
    if (rows <= 0) return 0;
    const int64_t blocks = (rows + kTsThreads / 64 - 1) / (kTsThreads / 64);
    if (blocks > INT32_MAX) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_tsne_calibrate, dim3((unsigned)blocks), dim3(kTsThreads), 0, stream, d_cells, n_cells, row0, rows, d_norms_sq, (double)d,
                       perplexity, std::log(perplexity), d_beta, d_c, d_keys, d_vals, d_counters);
    return 0;
}

int launch_tsne_check_edges(hipStream_t stream, const int32_t* d_lo, const int32_t* d_hi, const int32_t* d_s, int64_t n_edges, int64_t n,
                            unsigned long long* d_counters) {
    if (n_edges <= 0) return 0;
    hipLaunchKernelGGL(k_tsne_check_edges, dim3(grid_for(n_edges)), dim3(kTsThreads), 0, stream, d_lo, d_hi, d_s, n_edges, n, d_counters);
    return 0;
}

int launch_tsne_edges(hipStream_t stream, const int32_t* d_lo, const int32_t* d_hi, const int32_t* d_s, int64_t n_edges,
                      unsigned long long* d_keys, unsigned long long* d_vals, unsigned long long* d_counters) {
    if (n_edges <= 0) return 0;
    hipLaunchKernelGGL(k_tsne_edges, dim3(grid_for(n_edges)), dim3(kTsThreads), 0, stream, d_lo, d_hi, d_s, n_edges, d_keys, d_vals, d_counters);
    return 0;
}

int launch_tsne_total(hipStream_t stream, const unsigned long long* d_vals, int64_t m, unsigned long long* d_total) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_tsne_total, dim3(grid_for(m)), dim3(kTsThreads), 0, stream, d_vals, m, d_total);
    return 0;
}

int launch_tsne_p(hipStream_t stream, const unsigned long long* d_vals, int64_t m, unsigned long long S, double* d_p) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_tsne_p, dim3(grid_for(m)), dim3(kTsThreads), 0, stream, d_vals, m, (double)S, d_p);
    return 0;
}

int launch_tsne_repulse(hipStream_t stream, const double* d_y, int64_t n, int slice_cols, const TsneSums& sums, int64_t* units) {
    if (units) *units = 0;
    if (n <= 0) return 0;
    if (slice_cols < kTsneMinSlice || slice_cols > kTsneMaxSlice || n > (1LL << 21)) return MVS_E_INVALID;
    const int64_t row_blocks = (n + kTsneRows - 1) / kTsneRows, slices = (n + slice_cols - 1) / slice_cols;
    const int64_t count = row_blocks * slices;
    if (count > INT32_MAX) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_tsne_repulse, dim3((unsigned)count), dim3(kTsThreads), 0, stream, (const double2*)d_y, (int)n, slice_cols, (int)row_blocks,
                       sums.z_rows, sums.rep);
    if (units) *units = count;
    return 0;
}

int launch_tsne_attract(hipStream_t stream, const double* d_y, int64_t n, const long long* d_row_ptr, const int32_t* d_col, const double* d_p,
                        const TsneSums& sums) {
    if (n <= 0) return 0;
    const int64_t blocks = (n + kTsThreads / 64 - 1) / (kTsThreads / 64);
    hipLaunchKernelGGL(k_tsne_attract, dim3((unsigned)blocks), dim3(kTsThreads), 0, stream, (const double2*)d_y, n, d_row_ptr, d_col, d_p,
                       sums.z_rows, sums.att, sums.z);
    return 0;
}

int launch_tsne_update(hipStream_t stream, int64_t n, const TsneSums& sums, double exaggeration, double momentum, double learning_rate,
                       int advance, double* d_y, double* d_vel, double* d_gain, double* d_grad) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_tsne_update, dim3(grid_for(2 * n)), dim3(kTsThreads), 0, stream, 2 * n, sums.rep, sums.att, sums.z, exaggeration, momentum,
                       learning_rate, advance, d_y, d_vel, d_gain, d_grad);
    return 0;
}

int launch_tsne_kl(hipStream_t stream, const double* d_y, int64_t m, const int32_t* d_src, const int32_t* d_col, const double* d_p,
                   const TsneSums& sums, double* d_kl) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_tsne_kl, dim3(grid_for(m)), dim3(kTsThreads), 0, stream, (const double2*)d_y, m, d_src, d_col, d_p, sums.z, d_kl);
    return 0;
}

int launch_tsne_fill(hipStream_t stream, double* d_x, int64_t count, double value) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL(k_tsne_fill, dim3(grid_for(count)), dim3(kTsThreads), 0, stream, d_x, count, value);
    return 0;
}

}  // namespace mvs
