// mvs_tsne.h -- declaration of the t-SNE unit (not installed): the kernels of mvs_tsne.hip.  Kept beside mvs_community.h, whose
// sum-by-key and CSR helpers the graph of affinities is built with.
#ifndef MVS_TSNE_H
#define MVS_TSNE_H

#include "mvs_internal.h"

namespace mvs {

constexpr int kTsneMaxNeighbours = 256;    // cells of a row the calibration holds in a wave's registers (top-k's K <= 256)
constexpr int kTsneRows = 256;             // rows of a repulsion unit: one per lane of its workgroup
constexpr int kTsneMaxSlice = 1024;        // columns of a repulsion unit at most (16 KiB of LDS); option tsne_slice_cols
constexpr int kTsneMinSlice = 16;
constexpr int kTsneCounters = 8;           // 64-bit words of the unit's counters

// the per-iteration integer accumulators, one allocation of (5 n + 1) words: Z_i, (Rx_i, Ry_i), (Ax_i, Ay_i), Z
struct TsneSums {
    long long* z_rows = nullptr;   // n
    long long* rep = nullptr;      // 2 n
    long long* att = nullptr;      // 2 n
    long long* z = nullptr;        // 1
};

// counters[0] += cells that name a sample outside [0, n) or have row == col, [1] += places where the rows descend, [2] += cells
// beyond the 256th of their row
int launch_tsne_check_cells(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, int64_t n, unsigned long long* d_counters);
// One wave per row of [row0, row0 + rows): beta by bisection, c = rint(p * 2^30) of every cell of the row.  Cell i of the list
// becomes the two entries 2 i and 2 i + 1 of d_keys / d_vals ((row << 32 | col, c) and (col << 32 | row, c)); d_beta is indexed by
// the sample, d_c (may be NULL) by the cell; counters[3] += rows left at beta = 0.  The list must have passed the check above.
int launch_tsne_calibrate(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, int64_t row0, int64_t rows, const double* d_norms_sq,
                          int d, double perplexity, double* d_beta, int32_t* d_c, unsigned long long* d_keys, unsigned long long* d_vals,
                          unsigned long long* d_counters);
// counters[0] += edges that name a sample outside [0, n) or have a weight below 1
int launch_tsne_check_edges(hipStream_t stream, const int32_t* d_lo, const int32_t* d_hi, const int32_t* d_s, int64_t n_edges, int64_t n,
                            unsigned long long* d_counters);
// edge i -> the entries 2 i and 2 i + 1; lo == hi -> two entries with the key ~0 (they sort behind the rest); counters[1] += those
int launch_tsne_edges(hipStream_t stream, const int32_t* d_lo, const int32_t* d_hi, const int32_t* d_s, int64_t n_edges,
                      unsigned long long* d_keys, unsigned long long* d_vals, unsigned long long* d_counters);
// *d_total += the sum of d_vals[0 .. m)
int launch_tsne_total(hipStream_t stream, const unsigned long long* d_vals, int64_t m, unsigned long long* d_total);
// P[k] = (double)vals[k] / (double)S
int launch_tsne_p(hipStream_t stream, const unsigned long long* d_vals, int64_t m, unsigned long long S, double* d_p);
// the hot path: all ordered pairs.  z_rows / rep += the units' integer sums (both must be cleared before); -> units launched
int launch_tsne_repulse(hipStream_t stream, const double* d_y, int64_t n, int slice_cols, const TsneSums& sums, int64_t* units);
// one wave per row over the CSR: att := the row's sums; *z += z_rows[row] >> 20 (after the repulsion, z cleared before)
int launch_tsne_attract(hipStream_t stream, const double* d_y, int64_t n, const long long* d_row_ptr, const int32_t* d_col, const double* d_p,
                        const TsneSums& sums);
// the gradient of every coordinate from the sums; d_grad (may be NULL) := it; advance: gain, velocity and y take one step
int launch_tsne_update(hipStream_t stream, int64_t n, const TsneSums& sums, double exaggeration, double momentum, double learning_rate,
                       int advance, double* d_y, double* d_vel, double* d_gain, double* d_grad);
// *d_kl += sum over the entries with P > 0 of P log(P / (q / Zd)), Zd from *sums.z (fp64 atomics: not bit-stable)
int launch_tsne_kl(hipStream_t stream, const double* d_y, int64_t m, const int32_t* d_src, const int32_t* d_col, const double* d_p,
                   const TsneSums& sums, double* d_kl);
// x[0 .. count) = value
int launch_tsne_fill(hipStream_t stream, double* d_x, int64_t count, double value);

}  // namespace mvs

#endif
