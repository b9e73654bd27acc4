// mvs_kapply.hip -- the Jaccard kernel matrix applied to a thin block of vectors, straight from a block of int32 dots
// (mvs_jaccard_apply, mvs_pcoa_fit, mvs_pcoa_transform).  K is never stored: every cell is evaluated in a register and fed to
// the matrix cores as an A operand.
//
// The rule (the contract of mvs_jaccard_apply, include/mvs_hip.h).  Row i, column j by sample index, P the wrapped int32 dot,
// 0 <= floor < 1.  Everything is fp64 and every line is ONE rounding; a NaN compares false:
//     i == j : k = 1.0
//     i != j : inter = (double)P / (double)d
//              s     = n2[i] + n2[j]
//              den   = s - inter
//              J     = inter / den
//              k     = !(J > floor) ? 0.0 : (J > 1.0 ? 1.0 : J)
// -- the score of mvs_pairwise_topk with the writer's clamp.  It holds for any norms: NaN, +-inf, 0, negative.
//     Y[i - rb][c] = sum over j in [cb, ce) of k(i, j) * X[j - cb][c]
//
// Contraction.  As in mvs_levels.hip: no line may be joined with another into a fused multiply-add, so jaccard_k carries
// #pragma clang fp contract(off) and the Makefile builds the unit with -ffp-contract=off.
//
// The one shortcut.  Where d is a power of two (every real DB: 2048), (double)P / (double)d and (double)P * (1 / d) are the same
// double -- 1 / d is exact, the product of two doubles is rounded once, the quotient cannot leave the normal range for
// |P| <= 2^31 and d <= 2^30 -- so the first of the cell's two divisions becomes a multiply.  k stays bit-identical.
//
// Shape.  v_mfma_f64_16x16x4_f64: D (16 rows x 16 components) += A (16 rows x 4 columns) B (4 columns x 16 components); lane l
// holds A[l & 15][l >> 4], B[l >> 4][l & 15] and D[(l >> 4) + 4 r][l & 15] in register r.  So every lane evaluates the rule for
// ONE cell per instruction and the matrix cores do the "x X".  A workgroup of eight waves owns 16 rows and walks the column range
// in tiles of 128 columns; wave w takes columns 16 w .. 16 w + 15 of every tile.  A lane loads the four consecutive dots
// 4 q .. 4 q + 3 (q = l >> 4) of its row with one 16-byte load, so MFMA step s of a tile multiplies the cells of columns
// 4 q + s; the B operand of that step is row 4 q + s of the wave's slice of X, read straight from global memory (16 lanes x 8
// bytes = one 128-byte line per q: the slice is private to the wave, LDS staging would only add a round trip).  X arrives
// padded with zeros to whole tiles of 128 columns and to NB blocks of 16 components, so no load needs a bound.  The accumulators
// of all NB component blocks stay in registers for the whole column range.
//
// Order.  A wave's partial sums run over its columns in ascending tiles, inside a tile in the order the instruction fixes; the
// eight waves' partial sums are then added as (((w0 + w1) + w2) + ...) + w7 through one 16 x 16 NB block of LDS.  Every output element
// is its own chain: the order is a function of the column range and NB only, never of the row's place in its tile or block,
// so Y is the same bit for bit for every row blocking.  Cells outside the block (rows past its end, columns past the range)
// enter as k = 0 against X = 0.  No atomics.
#include "mvs_internal.h"

#include <climits>

namespace mvs {

namespace {

constexpr int kApplyRows = 16;    // rows per workgroup
constexpr int kApplyWaves = 8;    // waves per workgroup: the column range is cut over them
constexpr int kApplyTile = 16 * kApplyWaves;   // columns per tile: 16 per wave

using g4d = __attribute__((ext_vector_type(4))) double;

// k of the rule for i != j; pow2: d is a power of two and inv = 1 / d
__device__ __forceinline__ double jaccard_k(int32_t P, double n2r, double n2c, double dd, double inv, bool pow2, double floor_) {
#pragma clang fp contract(off)
    const double inter = pow2 ? (double)P * inv : (double)P / dd;
    const double s = n2r + n2c;
    const double den = s - inter;
    const double J = inter / den;
    return !(J > floor_) ? 0.0 : (J > 1.0 ? 1.0 : J);
}

// dots: rows x ld int32 (row r of the block is sample row0 + r, column j is sample c0 + j).  Xp: (ld rounded up to whole tiles) x
// 16 NB, zero-padded.  Y: rows x b.
template <int NB>
__global__ __launch_bounds__(64 * kApplyWaves) void k_jaccard_apply(const int32_t* __restrict__ dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                                                       const double* __restrict__ n2, double dd, double inv, int pow2, double floor_,
                                                       const double* __restrict__ Xp, int b, double* __restrict__ Y) {
#pragma clang fp contract(off)
    constexpr int CP = 16 * NB;
    __shared__ double part[kApplyRows * CP];
    const int t = threadIdx.x;
    const int wave = t >> 6, lane = t & 63;
    const int m = lane & 15, kq = lane >> 4;
    const int64_t r = (int64_t)blockIdx.x * kApplyRows + m;      // the lane's row of the block
    const bool row_in = r < rows;
    const int64_t row = row0 + r;
    const double n2r = row_in ? n2[row] : 0.0;
    const int32_t* __restrict__ dp = dots + (row_in ? r : 0) * ld;
    const bool vec = (ld & 3) == 0;                              // every row of the block is 16-byte aligned
    g4d acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = g4d{0.0, 0.0, 0.0, 0.0};

    int32_t P[4];
    double nc[4];
    auto fetch = [&](int64_t j) {                                // the lane's four cells: columns j .. j + 3 of its row
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            P[u] = 0;
            nc[u] = 0.0;
        }
        if (!row_in || j >= ld) return;
        if (vec) {                                               // ld % 4 == 0 and j % 4 == 0: j < ld implies j + 3 < ld
            const int4 v = *reinterpret_cast<const int4*>(dp + j);
            P[0] = v.x;
            P[1] = v.y;
            P[2] = v.z;
            P[3] = v.w;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (j + u < ld) P[u] = dp[j + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j + u < ld) nc[u] = n2[c0 + j + u];
    };
    const int64_t first = 16 * wave + 4 * kq;
    fetch(first);
    for (int64_t j = first; j - 4 * kq < ld; j += kApplyTile) {  // (the wave's 16 columns start below ld: uniform per wave)
        double kv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t col = j + u;
            kv[u] = (!row_in || col >= ld) ? 0.0 : (c0 + col == row) ? 1.0 : jaccard_k(P[u], n2r, nc[u], dd, inv, pow2 != 0, floor_);
        }
        const double* __restrict__ xr = Xp + j * CP + m;          // rows j .. j + 3 of the padded X: below its padded end
        double xb[4][NB];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) xb[u][nb] = xr[u * CP + nb * 16];
        fetch(j + kApplyTile);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[u], xb[u][nb], acc[nb], 0, 0, 0);
    }
    // (((w0 + w1) + w2) + ...) + w7: a wave at a time through the LDS block
    for (int w = 0; w < kApplyWaves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int rr = kq + 4 * q, j = nb * 16 + m;
                    const double v = w == 0 ? acc[nb][q] : part[rr * CP + j] + acc[nb][q];
                    if (w < kApplyWaves - 1) {
                        part[rr * CP + j] = v;
                    } else {
                        const int64_t ro = (int64_t)blockIdx.x * kApplyRows + rr;
                        if (ro < rows && j < b) Y[ro * b + j] = v;
                    }
                }
        }
        if (w < kApplyWaves - 1) __syncthreads();
    }
}

}  // namespace

int64_t apply_padded_cols(int64_t cols) { return (cols + kApplyTile - 1) / kApplyTile * kApplyTile; }
int apply_padded_b(int b) { return (b + 15) / 16 * 16; }

int launch_jaccard_apply(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                         const double* d_norms_sq, int d, double floor_, const double* d_Xp, int b, double* d_Y) {
    if (rows <= 0) return 0;
    if (ld <= 0 || ld > INT_MAX || rows > INT_MAX || d <= 0 || b < 1 || b > 128 || !(floor_ >= 0.0) || !(floor_ < 1.0)) return MVS_E_INVALID;
    const int pow2 = (d & (d - 1)) == 0;
    const unsigned blocks = (unsigned)((rows + kApplyRows - 1) / kApplyRows);
#define MVS_APPLY(NB) hipLaunchKernelGGL(k_jaccard_apply<NB>, dim3(blocks), dim3(64 * kApplyWaves), 0, stream, d_dots, rows, ld, row0, c0, d_norms_sq, \
                                         (double)d, 1.0 / (double)d, pow2, floor_, d_Xp, b, d_Y)
    switch ((b + 15) / 16) {
        case 1: MVS_APPLY(1); break;
        case 2: MVS_APPLY(2); break;
        case 3: MVS_APPLY(3); break;
        case 4: MVS_APPLY(4); break;
        case 5: MVS_APPLY(5); break;
        case 6: MVS_APPLY(6); break;
        case 7: MVS_APPLY(7); break;
        default: MVS_APPLY(8); break;
    }
#undef MVS_APPLY
    return 0;
}

}  // namespace mvs
