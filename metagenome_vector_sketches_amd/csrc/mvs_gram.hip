// mvs_gram.hip -- exact second moments of a sketch set over the SAMPLE axis (mvs_sketch_moments) and the device side of the PCA
// built on them (mvs_pca_fit, mvs_pca_transform).
//
// Every other matrix-core kernel of the library contracts over the dimension and yields X X^T (N x N).  A PCA needs X^T X
// (d x d), with the samples as the reduction axis.  mvs_pairwise_dots cannot be borrowed for a transposed set: its dots are
// wrapped mod 2^32, and a column's sum of squares passes 2^31 after a few thousand samples.
//
// Moments.  x[i][a] = sum_l limb_l[i][a] * W^l is the integer the planes encode (W = 256; the Karatsuba code: W = 128 and only
// its planes 0 and 1 are read).  With L limbs
//     gram[a][b] = sum_i x[i][a] x[i][b] = sum_{l,m} W^(l+m) G_lm[a][b],   G_lm[a][b] = sum_i limb_l[i][a] limb_m[i][b]
// and each G_lm is an int8 product the matrix cores do exactly.  Two passes per slab of samples:
//   k_gram_transpose  an operand fragment of v_mfma_i32_16x16x64_i8 wants, per lane, 16 consecutive SAMPLES of one dimension;
//                     in the planes those bytes lie P * d_pad apart.  The pass reads whole lines of the planes (64 samples x
//                     64 dimensions of one plane per workgroup), turns them through LDS and writes a dimension-major,
//                     fragment-major copy: fragment (sample block sb of 64, limb l, dimension block ab of 16) is 1 KiB at
//                     ((sb * L + l) * nab + ab) * 1024, lane = (sample / 16 % 4) * 16 + dimension % 16 holds its 16 samples --
//                     what a wave then loads with ONE coalesced instruction, as A or as B operand alike.  Samples outside the
//                     row range are written as zeros, so neither padding rows nor rows outside the range contribute.
//   k_gram_tiles      one workgroup per (64 x 64 output tile on or above the diagonal, chunk of the slab's sample blocks); wave
//                     w owns dimensions 16 w .. 16 w + 15 of the tile's rows against its 64 columns.  The 2 L - 1 accumulators
//                     per 16 x 16 block are indexed by l + m: pairs of equal weight share one, as in the comparison kernels.
//                     Bound: a chunk holds at most kGramChunkBlocks * 64 = 16 384 samples, at most L <= 4 pairs share an
//                     accumulator and |limb product| <= 128^2, so |accumulator| <= 4 * 2^14 * 2^14 = 2^30 < 2^31: int32 is
//                     exact.  (One pair alone would be safe up to 2^17 samples; the slab, which only bounds the scratch copy,
//                     is capped at 65 536.)  At the chunk's end the accumulators are recombined with their weights in 64-bit
//                     integers and added to gram[] with 64-bit integer atomics; tiles above the diagonal also add their mirror
//                     image (the weighted sum is symmetric because G_lm = G_ml^T).  Integer addition commutes and the true
//                     value fits int64 (the caller refuses n * B^2 > 2^62), so the result is exact and deterministic whatever
//                     the order; intermediate terms may wrap mod 2^64 without harm.  Only a < d and b < d are written: padding
//                     columns never reach the output.
//   k_gram_colsums    col_sums[a] = sum_i x[i][a], one thread per dimension and strip of rows, 64-bit atomics.
//
// PCA (fp64, deterministic: no floating-point atomics, every sum in a fixed order):
//   k_pca_matmul      Y = C Q for the d x d covariance and a block of b columns, one thread per output, k ascending
//   k_pca_ritz        V = Q S, W = Y S, R = W - V diag(theta): the Ritz vectors of the Rayleigh-Ritz step, C times them, and
//                     their residuals
//   k_pca_resnorm     res[i] = ||R[:, i]||_2, rows ascending
//   k_pca_scores      scores[i][j] = sum_a x[i][a] V[a][j] - off[j], off[j] = sum_a mean[a] V[a][j] (host): 64 rows per
//                     workgroup, dimensions in tiles of 32; the planes are read once and the integers rebuilt from the limbs
//                     in registers, the tile of V comes from L2 once per 64 rows into LDS, and the products run on the fp64
//                     matrix instruction (16 rows x 16 components x 4 dimensions).  Nothing of size N x c x anything exists.
#include "mvs_internal.h"

#include <climits>

namespace mvs {

namespace {

using g4i = __attribute__((ext_vector_type(4))) int;
using g2i = __attribute__((ext_vector_type(2))) int;

constexpr int kGramTile = 64;           // output tile edge (dimensions)
constexpr int kGramChunkBlocks = 256;   // sample blocks (of 64) per accumulator flush: 16 384 samples, see the bound above

// grid (dp / 64, sample blocks of the slab, L)
__global__ __launch_bounds__(256) void k_gram_transpose(const int8_t* __restrict__ planes, int P, int d_pad, int64_t row0, int64_t row_end,
                                                        int L, int nab, int8_t* __restrict__ T) {
    __shared__ unsigned tile[64][17];   // 64 samples x 64 bytes (+ 1 word: the column reads below spread over the banks)
    const int t = threadIdx.x;
    const int k0 = blockIdx.x * 64;
    const int64_t sb = blockIdx.y;
    const int plane = blockIdx.z;
    {
        const int r = t >> 2, seg = t & 3;
        const int64_t row = row0 + sb * 64 + r;
        const int k = k0 + seg * 16;
        g4i v = {0, 0, 0, 0};
        if (row < row_end && k < d_pad) v = *reinterpret_cast<const g4i*>(planes + (row * P + plane) * (int64_t)d_pad + k);
        tile[r][seg * 4 + 0] = (unsigned)v.x;
        tile[r][seg * 4 + 1] = (unsigned)v.y;
        tile[r][seg * 4 + 2] = (unsigned)v.z;
        tile[r][seg * 4 + 3] = (unsigned)v.w;
    }
    __syncthreads();
    const int f = t >> 6, ln = t & 63;
    const int dim = f * 16 + (ln & 15), sg = ln >> 4;
    const int word = dim >> 2, shift = (dim & 3) * 8;
    g4i out;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= ((tile[sg * 16 + q * 4 + j][word] >> shift) & 0xffu) << (8 * j);
        out[q] = (int)w;
    }
    *reinterpret_cast<g4i*>(T + ((size_t)(sb * L + plane) * nab + (k0 >> 4) + f) * 1024 + ln * 16) = out;
}

// grid (tiles on or above the diagonal, chunks of the slab)
template <int L>
__global__ __launch_bounds__(256) void k_gram_tiles(const int8_t* __restrict__ T, int nab, int n_tb, int slab_blocks, int chunk_blocks, int d,
                                                    unsigned long long W, unsigned long long* __restrict__ gram) {
    int ta = 0, idx = blockIdx.x;
    while (idx >= n_tb - ta) {
        idx -= n_tb - ta;
        ++ta;
    }
    const int tb = ta + idx;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int sb0 = blockIdx.y * chunk_blocks;
    const int sb1 = sb0 + chunk_blocks < slab_blocks ? sb0 + chunk_blocks : slab_blocks;
    g4i acc[2 * L - 1][4];
#pragma unroll
    for (int s = 0; s < 2 * L - 1; ++s)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[s][nb] = g4i{0, 0, 0, 0};
    const int8_t* base = T + lane * 16;
    const int ab = ta * 4 + wave;
    for (int sb = sb0; sb < sb1; ++sb) {
        g4i A[L];
#pragma unroll
        for (int l = 0; l < L; ++l) A[l] = *reinterpret_cast<const g4i*>(base + ((size_t)(sb * L + l) * nab + ab) * 1024);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int m = 0; m < L; ++m) {
                const g4i B = *reinterpret_cast<const g4i*>(base + ((size_t)(sb * L + m) * nab + tb * 4 + nb) * 1024);
#pragma unroll
                for (int l = 0; l < L; ++l) acc[l + m][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[l], B, acc[l + m][nb], 0, 0, 0);
            }
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = ta * kGramTile + wave * 16 + (lane >> 4) * 4 + r;
            const int b = tb * kGramTile + nb * 16 + (lane & 15);
            unsigned long long v = 0, w = 1;
#pragma unroll
            for (int s = 0; s < 2 * L - 1; ++s) {
                v += (unsigned long long)(long long)acc[s][nb][r] * w;
                w *= W;
            }
            if (a < d && b < d && v != 0) {
                atomicAdd(&gram[(size_t)a * d + b], v);
                if (ta != tb) atomicAdd(&gram[(size_t)b * d + a], v);
            }
        }
}

// The same for one or two limbs and d >= 128: a 128 x 128 output tile per workgroup, wave (wr, wc) owning its 64 x 64 quarter.  Per 64
// samples a wave loads 4 L A fragments once and 4 L B fragments for 16 L^2 MFMAs -- 0.25 KiB per MFMA at two limbs against
// the 0.625 of the 16 x 64 wave tile above, whose fragment loads, not its MFMAs, are what it waits for.  192 accumulator
// registers at two limbs: one wave per SIMD.  The last tile row / column may reach past the copy's dimension blocks (d rounded
// up to 64, not to 128): such a block index is clamped to the last one, its products land at a >= d or b >= d and are dropped.
template <int L>
__global__ __launch_bounds__(256) void k_gram_tiles_wide(const int8_t* __restrict__ T, int nab, int n_tb, int slab_blocks, int chunk_blocks,
                                                         int d, unsigned long long W, unsigned long long* __restrict__ gram) {
    int ta = 0, idx = blockIdx.x;
    while (idx >= n_tb - ta) {
        idx -= n_tb - ta;
        ++ta;
    }
    const int tb = ta + idx;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wr = wave >> 1, wc = wave & 1;
    const int sb0 = blockIdx.y * chunk_blocks;
    const int sb1 = sb0 + chunk_blocks < slab_blocks ? sb0 + chunk_blocks : slab_blocks;
    g4i acc[2 * L - 1][4][4];
#pragma unroll
    for (int s = 0; s < 2 * L - 1; ++s)
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[s][mb][nb] = g4i{0, 0, 0, 0};
    const int8_t* base = T + lane * 16;
    int abA[4], abB[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        abA[q] = ta * 8 + wr * 4 + q < nab ? ta * 8 + wr * 4 + q : nab - 1;
        abB[q] = tb * 8 + wc * 4 + q < nab ? tb * 8 + wc * 4 + q : nab - 1;
    }
    for (int sb = sb0; sb < sb1; ++sb) {
        g4i A[4][L];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int l = 0; l < L; ++l) A[mb][l] = *reinterpret_cast<const g4i*>(base + ((size_t)(sb * L + l) * nab + abA[mb]) * 1024);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int m = 0; m < L; ++m) {
                const g4i B = *reinterpret_cast<const g4i*>(base + ((size_t)(sb * L + m) * nab + abB[nb]) * 1024);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                    for (int l = 0; l < L; ++l)
                        acc[l + m][mb][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[mb][l], B, acc[l + m][mb][nb], 0, 0, 0);
            }
    }
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = ta * 128 + wr * 64 + mb * 16 + (lane >> 4) * 4 + r;
                const int b = tb * 128 + wc * 64 + nb * 16 + (lane & 15);
                unsigned long long v = 0, w = 1;
#pragma unroll
                for (int s = 0; s < 2 * L - 1; ++s) {
                    v += (unsigned long long)(long long)acc[s][mb][nb][r] * w;
                    w *= W;
                }
                if (a < d && b < d && v != 0) {
                    atomicAdd(&gram[(size_t)a * d + b], v);
                    if (ta != tb) atomicAdd(&gram[(size_t)b * d + a], v);
                }
            }
}

// the integer of (row, a): limbs from the highest down
__device__ __forceinline__ long long limb_value(const int8_t* __restrict__ p, int d_pad, int L, int W) {
    long long x = 0;
    for (int l = L - 1; l >= 0; --l) x = x * W + p[(int64_t)l * d_pad];
    return x;
}

// grid (ceil(d / 256), strips of rows_per rows)
__global__ __launch_bounds__(256) void k_gram_colsums(const int8_t* __restrict__ planes, int P, int d_pad, int d, int L, int W, int64_t rb,
                                                      int64_t re, int64_t rows_per, unsigned long long* __restrict__ sums) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= d) return;
    const int64_t r0 = rb + (int64_t)blockIdx.y * rows_per;
    const int64_t r1 = r0 + rows_per < re ? r0 + rows_per : re;
    long long s = 0;
    for (int64_t row = r0; row < r1; ++row) s += limb_value(planes + row * P * (int64_t)d_pad + a, d_pad, L, W);
    if (s != 0) atomicAdd(&sums[a], (unsigned long long)s);
}

// Y[a][j] = sum_k C[a][k] Q[k][j]; bp = the power of two >= b a row's threads are padded to
__global__ __launch_bounds__(256) void k_pca_matmul(const double* __restrict__ C, const double* __restrict__ Q, int d, int b, int bp,
                                                    double* __restrict__ Y) {
    const int j = threadIdx.x % bp;
    const int a = blockIdx.x * (256 / bp) + threadIdx.x / bp;
    if (a >= d || j >= b) return;
    const double* __restrict__ cr = C + (size_t)a * d;
    double acc = 0.0;
    for (int k = 0; k < d; ++k) acc = fma(cr[k], Q[(size_t)k * b + j], acc);
    Y[(size_t)a * b + j] = acc;
}

// V = Q S, W = Y S, R = W - V diag(theta); S[j * b + i] = component j of the i-th eigenvector of the projected matrix
__global__ __launch_bounds__(256) void k_pca_ritz(const double* __restrict__ Q, const double* __restrict__ Y, const double* __restrict__ S,
                                                  const double* __restrict__ theta, int d, int b, int bp, double* __restrict__ V,
                                                  double* __restrict__ Wm, double* __restrict__ R) {
    const int i = threadIdx.x % bp;
    const int a = blockIdx.x * (256 / bp) + threadIdx.x / bp;
    if (a >= d || i >= b) return;
    double v = 0.0, w = 0.0;
    for (int j = 0; j < b; ++j) {
        const double s = S[j * b + i];
        v = fma(Q[(size_t)a * b + j], s, v);
        w = fma(Y[(size_t)a * b + j], s, w);
    }
    V[(size_t)a * b + i] = v;
    Wm[(size_t)a * b + i] = w;
    R[(size_t)a * b + i] = fma(-theta[i], v, w);
}

__global__ __launch_bounds__(64) void k_pca_resnorm(const double* __restrict__ R, int d, int b, double* __restrict__ res) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= b) return;
    double s = 0.0;
    for (int a = 0; a < d; ++a) {
        const double r = R[(size_t)a * b + i];
        s = fma(r, r, s);
    }
    res[i] = sqrt(s);
}

constexpr int kScoreRows = 64;   // rows per workgroup
constexpr int kScoreKA = 32;     // dimensions per tile
constexpr int kScoreXS = kScoreKA + 4;   // row stride of the x tile in doubles: lanes (row, k quarter) of an A read fall on every bank pair twice

using g4d = __attribute__((ext_vector_type(4))) double;

// v_mfma_f64_16x16x4_f64: D (16 rows x 16 components) += A (16 rows x 4 dimensions) B (4 dimensions x 16 components); lane l holds
// A[l & 15][l >> 4], B[l >> 4][l & 15] and D[(l >> 4) + 4 r][l & 15] in register r.  Wave w owns rows 16 w .. 16 w + 15 of the
// workgroup's 64 against NB blocks of 16 components.  Per 4 dimensions a lane reads 1 + NB doubles from LDS for NB MFMAs: the
// vector-ALU form this replaces (a thread per row, 4 components each, V as LDS broadcasts) read 5 doubles per dimension and was
// bound by them (0.54 ms at 100k x 2048, c = 16).  The order of the sum over a is fixed by the instruction, the same every run.
template <int NB>
__global__ __launch_bounds__(256) void k_pca_scores(const int8_t* __restrict__ planes, int P, int d_pad, int d, int L, double W, int64_t rb,
                                                    int64_t re, const double* __restrict__ V, const double* __restrict__ off, int c,
                                                    double* __restrict__ scores) {
    constexpr int CP = 16 * NB;
    constexpr int VS = NB % 2 == 0 ? CP + 16 : CP;   // row stride of the V tile: the four k quarters of a B read two bank pairs apart
    __shared__ double xs[kScoreRows * kScoreXS];
    __shared__ double vs[kScoreKA * VS];
    const int t = threadIdx.x;
    const int64_t row0 = rb + (int64_t)blockIdx.x * kScoreRows;
    const int lr = t >> 2, seg = t & 3;   // loading: row of the block, 8 dimensions of the tile
    const int wave = t >> 6, lane = t & 63;
    const int m = lane & 15, kq = lane >> 4;
    g4d acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = g4d{0.0, 0.0, 0.0, 0.0};
    // the next tile's bytes and its part of V are fetched into registers while the matrix instructions of this one run
    constexpr int VU = kScoreKA * CP / 256;
    const int64_t lrow = row0 + lr;
    g2i pv[kMaxLimbs];
    double pw[VU];
    auto fetch = [&](int k0) {
        const int k = k0 + seg * 8;
        const bool in = lrow < re && k < d;                        // k is a multiple of 8 and k < d <= d_pad: the 8 bytes are in the row
#pragma unroll
        for (int l = 0; l < kMaxLimbs; ++l)
            pv[l] = (in && l < L) ? *reinterpret_cast<const g2i*>(planes + (lrow * P + l) * (int64_t)d_pad + k) : g2i{0, 0};
#pragma unroll
        for (int u = 0; u < VU; ++u) {
            const int i = t + u * 256, a = k0 + i / CP, j = i % CP;
            pw[u] = (a < d && j < c) ? V[(size_t)a * c + j] : 0.0;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < d; k0 += kScoreKA) {
        {
            const int k = k0 + seg * 8;
            double x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = 0.0;
#pragma unroll
            for (int l = kMaxLimbs - 1; l >= 0; --l)
                if (l < L) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)                    // integers below 2^53: every fma is exact
                        x[e] = fma(x[e], W, (double)(signed char)(((unsigned)pv[l][e >> 2] >> ((e & 3) * 8)) & 0xffu));
                }
#pragma unroll
            for (int e = 0; e < 8; ++e) xs[lr * kScoreXS + seg * 8 + e] = k + e < d ? x[e] : 0.0;
#pragma unroll
            for (int u = 0; u < VU; ++u) {
                const int i = t + u * 256;
                vs[(i / CP) * VS + i % CP] = pw[u];
            }
        }
        __syncthreads();
        if (k0 + kScoreKA < d) fetch(k0 + kScoreKA);
#pragma unroll
        for (int kk = 0; kk < kScoreKA / 4; ++kk) {
            const double A = xs[(wave * 16 + m) * kScoreXS + kk * 4 + kq];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
                acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(A, vs[(kk * 4 + kq) * VS + nb * 16 + m], acc[nb], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = row0 + wave * 16 + kq + 4 * r;
            const int j = nb * 16 + m;
            if (row < re && j < c) scores[(size_t)(row - rb) * c + j] = acc[nb][r] - off[j];
        }
}

inline int pow2_at_least(int b) {
    int p = 1;
    while (p < b) p <<= 1;
    return p;
}

}  // namespace

void gram_limbs(int code, int* L, int* W) {
    *L = is_k3(code) ? 2 : planes_of(code);
    *W = is_k3(code) ? 128 : 256;
}

size_t gram_scratch_bytes(int d, int code, int64_t slab_rows) {
    int L, W;
    gram_limbs(code, &L, &W);
    const size_t dp = (size_t)((d + 63) / 64) * 64;
    return (size_t)((slab_rows + 63) / 64) * 64 * L * dp;
}

int launch_gram_slab(hipStream_t stream, const int8_t* d_planes, int code, int d, int d_pad, int64_t row0, int64_t row_end, int8_t* d_T,
                     unsigned long long* d_gram, int variant) {
    const int64_t n = row_end - row0;
    if (n <= 0) return 0;
    if (d <= 0 || d > d_pad || (d_pad & 15) || !limb_code_ok(code) || n > 65536) return MVS_E_INVALID;
    int L, W;
    gram_limbs(code, &L, &W);
    const int P = planes_of(code);
    const int n_tb = (d + 63) / 64, nab = n_tb * 4;
    const int slab_blocks = (int)((n + 63) / 64);
    hipLaunchKernelGGL(k_gram_transpose, dim3((unsigned)n_tb, (unsigned)slab_blocks, (unsigned)L), dim3(256), 0, stream, d_planes, P, d_pad,
                       row0, row_end, L, nab, d_T);
    // chunks: enough workgroups to fill the device where the tiles alone do not, at least 8 sample blocks each (the atomics of a
    // chunk's flush are paid per chunk), at most kGramChunkBlocks (the int32 bound)
    const bool wide = L <= 2 && d >= 128 && variant != 1;
    const int n_t = wide ? (d + 127) / 128 : n_tb;
    const long long tiles = (long long)n_t * (n_t + 1) / 2;
    const long long want_wgs = wide ? 1024 : 2048;
    const long long want_chunks = (want_wgs + tiles - 1) / tiles;
    int chunk_blocks = (int)((slab_blocks + want_chunks - 1) / want_chunks);
    if (chunk_blocks < 8) chunk_blocks = 8;
    if (chunk_blocks > kGramChunkBlocks) chunk_blocks = kGramChunkBlocks;
    const int chunks = (slab_blocks + chunk_blocks - 1) / chunk_blocks;
    if (tiles > INT_MAX) return MVS_E_INVALID;
    const dim3 grid((unsigned)tiles, (unsigned)chunks);
#define MVS_GRAM(K, LL) hipLaunchKernelGGL(K<LL>, grid, dim3(256), 0, stream, d_T, nab, n_t, slab_blocks, chunk_blocks, d, \
                                           (unsigned long long)W, d_gram)
    if (wide && L == 1) MVS_GRAM(k_gram_tiles_wide, 1);
    else if (wide) MVS_GRAM(k_gram_tiles_wide, 2);
    else if (L == 1) MVS_GRAM(k_gram_tiles, 1);
    else if (L == 2) MVS_GRAM(k_gram_tiles, 2);
    else if (L == 3) MVS_GRAM(k_gram_tiles, 3);
    else MVS_GRAM(k_gram_tiles, 4);
#undef MVS_GRAM
    return 0;
}

int launch_gram_colsums(hipStream_t stream, const int8_t* d_planes, int code, int d, int d_pad, int64_t rb, int64_t re,
                        unsigned long long* d_sums) {
    const int64_t n = re - rb;
    if (n <= 0) return 0;
    if (d <= 0 || !limb_code_ok(code)) return MVS_E_INVALID;
    int L, W;
    gram_limbs(code, &L, &W);
    int64_t rows_per = (n + 16383) / 16384;
    if (rows_per < 256) rows_per = 256;
    const int64_t strips = (n + rows_per - 1) / rows_per;
    hipLaunchKernelGGL(k_gram_colsums, dim3((unsigned)((d + 255) / 256), (unsigned)strips), dim3(256), 0, stream, d_planes, planes_of(code), d_pad,
                       d, L, W, rb, re, rows_per, d_sums);
    return 0;
}

int launch_pca_matmul(hipStream_t stream, const double* d_C, const double* d_Q, int d, int b, double* d_Y) {
    if (d <= 0 || b <= 0 || b > 128) return MVS_E_INVALID;
    const int bp = pow2_at_least(b), per = 256 / bp;
    hipLaunchKernelGGL(k_pca_matmul, dim3((unsigned)((d + per - 1) / per)), dim3(256), 0, stream, d_C, d_Q, d, b, bp, d_Y);
    return 0;
}

int launch_pca_ritz(hipStream_t stream, const double* d_Q, const double* d_Y, const double* d_S, const double* d_theta, int d, int b,
                    double* d_V, double* d_W, double* d_R, double* d_res) {
    if (d <= 0 || b <= 0 || b > 128) return MVS_E_INVALID;
    const int bp = pow2_at_least(b), per = 256 / bp;
    hipLaunchKernelGGL(k_pca_ritz, dim3((unsigned)((d + per - 1) / per)), dim3(256), 0, stream, d_Q, d_Y, d_S, d_theta, d, b, bp, d_V, d_W, d_R);
    hipLaunchKernelGGL(k_pca_resnorm, dim3((unsigned)((b + 63) / 64)), dim3(64), 0, stream, d_R, d, b, d_res);
    return 0;
}

int launch_pca_scores(hipStream_t stream, const int8_t* d_planes, int code, int d, int d_pad, int64_t rb, int64_t re, const double* d_V,
                      const double* d_off, int c, double* d_scores) {
    const int64_t rows = re - rb;
    if (rows <= 0) return 0;
    if (d <= 0 || c < 1 || c > 64 || !limb_code_ok(code) || (d_pad & 7)) return MVS_E_INVALID;
    const int64_t blocks = (rows + kScoreRows - 1) / kScoreRows;
    if (blocks > INT_MAX) return MVS_E_INVALID;
    int L, W;
    gram_limbs(code, &L, &W);
#define MVS_SCORES(NB) hipLaunchKernelGGL(k_pca_scores<NB>, dim3((unsigned)blocks), dim3(256), 0, stream, d_planes, planes_of(code), d_pad, d, \
                                          L, (double)W, rb, re, d_V, d_off, c, d_scores)
    if (c <= 16) MVS_SCORES(1);
    else if (c <= 32) MVS_SCORES(2);
    else if (c <= 48) MVS_SCORES(3);
    else MVS_SCORES(4);
#undef MVS_SCORES
    return 0;
}

}  // namespace mvs
