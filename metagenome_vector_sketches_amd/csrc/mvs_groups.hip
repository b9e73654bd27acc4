// mvs_groups.hip -- within-group sums of squared Jaccard distances for many labellings at once, straight from a block of int32
// dots (mvs_group_sums, mvs_permanova).  The distance matrix is never stored: a block of rows is quantised in place and folded
// into per-(labelling, group) integers in the same visit.
//
// The weight of a cell (the contract of mvs_group_sums, include/mvs_hip.h).  k(i, j) is the rule of mvs_jaccard_apply
// (mvs_kapply.hip) word for word -- unit diagonal, the same floor, any norms.  Then, fp64, ONE rounding per line:
//     t = 1.0 - k(i, j)
//     w = (uint32) rint(t * 1073741824.0)                  2^30: 0 on the diagonal, 2^30 for k = 0
// k is symmetric bit for bit, so w is; every sum of w is an integer, hence independent of order, blocking and atomics.
//
// Contraction.  As in mvs_kapply.hip: no two lines may be joined into a fused multiply-add, so the rule carries
// #pragma clang fp contract(off) and the Makefile builds the unit with -ffp-contract=off.  The shortcut of mvs_kapply.hip holds
// here too: for d a power of two (double)P / (double)d is the multiply by the exact 1 / d, leaving ONE division per cell.
//
// k_dist_quantise.  Four consecutive cells of a row per lane of the rows x ld block: int32 dots in, uint32 w out, same bytes.
//
// k_labels_transpose.  The caller's label matrix is [slot][sample]; the sums read it [sample][slot], one 256-byte line per
// sample and tile of 256 slots, padded to whole tiles with the byte 255 (no label: labels are < groups <= 255).  Laid out once
// per call.
//
// k_group_sums.  Lanes own SLOTS, not cells: lane l of a wave owns slots 256 t + 4 l .. + 3 of slot tile t (one packed dword
// of labels per sample).  A wave owns kGroupRows rows of the block and keeps their packed labels in registers; it walks a chunk
// of the column range 64 columns at a time: lane l fetches the rows' weights of column j0 + l (one coalesced line per row), then
// per column the wave loads that sample's packed labels (64 lanes x 4 bytes: one coalesced line, shared by the wave's rows)
// and reads the cell's w out of its lane into a scalar register -- it is the same for every lane.  Per (cell, slot): a byte
// compare, a select and a 64-bit integer add into a register accumulator.  Nothing is reduced across lanes.  At the end of
// the chunk each lane adds its per-(row, slot) totals to acc[slot][label of the row] with 64-bit integer atomics: integer, so deterministic.  The four
// waves of a workgroup take four consecutive row groups of the same slot tile, so their column-label loads hit the same lines
// at about the same time; the tile does not go through LDS (145 vector instructions follow each 256-byte load).
//
// The sums are over ORDERED pairs: the whole rectangle rows x F.  The host adds the blocks in 128 bits and halves (the diagonal
// weighs 0).  Wrap: a lane's accumulator is at most cols x 2^30 and acc[slot][group] at most rows x ld x 2^30 per block; the
// launch refuses rows x ld >= 2^34, and the caller sizes its blocks under that bound and clears acc between them.
#include "mvs_internal.h"
#include "mvs_weight_dev.h"      // quantised_distance: the weight of a cell, shared with mvs_labelsum.hip

#include <climits>

namespace mvs {

namespace {

constexpr int kGroupRows = 8;        // rows per wave: 8 x 4 slots x 64-bit accumulators = 64 registers
constexpr int kGroupWaves = 4;       // waves per workgroup: consecutive row groups of one slot tile
constexpr int kGroupTile = 256;      // slots per tile: 64 lanes x 4 packed labels
constexpr int kGroupMinCols = 64;    // shortest column chunk of a workgroup

// cells: rows x ld, int32 dots in, uint32 weights out (row r of the block is sample row0 + r, column j is sample c0 + j); a lane
// takes four consecutive cells of a row, with one 16-byte load and store where every row of the block is 16-byte aligned
__global__ __launch_bounds__(256) void k_dist_quantise(int32_t* __restrict__ cells, int64_t rows, int64_t ld, int64_t row0, int64_t c0,
                                                       const double* __restrict__ n2, double dd, double inv, int pow2, double floor_) {
#pragma clang fp contract(off)
    const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const int64_t r = blockIdx.y;
    if (j >= ld || r >= rows) return;
    const int64_t row = row0 + r;
    const double n2r = n2[row];
    int32_t* cell = cells + r * ld + j;
    if ((ld & 3) == 0) {                                         // ld % 4 == 0 and j % 4 == 0: j < ld implies j + 3 < ld
        const int4 v = *reinterpret_cast<const int4*>(cell);
        const int32_t P[4] = {v.x, v.y, v.z, v.w};
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = row == c0 + j + u ? 0u : quantised_distance(P[u], n2r, n2[c0 + j + u], dd, inv, pow2 != 0, floor_);
        *reinterpret_cast<uint4*>(cell) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int u = 0; u < 4 && j + u < ld; ++u) {
            const uint32_t w = row == c0 + j + u ? 0u : quantised_distance(cell[u], n2r, n2[c0 + j + u], dd, inv, pow2 != 0, floor_);
            reinterpret_cast<uint32_t*>(cell)[u] = w;
        }
    }
}

// labels: slots x m bytes -> packed: m x (tiles * 64) dwords, dword q of sample j = labels of slots 4 q .. 4 q + 3 (255 past the end)
__global__ __launch_bounds__(256) void k_labels_transpose(const uint8_t* __restrict__ labels, int64_t slots, int64_t m, int64_t quads,
                                                          uint32_t* __restrict__ packed) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t q = blockIdx.y;
    if (j >= m || q >= quads) return;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int64_t s = 4 * q + b;
        const uint32_t l = s < slots ? labels[s * m + j] : 255u;
        v |= l << (8 * b);
    }
    packed[j * quads + q] = v;
}

// w: rows x ld quantised weights (row r of the block is sample f0 + r of the range, column j sample j of the range).
// packed: the transposed labels of the range, `quads` dwords per sample.  acc: slots x groups.
// grid: x = groups of kGroupWaves * kGroupRows rows, y = slot tiles, z = column chunks of `chunk` columns.
// Three waves per SIMD: asked for that, the compiler fits the 64 accumulator registers, four columns of labels in flight and
// the compare masks into 159 vector registers without a spill; left alone it takes 180 and two waves.
__global__ __attribute__((amdgpu_waves_per_eu(3, 3))) __launch_bounds__(64 * kGroupWaves) void k_group_sums(const uint32_t* __restrict__ w, int64_t rows, int64_t ld, int64_t f0, int64_t chunk,
                                                                 const uint32_t* __restrict__ packed, int64_t quads, int64_t slots, int groups,
                                                                 unsigned long long* __restrict__ acc) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t r0 = ((int64_t)blockIdx.x * kGroupWaves + wave) * kGroupRows;      // the wave's first row of the block
    if (r0 >= rows) return;
    const int64_t quad = (int64_t)blockIdx.y * 64 + lane;                            // below quads: quads is tiles * 64
    const int64_t c_begin = (int64_t)blockIdx.z * chunk;
    const int64_t c_end = c_begin + chunk < ld ? c_begin + chunk : ld;

    uint32_t rl[kGroupRows];                 // the rows' packed labels (a row past the block: the block's last row, weighing 0)
    unsigned long long sum[kGroupRows][4];
#pragma unroll
    for (int r = 0; r < kGroupRows; ++r) {
        const int64_t rr = r0 + r < rows ? r0 + r : rows - 1;
        rl[r] = packed[(f0 + rr) * quads + quad];
#pragma unroll
        for (int b = 0; b < 4; ++b) sum[r][b] = 0;
    }
    // 64 columns at a time: lane l fetches the rows' weights of column j0 + l (one coalesced line per row), then the columns
    // are walked with the weight read from its lane -- the same for every lane, so it sits in a scalar register
    auto cell = [&](const uint32_t (&wv)[kGroupRows], const uint32_t c, const int jj) {
#pragma unroll
        for (int r = 0; r < kGroupRows; ++r) {
            const uint32_t wj = __builtin_amdgcn_readlane(wv[r], jj);
            const uint32_t x = c ^ rl[r];
#pragma unroll
            for (int b = 0; b < 4; ++b) sum[r][b] += ((x >> (8 * b)) & 0xffu) == 0 ? wj : 0u;
        }
    };
    for (int64_t j0 = c_begin; j0 < c_end; j0 += 64) {
        const int64_t jl = j0 + lane;
        uint32_t wv[kGroupRows];
#pragma unroll
        for (int r = 0; r < kGroupRows; ++r) wv[r] = r0 + r < rows && jl < c_end ? w[(r0 + r) * ld + jl] : 0u;
        const uint32_t* __restrict__ cl = packed + j0 * quads + quad;
        if (c_end - j0 >= 64) {
#pragma unroll 4
            for (int jj = 0; jj < 64; ++jj) cell(wv, cl[(int64_t)jj * quads], jj);
        } else {
            const int n = (int)(c_end - j0);
            for (int jj = 0; jj < n; ++jj) cell(wv, cl[(int64_t)jj * quads], jj);
        }
    }
#pragma unroll
    for (int r = 0; r < kGroupRows; ++r)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t slot = 4 * quad + b;
            const uint32_t g = (rl[r] >> (8 * b)) & 0xffu;
            if (r0 + r < rows && slot < slots && g < (uint32_t)groups && sum[r][b]) atomicAdd(acc + slot * groups + g, sum[r][b]);
        }
}

}  // namespace

int64_t group_label_quads(int64_t slots) { return (slots + kGroupTile - 1) / kGroupTile * (kGroupTile / 4); }

int launch_dist_quantise(hipStream_t stream, int32_t* d_cells, int64_t rows, int64_t ld, int64_t row0, int64_t c0, const double* d_norms_sq,
                         int d, double floor_) {
    if (rows <= 0 || ld <= 0) return 0;
    if (ld > INT_MAX || rows > 65535 || d <= 0 || !(floor_ >= 0.0) || !(floor_ < 1.0)) return MVS_E_INVALID;
    const int pow2 = (d & (d - 1)) == 0;
    hipLaunchKernelGGL(k_dist_quantise, dim3((unsigned)((ld + 1023) / 1024), (unsigned)rows), dim3(256), 0, stream, d_cells, rows, ld, row0, c0,
                       d_norms_sq, (double)d, 1.0 / (double)d, pow2, floor_);
    return 0;
}

int launch_labels_transpose(hipStream_t stream, const uint8_t* d_labels, int64_t slots, int64_t m, uint32_t* d_packed) {
    if (slots <= 0 || m <= 0) return 0;
    const int64_t quads = group_label_quads(slots);
    if (m > INT_MAX || quads > 65535) return MVS_E_INVALID;
    hipLaunchKernelGGL(k_labels_transpose, dim3((unsigned)((m + 255) / 256), (unsigned)quads), dim3(256), 0, stream, d_labels, slots, m, quads,
                       d_packed);
    return 0;
}

int launch_group_sums(hipStream_t stream, const uint32_t* d_w, int64_t rows, int64_t ld, int64_t f0, const uint32_t* d_packed, int64_t slots,
                      int groups, unsigned long long* d_acc) {
    if (rows <= 0 || ld <= 0 || slots <= 0) return 0;
    // no wrap: acc[slot][group] gains at most rows x ld x 2^30 in one launch
    if (ld > INT_MAX || rows > INT_MAX || rows * ld >= (1LL << 34) || groups < 1 || groups > 255 || f0 < 0) return MVS_E_INVALID;
    const int64_t quads = group_label_quads(slots), tiles = quads / 64;
    const int64_t row_groups = (rows + kGroupWaves * kGroupRows - 1) / (kGroupWaves * kGroupRows);
    if (tiles > 65535) return MVS_E_INVALID;
    // enough workgroups to fill the device eight waves deep (2048 workgroups of four waves), never chunks under kGroupMinCols
    const int64_t want = std::max<int64_t>(1, 2048 / (row_groups * tiles));
    int64_t chunk = std::max<int64_t>(kGroupMinCols, (ld + want - 1) / want);
    int64_t chunks = (ld + chunk - 1) / chunk;
    if (chunks > 65535) {
        chunks = 65535;
        chunk = (ld + chunks - 1) / chunks;
        chunks = (ld + chunk - 1) / chunk;
    }
    hipLaunchKernelGGL(k_group_sums, dim3((unsigned)row_groups, (unsigned)tiles, (unsigned)chunks), dim3(64 * kGroupWaves), 0, stream, d_w, rows, ld,
                       f0, chunk, d_packed, quads, slots, groups, d_acc);
    return 0;
}

}  // namespace mvs
