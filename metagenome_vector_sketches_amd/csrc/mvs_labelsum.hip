// mvs_labelsum.hip -- per sample, the sums of quantised Jaccard distances to every group of a labelling, reduced to what a
// silhouette needs: the sum over the sample's own group and the nearest other group with its sum (mvs_label_sums,
// include/mvs_hip.h "Labelling quality").  The sample x group table is never stored and the number of groups is not bounded.
//
// Input.  The caller has put the samples into label order (mvs_capi_silhouette.hip), so every non-empty group is one interval
// of columns: segment s holds columns [seg_begin[s], seg_begin[s + 1]) and col_seg[j] names column j's segment.  Segments are
// numbered in ascending group id, so the tie rule "equal means go to the smaller id" is "to the smaller segment"; seg_id[s] is
// the id that is reported.  Rows are the same samples in the same order with the unlabelled ones behind the last column:
// row i < ld belongs to segment col_seg[i], a row >= ld to none.
//
// The weight of a cell is quantised_distance (mvs_weight_dev.h) of the int32 dot, taken in registers: the dots block is read
// once, 4 bytes per cell, and nothing is written back.  w(i, i) = 0.
//
// k_segment_nearest.  A wave owns a row and walks it 64 columns per trip, lane l taking column j0 + l.  A trip is one of two
// kinds.
//   * A trip that lies wholly inside ONE segment that goes on behind it -- the usual trip when groups are wide -- costs the load,
//     the weight and one add into a 64-bit partial sum that every lane keeps of its own columns of that segment; it reads no
//     segment ids.  This is the CARRIED segment: its number and its end sit in scalar registers.
//   * Any other trip is reduced by segments as k_core_kth does: six steps of "add the sum 2^s lanes up if that lane is still in
//     my run" leave a run's sum in its first lane (a run is an interval of lanes; by induction lane i holds the part
//     [i, i + 2^(s+1)) of its run after step s).  The first lane of a run whose segment ends in the trip closes the segment;
//     lane 0, whose run may have begun in an earlier trip, adds what is carried first -- a scalar partial from the trip the
//     segment began in, and the wave reduction of the lanes' partial sums if whole trips lay in between.  The run that reaches
//     lane 63 and goes on becomes the carried segment, its sum so far a scalar read from its first lane.
// At most one segment is carried at a time, and a labelling of narrow groups costs one segmented reduction per trip.
// Closing a segment: if it is the row's own, its sum is stored as own_sum.  Otherwise mean = (double)sum / (double)size, one
// IEEE division, and the lane keeps the smaller (mean, segment) of this and its best so far.  One wave reduction of
// (mean, segment, sum) ends the row.  No atomics, no LDS: sums are integers and every one is formed by one wave, so the result
// does not depend on the blocking; a lane's partial is at most ld x 2^30 < 2^61.
#include "mvs_labelsum.h"
#include "mvs_weight_dev.h"

#include <climits>

namespace mvs {

namespace {

constexpr int kSegWaves = 4;         // rows per workgroup

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the smaller (mean, segment) wins
struct Nearest {
    double mean;
    int seg;
    unsigned long long sum;
    __device__ __forceinline__ void offer(double m, int s, unsigned long long u) {
        if (m < mean || (m == mean && s < seg)) {
            mean = m;
            seg = s;
            sum = u;
        }
    }
};

// dots: rows x ld (row r of the block is sample row0 + r of the ordered range, column j its sample j); n2: the ordered norms;
// own_sum / near_group / near_sum: indexed by the ordered sample.  Every lane of a wave makes every trip: the shuffles are whole.
__global__ __launch_bounds__(64 * kSegWaves) void k_segment_nearest(const int32_t* __restrict__ dots, int64_t rows, int64_t ld, int64_t row0,
                                                                    const double* __restrict__ n2, const int32_t* __restrict__ col_seg,
                                                                    const int32_t* __restrict__ seg_begin, const int32_t* __restrict__ seg_id,
                                                                    double dd, double inv, int pow2, double floor_,
                                                                    unsigned long long* __restrict__ own_sum, int32_t* __restrict__ near_group,
                                                                    unsigned long long* __restrict__ near_sum) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t r = (int64_t)blockIdx.x * kSegWaves + wave;
    if (r >= rows) return;
    const int64_t row = row0 + r;
    const double n2r = n2[row];
    const int own = row < ld ? col_seg[row] : -1;
    const int32_t* __restrict__ drow = dots + r * ld;

    Nearest best{__longlong_as_double(0x7ff0000000000000LL), INT_MAX, 0ULL};
    auto close = [&](int s, unsigned long long sum, int size) {
        if (s == own) {
            own_sum[row] = sum;
        } else {
            best.offer((double)sum / (double)size, s, sum);
        }
    };
    int carry_seg = -1;                          // wave-uniform: the carried segment (-1: none), its end column,
    int64_t carry_end = 0;
    unsigned long long carry_part = 0;           // its sum over the trip it began in
    bool carry_whole = false;                    // whole trips lay inside it:
    unsigned long long carry = 0;                // this lane's part of their sum

    for (int64_t j0 = 0; j0 < ld; j0 += 64) {
        const int64_t j = j0 + lane;
        const bool valid = j < ld;
        uint32_t w = 0;
        if (valid && j != row) w = quantised_distance(drow[j], n2r, n2[j], dd, inv, pow2 != 0, floor_);
        if (carry_seg >= 0 && carry_end > j0 + 64) {             // the whole trip lies in the carried segment, which goes on
            carry += w;
            carry_whole = true;
            continue;
        }
        int seg = -1;
        int64_t sb = 0, se = 0;
        if (valid) {
            seg = col_seg[j];
            sb = seg_begin[seg];
            se = seg_begin[seg + 1];
        }
        unsigned long long sum = w;
        const int64_t to = se - 1 - j0;
        const int last = valid ? (int)(to < 63 ? to : 63) : lane;    // the last lane of my run
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = __shfl_down(sum, (unsigned)off, 64);
            if (lane + off <= last) sum += o;
        }
        if (carry_seg >= 0) {                                    // it ends in this trip, and lane 0 leads its last run
            unsigned long long before = carry_part;
            if (carry_whole) before += wave_sum(carry);
            if (lane == 0) sum += before;
            carry_seg = -1;
        }
        const bool first = valid && (lane == 0 || j == sb);
        if (first && se <= j0 + 64) close(seg, sum, (int)(se - sb));
        const int64_t se63 = (int64_t)__builtin_amdgcn_readlane((int)se, 63);     // (0 where lane 63 has no column)
        if (se63 > j0 + 64) {                                    // the run that reaches lane 63 goes on: carry it
            const int sb63 = __builtin_amdgcn_readlane((int)sb, 63);
            const int head = sb63 > j0 ? (int)(sb63 - j0) : 0;   // its first lane
            const unsigned long long part = __shfl(sum, head, 64);
            carry_part = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(part >> 32)) << 32) |
                         (unsigned)__builtin_amdgcn_readfirstlane((int)part);
            carry_seg = __builtin_amdgcn_readlane(seg, 63);
            carry_end = se63;
            carry = 0;
            carry_whole = false;
        }
    }
    // (the last segment ends at ld, in the last trip: nothing is carried here)
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const double om = __shfl_xor(best.mean, off, 64);
        const int os = __shfl_xor(best.seg, off, 64);
        const unsigned long long ou = __shfl_xor(best.sum, off, 64);
        best.offer(om, os, ou);
    }
    if (lane == 0) {
        const bool any = best.seg != INT_MAX;
        near_group[row] = any ? seg_id[best.seg] : -1;
        near_sum[row] = any ? best.sum : 0ULL;
        if (own < 0) own_sum[row] = 0ULL;
    }
}

}  // namespace

int launch_segment_nearest(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, const double* d_norms_sq, int d,
                           double floor_, const int32_t* d_col_seg, const int32_t* d_seg_begin, const int32_t* d_seg_id,
                           unsigned long long* d_own_sum, int32_t* d_near_group, unsigned long long* d_near_sum) {
    if (rows <= 0) return 0;
    if (ld <= 0 || ld > INT_MAX || rows > INT_MAX || row0 < 0 || d <= 0 || !(floor_ >= 0.0) || !(floor_ < 1.0)) return MVS_E_INVALID;
    const int pow2 = (d & (d - 1)) == 0;
    hipLaunchKernelGGL(k_segment_nearest, dim3((unsigned)((rows + kSegWaves - 1) / kSegWaves)), dim3(64 * kSegWaves), 0, stream, d_dots, rows, ld,
                       row0, d_norms_sq, d_col_seg, d_seg_begin, d_seg_id, (double)d, 1.0 / (double)d, pow2, floor_, d_own_sum, d_near_group,
                       d_near_sum);
    return 0;
}

}  // namespace mvs
