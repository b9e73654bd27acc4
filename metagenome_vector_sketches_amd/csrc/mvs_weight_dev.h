// mvs_weight_dev.h -- the fixed-point weight of a cell, w = rint((1 - k) * 2^30), from its dot and the two norms: the device
// function that k_dist_quantise (mvs_groups.hip) and k_segment_nearest (mvs_labelsum.hip) share, so that both evaluate the rule
// of include/mvs_hip.h "PERMANOVA" with the same operations in the same order.  A unit that includes this is built with
// -ffp-contract=off (Makefile): no two lines may be joined into a fused multiply-add.
#ifndef MVS_WEIGHT_DEV_H
#define MVS_WEIGHT_DEV_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mvs {

// w of the rule for i != j; pow2: d is a power of two and inv = 1 / d
__device__ __forceinline__ uint32_t quantised_distance(int32_t P, double n2r, double n2c, double dd, double inv, bool pow2, double floor_) {
#pragma clang fp contract(off)
    const double inter = pow2 ? (double)P * inv : (double)P / dd;
    const double s = n2r + n2c;
    const double den = s - inter;
    const double J = inter / den;
    const double k = !(J > floor_) ? 0.0 : (J > 1.0 ? 1.0 : J);
    const double t = 1.0 - k;
    return (uint32_t)rint(t * 1073741824.0);
}

// a = rint(k * 2^20), the similarity of the same cell: the operations of quantised_distance up to k, in its order, with its floor
// (include/mvs_hip.h "Communities")
__device__ __forceinline__ uint32_t quantised_similarity(int32_t P, double n2r, double n2c, double dd, double inv, bool pow2, double floor_) {
#pragma clang fp contract(off)
    const double inter = pow2 ? (double)P * inv : (double)P / dd;
    const double s = n2r + n2c;
    const double den = s - inter;
    const double J = inter / den;
    const double k = !(J > floor_) ? 0.0 : (J > 1.0 ? 1.0 : J);
    return (uint32_t)rint(k * 1048576.0);
}

}  // namespace mvs

#endif
