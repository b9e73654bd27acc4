// mvs_intersect_dev.h -- device code that the units-of-work kernels over sorted hash lists share (mvs_intersect.hip: counting
// |A n B|; mvs_gather.hip: marking the positions of Q that lie in H): the geometry of a unit and the wave-wide search.
#ifndef MVS_INTERSECT_DEV_H
#define MVS_INTERSECT_DEV_H

#include "mvs_internal.h"

namespace mvs {
namespace {

constexpr int kIxThreads = 256;                // 4 waves: 4 units in flight per workgroup
constexpr int kIxWaves = kIxThreads / 64;
constexpr int kTile = 1024;                    // elements of B a wave stages in LDS at a time (8 KiB per wave)
constexpr int kSkew = 32;                      // window / chunk ratio from which the window is searched in place

// First index i in [lo, hi) with !(arr[i] < key) (upper == false) or !(arr[i] <= key) (upper == true); hi if there is none.
// arr is non-decreasing on [lo, hi).  The whole wave calls it with the same arguments and gets the same answer.
template <typename T, typename I>
__device__ __forceinline__ I wave_bound(const T* __restrict__ arr, I lo, I hi, T key, bool upper, int lane) {
    // invariant: the answer lies in [lo, hi] (hi included)
    while (hi - lo > 64) {
        const I n = hi - lo;
        const I step = (n + 63) / 64;                                  // >= 2
        const I pos = lo + (I)(lane + 1) * step - 1;                   // splitter of this lane
        bool below = false;
        if (pos < hi) {
            const T v = arr[pos];
            below = upper ? (v <= key) : (v < key);
        }
        const int k = __popcll(__ballot(below));                       // splitters 0 .. k-1 are below: a prefix
        const I nlo = lo + (I)k * step;
        const I nhi = lo + (I)(k + 1) * step - 1;                      // splitter k is not below (if it exists)
        lo = nlo < hi ? nlo : hi;
        hi = (k < 64 && nhi < hi) ? nhi : hi;
    }
    bool below = false;
    const I pos = lo + (I)lane;
    if (pos < hi) {
        const T v = arr[pos];
        below = upper ? (v <= key) : (v < key);
    }
    return lo + (I)__popcll(__ballot(below));
}

// a wave's tile in LDS is final (or free again): its lanes run in lockstep, the compiler orders LDS stores and loads
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace
}  // namespace mvs

#endif
