// mvs_labelsum.h -- declaration of the labelling-quality unit (not installed): the segmented reduction of mvs_labelsum.hip.
// Kept beside mvs_internal.h, which describes the kernels of the comparison.
#ifndef MVS_LABELSUM_H
#define MVS_LABELSUM_H

#include "mvs_internal.h"

namespace mvs {

// per-sample sums of quantised distances to the groups of a labelling, reduced to the own group's sum and the nearest other
// group (mvs_labelsum.hip).  The samples are in label order: column j of the rows x ld dots block belongs to segment
// d_col_seg[j], segment s is columns [d_seg_begin[s], d_seg_begin[s + 1]) and reports the id d_seg_id[s]; row r of the block is
// ordered sample row0 + r, in segment d_col_seg[row0 + r] if row0 + r < ld and in none otherwise.  The outputs are indexed by
// the ordered sample.
int launch_segment_nearest(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t ld, int64_t row0, const double* d_norms_sq, int d,
                           double floor_, const int32_t* d_col_seg, const int32_t* d_seg_begin, const int32_t* d_seg_id,
                           unsigned long long* d_own_sum, int32_t* d_near_group, unsigned long long* d_near_sum);

}  // namespace mvs

#endif
