// mvs_core.h -- declarations of the HDBSCAN* units (not installed): the core pass of mvs_core.hip and the launches of
// mvs_linkage.hip that take core values.  Kept beside mvs_internal.h, which describes the kernels of the comparison.
#ifndef MVS_CORE_H
#define MVS_CORE_H

#include "mvs_internal.h"

namespace mvs {

// the K-th best score of every row out of a top-k cell list (mvs_core.hip): n_cells cells sorted by (row, col), rows in
// [row0, row0 + rows) of the n samples, at most k per row.  d_keys / d_counts: rows words each of scratch.  -> d_core[0 .. rows),
// the entry of row row0 first: the smallest score of a row that has k cells (-0.0 as +0.0), NaN for a row that has fewer
int launch_core_kth(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, int64_t row0, int64_t rows, int k,
                    const double* d_norms_sq, int64_t n, int d, unsigned long long* d_keys, int* d_counts, double* d_core);

// the launches of mvs_internal.h that compute an edge's weight, with the core values of mvs_linkage_set_core: d_core == NULL is
// the plain weight J (what the declarations there do), else n doubles on the device and the weight is min(J, core[lo], core[hi])
int launch_link_select(hipStream_t stream, const LinkState& s, const double* d_core, const mvs_cell* d_cells, int64_t n_cells, int pass,
                       bool first);
int launch_link_hook(hipStream_t stream, const LinkState& s, const double* d_core, const mvs_cell* d_cells);
int link_sorted(hipStream_t stream, const LinkState& s, const double* d_core, mvs_link* d_tmp, mvs_link* d_links, void* d_scratch,
                size_t scratch_bytes, size_t* scratch_needed);

}  // namespace mvs

#endif
