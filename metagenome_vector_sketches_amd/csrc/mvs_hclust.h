// mvs_hclust.h -- declaration of the average / complete linkage unit (not installed): the kernels of mvs_hclust.hip.  Kept
// beside mvs_internal.h, which describes the kernels of the comparison.
#ifndef MVS_HCLUST_H
#define MVS_HCLUST_H

#include "mvs_internal.h"

namespace mvs {

// The state of an agglomeration on the device (include/mvs_hip.h "Average and complete linkage").  The table has one row per
// slot, ld (even, >= m) entries apart; its columns follow a LAYOUT that starts as the identity and loses its dead columns at
// every compaction: column j holds slot col_slot[j], whose size is col_n[j] while it lives and 0 once it is dead (both arrays
// ld long; an odd layout's padding column has col_n = 0), and slot s sits in column slot_col[s].
struct HclustState {
    unsigned long long* table;
    int64_t ld;
    int32_t* col_slot;
    uint32_t* col_n;
    int32_t* slot_col;          // [m]
    int32_t* size;              // [m] n_s of a live slot
    int32_t* nearest;           // [m] of the round
    int32_t* pairs;             // [2 * (m / 2)] (a, b) of the round's merges, ascending in a
    int32_t* keep;              // [m] compaction: the old column of every new one
    int32_t* counters;          // [0] pairs of the round, [1] live rows after it, [2] flags of the input check
    mvs_hmerge* merges;         // [m - 1]
};

// rows x m int32 dots (row r is sample row0 + r, column j sample c0 + j) -> rows of the table from d_rows on: the weight of the
// cell, 0 on the diagonal and in the padding column
int launch_hclust_fill(hipStream_t stream, const int32_t* d_dots, int64_t rows, int64_t m, int64_t row0, int64_t c0, const double* d_norms_sq,
                       int d, double floor_, unsigned long long* d_rows, int64_t ld);
// m x m uint32 -> the table
int launch_hclust_widen(hipStream_t stream, const uint32_t* d_w, int64_t m, unsigned long long* d_table, int64_t ld);
// counters[2] |= 1 where S[i][j] != S[j][i], |= 2 where S[i][j] > n_i n_j 2^30, i < j
int launch_hclust_check(hipStream_t stream, const HclustState& st, int64_t m);
// nearest[r] of every row of d_live[0 .. n_live) over the layout's n_cols columns
int launch_hclust_nearest(hipStream_t stream, const HclustState& st, int method, const int32_t* d_live, int64_t n_live, int64_t n_cols);
// the round's mutual pairs in ascending a: records from merges[done] on, pairs[], sizes, col_n, the next live list, counters[0 .. 2)
int launch_hclust_pairs(hipStream_t stream, const HclustState& st, int method, const int32_t* d_live, int32_t* d_live_next, int64_t n_live,
                        int round, int64_t done);
// the column phase over the rows of d_live (the list from BEFORE the round's deaths), then the row phase
int launch_hclust_merge_cols(hipStream_t stream, const HclustState& st, int method, const int32_t* d_live, int64_t n_live, int64_t n_pairs);
int launch_hclust_merge_rows(hipStream_t stream, const HclustState& st, int method, int64_t n_pairs, int64_t n_cols);
// the layout without its dead columns (keep[], col_slot, col_n, slot_col), then the rows of d_live moved into it
int launch_hclust_layout(hipStream_t stream, const HclustState& st, int64_t n_cols);
int launch_hclust_compact(hipStream_t stream, const HclustState& st, const int32_t* d_live, int64_t n_live, int64_t n_cols_new);

}  // namespace mvs

#endif
