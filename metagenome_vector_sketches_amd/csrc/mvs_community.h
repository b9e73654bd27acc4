// mvs_community.h -- declaration of the modularity-community unit (not installed): the kernels of mvs_community.hip.  Kept
// beside mvs_internal.h, which describes the kernels of the comparison.
#ifndef MVS_COMMUNITY_H
#define MVS_COMMUNITY_H

#include "mvs_internal.h"

namespace mvs {

// the borders of the local-moving paths (include/mvs_hip.h "Communities"): a vertex of degree <= kCommWaveDegree starts in the
// wave path (one wave, kCommWaveSlots table slots in LDS), one of degree <= kCommBlockDegree in the workgroup path
// (kCommBlockSlots slots in LDS), the rest in the global path (a table of >= 2 * degree slots in device memory)
constexpr int kCommWaveDegree = 256, kCommWaveSlots = 128;
constexpr int kCommBlockDegree = 16384, kCommBlockSlots = 4096;
constexpr int kCommGlobalGroups = 128;     // workgroups of the global path, each with a table of its own
constexpr int kCommAcc = 8;                // 64-bit words of the round's accumulators (below)

// One level's graph on the device: a symmetric CSR without the diagonal (row_ptr n + 1, src / col m each: both directions of
// every edge), the weights as 32 bits (level 0) or 64 bits (coarser levels), self weights and strengths
struct CommLevel {
    int64_t n = 0, m = 0;
    const long long* row_ptr = nullptr;
    const int32_t* src = nullptr;
    const int32_t* col = nullptr;
    const uint32_t* w32 = nullptr;
    const unsigned long long* w64 = nullptr;
    const unsigned long long* self = nullptr;
    const unsigned long long* k = nullptr;
};

// what a round's kernels read besides the graph
struct CommRound {
    unsigned long long rw_hi = 0, rw_lo = 0;   // R * W
    unsigned long long g = 0;                  // the fixed-point resolution
    int level = 0, round = 0;
};

// cells -> (lo << 32 | hi, a) appended at d_keys[*count ...]; counters: [0] entries in the list, [1] cells / edges that name a
// sample outside [0, n), [2] raw edges with a weight outside [1, 2^20]
int launch_comm_cells(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, int64_t n, const double* d_norms_sq, int d, double floor_,
                      unsigned long long* d_keys, uint32_t* d_w, unsigned long long* d_counters);
int launch_comm_edges(hipStream_t stream, const int32_t* d_lo, const int32_t* d_hi, const int32_t* d_a, int64_t n_edges, int64_t n,
                      unsigned long long* d_keys, uint32_t* d_w, unsigned long long* d_counters);
// sorted by key, one entry per key with the larger weight: d_keys / d_w are rewritten in place, *d_count (device) := entries left.
// The two tmp arrays hold `count` entries each.
int comm_unique_max(hipStream_t stream, unsigned long long* d_keys, uint32_t* d_w, int64_t count, unsigned long long* d_tmp_keys,
                    uint32_t* d_tmp_w, unsigned long long* d_count);
// e unique edges -> 2 e directed entries sorted by (src, col): d_dir_keys / d_dir_w (2 e each; tmp the same)
int comm_mirror(hipStream_t stream, const unsigned long long* d_keys, const uint32_t* d_w, int64_t e, unsigned long long* d_dir_keys,
                uint32_t* d_dir_w, unsigned long long* d_tmp_keys, uint32_t* d_tmp_w);
// sorted directed keys -> row_ptr (n + 1), src, col (m each)
int launch_comm_csr(hipStream_t stream, const unsigned long long* d_dir_keys, int64_t m, int64_t n, long long* d_row_ptr, int32_t* d_src,
                    int32_t* d_col);
// k[v] = self[v] + the row's weights; *d_total += sum of k
int launch_comm_strength(hipStream_t stream, const CommLevel& g, unsigned long long* d_k, unsigned long long* d_total);
// the vertices of degree >= 1 into the three lists by the borders above (forced: 0 = by degree, 1 / 2 / 3 = all into the wave /
// workgroup / global list); d_counts: [0..2] list lengths, [3] the largest degree
int launch_comm_classify(hipStream_t stream, const CommLevel& g, int forced, int32_t* d_list0, int32_t* d_list1, int32_t* d_list2,
                         unsigned int* d_counts);
int launch_comm_identity(hipStream_t stream, int32_t* d_x, int64_t n);
// One path of the local moving over d_list[0 .. *d_list_count): next[v] of every active vertex that moves, *d_moved += moves.  A
// vertex whose table fills up is appended to d_over (counter d_over_count) untouched.  path 2: d_table holds groups * (slots * 12)
// bytes, slots a power of two >= 2 * the largest degree.
int launch_comm_move(hipStream_t stream, const CommLevel& g, int path, const CommRound& r, const int32_t* d_comm, int32_t* d_next,
                     const unsigned long long* d_tot, const int32_t* d_size, const int32_t* d_list, const unsigned int* d_list_count,
                     int64_t list_bound, int32_t* d_over, unsigned int* d_over_count, void* d_table, int64_t table_slots, int groups,
                     unsigned long long* d_moved);
// tot / size of the labelling (both cleared first); acc[0] += sum_v self + weights inside a community, acc[1..3] += sum of tot^2
// as limbs (bits 0..31, 32..63, 64..127)
int launch_comm_apply(hipStream_t stream, const CommLevel& g, const int32_t* d_comm, unsigned long long* d_tot, int32_t* d_size,
                      unsigned long long* d_acc);
// in(C) of every community id (d_inner, n entries, cleared first)
int launch_comm_inner_by(hipStream_t stream, const CommLevel& g, const int32_t* d_comm, unsigned long long* d_inner);
// communities numbered by smallest member: d_minm (n), d_flag / d_ids (n + 1; ids[n] = the count), d_new[v] = the new id of v's community
int comm_renumber(hipStream_t stream, const int32_t* d_comm, int64_t n, int32_t* d_minm, int32_t* d_flag, int32_t* d_ids, int32_t* d_new);
// member[s] = new[member[s]] for the n0 samples
int launch_comm_compose(hipStream_t stream, int32_t* d_member, int64_t n0, const int32_t* d_new);
// the next level: d_keys / d_vals (m each) := the directed cross entries (new[src] << 32 | new[col], w), ~0 keys for the rest;
// self2[new[v]] += self[v] + the weights inside; *d_cross += cross entries
int launch_comm_aggregate(hipStream_t stream, const CommLevel& g, const int32_t* d_new, unsigned long long* d_keys, unsigned long long* d_vals,
                          unsigned long long* d_self2, unsigned long long* d_cross);
// (keys, vals) sorted by key and summed per key into d_out_keys / d_out_vals; *d_count (device) := keys left
int comm_sum_by_key(hipStream_t stream, unsigned long long* d_keys, unsigned long long* d_vals, int64_t m, int64_t cross,
                    unsigned long long* d_tmp_keys, unsigned long long* d_tmp_vals, unsigned long long* d_count);
// the split's cell list of the directed entries [e0, e1): (src, col) where src < col share a community, (0, 0) otherwise
int launch_comm_split_cells(hipStream_t stream, const CommLevel& g, const int32_t* d_member, int64_t e0, int64_t e1, mvs_cell* d_cells);
// out[ids[v]] = in[comm[v]] for the first member v of every community (flag / ids of comm_renumber)
int launch_comm_gather_first(hipStream_t stream, const int32_t* d_comm, const int32_t* d_flag, const int32_t* d_ids, int64_t n,
                             const unsigned long long* d_in_a, const unsigned long long* d_in_b, unsigned long long* d_out_a,
                             unsigned long long* d_out_b);
int launch_comm_degree(hipStream_t stream, const CommLevel& g, int32_t* d_degree);

}  // namespace mvs

#endif
