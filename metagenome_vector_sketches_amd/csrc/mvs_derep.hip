// mvs_derep.hip -- greedy dereplication over device lists of kept cells (mvs_derep_*), and the row gather of limb planes that
// puts a sketch set into priority order (mvs_sketch_set_gather).
//
// The rule (include/mvs_hip.h): walk the samples in priority order; a sample becomes a REPRESENTATIVE iff none of the samples
// linked to it that come earlier is a representative, otherwise it is a MEMBER of the earliest representative linked to it.
// That is the lexicographically first maximal independent set of the threshold graph.  The reference has no such step; the
// edge rule is its Jaccard (src/pairwise_comp_optimized.cpp:661-662) against a threshold, as mvs_search_block tests it.
//
// Rank space.  The kernels know no order: row index = position in the order, row 0 goes first.  The caller permutes the set
// (k_gather_rows) and the norms before the comparison and maps the answer back afterwards (k_derep_scatter).  With that, the
// cells a row needs -- (r, c) with c < r -- all sit in row r's own list, and the row blocks of the threshold comparison arrive
// in ascending order: when block [rb, re) arrives every row before rb is FINAL.  So nothing is stored between blocks: a
// block's list is read in the staging buffer and forgotten.
//
// One block [rb, re), and why the result is exact.
//   pre      every cell (r, c), c < rb, whose column is a representative lowers assign[r] to c (atomic min).  state[c] is
//            final, so after this launch assign[r] = the earliest representative linked to r among the rows before the block.
//   rounds   scan, then decide, each a launch of its own, so that scan reads the states the round started with and decide
//            the marks the whole scan left.  scan: a cell (r, c), rb <= c < r, whose column is a representative lowers
//            assign[r]; one whose column is undecided marks an undecided row r as blocked in this round.  decide, per
//            undecided row: assign[r] set -> MEMBER (a representative earlier in the order is linked to it: nothing that
//            happens later can make it a representative); else not blocked -> REPRESENTATIVE (every earlier neighbour is
//            decided and none is a representative: the pre-pass and this round's scan have seen them all); else it waits.
//            Induction over the rounds: every decision equals the sequential walk's.  The earliest undecided row of the block
//            has no undecided earlier neighbour, so it is decided: each round decides at least one row and the loop ends
//            after at most re - rb rounds -- a path in priority order needs exactly that many, a clique two.
//   last scan  a row that became a MEMBER early may be linked to a row before assign[r] that was still undecided then and
//            became a representative later.  Hence scan lowers assign[r] for rows of ANY state, and one more scan runs after
//            the last decide: then every column's state is final and assign[r] is the minimum over all representatives linked
//            to r -- the earliest one, whatever the order of the cells, however often a cell occurs.
//   link     a cell with c == assign[r] stores its (dot, q) for row r.  Copies of a cell carry equal values, so the plain
//            8-byte stores may race.
//   Cells with c >= r are ignored: a mirrored cell (c, r) belongs to row c's list, where it is (row, col) = (c, r) with
//   col < row.  Cells naming a row outside the block or a column outside [0, n) are counted and ignored (MVS_E_RANGE, the
//   rule of mvs_cluster_add_cells): they never index anything.
//   What is NOT assumed: that a workgroup sees another workgroup's stores inside a launch.  Across launches the kernel
//   boundary publishes everything.  Inside a launch only assign[] is read while others write it -- to skip the atomic when
//   the value is already small enough.  It only ever decreases, so a stale read is merely conservative: the atomic is issued
//   once too often, never once too few.  That read is what keeps a clique of 50 000 at about one atomic per row instead of
//   50 000 on one address.  blocked[r] receives the same value from every writer.
#include "mvs_internal.h"

namespace mvs {

namespace {

constexpr int kDrThreads = 256;

// one atomic per wave for a counter every lane may bump (the idiom of k_cluster_hook)
__device__ __forceinline__ void wave_count(unsigned long long* counter, bool mine) {
    const unsigned long long mask = __ballot(mine);
    if (mask == 0ULL) return;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(counter, (unsigned long long)__popcll(mask));
}

// a cell as one 16-byte load
__device__ __forceinline__ int4 load_cell(const mvs_cell* cells, int64_t i) {
    return *reinterpret_cast<const int4*>(cells + i);   // x row, y col, z dot, w q
}

__device__ __forceinline__ void lower_assign(int32_t* assign, int32_t r, int32_t c) {
    if (__hip_atomic_load(assign + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > c) atomicMin(assign + r, c);
}

__global__ __launch_bounds__(kDrThreads) void k_derep_init(int32_t* __restrict__ state, int32_t* __restrict__ assign,
                                                           int32_t* __restrict__ blocked, int2* __restrict__ link, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kDrThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDrThreads) {
        state[i] = kDerepUndecided;
        assign[i] = kDerepNone;
        blocked[i] = 0;
        link[i] = make_int2(0, -1);
    }
}

// counters: [0] += cells with row != col in range, [1] += cells out of range
__global__ __launch_bounds__(kDrThreads) void k_derep_pre(const mvs_cell* __restrict__ cells, int64_t n_cells,
                                                          const int32_t* __restrict__ state, int32_t* __restrict__ assign, int64_t n,
                                                          int64_t rb, int64_t re, unsigned long long* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kDrThreads;
    const int64_t trips = (n_cells + stride - 1) / stride;            // every lane makes every trip: the ballots are whole
    int64_t i = (int64_t)blockIdx.x * kDrThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        const bool in = i < n_cells;
        int4 v = make_int4(0, 0, 0, 0);
        if (in) v = load_cell(cells, i);
        const int32_t r = v.x, c = v.y;
        const bool bad = in && (r < rb || r >= re || c < 0 || c >= n);
        const bool ok = in && !bad;
        wave_count(counters + 0, ok && r != c);
        wave_count(counters + 1, bad);
        if (ok && c < rb && state[c] == kDerepRep) lower_assign(assign, r, c);
    }
}

__global__ __launch_bounds__(kDrThreads) void k_derep_scan(const mvs_cell* __restrict__ cells, int64_t n_cells,
                                                           const int32_t* __restrict__ state, int32_t* __restrict__ assign,
                                                           int32_t* __restrict__ blocked, int64_t rb, int64_t re, int round) {
    const int64_t stride = (int64_t)gridDim.x * kDrThreads;
    for (int64_t i = (int64_t)blockIdx.x * kDrThreads + threadIdx.x; i < n_cells; i += stride) {
        const int4 v = load_cell(cells, i);
        const int32_t r = v.x, c = v.y;
        if (r < rb || r >= re || c < rb || c >= r) continue;           // (c < r < re: the column is in range)
        const int32_t sr = state[r];
        if (sr == kDerepRep) continue;                                 // no representative is linked to it
        const int32_t sc = state[c];
        if (sc == kDerepRep) lower_assign(assign, r, c);
        else if (sc == kDerepUndecided && sr == kDerepUndecided) blocked[r] = round;
    }
}

// counters[2] += rows of the block that stay undecided
__global__ __launch_bounds__(kDrThreads) void k_derep_decide(int32_t* __restrict__ state, const int32_t* __restrict__ assign,
                                                             const int32_t* __restrict__ blocked, int64_t rb, int64_t re, int round,
                                                             unsigned long long* __restrict__ counters) {
    const int64_t rows = re - rb, stride = (int64_t)gridDim.x * kDrThreads;
    const int64_t trips = (rows + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kDrThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        bool waits = false;
        if (i < rows) {
            const int64_t r = rb + i;
            if (state[r] == kDerepUndecided) {
                if (assign[r] != kDerepNone) state[r] = kDerepMember;
                else if (blocked[r] != round) state[r] = kDerepRep;
                else waits = true;
            }
        }
        wave_count(counters + 2, waits);
    }
}

__global__ __launch_bounds__(kDrThreads) void k_derep_link(const mvs_cell* __restrict__ cells, int64_t n_cells,
                                                           const int32_t* __restrict__ assign, int2* __restrict__ link, int64_t rb,
                                                           int64_t re) {
    const int64_t stride = (int64_t)gridDim.x * kDrThreads;
    for (int64_t i = (int64_t)blockIdx.x * kDrThreads + threadIdx.x; i < n_cells; i += stride) {
        const int4 v = load_cell(cells, i);
        const int32_t r = v.x, c = v.y;
        if (r < rb || r >= re || c < 0 || c >= r) continue;
        if (assign[r] == c) link[r] = make_int2(v.z, v.w);
    }
}

// counters[4] += entries of the order outside [0, n) or naming a sample that was named before
__global__ __launch_bounds__(kDrThreads) void k_derep_order_check(const int32_t* __restrict__ order, int64_t n, int32_t* __restrict__ marks,
                                                                  unsigned long long* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kDrThreads;
    const int64_t trips = (n + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kDrThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        bool bad = false;
        if (i < n) {
            const int32_t s = order[i];
            bad = s < 0 || s >= n || atomicAdd(marks + s, 1) != 0;
        }
        wave_count(counters + 4, bad);
    }
}

// rows -> the caller's samples: rep_of[order[i]] = order[representative of row i]; the order is a permutation (checked)
__global__ __launch_bounds__(kDrThreads) void k_derep_scatter(const int32_t* __restrict__ state, const int32_t* __restrict__ assign,
                                                              const int2* __restrict__ link, const int32_t* __restrict__ order, int64_t n,
                                                              int32_t* __restrict__ rep_of, int32_t* __restrict__ link_dot,
                                                              int32_t* __restrict__ link_q, int32_t* __restrict__ sizes,
                                                              unsigned long long* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kDrThreads;
    const int64_t trips = (n + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kDrThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        bool rep = false;
        if (i < n) {
            rep = state[i] == kDerepRep;
            const int32_t rr = rep ? (int32_t)i : assign[i];           // (a member's assign is a row before it)
            const int32_t s = order ? order[i] : (int32_t)i, sr = order ? order[rr] : rr;
            const int2 l = link[i];
            rep_of[s] = sr;
            link_dot[s] = l.x;
            link_q[s] = l.y;
            atomicAdd(sizes + sr, 1);
        }
        wave_count(counters + 3, rep);
    }
}

// one lane per 16 bytes of the output; *n_bad += rows outside the source (one count per row: its first lane)
__global__ __launch_bounds__(kDrThreads) void k_gather_rows(const int8_t* __restrict__ src, int64_t n_src, const int32_t* __restrict__ rows,
                                                            int64_t n_rows, int64_t vec_per_row, int8_t* __restrict__ dst,
                                                            unsigned long long* __restrict__ n_bad) {
    const int64_t total = n_rows * vec_per_row, stride = (int64_t)gridDim.x * kDrThreads;
    const int64_t trips = (total + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kDrThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        bool bad = false;
        if (i < total) {
            const int64_t row = i / vec_per_row, v = i - row * vec_per_row;
            const int64_t from = rows[row];
            if (from < 0 || from >= n_src) bad = v == 0;
            else reinterpret_cast<int4*>(dst)[i] = reinterpret_cast<const int4*>(src)[from * vec_per_row + v];
        }
        wave_count(n_bad, bad);
    }
}

unsigned grid_for(int64_t items) {
    const int64_t blocks = (items + kDrThreads - 1) / kDrThreads;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, 1 << 16));
}

}  // namespace

int launch_derep_init(hipStream_t stream, const DerepState& s) {
    if (s.n <= 0) return 0;
    hipLaunchKernelGGL(k_derep_init, dim3(grid_for(s.n)), dim3(kDrThreads), 0, stream, s.state, s.assign, s.blocked, s.link, s.n);
    return 0;
}

int launch_derep_pre(hipStream_t stream, const DerepState& s, const mvs_cell* d_cells, int64_t n_cells, int64_t rb, int64_t re) {
    if (n_cells <= 0) return 0;
    hipLaunchKernelGGL(k_derep_pre, dim3(grid_for(n_cells)), dim3(kDrThreads), 0, stream, d_cells, n_cells, s.state, s.assign, s.n, rb, re,
                       s.counters);
    return 0;
}

int launch_derep_scan(hipStream_t stream, const DerepState& s, const mvs_cell* d_cells, int64_t n_cells, int64_t rb, int64_t re,
                      int round) {
    if (n_cells <= 0) return 0;
    hipLaunchKernelGGL(k_derep_scan, dim3(grid_for(n_cells)), dim3(kDrThreads), 0, stream, d_cells, n_cells, s.state, s.assign, s.blocked,
                       rb, re, round);
    return 0;
}

int launch_derep_decide(hipStream_t stream, const DerepState& s, int64_t rb, int64_t re, int round) {
    if (re <= rb) return 0;
    hipLaunchKernelGGL(k_derep_decide, dim3(grid_for(re - rb)), dim3(kDrThreads), 0, stream, s.state, s.assign, s.blocked, rb, re, round,
                       s.counters);
    return 0;
}

int launch_derep_link(hipStream_t stream, const DerepState& s, const mvs_cell* d_cells, int64_t n_cells, int64_t rb, int64_t re) {
    if (n_cells <= 0) return 0;
    hipLaunchKernelGGL(k_derep_link, dim3(grid_for(n_cells)), dim3(kDrThreads), 0, stream, d_cells, n_cells, s.assign, s.link, rb, re);
    return 0;
}

int launch_derep_order_check(hipStream_t stream, const int32_t* d_order, int64_t n, int32_t* d_marks, unsigned long long* d_counters) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_derep_order_check, dim3(grid_for(n)), dim3(kDrThreads), 0, stream, d_order, n, d_marks, d_counters);
    return 0;
}

int launch_derep_scatter(hipStream_t stream, const DerepState& s, const int32_t* d_order, int32_t* d_rep_of, int32_t* d_link_dot,
                         int32_t* d_link_q, int32_t* d_sizes) {
    if (s.n <= 0) return 0;
    hipLaunchKernelGGL(k_derep_scatter, dim3(grid_for(s.n)), dim3(kDrThreads), 0, stream, s.state, s.assign, s.link, d_order, s.n, d_rep_of,
                       d_link_dot, d_link_q, d_sizes, s.counters);
    return 0;
}

int launch_gather_rows(hipStream_t stream, const int8_t* d_src, int64_t n_src, const int32_t* d_rows, int64_t n_rows, int64_t row_bytes,
                       int8_t* d_dst, unsigned long long* d_bad) {
    if (n_rows <= 0) return 0;
    if (row_bytes <= 0 || row_bytes % 16 != 0) return MVS_E_INVALID;
    const int64_t vec_per_row = row_bytes / 16;
    hipLaunchKernelGGL(k_gather_rows, dim3(grid_for(n_rows * vec_per_row)), dim3(kDrThreads), 0, stream, d_src, n_src, d_rows, n_rows,
                       vec_per_row, d_dst, d_bad);
    return 0;
}

}  // namespace mvs
