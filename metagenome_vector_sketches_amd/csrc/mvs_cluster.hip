// mvs_cluster.hip -- single-linkage clusters (connected components) over device lists of kept cells (mvs_cluster_*).
//
// The comparison kernels answer "which pairs have a Jaccard estimate above t"; this unit turns those pairs into groups
// without a cell ever leaving the device: a lock-free union-find over parent[n] eats each list (hook, flatten, verify),
// and the finish kernels number the components and pick sizes and representatives.  The reference has no clustering; the
// edge rule is its Jaccard (src/pairwise_comp_optimized.cpp:661-662) against a threshold, as mvs_search_block tests it.
//
// The forest, and why the result is exact.
//   Invariant I: every value ever stored into parent[x] is <= x, and < x once x stops being a root.  parent[] starts as the
//   identity; a hook stores lo < hi into parent[hi]; a path-splitting or flatten store puts a value read further up x's own
//   chain, which is smaller still.  So every chain strictly descends: no cycles, every walk ends, and the root of a tree is
//   its smallest member -- which is what the cluster numbering (ascending smallest member) needs.
//   Invariant II: the partition of the samples into trees only ever coarsens, and every merge joins the two endpoints' trees
//   of some fed cell.  A hook is a compare-and-swap parent[hi]: hi -> lo, so it takes effect only while hi is a root and
//   can never overwrite another link; lo belongs to the other endpoint's tree and lo < hi, so lo is not in hi's tree (a
//   root is its tree's smallest member).  A splitting / flatten store moves x under a node y that some earlier walk reached
//   from x: y and x's present parent a are in the same tree (the partition never splits), and both reach that tree's root
//   over chains that descend from values < x, hence without passing through x -- replacing the edge x -> a by x -> y keeps
//   the tree's members together.
//   What is NOT assumed: that a workgroup sees another workgroup's stores inside a launch.  The eight XCDs' L2s are not
//   coherent with each other and a CU's L1 is never refreshed by other CUs' stores, so inside the hook and flatten
//   kernels parent[] is read and written with agent-scope atomics only (loads and stores that bypass the L1, a
//   compare-and-swap for the link), and a walk that still reads an older parent merely takes a detour: any value it can
//   read obeys I and II.  Whether a list's cells really ended up with both endpoints in one tree is not argued but CHECKED:
//   after hook and flatten, k_cluster_verify -- a launch of its own, so the kernel boundary has made every store visible
//   -- walks both endpoints of every fed cell to their roots and counts the cells whose roots differ.  The host repeats
//   hook -> flatten -> verify on the list until that count is zero (mvs_capi_cluster.hip).  A round that missed a union
//   for whatever reason is repaired by the next one; with the compare-and-swap hook one round is what normally happens.
//   Completeness: after the loop every fed cell's endpoints share a root, so trees are unions of components; by II they
//   are never more than components.  Hence labels, sizes, representatives depend on the edge SET only -- not on the order
//   of the cells, the blocking or the comparison path -- and equal a brute force bit for bit.  degree[] counts fed cells
//   (one atomic add per cell with row != col on degree[row]), so it is exact when every ordered pair is fed once.
//
// Representative: the member with the largest norms_sq, equal values to the smaller index, NaN below every number.  A
// double and an index are 96 bits, more than one atomic holds, so it takes two passes: an atomic max of the
// order-preserving key of norms_sq per cluster, then an atomic min of the index over the members that hold that key.
#include "mvs_internal.h"

#include <climits>

#include <rocprim/device/device_scan.hpp>

namespace mvs {

namespace {

constexpr int kClThreads = 256;

__device__ __forceinline__ int32_t uf_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void uf_store(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x; path splitting: every node passed is re-pointed at its grandparent
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x) {
    int32_t p = uf_load(parent + x);
    while (p != x) {
        const int32_t g = uf_load(parent + p);
        if (g != p) uf_store(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// the same walk without a store
__device__ __forceinline__ int32_t uf_root(const int32_t* parent, int32_t x) {
    int32_t p = uf_load(parent + x);
    while (p != x) {
        x = p;
        p = uf_load(parent + x);
    }
    return x;
}

// one atomic per wave for a counter every lane may bump
__device__ __forceinline__ void wave_count(unsigned long long* counter, bool mine) {
    const unsigned long long mask = __ballot(mine);
    if (mask == 0ULL) return;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(counter, (unsigned long long)__popcll(mask));
}

__global__ __launch_bounds__(kClThreads) void k_cluster_init(int32_t* __restrict__ parent, int32_t* __restrict__ degree, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kClThreads) {
        parent[i] = (int32_t)i;
        degree[i] = 0;
    }
}

// counters: [0] cells with row != col (this launch adds to it when `first`), [1] cells with an index outside [0, n)
__global__ __launch_bounds__(kClThreads) void k_cluster_hook(const mvs_cell* __restrict__ cells, int64_t n_cells,
                                                             int32_t* __restrict__ parent, int32_t* __restrict__ degree, int64_t n,
                                                             int first, unsigned long long* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kClThreads;
    const int64_t rounds = (n_cells + stride - 1) / stride;            // every lane makes every trip: the ballots are whole
    int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x;
    for (int64_t t = 0; t < rounds; ++t, i += stride) {
        int32_t r = 0, c = 0;
        bool in = i < n_cells;
        if (in) {
            r = cells[i].row;
            c = cells[i].col;
        }
        const bool bad = in && (r < 0 || c < 0 || r >= n || c >= n);
        const bool edge = in && !bad && r != c;
        if (first) {
            wave_count(counters + 0, edge);
            wave_count(counters + 1, bad);
            if (edge) atomicAdd(degree + r, 1);
        }
        if (!edge) continue;
        int32_t a = r, b = c;
        for (;;) {
            a = uf_find(parent, a);
            b = uf_find(parent, b);
            if (a == b) break;
            const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
            int32_t seen = hi;
            if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT))
                break;
            a = seen;                                                  // hi had a parent already (< hi): go on from there
            b = lo;
        }
    }
}

// every parent[x] -> the root of x (no hook runs beside this: roots stay roots)
__global__ __launch_bounds__(kClThreads) void k_cluster_flatten(int32_t* __restrict__ parent, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kClThreads) {
        const int32_t r = uf_root(parent, (int32_t)i);
        if (r != uf_load(parent + i)) uf_store(parent + i, r);
    }
}

// counters[2] += fed cells whose endpoints have different roots
__global__ __launch_bounds__(kClThreads) void k_cluster_verify(const mvs_cell* __restrict__ cells, int64_t n_cells,
                                                               const int32_t* __restrict__ parent, int64_t n,
                                                               unsigned long long* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kClThreads;
    const int64_t rounds = (n_cells + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x;
    for (int64_t t = 0; t < rounds; ++t, i += stride) {
        bool apart = false;
        if (i < n_cells) {
            const int32_t r = cells[i].row, c = cells[i].col;
            if (r != c && r >= 0 && c >= 0 && r < n && c < n) apart = uf_root(parent, r) != uf_root(parent, c);
        }
        wave_count(counters + 2, apart);
    }
}

// ---- finish ----
// is_root[i] for i < n, is_root[n] = 0 (its exclusive scan ends with the number of clusters); rep / sizes / best cleared
__global__ __launch_bounds__(kClThreads) void k_cluster_roots(const int32_t* __restrict__ parent, int64_t n, int32_t* __restrict__ is_root,
                                                              int32_t* __restrict__ sizes, int32_t* __restrict__ rep,
                                                              unsigned long long* __restrict__ best) {
    for (int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x; i <= n; i += (int64_t)gridDim.x * kClThreads) {
        is_root[i] = (i < n && parent[i] == (int32_t)i) ? 1 : 0;
        if (i < n) {
            sizes[i] = 0;
            rep[i] = INT_MAX;
            best[i] = 0ULL;
        }
    }
}

// order-preserving map of a double onto 64 unsigned bits; -0.0 folded into +0.0 (equal as doubles: they must tie), NaN -> 0,
// below every number (-inf maps to 0x000fffffffffffff)
__device__ __forceinline__ unsigned long long norm_key(double v) {
    if (!(v == v)) return 0ULL;
    if (v == 0.0) v = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}

// parent[] is flat (every entry a root), ids = exclusive scan of is_root: labels, sizes, the best norm key per cluster
__global__ __launch_bounds__(kClThreads) void k_cluster_label(const int32_t* __restrict__ parent, const int32_t* __restrict__ ids,
                                                              const double* __restrict__ norms_sq, int64_t n,
                                                              int32_t* __restrict__ labels, int32_t* __restrict__ sizes,
                                                              unsigned long long* __restrict__ best) {
    for (int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kClThreads) {
        const int32_t l = ids[parent[i]];
        labels[i] = l;
        atomicAdd(sizes + l, 1);
        atomicMax(best + l, norm_key(norms_sq[i]));
    }
}

__global__ __launch_bounds__(kClThreads) void k_cluster_rep(const int32_t* __restrict__ labels, const double* __restrict__ norms_sq,
                                                            const unsigned long long* __restrict__ best, int64_t n,
                                                            int32_t* __restrict__ rep) {
    for (int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kClThreads) {
        const int32_t l = labels[i];
        if (norm_key(norms_sq[i]) == best[l]) atomicMin(rep + l, (int32_t)i);
    }
}

unsigned grid_for(int64_t items) {
    const int64_t blocks = (items + kClThreads - 1) / kClThreads;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, 1 << 16));
}

}  // namespace

int launch_cluster_init(hipStream_t stream, int32_t* d_parent, int32_t* d_degree, int64_t n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_cluster_init, dim3(grid_for(n)), dim3(kClThreads), 0, stream, d_parent, d_degree, n);
    return 0;
}

int launch_cluster_hook(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, int32_t* d_parent, int32_t* d_degree, int64_t n,
                        bool first, unsigned long long* d_counters) {
    if (n_cells <= 0) return 0;
    hipLaunchKernelGGL(k_cluster_hook, dim3(grid_for(n_cells)), dim3(kClThreads), 0, stream, d_cells, n_cells, d_parent, d_degree, n,
                       first ? 1 : 0, d_counters);
    return 0;
}

int launch_cluster_flatten(hipStream_t stream, int32_t* d_parent, int64_t n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_cluster_flatten, dim3(grid_for(n)), dim3(kClThreads), 0, stream, d_parent, n);
    return 0;
}

int launch_cluster_verify(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, const int32_t* d_parent, int64_t n,
                          unsigned long long* d_counters) {
    if (n_cells <= 0) return 0;
    hipLaunchKernelGGL(k_cluster_verify, dim3(grid_for(n_cells)), dim3(kClThreads), 0, stream, d_cells, n_cells, d_parent, n, d_counters);
    return 0;
}

// d_parent flat.  d_ids: n + 1 int32 (ids[n] = the number of clusters on return); d_labels, d_sizes, d_rep: n int32; d_best: n
// 64-bit words; scratch as rocprim's scan wants it (d_scratch == NULL: *scratch_needed only).
int cluster_finish(hipStream_t stream, const int32_t* d_parent, const double* d_norms_sq, int64_t n, int32_t* d_is_root, int32_t* d_ids,
                   int32_t* d_labels, int32_t* d_sizes, int32_t* d_rep, unsigned long long* d_best, void* d_scratch,
                   size_t scratch_bytes, size_t* scratch_needed) {
    size_t need = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, need, d_is_root, d_ids, 0, (size_t)n + 1, rocprim::plus<int32_t>(), stream);
    if (e != hipSuccess) return MVS_E_HIP;
    if (scratch_needed) *scratch_needed = need;
    if (d_scratch == nullptr) return 0;
    if (scratch_bytes < need) return MVS_E_CAPACITY;
    hipLaunchKernelGGL(k_cluster_roots, dim3(grid_for(n + 1)), dim3(kClThreads), 0, stream, d_parent, n, d_is_root, d_sizes, d_rep, d_best);
    e = rocprim::exclusive_scan(d_scratch, need, d_is_root, d_ids, 0, (size_t)n + 1, rocprim::plus<int32_t>(), stream);
    if (e != hipSuccess) return MVS_E_HIP;
    if (n > 0) {
        hipLaunchKernelGGL(k_cluster_label, dim3(grid_for(n)), dim3(kClThreads), 0, stream, d_parent, d_ids, d_norms_sq, n, d_labels,
                           d_sizes, d_best);
        hipLaunchKernelGGL(k_cluster_rep, dim3(grid_for(n)), dim3(kClThreads), 0, stream, d_labels, d_norms_sq, d_best, n, d_rep);
    }
    return 0;
}

}  // namespace mvs
