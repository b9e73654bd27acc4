// mvs_linkage.hip -- the single-linkage TREE over device lists of kept cells (mvs_linkage_*): the maximum spanning forest of the
// thresholded Jaccard graph, kept on the device while the row blocks of a comparison go by.
//
// mvs_cluster.hip keeps a partition: the answer for ONE level.  The maximum spanning forest of the same graph answers every
// level at or above the one it was built at (cutting it at u gives the components of the graph cut at u), has at most n - 1
// edges and is what these kernels maintain.  The reference has neither; the edge rule and the weight are its Jaccard
// (src/pairwise_comp_optimized.cpp:661-662), as mvs_search_block tests it and mvs_pairwise_topk scores it.
//
// Order.  An edge is a cell with row != col, both in [0, n), whose J = inter / (n2[lo] + n2[hi] - inter), inter = (double)dot / d,
// is not NaN (lo = min(row, col), hi = max: the sum of two doubles commutes, so J is the same for (r, c) and (c, r)).  Edges are
// totally ordered "best first" by (key(J) descending, lo ascending, hi ascending), key() = mvs_topk.hip's order-preserving
// map.  Two cells with the same (lo, hi) are the same edge: they carry the same dot, hence the same J.  Because the order is
// total the maximum spanning forest is unique -- a function of the edge set and the norms, nothing else.
//
// State: the forest F (at most n - 1 cells, row = lo, col = hi), comp[n], and three 64-bit selection slots per component.
// add_cells(L) replaces F by MSF(F u L), which is sound because MSF(E1 u E2) = MSF(MSF(E1) u E2) (an edge that is not the
// best across any cut of E1 is not the best across that cut of a superset).  It runs Boruvka rounds over the cells of F u L,
// starting from comp = identity; each phase below is a launch of its own:
//   slots    best_key[c] = 0, best_pair[c] = best_idx[c] = ~0, next[c] = c
//   key      every edge whose endpoints lie in different components: atomic max of key(J) into both components' best_key
//            (key() >= 1 for every non-NaN J, so 0 means "no edge"); counts those edges -- the host stops when there is none
//   pair     ... whose key equals its component's best_key: atomic min of lo << 32 | hi into best_pair
//   pick     ... that matches key and pair: atomic min of its index in F u L into best_idx (any copy would do: copies carry
//            the same dot; the smallest index makes the choice repeatable)
//   hook     a root c with a best edge e towards component o: next[c] = o and e is appended to the next forest -- unless o
//            chose the same edge and c < o: then c stays a root and appends nothing
//   flatten  next[c] := the root of c's chain, for every component c of this round
//   apply    comp[i] := next[comp[i]]
// A 128-bit order in 64-bit atomics is k_cluster_rep's two-pass idiom with one more pass.  (The alternative the design
// allowed -- a device sort of F u L by the order and one atomic on the rank -- sorts |F| + |L| 16-byte cells once per list
// to save two streaming passes per round; the passes read 16 B per cell, a radix sort moves each cell 8+ times.  Passes
// shipped.)  J is recomputed from dot and the norms wherever it is needed: nothing is stored per cell of L.
//
// Why the result is exact.
//   Selection.  After key / pair / pick, (best_key[c], best_pair[c]) is the best edge leaving c under the total order: the
//   maximum of an atomic max over a set is that set's maximum whatever the interleaving, likewise the minimum; each pass reads
//   the previous pass's slots only after the kernel boundary has made them final.
//   Hook.  Boruvka's step: the best edge leaving a component is in the MSF (cut property; unique because the order is strict).
//   An edge joins two components and only those two can choose it; if one does it appends the edge, if both do (a mutual
//   choice) the smaller one stands back: every forest edge is appended once.  The chosen edges
//   form no cycle other than those mutual pairs: along a chain c1 -> c2 -> ... each step's edge is at least as good as the
//   one before (c2 could have chosen c1's edge and chose something no worse), strictly better unless it is the same edge,
//   so a chain that came back to c1 would need an edge strictly better than itself.  With the mutual pairs broken, next[] is
//   a forest of chains that end in a root.
//   Visibility.  No phase relies on seeing another workgroup's plain stores inside a launch.  comp[] and the slots are
//   written in one launch and read in later ones; inside a launch the slots are touched with device-scope atomics only.  The
//   one structure read and written in the same launch is next[] in flatten -- there with agent-scope atomic loads and
//   stores (mvs_cluster.hip's uf_load / uf_store), and only ever overwritten by a root of the same chain: a walk that reads
//   the older value merely takes the longer way.  hook reads comp[] and the slots, which it does not write, and writes next[]
//   and the next forest, which it does not read.
//   Termination.  Every component that has an edge leaving it hooks or is hooked to, so a round at least halves the number
//   of components that still have one: at most ceil(log2 n) rounds.  The host loops on the count of crossing edges, read
//   back once per round; walks in flatten are bounded by n steps and report a longer one instead of spinning.
//   Hence F after add_cells is MSF(F u L) as a SET whatever the order of the cells, the blocking or the comparison path; its
//   order in memory is not defined, and finish sorts it (a total order: one result).
//
// Mutual reachability (mvs_linkage_set_core; HDBSCAN*, mvs_capi_hdbscan.hip).  With core values set, the weight of (lo, hi) is
// m = min(J, core[lo], core[hi]) by key order instead of J, and an edge with a NaN core value is ignored like one whose J is
// NaN.  lk_weight is the one place that decides it; select, hook and links read it through lk_edge / lk_weight, and the pointer
// is a parameter of their launches (mvs_core.h; the declarations of mvs_internal.h pass NULL).  Nothing in
// the argument above uses more of the weight than that it is a fixed function of the edge and the linkage's own arrays: the
// order (key(m) descending, lo, hi) is still total, so the forest is still unique and add_cells still exact.  Ties are far
// more common under m (every edge of a dense group may weigh its sparsest member's core value): the index rule decides them,
// as it decides the ties among identical rows today.  core == NULL is the plain weight, bit for bit.
#include "mvs_core.h"
#include "mvs_internal.h"
#include "mvs_pairwise_dev.h"

#include <rocprim/device/device_merge_sort.hpp>

namespace mvs {

namespace {

constexpr int kLkThreads = 256;
constexpr unsigned long long kNone = ~0ULL;

__device__ __forceinline__ int32_t lk_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lk_store(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one atomic per wave for a counter every lane may bump (every lane of the wave must call it)
__device__ __forceinline__ void lk_count(unsigned long long* counter, bool mine) {
    const unsigned long long mask = __ballot(mine);
    if (mask == 0ULL) return;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(counter, (unsigned long long)__popcll(mask));
}

// mvs_topk.hip's topk_key
__device__ __forceinline__ unsigned long long lk_key(double J) {
    if (J == 0.0) J = 0.0;                                          // -0.0 -> +0.0
    const unsigned long long u = (unsigned long long)__double_as_longlong(J);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double lk_jaccard(int32_t dot, int d, double n2a, double n2b) {
    const double inter = (double)dot / (double)d;                      // :661
    return inter / (n2a + n2b - inter);                                // :662
}

struct LkEdge {
    int32_t lo, hi, dot, q;
    unsigned long long key, pair;
};

enum { kLkEdge = 0, kLkIgnored = 1, kLkSelf = 2, kLkBad = 3 };

// cell e of F u L (e < n_f: F[e], else L[e - n_f]) as an edge
// the weight of the edge (lo, hi) whose Jaccard estimate is J (not NaN).  core == NULL: J itself.  Else the mutual reachability
// m = min(J, core[lo], core[hi]) by key order (J unless a core value's key is strictly smaller, then that value, lo before hi);
// false if either core value is NaN: the edge is ignored
__device__ __forceinline__ bool lk_weight(double J, const double* __restrict__ core, int32_t lo, int32_t hi, double& m,
                                          unsigned long long& key) {
    m = J;
    key = lk_key(J);
    if (core == nullptr) return true;
    const double ca = core[lo], cb = core[hi];
    if (!(ca == ca) || !(cb == cb)) return false;
    const unsigned long long ka = lk_key(ca);
    if (ka < key) {
        key = ka;
        m = ca;
    }
    const unsigned long long kb = lk_key(cb);
    if (kb < key) {
        key = kb;
        m = cb;
    }
    return true;
}

__device__ __forceinline__ int lk_edge(const mvs_cell* __restrict__ F, int64_t n_f, const mvs_cell* __restrict__ L, int64_t e,
                                       const double* __restrict__ norms_sq, const double* __restrict__ core, int64_t n, int d,
                                       LkEdge& out) {
    const mvs_cell c = e < n_f ? F[e] : L[e - n_f];
    if (c.row < 0 || c.col < 0 || c.row >= n || c.col >= n) return kLkBad;
    if (c.row == c.col) return kLkSelf;
    out.lo = c.row < c.col ? c.row : c.col;
    out.hi = c.row < c.col ? c.col : c.row;
    out.dot = c.dot;
    out.q = c.q;
    const double J = lk_jaccard(c.dot, d, norms_sq[out.lo], norms_sq[out.hi]);
    if (!(J == J)) return kLkIgnored;
    double m;
    if (!lk_weight(J, core, out.lo, out.hi, m, out.key)) return kLkIgnored;
    out.pair = ((unsigned long long)(unsigned)out.lo << 32) | (unsigned long long)(unsigned)out.hi;
    return kLkEdge;
}

__global__ __launch_bounds__(kLkThreads) void k_link_identity(int32_t* __restrict__ comp, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kLkThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLkThreads) comp[i] = (int32_t)i;
}

__global__ __launch_bounds__(kLkThreads) void k_link_slots(unsigned long long* __restrict__ best_key, unsigned long long* __restrict__ best_pair,
                                                           unsigned long long* __restrict__ best_idx, int32_t* __restrict__ next, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kLkThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLkThreads) {
        best_key[i] = 0ULL;
        best_pair[i] = kNone;
        best_idx[i] = kNone;
        next[i] = (int32_t)i;
    }
}

// pass 0: key; 1: pair; 2: pick.  counters: [0] cells of L with row != col in range (added when `first`), [1] cells of L with an
// index outside [0, n) (when `first`), [2] edges whose endpoints lie in different components (pass 0)
template <int PASS>
__global__ __launch_bounds__(kLkThreads) void k_link_select(const mvs_cell* __restrict__ F, int64_t n_f, const mvs_cell* __restrict__ L,
                                                            int64_t n_l, const double* __restrict__ norms_sq,
                                                            const double* __restrict__ core, int64_t n, int d,
                                                            const int32_t* __restrict__ comp, unsigned long long* __restrict__ best_key,
                                                            unsigned long long* __restrict__ best_pair,
                                                            unsigned long long* __restrict__ best_idx, int first,
                                                            unsigned long long* __restrict__ counters) {
    const int64_t total = n_f + n_l;
    const int64_t stride = (int64_t)gridDim.x * kLkThreads;
    const int64_t trips = (total + stride - 1) / stride;               // every lane makes every trip: the ballots are whole
    int64_t e = (int64_t)blockIdx.x * kLkThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, e += stride) {
        LkEdge g;
        const int kind = e < total ? lk_edge(F, n_f, L, e, norms_sq, core, n, d, g) : kLkSelf;
        bool apart = false;
        int32_t ca = 0, cb = 0;
        if (kind == kLkEdge) {
            ca = comp[g.lo];
            cb = comp[g.hi];
            apart = ca != cb;
        }
        if (PASS == 0) {
            if (first) {
                const bool fed = e < total && e >= n_f;
                lk_count(counters + 0, fed && (kind == kLkEdge || kind == kLkIgnored));
                lk_count(counters + 1, fed && kind == kLkBad);
            }
            lk_count(counters + 2, apart);
            if (apart) {
                atomicMax(best_key + ca, g.key);
                atomicMax(best_key + cb, g.key);
            }
        } else if (PASS == 1) {
            if (apart) {
                if (best_key[ca] == g.key) atomicMin(best_pair + ca, g.pair);
                if (best_key[cb] == g.key) atomicMin(best_pair + cb, g.pair);
            }
        } else {
            if (apart) {
                if (best_key[ca] == g.key && best_pair[ca] == g.pair) atomicMin(best_idx + ca, (unsigned long long)e);
                if (best_key[cb] == g.key && best_pair[cb] == g.pair) atomicMin(best_idx + cb, (unsigned long long)e);
            }
        }
    }
}

// counters: [3] cells in the next forest, [4] set if one did not fit (cannot happen: a forest has at most n - 1 edges)
__global__ __launch_bounds__(kLkThreads) void k_link_hook(const mvs_cell* __restrict__ F, int64_t n_f, const mvs_cell* __restrict__ L,
                                                          const double* __restrict__ norms_sq, const double* __restrict__ core,
                                                          int64_t n, int d, const int32_t* __restrict__ comp,
                                                          const unsigned long long* __restrict__ best_key,
                                                          const unsigned long long* __restrict__ best_pair,
                                                          const unsigned long long* __restrict__ best_idx, int32_t* __restrict__ next,
                                                          mvs_cell* __restrict__ F_next, int64_t capacity,
                                                          unsigned long long* __restrict__ counters) {
    for (int64_t c = (int64_t)blockIdx.x * kLkThreads + threadIdx.x; c < n; c += (int64_t)gridDim.x * kLkThreads) {
        const unsigned long long e = best_idx[c];
        if (e == kNone) continue;                                      // not a root, or a root nothing leaves
        LkEdge g;
        if (lk_edge(F, n_f, L, (int64_t)e, norms_sq, core, n, d, g) != kLkEdge) continue;   // (pick wrote the index of an edge)
        const int32_t ca = comp[g.lo], cb = comp[g.hi];
        const int32_t o = ca == (int32_t)c ? cb : ca;
        const bool mutual = best_key[o] == best_key[c] && best_pair[o] == best_pair[c];
        if (mutual && (int32_t)c < o) continue;
        next[c] = o;
        const unsigned long long pos = atomicAdd(counters + 3, 1ULL);
        if ((int64_t)pos < capacity) {
            mvs_cell out;
            out.row = g.lo;
            out.col = g.hi;
            out.dot = g.dot;
            out.q = g.q;
            F_next[pos] = out;
        } else {
            atomicMax(counters + 4, 1ULL);
        }
    }
}

// next[c] := the root of c's chain, for the components of this round (comp[c] == c); counters[4] |= 2 on a walk of more than n steps
__global__ __launch_bounds__(kLkThreads) void k_link_flatten(const int32_t* __restrict__ comp, int32_t* __restrict__ next, int64_t n,
                                                             unsigned long long* __restrict__ counters) {
    for (int64_t c = (int64_t)blockIdx.x * kLkThreads + threadIdx.x; c < n; c += (int64_t)gridDim.x * kLkThreads) {
        if (comp[c] != (int32_t)c) continue;
        int32_t r = (int32_t)c;
        int32_t p = lk_load(next + r);
        int64_t steps = 0;
        while (p != r && steps <= n) {
            r = p;
            p = lk_load(next + r);
            ++steps;
        }
        if (p != r) {
            atomicMax(counters + 4, 2ULL);
            continue;
        }
        if (r != (int32_t)c) lk_store(next + c, r);
    }
}

__global__ __launch_bounds__(kLkThreads) void k_link_apply(int32_t* __restrict__ comp, const int32_t* __restrict__ next, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kLkThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLkThreads) comp[i] = next[comp[i]];
}

// the forest as links (unsorted): a = lo, b = hi, dot, q as the comparison reports it, the fp64 weight (J; with core values m)
__global__ __launch_bounds__(kLkThreads) void k_link_links(const mvs_cell* __restrict__ F, int64_t n_f, const double* __restrict__ norms_sq,
                                                           const double* __restrict__ core, int d, mvs_link* __restrict__ links) {
    for (int64_t i = (int64_t)blockIdx.x * kLkThreads + threadIdx.x; i < n_f; i += (int64_t)gridDim.x * kLkThreads) {
        const mvs_cell c = F[i];
        mvs_link l;
        l.a = c.row;
        l.b = c.col;
        l.dot = c.dot;
        l.q = quantize_cell(c.dot, d, norms_sq[c.row], norms_sq[c.col]);
        unsigned long long key;
        (void)lk_weight(lk_jaccard(c.dot, d, norms_sq[c.row], norms_sq[c.col]), core, c.row, c.col, l.jaccard, key);
        links[i] = l;
    }
}

// links sorted best first: those with jaccard > level are a prefix; the first `capacity` of them as cells, all of them counted
__global__ __launch_bounds__(kLkThreads) void k_link_cells(const mvs_link* __restrict__ links, int64_t n_links, double level,
                                                           mvs_cell* __restrict__ cells, int64_t capacity,
                                                           unsigned long long* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kLkThreads;
    const int64_t trips = (n_links + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kLkThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        bool above = false;
        if (i < n_links) {
            const mvs_link l = links[i];
            above = l.jaccard > level;
            if (above && i < capacity) {
                mvs_cell c;
                c.row = l.a;
                c.col = l.b;
                c.dot = l.dot;
                c.q = l.q;
                cells[i] = c;
            }
        }
        lk_count(counters + 5, above);
    }
}

struct LinkBefore {
    __device__ bool operator()(const mvs_link& x, const mvs_link& y) const {
        const unsigned long long kx = lk_key(x.jaccard), ky = lk_key(y.jaccard);
        if (kx != ky) return kx > ky;
        if (x.a != y.a) return x.a < y.a;
        return x.b < y.b;
    }
};

unsigned lk_grid(int64_t items) {
    const int64_t blocks = (items + kLkThreads - 1) / kLkThreads;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, 1 << 16));
}

}  // namespace

int launch_link_identity(hipStream_t stream, int32_t* d_comp, int64_t n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_link_identity, dim3(lk_grid(n)), dim3(kLkThreads), 0, stream, d_comp, n);
    return 0;
}

int launch_link_slots(hipStream_t stream, const LinkState& s) {
    if (s.n <= 0) return 0;
    hipLaunchKernelGGL(k_link_slots, dim3(lk_grid(s.n)), dim3(kLkThreads), 0, stream, s.best_key, s.best_pair, s.best_idx, s.next, s.n);
    return 0;
}

int launch_link_select(hipStream_t stream, const LinkState& s, const double* d_core, const mvs_cell* d_cells, int64_t n_cells, int pass,
                       bool first) {
    const int64_t total = s.n_forest + n_cells;
    if (total <= 0) return 0;
    const dim3 grid(lk_grid(total)), block(kLkThreads);
#define MVS_LINK_SELECT(P)                                                                                                            \
    hipLaunchKernelGGL(k_link_select<P>, grid, block, 0, stream, s.forest, s.n_forest, d_cells, n_cells, s.norms_sq, d_core, s.n, s.d, \
                       s.comp, s.best_key, s.best_pair, s.best_idx, first ? 1 : 0, s.counters)
    if (pass == 0) MVS_LINK_SELECT(0);
    else if (pass == 1) MVS_LINK_SELECT(1);
    else MVS_LINK_SELECT(2);
#undef MVS_LINK_SELECT
    return 0;
}
int launch_link_select(hipStream_t stream, const LinkState& s, const mvs_cell* d_cells, int64_t n_cells, int pass, bool first) {
    return launch_link_select(stream, s, nullptr, d_cells, n_cells, pass, first);
}

int launch_link_hook(hipStream_t stream, const LinkState& s, const double* d_core, const mvs_cell* d_cells) {
    if (s.n <= 0) return 0;
    hipLaunchKernelGGL(k_link_hook, dim3(lk_grid(s.n)), dim3(kLkThreads), 0, stream, s.forest, s.n_forest, d_cells, s.norms_sq, d_core, s.n,
                       s.d, s.comp, s.best_key, s.best_pair, s.best_idx, s.next, s.forest_next, s.capacity, s.counters);
    return 0;
}
int launch_link_hook(hipStream_t stream, const LinkState& s, const mvs_cell* d_cells) { return launch_link_hook(stream, s, nullptr, d_cells); }

int launch_link_jump(hipStream_t stream, const LinkState& s) {
    if (s.n <= 0) return 0;
    hipLaunchKernelGGL(k_link_flatten, dim3(lk_grid(s.n)), dim3(kLkThreads), 0, stream, s.comp, s.next, s.n, s.counters);
    hipLaunchKernelGGL(k_link_apply, dim3(lk_grid(s.n)), dim3(kLkThreads), 0, stream, s.comp, s.next, s.n);
    return 0;
}

// the forest's links, sorted best first, into d_links (n_forest entries); d_tmp: as many again; scratch as rocprim's merge sort
// wants it (d_scratch == NULL: *scratch_needed only)
int link_sorted(hipStream_t stream, const LinkState& s, const double* d_core, mvs_link* d_tmp, mvs_link* d_links, void* d_scratch,
                size_t scratch_bytes, size_t* scratch_needed) {
    size_t need = 0;
    hipError_t e = rocprim::merge_sort(nullptr, need, d_tmp, d_links, (size_t)s.n_forest, LinkBefore(), stream);
    if (e != hipSuccess) return MVS_E_HIP;
    if (scratch_needed) *scratch_needed = need;
    if (d_scratch == nullptr) return 0;
    if (scratch_bytes < need) return MVS_E_CAPACITY;
    if (s.n_forest <= 0) return 0;
    hipLaunchKernelGGL(k_link_links, dim3(lk_grid(s.n_forest)), dim3(kLkThreads), 0, stream, s.forest, s.n_forest, s.norms_sq, d_core, s.d, d_tmp);
    e = rocprim::merge_sort(d_scratch, need, d_tmp, d_links, (size_t)s.n_forest, LinkBefore(), stream);
    return e == hipSuccess ? 0 : MVS_E_HIP;
}
int link_sorted(hipStream_t stream, const LinkState& s, mvs_link* d_tmp, mvs_link* d_links, void* d_scratch, size_t scratch_bytes,
                size_t* scratch_needed) {
    return link_sorted(stream, s, nullptr, d_tmp, d_links, d_scratch, scratch_bytes, scratch_needed);
}

// counters[5] += links above `level` (the caller cleared it)
int launch_link_cells(hipStream_t stream, const mvs_link* d_links, int64_t n_links, double level, mvs_cell* d_cells, int64_t capacity,
                      unsigned long long* d_counters) {
    if (n_links <= 0) return 0;
    hipLaunchKernelGGL(k_link_cells, dim3(lk_grid(n_links)), dim3(kLkThreads), 0, stream, d_links, n_links, level, d_cells, capacity,
                       d_counters);
    return 0;
}

}  // namespace mvs
