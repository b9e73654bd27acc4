// mvs_community.hip -- modularity communities (Louvain) of the thresholded Jaccard graph on the device (mvs_community_*).
//
// The rule is stated in include/mvs_hip.h "Communities" and DESIGN.md section 25; tests/communities_model.py is the same rule in
// Python integers.  Everything here is an integer: a weight is a = rint(k * 2^20), a gain and Qnum are 128-bit, and every sum is
// formed by integer atomics or integer reductions -- so no order of lanes, workgroups, blocks or fed cells can change a result.
//
// Graph.  Fed cells become (lo << 32 | hi, a) entries; a radix sort and a reduce-by-key (maximum) leave one entry per edge; both
// directions are sorted once more into a CSR (row_ptr, src, col, weight).  Level 0 keeps 32-bit weights, coarser levels 64-bit.
//
// Local moving, the hot path: a full sweep of the CSR per round.  A vertex's edge weights are summed by neighbour community in
// a hash table (key: the community, value: 64-bit sum, linear probing, compare-and-swap on the key, integer add on the value),
// then the table's slots are scanned for the largest (gain, smaller community).  Degrees run from 1 to tens of thousands, so
// three shapes share one kernel template:
//   path 0, wave:       one wave per vertex, 128 slots in LDS; vertices of degree <= 256
//   path 1, workgroup:  256 lanes per vertex, 4096 slots in LDS; degree <= 16384
//   path 2, global:     256 lanes per vertex, a table of >= 2 * degree slots in device memory, one per resident workgroup; the
//                       table is read and written with agent-scope atomics only (a CU's L1 is not refreshed by atomics that
//                       execute in the L2)
// A vertex with more neighbour communities than its path's table has slots leaves the table unfinished: NOTHING of it is used,
// the vertex is appended to the next path's hand-over list and done again there from the start.  The global table cannot fill
// (slots >= 2 * degree).  All reads of a round are from the state at its start (comm, tot, size); moves go to `next`.
//
// Why not matrix cores, why no packed math: the work per edge is one gather (comm[col]), one LDS compare-and-swap and one LDS
// 64-bit add; the 128-bit gain is per neighbour COMMUNITY, not per edge.  The sweep is bound by the gather and the LDS atomics.
#include "mvs_community.h"
#include "mvs_weight_dev.h"

#include <climits>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>

namespace mvs {

namespace {

typedef __int128 i128;
typedef unsigned __int128 u128;
typedef unsigned long long u64;

constexpr int kCmThreads = 256;

unsigned grid_for(int64_t items) {
    const int64_t blocks = (items + kCmThreads - 1) / kCmThreads;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, 1 << 16));
}

__device__ __forceinline__ u64 splitmix64(u64 x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// the slot a converged wave's lane gets in a list that every lane may append to: one atomic per wave
template <typename C>
__device__ __forceinline__ C wave_append(C* counter, bool mine) {
    const u64 mask = __ballot(mine);
    if (mask == 0ULL) return 0;
    const int lane = (int)(threadIdx.x & 63), leader = __ffsll((long long)mask) - 1;
    u64 base = 0;
    if (lane == leader) base = (u64)atomicAdd(counter, (C)__popcll(mask));
    base = __shfl(base, leader);
    return (C)(base + (u64)__popcll(mask & ((1ULL << lane) - 1ULL)));
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- feeding ----
__global__ __launch_bounds__(kCmThreads) void k_comm_cells(const mvs_cell* __restrict__ cells, int64_t n_cells, int64_t n,
                                                           const double* __restrict__ n2, double dd, double inv, int pow2, double floor_,
                                                           u64* __restrict__ keys, uint32_t* __restrict__ w, u64* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kCmThreads;
    const int64_t trips = (n_cells + stride - 1) / stride;             // every lane makes every trip: the ballots are whole
    int64_t i = (int64_t)blockIdx.x * kCmThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        int32_t r = 0, c = 0, P = 0;
        const bool in = i < n_cells;
        if (in) {
            r = cells[i].row;
            c = cells[i].col;
            P = cells[i].dot;
        }
        const bool bad = in && (r < 0 || c < 0 || r >= n || c >= n);
        uint32_t a = 0;
        if (in && !bad && r != c) a = quantised_similarity(P, n2[r], n2[c], dd, inv, pow2 != 0, floor_);
        (void)wave_append(counters + 1, bad);
        const u64 at = wave_append(counters + 0, a != 0u);
        if (a != 0u) {
            const uint32_t lo = (uint32_t)(r < c ? r : c), hi = (uint32_t)(r < c ? c : r);
            keys[at] = ((u64)lo << 32) | hi;
            w[at] = a;
        }
    }
}

__global__ __launch_bounds__(kCmThreads) void k_comm_edges(const int32_t* __restrict__ elo, const int32_t* __restrict__ ehi,
                                                           const int32_t* __restrict__ ea, int64_t n_edges, int64_t n, u64* __restrict__ keys,
                                                           uint32_t* __restrict__ w, u64* __restrict__ counters) {
    const int64_t stride = (int64_t)gridDim.x * kCmThreads;
    const int64_t trips = (n_edges + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kCmThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        int32_t r = 0, c = 0, a = 0;
        const bool in = i < n_edges;
        if (in) {
            r = elo[i];
            c = ehi[i];
            a = ea[i];
        }
        const bool bad = in && (r < 0 || c < 0 || r >= n || c >= n);
        const bool heavy = in && !bad && r != c && (a < 1 || a > (1 << 20));
        const bool keep = in && !bad && !heavy && r != c;
        (void)wave_append(counters + 1, bad);
        (void)wave_append(counters + 2, heavy);
        const u64 at = wave_append(counters + 0, keep);
        if (keep) {
            const uint32_t lo = (uint32_t)(r < c ? r : c), hi = (uint32_t)(r < c ? c : r);
            keys[at] = ((u64)lo << 32) | hi;
            w[at] = (uint32_t)a;
        }
    }
}

__global__ __launch_bounds__(kCmThreads) void k_comm_mirror(const u64* __restrict__ keys, const uint32_t* __restrict__ w, int64_t e,
                                                            u64* __restrict__ dk, uint32_t* __restrict__ dw) {
    for (int64_t i = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; i < e; i += (int64_t)gridDim.x * kCmThreads) {
        const u64 k = keys[i];
        dk[2 * i] = k;
        dk[2 * i + 1] = (k << 32) | (k >> 32);
        dw[2 * i] = w[i];
        dw[2 * i + 1] = w[i];
    }
}

__global__ __launch_bounds__(kCmThreads) void k_comm_csr(const u64* __restrict__ keys, int64_t m, int64_t n, long long* __restrict__ row_ptr,
                                                         int32_t* __restrict__ src, int32_t* __restrict__ col) {
    const int64_t stride = (int64_t)gridDim.x * kCmThreads;
    for (int64_t i = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; i < m; i += stride) {
        src[i] = (int32_t)(keys[i] >> 32);
        col[i] = (int32_t)(keys[i] & 0xffffffffULL);
    }
    for (int64_t r = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; r <= n; r += stride) {
        const u64 want = (u64)r << 32;                                  // the first entry whose key is >= (r, 0)
        int64_t lo = 0, hi = m;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        row_ptr[r] = lo;
    }
}

template <typename WT>
__global__ __launch_bounds__(kCmThreads) void k_comm_strength(CommLevel g, const WT* __restrict__ w, u64* __restrict__ k, u64* __restrict__ total) {
    const int64_t stride = (int64_t)gridDim.x * kCmThreads;
    const int64_t trips = (g.n + stride - 1) / stride;
    int64_t v = (int64_t)blockIdx.x * kCmThreads + threadIdx.x;
    u64 mine = 0;
    for (int64_t t = 0; t < trips; ++t, v += stride) {
        if (v >= g.n) continue;
        u64 s = g.self[v];
        for (long long e = g.row_ptr[v]; e < g.row_ptr[v + 1]; ++e) s += (u64)w[e];
        k[v] = s;
        mine += s;
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(total, mine);
}

__global__ __launch_bounds__(kCmThreads) void k_comm_classify(CommLevel g, int forced, int32_t* __restrict__ l0, int32_t* __restrict__ l1,
                                                              int32_t* __restrict__ l2, unsigned int* __restrict__ counts) {
    const int64_t stride = (int64_t)gridDim.x * kCmThreads;
    const int64_t trips = (g.n + stride - 1) / stride;
    int64_t v = (int64_t)blockIdx.x * kCmThreads + threadIdx.x;
    for (int64_t t = 0; t < trips; ++t, v += stride) {
        long long deg = 0;
        if (v < g.n) deg = g.row_ptr[v + 1] - g.row_ptr[v];
        int path = -1;
        if (deg > 0) path = forced ? forced - 1 : (deg <= kCommWaveDegree ? 0 : (deg <= kCommBlockDegree ? 1 : 2));
        const unsigned a0 = wave_append(counts + 0, path == 0);
        const unsigned a1 = wave_append(counts + 1, path == 1);
        const unsigned a2 = wave_append(counts + 2, path == 2);
        if (path == 0) l0[a0] = (int32_t)v;
        if (path == 1) l1[a1] = (int32_t)v;
        if (path == 2) l2[a2] = (int32_t)v;
        if (deg > 0) atomicMax(counts + 3, (unsigned)(deg < 0x7fffffffLL ? deg : 0x7fffffffLL));
    }
}

__global__ __launch_bounds__(kCmThreads) void k_comm_identity(int32_t* __restrict__ x, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCmThreads) x[i] = (int32_t)i;
}

__global__ __launch_bounds__(kCmThreads) void k_comm_fill(int32_t* __restrict__ x, int64_t n, int32_t value) {
    for (int64_t i = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCmThreads) x[i] = value;
}

// ---- local moving ----
// table accessors: LDS tables are read and cleared with plain accesses between workgroup barriers; the global table (PATH 2) only
// with agent-scope atomics
template <int PATH, typename T>
__device__ __forceinline__ T tab_load(const T* p) {
    if (PATH == 2) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <int PATH, typename T>
__device__ __forceinline__ void tab_store(T* p, T v) {
    if (PATH == 2) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

template <typename WT, int PATH>
__global__ __launch_bounds__(PATH == 0 ? 64 : 256) void k_comm_move(CommLevel g, const WT* __restrict__ w, CommRound r,
                                                                    const int32_t* __restrict__ comm, int32_t* __restrict__ next,
                                                                    const u64* __restrict__ tot, const int32_t* __restrict__ size,
                                                                    const int32_t* __restrict__ list, const unsigned int* __restrict__ list_count,
                                                                    int32_t* __restrict__ over, unsigned int* __restrict__ over_count,
                                                                    int32_t* __restrict__ gkeys, u64* __restrict__ gvals, int64_t gslots,
                                                                    u64* __restrict__ moved) {
    constexpr int T = PATH == 0 ? 64 : 256;
    constexpr int LS = PATH == 0 ? kCommWaveSlots : (PATH == 1 ? kCommBlockSlots : 1);
    __shared__ int32_t s_keys[LS];
    __shared__ u64 s_vals[LS];
    __shared__ int s_full;
    __shared__ u64 s_kA;
    __shared__ u64 s_ghi[4], s_glo[4];
    __shared__ int32_t s_c[4];
    const int tid = (int)threadIdx.x;
    int32_t* keys = PATH == 2 ? gkeys + (int64_t)blockIdx.x * gslots : s_keys;
    u64* vals = PATH == 2 ? gvals + (int64_t)blockIdx.x * gslots : s_vals;
    const u128 RW = ((u128)r.rw_hi << 64) | (u128)r.rw_lo;
    const unsigned count = *list_count;
    for (unsigned i = blockIdx.x; i < count; i += gridDim.x) {
        const int32_t v = list[i];
        // the half activation (uniform for the workgroup)
        if (!(splitmix64(((u64)r.level << 48) ^ ((u64)r.round << 32) ^ (u64)(uint32_t)v) & 1ULL)) continue;
        const long long e0 = g.row_ptr[v], e1 = g.row_ptr[v + 1];
        int64_t slots = LS;
        if (PATH == 2) {
            slots = 64;
            while (slots < 2 * (e1 - e0)) slots <<= 1;                 // <= gslots: the host sized the table by the largest degree
        }
        const u64 mask = (u64)slots - 1ULL;
        for (int64_t s = tid; s < slots; s += T) {
            tab_store<PATH>(keys + s, (int32_t)-1);
            tab_store<PATH>(vals + s, (u64)0);
        }
        if (tid == 0) {
            s_full = 0;
            s_kA = 0;
        }
        __syncthreads();
        for (long long e = e0 + tid; e < e1; e += T) {
            if (*(volatile int*)&s_full) break;                         // full already: the next path does this vertex
            const int32_t c = comm[g.col[e]];
            const u64 wt = (u64)w[e];
            u64 h = (((u64)(uint32_t)c * 0x9E3779B97F4A7C15ULL) >> 32) & mask;
            bool done = false;
            for (int64_t p = 0; p < slots; ++p) {
                int32_t seen = -1;
                bool mine;
                if (PATH == 2) {
                    mine = __hip_atomic_compare_exchange_strong(keys + h, &seen, c, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    seen = atomicCAS(keys + h, -1, c);
                    mine = seen == -1;
                }
                if (mine || seen == c) {
                    atomicAdd(vals + h, wt);
                    done = true;
                    break;
                }
                h = (h + 1ULL) & mask;
            }
            if (!done) s_full = 1;                                      // the table is full: nothing of it will be used
        }
        __syncthreads();
        if (s_full) {
            if (tid == 0) over[atomicAdd(over_count, 1u)] = v;          // PATH 2 cannot come here (slots >= 2 * degree)
            __syncthreads();
            continue;
        }
        const int32_t A = comm[v];
        for (int64_t s = tid; s < slots; s += T)
            if (tab_load<PATH>(keys + s) == A) s_kA = tab_load<PATH>(vals + s);
        __syncthreads();
        const u64 kA = s_kA, kv = g.k[v], totA = tot[A];
        const i128 gk = (i128)((u128)r.g * (u128)kv);
        i128 bg = 0;
        int32_t bc = -1;
        for (int64_t s = tid; s < slots; s += T) {
            const int32_t c = tab_load<PATH>(keys + s);
            if (c < 0 || c == A) continue;
            const u64 kvc = tab_load<PATH>(vals + s);
            const i128 gain = (i128)RW * ((i128)kvc - (i128)kA) - gk * ((i128)tot[c] - (i128)totA + (i128)kv);
            if (bc < 0 || gain > bg || (gain == bg && c < bc)) {
                bg = gain;
                bc = c;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const u64 ohi = __shfl_xor((u64)((u128)bg >> 64), off), olo = __shfl_xor((u64)(u128)bg, off);
            const int32_t oc = __shfl_xor(bc, off);
            const i128 og = (i128)(((u128)ohi << 64) | (u128)olo);
            if (oc >= 0 && (bc < 0 || og > bg || (og == bg && oc < bc))) {
                bg = og;
                bc = oc;
            }
        }
        if (PATH != 0) {
            if ((tid & 63) == 0) {
                s_ghi[tid >> 6] = (u64)((u128)bg >> 64);
                s_glo[tid >> 6] = (u64)(u128)bg;
                s_c[tid >> 6] = bc;
            }
            __syncthreads();
            if (tid == 0) {
                for (int q = 1; q < T / 64; ++q) {
                    const i128 og = (i128)(((u128)s_ghi[q] << 64) | (u128)s_glo[q]);
                    const int32_t oc = s_c[q];
                    if (oc >= 0 && (bc < 0 || og > bg || (og == bg && oc < bc))) {
                        bg = og;
                        bc = oc;
                    }
                }
            }
        }
        if (tid == 0 && bc >= 0 && bg > 0 && !(size[A] == 1 && size[bc] == 1 && bc > A)) {
            next[v] = bc;
            atomicAdd(moved, 1ULL);
        }
        __syncthreads();
    }
}

// ---- apply ----
__global__ __launch_bounds__(kCmThreads) void k_comm_tot(CommLevel g, const int32_t* __restrict__ comm, u64* __restrict__ tot,
                                                         int32_t* __restrict__ size) {
    for (int64_t v = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; v < g.n; v += (int64_t)gridDim.x * kCmThreads) {
        const int32_t c = comm[v];
        atomicAdd(tot + c, g.k[v]);
        atomicAdd(size + c, 1);
    }
}

// acc[0] += the self weights and the weights of the directed entries inside a community
template <typename WT>
__global__ __launch_bounds__(kCmThreads) void k_comm_inner(CommLevel g, const WT* __restrict__ w, const int32_t* __restrict__ comm,
                                                           u64* __restrict__ acc) {
    const int64_t stride = (int64_t)gridDim.x * kCmThreads;
    const int64_t items = g.n > g.m ? g.n : g.m;
    const int64_t trips = (items + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kCmThreads + threadIdx.x;
    u64 mine = 0;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        if (i < g.n) mine += g.self[i];
        if (i < g.m && comm[g.src[i]] == comm[g.col[i]]) mine += (u64)w[i];
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(acc, mine);
}

// acc[1..3] += sum of tot^2 as limbs: bits 0..31, 32..63, 64..127
__global__ __launch_bounds__(kCmThreads) void k_comm_sumsq(const u64* __restrict__ tot, int64_t n, u64* __restrict__ acc) {
    const int64_t stride = (int64_t)gridDim.x * kCmThreads;
    const int64_t trips = (n + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kCmThreads + threadIdx.x;
    u64 l0 = 0, l1 = 0, l2 = 0;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        if (i >= n) continue;
        const u128 sq = (u128)tot[i] * (u128)tot[i];
        l0 += (u64)sq & 0xffffffffULL;
        l1 += ((u64)sq >> 32);
        l2 += (u64)(sq >> 64);
    }
    l0 = wave_sum(l0);
    l1 = wave_sum(l1);
    l2 = wave_sum(l2);
    if ((threadIdx.x & 63) == 0) {
        if (l0) atomicAdd(acc + 1, l0);
        if (l1) atomicAdd(acc + 2, l1);
        if (l2) atomicAdd(acc + 3, l2);
    }
}

template <typename WT>
__global__ __launch_bounds__(kCmThreads) void k_comm_inner_by(CommLevel g, const WT* __restrict__ w, const int32_t* __restrict__ comm,
                                                              u64* __restrict__ inner) {
    const int64_t stride = (int64_t)gridDim.x * kCmThreads;
    for (int64_t i = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; i < (g.n > g.m ? g.n : g.m); i += stride) {
        if (i < g.n && g.self[i]) atomicAdd(inner + comm[i], g.self[i]);
        if (i < g.m) {
            const int32_t c = comm[g.src[i]];
            if (c == comm[g.col[i]]) atomicAdd(inner + c, (u64)w[i]);
        }
    }
}

// ---- numbering, composition, aggregation ----
__global__ __launch_bounds__(kCmThreads) void k_comm_minm(const int32_t* __restrict__ comm, int64_t n, int32_t* __restrict__ minm) {
    for (int64_t v = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kCmThreads) atomicMin(minm + comm[v], (int32_t)v);
}
__global__ __launch_bounds__(kCmThreads) void k_comm_flag(const int32_t* __restrict__ comm, int64_t n, const int32_t* __restrict__ minm,
                                                          int32_t* __restrict__ flag) {
    for (int64_t v = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; v <= n; v += (int64_t)gridDim.x * kCmThreads)
        flag[v] = (v < n && minm[comm[v]] == (int32_t)v) ? 1 : 0;
}
__global__ __launch_bounds__(kCmThreads) void k_comm_new(const int32_t* __restrict__ comm, int64_t n, const int32_t* __restrict__ minm,
                                                         const int32_t* __restrict__ ids, int32_t* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kCmThreads) out[v] = ids[minm[comm[v]]];
}
__global__ __launch_bounds__(kCmThreads) void k_comm_compose(int32_t* __restrict__ member, int64_t n0, const int32_t* __restrict__ nw) {
    for (int64_t s = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; s < n0; s += (int64_t)gridDim.x * kCmThreads) member[s] = nw[member[s]];
}

template <typename WT>
__global__ __launch_bounds__(kCmThreads) void k_comm_aggregate(CommLevel g, const WT* __restrict__ w, const int32_t* __restrict__ nw,
                                                               u64* __restrict__ keys, u64* __restrict__ vals, u64* __restrict__ self2,
                                                               u64* __restrict__ cross) {
    const int64_t stride = (int64_t)gridDim.x * kCmThreads;
    const int64_t items = g.n > g.m ? g.n : g.m;
    const int64_t trips = (items + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kCmThreads + threadIdx.x;
    u64 mine = 0;
    for (int64_t t = 0; t < trips; ++t, i += stride) {
        if (i < g.n && g.self[i]) atomicAdd(self2 + nw[i], g.self[i]);
        if (i < g.m) {
            const int32_t cu = nw[g.src[i]], cv = nw[g.col[i]];
            if (cu != cv) {
                keys[i] = ((u64)(uint32_t)cu << 32) | (u64)(uint32_t)cv;
                vals[i] = (u64)w[i];
                ++mine;
            } else {
                keys[i] = ~0ULL;
                vals[i] = 0;
                atomicAdd(self2 + cu, (u64)w[i]);
            }
        }
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(cross, mine);
}

__global__ __launch_bounds__(kCmThreads) void k_comm_split_cells(CommLevel g, const int32_t* __restrict__ member, int64_t e0, int64_t e1,
                                                                 mvs_cell* __restrict__ cells) {
    for (int64_t e = e0 + (int64_t)blockIdx.x * kCmThreads + threadIdx.x; e < e1; e += (int64_t)gridDim.x * kCmThreads) {
        const int32_t u = g.src[e], v = g.col[e];
        const bool link = u < v && member[u] == member[v];
        mvs_cell c;
        c.row = link ? u : 0;
        c.col = link ? v : 0;
        c.dot = 0;
        c.q = 0;
        cells[e - e0] = c;
    }
}

__global__ __launch_bounds__(kCmThreads) void k_comm_gather_first(const int32_t* __restrict__ comm, const int32_t* __restrict__ flag,
                                                                  const int32_t* __restrict__ ids, int64_t n, const u64* __restrict__ in_a,
                                                                  const u64* __restrict__ in_b, u64* __restrict__ out_a, u64* __restrict__ out_b) {
    for (int64_t v = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kCmThreads) {
        if (!flag[v]) continue;
        out_a[ids[v]] = in_a[comm[v]];
        out_b[ids[v]] = in_b[comm[v]];
    }
}

__global__ __launch_bounds__(kCmThreads) void k_comm_degree(CommLevel g, int32_t* __restrict__ degree) {
    for (int64_t v = (int64_t)blockIdx.x * kCmThreads + threadIdx.x; v < g.n; v += (int64_t)gridDim.x * kCmThreads)
        degree[v] = (int32_t)(g.row_ptr[v + 1] - g.row_ptr[v]);
}

// rocprim's two-call convention with a scratch buffer of the call's own
struct Scratch {
    void* p = nullptr;
    ~Scratch() {
        if (p) (void)hipFree(p);
    }
};

template <typename F>
int with_scratch(hipStream_t stream, F&& call) {
    size_t need = 0;
    if (call(nullptr, need) != hipSuccess) return MVS_E_HIP;
    Scratch s;
    if (hipMalloc(&s.p, need ? need : 1) != hipSuccess) return MVS_E_NOMEM;
    if (call(s.p, need) != hipSuccess) return MVS_E_HIP;
    if (hipStreamSynchronize(stream) != hipSuccess) return MVS_E_HIP;   // before the scratch is freed
    return 0;
}

}  // namespace

int launch_comm_cells(hipStream_t stream, const mvs_cell* d_cells, int64_t n_cells, int64_t n, const double* d_norms_sq, int d, double floor_,
                      unsigned long long* d_keys, uint32_t* d_w, unsigned long long* d_counters) {
    if (n_cells <= 0) return 0;
    const int pow2 = (d & (d - 1)) == 0;
    hipLaunchKernelGGL(k_comm_cells, dim3(grid_for(n_cells)), dim3(kCmThreads), 0, stream, d_cells, n_cells, n, d_norms_sq, (double)d,
                       1.0 / (double)d, pow2, floor_, d_keys, d_w, d_counters);
    return 0;
}

int launch_comm_edges(hipStream_t stream, const int32_t* d_lo, const int32_t* d_hi, const int32_t* d_a, int64_t n_edges, int64_t n,
                      unsigned long long* d_keys, uint32_t* d_w, unsigned long long* d_counters) {
    if (n_edges <= 0) return 0;
    hipLaunchKernelGGL(k_comm_edges, dim3(grid_for(n_edges)), dim3(kCmThreads), 0, stream, d_lo, d_hi, d_a, n_edges, n, d_keys, d_w, d_counters);
    return 0;
}

int comm_unique_max(hipStream_t stream, unsigned long long* d_keys, uint32_t* d_w, int64_t count, unsigned long long* d_tmp_keys,
                    uint32_t* d_tmp_w, unsigned long long* d_count) {
    if (count <= 0) return hipMemsetAsync(d_count, 0, 8, stream) == hipSuccess ? 0 : MVS_E_HIP;
    int rc = with_scratch(stream, [&](void* tmp, size_t& bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, d_keys, d_tmp_keys, d_w, d_tmp_w, (size_t)count, 0u, 64u, stream);
    });
    if (rc) return rc;
    return with_scratch(stream, [&](void* tmp, size_t& bytes) {
        return rocprim::reduce_by_key(tmp, bytes, d_tmp_keys, d_tmp_w, (size_t)count, d_keys, d_w, d_count, rocprim::maximum<uint32_t>(),
                                      rocprim::equal_to<unsigned long long>(), stream);
    });
}

int comm_mirror(hipStream_t stream, const unsigned long long* d_keys, const uint32_t* d_w, int64_t e, unsigned long long* d_dir_keys,
                uint32_t* d_dir_w, unsigned long long* d_tmp_keys, uint32_t* d_tmp_w) {
    if (e <= 0) return 0;
    hipLaunchKernelGGL(k_comm_mirror, dim3(grid_for(e)), dim3(kCmThreads), 0, stream, d_keys, d_w, e, d_tmp_keys, d_tmp_w);
    return with_scratch(stream, [&](void* tmp, size_t& bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, d_tmp_keys, d_dir_keys, d_tmp_w, d_dir_w, (size_t)(2 * e), 0u, 64u, stream);
    });
}

int launch_comm_csr(hipStream_t stream, const unsigned long long* d_dir_keys, int64_t m, int64_t n, long long* d_row_ptr, int32_t* d_src,
                    int32_t* d_col) {
    hipLaunchKernelGGL(k_comm_csr, dim3(grid_for(std::max(m, n + 1))), dim3(kCmThreads), 0, stream, d_dir_keys, m, n, d_row_ptr, d_src, d_col);
    return 0;
}

int launch_comm_strength(hipStream_t stream, const CommLevel& g, unsigned long long* d_k, unsigned long long* d_total) {
    if (g.n <= 0) return 0;
    if (g.w32) hipLaunchKernelGGL(k_comm_strength<uint32_t>, dim3(grid_for(g.n)), dim3(kCmThreads), 0, stream, g, g.w32, d_k, d_total);
    else hipLaunchKernelGGL(k_comm_strength<u64>, dim3(grid_for(g.n)), dim3(kCmThreads), 0, stream, g, g.w64, d_k, d_total);
    return 0;
}

int launch_comm_classify(hipStream_t stream, const CommLevel& g, int forced, int32_t* d_list0, int32_t* d_list1, int32_t* d_list2,
                         unsigned int* d_counts) {
    if (g.n <= 0) return 0;
    hipLaunchKernelGGL(k_comm_classify, dim3(grid_for(g.n)), dim3(kCmThreads), 0, stream, g, forced, d_list0, d_list1, d_list2, d_counts);
    return 0;
}

int launch_comm_identity(hipStream_t stream, int32_t* d_x, int64_t n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_comm_identity, dim3(grid_for(n)), dim3(kCmThreads), 0, stream, d_x, n);
    return 0;
}

int launch_comm_move(hipStream_t stream, const CommLevel& g, int path, const CommRound& r, const int32_t* d_comm, int32_t* d_next,
                     const unsigned long long* d_tot, const int32_t* d_size, const int32_t* d_list, const unsigned int* d_list_count,
                     int64_t list_bound, int32_t* d_over, unsigned int* d_over_count, void* d_table, int64_t table_slots, int groups,
                     unsigned long long* d_moved) {
    if (list_bound <= 0) return 0;
    int32_t* gkeys = nullptr;
    u64* gvals = nullptr;
    unsigned grid = (unsigned)std::min<int64_t>(list_bound, 1 << 16);
    if (path == 2) {
        if (!d_table || table_slots < 64 || groups < 1) return MVS_E_INVALID;
        gvals = (u64*)d_table;                                          // values first: 8-byte aligned
        gkeys = (int32_t*)(gvals + (int64_t)groups * table_slots);
        grid = (unsigned)std::min<int64_t>(list_bound, groups);
    }
#define MVS_COMM_MOVE(WT, P, warr)                                                                                                    \
    hipLaunchKernelGGL((k_comm_move<WT, P>), dim3(grid), dim3(P == 0 ? 64 : 256), 0, stream, g, warr, r, d_comm, d_next, d_tot, d_size, \
                       d_list, d_list_count, d_over, d_over_count, gkeys, gvals, table_slots, d_moved)
    if (g.w32) {
        if (path == 0) MVS_COMM_MOVE(uint32_t, 0, g.w32);
        else if (path == 1) MVS_COMM_MOVE(uint32_t, 1, g.w32);
        else MVS_COMM_MOVE(uint32_t, 2, g.w32);
    } else {
        if (path == 0) MVS_COMM_MOVE(u64, 0, g.w64);
        else if (path == 1) MVS_COMM_MOVE(u64, 1, g.w64);
        else MVS_COMM_MOVE(u64, 2, g.w64);
    }
#undef MVS_COMM_MOVE
    return 0;
}

int launch_comm_apply(hipStream_t stream, const CommLevel& g, const int32_t* d_comm, unsigned long long* d_tot, int32_t* d_size,
                      unsigned long long* d_acc) {
    if (g.n <= 0) return 0;
    if (hipMemsetAsync(d_tot, 0, (size_t)g.n * 8, stream) != hipSuccess || hipMemsetAsync(d_size, 0, (size_t)g.n * 4, stream) != hipSuccess)
        return MVS_E_HIP;
    hipLaunchKernelGGL(k_comm_tot, dim3(grid_for(g.n)), dim3(kCmThreads), 0, stream, g, d_comm, d_tot, d_size);
    const unsigned grid = grid_for(std::max(g.n, g.m));
    if (g.w32) hipLaunchKernelGGL(k_comm_inner<uint32_t>, dim3(grid), dim3(kCmThreads), 0, stream, g, g.w32, d_comm, d_acc);
    else hipLaunchKernelGGL(k_comm_inner<u64>, dim3(grid), dim3(kCmThreads), 0, stream, g, g.w64, d_comm, d_acc);
    hipLaunchKernelGGL(k_comm_sumsq, dim3(grid_for(g.n)), dim3(kCmThreads), 0, stream, d_tot, g.n, d_acc);
    return 0;
}

int launch_comm_inner_by(hipStream_t stream, const CommLevel& g, const int32_t* d_comm, unsigned long long* d_inner) {
    if (g.n <= 0) return 0;
    if (hipMemsetAsync(d_inner, 0, (size_t)g.n * 8, stream) != hipSuccess) return MVS_E_HIP;
    const unsigned grid = grid_for(std::max(g.n, g.m));
    if (g.w32) hipLaunchKernelGGL(k_comm_inner_by<uint32_t>, dim3(grid), dim3(kCmThreads), 0, stream, g, g.w32, d_comm, d_inner);
    else hipLaunchKernelGGL(k_comm_inner_by<u64>, dim3(grid), dim3(kCmThreads), 0, stream, g, g.w64, d_comm, d_inner);
    return 0;
}

int comm_renumber(hipStream_t stream, const int32_t* d_comm, int64_t n, int32_t* d_minm, int32_t* d_flag, int32_t* d_ids, int32_t* d_new) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_comm_fill, dim3(grid_for(n)), dim3(kCmThreads), 0, stream, d_minm, n, INT_MAX);
    hipLaunchKernelGGL(k_comm_minm, dim3(grid_for(n)), dim3(kCmThreads), 0, stream, d_comm, n, d_minm);
    hipLaunchKernelGGL(k_comm_flag, dim3(grid_for(n + 1)), dim3(kCmThreads), 0, stream, d_comm, n, d_minm, d_flag);
    const int rc = with_scratch(stream, [&](void* tmp, size_t& bytes) {
        return rocprim::exclusive_scan(tmp, bytes, d_flag, d_ids, 0, (size_t)n + 1, rocprim::plus<int32_t>(), stream);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_comm_new, dim3(grid_for(n)), dim3(kCmThreads), 0, stream, d_comm, n, d_minm, d_ids, d_new);
    return 0;
}

int launch_comm_compose(hipStream_t stream, int32_t* d_member, int64_t n0, const int32_t* d_new) {
    if (n0 <= 0) return 0;
    hipLaunchKernelGGL(k_comm_compose, dim3(grid_for(n0)), dim3(kCmThreads), 0, stream, d_member, n0, d_new);
    return 0;
}

int launch_comm_aggregate(hipStream_t stream, const CommLevel& g, const int32_t* d_new, unsigned long long* d_keys, unsigned long long* d_vals,
                          unsigned long long* d_self2, unsigned long long* d_cross) {
    if (g.n <= 0) return 0;
    const unsigned grid = grid_for(std::max(g.n, g.m));
    if (g.w32) hipLaunchKernelGGL(k_comm_aggregate<uint32_t>, dim3(grid), dim3(kCmThreads), 0, stream, g, g.w32, d_new, d_keys, d_vals, d_self2, d_cross);
    else hipLaunchKernelGGL(k_comm_aggregate<u64>, dim3(grid), dim3(kCmThreads), 0, stream, g, g.w64, d_new, d_keys, d_vals, d_self2, d_cross);
    return 0;
}

int comm_sum_by_key(hipStream_t stream, unsigned long long* d_keys, unsigned long long* d_vals, int64_t m, int64_t cross,
                    unsigned long long* d_tmp_keys, unsigned long long* d_tmp_vals, unsigned long long* d_count) {
    if (m <= 0 || cross <= 0) return hipMemsetAsync(d_count, 0, 8, stream) == hipSuccess ? 0 : MVS_E_HIP;
    int rc = with_scratch(stream, [&](void* tmp, size_t& bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, d_keys, d_tmp_keys, d_vals, d_tmp_vals, (size_t)m, 0u, 64u, stream);
    });
    if (rc) return rc;
    // the ~0 keys of the entries inside a community sorted behind the `cross` real ones
    return with_scratch(stream, [&](void* tmp, size_t& bytes) {
        return rocprim::reduce_by_key(tmp, bytes, d_tmp_keys, d_tmp_vals, (size_t)cross, d_keys, d_vals, d_count, rocprim::plus<unsigned long long>(),
                                      rocprim::equal_to<unsigned long long>(), stream);
    });
}

int launch_comm_split_cells(hipStream_t stream, const CommLevel& g, const int32_t* d_member, int64_t e0, int64_t e1, mvs_cell* d_cells) {
    if (e1 <= e0) return 0;
    hipLaunchKernelGGL(k_comm_split_cells, dim3(grid_for(e1 - e0)), dim3(kCmThreads), 0, stream, g, d_member, e0, e1, d_cells);
    return 0;
}

int launch_comm_gather_first(hipStream_t stream, const int32_t* d_comm, const int32_t* d_flag, const int32_t* d_ids, int64_t n,
                             const unsigned long long* d_in_a, const unsigned long long* d_in_b, unsigned long long* d_out_a,
                             unsigned long long* d_out_b) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_comm_gather_first, dim3(grid_for(n)), dim3(kCmThreads), 0, stream, d_comm, d_flag, d_ids, n, d_in_a, d_in_b, d_out_a, d_out_b);
    return 0;
}

int launch_comm_degree(hipStream_t stream, const CommLevel& g, int32_t* d_degree) {
    if (g.n <= 0) return 0;
    hipLaunchKernelGGL(k_comm_degree, dim3(grid_for(g.n)), dim3(kCmThreads), 0, stream, g, d_degree);
    return 0;
}

}  // namespace mvs
