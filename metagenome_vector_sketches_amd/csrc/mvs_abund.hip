// mvs_abund.hip -- the counted set build (mvs_hash_set_create_counted, mvs_kmer_sketcher_finish): values grouped by sample ->
// per sample the ascending distinct values whose abundance (the sum of the weights of their occurrences, 1 each without
// weights) passes a filter, with that abundance.  The contract is stated in include/mvs_hip.h ("abundances").
//
// Sort.  Samples of up to option abund_big_segment values go through rocprim's segmented radix sort in batches (one workgroup
// sorts a segment there, so a long one is slow); each longer sample is sorted by a device-wide radix sort of its own.
//
// Run sums.  After the sort equal values of a sample are neighbours: a RUN.  Its first position is its HEAD: the position
// starts a sample (a bit map of the samples' first positions says so) or its value differs from the one before it.  The sorted
// array is cut into units of U = option abund_unit positions wherever the samples' borders lie, ONE WAVE per unit, which walks
// its unit in chunks of 64 positions from the LAST chunk to the first, so that the weight behind a head is known when the head
// is met.  No wave's work depends on the length of a sample or of a run:
//   A  k_ab_units   per unit: has it a head, and the weight in front of its first head (all of it without one);
//   B  a segmented inclusive scan over the units in REVERSE order (pass A writes them reversed): tail[u] = the weight from
//      unit u's first position to the first head at or behind it; unit u's last run ends with tail[u + 1];
//   C  k_ab_count   redoes the unit's runs with that carry: every head now knows its abundance.  Counts the unit's heads and
//      the heads that pass the filter, feeds the histogram (the bins of the sample the unit starts in through the wave's LDS
//      counters, one atomic per touched bin; heads behind a border inside the unit straight to memory) and flags a sum >= 2^32;
//   S  two exclusive scans of the units' counts;
//   D  k_ab_fill    the same walk once more: passing heads write (value, abundance) at their rank; a position that starts a
//      sample writes the ranks it sees as that sample's offsets (among the passing heads and among all heads -- the second is
//      the statistic `distinct`); k_ab_tail, one thread per sample, then gives empty samples the offsets of the sample behind
//      them and samples that start at the array's end the totals.
// A value whose weights sum to zero counts as absent: no distinct value, no histogram bin (bin 0 stays 0), never kept.
// All sums are integers: no order of the units can change them.
#include "mvs_internal.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace mvs {

namespace {

constexpr int kAbThreads = 256;
constexpr int kAbWaves = kAbThreads / 64;

// the scan's element: v = weight in front of the first head, f = the stretch holds a head
struct AbCarryOp {
    __host__ __device__ AbCarry operator()(const AbCarry& left, const AbCarry& right) const {
        // `left` lies BEHIND `right` in the array (reverse order): right's weight reaches into left only without a head
        AbCarry r;
        r.v = right.f ? right.v : left.v + right.v;
        r.f = left.f | right.f;
        return r;
    }
};

__device__ __forceinline__ unsigned long long wave_incl_sum(unsigned long long x, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    return x;
}

// the sample that holds position p: the last s with off[s] <= p (p < off[n])
__device__ __forceinline__ long long ab_sample_of(const long long* __restrict__ off, long long n, long long p) {
    long long lo = 0, hi = n;          // answer in [lo, hi)
    while (hi - lo > 1) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// bit p of `borders` := 1 for every sample that starts at p < total
__global__ __launch_bounds__(kAbThreads) void k_ab_borders(const long long* __restrict__ off, long long n, long long total,
                                                           unsigned int* __restrict__ borders) {
    const long long s = (long long)blockIdx.x * kAbThreads + threadIdx.x;
    if (s >= n) return;
    const long long p = off[s];
    if (p < total) atomicOr(borders + (p >> 5), 1u << (p & 31));
}

// what one chunk of 64 positions looks like to its lanes
struct AbChunk {
    unsigned long long key, w, incl;   // the lane's value, weight, inclusive prefix sum of the weights over the chunk
    unsigned long long heads, live;    // ballots: head positions, positions inside the unit
    bool head, border;
};

__device__ __forceinline__ AbChunk ab_load(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ weights,
                                           const unsigned int* __restrict__ borders, long long p, long long end, int lane) {
    AbChunk c;
    const bool in = p < end;
    c.key = in ? keys[p] : 0ULL;
    c.w = in ? (weights ? (unsigned long long)weights[p] : 1ULL) : 0ULL;
    c.border = in && ((borders[p >> 5] >> (p & 31)) & 1u);
    unsigned long long prev = __shfl_up(c.key, 1);
    if (lane == 0 && in && p > 0) prev = keys[p - 1];
    c.head = in && (c.border || p == 0 || prev != c.key);
    c.heads = __ballot(c.head);
    c.live = __ballot(in);
    c.incl = wave_incl_sum(c.w, lane);
    return c;
}

// The abundance of the lane's head (valid where c.head): the weights from it to the next head of the chunk, or to the chunk's
// end plus `tail` (the weight behind the chunk up to the next head).  Also moves `tail` in front of the chunk.
__device__ __forceinline__ unsigned long long ab_runs(const AbChunk& c, unsigned long long& tail, int lane) {
    const unsigned long long total = __shfl(c.incl, 63);
    const unsigned long long excl = c.incl - c.w;
    const unsigned long long above = lane == 63 ? 0ULL : c.heads & ~((2ULL << lane) - 1ULL);
    const int next = above ? __ffsll((long long)above) - 1 : 63;
    const unsigned long long next_excl = __shfl(excl, next);        // (every lane takes part)
    const unsigned long long a = above ? next_excl - excl : total - excl + tail;
    if (c.heads) {
        const int first = __ffsll((long long)c.heads) - 1;
        tail = __shfl(excl, first);
    } else {
        tail += total;
    }
    return a;
}

// pass A: summary[n_units - 1 - u] of unit u
__global__ __launch_bounds__(kAbThreads) void k_ab_units(const unsigned long long* __restrict__ keys,
                                                         const uint32_t* __restrict__ weights,
                                                         const unsigned int* __restrict__ borders, long long total, int unit,
                                                         long long n_units, AbCarry* __restrict__ summary) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * kAbWaves + (threadIdx.x >> 6);
    if (u >= n_units) return;
    const long long b = u * unit, e = b + unit < total ? b + unit : total;
    unsigned long long pre = 0;
    bool found = false;
    for (long long p0 = b; p0 < e && !found; p0 += 64) {              // (uniform over the wave)
        const AbChunk c = ab_load(keys, weights, borders, p0 + lane, e, lane);
        if (c.heads) {
            const int first = __ffsll((long long)c.heads) - 1;
            pre += __shfl(c.incl - c.w, first);
            found = true;
        } else {
            pre += __shfl(c.incl, 63);
        }
    }
    if (lane == 0) {
        AbCarry s;
        s.v = pre;
        s.f = found ? 1ULL : 0ULL;
        summary[n_units - 1 - u] = s;
    }
}

// passes C (FILL = false) and D (FILL = true).  tails: pass B's result, reversed like the summaries.
// counts (C): [u] heads, [n_units + 1 + u] passing heads of unit u.  flags: [0] != 0 = an abundance reached 2^32.
template <bool FILL>
__global__ __launch_bounds__(kAbThreads) void k_ab_walk(const unsigned long long* __restrict__ keys,
                                                        const uint32_t* __restrict__ weights,
                                                        const unsigned int* __restrict__ borders, long long total, int unit,
                                                        long long n_units, const AbCarry* __restrict__ tails,
                                                        unsigned long long min_ab, unsigned long long max_ab,
                                                        long long* __restrict__ head_counts, long long* __restrict__ pass_counts,
                                                        unsigned int* __restrict__ flags, const long long* __restrict__ off,
                                                        long long n, unsigned long long* __restrict__ hist,
                                                        const long long* __restrict__ head_start,
                                                        const long long* __restrict__ pass_start,
                                                        unsigned long long* __restrict__ out_vals, uint32_t* __restrict__ out_ab,
                                                        long long* __restrict__ new_off, long long* __restrict__ distinct_off) {
    __shared__ unsigned int bins[kAbWaves][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long u = (long long)blockIdx.x * kAbWaves + wave;
    if (u >= n_units) return;                                          // (no workgroup barrier below)
    const long long b = u * unit, e = b + unit < total ? b + unit : total;
    // the weight behind the unit up to the next head: tail of unit u + 1 (0 where that unit starts with a head)
    unsigned long long tail = u + 1 < n_units ? tails[n_units - 2 - u].v : 0ULL;
    const bool want_hist = !FILL && hist != nullptr;
    long long s_first = 0, first_border = e;
    if (want_hist) {
        for (int i = lane; i < 256; i += 64) bins[wave][i] = 0u;
        s_first = ab_sample_of(off, n, b);
        // the first border behind the unit's first position
        for (long long p0 = b; p0 < e && first_border == e; p0 += 64) {
            const long long p = p0 + lane;
            const bool bd = p < e && p > b && ((borders[p >> 5] >> (p & 31)) & 1u);
            const unsigned long long m = __ballot(bd);
            if (m) first_border = p0 + __ffsll((long long)m) - 1;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    long long n_heads = 0, n_pass = 0;                                 // of the chunks walked so far (behind the current one)
    long long heads_left = 0, pass_left = 0;
    if (FILL) {
        heads_left = head_start[u + 1] - head_start[u];
        pass_left = pass_start[u + 1] - pass_start[u];
    }
    bool over = false;
    const long long chunks = (e - b + 63) >> 6;
    for (long long k = chunks - 1; k >= 0; --k) {                      // (uniform over the wave)
        const long long p = b + (k << 6) + lane;
        const AbChunk c = ab_load(keys, weights, borders, p, e, lane);
        const unsigned long long a = ab_runs(c, tail, lane);
        const bool pass = c.head && a >= min_ab && (max_ab == 0ULL || a <= max_ab);
        const unsigned long long pm = __ballot(pass);
        // a value whose weights sum to zero is not there: it is no distinct value and has no bin
        const unsigned long long hm = __ballot(c.head && a > 0ULL);
        const int ch = __popcll(hm), cp = __popcll(pm);
        if (!FILL) {
            over |= c.head && a > 0xffffffffULL;
            n_heads += ch;
            n_pass += cp;
            if (want_hist && c.head && a > 0ULL) {
                const unsigned int bin = a < 255ULL ? (unsigned int)a : 255u;
                if (p < first_border) atomicAdd(&bins[wave][bin], 1u);
                else atomicAdd(hist + (unsigned long long)ab_sample_of(off, n, p) * 256ULL + bin, 1ULL);
            }
        } else {
            heads_left -= ch;
            pass_left -= cp;
            const unsigned long long below = (1ULL << lane) - 1ULL;
            const long long pass_rank = pass_start[u] + pass_left + __popcll(pm & below);
            if (pass) {
                out_vals[pass_rank] = c.key;
                out_ab[pass_rank] = (uint32_t)a;
            }
            if (c.border) {
                const long long head_rank = head_start[u] + heads_left + __popcll(hm & below);
                // the sample that holds p starts here; the empty samples in front of it copy its offsets in k_ab_tail
                const long long s = ab_sample_of(off, n, p);
                new_off[s] = pass_rank;
                distinct_off[s] = head_rank;
            }
        }
    }
    if (!FILL) {
        if (lane == 0) {
            head_counts[u] = n_heads;
            pass_counts[u] = n_pass;
        }
        if (over) atomicOr(flags, 1u);
        if (want_hist) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int i = lane; i < 256; i += 64) {
                const unsigned int v = bins[wave][i];
                if (v) atomicAdd(hist + (unsigned long long)s_first * 256ULL + (unsigned int)i, (unsigned long long)v);
            }
        }
    }
}

// after pass D: samples that start at the array's end (and entry n) get the totals, empty samples elsewhere the offsets of the
// sample behind them; then nothing is left unwritten.  One thread per sample: no thread's work grows with a run of empty samples
__global__ __launch_bounds__(kAbThreads) void k_ab_tail(const long long* __restrict__ off, long long n, long long total,
                                                        const long long* __restrict__ head_total,
                                                        const long long* __restrict__ pass_total, long long* __restrict__ new_off,
                                                        long long* __restrict__ distinct_off) {
    const long long s = (long long)blockIdx.x * kAbThreads + threadIdx.x;
    if (s > n) return;
    if (s == n || off[s] >= total) {
        new_off[s] = pass_total ? *pass_total : 0;
        distinct_off[s] = head_total ? *head_total : 0;
    } else if (off[s + 1] == off[s]) {
        // an empty sample in front of the array's end: the offsets of the sample that holds its position, which pass D wrote
        const long long t = ab_sample_of(off, n, off[s]);
        new_off[s] = new_off[t];
        distinct_off[s] = distinct_off[t];
    }
}

__global__ __launch_bounds__(kAbThreads) void k_ab_sizes(const long long* __restrict__ new_off, long long n, int32_t* __restrict__ sizes) {
    const long long s = (long long)blockIdx.x * kAbThreads + threadIdx.x;
    if (s < n) sizes[s] = (int32_t)(new_off[s + 1] - new_off[s]);
}

unsigned ab_blocks(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

int ab_sort_segments(hipStream_t stream, const unsigned long long* d_in, unsigned long long* d_out, const uint32_t* d_win,
                     uint32_t* d_wout, unsigned int count, unsigned int segments, const unsigned int* d_begin,
                     const unsigned int* d_end, void* d_scratch, size_t scratch_bytes, size_t* scratch_needed) {
    if (!d_win) return hs_sort_segments(stream, d_in, d_out, count, segments, d_begin, d_end, d_scratch, scratch_bytes, scratch_needed);
    size_t need = 0;
    hipError_t e = rocprim::segmented_radix_sort_pairs(nullptr, need, d_in, d_out, d_win, d_wout, count, segments, d_begin, d_end, 0, 64, stream);
    if (e != hipSuccess) return MVS_E_HIP;
    if (scratch_needed) *scratch_needed = need;
    if (d_scratch == nullptr) return 0;
    if (scratch_bytes < need) return MVS_E_CAPACITY;
    e = rocprim::segmented_radix_sort_pairs(d_scratch, need, d_in, d_out, d_win, d_wout, count, segments, d_begin, d_end, 0, 64, stream);
    return e == hipSuccess ? 0 : MVS_E_HIP;
}

int ab_sort_whole(hipStream_t stream, const unsigned long long* d_in, unsigned long long* d_out, const uint32_t* d_win,
                  uint32_t* d_wout, unsigned int count, void* d_scratch, size_t scratch_bytes, size_t* scratch_needed) {
    size_t need = 0;
    hipError_t e = d_win ? rocprim::radix_sort_pairs(nullptr, need, d_in, d_out, d_win, d_wout, count, 0, 64, stream)
                         : rocprim::radix_sort_keys(nullptr, need, d_in, d_out, count, 0, 64, stream);
    if (e != hipSuccess) return MVS_E_HIP;
    if (scratch_needed) *scratch_needed = need;
    if (d_scratch == nullptr) return 0;
    if (scratch_bytes < need) return MVS_E_CAPACITY;
    e = d_win ? rocprim::radix_sort_pairs(d_scratch, need, d_in, d_out, d_win, d_wout, count, 0, 64, stream)
              : rocprim::radix_sort_keys(d_scratch, need, d_in, d_out, count, 0, 64, stream);
    return e == hipSuccess ? 0 : MVS_E_HIP;
}

size_t ab_work_bytes(long long n_units) {
    size_t need_c = 0, need_s = 0;
    (void)rocprim::inclusive_scan(nullptr, need_c, (AbCarry*)nullptr, (AbCarry*)nullptr, (size_t)n_units, AbCarryOp(), nullptr);
    (void)rocprim::exclusive_scan(nullptr, need_s, (long long*)nullptr, (long long*)nullptr, 0LL, (size_t)n_units + 1,
                                  rocprim::plus<long long>(), nullptr);
    return std::max(need_c, need_s) + 256;
}

int launch_ab_borders(hipStream_t stream, const long long* d_off, long long n, long long total, unsigned int* d_borders) {
    if (n <= 0 || total <= 0) return 0;
    hipLaunchKernelGGL(k_ab_borders, dim3(ab_blocks(n, kAbThreads)), dim3(kAbThreads), 0, stream, d_off, n, total, d_borders);
    return 0;
}

int ab_count(hipStream_t stream, const AbArgs& a, void* d_scratch, size_t scratch_bytes) {
    if (a.total <= 0 || a.n_units <= 0) return 0;
    if (a.unit < 64 || a.n_units >= (1LL << 31) * kAbWaves) return MVS_E_RANGE;
    const dim3 grid(ab_blocks(a.n_units, kAbWaves)), block(kAbThreads);
    hipLaunchKernelGGL(k_ab_units, grid, block, 0, stream, a.keys, a.weights, a.borders, a.total, a.unit, a.n_units, a.summary);
    size_t need = scratch_bytes;
    hipError_t e = rocprim::inclusive_scan(d_scratch, need, a.summary, a.tails, (size_t)a.n_units, AbCarryOp(), stream);
    if (e != hipSuccess) return MVS_E_HIP;
    hipLaunchKernelGGL(k_ab_walk<false>, grid, block, 0, stream, a.keys, a.weights, a.borders, a.total, a.unit, a.n_units, a.tails,
                       a.min_ab, a.max_ab, a.head_counts, a.pass_counts, a.flags, a.off, a.n, a.hist, (const long long*)nullptr,
                       (const long long*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr, (long long*)nullptr,
                       (long long*)nullptr);
    // (entry n_units of either count array is zero: the exclusive scans end with the totals)
    need = scratch_bytes;
    e = rocprim::exclusive_scan(d_scratch, need, a.head_counts, a.head_start, 0LL, (size_t)a.n_units + 1, rocprim::plus<long long>(), stream);
    if (e != hipSuccess) return MVS_E_HIP;
    need = scratch_bytes;
    e = rocprim::exclusive_scan(d_scratch, need, a.pass_counts, a.pass_start, 0LL, (size_t)a.n_units + 1, rocprim::plus<long long>(), stream);
    return e == hipSuccess ? 0 : MVS_E_HIP;
}

int ab_fill(hipStream_t stream, const AbArgs& a, unsigned long long* d_out_vals, uint32_t* d_out_ab, long long* d_new_off,
            long long* d_distinct_off, int32_t* d_sizes) {
    const bool any = a.total > 0 && a.n_units > 0;
    if (any) {
        const dim3 grid(ab_blocks(a.n_units, kAbWaves)), block(kAbThreads);
        hipLaunchKernelGGL(k_ab_walk<true>, grid, block, 0, stream, a.keys, a.weights, a.borders, a.total, a.unit, a.n_units, a.tails,
                           a.min_ab, a.max_ab, (long long*)nullptr, (long long*)nullptr, (unsigned int*)nullptr, a.off, a.n,
                           (unsigned long long*)nullptr, a.head_start, a.pass_start, d_out_vals, d_out_ab, d_new_off, d_distinct_off);
    }
    hipLaunchKernelGGL(k_ab_tail, dim3(ab_blocks(a.n + 1, kAbThreads)), dim3(kAbThreads), 0, stream, a.off, a.n, a.total,
                       any ? a.head_start + a.n_units : (const long long*)nullptr, any ? a.pass_start + a.n_units : (const long long*)nullptr,
                       d_new_off, d_distinct_off);
    if (a.n > 0) hipLaunchKernelGGL(k_ab_sizes, dim3(ab_blocks(a.n, kAbThreads)), dim3(kAbThreads), 0, stream, d_new_off, a.n, d_sizes);
    return 0;
}

}  // namespace mvs
