// mvs_kmer.hip -- FracMinHash values of DNA bytes (mvs_hash_set_from_sequences): for every position whose ksize bytes are all
// bases, the first word of MurmurHash3_x64_128 of the canonical k-mer, kept where it is <= max_hash.  The contract is stated in
// include/mvs_hip.h ("sketches from sequences"); mvs_kmer_hash in mvs_capi_kmer.hip is the same rule on the host.
//
// Units of work.  The host lays the samples out as units: up to U = option kmer_unit consecutive k-mer positions of ONE sample
// (a sample without a position has none), each read by one workgroup together with the ksize - 1 bytes behind its last
// position.  A workgroup
//   1. stages the unit's bytes in LDS with aligned 16-byte loads (the chunks that stick out of the input buffer byte by byte);
//   2. gives every thread R = ceil(positions / 256) consecutive positions.  The thread rolls two 2-bit words over its bytes,
//      the forward k-mer (first base in the top bits) and its reverse complement, and counts the bases since the last break:
//      ksize - 1 bytes of warm-up, then one position per byte.  The full unit has R = 68 = 4 x 17, so the lanes of a wave read
//      LDS bytes 17 dwords apart: no bank is asked twice;
//   3. per position: the smaller word is the canonical k-mer (2-bit order = string order).  With the complement of the OTHER
//      word the same k-mer stands first base in the lowest bits, and its ASCII bytes -- what the hash reads -- are 8 bits -> 4
//      selector bytes (two shift-or-mask steps) -> one v_perm_b32 into the word "ACGT".  The hash runs for every lane, valid or
//      not (no divergence), in the instantiation for the shape of its input (whole blocks, tail words: six cover ksize
//      1 .. 32), so the loop holds no branch on ksize; its 64-bit multiplies by constants are one v_mad_u64_u32 with the
//      cross terms in the addend (mad64 / mul64_mad of mvs_murmur_dev.h, shared with mvs_protein.hip);
//   4. kept values leave per wave: ballot, the lane's rank among the kept, the value into the wave's own LDS buffer of 512
//      entries; a buffer that cannot take the next ballot's values, and every buffer at the end, is flushed with ONE atomic on
//      the cursor of the staging list and coalesced stores of (value, sample) where cursor + i is below the list's capacity.
//      (An atomic per ballot was the first version: all of them hit one address, the L2 serves about one per 12 ns there, and
//      at scaled = 1000 the 10^6 kept values of 10^9 bases -- one per ballot -- cost 12 ms, 2.5 x the arithmetic.)  The counts
//      -- valid positions and kept values per sample, through LDS to one atomic per workgroup each; kept values in all, the
//      cursor itself -- are always exact, so a list that was too short is known to be, and by how much.
// k_kmer_scatter then moves the staged values to their samples' ranges (exclusive scan of the per-sample counts, done on the
// host), again with one atomic per wave and sample.  Arrival order is arbitrary; the segmented sort and unique compaction of
// mvs_hash_set_create make the result deterministic.
#include "mvs_internal.h"
#include "mvs_murmur_dev.h"

namespace mvs {

namespace {

constexpr int kKmThreads = 256;
constexpr int kWaveBuf = 512;                                   // kept values a wave collects in LDS between two flushes
constexpr int kKmBufBytes = kKmThreads / 64 * kWaveBuf * 8;     // ... of the four waves: 16 KiB

// four bases (2 bits each, the first in the lowest bits) -> their four ASCII bytes, the first in the lowest byte
__device__ __forceinline__ uint32_t ascii4(uint32_t x) {
    uint32_t y = (x | (x << 12)) & 0x000f000fu;
    y = (y | (y << 6)) & 0x03030303u;
    return __builtin_amdgcn_perm(0u, 0x54474341u, y);   // selector bytes 0..3 pick from "ACGT"
}
// bases [8w, 8w + 8) of a k-mer (first base in the lowest bits) as the hash's little-endian word w
__device__ __forceinline__ uint64_t ascii8(uint64_t lsb_first, int w) {
    const uint32_t x = (uint32_t)(lsb_first >> (16 * w)) & 0xffffu;
    return (uint64_t)ascii4(x & 0xffu) | ((uint64_t)ascii4(x >> 8) << 32);
}

// MurmurHash3_x64_128, first word, of the ksize ASCII bytes of the k-mer `lsb_first`.  The shape of the input is a template
// parameter, so that a kernel's loop holds no branch on it: BLOCKS whole 16-byte blocks (0 .. 2), then TAIL = 0 nothing, 1 a
// k1 word of 1 .. 8 bytes, 2 a full k1 word and a k2 word of 1 .. 7 bytes.  last_mask keeps the tail's last word's bytes.
template <int BLOCKS, int TAIL>
__device__ __forceinline__ uint64_t murmur_kmer(uint64_t lsb_first, int ksize, uint32_t seed, uint64_t last_mask) {
    uint64_t h1 = seed, h2 = seed;
    if (BLOCKS >= 1) murmur_block(h1, h2, ascii8(lsb_first, 0), ascii8(lsb_first, 1));
    if (BLOCKS == 2) murmur_block(h1, h2, ascii8(lsb_first, 2), ascii8(lsb_first, 3));
    if (TAIL == 2) h2 ^= mur_k2(ascii8(lsb_first, 2 * BLOCKS + 1) & last_mask);
    if (TAIL == 1) h1 ^= mur_k1(ascii8(lsb_first, 2 * BLOCKS) & last_mask);
    if (TAIL == 2) h1 ^= mur_k1(ascii8(lsb_first, 2 * BLOCKS));
    h1 ^= (uint64_t)ksize;
    h2 ^= (uint64_t)ksize;
    h1 += h2;
    h2 += h1;
    h1 = fmix64(h1);
    h2 = fmix64(h2);
    return h1 + h2;
}

// counters: [0] cursor of the staging list = kept values; sample_counts / sample_valid: kept values / valid positions per sample
template <int BLOCKS, int TAIL>
__global__ __launch_bounds__(kKmThreads) void k_kmer_hash(const uint8_t* __restrict__ bases, long long total_bytes,
                                                          const KmerUnit* __restrict__ units, int ksize, uint32_t seed,
                                                          uint64_t max_hash, unsigned long long* __restrict__ out_vals,
                                                          int32_t* __restrict__ out_sample, unsigned long long cap,
                                                          unsigned long long* __restrict__ counters,
                                                          unsigned long long* __restrict__ sample_counts,
                                                          unsigned long long* __restrict__ sample_valid) {
    // LDS: the waves' buffers of kept values | the workgroup's two counts | the unit's bytes
    extern __shared__ __attribute__((aligned(16))) uint8_t km_shared[];
    unsigned long long* wbuf = (unsigned long long*)km_shared + (threadIdx.x >> 6) * kWaveBuf;
    unsigned int* wg_counts = (unsigned int*)(km_shared + kKmBufBytes);
    uint8_t* km_lds = km_shared + kKmBufBytes + 16;
    const KmerUnit u = units[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63;
    if (t < 2) wg_counts[t] = 0;
    const int npos = u.npos;
    const int nbytes = npos + ksize - 1;

    // 1. the unit's bytes [byte0, byte0 + nbytes) of the buffer, staged so that byte j lies at km_lds[sh + j]
    const uint8_t* g0 = bases + u.byte0;
    const int sh = (int)((uintptr_t)g0 & 15);
    const uint8_t* a0 = g0 - sh;
    const uint8_t* lo = bases;
    const uint8_t* hi = bases + total_bytes;
    const int chunks = (sh + nbytes + 15) >> 4;
    for (int c = t; c < chunks; c += kKmThreads) {
        const uint8_t* a = a0 + 16 * (long long)c;
        if (a >= lo && a + 16 <= hi) {
            *(uint4*)(km_lds + 16 * c) = *(const uint4*)a;
        } else {
            for (int b = 0; b < 16; ++b) km_lds[16 * c + b] = (a + b >= lo && a + b < hi) ? a[b] : (uint8_t)0;
        }
    }
    __syncthreads();

    // 2. R consecutive positions per thread
    const int R = (npos + kKmThreads - 1) / kKmThreads;
    const uint64_t mask = ksize == 32 ? ~0ULL : ((1ULL << (2 * ksize)) - 1);
    const uint64_t last_mask = (ksize & 7) ? ((1ULL << (8 * (ksize & 7))) - 1) : ~0ULL;
    const int top = 2 * (ksize - 1);
    const uint8_t* mine = km_lds + sh + t * R;
    const int first = t * R;               // the thread's first byte = its first position
    uint64_t fw = 0, rc = 0;
    int run = 0;
    auto roll = [&](int idx) {
        const uint32_t b = idx < nbytes ? (uint32_t)mine[idx - first] : 0u;
        const uint32_t up = b & 0xdfu;
        const bool base = up == 0x41u || up == 0x43u || up == 0x47u || up == 0x54u;
        uint32_t code = (up >> 1) & 3u;      // A 0, C 1, G 3, T 2
        code ^= code >> 1;                    // A 0, C 1, G 2, T 3
        fw = ((fw << 2) | code) & mask;
        rc = (rc >> 2) | ((uint64_t)(3u - code) << top);
        run = base ? run + 1 : 0;
    };
    for (int j = 0; j < ksize - 1; ++j) roll(first + j);

    // the wave's buffer goes to the staging list: one atomic on the list's cursor, coalesced stores
    auto flush = [&](unsigned int fill) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(counters + 0, (unsigned long long)fill);
        at = __shfl(at, 0);
        for (unsigned int i = lane; i < fill; i += 64)
            if (at + i < cap) {
                out_vals[at + i] = wbuf[i];
                out_sample[at + i] = u.sample;
            }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    };
    unsigned int wave_kept = 0, wave_valid = 0, fill = 0;   // uniform over the wave: sums of ballots
    for (int j = 0; j < R; ++j) {
        const int p = first + j;              // the position; its last byte is p + ksize - 1
        roll(p + ksize - 1);
        const bool valid = p < npos && run >= ksize;
        // 3. canonical k-mer, first base in the lowest bits
        const uint64_t lsb_first = (fw <= rc ? ~rc : ~fw) & mask;
        const uint64_t h = murmur_kmer<BLOCKS, TAIL>(lsb_first, ksize, seed, last_mask);
        const bool keep = valid && h <= max_hash;
        // 4. the kept values to the wave's buffer, in lane order
        const unsigned long long vm = __ballot(valid);
        const unsigned long long km = __ballot(keep);
        wave_valid += (unsigned int)__popcll(vm);
        if (km) {
            const unsigned int n = (unsigned int)__popcll(km);
            if (fill + n > (unsigned int)kWaveBuf) {
                flush(fill);
                fill = 0;
            }
            if (keep) wbuf[fill + (unsigned int)__popcll(km & ((1ULL << lane) - 1))] = h;
            fill += n;
            wave_kept += n;
        }
    }
    if (fill) flush(fill);
    // the counts: one LDS atomic per wave, then one global atomic per workgroup and count
    if (lane == 0) {
        if (wave_valid) atomicAdd(wg_counts + 0, wave_valid);
        if (wave_kept) atomicAdd(wg_counts + 1, wave_kept);
    }
    __syncthreads();
    if (t == 0) {
        if (wg_counts[0]) atomicAdd(sample_valid + u.sample, (unsigned long long)wg_counts[0]);
        if (wg_counts[1]) atomicAdd(sample_counts + u.sample, (unsigned long long)wg_counts[1]);
    }
}

// staged (value, sample) -> out[offsets[sample] + the sample's cursor]; one atomic per wave and sample met
__global__ __launch_bounds__(kKmThreads) void k_kmer_scatter(const unsigned long long* __restrict__ vals,
                                                             const int32_t* __restrict__ samples, long long n,
                                                             const long long* __restrict__ offsets,
                                                             unsigned long long* __restrict__ cursors,
                                                             unsigned long long* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kKmThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = i < n;
    const int32_t s = active ? samples[i] : -1;
    const unsigned long long v = active ? vals[i] : 0;
    bool pending = active;
    unsigned long long pm = __ballot(pending);
    while (pm) {
        const int leader = __ffsll((long long)pm) - 1;
        const int32_t s0 = __shfl(s, leader);
        const bool mine = pending && s == s0;
        const unsigned long long mm = __ballot(mine);
        unsigned long long at = 0;
        if (lane == leader) at = atomicAdd(cursors + s0, (unsigned long long)__popcll(mm));
        at = __shfl(at, leader);
        if (mine) {
            out[offsets[s0] + (long long)at + __popcll(mm & ((1ULL << lane) - 1))] = v;
            pending = false;
        }
        pm = __ballot(pending);
    }
}

}  // namespace

size_t kmer_lds_bytes(int unit, int ksize) {
    return (size_t)kKmBufBytes + 16 + (((size_t)unit + (size_t)ksize - 1 + 15 + 15) & ~(size_t)15);
}

int launch_kmer_hash(hipStream_t stream, const uint8_t* d_bases, long long total_bytes, const KmerUnit* d_units, long long n_units,
                     int unit, int ksize, uint32_t seed, uint64_t max_hash, unsigned long long* d_vals, int32_t* d_sample,
                     unsigned long long cap, unsigned long long* d_counters, unsigned long long* d_sample_counts,
                     unsigned long long* d_sample_valid) {
    if (n_units <= 0) return 0;
    if (n_units >= (1LL << 31) || unit < 1 || unit > kKmerUnitMax || ksize < 1 || ksize > 32) return MVS_E_RANGE;
    // the shape of the hash's input picks the instantiation
    const int blocks = ksize / 16, rem = ksize % 16, tail = rem == 0 ? 0 : rem <= 8 ? 1 : 2;
    void (*kernel)(const uint8_t*, long long, const KmerUnit*, int, uint32_t, uint64_t, unsigned long long*, int32_t*, unsigned long long,
                   unsigned long long*, unsigned long long*, unsigned long long*) =
        blocks == 0 ? (tail == 1 ? k_kmer_hash<0, 1> : k_kmer_hash<0, 2>)
        : blocks == 1 ? (tail == 0 ? k_kmer_hash<1, 0> : tail == 1 ? k_kmer_hash<1, 1> : k_kmer_hash<1, 2>)
                      : k_kmer_hash<2, 0>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_units), dim3(kKmThreads), kmer_lds_bytes(unit, ksize), stream, d_bases, total_bytes,
                       d_units, ksize, seed, max_hash, d_vals, d_sample, cap, d_counters, d_sample_counts, d_sample_valid);
    return 0;
}

int launch_kmer_scatter(hipStream_t stream, const unsigned long long* d_vals, const int32_t* d_sample, long long n,
                        const long long* d_offsets, unsigned long long* d_cursors, unsigned long long* d_out) {
    if (n <= 0) return 0;
    const long long blocks = (n + kKmThreads - 1) / kKmThreads;
    if (blocks >= (1LL << 31)) return MVS_E_RANGE;
    hipLaunchKernelGGL(k_kmer_scatter, dim3((unsigned)blocks), dim3(kKmThreads), 0, stream, d_vals, d_sample, n, d_offsets, d_cursors,
                       d_out);
    return 0;
}

}  // namespace mvs
