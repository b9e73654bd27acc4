// mvs_protein.hip -- FracMinHash values of residues (mvs_hash_set_from_residues): for every window of ksize residues the first
// word of MurmurHash3_x64_128 of the window's bytes in the chosen alphabet, kept where it is <= max_hash; the residues are the
// input's own bytes (input kind protein) or the codons of DNA in all six reading frames (translate).  The contract is stated
// in include/mvs_hip.h ("protein sketches"); mvs_aa_hash and mvs_translate_codon in mvs_capi_protein.hip state it on the host.
//
// The frame is that of mvs_kmer.hip: units of up to U window positions of ONE sample, one workgroup of 256 threads per unit,
// the unit's bytes (positions + window - 1) staged in LDS with aligned, bounds-checked 16-byte loads, kept values through the
// wave's LDS buffer of 512 entries to the staging list with one atomic per flush, exact counters.  Between staging and
// hashing stands a classification pass, and the hashing loop reads what it wrote:
//   2. classification.  A plane is the residues of ONE reading frame on ONE strand, one encoded byte per residue, 0 for a break
//      (a byte that is no residue; a codon with a byte that is no base).  protein: one plane, plane[q] = the byte map of byte q.
//      translate: for frame f = 0, 1, 2, codon m of the frame is the bytes 3m + f .. 3m + f + 2; the forward plane holds its
//      residue at m, the reverse plane holds the residue of its reverse complement at M4 - 1 - m (M4 = the frame's codons,
//      rounded up to 4): a window of the reverse strand reads its codons last to first, so mirrored they lie first to last.
//      A thread makes four consecutive codons of one frame at a time: 14 byte reads, 14 look-ups in the byte map (base ->
//      T C A G = 0 1 2 3, else 0x80), per codon one index 16x + 4y + z and one look-up in each of two 64-entry tables (the
//      alphabet's residue of the codon, and of its reverse complement), one dword store per plane.  So every codon is
//      translated once per strand, and the alphabet lives in the tables, which the host fills: the hashing loop does not
//      know it.
//   3. hashing, one frame and strand per pass.  A window is ksize CONSECUTIVE bytes of its plane, window m of the frame at
//      byte m (forward) or M4 - m - ksize (reverse).  The lanes of a wave take consecutive m, so a wave's loads touch 16 or 17
//      consecutive dwords: every bank once, lanes of one dword served by broadcast.  A lane loads the dwords around its window
//      aligned and shifts them into place with v_alignbyte_b32 (ksize / 4 + 1 loads and ksize / 4 shifts against ksize
//      byte loads and as many merges for a walk that gathers F[p + 3i] from an interleaved plane; three rolling byte queues
//      per strand would need 96 registers at ksize 64 and a dynamic insert position).  A window is valid iff none of its
//      bytes is 0, tested on the words the hash reads.  The hash is instantiated per shape (0 .. 4 whole blocks x tail of 0,
//      <= 8, <= 15 bytes), so the loop holds no branch on ksize.
#include "mvs_internal.h"
#include "mvs_murmur_dev.h"

#include <cstring>

namespace mvs {

namespace {

constexpr int kAaThreads = 256;
constexpr int kAaWaveBuf = 512;                                   // kept values a wave collects in LDS between two flushes
constexpr int kAaBufBytes = kAaThreads / 64 * kAaWaveBuf * 8;     // ... of the four waves: 16 KiB
constexpr int kAaTabBytes = (int)sizeof(AaTables);                // 384
constexpr int kAaFixedBytes = kAaBufBytes + 16 + kAaTabBytes;     // buffers | two counts | tables
static_assert(kAaFixedBytes % 16 == 0, "the staged bytes start on a 16-byte border");

// (x - 0x01010101) & ~x has bit 7 of a byte set if a byte of x is 0 (and only then, taken over the whole word)
__device__ __forceinline__ uint32_t zero_bits(uint32_t x) { return (x - 0x01010101u) & ~x; }

// MurmurHash3_x64_128, first word, of the ksize bytes that start in d[0]'s lowest byte.  BLOCKS whole 16-byte blocks (0 .. 4),
// then TAIL = 0 nothing, 1 a k1 word of 1 .. 8 bytes, 2 a full k1 word and a k2 word of 1 .. 7 bytes; last_mask keeps the
// tail's last word's bytes.  has_zero: one of the ksize bytes is 0.
template <int BLOCKS, int TAIL>
__device__ __forceinline__ uint64_t murmur_bytes(const uint32_t* d, int ksize, uint32_t seed, uint64_t last_mask, bool& has_zero) {
    constexpr int kWords = 2 * BLOCKS + TAIL;
    uint64_t w[kWords > 0 ? kWords : 1];
    uint32_t z = 0;
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
        w[j] = (uint64_t)d[2 * j] | ((uint64_t)d[2 * j + 1] << 32);
        if (TAIL != 0 && j == kWords - 1) {
            w[j] &= last_mask;
            const uint64_t filled = w[j] | ~last_mask;
            z |= zero_bits((uint32_t)filled) | zero_bits((uint32_t)(filled >> 32));
        } else {
            z |= zero_bits(d[2 * j]) | zero_bits(d[2 * j + 1]);
        }
    }
    has_zero = (z & 0x80808080u) != 0;
    uint64_t h1 = seed, h2 = seed;
#pragma unroll
    for (int b = 0; b < BLOCKS; ++b) murmur_block(h1, h2, w[2 * b], w[2 * b + 1]);
    if (TAIL == 2) h2 ^= mur_k2(w[2 * BLOCKS + 1]);
    if (TAIL != 0) h1 ^= mur_k1(w[2 * BLOCKS]);
    h1 ^= (uint64_t)ksize;
    h2 ^= (uint64_t)ksize;
    h1 += h2;
    h2 += h1;
    h1 = fmix64(h1);
    h2 = fmix64(h2);
    return h1 + h2;
}

// counters: [0] cursor of the staging list = kept values; sample_counts / sample_valid: kept values / hashed k-mers per sample.
// plane_cap: bytes of LDS per plane (aa_plane_bytes of the launch's unit), raw_cap: of the staged bytes.
template <int BLOCKS, int TAIL, bool TRANSLATE>
__global__ __launch_bounds__(kAaThreads) void k_aa_hash(const uint8_t* __restrict__ bytes, long long total_bytes,
                                                        const KmerUnit* __restrict__ units, int ksize, uint32_t seed, uint64_t max_hash,
                                                        const AaTables tables, int raw_cap, int plane_cap,
                                                        unsigned long long* __restrict__ out_vals, int32_t* __restrict__ out_sample,
                                                        unsigned long long cap, unsigned long long* __restrict__ counters,
                                                        unsigned long long* __restrict__ sample_counts,
                                                        unsigned long long* __restrict__ sample_valid) {
    constexpr int NF = TRANSLATE ? 3 : 1;             // reading frames
    constexpr int NS = TRANSLATE ? 2 : 1;             // strands
    constexpr int kDwords = 4 * BLOCKS + 2 * TAIL;    // dwords the hash reads
    // LDS: the waves' buffers of kept values | the workgroup's two counts | the tables | the unit's bytes | the planes
    extern __shared__ __attribute__((aligned(16))) uint8_t aa_shared[];
    unsigned long long* wbuf = (unsigned long long*)aa_shared + (threadIdx.x >> 6) * kAaWaveBuf;
    unsigned int* wg_counts = (unsigned int*)(aa_shared + kAaBufBytes);
    uint8_t* tab = aa_shared + kAaBufBytes + 16;
    uint8_t* raw = aa_shared + kAaFixedBytes;
    uint8_t* planes = raw + raw_cap;
    const KmerUnit u = units[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63;
    if (t < 2) wg_counts[t] = 0;
    for (int i = t; i < kAaTabBytes; i += kAaThreads) tab[i] = ((const uint8_t*)&tables)[i];
    const int npos = u.npos;
    const int window = TRANSLATE ? 3 * ksize : ksize;
    const int nbytes = npos + window - 1;

    // 1. the unit's bytes [byte0, byte0 + nbytes) of the buffer, staged so that byte j lies at raw[sh + j]
    const uint8_t* g0 = bytes + u.byte0;
    const int sh = (int)((uintptr_t)g0 & 15);
    const uint8_t* a0 = g0 - sh;
    const uint8_t* lo = bytes;
    const uint8_t* hi = bytes + total_bytes;
    const int chunks = (sh + nbytes + 15) >> 4;
    for (int c = t; c < chunks; c += kAaThreads) {
        const uint8_t* a = a0 + 16 * (long long)c;
        if (a >= lo && a + 16 <= hi) {
            *(uint4*)(raw + 16 * c) = *(const uint4*)a;
        } else {
            for (int b = 0; b < 16; ++b) raw[16 * c + b] = (a + b >= lo && a + b < hi) ? a[b] : (uint8_t)0;
        }
    }
    __syncthreads();

    // 2. the planes: four consecutive residues of one frame per thread and step.  The reads run up to 11 bytes behind the
    //    unit's last byte (raw_cap has room); what they make there no window of the unit reads.
    const uint8_t* bmap = tab;
    const uint8_t* fw_tab = tab + 256;
    const uint8_t* rv_tab = tab + 320;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int nwin = (npos + NF - 1 - f) / NF;                 // windows of this frame
        const int m4 = nwin > 0 ? (nwin + ksize - 1 + 3) & ~3 : 0; // its residues, rounded up to 4
        uint32_t* fplane = (uint32_t*)(planes + (size_t)(NS * f) * plane_cap);
        uint32_t* rplane = (uint32_t*)(planes + (size_t)(NS * f + 1) * plane_cap);
        for (int q = t; q < m4 / 4; q += kAaThreads) {
            const uint8_t* src = raw + sh + (TRANSLATE ? 12 * q + f : 4 * q);
            if (TRANSLATE) {
                uint32_t c[14];
#pragma unroll
                for (int i = 0; i < 14; ++i) c[i] = bmap[src[i]];
                uint32_t fw = 0, rv = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t x = c[3 * j], y = c[3 * j + 1], z = c[3 * j + 2];
                    const bool bad = ((x | y | z) & 0x80u) != 0;
                    const uint32_t idx = (16 * x + 4 * y + z) & 63u;
                    const uint32_t a = bad ? 0u : (uint32_t)fw_tab[idx];
                    const uint32_t b = bad ? 0u : (uint32_t)rv_tab[idx];
                    fw |= a << (8 * j);
                    rv |= b << (8 * (3 - j));
                }
                fplane[q] = fw;
                rplane[m4 / 4 - 1 - q] = rv;
            } else {
                uint32_t fw = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) fw |= (uint32_t)bmap[src[j]] << (8 * j);
                fplane[q] = fw;
            }
        }
    }
    __syncthreads();

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

    // 3. one frame and strand per pass; the lanes of a wave take consecutive windows of the frame
    const uint64_t last_mask = (ksize & 7) ? ((1ULL << (8 * (ksize & 7))) - 1) : ~0ULL;
    unsigned int wave_kept = 0, wave_valid = 0, fill = 0;   // uniform over the wave: sums of ballots
    for (int pass = 0; pass < NF * NS; ++pass) {
        const int f = pass / NS;
        const bool reverse = (pass % NS) != 0;
        const int nwin = (npos + NF - 1 - f) / NF;
        const int m4 = nwin > 0 ? (nwin + ksize - 1 + 3) & ~3 : 0;
        const uint32_t* plane = (const uint32_t*)(planes + (size_t)pass * plane_cap);
        for (int m = t; (m & ~63) < nwin; m += kAaThreads) {    // the bound is uniform over the wave
            const bool inside = m < nwin;
            const int mm = inside ? m : nwin - 1;
            const int at = reverse ? m4 - mm - ksize : mm;        // the window's first byte in the plane
            const uint32_t* p = plane + (at >> 2);
            uint32_t ld[kDwords + 1], d[kDwords];
#pragma unroll
            for (int i = 0; i <= kDwords; ++i) ld[i] = p[i];
#pragma unroll
            for (int i = 0; i < kDwords; ++i) d[i] = __builtin_amdgcn_alignbyte(ld[i + 1], ld[i], (uint32_t)(at & 3));
            bool has_zero;
            const uint64_t h = murmur_bytes<BLOCKS, TAIL>(d, ksize, seed, last_mask, has_zero);
            const bool valid = inside && !has_zero;
            const bool keep = valid && h <= max_hash;
            // 4. the kept values to the wave's buffer, in lane order
            const unsigned long long vm = __ballot(valid);
            const unsigned long long km = __ballot(keep);
            wave_valid += (unsigned int)__popcll(vm);
            if (km) {
                const unsigned int n = (unsigned int)__popcll(km);
                if (fill + n > (unsigned int)kAaWaveBuf) {
                    flush(fill);
                    fill = 0;
                }
                if (keep) wbuf[fill + (unsigned int)__popcll(km & ((1ULL << lane) - 1))] = h;
                fill += n;
                wave_kept += n;
            }
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

using AaKernel = void (*)(const uint8_t*, long long, const KmerUnit*, int, uint32_t, uint64_t, const AaTables, int, int, unsigned long long*,
                          int32_t*, unsigned long long, unsigned long long*, unsigned long long*, unsigned long long*);

template <bool TRANSLATE>
AaKernel aa_kernel(int blocks, int tail) {
    switch (3 * blocks + tail) {
        case 1: return k_aa_hash<0, 1, TRANSLATE>;
        case 2: return k_aa_hash<0, 2, TRANSLATE>;
        case 3: return k_aa_hash<1, 0, TRANSLATE>;
        case 4: return k_aa_hash<1, 1, TRANSLATE>;
        case 5: return k_aa_hash<1, 2, TRANSLATE>;
        case 6: return k_aa_hash<2, 0, TRANSLATE>;
        case 7: return k_aa_hash<2, 1, TRANSLATE>;
        case 8: return k_aa_hash<2, 2, TRANSLATE>;
        case 9: return k_aa_hash<3, 0, TRANSLATE>;
        case 10: return k_aa_hash<3, 1, TRANSLATE>;
        case 11: return k_aa_hash<3, 2, TRANSLATE>;
        case 12: return k_aa_hash<4, 0, TRANSLATE>;
        default: return nullptr;
    }
}

int aa_raw_bytes(int unit, int ksize, bool translate) {
    const int window = translate ? 3 * ksize : ksize;
    return ((unit + window - 1 + 15 + 15) & ~15) + 32;
}
int aa_plane_bytes(int unit, int ksize, bool translate) {
    const int residues = (translate ? (unit + 2) / 3 : unit) + ksize - 1;
    return ((residues + 3 + 15) & ~15) + 16;
}

}  // namespace

int aa_unit_max(bool translate) { return translate ? kAaUnitTranslate : kAaUnitProtein; }

size_t aa_lds_bytes(int unit, int ksize, bool translate) {
    return (size_t)kAaFixedBytes + (size_t)aa_raw_bytes(unit, ksize, translate) +
           (size_t)(translate ? 6 : 1) * (size_t)aa_plane_bytes(unit, ksize, translate);
}

// the tables of the classification pass: the alphabet is applied here and nowhere else on the device
int aa_fill_tables(bool translate, int alphabet, AaTables* out) {
    if (alphabet < 0 || alphabet > 2) return MVS_E_RANGE;
    static const char* const kLetters = "ACDEFGHIKLMNPQRSTVWY";
    static const char* const kDayhoff = "baccfbdedeecbcdbbeff";   // aligned with kLetters
    static const char* const kHp = "hppphhphphhphpppphhh";
    uint8_t enc[256];
    std::memset(enc, 0, sizeof(enc));
    for (int i = 0; i < 20; ++i) {
        const uint8_t L = (uint8_t)kLetters[i];
        uint8_t e = L;
        if (alphabet == 1) e = (uint8_t)kDayhoff[i];
        if (alphabet == 2) e = (uint8_t)kHp[i];
        enc[L] = e;
        enc[L | 0x20] = e;
    }
    enc[(uint8_t)'*'] = (uint8_t)'*';
    std::memset(out, 0, sizeof(*out));
    if (!translate) {
        std::memcpy(out->byte_map, enc, 256);
        return 0;
    }
    std::memset(out->byte_map, 0x80, 256);
    const char* bases = "TCAG";
    for (int i = 0; i < 4; ++i) {
        out->byte_map[(uint8_t)bases[i]] = (uint8_t)i;
        out->byte_map[(uint8_t)bases[i] | 0x20] = (uint8_t)i;
    }
    static const char* const kCode = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
    for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y)
            for (int z = 0; z < 4; ++z) {
                out->codon_fw[16 * x + 4 * y + z] = enc[(uint8_t)kCode[16 * x + 4 * y + z]];
                // the reverse complement of xyz: the complements (T <-> A, C <-> G: code ^ 2) in reverse order
                out->codon_rv[16 * x + 4 * y + z] = enc[(uint8_t)kCode[16 * (z ^ 2) + 4 * (y ^ 2) + (x ^ 2)]];
            }
    return 0;
}

int launch_aa_hash(hipStream_t stream, const uint8_t* d_bytes, long long total_bytes, const KmerUnit* d_units, long long n_units, int unit,
                   bool translate, const AaTables& tables, int ksize, uint32_t seed, uint64_t max_hash, unsigned long long* d_vals,
                   int32_t* d_sample, unsigned long long cap, unsigned long long* d_counters, unsigned long long* d_sample_counts,
                   unsigned long long* d_sample_valid) {
    if (n_units <= 0) return 0;
    if (n_units >= (1LL << 31) || unit < 1 || unit > aa_unit_max(translate) || ksize < 1 || ksize > 64) return MVS_E_RANGE;
    // the shape of the hash's input picks the instantiation
    const int blocks = ksize / 16, rem = ksize % 16, tail = rem == 0 ? 0 : rem <= 8 ? 1 : 2;
    const AaKernel kernel = translate ? aa_kernel<true>(blocks, tail) : aa_kernel<false>(blocks, tail);
    if (!kernel) return MVS_E_RANGE;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_units), dim3(kAaThreads), aa_lds_bytes(unit, ksize, translate), stream, d_bytes, total_bytes,
                       d_units, ksize, seed, max_hash, tables, aa_raw_bytes(unit, ksize, translate), aa_plane_bytes(unit, ksize, translate),
                       d_vals, d_sample, cap, d_counters, d_sample_counts, d_sample_valid);
    return 0;
}

}  // namespace mvs
