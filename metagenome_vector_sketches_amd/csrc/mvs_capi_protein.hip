// mvs_capi_protein.hip -- C ABI of the protein sketches: mvs_translate_codon and mvs_aa_hash (pure host: the library's own
// statement of the contract, written without a table or a function of the kernel's), mvs_hash_set_from_residues (residues, or
// DNA in six frames -> a resident hash set) and mvs_ctx_aa_stats.  The kernel is in mvs_protein.hip; the units of work, the
// staging list, the scatter and the set are hash_set_from_bytes' (mvs_capi_kmer.hip), as for mvs_hash_set_from_sequences.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

using namespace mvs_capi;

namespace {

inline uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t fmix(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    return k ^ (k >> 33);
}
// MurmurHash3_x64_128 (Appleby, public domain), first word, byte by byte as the original reads its tail
uint64_t murmur3_first_word(const uint8_t* data, int len, uint32_t seed) {
    const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
    uint64_t h1 = seed, h2 = seed;
    int at = 0;
    for (; at + 16 <= len; at += 16) {
        uint64_t k1 = 0, k2 = 0;
        for (int i = 7; i >= 0; --i) {
            k1 = (k1 << 8) | data[at + i];
            k2 = (k2 << 8) | data[at + 8 + i];
        }
        k1 *= c1; k1 = rotl(k1, 31); k1 *= c2; h1 ^= k1;
        h1 = rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        k2 *= c2; k2 = rotl(k2, 33); k2 *= c1; h2 ^= k2;
        h2 = rotl(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    }
    uint64_t k1 = 0, k2 = 0;
    for (int i = len - 1; i >= at; --i) {
        if (i - at >= 8) k2 = (k2 << 8) | data[i];
        else k1 = (k1 << 8) | data[i];
    }
    if (len - at > 8) { k2 *= c2; k2 = rotl(k2, 33); k2 *= c1; h2 ^= k2; }
    if (len - at > 0) { k1 *= c1; k1 = rotl(k1, 31); k1 *= c2; h1 ^= k1; }
    h1 ^= (uint64_t)len; h2 ^= (uint64_t)len;
    h1 += h2; h2 += h1;
    h1 = fmix(h1); h2 = fmix(h2);
    return h1 + h2;
}

// the byte the hash reads for one residue byte in `alphabet`, or 0 for a break
uint8_t encode_residue(uint8_t b, int alphabet) {
    if (b == '*') return '*';
    if (b >= 'a' && b <= 'z') b = (uint8_t)(b - 'a' + 'A');
    if (!std::strchr("ACDEFGHIKLMNPQRSTVWY", (int)b) || b == 0) return 0;
    switch (alphabet) {
        case MVS_AA_PROTEIN: return b;
        case MVS_AA_DAYHOFF:
            if (b == 'C') return 'a';
            if (std::strchr("AGPST", b)) return 'b';
            if (std::strchr("DENQ", b)) return 'c';
            if (std::strchr("HKR", b)) return 'd';
            if (std::strchr("ILMV", b)) return 'e';
            return 'f';                                  // F W Y
        default: return std::strchr("AFGILMPVWY", b) ? 'h' : 'p';
    }
}

// T C A G in either case -> 0 1 2 3, else -1
int tcag(char b) {
    switch (b) {
        case 'T': case 't': return 0;
        case 'C': case 'c': return 1;
        case 'A': case 'a': return 2;
        case 'G': case 'g': return 3;
        default: return -1;
    }
}

bool alphabet_ok(int a) { return a == MVS_AA_PROTEIN || a == MVS_AA_DAYHOFF || a == MVS_AA_HP; }

}  // namespace

extern "C" {

int mvs_translate_codon(const char* codon3, char* aa, int* valid) {
    if (!codon3 || !aa || !valid) return fail(MVS_E_INVALID, "NULL argument");
    *aa = 0;
    *valid = 0;
    const int x = tcag(codon3[0]), y = tcag(codon3[1]), z = tcag(codon3[2]);
    if (x < 0 || y < 0 || z < 0) return MVS_OK;
    *aa = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"[16 * x + 4 * y + z];
    *valid = 1;
    return MVS_OK;
}

int mvs_aa_hash(const char* kmer, int ksize, int alphabet, uint32_t seed, uint64_t* h, int* valid) {
    if (!kmer || !h || !valid) return fail(MVS_E_INVALID, "NULL argument");
    if (ksize < 1 || ksize > 64) return fail(MVS_E_INVALID, "ksize = %d outside 1 .. 64", ksize);
    if (!alphabet_ok(alphabet)) return fail(MVS_E_INVALID, "alphabet = %d is none of MVS_AA_PROTEIN, MVS_AA_DAYHOFF, MVS_AA_HP", alphabet);
    *h = 0;
    *valid = 0;
    uint8_t enc[64];
    for (int i = 0; i < ksize; ++i) {
        enc[i] = encode_residue((uint8_t)kmer[i], alphabet);
        if (!enc[i]) return MVS_OK;
    }
    *h = murmur3_first_word(enc, ksize, seed);
    *valid = 1;
    return MVS_OK;
}

int mvs_hash_set_from_residues(mvs_ctx* c, const uint8_t* bytes, int mem_bytes, const int64_t* offsets, int64_t n_samples, int input_kind,
                               int alphabet, int ksize, uint32_t seed, uint64_t max_hash, mvs_hash_set** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n_samples < 0) return fail(MVS_E_INVALID, "n_samples = %lld is negative", (long long)n_samples);
    if (n_samples >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n_samples too large for int32 sample indices");
    if (!mem_ok(mem_bytes)) return fail(MVS_E_INVALID, "bad argument");
    if (input_kind != MVS_SEQ_PROTEIN && input_kind != MVS_SEQ_TRANSLATE)
        return fail(MVS_E_INVALID, "input_kind = %d is neither MVS_SEQ_PROTEIN nor MVS_SEQ_TRANSLATE", input_kind);
    if (!alphabet_ok(alphabet)) return fail(MVS_E_INVALID, "alphabet = %d is none of MVS_AA_PROTEIN, MVS_AA_DAYHOFF, MVS_AA_HP", alphabet);
    if (ksize < 1 || ksize > 64) return fail(MVS_E_INVALID, "ksize = %d outside 1 .. 64", ksize);
    if (const int rc = check_sample_bytes(bytes, offsets, n_samples)) return rc;
    const bool translate = input_kind == MVS_SEQ_TRANSLATE;
    mvs::AaTables tables;
    if (mvs::aa_fill_tables(translate, alphabet, &tables)) return fail(MVS_E_INTERNAL, "no tables for alphabet %d", alphabet);
    const int unit = std::min(c->opt.kmer_unit, mvs::aa_unit_max(translate));   // the planes of residues cost LDS
    return hash_set_from_bytes(c, "mvs_hash_set_from_residues", "k_aa_hash", bytes, mem_bytes, offsets, n_samples, translate ? 3 * ksize : ksize,
                               translate ? 2 : 1, unit, max_hash, &c->aa,
                               [&](const uint8_t* d_bytes, long long total, const mvs::KmerUnit* d_units, long long n_units,
                                   unsigned long long* d_vals, int32_t* d_sample, unsigned long long cap, unsigned long long* d_counters,
                                   unsigned long long* d_sample_counts, unsigned long long* d_sample_valid) {
                                   return mvs::launch_aa_hash(c->stream, d_bytes, total, d_units, n_units, unit, translate, tables, ksize, seed,
                                                              max_hash, d_vals, d_sample, cap, d_counters, d_sample_counts, d_sample_valid);
                               },
                               out);
}

int mvs_ctx_aa_stats(const mvs_ctx* c, double* kernel_ms, int64_t* bytes, int64_t* kmers, int64_t* kept, int64_t* units,
                     int64_t* second_trips) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (kernel_ms) *kernel_ms = c->aa.kernel_ms;
    if (bytes) *bytes = c->aa.bases;
    if (kmers) *kmers = c->aa.kmers;
    if (kept) *kept = c->aa.kept;
    if (units) *units = c->aa.units;
    if (second_trips) *second_trips = c->aa.second_trips;
    return MVS_OK;
}

int mvs_ctx_aa_sample_stats(const mvs_ctx* c, int64_t n_samples, int64_t* kmers, int64_t* kept) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (n_samples != (int64_t)c->aa.sample_kept.size())
        return fail(MVS_E_INVALID, "n_samples = %lld, the last call had %lld samples", (long long)n_samples, (long long)c->aa.sample_kept.size());
    for (int64_t s = 0; s < n_samples; ++s) {
        if (kmers) kmers[s] = c->aa.sample_kmers[(size_t)s];
        if (kept) kept[s] = c->aa.sample_kept[(size_t)s];
    }
    return MVS_OK;
}

}  // extern "C"
