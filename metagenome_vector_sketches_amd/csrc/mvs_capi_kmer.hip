// mvs_capi_kmer.hip -- C ABI of the sketches from sequences: mvs_kmer_max_hash and mvs_kmer_hash (pure host: the library's own
// statement of the contract), mvs_hash_set_from_sequences (DNA bytes -> a resident hash set), mvs_hash_set_export /
// mvs_hash_set_device (what a set holds, for the host and for mvs_project_csr) and mvs_ctx_kmer_stats.  The kernels and the
// layout of the units of work are in mvs_kmer.hip; the per-sample sort and unique compaction are mvs_hash_set_create's.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

using namespace mvs_capi;

namespace {

inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    return k ^ (k >> 33);
}
// MurmurHash3_x64_128 (Appleby, public domain), first word
uint64_t murmur3_h1(const uint8_t* data, int len, uint32_t seed) {
    const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
    uint64_t h1 = seed, h2 = seed;
    const int nblocks = len / 16;
    auto word = [](const uint8_t* p, int n) {
        uint64_t w = 0;
        for (int i = 0; i < n; ++i) w |= (uint64_t)p[i] << (8 * i);
        return w;
    };
    for (int b = 0; b < nblocks; ++b) {
        uint64_t k1 = word(data + 16 * b, 8), k2 = word(data + 16 * b + 8, 8);
        k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
        h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
        h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    }
    const uint8_t* tail = data + 16 * nblocks;
    const int rem = len & 15;
    if (rem > 8) {
        uint64_t k2 = word(tail + 8, rem - 8);
        k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
    }
    if (rem > 0) {
        uint64_t k1 = word(tail, rem > 8 ? 8 : rem);
        k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
    }
    h1 ^= (uint64_t)len; h2 ^= (uint64_t)len;
    h1 += h2; h2 += h1;
    h1 = fmix64(h1); h2 = fmix64(h2);
    return h1 + h2;
}

// 0..3 for A C G T in either case, -1 for a break
inline int base_code(uint8_t b) {
    switch (b) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
    }
}

}  // namespace

namespace mvs_capi {

int check_sample_bytes(const uint8_t* bases, const int64_t* offsets, int64_t n) {
    if (n > 0 && !offsets) return fail(MVS_E_INVALID, "offsets is NULL");
    const int64_t base = n > 0 ? offsets[0] : 0;
    if (base < 0) return fail(MVS_E_INVALID, "offsets[0] = %lld is negative", (long long)base);
    for (int64_t s = 0; s < n; ++s)
        if (offsets[s + 1] < offsets[s]) return fail(MVS_E_INVALID, "offsets are not non-decreasing at sample %lld", (long long)s);
    const long long total_bytes = n > 0 ? (long long)(offsets[n] - base) : 0;
    if (total_bytes > 0 && !bases) return fail(MVS_E_INVALID, "bases is NULL");
    return MVS_OK;
}

int hash_set_from_bytes(mvs_ctx* c, const char* call, const char* kernel, const uint8_t* bases, int mem_bases, const int64_t* offsets,
                        int64_t n, int window, int per_window, int unit, uint64_t max_hash, SeqStats* st, const HashLauncher& launch,
                        mvs_hash_set** out) {
    // the units of work, in sample order
    const int U = unit;
    const int64_t base = n > 0 ? offsets[0] : 0;
    const long long total_bytes = n > 0 ? (long long)(offsets[n] - base) : 0;
    std::vector<mvs::KmerUnit> units;
    long long positions = 0;
    for (int64_t s = 0; s < n; ++s) {
        const long long npos = (long long)(offsets[s + 1] - offsets[s]) - window + 1;
        for (long long p0 = 0; p0 < npos; p0 += U) {
            units.push_back({(long long)(offsets[s] - base) + p0, (int32_t)s, (int32_t)std::min<long long>(U, npos - p0)});
        }
        if (npos > 0) positions += npos;
    }
    const long long n_units = (long long)units.size();
    if (n_units >= (1LL << 31)) return fail(MVS_E_RANGE, "%lld units of work: raise option kmer_unit", n_units);

    *st = SeqStats();
    st->bases = total_bytes;
    st->units = n_units;
    st->sample_kmers.assign((size_t)n, 0);
    st->sample_kept.assign((size_t)n, 0);
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, call);
    std::vector<int64_t> hoff((size_t)n + 1, 0);
    if (n_units == 0) return mvs_hash_set_create(c, nullptr, MVS_MEM_HOST, hoff.data(), n, out);

    DevBuf dbases, dunits, dcount, dvals, dsamp;
    const uint8_t* d_bases = bases + base;
    if (mem_bases == MVS_MEM_HOST) {
        if (dbases.alloc((size_t)total_bytes) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %lld bases failed", total_bytes);
        HIP_TRY(hipMemcpyAsync(dbases.p, bases + base, (size_t)total_bytes, hipMemcpyHostToDevice, c->stream));
        d_bases = (const uint8_t*)dbases.p;
    }
    // counters (32 bytes) | kept values per sample | valid positions per sample
    const size_t count_bytes = 32 + (size_t)n * 16;
    if (dunits.alloc((size_t)n_units * sizeof(mvs::KmerUnit)) != hipSuccess || dcount.alloc(count_bytes) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of %lld units failed", n_units);
    HIP_TRY(hipMemcpyAsync(dunits.p, units.data(), (size_t)n_units * sizeof(mvs::KmerUnit), hipMemcpyHostToDevice, c->stream));
    unsigned long long* d_counters = (unsigned long long*)dcount.p;
    unsigned long long* d_sample_counts = d_counters + 4;
    unsigned long long* d_sample_valid = d_sample_counts + n;

    // the staging list: the expected number of kept values and a margin, never more than the positions; or what the option says
    unsigned long long cap;
    if (c->opt.kmer_capacity > 0) {
        cap = (unsigned long long)c->opt.kmer_capacity;
    } else {
        const double frac = ((double)max_hash + 1.0) / 18446744073709551616.0;
        cap = (unsigned long long)((double)positions * (double)per_window * frac * 1.125) + 65536;
    }
    cap = std::min<unsigned long long>(cap, (unsigned long long)positions * (unsigned long long)per_window);

    unsigned long long back[1] = {0};
    for (int trip = 0;; ++trip) {
        dvals.reset();
        dsamp.reset();
        if (dvals.alloc((size_t)cap * 8) != hipSuccess || dsamp.alloc((size_t)cap * 4) != hipSuccess)
            return fail(MVS_E_NOMEM, "hipMalloc of a staging list of %llu values failed", cap);
        HIP_TRY(hipMemsetAsync(dcount.p, 0, count_bytes, c->stream));
        StageTimer tm;
        int rc = tm.begin(c);
        if (rc) return rc;
        rc = launch(d_bases, total_bytes, (const mvs::KmerUnit*)dunits.p, n_units, (unsigned long long*)dvals.p, (int32_t*)dsamp.p, cap,
                    d_counters, d_sample_counts, d_sample_valid);
        if (rc) return fail(rc, "%s: bad launch geometry", kernel);
        rc = check_kernel(kernel);
        if (rc) return rc;
        rc = tm.mark_end();
        if (rc) return rc;
        rc = read_back(c, c->stream, {{back, d_counters, sizeof(back)}});
        if (rc) return rc;
        rc = tm.add_to(&st->kernel_ms);
        if (rc) return rc;
        if (back[0] <= cap) break;
        if (trip > 0) return fail(MVS_E_HIP, "%s kept %llu values where its first trip kept %llu", kernel, back[0], cap);
        cap = back[0];                     // the exact size: the second trip cannot miss
        ++st->second_trips;
    }
    units.clear();
    units.shrink_to_fit();
    const long long kept = (long long)back[0];
    st->kept = kept;

    std::vector<unsigned long long> counts((size_t)n * 2);
    HIP_TRY(hipMemcpyAsync(counts.data(), d_sample_counts, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int64_t s = 0; s < n; ++s) {
        st->sample_kept[(size_t)s] = (long long)counts[(size_t)s];
        st->sample_kmers[(size_t)s] = (long long)counts[(size_t)(n + s)];
        st->kmers += (long long)counts[(size_t)(n + s)];
    }
    for (int64_t s = 0; s < n; ++s) {
        if (counts[(size_t)s] >= (1ULL << 31)) return fail(MVS_E_RANGE, "sample %lld keeps 2^31 hashes or more", (long long)s);
        hoff[(size_t)s + 1] = hoff[(size_t)s] + (int64_t)counts[(size_t)s];
    }
    if (hoff[(size_t)n] != kept) return fail(MVS_E_HIP, "%s: the samples' counts sum to %lld, the list holds %lld", kernel, (long long)hoff[(size_t)n], kept);

    DevBuf doff, dgrouped;
    if (doff.alloc(hoff.size() * 8) != hipSuccess || dgrouped.alloc((size_t)std::max<long long>(kept, 1) * 8) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of %lld kept hashes failed", kept);
    HIP_TRY(hipMemcpyAsync(doff.p, hoff.data(), hoff.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_sample_counts, 0, (size_t)n * 8, c->stream));   // now the samples' cursors
    {
        StageTimer tm;
        int rc = tm.begin(c);
        if (rc) return rc;
        rc = mvs::launch_kmer_scatter(c->stream, (const unsigned long long*)dvals.p, (const int32_t*)dsamp.p, kept, (const long long*)doff.p,
                                      d_sample_counts, (unsigned long long*)dgrouped.p);
        if (rc) return fail(rc, "k_kmer_scatter: bad launch geometry");
        rc = check_kernel("k_kmer_scatter");
        if (rc) return rc;
        rc = tm.mark_end();
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        rc = tm.add_to(&st->kernel_ms);
        if (rc) return rc;
    }
    dvals.reset();
    dsamp.reset();
    dbases.reset();
    // per-sample sort and unique compaction: the set is built from the grouped values where they lie
    return mvs_hash_set_create(c, (const uint64_t*)dgrouped.p, MVS_MEM_DEVICE, hoff.data(), n, out);
}

}  // namespace mvs_capi

extern "C" {

int mvs_kmer_max_hash(int64_t scaled, uint64_t* max_hash) {
    if (!max_hash) return fail(MVS_E_INVALID, "max_hash is NULL");
    if (scaled < 1) return fail(MVS_E_INVALID, "scaled = %lld is below 1", (long long)scaled);
    *max_hash = scaled == 1 ? ~0ULL : (uint64_t)(18446744073709551616.0 / (double)scaled);
    return MVS_OK;
}

int mvs_kmer_hash(const char* kmer, int ksize, uint32_t seed, uint64_t* h, int* valid) {
    if (!kmer || !h || !valid) return fail(MVS_E_INVALID, "NULL argument");
    if (ksize < 1 || ksize > 32) return fail(MVS_E_INVALID, "ksize = %d outside 1 .. 32", ksize);
    *h = 0;
    *valid = 0;
    uint8_t fw[32], rc[32];
    for (int i = 0; i < ksize; ++i) {
        const int code = base_code((uint8_t)kmer[i]);
        if (code < 0) return MVS_OK;
        fw[i] = (uint8_t)"ACGT"[code];
        rc[ksize - 1 - i] = (uint8_t)"ACGT"[3 - code];
    }
    *h = murmur3_h1(std::memcmp(fw, rc, (size_t)ksize) <= 0 ? fw : rc, ksize, seed);
    *valid = 1;
    return MVS_OK;
}

int mvs_hash_set_from_sequences(mvs_ctx* c, const uint8_t* bases, int mem_bases, const int64_t* offsets, int64_t n_samples, int ksize,
                                uint32_t seed, uint64_t max_hash, mvs_hash_set** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n_samples < 0) return fail(MVS_E_INVALID, "n_samples = %lld is negative", (long long)n_samples);
    if (n_samples >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n_samples too large for int32 sample indices");
    if (!mem_ok(mem_bases)) return fail(MVS_E_INVALID, "bad argument");
    if (ksize < 1 || ksize > 32) return fail(MVS_E_INVALID, "ksize = %d outside 1 .. 32", ksize);
    if (const int rc = check_sample_bytes(bases, offsets, n_samples)) return rc;
    return hash_set_from_bytes(c, "mvs_hash_set_from_sequences", "k_kmer_hash", bases, mem_bases, offsets, n_samples, ksize, 1, c->opt.kmer_unit,
                               max_hash, &c->km,
                               [&](const uint8_t* d_bases, long long total, const mvs::KmerUnit* d_units, long long n_units,
                                   unsigned long long* d_vals, int32_t* d_sample, unsigned long long cap, unsigned long long* d_counters,
                                   unsigned long long* d_sample_counts, unsigned long long* d_sample_valid) {
                                   return mvs::launch_kmer_hash(c->stream, d_bases, total, d_units, n_units, c->opt.kmer_unit, ksize, seed,
                                                                max_hash, d_vals, d_sample, cap, d_counters, d_sample_counts, d_sample_valid);
                               },
                               out);
}

int mvs_hash_set_export(const mvs_hash_set* h, uint64_t* hashes, int mem_out, int64_t* offsets) {
    if (!h) return fail(MVS_E_INVALID, "NULL hash set");
    if (!mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    mvs_ctx* c = h->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if (offsets) HIP_TRY(hipMemcpyAsync(offsets, h->offsets.p, ((size_t)h->n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (hashes && h->total > 0)
        HIP_TRY(hipMemcpyAsync(hashes, h->hashes.p, (size_t)h->total * 8,
                               mem_out == MVS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_hash_set_device(const mvs_hash_set* h, const uint64_t** d_hashes) {
    if (!h || !d_hashes) return fail(MVS_E_INVALID, "NULL argument");
    *d_hashes = h->hashes.as<const uint64_t>();
    return MVS_OK;
}

int mvs_ctx_kmer_stats(const mvs_ctx* c, double* kernel_ms, int64_t* bases, int64_t* kmers, int64_t* kept, int64_t* units,
                       int64_t* second_trips) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (kernel_ms) *kernel_ms = c->km.kernel_ms;
    if (bases) *bases = c->km.bases;
    if (kmers) *kmers = c->km.kmers;
    if (kept) *kept = c->km.kept;
    if (units) *units = c->km.units;
    if (second_trips) *second_trips = c->km.second_trips;
    return MVS_OK;
}

int mvs_ctx_kmer_sample_stats(const mvs_ctx* c, int64_t n_samples, int64_t* kmers, int64_t* kept) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (n_samples != (int64_t)c->km.sample_kept.size())
        return fail(MVS_E_INVALID, "n_samples = %lld, the last call had %lld samples", (long long)n_samples, (long long)c->km.sample_kept.size());
    for (int64_t s = 0; s < n_samples; ++s) {
        if (kmers) kmers[s] = c->km.sample_kmers[(size_t)s];
        if (kept) kept[s] = c->km.sample_kept[(size_t)s];
    }
    return MVS_OK;
}

}  // extern "C"
