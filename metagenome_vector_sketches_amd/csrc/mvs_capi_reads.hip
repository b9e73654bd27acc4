// mvs_capi_reads.hip -- C ABI of the abundances (include/mvs_hip.h "abundances"): the sketcher that takes a sample's bases over
// any number of calls (mvs_kmer_sketcher_*), the counted set build for arbitrary hash lists (mvs_hash_set_create_counted), what
// such a set carries (mvs_hash_set_abundances) and mvs_ctx_abund_stats.  The hashing kernel and the scatter are mvs_kmer.hip's,
// unchanged; the sort and the run-sum passes are in mvs_abund.hip.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

using namespace mvs_capi;

struct mvs_kmer_sketcher {
    mvs_ctx* ctx = nullptr;
    int64_t n = 0;
    int ksize = 0;
    uint32_t seed = 0;
    uint64_t max_hash = 0;
    bool finished = false, broken = false;
    // the staging list of (value, sample) pairs: `len` of `cap` entries are filled
    DevBuf vals;   // unsigned long long
    DevBuf samp;   // int32_t
    long long cap = 0, len = 0;
    // what the adds did (mvs_kmer_sketcher_info): hashing time (timing enabled), second trips, times the list grew
    double hash_ms = 0.0;
    long long second_trips = 0, growths = 0, adds = 0;
    std::vector<long long> bases, kmers, kept, distinct, passed;   // per sample
};

namespace {

constexpr int64_t kSortBatch = 1LL << 30;   // keys per segmented sort (rocprim counts them in 32 bits)

struct SetGuard {
    mvs_hash_set* h;
    ~SetGuard() {
        if (h) mvs_hash_set_destroy(h);
    }
};

int filter_checks(uint32_t min_abundance, uint32_t max_abundance) {
    if (min_abundance == 0) return fail(MVS_E_INVALID, "min_abundance = 0 is below 1");
    if (max_abundance > 0 && max_abundance < min_abundance)
        return fail(MVS_E_INVALID, "max_abundance = %u is below min_abundance = %u", max_abundance, min_abundance);
    return MVS_OK;
}

// The samples' values sorted inside every sample: short samples in batches through the segmented sort, each long one alone.
// Everything the sorts need -- their plan, the segments' offsets on the device, one scratch buffer that fits the hungriest of
// them -- is made BEFORE the timed stretch, which then holds the sorts' launches and nothing else.
int sort_samples(mvs_ctx* c, const unsigned long long* d_in, const uint32_t* d_w, const std::vector<long long>& off, int64_t n,
                 unsigned long long* d_out, uint32_t* d_wout) {
    struct Job {
        long long base;
        unsigned int count, segments;   // segments 0: one device-wide sort
        size_t seg_at;                  // where the batch's offsets start in `seg`
    };
    const long long big = c->opt.abund_big_segment;
    std::vector<Job> jobs;
    std::vector<unsigned int> seg;
    for (int64_t s = 0; s < n;) {
        const long long len = off[(size_t)s + 1] - off[(size_t)s];
        const long long base = off[(size_t)s];
        if (len > big) {
            jobs.push_back({base, (unsigned int)len, 0u, 0});
            ++c->ab_big;
            ++s;
            continue;
        }
        int64_t s1 = s;
        while (s1 < n && off[(size_t)s1 + 1] - off[(size_t)s1] <= big && off[(size_t)s1 + 1] - base <= kSortBatch && s1 - s < (1LL << 30)) ++s1;
        const unsigned int count = (unsigned int)(off[(size_t)s1] - base);
        if (count > 0) {
            jobs.push_back({base, count, (unsigned int)(s1 - s), seg.size()});
            for (int64_t i = s; i <= s1; ++i) seg.push_back((unsigned int)(off[(size_t)i] - base));
        }
        s = s1;
    }
    DevBuf tmp, dseg;
    if (dseg.alloc(seg.size() * 4) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %zu segment offsets failed", seg.size());
    if (!seg.empty()) HIP_TRY(hipMemcpyAsync(dseg.p, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, c->stream));
    auto run = [&](const Job& j, void* scratch, size_t bytes, size_t* need) {
        const uint32_t* win = d_w ? d_w + j.base : nullptr;
        uint32_t* wout = d_w ? d_wout + j.base : nullptr;
        const unsigned int* d_begin = (const unsigned int*)dseg.p + j.seg_at;
        return j.segments ? mvs::ab_sort_segments(c->stream, d_in + j.base, d_out + j.base, win, wout, j.count, j.segments, d_begin, d_begin + 1,
                                                  scratch, bytes, need)
                          : mvs::ab_sort_whole(c->stream, d_in + j.base, d_out + j.base, win, wout, j.count, scratch, bytes, need);
    };
    size_t most = 0;
    for (const Job& j : jobs) {
        size_t need = 0;
        if (const int rc = run(j, nullptr, 0, &need)) return fail(rc, "counted build: sort sizing failed");
        most = std::max(most, need);
    }
    if (tmp.alloc(most) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %zu bytes for the sort failed", most);
    StageTimer tm;
    int rc = tm.begin(c);
    if (rc) return rc;
    for (const Job& j : jobs)
        if ((rc = run(j, tmp.p, most, nullptr)) != 0) return fail(rc, "counted build: sort failed");
    rc = check_kernel("counted build: sort");
    if (rc) return rc;
    rc = tm.mark_end();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));           // (before the scratch and the offsets are freed)
    return tm.add_to(&c->ab_sort_ms);
}

// the staging list holds at least `want` entries; what it held is kept (a device copy into a list at least twice as long)
int sketcher_reserve(mvs_kmer_sketcher* k, long long want) {
    if (want <= k->cap) return MVS_OK;
    mvs_ctx* c = k->ctx;
    const long long cap = std::max(want, 2 * k->cap);
    DevBuf nv, ns;
    if (nv.alloc((size_t)cap * 8) != hipSuccess || ns.alloc((size_t)cap * 4) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of a staging list of %lld values failed", cap);
    hipError_t e = hipSuccess;
    if (k->len > 0) {
        e = hipMemcpyAsync(nv.p, k->vals.p, (size_t)k->len * 8, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ns.p, k->samp.p, (size_t)k->len * 4, hipMemcpyDeviceToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(MVS_E_HIP, "growing the staging list: %s", hipGetErrorString(e));
    if (k->cap > 0) ++k->growths;
    k->vals = std::move(nv);
    k->samp = std::move(ns);
    k->cap = cap;
    return MVS_OK;
}

}  // namespace

namespace mvs_capi {

int counted_build(mvs_ctx* c, const unsigned long long* d_in, const uint32_t* d_w, const std::vector<long long>& off, int64_t n,
                  uint32_t min_abundance, uint32_t max_abundance, int64_t* histogram, std::vector<long long>* distinct,
                  std::vector<long long>* passed, mvs_hash_set** out) {
    const long long total = off[(size_t)n];
    const int U = c->opt.abund_unit;
    const long long n_units = (total + U - 1) / U;
    c->ab_sort_ms = c->ab_count_ms = 0.0;
    c->ab_values = total;
    c->ab_distinct = c->ab_passed = c->ab_big = 0;
    c->ab_units = n_units;
    mvs_hash_set* h = new (std::nothrow) mvs_hash_set();
    if (!h) return fail(MVS_E_NOMEM, "out of host memory");
    SetGuard guard{h};
    h->ctx = c;
    h->n = n;
    DevBuf doff, ddist, dsorted, dsortedw, dborders, dwork, dhist;
    if (h->offsets.alloc(((size_t)n + 1) * 8) != hipSuccess || h->sizes.alloc((size_t)std::max<int64_t>(n, 1) * 4) != hipSuccess ||
        doff.alloc(((size_t)n + 1) * 8) != hipSuccess || ddist.alloc(((size_t)n + 1) * 8) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of the offsets of %lld samples failed", (long long)n);
    HIP_TRY(hipMemcpyAsync(doff.p, off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (histogram) {
        if (dhist.alloc((size_t)std::max<int64_t>(n, 1) * 256 * 8) != hipSuccess)
            return fail(MVS_E_NOMEM, "hipMalloc of the histogram of %lld samples failed", (long long)n);
        HIP_TRY(hipMemsetAsync(dhist.p, 0, (size_t)std::max<int64_t>(n, 1) * 256 * 8, c->stream));
    }

    mvs::AbArgs a{};
    a.off = (const long long*)doff.p;
    a.n = n;
    a.total = total;
    a.n_units = n_units;
    a.unit = U;
    a.min_ab = min_abundance;
    a.max_ab = max_abundance;
    a.hist = (unsigned long long*)dhist.p;
    long long totals[2] = {0, 0};
    if (total > 0) {
        if (dsorted.alloc((size_t)total * 8) != hipSuccess || (d_w && dsortedw.alloc((size_t)total * 4) != hipSuccess))
            return fail(MVS_E_NOMEM, "hipMalloc of %lld values for the sort failed", total);
        if (const int rc = sort_samples(c, d_in, d_w, off, n, (unsigned long long*)dsorted.p, (uint32_t*)dsortedw.p)) return rc;
        // work space: flags | summaries | tails | four arrays of n_units + 1 counts | the scans' scratch
        const size_t words = (size_t)((total + 31) / 32);
        const size_t carry_bytes = (size_t)n_units * sizeof(mvs::AbCarry), count_bytes = (((size_t)n_units + 1) * 8 + 15) & ~(size_t)15;
        const size_t scan_bytes = mvs::ab_work_bytes(n_units);
        if (dborders.alloc(words * 4) != hipSuccess || dwork.alloc(16 + 2 * carry_bytes + 4 * count_bytes + scan_bytes) != hipSuccess)
            return fail(MVS_E_NOMEM, "hipMalloc of the work space of %lld units failed", n_units);
        uint8_t* w = (uint8_t*)dwork.p;
        a.keys = (const unsigned long long*)dsorted.p;
        a.weights = d_w ? (const uint32_t*)dsortedw.p : nullptr;
        a.borders = (const unsigned int*)dborders.p;
        a.flags = (unsigned int*)w;
        a.summary = (mvs::AbCarry*)(w + 16);
        a.tails = (mvs::AbCarry*)(w + 16 + carry_bytes);
        a.head_counts = (long long*)(w + 16 + 2 * carry_bytes);
        a.pass_counts = (long long*)(w + 16 + 2 * carry_bytes + count_bytes);
        a.head_start = (long long*)(w + 16 + 2 * carry_bytes + 2 * count_bytes);
        a.pass_start = (long long*)(w + 16 + 2 * carry_bytes + 3 * count_bytes);
        void* scan_scratch = w + 16 + 2 * carry_bytes + 4 * count_bytes;
        HIP_TRY(hipMemsetAsync(dborders.p, 0, words * 4, c->stream));
        HIP_TRY(hipMemsetAsync(a.flags, 0, 16, c->stream));
        HIP_TRY(hipMemsetAsync(a.head_counts, 0, 2 * count_bytes, c->stream));
        StageTimer tm;
        int rc = tm.begin(c);
        if (rc) return rc;
        rc = mvs::launch_ab_borders(c->stream, a.off, n, total, (unsigned int*)dborders.p);
        if (!rc) rc = mvs::ab_count(c->stream, a, scan_scratch, scan_bytes);
        if (rc) return fail(rc, "counted build: the run-sum passes were refused");
        rc = check_kernel("k_ab_count");
        if (rc) return rc;
        rc = tm.mark_end();                 // passes A to C and the scans; the read-back and the allocations below are not timed
        if (rc) return rc;
        unsigned int flag = 0;
        rc = read_back(c, c->stream, {{&flag, a.flags, 4}, {&totals[0], a.head_start + n_units, 8}, {&totals[1], a.pass_start + n_units, 8}});
        if (rc) return rc;
        rc = tm.add_to(&c->ab_count_ms);
        if (rc) return rc;
        if (flag) return fail(MVS_E_RANGE, "the abundance of a value reaches 2^32");
        if (h->hashes.alloc((size_t)std::max<long long>(totals[1], 1) * 8) != hipSuccess ||
            h->abund.alloc((size_t)std::max<long long>(totals[1], 1) * 4) != hipSuccess)
            return fail(MVS_E_NOMEM, "hipMalloc of %lld values and abundances failed", totals[1]);
        StageTimer tf;                      // pass D
        rc = tf.begin(c);
        if (rc) return rc;
        rc = mvs::ab_fill(c->stream, a, h->hashes.as<unsigned long long>(), h->abund.as<uint32_t>(), h->offsets.as<long long>(),
                          (long long*)ddist.p, h->sizes.as<int32_t>());
        if (!rc) rc = check_kernel("k_ab_fill");
        if (rc) return rc;
        rc = tf.mark_end();
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        rc = tf.add_to(&c->ab_count_ms);
        if (rc) return rc;
    } else {
        if (h->hashes.alloc(8) != hipSuccess || h->abund.alloc(4) != hipSuccess)
            return fail(MVS_E_NOMEM, "hipMalloc of an empty set failed");
        int rc = mvs::ab_fill(c->stream, a, h->hashes.as<unsigned long long>(), h->abund.as<uint32_t>(), h->offsets.as<long long>(),
                          (long long*)ddist.p, h->sizes.as<int32_t>());
        if (!rc) rc = check_kernel("k_ab_tail");
        if (rc) return rc;
    }
    h->total = totals[1];
    c->ab_distinct = totals[0];
    c->ab_passed = totals[1];
    if (distinct || passed) {
        std::vector<long long> d((size_t)n + 1), p((size_t)n + 1);
        HIP_TRY(hipMemcpyAsync(d.data(), ddist.p, d.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(p.data(), h->offsets.p, p.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (distinct) distinct->resize((size_t)n);
        if (passed) passed->resize((size_t)n);
        for (int64_t s = 0; s < n; ++s) {
            if (distinct) (*distinct)[(size_t)s] = d[(size_t)s + 1] - d[(size_t)s];
            if (passed) (*passed)[(size_t)s] = p[(size_t)s + 1] - p[(size_t)s];
        }
    }
    if (histogram && n > 0) HIP_TRY(hipMemcpyAsync(histogram, dhist.p, (size_t)n * 256 * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    guard.h = nullptr;
    *out = h;
    return MVS_OK;
}

}  // namespace mvs_capi

extern "C" {

int mvs_hash_set_create_counted(mvs_ctx* c, const uint64_t* hashes, int mem_hashes, const uint32_t* weights, int mem_weights,
                                const int64_t* offsets, int64_t n_samples, uint32_t min_abundance, uint32_t max_abundance,
                                int64_t* histogram, mvs_hash_set** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n_samples < 0) return fail(MVS_E_INVALID, "n_samples = %lld is negative", (long long)n_samples);
    if (n_samples >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n_samples too large for int32 sample indices");
    if (!mem_ok(mem_hashes) || (weights && !mem_ok(mem_weights))) return fail(MVS_E_INVALID, "bad argument");
    if (n_samples > 0 && !offsets) return fail(MVS_E_INVALID, "offsets is NULL");
    if (const int rc = filter_checks(min_abundance, max_abundance)) return rc;
    const int64_t n = n_samples;
    std::vector<long long> off((size_t)n + 1, 0);
    const int64_t base = n > 0 ? offsets[0] : 0;
    if (base < 0) return fail(MVS_E_INVALID, "offsets[0] = %lld is negative", (long long)base);
    for (int64_t s = 0; s < n; ++s) {
        const int64_t len = offsets[s + 1] - offsets[s];
        if (len < 0) return fail(MVS_E_INVALID, "offsets are not non-decreasing at sample %lld", (long long)s);
        if (len >= (1LL << 31)) return fail(MVS_E_RANGE, "sample %lld holds 2^31 hashes or more", (long long)s);
        off[(size_t)s + 1] = offsets[s + 1] - base;
    }
    const long long total = off[(size_t)n];
    if (total > 0 && !hashes) return fail(MVS_E_INVALID, "hashes is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_hash_set_create_counted");
    DevBuf dh, dw;
    const unsigned long long* d_in = (const unsigned long long*)hashes + base;
    const uint32_t* d_w = weights ? weights + base : nullptr;
    if (total > 0 && mem_hashes == MVS_MEM_HOST) {
        if (dh.alloc((size_t)total * 8) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %lld hashes failed", total);
        HIP_TRY(hipMemcpyAsync(dh.p, hashes + base, (size_t)total * 8, hipMemcpyHostToDevice, c->stream));
        d_in = (const unsigned long long*)dh.p;
    }
    if (total > 0 && weights && mem_weights == MVS_MEM_HOST) {
        if (dw.alloc((size_t)total * 4) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %lld weights failed", total);
        HIP_TRY(hipMemcpyAsync(dw.p, weights + base, (size_t)total * 4, hipMemcpyHostToDevice, c->stream));
        d_w = (const uint32_t*)dw.p;
    }
    const int rc = counted_build(c, d_in, d_w, off, n, min_abundance, max_abundance, histogram, nullptr, nullptr, out);
    (void)hipStreamSynchronize(c->stream);   // (the uploads' buffers are freed behind this)
    return rc;
}

int mvs_hash_set_abundances(const mvs_hash_set* h, uint32_t* out, int mem_out) {
    if (!h) return fail(MVS_E_INVALID, "NULL hash set");
    if (!mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (!h->abund.p) return fail(MVS_E_INVALID, "the hash set carries no abundances");
    if (h->total == 0) return MVS_OK;
    if (!out) return fail(MVS_E_INVALID, "out is NULL");
    mvs_ctx* c = h->ctx;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, h->abund.p, (size_t)h->total * 4, mem_out == MVS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_ctx_abund_stats(const mvs_ctx* c, double* sort_ms, double* count_ms, int64_t* values_in, int64_t* distinct, int64_t* passed,
                        int64_t* units, int64_t* big_segments) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (sort_ms) *sort_ms = c->ab_sort_ms;
    if (count_ms) *count_ms = c->ab_count_ms;
    if (values_in) *values_in = c->ab_values;
    if (distinct) *distinct = c->ab_distinct;
    if (passed) *passed = c->ab_passed;
    if (units) *units = c->ab_units;
    if (big_segments) *big_segments = c->ab_big;
    return MVS_OK;
}

int mvs_kmer_sketcher_create(mvs_ctx* c, int64_t n_samples, int ksize, uint32_t seed, uint64_t max_hash, mvs_kmer_sketcher** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n_samples < 0) return fail(MVS_E_INVALID, "n_samples = %lld is negative", (long long)n_samples);
    if (n_samples >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n_samples too large for int32 sample indices");
    if (ksize < 1 || ksize > 32) return fail(MVS_E_INVALID, "ksize = %d outside 1 .. 32", ksize);
    mvs_kmer_sketcher* k = new (std::nothrow) mvs_kmer_sketcher();
    if (!k) return fail(MVS_E_NOMEM, "out of host memory");
    k->ctx = c;
    k->n = n_samples;
    k->ksize = ksize;
    k->seed = seed;
    k->max_hash = max_hash;
    k->bases.assign((size_t)n_samples, 0);
    k->kmers.assign((size_t)n_samples, 0);
    k->kept.assign((size_t)n_samples, 0);
    k->distinct.assign((size_t)n_samples, 0);
    k->passed.assign((size_t)n_samples, 0);
    *out = k;
    return MVS_OK;
}

int mvs_kmer_sketcher_add(mvs_kmer_sketcher* k, const uint8_t* bases, int mem_bases, const int64_t* offsets, const int32_t* samples,
                          int64_t n_pieces) {
    if (!k) return fail(MVS_E_INVALID, "NULL sketcher");
    if (k->finished) return fail(MVS_E_INVALID, "the sketcher is finished");
    if (k->broken) return fail(MVS_E_INVALID, "an earlier add failed: the sketcher can only be destroyed");
    if (!mem_ok(mem_bases)) return fail(MVS_E_INVALID, "bad argument");
    if (n_pieces < 0) return fail(MVS_E_INVALID, "n_pieces = %lld is negative", (long long)n_pieces);
    if (n_pieces == 0) return MVS_OK;
    if (!offsets || !samples) return fail(MVS_E_INVALID, "offsets or samples is NULL");
    const int64_t base = offsets[0];
    if (base < 0) return fail(MVS_E_INVALID, "offsets[0] = %lld is negative", (long long)base);
    for (int64_t i = 0; i < n_pieces; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(MVS_E_INVALID, "offsets are not non-decreasing at piece %lld", (long long)i);
        if (samples[i] < 0 || samples[i] >= k->n)
            return fail(MVS_E_RANGE, "piece %lld names sample %d, the sketcher holds %lld", (long long)i, samples[i], (long long)k->n);
    }
    const long long total_bytes = (long long)(offsets[n_pieces] - base);
    if (total_bytes == 0) return MVS_OK;
    if (!bases) return fail(MVS_E_INVALID, "bases is NULL");
    mvs_ctx* c = k->ctx;
    const int64_t n = k->n;
    const int ksize = k->ksize;

    // the units of work, laid out per piece exactly as mvs_hash_set_from_sequences lays out a sample
    const int U = c->opt.kmer_unit;
    std::vector<mvs::KmerUnit> units;
    long long positions = 0;
    for (int64_t i = 0; i < n_pieces; ++i) {
        const long long npos = (long long)(offsets[i + 1] - offsets[i]) - ksize + 1;
        for (long long p0 = 0; p0 < npos; p0 += U)
            units.push_back({(long long)(offsets[i] - base) + p0, samples[i], (int32_t)std::min<long long>(U, npos - p0)});
        if (npos > 0) positions += npos;
    }
    const long long n_units = (long long)units.size();
    if (n_units >= (1LL << 31)) return fail(MVS_E_RANGE, "%lld units of work: raise option kmer_unit", n_units);
    if (n_units == 0) {
        for (int64_t i = 0; i < n_pieces; ++i) k->bases[(size_t)samples[i]] += offsets[i + 1] - offsets[i];
        return MVS_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_kmer_sketcher_add");
    DevBuf dbases, dunits, dcount;
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

    // room behind the staged pairs for this call's: the expected number and a margin, or what the option says
    unsigned long long room;
    if (c->opt.kmer_capacity > 0) {
        room = (unsigned long long)c->opt.kmer_capacity;
    } else {
        const double frac = ((double)k->max_hash + 1.0) / 18446744073709551616.0;
        room = (unsigned long long)((double)positions * frac * 1.125) + 65536;
    }
    room = std::min<unsigned long long>(room, (unsigned long long)positions);
    unsigned long long back[1] = {0};
    for (int trip = 0;; ++trip) {
        int rc = sketcher_reserve(k, k->len + (long long)room);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(dcount.p, 0, count_bytes, c->stream));
        StageTimer tm;
        rc = tm.begin(c);
        if (rc) return rc;
        rc = mvs::launch_kmer_hash(c->stream, d_bases, total_bytes, (const mvs::KmerUnit*)dunits.p, n_units, U, ksize, k->seed, k->max_hash,
                                   k->vals.as<unsigned long long>() + k->len, k->samp.as<int32_t>() + k->len, room, d_counters,
                                   d_sample_counts, d_sample_valid);
        if (rc) return fail(rc, "k_kmer_hash: bad launch geometry");
        rc = check_kernel("k_kmer_hash");
        if (rc) return rc;
        rc = tm.mark_end();
        if (rc) return rc;
        rc = read_back(c, c->stream, {{back, d_counters, sizeof(back)}});
        if (rc) return rc;
        rc = tm.add_to(&k->hash_ms);
        if (rc) return rc;
        if (back[0] <= room) break;
        if (trip > 0) return fail(MVS_E_HIP, "k_kmer_hash kept %llu values where its first trip kept %llu", back[0], room);
        room = back[0];                    // the exact size: the second trip cannot miss
        ++k->second_trips;
    }
    std::vector<unsigned long long> counts((size_t)n * 2);
    HIP_TRY(hipMemcpyAsync(counts.data(), d_sample_counts, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    k->len += (long long)back[0];
    ++k->adds;
    for (int64_t i = 0; i < n_pieces; ++i) k->bases[(size_t)samples[i]] += offsets[i + 1] - offsets[i];
    for (int64_t s = 0; s < n; ++s) {
        k->kept[(size_t)s] += (long long)counts[(size_t)s];
        k->kmers[(size_t)s] += (long long)counts[(size_t)(n + s)];
    }
    for (int64_t s = 0; s < n; ++s)
        if (k->kept[(size_t)s] >= (1LL << 31)) {
            k->broken = true;
            return fail(MVS_E_RANGE, "sample %lld keeps 2^31 values or more: the sketcher can only be destroyed", (long long)s);
        }
    return MVS_OK;
}

int mvs_kmer_sketcher_finish(mvs_kmer_sketcher* k, uint32_t min_abundance, uint32_t max_abundance, int64_t* histogram,
                             mvs_hash_set** out) {
    if (!k || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (k->finished) return fail(MVS_E_INVALID, "the sketcher is finished");
    if (k->broken) return fail(MVS_E_INVALID, "an earlier add failed: the sketcher can only be destroyed");
    if (const int rc = filter_checks(min_abundance, max_abundance)) return rc;
    mvs_ctx* c = k->ctx;
    const int64_t n = k->n;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_kmer_sketcher_finish");
    std::vector<long long> hoff((size_t)n + 1, 0);
    for (int64_t s = 0; s < n; ++s) hoff[(size_t)s + 1] = hoff[(size_t)s] + k->kept[(size_t)s];
    if (hoff[(size_t)n] != k->len)
        return fail(MVS_E_HIP, "the samples' counts sum to %lld, the staging list holds %lld", hoff[(size_t)n], k->len);
    DevBuf doff, dcur, dgrouped;
    if (k->len > 0) {
        if (doff.alloc(hoff.size() * 8) != hipSuccess || dcur.alloc((size_t)std::max<int64_t>(n, 1) * 8) != hipSuccess ||
            dgrouped.alloc((size_t)k->len * 8) != hipSuccess)
            return fail(MVS_E_NOMEM, "hipMalloc of %lld kept values failed", k->len);
        HIP_TRY(hipMemcpyAsync(doff.p, hoff.data(), hoff.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(dcur.p, 0, (size_t)std::max<int64_t>(n, 1) * 8, c->stream));
        StageTimer tm;
        int rc = tm.begin(c);
        if (rc) return rc;
        rc = mvs::launch_kmer_scatter(c->stream, k->vals.as<unsigned long long>(), k->samp.as<int32_t>(), k->len, (const long long*)doff.p,
                                      (unsigned long long*)dcur.p, (unsigned long long*)dgrouped.p);
        if (rc) return fail(rc, "k_kmer_scatter: bad launch geometry");
        rc = check_kernel("k_kmer_scatter");
        if (rc) return rc;
        rc = tm.mark_end();
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        rc = tm.add_to(&k->hash_ms);
        if (rc) return rc;
    }
    k->finished = true;                    // the staging list is gone: whatever follows, there is no second finish
    k->vals.reset();
    k->samp.reset();
    k->cap = 0;
    return counted_build(c, (const unsigned long long*)dgrouped.p, nullptr, hoff, n, min_abundance, max_abundance, histogram, &k->distinct,
                         &k->passed, out);
}

int mvs_kmer_sketcher_stats(const mvs_kmer_sketcher* k, int64_t* bases, int64_t* kmers, int64_t* kept, int64_t* distinct,
                            int64_t* passed) {
    if (!k) return fail(MVS_E_INVALID, "NULL sketcher");
    for (int64_t s = 0; s < k->n; ++s) {
        if (bases) bases[s] = k->bases[(size_t)s];
        if (kmers) kmers[s] = k->kmers[(size_t)s];
        if (kept) kept[s] = k->kept[(size_t)s];
        if (distinct) distinct[s] = k->distinct[(size_t)s];
        if (passed) passed[s] = k->passed[(size_t)s];
    }
    return MVS_OK;
}

int mvs_kmer_sketcher_info(const mvs_kmer_sketcher* k, double* kernel_ms, int64_t* staged, int64_t* capacity, int64_t* adds,
                           int64_t* second_trips, int64_t* growths) {
    if (!k) return fail(MVS_E_INVALID, "NULL sketcher");
    if (kernel_ms) *kernel_ms = k->hash_ms;
    if (staged) *staged = k->len;
    if (capacity) *capacity = k->cap;
    if (adds) *adds = k->adds;
    if (second_trips) *second_trips = k->second_trips;
    if (growths) *growths = k->growths;
    return MVS_OK;
}

int mvs_kmer_sketcher_destroy(mvs_kmer_sketcher* k) {
    if (!k) return MVS_OK;
    if (k->ctx) {
        (void)hipSetDevice(k->ctx->device);
        (void)hipStreamSynchronize(k->ctx->stream);
    }
    delete k;
    return MVS_OK;
}

}  // extern "C"
