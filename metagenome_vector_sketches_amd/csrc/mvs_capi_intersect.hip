// mvs_capi_intersect.hip -- C ABI of the exact hash-set intersections: mvs_hash_set_create / _info / _sizes / _destroy (a
// resident, per-sample sorted and de-duplicated copy of hash lists), mvs_intersect_cells (|H(row) n H(col)| for every cell of a
// list, whoever produced it) and mvs_ctx_intersect_stats.  The kernels and the layout of the units of work are in
// mvs_intersect.hip; the body of the cell-list call is cells_over_units (mvs_capi_internal.h), which mvs_abund_overlap_cells
// shares.  With device cells and device counts nothing but a few counters crosses the link.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

using namespace mvs_capi;

namespace {

constexpr int64_t kSortBatch = 1LL << 30;   // keys per segmented sort (rocprim counts them in 32 bits; a sample holds < 2^31)

struct SetGuard {
    mvs_hash_set* h;
    ~SetGuard() {
        if (h) mvs_hash_set_destroy(h);
    }
};

// lists that are not sorted and unique: segmented sort in batches of whole samples, then the distinct values of every sample
// move together.  On return h->hashes / offsets / sizes / total describe the compacted lists.
int sort_and_compact(mvs_ctx* c, mvs_hash_set* h, const std::vector<long long>& off) {
    const int64_t n = h->n;
    const long long total_in = off[(size_t)n];
    DevBuf sorted;
    if (sorted.alloc((size_t)total_in * 8) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %lld hashes for the sort failed", total_in);
    std::vector<unsigned int> seg;
    for (int64_t s0 = 0; s0 < n;) {
        int64_t s1 = s0 + 1;
        while (s1 < n && off[(size_t)s1 + 1] - off[(size_t)s0] <= kSortBatch && s1 - s0 < (1LL << 30)) ++s1;
        const long long base = off[(size_t)s0];
        const unsigned int count = (unsigned int)(off[(size_t)s1] - base);
        const unsigned int segments = (unsigned int)(s1 - s0);
        if (count > 0) {
            seg.resize((size_t)segments + 1);
            for (int64_t s = s0; s <= s1; ++s) seg[(size_t)(s - s0)] = (unsigned int)(off[(size_t)s] - base);
            DevBuf dseg, dtmp;
            HIP_TRY(dseg.alloc(seg.size() * 4));
            HIP_TRY(hipMemcpyAsync(dseg.p, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, c->stream));
            const unsigned int* d_begin = (const unsigned int*)dseg.p;
            size_t need = 0;
            int rc = mvs::hs_sort_segments(c->stream, h->hashes.as<unsigned long long>() + base, (unsigned long long*)sorted.p + base,
                                           count, segments, d_begin, d_begin + 1, nullptr, 0, &need);
            if (rc) return fail(rc, "hash set: sort sizing failed");
            HIP_TRY(dtmp.alloc(need));
            rc = mvs::hs_sort_segments(c->stream, h->hashes.as<unsigned long long>() + base, (unsigned long long*)sorted.p + base, count,
                                       segments, d_begin, d_begin + 1, dtmp.p, need, nullptr);
            if (rc) return fail(rc, "hash set: segmented sort failed");
            HIP_TRY(hipStreamSynchronize(c->stream));   // (before seg is rewritten and the DevBufs free their memory)
        }
        s0 = s1;
    }
    int rc = mvs::launch_hs_count(c->stream, (const unsigned long long*)sorted.p, h->offsets.as<long long>(), n, h->sizes.as<int32_t>());
    if (!rc) rc = check_kernel("k_hs_count");
    if (rc) return rc;
    std::vector<int32_t> sizes((size_t)n);
    HIP_TRY(hipMemcpyAsync(sizes.data(), h->sizes.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<long long> noff((size_t)n + 1);
    noff[0] = 0;
    for (int64_t s = 0; s < n; ++s) noff[(size_t)s + 1] = noff[(size_t)s] + sizes[(size_t)s];
    DevBuf dnoff;
    HIP_TRY(dnoff.alloc(noff.size() * 8));
    HIP_TRY(hipMemcpyAsync(dnoff.p, noff.data(), noff.size() * 8, hipMemcpyHostToDevice, c->stream));
    DevBuf out;
    if (out.alloc((size_t)std::max<long long>(noff[(size_t)n], 1) * 8) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of %lld distinct hashes failed", noff[(size_t)n]);
    rc = mvs::launch_hs_compact(c->stream, (const unsigned long long*)sorted.p, h->offsets.as<long long>(), (const long long*)dnoff.p, n,
                                out.as<unsigned long long>());
    if (!rc) rc = check_kernel("k_hs_compact");
    hipError_t e = hipStreamSynchronize(c->stream);
    if (rc || e != hipSuccess) return rc ? rc : fail(MVS_E_HIP, "hash set: compaction failed: %s", hipGetErrorString(e));
    h->hashes = std::move(out);
    h->total = noff[(size_t)n];
    std::swap(h->offsets, dnoff);   // the set keeps the new offsets, dnoff frees the old ones
    return MVS_OK;
}

}  // namespace

extern "C" {

int mvs_hash_set_create(mvs_ctx* c, const uint64_t* hashes, int mem_hashes, const int64_t* offsets, int64_t n_samples,
                        mvs_hash_set** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n_samples < 0) return fail(MVS_E_INVALID, "n_samples = %lld is negative", (long long)n_samples);
    if (n_samples >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n_samples too large for int32 sample indices");
    if (!mem_ok(mem_hashes)) return fail(MVS_E_INVALID, "bad argument");
    if (n_samples > 0 && !offsets) return fail(MVS_E_INVALID, "offsets is NULL");
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
    const long long total_in = off[(size_t)n];
    if (total_in > 0 && !hashes) return fail(MVS_E_INVALID, "hashes is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_hash_set_create");
    mvs_hash_set* h = new (std::nothrow) mvs_hash_set();
    if (!h) return fail(MVS_E_NOMEM, "out of host memory");
    SetGuard guard{h};
    h->ctx = c;
    h->n = n;
    h->total = total_in;
    if (h->hashes.alloc((size_t)std::max<long long>(total_in, 1) * 8) != hipSuccess ||
        h->offsets.alloc(((size_t)n + 1) * 8) != hipSuccess || h->sizes.alloc((size_t)std::max<int64_t>(n, 1) * 4) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of a hash set of %lld hashes failed", total_in);
    if (total_in > 0)
        HIP_TRY(hipMemcpyAsync(h->hashes.p, hashes + base, (size_t)total_in * 8,
                               mem_hashes == MVS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(h->offsets.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream));
    unsigned int unsorted = 0;
    if (n > 0) {
        unsigned int* d_flag = (unsigned int*)c->counters();
        HIP_TRY(hipMemsetAsync(d_flag, 0, 8, c->stream));
        int rc = mvs::launch_hs_check(c->stream, h->hashes.as<unsigned long long>(), h->offsets.as<long long>(), n, d_flag);
        if (!rc) rc = check_kernel("k_hs_check");
        if (rc) return rc;
        rc = read_back(c, c->stream, {{&unsorted, d_flag, 4}});
        if (rc) return rc;
    }
    h->was_sorted = unsorted ? 0 : 1;
    if (unsorted) {
        const int rc = sort_and_compact(c, h, off);
        if (rc) return rc;
    } else if (n > 0) {
        std::vector<int32_t> sizes((size_t)n);
        for (int64_t s = 0; s < n; ++s) sizes[(size_t)s] = (int32_t)(off[(size_t)s + 1] - off[(size_t)s]);
        HIP_TRY(hipMemcpyAsync(h->sizes.p, sizes.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    guard.h = nullptr;
    *out = h;
    return MVS_OK;
}

int mvs_hash_set_info(const mvs_hash_set* h, int64_t* n_samples, int64_t* n_hashes, int* was_sorted) {
    if (!h) return fail(MVS_E_INVALID, "NULL hash set");
    if (n_samples) *n_samples = h->n;
    if (n_hashes) *n_hashes = h->total;
    if (was_sorted) *was_sorted = h->was_sorted;
    return MVS_OK;
}

int mvs_hash_set_sizes(const mvs_hash_set* h, int32_t* sizes, int mem_out) {
    if (!h) return fail(MVS_E_INVALID, "NULL hash set");
    if (!mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (h->n == 0) return MVS_OK;
    if (!sizes) return fail(MVS_E_INVALID, "sizes is NULL");
    mvs_ctx* c = h->ctx;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(sizes, h->sizes.p, (size_t)h->n * 4, mem_out == MVS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_hash_set_destroy(mvs_hash_set* h) {
    if (!h) return MVS_OK;
    if (h->ctx) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
    }
    delete h;
    return MVS_OK;
}

int mvs_intersect_cells(mvs_ctx* c, const mvs_hash_set* hs_rows, const mvs_hash_set* hs_cols, const mvs_cell* cells, int mem_cells,
                        int64_t n_cells, int32_t* inter, int mem_out) {
    const mvs_hash_set* hc = hs_cols ? hs_cols : hs_rows;
    return cells_over_units(c, {"mvs_intersect_cells", "intersect", "counts", "inter", "k_isect_units"}, hs_rows, hs_cols, cells, mem_cells,
                            n_cells, inter, mem_out, [&](const mvs_cell* d_cells, const PlannedUnits& plan, int32_t* d_inter) {
                                return mvs::launch_isect_units(c->stream, d_cells, n_cells, plan.d_start, plan.n_units,
                                                               hs_rows->hashes.as<unsigned long long>(), hs_rows->offsets.as<long long>(),
                                                               hs_rows->sizes.as<int32_t>(), hc->hashes.as<unsigned long long>(),
                                                               hc->offsets.as<long long>(), hc->sizes.as<int32_t>(),
                                                               c->opt.intersect_unit, d_inter);
                            });
}

int mvs_ctx_intersect_stats(const mvs_ctx* c, double* kernel_ms, int64_t* units, int64_t* cut_pairs, int64_t* bytes) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (kernel_ms) *kernel_ms = c->ix_kernel_ms;
    if (units) *units = c->ix_units;
    if (cut_pairs) *cut_pairs = c->ix_cut;
    if (bytes) *bytes = c->ix_bytes;
    return MVS_OK;
}

}  // extern "C"
