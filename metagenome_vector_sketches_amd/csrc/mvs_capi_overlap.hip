// mvs_capi_overlap.hip -- C ABI of the abundance-weighted overlaps: mvs_abund_overlap_cells (the six integer sums of every cell
// of a list), mvs_hash_set_abundance_totals (the per-sample totals they are set against) and mvs_abund_similarity (pure host:
// the derived measures, one rounding per line).  The kernels are in mvs_overlap.hip; the body of the cell-list call is the one
// mvs_intersect_cells has (cells_over_units, mvs_capi_internal.h), so it leaves that call's statistics too.
#include "mvs_capi_internal.h"

#include <cmath>

#include <hip/hip_runtime.h>

using namespace mvs_capi;

static_assert(sizeof(mvs_abund_overlap) == 48, "record layout");

extern "C" {

int mvs_abund_overlap_cells(mvs_ctx* c, const mvs_hash_set* hs_rows, const mvs_hash_set* hs_cols, const mvs_cell* cells, int mem_cells,
                            int64_t n_cells, mvs_abund_overlap* out, int mem_out) {
    const mvs_hash_set* hc = hs_cols ? hs_cols : hs_rows;
    return cells_over_units(c, {"mvs_abund_overlap_cells", "overlap", "records", "out", "k_overlap_units"}, hs_rows, hs_cols, cells, mem_cells,
                            n_cells, out, mem_out, [&](const mvs_cell* d_cells, const PlannedUnits& plan, mvs_abund_overlap* d_out) {
                                return mvs::launch_overlap_units(c->stream, d_cells, n_cells, plan.d_start, plan.n_units,
                                                                 hs_rows->hashes.as<unsigned long long>(), hs_rows->offsets.as<long long>(),
                                                                 hs_rows->sizes.as<int32_t>(), hs_rows->abund.as<uint32_t>(),
                                                                 hc->hashes.as<unsigned long long>(), hc->offsets.as<long long>(),
                                                                 hc->sizes.as<int32_t>(), hc->abund.as<uint32_t>(), c->opt.intersect_unit,
                                                                 d_out);
                            });
}

int mvs_hash_set_abundance_totals(const mvs_hash_set* h, uint64_t* sum, uint64_t* sumsq_lo, uint64_t* sumsq_hi, int mem_out) {
    if (!h) return fail(MVS_E_INVALID, "NULL hash set");
    if (!mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    const int64_t n = h->n;
    if (n == 0 || (!sum && !sumsq_lo && !sumsq_hi)) return MVS_OK;
    mvs_ctx* c = h->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)n * 8;
    uint64_t* const outs[3] = {sum, sumsq_lo, sumsq_hi};
    if (!h->abund.p) {
        // no abundances: 1 for every value, so S = Q_lo = the sample's size and Q_hi = 0
        std::vector<int32_t> sizes((size_t)n);
        HIP_TRY(hipMemcpyAsync(sizes.data(), h->sizes.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::vector<uint64_t> wide(sizes.begin(), sizes.end()), zero((size_t)n, 0);
        for (int k = 0; k < 3; ++k) {
            const uint64_t* from = k < 2 ? wide.data() : zero.data();
            if (outs[k] && mem_out == MVS_MEM_HOST) memcpy(outs[k], from, bytes);
            else if (outs[k]) HIP_TRY(hipMemcpyAsync(outs[k], from, bytes, hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        return MVS_OK;
    }
    DevBuf tmp;
    unsigned long long* d[3] = {(unsigned long long*)sum, (unsigned long long*)sumsq_lo, (unsigned long long*)sumsq_hi};
    if (mem_out == MVS_MEM_HOST) {
        if (tmp.alloc(3 * bytes) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %lld totals failed", (long long)n);
        for (int k = 0; k < 3; ++k) d[k] = outs[k] ? tmp.as<unsigned long long>() + (size_t)k * (size_t)n : nullptr;
    }
    int rc = mvs::launch_abund_totals(c->stream, h->abund.as<uint32_t>(), h->offsets.as<long long>(), n, d[0], d[1], d[2]);
    if (!rc) rc = check_kernel("k_abund_totals");
    if (rc) return rc;
    if (mem_out == MVS_MEM_HOST)
        for (int k = 0; k < 3; ++k)
            if (outs[k]) HIP_TRY(hipMemcpyAsync(outs[k], d[k], bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

// Every line below is one rounding (this file is compiled without contraction into fused multiply-adds).
int mvs_abund_similarity(const mvs_abund_overlap* o, uint64_t sum_row, uint64_t sumsq_lo_row, uint64_t sumsq_hi_row, int64_t size_row,
                         uint64_t sum_col, uint64_t sumsq_lo_col, uint64_t sumsq_hi_col, int64_t size_col, double out[6]) {
    if (!o || !out) return fail(MVS_E_INVALID, "NULL argument");
    if (size_row < 0 || size_col < 0 || o->inter < 0 || o->inter > size_row || o->inter > size_col)
        return fail(MVS_E_INVALID, "inter = %lld does not fit samples of %lld and %lld values", (long long)o->inter, (long long)size_row,
                    (long long)size_col);
    if (o->w_min > sum_row || o->w_min > sum_col) return fail(MVS_E_INVALID, "w_min exceeds a sample's total abundance");
    typedef unsigned __int128 u128;
    const u128 both = (u128)sum_row + sum_col;
    const double s_row = (double)sum_row, s_col = (double)sum_col;
    const double w_min = (double)o->w_min;
    out[0] = (double)o->w_row / s_row;
    out[1] = (double)o->w_col / s_col;
    out[2] = (double)(both - 2 * (u128)o->w_min) / (double)both;
    out[3] = w_min / (double)(both - o->w_min);
    const double dot = (double)(((u128)o->dot_hi << 32) + o->dot_lo);
    const double q_row = (double)(((u128)sumsq_hi_row << 32) + sumsq_lo_row);
    const double q_col = (double)(((u128)sumsq_hi_col << 32) + sumsq_lo_col);
    const double product = q_row * q_col;
    const double root = std::sqrt(product);
    double cosine = dot / root;
    if (cosine > 1.0) cosine = 1.0;                                    // (a NaN stays one)
    out[4] = cosine;
    out[5] = 1.0 - 2.0 * std::acos(cosine) / M_PI;
    return MVS_OK;
}

}  // extern "C"
