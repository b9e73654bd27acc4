// mvs_capi_levels.hip -- C ABI of the level counts: mvs_pairwise_levels, mvs_ctx_levels_stats.
//
// Rows are taken in blocks of R (dots_block_rows): the dense-dots kernels fill an R x C int32 block
// (C = the column range), k_levels_count turns every row of it into m neighbour counts (mvs_levels.hip) and adds them to the
// m running totals, which live on the device and are read once, behind the last block.  Device memory besides the set:
// R x C x 4 bytes of dots, R x m counts when the caller's table is on the host, one pre-test integer per sample, m
// coefficients, m totals, one flag -- never N x N.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

#include <cmath>

using namespace mvs_capi;

extern "C" {

int mvs_pairwise_levels(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, const double* levels, int n_levels,
                        int64_t rb, int64_t re, int64_t cb, int64_t ce, int32_t* degrees, int mem_degrees, int64_t* totals) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    const int m = n_levels;
    if (m < 1 || m > mvs::kMaxLevels) return fail(MVS_E_INVALID, "n_levels = %d outside 1 .. %d", m, mvs::kMaxLevels);
    if (!levels) return fail(MVS_E_INVALID, "levels is NULL");
    double coef[mvs::kMaxLevels];
    for (int l = 0; l < m; ++l) {
        const double t = levels[l];
        if (!(t > 0.0) || !(t < 1.0)) return fail(MVS_E_INVALID, "level %d = %g outside (0, 1)", l, t);
        if (l > 0 && !(levels[l - 1] < t)) return fail(MVS_E_INVALID, "levels are not strictly ascending at %d", l);
        coef[l] = t / (1.0 + t);
        if (l > 0 && !(coef[l - 1] <= coef[l]))
            return fail(MVS_E_INVALID, "the coefficients t / (1 + t) of levels %d and %d decrease", l - 1, l);
    }
    if (!mem_ok(mem_norms) || !mem_ok(mem_degrees)) return fail(MVS_E_INVALID, "bad argument");
    if (rb < 0 || re > s->n || rb > re || cb < 0 || ce > s->n || cb > ce)
        return fail(MVS_E_INVALID, "range [%lld, %lld) x [%lld, %lld) outside the set's %lld samples", (long long)rb,
                    (long long)re, (long long)cb, (long long)ce, (long long)s->n);
    if (totals)
        for (int l = 0; l < m; ++l) totals[l] = 0;
    const int64_t rows = re - rb, cols = ce - cb;
    if (rows == 0 || cols == 0) return MVS_OK;
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    Range mark(c, "mvs_pairwise_levels");
    HIP_TRY(hipSetDevice(c->device));
    c->lv.reset();

    DevBuf dnorms;
    const double* d_n2 = nullptr;
    if (const int rc = norms_on_device(c, norms_sq, mem_norms, s->n, dnorms, &d_n2)) return rc;

    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const int64_t R = dots_block_rows(free_b / 4, (size_t)cols * 4, c->opt.levels_block_rows, rows);
    const bool stage = degrees && mem_degrees == MVS_MEM_HOST;   // a host table is filled block by block from a device copy
    DotsBlocks blocks;
    DevBuf dcoef, dtotal, dflag, ddeg, dthr;
    if (const int rc = blocks.init(c, s, cb, ce, R, c->opt.levels_dots, {"k_levels dots", "levels: dots launch rejected", "k_pairwise(levels dots)"}))
        return rc;
    HIP_TRY(dcoef.alloc(sizeof coef));
    HIP_TRY(dtotal.alloc((size_t)mvs::kMaxLevels * sizeof(unsigned long long)));
    HIP_TRY(dflag.alloc(sizeof(int)));
    HIP_TRY(dthr.alloc((size_t)s->n * sizeof(int)));
    if (stage) HIP_TRY(ddeg.alloc((size_t)R * m * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(dcoef.p, coef, (size_t)m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(dtotal.p, 0, (size_t)mvs::kMaxLevels * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemsetAsync(dflag.p, 0, sizeof(int), c->stream));
    {
        int rc = mvs::launch_levels_prep(c->stream, d_n2, s->n, cb, ce, coef[0], s->d, (int*)dthr.p, (int*)dflag.p);
        if (rc) return fail(rc, "levels: pre-test launch rejected");
        rc = check_kernel("k_levels_prep");
        if (rc) return rc;
    }
    const auto count = [&](int64_t r0, int64_t r1, const int32_t* dots) -> int {
        int32_t* d_deg = stage ? (int32_t*)ddeg.p : degrees ? degrees + (size_t)(r0 - rb) * m : nullptr;
        {
            Range rs(c, "k_levels count");
            int rc = mvs::launch_levels_count(c->stream, dots, r1 - r0, cols, r0, cb, d_n2, (const double*)dcoef.p, m, s->d,
                                              (const int*)dthr.p, (const int*)dflag.p, d_deg, (unsigned long long*)dtotal.p);
            if (rc) return fail(rc, "levels: count launch rejected");
            rc = check_kernel("k_levels_count");
            if (rc) return rc;
        }
        if (stage)                                               // (in stream order: the next block's kernel waits for the copy)
            HIP_TRY(hipMemcpyAsync(degrees + (size_t)(r0 - rb) * m, ddeg.p, (size_t)(r1 - r0) * m * sizeof(int32_t), hipMemcpyDeviceToHost,
                                   c->stream));
        return MVS_OK;
    };
    if (const int rc = blocks.run(rb, re, &c->lv.dots_ms, &c->lv.work_ms, &c->lv.blocks, count)) return rc;
    c->lv.block_rows = R;
    unsigned long long sums[mvs::kMaxLevels];
    HIP_TRY(hipMemcpyAsync(sums, dtotal.p, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                    // (also before the DevBufs free the scratch)
    if (totals)
        for (int l = 0; l < m; ++l) totals[l] = (int64_t)sums[l];
    return MVS_OK;
}

int mvs_ctx_levels_stats(const mvs_ctx* c, double* dots_ms, double* count_ms, int64_t* row_blocks, int64_t* block_rows) {
    return dots_stats_out(c, &mvs_ctx::lv, dots_ms, count_ms, row_blocks, block_rows);
}

}  // extern "C"
