// mvs_capi_contain.hip -- C ABI of the containment comparison: mvs_pairwise_contain, mvs_ctx_contain_stats.
//
// Rows are taken in blocks of R (dots_block_rows): the dense-dots kernels fill an R x C int32 block
// (C = the column range), k_contain_count / k_contain_scan / k_contain_fill select its cells in (row, col) order
// (mvs_contain.hip).  The running cell count lives on the device and is read once, behind the last block: a block whose rows
// do not fit the caller's capacity is counted and not written.  Device memory besides the set: R x C x 4 bytes of dots, a count
// and an offset per row of a block, one pre-test integer per sample -- never N x N.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

#include <cmath>

using namespace mvs_capi;

extern "C" {

int mvs_pairwise_contain(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double min_containment,
                         double slack, int flags, int64_t rb, int64_t re, int64_t cb, int64_t ce, mvs_cell* cells, int mem_cells,
                         int64_t capacity, int64_t* n_cells) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (!(min_containment > 0.0) || !(min_containment < 1.0))
        return fail(MVS_E_INVALID, "min_containment = %g outside (0, 1)", min_containment);
    if (!std::isfinite(slack)) return fail(MVS_E_INVALID, "slack is not a finite number");
    if (flags != MVS_CONTAIN_ROW && flags != MVS_CONTAIN_MAX) return fail(MVS_E_INVALID, "unknown flags %d", flags);
    if (!mem_ok(mem_norms) || !mem_ok(mem_cells) || capacity < 0) return fail(MVS_E_INVALID, "bad argument");
    if (rb < 0 || re > s->n || rb > re || cb < 0 || ce > s->n || cb > ce)
        return fail(MVS_E_INVALID, "range [%lld, %lld) x [%lld, %lld) outside the set's %lld samples", (long long)rb,
                    (long long)re, (long long)cb, (long long)ce, (long long)s->n);
    if (n_cells) *n_cells = 0;
    const int64_t rows = re - rb, cols = ce - cb;
    if (rows == 0 || cols == 0) return MVS_OK;
    if (!norms_sq || (!cells && capacity > 0)) return fail(MVS_E_INVALID, "norms_sq or cells is NULL");
    Range mark(c, "mvs_pairwise_contain");
    HIP_TRY(hipSetDevice(c->device));
    c->ct.reset();

    DevBuf dnorms;
    const double* d_n2 = nullptr;
    if (const int rc = norms_on_device(c, norms_sq, mem_norms, s->n, dnorms, &d_n2)) return rc;
    mvs::ContainRule ru{};
    ru.c = min_containment;
    ru.zz = slack * slack;
    ru.dd = (double)s->d;
    ru.zsign = slack > 0.0 ? 1 : slack < 0.0 ? -1 : 0;
    ru.mode = flags;
    ru.pretest = slack >= 0.0 ? 1 : 0;

    // the cells of a host caller are staged on the device: never more than the block of the call can hold
    DevBuf dout;
    mvs_cell* d_out = cells;
    if (mem_cells == MVS_MEM_HOST && capacity > 0) {
        const double most = (double)rows * (double)cols;
        const size_t room = (size_t)std::min((double)capacity, most);
        if (dout.alloc(room * sizeof(mvs_cell)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(MVS_E_NOMEM, "no device memory to stage %zu cells", room);
        }
        d_out = (mvs_cell*)dout.p;
    }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const int64_t R = dots_block_rows(free_b / 4, (size_t)cols * 4, c->opt.contain_block_rows, rows);
    DotsBlocks blocks;
    DevBuf dthr, dcounts, doffs, dtotal;
    if (const int rc = blocks.init(c, s, cb, ce, R, c->opt.contain_dots,
                                   {"k_contain dots", "containment: dots launch rejected", "k_pairwise(containment dots)"}))
        return rc;
    HIP_TRY(dthr.alloc((size_t)s->n * sizeof(int)));
    HIP_TRY(dcounts.alloc((size_t)R * sizeof(int)));
    HIP_TRY(doffs.alloc((size_t)R * sizeof(long long)));
    HIP_TRY(dtotal.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(dtotal.p, 0, sizeof(unsigned long long), c->stream));
    {
        int rc = mvs::launch_contain_thr(c->stream, d_n2, s->n, ru, (int*)dthr.p);
        if (rc) return fail(rc, "containment: pre-test launch rejected");
        rc = check_kernel("k_contain_thr");
        if (rc) return rc;
    }
    const auto select = [&](int64_t r0, int64_t r1, const int32_t* dots) -> int {
        Range rs(c, "k_contain select");
        int rc = mvs::launch_contain_count(c->stream, dots, r1 - r0, cols, r0, cb, d_n2, (const int*)dthr.p, ru, (int*)dcounts.p);
        if (rc) return fail(rc, "containment: count launch rejected");
        rc = check_kernel("k_contain_count");
        if (rc) return rc;
        rc = mvs::launch_contain_scan(c->stream, (const int*)dcounts.p, r1 - r0, (long long*)doffs.p, (unsigned long long*)dtotal.p);
        if (rc) return fail(rc, "containment: scan launch rejected");
        rc = check_kernel("k_contain_scan");
        if (rc || capacity <= 0) return rc;
        rc = mvs::launch_contain_fill(c->stream, dots, r1 - r0, cols, r0, cb, d_n2, (const int*)dthr.p, ru, (const int*)dcounts.p,
                                      (const long long*)doffs.p, d_out, capacity);
        if (rc) return fail(rc, "containment: fill launch rejected");
        return check_kernel("k_contain_fill");
    };
    if (const int rc = blocks.run(rb, re, &c->ct.dots_ms, &c->ct.work_ms, &c->ct.blocks, select)) return rc;
    c->ct.block_rows = R;
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, dtotal.p, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n_cells) *n_cells = (int64_t)total;
    if ((int64_t)total > capacity)
        return fail(MVS_E_CAPACITY, "containment keeps %llu cells, the buffer holds %lld", total, (long long)capacity);
    if (mem_cells == MVS_MEM_HOST && total > 0) {
        HIP_TRY(hipMemcpyAsync(cells, d_out, (size_t)total * sizeof(mvs_cell), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));   // (also before the DevBufs free the scratch)
    }
    return MVS_OK;
}

int mvs_ctx_contain_stats(const mvs_ctx* c, double* dots_ms, double* select_ms, int64_t* row_blocks, int64_t* block_rows) {
    return dots_stats_out(c, &mvs_ctx::ct, dots_ms, select_ms, row_blocks, block_rows);
}

}  // extern "C"
