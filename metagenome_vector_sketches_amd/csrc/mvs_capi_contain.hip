// mvs_capi_contain.hip -- C ABI of the containment comparison: mvs_pairwise_contain, mvs_ctx_contain_stats.
//
// Rows are taken in blocks of R, sized as mvs_pairwise_topk sizes them: the dense-dots kernels fill an R x C int32 block
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
    c->ct_dots_ms = c->ct_select_ms = 0.0;
    c->ct_blocks = c->ct_block_rows = 0;

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
    // rows per block: the dots block takes a quarter of the free memory (as mvs_pairwise_topk sizes its blocks)
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t row_bytes = (size_t)cols * 4;
    int64_t R = (int64_t)std::max<size_t>(1, (free_b / 4) / row_bytes);
    R = std::min<int64_t>(R, 8192);
    if (c->opt.contain_block_rows > 0) R = std::min<int64_t>(R, c->opt.contain_block_rows);
    R = std::min(R, rows);
    DevBuf ddots, dthr, dcounts, doffs, dtotal;
    HIP_TRY(ddots.alloc((size_t)R * row_bytes));
    HIP_TRY(dthr.alloc((size_t)s->n * sizeof(int)));
    HIP_TRY(dcounts.alloc((size_t)R * sizeof(int)));
    HIP_TRY(doffs.alloc((size_t)R * sizeof(long long)));
    HIP_TRY(dtotal.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(dtotal.p, 0, sizeof(unsigned long long), c->stream));
    struct Events {
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev;
    if (c->timing)
        for (hipEvent_t& x : ev.e) HIP_TRY(hipEventCreate(&x));
    {
        int rc = mvs::launch_contain_thr(c->stream, d_n2, s->n, ru, (int*)dthr.p);
        if (rc) return fail(rc, "containment: pre-test launch rejected");
        rc = check_kernel("k_contain_thr");
        if (rc) return rc;
    }
    const int algo = c->opt.contain_dots;
    for (int64_t r0 = rb; r0 < re; r0 += R) {
        const int64_t r1 = std::min(r0 + R, re);
        mvs::PairwiseArgs a{};
        a.planes = s->planes;
        a.n = s->n;
        a.n_alloc = s->n_alloc;
        a.d = s->d;
        a.d_pad = s->d_pad;
        a.limbs = s->limbs;
        a.row_begin = r0;
        a.row_end = r1;
        a.col_begin = cb;
        a.col_end = ce;
        a.dots = (int32_t*)ddots.p;
        if (c->timing) HIP_TRY(hipEventRecord(ev.e[0], c->stream));
        {
            Range rd(c, "k_contain dots");
            int rc = mvs::launch_pairwise(c->stream, a, 1, algo, c->opt);
            if (rc) return fail(rc, "containment: dots launch rejected");
            rc = check_kernel("k_pairwise(containment dots)");
            if (rc) return rc;
        }
        if (c->timing) HIP_TRY(hipEventRecord(ev.e[1], c->stream));
        {
            Range rs(c, "k_contain select");
            int rc = mvs::launch_contain_count(c->stream, (const int32_t*)ddots.p, r1 - r0, cols, r0, cb, d_n2, (const int*)dthr.p, ru,
                                               (int*)dcounts.p);
            if (rc) return fail(rc, "containment: count launch rejected");
            rc = check_kernel("k_contain_count");
            if (rc) return rc;
            rc = mvs::launch_contain_scan(c->stream, (const int*)dcounts.p, r1 - r0, (long long*)doffs.p, (unsigned long long*)dtotal.p);
            if (rc) return fail(rc, "containment: scan launch rejected");
            rc = check_kernel("k_contain_scan");
            if (rc) return rc;
            if (capacity > 0) {
                rc = mvs::launch_contain_fill(c->stream, (const int32_t*)ddots.p, r1 - r0, cols, r0, cb, d_n2, (const int*)dthr.p, ru,
                                              (const int*)dcounts.p, (const long long*)doffs.p, d_out, capacity);
                if (rc) return fail(rc, "containment: fill launch rejected");
                rc = check_kernel("k_contain_fill");
                if (rc) return rc;
            }
        }
        if (c->timing) {
            HIP_TRY(hipEventRecord(ev.e[2], c->stream));
            HIP_TRY(hipEventSynchronize(ev.e[2]));
            float m0 = 0.f, m1 = 0.f;
            HIP_TRY(hipEventElapsedTime(&m0, ev.e[0], ev.e[1]));
            HIP_TRY(hipEventElapsedTime(&m1, ev.e[1], ev.e[2]));
            c->ct_dots_ms += m0;
            c->ct_select_ms += m1;
        }
        ++c->ct_blocks;
    }
    c->ct_block_rows = R;
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
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (dots_ms) *dots_ms = c->ct_dots_ms;
    if (select_ms) *select_ms = c->ct_select_ms;
    if (row_blocks) *row_blocks = c->ct_blocks;
    if (block_rows) *block_rows = c->ct_block_rows;
    return MVS_OK;
}

}  // extern "C"
