// mvs_capi_topk.hip -- C ABI of the exact top-k comparison: mvs_pairwise_topk, mvs_ctx_topk_stats.
//
// Rows are taken in blocks of R (dots_block_rows): the dense-dots kernels fill an R x C int32 block (C = the column range), k_topk_select ranks
// each row of it (mvs_topk.hip), and after the last block the rows' padded lists are packed into the caller's array.  Device
// memory besides the set: R x C x 4 bytes of dots, (rows x k) padded cells, a count and an offset per row -- never N x N.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

using namespace mvs_capi;

extern "C" {

int mvs_pairwise_topk(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, int k, int64_t rb, int64_t re,
                      int64_t cb, int64_t ce, int flags, mvs_cell* cells, int mem_cells, int64_t* n_cells) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (k < 1 || k > mvs::kMaxTopk) return fail(MVS_E_INVALID, "k = %d outside 1..%d", k, mvs::kMaxTopk);
    if (!mem_ok(mem_norms) || !mem_ok(mem_cells) || (flags & ~MVS_TOPK_EXCLUDE_SELF) != 0)
        return fail(MVS_E_INVALID, "bad argument");
    if (rb < 0 || re > s->n || rb > re || cb < 0 || ce > s->n || cb > ce)
        return fail(MVS_E_INVALID, "range [%lld, %lld) x [%lld, %lld) outside the set's %lld samples", (long long)rb,
                    (long long)re, (long long)cb, (long long)ce, (long long)s->n);
    if (n_cells) *n_cells = 0;
    const int64_t rows = re - rb, cols = ce - cb;
    if (rows == 0 || cols == 0) return MVS_OK;
    if (!norms_sq || !cells) return fail(MVS_E_INVALID, "norms_sq or cells is NULL");
    Range mark(c, "mvs_pairwise_topk");
    HIP_TRY(hipSetDevice(c->device));
    c->tk.reset();

    DevBuf dnorms;
    const double* d_n2 = norms_sq;
    if (mem_norms == MVS_MEM_HOST) {
        HIP_TRY(dnorms.alloc((size_t)s->n * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(dnorms.p, norms_sq, (size_t)s->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        d_n2 = (const double*)dnorms.p;
    }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const int64_t R = dots_block_rows(free_b / 4, (size_t)cols * 4, c->opt.topk_block_rows, rows);
    DotsBlocks blocks;
    DevBuf dpad, dcounts, doffs, dout;
    if (const int rc = blocks.init(c, s, cb, ce, R, c->opt.topk_dots, {"k_topk dots", "top-k: dots launch rejected", "k_pairwise(top-k dots)"}))
        return rc;
    HIP_TRY(dpad.alloc((size_t)rows * (size_t)k * sizeof(mvs_cell)));
    HIP_TRY(dcounts.alloc((size_t)rows * sizeof(int)));
    const int excl = (flags & MVS_TOPK_EXCLUDE_SELF) ? 1 : 0;
    const auto select = [&](int64_t r0, int64_t r1, const int32_t* dots) -> int {
        Range rs(c, "k_topk_select");
        int rc = mvs::launch_topk_select(c->stream, dots, r1 - r0, cols, r0, cb, d_n2, s->d, k, excl, (mvs_cell*)dpad.p, (int*)dcounts.p, rb);
        if (rc) return fail(rc, "top-k: selection launch rejected");
        return check_kernel("k_topk_select");
    };
    if (const int rc = blocks.run(rb, re, &c->tk.dots_ms, &c->tk.work_ms, &c->tk.blocks, select)) return rc;
    c->tk.block_rows = R;
    // per-row counts -> offsets (host scan: 4 bytes down, 8 up per row), then the padded lists packed in row order
    std::vector<int> counts((size_t)rows);
    HIP_TRY(hipMemcpyAsync(counts.data(), dcounts.p, counts.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int64_t> offs((size_t)rows);
    int64_t total = 0;
    for (size_t i = 0; i < counts.size(); ++i) {
        offs[i] = total;
        total += counts[i];
    }
    HIP_TRY(doffs.alloc(offs.size() * sizeof(int64_t)));
    HIP_TRY(hipMemcpyAsync(doffs.p, offs.data(), offs.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    mvs_cell* d_out = cells;
    if (mem_cells == MVS_MEM_HOST) {
        HIP_TRY(dout.alloc((size_t)total * sizeof(mvs_cell)));
        d_out = (mvs_cell*)dout.p;
    }
    int rc = mvs::launch_topk_compact(c->stream, (const mvs_cell*)dpad.p, (const int*)dcounts.p, (const int64_t*)doffs.p, rows, k,
                                      d_out);
    if (rc) return fail(rc, "top-k: compaction launch rejected");
    rc = check_kernel("k_topk_compact");
    if (rc) return rc;
    if (mem_cells == MVS_MEM_HOST && total > 0)
        HIP_TRY(hipMemcpyAsync(cells, d_out, (size_t)total * sizeof(mvs_cell), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (also before the DevBufs free the scratch)
    if (n_cells) *n_cells = total;
    return MVS_OK;
}

int mvs_ctx_topk_stats(const mvs_ctx* c, double* dots_ms, double* select_ms, int64_t* row_blocks, int64_t* block_rows) {
    return dots_stats_out(c, &mvs_ctx::tk, dots_ms, select_ms, row_blocks, block_rows);
}

}  // extern "C"
