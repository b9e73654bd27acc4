// mvs_capi_topk.hip -- C ABI of the exact top-k comparison: mvs_pairwise_topk, mvs_ctx_topk_stats.
//
// Rows are taken in blocks of R: the dense-dots kernels fill an R x C int32 block (C = the column range), k_topk_select ranks
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
    c->tk_dots_ms = c->tk_select_ms = 0.0;
    c->tk_blocks = c->tk_block_rows = 0;

    DevBuf dnorms;
    const double* d_n2 = norms_sq;
    if (mem_norms == MVS_MEM_HOST) {
        HIP_TRY(dnorms.alloc((size_t)s->n * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(dnorms.p, norms_sq, (size_t)s->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        d_n2 = (const double*)dnorms.p;
    }
    // rows per block: the dots block takes a quarter of the free memory (as mvs_pairwise_stream sizes its blocks)
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t pad_bytes = (size_t)rows * (size_t)k * sizeof(mvs_cell);
    const size_t row_bytes = (size_t)cols * 4;
    int64_t R = (int64_t)std::max<size_t>(1, (free_b / 4) / row_bytes);
    R = std::min<int64_t>(R, 8192);
    if (c->opt.topk_block_rows > 0) R = std::min<int64_t>(R, c->opt.topk_block_rows);
    R = std::min(R, rows);
    DevBuf ddots, dpad, dcounts, doffs, dout;
    HIP_TRY(ddots.alloc((size_t)R * row_bytes));
    HIP_TRY(dpad.alloc(pad_bytes));
    HIP_TRY(dcounts.alloc((size_t)rows * sizeof(int)));
    struct Events {
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev;
    if (c->timing)
        for (hipEvent_t& x : ev.e) HIP_TRY(hipEventCreate(&x));
    const int algo = c->opt.topk_dots;
    const int excl = (flags & MVS_TOPK_EXCLUDE_SELF) ? 1 : 0;
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
            Range rd(c, "k_topk dots");
            int rc = mvs::launch_pairwise(c->stream, a, 1, algo, c->opt);
            if (rc) return fail(rc, "top-k: dots launch rejected");
            rc = check_kernel("k_pairwise(top-k dots)");
            if (rc) return rc;
        }
        if (c->timing) HIP_TRY(hipEventRecord(ev.e[1], c->stream));
        {
            Range rs(c, "k_topk_select");
            int rc = mvs::launch_topk_select(c->stream, (const int32_t*)ddots.p, r1 - r0, cols, r0, cb, d_n2, s->d, k, excl,
                                             (mvs_cell*)dpad.p, (int*)dcounts.p, rb);
            if (rc) return fail(rc, "top-k: selection launch rejected");
            rc = check_kernel("k_topk_select");
            if (rc) return rc;
        }
        if (c->timing) {
            HIP_TRY(hipEventRecord(ev.e[2], c->stream));
            HIP_TRY(hipEventSynchronize(ev.e[2]));
            float m0 = 0.f, m1 = 0.f;
            HIP_TRY(hipEventElapsedTime(&m0, ev.e[0], ev.e[1]));
            HIP_TRY(hipEventElapsedTime(&m1, ev.e[1], ev.e[2]));
            c->tk_dots_ms += m0;
            c->tk_select_ms += m1;
        }
        ++c->tk_blocks;
    }
    c->tk_block_rows = R;
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
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (dots_ms) *dots_ms = c->tk_dots_ms;
    if (select_ms) *select_ms = c->tk_select_ms;
    if (row_blocks) *row_blocks = c->tk_blocks;
    if (block_rows) *block_rows = c->tk_block_rows;
    return MVS_OK;
}

}  // extern "C"
