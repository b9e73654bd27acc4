// mvs_capi_pcoa.hip -- C ABI of the Jaccard kernel as an operator and of the principal coordinates built on it: mvs_jaccard_apply,
// mvs_pcoa_fit / _info / _get / _transform / _destroy, mvs_ctx_pcoa_stats.  The kernel and the rule are in mvs_kapply.hip.
//
// Apply.  Rows are taken in blocks of R (dots_block_rows): the dense-dots kernels fill an R x C int32
// block (C = the column range), k_jaccard_apply turns it into R x b sums against the zero-padded copy of X.  Device memory
// besides the set: R x C x 4 bytes of dots, the padded X, the rows x b result -- never N x N.
//
// Fit.  B = 1/2 H K H over the fitted range F (m samples), H = I - 11^T / m.  One apply against a column of ones gives the row
// sums of K, hence rowmean, grand and trace.  The leading eigenpairs come from the solver mvs_pca_fit uses (subspace_iterate,
// mvs_capi_pca.hip), whose operator here is: centre the block's columns on the host, apply K on the device row block by row
// block, centre the result's columns and halve it on the host.  Every host sum runs in index order on one thread.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

#include <cmath>

using namespace mvs_capi;

struct mvs_pcoa {
    mvs_ctx* ctx = nullptr;
    const mvs_sketch_set* set = nullptr;
    unsigned long long set_id = 0;
    int64_t fb = 0, fe = 0, m = 0;
    int c = 0, block = 0, iterations = 0, converged = 0, negative = 0;
    double floor = 0.0, grand = 0.0, trace = 0.0;
    std::vector<double> lambda, vectors, coords, rowmean, residuals, off;   // vectors, coords: m x c row-major; off[j] = sum_i rowmean[i] v[i][j]
    DevBuf d_Vp;                                                            // the vectors, padded as k_jaccard_apply reads its operand
};

namespace {

// K over rows x [cb, ce) applied to padded operands, row block by row block; the times and counts go to the context's po fields
struct Applier {
    DotsBlocks blocks;
    const double* d_n2 = nullptr;
    double floor = 0.0;
    int init(mvs_ctx* c, const mvs_sketch_set* s, const double* n2, double floor_, int64_t cb, int64_t ce, int64_t max_rows) {
        d_n2 = n2, floor = floor_;
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        c->po.block_rows = dots_block_rows(free_b / 4, (size_t)(ce - cb) * 4, c->opt.pcoa_block_rows, max_rows);
        return blocks.init(c, s, cb, ce, c->po.block_rows, c->opt.pcoa_dots,
                           {"k_jaccard_apply dots", "jaccard apply: dots launch rejected", "k_pairwise(apply dots)"});
    }
    // d_Y ((re - rb) x b) = K(rows [rb, re) x [cb, ce)) Xp; queued on the context's stream (with timing on it waits per block)
    int run(int64_t rb, int64_t re, const double* d_Xp, int b, double* d_Y) {
        mvs_ctx* c = blocks.c;
        const auto apply = [&](int64_t r0, int64_t r1, const int32_t* dots) -> int {
            Range rs(c, "k_jaccard_apply");
            const int rc = mvs::launch_jaccard_apply(c->stream, dots, r1 - r0, blocks.ce - blocks.cb, r0, blocks.cb, d_n2, blocks.s->d, floor,
                                                     d_Xp, b, d_Y + (size_t)(r0 - rb) * b);
            if (rc) return fail(rc, "jaccard apply: launch rejected");
            return check_kernel("k_jaccard_apply");
        };
        if (const int rc = blocks.run(rb, re, &c->po.dots_ms, &c->po.work_ms, &c->po.blocks, apply)) return rc;
        ++c->po_passes;
        return MVS_OK;
    }
};

void reset_stats(mvs_ctx* c) {
    c->po.reset();
    c->po_eigen_ms = 0.0;
    c->po_passes = 0;
}

inline size_t padded_doubles(int64_t cols, int b) { return (size_t)mvs::apply_padded_cols(cols) * (size_t)mvs::apply_padded_b(b); }

// x (cols x b, row-major, on the host) into the zeroed padded image `padded`
void pad_on_host(const double* x, int64_t cols, int b, std::vector<double>& padded) {
    const int cp = mvs::apply_padded_b(b);
    padded.assign(padded_doubles(cols, b), 0.0);
    for (int64_t j = 0; j < cols; ++j) std::memcpy(padded.data() + (size_t)j * cp, x + (size_t)j * b, (size_t)b * 8);
}

int common_checks(const mvs_ctx* c, const mvs_sketch_set* s, int mem_norms, double floor) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (!(floor >= 0.0) || !(floor < 1.0)) return fail(MVS_E_INVALID, "floor = %g outside [0, 1)", floor);
    if (!mem_ok(mem_norms)) return fail(MVS_E_INVALID, "bad argument");
    return MVS_OK;
}

}  // namespace

extern "C" {

int mvs_jaccard_apply(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double floor, int64_t rb, int64_t re,
                      int64_t cb, int64_t ce, const double* X, int b, int mem_x, double* Y, int mem_y) {
    if (const int rc = common_checks(c, s, mem_norms, floor)) return rc;
    if (b < 1 || b > 128) return fail(MVS_E_INVALID, "b = %d outside 1 .. 128", b);
    if (!mem_ok(mem_x) || !mem_ok(mem_y)) return fail(MVS_E_INVALID, "bad argument");
    if (rb < 0 || re > s->n || rb > re || cb < 0 || ce > s->n || cb > ce)
        return fail(MVS_E_INVALID, "range [%lld, %lld) x [%lld, %lld) outside the set's %lld samples", (long long)rb, (long long)re,
                    (long long)cb, (long long)ce, (long long)s->n);
    const int64_t rows = re - rb, cols = ce - cb;
    if (rows == 0) return MVS_OK;
    if (!Y) return fail(MVS_E_INVALID, "Y is NULL");
    HIP_TRY(hipSetDevice(c->device));
    reset_stats(c);
    const size_t y_bytes = (size_t)rows * b * 8;
    if (cols == 0) {
        if (mem_y == MVS_MEM_HOST) {
            std::memset(Y, 0, y_bytes);
        } else {
            HIP_TRY(hipMemsetAsync(Y, 0, y_bytes, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        return MVS_OK;
    }
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    if (!X) return fail(MVS_E_INVALID, "X is NULL");
    Range mark(c, "mvs_jaccard_apply");
    DevBuf dnorms, dXp, dY;
    const double* d_n2 = nullptr;
    if (const int rc = norms_on_device(c, norms_sq, mem_norms, s->n, dnorms, &d_n2)) return rc;
    const int cp = mvs::apply_padded_b(b);
    HIP_TRY(dXp.alloc(padded_doubles(cols, b) * 8));
    std::vector<double> padded;                                  // (alive until the synchronise below)
    if (mem_x == MVS_MEM_HOST) {
        pad_on_host(X, cols, b, padded);
        HIP_TRY(hipMemcpyAsync(dXp.p, padded.data(), padded.size() * 8, hipMemcpyHostToDevice, c->stream));
    } else {
        HIP_TRY(hipMemsetAsync(dXp.p, 0, padded_doubles(cols, b) * 8, c->stream));
        HIP_TRY(hipMemcpy2DAsync(dXp.p, (size_t)cp * 8, X, (size_t)b * 8, (size_t)b * 8, (size_t)cols, hipMemcpyDeviceToDevice, c->stream));
    }
    double* d_Y = Y;
    if (mem_y == MVS_MEM_HOST) {
        HIP_TRY(dY.alloc(y_bytes));
        d_Y = (double*)dY.p;
    }
    Applier ap;
    if (const int rc = ap.init(c, s, d_n2, floor, cb, ce, rows)) return rc;
    if (const int rc = ap.run(rb, re, (const double*)dXp.p, b, d_Y)) return rc;
    if (mem_y == MVS_MEM_HOST) HIP_TRY(hipMemcpyAsync(Y, d_Y, y_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                    // (also before the DevBufs free the scratch)
    return MVS_OK;
}

int mvs_pcoa_fit(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, int64_t fb, int64_t fe, int components,
                 double floor, double tol, int max_iters, mvs_pcoa** out) {
    if (!out) return fail(MVS_E_INVALID, "NULL output");
    *out = nullptr;
    if (const int rc = common_checks(c, s, mem_norms, floor)) return rc;
    if (fb < 0 || fe > s->n || fb > fe) return fail(MVS_E_INVALID, "rows [%lld, %lld) outside the set's %lld samples", (long long)fb, (long long)fe, (long long)s->n);
    const int64_t m = fe - fb;
    if (m < 2) return fail(MVS_E_INVALID, "principal coordinates need at least two samples");
    if (m > INT32_MAX) return fail(MVS_E_INVALID, "%lld samples exceed the solver's size", (long long)m);
    const int cmax = (int)std::min<int64_t>(64, m - 1);
    if (components < 1 || components > cmax) return fail(MVS_E_INVALID, "components = %d outside 1 .. %d", components, cmax);
    if (!(tol >= 0.0) || !(tol < 1.0)) return fail(MVS_E_INVALID, "tol = %g outside [0, 1)", tol);
    if (max_iters < 1) return fail(MVS_E_INVALID, "max_iters = %d < 1", max_iters);
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    Range mark(c, "mvs_pcoa_fit");
    HIP_TRY(hipSetDevice(c->device));
    reset_stats(c);
    const int cc = components, block = (int)std::min<int64_t>(m, cc + 8);
    const double dm = (double)m;

    DevBuf dnorms, dXp, dZ;
    const double* d_n2 = nullptr;
    if (const int rc = norms_on_device(c, norms_sq, mem_norms, s->n, dnorms, &d_n2)) return rc;
    Applier ap;
    if (const int rc = ap.init(c, s, d_n2, floor, fb, fe, m)) return rc;
    HIP_TRY(dXp.alloc(padded_doubles(m, block) * 8));
    HIP_TRY(dZ.alloc((size_t)m * block * 8));
    std::unique_ptr<mvs_pcoa> p(new (std::nothrow) mvs_pcoa());
    if (!p) return fail(MVS_E_NOMEM, "out of host memory");
    p->ctx = c;
    p->set = s;
    p->set_id = s->id;
    p->fb = fb, p->fe = fe, p->m = m;
    p->c = cc, p->block = block;
    p->floor = floor;

    // ---- the row means of K: one pass against a column of ones ----
    std::vector<double> padded, Z((size_t)m * block), Yh((size_t)m * block);
    {
        const std::vector<double> ones((size_t)m, 1.0);
        pad_on_host(ones.data(), m, 1, padded);
        HIP_TRY(hipMemcpyAsync(dXp.p, padded.data(), padded.size() * 8, hipMemcpyHostToDevice, c->stream));
        if (const int rc = ap.run(fb, fe, (const double*)dXp.p, 1, (double*)dZ.p)) return rc;
        p->rowmean.resize((size_t)m);
        HIP_TRY(hipMemcpyAsync(p->rowmean.data(), dZ.p, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        double sum = 0.0;
        for (int64_t i = 0; i < m; ++i) {
            p->rowmean[(size_t)i] /= dm;
            sum += p->rowmean[(size_t)i];
        }
        p->grand = sum / dm;
        p->trace = 0.5 * dm * (1.0 - p->grand);
    }

    // ---- leading eigenpairs of B = 1/2 H K H ----
    const int cp = mvs::apply_padded_b(block);
    padded.assign(padded_doubles(m, block), 0.0);
    std::vector<double> mean((size_t)block);
    const SubspaceOp product = [&](const double* q, const double*, double* d_Y) -> int {
        mean.assign((size_t)block, 0.0);
        for (int64_t i = 0; i < m; ++i)
            for (int j = 0; j < block; ++j) mean[(size_t)j] += q[(size_t)i * block + j];
        for (int j = 0; j < block; ++j) mean[(size_t)j] /= dm;
        for (int64_t i = 0; i < m; ++i)
            for (int j = 0; j < block; ++j) padded[(size_t)i * cp + j] = q[(size_t)i * block + j] - mean[(size_t)j];
        HIP_TRY(hipMemcpyAsync(dXp.p, padded.data(), padded.size() * 8, hipMemcpyHostToDevice, c->stream));
        if (const int rc = ap.run(fb, fe, (const double*)dXp.p, block, (double*)dZ.p)) return rc;
        HIP_TRY(hipMemcpyAsync(Z.data(), dZ.p, Z.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        mean.assign((size_t)block, 0.0);
        for (int64_t i = 0; i < m; ++i)
            for (int j = 0; j < block; ++j) mean[(size_t)j] += Z[(size_t)i * block + j];
        for (int j = 0; j < block; ++j) mean[(size_t)j] /= dm;
        for (int64_t i = 0; i < m; ++i)
            for (int j = 0; j < block; ++j) Yh[(size_t)i * block + j] = 0.5 * (Z[(size_t)i * block + j] - mean[(size_t)j]);
        HIP_TRY(hipMemcpyAsync(d_Y, Yh.data(), Yh.size() * 8, hipMemcpyHostToDevice, c->stream));
        return MVS_OK;
    };
    SubspaceResult sr;
    if (const int rc = subspace_iterate(c, (int)m, block, cc, tol, max_iters, product, sr)) return rc;
    c->po_eigen_ms = sr.ms;
    p->iterations = sr.iterations;
    p->converged = sr.converged;
    for (int j = 0; j < block; ++j) p->negative += sr.theta[(size_t)j] < 0.0;

    // ---- vectors (unit length, the entry of largest magnitude positive), coordinates, what the transform needs ----
    p->lambda.assign(sr.theta.begin(), sr.theta.begin() + cc);
    p->residuals.assign(sr.res.begin(), sr.res.begin() + cc);
    p->vectors.resize((size_t)m * cc);
    p->coords.resize((size_t)m * cc);
    p->off.assign((size_t)cc, 0.0);
    std::vector<double> col((size_t)m);
    for (int j = 0; j < cc; ++j) {
        signed_unit_column(sr.V.data(), m, block, j, col.data());
        const double root = std::sqrt(std::max(p->lambda[(size_t)j], 0.0));
        for (int64_t i = 0; i < m; ++i) {
            p->vectors[(size_t)i * cc + j] = col[(size_t)i];
            p->coords[(size_t)i * cc + j] = root * col[(size_t)i];
            p->off[(size_t)j] += p->rowmean[(size_t)i] * col[(size_t)i];
        }
    }
    pad_on_host(p->vectors.data(), m, cc, padded);
    if (p->d_Vp.alloc(padded.size() * 8) != hipSuccess) return fail(MVS_E_NOMEM, "out of device memory");
    const hipError_t e1 = hipMemcpyAsync(p->d_Vp.p, padded.data(), padded.size() * 8, hipMemcpyHostToDevice, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(MVS_E_HIP, "uploading the vectors: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    *out = p.release();
    return MVS_OK;
}

int mvs_pcoa_info(const mvs_pcoa* p, int64_t* row_begin, int64_t* row_end, int* components, int* block, int* iterations, int* converged,
                  int* negative_ritz, double* floor, double* grand_mean, double* trace) {
    if (!p) return fail(MVS_E_INVALID, "NULL pcoa");
    if (row_begin) *row_begin = p->fb;
    if (row_end) *row_end = p->fe;
    if (components) *components = p->c;
    if (block) *block = p->block;
    if (iterations) *iterations = p->iterations;
    if (converged) *converged = p->converged;
    if (negative_ritz) *negative_ritz = p->negative;
    if (floor) *floor = p->floor;
    if (grand_mean) *grand_mean = p->grand;
    if (trace) *trace = p->trace;
    return MVS_OK;
}

int mvs_pcoa_get(const mvs_pcoa* p, double* eigenvalues, double* vectors, double* coordinates, double* row_means, double* residuals) {
    if (!p) return fail(MVS_E_INVALID, "NULL pcoa");
    if (eigenvalues) std::memcpy(eigenvalues, p->lambda.data(), p->lambda.size() * 8);
    if (vectors) std::memcpy(vectors, p->vectors.data(), p->vectors.size() * 8);
    if (coordinates) std::memcpy(coordinates, p->coords.data(), p->coords.size() * 8);
    if (row_means) std::memcpy(row_means, p->rowmean.data(), p->rowmean.size() * 8);
    if (residuals) std::memcpy(residuals, p->residuals.data(), p->residuals.size() * 8);
    return MVS_OK;
}

int mvs_pcoa_transform(mvs_ctx* c, const mvs_pcoa* p, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, int64_t rb, int64_t re,
                       double* scores, int mem_out) {
    if (!c || !p || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (p->ctx != c) return fail(MVS_E_INVALID, "the pcoa belongs to another context");
    if (s != p->set || s->id != p->set_id) return fail(MVS_E_INVALID, "the pcoa was fitted on another sketch set");
    if (!mem_ok(mem_norms) || !mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (rb < 0 || re > s->n || rb > re) return fail(MVS_E_INVALID, "rows [%lld, %lld) outside the set's %lld samples", (long long)rb, (long long)re, (long long)s->n);
    const int64_t rows = re - rb;
    if (rows == 0) return MVS_OK;
    if (!scores) return fail(MVS_E_INVALID, "scores is NULL");
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    Range mark(c, "mvs_pcoa_transform");
    HIP_TRY(hipSetDevice(c->device));
    reset_stats(c);
    const int cc = p->c;
    DevBuf dnorms, dY;
    const double* d_n2 = nullptr;
    if (const int rc = norms_on_device(c, norms_sq, mem_norms, s->n, dnorms, &d_n2)) return rc;
    const size_t bytes = (size_t)rows * cc * 8;
    HIP_TRY(dY.alloc(bytes));
    Applier ap;
    if (const int rc = ap.init(c, s, d_n2, p->floor, p->fb, p->fe, rows)) return rc;
    if (const int rc = ap.run(rb, re, p->d_Vp.as<const double>(), cc, (double*)dY.p)) return rc;
    std::vector<double> y((size_t)rows * cc);
    HIP_TRY(hipMemcpyAsync(y.data(), dY.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    double* dst = mem_out == MVS_MEM_HOST ? scores : y.data();
    for (int j = 0; j < cc; ++j) {
        const double lam = p->lambda[(size_t)j], root = std::sqrt(lam > 0.0 ? lam : 0.0), off = p->off[(size_t)j];
        for (int64_t i = 0; i < rows; ++i) {
            const size_t at = (size_t)i * cc + j;
            dst[at] = lam > 0.0 ? (0.5 * (y[at] - off)) / root : 0.0;
        }
    }
    if (mem_out == MVS_MEM_DEVICE) {
        HIP_TRY(hipMemcpyAsync(scores, y.data(), bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return MVS_OK;
}

int mvs_pcoa_destroy(mvs_pcoa* p) {
    if (!p) return MVS_OK;
    delete p;
    return MVS_OK;
}

int mvs_ctx_pcoa_stats(const mvs_ctx* c, double* dots_ms, double* apply_ms, double* eigen_ms, int64_t* passes, int64_t* row_blocks,
                       int64_t* block_rows) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (eigen_ms) *eigen_ms = c->po_eigen_ms;
    if (passes) *passes = c->po_passes;
    return dots_stats_out(c, &mvs_ctx::po, dots_ms, apply_ms, row_blocks, block_rows);
}

}  // extern "C"
