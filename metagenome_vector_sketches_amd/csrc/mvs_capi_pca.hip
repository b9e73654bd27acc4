// mvs_capi_pca.hip -- C ABI of the ordination: mvs_sketch_moments, mvs_pca_fit / _info / _get / _transform / _destroy,
// mvs_ctx_pca_stats.  The kernels and the argument for the moments' exactness are in mvs_gram.hip.
//
// Fit.  The moments of the row range (exact integers) -> the covariance on the host, its numerators formed in 128-bit integers
// and rounded once -> block subspace iteration with a Rayleigh-Ritz step for the leading eigenpairs.  A block of
// b = min(d, components + 8) columns; per iteration
//     Y = C Q                      device (k_pca_matmul), Q orthonormal
//     T = Q^T Y, symmetrised       host, b x b
//     T = S diag(theta) S^T        host, cyclic Jacobi, theta descending
//     V = Q S, W = Y S = C V, R = W - V diag(theta), res_i = ||R_i||      device (k_pca_ritz, k_pca_resnorm)
//     stop when max_{i < components} res_i <= tol * theta_1, or after max_iters; else Q = orth(W)    host, Gram-Schmidt twice
// W = C V is the power step applied to the Ritz vectors, so one d x d x b product per iteration serves both the Rayleigh
// quotient and the next block.  Everything is a fixed function of the integers: the start block comes from splitmix64 of
// (row, column), every sum runs in a fixed order on one host thread or one device thread, nothing uses floating-point atomics.
// The loop is subspace_iterate (declared in mvs_capi_internal.h): it takes the product as a callable, and mvs_pcoa_fit
// (mvs_capi_pcoa.hip) runs it on B = 1/2 H K H of the Jaccard kernel instead of C.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

#include <cmath>

using namespace mvs_capi;

struct mvs_pca {
    mvs_ctx* ctx = nullptr;
    int d = 0, c = 0;
    int64_t n = 0;
    int iterations = 0, converged = 0;
    double total_variance = 0.0;
    std::vector<double> mean, axes, variances, residuals;   // axes: c x d, one axis per row
    DevBuf d_V;     // d x c, row-major: what k_pca_scores reads
    DevBuf d_off;   // c: sum_a mean[a] V[a][j]
};

namespace {

// the largest magnitude a limb code can hold
double limb_bound(int code) {
    if (mvs::is_k3(code)) return 8127.0;
    switch (code) {
        case 1: return 127.0;
        case 2: return 32639.0;
        case 3: return 8388608.0;
        default: return 2147483648.0;
    }
}

// gram (d x d) and col_sums (d) of rows [rb, re) into zeroed-here device buffers; queued on the context's stream
int moments_on_device(mvs_ctx* c, const mvs_sketch_set* s, int64_t rb, int64_t re, unsigned long long* d_gram, unsigned long long* d_sums,
                      DevBuf& scratch) {
    const int d = s->d;
    int64_t slab = (c->opt.gram_slab_rows / 64) * 64;
    slab = std::max<int64_t>(64, std::min<int64_t>(slab, 65536));
    slab = std::min<int64_t>(slab, (re - rb + 63) / 64 * 64);
    HIP_TRY(scratch.alloc(mvs::gram_scratch_bytes(d, s->limbs, slab)));
    HIP_TRY(hipMemsetAsync(d_gram, 0, (size_t)d * d * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemsetAsync(d_sums, 0, (size_t)d * sizeof(unsigned long long), c->stream));
    StageTimer timer;
    if (const int rc = timer.begin(c)) return rc;
    c->pc_slabs = 0;
    for (int64_t r0 = rb; r0 < re; r0 += slab) {
        const int rc = mvs::launch_gram_slab(c->stream, s->planes, s->limbs, d, s->d_pad, r0, std::min(r0 + slab, re), (int8_t*)scratch.p, d_gram,
                                             c->opt.gram_variant);
        if (rc) return fail(rc, "moments: slab launch rejected");
        if (const int ck = check_kernel("k_gram_tiles")) return ck;
        ++c->pc_slabs;
    }
    {
        const int rc = mvs::launch_gram_colsums(c->stream, s->planes, s->limbs, d, s->d_pad, rb, re, d_sums);
        if (rc) return fail(rc, "moments: column sums launch rejected");
        if (const int ck = check_kernel("k_gram_colsums")) return ck;
    }
    if (const int rc = timer.mark_end()) return rc;
    c->pc_gram_ms = 0.0;
    return timer.add_to(&c->pc_gram_ms);
}

int moments_checks(const mvs_ctx* c, const mvs_sketch_set* s, int64_t rb, int64_t re) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (rb < 0 || re > s->n || rb > re) return fail(MVS_E_INVALID, "rows [%lld, %lld) outside the set's %lld samples", (long long)rb, (long long)re, (long long)s->n);
    if (re - rb < 1) return fail(MVS_E_INVALID, "the row range is empty");
    const double B = limb_bound(s->limbs);
    const unsigned __int128 need = (unsigned __int128)(re - rb) * (unsigned __int128)(B * B);
    if (need > ((unsigned __int128)1 << 62))
        return fail(MVS_E_RANGE, "%lld samples of magnitude up to %.0f: a moment may pass 2^62", (long long)(re - rb), B);
    return MVS_OK;
}

inline uint64_t splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// the columns of q (b columns of d, column j at q + j * d) made orthonormal in place: Gram-Schmidt against the earlier columns,
// twice; a column that vanishes (the block's span is deficient) is replaced by the next unit vector not tried yet
void orthonormalise(std::vector<double>& q, int d, int b) {
    int next_unit = 0;
    for (int j = 0; j < b; ++j) {
        double* x = q.data() + (size_t)j * d;
        for (int attempt = 0; attempt <= d; ++attempt) {
            double before = 0.0;
            for (int a = 0; a < d; ++a) before += x[a] * x[a];
            for (int pass = 0; pass < 2; ++pass)
                for (int i = 0; i < j; ++i) {
                    const double* y = q.data() + (size_t)i * d;
                    double dot = 0.0;
                    for (int a = 0; a < d; ++a) dot += y[a] * x[a];
                    for (int a = 0; a < d; ++a) x[a] -= dot * y[a];
                }
            double after = 0.0;
            for (int a = 0; a < d; ++a) after += x[a] * x[a];
            if (after > 0.0 && after >= before * 1e-24) {
                const double inv = 1.0 / std::sqrt(after);
                for (int a = 0; a < d; ++a) x[a] *= inv;
                break;
            }
            for (int a = 0; a < d; ++a) x[a] = 0.0;
            x[next_unit++ % d] = 1.0;
        }
    }
}

// cyclic Jacobi on the symmetric b x b matrix t (destroyed): theta descending, S[j * b + i] = component j of eigenvector i
void jacobi_eigen(std::vector<double>& t, int b, std::vector<double>& theta, std::vector<double>& S) {
    std::vector<double> v((size_t)b * b, 0.0);
    for (int i = 0; i < b; ++i) v[(size_t)i * b + i] = 1.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < b; ++p) {
            diag += t[(size_t)p * b + p] * t[(size_t)p * b + p];
            for (int q = p + 1; q < b; ++q) off += t[(size_t)p * b + q] * t[(size_t)p * b + q];
        }
        if (off == 0.0 || off <= 1e-40 * diag) break;
        for (int p = 0; p < b; ++p)
            for (int q = p + 1; q < b; ++q) {
                const double apq = t[(size_t)p * b + q];
                if (apq == 0.0) continue;
                const double tau = (t[(size_t)q * b + q] - t[(size_t)p * b + p]) / (2.0 * apq);
                const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(tau * tau + 1.0));
                const double cs = 1.0 / std::sqrt(tt * tt + 1.0), sn = tt * cs;
                for (int k = 0; k < b; ++k) {                      // columns p, q
                    const double kp = t[(size_t)k * b + p], kq = t[(size_t)k * b + q];
                    t[(size_t)k * b + p] = cs * kp - sn * kq;
                    t[(size_t)k * b + q] = sn * kp + cs * kq;
                }
                for (int k = 0; k < b; ++k) {                      // rows p, q
                    const double pk = t[(size_t)p * b + k], qk = t[(size_t)q * b + k];
                    t[(size_t)p * b + k] = cs * pk - sn * qk;
                    t[(size_t)q * b + k] = sn * pk + cs * qk;
                }
                for (int k = 0; k < b; ++k) {
                    const double kp = v[(size_t)k * b + p], kq = v[(size_t)k * b + q];
                    v[(size_t)k * b + p] = cs * kp - sn * kq;
                    v[(size_t)k * b + q] = sn * kp + cs * kq;
                }
            }
    }
    std::vector<int> order(b);
    for (int i = 0; i < b; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return t[(size_t)x * b + x] > t[(size_t)y * b + y]; });
    theta.resize(b);
    S.resize((size_t)b * b);
    for (int i = 0; i < b; ++i) {
        theta[i] = t[(size_t)order[i] * b + order[i]];
        for (int j = 0; j < b; ++j) S[(size_t)j * b + i] = v[(size_t)j * b + order[i]];
    }
}

}  // namespace

namespace mvs_capi {

int subspace_iterate(mvs_ctx* c, int d, int b, int components, double tol, int max_iters, const SubspaceOp& op, SubspaceResult& out) {
    DevBuf dQ, dY, dS, dTheta, dV, dW, dR, dRes;
    const size_t db = (size_t)d * b * 8;
    HIP_TRY(dQ.alloc(db));
    HIP_TRY(dY.alloc(db));
    HIP_TRY(dV.alloc(db));
    HIP_TRY(dW.alloc(db));
    HIP_TRY(dR.alloc(db));
    HIP_TRY(dS.alloc((size_t)b * b * 8));
    HIP_TRY(dTheta.alloc((size_t)b * 8));
    HIP_TRY(dRes.alloc((size_t)b * 8));
    StageTimer timer;
    if (const int rc = timer.begin(c)) return rc;
    std::vector<double> q((size_t)b * d), rowmajor((size_t)d * b), Y((size_t)d * b), W((size_t)d * b), T, S;
    std::vector<double>&V = out.V, &theta = out.theta, &res = out.res;
    V.assign((size_t)d * b, 0.0);
    res.assign((size_t)b, 0.0);
    for (int j = 0; j < b; ++j)
        for (int a = 0; a < d; ++a)
            q[(size_t)j * d + a] = (double)(splitmix64(((uint64_t)a << 20) + (uint64_t)j) >> 11) * 0x1p-53 - 0.5;
    orthonormalise(q, d, b);
    int iters = 0, converged = 0;
    while (true) {
        for (int a = 0; a < d; ++a)
            for (int j = 0; j < b; ++j) rowmajor[(size_t)a * b + j] = q[(size_t)j * d + a];
        HIP_TRY(hipMemcpyAsync(dQ.p, rowmajor.data(), db, hipMemcpyHostToDevice, c->stream));
        if (const int rc = op(rowmajor.data(), (const double*)dQ.p, (double*)dY.p)) return rc;
        HIP_TRY(hipMemcpyAsync(Y.data(), dY.p, db, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        T.assign((size_t)b * b, 0.0);
        for (int a = 0; a < d; ++a)
            for (int i = 0; i < b; ++i) {
                const double qi = rowmajor[(size_t)a * b + i];
                for (int j = 0; j < b; ++j) T[(size_t)i * b + j] += qi * Y[(size_t)a * b + j];
            }
        for (int i = 0; i < b; ++i)
            for (int j = i + 1; j < b; ++j) T[(size_t)i * b + j] = T[(size_t)j * b + i] = 0.5 * (T[(size_t)i * b + j] + T[(size_t)j * b + i]);
        jacobi_eigen(T, b, theta, S);
        HIP_TRY(hipMemcpyAsync(dS.p, S.data(), (size_t)b * b * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(dTheta.p, theta.data(), (size_t)b * 8, hipMemcpyHostToDevice, c->stream));
        if (const int rc = mvs::launch_pca_ritz(c->stream, (const double*)dQ.p, (const double*)dY.p, (const double*)dS.p, (const double*)dTheta.p, d, b,
                                                (double*)dV.p, (double*)dW.p, (double*)dR.p, (double*)dRes.p))
            return fail(rc, "eigensolver: Ritz launch rejected");
        if (const int ck = check_kernel("k_pca_ritz")) return ck;
        HIP_TRY(hipMemcpyAsync(V.data(), dV.p, db, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(W.data(), dW.p, db, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(res.data(), dRes.p, (size_t)b * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ++iters;
        double worst = 0.0;
        bool finite = true;
        for (int i = 0; i < components; ++i) {
            worst = std::max(worst, res[(size_t)i]);
            finite = finite && std::isfinite(res[(size_t)i]);
        }
        converged = finite && worst <= tol * theta[0];
        if (converged || iters >= max_iters) break;
        for (int j = 0; j < b; ++j)
            for (int a = 0; a < d; ++a) q[(size_t)j * d + a] = W[(size_t)a * b + j];
        orthonormalise(q, d, b);
    }
    if (const int rc = timer.mark_end()) return rc;
    out.ms = 0.0;
    if (const int rc = timer.add_to(&out.ms)) return rc;
    out.iterations = iters;
    out.converged = converged;
    return MVS_OK;
}

void signed_unit_column(const double* v, int64_t d, int ld, int j, double* out) {
    double norm2 = 0.0;
    for (int64_t a = 0; a < d; ++a) {
        out[a] = v[(size_t)a * ld + j];
        norm2 += out[a] * out[a];
    }
    int64_t big = 0;
    for (int64_t a = 1; a < d; ++a)
        if (std::fabs(out[a]) > std::fabs(out[big])) big = a;
    const double scale = (norm2 > 0.0 ? 1.0 / std::sqrt(norm2) : 1.0) * (out[big] < 0.0 ? -1.0 : 1.0);
    for (int64_t a = 0; a < d; ++a) out[a] *= scale;
}

}  // namespace mvs_capi

extern "C" {

int mvs_sketch_moments(mvs_ctx* c, const mvs_sketch_set* s, int64_t rb, int64_t re, int64_t* gram, int64_t* col_sums, int mem_out) {
    if (const int rc = moments_checks(c, s, rb, re)) return rc;
    if (!gram || !col_sums) return fail(MVS_E_INVALID, "NULL output");
    if (!mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    Range mark(c, "mvs_sketch_moments");
    HIP_TRY(hipSetDevice(c->device));
    const size_t d = (size_t)s->d;
    DevBuf dgram, dsums, scratch;
    unsigned long long* g = (unsigned long long*)gram;
    unsigned long long* cs = (unsigned long long*)col_sums;
    if (mem_out == MVS_MEM_HOST) {
        HIP_TRY(dgram.alloc(d * d * 8));
        HIP_TRY(dsums.alloc(d * 8));
        g = (unsigned long long*)dgram.p;
        cs = (unsigned long long*)dsums.p;
    }
    if (const int rc = moments_on_device(c, s, rb, re, g, cs, scratch)) return rc;
    if (mem_out == MVS_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(gram, g, d * d * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(col_sums, cs, d * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));                    // (also before the DevBufs free the scratch)
    return MVS_OK;
}

int mvs_pca_fit(mvs_ctx* c, const mvs_sketch_set* s, int64_t rb, int64_t re, int components, double tol, int max_iters, mvs_pca** out) {
    if (!out) return fail(MVS_E_INVALID, "NULL output");
    *out = nullptr;
    if (const int rc = moments_checks(c, s, rb, re)) return rc;
    const int d = s->d;
    const int64_t n = re - rb;
    if (n < 2) return fail(MVS_E_INVALID, "a covariance needs at least two samples");
    if (components < 1 || components > std::min(64, d)) return fail(MVS_E_INVALID, "components = %d outside 1 .. %d", components, std::min(64, d));
    if (!(tol >= 0.0) || !(tol < 1.0)) return fail(MVS_E_INVALID, "tol = %g outside [0, 1)", tol);
    if (max_iters < 1) return fail(MVS_E_INVALID, "max_iters = %d < 1", max_iters);
    Range mark(c, "mvs_pca_fit");
    HIP_TRY(hipSetDevice(c->device));
    const size_t dd = (size_t)d * d;
    const int b = std::min(d, components + 8);
    c->pc_eigen_ms = 0.0;
    c->pc_iters = 0;

    // ---- moments, then the covariance on the host ----
    std::vector<int64_t> gram(dd), sums((size_t)d);
    DevBuf dC;                                                   // the Gram matrix first, the covariance after
    {
        DevBuf dsums, scratch;
        HIP_TRY(dC.alloc(dd * 8));
        HIP_TRY(dsums.alloc((size_t)d * 8));
        if (const int rc = moments_on_device(c, s, rb, re, (unsigned long long*)dC.p, (unsigned long long*)dsums.p, scratch)) return rc;
        HIP_TRY(hipMemcpyAsync(gram.data(), dC.p, dd * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(sums.data(), dsums.p, (size_t)d * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    std::unique_ptr<mvs_pca> p(new (std::nothrow) mvs_pca());
    if (!p) return fail(MVS_E_NOMEM, "out of host memory");
    p->ctx = c;
    p->d = d;
    p->c = components;
    p->n = n;
    p->mean.resize((size_t)d);
    std::vector<double> C(dd);
    const double denom = (double)n * (double)(n - 1);
    for (int a = 0; a < d; ++a) {
        p->mean[(size_t)a] = (double)sums[(size_t)a] / (double)n;
        for (int k = a; k < d; ++k) {
            const __int128 num = (__int128)n * (__int128)gram[(size_t)a * d + k] - (__int128)sums[(size_t)a] * (__int128)sums[(size_t)k];
            const double v = (double)num / denom;
            C[(size_t)a * d + k] = v;
            C[(size_t)k * d + a] = v;
        }
    }
    double total = 0.0;
    for (int a = 0; a < d; ++a) total += C[(size_t)a * d + a];
    p->total_variance = total;
    std::vector<int64_t>().swap(gram);

    // ---- leading eigenpairs ----
    HIP_TRY(hipMemcpyAsync(dC.p, C.data(), dd * 8, hipMemcpyHostToDevice, c->stream));
    SubspaceResult sr;
    const SubspaceOp product = [&](const double*, const double* d_Q, double* d_Y) -> int {
        if (const int rc = mvs::launch_pca_matmul(c->stream, (const double*)dC.p, d_Q, d, b, d_Y)) return fail(rc, "pca: product launch rejected");
        return check_kernel("k_pca_matmul");
    };
    if (const int rc = subspace_iterate(c, d, b, components, tol, max_iters, product, sr)) return rc;
    c->pc_eigen_ms = sr.ms;
    c->pc_iters = sr.iterations;
    p->iterations = sr.iterations;
    p->converged = sr.converged;
    const std::vector<double>&theta = sr.theta, &res = sr.res;

    // ---- the axes: unit length, the entry of largest magnitude (the smaller index on ties) positive ----
    const int cc = components;
    p->axes.resize((size_t)cc * d);
    p->variances.assign(theta.begin(), theta.begin() + cc);
    p->residuals.assign(res.begin(), res.begin() + cc);
    std::vector<double> vc((size_t)d * cc), off((size_t)cc, 0.0);
    for (int j = 0; j < cc; ++j) {
        double* ax = p->axes.data() + (size_t)j * d;
        signed_unit_column(sr.V.data(), d, b, j, ax);
        for (int a = 0; a < d; ++a) {
            vc[(size_t)a * cc + j] = ax[a];
            off[(size_t)j] += p->mean[(size_t)a] * ax[a];
        }
    }
    if (p->d_V.alloc((size_t)d * cc * 8) != hipSuccess || p->d_off.alloc((size_t)cc * 8) != hipSuccess)
        return fail(MVS_E_NOMEM, "out of device memory");
    HIP_TRY(hipMemcpyAsync(p->d_V.p, vc.data(), (size_t)d * cc * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(p->d_off.p, off.data(), (size_t)cc * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = p.release();
    return MVS_OK;
}

int mvs_pca_info(const mvs_pca* p, int* d, int* components, int64_t* n, int* iterations, int* converged, double* total_variance) {
    if (!p) return fail(MVS_E_INVALID, "NULL pca");
    if (d) *d = p->d;
    if (components) *components = p->c;
    if (n) *n = p->n;
    if (iterations) *iterations = p->iterations;
    if (converged) *converged = p->converged;
    if (total_variance) *total_variance = p->total_variance;
    return MVS_OK;
}

int mvs_pca_get(const mvs_pca* p, double* mean, double* axes, double* variances, double* residuals) {
    if (!p) return fail(MVS_E_INVALID, "NULL pca");
    if (mean) std::memcpy(mean, p->mean.data(), p->mean.size() * 8);
    if (axes) std::memcpy(axes, p->axes.data(), p->axes.size() * 8);
    if (variances) std::memcpy(variances, p->variances.data(), p->variances.size() * 8);
    if (residuals) std::memcpy(residuals, p->residuals.data(), p->residuals.size() * 8);
    return MVS_OK;
}

int mvs_pca_transform(mvs_ctx* c, const mvs_pca* p, const mvs_sketch_set* s, int64_t rb, int64_t re, double* scores, int mem_out) {
    if (!c || !p || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (p->ctx != c) return fail(MVS_E_INVALID, "the pca belongs to another context");
    if (s->d != p->d) return fail(MVS_E_INVALID, "the set has dimension %d, the pca %d", s->d, p->d);
    if (!mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (rb < 0 || re > s->n || rb > re) return fail(MVS_E_INVALID, "rows [%lld, %lld) outside the set's %lld samples", (long long)rb, (long long)re, (long long)s->n);
    c->pc_scores_ms = 0.0;
    const int64_t rows = re - rb;
    if (rows == 0) return MVS_OK;
    if (!scores) return fail(MVS_E_INVALID, "scores is NULL");
    Range mark(c, "mvs_pca_transform");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf stage;
    double* d_scores = scores;
    const size_t bytes = (size_t)rows * p->c * 8;
    if (mem_out == MVS_MEM_HOST) {
        HIP_TRY(stage.alloc(bytes));
        d_scores = (double*)stage.p;
    }
    StageTimer timer;
    if (const int rc = timer.begin(c)) return rc;
    if (const int rc = mvs::launch_pca_scores(c->stream, s->planes, s->limbs, s->d, s->d_pad, rb, re, p->d_V.as<const double>(), p->d_off.as<const double>(),
                                              p->c, d_scores))
        return fail(rc, "pca: scores launch rejected");
    if (const int ck = check_kernel("k_pca_scores")) return ck;
    if (const int rc = timer.mark_end()) return rc;
    if (mem_out == MVS_MEM_HOST) HIP_TRY(hipMemcpyAsync(scores, d_scores, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return timer.add_to(&c->pc_scores_ms);
}

int mvs_pca_destroy(mvs_pca* p) {
    if (!p) return MVS_OK;
    delete p;
    return MVS_OK;
}

int mvs_ctx_pca_stats(const mvs_ctx* c, double* gram_ms, double* eigen_ms, double* scores_ms, int64_t* slabs, int64_t* iterations) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (gram_ms) *gram_ms = c->pc_gram_ms;
    if (eigen_ms) *eigen_ms = c->pc_eigen_ms;
    if (scores_ms) *scores_ms = c->pc_scores_ms;
    if (slabs) *slabs = c->pc_slabs;
    if (iterations) *iterations = c->pc_iters;
    return MVS_OK;
}

}  // extern "C"
