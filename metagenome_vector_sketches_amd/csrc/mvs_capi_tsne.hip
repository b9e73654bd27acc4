// mvs_capi_tsne.hip -- C ABI of the exact t-SNE map: mvs_tsne_create / _add_edges / _add_neighbours / _finish_graph / _edges /
// _set_state / _get_state / _gradient / _run / _kl / _destroy (a graph of integer affinities and the optimiser's state on the
// device), mvs_tsne (top-k, calibration, graph, initial state, schedule, centring in one call) and mvs_ctx_tsne_stats.  The
// kernels are in mvs_tsne.hip; the rule is stated in include/mvs_hip.h "t-SNE".  The graph is built with the community unit's
// sort + sum-by-key and its CSR kernel (mvs_community.h), unchanged.  An iteration is three launches and one clear of the
// integer accumulators, all queued: the host reads nothing back while the optimiser runs.
#include "mvs_capi_internal.h"
#include "mvs_community.h"
#include "mvs_tsne.h"

#include <hip/hip_runtime.h>

#include <cmath>

using namespace mvs_capi;

typedef unsigned long long u64;

struct mvs_tsne_graph {
    mvs_ctx* ctx = nullptr;
    int64_t n = 0;
    // the fed directed entries (row << 32 | col, value): `count` of them, `dead` of those with the key ~0 (self loops)
    DevBuf keys, vals;                       // u64
    int64_t cap = 0, count = 0, dead = 0;
    DevBuf counters;                         // u64
    // the symmetric graph (finish_graph)
    bool built = false;
    int64_t m = 0;
    DevBuf row_ptr;                          // long long
    DevBuf src, col;                         // int32_t
    DevBuf p;                                // double
    u64 S = 0;
    // the optimiser's state and its accumulators
    DevBuf y, vel, gain;                     // double
    DevBuf sums;                             // long long, 5 n + 1 words (mvs::TsneSums)
    DevBuf beta;                             // double, n
};

namespace {

constexpr int64_t kMaxN = 1LL << 21;
constexpr int64_t kTopkCells = 1LL << 24;    // cells of a top-k range kept on the device at a time (256 MiB)

void drop_graph(mvs_tsne_graph* t) {
    for (DevBuf* b : {&t->row_ptr, &t->src, &t->col, &t->p}) b->reset();
    t->built = false;
    t->m = 0;
    t->S = 0;
}

mvs::TsneSums sums_of(const mvs_tsne_graph* t) {
    mvs::TsneSums s;
    s.z_rows = t->sums.as<long long>();
    s.rep = t->sums.as<long long>() + t->n;
    s.att = t->sums.as<long long>() + 3 * t->n;
    s.z = t->sums.as<long long>() + 5 * t->n;
    return s;
}

int ensure_room(mvs_tsne_graph* t, int64_t extra) {
    if (t->count + extra <= t->cap) return MVS_OK;
    const int64_t cap = std::max<int64_t>({2 * t->cap, t->count + extra, 1024});
    DevBuf nk, nv;
    if (nk.alloc((size_t)cap * 8) != hipSuccess || nv.alloc((size_t)cap * 8) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of %lld graph entries failed", (long long)cap);
    mvs_ctx* c = t->ctx;
    if (t->count > 0) {
        HIP_TRY(hipMemcpyAsync(nk.p, t->keys.p, (size_t)t->count * 8, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(nv.p, t->vals.p, (size_t)t->count * 8, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    t->keys = std::move(nk);
    t->vals = std::move(nv);
    t->cap = cap;
    return MVS_OK;
}

bool perplexity_ok(double perplexity) { return perplexity >= 1.0 && perplexity <= (double)mvs::kTsneMaxNeighbours; }

// DEVICE cells (sorted by row, <= 256 per row, no self cells) -> 2 n_cells entries; rows [row0, row0 + rows) get their beta.
// d_c: NULL or n_cells int32 on the device.  *beta_zero += rows left at beta = 0
int consume_neighbours(mvs_tsne_graph* t, const mvs_cell* d_cells, int64_t n_cells, int64_t row0, int64_t rows, const double* d_n2, int d,
                       double perplexity, int32_t* d_c, int64_t* beta_zero) {
    mvs_ctx* c = t->ctx;
    HIP_TRY(hipMemsetAsync(t->counters.as<u64>(), 0, mvs::kTsneCounters * 8, c->stream));
    int rc = mvs::launch_tsne_check_cells(c->stream, d_cells, n_cells, t->n, t->counters.as<u64>());
    if (!rc) rc = check_kernel("k_tsne_check_cells");
    if (rc) return rc;
    u64 back[3] = {0, 0, 0};
    rc = read_back(c, c->stream, {{back, t->counters.as<u64>(), sizeof(back)}});
    if (rc) return rc;
    if (back[0] != 0)
        return fail(MVS_E_RANGE, "%llu cells name a sample outside [0, %lld) or have row == col: nothing was added", back[0], (long long)t->n);
    if (back[1] != 0) return fail(MVS_E_INVALID, "the cell list is not sorted by row: nothing was added");
    if (back[2] != 0) return fail(MVS_E_INVALID, "a row has more than %d cells: nothing was added", mvs::kTsneMaxNeighbours);
    rc = ensure_room(t, 2 * n_cells);
    if (rc) return rc;
    StageTimer timer;
    rc = timer.begin(c);
    if (rc) return rc;
    rc = mvs::launch_tsne_calibrate(c->stream, d_cells, n_cells, row0, rows, d_n2, d, perplexity, t->beta.as<double>(), d_c,
                                    t->keys.as<u64>() + t->count, t->vals.as<u64>() + t->count, t->counters.as<u64>());
    if (rc) return fail(rc, "t-SNE: calibration launch rejected");
    rc = check_kernel("k_tsne_calibrate");
    if (!rc) rc = timer.mark_end();
    if (rc) return rc;
    u64 zero = 0;
    rc = read_back(c, c->stream, {{&zero, t->counters.as<u64>() + 3, 8}});
    if (!rc) rc = timer.add_to(&c->ts.calibrate_ms);
    if (rc) return rc;
    if (beta_zero) *beta_zero += (int64_t)zero;
    if (n_cells > 0) {
        t->count += 2 * n_cells;
        t->built = false;
    }
    return MVS_OK;
}

// one evaluation into the accumulators: repulsion, attraction + the fold of Z
int evaluate(mvs_tsne_graph* t, bool timed) {
    mvs_ctx* c = t->ctx;
    const mvs::TsneSums s = sums_of(t);
    HIP_TRY(hipMemsetAsync(t->sums.as<long long>(), 0, (size_t)(5 * t->n + 1) * 8, c->stream));
    StageTimer tr, ta;
    int rc = timed ? tr.begin(c) : MVS_OK;
    if (rc) return rc;
    int64_t units = 0;
    rc = mvs::launch_tsne_repulse(c->stream, t->y.as<double>(), t->n, c->tsne_slice_cols, s, &units);
    if (rc) return fail(rc, "t-SNE: %lld samples at slices of %d columns are more units than a launch holds", (long long)t->n, c->tsne_slice_cols);
    rc = check_kernel("k_tsne_repulse");
    if (!rc && timed) rc = tr.mark_end();
    if (!rc && timed) rc = ta.begin(c);
    if (rc) return rc;
    rc = mvs::launch_tsne_attract(c->stream, t->y.as<double>(), t->n, t->row_ptr.as<long long>(), t->col.as<int32_t>(), t->p.as<double>(), s);
    if (!rc) rc = check_kernel("k_tsne_attract");
    if (!rc && timed) rc = ta.mark_end();
    if (!rc && timed) rc = tr.add_to(&c->ts.repulse_ms);
    if (!rc && timed) rc = ta.add_to(&c->ts.attract_ms);
    c->ts.units = units;
    return rc;
}

int need_graph(const mvs_tsne_graph* t, const char* what) {
    if (!t) return fail(MVS_E_INVALID, "NULL graph");
    if (!t->built) return fail(MVS_E_INVALID, "%s before mvs_tsne_finish_graph", what);
    return MVS_OK;
}

inline u64 splitmix64(u64 x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

}  // namespace

extern "C" {

int mvs_tsne_create(mvs_ctx* c, int64_t n, mvs_tsne_graph** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n < 1) return fail(MVS_E_INVALID, "n = %lld is below 1", (long long)n);
    if (n > kMaxN) return fail(MVS_E_INVALID, "n = %lld exceeds 2^21: the sum Z of the rows' Z_i >> 20 would leave int64", (long long)n);
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<mvs_tsne_graph> t(new (std::nothrow) mvs_tsne_graph());
    if (!t) return fail(MVS_E_NOMEM, "out of host memory");
    t->ctx = c;
    t->n = n;
    const size_t nn = (size_t)n;
    bool ok = t->counters.alloc(mvs::kTsneCounters * 8) == hipSuccess && t->y.alloc(nn * 16) == hipSuccess &&
              t->vel.alloc(nn * 16) == hipSuccess && t->gain.alloc(nn * 16) == hipSuccess &&
              t->sums.alloc((5 * nn + 1) * 8) == hipSuccess && t->beta.alloc(nn * 8) == hipSuccess;
    if (ok)
        ok = hipMemsetAsync(t->y.as<double>(), 0, nn * 16, c->stream) == hipSuccess && hipMemsetAsync(t->vel.as<double>(), 0, nn * 16,
                                                                                                      c->stream) == hipSuccess &&
            hipMemsetAsync(t->beta.as<double>(), 0, nn * 8, c->stream) == hipSuccess && mvs::launch_tsne_fill(c->stream,
                                                                                                              t->gain.as<double>(), 2 * n,
                                                                                                              1.0) == 0 &&
            hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) return fail(MVS_E_NOMEM, "hipMalloc of the state of %lld samples failed", (long long)n);
    c->ts.reset();
    *out = t.release();
    return MVS_OK;
}

int mvs_tsne_destroy(mvs_tsne_graph* t) {
    if (!t) return MVS_OK;
    if (t->ctx) {
        (void)hipSetDevice(t->ctx->device);
        (void)hipStreamSynchronize(t->ctx->stream);
    }
    delete t;
    return MVS_OK;
}

int mvs_tsne_add_edges(mvs_tsne_graph* t, const int32_t* lo, const int32_t* hi, const int32_t* s, int64_t n_edges, int mem) {
    if (!t) return fail(MVS_E_INVALID, "NULL graph");
    if (n_edges < 0 || !mem_ok(mem) || (n_edges > 0 && (!lo || !hi || !s))) return fail(MVS_E_INVALID, "bad edge list");
    if (n_edges == 0) return MVS_OK;
    mvs_ctx* c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_tsne_add_edges");
    DevBuf stage;
    const int32_t *dlo = lo, *dhi = hi, *ds = s;
    if (mem == MVS_MEM_HOST) {
        HIP_TRY(stage.alloc((size_t)n_edges * 12));
        int32_t* p = (int32_t*)stage.p;
        HIP_TRY(hipMemcpyAsync(p, lo, (size_t)n_edges * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(p + n_edges, hi, (size_t)n_edges * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(p + 2 * n_edges, s, (size_t)n_edges * 4, hipMemcpyHostToDevice, c->stream));
        dlo = p;
        dhi = p + n_edges;
        ds = p + 2 * n_edges;
    }
    HIP_TRY(hipMemsetAsync(t->counters.as<u64>(), 0, mvs::kTsneCounters * 8, c->stream));
    int rc = mvs::launch_tsne_check_edges(c->stream, dlo, dhi, ds, n_edges, t->n, t->counters.as<u64>());
    if (!rc) rc = check_kernel("k_tsne_check_edges");
    if (rc) return rc;
    u64 bad = 0;
    rc = read_back(c, c->stream, {{&bad, t->counters.as<u64>(), 8}});
    if (rc) return rc;
    if (bad != 0)
        return fail(MVS_E_RANGE, "%llu edges name a sample outside [0, %lld) or have a weight below 1: nothing was added", bad, (long long)t->n);
    rc = ensure_room(t, 2 * n_edges);
    if (rc) return rc;
    rc = mvs::launch_tsne_edges(c->stream, dlo, dhi, ds, n_edges, t->keys.as<u64>() + t->count, t->vals.as<u64>() + t->count,
                                t->counters.as<u64>());
    if (!rc) rc = check_kernel("k_tsne_edges");
    if (rc) return rc;
    u64 selfs = 0;
    rc = read_back(c, c->stream, {{&selfs, t->counters.as<u64>() + 1, 8}});     // (also before `stage` is freed)
    if (rc) return rc;
    t->count += 2 * n_edges;
    t->dead += 2 * (int64_t)selfs;
    t->built = false;
    return MVS_OK;
}

int mvs_tsne_add_neighbours(mvs_tsne_graph* t, const mvs_cell* cells, int64_t n_cells, int mem_cells, const double* norms_sq, int mem_norms,
                            int d, double perplexity, double* beta_out, int32_t* c_out) {
    if (!t) return fail(MVS_E_INVALID, "NULL graph");
    if (n_cells < 0 || !mem_ok(mem_cells) || !mem_ok(mem_norms) || (n_cells > 0 && !cells) || !norms_sq || d < 1)
        return fail(MVS_E_INVALID, "bad argument");
    if (!perplexity_ok(perplexity)) return fail(MVS_E_INVALID, "perplexity = %g outside [1, %d]", perplexity, mvs::kTsneMaxNeighbours);
    if (n_cells == 0) return MVS_OK;
    mvs_ctx* c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_tsne_add_neighbours");
    DevBuf dcells, dnorms, dc;
    const mvs_cell* d_cells = cells;
    if (mem_cells == MVS_MEM_HOST) {
        HIP_TRY(dcells.alloc((size_t)n_cells * sizeof(mvs_cell)));
        HIP_TRY(hipMemcpyAsync(dcells.p, cells, (size_t)n_cells * sizeof(mvs_cell), hipMemcpyHostToDevice, c->stream));
        d_cells = (const mvs_cell*)dcells.p;
    }
    const double* d_n2 = nullptr;
    int rc = norms_on_device(c, norms_sq, mem_norms, t->n, dnorms, &d_n2);
    if (rc) return rc;
    if (c_out) HIP_TRY(dc.alloc((size_t)n_cells * 4));
    // the rows between the list's first and last (the check proves the list sorted before anything is used)
    int32_t ends[2] = {0, 0};
    rc = read_back(c, c->stream, {{&ends[0], &d_cells[0].row, 4}, {&ends[1], &d_cells[n_cells - 1].row, 4}});
    if (rc) return rc;
    if (ends[0] < 0 || ends[1] >= t->n || ends[0] > ends[1])
        return fail(MVS_E_RANGE, "the cell list's rows %d .. %d leave [0, %lld) or descend: nothing was added", ends[0], ends[1], (long long)t->n);
    rc = consume_neighbours(t, d_cells, n_cells, ends[0], (int64_t)ends[1] - ends[0] + 1, d_n2, d, perplexity, (int32_t*)dc.p, nullptr);
    if (rc) return rc;
    if (beta_out) HIP_TRY(hipMemcpyAsync(beta_out + ends[0], t->beta.as<double>() + ends[0], (size_t)(ends[1] - ends[0] + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (c_out) HIP_TRY(hipMemcpyAsync(c_out, dc.p, (size_t)n_cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_tsne_finish_graph(mvs_tsne_graph* t) {
    if (!t) return fail(MVS_E_INVALID, "NULL graph");
    if (t->built) return MVS_OK;
    mvs_ctx* c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_tsne_finish_graph");
    drop_graph(t);
    StageTimer timer;
    int rc = timer.begin(c);
    if (rc) return rc;
    int64_t m = 0;
    if (t->count > 0) {
        DevBuf tk, tv;
        HIP_TRY(tk.alloc((size_t)t->count * 8));
        HIP_TRY(tv.alloc((size_t)t->count * 8));
        rc = mvs::comm_sum_by_key(c->stream, t->keys.as<u64>(), t->vals.as<u64>(), t->count, t->count - t->dead, (u64*)tk.p, (u64*)tv.p,
                                  t->counters.as<u64>() + 4);
        if (rc) return fail(rc, "t-SNE: summing the entries by key failed");
        u64 left = 0;
        rc = read_back(c, c->stream, {{&left, t->counters.as<u64>() + 4, 8}});
        if (rc) return rc;
        m = (int64_t)left;
        t->count = m;                                                   // the list stays: one entry per directed pair now
        t->dead = 0;
    }
    const size_t mm = (size_t)std::max<int64_t>(m, 1);
    if (t->row_ptr.alloc(((size_t)t->n + 1) * 8) != hipSuccess || t->src.alloc(mm * 4) != hipSuccess ||
        t->col.alloc(mm * 4) != hipSuccess || t->p.alloc(mm * 8) != hipSuccess) {
        drop_graph(t);
        return fail(MVS_E_NOMEM, "hipMalloc of the graph of %lld entries failed", (long long)m);
    }
    rc = mvs::launch_comm_csr(c->stream, t->keys.as<u64>(), m, t->n, t->row_ptr.as<long long>(), t->src.as<int32_t>(), t->col.as<int32_t>());
    if (!rc) rc = check_kernel("k_comm_csr");
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(t->counters.as<u64>() + 5, 0, 8, c->stream));
    rc = mvs::launch_tsne_total(c->stream, t->vals.as<u64>(), m, t->counters.as<u64>() + 5);
    if (!rc) rc = check_kernel("k_tsne_total");
    if (rc) return rc;
    u64 S = 0;
    rc = read_back(c, c->stream, {{&S, t->counters.as<u64>() + 5, 8}});
    if (rc) return rc;
    rc = mvs::launch_tsne_p(c->stream, t->vals.as<u64>(), m, S, t->p.as<double>());
    if (!rc) rc = check_kernel("k_tsne_p");
    if (!rc) rc = timer.mark_end();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    rc = timer.add_to(&c->ts.graph_ms);
    if (rc) return rc;
    t->m = m;
    t->S = S;
    t->built = true;
    c->ts.edges = m;
    return MVS_OK;
}

int mvs_tsne_edges(mvs_tsne_graph* t, int32_t* row, int32_t* col, int64_t* s, int64_t capacity, int64_t* n_entries, uint64_t* S) {
    if (const int rc = need_graph(t, "mvs_tsne_edges")) return rc;
    if (capacity < 0) return fail(MVS_E_INVALID, "bad argument");
    mvs_ctx* c = t->ctx;
    if (n_entries) *n_entries = t->m;
    if (S) *S = t->S;
    if (!row && !col && !s) return MVS_OK;
    if (capacity < t->m) return fail(MVS_E_CAPACITY, "%lld entries, room for %lld", (long long)t->m, (long long)capacity);
    HIP_TRY(hipSetDevice(c->device));
    int rc = give_out(c, row, t->src.as<int32_t>(), t->m, MVS_MEM_HOST);
    if (!rc) rc = give_out(c, col, t->col.as<int32_t>(), t->m, MVS_MEM_HOST);
    if (!rc) rc = give_out(c, s, t->vals.as<u64>(), t->m, MVS_MEM_HOST);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_tsne_set_state(mvs_tsne_graph* t, const double* y, const double* velocity, const double* gain) {
    if (!t) return fail(MVS_E_INVALID, "NULL graph");
    mvs_ctx* c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)t->n * 16;
    if (y) HIP_TRY(hipMemcpyAsync(t->y.as<double>(), y, bytes, hipMemcpyHostToDevice, c->stream));
    if (velocity) HIP_TRY(hipMemcpyAsync(t->vel.as<double>(), velocity, bytes, hipMemcpyHostToDevice, c->stream));
    if (gain) HIP_TRY(hipMemcpyAsync(t->gain.as<double>(), gain, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_tsne_get_state(mvs_tsne_graph* t, double* y, double* velocity, double* gain) {
    if (!t) return fail(MVS_E_INVALID, "NULL graph");
    mvs_ctx* c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = give_out(c, y, t->y.as<double>(), 2 * t->n, MVS_MEM_HOST);
    if (!rc) rc = give_out(c, velocity, t->vel.as<double>(), 2 * t->n, MVS_MEM_HOST);
    if (!rc) rc = give_out(c, gain, t->gain.as<double>(), 2 * t->n, MVS_MEM_HOST);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_tsne_gradient(mvs_tsne_graph* t, double exaggeration, double* grad, int64_t* z_rows, int64_t* z) {
    if (const int rc = need_graph(t, "mvs_tsne_gradient")) return rc;
    if (!std::isfinite(exaggeration)) return fail(MVS_E_INVALID, "exaggeration = %g", exaggeration);
    mvs_ctx* c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_tsne_gradient");
    int rc = evaluate(t, false);
    if (rc) return rc;
    DevBuf dg;
    HIP_TRY(dg.alloc((size_t)t->n * 16));
    const mvs::TsneSums s = sums_of(t);
    rc = mvs::launch_tsne_update(c->stream, t->n, s, exaggeration, 0.0, 0.0, 0, t->y.as<double>(), t->vel.as<double>(),
                                 t->gain.as<double>(), (double*)dg.p);
    if (!rc) rc = check_kernel("k_tsne_update");
    if (!rc) rc = give_out(c, grad, dg.p, 2 * t->n, MVS_MEM_HOST);
    if (!rc) rc = give_out(c, (long long*)z_rows, s.z_rows, t->n, MVS_MEM_HOST);
    if (!rc) rc = give_out(c, (long long*)z, s.z, 1, MVS_MEM_HOST);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));                         // (also before `dg` is freed)
    return MVS_OK;
}

int mvs_tsne_run(mvs_tsne_graph* t, int64_t iterations, double exaggeration, double momentum, double learning_rate) {
    if (const int rc = need_graph(t, "mvs_tsne_run")) return rc;
    if (iterations < 0 || iterations > (1 << 30)) return fail(MVS_E_INVALID, "iterations = %lld outside [0, 2^30]", (long long)iterations);
    if (!std::isfinite(exaggeration) || !std::isfinite(momentum) || !std::isfinite(learning_rate))
        return fail(MVS_E_INVALID, "exaggeration, momentum and learning rate must be finite");
    mvs_ctx* c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_tsne_run");
    const mvs::TsneSums s = sums_of(t);
    for (int64_t it = 0; it < iterations; ++it) {
        int rc = evaluate(t, true);
        if (rc) return rc;
        StageTimer tu;
        rc = tu.begin(c);
        if (rc) return rc;
        rc = mvs::launch_tsne_update(c->stream, t->n, s, exaggeration, momentum, learning_rate, 1, t->y.as<double>(), t->vel.as<double>(),
                                     t->gain.as<double>(), nullptr);
        if (!rc) rc = check_kernel("k_tsne_update");
        if (!rc) rc = tu.mark_end();
        if (!rc) rc = tu.add_to(&c->ts.update_ms);
        if (rc) return rc;
        ++c->ts.iterations;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_tsne_kl(mvs_tsne_graph* t, double* kl) {
    if (const int rc = need_graph(t, "mvs_tsne_kl")) return rc;
    if (!kl) return fail(MVS_E_INVALID, "NULL argument");
    mvs_ctx* c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = evaluate(t, false);
    if (rc) return rc;
    DevBuf dk;
    HIP_TRY(dk.alloc(8));
    HIP_TRY(hipMemsetAsync(dk.p, 0, 8, c->stream));
    rc = mvs::launch_tsne_kl(c->stream, t->y.as<double>(), t->m, t->src.as<int32_t>(), t->col.as<int32_t>(), t->p.as<double>(), sums_of(t),
                             (double*)dk.p);
    if (!rc) rc = check_kernel("k_tsne_kl");
    if (rc) return rc;
    return read_back(c, c->stream, {{kl, dk.p, 8}});
}

int mvs_tsne(mvs_ctx* c, const mvs_sketch_set* set, const double* norms_sq, int mem_norms, const mvs_tsne_params* params, double* Y, double* Y0,
             double* beta, mvs_tsne_result* result, mvs_tsne_graph** graph_out) {
    if (graph_out) *graph_out = nullptr;
    if (!c || !set || !params || !norms_sq) return fail(MVS_E_INVALID, "NULL argument");
    if (!mem_ok(mem_norms)) return fail(MVS_E_INVALID, "bad argument");
    const mvs_tsne_params& p = *params;
    if (!perplexity_ok(p.perplexity)) return fail(MVS_E_INVALID, "perplexity = %g outside [1, %d]", p.perplexity, mvs::kTsneMaxNeighbours);
    const int64_t K = p.neighbours > 0 ? p.neighbours : (int64_t)std::ceil(3.0 * p.perplexity);
    if (p.neighbours < 0 || K > mvs::kTsneMaxNeighbours)
        return fail(MVS_E_INVALID, "neighbours = %lld outside 1 .. %d (top-k's K; the default 3 x perplexity allows a perplexity of 85)",
                    (long long)K, mvs::kTsneMaxNeighbours);
    if (p.perplexity > (double)K) return fail(MVS_E_INVALID, "perplexity = %g exceeds the %lld neighbours: every row would be uniform", p.perplexity, (long long)K);
    if (p.iterations < 0 || p.exaggeration_iters < 0 || p.iterations > (1 << 30))
        return fail(MVS_E_INVALID, "iterations and exaggeration_iters must be 0 .. 2^30");
    if (!std::isfinite(p.exaggeration) || !(p.exaggeration > 0.0)) return fail(MVS_E_INVALID, "exaggeration = %g is not positive", p.exaggeration);
    if (std::isnan(p.learning_rate) || std::isinf(p.learning_rate)) return fail(MVS_E_INVALID, "learning_rate = %g", p.learning_rate);
    if (p.init != MVS_TSNE_INIT_PCOA && p.init != MVS_TSNE_INIT_RANDOM) return fail(MVS_E_INVALID, "init = %lld: 0 (pcoa) or 1 (random)", (long long)p.init);
    const int64_t n = set->n;
    if (p.init == MVS_TSNE_INIT_PCOA && n < 3) return fail(MVS_E_INVALID, "init pcoa needs two coordinates: at least 3 samples, not %lld", (long long)n);
    mvs_tsne_result r;
    std::memset(&r, 0, sizeof(r));
    r.n = n;
    r.neighbours = K;
    r.learning_rate = p.learning_rate > 0.0 ? p.learning_rate : std::max((double)n / 12.0 / 4.0, 50.0);
    if (result) *result = r;
    mvs_tsne_graph* t = nullptr;
    int rc = mvs_tsne_create(c, n, &t);
    if (rc) return rc;
    struct Guard {
        mvs_tsne_graph* t;
        ~Guard() { mvs_tsne_destroy(t); }
    } guard{t};
    const Range range(c, "mvs_tsne");

    // the initial state first: PCoA's solver owns the device while it runs
    std::vector<double> y0((size_t)n * 2);
    if (p.init == MVS_TSNE_INIT_PCOA) {
        mvs_pcoa* pc = nullptr;
        rc = mvs_pcoa_fit(c, set, norms_sq, mem_norms, 0, n, 2, 0.0, 1e-10, 300, &pc);
        if (rc) return rc;
        rc = mvs_pcoa_get(pc, nullptr, nullptr, y0.data(), nullptr, nullptr);
        mvs_pcoa_destroy(pc);
        if (rc) return rc;
        double sum = 0.0;
        for (int64_t i = 0; i < n; ++i) sum += y0[(size_t)i * 2];
        const double mean = sum / (double)n;
        double ss = 0.0;
        for (int64_t i = 0; i < n; ++i) ss += (y0[(size_t)i * 2] - mean) * (y0[(size_t)i * 2] - mean);
        const double sd = std::sqrt(ss / (double)n);
        if (!(sd > 0.0) || !std::isfinite(sd)) return fail(MVS_E_INVALID, "init pcoa: the first coordinate has standard deviation %g; use init random", sd);
        const double f = 1e-4 / sd;
        for (double& v : y0) v = v * f;
    } else {
        const u64 base = splitmix64((u64)p.seed);
        for (int64_t k = 0; k < 2 * n; ++k) {
            const double u = (double)(splitmix64(base ^ (u64)k) >> 11) * (1.0 / 9007199254740992.0);
            y0[(size_t)k] = (2.0 * u - 1.0) * 1e-4;
        }
    }
    if (Y0) std::copy(y0.begin(), y0.end(), Y0);
    rc = mvs_tsne_set_state(t, y0.data(), nullptr, nullptr);
    if (rc) return rc;

    // top-k over row ranges, each range calibrated where it lies
    {
        DevBuf dnorms, dcells;
        const double* d_n2 = nullptr;
        rc = norms_on_device(c, norms_sq, mem_norms, n, dnorms, &d_n2);
        if (rc) return rc;
        int64_t R = std::max<int64_t>(1, kTopkCells / K);
        if (c->opt.cluster_block_rows > 0) R = std::min<int64_t>(R, c->opt.cluster_block_rows);
        R = std::min(R, n);
        HIP_TRY(dcells.alloc((size_t)R * (size_t)K * sizeof(mvs_cell)));
        for (int64_t r0 = 0; r0 < n; r0 += R) {
            const int64_t r1 = std::min(r0 + R, n);
            int64_t cells = 0;
            rc = mvs_pairwise_topk(c, set, d_n2, MVS_MEM_DEVICE, (int)K, r0, r1, 0, n, MVS_TOPK_EXCLUDE_SELF, (mvs_cell*)dcells.p, MVS_MEM_DEVICE, &cells);
            if (rc) return rc;
            c->ts.topk_ms += c->tk.dots_ms + c->tk.work_ms;
            ++c->ts.blocks;
            if (cells > (r1 - r0) * K) return fail(MVS_E_INTERNAL, "top-k returned %lld cells for %lld rows at k = %lld", (long long)cells, (long long)(r1 - r0), (long long)K);
            rc = consume_neighbours(t, (const mvs_cell*)dcells.p, cells, r0, r1 - r0, d_n2, set->d, p.perplexity, nullptr, &r.beta_zero_rows);
            if (rc) return rc;
        }
        HIP_TRY(hipStreamSynchronize(c->stream));                     // (also before the DevBufs free their arrays)
    }
    rc = mvs_tsne_finish_graph(t);
    if (rc) return rc;
    r.entries = t->m;
    r.S = t->S;
    if (beta) {
        HIP_TRY(hipMemcpyAsync(beta, t->beta.as<double>(), (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }

    // the schedule
    const int64_t first = std::min<int64_t>(p.iterations, p.exaggeration_iters);
    rc = mvs_tsne_run(t, first, p.exaggeration, 0.5, r.learning_rate);
    if (!rc) rc = mvs_tsne_run(t, p.iterations - first, 1.0, 0.8, r.learning_rate);
    if (rc) return rc;
    r.iterations = p.iterations;
    rc = mvs_tsne_kl(t, &r.kl);
    if (rc) return rc;

    // the output, centred once: the mean from integer sums of rint(y * 2^30)
    if (Y) {
        rc = mvs_tsne_get_state(t, Y, nullptr, nullptr);
        if (rc) return rc;
        for (int a = 0; a < 2; ++a) {
            long long total = 0;
            for (int64_t i = 0; i < n; ++i) total += std::llrint(Y[(size_t)i * 2 + a] * 1073741824.0);
            const double mean = ((double)total / 1073741824.0) / (double)n;
            for (int64_t i = 0; i < n; ++i) Y[(size_t)i * 2 + a] = Y[(size_t)i * 2 + a] - mean;
        }
    }
    if (result) *result = r;
    if (graph_out) {
        *graph_out = t;
        guard.t = nullptr;
    }
    return MVS_OK;
}

int mvs_ctx_tsne_stats(const mvs_ctx* c, double* topk_ms, double* calibrate_ms, double* graph_ms, double* repulse_ms, double* attract_ms,
                       double* update_ms, int64_t* iterations, int64_t* entries, int64_t* units, int64_t* row_blocks) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    const TsneStats& st = c->ts;
    if (topk_ms) *topk_ms = st.topk_ms;
    if (calibrate_ms) *calibrate_ms = st.calibrate_ms;
    if (graph_ms) *graph_ms = st.graph_ms;
    if (repulse_ms) *repulse_ms = st.repulse_ms;
    if (attract_ms) *attract_ms = st.attract_ms;
    if (update_ms) *update_ms = st.update_ms;
    if (iterations) *iterations = st.iterations;
    if (entries) *entries = st.edges;
    if (units) *units = st.units;
    if (row_blocks) *row_blocks = st.blocks;
    return MVS_OK;
}

}  // extern "C"
