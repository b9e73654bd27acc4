// mvs_capi_linkage.hip -- C ABI of the single-linkage tree: mvs_linkage_create / _set_core / _add_cells / _finish / _cells / _destroy (a
// consumer of DEVICE cell lists that keeps the maximum spanning forest of everything it was fed), mvs_pairwise_linkage (the
// one-call producer: mvs_pairwise_cluster's row-block loop with this consumer) and mvs_ctx_linkage_stats.  The kernels and the
// argument for their exactness are in mvs_linkage.hip.  What comes back is at most n - 1 links of 24 bytes.
#include "mvs_capi_internal.h"
#include "mvs_core.h"

#include <hip/hip_runtime.h>

using namespace mvs_capi;

struct mvs_linkage {
    mvs_ctx* ctx = nullptr;
    int64_t n = 0;
    int d = 0;
    DevBuf norms_sq;                         // double, the linkage's own copy: every weight comes from it
    DevBuf core;                             // empty, or the core values (double) of mvs_linkage_set_core: the weight is min(J, core, core)
    bool fed = false;                        // a cell has been fed: the weight is fixed from here on
    DevBuf forest[2];                        // mvs_cell: the forest and the one the rounds build; `cur` says which is which
    int cur = 0;
    int64_t n_forest = 0;
    DevBuf comp, next;                       // int32_t
    DevBuf slots;                            // unsigned long long: best_key | best_pair | best_idx, n words each
    DevBuf counters;                         // unsigned long long (mvs_internal.h: LinkState)
    DevBuf links;                            // mvs_link: the forest sorted best first (n_forest entries) while links_valid
    bool links_valid = false;
};

namespace {

constexpr int kMaxRounds = 64;   // Boruvka rounds per list before the call gives up (at most ceil(log2 n) are needed)

mvs::LinkState state_of(const mvs_linkage* k) {
    mvs::LinkState s;
    const size_t words = (size_t)std::max<int64_t>(k->n, 1);
    s.n = k->n;
    s.d = k->d;
    s.norms_sq = k->norms_sq.as<double>();
    s.forest = k->forest[k->cur].as<mvs_cell>();
    s.n_forest = k->n_forest;
    s.forest_next = k->forest[k->cur ^ 1].as<mvs_cell>();
    s.capacity = std::max<int64_t>(k->n - 1, 0);
    s.comp = k->comp.as<int32_t>();
    s.next = k->next.as<int32_t>();
    s.best_key = k->slots.as<unsigned long long>();
    s.best_pair = k->slots.as<unsigned long long>() + words;
    s.best_idx = k->slots.as<unsigned long long>() + 2 * words;
    s.counters = k->counters.as<unsigned long long>();
    return s;
}

// forest := the maximum spanning forest of forest u list; the list is consumed when this returns
int consume_cells(mvs_linkage* k, const mvs_cell* d_cells, int64_t n_cells) {
    mvs_ctx* c = k->ctx;
    if (n_cells == 0) return MVS_OK;
    k->fed = true;
    StageTimer timer;
    int rc = timer.begin(c);
    if (rc) return rc;
    const mvs::LinkState s = state_of(k);
    HIP_TRY(hipMemsetAsync(k->counters.as<unsigned long long>(), 0, 8 * sizeof(unsigned long long), c->stream));
    rc = mvs::launch_link_identity(c->stream, k->comp.as<int32_t>(), k->n);
    if (!rc) rc = check_kernel("k_link_identity");
    if (rc) return rc;
    unsigned long long back[5] = {0, 0, 0, 0, 0};
    int round = 0;
    for (;;) {
        rc = mvs::launch_link_slots(c->stream, s);
        if (!rc) rc = check_kernel("k_link_slots");
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(k->counters.as<unsigned long long>() + 2, 0, sizeof(unsigned long long), c->stream));
        rc = mvs::launch_link_select(c->stream, s, k->core.as<double>(), d_cells, n_cells, 0, round == 0);
        if (!rc) rc = check_kernel("k_link_select<0>");
        if (rc) return rc;
        rc = read_back(c, c->stream, {{back, k->counters.as<unsigned long long>(), sizeof(back)}});
        if (rc) return rc;
        if (back[4] != 0) return fail(MVS_E_HIP, "internal: the forest rounds left their bounds (flag %llu)", back[4]);
        if (back[2] == 0) break;
        if (round >= kMaxRounds)
            return fail(MVS_E_HIP, "internal: %llu edges still join different components after %d rounds", back[2], round);
        ++round;
        for (int pass = 1; pass <= 2 && !rc; ++pass) {
            rc = mvs::launch_link_select(c->stream, s, k->core.as<double>(), d_cells, n_cells, pass, false);
            if (!rc) rc = check_kernel("k_link_select");
        }
        if (!rc) rc = mvs::launch_link_hook(c->stream, s, k->core.as<double>(), d_cells);
        if (!rc) rc = check_kernel("k_link_hook");
        if (!rc) rc = mvs::launch_link_jump(c->stream, s);
        if (!rc) rc = check_kernel("k_link_flatten");
        if (rc) return rc;
    }
    if ((int64_t)back[3] > s.capacity) return fail(MVS_E_HIP, "internal: a forest of %llu edges over %lld samples", back[3], (long long)k->n);
    k->cur ^= 1;
    k->n_forest = (int64_t)back[3];
    k->links_valid = false;
    rc = timer.mark_end();
    if (!rc) rc = timer.add_to(&c->lk.work_ms);
    if (rc) return rc;
    c->lk.edges += (long long)back[0];
    c->lk.rounds = std::max<long long>(c->lk.rounds, round);
    if (back[1] != 0)
        return fail(MVS_E_RANGE, "%llu cells name a sample outside [0, %lld): they were ignored", back[1], (long long)k->n);
    return MVS_OK;
}

// k->links := the forest sorted best first
int sort_links(mvs_linkage* k) {
    if (k->links_valid || k->n_forest == 0) {
        k->links_valid = true;
        return MVS_OK;
    }
    mvs_ctx* c = k->ctx;
    const mvs::LinkState s = state_of(k);
    DevBuf dtmp, dscratch;
    size_t need = 0;
    int rc = mvs::link_sorted(c->stream, s, k->core.as<double>(), nullptr, nullptr, nullptr, 0, &need);
    if (rc) return fail(rc, "linkage finish: sort sizing failed");
    HIP_TRY(dtmp.alloc((size_t)k->n_forest * sizeof(mvs_link)));
    HIP_TRY(dscratch.alloc(need));
    StageTimer timer;
    rc = timer.begin(c);
    if (rc) return rc;
    rc = mvs::link_sorted(c->stream, s, k->core.as<double>(), (mvs_link*)dtmp.p, k->links.as<mvs_link>(), dscratch.p, need, nullptr);
    if (rc) return fail(rc, "linkage finish: sort failed");
    rc = check_kernel("k_link_links");
    if (rc) return rc;
    rc = timer.mark_end();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));   // (also before the DevBufs free the scratch)
    rc = timer.add_to(&c->lk.work_ms);
    if (rc) return rc;
    k->links_valid = true;
    return MVS_OK;
}

}  // namespace

extern "C" {

int mvs_linkage_create(mvs_ctx* c, int64_t n, int d, const double* norms_sq, int mem_norms, mvs_linkage** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n < 0) return fail(MVS_E_INVALID, "n = %lld is negative", (long long)n);
    if (d <= 0) return fail(MVS_E_INVALID, "d = %d is not positive", d);
    if (!mem_ok(mem_norms)) return fail(MVS_E_INVALID, "bad argument");
    if (n > 0 && !norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    if (n >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n too large for int32 sample indices");
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<mvs_linkage> k(new (std::nothrow) mvs_linkage());
    if (!k) return fail(MVS_E_NOMEM, "out of host memory");
    k->ctx = c;
    k->n = n;
    k->d = d;
    const size_t words = (size_t)std::max<int64_t>(n, 1);
    if (k->norms_sq.alloc(words * 8) != hipSuccess || k->forest[0].alloc(words * sizeof(mvs_cell)) != hipSuccess ||
        k->forest[1].alloc(words * sizeof(mvs_cell)) != hipSuccess || k->comp.alloc(words * 4) != hipSuccess ||
        k->next.alloc(words * 4) != hipSuccess || k->slots.alloc(3 * words * 8) != hipSuccess ||
        k->links.alloc(words * sizeof(mvs_link)) != hipSuccess || k->counters.alloc(64) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of the forest of %lld samples failed", (long long)n);
    if (n > 0) {
        const hipError_t e = hipMemcpyAsync(k->norms_sq.as<double>(), norms_sq, (size_t)n * 8,
                                            mem_norms == MVS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream);
        const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
        if (e2 != hipSuccess) return fail(MVS_E_HIP, "copying the norms: %s", hipGetErrorString(e2));
    }
    c->lk.reset();
    *out = k.release();
    return MVS_OK;
}

int mvs_linkage_set_core(mvs_linkage* k, const double* core, int mem_core) {
    if (!k) return fail(MVS_E_INVALID, "NULL linkage");
    if (!mem_ok(mem_core)) return fail(MVS_E_INVALID, "bad argument");
    if (k->n > 0 && !core) return fail(MVS_E_INVALID, "core is NULL");
    if (k->fed) return fail(MVS_E_INVALID, "the linkage has been fed cells: the core values decide every weight and must come first");
    mvs_ctx* c = k->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if (!k->core.p && k->core.alloc((size_t)std::max<int64_t>(k->n, 1) * 8) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of %lld core values failed", (long long)k->n);
    if (k->n > 0) {
        HIP_TRY(hipMemcpyAsync(k->core.as<double>(), core, (size_t)k->n * 8,
                               mem_core == MVS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return MVS_OK;
}

int mvs_linkage_add_cells(mvs_linkage* k, const mvs_cell* d_cells, int64_t n_cells) {
    if (!k) return fail(MVS_E_INVALID, "NULL linkage");
    if (n_cells < 0 || (n_cells > 0 && !d_cells)) return fail(MVS_E_INVALID, "bad cell list");
    HIP_TRY(hipSetDevice(k->ctx->device));
    const Range range(k->ctx, "mvs_linkage_add_cells");
    return consume_cells(k, d_cells, n_cells);
}

int mvs_pairwise_linkage(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double min_jaccard,
                         mvs_linkage* k) {
    const int rc = consumer_checks("linkage", c, s, k, mem_norms, min_jaccard);
    if (rc) return rc;
    if (k->d != s->d) return fail(MVS_E_INVALID, "the linkage was created for dimension %d, the sketch set has %d", k->d, s->d);
    return feed_consumer("mvs_pairwise_linkage", c, s, norms_sq, mem_norms, min_jaccard, c->lk,
                         [k](const mvs_cell* d_cells, int64_t n_cells, int64_t, int64_t) { return consume_cells(k, d_cells, n_cells); });
}

int mvs_linkage_finish(mvs_linkage* k, mvs_link* links, int64_t capacity, int mem_out, int64_t* n_links) {
    if (!k) return fail(MVS_E_INVALID, "NULL linkage");
    if (!mem_ok(mem_out) || capacity < 0) return fail(MVS_E_INVALID, "bad argument");
    if (n_links) *n_links = k->n_forest;
    if (k->n_forest > capacity)
        return fail(MVS_E_CAPACITY, "the forest has %lld links, the buffer holds %lld", (long long)k->n_forest, (long long)capacity);
    if (k->n_forest == 0) return MVS_OK;
    if (!links) return fail(MVS_E_INVALID, "links is NULL");
    mvs_ctx* c = k->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_linkage_finish");
    const int rc = sort_links(k);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(links, k->links.as<mvs_link>(), (size_t)k->n_forest * sizeof(mvs_link),
                           mem_out == MVS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_linkage_cells(mvs_linkage* k, double level, mvs_cell* d_cells, int64_t capacity, int64_t* n_cells) {
    if (!k) return fail(MVS_E_INVALID, "NULL linkage");
    if (n_cells) *n_cells = 0;
    if (!(level == level)) return fail(MVS_E_INVALID, "level is NaN");
    if (capacity < 0 || (capacity > 0 && !d_cells)) return fail(MVS_E_INVALID, "bad cell buffer");
    if (k->n_forest == 0) return MVS_OK;
    mvs_ctx* c = k->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_linkage_cells");
    int rc = sort_links(k);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(k->counters.as<unsigned long long>() + 5, 0, sizeof(unsigned long long), c->stream));
    rc = mvs::launch_link_cells(c->stream, k->links.as<mvs_link>(), k->n_forest, level, d_cells, capacity, k->counters.as<unsigned long long>());
    if (!rc) rc = check_kernel("k_link_cells");
    if (rc) return rc;
    unsigned long long above = 0;
    rc = read_back(c, c->stream, {{&above, k->counters.as<unsigned long long>() + 5, 8}});
    if (rc) return rc;
    if (n_cells) *n_cells = (int64_t)above;
    if ((int64_t)above > capacity)
        return fail(MVS_E_CAPACITY, "%llu links lie above the level, the buffer holds %lld", above, (long long)capacity);
    return MVS_OK;
}

int mvs_linkage_destroy(mvs_linkage* k) {
    if (!k) return MVS_OK;
    if (k->ctx) {
        (void)hipSetDevice(k->ctx->device);
        (void)hipStreamSynchronize(k->ctx->stream);
    }
    delete k;
    return MVS_OK;
}

int mvs_ctx_linkage_stats(const mvs_ctx* c, double* compare_ms, double* forest_ms, int64_t* edges, int64_t* row_blocks,
                          int64_t* rounds) {
    return consumer_stats_out(c, &mvs_ctx::lk, compare_ms, forest_ms, edges, row_blocks, rounds);
}

}  // extern "C"
