// mvs_capi_cluster.hip -- C ABI of the single-linkage clustering: mvs_cluster_create / _add_cells / _finish / _destroy (a
// consumer of DEVICE cell lists, whoever produced them), mvs_pairwise_cluster (the one-call producer: the threshold comparison
// of a sketch set, row block by row block, each block's unsorted cells fed straight into the consumer) and
// mvs_ctx_cluster_stats.  The kernels and the argument for their exactness are in mvs_cluster.hip.  No cell crosses the link:
// what comes back is four int32 arrays.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

using namespace mvs_capi;

struct mvs_cluster {
    mvs_ctx* ctx = nullptr;
    int64_t n = 0;
    DevBuf parent;     // int32_t, the forest: parent[x] <= x
    DevBuf degree;     // int32_t
    DevBuf counters;   // unsigned long long (mvs_cluster.hip): edges, cells out of range, cells whose endpoints are apart
};

namespace {

constexpr int kMaxRounds = 64;   // hook -> flatten -> verify rounds per list before the call gives up (one is the normal case)

// the union-find rounds over one device list; the list is consumed when this returns
int consume_cells(mvs_cluster* k, const mvs_cell* d_cells, int64_t n_cells) {
    mvs_ctx* c = k->ctx;
    if (n_cells == 0) return MVS_OK;
    StageTimer timer;
    int rc = timer.begin(c);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(k->counters.as<unsigned long long>(), 0, 3 * sizeof(unsigned long long), c->stream));
    unsigned long long back[3] = {0, 0, 0};
    int round = 0;
    for (;;) {
        ++round;
        rc = mvs::launch_cluster_hook(c->stream, d_cells, n_cells, k->parent.as<int32_t>(), k->degree.as<int32_t>(), k->n, round == 1,
                                      k->counters.as<unsigned long long>());
        if (!rc) rc = check_kernel("k_cluster_hook");
        if (rc) return rc;
        rc = mvs::launch_cluster_flatten(c->stream, k->parent.as<int32_t>(), k->n);
        if (!rc) rc = check_kernel("k_cluster_flatten");
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(k->counters.as<unsigned long long>() + 2, 0, sizeof(unsigned long long), c->stream));
        rc = mvs::launch_cluster_verify(c->stream, d_cells, n_cells, k->parent.as<int32_t>(), k->n, k->counters.as<unsigned long long>());
        if (!rc) rc = check_kernel("k_cluster_verify");
        if (rc) return rc;
        rc = read_back(c, c->stream, {{back, k->counters.as<unsigned long long>(), sizeof(back)}});
        if (rc) return rc;
        if (back[1] != 0) break;
        if (back[2] == 0) break;
        if (round >= kMaxRounds)
            return fail(MVS_E_HIP, "internal: %llu cells still join different trees after %d union-find rounds", back[2], round);
    }
    rc = timer.mark_end();
    if (!rc) rc = timer.add_to(&c->cl.work_ms);
    if (rc) return rc;
    c->cl.edges += (long long)back[0];
    c->cl.rounds = std::max<long long>(c->cl.rounds, round);
    if (back[1] != 0)
        return fail(MVS_E_RANGE, "%llu cells name a sample outside [0, %lld): they were ignored", back[1], (long long)k->n);
    return MVS_OK;
}

}  // namespace

namespace mvs_capi {

// The threshold comparison of a sketch set with itself at level min_jaccard, row block by row block: each block's unsorted
// cells (every ordered pair of linked samples exactly once) are handed to `consume` while they sit in the staging buffer.
// Shared by mvs_pairwise_cluster, mvs_pairwise_linkage (mvs_capi_linkage.hip) and mvs_pairwise_derep (mvs_capi_derep.hip)
// through feed_consumer: one launch, one staging buffer, one halving and grow rule.  `consume` is also told the block's rows
// [rb, re): the blocks come in ascending order.  d_n2: the norms on the device; *compare_ms (timing on) and *row_blocks are
// added to.
int pairwise_feed(mvs_ctx* c, const mvs_sketch_set* s, const double* d_n2, double min_jaccard, double* compare_ms, long long* row_blocks,
                  const ConsumeCells& consume) {
    const int64_t n = s->n;
    // J > t  <=>  double(P)/d > t/(1+t) * (n2r + n2c): mvs_search_block's coefficient
    const double coeff = min_jaccard / (1.0 + min_jaccard);
    // rows per block: the bound mvs_pairwise_rows puts on its chunks (borders on multiples of 256 rows: the symmetric schedule)
    int64_t R = (int64_t)(c->opt.pairwise_block_cells / (double)n);
    R = std::max<int64_t>(256, R / 256 * 256);
    if (c->opt.cluster_block_rows > 0) R = std::min<int64_t>(R, std::max<int64_t>(256, (int64_t)c->opt.cluster_block_rows / 256 * 256));
    // the staging buffer: a fixed share of the free memory, never more than the first block can produce
    int64_t capacity = c->opt.cluster_cells;
    if (capacity <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t have = free_b + c->pw_tmp.bytes;               // (the buffer below is the context's own, counted as free)
        capacity = (int64_t)std::min<size_t>(std::max<size_t>(4096, have / 4 / sizeof(mvs_cell)), (size_t)1 << 30);   // (the option's range)
        const double block = (double)std::min(R, n) * (double)n;
        if (block < (double)capacity) capacity = (int64_t)block;
    }
    capacity = std::max<int64_t>(capacity, 1);
    int rc = ensure_buf(c, c->pw_tmp, (size_t)capacity * sizeof(mvs_cell));
    if (rc) return rc;
    for (int64_t rb = 0; rb < n;) {
        const int64_t re = std::min(n, rb + R);
        unsigned long long count = 0;
        rc = pairwise_launch(c, s, d_n2, MVS_KEEP_INT16, rb, re, 0, n, true, false, (mvs_cell*)c->pw_tmp.p, capacity, 0, &count, coeff);
        if (rc) return rc;
        if (count == ~0ULL) {
            rc = read_back(c, c->stream, {{&count, c->counters(), 8}});
            if (rc) return rc;
        }
        if (c->timing && c->ev_valid[1]) {
            float ms = 0.f;
            if (mvs_ctx_kernel_ms(c, 1, &ms) == MVS_OK) *compare_ms += ms;
        }
        if ((int64_t)count > capacity) {
            // a dense block: the list was cut off at the buffer's end.  Half the rows and again; a block of 256 rows cannot
            // shrink (the symmetric schedule's granule), so there the buffer takes what the block was seen to need.
            if (re - rb > 256) {
                R = std::max<int64_t>(256, ((re - rb) / 2 + 255) / 256 * 256);
                continue;
            }
            capacity = (int64_t)count;
            rc = ensure_buf(c, c->pw_tmp, (size_t)capacity * sizeof(mvs_cell));
            if (rc) return rc;
            continue;
        }
        rc = consume((const mvs_cell*)c->pw_tmp.p, (int64_t)count, rb, re);
        if (rc) return rc;
        ++*row_blocks;
        rb = re;
    }
    return MVS_OK;
}

int norms_on_device(mvs_ctx* c, const double* norms_sq, int mem_norms, int64_t n, DevBuf& staging, const double** d_n2) {
    *d_n2 = norms_sq;
    if (mem_norms == MVS_MEM_HOST) {
        HIP_TRY(staging.alloc((size_t)n * 8));
        HIP_TRY(hipMemcpyAsync(staging.p, norms_sq, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        *d_n2 = (const double*)staging.p;
    }
    return MVS_OK;
}

int feed_consumer(const char* entry, mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double min_jaccard,
                  ConsumerStats& st, const ConsumeCells& consume) {
    const int64_t n = s->n;
    if (n == 0) return MVS_OK;
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    const Range range(c, entry);
    HIP_TRY(hipSetDevice(c->device));
    DevBuf dn;
    const double* d_n2 = nullptr;
    const int rc = norms_on_device(c, norms_sq, mem_norms, n, dn, &d_n2);
    if (rc) return rc;
    return pairwise_feed(c, s, d_n2, min_jaccard, &st.compare_ms, &st.blocks, consume);
}

int consumer_stats_out(const mvs_ctx* c, ConsumerStats mvs_ctx::*which, double* compare_ms, double* work_ms, int64_t* edges,
                       int64_t* row_blocks, int64_t* rounds) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    const ConsumerStats& st = c->*which;
    if (compare_ms) *compare_ms = st.compare_ms;
    if (work_ms) *work_ms = st.work_ms;
    if (edges) *edges = st.edges;
    if (row_blocks) *row_blocks = st.blocks;
    if (rounds) *rounds = st.rounds;
    return MVS_OK;
}

}  // namespace mvs_capi

extern "C" {

int mvs_cluster_create(mvs_ctx* c, int64_t n, mvs_cluster** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n < 0) return fail(MVS_E_INVALID, "n = %lld is negative", (long long)n);
    if (n >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n too large for int32 sample indices");
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<mvs_cluster> k(new (std::nothrow) mvs_cluster());
    if (!k) return fail(MVS_E_NOMEM, "out of host memory");
    k->ctx = c;
    k->n = n;
    const size_t words = (size_t)std::max<int64_t>(n, 1);
    if (k->parent.alloc(words * 4) != hipSuccess || k->degree.alloc(words * 4) != hipSuccess || k->counters.alloc(64) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of the forest of %lld samples failed", (long long)n);
    int rc = mvs::launch_cluster_init(c->stream, k->parent.as<int32_t>(), k->degree.as<int32_t>(), n);
    if (!rc) rc = check_kernel("k_cluster_init");
    if (rc) return rc;
    c->cl.reset();
    *out = k.release();
    return MVS_OK;
}

int mvs_cluster_add_cells(mvs_cluster* k, const mvs_cell* d_cells, int64_t n_cells) {
    if (!k) return fail(MVS_E_INVALID, "NULL cluster");
    if (n_cells < 0 || (n_cells > 0 && !d_cells)) return fail(MVS_E_INVALID, "bad cell list");
    HIP_TRY(hipSetDevice(k->ctx->device));
    const Range range(k->ctx, "mvs_cluster_add_cells");
    return consume_cells(k, d_cells, n_cells);
}

int mvs_pairwise_cluster(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double min_jaccard,
                         mvs_cluster* k) {
    const int rc = consumer_checks("cluster", c, s, k, mem_norms, min_jaccard);
    if (rc) return rc;
    return feed_consumer("mvs_pairwise_cluster", c, s, norms_sq, mem_norms, min_jaccard, c->cl,
                         [k](const mvs_cell* d_cells, int64_t n_cells, int64_t, int64_t) { return consume_cells(k, d_cells, n_cells); });
}

int mvs_cluster_finish(mvs_cluster* k, const double* norms_sq, int mem_norms, int32_t* labels, int32_t* degree,
                       int32_t* representatives, int32_t* sizes, int mem_out, int64_t* n_clusters) {
    if (!k) return fail(MVS_E_INVALID, "NULL cluster");
    if (!mem_ok(mem_norms) || !mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (n_clusters) *n_clusters = 0;
    mvs_ctx* c = k->ctx;
    const int64_t n = k->n;
    if (n == 0) return MVS_OK;
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_cluster_finish");
    DevBuf dn, dwork, dbest, dscan;
    const double* d_n2 = nullptr;
    int rc = norms_on_device(c, norms_sq, mem_norms, n, dn, &d_n2);
    if (rc) return rc;
    // is_root, ids (n + 1 each), labels, sizes, representatives (n each)
    const size_t np1 = ((size_t)n + 1 + 63) / 64 * 64;
    HIP_TRY(dwork.alloc(5 * np1 * 4));
    HIP_TRY(dbest.alloc((size_t)n * 8));
    int32_t* d_is_root = (int32_t*)dwork.p;
    int32_t* d_ids = d_is_root + np1;
    int32_t* d_labels = d_ids + np1;
    int32_t* d_sizes = d_labels + np1;
    int32_t* d_rep = d_sizes + np1;
    size_t need = 0;
    rc = mvs::cluster_finish(c->stream, k->parent.as<int32_t>(), d_n2, n, d_is_root, d_ids, d_labels, d_sizes, d_rep,
                             (unsigned long long*)dbest.p, nullptr, 0, &need);
    if (rc) return fail(rc, "cluster finish: scan sizing failed");
    HIP_TRY(dscan.alloc(need));
    StageTimer timer;
    rc = timer.begin(c);
    if (rc) return rc;
    rc = mvs::launch_cluster_flatten(c->stream, k->parent.as<int32_t>(), n);
    if (!rc) rc = check_kernel("k_cluster_flatten");
    if (rc) return rc;
    rc = mvs::cluster_finish(c->stream, k->parent.as<int32_t>(), d_n2, n, d_is_root, d_ids, d_labels, d_sizes, d_rep,
                             (unsigned long long*)dbest.p, dscan.p, need, nullptr);
    if (rc) return fail(rc, "cluster finish failed");
    rc = check_kernel("k_cluster_label");
    if (rc) return rc;
    rc = timer.mark_end();
    if (rc) return rc;
    int32_t total = 0;
    rc = read_back(c, c->stream, {{&total, d_ids + n, 4}});
    if (!rc) rc = timer.add_to(&c->cl.work_ms);
    if (rc) return rc;
    if (n_clusters) *n_clusters = total;
    rc = give_out(c, labels, d_labels, n, mem_out);
    if (!rc) rc = give_out(c, degree, k->degree.as<int32_t>(), n, mem_out);
    if (!rc) rc = give_out(c, representatives, d_rep, total, mem_out);
    if (!rc) rc = give_out(c, sizes, d_sizes, total, mem_out);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));   // (also before the DevBufs free the scratch)
    return MVS_OK;
}

int mvs_cluster_destroy(mvs_cluster* k) {
    if (!k) return MVS_OK;
    if (k->ctx) {
        (void)hipSetDevice(k->ctx->device);
        (void)hipStreamSynchronize(k->ctx->stream);
    }
    delete k;
    return MVS_OK;
}

int mvs_ctx_cluster_stats(const mvs_ctx* c, double* compare_ms, double* union_ms, int64_t* edges, int64_t* row_blocks,
                          int64_t* rounds) {
    return consumer_stats_out(c, &mvs_ctx::cl, compare_ms, union_ms, edges, row_blocks, rounds);
}

}  // extern "C"
