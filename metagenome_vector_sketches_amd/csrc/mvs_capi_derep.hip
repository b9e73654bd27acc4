// mvs_capi_derep.hip -- C ABI of the greedy dereplication: mvs_derep_create / _add_rows / _finish / _destroy (a consumer of DEVICE
// cell lists that arrive row block by row block, in rank space), mvs_pairwise_derep (the one-call producer:
// mvs_pairwise_cluster's row-block loop with this consumer), mvs_sketch_set_gather (a sketch set in another row order),
// mvs_dereplicate (order, gather, compare, map back) and mvs_ctx_derep_stats.  The kernels and the argument for their
// exactness are in mvs_derep.hip.  No cell crosses the link: what comes back is four int32 arrays.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

#include <numeric>

using namespace mvs_capi;

struct mvs_derep {
    mvs_ctx* ctx = nullptr;
    int64_t n = 0;
    int64_t decided = 0;                     // rows [0, decided) are final
    DevBuf words;                            // int32_t: state | assign | blocked, n each
    DevBuf link;                             // int2
    DevBuf counters;                         // unsigned long long (mvs_internal.h: DerepState)
};

namespace {

mvs::DerepState state_of(const mvs_derep* k) {
    mvs::DerepState s;
    const size_t words = (size_t)std::max<int64_t>(k->n, 1);
    s.n = k->n;
    s.state = k->words.as<int32_t>();
    s.assign = k->words.as<int32_t>() + words;
    s.blocked = k->words.as<int32_t>() + 2 * words;
    s.link = k->link.as<int2>();
    s.counters = k->counters.as<unsigned long long>();
    return s;
}

// rows [rb, re) from one device list; the list is consumed when this returns
int consume_rows(mvs_derep* k, const mvs_cell* d_cells, int64_t n_cells, int64_t rb, int64_t re) {
    mvs_ctx* c = k->ctx;
    if (rb != k->decided)
        return fail(MVS_E_INVALID, "rows [%lld, %lld) do not continue the %lld rows decided so far", (long long)rb, (long long)re,
                    (long long)k->decided);
    if (re < rb || re > k->n) return fail(MVS_E_INVALID, "rows [%lld, %lld) outside [0, %lld)", (long long)rb, (long long)re, (long long)k->n);
    if (re == rb) return MVS_OK;
    StageTimer timer;
    int rc = timer.begin(c);
    if (rc) return rc;
    const mvs::DerepState s = state_of(k);
    HIP_TRY(hipMemsetAsync(k->counters.as<unsigned long long>(), 0, 3 * sizeof(unsigned long long), c->stream));
    rc = mvs::launch_derep_pre(c->stream, s, d_cells, n_cells, rb, re);
    if (!rc) rc = check_kernel("k_derep_pre");
    if (rc) return rc;
    unsigned long long back[3] = {0, 0, 0};
    int64_t round = 0;
    for (;;) {
        ++round;
        rc = mvs::launch_derep_scan(c->stream, s, d_cells, n_cells, rb, re, (int)round);
        if (!rc) rc = check_kernel("k_derep_scan");
        if (rc) return rc;
        if (round > 1) HIP_TRY(hipMemsetAsync(k->counters.as<unsigned long long>() + 2, 0, sizeof(unsigned long long), c->stream));
        rc = mvs::launch_derep_decide(c->stream, s, rb, re, (int)round);
        if (!rc) rc = check_kernel("k_derep_decide");
        if (rc) return rc;
        rc = read_back(c, c->stream, {{back, k->counters.as<unsigned long long>(), sizeof(back)}});
        if (rc) return rc;
        if (back[2] == 0) break;
        // every round decides the earliest undecided row: a block of R rows is through after R rounds (a path in priority order)
        if (round >= re - rb)
            return fail(MVS_E_HIP, "internal: %llu of %lld rows still undecided after %lld rounds", back[2], (long long)(re - rb),
                        (long long)round);
    }
    // representatives of the last round against the members decided before it (none in a block of one round: there the
    // members all come from the pre-pass, whose representatives precede the block)
    if (round > 1) {
        rc = mvs::launch_derep_scan(c->stream, s, d_cells, n_cells, rb, re, (int)round + 1);
        if (!rc) rc = check_kernel("k_derep_scan");
        if (rc) return rc;
    }
    rc = mvs::launch_derep_link(c->stream, s, d_cells, n_cells, rb, re);
    if (!rc) rc = check_kernel("k_derep_link");
    if (rc) return rc;
    // the list is the caller's again when this returns: the timer waits for its end mark, without it the stream is waited for
    rc = timer.mark_end();
    if (!rc) rc = timer.add_to(&c->dr.work_ms);
    if (rc) return rc;
    if (!timer.on) HIP_TRY(hipStreamSynchronize(c->stream));
    k->decided = re;
    c->dr.edges += (long long)back[0];
    c->dr.rounds = std::max<long long>(c->dr.rounds, round);
    if (back[1] != 0)
        return fail(MVS_E_RANGE, "%llu cells name a row outside [%lld, %lld) or a column outside [0, %lld): they were ignored", back[1],
                    (long long)rb, (long long)re, (long long)k->n);
    return MVS_OK;
}

// mvs_cluster.hip's norm_key on the host: an order-preserving map of a double onto 64 unsigned bits, -0.0 folded into +0.0,
// NaN -> 0 (below every number)
unsigned long long norm_key(double v) {
    if (!(v == v)) return 0ULL;
    if (v == 0.0) v = 0.0;
    unsigned long long u = 0;
    std::memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}

}  // namespace

extern "C" {

int mvs_sketch_set_gather(mvs_ctx* c, const mvs_sketch_set* src, const int32_t* rows, int mem_rows, int64_t n_rows,
                          mvs_sketch_set** out) {
    if (!c || !src || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (!mem_ok(mem_rows) || n_rows < 0) return fail(MVS_E_INVALID, "bad argument");
    if (src->ctx != c) return fail(MVS_E_INVALID, "the sketch set belongs to another context");
    if (n_rows > 0 && !rows) return fail(MVS_E_INVALID, "rows is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_sketch_set_gather");
    mvs_sketch_set* s = nullptr;
    int rc = mvs_sketch_set_alloc(c, n_rows, src->d, src->limbs, &s);   // (zeroed: the padding rows stay zero)
    if (rc) return rc;
    if (n_rows > 0) {
        DevBuf dr;
        const int32_t* d_rows = rows;
        hipError_t e = hipSuccess;
        if (mem_rows == MVS_MEM_HOST) {
            e = dr.alloc((size_t)n_rows * 4);
            if (e == hipSuccess) e = hipMemcpyAsync(dr.p, rows, (size_t)n_rows * 4, hipMemcpyHostToDevice, c->stream);
            d_rows = (const int32_t*)dr.p;
        }
        if (e == hipSuccess) e = hipMemsetAsync(c->counters(), 0, 8, c->stream);
        if (e != hipSuccess) {
            mvs_sketch_set_destroy(s);
            return fail(MVS_E_HIP, "staging the row list: %s", hipGetErrorString(e));
        }
        // a row is planes x d_pad contiguous bytes whatever the limb code means; d_pad is a multiple of 128
        const int64_t row_bytes = (int64_t)mvs::planes_of(src->limbs) * src->d_pad;
        rc = mvs::launch_gather_rows(c->stream, src->planes, src->n, d_rows, n_rows, row_bytes, s->owned.as<int8_t>(), c->counters());
        if (!rc) rc = check_kernel("k_gather_rows");
        unsigned long long bad = 0;
        if (!rc) rc = read_back(c, c->stream, {{&bad, c->counters(), 8}});   // (synchronises: the staged list may go)
        if (!rc && bad != 0)
            rc = fail(MVS_E_RANGE, "%llu of the %lld rows lie outside [0, %lld)", bad, (long long)n_rows, (long long)src->n);
        if (rc) {
            mvs_sketch_set_destroy(s);
            return rc;
        }
    }
    *out = s;
    return MVS_OK;
}

int mvs_derep_create(mvs_ctx* c, int64_t n, mvs_derep** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n < 0) return fail(MVS_E_INVALID, "n = %lld is negative", (long long)n);
    if (n >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n too large for int32 sample indices");
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<mvs_derep> k(new (std::nothrow) mvs_derep());
    if (!k) return fail(MVS_E_NOMEM, "out of host memory");
    k->ctx = c;
    k->n = n;
    const size_t words = (size_t)std::max<int64_t>(n, 1);
    if (k->words.alloc(3 * words * 4) != hipSuccess || k->link.alloc(words * sizeof(int2)) != hipSuccess || k->counters.alloc(64) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of the state of %lld samples failed", (long long)n);
    int rc = mvs::launch_derep_init(c->stream, state_of(k.get()));
    if (!rc) rc = check_kernel("k_derep_init");
    if (rc) return rc;
    c->dr.reset();
    *out = k.release();
    return MVS_OK;
}

int mvs_derep_add_rows(mvs_derep* k, const mvs_cell* d_cells, int64_t n_cells, int64_t row_begin, int64_t row_end) {
    if (!k) return fail(MVS_E_INVALID, "NULL dereplication");
    if (n_cells < 0 || (n_cells > 0 && !d_cells)) return fail(MVS_E_INVALID, "bad cell list");
    if (((uintptr_t)d_cells & 15) != 0) return fail(MVS_E_INVALID, "the cell list is not aligned to 16 bytes");
    HIP_TRY(hipSetDevice(k->ctx->device));
    const Range range(k->ctx, "mvs_derep_add_rows");
    return consume_rows(k, d_cells, n_cells, row_begin, row_end);
}

int mvs_pairwise_derep(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double min_jaccard, mvs_derep* k) {
    const int rc = consumer_checks("dereplication", c, s, k, mem_norms, min_jaccard);
    if (rc) return rc;
    if (k->decided != 0) return fail(MVS_E_INVALID, "%lld rows of the dereplication are decided already", (long long)k->decided);
    return feed_consumer("mvs_pairwise_derep", c, s, norms_sq, mem_norms, min_jaccard, c->dr,
                         [k](const mvs_cell* d_cells, int64_t n_cells, int64_t rb, int64_t re) { return consume_rows(k, d_cells, n_cells, rb, re); });
}

int mvs_derep_finish(mvs_derep* k, const int32_t* order, int mem_order, int32_t* rep_of, int32_t* link_dot, int32_t* link_q,
                     int32_t* sizes, int mem_out, int64_t* n_reps) {
    if (!k) return fail(MVS_E_INVALID, "NULL dereplication");
    if (!mem_ok(mem_order) || !mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (n_reps) *n_reps = 0;
    mvs_ctx* c = k->ctx;
    const int64_t n = k->n;
    if (k->decided != n) return fail(MVS_E_INVALID, "%lld of %lld rows are still undecided", (long long)(n - k->decided), (long long)n);
    if (n == 0) return MVS_OK;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_derep_finish");
    DevBuf dorder, dwork;
    const int32_t* d_order = order;
    if (order && mem_order == MVS_MEM_HOST) {
        HIP_TRY(dorder.alloc((size_t)n * 4));
        HIP_TRY(hipMemcpyAsync(dorder.p, order, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        d_order = (const int32_t*)dorder.p;
    }
    // rep_of, link_dot, link_q, sizes (n each); sizes doubles as the marks of the permutation check
    const size_t np = ((size_t)n + 63) / 64 * 64;
    HIP_TRY(dwork.alloc(4 * np * 4));
    int32_t* d_rep_of = (int32_t*)dwork.p;
    int32_t* d_link_dot = d_rep_of + np;
    int32_t* d_link_q = d_link_dot + np;
    int32_t* d_sizes = d_link_q + np;
    const mvs::DerepState s = state_of(k);
    StageTimer timer;
    int rc = timer.begin(c);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(k->counters.as<unsigned long long>() + 3, 0, 2 * sizeof(unsigned long long), c->stream));
    unsigned long long back[2] = {0, 0};
    if (d_order) {
        HIP_TRY(hipMemsetAsync(d_sizes, 0, (size_t)n * 4, c->stream));
        rc = mvs::launch_derep_order_check(c->stream, d_order, n, d_sizes, k->counters.as<unsigned long long>());
        if (!rc) rc = check_kernel("k_derep_order_check");
        if (!rc) rc = read_back(c, c->stream, {{back, k->counters.as<unsigned long long>() + 3, sizeof(back)}});
        if (rc) return rc;
        if (back[1] != 0) return fail(MVS_E_INVALID, "order is not a permutation of [0, %lld): %llu bad entries", (long long)n, back[1]);
    }
    HIP_TRY(hipMemsetAsync(d_sizes, 0, (size_t)n * 4, c->stream));
    rc = mvs::launch_derep_scatter(c->stream, s, d_order, d_rep_of, d_link_dot, d_link_q, d_sizes);
    if (!rc) rc = check_kernel("k_derep_scatter");
    if (rc) return rc;
    rc = timer.mark_end();
    if (rc) return rc;
    rc = read_back(c, c->stream, {{back, k->counters.as<unsigned long long>() + 3, sizeof(back)}});
    if (!rc) rc = timer.add_to(&c->dr.work_ms);
    if (rc) return rc;
    if (n_reps) *n_reps = (int64_t)back[0];
    rc = give_out(c, rep_of, d_rep_of, n, mem_out);
    if (!rc) rc = give_out(c, link_dot, d_link_dot, n, mem_out);
    if (!rc) rc = give_out(c, link_q, d_link_q, n, mem_out);
    if (!rc) rc = give_out(c, sizes, d_sizes, n, mem_out);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));   // (also before the DevBufs free the scratch)
    return MVS_OK;
}

int mvs_derep_destroy(mvs_derep* k) {
    if (!k) return MVS_OK;
    if (k->ctx) {
        (void)hipSetDevice(k->ctx->device);
        (void)hipStreamSynchronize(k->ctx->stream);
    }
    delete k;
    return MVS_OK;
}

int mvs_ctx_derep_stats(const mvs_ctx* c, double* compare_ms, double* greedy_ms, int64_t* edges, int64_t* row_blocks, int64_t* rounds) {
    return consumer_stats_out(c, &mvs_ctx::dr, compare_ms, greedy_ms, edges, row_blocks, rounds);
}

int mvs_dereplicate(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double min_jaccard, const int32_t* order,
                    int32_t* rep_of, int32_t* link_dot, int32_t* link_q, int32_t* sizes, int mem_out, int64_t* n_reps) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (n_reps) *n_reps = 0;
    if (!(min_jaccard > 0.0) || !(min_jaccard < 1.0)) return fail(MVS_E_INVALID, "min_jaccard = %g outside (0, 1)", min_jaccard);
    if (!mem_ok(mem_norms) || !mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (s->ctx != c) return fail(MVS_E_INVALID, "the sketch set belongs to another context");
    const int64_t n = s->n;
    if (n > 0 && !norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_dereplicate");

    // 1. the order (host: a sort of n keys is not the hot path) and the norms in that order
    std::vector<double> n2((size_t)n);
    if (n > 0) {
        if (mem_norms == MVS_MEM_HOST) {
            std::memcpy(n2.data(), norms_sq, (size_t)n * 8);
        } else {
            HIP_TRY(hipMemcpyAsync(n2.data(), norms_sq, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
    }
    std::vector<int32_t> ord((size_t)n);
    if (order) {
        std::vector<char> seen((size_t)n, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t v = order[i];
            if (v < 0 || v >= n || seen[(size_t)v])
                return fail(MVS_E_INVALID, "order is not a permutation of [0, %lld): entry %lld is %d", (long long)n, (long long)i, v);
            seen[(size_t)v] = 1;
            ord[(size_t)i] = v;
        }
    } else {
        std::iota(ord.begin(), ord.end(), 0);
        std::vector<unsigned long long> key((size_t)n);
        for (int64_t i = 0; i < n; ++i) key[(size_t)i] = norm_key(n2[(size_t)i]);
        std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] > key[(size_t)b]; });
    }
    bool identity = true;
    for (int64_t i = 0; i < n && identity; ++i) identity = ord[(size_t)i] == (int32_t)i;

    // 2. the set and the norms in rank space
    struct Temps {
        mvs_sketch_set* set = nullptr;
        mvs_derep* derep = nullptr;
        ~Temps() {
            if (derep) mvs_derep_destroy(derep);
            if (set) mvs_sketch_set_destroy(set);
        }
    } tmp;
    const mvs_sketch_set* ranked = s;
    if (!identity) {
        const int rc = mvs_sketch_set_gather(c, s, ord.data(), MVS_MEM_HOST, n, &tmp.set);
        if (rc) return rc;
        ranked = tmp.set;
        std::vector<double> permuted((size_t)n);
        for (int64_t i = 0; i < n; ++i) permuted[(size_t)i] = n2[(size_t)ord[(size_t)i]];
        n2.swap(permuted);
    }

    // 3. compare and decide, row block by row block; 4. the temporaries go with `tmp`
    int rc = mvs_derep_create(c, n, &tmp.derep);
    if (!rc) rc = mvs_pairwise_derep(c, ranked, n2.data(), MVS_MEM_HOST, min_jaccard, tmp.derep);
    if (!rc) rc = mvs_derep_finish(tmp.derep, identity ? nullptr : ord.data(), MVS_MEM_HOST, rep_of, link_dot, link_q, sizes, mem_out, n_reps);
    return rc;
}

}  // extern "C"
