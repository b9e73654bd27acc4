// mvs_capi_hclust.hip -- C ABI of the average / complete linkage on the Jaccard distances: mvs_hclust_sums, mvs_hclust_weights,
// mvs_hclust, mvs_hclust_order, mvs_hclust_cut, mvs_hclust_cut_count, mvs_ctx_hclust_stats (include/mvs_hip.h "Average and
// complete linkage").  The kernels are in mvs_hclust.hip.
//
// The three device entry points differ in how the table is filled -- a copy of the caller's sums, the caller's weights widened,
// or dense dots quantised block of rows by block of rows -- and share the rounds: nearest, pairs, one read-back of two counters
// (the host sizes the next launches by them), the two merge phases, and a compaction of the columns where option hclust_compact
// asks for one.  Only the records come back.  The tree functions are pure host.
#include "mvs_capi_internal.h"
#include "mvs_hclust.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <numeric>

using namespace mvs_capi;

namespace {

struct Engine {
    DevBuf table, col_slot, col_n, slot_col, size, nearest, pairs, keep, counters, merges, live[2];
    mvs::HclustState st{};
    int64_t m = 0;
};

// the table and the O(m) arrays of m slots; `extra` bytes are the caller's own (a dots block) and only named in the refusal
int engine_alloc(mvs_ctx* c, int64_t m, size_t extra, Engine& e) {
    e.m = m;
    const int64_t ld = (m + 1) & ~(int64_t)1;
    const size_t table_bytes = (size_t)m * (size_t)ld * 8;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (table_bytes + extra + (size_t)ld * 64 > free_b || e.table.alloc(table_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MVS_E_NOMEM, "the table of %lld slots needs %zu bytes and the dots block %zu: %zu asked for, %zu free on the device",
                    (long long)m, table_bytes, extra, table_bytes + extra, free_b);
    }
    HIP_TRY(e.col_slot.alloc((size_t)ld * 4));
    HIP_TRY(e.col_n.alloc((size_t)ld * 4));
    HIP_TRY(e.slot_col.alloc((size_t)m * 4));
    HIP_TRY(e.size.alloc((size_t)m * 4));
    HIP_TRY(e.nearest.alloc((size_t)m * 4));
    HIP_TRY(e.pairs.alloc((size_t)ld * 4));
    HIP_TRY(e.keep.alloc((size_t)m * 4));
    HIP_TRY(e.counters.alloc(4 * 4));
    HIP_TRY(e.merges.alloc((size_t)m * sizeof(mvs_hmerge)));
    HIP_TRY(e.live[0].alloc((size_t)m * 4));
    HIP_TRY(e.live[1].alloc((size_t)m * 4));
    e.st.table = (unsigned long long*)e.table.p;
    e.st.ld = ld;
    e.st.col_slot = (int32_t*)e.col_slot.p;
    e.st.col_n = (uint32_t*)e.col_n.p;
    e.st.slot_col = (int32_t*)e.slot_col.p;
    e.st.size = (int32_t*)e.size.p;
    e.st.nearest = (int32_t*)e.nearest.p;
    e.st.pairs = (int32_t*)e.pairs.p;
    e.st.keep = (int32_t*)e.keep.p;
    e.st.counters = (int32_t*)e.counters.p;
    e.st.merges = (mvs_hmerge*)e.merges.p;
    return MVS_OK;
}

int sizes_checks(const int32_t* sizes, int64_t m) {
    if (m > MVS_HCLUST_MAX_TOTAL) return fail(MVS_E_INVALID, "%lld slots exceed the total of %d", (long long)m, MVS_HCLUST_MAX_TOTAL);
    if (!sizes) return MVS_OK;
    int64_t total = 0;
    for (int64_t i = 0; i < m; ++i) {
        if (sizes[i] < 1) return fail(MVS_E_INVALID, "sizes[%lld] = %d < 1", (long long)i, (int)sizes[i]);
        total += sizes[i];
    }
    if (total > MVS_HCLUST_MAX_TOTAL) return fail(MVS_E_INVALID, "the sizes total %lld > %d", (long long)total, MVS_HCLUST_MAX_TOTAL);
    return MVS_OK;
}

int method_check(int method) {
    if (method != MVS_HCLUST_AVERAGE && method != MVS_HCLUST_COMPLETE) return fail(MVS_E_INVALID, "unknown method %d", method);
    return MVS_OK;
}

#define HCLUST_LAUNCH(call, name)                                  \
    do {                                                           \
        int rc_ = (call);                                          \
        if (rc_) return fail(rc_, "hclust: %s launch rejected", name); \
        rc_ = check_kernel(name);                                  \
        if (rc_) return rc_;                                       \
    } while (0)

// the rounds on a filled table; sizes: HOST, NULL = ones; check_input: the table is a caller's
int engine_run(mvs_ctx* c, Engine& e, const int32_t* sizes, int method, bool check_input, mvs_hmerge* merges, int64_t* rounds) {
    const int64_t m = e.m, ld = e.st.ld;
    const mvs::HclustState& st = e.st;
    {
        std::vector<int32_t> ident((size_t)ld, -1), n((size_t)ld, 0);
        std::iota(ident.begin(), ident.begin() + m, 0);
        for (int64_t i = 0; i < m; ++i) n[(size_t)i] = sizes ? sizes[i] : 1;
        HIP_TRY(hipMemcpyAsync(st.col_slot, ident.data(), (size_t)ld * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(st.col_n, n.data(), (size_t)ld * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(st.slot_col, ident.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(st.size, n.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(e.live[0].p, ident.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(st.counters, 0, 4 * 4, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));                // (the vectors leave scope)
    }
    if (check_input) {
        HCLUST_LAUNCH(mvs::launch_hclust_check(c->stream, st, m), "k_hclust_check");
        int32_t flags = 0;
        if (const int rc = read_back(c, c->stream, {{&flags, st.counters + 2, 4}})) return rc;
        if (flags & 1) return fail(MVS_E_INVALID, "the table is not symmetric");
        if (flags & 2) return fail(MVS_E_INVALID, "an entry exceeds n_a x n_b x 2^30");
    }
    int64_t n_live = m, n_cols = m, done = 0;
    int cur = 0, round = 0;
    while (n_live > 1) {
        const int32_t* live = (const int32_t*)e.live[cur].p;
        int32_t* next = (int32_t*)e.live[cur ^ 1].p;
        StageTimer t_near, t_merge, t_compact;
        if (const int rc = t_near.begin(c)) return rc;
        HCLUST_LAUNCH(mvs::launch_hclust_nearest(c->stream, st, method, live, n_live, n_cols), "k_hclust_nearest");
        if (const int rc = t_near.mark_end()) return rc;
        c->hc.row_scans += n_live;
        c->hc.bytes_scanned += n_live * n_cols * 8;
        if (const int rc = t_merge.begin(c)) return rc;
        HCLUST_LAUNCH(mvs::launch_hclust_pairs(c->stream, st, method, live, next, n_live, round, done), "k_hclust_pairs");
        int32_t counts[2] = {0, 0};
        if (const int rc = read_back(c, c->stream, {{counts, st.counters, 8}})) return rc;
        const int64_t n_pairs = counts[0];
        if (n_pairs < 1 || counts[1] != n_live - n_pairs || done + n_pairs > m - 1)
            return fail(MVS_E_INTERNAL, "round %d of %lld live rows: %d pairs, %d rows left", round, (long long)n_live, (int)counts[0], (int)counts[1]);
        HCLUST_LAUNCH(mvs::launch_hclust_merge_cols(c->stream, st, method, live, n_live, n_pairs), "k_hclust_merge_cols");
        HCLUST_LAUNCH(mvs::launch_hclust_merge_rows(c->stream, st, method, n_pairs, n_cols), "k_hclust_merge_rows");
        if (const int rc = t_merge.mark_end()) return rc;
        n_live -= n_pairs;
        done += n_pairs;
        cur ^= 1;
        ++round;
        const bool compact = n_live > 1 && n_live < n_cols && (c->hclust_compact == 2 || (c->hclust_compact == 1 && 2 * n_live <= n_cols));
        if (compact) {
            if (const int rc = t_compact.begin(c)) return rc;
            HCLUST_LAUNCH(mvs::launch_hclust_layout(c->stream, st, n_cols), "k_hclust_layout");
            HCLUST_LAUNCH(mvs::launch_hclust_compact(c->stream, st, (const int32_t*)e.live[cur].p, n_live, n_live), "k_hclust_compact");
            if (const int rc = t_compact.mark_end()) return rc;
            n_cols = n_live;
            ++c->hc.compactions;
        }
        if (const int rc = t_near.add_to(&c->hc.nearest_ms)) return rc;
        if (const int rc = t_merge.add_to(&c->hc.merge_ms)) return rc;
        if (compact)
            if (const int rc = t_compact.add_to(&c->hc.compact_ms)) return rc;
    }
    c->hc.rounds = round;
    if (done != m - 1) return fail(MVS_E_INTERNAL, "%lld merges of %lld slots", (long long)done, (long long)m);
    if (m > 1) HIP_TRY(hipMemcpyAsync(merges, st.merges, (size_t)(m - 1) * sizeof(mvs_hmerge), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (rounds) *rounds = round;
    return MVS_OK;
}

// what the three entry points check alike; *trivial: m == 1, nothing to do
int common_checks(mvs_ctx* c, int64_t m, int method, const mvs_hmerge* merges, int64_t* rounds, bool* trivial) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (const int rc = method_check(method)) return rc;
    if (m < 1) return fail(MVS_E_INVALID, "m = %lld < 1", (long long)m);
    c->hc.reset();
    *trivial = m == 1;
    if (m == 1) {
        if (rounds) *rounds = 0;
        return MVS_OK;
    }
    if (!merges) return fail(MVS_E_INVALID, "merges is NULL");
    return MVS_OK;
}

// ---- the tree, on the host ----
// the merges' indices in (height, round, a) order; MVS_E_INVALID for records that are no tree of m leaves
int sorted_merges(int64_t m, const mvs_hmerge* merges, std::vector<int64_t>& order) {
    if (m < 1) return fail(MVS_E_INVALID, "m = %lld < 1", (long long)m);
    if (m > 1 && !merges) return fail(MVS_E_INVALID, "merges is NULL");
    for (int64_t t = 0; t + 1 < m; ++t) {
        const mvs_hmerge& r = merges[t];
        if (r.a < 0 || r.a >= r.b || r.b >= m) return fail(MVS_E_INVALID, "merge %lld joins slots %d and %d of %lld", (long long)t, r.a, r.b, (long long)m);
        if (std::isnan(r.height)) return fail(MVS_E_INVALID, "merge %lld has no height", (long long)t);
    }
    order.resize((size_t)(m - 1));
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        const mvs_hmerge &p = merges[x], &q = merges[y];
        if (p.height != q.height) return p.height < q.height;
        if (p.round != q.round) return p.round < q.round;
        return p.a < q.a;
    });
    return MVS_OK;
}

struct Forest {
    std::vector<int32_t> parent;
    explicit Forest(int64_t m) : parent((size_t)m) { std::iota(parent.begin(), parent.end(), 0); }
    int32_t find(int32_t x) {
        while (parent[(size_t)x] != x) x = parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
        return x;
    }
    // the root is the smaller index: a cluster's root is its smallest member
    void join(int32_t x, int32_t y) {
        x = find(x), y = find(y);
        if (x == y) return;
        if (x < y) parent[(size_t)y] = x;
        else parent[(size_t)x] = y;
    }
    void labels(int32_t* out) {
        const int64_t m = (int64_t)parent.size();
        int32_t next = 0;
        for (int64_t i = 0; i < m; ++i) {
            const int32_t r = find((int32_t)i);
            out[i] = r == i ? next++ : out[r];                   // (r < i has its label)
        }
    }
};

}  // namespace

extern "C" {

int mvs_hclust_sums(mvs_ctx* c, const uint64_t* sums, int mem, const int32_t* sizes, int64_t m, int method, mvs_hmerge* merges, int64_t* rounds) {
    bool trivial = false;
    if (const int rc = common_checks(c, m, method, merges, rounds, &trivial)) return rc;
    if (!mem_ok(mem)) return fail(MVS_E_INVALID, "bad argument");
    if (const int rc = sizes_checks(sizes, m)) return rc;
    if (trivial) return MVS_OK;
    if (!sums) return fail(MVS_E_INVALID, "sums is NULL");
    Range mark(c, "mvs_hclust_sums");
    HIP_TRY(hipSetDevice(c->device));
    Engine e;
    if (const int rc = engine_alloc(c, m, 0, e)) return rc;
    HIP_TRY(hipMemcpy2DAsync(e.st.table, (size_t)e.st.ld * 8, sums, (size_t)m * 8, (size_t)m * 8, (size_t)m,
                             mem == MVS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    return engine_run(c, e, sizes, method, true, merges, rounds);
}

int mvs_hclust_weights(mvs_ctx* c, const uint32_t* w, int mem, int64_t m, int method, mvs_hmerge* merges, int64_t* rounds) {
    bool trivial = false;
    if (const int rc = common_checks(c, m, method, merges, rounds, &trivial)) return rc;
    if (!mem_ok(mem)) return fail(MVS_E_INVALID, "bad argument");
    if (const int rc = sizes_checks(nullptr, m)) return rc;
    if (trivial) return MVS_OK;
    if (!w) return fail(MVS_E_INVALID, "w is NULL");
    Range mark(c, "mvs_hclust_weights");
    HIP_TRY(hipSetDevice(c->device));
    Engine e;
    const size_t w_bytes = (size_t)m * m * 4;
    if (const int rc = engine_alloc(c, m, mem == MVS_MEM_HOST ? w_bytes : 0, e)) return rc;
    DevBuf staged;
    const uint32_t* d_w = w;
    if (mem == MVS_MEM_HOST) {
        HIP_TRY(staged.alloc(w_bytes));
        HIP_TRY(hipMemcpyAsync(staged.p, w, w_bytes, hipMemcpyHostToDevice, c->stream));
        d_w = (const uint32_t*)staged.p;
    }
    StageTimer t_fill;
    if (const int rc = t_fill.begin(c)) return rc;
    HCLUST_LAUNCH(mvs::launch_hclust_widen(c->stream, d_w, m, e.st.table, e.st.ld), "k_hclust_widen");
    if (const int rc = t_fill.mark_end()) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (const int rc = t_fill.add_to(&c->hc.fill_ms)) return rc;
    return engine_run(c, e, nullptr, method, true, merges, rounds);      // (unit sizes: the entry bound is w <= 2^30)
}

int mvs_hclust(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double floor, int64_t rb, int64_t re, int method,
               mvs_hmerge* merges, int64_t* rounds) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (!(floor >= 0.0) || !(floor < 1.0)) return fail(MVS_E_INVALID, "floor = %g outside [0, 1)", floor);
    if (!mem_ok(mem_norms)) return fail(MVS_E_INVALID, "bad argument");
    if (rb < 0 || re > s->n || rb > re) return fail(MVS_E_INVALID, "rows [%lld, %lld) outside the set's %lld samples", (long long)rb, (long long)re, (long long)s->n);
    if (s->ctx != c) return fail(MVS_E_INVALID, "the sketch set belongs to another context");
    const int64_t m = re - rb;
    bool trivial = false;
    if (const int rc = common_checks(c, m, method, merges, rounds, &trivial)) return rc;
    if (const int rc = sizes_checks(nullptr, m)) return rc;
    if (trivial) return MVS_OK;
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    Range mark(c, "mvs_hclust");
    HIP_TRY(hipSetDevice(c->device));

    // rows per block of the fill: the dots block takes half of what the table leaves free
    const size_t row_bytes = (size_t)m * 4;
    const size_t table_bytes = (size_t)m * (size_t)((m + 1) & ~(int64_t)1) * 8;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t left = free_b > table_bytes ? free_b - table_bytes : 0;
    const int64_t R = dots_block_rows(left / 2, row_bytes, c->hclust_block_rows, m);
    Engine e;
    if (const int rc = engine_alloc(c, m, (size_t)R * row_bytes, e)) return rc;
    DevBuf dnorms;
    const double* d_n2 = nullptr;
    if (const int rc = norms_on_device(c, norms_sq, mem_norms, s->n, dnorms, &d_n2)) return rc;
    DotsBlocks blocks;
    if (const int rc = blocks.init(c, s, rb, re, R, c->hclust_dots, {"k_hclust_fill dots", "hclust: dots launch rejected", "k_pairwise(hclust dots)"}))
        return rc;
    const auto fill = [&](int64_t r0, int64_t r1, const int32_t* dots) -> int {
        HCLUST_LAUNCH(mvs::launch_hclust_fill(c->stream, dots, r1 - r0, m, r0, rb, d_n2, s->d, floor, e.st.table + (r0 - rb) * e.st.ld, e.st.ld),
                      "k_hclust_fill");
        HIP_TRY(hipStreamSynchronize(c->stream));
        return MVS_OK;
    };
    if (const int rc = blocks.run(rb, re, &c->hc.dots_ms, &c->hc.fill_ms, nullptr, fill)) return rc;
    return engine_run(c, e, nullptr, method, false, merges, rounds);     // (a table of this fill is symmetric and bounded)
}

int mvs_hclust_order(int64_t m, const mvs_hmerge* merges, double* Z) {
    std::vector<int64_t> order;
    if (const int rc = sorted_merges(m, merges, order)) return rc;
    if (m == 1) return MVS_OK;
    if (!Z) return fail(MVS_E_INVALID, "Z is NULL");
    std::vector<int64_t> id((size_t)m);                          // of the cluster in a slot
    std::iota(id.begin(), id.end(), (int64_t)0);
    for (int64_t t = 0; t < m - 1; ++t) {
        const mvs_hmerge& r = merges[order[(size_t)t]];
        const int64_t x = id[(size_t)r.a], y = id[(size_t)r.b];
        double* z = Z + 4 * t;
        z[0] = (double)std::min(x, y);
        z[1] = (double)std::max(x, y);
        z[2] = r.height;
        z[3] = (double)r.size;
        id[(size_t)r.a] = m + t;
    }
    return MVS_OK;
}

int mvs_hclust_cut(int64_t m, const mvs_hmerge* merges, double height, int32_t* labels) {
    std::vector<int64_t> order;
    if (const int rc = sorted_merges(m, merges, order)) return rc;
    if (std::isnan(height)) return fail(MVS_E_INVALID, "height is NaN");
    if (!labels) return fail(MVS_E_INVALID, "labels is NULL");
    Forest f(m);
    for (int64_t t = 0; t < m - 1; ++t)
        if (merges[t].height <= height) f.join(merges[t].a, merges[t].b);
    f.labels(labels);
    return MVS_OK;
}

int mvs_hclust_cut_count(int64_t m, const mvs_hmerge* merges, int64_t k, int32_t* labels) {
    std::vector<int64_t> order;
    if (const int rc = sorted_merges(m, merges, order)) return rc;
    if (k < 1 || k > m) return fail(MVS_E_INVALID, "k = %lld outside 1 .. %lld", (long long)k, (long long)m);
    if (!labels) return fail(MVS_E_INVALID, "labels is NULL");
    Forest f(m);
    for (int64_t t = 0; t < m - k; ++t) f.join(merges[order[(size_t)t]].a, merges[order[(size_t)t]].b);
    f.labels(labels);
    return MVS_OK;
}

int mvs_ctx_hclust_stats(const mvs_ctx* c, double* dots_ms, double* fill_ms, double* nearest_ms, double* merge_ms, double* compact_ms,
                         int64_t* rounds, int64_t* row_scans, int64_t* bytes_scanned, int64_t* compactions) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (dots_ms) *dots_ms = c->hc.dots_ms;
    if (fill_ms) *fill_ms = c->hc.fill_ms;
    if (nearest_ms) *nearest_ms = c->hc.nearest_ms;
    if (merge_ms) *merge_ms = c->hc.merge_ms;
    if (compact_ms) *compact_ms = c->hc.compact_ms;
    if (rounds) *rounds = c->hc.rounds;
    if (row_scans) *row_scans = c->hc.row_scans;
    if (bytes_scanned) *bytes_scanned = c->hc.bytes_scanned;
    if (compactions) *compactions = c->hc.compactions;
    return MVS_OK;
}

}  // extern "C"
