// mvs_capi_hdbscan.hip -- C ABI of HDBSCAN* on the Jaccard estimates: mvs_core_jaccard (the K-th neighbour's score of every
// sample: mvs_pairwise_topk over row ranges, each range's cell list reduced on the device by mvs_core.hip), mvs_hdbscan_select
// (pure host: dendrogram of the links, condensed tree, selection by excess of mass -- integer levels, exact int64 stabilities),
// mvs_hdbscan (core, linkage under the mutual-reachability weight, finish, select) and mvs_ctx_hdbscan_stats.  The weight itself
// lives in mvs_linkage.hip (mvs_linkage_set_core); the contract is in include/mvs_hip.h "HDBSCAN*".
#include "mvs_capi_internal.h"
#include "mvs_core.h"

#include <hip/hip_runtime.h>

#include <cmath>

using namespace mvs_capi;

namespace {

constexpr int64_t kCoreCells = 1LL << 24;   // cells the core pass keeps on the device at a time (256 MiB)

// core[0 .. n) on the device from top-k over row ranges; d_n2, d_core: n doubles on the device
int core_pass(mvs_ctx* c, const mvs_sketch_set* s, const double* d_n2, int k, double* d_core) {
    const int64_t n = s->n;
    int64_t R = std::max<int64_t>(1, kCoreCells / k);
    if (c->core_block_rows > 0) R = std::min<int64_t>(R, c->core_block_rows);
    R = std::min(R, n);
    DevBuf dcells, dkeys, dcounts;
    HIP_TRY(dcells.alloc((size_t)R * (size_t)k * sizeof(mvs_cell)));
    HIP_TRY(dkeys.alloc((size_t)R * sizeof(unsigned long long)));
    HIP_TRY(dcounts.alloc((size_t)R * sizeof(int)));
    for (int64_t r0 = 0; r0 < n; r0 += R) {
        const int64_t r1 = std::min(r0 + R, n);
        int64_t m = 0;
        int rc = mvs_pairwise_topk(c, s, d_n2, MVS_MEM_DEVICE, k, r0, r1, 0, n, MVS_TOPK_EXCLUDE_SELF, (mvs_cell*)dcells.p, MVS_MEM_DEVICE, &m);
        if (rc) return rc;
        c->hd.core_dots_ms += c->tk.dots_ms;
        c->hd.core_select_ms += c->tk.work_ms;
        if (m > (r1 - r0) * (int64_t)k) return fail(MVS_E_INTERNAL, "top-k returned %lld cells for %lld rows at k = %d", (long long)m, (long long)(r1 - r0), k);
        StageTimer timer;
        rc = timer.begin(c);
        if (rc) return rc;
        rc = mvs::launch_core_kth(c->stream, (const mvs_cell*)dcells.p, m, r0, r1 - r0, k, d_n2, n, s->d, (unsigned long long*)dkeys.p,
                                  (int*)dcounts.p, d_core + r0);
        if (rc) return fail(rc, "core: reduction launch rejected");
        rc = check_kernel("k_core_kth");
        if (!rc) rc = timer.mark_end();
        if (!rc) rc = timer.add_to(&c->hd.core_kth_ms);
        if (rc) return rc;
        ++c->hd.ranges;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));   // (also before the DevBufs free the scratch)
    return MVS_OK;
}

int core_checks(const mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, int k) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (!mem_ok(mem_norms)) return fail(MVS_E_INVALID, "bad argument");
    if (k < 1 || k > mvs::kMaxTopk) return fail(MVS_E_INVALID, "min_samples = %d outside 1..%d", k, mvs::kMaxTopk);
    if ((int64_t)k > s->n - 1)
        return fail(MVS_E_INVALID, "min_samples = %d: a sample of a set of %lld has only %lld neighbours", k, (long long)s->n,
                    (long long)std::max<int64_t>(s->n - 1, 0));
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    return MVS_OK;
}

inline unsigned long long host_key(double J) {
    if (J == 0.0) J = 0.0;                                          // -0.0 -> +0.0
    unsigned long long u;
    std::memcpy(&u, &J, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
// a core value in key order, NaN below every number
inline unsigned long long core_rank(double v) { return v == v ? host_key(v) : 0ULL; }

inline int64_t level_of(double x) {
    const double y = x > 0.0 ? (x < 1.0 ? x : 1.0) : 0.0;             // min(max(x, 0), 1)
    return (int64_t)std::llrint(y * 1073741824.0);
}

struct Condensed {
    int32_t parent = -1, top = 0, size = 0, child[2] = {-1, -1};
    int64_t birth = 0, death = 0, stability = 0, lmax = 0, shat = 0;
    bool chosen = false, selected = false;
};

}  // namespace

extern "C" {

int mvs_core_jaccard(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, int k, double* core_out, int mem_out) {
    int rc = core_checks(c, s, norms_sq, mem_norms, k);
    if (rc) return rc;
    if (!mem_ok(mem_out) || !core_out) return fail(MVS_E_INVALID, "bad output buffer");
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_core_jaccard");
    c->hd.reset();
    DevBuf dnorms, dcore;
    const double* d_n2 = nullptr;
    rc = norms_on_device(c, norms_sq, mem_norms, s->n, dnorms, &d_n2);
    if (rc) return rc;
    double* d_core = core_out;
    if (mem_out == MVS_MEM_HOST) {
        HIP_TRY(dcore.alloc((size_t)s->n * sizeof(double)));
        d_core = (double*)dcore.p;
    }
    rc = core_pass(c, s, d_n2, k, d_core);
    if (rc) return rc;
    if (mem_out == MVS_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(core_out, d_core, (size_t)s->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return MVS_OK;
}

int mvs_hdbscan_select(int64_t n, const mvs_link* links, int64_t n_links, const double* core, double floor_, int64_t min_cluster_size,
                       int flags, int32_t* labels, double* strength, int64_t* lambda_out, mvs_hdbscan_cluster* clusters,
                       int64_t capacity, int64_t* n_clusters) {
    if (n_clusters) *n_clusters = 0;
    if (n < 0 || n >= (1LL << 31) - 256) return fail(MVS_E_INVALID, "n = %lld outside the int32 sample indices", (long long)n);
    if (n_links < 0 || (n_links > 0 && !links)) return fail(MVS_E_INVALID, "bad link list");
    if (!(floor_ == floor_)) return fail(MVS_E_INVALID, "floor is NaN");
    if (min_cluster_size < 2) return fail(MVS_E_INVALID, "min_cluster_size = %lld: a cluster holds at least 2 samples", (long long)min_cluster_size);
    if ((flags & ~MVS_HDBSCAN_NO_ROOTS) != 0 || capacity < 0) return fail(MVS_E_INVALID, "bad argument");
    const int64_t s = min_cluster_size;
    // ---- the dendrogram: Kruskal merges of the links with m > floor, in the given order (checked: best first) ----
    // nodes 0 .. n - 1 are the samples, n + i is the merge of link i
    std::vector<int32_t> uf((size_t)n), top((size_t)n);                // union-find over samples; the node on top of a root's component
    for (int64_t i = 0; i < n; ++i) uf[(size_t)i] = top[(size_t)i] = (int32_t)i;
    auto find = [&](int32_t x) {
        while (uf[(size_t)x] != x) {
            uf[(size_t)x] = uf[(size_t)uf[(size_t)x]];
            x = uf[(size_t)x];
        }
        return x;
    };
    std::vector<int32_t> left, right, nsize((size_t)n, 1), nmin((size_t)n), nrep((size_t)n);
    std::vector<int64_t> nlam;
    std::vector<char> has_parent((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) nmin[(size_t)i] = nrep[(size_t)i] = (int32_t)i;
    auto better_rep = [&](int32_t x, int32_t y) {                      // larger core in key order, then the smaller index
        if (core) {
            const unsigned long long kx = core_rank(core[x]), ky = core_rank(core[y]);
            if (kx != ky) return kx > ky ? x : y;
        }
        return x < y ? x : y;
    };
    int64_t merges = 0;
    bool below = false;                                                // a link at or under the floor has been seen
    for (int64_t i = 0; i < n_links; ++i) {
        const mvs_link& l = links[i];
        if (l.a < 0 || l.b < 0 || l.a >= n || l.b >= n || l.a == l.b) return fail(MVS_E_INVALID, "link %lld joins samples %d and %d of %lld", (long long)i, l.a, l.b, (long long)n);
        if (!(l.jaccard == l.jaccard)) return fail(MVS_E_INVALID, "link %lld has a NaN weight", (long long)i);
        if (i > 0) {
            const mvs_link& p = links[i - 1];
            const unsigned long long kp = host_key(p.jaccard), kl = host_key(l.jaccard);
            const bool ordered = kp > kl || (kp == kl && (p.a < l.a || (p.a == l.a && p.b < l.b)));
            if (!ordered) return fail(MVS_E_INVALID, "link %lld is not behind link %lld in the order (weight descending, a, b)", (long long)i, (long long)(i - 1));
        }
        const int32_t ra = find(l.a), rb = find(l.b);
        if (ra == rb) return fail(MVS_E_INVALID, "link %lld closes a cycle: the links are no forest", (long long)i);
        if (!(l.jaccard > floor_)) below = true;
        uf[(size_t)std::max(ra, rb)] = std::min(ra, rb);               // (cycles are checked among all links, merges made above the floor)
        if (below) continue;
        const int32_t v = (int32_t)(n + merges), x = top[(size_t)ra], y = top[(size_t)rb];
        left.push_back(x);
        right.push_back(y);
        nlam.push_back(level_of(l.jaccard));
        nsize.push_back(nsize[(size_t)x] + nsize[(size_t)y]);
        nmin.push_back(std::min(nmin[(size_t)x], nmin[(size_t)y]));
        nrep.push_back(better_rep(nrep[(size_t)x], nrep[(size_t)y]));
        has_parent[(size_t)x] = has_parent[(size_t)y] = 1;
        has_parent.push_back(0);
        top[(size_t)std::min(ra, rb)] = v;
        ++merges;
    }
    const int64_t nodes = n + merges;
    // ---- the condensed tree, top-down from every root of size >= s ----
    std::vector<Condensed> cl;
    std::vector<int64_t> lam((size_t)n, -1);
    std::vector<int32_t> last((size_t)n, -1);                          // the last cluster a sample was in
    std::vector<int32_t> walk;
    auto leave = [&](int32_t node, int32_t ci, int64_t at) {           // every sample under `node` leaves cluster ci at level `at`
        walk.assign(1, node);
        while (!walk.empty()) {
            const int32_t v = walk.back();
            walk.pop_back();
            if (v < n) {
                lam[(size_t)v] = at;
                last[(size_t)v] = ci;
            } else {
                walk.push_back(left[(size_t)(v - n)]);
                walk.push_back(right[(size_t)(v - n)]);
            }
        }
    };
    const int64_t birth0 = level_of(floor_);
    for (int64_t v = 0; v < nodes; ++v) {
        if (has_parent[(size_t)v] || nsize[(size_t)v] < s) continue;
        Condensed r;
        r.top = (int32_t)v;
        r.size = nsize[(size_t)v];
        r.birth = birth0;
        cl.push_back(r);
    }
    for (size_t ci = 0; ci < cl.size(); ++ci) {                        // (children are appended behind their parent)
        int32_t v = cl[ci].top;
        const int64_t birth = cl[ci].birth;
        int64_t stab = 0, death = birth;
        for (;;) {                                                     // v is a merge: its size is >= s >= 2
            const int32_t x = left[(size_t)(v - n)], y = right[(size_t)(v - n)];
            const int64_t at = nlam[(size_t)(v - n)];
            const bool bx = nsize[(size_t)x] >= s, by = nsize[(size_t)y] >= s;
            death = std::max(death, at);
            if (bx && by) {
                stab += (int64_t)nsize[(size_t)v] * (at - birth);
                for (int side = 0; side < 2; ++side) {
                    Condensed k;
                    k.parent = (int32_t)ci;
                    k.top = side ? y : x;
                    k.size = nsize[(size_t)k.top];
                    k.birth = at;
                    cl[ci].child[side] = (int32_t)cl.size();
                    cl.push_back(k);
                }
                break;
            }
            if (!bx && !by) {
                stab += (int64_t)nsize[(size_t)v] * (at - birth);
                leave(v, (int32_t)ci, at);
                break;
            }
            const int32_t small = bx ? y : x;
            stab += (int64_t)nsize[(size_t)small] * (at - birth);
            leave(small, (int32_t)ci, at);
            v = bx ? x : y;
        }
        cl[ci].stability = stab;
        cl[ci].death = death;
    }
    const int64_t m = (int64_t)cl.size();
    if (n_clusters) *n_clusters = m;
    // ---- selection by excess of mass, bottom-up; lmax on the way ----
    for (int64_t ci = m - 1; ci >= 0; --ci) {
        Condensed& k = cl[(size_t)ci];
        if (k.child[0] < 0) {
            k.lmax = k.death;
            k.shat = k.stability;
            k.chosen = true;
            continue;
        }
        const Condensed &a = cl[(size_t)k.child[0]], &b = cl[(size_t)k.child[1]];
        k.lmax = std::max(k.death, std::max(a.lmax, b.lmax));
        const int64_t sum = a.shat + b.shat;
        const bool barred = k.parent < 0 && (flags & MVS_HDBSCAN_NO_ROOTS) != 0;
        k.chosen = !barred && k.stability >= sum;
        k.shat = k.chosen ? k.stability : sum;
    }
    std::vector<char> covered((size_t)m, 0);                           // the cluster or one above it is selected
    for (int64_t ci = 0; ci < m; ++ci) {
        Condensed& k = cl[(size_t)ci];
        const bool above = k.parent >= 0 && covered[(size_t)k.parent];
        k.selected = k.chosen && !above;
        covered[(size_t)ci] = above || k.chosen;
    }
    // ---- output: records by (smallest member, size descending); labels, strengths, levels ----
    std::vector<int32_t> order((size_t)m), rank((size_t)m);
    for (int64_t i = 0; i < m; ++i) order[(size_t)i] = (int32_t)i;
    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        const int32_t mx = nmin[(size_t)cl[(size_t)x].top], my = nmin[(size_t)cl[(size_t)y].top];
        if (mx != my) return mx < my;
        if (cl[(size_t)x].size != cl[(size_t)y].size) return cl[(size_t)x].size > cl[(size_t)y].size;
        return x < y;
    });
    for (int64_t i = 0; i < m; ++i) rank[(size_t)order[(size_t)i]] = (int32_t)i;
    std::vector<int32_t> label_of((size_t)m, -1), owner((size_t)m, -1);   // a cluster's label; the selected cluster at or above it
    int32_t next_label = 0;
    for (int64_t i = 0; i < m; ++i)
        if (cl[(size_t)order[(size_t)i]].selected) label_of[(size_t)order[(size_t)i]] = next_label++;
    for (int64_t ci = 0; ci < m; ++ci) {
        const Condensed& k = cl[(size_t)ci];
        owner[(size_t)ci] = k.selected ? (int32_t)ci : (k.parent >= 0 ? owner[(size_t)k.parent] : -1);
    }
    for (int64_t i = 0; i < n; ++i) {
        const int32_t own = last[(size_t)i] >= 0 ? owner[(size_t)last[(size_t)i]] : -1;
        if (labels) labels[i] = own >= 0 ? label_of[(size_t)own] : -1;
        if (lambda_out) lambda_out[i] = lam[(size_t)i];
        if (strength) {
            double v = 0.0;
            if (own >= 0) {
                const Condensed& k = cl[(size_t)own];
                const int64_t den = k.lmax - k.birth;
                v = den == 0 ? 1.0 : (double)(std::min(lam[(size_t)i], k.lmax) - k.birth) / (double)den;
            }
            strength[i] = v;
        }
    }
    if (m > capacity && clusters) return fail(MVS_E_CAPACITY, "%lld condensed clusters, the buffer holds %lld", (long long)m, (long long)capacity);
    if (clusters) {
        for (int64_t i = 0; i < m; ++i) {
            const Condensed& k = cl[(size_t)order[(size_t)i]];
            mvs_hdbscan_cluster out;
            out.parent = k.parent >= 0 ? rank[(size_t)k.parent] : -1;
            out.size = k.size;
            out.selected = k.selected ? 1 : 0;
            out.representative = nrep[(size_t)k.top];
            out.birth = k.birth;
            out.death = k.death;
            out.stability = k.stability;
            clusters[i] = out;
        }
    }
    return MVS_OK;
}

int mvs_hdbscan(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, int min_samples, double floor_,
                int64_t min_cluster_size, int flags, double* core_out, mvs_link* links, int64_t* n_links, int32_t* labels, double* strength,
                int64_t* lambda_out, mvs_hdbscan_cluster* clusters, int64_t cluster_capacity, int64_t* n_clusters) {
    if (n_links) *n_links = 0;
    if (n_clusters) *n_clusters = 0;
    int rc = core_checks(c, s, norms_sq, mem_norms, min_samples);
    if (rc) return rc;
    if (!(floor_ > 0.0) || !(floor_ < 1.0)) return fail(MVS_E_INVALID, "floor = %g outside (0, 1)", floor_);
    if (min_cluster_size < 2) return fail(MVS_E_INVALID, "min_cluster_size = %lld: a cluster holds at least 2 samples", (long long)min_cluster_size);
    if ((flags & ~MVS_HDBSCAN_NO_ROOTS) != 0 || cluster_capacity < 0) return fail(MVS_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_hdbscan");
    c->hd.reset();
    const int64_t n = s->n;
    DevBuf dnorms, dcore;
    const double* d_n2 = nullptr;
    rc = norms_on_device(c, norms_sq, mem_norms, n, dnorms, &d_n2);
    if (rc) return rc;
    HIP_TRY(dcore.alloc((size_t)n * sizeof(double)));
    rc = core_pass(c, s, d_n2, min_samples, (double*)dcore.p);
    if (rc) return rc;
    std::vector<double> core((size_t)n);
    HIP_TRY(hipMemcpyAsync(core.data(), dcore.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (core_out) std::memcpy(core_out, core.data(), (size_t)n * sizeof(double));
    struct Holder {
        mvs_linkage* k = nullptr;
        ~Holder() {
            if (k) mvs_linkage_destroy(k);
        }
    } h;
    rc = mvs_linkage_create(c, n, s->d, d_n2, MVS_MEM_DEVICE, &h.k);
    if (!rc) rc = mvs_linkage_set_core(h.k, (const double*)dcore.p, MVS_MEM_DEVICE);
    if (!rc) rc = mvs_pairwise_linkage(c, s, d_n2, MVS_MEM_DEVICE, floor_, h.k);
    if (rc) return rc;
    std::vector<mvs_link> own;
    mvs_link* out = links;
    if (!out) {
        own.resize((size_t)std::max<int64_t>(n - 1, 1));
        out = own.data();
    }
    int64_t m = 0;
    rc = mvs_linkage_finish(h.k, out, std::max<int64_t>(n - 1, 0), MVS_MEM_HOST, &m);
    if (rc) return rc;
    if (n_links) *n_links = m;
    c->hd.compare_ms = c->lk.compare_ms;
    c->hd.forest_ms = c->lk.work_ms;
    c->hd.rounds = c->lk.rounds;
    c->hd.edges = c->lk.edges;
    c->hd.links = m;
    const auto t0 = std::chrono::steady_clock::now();
    rc = mvs_hdbscan_select(n, out, m, core.data(), floor_, min_cluster_size, flags, labels, strength, lambda_out, clusters, cluster_capacity,
                            n_clusters);
    c->hd.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int mvs_ctx_hdbscan_stats(const mvs_ctx* c, double* core_dots_ms, double* core_select_ms, double* core_kth_ms, double* compare_ms,
                          double* forest_ms, double* host_ms, int64_t* ranges, int64_t* rounds, int64_t* links, int64_t* edges) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (core_dots_ms) *core_dots_ms = c->hd.core_dots_ms;
    if (core_select_ms) *core_select_ms = c->hd.core_select_ms;
    if (core_kth_ms) *core_kth_ms = c->hd.core_kth_ms;
    if (compare_ms) *compare_ms = c->hd.compare_ms;
    if (forest_ms) *forest_ms = c->hd.forest_ms;
    if (host_ms) *host_ms = c->hd.host_ms;
    if (ranges) *ranges = c->hd.ranges;
    if (rounds) *rounds = c->hd.rounds;
    if (links) *links = c->hd.links;
    if (edges) *edges = c->hd.edges;
    return MVS_OK;
}

}  // extern "C"
