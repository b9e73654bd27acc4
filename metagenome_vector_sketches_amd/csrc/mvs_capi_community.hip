// mvs_capi_community.hip -- C ABI of the modularity communities: mvs_community_create / _add_cells / _add_edges / _finish /
// _destroy (a consumer of DEVICE cell lists or raw integer edges), mvs_pairwise_community (the one-call producer over
// feed_consumer), mvs_communities (everything in one call), mvs_community_modularity (pure host) and mvs_ctx_community_stats.
// The kernels are in mvs_community.hip; the rule is stated in include/mvs_hip.h "Communities".  The host drives the rounds: one
// read-back of five words per round decides whether the level goes on.
#include "mvs_capi_internal.h"
#include "mvs_community.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <map>

using namespace mvs_capi;

typedef __int128 i128;
typedef unsigned __int128 u128;
typedef unsigned long long u64;

struct mvs_community {
    mvs_ctx* ctx = nullptr;
    int64_t n = 0;
    int d = 0;
    double floor_ = 0.0;
    DevBuf d_n2;                             // double, or empty
    // the fed entries (lo << 32 | hi, a): `count` of them; `unique`: sorted, one per edge
    DevBuf keys;                             // u64
    DevBuf w;                                // uint32_t
    int64_t cap = 0, count = 0;
    bool unique = true;
    DevBuf counters;                         // u64 (mvs_community.hip): [0] entries, [1] out of range, [2] bad weights; [4..7] scratch words
    // level 0 (built by the first finish after a feed)
    bool built = false;
    int64_t m = 0;
    DevBuf row_ptr;                          // long long
    DevBuf src, col;                         // int32_t
    DevBuf w32;                              // uint32_t
    DevBuf self0, k0;                        // u64
    u64 W = 0;
};

namespace {

constexpr int kMaxLevels = MVS_COMMUNITY_MAX_LEVELS;
constexpr int kPatience = 3;
constexpr int kMaxUnionRounds = 64;
constexpr int64_t kSplitChunk = 1LL << 22;   // cells of the connected split per union-find pass

void drop_level0(mvs_community* k) {
    for (DevBuf* b : {&k->row_ptr, &k->src, &k->col, &k->w32, &k->self0, &k->k0}) b->reset();
    k->built = false;
    k->m = 0;
}

int ensure_room(mvs_community* k, int64_t extra) {
    if (k->count + extra <= k->cap) return MVS_OK;
    const int64_t cap = std::max<int64_t>({2 * k->cap, k->count + extra, 1024});
    DevBuf nk, nw;
    if (nk.alloc((size_t)cap * 8) != hipSuccess || nw.alloc((size_t)cap * 4) != hipSuccess)
        return fail(MVS_E_NOMEM, "hipMalloc of %lld graph entries failed", (long long)cap);
    mvs_ctx* c = k->ctx;
    if (k->count > 0) {
        HIP_TRY(hipMemcpyAsync(nk.p, k->keys.p, (size_t)k->count * 8, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(nw.p, k->w.p, (size_t)k->count * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    k->keys = std::move(nk);
    k->w = std::move(nw);
    k->cap = cap;
    return MVS_OK;
}

// what follows a feeding launch: the counters, the errors they name
int after_feed(mvs_community* k, const char* what) {
    mvs_ctx* c = k->ctx;
    u64 back[3] = {0, 0, 0};
    const int rc = read_back(c, c->stream, {{back, k->counters.as<u64>(), sizeof(back)}});
    if (rc) return rc;
    if ((int64_t)back[0] != k->count) {
        k->unique = false;
        drop_level0(k);
    }
    k->count = (int64_t)back[0];
    if (back[1] != 0)
        return fail(MVS_E_RANGE, "%llu %s name a sample outside [0, %lld): they were ignored", back[1], what, (long long)k->n);
    if (back[2] != 0) return fail(MVS_E_RANGE, "%llu edges have a weight outside [1, 2^20]: they were ignored", back[2]);
    return MVS_OK;
}

int consume_cells(mvs_community* k, const mvs_cell* d_cells, int64_t n_cells) {
    mvs_ctx* c = k->ctx;
    if (n_cells == 0) return MVS_OK;
    if (!k->d_n2.as<double>()) return fail(MVS_E_INVALID, "the graph was created without norms: it takes raw edges only");
    int rc = ensure_room(k, n_cells);
    if (rc) return rc;
    StageTimer timer;
    rc = timer.begin(c);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(k->counters.as<u64>() + 1, 0, 2 * sizeof(u64), c->stream));
    rc = mvs::launch_comm_cells(c->stream, d_cells, n_cells, k->n, k->d_n2.as<double>(), k->d, k->floor_, k->keys.as<u64>(),
                                k->w.as<uint32_t>(), k->counters.as<u64>());
    if (!rc) rc = check_kernel("k_comm_cells");
    if (!rc) rc = timer.mark_end();
    if (rc) return rc;
    rc = after_feed(k, "cells");
    const int rt = timer.add_to(&c->cm.build_ms);
    return rc ? rc : rt;
}

// the fed entries -> level 0
int build_level0(mvs_community* k) {
    mvs_ctx* c = k->ctx;
    if (k->built) return MVS_OK;
    drop_level0(k);
    StageTimer timer;
    int rc = timer.begin(c);
    if (rc) return rc;
    if (!k->unique && k->count > 0) {
        DevBuf tk, tw;
        HIP_TRY(tk.alloc((size_t)k->count * 8));
        HIP_TRY(tw.alloc((size_t)k->count * 4));
        rc = mvs::comm_unique_max(c->stream, k->keys.as<u64>(), k->w.as<uint32_t>(), k->count, (u64*)tk.p, (uint32_t*)tw.p,
                                  k->counters.as<u64>());
        if (rc) return fail(rc, "communities: sorting the fed cells failed");
        u64 left = 0;
        rc = read_back(c, c->stream, {{&left, k->counters.as<u64>(), 8}});
        if (rc) return rc;
        k->count = (int64_t)left;
    }
    k->unique = true;
    const int64_t n = k->n, e = k->count, m = 2 * e;
    const size_t mm = (size_t)std::max<int64_t>(m, 1), nn = (size_t)std::max<int64_t>(n, 1);
    if (k->row_ptr.alloc((nn + 1) * 8) != hipSuccess || k->src.alloc(mm * 4) != hipSuccess || k->col.alloc(mm * 4) != hipSuccess ||
        k->w32.alloc(mm * 4) != hipSuccess || k->self0.alloc(nn * 8) != hipSuccess || k->k0.alloc(nn * 8) != hipSuccess) {
        drop_level0(k);
        return fail(MVS_E_NOMEM, "hipMalloc of the graph of %lld edges failed", (long long)e);
    }
    {
        DevBuf dk, tk, tw;
        HIP_TRY(dk.alloc(mm * 8));
        HIP_TRY(tk.alloc(mm * 8));
        HIP_TRY(tw.alloc(mm * 4));
        rc = mvs::comm_mirror(c->stream, k->keys.as<u64>(), k->w.as<uint32_t>(), e, (u64*)dk.p, k->w32.as<uint32_t>(), (u64*)tk.p,
                              (uint32_t*)tw.p);
        if (rc) return fail(rc, "communities: sorting the directed entries failed");
        rc = mvs::launch_comm_csr(c->stream, (const u64*)dk.p, m, n, k->row_ptr.as<long long>(), k->src.as<int32_t>(), k->col.as<int32_t>());
        if (!rc) rc = check_kernel("k_comm_csr");
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    HIP_TRY(hipMemsetAsync(k->self0.as<u64>(), 0, nn * 8, c->stream));
    HIP_TRY(hipMemsetAsync(k->counters.as<u64>() + 4, 0, 8, c->stream));
    mvs::CommLevel g;
    g.n = n;
    g.m = m;
    g.row_ptr = k->row_ptr.as<long long>();
    g.src = k->src.as<int32_t>();
    g.col = k->col.as<int32_t>();
    g.w32 = k->w32.as<uint32_t>();
    g.self = k->self0.as<u64>();
    rc = mvs::launch_comm_strength(c->stream, g, k->k0.as<u64>(), k->counters.as<u64>() + 4);
    if (!rc) rc = check_kernel("k_comm_strength");
    if (!rc) rc = timer.mark_end();
    if (rc) return rc;
    rc = read_back(c, c->stream, {{&k->W, k->counters.as<u64>() + 4, 8}});
    if (!rc) rc = timer.add_to(&c->cm.build_ms);
    if (rc) return rc;
    k->m = m;
    k->built = true;
    return MVS_OK;
}

// a coarser level's arrays
struct LevelBufs {
    DevBuf row_ptr, src, col, w64, self, k;
};

i128 qnum_of(u64 W, u64 g, const u64* acc) {
    const u128 sumsq = ((u128)acc[3] << 64) + ((u128)acc[2] << 32) + (u128)acc[1];
    return (i128)(((u128)W << 12) * (u128)acc[0]) - (i128)((u128)g * sumsq);
}

}  // namespace

extern "C" {

int mvs_community_create(mvs_ctx* c, int64_t n, int d, const double* norms_sq, int mem_norms, double floor_, mvs_community** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n < 0) return fail(MVS_E_INVALID, "n = %lld is negative", (long long)n);
    if (n >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n too large for int32 sample indices");
    if (!(floor_ >= 0.0) || !(floor_ < 1.0)) return fail(MVS_E_INVALID, "floor = %g outside [0, 1)", floor_);
    if (norms_sq && (d < 1 || !mem_ok(mem_norms))) return fail(MVS_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<mvs_community> k(new (std::nothrow) mvs_community());
    if (!k) return fail(MVS_E_NOMEM, "out of host memory");
    k->ctx = c;
    k->n = n;
    k->d = d;
    k->floor_ = floor_;
    bool ok = k->counters.alloc(64) == hipSuccess && hipMemsetAsync(k->counters.p, 0, 64, c->stream) == hipSuccess;
    if (ok && norms_sq && n > 0)
        ok = k->d_n2.alloc((size_t)n * 8) == hipSuccess &&
             hipMemcpyAsync(k->d_n2.p, norms_sq, (size_t)n * 8, mem_norms == MVS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                            c->stream) == hipSuccess;
    if (ok) ok = hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) return fail(MVS_E_NOMEM, "hipMalloc of the graph of %lld samples failed", (long long)n);
    c->cm.reset();
    *out = k.release();
    return MVS_OK;
}

int mvs_community_add_cells(mvs_community* k, const mvs_cell* d_cells, int64_t n_cells) {
    if (!k) return fail(MVS_E_INVALID, "NULL graph");
    if (n_cells < 0 || (n_cells > 0 && !d_cells)) return fail(MVS_E_INVALID, "bad cell list");
    HIP_TRY(hipSetDevice(k->ctx->device));
    const Range range(k->ctx, "mvs_community_add_cells");
    return consume_cells(k, d_cells, n_cells);
}

int mvs_community_add_edges(mvs_community* k, const int32_t* lo, const int32_t* hi, const int32_t* a, int64_t n_edges, int mem) {
    if (!k) return fail(MVS_E_INVALID, "NULL graph");
    if (n_edges < 0 || !mem_ok(mem) || (n_edges > 0 && (!lo || !hi || !a))) return fail(MVS_E_INVALID, "bad edge list");
    if (n_edges == 0) return MVS_OK;
    mvs_ctx* c = k->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_community_add_edges");
    DevBuf stage;
    const int32_t *dlo = lo, *dhi = hi, *da = a;
    if (mem == MVS_MEM_HOST) {
        HIP_TRY(stage.alloc((size_t)n_edges * 12));
        int32_t* p = (int32_t*)stage.p;
        HIP_TRY(hipMemcpyAsync(p, lo, (size_t)n_edges * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(p + n_edges, hi, (size_t)n_edges * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(p + 2 * n_edges, a, (size_t)n_edges * 4, hipMemcpyHostToDevice, c->stream));
        dlo = p;
        dhi = p + n_edges;
        da = p + 2 * n_edges;
    }
    int rc = ensure_room(k, n_edges);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(k->counters.as<u64>() + 1, 0, 2 * sizeof(u64), c->stream));
    rc = mvs::launch_comm_edges(c->stream, dlo, dhi, da, n_edges, k->n, k->keys.as<u64>(), k->w.as<uint32_t>(), k->counters.as<u64>());
    if (!rc) rc = check_kernel("k_comm_edges");
    if (rc) return rc;
    return after_feed(k, "edges");
}

int mvs_pairwise_community(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double floor_, mvs_community* k) {
    const int rc = consumer_checks("community graph", c, s, k, mem_norms, floor_);
    if (rc) return rc;
    if (s->d != k->d) return fail(MVS_E_INVALID, "the graph was created for dimension %d, the sketch set has %d", k->d, s->d);
    // The comparison's keep test, double(P)/d > t/(1+t) * (n2r + n2c), and the rule's J > floor are one inequality in algebra and
    // differ in fp64 within a few doubles of the boundary (at floor 0.1, d = 384 the keep test drops pairs the rule calls edges:
    // tests/rule_edges_model.py).  The graph's edge set is the rule's alone: the comparison runs at a level 2^-40 (relative) below
    // the floor -- 2^12 times the disagreement -- so it keeps a superset, and k_comm_cells decides every kept cell with J > floor.
    const double feed_level = floor_ * (1.0 - 1.0 / 1099511627776.0);                    // (1 - 2^-40)
    ConsumerStats st;
    const int rf = feed_consumer("mvs_pairwise_community", c, s, norms_sq, mem_norms, feed_level, st,
                                 [k](const mvs_cell* d_cells, int64_t n_cells, int64_t, int64_t) { return consume_cells(k, d_cells, n_cells); });
    c->cm.compare_ms += st.compare_ms;
    c->cm.blocks += st.blocks;
    return rf;
}

int mvs_community_finish(mvs_community* k, double resolution, int64_t max_rounds, int32_t* labels, int32_t* level_labels,
                         int64_t level_capacity, int32_t* degree, uint64_t* strength, uint64_t* internal, uint64_t* total, int mem_out,
                         int64_t* level_communities, int64_t* level_rounds, uint64_t* level_qnum_hi, uint64_t* level_qnum_lo,
                         mvs_community_result* res) {
    if (!k) return fail(MVS_E_INVALID, "NULL graph");
    if (!mem_ok(mem_out) || level_capacity < 0) return fail(MVS_E_INVALID, "bad argument");
    if (!(resolution >= 1.0 / 4096.0) || !(resolution <= 16.0)) return fail(MVS_E_INVALID, "resolution = %g outside [2^-12, 16]", resolution);
    if (max_rounds < 1 || max_rounds > (1 << 30)) return fail(MVS_E_INVALID, "max_rounds = %lld outside [1, 2^30]", (long long)max_rounds);
    mvs_ctx* c = k->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_community_finish");
    const u64 gfix = (u64)std::llrint(resolution * 4096.0);
    mvs_community_result r;
    std::memset(&r, 0, sizeof(r));
    r.n = k->n;
    r.g_fixed = (int64_t)gfix;
    if (res) *res = r;
    int rc = build_level0(k);
    if (rc) return rc;
    r.edges = k->count;
    r.total_weight = k->W;
    c->cm.edges = k->count;
    if (res) *res = r;
    if (k->W >= (1ULL << 55)) return fail(MVS_E_RANGE, "the graph's total weight W = %llu is not below 2^55", k->W);
    const int64_t n = k->n;
    if (n == 0) return MVS_OK;

    // work arrays sized by level 0 (no level is larger)
    const size_t np1 = ((size_t)n + 1 + 63) / 64 * 64;
    DevBuf di, du, dtab, dacc;
    HIP_TRY(di.alloc(14 * np1 * 4));
    HIP_TRY(du.alloc(4 * np1 * 8));
    HIP_TRY(dacc.alloc(128));
    int32_t* p = (int32_t*)di.p;
    int32_t *d_comm = p, *d_next = p + np1, *d_best = p + 2 * np1, *d_size = p + 3 * np1, *d_l0 = p + 4 * np1, *d_l1 = p + 5 * np1,
            *d_l2 = p + 6 * np1, *d_o1 = p + 7 * np1, *d_o2 = p + 8 * np1, *d_minm = p + 9 * np1, *d_flag = p + 10 * np1,
            *d_ids = p + 11 * np1, *d_new = p + 12 * np1, *d_member = p + 13 * np1;
    u64* d_tot = (u64*)du.p;
    u64 *d_inner = d_tot + np1, *d_out_a = d_tot + 2 * np1, *d_out_b = d_tot + 3 * np1;
    u64* d_acc = (u64*)dacc.p;                          // [0..3] the apply's sums, [4] moves, [5] cross entries, [6] keys left
    unsigned int* d_counts = (unsigned int*)(d_acc + 8);  // [0..2] lists, [3] largest degree, [4] / [5] hand-overs, [6] never

    mvs::CommLevel g;
    g.n = n;
    g.m = k->m;
    g.row_ptr = k->row_ptr.as<long long>();
    g.src = k->src.as<int32_t>();
    g.col = k->col.as<int32_t>();
    g.w32 = k->w32.as<uint32_t>();
    g.self = k->self0.as<u64>();
    g.k = k->k0.as<u64>();
    const mvs::CommLevel g0 = g;
    std::unique_ptr<LevelBufs> cur;

    mvs::CommRound round;
    {
        const u128 RW = (u128)k->W << 12;
        round.rw_hi = (u64)(RW >> 64);
        round.rw_lo = (u64)RW;
        round.g = gfix;
    }
    std::vector<int32_t> host_levels;
    rc = mvs::launch_comm_identity(c->stream, d_member, n);
    if (rc) return rc;
    int levels = 0;
    for (;;) {
        // the lists of the three paths
        HIP_TRY(hipMemsetAsync(d_counts, 0, 32, c->stream));
        rc = mvs::launch_comm_classify(c->stream, g, c->community_path, d_l0, d_l1, d_l2, d_counts);
        if (!rc) rc = check_kernel("k_comm_classify");
        if (rc) return rc;
        unsigned int cnt[4] = {0, 0, 0, 0};
        rc = read_back(c, c->stream, {{cnt, d_counts, sizeof(cnt)}});
        if (rc) return rc;
        const int64_t c0 = cnt[0], c1 = cnt[1], c2 = cnt[2], maxdeg = cnt[3];
        for (int q = 0; q < 3; ++q) c->cm.paths[q] += cnt[q];
        const bool hand1 = c0 > 0 && maxdeg > mvs::kCommWaveSlots, hand2 = (c0 + c1) > 0 && maxdeg > mvs::kCommBlockSlots;
        int64_t slots = 64;
        int groups = 0;
        if (c2 > 0 || hand2) {
            while (slots < 2 * maxdeg) slots <<= 1;
            groups = (int)std::min<int64_t>(mvs::kCommGlobalGroups, std::max<int64_t>(c2, hand2 ? c0 + c1 : 0));
            if (dtab.p) HIP_TRY(hipStreamSynchronize(c->stream));
            if (dtab.alloc((size_t)groups * (size_t)slots * 12) != hipSuccess)
                return fail(MVS_E_NOMEM, "hipMalloc of %d tables of %lld slots failed", groups, (long long)slots);
        }
        // the singleton state is seen first
        rc = mvs::launch_comm_identity(c->stream, d_comm, g.n);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(d_acc, 0, 64, c->stream));
        rc = mvs::launch_comm_apply(c->stream, g, d_comm, d_tot, d_size, d_acc);
        if (!rc) rc = check_kernel("k_comm_apply");
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(d_best, d_comm, (size_t)g.n * 4, hipMemcpyDeviceToDevice, c->stream));
        u64 acc[5] = {0, 0, 0, 0, 0};
        rc = read_back(c, c->stream, {{acc, d_acc, sizeof(acc)}});
        if (rc) return rc;
        i128 best_q = qnum_of(k->W, gfix, acc);
        int stall = 0;
        int64_t rounds = 0;
        round.level = levels;
        for (;;) {
            round.round = (int)rounds;
            StageTimer timer;
            rc = timer.begin(c);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(d_next, d_comm, (size_t)g.n * 4, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemsetAsync(d_acc, 0, 64, c->stream));
            HIP_TRY(hipMemsetAsync(d_counts + 4, 0, 16, c->stream));
            rc = mvs::launch_comm_move(c->stream, g, 0, round, d_comm, d_next, d_tot, d_size, d_l0, d_counts + 0, c0, d_o1, d_counts + 4, nullptr,
                                       0, 0, d_acc + 4);
            if (!rc)
                rc = mvs::launch_comm_move(c->stream, g, 1, round, d_comm, d_next, d_tot, d_size, d_l1, d_counts + 1, c1, d_o2, d_counts + 5,
                                           nullptr, 0, 0, d_acc + 4);
            if (!rc && hand1)
                rc = mvs::launch_comm_move(c->stream, g, 1, round, d_comm, d_next, d_tot, d_size, d_o1, d_counts + 4, c0, d_o2, d_counts + 5,
                                           nullptr, 0, 0, d_acc + 4);
            if (!rc)
                rc = mvs::launch_comm_move(c->stream, g, 2, round, d_comm, d_next, d_tot, d_size, d_l2, d_counts + 2, c2, d_o1, d_counts + 6,
                                           dtab.p, slots, groups, d_acc + 4);
            if (!rc && hand2)
                rc = mvs::launch_comm_move(c->stream, g, 2, round, d_comm, d_next, d_tot, d_size, d_o2, d_counts + 5, c0 + c1, d_o1,
                                           d_counts + 6, dtab.p, slots, groups, d_acc + 4);
            if (!rc) rc = check_kernel("k_comm_move");
            if (!rc) rc = timer.mark_end();
            if (rc) return rc;
            // all moves together: tot, size and the sums of Qnum of the new state
            rc = mvs::launch_comm_apply(c->stream, g, d_next, d_tot, d_size, d_acc);
            if (!rc) rc = check_kernel("k_comm_apply");
            if (rc) return rc;
            unsigned int over[3] = {0, 0, 0};
            rc = read_back(c, c->stream, {{acc, d_acc, sizeof(acc)}, {over, d_counts + 4, sizeof(over)}});
            if (rc) return rc;
            double ms = 0.0;
            rc = timer.add_to(&ms);
            if (rc) return rc;
            c->cm.move_ms += ms;
            if (levels == 0) {
                c->cm.level0_move_ms += ms;
                ++c->cm.level0_rounds;
            }
            if (over[2] != 0) return fail(MVS_E_INTERNAL, "a table of 2 x degree slots filled up");
            c->cm.paths[3] += over[0];
            c->cm.paths[4] += over[1];
            std::swap(d_comm, d_next);
            ++rounds;
            const i128 q = qnum_of(k->W, gfix, acc);
            if (q > best_q) {
                best_q = q;
                stall = 0;
                HIP_TRY(hipMemcpyAsync(d_best, d_comm, (size_t)g.n * 4, hipMemcpyDeviceToDevice, c->stream));
            } else {
                ++stall;
            }
            if (acc[4] == 0 || stall >= kPatience || rounds >= max_rounds) break;
        }
        // the level's result: numbered by smallest member, composed with the levels below
        StageTimer atimer;
        rc = atimer.begin(c);
        if (rc) return rc;
        rc = mvs::comm_renumber(c->stream, d_best, g.n, d_minm, d_flag, d_ids, d_new);
        if (rc) return fail(rc, "communities: numbering failed");
        rc = mvs::launch_comm_compose(c->stream, d_member, n, d_new);
        if (!rc) rc = check_kernel("k_comm_compose");
        if (rc) return rc;
        int32_t count = 0;
        rc = read_back(c, c->stream, {{&count, d_ids + g.n, 4}});
        if (rc) return rc;
        if (level_labels && levels < level_capacity) {
            if (mem_out == MVS_MEM_HOST) {
                HIP_TRY(hipMemcpyAsync(level_labels + (size_t)levels * n, d_member, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
            } else {
                HIP_TRY(hipMemcpyAsync(level_labels + (size_t)levels * n, d_member, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
            }
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        if (levels < level_capacity) {
            if (level_communities) level_communities[levels] = count;
            if (level_rounds) level_rounds[levels] = rounds;
            if (level_qnum_hi) level_qnum_hi[levels] = (u64)((u128)best_q >> 64);
            if (level_qnum_lo) level_qnum_lo[levels] = (u64)(u128)best_q;
        }
        if (levels == 0) c->cm.level0_bytes = (long long)((g.n + 1) * 8 + g.m * 12);
        c->cm.rounds += rounds;
        r.rounds += rounds;
        ++levels;
        r.composed = count;
        if (count == g.n || levels >= kMaxLevels) {
            rc = atimer.mark_end();
            if (!rc) rc = atimer.add_to(&c->cm.aggregate_ms);
            if (rc) return rc;
            break;
        }
        // the next level's graph
        std::unique_ptr<LevelBufs> nxt(new LevelBufs());
        const size_t mm = (size_t)std::max<int64_t>(g.m, 1);
        DevBuf keys, tk, tv;
        HIP_TRY(keys.alloc(mm * 8));
        HIP_TRY(tk.alloc(mm * 8));
        HIP_TRY(tv.alloc(mm * 8));
        HIP_TRY(nxt->w64.alloc(mm * 8));
        HIP_TRY(nxt->self.alloc((size_t)count * 8));
        HIP_TRY(nxt->k.alloc((size_t)count * 8));
        HIP_TRY(nxt->row_ptr.alloc(((size_t)count + 1) * 8));
        HIP_TRY(hipMemsetAsync(nxt->self.p, 0, (size_t)count * 8, c->stream));
        HIP_TRY(hipMemsetAsync(d_acc + 5, 0, 24, c->stream));
        rc = mvs::launch_comm_aggregate(c->stream, g, d_new, (u64*)keys.p, (u64*)nxt->w64.p, (u64*)nxt->self.p, d_acc + 5);
        if (!rc) rc = check_kernel("k_comm_aggregate");
        if (rc) return rc;
        u64 cross = 0;
        rc = read_back(c, c->stream, {{&cross, d_acc + 5, 8}});
        if (rc) return rc;
        rc = mvs::comm_sum_by_key(c->stream, (u64*)keys.p, (u64*)nxt->w64.p, g.m, (int64_t)cross, (u64*)tk.p, (u64*)tv.p, d_acc + 6);
        if (rc) return fail(rc, "communities: summing the aggregated entries failed");
        u64 m2 = 0;
        rc = read_back(c, c->stream, {{&m2, d_acc + 6, 8}});
        if (rc) return rc;
        HIP_TRY(nxt->src.alloc((size_t)std::max<u64>(m2, 1) * 4));
        HIP_TRY(nxt->col.alloc((size_t)std::max<u64>(m2, 1) * 4));
        rc = mvs::launch_comm_csr(c->stream, (const u64*)keys.p, (int64_t)m2, count, (long long*)nxt->row_ptr.p, (int32_t*)nxt->src.p,
                                  (int32_t*)nxt->col.p);
        if (!rc) rc = check_kernel("k_comm_csr");
        if (rc) return rc;
        mvs::CommLevel g2;
        g2.n = count;
        g2.m = (int64_t)m2;
        g2.row_ptr = (const long long*)nxt->row_ptr.p;
        g2.src = (const int32_t*)nxt->src.p;
        g2.col = (const int32_t*)nxt->col.p;
        g2.w64 = (const u64*)nxt->w64.p;
        g2.self = (const u64*)nxt->self.p;
        HIP_TRY(hipMemsetAsync(d_acc + 7, 0, 8, c->stream));
        rc = mvs::launch_comm_strength(c->stream, g2, (u64*)nxt->k.p, d_acc + 7);
        if (!rc) rc = check_kernel("k_comm_strength");
        if (!rc) rc = atimer.mark_end();
        if (rc) return rc;
        u64 w2 = 0;
        rc = read_back(c, c->stream, {{&w2, d_acc + 7, 8}});      // (also before the DevBufs of this level free their arrays)
        if (!rc) rc = atimer.add_to(&c->cm.aggregate_ms);
        if (rc) return rc;
        if (w2 != k->W) return fail(MVS_E_INTERNAL, "the aggregated graph weighs %llu, the graph %llu", w2, k->W);
        g2.k = (const u64*)nxt->k.p;
        cur = std::move(nxt);
        g = g2;
    }
    r.levels = levels;
    c->cm.levels = levels;

    // the connected split: the components of the level-0 edges inside a community, over the union-find of mvs_cluster.hip
    {
        int32_t* parent = d_comm;                       // the level arrays are free again
        int32_t* dummy_degree = d_next;
        u64* cl_counters = d_acc + 8 + 4;               // three words behind the lists' counters
        rc = mvs::launch_cluster_init(c->stream, parent, dummy_degree, n);
        if (!rc) rc = check_kernel("k_cluster_init");
        if (rc) return rc;
        DevBuf cells;
        const int64_t chunk = std::min<int64_t>(kSplitChunk, std::max<int64_t>(g0.m, 1));
        HIP_TRY(cells.alloc((size_t)chunk * sizeof(mvs_cell)));
        for (int64_t e0 = 0; e0 < g0.m; e0 += chunk) {
            const int64_t e1 = std::min(g0.m, e0 + chunk);
            rc = mvs::launch_comm_split_cells(c->stream, g0, d_member, e0, e1, (mvs_cell*)cells.p);
            if (!rc) rc = check_kernel("k_comm_split_cells");
            if (rc) return rc;
            for (int pass = 1;; ++pass) {
                HIP_TRY(hipMemsetAsync(cl_counters, 0, 24, c->stream));
                rc = mvs::launch_cluster_hook(c->stream, (const mvs_cell*)cells.p, e1 - e0, parent, dummy_degree, n, false, cl_counters);
                if (!rc) rc = check_kernel("k_cluster_hook");
                if (!rc) rc = mvs::launch_cluster_flatten(c->stream, parent, n);
                if (!rc) rc = check_kernel("k_cluster_flatten");
                if (!rc) rc = mvs::launch_cluster_verify(c->stream, (const mvs_cell*)cells.p, e1 - e0, parent, n, cl_counters);
                if (!rc) rc = check_kernel("k_cluster_verify");
                if (rc) return rc;
                u64 apart = 0;
                rc = read_back(c, c->stream, {{&apart, cl_counters + 2, 8}});
                if (rc) return rc;
                if (apart == 0) break;
                if (pass >= kMaxUnionRounds)
                    return fail(MVS_E_HIP, "internal: %llu edges still join different trees after %d union-find rounds", apart, pass);
            }
        }
        rc = mvs::launch_cluster_flatten(c->stream, parent, n);
        if (!rc) rc = check_kernel("k_cluster_flatten");
        if (rc) return rc;
        // final labels by smallest member (a root is its tree's smallest member), the final Qnum, in(C) and tot(C)
        rc = mvs::comm_renumber(c->stream, parent, n, d_minm, d_flag, d_ids, d_new);
        if (rc) return fail(rc, "communities: numbering failed");
        HIP_TRY(hipMemsetAsync(d_acc, 0, 64, c->stream));
        rc = mvs::launch_comm_apply(c->stream, g0, parent, d_tot, d_size, d_acc);
        if (!rc) rc = check_kernel("k_comm_apply");
        if (!rc) rc = mvs::launch_comm_inner_by(c->stream, g0, parent, d_inner);
        if (!rc) rc = check_kernel("k_comm_inner_by");
        if (!rc) rc = mvs::launch_comm_gather_first(c->stream, parent, d_flag, d_ids, n, d_inner, d_tot, d_out_a, d_out_b);
        if (!rc) rc = check_kernel("k_comm_gather_first");
        if (!rc) rc = mvs::launch_comm_degree(c->stream, g0, d_size);
        if (!rc) rc = check_kernel("k_comm_degree");
        if (rc) return rc;
        u64 acc[4] = {0, 0, 0, 0};
        int32_t final_count = 0;
        rc = read_back(c, c->stream, {{acc, d_acc, sizeof(acc)}, {&final_count, d_ids + n, 4}});
        if (rc) return rc;
        const i128 q = qnum_of(k->W, gfix, acc);
        r.qnum_hi = (u64)((u128)q >> 64);
        r.qnum_lo = (u64)(u128)q;
        r.communities = final_count;
        rc = give_out(c, labels, d_new, n, mem_out);
        if (!rc) rc = give_out(c, degree, d_size, n, mem_out);
        if (!rc) rc = give_out(c, strength, k->k0.as<u64>(), n, mem_out);
        if (!rc) rc = give_out(c, internal, d_out_a, final_count, mem_out);
        if (!rc) rc = give_out(c, total, d_out_b, final_count, mem_out);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));       // (also before the DevBufs free the scratch)
    }
    if (res) *res = r;
    if (levels > level_capacity && (level_labels || level_communities || level_rounds || level_qnum_hi || level_qnum_lo))
        return fail(MVS_E_CAPACITY, "%d levels, room for %lld", levels, (long long)level_capacity);
    return MVS_OK;
}

int mvs_community_destroy(mvs_community* k) {
    if (!k) return MVS_OK;
    if (k->ctx) {
        (void)hipSetDevice(k->ctx->device);
        (void)hipStreamSynchronize(k->ctx->stream);
    }
    delete k;
    return MVS_OK;
}

int mvs_communities(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double floor_, double resolution,
                    int64_t max_rounds, int32_t* labels, int32_t* level_labels, int64_t level_capacity, int32_t* degree, uint64_t* strength,
                    uint64_t* internal, uint64_t* total, int mem_out, int64_t* level_communities, int64_t* level_rounds,
                    uint64_t* level_qnum_hi, uint64_t* level_qnum_lo, mvs_community_result* res) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (!norms_sq || !mem_ok(mem_norms)) return fail(MVS_E_INVALID, "bad argument");
    if (!(resolution >= 1.0 / 4096.0) || !(resolution <= 16.0)) return fail(MVS_E_INVALID, "resolution = %g outside [2^-12, 16]", resolution);
    if (!(floor_ > 0.0) || !(floor_ < 1.0)) return fail(MVS_E_INVALID, "floor = %g outside (0, 1)", floor_);
    mvs_community* k = nullptr;
    int rc = mvs_community_create(c, s->n, s->d, norms_sq, mem_norms, floor_, &k);
    if (rc) return rc;
    rc = mvs_pairwise_community(c, s, norms_sq, mem_norms, floor_, k);
    if (!rc)
        rc = mvs_community_finish(k, resolution, max_rounds, labels, level_labels, level_capacity, degree, strength, internal, total, mem_out,
                                  level_communities, level_rounds, level_qnum_hi, level_qnum_lo, res);
    mvs_community_destroy(k);
    return rc;
}

int mvs_community_modularity(int64_t n, const int32_t* lo, const int32_t* hi, const int64_t* a, int64_t n_edges, const int32_t* labels,
                             int64_t g_fixed, uint64_t* qnum_hi, uint64_t* qnum_lo) {
    if (n < 0 || n_edges < 0 || (n_edges > 0 && (!lo || !hi || !a)) || (n > 0 && !labels)) return fail(MVS_E_INVALID, "bad argument");
    if (g_fixed < 1 || g_fixed > 16 * 4096) return fail(MVS_E_INVALID, "g_fixed = %lld outside [1, 65536]", (long long)g_fixed);
    std::map<u64, u64> edges;
    for (int64_t i = 0; i < n_edges; ++i) {
        if (lo[i] < 0 || hi[i] < 0 || lo[i] >= n || hi[i] >= n) return fail(MVS_E_RANGE, "edge %lld names a sample outside [0, %lld)", (long long)i, (long long)n);
        if (a[i] < 1 || a[i] >= (1LL << 55)) return fail(MVS_E_RANGE, "edge %lld has a weight outside [1, 2^55)", (long long)i);
        if (lo[i] == hi[i]) continue;
        const u64 key = ((u64)(uint32_t)std::min(lo[i], hi[i]) << 32) | (u64)(uint32_t)std::max(lo[i], hi[i]);
        u64& slot = edges[key];
        slot = std::max<u64>(slot, (u64)a[i]);
    }
    u128 W = 0;
    u64 inner = 0;
    std::map<int32_t, u128> tot;
    for (const auto& e : edges) {
        const int32_t u = (int32_t)(e.first >> 32), v = (int32_t)(e.first & 0xffffffffULL);
        W += 2 * (u128)e.second;
        if (W >= ((u128)1 << 55)) return fail(MVS_E_RANGE, "the graph's total weight W is not below 2^55");
        tot[labels[u]] += e.second;
        tot[labels[v]] += e.second;
        if (labels[u] == labels[v]) inner += 2 * e.second;
    }
    u128 sumsq = 0;
    for (const auto& t : tot) sumsq += t.second * t.second;
    const i128 q = (i128)((W << 12) * (u128)inner) - (i128)((u128)g_fixed * sumsq);
    if (qnum_hi) *qnum_hi = (u64)((u128)q >> 64);
    if (qnum_lo) *qnum_lo = (u64)(u128)q;
    return MVS_OK;
}

int mvs_ctx_community_stats(const mvs_ctx* c, double* compare_ms, double* build_ms, double* move_ms, double* aggregate_ms,
                            double* level0_move_ms, int64_t* edges, int64_t* levels, int64_t* rounds, int64_t* row_blocks,
                            int64_t* level0_rounds, int64_t* level0_bytes, int64_t* paths) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    const CommunityStats& st = c->cm;
    if (compare_ms) *compare_ms = st.compare_ms;
    if (build_ms) *build_ms = st.build_ms;
    if (move_ms) *move_ms = st.move_ms;
    if (aggregate_ms) *aggregate_ms = st.aggregate_ms;
    if (level0_move_ms) *level0_move_ms = st.level0_move_ms;
    if (edges) *edges = st.edges;
    if (levels) *levels = st.levels;
    if (rounds) *rounds = st.rounds;
    if (row_blocks) *row_blocks = st.blocks;
    if (level0_rounds) *level0_rounds = st.level0_rounds;
    if (level0_bytes) *level0_bytes = st.level0_bytes;
    if (paths)
        for (int q = 0; q < 5; ++q) paths[q] = st.paths[q];
    return MVS_OK;
}

}  // extern "C"
