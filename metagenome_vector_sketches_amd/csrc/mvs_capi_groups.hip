// mvs_capi_groups.hip -- C ABI of the within-group sums of squared Jaccard distances and of the PERMANOVA built on them:
// mvs_group_sums, mvs_permutation_labels, mvs_permanova_stats, mvs_permanova, mvs_ctx_groups_stats.  The kernels and the weight
// of a cell are in mvs_groups.hip.
//
// Sums.  Rows are taken in blocks of R (dots_block_rows), clamped to R x m < 2^34: a block's partial
// per (slot, group) is at most R x m x 2^30 < 2^64.  Per block: the dense-dots kernels fill an R x m int32 block, k_dist_quantise
// turns it into weights in place, k_group_sums adds the block's ordered-pair sums to the cleared slots x groups accumulators,
// which come back and are added on the host in unsigned __int128.  The host halves at the end (the diagonal weighs 0 and w is
// symmetric, so an ordered-pair sum is even; an odd one is MVS_E_INTERNAL).  Device memory besides the set: R x m x 4 bytes of
// dots, the labels as given and sample-major, the accumulators -- never n x n.
//
// Statistic.  Pure host, fp64, one rounding per line (include/mvs_hip.h "PERMANOVA"); needs no device.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

#include <cmath>

using namespace mvs_capi;

namespace {

typedef unsigned __int128 u128;
constexpr uint64_t kGamma = 0x9e3779b97f4a7c15ULL;

inline uint64_t mix(uint64_t x) {
    x += kGamma;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

int label_checks(const uint8_t* labels, int64_t count, int groups) {
    uint8_t top = 0;
    for (int64_t i = 0; i < count; ++i) top = std::max(top, labels[i]);
    if (count > 0 && top >= groups) return fail(MVS_E_INVALID, "a label of %d with groups = %d", (int)top, groups);
    return MVS_OK;
}

// ss_within of one labelling: the terms S_g / n_g in ascending order of value, times 2^-30
double within_of(const uint64_t* lo, const uint64_t* hi, const int64_t* sizes, int groups, std::vector<double>& terms) {
    terms.clear();
    for (int g = 0; g < groups; ++g)
        if (sizes[g] > 0) {
            const u128 s = ((u128)(hi ? hi[g] : 0) << 64) | lo[g];
            const double num = (double)s;
            const double den = (double)sizes[g];
            terms.push_back(num / den);
        }
    std::sort(terms.begin(), terms.end());
    double sum = 0.0;
    for (const double t : terms) sum += t;
    return sum * 0x1p-30;
}

}  // namespace

extern "C" {

int mvs_group_sums(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double floor, int64_t rb, int64_t re,
                   const uint8_t* labels, int64_t slots, int groups, uint64_t* sums_lo, uint64_t* sums_hi, int64_t* sizes) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (!(floor >= 0.0) || !(floor < 1.0)) return fail(MVS_E_INVALID, "floor = %g outside [0, 1)", floor);
    if (!mem_ok(mem_norms)) return fail(MVS_E_INVALID, "bad argument");
    if (groups < 1 || groups > 255) return fail(MVS_E_INVALID, "groups = %d outside 1 .. 255", groups);
    if (slots < 1 || slots > MVS_MAX_GROUP_SLOTS) return fail(MVS_E_INVALID, "slots = %lld outside 1 .. %d", (long long)slots, MVS_MAX_GROUP_SLOTS);
    if (rb < 0 || re > s->n || rb > re) return fail(MVS_E_INVALID, "rows [%lld, %lld) outside the set's %lld samples", (long long)rb, (long long)re, (long long)s->n);
    if (!sums_lo) return fail(MVS_E_INVALID, "sums_lo is NULL");
    const int64_t m = re - rb;
    const size_t cells = (size_t)slots * groups;
    c->gs.reset();
    c->gs.slots = slots;
    std::memset(sums_lo, 0, cells * 8);
    if (sums_hi) std::memset(sums_hi, 0, cells * 8);
    if (sizes) std::memset(sizes, 0, cells * 8);
    if (m == 0) return MVS_OK;
    if (!labels) return fail(MVS_E_INVALID, "labels is NULL");
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    // the block's partial must fit 64 bits with at least one row per block: m x 2^30 x R < 2^64; the kernels index columns in int32
    if (m > INT32_MAX) return fail(MVS_E_INVALID, "%lld samples exceed the sums' range", (long long)m);
    if (const int rc = label_checks(labels, slots * m, groups)) return rc;
    Range mark(c, "mvs_group_sums");
    HIP_TRY(hipSetDevice(c->device));

    DevBuf dnorms, dlabels, dpacked, dacc;
    const double* d_n2 = nullptr;
    if (const int rc = norms_on_device(c, norms_sq, mem_norms, s->n, dnorms, &d_n2)) return rc;
    const int64_t quads = mvs::group_label_quads(slots);
    HIP_TRY(dlabels.alloc((size_t)slots * m));
    HIP_TRY(dpacked.alloc((size_t)m * quads * 4));
    HIP_TRY(dacc.alloc(cells * 8));
    HIP_TRY(hipMemcpyAsync(dlabels.p, labels, (size_t)slots * m, hipMemcpyHostToDevice, c->stream));
    {
        int rc = mvs::launch_labels_transpose(c->stream, (const uint8_t*)dlabels.p, slots, m, (uint32_t*)dpacked.p);
        if (rc) return fail(rc, "group sums: label launch rejected");
        rc = check_kernel("k_labels_transpose");
        if (rc) return rc;
    }
    // R x m < 2^34 keeps a block's partial per (slot, group), at most R x m x 2^30, inside 64 bits
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const int64_t R = std::min<int64_t>(dots_block_rows(free_b / 4, (size_t)m * 4, c->opt.groups_block_rows, m), ((1LL << 34) - 1) / m);
    DotsBlocks blocks;
    if (const int rc = blocks.init(c, s, rb, re, R, c->opt.groups_dots,
                                   {"k_group_sums dots", "group sums: dots launch rejected", "k_pairwise(group sums dots)"}))
        return rc;
    c->gs.block_rows = R;

    std::vector<u128> total(cells, 0);
    std::vector<unsigned long long> part(cells);
    bool sized = !sizes;
    // per block: the dots become weights in place, their sums come back (the one wait of a block) and are added
    const auto sum = [&](int64_t r0, int64_t r1, int32_t* dots) -> int {
        StageTimer t_quant, t_sums;
        if (const int rc = t_quant.begin(c)) return rc;
        {
            Range rq(c, "k_dist_quantise");
            int rc = mvs::launch_dist_quantise(c->stream, dots, r1 - r0, m, r0, rb, d_n2, s->d, floor);
            if (rc) return fail(rc, "group sums: quantise launch rejected");
            rc = check_kernel("k_dist_quantise");
            if (rc) return rc;
        }
        if (const int rc = t_quant.mark_end()) return rc;
        HIP_TRY(hipMemsetAsync(dacc.p, 0, cells * 8, c->stream));
        if (const int rc = t_sums.begin(c)) return rc;
        {
            Range rs(c, "k_group_sums");
            int rc = mvs::launch_group_sums(c->stream, (const uint32_t*)dots, r1 - r0, m, r0 - rb, (const uint32_t*)dpacked.p, slots, groups,
                                            (unsigned long long*)dacc.p);
            if (rc) return fail(rc, "group sums: launch rejected");
            rc = check_kernel("k_group_sums");
            if (rc) return rc;
        }
        if (const int rc = t_sums.mark_end()) return rc;
        HIP_TRY(hipMemcpyAsync(part.data(), dacc.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
        if (!sized) {                                            // the group sizes, while the first block runs
            for (int64_t sl = 0; sl < slots; ++sl)
                for (int64_t i = 0; i < m; ++i) ++sizes[(size_t)sl * groups + labels[(size_t)sl * m + i]];
            sized = true;
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < cells; ++i) total[i] += part[i];
        if (const int rc = t_quant.add_to(&c->gs.quantise_ms)) return rc;
        return t_sums.add_to(&c->gs.sums_ms);
    };
    if (const int rc = blocks.run(rb, re, &c->gs.dots_ms, nullptr, &c->gs.blocks, sum)) return rc;
    for (size_t i = 0; i < cells; ++i) {
        if (total[i] & 1) return fail(MVS_E_INTERNAL, "the ordered-pair sum of slot %lld, group %lld is odd", (long long)(i / groups), (long long)(i % groups));
        const u128 half = total[i] >> 1;
        sums_lo[i] = (uint64_t)half;
        if (sums_hi) sums_hi[i] = (uint64_t)(half >> 64);
        else if (half >> 64) return fail(MVS_E_INVALID, "a sum exceeds 64 bits and sums_hi is NULL");
    }
    return MVS_OK;
}

int mvs_permutation_labels(const uint8_t* labels, int64_t m, int64_t permutations, uint64_t seed, uint8_t* out) {
    if (m < 0 || permutations < 0) return fail(MVS_E_INVALID, "m = %lld, permutations = %lld", (long long)m, (long long)permutations);
    if (m == 0) return MVS_OK;
    if (!labels || !out) return fail(MVS_E_INVALID, "NULL argument");
    for (int64_t p = 0; p <= permutations; ++p) {
        uint8_t* o = out + (size_t)p * m;
        std::memcpy(o, labels, (size_t)m);
        if (p == 0) continue;
        uint64_t state = mix(seed ^ mix((uint64_t)p));
        for (int64_t i = m - 1; i >= 1; --i) {
            const uint64_t r = mix(state) % (uint64_t)(i + 1);
            state += kGamma;
            std::swap(o[i], o[r]);
        }
    }
    return MVS_OK;
}

int mvs_permanova_stats(const uint64_t* sums_lo, const uint64_t* sums_hi, const int64_t* sizes, int64_t permutations, int groups, int64_t m,
                        mvs_permanova_result* out, double* group_mean_d2, double* perm_f) {
    if (!sums_lo || !sizes || !out) return fail(MVS_E_INVALID, "NULL argument");
    if (groups < 1 || groups > 255) return fail(MVS_E_INVALID, "groups = %d outside 1 .. 255", groups);
    if (permutations < 0) return fail(MVS_E_INVALID, "permutations = %lld < 0", (long long)permutations);
    int64_t G = 0, covered = 0;
    for (int g = 0; g < groups; ++g) {
        if (sizes[g] < 0) return fail(MVS_E_INVALID, "a negative group size");
        G += sizes[g] > 0;
        covered += sizes[g];
    }
    if (covered != m) return fail(MVS_E_INVALID, "the group sizes add up to %lld, not %lld", (long long)covered, (long long)m);
    if (G < 2 || G >= m) return fail(MVS_E_INVALID, "%lld non-empty groups of %lld samples: PERMANOVA needs 2 <= groups < samples", (long long)G, (long long)m);
    const size_t last = (size_t)(permutations + 1) * groups;
    if (sizes[last] != m) return fail(MVS_E_INVALID, "the last slot is not the all-zero labelling");
    std::vector<double> terms;
    auto within = [&](int64_t slot) {
        const size_t at = (size_t)slot * groups;
        return within_of(sums_lo + at, sums_hi ? sums_hi + at : nullptr, sizes + at, groups, terms);
    };
    const u128 s_all = ((u128)(sums_hi ? sums_hi[last] : 0) << 64) | sums_lo[last];
    const double all_num = (double)s_all;
    const double all_mean = all_num / (double)m;
    const double ss_total = all_mean * 0x1p-30;
    const double df_b = (double)(G - 1), df_w = (double)(m - G);
    auto f_of = [&](double ssw) {
        const double ssb = ss_total - ssw;
        const double msb = ssb / df_b;
        const double msw = ssw / df_w;
        return msb / msw;
    };
    const double ssw0 = within(0);
    int64_t reached = 0;
    for (int64_t p = 1; p <= permutations; ++p) {
        const double ssw = within(p);
        reached += ssw <= ssw0;
        if (perm_f) perm_f[p - 1] = f_of(ssw);
    }
    out->ss_total = ss_total;
    out->ss_within = ssw0;
    out->ss_between = ss_total - ssw0;
    out->f = f_of(ssw0);
    out->r2 = out->ss_between / ss_total;
    out->p_value = (double)(1 + reached) / (double)(permutations + 1);
    out->df_between = G - 1;
    out->df_within = m - G;
    out->samples = m;
    out->groups = G;
    out->permutations = permutations;
    if (group_mean_d2)
        for (int g = 0; g < groups; ++g) {
            const int64_t n = sizes[g];
            if (n < 2) {
                group_mean_d2[g] = 0.0;
                continue;
            }
            const u128 sg = ((u128)(sums_hi ? sums_hi[g] : 0) << 64) | sums_lo[g];
            const double num = (double)sg;
            const double pairs = (double)(n * (n - 1) / 2);
            const double mean = num / pairs;
            group_mean_d2[g] = mean * 0x1p-30;
        }
    return MVS_OK;
}

int mvs_permanova(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double floor, int64_t rb, int64_t re,
                  const uint8_t* labels, int groups, int64_t permutations, uint64_t seed, mvs_permanova_result* out, int64_t* group_sizes,
                  double* group_mean_d2, double* perm_f) {
    if (!c || !s || !out) return fail(MVS_E_INVALID, "NULL argument");
    if (groups < 1 || groups > 255) return fail(MVS_E_INVALID, "groups = %d outside 1 .. 255", groups);
    if (permutations < 0 || permutations > MVS_MAX_GROUP_SLOTS - 2)
        return fail(MVS_E_INVALID, "permutations = %lld outside 0 .. %d", (long long)permutations, MVS_MAX_GROUP_SLOTS - 2);
    if (rb < 0 || re > s->n || rb > re) return fail(MVS_E_INVALID, "rows [%lld, %lld) outside the set's %lld samples", (long long)rb, (long long)re, (long long)s->n);
    if (!(floor >= 0.0) || !(floor < 1.0)) return fail(MVS_E_INVALID, "floor = %g outside [0, 1)", floor);
    if (!mem_ok(mem_norms)) return fail(MVS_E_INVALID, "bad argument");
    const int64_t m = re - rb;
    if (m > 0 && !labels) return fail(MVS_E_INVALID, "labels is NULL");
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    if (const int rc = label_checks(labels, m, groups)) return rc;
    std::vector<int64_t> count((size_t)groups, 0);
    for (int64_t i = 0; i < m; ++i) ++count[labels[i]];
    int64_t G = 0;
    for (const int64_t n : count) G += n > 0;
    if (G < 2 || G >= m) return fail(MVS_E_INVALID, "%lld non-empty groups of %lld samples: PERMANOVA needs 2 <= groups < samples", (long long)G, (long long)m);
    const int64_t slots = permutations + 2;
    const size_t cells = (size_t)slots * groups;
    std::vector<uint8_t> all((size_t)slots * m, 0);              // the last slot stays all zeros
    if (const int rc = mvs_permutation_labels(labels, m, permutations, seed, all.data())) return rc;
    std::vector<uint64_t> lo(cells), hi(cells);
    std::vector<int64_t> sizes(cells);
    if (const int rc = mvs_group_sums(c, s, norms_sq, mem_norms, floor, rb, re, all.data(), slots, groups, lo.data(), hi.data(), sizes.data())) return rc;
    if (const int rc = mvs_permanova_stats(lo.data(), hi.data(), sizes.data(), permutations, groups, m, out, group_mean_d2, perm_f)) return rc;
    if (group_sizes) std::memcpy(group_sizes, sizes.data(), (size_t)groups * 8);
    return MVS_OK;
}

int mvs_ctx_groups_stats(const mvs_ctx* c, double* dots_ms, double* quantise_ms, double* sums_ms, int64_t* row_blocks, int64_t* block_rows,
                         int64_t* slots) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (dots_ms) *dots_ms = c->gs.dots_ms;
    if (quantise_ms) *quantise_ms = c->gs.quantise_ms;
    if (sums_ms) *sums_ms = c->gs.sums_ms;
    if (row_blocks) *row_blocks = c->gs.blocks;
    if (block_rows) *block_rows = c->gs.block_rows;
    if (slots) *slots = c->gs.slots;
    return MVS_OK;
}

}  // extern "C"
