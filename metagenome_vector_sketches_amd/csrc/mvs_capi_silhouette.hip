// mvs_capi_silhouette.hip -- C ABI of the quality of a labelling on the Jaccard estimates: mvs_label_sums,
// mvs_silhouette_stats, mvs_silhouette, mvs_ctx_label_stats (include/mvs_hip.h "Labelling quality").  The kernel is in
// mvs_labelsum.hip, the weight of a cell in mvs_weight_dev.h.
//
// Sums.  The host sorts the samples of the range by label (stable, unlabelled last) and gathers the set and the norms into that
// order: every non-empty group is then one interval of columns, and the columns of every dots launch are the labelled samples
// [0, m_labelled) alone -- unlabelled samples are rows, never columns.  Rows go in blocks of dots_block_rows
// (nothing is summed across rows, so there is no R x m clamp); per block one dense-dots launch and k_segment_nearest, which
// leaves (own_sum, near_group, near_sum) per row.  The three arrays come back once, at the end, and are scattered through the
// permutation: O(m) bytes cross the link.  Device memory besides the set: the gathered copy, one dots block, O(m) arrays.
//
// Statistic.  Pure host, fp64, one rounding per line; needs no device.
#include "mvs_capi_internal.h"
#include "mvs_labelsum.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

using namespace mvs_capi;

namespace {

typedef unsigned __int128 u128;

// sizes[groups] of the labelling, or MVS_E_INVALID for a label outside [-1, groups)
int count_labels(const int32_t* labels, int64_t m, int groups, std::vector<int64_t>& sizes) {
    sizes.assign((size_t)groups, 0);
    for (int64_t i = 0; i < m; ++i) {
        const int32_t g = labels[i];
        if (g < -1 || g >= groups) return fail(MVS_E_INVALID, "label %d of sample %lld outside [-1, %d)", (int)g, (long long)i, groups);
        if (g >= 0) ++sizes[(size_t)g];
    }
    return MVS_OK;
}

struct OrderedSet {
    mvs_sketch_set* set = nullptr;
    ~OrderedSet() {
        if (set) mvs_sketch_set_destroy(set);
    }
};

}  // namespace

extern "C" {

int mvs_label_sums(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double floor, int64_t rb, int64_t re,
                   const int32_t* labels, int groups, uint64_t* own_sum, int32_t* near_group, uint64_t* near_sum, int64_t* sizes) {
    if (!c || !s) return fail(MVS_E_INVALID, "NULL argument");
    if (!(floor >= 0.0) || !(floor < 1.0)) return fail(MVS_E_INVALID, "floor = %g outside [0, 1)", floor);
    if (!mem_ok(mem_norms)) return fail(MVS_E_INVALID, "bad argument");
    if (groups < 1) return fail(MVS_E_INVALID, "groups = %d < 1", groups);
    if (rb < 0 || re > s->n || rb > re) return fail(MVS_E_INVALID, "rows [%lld, %lld) outside the set's %lld samples", (long long)rb, (long long)re, (long long)s->n);
    if (s->ctx != c) return fail(MVS_E_INVALID, "the sketch set belongs to another context");
    const int64_t m = re - rb;
    c->ls.reset();
    if (sizes) std::memset(sizes, 0, (size_t)groups * 8);
    if (m == 0) return MVS_OK;
    if (!labels) return fail(MVS_E_INVALID, "labels is NULL");
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    if (!own_sum || !near_group || !near_sum) return fail(MVS_E_INVALID, "an output array is NULL");
    // a row's sum is at most m x 2^30; the kernel indexes columns in int32
    if (m > INT32_MAX) return fail(MVS_E_INVALID, "%lld samples exceed the sums' range", (long long)m);
    std::vector<int64_t> count;
    if (const int rc = count_labels(labels, m, groups, count)) return rc;
    if (sizes) std::memcpy(sizes, count.data(), (size_t)groups * 8);

    // the stable order by label, unlabelled last; the non-empty groups become segments in ascending id
    std::vector<int32_t> seg_of((size_t)groups, -1), seg_begin(1, 0), seg_id;
    for (int g = 0; g < groups; ++g)
        if (count[(size_t)g] > 0) {
            seg_of[(size_t)g] = (int32_t)seg_id.size();
            seg_id.push_back(g);
            seg_begin.push_back(seg_begin.back() + (int32_t)count[(size_t)g]);
        }
    const int64_t m_lab = seg_begin.back();
    for (int64_t i = 0; i < m; ++i) {
        own_sum[i] = 0;
        near_group[i] = -1;
        near_sum[i] = 0;
    }
    if (m_lab == 0) return MVS_OK;                               // nobody to be near to
    std::vector<int32_t> order((size_t)m), col_seg((size_t)m_lab);
    {
        std::vector<int32_t> next(seg_begin.begin(), seg_begin.end() - 1);
        int64_t tail = m_lab;
        for (int64_t i = 0; i < m; ++i) {
            const int32_t g = labels[i];
            const int64_t at = g < 0 ? tail++ : next[(size_t)seg_of[(size_t)g]]++;
            order[(size_t)at] = (int32_t)i;
            if (g >= 0) col_seg[(size_t)at] = seg_of[(size_t)g];
        }
    }
    Range mark(c, "mvs_label_sums");
    HIP_TRY(hipSetDevice(c->device));

    // the norms of the range, in that order
    std::vector<double> n2h((size_t)m), n2o((size_t)m);
    if (mem_norms == MVS_MEM_DEVICE) {
        HIP_TRY(hipMemcpyAsync(n2h.data(), norms_sq + rb, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
        std::memcpy(n2h.data(), norms_sq + rb, (size_t)m * 8);
    }
    for (int64_t k = 0; k < m; ++k) n2o[(size_t)k] = n2h[(size_t)order[(size_t)k]];
    // ... and the set
    OrderedSet ordered;
    {
        std::vector<int32_t> rows((size_t)m);
        for (int64_t k = 0; k < m; ++k) rows[(size_t)k] = (int32_t)(rb + order[(size_t)k]);
        StageTimer t_gather;
        if (const int rc = t_gather.begin(c)) return rc;
        if (const int rc = mvs_sketch_set_gather(c, s, rows.data(), MVS_MEM_HOST, m, &ordered.set)) return rc;
        if (const int rc = t_gather.mark_end()) return rc;
        if (const int rc = t_gather.add_to(&c->ls.gather_ms)) return rc;
    }
    const mvs_sketch_set* o = ordered.set;

    DevBuf dnorms, dcolseg, dbegin, did, down, dnear, dnsum;
    const size_t segs = seg_id.size();
    HIP_TRY(dnorms.alloc((size_t)m * 8));
    HIP_TRY(dcolseg.alloc((size_t)m_lab * 4));
    HIP_TRY(dbegin.alloc((segs + 1) * 4));
    HIP_TRY(did.alloc(segs * 4));
    HIP_TRY(down.alloc((size_t)m * 8));
    HIP_TRY(dnear.alloc((size_t)m * 4));
    HIP_TRY(dnsum.alloc((size_t)m * 8));
    HIP_TRY(hipMemcpyAsync(dnorms.p, n2o.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dcolseg.p, col_seg.data(), (size_t)m_lab * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dbegin.p, seg_begin.data(), (segs + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(did.p, seg_id.data(), segs * 4, hipMemcpyHostToDevice, c->stream));

    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const int64_t R = dots_block_rows(free_b / 4, (size_t)m_lab * 4, c->labels_block_rows, m);
    DotsBlocks blocks;
    if (const int rc = blocks.init(c, o, 0, m_lab, R, c->labels_dots,
                                   {"k_segment_nearest dots", "label sums: dots launch rejected", "k_pairwise(label sums dots)"}))
        return rc;
    c->ls.block_rows = R;

    const auto reduce = [&](int64_t r0, int64_t r1, const int32_t* dots) -> int {
        Range rs(c, "k_segment_nearest");
        const int rc = mvs::launch_segment_nearest(c->stream, dots, r1 - r0, m_lab, r0, (const double*)dnorms.p, o->d, floor,
                                                   (const int32_t*)dcolseg.p, (const int32_t*)dbegin.p, (const int32_t*)did.p,
                                                   (unsigned long long*)down.p, (int32_t*)dnear.p, (unsigned long long*)dnsum.p);
        if (rc) return fail(rc, "label sums: launch rejected");
        return check_kernel("k_segment_nearest");
    };
    if (const int rc = blocks.run(0, m, &c->ls.dots_ms, &c->ls.reduce_ms, &c->ls.blocks, reduce)) return rc;
    // back, and through the permutation
    std::vector<uint64_t> h_own((size_t)m), h_nsum((size_t)m);
    std::vector<int32_t> h_near((size_t)m);
    HIP_TRY(hipMemcpyAsync(h_own.data(), down.p, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_near.data(), dnear.p, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_nsum.data(), dnsum.p, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int64_t k = 0; k < m; ++k) {
        const int32_t i = order[(size_t)k];
        own_sum[i] = h_own[(size_t)k];
        near_group[i] = h_near[(size_t)k];
        near_sum[i] = h_nsum[(size_t)k];
    }
    return MVS_OK;
}

int mvs_silhouette_stats(const int32_t* labels, int64_t m, int groups, const int64_t* sizes, const uint64_t* own_sum,
                         const int32_t* near_group, const uint64_t* near_sum, mvs_silhouette_result* out, double* s, double* a, double* b,
                         double* centroid_d2, double* group_mean_s, double* group_within, double* group_dispersion, int64_t* medoids) {
    if (!labels || !sizes || !own_sum || !near_group || !near_sum || !out) return fail(MVS_E_INVALID, "NULL argument");
    if (groups < 1) return fail(MVS_E_INVALID, "groups = %d < 1", groups);
    if (m < 0) return fail(MVS_E_INVALID, "m = %lld < 0", (long long)m);
    std::vector<int64_t> count;
    if (const int rc = count_labels(labels, m, groups, count)) return rc;
    int64_t G = 0, labelled = 0;
    for (int g = 0; g < groups; ++g) {
        if (sizes[g] != count[(size_t)g]) return fail(MVS_E_INVALID, "sizes[%d] = %lld, the labels hold %lld", g, (long long)sizes[g], (long long)count[(size_t)g]);
        G += sizes[g] > 0;
        labelled += sizes[g];
    }
    if (G < 2) return fail(MVS_E_INVALID, "%lld non-empty groups: a silhouette needs at least two", (long long)G);
    for (int64_t i = 0; i < m; ++i) {
        const int32_t h = near_group[i];
        if (h < 0 || h >= groups || sizes[h] == 0 || h == labels[i])
            return fail(MVS_E_INVALID, "near_group[%lld] = %d is not another non-empty group", (long long)i, (int)h);
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // W_g: half the group's sum of own sums, in 128 bits; the medoids
    std::vector<u128> within((size_t)groups, 0);
    std::vector<int64_t> medoid((size_t)groups, -1);
    for (int64_t i = 0; i < m; ++i) {
        const int32_t g = labels[i];
        if (g < 0) continue;
        within[(size_t)g] += own_sum[i];
        if (medoid[(size_t)g] < 0 || own_sum[i] < own_sum[medoid[(size_t)g]]) medoid[(size_t)g] = i;
    }
    std::vector<double> centre((size_t)groups, 0.0);             // ((double)W_g / n_g) / n_g
    for (int g = 0; g < groups; ++g) {
        if (within[(size_t)g] & 1) return fail(MVS_E_INTERNAL, "the sum of the own sums of group %d is odd", g);
        within[(size_t)g] >>= 1;
        if (sizes[g] > 0) {
            const double wg = (double)within[(size_t)g];
            const double per = wg / (double)sizes[g];
            centre[(size_t)g] = per / (double)sizes[g];
        }
    }
    std::vector<double> sum_s((size_t)groups, 0.0), sum_c((size_t)groups, 0.0);
    double all_s = 0.0;
    int64_t negative = 0;
    for (int64_t i = 0; i < m; ++i) {
        const int32_t g = labels[i];
        const double bn = (double)near_sum[i] / (double)sizes[near_group[i]];
        const double bi = bn * 0x1p-30;
        double ai = nan, si = nan, ci = nan;
        if (g >= 0) {
            const int64_t n = sizes[g];
            const double own = (double)own_sum[i];
            if (n > 1) {
                const double an = own / (double)(n - 1);
                ai = an * 0x1p-30;
                const double diff = bi - ai;
                const double top = ai > bi ? ai : bi;
                si = top == 0.0 ? 0.0 : diff / top;
            } else {
                ai = 0.0;
                si = 0.0;
            }
            const double mine = own / (double)n;
            const double off = mine - centre[(size_t)g];
            ci = off * 0x1p-30;
            sum_s[(size_t)g] += si;
            sum_c[(size_t)g] += ci;
            all_s += si;
            negative += si < 0.0;
        }
        if (s) s[i] = si;
        if (a) a[i] = ai;
        if (b) b[i] = bi;
        if (centroid_d2) centroid_d2[i] = ci;
    }
    for (int g = 0; g < groups; ++g) {
        const int64_t n = sizes[g];
        if (group_mean_s) group_mean_s[g] = n > 0 ? sum_s[(size_t)g] / (double)n : nan;
        if (group_dispersion) group_dispersion[g] = n > 0 ? sum_c[(size_t)g] / (double)n : nan;
        if (group_within) {
            if (n < 2) {
                group_within[g] = 0.0;
            } else {
                const double num = (double)within[(size_t)g];
                const double pairs = (double)(n * (n - 1) / 2);
                const double mean = num / pairs;
                group_within[g] = mean * 0x1p-30;
            }
        }
        if (medoids) medoids[g] = medoid[(size_t)g];
    }
    out->mean = all_s / (double)labelled;
    out->negative = negative;
    out->samples = m;
    out->labelled = labelled;
    out->groups = G;
    return MVS_OK;
}

int mvs_silhouette(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, double floor, int64_t rb, int64_t re,
                   const int32_t* labels, int groups, mvs_silhouette_result* out, int64_t* group_sizes, int32_t* nearest, double* sil, double* a,
                   double* b, double* centroid_d2, double* group_mean_s, double* group_within, double* group_dispersion, int64_t* medoids) {
    if (!c || !s || !out) return fail(MVS_E_INVALID, "NULL argument");
    if (groups < 1) return fail(MVS_E_INVALID, "groups = %d < 1", groups);
    if (rb < 0 || re > s->n || rb > re) return fail(MVS_E_INVALID, "rows [%lld, %lld) outside the set's %lld samples", (long long)rb, (long long)re, (long long)s->n);
    const int64_t m = re - rb;
    if (m > 0 && !labels) return fail(MVS_E_INVALID, "labels is NULL");
    std::vector<int64_t> count;
    if (const int rc = count_labels(labels, m, groups, count)) return rc;
    int64_t G = 0;
    for (const int64_t n : count) G += n > 0;
    if (G < 2) return fail(MVS_E_INVALID, "%lld non-empty groups: a silhouette needs at least two", (long long)G);
    std::vector<uint64_t> own((size_t)m), nsum((size_t)m);
    std::vector<int32_t> near((size_t)m);
    std::vector<int64_t> sizes((size_t)groups);
    if (const int rc = mvs_label_sums(c, s, norms_sq, mem_norms, floor, rb, re, labels, groups, own.data(), near.data(), nsum.data(), sizes.data())) return rc;
    if (const int rc = mvs_silhouette_stats(labels, m, groups, sizes.data(), own.data(), near.data(), nsum.data(), out, sil, a, b, centroid_d2,
                                            group_mean_s, group_within, group_dispersion, medoids))
        return rc;
    if (group_sizes) std::memcpy(group_sizes, sizes.data(), (size_t)groups * 8);
    if (nearest) std::memcpy(nearest, near.data(), (size_t)m * 4);
    return MVS_OK;
}

int mvs_ctx_label_stats(const mvs_ctx* c, double* dots_ms, double* reduce_ms, double* gather_ms, int64_t* row_blocks, int64_t* block_rows) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (dots_ms) *dots_ms = c->ls.dots_ms;
    if (reduce_ms) *reduce_ms = c->ls.reduce_ms;
    if (gather_ms) *gather_ms = c->ls.gather_ms;
    if (row_blocks) *row_blocks = c->ls.blocks;
    if (block_rows) *block_rows = c->ls.block_rows;
    return MVS_OK;
}

}  // extern "C"
