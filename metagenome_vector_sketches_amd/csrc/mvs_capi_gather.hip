// mvs_capi_gather.hip -- C ABI of the greedy decomposition of a query into samples of a hash set: mvs_gather,
// mvs_ctx_gather_stats and mvs_ctx_gather_round_bytes (include/mvs_hip.h "gather").  Three phases: the original overlaps of all
// candidates through mvs_intersect_cells as it is, the bit rows of the survivors (k_gather_mark over the units plan_units lays
// out), then the rounds, queued option gather_batch at a time with one read-back of the walk's state per batch.  The kernels
// are in mvs_gather.hip.
#include "mvs_capi_internal.h"

#include <hip/hip_runtime.h>

using namespace mvs_capi;

namespace {

int alloc_or_nomem(DevBuf& b, size_t bytes, const char* what) {
    if (b.alloc(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MVS_E_NOMEM, "gather: hipMalloc of %zu bytes for %s failed", bytes, what);
    }
    return MVS_OK;
}

}  // namespace

extern "C" {

int mvs_gather(mvs_ctx* c, const mvs_hash_set* hs_query, int64_t query, const mvs_hash_set* hs_db, const int32_t* candidates,
               int mem_candidates, int64_t n_candidates, int32_t min_hashes, int64_t max_matches, mvs_gather_match* out, int mem_out,
               int64_t* n_matches, int32_t* query_size) {
    if (n_matches) *n_matches = 0;
    if (!c || !hs_query || !hs_db || !n_matches) return fail(MVS_E_INVALID, "NULL argument");
    if (!mem_ok(mem_candidates) || !mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (hs_query->ctx != c || hs_db->ctx != c) return fail(MVS_E_INVALID, "a hash set belongs to another context");
    if (min_hashes < 1) return fail(MVS_E_INVALID, "min_hashes = %d is below 1", (int)min_hashes);
    if (max_matches < 0) return fail(MVS_E_INVALID, "max_matches = %lld is negative", (long long)max_matches);
    if (candidates && n_candidates < 0) return fail(MVS_E_INVALID, "n_candidates = %lld is negative", (long long)n_candidates);
    if (max_matches > 0 && !out) return fail(MVS_E_INVALID, "out is NULL");
    if (query < 0 || query >= hs_query->n)
        return fail(MVS_E_RANGE, "query %lld outside the set of %lld samples", (long long)query, (long long)hs_query->n);
    HIP_TRY(hipSetDevice(c->device));
    const Range range(c, "mvs_gather");

    // the candidates: distinct, ascending (the tie rule then is "the smaller survivor index")
    std::vector<int32_t> cand;
    if (!candidates) {
        cand.resize((size_t)hs_db->n);
        for (int64_t i = 0; i < hs_db->n; ++i) cand[(size_t)i] = (int32_t)i;
    } else if (n_candidates > 0) {
        cand.resize((size_t)n_candidates);
        if (mem_candidates == MVS_MEM_HOST) {
            memcpy(cand.data(), candidates, (size_t)n_candidates * 4);
        } else {
            HIP_TRY(hipMemcpyAsync(cand.data(), candidates, (size_t)n_candidates * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        for (int32_t s : cand)
            if (s < 0 || s >= hs_db->n)
                return fail(MVS_E_RANGE, "candidate %d outside the set of %lld samples", (int)s, (long long)hs_db->n);
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    }
    const int64_t nc = (int64_t)cand.size();

    c->ga_survivors = c->ga_rounds = c->ga_batches = c->ga_row_bytes = c->ga_round_bytes = 0;
    c->ga_overlap_ms = c->ga_mark_ms = c->ga_rounds_ms = 0.0;
    int32_t q_size = 0;
    HIP_TRY(hipMemcpyAsync(&q_size, hs_query->sizes.as<int32_t>() + query, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (query_size) *query_size = q_size;
    if (max_matches == 0 || q_size == 0 || nc == 0) return MVS_OK;

    // ---- phase 0: orig[c] = |Q n H(c)| for every candidate, by the intersection kernels as they are ----
    std::vector<mvs_cell> cells((size_t)nc);
    for (int64_t i = 0; i < nc; ++i) cells[(size_t)i] = mvs_cell{(int32_t)query, cand[(size_t)i], 0, 0};
    std::vector<int32_t> orig((size_t)nc);
    int rc = mvs_intersect_cells(c, hs_query, hs_db, cells.data(), MVS_MEM_HOST, nc, orig.data(), MVS_MEM_HOST);
    if (rc) return rc;
    c->ga_overlap_ms = c->ix_kernel_ms;
    // ... and only those at min_hashes or above can ever be written (f only falls): everything below scales with them
    int64_t ns = 0;
    for (int64_t i = 0; i < nc; ++i) {
        if (orig[(size_t)i] < min_hashes) continue;
        cells[(size_t)ns] = cells[(size_t)i];
        orig[(size_t)ns] = orig[(size_t)i];
        ++ns;
    }
    std::vector<int32_t> surv((size_t)ns * 2);    // the survivors' samples (ascending), then their original overlaps
    for (int64_t s = 0; s < ns; ++s) {
        surv[(size_t)s] = cells[(size_t)s].col;
        surv[(size_t)(ns + s)] = orig[(size_t)s];
    }
    c->ga_survivors = ns;
    if (ns == 0) return MVS_OK;

    const int64_t W = ((int64_t)q_size + 63) / 64;
    const size_t row_bytes = (size_t)ns * (size_t)W * 8;
    const int64_t rec_cap = std::min<int64_t>(max_matches, ns);
    DevBuf rows, small;
    if ((rc = alloc_or_nomem(rows, row_bytes, "the survivors' bit rows"))) return rc;
    // alive | records | cells | sample, orig, retired, count | state
    const size_t o_rec = (size_t)W * 8, o_cells = o_rec + (size_t)rec_cap * sizeof(mvs_gather_match);
    const size_t o_surv = o_cells + (size_t)ns * sizeof(mvs_cell), o_state = (o_surv + (size_t)ns * 16 + 7) & ~(size_t)7;
    if ((rc = alloc_or_nomem(small, o_state + sizeof(mvs::GatherState), "the walk's state"))) return rc;
    c->ga_row_bytes = (long long)row_bytes;
    unsigned long long* d_rows = (unsigned long long*)rows.p;
    unsigned long long* d_alive = (unsigned long long*)small.p;
    mvs_gather_match* d_rec = (mvs_gather_match*)((char*)small.p + o_rec);
    mvs_cell* d_cells = (mvs_cell*)((char*)small.p + o_cells);
    int32_t* d_sample = (int32_t*)((char*)small.p + o_surv);
    int32_t *d_orig = d_sample + ns, *d_retired = d_sample + 2 * ns, *d_count = d_sample + 3 * ns;
    mvs::GatherState* d_state = (mvs::GatherState*)((char*)small.p + o_state);
    HIP_TRY(hipMemcpyAsync(d_cells, cells.data(), (size_t)ns * sizeof(mvs_cell), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_sample, surv.data(), (size_t)ns * 8, hipMemcpyHostToDevice, c->stream));

    // ---- phase 1: the survivors' bit rows over the positions of Q, in the units of the intersection ----
    const int unit = std::max(64, c->opt.intersect_unit & ~63);        // a word of a row belongs to one unit
    PlannedUnits plan;
    if ((rc = plan_units(c, "gather", d_cells, ns, hs_query, hs_db, unit, d_count, false, nullptr, false, plan))) return rc;
    StageTimer t_mark, t_rounds;
    if ((rc = t_mark.begin(c))) return rc;
    HIP_TRY(hipMemsetAsync(d_rows, 0, row_bytes, c->stream));
    rc = mvs::launch_gather_mark(c->stream, d_cells, ns, plan.d_start, plan.n_units, hs_query->hashes.as<unsigned long long>(),
                                 hs_query->offsets.as<long long>(), hs_query->sizes.as<int32_t>(), hs_db->hashes.as<unsigned long long>(),
                                 hs_db->offsets.as<long long>(), hs_db->sizes.as<int32_t>(), unit, d_rows, W);
    if (!rc) rc = check_kernel("k_gather_mark");
    if (rc) return rc;
    if ((rc = t_mark.mark_end())) return rc;

    // ---- phase 2: the rounds, a batch at a time; a round that finds the walk ended returns at once ----
    if ((rc = t_rounds.begin(c))) return rc;
    mvs::launch_gather_init(c->stream, d_alive, W, q_size, d_retired, d_count, ns, d_state);
    if ((rc = check_kernel("k_gather_init"))) return rc;
    const int64_t bound = max_matches <= ns ? max_matches : ns + 1;    // rounds after which the walk has ended for certain
    mvs::GatherState st{};
    int64_t queued = 0, batches = 0;
    while (!st.done && queued < bound) {
        const int64_t n = std::min<int64_t>(c->opt.gather_batch, bound - queued);
        for (int64_t i = 0; i < n; ++i)
            mvs::launch_gather_round(c->stream, d_rows, W, ns, d_alive, d_retired, min_hashes, d_count, d_sample, d_orig, d_rec,
                                     max_matches, d_state, (int)((queued + i) & 1));
        if ((rc = check_kernel("k_gather_count / k_gather_bid / k_gather_pick"))) return rc;
        if ((rc = read_back(c, c->stream, {{&st, d_state, sizeof st}}))) return rc;
        queued += n;
        ++batches;
    }
    if ((rc = t_rounds.mark_end())) return rc;
    if (!st.done || st.n_records < 0 || st.n_records > rec_cap)
        return fail(MVS_E_HIP, "gather: the walk did not end within %lld rounds", (long long)bound);
    if (st.n_records > 0)
        HIP_TRY(hipMemcpyAsync(out, d_rec, (size_t)st.n_records * sizeof(mvs_gather_match),
                               mem_out == MVS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = t_mark.add_to(&c->ga_mark_ms))) return rc;
    if ((rc = t_rounds.add_to(&c->ga_rounds_ms))) return rc;
    c->ga_rounds = st.rounds;
    c->ga_batches = batches;
    c->ga_round_bytes = (long long)st.rows_read * W * 8;
    *n_matches = st.n_records;
    return MVS_OK;
}

int mvs_ctx_gather_stats(const mvs_ctx* c, int64_t* survivors, int64_t* rounds, int64_t* batches, int64_t* row_bytes,
                         double* overlap_ms, double* mark_ms, double* rounds_ms) {
    if (!c) return fail(MVS_E_INVALID, "NULL context");
    if (survivors) *survivors = c->ga_survivors;
    if (rounds) *rounds = c->ga_rounds;
    if (batches) *batches = c->ga_batches;
    if (row_bytes) *row_bytes = c->ga_row_bytes;
    if (overlap_ms) *overlap_ms = c->ga_overlap_ms;
    if (mark_ms) *mark_ms = c->ga_mark_ms;
    if (rounds_ms) *rounds_ms = c->ga_rounds_ms;
    return MVS_OK;
}

int mvs_ctx_gather_round_bytes(const mvs_ctx* c, int64_t* bytes) {
    if (!c || !bytes) return fail(MVS_E_INVALID, "NULL argument");
    *bytes = c->ga_round_bytes;
    return MVS_OK;
}

}  // extern "C"
