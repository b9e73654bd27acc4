// mvs_capi_sketch.hip -- C ABI: projection, sketch statistics, limb planes, sketch sets (include/mvs_hip.h)
#include "mvs_capi_internal.h"

using namespace mvs_capi;

namespace mvs_capi {

// -------------------------------------------------------------------------------------------------
// projection units
// -------------------------------------------------------------------------------------------------
// k_project runs one workgroup per (unit, group of 4 * BPW blocks), all of a launch's workgroups about equally long when the
// samples are, and the device holds `slots` of them at a time: 20 000 workgroups on 512 slots are 39.06 rounds, 40 are paid,
// and in the last one 480 slots idle.  The planner cuts the units that would end behind the launch's ideal end -- the last
// partial round, a long sample late in a ragged list, every unit of a launch too small to fill the slots -- into pieces
// that fit in front of it.
//
// Model: a workgroup of a unit of `count` hashes costs count + kProjOverhead hash-times (the overhead is the counters'
// cross-lane reduction, the masked tail batch and the start of the workgroup), and workgroups start in list order, each on
// the slot that frees first.  That greedy dispatch is followed exactly but in time quanta, so that the free times of the
// slots are a histogram and the earliest one a cursor that only moves forward: O(workgroups + buckets), no heap.  Before
// a unit is placed, the ideal end of the launch is (work placed so far + parent cost of the rest) / slots; a unit
// whose last workgroup starts at `start` and would end more than one overhead behind the ideal end is cut into pieces of
// at most ideal end - start each, in multiples of one main-loop iteration of the kernel and never below kProjPieceMin.
constexpr int kProjOverhead = 2000;    // hash-times per workgroup that do not depend on its hashes (LABNOTES, round 8)
constexpr int kProjPieceStep = 2048;   // one iteration of the kernel's main loop: 4 batches of 512 hashes
constexpr int kProjPieceMin = 4096;    // shortest piece: below two iterations the overhead passes a third of a piece's time
constexpr int64_t kProjBuckets = 1 << 16;

struct RowRange {
    int64_t lo, hi;
};

// Writes the unit list of (offsets, n_samples) to dst[0 .. cap) and returns in *n_units how many units it has -- when that
// is more than cap, the caller repeats the call with room for all.  cut_rows (may be NULL) receives the ranges of samples
// that consist of several units, in order.
int plan_project_units(const int64_t* offsets, int64_t n_samples, int ny, int slots, int overhead, bool balance,
                       mvs::ProjUnit* dst, size_t cap, size_t* n_units, std::vector<RowRange>* cut_rows) {
    constexpr int64_t kMax = mvs::kProjUnitMax;
    const int64_t E = overhead;
    const int64_t total_end = offsets[n_samples];
    balance = balance && slots > 0 && ny > 0 && total_end >= offsets[0];
    // greedy list scheduling makes a launch at most (work / slots + longest workgroup) long; twice that leaves room for the
    // overheads of the pieces.  Free times that would still pass the last bucket stay in it.
    int qs = 0;                                  // the time quantum is 2^qs hash-times
    int64_t nb = 0;
    if (balance) {
        const int64_t span = total_end - offsets[0], most_units = n_samples + span / kMax;
        const int64_t horizon = 2 * ((span + most_units * E) / slots * ny + ny * (kMax + E) + 1);
        while ((horizon >> qs) > kProjBuckets) ++qs;
        nb = (horizon >> qs) + 2;
    }
    const int64_t round_up = ((int64_t)1 << qs) - 1;
    auto cost = [&](int64_t count) { return (count + E + round_up) >> qs; };
    int64_t rest = 0;                            // parent cost of the units not yet placed: quanta x workgroups
    for (int64_t s = 0; s < n_samples; ++s) {
        const int64_t b = offsets[s], e = offsets[s + 1], len = e - b;
        if (e < b) return fail(MVS_E_INVALID, "offsets not monotone at sample %lld", (long long)s);
        if (len >= (1LL << 31)) return fail(MVS_E_RANGE, "sample %lld has >= 2^31 hashes", (long long)s);
        // (an empty sample gets one unit of zero hashes: the kernel then stores its row of zeros itself)
        rest += len <= kMax ? cost(len) : (len / kMax) * cost(kMax) + (len % kMax ? cost(len % kMax) : 0);
    }
    rest *= ny;
    if (cut_rows) cut_rows->clear();
    size_t w = 0;
    auto put = [&](int64_t begin, int64_t count, int64_t s, bool single) {
        if (w < cap) {
            mvs::ProjUnit u{begin, (int32_t)count, (int32_t)s, single ? 1 : 0, 0};
            if (begin + (((count >> 9) + 1) << 9) > total_end) u.flags = mvs::kProjTailGuard;
            dst[w] = u;
        }
        ++w;
    };
    auto note_cut = [&](int64_t s) {
        if (!cut_rows) return;
        if (!cut_rows->empty() && cut_rows->back().hi == s) cut_rows->back().hi = s + 1;
        else cut_rows->push_back(RowRange{s, s + 1});
    };
    if (!balance) {   // samples cut at kProjUnitMax only
        for (int64_t s = 0; s < n_samples; ++s) {
            const int64_t b = offsets[s], e = offsets[s + 1];
            const bool single = (e - b) <= kMax;
            if (e == b) put(b, 0, s, true);
            for (int64_t p = b; p < e; p += kMax) put(p, std::min<int64_t>(kMax, e - p), s, single);
            if (!single) note_cut(s);
        }
        *n_units = w;
        return MVS_OK;
    }

    thread_local std::vector<int32_t> free_buckets;
    free_buckets.assign((size_t)nb, 0);
    int32_t* const free_at = free_buckets.data();   // slots that become free in each time bucket
    free_at[0] = slots;
    int64_t placed = 0, cur = 0;                 // work placed; no slot becomes free before bucket `cur`
    auto place = [&](int64_t c, int64_t m) {     // m workgroups of c quanta each, every one on the slot that frees first
        placed += c * m;
        while (m > 0) {
            while (free_at[cur] == 0) ++cur;     // some slot is free at or after `cur`: the loop ends inside the array
            const int64_t t = std::min<int64_t>(m, free_at[cur]);
            free_at[cur] -= (int32_t)t;
            free_at[std::min(cur + c, nb - 1)] += (int32_t)t;
            m -= t;
        }
    };
    // when the last of a unit's ny workgroups starts: the time the ny-th slot becomes free
    const int need = std::min(ny, slots);
    auto start_of_unit = [&]() {
        while (free_at[cur] == 0) ++cur;
        int64_t i = cur;
        for (int have = free_at[i]; have < need; have += free_at[i]) ++i;
        return i;
    };
    // the ideal end of the launch as it stands is `work` / slots, work = placed + parent cost of all that is not (`rest`
    // does not change it while units go in whole): does a unit of c quanta that starts at `start` end within one overhead of it?
    const int64_t slack = E >> qs;
    auto fits = [&](int64_t start, int64_t c, int64_t work) { return (start + c - slack) * slots <= work; };
    auto one_unit = [&](int64_t p, int64_t n, int64_t s, bool single) {
        const int64_t c = cost(n);
        if (n == 0 || fits(start_of_unit(), c, placed + rest)) {
            put(p, n, s, single);
            rest -= c * ny;
            place(c, ny);
            return;
        }
        // the unit would end behind the ideal end: pieces of what still fits in front of it, looked at again for every
        // piece because each one takes slots the next finds gone
        rest -= c * ny;
        for (int64_t left = n; left > 0;) {
            const int64_t ideal = (placed + rest + cost(left) * ny) / slots;
            const int64_t room = ((ideal - start_of_unit()) << qs) - E;
            const int64_t g = std::max<int64_t>(kProjPieceMin, room / kProjPieceStep * kProjPieceStep);
            const int64_t pn = left - g < kProjPieceMin / 2 ? left : g;   // no crumb of a last piece
            put(p, pn, s, single && pn == n);
            place(cost(pn), ny);
            if (single && pn != n && left == n) note_cut(s);
            p += pn;
            left -= pn;
        }
    };
    for (int64_t s = 0; s < n_samples;) {
        const int64_t b = offsets[s], len = offsets[s + 1] - b;
        if (len > kMax) {
            for (int64_t p = b; p < b + len; p += kMax) one_unit(p, std::min<int64_t>(kMax, b + len - p), s, false);
            note_cut(s++);
            continue;
        }
        // a run of samples of one length: those whose workgroups all start in the same bucket go in together
        int64_t run = 1;
        while (s + run < n_samples && offsets[s + run + 1] - offsets[s + run] == len) ++run;
        const int64_t c = cost(len);
        while (run > 0) {
            while (free_at[cur] == 0) ++cur;
            const int64_t m = std::min<int64_t>(free_at[cur] / ny, run);
            if (m >= 1 && fits(cur, c, placed + rest)) {
                for (int64_t i = 0; i < m; ++i) put(offsets[s + i], len, s + i, true);
                rest -= c * ny * m;
                place(c, ny * m);
                s += m;
                run -= m;
            } else {
                one_unit(offsets[s], len, s, true);
                ++s;
                --run;
            }
        }
    }
    *n_units = w;
    return MVS_OK;
}

// workgroups of the projection kernel `variant` the device holds at a time; an error if the runtime will not say
static int project_slots(mvs_ctx* c, int variant, bool stats, int* slots) {
    int& have = c->proj_slots[variant][stats ? 1 : 0];
    if (have == 0) {
        const int per_cu = mvs::project_blocks_per_cu(variant, stats);
        if (per_cu <= 0 || c->cu_count <= 0)
            return fail(MVS_E_HIP, "occupancy query of k_project variant %d failed (%d workgroups per CU, %d CUs)", variant, per_cu,
                        c->cu_count);
        have = per_cu * c->cu_count;
    }
    *slots = have;
    return MVS_OK;
}

}  // namespace mvs_capi

extern "C" {

int mvs_project_plan(const int64_t* offsets, int64_t n_samples, int ny, int slots, int overhead, int balance,
                     mvs_proj_unit* units, int64_t capacity, int64_t* n_units) {
    static_assert(sizeof(mvs_proj_unit) == sizeof(mvs::ProjUnit), "one layout");
    if (!offsets || !n_units || n_samples < 0 || capacity < 0 || (capacity > 0 && !units) || ny < 1 || overhead > (1 << 20))
        return fail(MVS_E_INVALID, "bad argument");
    if (n_samples >= (1LL << 31)) return fail(MVS_E_RANGE, "too many samples");
    size_t n = 0;
    const int rc = plan_project_units(offsets, n_samples, ny, slots, overhead < 0 ? kProjOverhead : overhead, balance != 0,
                                      reinterpret_cast<mvs::ProjUnit*>(units), (size_t)capacity, &n, nullptr);
    if (rc) return rc;
    *n_units = (int64_t)n;
    return MVS_OK;
}

int mvs_ctx_project_stats(const mvs_ctx* c, int64_t* n_units, int64_t* cut_samples, int* slots, int* ny) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    if (n_units) *n_units = c->pj_units;
    if (cut_samples) *cut_samples = c->pj_cut_samples;
    if (slots) *slots = c->pj_slots;
    if (ny) *ny = c->pj_ny;
    return MVS_OK;
}

// -------------------------------------------------------------------------------------------------
// projection
// -------------------------------------------------------------------------------------------------
int mvs_project_csr(mvs_ctx* c, const uint64_t* hashes, int mem_hashes, const int64_t* offsets,
                    int64_t n_samples, int d, int32_t* out, int mem_out) {
    return mvs_project_csr_stats(c, hashes, mem_hashes, offsets, n_samples, d, out, mem_out, nullptr, nullptr);
}

int mvs_project_csr_stats(mvs_ctx* c, const uint64_t* hashes, int mem_hashes, const int64_t* offsets,
                          int64_t n_samples, int d, int32_t* out, int mem_out, int64_t* sumsq, int64_t* max_abs) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    const Range range(c, "mvs_project_csr");
    if ((sumsq == nullptr) != (max_abs == nullptr)) return fail(MVS_E_INVALID, "sumsq and max_abs go together");
    // sumsq lives where the sketches live: device array for device sketches, host array for host sketches
    int64_t* const sumsq_user = sumsq;
    DevBuf dsum;
    if (max_abs) *max_abs = 0;
    if (n_samples < 0 || d <= 0) return fail(MVS_E_INVALID, "n_samples=%lld d=%d", (long long)n_samples, d);
    if (!mem_ok(mem_hashes) || !mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad mem flag");
    if (n_samples == 0) return MVS_OK;
    if (!offsets || !out) return fail(MVS_E_INVALID, "offsets/out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (n_samples >= (1LL << 31)) return fail(MVS_E_RANGE, "too many samples");

    const int nblk = (d + 63) / 64;
    // kernel variant (launch_project): four blocks per wave sharing the first splitmix64 round, with the deep carry-save tree and
    // the VALU epilogue, where the dimension fills them (variant 24; 14 measured 8.97 vs 9.44 ms for 2 on 10k x
    // 50k hashes, d = 2048), else two or one block per wave; option project_variant forces one
    int bpw = (nblk % 4 == 0 && nblk >= 8) ? 24 : (nblk >= 2 ? 2 : 1);
    if (c->opt.project_variant == 24 && nblk >= 4) bpw = 24;
    if (c->opt.project_variant == 14 && nblk >= 4) bpw = 14;
    if (c->opt.project_variant == 12 && nblk >= 2) bpw = 12;
    if (c->opt.project_variant == 2 && nblk >= 2) bpw = 2;
    if (c->opt.project_variant == 1) bpw = 1;
    const int ny = mvs::project_ny(bpw, d);

    // Host hash lists larger than one staging piece go up through the two-buffer pipeline: while piece k is on the
    // link, piece k+1 is being copied into pinned memory and the samples that piece k-1 completed are being projected.
    // Its launches take the units in hash order as the pieces arrive, each far from filling the device's last round
    // alone: that path keeps the list cut at kProjUnitMax only.
    const bool pipelined = mem_hashes == MVS_MEM_HOST && offsets[n_samples] > 0 && (size_t)offsets[n_samples] * 8 > kUploadPiece;
    const bool balance = c->opt.project_balance != 0 && !pipelined;
    int slots = 0;
    int rc = balance ? project_slots(c, bpw, sumsq != nullptr, &slots) : MVS_OK;
    if (rc) return rc;

    // units, written straight into pinned memory: the buffer as it stands holds the list of all but the first call of a size
    rc = acquire_pinned(c, 256);
    if (rc) return rc;
    size_t n_units = 0;
    thread_local std::vector<RowRange> cut_rows;   // samples of several units: combined with atomics, statistics afterwards
    rc = plan_project_units(offsets, n_samples, ny, slots, kProjOverhead, balance, (mvs::ProjUnit*)c->pinned.p,
                            c->pinned.bytes / sizeof(mvs::ProjUnit), &n_units, &cut_rows);
    if (rc) return rc;
    if (n_units * sizeof(mvs::ProjUnit) > c->pinned.bytes) {
        rc = acquire_pinned(c, n_units * sizeof(mvs::ProjUnit));
        if (rc) return rc;
        rc = plan_project_units(offsets, n_samples, ny, slots, kProjOverhead, balance, (mvs::ProjUnit*)c->pinned.p,
                                c->pinned.bytes / sizeof(mvs::ProjUnit), &n_units, &cut_rows);
        if (rc) return rc;
    }
    mvs::ProjUnit* units = (mvs::ProjUnit*)c->pinned.p;
    // many scattered ranges (long samples all over a ragged list) are not worth a memset and a launch each: rows between
    // them may be cleared before and measured again after the projection without changing anything
    c->pj_units = (long long)n_units;
    c->pj_cut_samples = 0;
    for (const RowRange& r : cut_rows) c->pj_cut_samples += r.hi - r.lo;
    c->pj_slots = slots;
    c->pj_ny = ny;
    if (cut_rows.size() > 16) cut_rows.assign(1, RowRange{cut_rows.front().lo, cut_rows.back().hi});
    const int64_t total = offsets[n_samples];
    if (total > 0 && !hashes) return fail(MVS_E_INVALID, "hashes is NULL");

    DevBuf dh, dout;
    const uint64_t* d_hashes = hashes;
    if (mem_hashes == MVS_MEM_HOST) {
        HIP_TRY(dh.alloc((size_t)total * 8));
        if (!pipelined) HIP_TRY(hipMemcpyAsync(dh.p, hashes, (size_t)total * 8, hipMemcpyHostToDevice, c->stream));
        d_hashes = (const uint64_t*)dh.p;
    }
    int32_t* d_out = out;
    const size_t out_bytes = (size_t)n_samples * (size_t)d * 4;
    if (mem_out == MVS_MEM_HOST) {
        HIP_TRY(dout.alloc(out_bytes));
        d_out = (int32_t*)dout.p;
        if (sumsq) {
            HIP_TRY(dsum.alloc((size_t)n_samples * 8));
            sumsq = (int64_t*)dsum.p;
        }
    }
    const size_t ubytes = n_units * sizeof(mvs::ProjUnit);
    rc = ensure_scratch(c, std::max<size_t>(ubytes, 256));
    if (rc) return rc;
    if (n_units) {
        HIP_TRY(hipMemcpyAsync(c->scratch.p, units, ubytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->pinned_ev, c->stream));
        c->pinned_busy = true;
    }

    // samples cut into several units are combined with atomics and start from zero; single units store
    for (const RowRange& r : cut_rows)
        HIP_TRY(hipMemsetAsync(d_out + r.lo * (int64_t)d, 0, (size_t)(r.hi - r.lo) * (size_t)d * 4, c->stream));
    // statistics: inside the projection kernel for the samples that are one unit, by k_stats over the rows of the others
    // once the kernel is through; both feed the same sumsq array and the same running maximum
    const bool fused = sumsq != nullptr;
    if (fused) {
        HIP_TRY(hipMemsetAsync(sumsq, 0, (size_t)n_samples * 8, c->stream));
        HIP_TRY(hipMemsetAsync(c->counters(), 0, 8, c->stream));
    }
    if (c->timing) HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if (!pipelined) {
        mvs::launch_project(c->stream, d_hashes, (const mvs::ProjUnit*)c->scratch.p, (int64_t)n_units, d, d_out, bpw,
                            fused ? (unsigned long long*)sumsq : nullptr, fused ? c->counters() : nullptr);
        rc = check_kernel("k_project");
        if (rc) return rc;
    } else {
        rc = ensure_upload_pipeline(c);
        if (rc) return rc;
        // the unit list is in hash order: units [u_done, u_next) are those whose hashes the pieces sent so far cover
        size_t u_done = 0;
        const size_t total_bytes = (size_t)total * 8;
        int piece = 0;
        for (size_t off = 0; off < total_bytes; off += kUploadPiece, ++piece) {
            const int b = piece & 1;
            const size_t len = std::min(kUploadPiece, total_bytes - off);
            if (piece >= 2) HIP_TRY(hipEventSynchronize(c->up_done[b]));      // staging buffer b is free again
            parallel_copy(c->up_pinned[b].p, (const char*)hashes + off, len);
            HIP_TRY(hipMemcpyAsync((char*)dh.p + off, c->up_pinned[b].p, len, hipMemcpyHostToDevice, c->up_stream));
            HIP_TRY(hipEventRecord(c->up_done[b], c->up_stream));
            const int64_t covered = (int64_t)((off + len) / 8);
            size_t u_next = u_done;
            while (u_next < n_units && units[u_next].begin + units[u_next].count <= covered) ++u_next;
            if (u_next > u_done) {
                HIP_TRY(hipStreamWaitEvent(c->stream, c->up_done[b], 0));
                mvs::launch_project(c->stream, d_hashes, (const mvs::ProjUnit*)c->scratch.p + u_done, (int64_t)(u_next - u_done), d,
                                    d_out, bpw, fused ? (unsigned long long*)sumsq : nullptr, fused ? c->counters() : nullptr);
                rc = check_kernel("k_project");
                if (rc) return rc;
                u_done = u_next;
            }
        }
        if (u_done != n_units) return fail(MVS_E_INVALID, "internal: %zu of %zu projection units launched", u_done, n_units);
    }
    if (c->timing) {
        HIP_TRY(hipEventRecord(c->ev[1], c->stream));
        c->ev_valid[0] = true;
    }
    if (fused) {
        for (const RowRange& r : cut_rows) {   // their entries are final only now
            mvs::launch_stats(c->stream, d_out + r.lo * (int64_t)d, r.hi - r.lo, d, sumsq + r.lo, c->counters());
            rc = check_kernel("k_stats");
            if (rc) return rc;
        }
        unsigned long long m = 0;
        {
            const int rb_rc = read_back(c, c->stream, {{&m, c->counters(), 8}});
            if (rb_rc) return rb_rc;
        }
        *max_abs = (int64_t)m;
    }
    if (mem_out == MVS_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
        if (sumsq_user) HIP_TRY(hipMemcpyAsync(sumsq_user, sumsq, (size_t)n_samples * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    } else if (mem_hashes == MVS_MEM_HOST) {
        HIP_TRY(hipStreamSynchronize(c->stream));   // staging buffer is freed on return
    } else {
        // the unit list lives in ctx scratch, which stays valid; nothing to wait for
    }
    return MVS_OK;
}

int mvs_sketch_sumsq(mvs_ctx* c, const int32_t* sketches, int mem_in, int64_t n, int d, int64_t* sumsq,
                     int mem_out) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    if (n < 0 || d <= 0 || !mem_ok(mem_in) || !mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (n == 0) return MVS_OK;
    if (!sketches || !sumsq) return fail(MVS_E_INVALID, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf din, dout;
    const int32_t* d_in = sketches;
    if (mem_in == MVS_MEM_HOST) {
        HIP_TRY(din.alloc((size_t)n * d * 4));
        HIP_TRY(hipMemcpyAsync(din.p, sketches, (size_t)n * d * 4, hipMemcpyHostToDevice, c->stream));
        d_in = (const int32_t*)din.p;
    }
    int64_t* d_out = sumsq;
    if (mem_out == MVS_MEM_HOST) {
        HIP_TRY(dout.alloc((size_t)n * 8));
        d_out = (int64_t*)dout.p;
    }
    mvs::launch_sumsq(c->stream, d_in, n, d, d_out);
    int rc = check_kernel("k_sumsq");
    if (rc) return rc;
    if (mem_out == MVS_MEM_HOST)
        HIP_TRY(hipMemcpyAsync(sumsq, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    if (mem_out == MVS_MEM_HOST || mem_in == MVS_MEM_HOST) HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

}  // extern "C"

namespace mvs_capi {

// "%g" keeps 6 significant digits: x -> the decimal r * 10^-j (r an integer of 6 digits, round-half-even on the exact
// binary value of x as printf does) -> the double nearest to that decimal (what strtod returns) -> squared.
// The product x * 10^j is rounded once; only when it lands exactly on k + 0.5 can the true product lie on either side,
// and the fma residual says which (rounding is monotonic, so a product off the tie is on the true side of it).  An
// exponent estimate that is off by one next to a power of ten yields the same decimal (r = 10^6 is renormalised).
__device__ double norm_sq_from_text(long long sumsq, int d) {
    if (sumsq <= 0) return 0.0;
    const double x = sqrt((double)sumsq / (double)d);
    constexpr double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    int e = 0;                                   // 10^e <= x < 10^(e+1), up to the off-by-one noted above
    if (x >= 1.0) {
        while (e < 21 && x >= p10[e + 1]) ++e;
    } else {
        double y = x;
        while (e > -16 && y < 1.0) {
            y *= 10.0;
            --e;
        }
    }
    int j = 5 - e;                               // x * 10^j has 6 digits before the point
    double m, err;
    if (j >= 0) {
        m = x * p10[j];
        err = fma(x, p10[j], -m);                // exact: true product = m + err
    } else {
        m = x / p10[-j];
        err = -fma(m, p10[-j], -x);              // sign of (true quotient - m)
    }
    double r = rint(m);                          // half-even
    const double fl = floor(m);
    if (m - fl == 0.5 && err != 0.0) r = err > 0.0 ? fl + 1.0 : fl;
    if (r >= 1e6) {
        r = 1e5;
        --j;
    }
    const double v = j >= 0 ? r / p10[j] : r * p10[-j];
    return v * v;
}

__global__ __launch_bounds__(256) void k_norms_sq_text(const int64_t* __restrict__ sumsq, int64_t n, int d,
                                                       double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = norm_sq_from_text(sumsq[i], d);
}

}  // namespace mvs_capi

extern "C" {

int mvs_norms_sq_text(mvs_ctx* c, const int64_t* sumsq, int64_t n, int d, double* out) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    if (n < 0 || d <= 0) return fail(MVS_E_INVALID, "bad argument");
    if (n == 0) return MVS_OK;
    if (!sumsq || !out) return fail(MVS_E_INVALID, "NULL buffer");
    if ((n + 255) / 256 > 0x7fffffffLL) return fail(MVS_E_INVALID, "too many entries");
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_norms_sq_text, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, sumsq, n, d, out);
    return check_kernel("k_norms_sq_text");
}

int mvs_sketch_stats(mvs_ctx* c, const int32_t* sketches, int mem_in, int64_t n, int d, int64_t* sumsq, int mem_out,
                     int64_t* max_abs) {
    if (!c || !max_abs) return fail(MVS_E_INVALID, "NULL argument");
    *max_abs = 0;
    if (n < 0 || d <= 0 || !mem_ok(mem_in) || !mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (n == 0) return MVS_OK;
    if (!sketches || !sumsq) return fail(MVS_E_INVALID, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf din, dout;
    const int32_t* d_in = sketches;
    if (mem_in == MVS_MEM_HOST) {
        HIP_TRY(din.alloc((size_t)n * d * 4));
        HIP_TRY(hipMemcpyAsync(din.p, sketches, (size_t)n * d * 4, hipMemcpyHostToDevice, c->stream));
        d_in = (const int32_t*)din.p;
    }
    int64_t* d_out = sumsq;
    if (mem_out == MVS_MEM_HOST) {
        HIP_TRY(dout.alloc((size_t)n * 8));
        d_out = (int64_t*)dout.p;
    }
    HIP_TRY(hipMemsetAsync(c->counters(), 0, 8, c->stream));
    mvs::launch_stats(c->stream, d_in, n, d, d_out, c->counters());
    int rc = check_kernel("k_stats");
    if (rc) return rc;
    if (mem_out == MVS_MEM_HOST)
        HIP_TRY(hipMemcpyAsync(sumsq, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    unsigned long long m = 0;
    {
        const int rb_rc = read_back(c, c->stream, {{&m, c->counters(), 8}});
        if (rb_rc) return rb_rc;
    }
    *max_abs = (int64_t)m;
    return MVS_OK;
}

int mvs_sketch_saturate_i16(mvs_ctx* c, const int32_t* sketches, int mem_in, int64_t n_elems, int16_t* out,
                            int mem_out) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    if (n_elems < 0 || !mem_ok(mem_in) || !mem_ok(mem_out)) return fail(MVS_E_INVALID, "bad argument");
    if (n_elems == 0) return MVS_OK;
    if (!sketches || !out) return fail(MVS_E_INVALID, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf din, dout;
    const int32_t* d_in = sketches;
    if (mem_in == MVS_MEM_HOST) {
        HIP_TRY(din.alloc((size_t)n_elems * 4));
        HIP_TRY(hipMemcpyAsync(din.p, sketches, (size_t)n_elems * 4, hipMemcpyHostToDevice, c->stream));
        d_in = (const int32_t*)din.p;
    }
    int16_t* d_out = out;
    if (mem_out == MVS_MEM_HOST) {
        HIP_TRY(dout.alloc((size_t)n_elems * 2));
        d_out = (int16_t*)dout.p;
    }
    mvs::launch_saturate_i16(c->stream, d_in, n_elems, d_out);
    int rc = check_kernel("k_saturate_i16");
    if (rc) return rc;
    if (mem_out == MVS_MEM_HOST)
        HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n_elems * 2, hipMemcpyDeviceToHost, c->stream));
    if (mem_out == MVS_MEM_HOST || mem_in == MVS_MEM_HOST) HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

// -------------------------------------------------------------------------------------------------
// pairwise
// -------------------------------------------------------------------------------------------------
int mvs_sketch_max_abs(mvs_ctx* c, const void* sketches, int elem_bytes, int mem, int64_t n_elems,
                       int64_t* max_abs) {
    if (!c || !max_abs) return fail(MVS_E_INVALID, "NULL argument");
    if ((elem_bytes != 4 && elem_bytes != 2) || !mem_ok(mem) || n_elems < 0)
        return fail(MVS_E_INVALID, "bad argument");
    *max_abs = 0;
    if (n_elems == 0) return MVS_OK;
    if (!sketches) return fail(MVS_E_INVALID, "sketches is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const void* d_in = sketches;
    if (mem == MVS_MEM_HOST) {
        int rc0 = ensure_buf(c, c->stage, (size_t)n_elems * elem_bytes);
        if (rc0) return rc0;
        HIP_TRY(hipMemcpyAsync(c->stage.p, sketches, (size_t)n_elems * elem_bytes, hipMemcpyHostToDevice, c->stream));
        d_in = c->stage.p;
    }
    HIP_TRY(hipMemsetAsync(c->counters(), 0, 8, c->stream));
    mvs::launch_max_abs(c->stream, d_in, elem_bytes, n_elems, c->counters());
    int rc = check_kernel("k_max_abs");
    if (rc) return rc;
    unsigned long long m = 0;
    {
        const int rb_rc = read_back(c, c->stream, {{&m, c->counters(), 8}});
        if (rb_rc) return rb_rc;
    }
    *max_abs = (int64_t)m;
    return MVS_OK;
}

int mvs_limbs_for_max_abs(int64_t max_abs) {
    if (max_abs < 0) max_abs = -max_abs;
    if (max_abs <= 127) return 1;
    if (max_abs <= 32639) return 2;      // 127 * (1 + 256)
    if (max_abs <= 8355711) return 3;    // 127 * (1 + 256 + 65536)
    return 4;                            // exact mod 2^32 for every int32
}

int mvs_limb_geometry(int64_t n, int d, int limbs, int64_t* n_alloc, int* d_pad, size_t* bytes) {
    if (n < 0 || d <= 0 || !mvs::limb_code_ok(limbs)) return fail(MVS_E_INVALID, "bad argument");
    // tiles are up to 256 rows: pad to a multiple of 256 plus one spare tile
    const int64_t na = (n + 255) / 256 * 256 + 256;
    const int dp = (d + mvs::kBK - 1) / mvs::kBK * mvs::kBK;
    if (n_alloc) *n_alloc = na;
    if (d_pad) *d_pad = dp;
    if (bytes) *bytes = (size_t)na * (size_t)mvs::planes_of(limbs) * (size_t)dp;
    return MVS_OK;
}

int mvs_limb_split(mvs_ctx* c, const void* sketches, int elem_bytes, int mem, int64_t n_rows, int d, int limbs,
                   int8_t* planes, int d_pad, int64_t row_offset) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    if ((elem_bytes != 4 && elem_bytes != 2) || !mem_ok(mem) || n_rows < 0 || d <= 0 || !mvs::limb_code_ok(limbs) ||
        d_pad < d || d_pad % mvs::kBK != 0 || row_offset < 0)
        return fail(MVS_E_INVALID, "bad argument");
    if (n_rows == 0) return MVS_OK;
    if (!sketches || !planes) return fail(MVS_E_INVALID, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    const void* d_in = sketches;
    if (mem == MVS_MEM_HOST) {   // grow-only staging buffer of the context (no allocation per chunk)
        int rc0 = ensure_buf(c, c->stage, (size_t)n_rows * d * elem_bytes);
        if (rc0) return rc0;
        HIP_TRY(hipMemcpyAsync(c->stage.p, sketches, (size_t)n_rows * d * elem_bytes, hipMemcpyHostToDevice, c->stream));
        d_in = c->stage.p;
    }
    mvs::launch_limb_split(c->stream, d_in, elem_bytes, n_rows, d, limbs, planes, d_pad, row_offset);
    int rc = check_kernel("k_limb_split");
    if (rc) return rc;
    if (mem == MVS_MEM_HOST) HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_sketch_set_create(mvs_ctx* c, const void* sketches, int elem_bytes, int mem, int64_t n, int d,
                          mvs_sketch_set** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if ((elem_bytes != 4 && elem_bytes != 2) || !mem_ok(mem) || n < 0 || d <= 0)
        return fail(MVS_E_INVALID, "bad argument");
    if (n >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n too large for int32 row/col indices");
    if (n > 0 && !sketches) return fail(MVS_E_INVALID, "sketches is NULL");
    HIP_TRY(hipSetDevice(c->device));
    // stage once if the input is on the host
    DevBuf din;
    const void* d_in = sketches;
    if (mem == MVS_MEM_HOST && n > 0) {
        HIP_TRY(din.alloc((size_t)n * d * elem_bytes));
        HIP_TRY(hipMemcpyAsync(din.p, sketches, (size_t)n * d * elem_bytes, hipMemcpyHostToDevice, c->stream));
        d_in = din.p;
    }
    int64_t max_abs = 0;
    int rc = mvs_sketch_max_abs(c, d_in, elem_bytes, MVS_MEM_DEVICE, n * d, &max_abs);
    if (rc) return rc;
    int limbs = mvs_limbs_for_max_abs(max_abs);
    // The 3-pass Karatsuba scheme (63 * (1 + 128): digits in [-64,63], their sum in int8) is exact and tested but
    // measures 9-19 % SLOWER than two base-256 limbs on MI355X (25 % fewer MFMAs, 1.5x the LDS traffic), so it is
    // opt-in: option enable_k3.
    if (c->opt.enable_k3 && max_abs > 127 && max_abs <= 8127) limbs = MVS_LIMBS_K3;
    int64_t n_alloc = 0;
    int d_pad = 0;
    size_t bytes = 0;
    mvs_limb_geometry(n, d, limbs, &n_alloc, &d_pad, &bytes);
    std::unique_ptr<mvs_sketch_set> s(new (std::nothrow) mvs_sketch_set());
    if (!s) return fail(MVS_E_NOMEM, "out of host memory");
    if (s->owned.alloc(bytes) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %zu bytes of limb planes failed", bytes);
    s->ctx = c;
    s->planes = s->owned.as<int8_t>();
    s->n = n;
    s->n_alloc = n_alloc;
    s->d = d;
    s->d_pad = d_pad;
    s->limbs = limbs;
    s->id = ++g_set_ids;
    hipError_t e = hipMemsetAsync(s->owned.p, 0, bytes, c->stream);
    if (e == hipSuccess) {
        rc = mvs_limb_split(c, d_in, elem_bytes, MVS_MEM_DEVICE, n, d, limbs, s->owned.as<int8_t>(), d_pad, 0);
        if (rc == MVS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(MVS_E_HIP, "sync failed");
    } else {
        rc = fail(MVS_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    if (rc) return rc;
    *out = s.release();
    return MVS_OK;
}

int mvs_sketch_set_from_planes(mvs_ctx* c, const int8_t* planes, int64_t n, int64_t n_alloc, int d, int d_pad,
                               int limbs, mvs_sketch_set** out) {
    if (!c || !out || !planes) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    int64_t need_alloc = 0;
    int need_pad = 0;
    if (mvs_limb_geometry(n, d, limbs, &need_alloc, &need_pad, nullptr)) return MVS_E_INVALID;
    if (n_alloc < need_alloc || d_pad != need_pad)
        return fail(MVS_E_INVALID, "plane buffer geometry: need n_alloc >= %lld and d_pad == %d",
                    (long long)need_alloc, need_pad);
    if (n >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n too large for int32 row/col indices");
    mvs_sketch_set* s = new (std::nothrow) mvs_sketch_set();
    if (!s) return fail(MVS_E_NOMEM, "out of host memory");
    s->ctx = c;
    s->planes = planes;
    s->n = n;
    s->n_alloc = n_alloc;
    s->d = d;
    s->d_pad = d_pad;
    s->limbs = limbs;
    s->id = ++g_set_ids;
    *out = s;
    return MVS_OK;
}

int mvs_sketch_set_alloc(mvs_ctx* c, int64_t n, int d, int limbs, mvs_sketch_set** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (n < 0 || d <= 0 || !mvs::limb_code_ok(limbs)) return fail(MVS_E_INVALID, "bad argument");
    if (n >= (1LL << 31) - 256) return fail(MVS_E_RANGE, "n too large for int32 row/col indices");
    HIP_TRY(hipSetDevice(c->device));
    int64_t n_alloc = 0;
    int d_pad = 0;
    size_t bytes = 0;
    mvs_limb_geometry(n, d, limbs, &n_alloc, &d_pad, &bytes);
    std::unique_ptr<mvs_sketch_set> s(new (std::nothrow) mvs_sketch_set());
    if (!s) return fail(MVS_E_NOMEM, "out of host memory");
    if (s->owned.alloc(bytes) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %zu bytes of limb planes failed", bytes);
    s->ctx = c;
    s->planes = s->owned.as<int8_t>();
    s->n = n;
    s->n_alloc = n_alloc;
    s->d = d;
    s->d_pad = d_pad;
    s->limbs = limbs;
    s->id = ++g_set_ids;
    if (hipMemsetAsync(s->owned.p, 0, bytes, c->stream) != hipSuccess) return fail(MVS_E_HIP, "hipMemsetAsync failed");
    *out = s.release();
    return MVS_OK;
}

}  // extern "C"

namespace mvs_capi {
// Rows [lo, hi) of an owned set are about to be rewritten.  If the context holds data derived from the set's present
// contents (coarse plane, fragment-major copies) and the range is a small part of it, the set keeps its generation and
// remembers the range: refresh_derived() re-derives just those rows before the next comparison.  A search front end
// that appends its queries behind a resident database (search.py: SearchIndex) thus keeps the database's coarse plane --
// bumping the generation made every search rebuild it (6 ms per 10^6 sketches) or fall back to the exact kernels.
void note_rows_rewritten(mvs_sketch_set* s, int64_t lo, int64_t hi) {
    mvs_ctx* c = s->ctx;
    // (the "a block of few rows went to the exact kernel for lack of a coarse plane" marker counts as well: it is what makes
    // the SECOND such block build the plane, and it must survive the upload of that block's rows)
    const bool cached = (c->coarse_id == s->id && c->coarse_gen == s->gen) || (c->planes_fm_id == s->id && c->planes_fm_gen == s->gen) ||
                        (c->few_rows_id == s->id && c->few_rows_gen == s->gen);
    const int64_t u_lo = s->dirty_hi > s->dirty_lo ? std::min(s->dirty_lo, lo) : lo;
    const int64_t u_hi = s->dirty_hi > s->dirty_lo ? std::max(s->dirty_hi, hi) : hi;
    if (cached && (u_hi - u_lo) * 8 <= s->n) {
        s->dirty_lo = u_lo;
        s->dirty_hi = u_hi;
        return;
    }
    ++s->gen;   // derived data of the old contents is stale as a whole
    s->dirty_lo = s->dirty_hi = 0;
}
}  // namespace mvs_capi

extern "C" {

int mvs_sketch_set_fill(mvs_sketch_set* s, const void* sketches, int elem_bytes, int mem, int64_t row_offset,
                        int64_t n_rows) {
    if (!s || !s->owned.p) return fail(MVS_E_INVALID, "set is NULL or not owned by the library");
    if (row_offset < 0 || n_rows < 0 || row_offset + n_rows > s->n)
        return fail(MVS_E_INVALID, "rows [%lld,%lld) outside the set", (long long)row_offset,
                    (long long)(row_offset + n_rows));
    // (what mvs_limb_split would refuse is refused before the rows are noted: a refused call rewrites nothing)
    if ((elem_bytes != 4 && elem_bytes != 2) || !mem_ok(mem)) return fail(MVS_E_INVALID, "bad argument");
    if (n_rows > 0 && !sketches) return fail(MVS_E_INVALID, "sketches is NULL");
    if (n_rows > 0) note_rows_rewritten(s, row_offset, row_offset + n_rows);
    return mvs_limb_split(s->ctx, sketches, elem_bytes, mem, n_rows, s->d, s->limbs, s->owned.as<int8_t>(), s->d_pad, row_offset);
}

int mvs_sketch_set_fill_stats(mvs_sketch_set* s, const void* sketches, int elem_bytes, int mem, int64_t row_offset,
                              int64_t n_rows, int64_t* max_abs) {
    if (!s || !s->owned.p) return fail(MVS_E_INVALID, "set is NULL or not owned by the library");
    if (!max_abs) return fail(MVS_E_INVALID, "max_abs is NULL");
    *max_abs = 0;
    if ((elem_bytes != 4 && elem_bytes != 2) || !mem_ok(mem)) return fail(MVS_E_INVALID, "bad argument");
    if (row_offset < 0 || n_rows < 0 || row_offset + n_rows > s->n)
        return fail(MVS_E_INVALID, "rows [%lld,%lld) outside the set", (long long)row_offset,
                    (long long)(row_offset + n_rows));
    if (n_rows == 0) return MVS_OK;
    if (!sketches) return fail(MVS_E_INVALID, "sketches is NULL");
    mvs_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)n_rows * s->d * elem_bytes;
    const void* d_in = sketches;
    if (mem == MVS_MEM_HOST) {   // one upload serves both kernels
        int rc0 = ensure_buf(c, c->stage, bytes);
        if (rc0) return rc0;
        HIP_TRY(hipMemcpyAsync(c->stage.p, sketches, bytes, hipMemcpyHostToDevice, c->stream));
        d_in = c->stage.p;
    }
    note_rows_rewritten(s, row_offset, row_offset + n_rows);
    HIP_TRY(hipMemsetAsync(c->counters(), 0, 8, c->stream));
    mvs::launch_max_abs(c->stream, d_in, elem_bytes, n_rows * s->d, c->counters());
    int rc = check_kernel("k_max_abs");
    if (rc) return rc;
    mvs::launch_limb_split(c->stream, d_in, elem_bytes, n_rows, s->d, s->limbs, s->owned.as<int8_t>(), s->d_pad, row_offset);
    rc = check_kernel("k_limb_split");
    if (rc) return rc;
    unsigned long long m = 0;
    {
        const int rb_rc = read_back(c, c->stream, {{&m, c->counters(), 8}});
        if (rb_rc) return rb_rc;
    }
    *max_abs = (int64_t)m;
    return MVS_OK;
}

int mvs_sketch_set_info(const mvs_sketch_set* s, int64_t* n, int* d, int* limbs, int64_t* n_alloc, int* d_pad) {
    if (!s) return fail(MVS_E_INVALID, "set is NULL");
    if (n) *n = s->n;
    if (d) *d = s->d;
    if (limbs) *limbs = s->limbs;
    if (n_alloc) *n_alloc = s->n_alloc;
    if (d_pad) *d_pad = s->d_pad;
    return MVS_OK;
}

int mvs_sketch_set_planes(mvs_sketch_set* s, int8_t** planes) {
    if (!s || !planes) return fail(MVS_E_INVALID, "NULL argument");
    if (!s->owned.p) return fail(MVS_E_INVALID, "the set is a view of a caller-owned buffer");
    *planes = s->owned.as<int8_t>();
    return MVS_OK;
}

int mvs_sketch_set_touch(mvs_sketch_set* s) {
    if (!s) return fail(MVS_E_INVALID, "set is NULL");
    ++s->gen;
    s->dirty_lo = s->dirty_hi = 0;
    return MVS_OK;
}

int mvs_ctx_derived_stats(mvs_ctx* c, int64_t* coarse_builds, int64_t* coarse_rows_refreshed, int64_t* coarse_fm_builds,
                          int64_t* planes_fm_builds, int64_t* planes_fm_rows_refreshed) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    if (coarse_builds) *coarse_builds = c->dv_coarse_builds;
    if (coarse_rows_refreshed) *coarse_rows_refreshed = c->dv_coarse_rows;
    if (coarse_fm_builds) *coarse_fm_builds = c->dv_coarse_fm_builds;
    if (planes_fm_builds) *planes_fm_builds = c->dv_planes_fm_builds;
    if (planes_fm_rows_refreshed) *planes_fm_rows_refreshed = c->dv_planes_fm_rows;
    return MVS_OK;
}

int mvs_sketch_set_destroy(mvs_sketch_set* s) {
    if (!s) return MVS_OK;
    if (s->owned.p) {
        (void)hipSetDevice(s->ctx->device);
        (void)hipStreamSynchronize(s->ctx->stream);
    }
    delete s;
    return MVS_OK;
}


}  // extern "C"
