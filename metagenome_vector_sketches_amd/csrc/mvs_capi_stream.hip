// mvs_capi_stream.hip -- C ABI: the comparison with its result streamed out in row blocks (mvs_pairwise_stream[_encoded])
#include "mvs_capi_internal.h"
#include "mvs_stream_plan.h"

#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

using namespace mvs_capi;

// -------------------------------------------------------------------------------------------------
// streamed output
// -------------------------------------------------------------------------------------------------
namespace mvs_capi {

// Device -> host copies on a DMA engine instead of the runtime's copy kernel (option stream_copy = 1).  hipMemcpyAsync into pinned
// memory is a blit KERNEL on this stack (__amd_rocclr_copyBuffer in the traces): it reaches the link's rate but holds compute units
// while the link drains it.  hsa_amd_memory_async_copy moves the same bytes at the same 56 GB/s with no CU involved
// (tools/microbench/sdma_copy.hip).  ROCr is the layer HIP itself sits on: same process, same address space, pointers of hipMalloc /
// hipHostMalloc are valid as they are.  The copies are not on a HIP stream any more, so their ordering is the host's: the feeder
// waits for the block's arrays (dl_ready) before the first copy, the callback thread waits for a piece's completion signal, and
// the driving thread re-uses a set of arrays once the callback thread has seen the last piece of the block that used it.
struct HsaCopy {
    hsa_agent_t gpu{}, cpu{};
    hsa_signal_t sig[2]{};
    bool ok = false;
};
struct HsaAgents {
    std::vector<hsa_agent_t> gpus;
    hsa_agent_t cpu{};
    bool have_cpu = false;
};
hsa_status_t hsa_on_agent(hsa_agent_t a, void* data) {
    HsaAgents* ag = static_cast<HsaAgents*>(data);
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (t == HSA_DEVICE_TYPE_GPU) ag->gpus.push_back(a);
    if (t == HSA_DEVICE_TYPE_CPU && !ag->have_cpu) {
        ag->cpu = a;
        ag->have_cpu = true;
    }
    return HSA_STATUS_SUCCESS;
}
void hsa_copy_free(void* p) {
    HsaCopy* h = static_cast<HsaCopy*>(p);
    if (h->ok) {
        for (hsa_signal_t& s : h->sig) (void)hsa_signal_destroy(s);
        (void)hsa_shut_down();
    }
    delete h;
}
int ensure_hsa_copy(mvs_ctx* c) {
    if (c->dl_hsa) return static_cast<HsaCopy*>(c->dl_hsa.get())->ok ? MVS_OK : fail(MVS_E_HIP, "the DMA copy path is not available");
    HsaCopy* h = new (std::nothrow) HsaCopy();
    if (!h) return fail(MVS_E_NOMEM, "out of host memory");
    c->dl_hsa = {h, hsa_copy_free};
    if (hsa_init() != HSA_STATUS_SUCCESS) return fail(MVS_E_HIP, "hsa_init failed");
    HsaAgents ag;
    if (hsa_iterate_agents(hsa_on_agent, &ag) != HSA_STATUS_SUCCESS || ag.gpus.empty() || !ag.have_cpu) {
        (void)hsa_shut_down();
        return fail(MVS_E_HIP, "no HSA agents");
    }
    // the context's device among the GPU agents: by PCI bus / device / function, by index if that cannot be read
    size_t pick = (size_t)c->device < ag.gpus.size() ? (size_t)c->device : 0;
    char bus[32] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, c->device) == hipSuccess) {
        unsigned dom = 0, b = 0, d = 0, f = 0;
        if (sscanf(bus, "%x:%x:%x.%x", &dom, &b, &d, &f) == 4)
            for (size_t k = 0; k < ag.gpus.size(); ++k) {
                uint32_t bdf = 0;
                if (hsa_agent_get_info(ag.gpus[k], (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) == HSA_STATUS_SUCCESS &&
                    ((bdf >> 8) & 0xff) == b && ((bdf >> 3) & 0x1f) == d && (bdf & 0x7) == f)
                    pick = k;
            }
    }
    h->gpu = ag.gpus[pick];
    h->cpu = ag.cpu;
    for (hsa_signal_t& sg : h->sig)
        if (hsa_signal_create(0, 0, nullptr, &sg) != HSA_STATUS_SUCCESS) {
            (void)hsa_shut_down();
            return fail(MVS_E_HIP, "hsa_signal_create failed");
        }
    h->ok = true;
    return MVS_OK;
}

// Hand-over between the thread that drives the GPU and the one that runs the caller's callback: two pinned buffers,
// a queue of filled ones.  The callback therefore runs beside the next block's kernels and downloads.
struct StreamOut {
    struct Item {
        int slot;
        int64_t row_begin, row_end, n_cells;
        std::vector<int64_t> row_ptr;      // rebased to the block's first cell
        bool wide;
        // encoded pieces: the directory of the piece's non-empty rows, the records' byte count
        std::vector<uint32_t> rows, first_col, jac_bytes;
        std::vector<uint64_t> offset;
        int64_t n_bytes = 0;
        bool dma = false;                  // the piece was copied by a DMA engine: its completion is the slot's HSA signal
        bool last_of_block = false;        // (DMA copies) the callback thread has seen a block's last piece: its arrays are free again
    };
    mvs_ctx* c;
    mvs_row_block_cb cb;
    mvs_encoded_rows_cb ecb;               // set instead of cb by mvs_pairwise_stream_encoded
    void* user;
    StreamOut(mvs_ctx* ctx, mvs_row_block_cb on_block, mvs_encoded_rows_cb on_rows, void* u) : c(ctx), cb(on_block), ecb(on_rows), user(u) {}
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Item> queue;
    bool slot_busy[2] = {false, false};
    bool closing = false;
    int cb_status = 0;                     // first non-zero return of the callback
    std::string error;
    std::thread worker;
    // The feeder: hands finished row blocks to the link piece by piece (it blocks on the two pinned buffers), so that the
    // thread that drives the device never waits for the link -- it runs at most two blocks ahead (the device-side arrays
    // of a block are double-buffered: set k & 1).
    std::thread feeder;
    std::deque<std::function<int()>> feed_queue;
    bool feed_closing = false;
    int64_t fed_blocks = 0;                // blocks whose pieces have all been queued on the download stream
    int64_t done_blocks = 0;               // (DMA copies) blocks whose last piece the callback thread has consumed
    int feed_rc = 0;

    void feed_run() {
        (void)hipSetDevice(c->device);
        for (;;) {
            std::function<int()> task;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return feed_closing || !feed_queue.empty(); });
                if (feed_queue.empty()) return;
                task = std::move(feed_queue.front());
                feed_queue.pop_front();
            }
            const int r = task();
            {
                std::lock_guard<std::mutex> lk(mu);
                if (r != 0 && feed_rc == 0) {
                    feed_rc = r;
                    if (error.empty()) error = std::string("feeding the link failed: ") + mvs_last_error();
                }
                ++fed_blocks;
            }
            cv.notify_all();
        }
    }
    void enqueue_feed(std::function<int()> task) {
        {
            std::lock_guard<std::mutex> lk(mu);
            feed_queue.push_back(std::move(task));
        }
        cv.notify_all();
    }
    void wait_fed(int64_t blocks) {         // until that many blocks have been handed to the download stream
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return fed_blocks >= blocks; });
    }
    void wait_done(int64_t blocks) {        // (DMA copies) until that many blocks have left the device entirely
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done_blocks >= blocks || cb_status != 0 || !error.empty() || feed_rc != 0; });
    }
    void close_feeder() {
        {
            std::lock_guard<std::mutex> lk(mu);
            feed_closing = true;
        }
        cv.notify_all();
        if (feeder.joinable()) feeder.join();
    }

    void run() {
        (void)hipSetDevice(c->device);
        for (;;) {
            Item it;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return closing || !queue.empty(); });
                if (queue.empty()) return;
                it = std::move(queue.front());
                queue.pop_front();
            }
            int status = 0;
            hipError_t e = hipSuccess;
            if (it.dma) {
                const HsaCopy* h = static_cast<const HsaCopy*>(c->dl_hsa.get());
                if (hsa_signal_wait_scacquire(h->sig[it.slot], HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED) != 0)
                    e = hipErrorUnknown;       // (a negative value: the copy failed)
            } else {
                e = hipEventSynchronize(c->dl_done[it.slot]);
            }
            if (e != hipSuccess) {
                std::lock_guard<std::mutex> lk(mu);
                if (error.empty()) error = std::string("download failed: ") + hipGetErrorString(e);
            } else {
                bool skip;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    skip = cb_status != 0 || !error.empty();
                }
                if (!skip && ecb) {
                    mvs_encoded_rows b{};
                    b.row_begin = it.row_begin;
                    b.row_end = it.row_end;
                    b.n_cells = it.n_cells;
                    b.n_rows = (int64_t)it.rows.size();
                    b.rows = it.rows.data();
                    b.first_col = it.first_col.data();
                    b.offset = it.offset.data();
                    b.jac_bytes = it.jac_bytes.data();
                    b.bytes = static_cast<const uint8_t*>(c->dl_pinned[it.slot].p);
                    b.n_bytes = it.n_bytes;
                    try {
                        status = ecb(user, &b);
                    } catch (...) {
                        status = -1;
                    }
                } else if (!skip) {
                    mvs_row_block b{};
                    b.row_begin = it.row_begin;
                    b.row_end = it.row_end;
                    b.n_cells = it.n_cells;
                    b.row_ptr = it.row_ptr.data();
                    const char* base = static_cast<const char*>(c->dl_pinned[it.slot].p);
                    b.col = reinterpret_cast<const int32_t*>(base);
                    const char* qbase = base + (size_t)it.n_cells * 4;
                    b.q = it.wide ? nullptr : reinterpret_cast<const uint8_t*>(qbase);
                    b.q16 = it.wide ? reinterpret_cast<const uint16_t*>(qbase) : nullptr;
                    try {
                        status = cb(user, &b);
                    } catch (...) {            // a C++ callback that throws: no exception crosses the C boundary
                        status = -1;
                    }
                }
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                if (status != 0 && cb_status == 0) cb_status = status;
                slot_busy[it.slot] = false;
                if (it.last_of_block) ++done_blocks;
            }
            cv.notify_all();
        }
    }
    int acquire_slot() {                    // blocks until one of the two pinned buffers is free
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !slot_busy[0] || !slot_busy[1]; });
        const int sl = slot_busy[0] ? 1 : 0;
        slot_busy[sl] = true;
        return sl;
    }
    void release_slot(int sl) {
        {
            std::lock_guard<std::mutex> lk(mu);
            slot_busy[sl] = false;
        }
        cv.notify_all();
    }
    void push(Item&& it) {
        {
            std::lock_guard<std::mutex> lk(mu);
            queue.push_back(std::move(it));
        }
        cv.notify_all();
    }
    bool failed() {
        std::lock_guard<std::mutex> lk(mu);
        return cb_status != 0 || !error.empty();
    }
    void close() {
        {
            std::lock_guard<std::mutex> lk(mu);
            closing = true;
        }
        cv.notify_all();
        if (worker.joinable()) worker.join();
    }
    ~StreamOut() {
        close_feeder();
        close();
    }
};

int ensure_download_side(mvs_ctx* c) {
    if (!c->dl_stream) {
        HIP_TRY(c->dl_stream.create(hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            HIP_TRY(c->dl_done[i].create(hipEventDisableTiming));
            HIP_TRY(c->dl_block[i].create(hipEventDisableTiming));
        }
        for (int i = 0; i < 2; ++i) HIP_TRY(c->dl_ready[i].create(hipEventDisableTiming));
        HIP_TRY(c->post_stream.create(hipStreamNonBlocking));
        HIP_TRY(c->cmp_done.create(hipEventDisableTiming));
    }
    return MVS_OK;
}

// pinned buffer `slot` holds at least `bytes`; called by the producer while it owns the slot (nobody reads it)
int ensure_pinned_slot(mvs_ctx* c, int slot, size_t bytes) {
    if (c->dl_pinned[slot].bytes >= bytes) return MVS_OK;
    HIP_TRY(c->dl_pinned[slot].alloc(bytes));
    return MVS_OK;
}

// A row block on its way out: its CSR arrays sit in set `set` of the context (device), row_ptr is on the host.
struct BlockCsr {
    int64_t rb = 0, re = 0, n = 0;
    std::vector<int64_t> row_ptr;      // re - rb + 1 entries
    bool wide = false;                 // q is 16 bits wide in this block
    int set = 0;
    // rows encoded on the device: byte offset of every row's record (rows + 1 entries), directory values per row
    bool sizes_ready = false;          // the encoder's per-row sizes (en_size / en_jac / en_first / en_par) are on the device already
    bool encoded = false;
    std::vector<uint64_t> enc_off;
    std::vector<uint32_t> enc_jac, enc_first;
};

// The CSR arrays of `b` (set b.set) -> the rows' shard records in c->st_enc[b.set].p, directory on the host; on stream `ps`
// (the context's stream, or the side stream on which a dense block is post-processed beside the next comparison)
int encode_block(mvs_ctx* c, BlockCsr& b, hipStream_t ps) {
    const int64_t rows = b.re - b.rb;
    b.encoded = true;
    b.enc_off.assign((size_t)rows + 1, 0);
    b.enc_jac.assign((size_t)rows, 0);
    b.enc_first.assign((size_t)rows, 0);
    if (b.n == 0 || rows == 0) {
        HIP_TRY(hipEventRecord(c->dl_ready[b.set], ps));
        return MVS_OK;
    }
    int rc = ensure_buf(c, c->en_size, (size_t)(rows + 1) * 8);
    if (rc == MVS_OK) rc = ensure_buf(c, c->en_off, (size_t)(rows + 1) * 8);
    if (rc == MVS_OK) rc = ensure_buf(c, c->en_jac, (size_t)rows * 4);
    if (rc == MVS_OK) rc = ensure_buf(c, c->en_first, (size_t)rows * 4);
    if (rc == MVS_OK) rc = ensure_buf(c, c->en_par, (size_t)rows * sizeof(mvs::EncRow));
    if (rc) return rc;
    const int qb = b.wide ? 2 : 1;
    HIP_TRY(hipMemsetAsync((char*)c->en_size.p + (size_t)rows * 8, 0, 8, ps));
    if (!b.sizes_ready) {                  // (a dense block's fill pass has computed them already)
        mvs::launch_encode_sizes(ps, (const long long*)c->st_rowptr.p, (const int32_t*)c->st_col[b.set].p, c->st_q[b.set].p, qb, rows,
                                 (unsigned long long*)c->en_size.p, (unsigned int*)c->en_jac.p, (unsigned int*)c->en_first.p,
                                 (mvs::EncRow*)c->en_par.p);
        rc = check_kernel("k_enc_size");
        if (rc) return rc;
    }
    size_t need = 0;
    rc = mvs::encode_offsets(ps, (unsigned long long*)c->en_size.p, (unsigned long long*)c->en_off.p, rows, nullptr, 0, &need);
    if (rc) return fail(rc, "scan sizing failed");
    rc = ensure_buf(c, c->pw_sort, need);
    if (rc) return rc;
    rc = mvs::encode_offsets(ps, (unsigned long long*)c->en_size.p, (unsigned long long*)c->en_off.p, rows, c->pw_sort.p,
                             c->pw_sort.bytes, nullptr);
    if (rc) return fail(rc, "scan of the record sizes failed");
    rc = read_back(c, ps, {{b.enc_off.data(), c->en_off.p, (size_t)(rows + 1) * 8},
                           {b.enc_jac.data(), c->en_jac.p, (size_t)rows * 4},
                           {b.enc_first.data(), c->en_first.p, (size_t)rows * 4}});
    if (rc) return rc;
    const size_t total = (size_t)b.enc_off[(size_t)rows];
    rc = ensure_buf(c, c->st_enc[b.set], std::max<size_t>(total, 8));
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->st_enc[b.set].p, 0, total, ps));       // the unary parts are OR-ed into zeroed words
    mvs::launch_encode_fill(ps, (const long long*)c->st_rowptr.p, (const int32_t*)c->st_col[b.set].p, c->st_q[b.set].p, qb, rows,
                            (const unsigned long long*)c->en_off.p, (const mvs::EncRow*)c->en_par.p, (unsigned char*)c->st_enc[b.set].p,
                            c->opt.encode_stage_words);
    rc = check_kernel("k_enc_fill");
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->dl_ready[b.set], ps));
    return MVS_OK;
}

// before the CSR arrays of set `set` are rewritten: the downloads of the block that used them last (two blocks ago) are through
int claim_csr_set(mvs_ctx* c, int set, int64_t block_index, int64_t n, bool wide, hipStream_t ps) {
    // (with DMA copies the driving thread has waited for the callback thread to see that block's last piece: StreamOut::wait_done)
    if (block_index >= 2 && c->opt.stream_copy == 0) HIP_TRY(hipStreamWaitEvent(ps, c->dl_block[set], 0));
    int rc = ensure_buf(c, c->st_col[set], (size_t)std::max<int64_t>(n, 1) * 4);
    if (rc) return rc;
    return ensure_buf(c, c->st_q[set], (size_t)std::max<int64_t>(n, 1) * (wide ? 2 : 1));
}

// n packed cells of rows [rb, re) sit in c->st_raw.p: radix sort on the (row, col) bits, then row_ptr / col / q
int csr_from_packed(mvs_ctx* c, int64_t rb, int64_t re, int64_t n, int shift, int col_bits, int64_t block_index, BlockCsr& out) {
    const int64_t rows = re - rb;
    const int row_bits = bits_for(std::max<int64_t>(rows - 1, 1));
    out.rb = rb;
    out.re = re;
    out.n = n;
    out.wide = false;
    out.set = (int)(block_index & 1);
    out.row_ptr.assign((size_t)rows + 1, 0);
    if (n == 0) {
        HIP_TRY(hipEventRecord(c->dl_ready[out.set], c->stream));
        return MVS_OK;
    }
    int rc = ensure_buf(c, c->st_rowptr, (size_t)(rows + 1) * 8);
    if (rc) return rc;
    rc = ensure_buf(c, c->st_sorted, (size_t)n * 8);
    if (rc) return rc;
    size_t need = 0;
    rc = mvs::sort_packed(c->stream, (unsigned long long*)c->st_raw.p, (unsigned long long*)c->st_sorted.p, n, 16, shift + row_bits,
                          nullptr, 0, &need);
    if (rc) return fail(rc, "sort sizing failed");
    rc = ensure_buf(c, c->pw_sort, need);
    if (rc) return rc;
    rc = mvs::sort_packed(c->stream, (unsigned long long*)c->st_raw.p, (unsigned long long*)c->st_sorted.p, n, 16, shift + row_bits,
                          c->pw_sort.p, c->pw_sort.bytes, nullptr);
    if (rc) return fail(rc, "sort of the kept cells failed");
    rc = claim_csr_set(c, out.set, block_index, n, false, c->stream);
    if (rc) return rc;
    unsigned int* d_wide = reinterpret_cast<unsigned int*>(c->counters() + 3);
    HIP_TRY(hipMemsetAsync(d_wide, 0, 4, c->stream));
    const unsigned long long col_mask = (1ULL << col_bits) - 1ULL;
    mvs::launch_packed_csr(c->stream, (const unsigned long long*)c->st_sorted.p, n, shift, rows, col_mask, (long long*)c->st_rowptr.p,
                           (int32_t*)c->st_col[out.set].p, (uint8_t*)c->st_q[out.set].p, nullptr, d_wide);
    rc = check_kernel("k_packed_csr");
    if (rc) return rc;
    unsigned int h_wide = 0;
    HIP_TRY(hipMemcpyAsync(out.row_ptr.data(), c->st_rowptr.p, (size_t)(rows + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&h_wide, d_wide, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h_wide) {                      // some q needs 16 bits (norms that do not belong to the vectors): redo the q array
        out.wide = true;
        rc = ensure_buf(c, c->st_q[out.set], (size_t)n * 2);
        if (rc) return rc;
        mvs::launch_packed_csr(c->stream, (const unsigned long long*)c->st_sorted.p, n, shift, rows, col_mask, nullptr,
                               (int32_t*)c->st_col[out.set].p, nullptr, (uint16_t*)c->st_q[out.set].p, nullptr);
        rc = check_kernel("k_packed_csr(16-bit q)");
        if (rc) return rc;
    }
    if (out.row_ptr[(size_t)rows] != n) return fail(MVS_E_HIP, "internal: row index of the sorted cells is inconsistent");
    HIP_TRY(hipEventRecord(c->dl_ready[out.set], c->stream));          // the downloads of this block wait for exactly this point
    return MVS_OK;
}

// What the two row passes of a dense block share: rows [rb, re) of the dense byte matrix (first row dense_row0, leading dimension
// ld) become block `block_index`, the buffers of count and scan, the active tiles of the block's tile rows and every row's first /
// last kept column; *first = the block's first row in the matrix
int dense_rows_head(mvs_ctx* c, int64_t rb, int64_t re, int64_t n_cols, int64_t dense_row0, int64_t ld, int64_t block_index,
                    BlockCsr& out, mvs::DenseActive& active, const uint8_t** first) {
    active.row_rel0 = rb - dense_row0;
    const int64_t rows = re - rb;
    out.rb = rb;
    out.re = re;
    out.wide = false;
    out.set = (int)(block_index & 1);
    out.row_ptr.assign((size_t)rows + 1, 0);
    int rc = ensure_buf(c, c->st_rowptr, (size_t)(rows + 1) * 8);
    if (rc == MVS_OK) rc = ensure_buf(c, c->st_counts, (size_t)(rows + 1) * 8);
    if (rc) return rc;
    int tr0 = 0, n_trows = 0, n_tc = 0;
    mvs::dense_tile_rows(active, rows, n_cols, &tr0, &n_trows, &n_tc);
    rc = ensure_buf(c, c->st_tlist, std::max<size_t>((size_t)n_trows * (size_t)n_tc * 4, 4));
    if (rc == MVS_OK) rc = ensure_buf(c, c->st_tlist_n, std::max<size_t>((size_t)n_trows * 4, 4));
    if (rc == MVS_OK) rc = ensure_buf(c, c->st_ends, std::max<size_t>((size_t)rows * sizeof(int2), 8));
    *first = (const uint8_t*)c->st_dense.p + (size_t)(rb - dense_row0) * (size_t)ld;
    return rc;
}

// rows [rb, re) of the dense byte matrix are final: count, scan, fill.
// *odd: some kept cell of the launches so far has a q the byte cannot hold -- the caller redoes the block as a list.
int csr_from_dense(mvs_ctx* c, int64_t rb, int64_t re, int64_t n_cols, int64_t dense_row0, int64_t ld, int64_t block_index,
                   BlockCsr& out, bool* odd, hipStream_t ps, mvs::DenseActive active, bool want_sizes) {
    const int64_t rows = re - rb;
    const uint8_t* first = nullptr;
    int rc = dense_rows_head(c, rb, re, n_cols, dense_row0, ld, block_index, out, active, &first);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync((char*)c->st_counts.p + (size_t)rows * 8, 0, 8, ps));
    mvs::launch_dense_count(ps, first, ld, n_cols, rows, (long long*)c->st_counts.p, (int2*)c->st_ends.p, active, (int*)c->st_tlist.p,
                            (int*)c->st_tlist_n.p);
    rc = check_kernel("k_dense_count");
    if (rc) return rc;
    size_t need = 0;
    rc = mvs::dense_row_ptr(ps, (long long*)c->st_counts.p, (long long*)c->st_rowptr.p, rows, nullptr, 0, &need);
    if (rc) return fail(rc, "scan sizing failed");
    rc = ensure_buf(c, c->pw_sort, need);
    if (rc) return rc;
    rc = mvs::dense_row_ptr(ps, (long long*)c->st_counts.p, (long long*)c->st_rowptr.p, rows, c->pw_sort.p, c->pw_sort.bytes, nullptr);
    if (rc) return fail(rc, "scan of the row counts failed");
    unsigned int h_odd = 0;
    rc = read_back(c, ps, {{out.row_ptr.data(), c->st_rowptr.p, (size_t)(rows + 1) * 8}, {&h_odd, c->counters() + 4, 4}});
    if (rc) return rc;
    *odd = h_odd != 0;
    if (*odd) return MVS_OK;
    out.n = out.row_ptr[(size_t)rows];
    rc = claim_csr_set(c, out.set, block_index, out.n, false, ps);
    if (rc) return rc;
    // rows that will be encoded on the device: the record sizes come out of the fill pass (k_enc_size would read the CSR
    // arrays this pass is writing once more)
    if (want_sizes && rows > 0) {
        rc = ensure_buf(c, c->en_size, (size_t)(rows + 1) * 8);
        if (rc == MVS_OK) rc = ensure_buf(c, c->en_jac, (size_t)rows * 4);
        if (rc == MVS_OK) rc = ensure_buf(c, c->en_first, (size_t)rows * 4);
        if (rc == MVS_OK) rc = ensure_buf(c, c->en_par, (size_t)rows * sizeof(mvs::EncRow));
        if (rc) return rc;
    }
    const bool sizes = want_sizes && rows > 0 && out.n > 0;
    mvs::launch_dense_fill(ps, first, ld, n_cols, rows, (const long long*)c->st_rowptr.p, (int32_t*)c->st_col[out.set].p,
                           (uint8_t*)c->st_q[out.set].p, active, (const int*)c->st_tlist.p, (const int*)c->st_tlist_n.p,
                           (const int2*)c->st_ends.p, sizes ? (unsigned long long*)c->en_size.p : nullptr, (unsigned int*)c->en_jac.p,
                           (unsigned int*)c->en_first.p, (mvs::EncRow*)c->en_par.p);
    rc = check_kernel("k_dense_fill");
    if (rc) return rc;
    out.sizes_ready = sizes;
    HIP_TRY(hipEventRecord(c->dl_ready[out.set], ps));
    return MVS_OK;
}

// The row passes of a dense block WITHOUT a host round trip in their middle (rows delivered encoded): csr_from_dense reads the
// block's cell count back before it sizes the CSR arrays, encode_block the record sizes before it sizes the record buffer -- two
// host round trips per block, each of them a bubble in front of kernels that then queue behind the link's copy kernels.  Here the
// arrays are sized from what the blocks before this one held (cap_cells, cap_bytes: the caller's estimate with head room), all
// passes are queued in one go -- the kernels drop what would not fit --, and ONE read-back at the end brings the row index, the
// record directory and the totals: *held says whether the sizes held (if not, nothing of this block has been delivered and the
// caller does it again the careful way).
int rows_from_dense_spec(mvs_ctx* c, int64_t rb, int64_t re, int64_t n_cols, int64_t dense_row0, int64_t ld, int64_t block_index,
                         BlockCsr& out, bool* odd, hipStream_t ps, mvs::DenseActive active, int64_t cap_cells, size_t cap_bytes,
                         int stage_words, bool* held) {
    *held = false;
    *odd = false;
    const int64_t rows = re - rb;
    const uint8_t* first = nullptr;
    int rc = dense_rows_head(c, rb, re, n_cols, dense_row0, ld, block_index, out, active, &first);
    if (rc == MVS_OK) rc = ensure_buf(c, c->en_size, (size_t)(rows + 1) * 8);
    if (rc == MVS_OK) rc = ensure_buf(c, c->en_off, (size_t)(rows + 1) * 8);
    if (rc == MVS_OK) rc = ensure_buf(c, c->en_jac, (size_t)rows * 4);
    if (rc == MVS_OK) rc = ensure_buf(c, c->en_first, (size_t)rows * 4);
    if (rc == MVS_OK) rc = ensure_buf(c, c->en_par, (size_t)rows * sizeof(mvs::EncRow));
    if (rc == MVS_OK) rc = claim_csr_set(c, out.set, block_index, cap_cells, false, ps);
    if (rc == MVS_OK) rc = ensure_buf(c, c->st_enc[out.set], std::max<size_t>(cap_bytes, 8));
    if (rc) return rc;
    size_t need = 0, need2 = 0;
    rc = mvs::dense_row_ptr(ps, (long long*)c->st_counts.p, (long long*)c->st_rowptr.p, rows, nullptr, 0, &need);
    if (rc == MVS_OK) rc = mvs::encode_offsets(ps, (unsigned long long*)c->en_size.p, (unsigned long long*)c->en_off.p, rows, nullptr, 0, &need2);
    if (rc) return fail(rc, "scan sizing failed");
    rc = ensure_buf(c, c->pw_sort, std::max(need, need2));
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync((char*)c->st_counts.p + (size_t)rows * 8, 0, 8, ps));
    mvs::launch_dense_count(ps, first, ld, n_cols, rows, (long long*)c->st_counts.p, (int2*)c->st_ends.p, active, (int*)c->st_tlist.p,
                            (int*)c->st_tlist_n.p);
    rc = check_kernel("k_dense_count");
    if (rc) return rc;
    rc = mvs::dense_row_ptr(ps, (long long*)c->st_counts.p, (long long*)c->st_rowptr.p, rows, c->pw_sort.p, c->pw_sort.bytes, nullptr);
    if (rc) return fail(rc, "scan of the row counts failed");
    HIP_TRY(hipMemsetAsync((char*)c->en_size.p + (size_t)rows * 8, 0, 8, ps));
    mvs::launch_dense_fill(ps, first, ld, n_cols, rows, (const long long*)c->st_rowptr.p, (int32_t*)c->st_col[out.set].p,
                           (uint8_t*)c->st_q[out.set].p, active, (const int*)c->st_tlist.p, (const int*)c->st_tlist_n.p,
                           (const int2*)c->st_ends.p, (unsigned long long*)c->en_size.p, (unsigned int*)c->en_jac.p, (unsigned int*)c->en_first.p,
                           (mvs::EncRow*)c->en_par.p, (long long)cap_cells);
    rc = check_kernel("k_dense_fill");
    if (rc) return rc;
    rc = mvs::encode_offsets(ps, (unsigned long long*)c->en_size.p, (unsigned long long*)c->en_off.p, rows, c->pw_sort.p, c->pw_sort.bytes,
                             nullptr);
    if (rc) return fail(rc, "scan of the record sizes failed");
    HIP_TRY(hipMemsetAsync(c->st_enc[out.set].p, 0, cap_bytes, ps));        // the unary parts are OR-ed into zeroed words
    mvs::launch_encode_fill(ps, (const long long*)c->st_rowptr.p, (const int32_t*)c->st_col[out.set].p, c->st_q[out.set].p, 1, rows,
                            (const unsigned long long*)c->en_off.p, (const mvs::EncRow*)c->en_par.p, (unsigned char*)c->st_enc[out.set].p,
                            stage_words, (unsigned long long)cap_cells, (unsigned long long)cap_bytes);
    rc = check_kernel("k_enc_fill");
    if (rc) return rc;
    out.enc_off.assign((size_t)rows + 1, 0);
    out.enc_jac.assign((size_t)rows, 0);
    out.enc_first.assign((size_t)rows, 0);
    unsigned int h_odd = 0;
    rc = read_back(c, ps, {{out.row_ptr.data(), c->st_rowptr.p, (size_t)(rows + 1) * 8},
                           {out.enc_off.data(), c->en_off.p, (size_t)(rows + 1) * 8},
                           {out.enc_jac.data(), c->en_jac.p, (size_t)rows * 4},
                           {out.enc_first.data(), c->en_first.p, (size_t)rows * 4},
                           {&h_odd, c->counters() + 4, 4}});
    if (rc) return rc;
    *odd = h_odd != 0;
    out.n = out.row_ptr[(size_t)rows];
    if (*odd || out.n > cap_cells || out.enc_off[(size_t)rows] > (uint64_t)cap_bytes) return MVS_OK;     // (*held stays false)
    out.sizes_ready = true;
    out.encoded = true;
    *held = true;
    HIP_TRY(hipEventRecord(c->dl_ready[out.set], ps));
    return MVS_OK;
}

// What leaves the device of a block, in one of two forms: its CSR arrays (columns, then q) or its encoded records.  offsets[0 ..
// rows] count the units a piece is measured in (cells / bytes); a piece of `units` from offset o0 is, per range, units * per_unit
// bytes from base + o0 * per_unit, one range after the other in the pinned buffer.
struct CopyRange {
    const void* base;
    size_t per_unit;
};
template <class Off>
struct PieceForm {
    const Off* offsets;
    int n_ranges;
    CopyRange ranges[2];
    const char* what;                                          // (in the error texts)
    void (*fill)(StreamOut::Item& it, const BlockCsr& b, int64_t r0, int64_t r1);      // the piece's row index / directory
};
void fill_csr(StreamOut::Item& it, const BlockCsr& b, int64_t r0, int64_t r1) {
    const int64_t c0 = b.row_ptr[(size_t)r0];
    it.n_cells = b.row_ptr[(size_t)r1] - c0;
    it.row_ptr.resize((size_t)(r1 - r0) + 1);
    for (int64_t r = r0; r <= r1; ++r) it.row_ptr[(size_t)(r - r0)] = b.row_ptr[(size_t)r] - c0;
}
void fill_encoded(StreamOut::Item& it, const BlockCsr& b, int64_t r0, int64_t r1) {      // the directory of the piece's non-empty rows
    it.n_cells = b.row_ptr[(size_t)r1] - b.row_ptr[(size_t)r0];
    it.n_bytes = (int64_t)(b.enc_off[(size_t)r1] - b.enc_off[(size_t)r0]);
    for (int64_t r = r0; r < r1; ++r)
        if (b.row_ptr[(size_t)r + 1] > b.row_ptr[(size_t)r]) {
            it.rows.push_back((uint32_t)(b.rb + r));
            it.first_col.push_back(b.enc_first[(size_t)r]);
            it.jac_bytes.push_back(b.enc_jac[(size_t)r]);
            it.offset.push_back(b.enc_off[(size_t)r] - b.enc_off[(size_t)r0]);
        }
}

// the block out through the two pinned buffers, in pieces of whole rows of at most piece_bytes (one row alone may exceed that);
// the host blocks here only on the pinned buffers (the device is free to run the next block's comparison meanwhile)
template <class Off>
int feed_pieces(mvs_ctx* c, StreamOut& out, const BlockCsr& b, size_t piece_bytes, const PieceForm<Off>& form) {
    const int64_t rows = b.re - b.rb;
    const Off* off = form.offsets;
    size_t unit = 0;                                           // bytes of one unit in the pinned buffer
    for (int i = 0; i < form.n_ranges; ++i) unit += form.ranges[i].per_unit;
    const Off limit = std::max<Off>(1, (Off)(piece_bytes / unit));
    // a pinned buffer is sized for the block's largest piece when the producer takes it (it is idle then)
    const size_t need_bytes = std::max(std::min<size_t>(piece_bytes, std::max<size_t>((size_t)off[rows] * unit, 1u << 16)),
                                       (size_t)largest_piece(off, rows, limit) * unit);
    int rc = MVS_OK;
    const bool dma = c->opt.stream_copy != 0;
    const HsaCopy* h = nullptr;
    if (dma) {
        rc = ensure_hsa_copy(c);
        if (rc) return rc;
        h = static_cast<const HsaCopy*>(c->dl_hsa.get());
        HIP_TRY(hipEventSynchronize(c->dl_ready[b.set]));      // the block's arrays are final (this thread only feeds)
    }
    for (int64_t r0 = 0; r0 < rows;) {
        const int64_t r1 = piece_end(off, rows, r0, limit);
        const size_t o0 = (size_t)off[r0], units = (size_t)(off[r1] - off[r0]);
        if (out.failed()) return MVS_OK;                        // the caller reports the callback's status
        const int sl = out.acquire_slot();
        rc = ensure_pinned_slot(c, sl, need_bytes);
        if (rc) {
            out.release_slot(sl);
            return rc;
        }
        StreamOut::Item it;
        it.slot = sl;
        it.row_begin = b.rb + r0;
        it.row_end = b.rb + r1;
        it.wide = b.wide;
        form.fill(it, b, r0, r1);
        it.dma = dma;
        it.last_of_block = dma && r1 == rows;
        // DMA: the slot's signal counts the copies down; otherwise the copies wait for the block on the download stream
        hsa_status_t hs = HSA_STATUS_SUCCESS;
        hipError_t e = hipSuccess;
        if (dma) hsa_signal_store_relaxed(h->sig[sl], units > 0 ? form.n_ranges : 0);
        else e = hipStreamWaitEvent(c->dl_stream, c->dl_ready[b.set], 0);
        char* dst = static_cast<char*>(c->dl_pinned[sl].p);
        for (int i = 0; i < form.n_ranges && units > 0 && hs == HSA_STATUS_SUCCESS && e == hipSuccess; ++i) {
            const size_t per = form.ranges[i].per_unit;
            const char* src = (const char*)form.ranges[i].base + o0 * per;
            if (dma) hs = hsa_amd_memory_async_copy(dst, h->cpu, src, h->gpu, units * per, 0, nullptr, h->sig[sl]);
            else e = hipMemcpyAsync(dst, src, units * per, hipMemcpyDeviceToHost, c->dl_stream);
            dst += units * per;
        }
        if (!dma && e == hipSuccess) e = hipEventRecord(c->dl_done[sl], c->dl_stream);
        if (hs != HSA_STATUS_SUCCESS || e != hipSuccess) {
            if (dma) hsa_signal_store_relaxed(h->sig[sl], 0);
            out.release_slot(sl);
            return dma ? fail(MVS_E_HIP, "DMA download of %s failed (hsa status %d)", form.what, (int)hs)
                       : fail(MVS_E_HIP, "download of %s: %s", form.what, hipGetErrorString(e));
        }
        out.push(std::move(it));
        ++c->st.pieces;
        c->st.bytes += (long long)(units * unit);
        r0 = r1;
    }
    if (!dma) HIP_TRY(hipEventRecord(c->dl_block[b.set], c->dl_stream));
    return MVS_OK;
}
int feed(mvs_ctx* c, StreamOut& out, const BlockCsr& b, size_t piece_bytes, bool encoded) {
    if (encoded)
        return feed_pieces(c, out, b, piece_bytes, PieceForm<uint64_t>{b.enc_off.data(), 1, {{c->st_enc[b.set].p, 1}, {}}, "encoded rows", fill_encoded});
    const PieceForm<int64_t> csr{b.row_ptr.data(), 2, {{c->st_col[b.set].p, 4}, {c->st_q[b.set].p, (size_t)(b.wide ? 2 : 1)}}, "a row block", fill_csr};
    return feed_pieces(c, out, b, piece_bytes, csr);
}

// One call of mvs_pairwise_stream[_encoded] after its arguments have been checked: what the routes share, and the routes.
// decide() chooses one, run_list() / run_blocks() take it, and finish() is the only way out once the threads run: the methods
// return a status and the caller hands it to finish().
struct StreamJob {
    enum Route { kList, kMatrixPipeline, kMatrixWholePass, kExactBlocks };     // plans A, M1, M2, B of decide()

    // ---- the call ----
    mvs_ctx* c;
    const mvs_sketch_set* s;
    const double* d_n2;
    int keep_mode;
    int64_t row_begin, row_end, rows_all;
    mvs_encoded_rows_cb ecb;
    int64_t* n_cells;
    int64_t budget_cells;
    size_t dense_budget, piece_bytes;
    int col_bits, shift;
    int64_t ld;                                                // leading dimension of the dense byte matrix
    int64_t total = 0;                                         // kept cells delivered so far
    // option stream_trace: where the host is when (ms since the call started)
    std::chrono::steady_clock::time_point t_call;
    std::vector<std::pair<std::string, double>> trace;
    // ---- the route ----
    // M1 pins the filter kernel the whole range would get, the exact-kernel blocks switch the filter off: both in a COPY of
    // the context's options that the comparison stages below are handed (the context itself is never written: a host that
    // drives several contexts from several threads must not find another call's forced variant in one of them)
    mvs::Options lopt;
    int saved_variant;
    Route route = kExactBlocks;                                // (of the blocks still to come: a list fallback makes it kExactBlocks)
    bool fits_word = false, dense_ok = false, matrix_fits = false, can_matrix = false;
    mvs::PairwiseArgs wa{};                                    // the whole row range as one symmetric block
    int n_tr_all = 0, n_tc_all = 0, tile_o = 0;                // its grid of 256 x 256 tiles, the tile row of row_begin
    TwoStage ts;                                               // M2, plan A: the whole pass; M1: the current segment's pass
    unsigned long long bound = 0;                              // plan A: the list's size (list_bound)
    mvs::DenseActive active{};                                 // flags == NULL: every tile (plan B)
    // ---- the row blocks ----
    hipStream_t ps;                                            // where a block is turned into CSR / encoded rows (see `side`)
    bool side = false;
    bool tiles_phase = false;   // the launches being timed are runs of flagged tiles (ev[6] .. ev[3]), not whole comparisons
    bool dense = false, whole = false;
    int64_t block_rows = 0;
    RowBlocks blocks;
    std::vector<char> seg_first;                               // M1: the blocks that open a filter segment (segment_opens)
    int64_t seg_row0 = 0;
    bool seg_exact = false;
    // what the dense blocks so far held per row (cells, record bytes): sizes the next block's buffers when its row passes are
    // queued without reading its own totals first (rows_from_dense_spec, option stream_spec)
    double spec_cells_per_row = -1.0, spec_bytes_per_row = -1.0;
    StreamOut out;                                             // (last: its threads are joined before anything above goes)

    StreamJob(mvs_ctx* ctx, const mvs_sketch_set* set, const double* norms, int keep, int64_t rb, int64_t re, size_t budget,
              size_t dense_budget_bytes, mvs_row_block_cb cb, mvs_encoded_rows_cb encoded_cb, void* user, int64_t* cells_out)
        : c(ctx), s(set), d_n2(norms), keep_mode(keep), row_begin(rb), row_end(re), rows_all(re - rb), ecb(encoded_cb),
          n_cells(cells_out), budget_cells(std::max<int64_t>(1 << 16, (int64_t)(budget / 22))), dense_budget(dense_budget_bytes),
          piece_bytes((size_t)ctx->opt.stream_piece_mib << 20),   // pinned buffer size (32 MiB): pinning costs ~0.3 ms per MiB
          col_bits(bits_for(std::max<int64_t>(set->n - 1, 1))), shift(16 + col_bits), ld((set->n + 127) / 128 * 128),
          lopt(ctx->opt), saved_variant(lopt.filter_variant), ps(ctx->stream), out(ctx, cb, encoded_cb, user) {}
    void start() {
        out.worker = std::thread([this] { out.run(); });
        out.feeder = std::thread([this] { out.feed_run(); });
        t_call = std::chrono::steady_clock::now();
    }

    void add_kernel_ms() {
        float ms = 0.0f;
        if (c->timing && c->ev_valid[1] && hipEventSynchronize(c->ev[3]) == hipSuccess &&
            hipEventElapsedTime(&ms, tiles_phase ? c->ev[6] : c->ev[2], c->ev[3]) == hipSuccess)
            c->st.kernel_ms += ms;
    }
    // a block's way out, in two steps so that the next block's comparison can be queued between them: prepare = the
    // device-side work that is left (encoding the rows, where the caller asked for that), deliver = pieces to the link
    int prepare(BlockCsr& blk) { return (ecb && !blk.encoded) ? encode_block(c, blk, ps) : MVS_OK; }
    void deliver(BlockCsr& blk) {
        auto sp = std::make_shared<BlockCsr>(std::move(blk));
        out.enqueue_feed([ctx = c, o = &out, sp, piece = piece_bytes, enc = ecb != nullptr]() -> int { return feed(ctx, *o, *sp, piece, enc); });
    }
    // the arrays of block k live in set k & 1: before block k is built the feeder must be through with block k - 2
    void wait_for_set(int64_t k) {
        if (k >= 2) out.wait_fed(k - 1);
        if (k >= 2 && c->opt.stream_copy != 0) out.wait_done(k - 1);      // (DMA copies: block k - 2 has left the device)
    }
    void mark(const char* what, long k) {
        if (!c->opt.stream_trace) return;
        char buf[64];
        snprintf(buf, sizeof buf, "%s[%ld]", what, k);
        trace.emplace_back(buf, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count());
    }
    int finish(int status) {
        mark("close", -1);
        out.close_feeder();                                     // every delivered block has been handed to the link
        out.close();                                            // ... and consumed
        (void)hipStreamSynchronize(c->dl_stream);
        if (side) (void)hipStreamSynchronize(c->post_stream);
        mark("done", -1);
        if (c->opt.stream_trace) {
            std::string line = "[mvs stream trace]";
            for (auto& t : trace) {
                char buf[96];
                snprintf(buf, sizeof buf, " %s %.2f", t.first.c_str(), t.second);
                line += buf;
            }
            fprintf(stderr, "%s\n", line.c_str());
        }
        if (n_cells) *n_cells = total;
        if (status != MVS_OK) return status;
        if (!out.error.empty()) return fail(MVS_E_HIP, "%s", out.error.c_str());
        if (out.cb_status != 0) return fail(MVS_E_ABORTED, "the row-block callback returned %d", out.cb_status);
        return MVS_OK;
    }

    // re-check of t's candidates with the kept cells going into the matrix: a packed list first (the re-check decides
    // which candidates are kept), then mark / clear / scatter (mvs_internal.h: launch_packed_to_dense)
    int recheck_into_matrix(TwoStage& t) {
        int r = ensure_buf(c, c->st_raw, (size_t)(2 * t.n_cand + 64) * 8);
        if (r) return r;
        t.a.dense = nullptr;
        t.a.packed = (unsigned long long*)c->st_raw.p;
        t.a.capacity = c->st_raw.bytes / 8;
        t.a.pack_row0 = row_begin;
        t.a.pack_shift = shift;
        r = two_stage_recheck(c, t);
        if (r) return r;
        HIP_TRY(hipMemsetAsync(c->counters() + 10, 0, 8, c->stream));     // count of newly touched tiles
        mvs::launch_packed_to_dense(c->stream, (const unsigned long long*)c->st_raw.p, c->counters(), shift,
                                    (1ULL << col_bits) - 1ULL, (uint8_t*)c->st_dense.p, ld, rows_all, (unsigned int*)c->pw_ttouch.p, n_tc_all,
                                    (int*)c->pw_tnew.p, reinterpret_cast<unsigned int*>(c->counters() + 10),
                                    reinterpret_cast<unsigned int*>(c->counters() + 4));
        r = check_kernel("k_packed_touch / k_clear_tiles / k_packed_scatter");
        if (r) return r;
        // from here on t.a describes the exact kernel's launches on the flagged tiles: bytes of whole tiles into the matrix
        t.a.packed = nullptr;
        t.a.dense = (uint8_t*)c->st_dense.p;
        t.a.dense_row0 = row_begin;
        t.a.dense_ld = ld;
        t.a.dense_flag = reinterpret_cast<unsigned int*>(c->counters() + 4);
        return MVS_OK;
    }
    // M1, one block: filter its rows (symmetric square = the whole row range), re-check into the matrix, its flagged tiles
    int pipeline_filter(int64_t rb, int64_t re, TwoStage& t) {
        mvs::PairwiseArgs fa{};
        fill_args(c, s, d_n2, keep_mode, rb, re, 0, s->n, true, false, 0.05, fa, &lopt);
        fa.sym_begin = row_begin;
        fa.sym_end = row_end;
        t = TwoStage();
        t.ext_flags = (unsigned int*)c->pw_tflag.p + (size_t)((rb - row_begin) / 256) * (size_t)n_tc_all;
        return two_stage_filter(c, s, d_n2, 0.05, 0, true, 0, fa, t, &lopt);
    }

    // ---------------------------------------------------------------------------------------------------------------
    // How the kept cells leave the device is decided by how dense the result is, which only the filter can tell:
    //  A. sparse: ONE filter pass over the whole row range, candidates re-checked, the few flagged tiles computed, all kept
    //     cells in ONE packed list that is sorted on the device (needs the row field to fit the packed word).
    //  M. dense regions: the dense byte matrix -- one byte per cell, rows -> CSR / encoded rows by count / scan / fill passes
    //     that read only the tiles that can hold something (flagged by the filter, mirror images of those, touched by the
    //     re-check's kept cells: nothing else of the matrix is ever cleared or read) -- in row blocks, so that the link is
    //     fed while the comparison goes on.  Two ways to get there:
    //       M1 (pipeline): the filter itself runs block by block (first block one tile row: its flagged share tells sparse
    //          from dense, and costs 1 % of a whole pass when the answer is "sparse"), so a block's rows are final -- and
    //          on the link -- a millisecond after the call started instead of after the whole filter pass;
    //       M2: plan A's whole filter pass found too many cells for a list: its flags and candidates feed the matrix, the
    //          flagged tiles are computed block by block.
    //  B. the filter does not apply or gave up (nearly every tile dense): the exact kernel in row blocks (dense matrix with
    //     every tile active, or packed lists), as up to round 3.
    // ---------------------------------------------------------------------------------------------------------------
    // Sets `route`; the probe (M1) or the whole filter pass (A, M2) has run then and `ts` holds it.
    int decide() {
        fits_word = shift + bits_for(std::max<int64_t>(rows_all - 1, 1)) <= 64;
        mvs::PairwiseArgs probe{};
        probe.limbs = s->limbs;
        probe.d_pad = s->d_pad;
        dense_ok = mvs::exact_kernel_writes_dense(probe, lopt) && lopt.stream_dense != 0;
        matrix_fits = (size_t)rows_all * (size_t)ld <= dense_budget;
        const bool applies = two_stage_applies(c, s, row_begin, row_end, 0, s->n, 0.05, true, &lopt);
        fill_args(c, s, d_n2, keep_mode, row_begin, row_end, 0, s->n, true, false, 0.05, wa, &lopt);
        // the matrix flows need the tile grids to line up with the matrix's rows and the packed word to hold a row
        can_matrix = applies && dense_ok && matrix_fits && fits_word && row_begin % 256 == 0 && mvs::filter_flags_tiles(wa, lopt);
        mvs::filter_tile_grid(wa, &n_tr_all, &n_tc_all);
        tile_o = (int)(row_begin / 256);
        route = kExactBlocks;
        if (!applies) return MVS_OK;
        bool whole_pass = true;
        int rc = MVS_OK;
        if (can_matrix && rows_all > 512 && lopt.stream_pipeline != 0) {
            // M1's first block doubles as the probe: one tile row of the filter
            rc = ensure_buf(c, c->pw_tflag, (size_t)n_tr_all * (size_t)n_tc_all * 4);
            if (rc) return rc;
            if (lopt.filter_variant < 0) lopt.filter_variant = 8;    // what the whole range gets (filter_flags_tiles said so)
            rc = pipeline_filter(row_begin, row_begin + 256, ts);
            if (rc != MVS_OK && rc != kNeedExact) return rc;
            if (rc == kNeedExact) {                                  // the pass stopped: dense everywhere (never M1 then)
                // more than 70 % of the first tile row is dense: its cluster alone covers half of the matrix -- no further
                // filter pass, the exact kernel does the shard (plan B; the set is marked, two_stage_filter did that)
                whole_pass = false;
                lopt.filter_variant = saved_variant;
            } else if (probe_list_cells(ts.n_flagged, ts.n_cand, n_tr_all, n_tc_all) > (double)lopt.stream_list_cells) {
                route = kMatrixPipeline;
                whole_pass = false;
            } else {
                lopt.filter_variant = saved_variant;
            }
        }
        if (whole_pass && two_stage_applies(c, s, row_begin, row_end, 0, s->n, 0.05, true, &lopt)) {
            ts = TwoStage();
            rc = two_stage_filter(c, s, d_n2, 0.05, 0, true, 0, wa, ts, &lopt);
            if (rc != MVS_OK && rc != kNeedExact) return rc;
            if (rc == MVS_OK) {
                bound = list_bound(ts.n_cand, ts.n_flagged);
                size_t free_b = 0, total_b = 0;
                HIP_TRY(hipMemGetInfo(&free_b, &total_b));
                const bool list_fits = fits_word && (double)bound * 22.0 <= (double)free_b * 0.5;
                // stream_list_cells (2^26): below that the list (8 B per cell written, a radix sort over the key bits) is
                // cheaper than counting and filling a matrix of rows x n bytes
                if (list_fits && (bound <= (unsigned long long)lopt.stream_list_cells || !can_matrix || ts.n_flagged == 0)) route = kList;
                else if (can_matrix) route = kMatrixWholePass;
                // neither a list nor the matrix fits: plan B (the filter pass was in vain)
            }
        }
        return MVS_OK;
    }

    // plan A: the whole pass's candidates re-checked, its flagged tiles computed, one list, one block
    int run_list() {
        int rc = ensure_buf(c, c->st_raw, (size_t)(bound + 64) * 8);
        if (rc) return rc;
        ts.a.packed = (unsigned long long*)c->st_raw.p;
        ts.a.capacity = c->st_raw.bytes / 8;
        ts.a.pack_row0 = row_begin;
        ts.a.pack_shift = shift;
        rc = two_stage_recheck(c, ts);
        if (rc == MVS_OK) rc = two_stage_tiles(c, ts, 0, ts.n_flagged, true);
        if (rc) return rc;
        unsigned long long got = 0;
        rc = read_cell_count(&got);
        if (rc) return rc;
        if ((size_t)got * 8 > c->st_raw.bytes) return fail(MVS_E_HIP, "internal: kept cells beyond the sized output");
        total = (int64_t)got;
        add_kernel_ms();
        c->st.blocks = 1;
        c->st.two_stage = 1;
        BlockCsr blk;
        rc = csr_from_packed(c, row_begin, row_end, (int64_t)got, shift, col_bits, 0, blk);
        if (rc == MVS_OK) rc = prepare(blk);
        if (rc == MVS_OK) deliver(blk);
        return rc;
    }

    // the block list: dense blocks or list blocks, their size, the ramp, M1's segments
    void plan_blocks() {
        dense = dense_ok;
        whole = false;
        if (dense) {
            whole = row_begin % 128 == 0 && matrix_fits;             // the symmetric schedule needs the tile grids to line up
                                                                     // (the matrix flows imply both)
            block_rows = dense_block_rows(whole, rows_all, dense_budget, ld, lopt.stream_block_rows);
            dense = block_rows > 0;                                  // not even 256 rows of bytes: list blocks instead
        }
        if (!dense) block_rows = list_block_rows(budget_cells, s->n, shift);
        // blocks of one shared matrix start small (M1: one tile row, the probe; otherwise 1024 rows) and double: the link has
        // nothing to do until the first block has been compared, counted, filled and encoded
        int64_t ramp = block_rows;
        if (dense && whole && lopt.stream_block_rows == 0 && block_rows > 1024) ramp = 1024;
        if (route == kMatrixPipeline) ramp = 256;
        blocks = row_blocks(row_begin, row_end, block_rows, ramp);
        if (route == kMatrixPipeline) seg_first = segment_opens(blocks, row_begin, row_end, lopt.stream_block_rows > 0);
    }
    // the dense byte matrix before the first launch.  Matrix flows: the matrix of all rows, the touch map, the list of newly
    // touched tiles, the first re-check (M2: all candidates; M1: block 0's); plan B: the matrix of a block or of all rows
    int matrix_setup() {
        int rc = MVS_OK;
        if (route == kExactBlocks) {
            if (!dense) return MVS_OK;
            rc = ensure_buf(c, c->st_dense, (size_t)(whole ? rows_all : std::min(block_rows + 256, rows_all)) * (size_t)ld);
            if (rc) return rc;
            c->st_dense_zero = 0;
            const hipError_t e = hipMemsetAsync(c->counters() + 4, 0, 8, c->stream);      // the "q beyond a byte" flag
            return e == hipSuccess ? MVS_OK : fail(MVS_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
        }
        const void* before = c->st_dense.p;
        rc = ensure_buf(c, c->st_dense, (size_t)rows_all * (size_t)ld);
        if (rc) return rc;
        if (c->st_dense.p != before) c->st_dense_zero = 0;
        const size_t n_tiles = (size_t)n_tr_all * (size_t)n_tc_all;
        rc = ensure_buf(c, c->pw_ttouch, n_tiles * 4);
        if (rc) return rc;
        rc = ensure_buf(c, c->pw_tnew, (n_tiles + 1) * 4);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(c->pw_ttouch.p, 0, n_tiles * 4, c->stream));
        HIP_TRY(hipMemsetAsync(c->counters() + 4, 0, 8, c->stream));      // the "q beyond a byte" flag
        c->st_dense_zero = 0;
        active.touch = (const unsigned int*)c->pw_ttouch.p;
        active.n_tr = n_tr_all;
        active.n_tc = n_tc_all;
        active.o = tile_o;
        active.sym = (lopt.pairwise_symmetric != 0) ? 1 : 0;
        active.flags = route == kMatrixPipeline ? (const unsigned int*)c->pw_tflag.p : (const unsigned int*)ts.a.tile_flag;
        if (route == kMatrixPipeline) {
            // flags of blocks not yet filtered read as "not flagged"; block 0 has been filtered already (the probe)
            const size_t done = (size_t)n_tc_all;
            HIP_TRY(hipMemsetAsync((unsigned int*)c->pw_tflag.p + done, 0, ((size_t)n_tr_all * (size_t)n_tc_all - done) * 4, c->stream));
        }
        rc = recheck_into_matrix(ts);
        if (rc) return rc;
        add_kernel_ms();                                             // filter + re-check
        c->st.two_stage = route == kMatrixPipeline ? 3 : 2;
        return MVS_OK;
    }

    // the exact kernel on every tile of rows [rb, re) (plan B; also a block of M1 whose filter pass gave up)
    int launch_exact(int64_t rb, int64_t re, bool as_dense) {
        unsigned long long got = 0;
        mvs::Options exact_opt = lopt;                               // lopt with the filter switched off
        exact_opt.pairwise_filter = 0;
        if (as_dense) {
            DenseOut dno{(uint8_t*)c->st_dense.p, whole ? row_begin : rb, ld, whole ? row_begin : rb, whole ? row_end : re,
                         reinterpret_cast<unsigned int*>(c->counters() + 4)};
            return pairwise_launch(c, s, d_n2, keep_mode, rb, re, 0, s->n, true, false, nullptr, 0, 0, &got, 0.05, nullptr, &dno, &exact_opt);
        }
        const int64_t worst = (re - rb) * s->n;
        const int r = ensure_buf(c, c->st_raw, (size_t)worst * 8);
        if (r) return r;
        PackedOut po{&c->st_raw, rb, shift, false};
        return pairwise_launch(c, s, d_n2, keep_mode, rb, re, 0, s->n, true, false, nullptr, 0, 0, &got, 0.05, &po, nullptr, &exact_opt);
    }
    // M1, block k of the shared matrix
    int launch_pipeline(size_t k) {
        const int64_t rb = blocks[k].first, re = blocks[k].second;
        // The filter runs per SEGMENT of consecutive row blocks (seg_first: the blocks that open one; the probe's tile
        // row is segment 0): few passes -- each costs a launch over the whole column range and a host round trip -- yet
        // the first rows are final, and on the link, a millisecond after the call started.
        int r = MVS_OK;
        const bool opens = k < seg_first.size() && seg_first[k];
        if (k == 0) {
            seg_row0 = rb;                                       // the probe's tile row: filtered and re-checked already
            seg_exact = false;
        } else if (opens) {
            size_t last = k;
            while (last + 1 < blocks.size() && !seg_first[last + 1]) ++last;
            r = pipeline_filter(rb, blocks[last].second, ts);
            seg_row0 = rb;
            seg_exact = r == kNeedExact;
            if (r == MVS_OK) r = recheck_into_matrix(ts);
        } else if (seg_exact) {
            r = kNeedExact;
        }
        tiles_phase = !(opens && k > 0) && !seg_exact;           // a block that opens a segment is timed ev[2] .. ev[3]
        if (r == kNeedExact) {
            // nearly every tile of these rows is dense: the exact kernel on all of them.  Flag the tiles it writes itself
            // -- outside the square, on and above its diagonal -- so that the row passes read them and their mirror
            // images; the tiles below the diagonal stay what earlier blocks made of them
            const int t0 = (int)((rb - row_begin) / 256), t1 = (int)((re - row_begin + 255) / 256);
            for (int t = t0; t < t1; ++t) {
                unsigned int* rowf = (unsigned int*)c->pw_tflag.p + (size_t)t * (size_t)n_tc_all;
                hipError_t e = hipSuccess;
                if (tile_o > 0) e = hipMemsetD32Async((hipDeviceptr_t)rowf, 1, (size_t)tile_o, c->stream);
                if (e == hipSuccess && t + tile_o < n_tc_all)
                    e = hipMemsetD32Async((hipDeviceptr_t)(rowf + t + tile_o), 1, (size_t)(n_tc_all - t - tile_o), c->stream);
                if (e != hipSuccess) return fail(MVS_E_HIP, "hipMemsetD32Async: %s", hipGetErrorString(e));
            }
            c->filter_off_id = 0;                                // a verdict on these rows, not on the set
            return launch_exact(rb, re, true);
        }
        if (r) return r;
        // this block's share of the segment's flagged tiles (tile rows relative to the segment's first row)
        const int t0 = (int)((rb - seg_row0) / 256), t1 = (int)std::min<int64_t>(ts.n_tr, (re - seg_row0 + 255) / 256);
        return two_stage_tiles(c, ts, ts.row_first[(size_t)t0], ts.row_first[(size_t)t1] - ts.row_first[(size_t)t0], true);
    }
    // the comparison of block k: what a block's "launch" is depends on the route
    int launch(size_t k, bool as_dense) {
        const int64_t rb = blocks[k].first, re = blocks[k].second;
        if (route == kMatrixWholePass && as_dense) {                 // this block's share of the whole pass's flagged tiles
            tiles_phase = true;
            const int t0 = (int)((rb - row_begin) / 256), t1 = (int)std::min<int64_t>(ts.n_tr, (re - row_begin + 255) / 256);
            return two_stage_tiles(c, ts, ts.row_first[(size_t)t0], ts.row_first[(size_t)t1] - ts.row_first[(size_t)t0], true);
        }
        if (route == kMatrixPipeline && as_dense) return launch_pipeline(k);
        return launch_exact(rb, re, as_dense);
    }
    int read_cell_count(unsigned long long* got) {                   // of the launches queued so far, once they are through
        hipError_t e = hipMemcpyAsync(got, c->counters(), 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        return e == hipSuccess ? MVS_OK : fail(MVS_E_HIP, "reading the cell count: %s", hipGetErrorString(e));
    }
    // the row passes of dense block k: all queued at once with buffers sized from the blocks before where that is allowed and
    // holds, the careful way otherwise.  *odd: see csr_from_dense
    int rows_of_dense_block(size_t k, BlockCsr& blk, bool* odd) {
        const int64_t rb = blocks[k].first, re = blocks[k].second;
        int rc = MVS_OK;
        bool held = false;
        if (ecb && lopt.stream_spec != 0 && spec_cells_per_row >= 0.0) {
            const double rows_k = (double)(re - rb);
            const int64_t cap_cells = (int64_t)(rows_k * spec_cells_per_row * 1.3) + 65536;
            const size_t cap_bytes = ((size_t)(rows_k * spec_bytes_per_row * 1.3) + ((size_t)1 << 20) + 7) & ~(size_t)7;
            rc = rows_from_dense_spec(c, rb, re, s->n, whole ? row_begin : rb, ld, (int64_t)k, blk, odd, ps, active, cap_cells, cap_bytes,
                                      lopt.encode_stage_words, &held);
            if (rc) return rc;
            ++c->st.spec_blocks;
            if (!held) ++c->st.spec_redone;
            if (!held) blk = BlockCsr();          // the sizes did not hold (or a 16-bit q): the careful way below
        }
        if (!held) rc = csr_from_dense(c, rb, re, s->n, whole ? row_begin : rb, ld, (int64_t)k, blk, odd, ps, active, ecb != nullptr);
        if (rc) return rc;
        mark("csr", (long)k);
        if (!side) add_kernel_ms();
        if (!*odd) ++c->st.dense_blocks;
        return MVS_OK;
    }
    // a kept cell of dense block k whose q a byte cannot hold (norms that do not belong to the vectors): this block and the
    // rest go through the packed list, each block inside its own square -- the one case where a block is compared a second
    // time.  Block k has been launched again, as a list, when this returns.
    int fall_back_to_lists(size_t k) {
        ++c->st.list_fallbacks;
        if (side) {                 // back to one stream; a launch already queued for block k + 1 is wasted, not wrong
            (void)hipStreamSynchronize(c->stream);
            side = false;
            ps = c->stream;
        }
        dense = false;
        route = kExactBlocks;
        tiles_phase = false;
        lopt.filter_variant = saved_variant;
        const int64_t br = list_block_rows(budget_cells, s->n, shift);
        const RowBlocks rest = row_blocks(blocks[k].first, row_end, br, br);
        blocks.resize(k);
        blocks.insert(blocks.end(), rest.begin(), rest.end());
        return launch(k, false);
    }

    // Plan B proper: the exact kernel, software-pipelined -- block k+1 is launched before block k's pieces are fed to the
    // link.  Two ways for a block's cells to leave the kernel:
    //  * dense (two limbs on the ping-pong kernel): one byte per cell in a row-major matrix.  If the matrix of ALL the rows
    //    fits the budget the blocks share it and the symmetric schedule spans the whole square: a block's launch computes its
    //    tiles on and above the diagonal and writes the mirror images into later blocks' rows, so block k is final when
    //    launch k is.  Otherwise the matrix holds one block at a time and the symmetric schedule works inside each block's
    //    own square only;
    //  * packed list (any other kernel): blocks whose worst case -- every cell kept -- fits the budget.
    // The matrix flows M1 / M2 use the same loop with the shared matrix; only what a block's "launch" is differs.
    int run_blocks() {
        plan_blocks();
        int rc = matrix_setup();
        if (rc) return rc;
        // Blocks of ONE shared matrix: block k's rows are final when launch k is and launch k + 1 never touches them (its
        // mirror images land in later blocks' rows), so block k is counted / scanned / filled / encoded on a SIDE stream while
        // launch k + 1 already runs on the context's stream -- memory-bound passes beside a matrix-core-bound kernel instead
        // of between two of them.  (stream_dense = 2: everything on the context's stream, one after the other.)
        side = dense && whole && blocks.size() > 1 &&
               (lopt.stream_dense >= 3 || (lopt.stream_dense == 1 && route != kMatrixWholePass));
        // stream_dense = 4 (experiment): the row passes on the DOWNLOAD stream itself -- between two pieces' copies instead of beside
        // one (a device-to-host copy is a blit kernel that fills the card; a kernel that starts beside it ends with it)
        // stream_dense = 5 (experiment): ONE stream, but launch k + 1 is queued IN FRONT of block k's row passes (as with the side stream):
        // exact(k + 1), row passes(k), exact(k + 2), ... run one after the other at their un-contended speed and the host's read-backs of
        // block k fall into the shadow of a launch that is already queued -- the row passes beside an exact kernel wait for its
        // workgroups to leave the CUs one kernel after the other (a 49-us count took 659 us there)
        if (side) ps = lopt.stream_dense == 4 ? c->dl_stream : (lopt.stream_dense == 5 ? c->stream : c->post_stream);
        mark("setup", -1);
        if (!blocks.empty()) {
            rc = launch(0, dense);
            if (rc) return rc;
        }
        mark("launched", 0);
        for (size_t k = 0; k < blocks.size(); ++k) {
            BlockCsr blk;
            bool next_launched = false;
            if (side) {
                hipError_t e = hipEventRecord(c->cmp_done, c->stream);              // launch k is the last thing queued there
                if (e == hipSuccess) e = hipStreamWaitEvent(ps, c->cmp_done, 0);
                if (e != hipSuccess) return fail(MVS_E_HIP, "ordering the side stream: %s", hipGetErrorString(e));
                if (c->timing && c->ev_valid[1]) add_kernel_ms();                    // launch k's time, before its events are reused
                if (k + 1 < blocks.size() && !out.failed()) {
                    rc = launch(k + 1, true);
                    if (rc) return rc;
                    next_launched = true;
                    mark("launched", (long)k + 1);
                }
            }
            wait_for_set((int64_t)k);
            if (dense) {
                bool odd = false;
                rc = rows_of_dense_block(k, blk, &odd);
                if (rc == MVS_OK && odd) {
                    rc = fall_back_to_lists(k);       // `dense` is false from here on: the block is taken again below, as a list
                    blk = BlockCsr();
                    next_launched = false;            // (what the side stream's turn queued for block k + 1 is void)
                }
                if (rc) return rc;
            }
            const int64_t rb = blocks[k].first, re = blocks[k].second;
            if (!dense) {
                unsigned long long got = 0;
                rc = read_cell_count(&got);
                if (rc == MVS_OK && (int64_t)got > (re - rb) * s->n) rc = fail(MVS_E_HIP, "internal: more kept cells than cells");
                if (rc) return rc;
                add_kernel_ms();
                rc = csr_from_packed(c, rb, re, (int64_t)got, shift, col_bits, (int64_t)k, blk);
                if (rc) return rc;
            }
            total += blk.n;
            ++c->st.blocks;
            rc = prepare(blk);
            if (rc) return rc;
            if (dense && ecb && blk.encoded && re > rb) {
                spec_cells_per_row = std::max(spec_cells_per_row, (double)blk.n / (double)(re - rb));
                spec_bytes_per_row = std::max(spec_bytes_per_row, (double)blk.enc_off[(size_t)(re - rb)] / (double)(re - rb));
            }
            mark("enc", (long)k);
            if (!next_launched && k + 1 < blocks.size() && !out.failed()) {   // the next block computes while this one is fed to the link
                rc = launch(k + 1, dense);
                if (rc) return rc;
                mark("launched", (long)k + 1);
            }
            deliver(blk);
            mark("fed", (long)k);
            if (out.failed()) break;
        }
        return MVS_OK;
    }
};

int pairwise_stream_impl(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, int keep_mode,
                         int64_t row_begin, int64_t row_end, size_t device_budget_bytes, mvs_row_block_cb cb,
                         mvs_encoded_rows_cb ecb, void* user, int64_t* n_cells) {
    if (!c || !s || (!cb && !ecb)) return fail(MVS_E_INVALID, "NULL argument");
    const Range range(c, "mvs_pairwise_stream");
    if (n_cells) *n_cells = 0;
    if (!mem_ok(mem_norms) || (keep_mode != MVS_KEEP_INT32 && keep_mode != MVS_KEEP_INT16)) return fail(MVS_E_INVALID, "bad argument");
    if (row_begin < 0 || row_end > s->n || row_begin > row_end)
        return fail(MVS_E_INVALID, "row range [%lld,%lld) outside [0,%lld)", (long long)row_begin, (long long)row_end, (long long)s->n);
    if (row_begin == row_end || s->n == 0) return MVS_OK;
    if (!norms_sq) return fail(MVS_E_INVALID, "norms_sq is NULL");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf dn;
    const double* d_n2 = norms_sq;
    if (mem_norms == MVS_MEM_HOST) {
        HIP_TRY(dn.alloc((size_t)s->n * 8));
        HIP_TRY(hipMemcpyAsync(dn.p, norms_sq, (size_t)s->n * 8, hipMemcpyHostToDevice, c->stream));
        d_n2 = (const double*)dn.p;
    }
    // Device budget for the kept cells of one row block (raw + sorted words, CSR arrays: 21-22 bytes per cell).  Only a block
    // that goes through the exact kernel is planned against it (worst case: every cell kept); the two-stage comparison's
    // output is sized from its candidate count.  The dense byte matrix (one byte per cell of a row block) has a budget of
    // its own.  Both are what the caller says, or by default:
    size_t budget = device_budget_bytes, dense_budget = device_budget_bytes;
    if (device_budget_bytes == 0) {
        // a quarter of what is free, but no more than 2^30 worst-case cells per block (8 GiB of packed words): where the
        // exact kernel runs the result is dense and the link, not the kernel, sets the pace -- blocks of that size keep the
        // head of the pipeline (first block computed, nothing to download yet) short; the matrix may take a third
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<size_t>(free_b / 4, (size_t)22 << 30);
        dense_budget = free_b / 3;
    }
    int rc = ensure_download_side(c);
    if (rc) return rc;
    c->st.reset();
    StreamJob job(c, s, d_n2, keep_mode, row_begin, row_end, budget, dense_budget, cb, ecb, user, n_cells);
    job.start();
    rc = job.decide();
    if (rc == MVS_OK) rc = job.route == StreamJob::kList ? job.run_list() : job.run_blocks();
    return job.finish(rc);
}

// -------------------------------------------------------------------------------------------------
// a shard's sorted cell list -> the same pieces (mvs_cells_stream / mvs_cells_stream_encoded)
// -------------------------------------------------------------------------------------------------
int cells_stream_impl(mvs_ctx* c, const mvs_cell* cells, int64_t n, int64_t rb, int64_t re, mvs_row_block_cb cb, mvs_encoded_rows_cb ecb,
                      void* user, int64_t* n_delivered) {
    if (!c || (!cb && !ecb)) return fail(MVS_E_INVALID, "NULL argument");
    if (n_delivered) *n_delivered = 0;
    if (n < 0 || rb < 0 || re < rb || re >= (1LL << 31) || (n > 0 && !cells)) return fail(MVS_E_INVALID, "bad argument");
    if (re == rb) return MVS_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_download_side(c);
    if (rc) return rc;
    c->st.reset();
    const int64_t rows = re - rb;
    const size_t piece_bytes = (size_t)c->opt.stream_piece_mib << 20;
    BlockCsr blk;
    blk.rb = rb;
    blk.re = re;
    blk.set = 0;
    blk.row_ptr.assign((size_t)rows + 1, 0);
    // the arrays of set 0 may still be on their way out of an earlier call's last block: that call drained its download stream
    // before it returned (finish / below), so nothing is in flight here
    if (n > 0) {
        rc = ensure_buf(c, c->st_rowptr, (size_t)(rows + 1) * 8);
        if (rc == MVS_OK) rc = ensure_buf(c, c->st_counts, (size_t)(rows + 2) * 8);   // index into the list + the "wide q" flag
        if (rc == MVS_OK) rc = claim_csr_set(c, 0, 0, n, false, c->stream);
        if (rc) return rc;
        unsigned int* d_wide = reinterpret_cast<unsigned int*>((long long*)c->st_counts.p + rows + 1);
        HIP_TRY(hipMemsetAsync(d_wide, 0, 8, c->stream));
        mvs::launch_cells_rowptr(c->stream, cells, n, rb, rows, (long long*)c->st_counts.p);
        rc = check_kernel("k_cells_rowptr");
        if (rc) return rc;
        mvs::launch_cells_split(c->stream, cells, (const long long*)c->st_counts.p, rows, n, (long long*)c->st_rowptr.p, (int32_t*)c->st_col[0].p,
                                c->st_q[0].p, 1, d_wide);
        rc = check_kernel("k_cells_split");
        if (rc) return rc;
        unsigned int h_wide = 0;
        rc = read_back(c, c->stream, {{blk.row_ptr.data(), c->st_rowptr.p, (size_t)(rows + 1) * 8}, {&h_wide, d_wide, 4}});
        if (rc) return rc;
        blk.n = blk.row_ptr[(size_t)rows];
        if (blk.n < 0 || blk.n > n) return fail(MVS_E_INVALID, "the cell list is not ordered by row");
        if (h_wide) {                      // some q needs 16 bits (norms that do not belong to the vectors): the q array again
            blk.wide = true;
            rc = ensure_buf(c, c->st_q[0], (size_t)n * 2);
            if (rc) return rc;
            mvs::launch_cells_split(c->stream, cells, (const long long*)c->st_counts.p, rows, n, nullptr, (int32_t*)c->st_col[0].p,
                                    c->st_q[0].p, 2, nullptr);
            rc = check_kernel("k_cells_split(16-bit q)");
            if (rc) return rc;
        }
    }
    HIP_TRY(hipEventRecord(c->dl_ready[0], c->stream));
    c->st.blocks = 1;
    StreamOut out(c, cb, ecb, user);
    out.worker = std::thread([&out] { out.run(); });
    if (ecb) rc = encode_block(c, blk, c->stream);
    if (rc == MVS_OK) rc = feed(c, out, blk, piece_bytes, ecb != nullptr);
    out.close();
    (void)hipStreamSynchronize(c->dl_stream);
    if (rc) return rc;
    if (!out.error.empty()) return fail(MVS_E_HIP, "%s", out.error.c_str());
    if (out.cb_status != 0) return fail(MVS_E_ABORTED, "the row-block callback returned %d", out.cb_status);
    if (n_delivered) *n_delivered = blk.n;
    return MVS_OK;
}

// the host side keeps per-row directories in std::vector: no exception may cross the C boundary
template <class Call>
int no_throw(const char* entry, const char* streaming, Call call) {
    try {
        return call();
    } catch (const std::bad_alloc&) {
        return fail(MVS_E_NOMEM, "out of host memory while streaming %s", streaming);
    } catch (const std::exception& e) {
        return fail(MVS_E_HIP, "%s: %s", entry, e.what());
    }
}
}  // namespace mvs_capi

extern "C" {

int mvs_pairwise_stream(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, int keep_mode,
                        int64_t row_begin, int64_t row_end, size_t device_budget_bytes, mvs_row_block_cb cb, void* user,
                        int64_t* n_cells) {
    return no_throw("mvs_pairwise_stream", "the comparison result", [&] {
        return pairwise_stream_impl(c, s, norms_sq, mem_norms, keep_mode, row_begin, row_end, device_budget_bytes, cb, nullptr, user, n_cells);
    });
}

int mvs_pairwise_stream_encoded(mvs_ctx* c, const mvs_sketch_set* s, const double* norms_sq, int mem_norms, int keep_mode,
                                int64_t row_begin, int64_t row_end, size_t device_budget_bytes, mvs_encoded_rows_cb cb, void* user,
                                int64_t* n_cells) {
    return no_throw("mvs_pairwise_stream_encoded", "the comparison result", [&] {
        return pairwise_stream_impl(c, s, norms_sq, mem_norms, keep_mode, row_begin, row_end, device_budget_bytes, nullptr, cb, user, n_cells);
    });
}

int mvs_ctx_stream_stats(const mvs_ctx* c, double* kernel_ms, int64_t* bytes_out, int64_t* row_blocks, int64_t* pieces,
                         int* two_stage) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    if (kernel_ms) *kernel_ms = c->st.kernel_ms;
    if (bytes_out) *bytes_out = c->st.bytes;
    if (row_blocks) *row_blocks = c->st.blocks;
    if (pieces) *pieces = c->st.pieces;
    if (two_stage) *two_stage = (int)c->st.two_stage;
    return MVS_OK;
}

int mvs_ctx_stream_dense_stats(const mvs_ctx* c, int64_t* dense_blocks, int64_t* spec_blocks, int64_t* spec_redone,
                               int64_t* list_fallbacks) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    if (dense_blocks) *dense_blocks = c->st.dense_blocks;
    if (spec_blocks) *spec_blocks = c->st.spec_blocks;
    if (spec_redone) *spec_redone = c->st.spec_redone;
    if (list_fallbacks) *list_fallbacks = c->st.list_fallbacks;
    return MVS_OK;
}

int mvs_cells_stream(mvs_ctx* c, const mvs_cell* cells, int64_t n_cells, int64_t row_begin, int64_t row_end, mvs_row_block_cb cb,
                     void* user, int64_t* n_delivered) {
    return no_throw("mvs_cells_stream", "a shard's cells",
                    [&] { return cells_stream_impl(c, cells, n_cells, row_begin, row_end, cb, nullptr, user, n_delivered); });
}

int mvs_cells_stream_encoded(mvs_ctx* c, const mvs_cell* cells, int64_t n_cells, int64_t row_begin, int64_t row_end,
                             mvs_encoded_rows_cb cb, void* user, int64_t* n_delivered) {
    return no_throw("mvs_cells_stream_encoded", "a shard's cells",
                    [&] { return cells_stream_impl(c, cells, n_cells, row_begin, row_end, nullptr, cb, user, n_delivered); });
}

}  // extern "C"
