// mvs_capi.hip -- the C ABI of libmvs_hip.so (include/mvs_hip.h): contexts, options, buffer staging helpers shared by the
// other mvs_capi_*.hip units.  No compute happens on the host here and there is no CPU fallback.
#include "mvs_capi_internal.h"

using namespace mvs_capi;

namespace mvs {
int capi_fail(int code, const char* fmt, ...);
hipStream_t capi_stream(mvs_ctx* c) { return c->stream; }
int capi_device(mvs_ctx* c) { return c->device; }
const Options& capi_options(mvs_ctx* c) { return c->opt; }
}  // namespace mvs

namespace {
thread_local std::string g_err;
}  // namespace

std::atomic<unsigned long long> mvs_capi::g_set_ids{0};

int mvs_capi::fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int mvs::capi_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {

// rocprofv3 --marker-trace ranges around the ABI's main entry points (option `markers`, off by default).  The roctx
// library (librocprofiler-sdk-roctx / libroctx64) is bound at run time: without it the ranges are no-ops.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4",
                                 "libroctx64.so", "/opt/rocm/lib/librocprofiler-sdk-roctx.so"}) {
            if (void* h = dlopen(name, RTLD_NOW | RTLD_LOCAL)) {
                push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop) return;
                push = nullptr;
                pop = nullptr;
            }
        }
    }
};
const Roctx& roctx() {
    static const Roctx r;
    return r;
}

}  // namespace

namespace mvs_capi {

Range::Range(const mvs_ctx* c, const char* name) {
    if (c && c->opt.markers && roctx().push) {
        roctx().push(name);
        on = true;
    }
}
Range::~Range() {
    if (on) roctx().pop();
}

int ensure_buf(mvs_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes) return MVS_OK;
    if (b.p) HIP_TRY(hipStreamSynchronize(c->stream));
    if (b.grow(bytes) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %zu bytes failed", DevBuf::grown(bytes));
    return MVS_OK;
}

// Several small device -> host read-backs with ONE synchronisation: the copies land in a pinned buffer of the context (a copy
// into pageable memory is staged by the runtime and blocks the host once per copy), the stream is synchronised once, then
// the values are copied out.  Only the thread that drives the context's comparison calls this.
int ensure_read_back(mvs_ctx* c, size_t total) {
    if (c->rb_pinned.p && c->rb_pinned.bytes >= total) return MVS_OK;
    HIP_TRY(c->rb_pinned.alloc(std::max<size_t>(total * 2, (size_t)1 << 20)));
    return MVS_OK;
}
int read_back(mvs_ctx* c, hipStream_t st, std::initializer_list<ReadBack> items) {
    size_t total = 0;
    for (const ReadBack& it : items) total += (it.bytes + 63) & ~(size_t)63;
    const int rc_rb = ensure_read_back(c, total);
    if (rc_rb) return rc_rb;
    size_t at = 0;
    for (const ReadBack& it : items) {
        if (it.bytes) HIP_TRY(hipMemcpyAsync((char*)c->rb_pinned.p + at, it.src, it.bytes, hipMemcpyDeviceToHost, st));
        at += (it.bytes + 63) & ~(size_t)63;
    }
    HIP_TRY(hipStreamSynchronize(st));
    at = 0;
    for (const ReadBack& it : items) {
        if (it.bytes) memcpy(it.dst, (const char*)c->rb_pinned.p + at, it.bytes);
        at += (it.bytes + 63) & ~(size_t)63;
    }
    return MVS_OK;
}

int ensure_scratch(mvs_ctx* c, size_t bytes) {
    if (c->scratch.bytes >= bytes) return MVS_OK;
    if (c->scratch.p) HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(c->scratch.alloc(bytes));
    return MVS_OK;
}

// pinned host buffer whose previous upload has completed
int acquire_pinned(mvs_ctx* c, size_t bytes) {
    if (c->pinned_busy) {
        HIP_TRY(hipEventSynchronize(c->pinned_ev));
        c->pinned_busy = false;
    }
    if (c->pinned.bytes >= bytes) return MVS_OK;
    HIP_TRY(c->pinned.alloc(bytes < (1u << 20) ? (1u << 20) : bytes));
    return MVS_OK;
}

// ---- options: one table drives the environment defaults, the setter and the getter ----
struct OptionSpec {
    const char* name;      // mvs_ctx_set_option name; the environment variable is MVS_<NAME in upper case>
    int mvs::Options::*ifield;
    double mvs::Options::*dfield;
    long long lo, hi;
    bool no_env = false;   // the option has no environment default
};
const OptionSpec kOptions[] = {
    {"pairwise_filter", &mvs::Options::pairwise_filter, nullptr, 0, 2},
    {"filter_variant", &mvs::Options::filter_variant, nullptr, -1, 99},
    {"exact_variant", &mvs::Options::exact_variant, nullptr, 0, 3},
    {"pairwise_variant", &mvs::Options::pairwise_variant, nullptr, 0, 9},
    {"pairwise_symmetric", &mvs::Options::pairwise_symmetric, nullptr, 0, 1},
    {"pairwise_debug", &mvs::Options::pairwise_debug, nullptr, 0, 15},
    {"sort", &mvs::Options::sort, nullptr, 0, 2},
    {"enable_k3", &mvs::Options::enable_k3, nullptr, 0, 1},
    {"markers", &mvs::Options::markers, nullptr, 0, 1},
    {"project_variant", &mvs::Options::project_variant, nullptr, 0, 24},
    {"project_balance", &mvs::Options::project_balance, nullptr, 0, 1},
    {"comm_timeout_s", &mvs::Options::comm_timeout_s, nullptr, 1, 86400},
    {"pairwise_map", &mvs::Options::pairwise_map, nullptr, 0, 2},
    {"coarse_radix", &mvs::Options::coarse_radix, nullptr, 0, 1},
    {"cand_regions", &mvs::Options::cand_regions, nullptr, 0, 1},
    {"recheck_mode", &mvs::Options::recheck_mode, nullptr, 0, 3},
    {"recheck_blocks", &mvs::Options::recheck_blocks, nullptr, 1, 64},
    {"stream_dense", &mvs::Options::stream_dense, nullptr, 0, 5},
    {"encode_stage_words", &mvs::Options::encode_stage_words, nullptr, 1, 64},
    {"stream_block_rows", &mvs::Options::stream_block_rows, nullptr, 0, 1 << 30},
    {"tile_dense_thr", &mvs::Options::tile_dense_thr, nullptr, 0, 8192},
    {"stream_list_cells", &mvs::Options::stream_list_cells, nullptr, 0, 1 << 30},
    {"stream_pipeline", &mvs::Options::stream_pipeline, nullptr, 0, 1},
    {"stream_trace", &mvs::Options::stream_trace, nullptr, 0, 1},
    {"search_stream", &mvs::Options::search_stream, nullptr, 0, 1},
    {"search_depth", &mvs::Options::search_depth, nullptr, 3, 6},
    {"fragment_major", &mvs::Options::fragment_major, nullptr, 0, 1},
    {"pairwise_bdirect", &mvs::Options::pairwise_bdirect, nullptr, 0, 1},
    {"plan_strip_wgs", &mvs::Options::plan_strip_wgs, nullptr, 256, 1 << 22},
    {"recode_rows_wg", &mvs::Options::recode_rows_wg, nullptr, 8, 16},
    {"plan_speculate", &mvs::Options::plan_speculate, nullptr, 0, 1},
    {"plan_order", &mvs::Options::plan_order, nullptr, 0, 1},
    {"stream_piece_mib", &mvs::Options::stream_piece_mib, nullptr, 1, 1024},
    {"stream_spec", &mvs::Options::stream_spec, nullptr, 0, 1},
    {"stream_copy", &mvs::Options::stream_copy, nullptr, 0, 1},
    {"topk_dots", &mvs::Options::topk_dots, nullptr, 0, 1},
    {"topk_block_rows", &mvs::Options::topk_block_rows, nullptr, 0, 1 << 30},
    {"contain_dots", &mvs::Options::contain_dots, nullptr, 0, 1},
    {"contain_block_rows", &mvs::Options::contain_block_rows, nullptr, 0, 1 << 30},
    {"levels_dots", &mvs::Options::levels_dots, nullptr, 0, 1},
    {"levels_block_rows", &mvs::Options::levels_block_rows, nullptr, 0, 1 << 30},
    {"pcoa_dots", &mvs::Options::pcoa_dots, nullptr, 0, 1},
    {"pcoa_block_rows", &mvs::Options::pcoa_block_rows, nullptr, 0, 1 << 30},
    {"groups_dots", &mvs::Options::groups_dots, nullptr, 0, 1},
    {"groups_block_rows", &mvs::Options::groups_block_rows, nullptr, 0, 1 << 30},
    {"gram_slab_rows", &mvs::Options::gram_slab_rows, nullptr, 64, 65536},
    {"gram_variant", &mvs::Options::gram_variant, nullptr, 0, 1},
    {"cluster_cells", &mvs::Options::cluster_cells, nullptr, 0, 1 << 30},
    {"cluster_block_rows", &mvs::Options::cluster_block_rows, nullptr, 0, 1 << 30},
    {"intersect_unit", &mvs::Options::intersect_unit, nullptr, 64, 1 << 30},
    {"gather_batch", &mvs::Options::gather_batch, nullptr, 1, 1024},
    {"kmer_unit", &mvs::Options::kmer_unit, nullptr, 64, mvs::kKmerUnitMax},
    {"kmer_capacity", &mvs::Options::kmer_capacity, nullptr, 0, 1 << 30},
    {"abund_unit", &mvs::Options::abund_unit, nullptr, 64, 1 << 20, true},
    {"abund_big_segment", &mvs::Options::abund_big_segment, nullptr, 64, 1 << 30, true},
    {"pairwise_block_cells", nullptr, &mvs::Options::pairwise_block_cells, 1, (1LL << 62)},
};

// ... and the options that are fields of the context: host-side scheduling, blocking and path choices that never change a
// result.  No environment default; mvs_ctx_set_option / _get_option look here first.
struct CtxOptionSpec {
    const char* name;
    int mvs_ctx::*field;
    long long lo, hi;
};
const CtxOptionSpec kCtxOptions[] = {
    {"plan_overlap", &mvs_ctx::plan_overlap, 0, 1},
    {"core_block_rows", &mvs_ctx::core_block_rows, 0, 1 << 30},
    {"labels_dots", &mvs_ctx::labels_dots, 0, 1},
    {"labels_block_rows", &mvs_ctx::labels_block_rows, 0, 1 << 30},
    {"hclust_dots", &mvs_ctx::hclust_dots, 0, 1},
    {"hclust_block_rows", &mvs_ctx::hclust_block_rows, 0, 1 << 30},
    {"hclust_compact", &mvs_ctx::hclust_compact, 0, 2},
    {"community_path", &mvs_ctx::community_path, 0, 3},
    {"tsne_slice_cols", &mvs_ctx::tsne_slice_cols, 16, 1024},
    {"report_spin", &mvs_ctx::report_spin, 0, 1000000},
};

int apply_option(mvs::Options& o, const OptionSpec& sp, long long v) {
#ifndef MVS_ABLATIONS
    if (sp.ifield == &mvs::Options::pairwise_debug && v != 0)
        return fail(MVS_E_INVALID, "pairwise_debug needs a library built with -DMVS_ABLATIONS");
    if (sp.ifield == &mvs::Options::filter_variant && v >= 11 && v <= 33)
        return fail(MVS_E_INVALID, "filter_variant %lld is a k-loop ablation: needs -DMVS_ABLATIONS", v);
#endif
    if (v < sp.lo || v > sp.hi) return fail(MVS_E_INVALID, "option %s: %lld outside [%lld, %lld]", sp.name, v, sp.lo, sp.hi);
    if (sp.ifield) o.*(sp.ifield) = (int)v;
    else o.*(sp.dfield) = (double)v;
    return MVS_OK;
}

// MVS_<NAME> environment variables give the initial values (MVS_SORT also takes "merge" / "radix");
// values the setter would reject are ignored
void options_from_env(mvs::Options& o) {
    for (const OptionSpec& sp : kOptions) {
        if (sp.no_env) continue;
        std::string env = "MVS_";
        for (const char* p = sp.name; *p; ++p) env += (char)toupper((unsigned char)*p);
        const char* e = getenv(env.c_str());
        if (!e || !*e) continue;
        long long v;
        if (sp.ifield == &mvs::Options::sort && (e[0] == 'm' || e[0] == 'r')) v = e[0] == 'r' ? 2 : 1;
        else v = sp.dfield ? (long long)atof(e) : atoll(e);
        const std::string keep = g_err;
        if (apply_option(o, sp, v) != MVS_OK) g_err = keep;
    }
}

// Copy `bytes` from pageable host memory into pinned memory on several threads: one thread moves ~10 GB/s, the PCIe
// link 50+ GB/s, so a single memcpy would be what bounds the upload.
void parallel_copy(void* dst, const void* src, size_t bytes) {
    const size_t kMin = 8u << 20;
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 4 : (nt > 16 ? 16 : nt);
    if (bytes < 2 * kMin) nt = 1;
    if (nt <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> pool;
    const size_t per = (bytes / nt + 4095) & ~(size_t)4095;
    for (unsigned t = 0; t < nt; ++t) {
        const size_t b = (size_t)t * per;
        if (b >= bytes) break;
        const size_t n = std::min(per, bytes - b);
        pool.emplace_back([=]() { std::memcpy((char*)dst + b, (const char*)src + b, n); });
    }
    for (auto& th : pool) th.join();
}

int ensure_upload_pipeline(mvs_ctx* c) {
    if (c->up_done[1]) return MVS_OK;
    HIP_TRY(c->up_stream.create(hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(c->up_pinned[i].alloc(kUploadPiece));
        HIP_TRY(c->up_done[i].create(hipEventDisableTiming));
    }
    return MVS_OK;
}

int check_kernel(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MVS_E_HIP, "%s launch: %s", what, hipGetErrorString(e));
    return MVS_OK;
}

}  // namespace mvs_capi

mvs_ctx::~mvs_ctx() {
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
    plan_state_free(this);
}

extern "C" {

const char* mvs_version(void) { return "mvs_hip 0.1 (gfx950)"; }
const char* mvs_last_error(void) { return g_err.c_str(); }

int mvs_device_count(int* count) {
    if (!count) return fail(MVS_E_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(MVS_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return MVS_OK;
}

int mvs_ctx_create(int device, mvs_ctx** out) {
    if (!out) return fail(MVS_E_INVALID, "ctx out pointer is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(MVS_E_HIP, "no HIP device available (%s); libmvs_hip has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= n) return fail(MVS_E_INVALID, "device %d out of range [0,%d)", device, n);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MVS_E_HIP, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    mvs_ctx* c = new (std::nothrow) mvs_ctx();
    if (!c) return fail(MVS_E_NOMEM, "out of host memory");
    c->device = device;
    c->cu_count = prop.multiProcessorCount;
#ifdef MVS_ABLATIONS
    // The profiling build compiles the ping-pong kernels with extra code (time stamps, injected candidates), and with it
    // hipcc no longer keeps the fragment registers of the direct-B loop's hand-counted loads untouched: measured in round 5,
    // the ablation build's direct-B filter lost candidates at random (499 k +- 300 listed against 413 702, a few dozen kept
    // cells missing) while the shipped library -- which tools/check_isa.py gates -- is exact and deterministic.  So this build
    // runs both operands through LDS unless asked otherwise, and what it measures is the LDS-only kernel.
    c->opt.pairwise_bdirect = 0;
#endif
    options_from_env(c->opt);
    if (c->own_stream.create(hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(MVS_E_HIP, "hipStreamCreate failed");
    }
    c->stream = c->own_stream;
    bool events = true;
    for (Event& ev : c->ev) events = events && ev.create() == hipSuccess;
    if (!events || c->pinned_ev.create(hipEventDisableTiming) != hipSuccess) {
        delete c;
        return fail(MVS_E_HIP, "hipEventCreate failed");
    }
    // 8 counter slots; +256 B: the filter's stop flag; +1024 B: the re-check's eight round counters, 64 B apart
    if (c->d_counter.alloc(2048) != hipSuccess) {
        delete c;
        return fail(MVS_E_HIP, "hipMalloc failed");
    }
    *out = c;
    return MVS_OK;
}

int mvs_ctx_destroy(mvs_ctx* c) {
    if (!c) return MVS_OK;
    delete c;
    return MVS_OK;
}

int mvs_ctx_set_option(mvs_ctx* c, const char* name, int64_t value) {
    if (!c || !name) return fail(MVS_E_INVALID, "NULL argument");
    for (const CtxOptionSpec& sp : kCtxOptions)
        if (std::strcmp(sp.name, name) == 0) {
            if (value < sp.lo || value > sp.hi)
                return fail(MVS_E_INVALID, "option %s: %lld outside [%lld, %lld]", sp.name, (long long)value, sp.lo, sp.hi);
            c->*(sp.field) = (int)value;
            return MVS_OK;
        }
    for (const OptionSpec& sp : kOptions)
        if (std::strcmp(sp.name, name) == 0) return apply_option(c->opt, sp, (long long)value);
    return fail(MVS_E_INVALID, "unknown option '%s'", name);
}

int mvs_ctx_get_option(const mvs_ctx* c, const char* name, int64_t* value) {
    if (!c || !name || !value) return fail(MVS_E_INVALID, "NULL argument");
    for (const CtxOptionSpec& sp : kCtxOptions)
        if (std::strcmp(sp.name, name) == 0) {
            *value = c->*(sp.field);
            return MVS_OK;
        }
    for (const OptionSpec& sp : kOptions)
        if (std::strcmp(sp.name, name) == 0) {
            *value = sp.ifield ? (int64_t)(c->opt.*(sp.ifield)) : (int64_t)(c->opt.*(sp.dfield));
            return MVS_OK;
        }
    return fail(MVS_E_INVALID, "unknown option '%s'", name);
}

int mvs_ctx_set_stream(mvs_ctx* c, void* hip_stream) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    c->stream = (hipStream_t)hip_stream;
    return MVS_OK;
}

int mvs_ctx_use_own_stream(mvs_ctx* c) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    c->stream = c->own_stream;
    return MVS_OK;
}

int mvs_ctx_synchronize(mvs_ctx* c) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_ctx_set_timing(mvs_ctx* c, int enabled) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    c->timing = enabled != 0;
    for (bool& v : c->ev_valid) v = false;
    return MVS_OK;
}

int mvs_ctx_pairwise_candidates(mvs_ctx* c, int64_t* candidates) {
    if (!c || !candidates) return fail(MVS_E_INVALID, "NULL argument");
    *candidates = (int64_t)c->last_candidates;
    return MVS_OK;
}

int mvs_ctx_pairwise_stats(mvs_ctx* c, int64_t* candidates, int64_t* flagged_tiles, int64_t* filter_tiles) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    if (candidates) *candidates = (int64_t)c->last_candidates;
    if (flagged_tiles) *flagged_tiles = (int64_t)c->last_flagged_tiles;
    if (filter_tiles) *filter_tiles = (int64_t)c->last_filter_tiles;
    return MVS_OK;
}

int mvs_ctx_kernel_ms(mvs_ctx* c, int which, float* ms) {
    if (!c || !ms || which < 0 || which > 4) return fail(MVS_E_INVALID, "bad argument");
    if (!c->ev_valid[which]) return fail(MVS_E_INVALID, "no timing recorded for kernel %d", which);
    // pairs 2, 3 and 4 share events with pair 1: filter = ev[2]..ev[5], re-check (with the gather / tile list / prune
    // passes in front of it) = ev[5]..ev[7], exact kernel on the flagged tiles (the last such launch) = ev[6]..ev[3]
    hipEvent_t b = which == 2 ? c->ev[2] : which == 3 ? c->ev[5] : which == 4 ? c->ev[6] : c->ev[2 * which];
    hipEvent_t e = which == 2 ? c->ev[5] : which == 3 ? c->ev[7] : which == 4 ? c->ev[3] : c->ev[2 * which + 1];
    HIP_TRY(hipEventSynchronize(e));
    HIP_TRY(hipEventElapsedTime(ms, b, e));
    return MVS_OK;
}


// -------------------------------------------------------------------------------------------------
// device memory and events for hosts above the ABI (csrc/host/mvs_step.hpp)
// -------------------------------------------------------------------------------------------------
struct mvs_event {
    int device = 0;
    Event ev;
    bool timing = false, recorded = false;
};

int mvs_device_alloc(mvs_ctx* c, size_t bytes, int zero, void** ptr) {
    if (!c || !ptr) return fail(MVS_E_INVALID, "NULL argument");
    *ptr = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf b;
    if (b.alloc(bytes) != hipSuccess) return fail(MVS_E_NOMEM, "hipMalloc of %zu bytes failed", bytes);
    if (zero && bytes) {
        const hipError_t e = hipMemsetAsync(b.p, 0, bytes, c->stream);
        if (e != hipSuccess) return fail(MVS_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    *ptr = std::exchange(b.p, nullptr);   // the caller's from here on (mvs_device_free)
    return MVS_OK;
}

int mvs_device_free(mvs_ctx* c, void* ptr) {
    if (!c) return fail(MVS_E_INVALID, "ctx is NULL");
    if (!ptr) return MVS_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(ptr));
    return MVS_OK;
}

int mvs_device_zero(mvs_ctx* c, void* ptr, size_t bytes) {
    if (!c || (!ptr && bytes)) return fail(MVS_E_INVALID, "NULL argument");
    if (bytes == 0) return MVS_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(ptr, 0, bytes, c->stream));
    return MVS_OK;
}

int mvs_device_copy(mvs_ctx* c, void* dst, int mem_dst, const void* src, int mem_src, size_t bytes) {
    if (!c || !mem_ok(mem_dst) || !mem_ok(mem_src)) return fail(MVS_E_INVALID, "bad argument");
    if (bytes == 0) return MVS_OK;
    if (!dst || !src) return fail(MVS_E_INVALID, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    if (mem_dst == MVS_MEM_HOST && mem_src == MVS_MEM_HOST) {
        memcpy(dst, src, bytes);
        return MVS_OK;
    }
    const hipMemcpyKind kind = mem_dst == MVS_MEM_DEVICE ? (mem_src == MVS_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)
                                                         : hipMemcpyDeviceToHost;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    if (kind != hipMemcpyDeviceToDevice) HIP_TRY(hipStreamSynchronize(c->stream));
    return MVS_OK;
}

int mvs_event_create(mvs_ctx* c, int timing, mvs_event** out) {
    if (!c || !out) return fail(MVS_E_INVALID, "NULL argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    mvs_event* e = new (std::nothrow) mvs_event();
    if (!e) return fail(MVS_E_NOMEM, "out of host memory");
    e->device = c->device;
    e->timing = timing != 0;
    const hipError_t rc = e->ev.create(timing ? hipEventDefault : hipEventDisableTiming);
    if (rc != hipSuccess) {
        delete e;
        return fail(MVS_E_HIP, "hipEventCreate: %s", hipGetErrorString(rc));
    }
    *out = e;
    return MVS_OK;
}

int mvs_event_record(mvs_ctx* c, mvs_event* e) {
    if (!c || !e) return fail(MVS_E_INVALID, "NULL argument");
    if (c->device != e->device) return fail(MVS_E_INVALID, "the event belongs to device %d, the context to device %d", e->device, c->device);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(e->ev, c->stream));
    e->recorded = true;
    return MVS_OK;
}

int mvs_ctx_wait_event(mvs_ctx* c, mvs_event* e) {
    if (!c || !e) return fail(MVS_E_INVALID, "NULL argument");
    if (!e->recorded) return MVS_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamWaitEvent(c->stream, e->ev, 0));
    return MVS_OK;
}

int mvs_event_synchronize(mvs_event* e) {
    if (!e) return fail(MVS_E_INVALID, "event is NULL");
    if (!e->recorded) return MVS_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventSynchronize(e->ev));
    return MVS_OK;
}

int mvs_event_elapsed_ms(mvs_event* b, mvs_event* e, float* ms) {
    if (!b || !e || !ms) return fail(MVS_E_INVALID, "NULL argument");
    *ms = 0.0f;
    if (!b->timing || !e->timing || !b->recorded || !e->recorded) return fail(MVS_E_INVALID, "both events must have been created with timing and recorded");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventSynchronize(e->ev));
    HIP_TRY(hipEventElapsedTime(ms, b->ev, e->ev));
    return MVS_OK;
}

int mvs_event_destroy(mvs_event* e) {
    if (!e) return MVS_OK;
    (void)hipSetDevice(e->device);
    delete e;
    return MVS_OK;
}

}  // extern "C"
