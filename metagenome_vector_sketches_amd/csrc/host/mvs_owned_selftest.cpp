// mvs_owned_selftest.cpp -- the owning types of ../mvs_owned.h against counting stand-ins for the runtime's calls: every
// resource created is released exactly once whatever the object went through, a moved-from object releases nothing, the
// grow-only rule asks for what it says and frees first, a refused allocation leaves an empty object, and members go in
// reverse order of declaration.  No device and no HIP library; `make asan` builds it again with the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

// ---- the stand-ins: a resource is a small heap block (so the sanitizers watch it too), a call is a line of the log ----
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
typedef struct FakeEvent* hipEvent_t;
typedef struct FakeStream* hipStream_t;
constexpr unsigned hipHostMallocDefault = 0, hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1;

struct Call {
    std::string what;
    void* handle;
    size_t arg;   // bytes or flags
};
static std::vector<Call> g_log;
static std::set<void*> g_live;
static bool g_refuse = false;   // the next creation fails
static int g_bad = 0;

static void check(bool ok, const char* what, int line) {
    if (!ok) {
        std::printf("FAILED line %d: %s\n", line, what);
        ++g_bad;
    }
}
#define CHECK(x) check((x), #x, __LINE__)

static hipError_t create(const char* what, void** out, size_t arg) {
    if (g_refuse) {
        g_refuse = false;
        *out = (void*)0x1;   // a runtime need not leave the output alone when it refuses
        g_log.push_back({std::string(what) + " refused", nullptr, arg});
        return hipErrorOutOfMemory;
    }
    *out = std::malloc(16);
    g_live.insert(*out);
    g_log.push_back({what, *out, arg});
    return hipSuccess;
}
static hipError_t release(const char* what, void* h) {
    check(g_live.erase(h) == 1, "released something live, once", __LINE__);
    g_log.push_back({what, h, 0});
    std::free(h);
    return hipSuccess;
}
static hipError_t hipMalloc(void** p, size_t n) { return create("malloc", p, n); }
static hipError_t hipFree(void* p) { return release("free", p); }
static hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return create("host_malloc", p, n); }
static hipError_t hipHostFree(void* p) { return release("host_free", p); }
static hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) { return create("event", (void**)e, flags); }
static hipError_t hipEventDestroy(hipEvent_t e) { return release("event_destroy", e); }
static hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { return create("stream", (void**)s, flags); }
static hipError_t hipStreamDestroy(hipStream_t s) { return release("stream_destroy", s); }

#define MVS_OWNED_NO_RUNTIME
#include "../mvs_owned.h"

using namespace mvs_capi;

static size_t count(const char* what) {
    size_t n = 0;
    for (const Call& c : g_log) n += c.what == what;
    return n;
}
static void fresh() {
    CHECK(g_live.empty());
    g_log.clear();
}

// construct, move-construct, move-assign onto a live object, reset(), destruction: `make` fills an object
template <typename T, typename Make>
static void lifetimes(const char* created, const char* released, Make make) {
    fresh();
    {
        T a, b, empty;
        make(a);
        make(b);
        T c(std::move(a));                    // a is empty now
        CHECK(count(released) == 0);
        b = std::move(c);                     // b's own resource goes, c is empty
        CHECK(count(released) == 1 && g_live.size() == 1);
        T& same = b;
        b = std::move(same);                  // (self-assignment keeps it)
        CHECK(count(released) == 1 && g_live.size() == 1);
        T d;
        make(d);
        d.reset();
        CHECK(count(released) == 2 && g_live.size() == 1);
        d.reset();                            // nothing left to release
        a.reset();
        CHECK(count(released) == 2);
        make(d);                              // an object is usable again after reset()
        make(d);                              // ... and creating over a live resource releases it first
        CHECK(count(created) == 5 && count(released) == 3 && g_log[g_log.size() - 2].what == released);
    }
    CHECK(count(created) == 5 && count(released) == 5);
    // a refused creation: empty, safe to destroy, safe to use again
    fresh();
    {
        T a;
        g_refuse = true;
        make(a);
        CHECK(g_live.empty());
        a.reset();
        make(a);
        CHECK(g_live.size() == 1);
        g_refuse = true;
        make(a);                              // what it held went before the refused call
        CHECK(g_live.empty());
    }
    CHECK(count(created) == 1 && count(released) == 1);
}

static void growth_rule() {
    fresh();
    {
        DevBuf b;
        CHECK(b.grow(1000) == hipSuccess && b.bytes == 1000 + 250 + 4096 && g_log.size() == 1 && g_log[0].arg == b.bytes);
        void* first = b.p;
        CHECK(b.grow(1000) == hipSuccess && b.grow(b.bytes) == hipSuccess && b.grow(0) == hipSuccess);
        CHECK(g_log.size() == 1 && b.p == first);                        // it held the request: no call at all
        CHECK(b.grow(b.bytes + 1) == hipSuccess && g_log.size() == 3);
        CHECK(g_log[1].what == "free" && g_log[1].handle == first);      // the old block goes before the new one is asked for
        CHECK(g_log[2].what == "malloc" && g_log[2].arg == DevBuf::grown(1000 + 250 + 4096 + 1) && b.bytes == g_log[2].arg);
        // the head room stops at 256 MiB
        const size_t big = (size_t)3 << 30;
        CHECK(DevBuf::grown(big) == big + ((size_t)256 << 20) + 4096 && DevBuf::grown(0) == 4096);
        CHECK(DevBuf::grown((size_t)1 << 30) == ((size_t)1 << 30) + ((size_t)256 << 20) + 4096);
        // a refused growth leaves it empty, and the next call starts over
        g_refuse = true;
        CHECK(b.grow(1 << 20) != hipSuccess && b.p == nullptr && b.bytes == 0 && g_live.empty());
        CHECK(b.grow(8) == hipSuccess && b.bytes == 8 + 2 + 4096);
        // alloc: exactly what was asked for, one byte for nothing
        CHECK(b.alloc(0) == hipSuccess && b.bytes == 1 && b.alloc(77) == hipSuccess && b.bytes == 77 && b.as<char>() == b.p);
        PinnedBuf h;
        CHECK(h.alloc(4096) == hipSuccess && h.bytes == 4096 && g_log.back().what == "host_malloc" && g_log.back().arg == 4096);
    }
    Event e;
    Stream s;
    CHECK(e.create(hipEventDisableTiming) == hipSuccess && g_log.back().arg == hipEventDisableTiming && (hipEvent_t)e == e.e);
    CHECK(e.create() == hipSuccess && g_log.back().arg == hipEventDefault);
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess && g_log.back().arg == hipStreamNonBlocking && (hipStream_t)s == s.s);
}

// members of each type: destroyed in reverse order of declaration, so a stream declared first outlives the buffers
struct Holder {
    Stream stream;
    Event event;
    DevBuf dev[2];
    PinnedBuf pinned;
};
static void member_order() {
    fresh();
    void* h[5];
    {
        Holder x;
        CHECK(x.stream.create(hipStreamNonBlocking) == hipSuccess && x.event.create() == hipSuccess && x.dev[0].alloc(8) == hipSuccess &&
              x.dev[1].alloc(8) == hipSuccess && x.pinned.alloc(8) == hipSuccess);
        h[0] = x.stream.s, h[1] = x.event.e, h[2] = x.dev[0].p, h[3] = x.dev[1].p, h[4] = x.pinned.p;
        g_log.clear();
    }
    CHECK(g_log.size() == 5);
    const char* want[5] = {"host_free", "free", "free", "event_destroy", "stream_destroy"};
    for (int i = 0; i < 5 && g_log.size() == 5; ++i) CHECK(g_log[i].what == want[i] && g_log[i].handle == h[4 - i]);
    // a holder on the heap that was only partly filled, as a failed *_create leaves it
    fresh();
    {
        Holder* y = new Holder();
        CHECK(y->dev[1].alloc(8) == hipSuccess);
        g_refuse = true;
        CHECK(y->pinned.alloc(8) != hipSuccess);
        delete y;
    }
    CHECK(count("free") == 1 && count("host_free") == 0);
}

int main() {
    lifetimes<DevBuf>("malloc", "free", [](DevBuf& b) { (void)b.alloc(64); });
    lifetimes<DevBuf>("malloc", "free", [](DevBuf& b) { (void)b.grow(b.bytes + 64); });
    lifetimes<PinnedBuf>("host_malloc", "host_free", [](PinnedBuf& b) { (void)b.alloc(64); });
    lifetimes<Event>("event", "event_destroy", [](Event& e) { (void)e.create(); });
    lifetimes<Stream>("stream", "stream_destroy", [](Stream& s) { (void)s.create(hipStreamNonBlocking); });
    growth_rule();
    member_order();
    fresh();
    if (g_bad) {
        std::printf("mvs_owned_selftest: %d checks FAILED\n", g_bad);
        return 1;
    }
    std::printf("mvs_owned_selftest: all checks passed\n");
    return 0;
}
