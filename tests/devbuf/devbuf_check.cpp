// devbuf_check.cpp — the owners of mesh2splat_amd/csrc/m2s_devbuf.h against a malloc-backed stand-in for the runtime, built with the host
// compiler under AddressSanitizer + UBSan (tests/test_devbuf_cpu.py).  Links no HIP runtime; exits non-zero at the first failure.
#include "../../mesh2splat_amd/csrc/m2s_devbuf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

namespace {
std::map<void*, size_t> g_live;          // every live "device" or pinned block and its size
long g_live_events = 0, g_live_streams = 0, g_frees = 0, g_last_error_reads = 0;
unsigned g_event_flags = 0;              // flags of the event created last
size_t g_fail_above = SIZE_MAX;          // armed: an allocation of more bytes than this fails (once) ...
int g_fail_skip = 0;                     // ... after this many such allocations have been let through

void arm(size_t above, int skip = 0) { g_fail_above = above; g_fail_skip = skip; }

hipError_t fake_alloc(void** p, size_t bytes) {
    if (bytes > g_fail_above && g_fail_skip-- == 0) {
        g_fail_above = SIZE_MAX;
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes);             // exactly what was asked for: ASan judges every access against it
    g_live[*p] = bytes;
    return hipSuccess;
}
hipError_t fake_free(void* p) {
    if (!p) return hipSuccess;
    if (!g_live.erase(p)) { std::fprintf(stderr, "free of a block that is not live (double free?)\n"); std::exit(3); }
    std::free(p);
    ++g_frees;
    return hipSuccess;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes); }
hipError_t hipFree(void* p) { return fake_free(p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return fake_alloc(p, bytes); }
hipError_t hipHostFree(void* p) { return fake_free(p); }
hipError_t hipEventCreate(hipEvent_t* e) { *e = static_cast<hipEvent_t>(std::malloc(1)); ++g_live_events; g_event_flags = hipEventDefault; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    *e = static_cast<hipEvent_t>(std::malloc(1));
    ++g_live_events;
    g_event_flags = flags;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { std::free(e); --g_live_events; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = static_cast<hipStream_t>(std::malloc(1)); ++g_live_streams; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { std::free(s); --g_live_streams; return hipSuccess; }
hipError_t hipGetLastError(void) { ++g_last_error_reads; return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

using namespace m2s_host;

static void fill(void* p, size_t bytes) { std::memset(p, 0xA5, bytes); }
static bool disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const char *x = static_cast<const char*>(a), *y = static_cast<const char*>(b);
    return x + na <= y || y + nb <= x;
}

static void check_devbuf() {
    std::string err;
    DevBuf<uint32_t> b;
    bool fresh = true;
    CHECK(b.get() == nullptr && b.cap() == 0);
    CHECK(b.reserve(err, 0, 4, &fresh) == M2S_OK && !fresh && b.get() == nullptr);      // nothing wanted, nothing allocated
    CHECK(b.reserve(err, 1, 1, &fresh) == M2S_OK && fresh && b.cap() == 1);             // one unit: at least 256 bytes
    fill(b.get(), 256);
    CHECK(g_live.at(b.get()) == 256);
    uint32_t* first = b;
    CHECK(b.reserve(err, 1, 1, &fresh) == M2S_OK && !fresh && b.get() == first);        // want <= cap: kept
    const long frees = g_frees;
    CHECK(b.reserve(err, 100, 4, &fresh) == M2S_OK && fresh && b.cap() == 100);         // larger: the old block goes, once
    CHECK(g_frees == frees + 1 && g_live.size() == 1 && g_live.at(b.get()) == 400);
    fill(b.get(), 400);
    uint32_t* second = b;
    CHECK(b.reserve(err, 37, 4, &fresh) == M2S_OK && !fresh && b.get() == second && b.cap() == 100);   // cap is what was asked for, never less
    CHECK(err.empty());
    arm(0);
    CHECK(b.reserve(err, 101, 4, &fresh) == M2S_ERR_OOM && !fresh);                     // failure: empty, reported, clean for the next call
    CHECK(!err.empty() && b.get() == nullptr && b.cap() == 0 && g_live.empty());
    CHECK(b.reserve(err, 5, 4, &fresh) == M2S_OK && fresh && b.cap() == 5 && b.get() != nullptr);
    fill(b.get(), 256);

    // the form whose failure is tolerated: false, nothing reported, the runtime's error read (cleared), the buffer empty
    DevBuf<char> plane;
    err.clear();
    CHECK(plane.try_reserve(10, 16) && plane.cap() == 10);
    fill(plane.get(), 256);
    char* kept = plane;
    CHECK(plane.try_reserve(7, 16) && plane.get() == kept);
    const long reads = g_last_error_reads;
    arm(0);
    CHECK(!plane.try_reserve(1000, 16));
    CHECK(err.empty() && g_last_error_reads == reads + 1 && plane.get() == nullptr && plane.cap() == 0);
    CHECK(plane.try_reserve(1000, 16) && plane.cap() == 1000);
    fill(plane.get(), 16000);

    PinnedBuf<unsigned long long> pin;
    CHECK(pin.ensure(err, 64) == M2S_OK);
    unsigned long long* h = pin;
    fill(h, 64);
    CHECK(pin.ensure(err, 64) == M2S_OK && static_cast<unsigned long long*>(pin) == h);
    EventSet<6> ev;
    CHECK(ev.ensure(err) == M2S_OK && g_live_events == 6);
    CHECK(ev.ensure(err) == M2S_OK && g_live_events == 6);
    hipEvent_t* e = ev;
    for (int i = 0; i < 6; ++i) CHECK(e[i] != nullptr);
    EventSet<2> never_used;
}

static void check_binwork() {
    std::string err;
    BinWork w;
    BinWork::Pairs p{}, q{};
    CHECK(w.reserve_items(err, 7, 48) == M2S_OK);
    CHECK(w.reserve_pairs(err, 5, &p) == M2S_OK);
    CHECK(w.reserve_temp(err, 1000) == M2S_OK && w.temp.cap() == 1000);
    CHECK(w.reserve_totals(err, 4, 32) == M2S_OK);
    fill(w.rec.get(), 7 * 48); fill(w.cnt.get(), 7 * 4); fill(w.off.get(), 7 * 8); fill(w.temp.get(), 1000); fill(w.d_totals.get(), 32);
    uint32_t* s[4] = { p.keys_in, p.vals_in, p.keys_out, p.vals_out };
    for (int i = 0; i < 4; ++i) {
        fill(s[i], 5 * 4);
        CHECK(s[i] == w.pairs.get() + 5 * i);
        for (int j = i + 1; j < 4; ++j) CHECK(disjoint(s[i], 5 * 4, s[j], 5 * 4));
    }
    CHECK(w.reserve_pairs(err, 3, &q) == M2S_OK);          // fewer pairs: the slices stay at the stride of the capacity
    CHECK(q.keys_in == p.keys_in && q.vals_in == p.keys_in + 5 && q.keys_out == p.keys_in + 10 && q.vals_out == p.keys_in + 15);
    CHECK(w.reserve_pairs(err, 9, &q) == M2S_OK && w.pairs.cap() == 9);
    CHECK(q.keys_in == w.pairs.get() && q.vals_in == q.keys_in + 9 && q.keys_out == q.keys_in + 18 && q.vals_out == q.keys_in + 27);
    fill(q.keys_in, 4 * 9 * 4);
    // the second of the three item allocations fails: whatever is live afterwards is the work set's own, released by the next
    // successful call or by the destructor
    arm(0, 1);
    CHECK(w.reserve_items(err, 100, 48) == M2S_ERR_OOM && !err.empty());
    size_t owned = 0;
    for (void* b : { w.rec.get(), static_cast<void*>(w.cnt.get()), static_cast<void*>(w.off.get()), static_cast<void*>(w.pairs.get()),
                     w.temp.get(), static_cast<void*>(w.d_totals.get()), static_cast<void*>(static_cast<unsigned long long*>(w.h_totals)) })
        if (b) { CHECK(g_live.count(b) == 1); ++owned; }
    CHECK(owned == g_live.size());
    CHECK(w.reserve_items(err, 100, 48) == M2S_OK && w.rec.cap() == 100 && w.cnt.cap() == 100 && w.off.cap() == 100);
    fill(w.rec.get(), 100 * 48); fill(w.cnt.get(), 100 * 4); fill(w.off.get(), 100 * 8);
    CHECK(g_live.size() == 7);
    {   // ... or by destruction, with the failure left standing
        BinWork dying;
        arm(0, 1);
        CHECK(dying.reserve_items(err, 3, 48) == M2S_ERR_OOM);
    }
    CHECK(g_live.size() == 7);
}

// the conversion side: events of a kind, streams, the record pool's fallback, a lane's work set through two scenes
static void check_conversion_owners() {
    std::string err;
    {
        EventSet<2> stage;
        EventSet<1> done;
        CHECK(stage.ensure(err, hipEventDisableTiming) == M2S_OK && g_live_events == 2 && g_event_flags == hipEventDisableTiming);
        CHECK(done.ensure(err, hipEventDisableTiming | hipEventBlockingSync) == M2S_OK && g_live_events == 3);
        CHECK(g_event_flags == (hipEventDisableTiming | hipEventBlockingSync));
        CHECK(stage.ensure(err) == M2S_OK && g_live_events == 3);                       // they exist: none created, whatever the flags
        EventSet<8> timing;
        CHECK(timing.ensure(err) == M2S_OK && g_live_events == 11 && g_event_flags == hipEventDefault);
    }
    CHECK(g_live_events == 0);                                                          // every event created was destroyed
    {
        StreamSet<2> st;
        CHECK(st[0] == nullptr && st[1] == nullptr);
        CHECK(st.ensure(err, 0) == M2S_OK && st[0] != nullptr && st[1] == nullptr && g_live_streams == 1);
        hipStream_t first = st[0];
        CHECK(st.ensure(err, 0) == M2S_OK && st[0] == first && g_live_streams == 1);
        CHECK(st.ensure(err, 1) == M2S_OK && st[1] != nullptr && st[1] != first && g_live_streams == 2);
    }
    CHECK(g_live_streams == 0);

    // the record pool (ensure_records): the doubled request is tried first and may fail, the one the caller needs is then reported
    const size_t rec = 96;
    DevBuf<void> pool;
    CHECK(pool.reserve(err, 10, rec) == M2S_OK);
    const long reads = g_last_error_reads;
    arm(0);                                                                             // the first allocation from here on fails
    CHECK(!pool.try_reserve(20, rec) && g_last_error_reads == reads + 1 && pool.get() == nullptr && pool.cap() == 0);
    CHECK(pool.reserve(err, 12, rec) == M2S_OK && pool.cap() == 12 && g_live.at(pool.get()) == 12 * rec && g_live.size() == 1);
    fill(pool.get(), 12 * rec);
    arm(0);
    CHECK(!pool.try_reserve(24, rec));
    arm(0);
    err.clear();
    CHECK(pool.reserve(err, 13, rec) == M2S_ERR_OOM && !err.empty() && pool.get() == nullptr && pool.cap() == 0 && g_live.empty());
    err.clear();

    // a lane: reserved, grown within a scene, released with the scene, reserved for the next one, destroyed
    {
        Lane ln;
        bool fresh = true;
        CHECK(ln.reserve_work(err, 16384, 1000, &fresh) == M2S_OK && fresh);            // the TriSetup block is new: its counter gets zeroed
        CHECK(ln.start.cap() == 16384 && ln.setup.cap() == 1000 && ln.total.cap() == 1 && g_live.size() == 3);
        fill(ln.start.get(), 16384 * 4); fill(ln.setup.get(), 1000); fill(ln.total.get(), 8);
        void* block = ln.setup.get();
        CHECK(ln.reserve_work(err, 100, 1000, &fresh) == M2S_OK && !fresh && ln.setup.get() == block && ln.start.cap() == 16384);
        long frees = g_frees;
        CHECK(ln.reserve_work(err, 40000, 1000, &fresh) == M2S_OK && !fresh);           // more slices: the table alone is replaced, once
        CHECK(g_frees == frees + 1 && ln.start.cap() == 40000 && ln.setup.get() == block && g_live.size() == 3);
        fill(ln.start.get(), 40000 * 4);
        CHECK(ln.chain_own.reserve(err, 7, 8, &fresh) == M2S_OK && fresh && ln.off_own.reserve(err, 9, 4) == M2S_OK);
        ln.chain = ln.chain_own; ln.off = ln.off_own;
        CHECK(g_live.size() == 5);
        // lane 0's release: what is sized by the scene goes, its slice starts and its counter stay
        frees = g_frees;
        ln.release_scene(false);
        CHECK(g_frees == frees + 3 && g_live.size() == 2 && ln.chain == nullptr && ln.off == nullptr && !ln.setup && ln.setup.cap() == 0);
        CHECK(ln.start.cap() == 40000 && ln.total.get() != nullptr);
        ln.release_scene(false);                                                        // again: nothing left to free
        CHECK(g_frees == frees + 3);
        CHECK(ln.reserve_work(err, 100, 500, &fresh) == M2S_OK && fresh && ln.setup.cap() == 500 && g_live.size() == 3);   // the next scene's block
        fill(ln.setup.get(), 500);
        // lane 1's release: everything but the record buffer
        CHECK(ln.records.reserve(err, 5, rec) == M2S_OK);
        frees = g_frees;
        ln.release_scene(true);
        CHECK(g_frees == frees + 3 && g_live.size() == 1 && ln.start.cap() == 0 && !ln.total && ln.records.cap() == 5);
        CHECK(ln.reserve_work(err, 16384, 700, &fresh) == M2S_OK && fresh && g_live.size() == 4);
        // a failure in the middle (the slice table) leaves what is live to the lane
        ln.release_scene(true);
        arm(0, 1);
        CHECK(ln.reserve_work(err, 16384, 700, &fresh) == M2S_ERR_OOM && !fresh && ln.total.get() != nullptr && !ln.start && !ln.setup);
        ln.release_scene(true);
        // (released, then destroyed: the destructors find nothing but the record buffer)
    }
    CHECK(g_live.empty());
}

int main() {
    check_devbuf();
    CHECK(g_live.empty() && g_live_events == 0);
    check_conversion_owners();
    CHECK(g_live.empty() && g_live_events == 0 && g_live_streams == 0);
    check_binwork();
    CHECK(g_live.empty() && g_live_events == 0);
    std::puts("devbuf_check ok");
    return 0;
}
