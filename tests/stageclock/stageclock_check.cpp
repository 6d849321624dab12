// stageclock_check.cpp — StageClock / StageMarks of mesh2splat_amd/csrc/m2s_stageclock.h against a malloc-backed stand-in for the event
// calls, built with the host compiler under AddressSanitizer + UBSan (tests/test_stageclock_cpu.py).  An event is a heap cell holding
// the sequence number of its last record; the elapsed time of two events is the difference.  Links no HIP runtime; exits non-zero at
// the first failure.
#include "../../mesh2splat_amd/csrc/m2s_stageclock.h"

#include <cstdio>
#include <cstdlib>
#include <set>

namespace {
std::set<long*> g_live;                  // every live event
long g_calls = 0, g_creates = 0, g_destroys = 0, g_records = 0, g_elapsed = 0, g_seq = 0;
int g_fail_create_at = -1;               // armed: the create with this number (counted from 0) fails

long* cell(hipEvent_t e) {
    long* p = reinterpret_cast<long*>(e);
    if (!g_live.count(p)) { std::fprintf(stderr, "an event that is not live (destroyed twice, or never created)\n"); std::exit(3); }
    return p;
}
}  // namespace

extern "C" {
hipError_t hipEventCreate(hipEvent_t* e) {
    ++g_calls;
    if (g_fail_create_at == g_creates++) { *e = nullptr; return hipErrorOutOfMemory; }
    long* p = static_cast<long*>(std::malloc(sizeof(long)));
    *p = -1;
    g_live.insert(p);
    *e = reinterpret_cast<hipEvent_t>(p);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { ++g_calls; ++g_destroys; long* p = cell(e); g_live.erase(p); std::free(p); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { ++g_calls; ++g_records; *cell(e) = ++g_seq; return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    ++g_calls; ++g_elapsed;
    if (*cell(a) < 0 || *cell(b) < 0) return hipErrorInvalidHandle;      // never recorded
    *ms = static_cast<float>(*cell(b) - *cell(a));
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

using namespace m2s_host;
enum class Mark { A, B, C, D, E, N };

int main() {
    std::string err;
    hipStream_t st = nullptr;
    float ms = -1.0f;
    {
        ClockOf<Mark> clock;
        // off: no call into the runtime at all, span writes 0
        CHECK(clock.begin(err, false) == M2S_OK && !clock.on());
        CHECK(clock.mark(Mark::A, st) == hipSuccess && clock.mark(Mark::B, st) == hipSuccess);
        CHECK(clock.marks(Mark::B).mark(1, st) == hipSuccess);
        CHECK(clock.span(Mark::A, Mark::B, &ms) == hipSuccess && ms == 0.0f);
        CHECK(g_calls == 0 && g_live.empty());
        // a default view is a no-op too
        CHECK(StageMarks().mark(0, st) == hipSuccess && StageMarks().mark(3, st) == hipSuccess && g_calls == 0);
        // on: the events are created by the first begin, once
        CHECK(clock.begin(err, true) == M2S_OK && clock.on() && g_creates == 5 && g_live.size() == 5 && g_records == 0);
        ms = -1.0f;
        CHECK(clock.span(Mark::A, Mark::B, &ms) == hipSuccess && ms == 0.0f && g_elapsed == 0);      // nothing recorded yet: 0, no call
        CHECK(clock.mark(Mark::A, st) == hipSuccess && clock.mark(Mark::B, st) == hipSuccess && clock.mark(Mark::D, st) == hipSuccess);
        CHECK(g_records == 3);
        CHECK(clock.span(Mark::A, Mark::B, &ms) == hipSuccess && ms == 1.0f);
        CHECK(clock.span(Mark::A, Mark::D, &ms) == hipSuccess && ms == 2.0f && g_elapsed == 2);
        ms = -1.0f;
        CHECK(clock.span(Mark::B, Mark::C, &ms) == hipSuccess && ms == 0.0f && g_elapsed == 2);      // C was never recorded
        // the next call: no new events; what the call before recorded does not count
        CHECK(clock.begin(err, true) == M2S_OK && g_creates == 5 && g_live.size() == 5);
        CHECK(clock.mark(Mark::A, st) == hipSuccess);
        ms = -1.0f;
        CHECK(clock.span(Mark::A, Mark::B, &ms) == hipSuccess && ms == 0.0f && g_elapsed == 2);      // B: recorded by the call before only
        CHECK(clock.span(Mark::B, Mark::D, &ms) == hipSuccess && ms == 0.0f && g_elapsed == 2);
        // a view with a base: its mark k is the clock's mark base + k; ints name marks as well as the enum does
        const StageMarks view = clock.marks(Mark::C);
        const long before = g_seq;
        CHECK(view.mark(0, st) == hipSuccess && view.mark(2, st) == hipSuccess && g_seq == before + 2);
        CHECK(clock.span(Mark::C, Mark::E, &ms) == hipSuccess && ms == 1.0f);
        CHECK(clock.span(2, 4, &ms) == hipSuccess && ms == 1.0f);
        CHECK(clock.span(Mark::A, Mark::E, &ms) == hipSuccess && ms == 2.0f);
        CHECK(clock.span(Mark::C, Mark::D, &ms) == hipSuccess && ms == 0.0f);                        // D: not in this call
        // off again: the events stay, nothing reaches the runtime, the marks of the call before are forgotten
        const long calls = g_calls;
        CHECK(clock.begin(err, false) == M2S_OK && !clock.on());
        CHECK(clock.mark(Mark::A, st) == hipSuccess && clock.marks().mark(1, st) == hipSuccess);
        ms = -1.0f;
        CHECK(clock.span(Mark::A, Mark::E, &ms) == hipSuccess && ms == 0.0f);
        CHECK(g_calls == calls && g_live.size() == 5);
        // ... and on once more: still the same five events
        CHECK(clock.begin(err, true) == M2S_OK && g_creates == 5);
        CHECK(clock.span(Mark::A, Mark::E, &ms) == hipSuccess && ms == 0.0f);
        CHECK(err.empty());
    }
    CHECK(g_destroys == 5 && g_live.empty());                                                         // every event freed, once
    {
        // a create that fails: reported, the clock stays off, the events made so far are kept for the next begin and freed at the end
        StageClock<3> clock;
        g_fail_create_at = g_creates + 1;
        CHECK(clock.begin(err, true) == M2S_ERR_OOM && !err.empty() && !clock.on() && g_live.size() == 1);
        const long calls = g_calls;
        CHECK(clock.mark(0, st) == hipSuccess && g_calls == calls);
        g_fail_create_at = -1;
        CHECK(clock.begin(err, true) == M2S_OK && clock.on() && g_live.size() == 3);
    }
    CHECK(g_live.empty() && g_destroys == 8);
    {
        StageClock<2> never;                                                                          // never opened: nothing to free
    }
    CHECK(g_destroys == 8);
    std::printf("stageclock_check ok: %ld runtime calls, %ld events\n", g_calls, g_creates);
    return 0;
}
