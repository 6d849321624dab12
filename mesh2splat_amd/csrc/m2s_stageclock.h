// m2s_stageclock.h — stage timing: one clock per pass.  A clock owns the N timing events of a pass ("marks", named by the enums at
// the end of this file) and remembers which of them the current call has recorded, so that a span over a mark this call never reached is
// 0 and never the time between two events of earlier calls (hipEventElapsedTime over stale events does not fail: it answers).
//   begin(err, on)   opens one call's measurement: forgets the marks; on == false makes every mark() until the next begin() a no-op.
//                    The policy of a pass is what it passes for `on`: c->profiling for most, true for the passes that always measure.
//   mark(k, st)      records event k on st.
//   span(a, b, &ms)  after the stream has been synchronised: the time from mark a to mark b of THIS call; 0 where either is missing.
//   marks(base)      the view a launcher in a .hip file takes (StageMarks): its mark(k) is the clock's mark(base + k).
// The events are created by the first begin(err, true): a context that never profiles a pass creates none for it; with the clock off
// no call reaches the runtime.
// Self-contained like m2s_devbuf.h (the runtime's API header, the standard library, m2s.h): a plain host compiler builds
// tests/stageclock against it.
#pragma once
#include "../../include/m2s.h"

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>

namespace m2s_host {

// What a launcher records its stages through.  Default-constructed: off, mark() does nothing.
struct StageMarks {
    hipEvent_t* ev = nullptr;
    uint32_t* recorded = nullptr;
    int base = 0;
    hipError_t mark(int k, hipStream_t st) const {
        if (!ev) return hipSuccess;
        const hipError_t e = hipEventRecord(ev[base + k], st);
        if (e == hipSuccess) *recorded |= 1u << (base + k);
        return e;
    }
};

template <int N>
class StageClock {
    static_assert(N >= 2 && N <= 32, "the recorded marks are one bit each of a 32-bit word");

public:
    StageClock() = default;
    StageClock(const StageClock&) = delete;
    StageClock& operator=(const StageClock&) = delete;
    ~StageClock() { for (hipEvent_t e : ev_) if (e) (void)hipEventDestroy(e); }

    m2s_status begin(std::string& err, bool on) {
        recorded_ = 0;
        on_ = false;
        if (!on) return M2S_OK;
        for (hipEvent_t& e : ev_)
            if (!e) {
                const hipError_t r = hipEventCreate(&e);
                if (r != hipSuccess) {
                    err = std::string("hipEventCreate: ") + hipGetErrorString(r);
                    return r == hipErrorOutOfMemory ? M2S_ERR_OOM : M2S_ERR_HIP;
                }
            }
        on_ = true;
        return M2S_OK;
    }
    bool on() const { return on_; }
    // (K: an int or the pass's enum of marks)
    template <class K = int> StageMarks marks(K base = K()) { return on_ ? StageMarks{ ev_, &recorded_, static_cast<int>(base) } : StageMarks{}; }
    template <class K> hipError_t mark(K k, hipStream_t st) { return marks().mark(static_cast<int>(k), st); }
    template <class K> hipError_t span(K from, K to, float* ms) const {
        const int a = static_cast<int>(from), b = static_cast<int>(to);
        *ms = 0.0f;
        if (!on_ || !(recorded_ >> a & 1u) || !(recorded_ >> b & 1u)) return hipSuccess;
        return hipEventElapsedTime(ms, ev_[a], ev_[b]);
    }

private:
    hipEvent_t ev_[N] = {};
    uint32_t recorded_ = 0;
    bool on_ = false;
};

// The marks of every pass's clock (the members of m2s_ctx), in the order a call records them.  A clock of one span: SpanMark.
enum class SpanMark { Begin, End, N };
enum class ConvMark { Count, Counted, Emit, Emitted, Fused, FusedEnd, N };          // multi-pass: 0-1, 2-3 | second stage: 2-3 | single pass: 4-5
enum class SortMark { Start, Keyed, Sorted, Gathered, Prepassed, N };               // Gathered: m2s_sort_by_depth's end, m2s_prepass_sorted's prepass start
enum class BinMark { Setup, SetupEnd, Pairs, Paired, Grouped, Blended, N };         // splat_bin: 0-4 | its caller's blend: 5
enum class BudgetMark { Start, Selected, Scanned, Compact, Compacted, N };          // (the round trip between Scanned and Compact is in no stage)
enum class MergeMark { Start, Keyed, Sorted, Segments, Segmented, Reduced, N };
enum class LodCutMark { Start, Swept, Indexed, Compacted, N };
enum class LodBudgetMark { Start, Thresholds, Searched, N };
enum class LodBlendMark { Start, Weighted, Blended, ShBlended, N };
enum class ShadowMark { Count, Counted, Emit, Emitted, Setup, SetupEnd, Bin, Binned, Rastered, N };   // stage A: 0-3 | stage B: 4-8
enum class MeshMark { Start, SetupEnd, Deferred, Binned, Rastered, N };
enum class CompactMark { Start, Keyed, Sorted, Pack, Packed, N };
template <class E> using ClockOf = StageClock<static_cast<int>(E::N)>;

}  // namespace m2s_host
