// m2s_devbuf.h — owners of what the context keeps between calls: grow-only device buffers, pinned host blocks, events, streams, the
// work set of a binned rasteriser (viewer passes) and what a lane of conversions works in.  Each releases in its destructor (the context
// is deleted after its streams have been synchronised), so a member of m2s_ctx cannot be forgotten in m2s_destroy, a failed m2s_create
// leaks nothing and a capacity cannot outlive its pointer.
// Self-contained on purpose (the runtime's API header, the standard library, m2s.h): a plain host compiler builds tests/devbuf against it.
#pragma once
#include "../../include/m2s.h"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>

namespace m2s_host {

inline m2s_status hip_status(std::string& err, const char* what, hipError_t e) {
    if (e == hipSuccess) return M2S_OK;
    err = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? M2S_ERR_OOM : M2S_ERR_HIP;
}

// A grow-only device buffer with its capacity in units the caller chooses (records, pixels, bytes, ...).
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    uint64_t cap() const { return cap_; }      // the count last asked for, never rounded: callers slice by it
    void release() {
        if (p_) (void)hipFree((void*)p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Trade places with another buffer: how a caller grows one whose contents it has copied over (LodTree::reserve, m2s_lodtree.h).
    void swap(DevBuf& o) {
        T* const p = p_; p_ = o.p_; o.p_ = p;
        const uint64_t c = cap_; cap_ = o.cap_; o.cap_ = c;
    }
    // Room for `want` units of `unit` bytes: kept when large enough, else freed and allocated anew (contents lost; at least 256 bytes).
    // *fresh: this call allocated.  On failure the buffer is empty, so the next call starts clean.
    m2s_status reserve(std::string& err, uint64_t want, size_t unit, bool* fresh = nullptr) {
        if (fresh) *fresh = false;
        if (cap_ >= want) return M2S_OK;
        const hipError_t e = allocate(want, unit);
        if (fresh) *fresh = e == hipSuccess;
        return hip_status(err, "hipMalloc (grow-only buffer)", e);
    }
    // The same for a buffer the caller can do without: false (and nothing reported, the runtime's sticky error cleared) when there is no room.
    bool try_reserve(uint64_t want, size_t unit) {
        if (cap_ >= want) return true;
        if (allocate(want, unit) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    }

private:
    hipError_t allocate(uint64_t want, size_t unit) {
        release();
        void* q = nullptr;
        const size_t bytes = (size_t)want * unit;
        const hipError_t e = hipMalloc(&q, bytes < 256 ? 256 : bytes);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(q);
        cap_ = want;
        return hipSuccess;
    }
    T* p_ = nullptr;
    uint64_t cap_ = 0;
};

// A pinned host block of a fixed size, allocated at its first use.
template <typename T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p_) (void)hipHostFree((void*)p_); }
    operator T*() const { return p_; }
    m2s_status ensure(std::string& err, size_t bytes) {
        if (p_) return M2S_OK;
        return hip_status(err, "hipHostMalloc", hipHostMalloc((void**)&p_, bytes, hipHostMallocDefault));
    }

private:
    T* p_ = nullptr;
};

// N events of one kind (timing events, or with the flags of hipEventCreateWithFlags), created by the first ensure().
template <int N>
class EventSet {
public:
    EventSet() = default;
    EventSet(const EventSet&) = delete;
    EventSet& operator=(const EventSet&) = delete;
    ~EventSet() { for (hipEvent_t e : ev_) if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t*() { return ev_; }
    m2s_status ensure(std::string& err) {
        for (hipEvent_t& e : ev_)
            if (!e) if (m2s_status s = hip_status(err, "hipEventCreate", hipEventCreate(&e))) return s;
        return M2S_OK;
    }
    m2s_status ensure(std::string& err, unsigned flags) {
        for (hipEvent_t& e : ev_)
            if (!e) if (m2s_status s = hip_status(err, "hipEventCreate", hipEventCreateWithFlags(&e, flags))) return s;
        return M2S_OK;
    }

private:
    hipEvent_t ev_[N] = {};
};

// N non-blocking streams, each created by its first ensure().  Declared in front of the buffers and events whose work runs on them, so
// that it is destroyed after them.
template <int N>
class StreamSet {
public:
    StreamSet() = default;
    StreamSet(const StreamSet&) = delete;
    StreamSet& operator=(const StreamSet&) = delete;
    ~StreamSet() { for (hipStream_t s : st_) if (s) (void)hipStreamDestroy(s); }
    hipStream_t operator[](int k) const { return st_[k]; }
    m2s_status ensure(std::string& err, int k) {
        if (st_[k]) return M2S_OK;
        return hip_status(err, "hipStreamCreate", hipStreamCreateWithFlags(&st_[k], hipStreamNonBlocking));
    }

private:
    hipStream_t st_[N] = {};
};

// What a binned rasteriser (splat pass, shadow stage B, mesh depth / visibility) keeps between calls: per item a record, a tile count
// and the exclusive scan of the counts; the (tile, item) pairs before and after their sort; the scan / sort work area; the pass's
// counters on the device and their pinned copy.
struct BinWork {
    DevBuf<void> rec;
    DevBuf<uint32_t> cnt;
    DevBuf<unsigned long long> off;
    DevBuf<uint32_t> pairs;                 // keys_in | vals_in | keys_out | vals_out, pairs.cap() words each
    DevBuf<void> temp;                      // temp.cap(): the bytes last asked for
    DevBuf<unsigned long long> d_totals;
    PinnedBuf<unsigned long long> h_totals;
    struct Pairs { uint32_t *keys_in, *vals_in, *keys_out, *vals_out; };

    m2s_status reserve_items(std::string& err, uint64_t n, size_t rec_bytes) {
        if (m2s_status s = rec.reserve(err, n, rec_bytes)) return s;
        if (m2s_status s = cnt.reserve(err, n, sizeof(uint32_t))) return s;
        return off.reserve(err, n, sizeof(unsigned long long));
    }
    m2s_status reserve_pairs(std::string& err, uint64_t n, Pairs* out) {
        if (m2s_status s = pairs.reserve(err, n, 4 * sizeof(uint32_t))) return s;
        const uint64_t pc = pairs.cap();
        *out = Pairs{ pairs.get(), pairs.get() + pc, pairs.get() + 2 * pc, pairs.get() + 3 * pc };
        return M2S_OK;
    }
    m2s_status reserve_temp(std::string& err, uint64_t bytes) { return temp.reserve(err, bytes, 1); }
    m2s_status reserve_totals(std::string& err, size_t device_words, size_t pinned_bytes) {
        if (m2s_status s = h_totals.ensure(err, pinned_bytes)) return s;
        return d_totals.reserve(err, device_words, sizeof(unsigned long long));
    }
};

// What one lane of conversions works in: the stream its kernels run on, the look-back chain they publish to, the record buffer they
// write, and the work set of the multi-pass pipeline.  Owners, and the pointers as the kernels take them: lane 0's chain and offsets
// live inside the scene arena (the upload makes one allocation for them and everything else), lane 1 owns its pair.
struct Lane {
    hipStream_t stream = nullptr;            // (the context's StreamSet owns it)
    unsigned long long* chain = nullptr;     // one word per wave
    uint32_t* off = nullptr;                 // multi-pass: where every triangle's output starts, and the total
    DevBuf<unsigned long long> chain_own;    // behind chain / off where the lane owns them
    DevBuf<uint32_t> off_own;
    DevBuf<void> records;                    // context-owned record buffer; capacity in records
    uint32_t rec_R = 0;                      // R of the newest conversion enqueued into it ...
    uint32_t rec_gen = 0;                    // ... and a generation that advances whenever that R changes or the buffer is replaced
    DevBuf<uint32_t> start;                  // multi-pass: slice starts
    DevBuf<void> setup;                      // ... per-triangle TriSetup records, then the tall-triangle table; capacity in bytes
    DevBuf<unsigned long long> total;        // ... the fragment counter

    // The multi-pass work set for n_start slices of a scene whose TriSetup block takes setup_bytes.  *setup_fresh: the block was
    // allocated by this call (its slot counter has to be zeroed).  The caller lets the readers of an old slice table finish first.
    m2s_status reserve_work(std::string& err, uint64_t n_start, size_t setup_bytes, bool* setup_fresh) {
        *setup_fresh = false;
        if (m2s_status s = total.reserve(err, 1, sizeof(unsigned long long))) return s;
        if (m2s_status s = start.reserve(err, n_start, sizeof(uint32_t))) return s;
        return setup.reserve(err, setup_bytes, 1, setup_fresh);
    }
    // What is sized by the scene goes with it (released, not kept: the TriSetup block's layout depends on the triangle count); with
    // `all` (lane 1) the slice starts and the counter as well.
    void release_scene(bool all) {
        if (all) { start.release(); total.release(); }
        chain_own.release(); off_own.release(); setup.release();
        chain = nullptr; off = nullptr;
    }
};

}  // namespace m2s_host
