// m2s_async.cpp — m2s_convert_submit / m2s_convert_wait: a ring of result slots so that consecutive conversions run back to
// back (the reference blocks in glFinish once per conversion, ConversionPass.cpp:54).
#include "m2s_ctx.h"

#include <algorithm>
#include <cstring>

using namespace m2s;
using namespace m2s_host;

extern "C" {

// ---- asynchronous submissions --------------------------------------------------------------------------
m2s_status m2s_convert_submit(m2s_ctx* c, uint32_t R, void* d_records, uint64_t capacity_records, void* hip_stream) {
    if (!c) return M2S_ERR_INVALID;
    if (!d_records && capacity_records) return fail(c, M2S_ERR_INVALID, "d_records is NULL");
    if (c->slot_count == M2S_MAX_IN_FLIGHT) return fail(c, M2S_ERR_STATE, "M2S_MAX_IN_FLIGHT conversions already in flight");
    if (!c->has_scene) return fail(c, M2S_ERR_STATE, "m2s_upload_scene has not been called");
    if (R == 0 || R > 4096) return fail(c, M2S_ERR_INVALID, "R must be in [1, 4096]");
    const uint32_t k = (c->slot_head + c->slot_count) % M2S_MAX_IN_FLIGHT;
    m2s_ctx::Slot& sl = c->slot[k];
    const uint64_t cap = resolve_cap(c, R);
    m2s_ctx::RInfo& ri = rinfo_for(c, R);
    const m2s_host::Lane& l0 = c->lane[0];
    uint64_t limit = d_records ? (cap ? std::min(cap, capacity_records) : capacity_records) : cap ? cap : l0.records.cap();
    if (limit > 0xFFFFFFFFull) limit = 0xFFFFFFFFull;
    const uint32_t n_start = emit2_slices(limit);
    // Fast path, enqueued without waiting: this scene at this R already converted cleanly with the single kernel (no deferred
    // triangles, so no host decision between kernels), or with the multi-pass pipeline, which has no host decision between its
    // kernels either (work buffers sized; under AUTO and MULTIPASS — a forced single-pass setting that fell back to it converts
    // synchronously; with kernel timing on it runs synchronously: the per-kernel events are shared); and the output buffer needs no
    // (re)allocation.
    const bool mp = ri.form == M2S_PIPELINE_MULTIPASS;
    const bool own_ready = d_records || (l0.records && l0.rec_R == R && (cap ? l0.records.cap() >= cap : true));
    const bool fast = c->scene.n_tri > 0 && own_ready &&
                      (mp ? ri.mp_ready && !c->profiling && (c->pipeline == M2S_PIPELINE_AUTO || c->pipeline == M2S_PIPELINE_MULTIPASS) &&
                                l0.start.cap() >= n_start && l0.setup
                          : ri.async_ok);
    sl.R = R;
    sl.wrote_bands = false;
    if (!fast) {
        // first conversion of a (scene, R), or one that needs the second stage / the multi-pass pipeline: run it now
        // (run_pass first lets everything in flight finish: it may re-allocate the record pool and reuses the work buffers)
        uint64_t total = 0;
        M2S_TRY(run_pass(c, R, d_records, capacity_records, d_records ? (hipStream_t)hip_stream : c->stream, &total, true));
        sl.sync_result = true;
        sl.shared_work = false;
        sl.sync_total = total;
        memcpy(sl.ms, c->last_ms, sizeof sl.ms);   // a later submit overwrites last_ms before this slot is waited for
        sl.limit = c->last_stored;   // already clamped
        sl.d_out = const_cast<void*>(c->last_records);
        sl.own_lane = d_records ? -1 : 0;
        sl.gen = l0.rec_gen;
        ++c->slot_count;
        return M2S_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    // Odd slots of a context-owned submission take lane 1 where the caller has asked for two lanes: with a stream, a chain, a record
    // buffer and a work set of its own nothing is shared with the conversion before it, so its kernels run beside that conversion's
    // tail.  Records of consecutive conversions then alternate between two context-owned buffers; m2s_device_records / m2s_download
    // follow the conversion last waited for.
    const int L = !d_records && (k & 1u) && c->lanes == 2 ? 1 : 0;
    M2S_TRY(ensure_lane(c, L, L && mp, n_start));   // (lane 0: `fast` has seen its work set)
    m2s_host::Lane& ln = c->lane[L];
    hipStream_t st = d_records ? (hipStream_t)hip_stream : ln.stream;
    void* d_out = d_records ? d_records : ln.records.get();
    sl.own_lane = d_records ? -1 : L;
    // All conversions on lane 0 share its work buffers (look-back chain, counts, offsets, the deferred-triangle list) whatever stream
    // they run on: they must execute in submission order.  On one stream that is automatic; otherwise this one is ordered behind the
    // newest in flight that used them, with an event — a lane-0 submission after a conversion into a caller's buffer on the caller's
    // stream included
    if (L == 0)
        if (m2s_ctx::Slot* prev = newest_in_flight(c, [](const m2s_ctx::Slot& o) { return !o.sync_result && o.shared_work; }))
            if (prev->st != st) HIPCHK(c, hipStreamWaitEvent(st, prev->done[0], 0));
    if (sl.own_lane >= 0) {
        if (ln.rec_R != R) { ln.rec_R = R; ++ln.rec_gen; }
        sl.gen = ln.rec_gen;
    }
    unsigned long long* res = &c->h_total[2 + 2 * k];
    res[0] = 0; res[1] = 0;
    sl.prof = c->profiling;
    if (mp) {
        M2S_TRY(enqueue_multipass(c, L, R, (float4*)d_out, limit, StageMarks(), res, st));
    } else {
        uint32_t epoch;
        HIPCHK(c, next_epoch(c, &epoch));
        if (sl.prof) HIPCHK(c, hipEventRecord(sl.t[0], st));
        sl.bands_unit = unit_of(ri.form);
        launch_single(c, ri, R, ln.chain, limit, (float4*)d_out, res, epoch, bands_for(c, ri, sl.bands_unit, L == 0 && c->lanes == 1, &sl.wrote_bands),
                      st, nullptr);
        if (sl.prof) HIPCHK(c, hipEventRecord(sl.t[1], st));
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(sl.done[0], st));
    c->last_pipeline = ri.form;
    sl.st = st; sl.shared_work = L == 0; sl.ri_gen = ri.gen;
    sl.sync_result = false;
    sl.limit = limit;
    sl.d_out = d_out;
    ++c->slot_count;
    return M2S_OK;
}

m2s_status m2s_convert_wait(m2s_ctx* c, uint64_t* out_total) {
    if (!c) return M2S_ERR_INVALID;
    if (!c->slot_count) return fail(c, M2S_ERR_STATE, "no conversion in flight");
    const uint32_t k = c->slot_head;
    m2s_ctx::Slot& sl = c->slot[k];
    c->slot_head = (c->slot_head + 1) % M2S_MAX_IN_FLIGHT;
    --c->slot_count;
    // Conversions into a context-owned buffer overwrite each other in order, like repeated draws into one SSBO.  If a
    // LATER submission at another R has been enqueued into the buffer this conversion wrote, its records are not what
    // that buffer holds (any more): consumers (m2s_download, m2s_export_ply, m2s_prepass, sorts) then refuse instead of
    // returning the other conversion's records.
    const bool stale = sl.own_lane >= 0 && sl.gen != c->lane[sl.own_lane].rec_gen;
    if (sl.sync_result) {   // run_pass has run it already; its records may not be the current ones any more
        if (out_total) *out_total = sl.sync_total;
        c->slot_adopted(sl.d_out, sl.sync_total, sl.limit, sl.R, stale);
        memcpy(c->last_ms, sl.ms, sizeof sl.ms);
        return M2S_OK;
    }
    HIPCHK(c, wait_event(sl.done[0]));
    const uint64_t total = c->h_total[2 + 2 * k];
    const uint32_t any_big = (uint32_t)(c->h_total[3 + 2 * k] & 0xFFFFFFFFull), err = (uint32_t)(c->h_total[3 + 2 * k] >> 32);
    memset(c->last_ms, 0, sizeof c->last_ms);
    if (sl.prof) HIPCHK(c, hipEventElapsedTime(&c->last_ms[M2S_K_FUSED], sl.t[0], sl.t[1]));
    // what is remembered about (scene, R) may have been dropped since the submission (full table, m2s_set_pipeline): only an
    // entry of the generation the submission was made under is updated, and none is created here
    auto rit = c->rinfo.find(sl.R);
    m2s_ctx::RInfo* rip = (rit != c->rinfo.end() && rit->second.gen == sl.ri_gen) ? &rit->second : nullptr;
    if (err || any_big) {   // cannot happen for a scene/R that converted cleanly before; never return partial output silently
        if (rip) rip->async_ok = false;
        (void)hipMemsetAsync(c->d_bigmeta, 0, 4 * sizeof(uint32_t), c->stream);
        (void)hipStreamSynchronize(c->stream);
        return fail(c, M2S_ERR_STATE, "asynchronous conversion needed a host decision; convert synchronously");
    }
    if (sl.wrote_bands && rip) { rip->bands_ready = true; rip->bands_unit = sl.bands_unit; }   // that launch has completed: its run table is in place
    if (total > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 fragments: offsets are 32-bit");
    c->slot_adopted(sl.d_out, total, std::min(total, sl.limit), sl.R, stale);
    if (out_total) *out_total = total;
    return M2S_OK;
}

}  // extern "C"
