// m2s_context.cpp — context lifetime, policy setters, the record pool and the launch tags of the look-back chains.
#include "m2s_ctx.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

using namespace m2s;
using namespace m2s_host;

namespace {
thread_local std::string g_create_error = "";
}  // namespace

namespace m2s_host {
void free_scene(m2s_ctx* c) {
    c->tri_mem.release(); c->scene_arena.release();
    c->lane[0].release_scene(false); c->lane[1].release_scene(true);
    // everything below lived inside the arena (lane 0's chain and offsets too)
    c->d_meshes = nullptr; c->d_mesh_first = nullptr;
    c->d_cnt = c->d_partials = nullptr;
    c->d_biglist = nullptr; c->d_bigmeta = nullptr; c->d_bands = nullptr; c->run_table_words = 0; c->d_run_order = nullptr; c->d_run_rank = nullptr; c->run_order_unit = 0;
    c->d_batch_first = nullptr; c->n_batch_tab = 0; c->chain_words = 0;
    c->rinfo.clear();
    ++c->rinfo_gen;
    c->frag_per_R2 = -1.0;
    c->warm_R = 0; c->warm_total = 0; c->warm_mismatch_seen = false;
    c->sparse_off_R = c->team_off_R = c->lean_off_R = UINT32_MAX;
    c->lean_ok = false;
    c->d_vt_rows.release(); c->d_vt_ids.release();
    c->vt_rows = 0; c->vt_use = false;
    c->geo_stride = 0; c->geo_use = false;   // (d_geo itself is grow-only: the next upload keeps, regrows or releases it)
    c->scene = SceneDev{};
    c->has_scene = false;
}

// What is remembered about this scene at resolution R (created on first use, its form decided before its first launch: decide in
// m2s_pass.cpp; the table is bounded: a slider dragged through hundreds of densities simply starts over).
m2s_ctx::RInfo& rinfo_for(m2s_ctx* c, uint32_t R) {
    auto it = c->rinfo.find(R);
    if (it != c->rinfo.end()) return it->second;
    // (a full table starts over; submissions still in flight remember the generation they were made under, so that a band
    //  slot which now belongs to another density is never marked ready on their behalf: m2s_convert_wait)
    // (the slots' run tables are about to be re-used by other densities: nothing in flight may still be reading one)
    if (c->rinfo.size() >= (size_t)kBandSlots) { drain_in_flight(c); c->rinfo.clear(); ++c->rinfo_gen; }
    m2s_ctx::RInfo ri;
    ri.gen = c->rinfo_gen;
    ri.band_slot = (int)c->rinfo.size();
    return c->rinfo.emplace(R, ri).first->second;
}

static bool spin_waits() { static const bool on = !debug_on("M2S_NO_SPIN"); return on; }
template <class Query, class Block>
static hipError_t spin_then_block(Query query, Block block) {
    if (spin_waits()) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t i = 0;; ++i) {
            const hipError_t e = query();
            if (e != hipErrorNotReady) return e;
            if ((i & 15u) == 15u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(400)) break;
        }
        (void)hipGetLastError();   // (hipErrorNotReady is sticky in hipGetLastError)
    }
    return block();
}
hipError_t wait_stream(hipStream_t st) { return spin_then_block([&] { return hipStreamQuery(st); }, [&] { return hipStreamSynchronize(st); }); }
hipError_t wait_event(hipEvent_t ev) { return spin_then_block([&] { return hipEventQuery(ev); }, [&] { return hipEventSynchronize(ev); }); }

// every conversion still in flight has finished when this returns (their slots stay queued for m2s_convert_wait)
void drain_in_flight(m2s_ctx* c, int lane) {
    each_in_flight(c, [&](m2s_ctx::Slot& sl) {
        if (!sl.sync_result && (lane < 0 || sl.own_lane == lane)) (void)hipEventSynchronize(sl.done[0]);
    });
}

// Chain words carry a 16-bit launch tag instead of being cleared per launch.  The two single-pass kernels use different
// numbers of words, so a word one of them left behind could read as freshly published 65 536 launches later: when the
// tag wraps, everything in flight is drained and every lane's chain is cleared (once per ~10 s of back-to-back conversions).
hipError_t next_epoch(m2s_ctx* c, uint32_t* out) {
    const uint32_t e = ++c->epoch;
    *out = e;
    if ((e & 0xFFFFu) != 0) return hipSuccess;
    const size_t bytes = std::max<size_t>(c->chain_words, 1) * sizeof(unsigned long long);
    hipError_t r = hipDeviceSynchronize();
    for (const Lane& ln : c->lane)
        if (r == hipSuccess && ln.chain) r = hipMemset(ln.chain, 0, bytes);
    return r;
}

// The context-owned record buffer is a grow-only pool.  The reference re-creates its SSBO whenever the cap changes
// (ConversionPass.cpp:25-33), i.e. on every move of the density slider; here a change of R costs no allocation: the pool
// doubles until it reaches the largest size the cap policy can ask for (7 M records = 672 MB for the reference formula).
m2s_status ensure_records(m2s_ctx* c, uint64_t want) {
    Lane& l0 = c->lane[0];
    if (l0.records.cap() >= want && l0.records) return M2S_OK;
    uint64_t grow = std::max<uint64_t>(want, 1);
    if (l0.records.cap()) grow = std::max(grow, 2 * l0.records.cap());
    if (c->cap_policy < 0) grow = std::max(want, std::min<uint64_t>(grow, kMaxGaussiansToSort));
    drain_in_flight(c);   // nothing may still be writing the buffer that is about to be released
    c->pool_released(l0.records.get());   // current records that live there go with the old pool
    // (the larger request may fail where the one the caller needs still fits)
    if (grow == want || !l0.records.try_reserve(grow, sizeof(m2s_gaussian))) M2S_TRY(l0.records.reserve(c->err, want, sizeof(m2s_gaussian)));
    // in-flight conversions into the old buffer are complete but their records are gone
    each_in_flight(c, [&](m2s_ctx::Slot& sl) {
        if (sl.own_lane == 0) { sl.d_out = l0.records; sl.gen = l0.rec_gen - 1u; }
    });
    return M2S_OK;
}
}  // namespace m2s_host

extern "C" {

uint32_t m2s_abi_version(void) { return M2S_ABI_VERSION; }

const char* m2s_last_error(const m2s_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

m2s_status m2s_create(int device, m2s_ctx** out_ctx) {
    if (!out_ctx) { g_create_error = "out_ctx is NULL"; return M2S_ERR_INVALID; }
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_error = std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "count=0") +
                         "); this library has no CPU path";
        return M2S_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) { g_create_error = "device index out of range"; return M2S_ERR_NO_DEVICE; }
    m2s_ctx* c = new (std::nothrow) m2s_ctx();
    if (!c) { g_create_error = "host allocation failed"; return M2S_ERR_OOM; }
    c->device = device;
    unsigned done_flags = hipEventDisableTiming;   // (completion only: its time is never asked for)
    if (const char* v = debug_env("M2S_DONE_EVENT_FLAGS")) {   // debug: A/B of event kinds; anything but a combination of the known bits is ignored
        const unsigned f = (unsigned)strtoul(v, nullptr, 0);
        if ((f & ~(hipEventBlockingSync | hipEventDisableTiming | hipEventReleaseToDevice | hipEventReleaseToSystem)) == 0u) done_flags = f;
    }
    // everything a conversion needs is created here, none of it inside one; what exists when a step fails goes with the context
    m2s_status s = hip_status(c->err, "hipSetDevice", hipSetDevice(device));
    if (!s) s = c->streams.ensure(c->err, 0);
    if (!s) s = c->lane[0].total.reserve(c->err, 1, sizeof(unsigned long long));
    if (!s) s = c->h_total.ensure(c->err, m2s_ctx::kPinnedWords * sizeof(unsigned long long));
    if (!s) s = c->stage_ev.ensure(c->err, hipEventDisableTiming);
    for (auto& sl : c->slot) {
        if (!s) s = sl.done.ensure(c->err, done_flags);
        if (!s) s = sl.t.ensure(c->err);
    }
    if (s) {
        g_create_error = c->err;
        delete c;
        return M2S_ERR_HIP;
    }
    c->stream = c->lane[0].stream = c->streams[0];
    *out_ctx = c;
    return M2S_OK;
}

void m2s_destroy(m2s_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (const Lane& ln : c->lane)
        if (ln.stream) (void)hipStreamSynchronize(ln.stream);
    drain_in_flight(c);   // conversions still in flight on a caller's stream
    delete c;   // buffers, pinned blocks and events go with their members, the streams last (m2s_devbuf.h)
}

m2s_status m2s_set_triangle_range(m2s_ctx* c, uint64_t first, uint64_t count) {
    if (!c) return M2S_ERR_INVALID;
    c->range_first = first;
    c->range_count = count;
    return M2S_OK;
}

m2s_status m2s_set_max_gaussians(m2s_ctx* c, int64_t cap) {
    if (!c) return M2S_ERR_INVALID;
    if (cap < -1) return fail(c, M2S_ERR_INVALID, "cap must be -1 (reference formula), 0 (unlimited) or > 0");
    c->cap_policy = cap;
    return M2S_OK;
}

m2s_status m2s_set_profiling(m2s_ctx* c, int enabled) {
    if (!c) return M2S_ERR_INVALID;
    c->profiling = enabled != 0;
    return M2S_OK;
}

m2s_status m2s_set_pipeline(m2s_ctx* c, int pipeline) {
    if (!c) return M2S_ERR_INVALID;
    if (pipeline < M2S_PIPELINE_AUTO || pipeline > M2S_PIPELINE_LEAN) return fail(c, M2S_ERR_INVALID, "unknown pipeline");
    if (pipeline == 2) return fail(c, M2S_ERR_INVALID, "pipeline 2 (the one-wave-per-batch kernel of rounds 1-5) no longer exists: use M2S_PIPELINE_TEAM");
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    if (c->pipeline != pipeline) {   // what was remembered about this scene under the old setting no longer applies
        c->rinfo.clear();
        ++c->rinfo_gen;
    }
    c->pipeline = pipeline;
    return M2S_OK;
}

int m2s_last_pipeline(const m2s_ctx* c) { return c ? c->last_pipeline : 0; }

m2s_status m2s_vertex_table(const m2s_ctx* c, uint64_t* out_rows, int* out_in_use) {
    if (!c) return M2S_ERR_INVALID;
    if (out_rows) *out_rows = c->vt_rows;
    if (out_in_use) *out_in_use = c->vt_use ? 1 : 0;
    return M2S_OK;
}

m2s_status m2s_geo_planes(const m2s_ctx* c, uint64_t* out_bytes, int* out_in_use) {
    if (!c) return M2S_ERR_INVALID;
    if (out_bytes) *out_bytes = c->geo_use ? (uint64_t)c->scene.n_tri * 3u * sizeof(float4) : 0u;
    if (out_in_use) *out_in_use = c->geo_use ? 1 : 0;
    return M2S_OK;
}

int m2s_positions_ready(const m2s_ctx* c) {
    return c && c->last_stored && positions_valid(c, c->last_stored) ? 1 : 0;
}

m2s_status m2s_set_keep_positions(m2s_ctx* c, int enabled) {
    if (!c) return M2S_ERR_INVALID;
    c->keep_positions = enabled != 0;
    return M2S_OK;
}

m2s_status m2s_set_carry_sh(m2s_ctx* c, int enabled) {
    if (!c) return M2S_ERR_INVALID;
    c->carry_sh = enabled != 0;
    return M2S_OK;
}

int m2s_carry_sh(const m2s_ctx* c) { return c && c->carry_sh ? 1 : 0; }

m2s_status m2s_set_merge_model(m2s_ctx* c, uint32_t model, float sigma) {
    if (!c) return M2S_ERR_INVALID;
    if (model != M2S_MERGE_MODEL_FOOTPRINT && model != M2S_MERGE_MODEL_GAUSSIAN) return fail(c, M2S_ERR_INVALID, "model is neither M2S_MERGE_MODEL_FOOTPRINT nor M2S_MERGE_MODEL_GAUSSIAN");
    if (!std::isfinite(sigma) || !(sigma > 0.0f)) return fail(c, M2S_ERR_INVALID, "sigma is not finite or not positive");
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    c->merge_model = model;
    c->merge_sigma = sigma;
    return M2S_OK;
}

uint32_t m2s_merge_model(const m2s_ctx* c) { return c ? c->merge_model : (uint32_t)M2S_MERGE_MODEL_FOOTPRINT; }

float m2s_merge_sigma(const m2s_ctx* c) { return c ? c->merge_sigma : 1.0f; }

m2s_status m2s_debug_set_launch_counter(m2s_ctx* c, uint32_t value) {
    if (!c) return M2S_ERR_INVALID;
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    c->epoch = value;
    return M2S_OK;
}

m2s_status m2s_set_async_lanes(m2s_ctx* c, int lanes) {
    if (!c) return M2S_ERR_INVALID;
    if (lanes != 1 && lanes != 2) return fail(c, M2S_ERR_INVALID, "lanes must be 1 or 2");
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    c->lanes = lanes;
    return M2S_OK;
}

m2s_status m2s_last_kernel_ms(const m2s_ctx* c, float out_ms[M2S_K_N]) { return get_array(c, &m2s_ctx::last_ms, out_ms); }

}  // extern "C"
