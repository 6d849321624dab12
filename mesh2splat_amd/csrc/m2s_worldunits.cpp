// m2s_worldunits.cpp — m2s_records_to_world_units: host side of m2s_worldunits.hip.  What the pass does to the context is what
// m2s_refit_apply does (m2s_refit.cpp), with the resolutionTarget going to 1 and the R of the conversion kept apart (conv_R) for the
// two readers that mean the scene's density, not the records' unit.
#include "m2s_ctx.h"

using namespace m2s;
using namespace m2s_host;

extern "C" {

m2s_status m2s_records_to_world_units(m2s_ctx* c, uint32_t* out_previous_R) {
    if (out_previous_R) *out_previous_R = 0;
    if (!c) return M2S_ERR_INVALID;
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    if (!c->last_records) return fail(c, M2S_ERR_STATE, "no conversion has run and no records were uploaded");
    if (c->records_stale) return fail(c, M2S_ERR_STATE, kStaleMsg);
    const uint64_t n = c->last_stored;
    if (n > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 records");
    const uint32_t R = c->last_R;
    if (out_previous_R) *out_previous_R = R;
    if (R <= 1) return M2S_OK;                  // world units already (uploaded records: taken as R = 1): nothing of the context changes
    HIPCHK(c, hipSetDevice(c->device));
    M2S_TRY(c->wu_ev.ensure(c->err));
    if (c->profiling) HIPCHK(c, hipEventRecord(c->wu_ev[0], c->stream));
    if (n) {
        // the pool holds the result: records that live elsewhere (adopted, a second lane's) are divided on their way there
        const float4* src = (const float4*)c->last_records;
        if (c->last_records != c->lane[0].records) M2S_TRY(ensure_records(c, n));
        HIPCHK(c, world_units(src, (float4*)c->lane[0].records.get(), (uint32_t)n, R, c->stream));
    } else {
        M2S_TRY(prune_compact_enqueue(c, 0, 0, nullptr, nullptr, false));
    }
    if (c->profiling) HIPCHK(c, hipEventRecord(c->wu_ev[1], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->last_world_units_ms = 0.0f;
    if (c->profiling) HIPCHK(c, hipEventElapsedTime(&c->last_world_units_ms, c->wu_ev[0], c->wu_ev[1]));
    prune_adopt(c, n, 1, false);
    c->refit_active = false;
    c->sh_valid = false;                        // (its rows belong to these records, but whatever m2s_refit_apply drops is dropped here)
    if (!c->conv_R) c->conv_R = R;              // (set already: a cut through a tree of stored-unit leaves brought their R back since)
    return M2S_OK;
}

float m2s_last_world_units_ms(const m2s_ctx* c) { return c ? c->last_world_units_ms : 0.0f; }

}  // extern "C"
