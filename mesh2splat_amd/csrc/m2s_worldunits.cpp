// m2s_worldunits.cpp — m2s_records_to_world_units: host side of m2s_worldunits.hip.  What the pass does to the context (m2s_recstate.h,
// Rewrite::WorldUnits): the resolutionTarget goes to 1 and the R of the conversion is kept apart (conv_R) for the two readers that mean
// the scene's density, not the records' unit.
#include "m2s_ctx.h"

using namespace m2s;
using namespace m2s_host;

extern "C" {

m2s_status m2s_records_to_world_units(m2s_ctx* c, uint32_t* out_previous_R) {
    if (out_previous_R) *out_previous_R = 0;
    if (!c) return M2S_ERR_INVALID;
    uint64_t n = 0;
    M2S_TRY(need_records(c, &n));
    const uint32_t R = c->last_R;
    if (out_previous_R) *out_previous_R = R;
    if (R <= 1) return M2S_OK;                  // world units already (uploaded records: taken as R = 1): nothing of the context changes
    HIPCHK(c, hipSetDevice(c->device));
    M2S_TRY(c->wu_clock.begin(c->err, c->profiling));
    HIPCHK(c, c->wu_clock.mark(SpanMark::Begin, c->stream));
    if (n) {
        // the pool holds the result: records that live elsewhere (adopted, a second lane's) are divided on their way there
        const float4* src = (const float4*)c->last_records;
        if (c->last_records != c->lane[0].records) M2S_TRY(ensure_records(c, n));
        HIPCHK(c, world_units(src, (float4*)c->lane[0].records.get(), (uint32_t)n, R, c->stream));
    } else {
        M2S_TRY(prune_compact_enqueue(c, 0, 0, nullptr, nullptr, false));
    }
    HIPCHK(c, c->wu_clock.mark(SpanMark::End, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->wu_clock.span(SpanMark::Begin, SpanMark::End, &c->last_world_units_ms));   // (0 without profiling)
    c->rewritten(c->lane[0].records, n, 1, Rewrite::WorldUnits);
    return M2S_OK;
}

float m2s_last_world_units_ms(const m2s_ctx* c) { return c ? c->last_world_units_ms : 0.0f; }

}  // extern "C"
