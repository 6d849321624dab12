// m2s_budget.cpp — pruning to a budget (m2s_prune_budget): host side of m2s_budget.hip.  The select leaves keep flags and their offsets
// where m2s_prune leaves its own; the compaction and what follows it are m2s_prune's (m2s_contrib.cpp: prune_compact_enqueue; m2s_recstate.h: rewritten).
#include "m2s_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace m2s;
using namespace m2s_host;

extern "C" {

m2s_status m2s_prune_budget(m2s_ctx* c, const m2s_budget_params* p, uint64_t* out_kept) {
    if (!c || !p) return M2S_ERR_INVALID;
    if (p->max_records == 0 || p->reserved != 0) return fail(c, M2S_ERR_INVALID, "max_records is 0 or reserved != 0");
    if (p->importance != M2S_IMPORTANCE_VIEWS && p->importance != M2S_IMPORTANCE_AREA) return fail(c, M2S_ERR_INVALID, "unknown importance");
    const bool views = p->importance == M2S_IMPORTANCE_VIEWS;
    if (views && std::isnan(p->min_weight)) return fail(c, M2S_ERR_INVALID, "min_weight is NaN");
    M2S_TRY(have_records(c));
    if (views && !contrib_valid(c)) return fail(c, M2S_ERR_STATE, "no accumulators of the current records (m2s_contrib_begin, m2s_contrib_accumulate)");
    const uint64_t n = c->last_stored;
    if (n > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 records");
    HIPCHK(c, hipSetDevice(c->device));
    ClockOf<BudgetMark>& clock = c->budget_clock;
    M2S_TRY(clock.begin(c->err, c->profiling));
    const uint32_t R = c->last_R;
    const uint32_t budget = (uint32_t)std::min<uint64_t>(p->max_records, 0xFFFFFFFFull);
    const bool sh = prune_sh_plane(c, n);
    uint32_t h[8] = {};
    uint64_t kept = 0, candidates = 0;
    if (n) {
        M2S_TRY(c->d_prune_u32.reserve(c->err, n, 2 * sizeof(uint32_t)));
        M2S_TRY(c->d_prune_temp.reserve(c->err, align_up(prune_scan_temp_bytes((uint32_t)n), 16) + 2 * sizeof(unsigned long long), 1));
        M2S_TRY(c->d_budget_keys.reserve(c->err, n, sizeof(uint32_t)));
        M2S_TRY(c->d_budget_state.reserve(c->err, kBudgetStateWords, sizeof(uint32_t)));
        HIPCHK(c, clock.mark(BudgetMark::Start, c->stream));   // (behind the allocations: stage [0] is keys + rounds)
        uint32_t* flags = c->d_prune_u32;
        uint32_t* offsets = flags + c->d_prune_u32.cap();
        const uint32_t* wmax = views ? c->d_contrib.get() : nullptr;
        const uint32_t* npix = views ? c->d_contrib + c->d_contrib.cap() : nullptr;
        HIPCHK(c, budget_select((const float4*)c->last_records, wmax, npix, (uint32_t)n, p->importance, p->min_weight, p->min_pixels, budget,
                                c->d_budget_keys, c->d_budget_state, flags, offsets, c->d_prune_temp,
                                c->d_prune_temp.cap() - 2 * sizeof(unsigned long long), clock.marks(BudgetMark::Selected), c->stream));
        HIPCHK(c, hipMemcpyAsync(h, c->d_budget_state, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < kBudgetShards; ++k) candidates += h[kBudgetCandidates + k];
        kept = h[kBudgetActive] ? budget : candidates;
        HIPCHK(c, clock.mark(BudgetMark::Compact, c->stream));   // (the round trip above is in no stage)
        M2S_TRY(prune_compact_enqueue(c, n, kept, flags, offsets, sh));
    } else {
        M2S_TRY(prune_compact_enqueue(c, 0, 0, nullptr, nullptr, false));
    }
    HIPCHK(c, clock.mark(BudgetMark::Compacted, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (clock.on()) {   // (no records: no marks, three zeros)
        HIPCHK(c, clock.span(BudgetMark::Start, BudgetMark::Selected, &c->last_budget_stage_ms[0]));
        HIPCHK(c, clock.span(BudgetMark::Selected, BudgetMark::Scanned, &c->last_budget_stage_ms[1]));
        HIPCHK(c, clock.span(BudgetMark::Compact, BudgetMark::Compacted, &c->last_budget_stage_ms[2]));
    }
    c->rewritten(c->lane[0].records, kept, R, sh ? Rewrite::PruneWithSh : Rewrite::Prune);
    const bool active = h[kBudgetActive] != 0;
    c->last_budget_counts[0] = n;
    c->last_budget_counts[1] = candidates;
    c->last_budget_counts[2] = kept;
    c->last_budget_counts[3] = active ? h[kBudgetPrefix] : 0;
    c->last_budget_counts[4] = active ? h[kBudgetQuota] : 0;
    c->last_budget_counts[5] = active ? h[kBudgetTies] : 0;
    if (out_kept) *out_kept = kept;
    return M2S_OK;
}

m2s_status m2s_last_budget_counts(const m2s_ctx* c, uint64_t out[6]) { return get_array(c, &m2s_ctx::last_budget_counts, out); }

m2s_status m2s_last_budget_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_budget_stage_ms, out_ms); }

}  // extern "C"
