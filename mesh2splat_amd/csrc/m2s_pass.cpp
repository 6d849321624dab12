// m2s_pass.cpp — the conversion pass driver (== ConversionPass::execute, src/renderer/renderPasses/ConversionPass.cpp:9-68):
// pipeline choice, XCD band tables, the single-pass kernels with their fallbacks, the multi-pass pipeline.
#include "m2s_ctx.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace m2s;
using namespace m2s_host;

namespace {
// AUTO: below this many fragments per triangle the sparse kernel runs.  Measured against k_fused2 on cube-spheres
// (tools/sparse_crossover.py, profiles/r03/v3_sparse_crossover_*): with 3 M and 6.2 M triangles k_sparse is ahead up to 1.75
// fragments per triangle (a workgroup's stream overflows from ~2.5); with 1 M triangles — 2.5 generations of its 512-triangle
// workgroups — k_fused2 is ahead down to 0.68 at least.
static double sparse_frags_per_triangle(uint32_t n_tri) { return n_tri >= 2000000u ? 1.75 : 0.5; }
// XCD runs (RunInfo, m2s_device.h) for this launch of k_fused2 (unit 256) or k_sparse (unit 512 triangles): the table an earlier
// launch of the same kernel at this R — or the count at upload — left behind; or, if there is none, ask this launch to record
// where every run's output starts (second lane: never asked to — two lanes would race on the table)
static uint32_t band_workgroups(const m2s_ctx* c, uint32_t unit) {
    const uint32_t team = fused2_band_workgroups(c->scene.n_tri);
    return !team ? 0u : unit == 256u ? team : sparse_workgroups(c->scene.n_tri);
}
}  // namespace

namespace m2s_host {
RunInfo bands_for(const m2s_ctx* c, const m2s_ctx::RInfo& ri, uint32_t unit, bool may_write, bool* writes) {
    RunInfo r{ nullptr, nullptr, 0u, nullptr };
    if (writes) *writes = false;
    const uint32_t n_wg = band_workgroups(c, unit);
    const uint32_t shift = run_shift_for(n_wg);
    if (!n_wg || !shift || !c->d_bands || !c->run_table_words || (unit == 256u && (c->n_batch_tab || ri.tpw)) || debug_on("M2S_NO_BANDS")) return r;
    if ((size_t)n_runs(n_wg, shift) > c->run_table_words) return r;
    unsigned long long* table = c->d_bands + (size_t)ri.band_slot * c->run_table_words;
    r.shift = shift;
    if (ri.bands_ready && ri.bands_unit == unit) {
        r.base = table;
        // heaviest runs first (built by warm_scene from the exact counts at ITS R: the ranking of the runs is a property of the mesh)
        if (c->run_order_unit == unit && c->run_order_shift == shift && !debug_on("M2S_NO_RUN_ORDER")) r.order = c->d_run_order;
    }
    else if (may_write) { r.out = table; if (writes) *writes = true; }
    return r;
}

BatchTable batches_for(const m2s_ctx* c, const m2s_ctx::RInfo& ri) {
    return c->n_batch_tab ? BatchTable{ c->d_batch_first, c->n_batch_tab, 0u } : BatchTable{ nullptr, 0u, ri.tpw };
}

uint32_t unit_of(int form) { return form == M2S_PIPELINE_SPARSE ? kSparseTrianglesPerWorkgroup : 256u; }

// One launch of the single-pass form ri.form: the kernel writes its fragment counter to res[0] and its two status words to res[1]
// (pinned host memory).  Only k_sparse takes the position plane.
void launch_single(const m2s_ctx* c, const m2s_ctx::RInfo& ri, uint32_t R, unsigned long long* chain, uint64_t limit, float4* d_out,
                   unsigned long long* res, uint32_t epoch, const RunInfo& runs, hipStream_t st, float4* plane) {
    uint32_t* status = reinterpret_cast<uint32_t*>(&res[1]);
    if (ri.form == M2S_PIPELINE_SPARSE)
        launch_sparse(c->scene, R, chain, limit, d_out, &res[0], status, epoch, c->d_biglist, c->d_bigmeta, runs, st, plane);
    else if (ri.form == M2S_PIPELINE_LEAN) {
        const VtxTable vt{ c->d_vt_rows.get(), c->d_vt_ids.get() };
        const GeoPlanes gp{ c->d_geo.get(), c->d_geo.get() + c->geo_stride, c->d_geo.get() + 2 * c->geo_stride };
        launch_fused3(c->scene, R, chain, limit, d_out, &res[0], status, epoch, c->d_biglist, c->d_bigmeta, runs, batches_for(c, ri), st,
                      c->vt_use ? &vt : nullptr, c->geo_use ? &gp : nullptr);
    }
    else
        launch_fused2(c->scene, R, chain, limit, d_out, &res[0], status, epoch, c->d_biglist, c->d_bigmeta, runs, batches_for(c, ri), st);
}

uint64_t resolve_cap(const m2s_ctx* c, uint32_t R) {
    if (c->cap_policy == 0) return 0;
    if (c->cap_policy > 0) return (uint64_t)c->cap_policy;
    // ConversionPass.cpp:21-24 (unsigned int arithmetic wraps)
    const uint32_t mc = std::max<uint32_t>(1u, c->n_meshes_total);
    const uint32_t mx = R * R * 6u * mc;
    return std::min(mx, kMaxGaussiansToSort);
}
}  // namespace m2s_host

// The team kernel in its lean form (m2s_fused3.hip): LEAN uses it where the scene allows it (m2s_ctx::lean_ok) below the R at which
// it overflowed its LDS stream or deferred many triangles; AUTO only for scenes of more than one generation of workgroups (64
// triangles per wave: a fourth workgroup per CU does nothing for a launch that fits the GPU once — C2 stand-in 0.0354 (k_fused2) vs
// 0.0362 ms, config 3 0.1170 vs 0.1138, profiles/r05/ab_lean_team_kernel.log)
static bool lean_eligible(const m2s_ctx* c, uint32_t R) {
    if (!c->lean_ok || R >= c->lean_off_R || debug_on("M2S_NO_LEAN")) return false;
    return c->pipeline == M2S_PIPELINE_LEAN || (c->pipeline == M2S_PIPELINE_AUTO && fused_tpw(c->scene.n_tri) == 64u);
}

// The starting form of this scene at R: the setting's, or AUTO's from the (exact or predicted) fragment count; a form whose
// threshold (m2s_ctx::*_off_R) is at or below R is passed over.
// AUTO: the single-pass kernel wins while triangles are small (it does the per-triangle work once and needs no second
// sweep); with more than ~11 fragments per triangle on average the output-partitioned multi-pass pipeline is
// faster and soon much faster (2.74 M fragments at R = 1024 from 1 M / 250 k / 125 k / 62 k triangles: fused 0.167 /
// 0.138 / 0.323 / 0.626 ms, multi-pass 0.214 / 0.137 / 0.136 / 0.154 ms; tools/auto_probe.py).
// Round 5, the lower edge of the multi-pass range: from 11 to 13 fragments per triangle the team kernel in SMALLER batches (40 triangles
// per wave, so that a workgroup's 160 triangles still fit its 4096-entry LDS stream) beats the multi-pass pipeline — 235 200 triangles
// at 11.6 fragments each: kernels 0.113 against 0.118 ms, one blocking call 0.127 against 0.146 (one launch instead of two;
// profiles/r05/band_probe.jsonl); at 14 fragments per triangle a cube-sphere's densest workgroups overflow the stream even at 40
// (the launch is then repeated by the multi-pass pipeline, which wins from there on anyway: 0.110 ms).  Taken only at the R the
// scene was counted at (R == warm_R: the first conversion after an upload, the reference's case) and only if triangles of more than
// 96 fragments — which a single-pass kernel defers — hold less than an eighth of the fragments: a scene whose MEAN falls in the band
// because it mixes planes with foliage (synth.sponza_like: 16 per triangle) belongs to the multi-pass pipeline and its fine blocks.
static void decide(const m2s_ctx* c, m2s_ctx::RInfo& ri, double frags, uint32_t R) {
    const double n_tri = (double)c->scene.n_tri;
    ri.tpw = 0;
    ri.form = M2S_PIPELINE_MULTIPASS;
    if (c->pipeline == M2S_PIPELINE_MULTIPASS || R >= c->team_off_R) return;
    if (c->pipeline == M2S_PIPELINE_AUTO && frags >= 11.0 * n_tri) {
        if (frags < 13.0 * n_tri && R == c->warm_R && c->warm_total > 0 && c->warm_big * 8ull < c->warm_total &&
            fused_tpw(c->scene.n_tri) == 64u && !c->n_batch_tab && !debug_on("M2S_NO_BAND_TPW")) {
            ri.form = M2S_PIPELINE_TEAM;
            ri.tpw = 40;
        }
        return;
    }
    // about as many fragments as triangles, or fewer: many triangles cover no pixel centre, the sparse form drops them cheaply
    // (crossover measured with tools/sparse_probe.py: see DESIGN.md); it needs scenes large enough for 64-triangle batches
    const bool sparse = c->pipeline == M2S_PIPELINE_SPARSE ||
                        (c->pipeline == M2S_PIPELINE_AUTO && frags < sparse_frags_per_triangle(c->scene.n_tri) * n_tri && !debug_on("M2S_NO_SPARSE"));
    if (sparse && R < c->sparse_off_R && sparse_supported(c->scene.n_tri)) ri.form = M2S_PIPELINE_SPARSE;
    else ri.form = lean_eligible(c, R) ? M2S_PIPELINE_LEAN : M2S_PIPELINE_TEAM;
}

// What a single-pass launch ran into (run_pass): status 2, a workgroup's entries did not fit the kernel's LDS stream (true of every
// larger R as well); any other status, a bounded look-back wait gave up (never observed; would need a dispatcher that starves earlier
// workgroups); many triangles deferred by AUTO's k_fused3; deferred triangles holding much of the output
enum class Trouble { full, stalled, lean_defers, big_share };

// The ladder: demote() is the only code that moves a (scene, R) down it, after a launch of ri.form ran into `why`.
//
//   ri.form  why                          next form                            remembered for every larger R
//   SPARSE   full / stalled               LEAN if lean_eligible, else TEAM     full: sparse_off_R
//   LEAN     full / stalled               TEAM                                 full: lean_off_R
//   LEAN     lean_defers                  TEAM                                 lean_off_R
//   TEAM     full / stalled, tpw != 0     MULTIPASS, tpw = 0                   -
//   TEAM     full / stalled               MULTIPASS                            full: team_off_R
//   any      big_share                    MULTIPASS                            -
//
// The multi-pass pipeline has neither limit; it is where every (scene, R) can end.
static void demote(m2s_ctx* c, m2s_ctx::RInfo& ri, uint32_t R, Trouble why) {
    const bool every_larger_R = why == Trouble::full || why == Trouble::lean_defers;
    if (why == Trouble::big_share) {
        ri.form = M2S_PIPELINE_MULTIPASS;
    } else if (ri.form == M2S_PIPELINE_SPARSE) {
        if (every_larger_R) c->sparse_off_R = std::min(c->sparse_off_R, R);
        ri.form = lean_eligible(c, R) ? M2S_PIPELINE_LEAN : M2S_PIPELINE_TEAM;
    } else if (ri.form == M2S_PIPELINE_LEAN) {
        if (every_larger_R) c->lean_off_R = std::min(c->lean_off_R, R);
        ri.form = M2S_PIPELINE_TEAM;
    } else {
        if (ri.tpw) ri.tpw = 0;
        else if (every_larger_R) c->team_off_R = std::min(c->team_off_R, R);
        ri.form = M2S_PIPELINE_MULTIPASS;
    }
}

namespace m2s_host {
// Everything a FIRST conversion of a scene used to find out inside its own call — round 3: an exact count, a host round trip,
// the record pool's hipMalloc, a launch without bands: 0.45 ms on config 3 against 0.13 ms for a repeated conversion — is
// found out here, behind the upload's own kernels, at the resolution the caller is about to convert at (m2s_set_resolution_hint;
// default: the last R this context converted at, else 1024).  The reference converts right after SceneManager::loadModel at the
// RenderContext's current resolutionTarget (guiRendererConcreteMediator.cpp:11-29), never twice at one (scene, R): its first
// conversion is the one that counts.  Left behind: the scene's fragments / R^2 (AUTO's decision and the pool size at ANY R
// without touching the device), and for R itself the decision, the XCD run table from the exact counts (k_unit_bases), the batch table of one-generation scenes, the multi-pass work buffers, the record pool.
// The count itself, enqueued by m2s_upload_scene behind the geometry and in front of the texture copies: exact fragments per triangle
// (d_cnt), their scanned partial sums, the total on its way to pinned memory.  warm_scene(counted = true) picks it up after the
// upload's own synchronisation.
m2s_status warm_count_enqueue(m2s_ctx* c, uint32_t R) {
    const SceneDev& sc = c->scene;
    if (!sc.n_tri || R == 0 || R > 4096) return M2S_ERR_INVALID;
    hipStream_t st = c->stream;
    launch_count(sc, R, c->d_cnt, c->d_partials, st);
    launch_scan_partials(c->d_partials, n_count_blocks(sc.n_tri), c->lane[0].total, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_total, c->lane[0].total, 8, hipMemcpyDeviceToHost, st));
    // ... and, on the expectation that AUTO will take the team kernel (units of 256 triangles) — the common case —, the run table and
    // the dispatch order of its first launch at R, which depend on the counts only: if the decision turns out otherwise, warm_scene
    // builds what it needs as before
    c->warm_spec_unit = 0;
    if (!debug_on("M2S_NO_WARM_BANDS")) {
        m2s_ctx::RInfo& ri = rinfo_for(c, R);
        const uint32_t unit = unit_of(M2S_PIPELINE_TEAM);
        bool writes = false;
        const RunInfo table = bands_for(c, ri, unit, true, &writes);
        if (writes) {
            const uint32_t n_units = band_workgroups(c, unit);
            launch_unit_bases(c->d_cnt, c->d_partials, sc.n_tri, unit, table.shift, table.out, st);
            launch_run_order(table.out, n_runs(n_units, table.shift), c->lane[0].total, c->d_run_order, run_order_slots(n_units, table.shift),
                             c->d_run_rank, st);
            HIPCHK(c, hipGetLastError());
            c->warm_spec_unit = unit; c->warm_spec_shift = table.shift;
        }
    }
    return M2S_OK;
}

m2s_status warm_scene(m2s_ctx* c, uint32_t R, bool counted) {
    const SceneDev& sc = c->scene;
    if (!sc.n_tri || R == 0 || R > 4096) return M2S_OK;
    hipStream_t st = c->stream;
    if (!counted) {
        const m2s_status s = warm_count_enqueue(c, R);
        if (s != M2S_OK) return s;
        HIPCHK(c, hipStreamSynchronize(st));
    }
    const uint64_t total = c->h_total[0];
    c->frag_per_R2 = (double)total / ((double)R * (double)R);
    c->warm_R = R;
    c->warm_total = total;
    c->warm_big = 0;
    if (total >= 11ull * sc.n_tri && total < 13ull * sc.n_tri) {   // (the only case decide() asks for it)
        HIPCHK(c, hipMemsetAsync(c->lane[0].total, 0, 8, st));
        launch_big_share(c->d_cnt, sc.n_tri, 96u, c->lane[0].total, st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&c->h_total[1], c->lane[0].total, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->warm_big = c->h_total[1];
        c->h_total[1] = 0;
        const unsigned long long tot = total;      // (d_total served as the accumulator: the total goes back, launch_run_order below reads it)
        HIPCHK(c, hipMemcpy(c->lane[0].total, &tot, sizeof tot, hipMemcpyHostToDevice));
    }
    // A scene small enough for ONE generation of workgroups (fused_tpw < 64) lasts as long as its slowest workgroup: cut it into
    // batches of equal estimated work instead of equal triangle counts (C2 stand-in: fragments per workgroup vary 1 : 3 over a
    // cube-sphere face).  Work = 214 per triangle + 140 per fragment (cycles of the triangle phase per 64 triangles and of a strip
    // per 64 fragments, tools/team_timing.py); fragments scale with R^2 everywhere alike, so the table serves every density.
    if (batch_table_capacity(sc.n_tri) && !c->n_batch_tab && !debug_on("M2S_NO_BATCH_TABLE")) {
        try {
            std::vector<uint32_t> cnt(sc.n_tri), first;
            HIPCHK(c, hipMemcpy(cnt.data(), c->d_cnt, (size_t)sc.n_tri * sizeof(uint32_t), hipMemcpyDeviceToHost));
            uint32_t n_target = n_fused_waves(sc.n_tri);
            if (const char* v = debug_env("M2S_BATCH_TARGET")) { const unsigned long q = strtoul(v, nullptr, 10); if (q >= 1 && q <= 8192) n_target = (uint32_t)q; }   // debug: A/B
            double ct = 214.0;
            const double cf = 140.0;
            if (const char* v = debug_env("M2S_BATCH_CT")) ct = atof(v);   // debug: A/B of the work model
            double total = 0.0;
            for (uint32_t t = 0; t < sc.n_tri; ++t) total += ct + cf * (double)cnt[t];
            const double quota = total / (double)n_target;
            first.reserve(batch_table_capacity(sc.n_tri));
            first.push_back(0);
            double acc = 0.0;
            uint32_t in_batch = 0;
            for (uint32_t g = 0; g < sc.n_tri; g += 8) {          // batches start at multiples of 8 (mesh_of8)
                const uint32_t ge = std::min(g + 8u, sc.n_tri);
                double gc = 0.0;
                for (uint32_t t = g; t < ge; ++t) gc += ct + cf * (double)cnt[t];
                // close the batch before this group if it is full, or if the work so far has reached the batch's share
                if (in_batch && (in_batch + (ge - g) > 64u || acc + 0.5 * gc >= quota * (double)first.size())) { first.push_back(g); in_batch = 0; }
                acc += gc;
                in_batch += ge - g;
            }
            first.push_back(sc.n_tri);
            if (first.size() <= batch_table_capacity(sc.n_tri)) {
                HIPCHK(c, hipMemcpy(c->d_batch_first, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
                c->n_batch_tab = (uint32_t)first.size() - 1u;
            }
        } catch (...) { /* no table: uniform batches */ }
    }
    m2s_ctx::RInfo& ri = rinfo_for(c, R);
    if (ri.form == M2S_PIPELINE_AUTO) decide(c, ri, (double)total, R);
    const uint64_t cap = resolve_cap(c, R);
    const bool single = ri.form != M2S_PIPELINE_MULTIPASS;
    // the code object of the pipeline this scene is about to run: loaded here, not inside the first conversion of the process
    if (!debug_on("M2S_NO_PRELOAD")) {
        if (!single) { (void)preload_multipass(); if (!debug_on("M2S_NO_SCRATCH_WARM")) launch_scratch_warm(st); }
        else if (ri.form == M2S_PIPELINE_SPARSE) { (void)preload_sparse(); (void)preload_fused2(); }   // (the sparse form falls back to the team on a stream overflow)
        else if (ri.form == M2S_PIPELINE_LEAN) { (void)preload_fused3(); }
        else { (void)preload_fused2(); }
        (void)hipGetLastError();
    }
    if (single && !debug_on("M2S_NO_WARM_BANDS")) {
        // the run table of the first launch at R, from the exact counts (the same table a launch without runs leaves behind)
        const uint32_t unit = unit_of(ri.form);
        bool writes = false;
        const RunInfo table = bands_for(c, ri, unit, true, &writes);
        if (writes) {
            // (already there if the count was enqueued by the upload and the expectation — units of 256 triangles — held)
            if (!(counted && c->warm_spec_unit == unit && c->warm_spec_shift == table.shift)) {
                launch_unit_bases(c->d_cnt, c->d_partials, sc.n_tri, unit, table.shift, table.out, st);
                const uint32_t n_units = band_workgroups(c, unit);
                launch_run_order(table.out, n_runs(n_units, table.shift), c->lane[0].total, c->d_run_order, run_order_slots(n_units, table.shift),
                                 c->d_run_rank, st);
                HIPCHK(c, hipGetLastError());
                HIPCHK(c, hipStreamSynchronize(st));
            }
            c->run_order_unit = unit; c->run_order_shift = table.shift;
            ri.bands_ready = true; ri.bands_unit = unit;
        }
    }
    // allocations a first conversion would otherwise make inside its own call; best effort (the conversion reports a failure).
    // Only for a caller that has said at which R it is about to convert (m2s_set_resolution_hint: the command line, the drop-in
    // ConversionPass, the reference's load-then-convert flow) or whose context already owns a record pool: a context that only ever
    // converts into its caller's buffers (m2s_convert_into: the ranks of a multi-GPU job) does not carry 600 MB it never uses.
    const uint64_t want = cap ? cap : std::max<uint64_t>(total, 1);
    if (c->hint_R != 0 || c->lane[0].records) {
        if (!single || total >= 8ull * sc.n_tri) (void)ensure_lane(c, 0, true, emit2_slices(std::min<uint64_t>(cap ? cap : want, 0xFFFFFFFFull)));
        // (touching the pool here does not pay: a hipMemset of the part the first conversion writes made that conversion 0.014 ms
        //  SLOWER on config 3, 0.185 vs 0.171 ms — profiles/r04/first_call_probe.jsonl)
        (void)ensure_records(c, want);
    }
    c->err.clear();
    return M2S_OK;
}
}  // namespace m2s_host

// Multi-pass pipeline: handles every triangle size, output-balanced (m2s_emit2.hip): k_count_scan (count + offsets + per-triangle
// setup records, one kernel) -> k_emit2 (wave-granular).

namespace m2s_host {
// What lane L needs before a conversion is enqueued on it.  Lane 0 has its stream, its chain and (ensure_records) its record pool;
// lane 1 gets them at its first use — the record buffer follows the pool's capacity, and one that has become too small is replaced
// after every conversion still writing it has finished.  multipass: and the lane's work set for n_start slices.  With a work set per
// lane, k_count_scan of one conversion runs beside k_emit2 of the previous one.
m2s_status ensure_lane(m2s_ctx* c, int L, bool multipass, uint32_t n_start) {
    Lane& ln = c->lane[L];
    const Lane& l0 = c->lane[0];
    const uint32_t n_tri = c->scene.n_tri;
    bool fresh = false;
    if (L) {
        M2S_TRY(c->streams.ensure(c->err, L));
        ln.stream = c->streams[L];
        const size_t words = std::max<size_t>(c->chain_words, 1);
        M2S_TRY(ln.chain_own.reserve(c->err, words, sizeof(unsigned long long), &fresh));
        ln.chain = ln.chain_own;
        if (fresh) HIPCHK(c, hipMemsetAsync(ln.chain, 0, words * sizeof(unsigned long long), ln.stream));
        if (ln.records.cap() < l0.records.cap()) {
            drain_in_flight(c, L);
            M2S_TRY(ln.records.reserve(c->err, l0.records.cap(), sizeof(m2s_gaussian)));
            ++ln.rec_gen;
        }
    }
    if (!multipass) return M2S_OK;
    if (L) {   // (lane 0's offsets are the arena's)
        M2S_TRY(ln.off_own.reserve(c->err, std::max<size_t>(n_tri, 1) + 1, sizeof(uint32_t)));
        ln.off = ln.off_own;
    }
    // A slice table that is too small is replaced by one of at least twice its size, at least lane 0's and at least 16384 slices,
    // after its readers have finished: lane 0's are whatever is in flight (synchronous conversions use it), lane 1's its own slots
    uint64_t slices = ln.start.cap();
    if (slices < n_start) {
        drain_in_flight(c, L ? L : -1);
        slices = std::max<uint64_t>(std::max<uint64_t>(n_start, 2 * slices), std::max<uint64_t>(l0.start.cap(), 16384));
    }
    M2S_TRY(ln.reserve_work(c->err, slices, setup_bytes(n_tri), &fresh));
    if (fresh) {   // the tall-triangle table's slot counter
        HIPCHK(c, hipMemsetAsync((char*)ln.setup.get() + setup_tall_offset(n_tri), 0, 16, ln.stream));
        HIPCHK(c, hipStreamSynchronize(ln.stream));
    }
    return M2S_OK;
}

// enqueues the pipeline's kernels on `st` in lane L's work set, the counter written to *h_res (pinned) by k_count_scan's last
// workgroup itself; no synchronisation.  marks: the conversion clock's where the caller reads its times (lane 0, synchronous), else none
m2s_status enqueue_multipass(m2s_ctx* c, int L, uint32_t R, float4* d_out, uint64_t limit, const StageMarks& marks, unsigned long long* h_res, hipStream_t st) {
    const SceneDev& sc = c->scene;
    const Lane& ln = c->lane[L];
    uint32_t epoch;
    HIPCHK(c, next_epoch(c, &epoch));
    HIPCHK(c, marks.mark((int)ConvMark::Count, st));
    launch_count_scan(sc, R, ln.off, ln.start, emit2_slices(limit), ln.chain, epoch, ln.total, ln.setup, reinterpret_cast<uint32_t*>(&h_res[1]),
                      &h_res[0], st);
    HIPCHK(c, marks.mark((int)ConvMark::Counted, st)); HIPCHK(c, marks.mark((int)ConvMark::Emit, st));
    launch_emit2(sc, R, ln.off, ln.start, ln.total, limit, ln.setup, d_out, st);
    HIPCHK(c, marks.mark((int)ConvMark::Emitted, st));
    HIPCHK(c, hipGetLastError());
    return M2S_OK;
}
}  // namespace m2s_host

static m2s_status run_multipass(m2s_ctx* c, uint32_t R, float4* d_out, uint64_t limit, hipStream_t st) {
    M2S_TRY(ensure_lane(c, 0, true, emit2_slices(limit)));
    c->h_total[0] = 0; c->h_total[1] = 0;
    M2S_TRY(enqueue_multipass(c, 0, R, d_out, limit, c->conv_clock.marks(), c->h_total, st));
    HIPCHK(c, wait_stream(st));  // glFinish + counter read-back (ConversionPass.cpp:54-59)
    if (c->h_total[1] >> 32) return fail(c, M2S_ERR_HIP, "multi-pass pipeline: look-back chain timed out");
    HIPCHK(c, c->conv_clock.span(ConvMark::Count, ConvMark::Counted, &c->last_ms[M2S_K_COUNT]));
    HIPCHK(c, c->conv_clock.span(ConvMark::Emit, ConvMark::Emitted, &c->last_ms[M2S_K_EMIT]));
    return M2S_OK;
}

namespace m2s_host {
m2s_status run_pass(m2s_ctx* c, uint32_t R, void* d_user, uint64_t user_cap, hipStream_t st, uint64_t* out_total,
                           bool from_submit) {
    if (!c->has_scene) return fail(c, M2S_ERR_STATE, "m2s_upload_scene has not been called");
    if (c->slot_count && !from_submit)
        return fail(c, M2S_ERR_STATE, "conversions submitted with m2s_convert_submit are still in flight: m2s_convert_wait first");
    if (R == 0 || R > 4096) return fail(c, M2S_ERR_INVALID, "R must be in [1, 4096]");
    HIPCHK(c, hipSetDevice(c->device));
    // A synchronous conversion shares the work buffers (chain, counts, offsets, deferred-triangle list) with whatever
    // was submitted before it, possibly on other streams: let that finish first.
    if (from_submit) drain_in_flight(c);
    const SceneDev& sc = c->scene;
    const uint64_t cap = resolve_cap(c, R);
    ClockOf<ConvMark>& clock = c->conv_clock;
    M2S_TRY(clock.begin(c->err, c->profiling));
    c->conversion_started(R);
    memset(c->last_ms, 0, sizeof c->last_ms);

    if (sc.n_tri == 0) {
        if (!d_user && !c->lane[0].records) {   // (an empty shard is a conversion like any other: its consumers see zero records, not "no conversion")
            const m2s_status s = ensure_records(c, 1);
            if (s != M2S_OK) return s;
        }
        c->conversion_finished(d_user ? d_user : c->lane[0].records.get(), 0, 0);
        if (out_total) *out_total = 0;
        return M2S_OK;
    }
    m2s_ctx::RInfo& ri = rinfo_for(c, R);

    // ---- which form for this scene at this R (decide; AUTO: from the fragment count)? -------------------
    // The fragment count of a scene is proportional to R^2 (window coordinates scale with R), so the ONE exact count
    // m2s_upload_scene took (warm_scene) decides for every R without touching the device: the threshold is not sharp, and
    // all pipelines produce the same bytes anyway.
    if (c->frag_per_R2 < 0.0) {   // only with the debug switch M2S_NO_WARM (round 3's behaviour: the analysis inside the first conversion)
        const m2s_status s = warm_scene(c, R);
        if (s != M2S_OK) return s;
    }
    const double predicted = c->frag_per_R2 * (double)R * (double)R;
    if (ri.form == M2S_PIPELINE_AUTO) decide(c, ri, predicted, R);

    // ---- where do the records go, and how many may be stored? ------------------------------------
    uint64_t limit;
    float4* d_out;
    if (d_user) {
        limit = cap ? std::min(cap, user_cap) : user_cap;
        d_out = (float4*)d_user;
    } else {
        // unlimited policy: room for the predicted count plus slack; a conversion that still overflows is repeated below
        const uint64_t want = cap ? cap : (uint64_t)(predicted * 1.02) + 4096;
        const m2s_status s = ensure_records(c, want);
        if (s != M2S_OK) return s;
        limit = cap ? cap : c->lane[0].records.cap();
        d_out = (float4*)c->lane[0].records.get();
    }
    if (limit > 0xFFFFFFFFull) limit = 0xFFFFFFFFull;

    bool wrote_plane = false;      // the last single-pass launch also wrote the position plane (k_sparse, m2s_set_keep_positions)
    bool grown = false;
    // ---- run: one launch of ri.form per pass.  Trouble moves ri.form down the ladder (demote) and the next pass runs that.  At
    // most nine passes: a repeat after a run-table mismatch (once per context), sparse -> lean -> team -> multi-pass, and those
    // four again after the pool has grown.
    for (int pass = 0;; ++pass) {
        if (pass == 9) return fail(c, M2S_ERR_STATE, "conversion pass: no pipeline settled");
        if (ri.form == M2S_PIPELINE_MULTIPASS) {
            const m2s_status s = run_multipass(c, R, d_out, limit, st);
            if (s != M2S_OK) return s;
            ri.mp_ready = true;
            c->last_pipeline = M2S_PIPELINE_MULTIPASS;
        } else {
            // single-pass kernel; triangles too large for its in-workgroup budget are only counted.
            // No memset, no memcpy: the look-back chain is epoch-tagged and the kernel writes the fragment
            // counter and its two status words straight into pinned host memory.
            c->h_total[0] = 0;
            c->h_total[1] = 0;
            uint32_t epoch;
            HIPCHK(c, next_epoch(c, &epoch));
            HIPCHK(c, clock.mark(ConvMark::Fused, st));
            const uint32_t unit = unit_of(ri.form);
            bool wrote_bands = false;
            const RunInfo runs = bands_for(c, ri, unit, true, &wrote_bands);
            // m2s_set_keep_positions: the sparse kernel — the one that runs on scenes of tens of millions of records, where a depth sort
            // is worth preparing for — also writes the records' positions as a 16-byte plane (the context's, grown here if need be)
            float4* plane = nullptr;
            if (ri.form == M2S_PIPELINE_SPARSE && c->keep_positions && st == c->stream) {
                (void)c->d_pos_plane.try_reserve(limit, 16);
                c->pos_plane_tag.clear();
                plane = c->d_pos_plane;
            }
            wrote_plane = plane != nullptr;
            launch_single(c, ri, R, c->lane[0].chain, limit, d_out, c->h_total, epoch, runs, st, plane);
            HIPCHK(c, clock.mark(ConvMark::FusedEnd, st));
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, wait_stream(st));  // glFinish + counter read-back (ConversionPass.cpp:54-59)
            HIPCHK(c, clock.span(ConvMark::Fused, ConvMark::FusedEnd, &c->last_ms[M2S_K_FUSED]));
            const uint32_t any_big = (uint32_t)(c->h_total[1] & 0xFFFFFFFFull);
            const uint32_t err = (uint32_t)(c->h_total[1] >> 32);
            c->last_pipeline = ri.form;
            if (!err && wrote_bands) { ri.bands_ready = true; ri.bands_unit = unit; }
            // A launch in runs trusts the run table: at the R the scene was counted at (warm_scene), that table comes from k_count's
            // counts, not from a launch of this kernel.  The two must agree on every triangle; if the totals ever differ, the table is
            // dropped and the conversion repeated in plain order (until now only the parity tests guarded this)
            if (runs.base && !err && R == c->warm_R && c->h_total[0] != c->warm_total && !c->warm_mismatch_seen) {
                c->warm_mismatch_seen = true;
                ri.bands_ready = false;
                if (debug_on("M2S_DEBUG")) fprintf(stderr, "[m2s] run table of R = %u disagrees with the launch (%llu vs %llu fragments): repeated without runs\n",
                                                   R, (unsigned long long)c->warm_total, (unsigned long long)c->h_total[0]);
                HIPCHK(c, hipMemsetAsync(c->d_bigmeta, 0, 4 * sizeof(uint32_t), st));
                continue;
            }
            // a clean single-kernel conversion: the same scene at the same R can be submitted asynchronously from now on
            ri.async_ok = !err && !any_big;
            if (err) {
                if (debug_on("M2S_DEBUG")) fprintf(stderr, "[m2s] single-pass kernel (form %d) reported 0x%x at R = %u: trying the next form\n", ri.form, err, R);
                demote(c, ri, R, (err & 0xFu) == 2u ? Trouble::full : Trouble::stalled);
                HIPCHK(c, hipMemsetAsync(c->d_bigmeta, 0, 4 * sizeof(uint32_t), st));   // forget what the aborted launch listed
                continue;
            }
            if (any_big) {
                uint32_t meta[4] = { 0, 0, 0, 0 };
                if (ri.form == M2S_PIPELINE_LEAN && c->pipeline == M2S_PIPELINE_AUTO) {
                    // k_fused3 shades only triangles of at most 8 x 8 pixels itself.  A few deferred ones are what k_emit_big is for;
                    // MANY mean the scene at this R belongs to k_fused2
                    HIPCHK(c, hipMemcpyAsync(meta, c->d_bigmeta, sizeof meta, hipMemcpyDeviceToHost, st));
                    HIPCHK(c, hipStreamSynchronize(st));
                    if (meta[0] > 64u && (uint64_t)meta[0] * 256u > sc.n_tri) {
                        demote(c, ri, R, Trouble::lean_defers);
                        HIPCHK(c, hipMemsetAsync(c->d_bigmeta, 0, sizeof meta, st));
                        continue;
                    }
                }
                HIPCHK(c, hipMemcpyAsync(meta, c->d_bigmeta, sizeof meta, hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
                HIPCHK(c, hipMemsetAsync(c->d_bigmeta, 0, sizeof meta, st));   // restore the "zero between conversions" invariant
                if (meta[0] > 256 && (uint64_t)meta[2] * 8 > c->h_total[0]) {
                    // Scene dominated by mid-size / big triangles (e.g. a coarse mesh at high density): the output-partitioned
                    // multi-pass pipeline packs them densely
                    demote(c, ri, R, Trouble::big_share);
                    continue;
                }
                // second stage: emit exactly the deferred triangles, one workgroup per 1024-fragment chunk
                HIPCHK(c, clock.mark(ConvMark::Emit, st));
                launch_emit_big(sc, R, c->d_biglist, meta[0], meta[1], limit, d_out, st);
                HIPCHK(c, clock.mark(ConvMark::Emitted, st));
                HIPCHK(c, hipGetLastError());
                HIPCHK(c, hipStreamSynchronize(st));
                HIPCHK(c, clock.span(ConvMark::Emit, ConvMark::Emitted, &c->last_ms[M2S_K_EMIT]));
            }
        }
        // unlimited policy, context-owned buffer: the prediction was too low — make room for the exact count and repeat
        // (never seen with the 2 % slack; the fragment count scales with R^2 up to clipping at the viewport edge)
        if (!d_user && !cap && c->h_total[0] > limit && limit < 0xFFFFFFFFull && !grown) {
            const m2s_status s = ensure_records(c, c->h_total[0]);
            if (s != M2S_OK) return s;
            limit = std::min<uint64_t>(c->lane[0].records.cap(), 0xFFFFFFFFull);
            d_out = (float4*)c->lane[0].records.get();
            grown = true;
            continue;
        }
        break;
    }
    const uint64_t total = c->h_total[0];
    if (total > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 fragments: offsets are 32-bit");
    c->frag_per_R2 = (double)total / ((double)R * (double)R);
    c->conversion_finished(d_out, total, std::min(total, limit));
    // the plane is these records' if the sparse kernel wrote every one of them (no deferred triangle went to k_emit_big, no fallback ran)
    if (wrote_plane && c->last_pipeline == M2S_PIPELINE_SPARSE && !c->h_total[1] && c->d_pos_plane) c->pos_plane_tag.set(*c, c->last_stored);
    if (!d_user && c->lane[0].rec_R != R) { c->lane[0].rec_R = R; ++c->lane[0].rec_gen; }
    if (out_total) *out_total = total;
    return M2S_OK;
}
}  // namespace m2s_host

extern "C" {

m2s_status m2s_convert(m2s_ctx* c, uint32_t R, uint64_t* out_total) {
    if (!c) return M2S_ERR_INVALID;
    return run_pass(c, R, nullptr, 0, c->stream, out_total);
}

m2s_status m2s_convert_into(m2s_ctx* c, uint32_t R, void* d_records, uint64_t capacity_records, void* hip_stream,
                            uint64_t* out_total) {
    if (!c) return M2S_ERR_INVALID;
    if (!d_records && capacity_records) return fail(c, M2S_ERR_INVALID, "d_records is NULL");
    if (!d_records) return fail(c, M2S_ERR_INVALID, "d_records is NULL (use m2s_convert for the context-owned buffer)");
    return run_pass(c, R, d_records, capacity_records, (hipStream_t)hip_stream, out_total);
}

}  // extern "C"
