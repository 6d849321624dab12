// m2s_device.h — device-side data layout and launcher prototypes (internal; the public
// boundary is include/m2s.h).  gfx950 only.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "m2s_stageclock.h"   // StageMarks: what the launchers that time their own stages record through
#include "m2s_vtable.h"

namespace m2s {
using m2s_host::StageMarks;

// Debug / A-B switches of the library (M2S_NO_BANDS, M2S_NO_LEAN, M2S_NO_WARM, ...) exist only in a DEBUG BUILD (`make EXTRA=-DM2S_DEBUG_BUILD
// OUT=../_build_debug`: what tools/first_call_probe.py, tools/mp_probe.py and the A/B scripts under tools/ab/ load through M2S_LIB_PATH), and
// even there they are only looked at when M2S_DEBUG is set in the environment.  In the library that ships every debug_on() is the constant
// false: the conversion path reads no environment and carries no switch (round 6).
#ifdef M2S_DEBUG_BUILD
inline const char* debug_env(const char* name) {
    static const bool enabled = std::getenv("M2S_DEBUG") != nullptr;
    return enabled ? std::getenv(name) : nullptr;
}
#else
inline const char* debug_env(const char*) { return nullptr; }
#endif
inline bool debug_on(const char* name) { const char* v = debug_env(name); return v && *v && *v != '0'; }

// ---- launch geometry ----------------------------------------------------------------------
constexpr int kBlock = 256;              // 4 wave64 per workgroup
constexpr int kTriPerBlock = 1024;       // triangles per workgroup in the upload's count kernel
constexpr int kEmitF = 1024;             // output records per workgroup of k_emit_big
constexpr int kRowsThread = 32;          // k_emit2: triangles with more pixel rows are expanded wave-cooperatively
constexpr int kRowsCount = 128;          // k_count: triangles with more pixel rows are counted wave-cooperatively
constexpr int kStageStride = 7;          // float4 per staged record in LDS (6 + 1 pad: conflict-free b128)

// ---- HBM layout of the geometry: 144 B / triangle in 11 coalescable planes ------------------
// (reference VBO: 17 floats/vertex AoS with 5 dead floats, SceneManager.cpp:483-512)
struct TriPlanes {
    const float4* A0;  // p0.x p0.y p0.z p1.x
    const float4* A1;  // p1.y p1.z p2.x p2.y
    const float*  A2;  // p2.z
    const float4* B0;  // uv0.x uv0.y uv1.x uv1.y
    const float2* B1;  // uv2.x uv2.y
    const float4* C0;  // n0.x n0.y n0.z n1.x
    const float4* C1;  // n1.y n1.z n2.x n2.y
    const float*  C2;  // n2.z
    const float4* D0;  // tangent 0 (xyz w)
    const float4* D1;  // tangent 1
    const float4* D2;  // tangent 2
};

struct TexDesc {
    const uint32_t* texels;  // RGBA8 mip chain, level 0 first; nullptr = map absent
    uint32_t w, h, n_levels;
    uint32_t off[5];         // level offsets in texels
};

// per-mesh "uniforms" (ConversionPass.cpp:77-112)
// "Combo" texture: when the three maps of a material exist and have identical dimensions their texels
// are interleaved — texel (i,j) of level l is the 12-byte triple {albedo, normal, metallic-roughness}
// at combo + coff[l] + (j*(W_l+1) + i)*3 dwords, and every row carries one extra wrapped texel
// (column W_l == column 0).  A bilinear footprint of ALL THREE maps is then two contiguous 24-byte
// row reads instead of twelve scattered 4-byte gathers.
struct ComboDesc {
    const uint32_t* texels;  // nullptr = not available (fallback: the separate maps)
    uint32_t coff[5];        // level offsets in dwords
};

struct MeshParams {
    float bmin[3];
    float bmax[3];
    float color[4];
    TexDesc tex[3];
    ComboDesc combo;
};

// One triangle deferred by the fused kernel (too large for its in-workgroup budget): emitted by k_emit_big.
struct BigItem {
    uint32_t t, cnt;           // local triangle index, fragment count
    unsigned long long off;    // index of its first record in the canonically ordered output
};

struct SceneDev {
    TriPlanes tri;
    const MeshParams* meshes;
    const uint32_t* mesh_first;  // n_meshes+1 prefix of GLOBAL triangle indices
    const uint2* mesh_of8;       // per 8 local triangles: {mesh of local triangle 8k, local index one past that mesh's last
                                 // triangle}: ONE scalar load tells a wave / workgroup its mesh and whether its range lies
                                 // inside it (round 3; before: a binary search over mesh_first = log2(meshes) + 1 dependent
                                 // scalar loads in front of every batch's position loads)
    uint32_t n_meshes;
    uint32_t n_tri;              // triangles resident on this device (the shard)
    uint32_t tri_first;          // global index of local triangle 0
};

// ---- launchers (all asynchronous on `st`) ----------------------------------------------------
void launch_repack(const float* d_aos, uint32_t stride_floats, uint32_t n_tri_src, uint32_t src_first,
                   uint32_t n, uint32_t dst_first, TriPlanes dst /*non-const view*/, hipStream_t st);
void launch_mesh_table(const SceneDev& sc, uint2* table, hipStream_t st);   // fills mesh_of8 (ceil(n_tri / 8) entries)
void launch_mip_level(const uint32_t* src, uint32_t sw, uint32_t sh, uint32_t* dst, uint32_t dw, uint32_t dh,
                      hipStream_t st);
void launch_combo_level(const uint32_t* a, const uint32_t* n, const uint32_t* m, uint32_t w, uint32_t h, uint32_t* dst,
                        hipStream_t st);
void launch_count(const SceneDev& sc, uint32_t R, uint32_t* cnt, uint32_t* partials, hipStream_t st);
void launch_scan_partials(uint32_t* partials, uint32_t n_partials, unsigned long long* total, hipStream_t st);
// *out (zero before) += fragments of the triangles with more than `threshold` fragments (cnt: launch_count's counts)
void launch_big_share(const uint32_t* cnt, uint32_t n_tri, uint32_t threshold, unsigned long long* out, hipStream_t st);
// where the output of every RUN (1 << shift units of `unit` = 256 / 512 triangles) starts, from launch_count's counts and the
// scanned partial sums: the table a launch in runs reads (RunInfo::base)
void launch_unit_bases(const uint32_t* cnt, const uint32_t* partials, uint32_t n_tri, uint32_t unit, uint32_t shift, unsigned long long* run_base, hipStream_t st);
// Dispatch order of the runs of a launch in runs: order[slot] = run.  A launch lasts until its last workgroup has finished; in mesh
// order the units dispatched last are as heavy as any (config 3: 9 ... 1592 fragments per unit), so the GPU drains for a whole heavy
// workgroup's lifetime.  Slot s is dispatched on XCD s % 8: the runs are dealt to the eight XCD queues so that the queues hold equal
// numbers of fragments, and every queue holds its heaviest runs first — the light runs last, a short drain, on every XCD at about the
// same time (m2s_run_balance.h).  Runs are independent (the look-back chain restarts at every run, whose base comes from the table),
// so any order is correct.
// n_slots = runs rounded up to whole groups of eight (slots past the last run map to themselves: their workgroups exit at once).
// scratch: run_order_scratch_bytes(n_slots) bytes of device memory (the runs' costs and ids in rank order).
void launch_run_order(const unsigned long long* run_base, uint32_t n_runs, const unsigned long long* total, uint32_t* order, uint32_t n_slots,
                      void* scratch, hipStream_t st);
// workgroups of `kernel` (of `threads` threads, no dynamic LDS) the current device holds at once: occupancy per CU x CUs; 0 if unknown
inline uint32_t resident_workgroups(const void* kernel, int threads) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || cus <= 0 || per_cu <= 0) {
        (void)hipGetLastError();
        return 0u;
    }
    return (uint32_t)per_cu * (uint32_t)cus;
}
uint32_t fused2_resident_workgroups();
uint32_t fused3_resident_workgroups();
uint32_t sparse_resident_workgroups();
inline uint32_t run_order_slots(uint32_t n_units, uint32_t shift) { return ((n_units + (8u << shift) - 1u) / (8u << shift)) * 8u; }
inline size_t run_order_scratch_bytes(uint32_t n_slots) { return (size_t)n_slots * (sizeof(unsigned long long) + sizeof(uint32_t)); }
// multi-pass pipeline (m2s_emit2.hip): count + scan + offsets in one kernel, wave-granular emit
uint32_t emit2_slices(uint64_t limit);       // entries of start[] needed for `limit` output records
uint32_t count_scan_blocks(uint32_t n_tri);  // chain words k_count_scan uses
size_t setup_bytes(uint32_t n_tri);          // per-triangle TriSetup array + the tall-triangle table behind it
size_t setup_tall_offset(uint32_t n_tri);    // where that table's 16-byte header starts (zero when the buffer is allocated)
// total_host (pinned, may be nullptr): the last workgroup also stores the fragment counter there
void launch_count_scan(const SceneDev& sc, uint32_t R, uint32_t* off, uint32_t* start, uint32_t n_start, unsigned long long* chain,
                       uint32_t epoch, unsigned long long* total, void* setup, uint32_t* status, unsigned long long* total_host, hipStream_t st);
void launch_emit2(const SceneDev& sc, uint32_t R, const uint32_t* off, const uint32_t* start, const unsigned long long* total,
                  uint64_t limit, const void* setup, float4* out, hipStream_t st);

// device-side .ply row encoder, formats 1 and 2 (m2s_export.hip)
void launch_encode_rows(const float4* rec, uint64_t n, uint32_t format, float scale_multiplier, uint8_t* out, hipStream_t st);

// XCD runs of k_fused2 / k_sparse.  Hardware workgroup h runs on XCD h % 8 and every XCD has a private L2: consecutive units
// (workgroups' worth of triangles: neighbours on the mesh, neighbouring texels) should meet in ONE L2.  A launch "in runs" gives
// XCD x the runs x, x + 8, x + 16, ... of `1 << shift` consecutive units each; the look-back chain restarts at every run, whose
// first unit reads where the run's output starts from a table (`base`) — so a unit still only waits for units dispatched before
// it (its own run's), whatever the other XCDs are doing.  The table is a by-product: a launch WITHOUT runs (plain order, one
// chain) stores where every run's output starts (`out`), and so does the exact count m2s_upload_scene takes (k_unit_bases); the
// next launches of the scene at that R read it.  No counting pass, no host round trip, no picker kernel.
// (Rounds 1-3 cut the unit list into EIGHT contiguous bands of equal estimated work, one per XCD.  A launch then lasted as long as
// its slowest band — the linear work model left the XCDs' finishing times 4-9 % apart — and as wide as its widest; the cuts had to
// travel to the host.  With runs every XCD gets work until the end; how much work depends on which runs it gets.  In mesh order ~15
// runs per XCD leave the heaviest XCD of config 3 2.1 % above the mean; sorted by weight and dealt round-robin, as rounds 7-11 shipped
// it, XCD 0 got the heaviest run of every group of eight and XCD 7 the lightest: 5.1 % above, 8.8 % between them.  launch_run_order
// deals the sorted runs by weight instead: 2.1 % above the mean, the bound that 123 runs of 32 units allow (tools/xcd_balance.py).)
struct RunInfo {
    const unsigned long long* base;  // launch in runs: base[j] = record index at which the output of run j starts; else nullptr
    unsigned long long* out;         // launch without runs: out[j] = the same, recorded for the next launches (or nullptr)
    uint32_t shift;                  // log2 of the run length in units
    const uint32_t* order;           // launch in runs: dispatch slot -> run (equal work per XCD queue, heaviest runs first: launch_run_order); nullptr: identity
};
// run length for a scene of n_units units (0: too few units for runs to make sense — plain order): 32 units (8192 triangles of
// k_fused2) where that still leaves every XCD four runs, else 16 or 8.  Measured on config 3 (3916 units), kernel time / read
// traffic: runs of 8 / 16 / 32 / 64 units 0.117-0.118 / 0.120 / 0.118-0.119 / 0.124-0.125 ms, eight equal-work bands 0.118-0.119
// (profiles/r04/ab_xcd_runs_vs_equal_work_bands.log); longer runs keep more neighbours in one L2 (fewer texel re-reads), shorter
// ones even the XCDs' work out.
inline uint32_t run_shift_for(uint32_t n_units) {
    if (const char* v = debug_env("M2S_RUN_SHIFT")) { const uint32_t s = (uint32_t)std::atoi(v) & 15u; return n_units >= (32u << s) ? s : 0u; }   // debug: A/B
    for (uint32_t shift = 5; shift >= 3; --shift)
        if (n_units >= (32u << shift)) return shift;      // at least four runs per XCD
    return 0u;
}
inline uint32_t n_runs(uint32_t n_units, uint32_t shift) { return (n_units + (1u << shift) - 1u) >> shift; }
// Work-balanced batches of k_fused2 for scenes that one generation of workgroups converts (fewer than ~172 k triangles): batch b
// = triangles [first[b], first[b + 1]), at most 64, starts at multiples of 8.  first == nullptr: uniform batches of fused_tpw.
struct BatchTable {
    const uint32_t* first;   // device, n + 1 entries
    uint32_t n;
    uint32_t tpw;            // k_fused2 only, first == nullptr: uniform batches of this many triangles instead of fused_tpw (0: fused_tpw);
                             // a multiple of 8, at most 64 — AUTO's choice for scenes of 11-18 fragments per triangle (run_pass: decide)
};
// units (workgroups of 256 triangles) of k_fused2 for a scene of n_tri triangles that can be converted in runs (0: too small for
// 64-triangle batches)
uint32_t fused2_band_workgroups(uint32_t n_tri);
void launch_fused2(const SceneDev& sc, uint32_t R, unsigned long long* chain, uint64_t limit, float4* out,
                   unsigned long long* total, uint32_t* status, uint32_t epoch, BigItem* biglist, uint32_t* bigmeta,
                   const RunInfo& runs, const BatchTable& batches, hipStream_t st);
// lean form of the team kernel (m2s_fused3.hip): same units, same run tables, same output; only for scenes whose meshes all sample
// a combo texture or no map at all (m2s_ctx::lean_ok); triangles larger than an 8 x 8 pixel box are deferred to k_emit_big.
// vt (or nullptr): the scene's vertex table (m2s_vtable.h) — the indexed instance runs, whose strips gather from it instead of the planes
// gp (or nullptr): the scene's geometry planes — the kGeo instance runs, whose triangle phase reads them instead of the positions
struct GeoPlanes {               // per resident triangle, built once per upload (m2s_geoplanes.hip)
    const float4* G0;            // Quaternion (w, x, y, z)
    const float4* G1;            // Scale.x, Scale.y, ou[0], ov[0]   (Geo::ou / ov: geo_setup's box-normalised orthogonal UVs)
    const float4* G2;            // ou[1], ov[1], ou[2], ov[2]
};
void launch_geo_planes(const SceneDev& sc, float4* g0, float4* g1, float4* g2, hipStream_t st);   // n_tri entries each; needs mesh_of8
void launch_fused3(const SceneDev& sc, uint32_t R, unsigned long long* chain, uint64_t limit, float4* out,
                   unsigned long long* total, uint32_t* status, uint32_t epoch, BigItem* biglist, uint32_t* bigmeta,
                   const RunInfo& runs, const BatchTable& batches, hipStream_t st, const VtxTable* vt = nullptr,
                   const GeoPlanes* gp = nullptr);
// sparse form of the single-pass kernel (m2s_sparse.hip); `runs` as for launch_fused2, in ITS units (512 triangles)
// plane (or nullptr): the positions of the records as a compact plane (16 B each, record order): what a depth sort builds its keys from
void launch_sparse(const SceneDev& sc, uint32_t R, unsigned long long* chain, uint64_t limit, float4* out,
                   unsigned long long* total, uint32_t* status, uint32_t epoch, BigItem* biglist, uint32_t* bigmeta,
                   const RunInfo& runs, hipStream_t st, float4* plane = nullptr);
bool sparse_supported(uint32_t n_tri);
uint32_t sparse_workgroups(uint32_t n_tri);   // workgroups of kSpCand = 512 triangles
constexpr uint32_t kSparseTrianglesPerWorkgroup = 512;
void launch_emit_big(const SceneDev& sc, uint32_t R, const BigItem* biglist, uint32_t n_big, uint32_t max_cnt, uint64_t limit,
                     float4* out, hipStream_t st);

// ---- viewer prepass (m2s_prepass.hip) --------------------------------------------------------------------------
// kernel-side uniforms: the shader's uniforms plus its per-dispatch invariants, prepared by prepass_prepare()
struct PrepassK {
    float M[16], V[16], P[16];   // u_modelToWorld, u_worldToView, u_viewToClip (column-major)
    float MinvT[16];             // transpose(inverse(u_modelToWorld))
    float mr_inv[9];             // inverse(mat3(u_modelToWorld)), [col*3 + row]
    float ms2[3];                // (modelScale * modelScale)
    float res[2], near_far[2], std_dev;
    int32_t render_mode;
    uint32_t format, ply_has_pbr, depth_test, arrival_order;
    const float* depth;          // device pointer (window-space depth, row 0 = bottom) or nullptr
    uint32_t depth_w, depth_h;
    uint32_t global_w;           // width in invocations of the reference's dispatch (gl_GlobalInvocationID of a linear index)
};
}  // namespace m2s
struct m2s_prepass_params;
namespace m2s {
void prepass_prepare(const m2s_prepass_params& p, uint64_t n, PrepassK* out);
// perm (or nullptr): record index of every position — the prepass then reads record perm[i] at position i (m2s_prepass_sorted);
// dense: every one of the n positions passed the frustum test (the sort in front applied it): written at its own position, no append;
// status[1] = 2 when one of them fails the prepass's last test (lambda2 < 0) — the output is then to be discarded and the frame repeated compacting
hipError_t launch_prepass(const PrepassK& k, const float4* rec, uint32_t n, float4* quads, float* depths, unsigned long long* chain,
                          uint32_t epoch, unsigned long long* counter, unsigned long long* total, uint32_t* status, hipStream_t st,
                          const uint32_t* perm = nullptr, bool dense = false, uint32_t* sources = nullptr);

size_t sort_prepass_temp_bytes(uint32_t n);
hipError_t sort_prepass(const float* depths, const float4* quads, uint32_t n, uint32_t* keys_out, uint32_t* vals_out, void* temp,
                        size_t temp_bytes, float4* sorted, hipStream_t st);
size_t sort_temp_bytes(uint32_t n);
// *key_offset_out (may be NULL: then keys_out is made whole before returning): keys_out holds `key - offset` (the sort ran over the bits in
// which the keys differ); launch_add_to_keys puts it back.  marks: 0..3 around keys | radix sort | gather
hipError_t sort_by_depth(const float4* rec, uint32_t n, const float view[16], uint32_t* keys_in, uint32_t* keys_out, uint32_t* vals_out,
                         void* temp, size_t temp_bytes, float4* sorted, float4* plane, bool plane_valid, const StageMarks& marks, hipStream_t st,
                         uint32_t* key_offset_out, uint32_t* pinned_mm /* two pinned host words for the key range, or NULL */);
void launch_add_to_keys(uint32_t* keys, uint32_t n, uint32_t offset, hipStream_t st);
// keys = the depth bits the PREPASS stores (model, view as in PrepassK), stable radix sort, no gather: vals_out = the permutation
// cull: the prepass's frustum test applied to the keys (survivors first: *n_visible of them; *clash: call again without cull); pinned_mm4: FOUR words
// marks: 0..2 around keys | radix sort
hipError_t sort_prepass_permutation(const float4* rec, uint32_t n, const float model[16], const float view[16], const float proj[16], bool cull,
                                    uint32_t* keys_in, uint32_t* keys_out, uint32_t* vals_out, void* temp, size_t temp_bytes, float4* plane, bool plane_valid,
                                    const StageMarks& marks, hipStream_t st, uint32_t* pinned_mm4, uint32_t* n_visible, bool* clash);

// ---- splat pass (m2s_splat.hip): GaussianSplattingPass over sorted quads into the five-target G-buffer ---------------------------
constexpr int kSplatTile = 16;                 // tiles of 16 x 16 pixels, one workgroup (one lane per pixel) each
constexpr size_t kSplatRecBytes = 128;         // compact per-quad record written by the setup kernel
size_t splat_scan_temp_bytes(uint32_t n);
size_t splat_sort_temp_bytes(uint32_t pairs, uint32_t n_tiles);
// setup: records, per-quad tile counts, their exclusive scan; totals[0] = (tile, quad) pairs, totals[1] += skipped quads
hipError_t splat_setup(const float4* quads, uint32_t n, int W, int H, float4* rec, uint32_t* cnt, unsigned long long* off, void* temp,
                       size_t temp_bytes, unsigned long long* totals, hipStream_t st);
hipError_t splat_pairs(const float4* rec, const uint32_t* cnt, const unsigned long long* off, uint32_t n, int tiles_x, uint32_t* keys,
                       uint32_t* vals, hipStream_t st);
// stable grouping of the pairs by tile, every tile's [start, end), the tiles ordered by list length (longest first)
hipError_t splat_group(uint32_t* keys_in, uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, uint32_t pairs, uint32_t n_tiles,
                       uint2* ranges, uint32_t* len, uint32_t* len_sorted, uint32_t* order, void* temp, size_t temp_bytes, hipStream_t st);
// ranges / order NULL: every tile empty (cleared planes); frag_count (or NULL) += fragments blended
hipError_t splat_blend(const float4* rec, const uint32_t* vals, const uint2* ranges, const uint32_t* order, int W, int H, int render_mode,
                       void* const planes[5], unsigned long long* frag_count, hipStream_t st);
hipError_t preload_splat();

// ---- contribution pass and pruning (m2s_contrib.hip) -----------------------------------------------------------------------------
// k_splat_contrib over the records / pairs / ranges / order of the splat pass's binning stages (splat_setup .. splat_group): per record
// sources[quad], wmax (bits of the largest fragment weight, integer max) and npix (fragments with weight > count_weight, integer sum)
hipError_t contrib_blend(const float4* rec, const uint32_t* vals, const uint2* ranges, const uint32_t* order, int W, int H,
                         const uint32_t* sources, float count_weight, uint32_t* wmax, uint32_t* npix, hipStream_t st);
size_t prune_scan_temp_bytes(uint32_t n);
// flags[i] = wmax[i] > min_weight && npix[i] >= min_pixels; counters[0] += dropped by weight, [1] += dropped by pixels alone (zeroed by
// the caller); offsets = exclusive scan of the flags
hipError_t prune_flags_scan(const uint32_t* wmax, const uint32_t* npix, uint32_t n, float min_weight, uint32_t min_pixels, uint32_t* flags,
                            uint32_t* offsets, unsigned long long* counters, void* temp, size_t temp_bytes, hipStream_t st);
// rows of f4_per_row float4 each: row i of src goes to row offsets[i] of dst where flags[i] is set; 16 bytes per lane
hipError_t prune_compact(const float4* src, const uint32_t* flags, const uint32_t* offsets, uint32_t n, uint32_t f4_per_row, float4* dst,
                         hipStream_t st);

// ---- pruning to a budget (m2s_budget.hip): a radix select over one 32-bit key per record --------------------------------------------
// The select's words on the device: the candidates (kBudgetShards partial counts), then — once the candidates exceed the budget — the
// digits of T found so far, the quota still to fill (after the last round: how many of the records with key == T are kept), 1 once T is
// complete, the candidates with key == T; then per round kBudgetShards copies of its 256 bins.  The shards are summed by their readers.
constexpr uint32_t kBudgetShards = 4;      // (a power of two)
constexpr uint32_t kBudgetCandidates = 0, kBudgetPrefix = 4, kBudgetQuota = 5, kBudgetActive = 6, kBudgetTies = 7, kBudgetHist = 8;
constexpr uint32_t kBudgetStateWords = kBudgetHist + 4 * kBudgetShards * 256;
// keys (importance 0: from wmax / npix and m2s_prune's thresholds; 1: from rec, the accumulators are not read), the four histogram /
// pick rounds, mark 0; tie flags, their ranks, keep flags, offsets = exclusive scan of the keep flags, mark 1.
// keys, flags, offsets: n words each; state: kBudgetStateWords; temp: prune_scan_temp_bytes(n).  budget >= 1, n > 0.
hipError_t budget_select(const float4* rec, const uint32_t* wmax, const uint32_t* npix, uint32_t n, uint32_t importance, float min_weight,
                         uint32_t min_pixels, uint32_t budget, uint32_t* keys, uint32_t* state, uint32_t* flags, uint32_t* offsets, void* temp,
                         size_t temp_bytes, const StageMarks& marks, hipStream_t st);
hipError_t preload_budget();

// ---- colour refit (m2s_refit.hip) --------------------------------------------------------------------------------------------------
// k_splat_refit over the records / pairs / ranges / order of the splat pass's binning stages, one workgroup per tile of the W x H
// viewport (vals / ranges / order NULL: no pairs, the participating pixels are still counted): per record sources[quad],
// num[3 r + k] += wq * eq_k and den[r] += wq over the fragments on participating pixels; *pixels += participating pixels
hipError_t refit_blend(const float4* rec, const uint32_t* vals, const uint2* ranges, const uint32_t* order, int W, int H,
                       const uint32_t* sources, const uint32_t* target, const uint32_t* render, uint32_t min_cover, long long* num,
                       unsigned long long* den, unsigned long long* pixels, hipStream_t st);
// k_refit_apply, one lane per 96-byte record: the pinned update of color[0..2] where den >= max(D, 1);
// counters[0] += updated, [1] += updated with a channel clamped, [2] += left for lack of weight (zeroed by the caller)
hipError_t refit_apply(float4* records, const long long* num, const unsigned long long* den, uint32_t n, double step, unsigned long long D,
                       unsigned long long* counters, hipStream_t st);

// ---- merge pass (m2s_merge.hip): runs and segments over the compact export's sorted order, one parent per segment --------------------
constexpr uint32_t kMergeTotalsWords = 2;  // segments, segments of two members or more
size_t merge_scan_temp_bytes(uint32_t n);
// keys / perm: the sorted keys and the permutation of compact_keys_and_sort (n words each).  flag, run_start: n words each, packed,
// sums: n 64-bit words each of work area; seg_start: n + 1 words, afterwards the first sorted position of every segment and n behind
// the last; totals: kMergeTotalsWords; temp: merge_scan_temp_bytes(n).  level 0..10, max_group >= 1, n > 0.  unsigned_axis: the
// M2S_MERGE_UNSIGNED_AXIS instances of k_merge_heads / k_merge_reduce (pins 2u, 5u), here and in merge_reduce.  gauss: the heads of
// pin 2g (M2S_MERGE_MODEL_GAUSSIAN), whatever unsigned_axis says.
hipError_t merge_segments(const float4* rec, const uint32_t* keys, const uint32_t* perm, uint32_t n, uint32_t level, uint32_t max_group, float min_axis_dot,
                          uint32_t* flag, uint32_t* run_start, unsigned long long* packed, unsigned long long* sums, uint32_t* seg_start, uint32_t* totals,
                          void* temp, size_t temp_bytes, bool unsigned_axis, bool gauss, hipStream_t st);
// k_merge_reduce, one lane per segment: out[s] = the parent of segment s (a copy of its member where it has one), map[i] = s for every
// member i.  out: `segments` records, not the memory rec points into; map: n words.
hipError_t merge_reduce(const float4* rec, const uint32_t* perm, const uint32_t* seg_start, const uint32_t* totals, uint32_t segments, float4* out,
                        uint32_t* map, bool unsigned_axis, hipStream_t st);
// k_merge_reduce_gauss (pins 4, 5g), as merge_reduce under M2S_MERGE_MODEL_GAUSSIAN; sigma: m2s_merge_sigma, finite and > 0
hipError_t merge_reduce_gauss(const float4* rec, const uint32_t* perm, const uint32_t* seg_start, const uint32_t* totals, uint32_t segments, float sigma,
                              float4* out, uint32_t* map, hipStream_t st);
// k_merge_reduce_sh (pin 5s; gauss: the weights of pin 5sg), one lane per (segment, float4 column) of the SH plane: out row s = the weighted mean of the members' rows
// of sh (a copy where it has one member).  sh: n rows of 48 floats; out: `segments` rows, not the memory sh points into.
constexpr uint32_t kMergeShLanes = 12;     // float4 per row of the plane
hipError_t merge_reduce_sh(const float4* rec, const float4* sh, const uint32_t* perm, const uint32_t* seg_start, const uint32_t* totals, uint32_t segments,
                           float4* out, bool gauss, hipStream_t st);

// ---- level-of-detail tree and its cut (m2s_lod.hip) ------------------------------------------------------------------------------------
// k_lod_link.  parent[t] = offset + map[t] for t < n_map (map NULL: M2S_LOD_NO_PARENT, the last level); bounds[t] = (position.xyz,
// fmaxf(|scale[0]|, |scale[1]|)) of rec[t] for t < n_rec.  parent, rec and bounds point at the first node they concern.
// gauss (pin 4g): the bound's fourth float is sigma * fmaxf(fmaxf(|scale[0]|, |scale[1]|), |scale[2]|) (k_lod_link_gauss); sigma is not read otherwise.
hipError_t lod_link(const uint32_t* map, uint32_t n_map, uint32_t offset, uint32_t* parent, const float4* rec, uint32_t n_rec, float4* bounds,
                    bool gauss, float sigma, hipStream_t st);
struct LodSelectK { float cx, cy, cz, focal, tau2, near2; };
// What a launcher that goes through the tree level by level reads of it (LodTree::levels_k, m2s_lodtree.h): the bound and the parent
// word of every node, the first node of every level ([levels]: the nodes; host memory), the levels.
struct LodLevelsK { const float4* bounds; const uint32_t* parent; const uint64_t* first; uint32_t levels; };
constexpr uint32_t kLodRefineWord = 17;    // counts: [l] selected nodes of level l (0..16), [17] nodes that refine,
constexpr uint32_t kLodPlainWord = 18;     // [18] nodes the cut selects before the visibility plane masks it (written with a plane only),
constexpr uint32_t kLodInsideWord = 19;    // [19] leaves inside the frustum (written by lod_visibility),
constexpr uint32_t kLodOccludedWord = 20;  // [20] of those, the leaves an occluder's depth image hides, [21] of those inside, the leaves behind
constexpr uint32_t kLodKeptWord = 21;      // the image that stay for their alpha (both written by lod_visibility with an occluder only: the three are neighbours)
constexpr uint32_t kLodCountWords = 22;
// The sweep, one launch per level from the last to the leaves: per node of [first[l], first[l + 1]) the pinned comparison,
// open[i] = refine && open[parent[i]] (levels above the leaves), flags[i] = selected; counts (zeroed by the caller) as above.
// vis (NULL: none): the visibility plane of lod_visibility; flags[i] = selected && vis[i] then, and the per-level counts are the masked ones.
hipError_t lod_sweep(const LodLevelsK& t, const LodSelectK& k, uint8_t* open, uint32_t* flags, uint32_t* counts, const uint8_t* vis, hipStream_t st);
// ids[offsets[i]] = i where flags[i] is set
hipError_t lod_node_ids(const uint32_t* flags, const uint32_t* offsets, uint32_t n, uint32_t* ids, hipStream_t st);
// offsets = exclusive scan of flags (n words each); temp: prune_scan_temp_bytes(n)
hipError_t lod_scan(const uint32_t* flags, uint32_t* offsets, uint32_t n, void* temp, size_t temp_bytes, hipStream_t st);

// ---- the cut that fits a record budget (m2s_lodbudget.hip): a radix descent over two 32-bit key planes ---------------------------------
// The search's words on the device: the digits of the key found so far, the count at the key just under the prefix's range, the count at
// the key in front of the answer (written once a digit above 0 is chosen: the answer is not key 0); then per round kLodBudgetShards copies of 256 bins for L and 256 for H.
constexpr uint32_t kLodBudgetShards = 4;   // (a power of two)
constexpr uint32_t kLodBudgetPrefix = 0, kLodBudgetBelow = 1, kLodBudgetFiner = 2, kLodBudgetEff = 3, kLodBudgetHist = 4;
constexpr uint32_t kLodBudgetStateWords = kLodBudgetHist + 4 * kLodBudgetShards * 512;
// One launch per level from the last to the leaves: lh[i] = (L, H), the keys (bits of tau_px) from which node i is no longer refined
// (0 for a leaf) and from which one of its proper ancestors is not (0xFFFFFFFF on the last level); k.tau2 is not read.
// vis (NULL: none): the visibility plane of lod_visibility; a node whose byte is 0 gets L = H (selected at no key), H as without.
hipError_t lod_thresholds(const LodLevelsK& t, const LodSelectK& k, uint2* lh, const uint8_t* vis, hipStream_t st);
// The four histogram / pick rounds over the n nodes: afterwards state[kLodBudgetPrefix] is the smallest key whose cut holds at most
// `budget` nodes (budget >= the nodes of the last level, n > 0), state[kLodBudgetFiner] the count at the key before it where
// that key is not 0.  state: kLodBudgetStateWords, zeroed here.
// raise_to_last: the budget is raised on the device to count(0x7F7FFFFF), the nodes of the last level left with L < H, which the first
// round's sums hold (no key lies in 0x7F800000 .. 0x7FFFFFFF); state[kLodBudgetEff] keeps it.  For planes whose last level is masked.
hipError_t lod_budget_search(const uint2* lh, uint32_t n, uint32_t budget, bool raise_to_last, uint32_t* state, hipStream_t st);

// ---- the visibility plane of the frustum cuts (m2s_lodfrustum.hip) -----------------------------------------------------------------------
// The three matrices of m2s_prepass_params (column-major) and the guard band, as a kernel argument.
struct LodFrustumK { float M[16], V[16], P[16]; float guard; };
// The depth image behind m2s_lod_occluder, on the device: depth_w x depth_h floats, row 0 = bottom; the tree's node records (plane 0, 24
// floats each), whose color[3] the test reads; the bias of the comparison.
struct LodOccluderK { const float* depth; const float* nodes; uint32_t depth_w, depth_h; float bias; };
// vis: one byte per node.  Zeroes them (stream-ordered memset), then one launch per level from the leaves up to the level below the last
// (one launch for a tree of one level): vis[i] = 1 for a leaf whose position passes the prepass's frustum test with this guard band, and
// for every node with a visible child; the leaves that pass are added to *inside_word (zeroed by the caller).
// occ (NULL: none): a leaf that passes the frustum test, lies behind the image by more than the bias and has alpha > .95 is not
// visible; inside_word[0] counts the leaves that pass the frustum test all the same, inside_word[1] the ones hidden, inside_word[2]
// the ones behind the image that stay (kLodInsideWord, kLodOccludedWord, kLodKeptWord).
hipError_t lod_visibility(const LodLevelsK& t, const LodFrustumK& f, const LodOccluderK* occ, uint8_t* vis, uint32_t* inside_word, hipStream_t st);

// ---- the blend of a cut's records towards their parents (m2s_lodblend.hip; the pin: include/m2s.h, m2s_lod_blend) -----------------------
struct LodBlendK { float cx, cy, cz, focal, tau2, near2, band; };
constexpr uint32_t kLodBlendBlended = 0, kLodBlendSaturated = 1, kLodBlendTurned = 2, kLodBlendCountWords = 3;
// k_lod_blend_t: t[j] for the n records whose nodes are ids[j] (pin 2); counts[kLodBlendBlended] += #{t > 0},
// counts[kLodBlendSaturated] += #{t == 1} (zeroed by the caller).
hipError_t lod_blend_weights(const uint32_t* ids, const uint32_t* parent, const float4* bounds, uint32_t n, const LodBlendK& k, float* t,
                             uint32_t* counts, hipStream_t st);
// k_lod_blend: out[j] = node ids[j] of `nodes` at weight 1 - t[j], its parent at t[j] (pins 3 to 5); counts[kLodBlendTurned] +=
// #{t > 0, k != 0}.  out: n records, not memory `nodes` points into.
hipError_t lod_blend_records(const float4* nodes, const uint32_t* ids, const uint32_t* parent, const float* t, uint32_t n, float4* out,
                             uint32_t* counts, hipStream_t st);
// k_lod_blend_sh: the same for the rows of the SH plane (pin 6).  out: n rows of 48 floats, not memory `sh` points into.
hipError_t lod_blend_sh(const float4* sh, const uint32_t* ids, const uint32_t* parent, const float* t, uint32_t n, float4* out, hipStream_t st);

// ---- world units (m2s_worldunits.hip) ------------------------------------------------------------------------------------------------
// dst[i] = src[i] with scale[0..2] divided by (float)R (IEEE, correctly rounded), every other word with its bits, for the n records.
// src == dst: in place, only the scale words move; else the two do not overlap.  R >= 1.
hipError_t world_units(const float4* src, float4* dst, uint32_t n, uint32_t R, hipStream_t st);

// ---- shadow and relighting passes (m2s_light.hip): GaussianShadowPass + GaussianRelightingPass ---------------------------------------
struct ShadowBases { uint32_t b[7]; };         // first quad of every face's list in the one buffer that holds the six lists; b[6] = all quads
struct RelightK {                              // uniforms of gaussianSplattingDeferredPS.glsl
    float light[3], cam[3], color[3];
    float intensity, far_plane;
    int32_t mode, W, H, S;
};
inline uint32_t shadow_blocks(uint32_t n) { return (n + 255u) / 256u; }   // workgroups of stage A; its tables hold 6 * blocks + 1 words
size_t shadow_temp_bytes(uint32_t n_words, uint32_t n_quads, uint32_t pairs);
// stage A, first half: per (face, workgroup) survivor counts, their exclusive scan (off), bases[7] (device)
hipError_t shadow_count(const PrepassK& k, const float* views, const float light[3], const float4* rec, uint32_t n, uint32_t* cnt, uint32_t* off,
                        void* temp, size_t temp_bytes, uint32_t* bases, hipStream_t st);
// ... second half: the 48-byte quads, every face's list in input order
hipError_t shadow_emit(const PrepassK& k, const float* views, const float light[3], const float4* rec, uint32_t n, const uint32_t* off, float4* quads,
                       hipStream_t st);
// stage B: per-quad records (48 B), tile counts and their scan; totals[0] = (tile, quad) pairs, totals[1] += skipped quads
hipError_t shadow_setup(const float4* quads, uint32_t n, const ShadowBases& fb, int S, const float light[3], float far_plane, float4* rec, uint32_t* cnt,
                        unsigned long long* off, void* temp, size_t temp_bytes, unsigned long long* totals, hipStream_t st);
hipError_t shadow_bin(const float4* rec, const uint32_t* cnt, const unsigned long long* off, uint32_t n, int S, uint32_t* keys_in, uint32_t* vals_in,
                      uint32_t* keys_out, uint32_t* vals_out, uint32_t pairs, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t shadow_clear(float* cube, int S, hipStream_t st);                      // every texel 1.0
hipError_t shadow_raster(const float4* rec, const uint32_t* keys, const uint32_t* vals, uint32_t pairs, int S, float* cube, unsigned long long* writes,
                         hipStream_t st);
// planes: the five G-buffer attachments (3, depth, is not read); counts (or NULL): the 20-tap shadow count per pixel
// left_planes (or NULL): split screen — pixels with x < split_x are lit from these planes, columns div_x and div_x + 1 are white
hipError_t launch_relight(const RelightK& k, const void* const planes[5], const float* cube, uint32_t* frame, uint8_t* counts, hipStream_t st,
                          const void* const left_planes[5] = nullptr, int split_x = 0, int div_x = 0);
hipError_t preload_light();

// ---- light baked into spherical harmonics (m2s_bake.hip): the deferred shader per Gaussian, projected onto the 16 harmonics of the .ply ----
struct BakeK {
    float M[16], MinvT[16];     // u_modelToWorld, transpose(inverse(u_modelToWorld)): PrepassK's
    float light[3], color[3];
    float intensity, far_plane;
    int32_t S;                  // side of a cube face (0 without shadows)
    uint32_t n_dirs;            // rows of the table: n_theta * n_phi
    uint32_t n_coef;            // (degree + 1)^2: coefficients kept per channel
    uint32_t use_shadows, viewer_metallic;
};
struct ShadeK { float M[16]; float cam[3]; };
constexpr int kBakeTableRow = 20;   // floats per direction: d.xyz, w, w * B_0..15
// plane: float[n][48] (f_dc[3], f_rest[45] channel-major); counts (or NULL): uint8[n], the 20-tap counts
hipError_t launch_bake_sh(const BakeK& k, const float4* rec, uint32_t n, const float* table, const float* cube, float* plane, uint8_t* counts,
                          hipStream_t st);
hipError_t launch_sh_shade(const ShadeK& k, const float4* rec, const float* sh, uint32_t n, float4* dst, hipStream_t st);

// ---- mesh depth prepass (m2s_meshdepth.hip): DepthPrepass over the uploaded scene's position planes -------------------------------
struct MeshDepthK {
    float PVM[16];      // (view_to_clip * world_to_view) * model_to_world, fp32 in glm's order (m2s_meshdepth.cpp), column-major
    int32_t W, H;
    int32_t inplace;    // an unclipped triangle whose pixel box is at most this many pixels wide AND high is covered by its own lane
};
constexpr int kMdInplace = 4;                  // the default of MeshDepthK::inplace
constexpr int kMdSlotsPerTriangle = 6;         // records (48 B) and tile counts per deferred triangle
size_t meshdepth_temp_bytes(uint32_t n_slots, uint32_t pairs);
hipError_t meshdepth_clear(float* image, int W, int H, hipStream_t st);        // every texel 1.0
// totals (zero before): [0] triangles drawn, [1] clipped, [2] non-finite, [3] (tile, piece) pairs, [4] texel updates sent, [5] deferred
hipError_t meshdepth_setup(const MeshDepthK& k, const SceneDev& sc, float* image, uint32_t* deferred, unsigned long long* totals, hipStream_t st);
hipError_t meshdepth_deferred(const MeshDepthK& k, const SceneDev& sc, const uint32_t* deferred, uint32_t nd, float4* rec, uint32_t* cnt,
                              unsigned long long* off, void* temp, size_t temp_bytes, unsigned long long* totals, hipStream_t st, bool vis = false);
hipError_t meshdepth_bin(const MeshDepthK& k, const float4* rec, const uint32_t* cnt, const unsigned long long* off, uint32_t nd, uint32_t* keys_in,
                         uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, uint32_t pairs, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t meshdepth_raster(const MeshDepthK& k, const float4* rec, const uint32_t* keys, const uint32_t* vals, uint32_t pairs, float* image,
                            unsigned long long* totals, hipStream_t st);
hipError_t preload_meshdepth();

// ---- mesh render pass (m2s_meshdepth.hip: the visibility stage, the k_md_* kernels with a 64-bit payload; m2s_meshrender.hip: shading)
// visibility image: per pixel (bits of z) << 32 | global triangle index, the minimum over the fragments that pass GL_LESS;
// cleared to (bits of 1.0f) << 32 | 0xFFFFFFFF.  totals as meshdepth_setup, and [6] triangles culled as back-facing; the binning
// (meshdepth_deferred with vis = true, meshdepth_bin) is the depth pass's.
hipError_t meshvis_clear(unsigned long long* image, int W, int H, hipStream_t st);
hipError_t meshvis_setup(const MeshDepthK& k, const SceneDev& sc, unsigned long long* image, uint32_t* deferred, unsigned long long* totals, hipStream_t st);
hipError_t meshvis_raster(const MeshDepthK& k, const float4* rec, const uint32_t* keys, const uint32_t* vals, uint32_t pairs, unsigned long long* image,
                          unsigned long long* totals, hipStream_t st);
struct MeshRenderK {                           // uniforms of meshRender{VS,PS}.glsl
    float PVM[16];      // MeshDepthK::PVM: the clip positions are the visibility stage's, bit for bit
    float M[16], V[16]; // u_modelToWorld, u_worldToView
    float N[9];         // mat3(transpose(inverse(M))), [col * 3 + row]: float64 on the host, rounded
    float near_far[2];
    int32_t W, H, mode;
};
// one lane per pixel of the visibility image -> the five planes (layouts of the splat G-buffer); an empty pixel gets zeros
hipError_t meshrender_shade(const MeshRenderK& k, const SceneDev& sc, const unsigned long long* vis, void* const planes[5], hipStream_t st);
hipError_t preload_meshrender();

// ---- fidelity score (m2s_score.hip): image B against image A, integer sums -----------------------------------------------------------
struct ScoreK {
    int32_t W, H;
    uint32_t mask_mode;     // 0 every pixel, 1 covered by A, 2 by A or B, 3 by A and B
    uint32_t tiles_x;       // workgroup tiles per row of tiles
};
constexpr int kScoreTileCells = 16;            // a workgroup's tile: 16 x 16 cells of 4 x 4 pixels (64 x 64 pixels) ...
constexpr int kScoreGridCells = 17;            // ... plus one cell of halo to the right and above, for the windows that start in its last column / row
constexpr int kScoreThreads = 320;             // one lane per cell of the 17 x 17 grid (289), rounded up to whole waves
// counters of one shard: [0] pixels, [1..4] cover, [5..7] sse, [8..10] sad, [11..13] max_abs, [14] windows, [15] ssim_q32 (two's complement)
constexpr int kScoreCounters = 16;
constexpr int kScoreMaxFirst = 11, kScoreMaxLast = 13;   // the counters combined by max instead of +
constexpr int kScoreShards = 32;               // workgroup b adds into shard b % 32: same-address atomics serialise, the host sums the shards
inline uint32_t score_tiles(int n) { return (uint32_t)((n + 4 * kScoreTileCells - 1) / (4 * kScoreTileCells)); }
// acc: kScoreShards * kScoreCounters words, zero before.  cover_a / cover_b NULL (both): the planes are not read, every pixel counts as
// covered by both.  map (or NULL): the error map.  Row loads are 16 bytes wide when W % 4 == 0 and every pointer is 16-byte aligned.
hipError_t launch_score(const ScoreK& k, const uint32_t* a, const uint32_t* b, const uint32_t* cover_a, const uint32_t* cover_b, uint32_t* map,
                        unsigned long long* acc, hipStream_t st);
hipError_t preload_score();

// ---- compact .ply export (m2s_compact.hip): validity + box, Morton keys, stable sort, chunk encoder -----------------------------------
inline uint32_t compact_waves(uint32_t n) { return (n + kBlock - 1) / kBlock * (kBlock / 64); }   // entries of the per-wave box table
size_t compact_sort_temp_bytes(uint32_t n);
// keys_in / vals_in / keys_out / vals_out: n words each; wave_box: compact_waves(n) * 8 words; head: 8 words, afterwards { min.xyz,
// max.xyz of the valid positions in the order of m2s_compactmath.h's ord(), N, skipped }; the first N words of vals_out: the permutation.
// marks: 0..2, around box + keys and around the sort.  n > 0.
hipError_t compact_keys_and_sort(const float4* rec, const float4* plane, uint32_t n, uint32_t* wave_box, uint32_t* head, uint32_t* keys_in, uint32_t* vals_in,
                                 uint32_t* keys_out, uint32_t* vals_out, void* temp, size_t temp_bytes, const StageMarks& marks, hipStream_t st);
// table: 18 floats per chunk; rows: N x 16 bytes; sh_out (K = 3 | 8 | 15): WHOLE chunks of 256 x 3 K bytes; sh: the baked plane or NULL
hipError_t compact_pack(const float4* rec, const float* sh, const uint32_t* perm, uint32_t N, float sm, uint32_t K, float* table, void* rows, void* sh_out,
                        hipStream_t st);

// sample sort across ranks (m2s_dist.cpp): evenly spaced samples of sorted keys; split points of sorted keys
void launch_pick_samples(const uint32_t* keys, uint64_t n, uint32_t s, unsigned long long* out, hipStream_t st);
void launch_lower_bounds(const uint32_t* keys, uint64_t n, const unsigned long long* splitters, uint32_t m, unsigned long long* out, hipStream_t st);

// The runtime loads a file's code object inside the first launch of one of its kernels (0.2-0.6 ms each: the first conversion of
// a PROCESS).  These make it happen now — hipFuncGetAttributes on one kernel of the file — without launching anything:
// m2s_upload_scene asks for the pipeline it has just decided on, m2s_prepare(M2S_PREPARE_KERNELS) for all of them.
hipError_t preload_fused2();
hipError_t preload_fused3();
hipError_t preload_sparse();
hipError_t preload_multipass();
void launch_scratch_warm(hipStream_t st);   // the queue's scratch memory set up now, not inside the first multi-pass conversion (m2s_emit2.hip)
hipError_t preload_export();
hipError_t preload_prepass();
hipError_t preload_sort();

inline uint32_t n_count_blocks(uint32_t n_tri) { return (n_tri + kTriPerBlock - 1) / kTriPerBlock; }
// fused kernel: triangles per wave.  64 as soon as that fills the GPU's 3072 wave slots once.  A smaller scene gets just
// enough triangles per wave to occupy every slot ONCE (one round of waves instead of two: the C2 stand-in, 69 312
// triangles, ran 16 per wave = 4332 waves = 1.4 rounds in round 1), in multiples of 8, at least 8.  With the slots
// filled, fewer triangles per wave only adds instructions (500 k triangles: 0.126 -> 0.156 ms at 32).
#ifndef M2S_TPW_SLOTS
#define M2S_TPW_SLOTS 3072u
#endif
inline uint32_t fused_tpw(uint32_t n_tri) {
    const uint32_t per = (n_tri + M2S_TPW_SLOTS - 1u) / M2S_TPW_SLOTS;
    const uint32_t r8 = (per + 7u) & ~7u;
    return r8 < 8u ? 8u : r8 > 64u ? 64u : r8;
}
inline uint32_t n_fused_waves(uint32_t n_tri) { const uint32_t w = fused_tpw(n_tri); return (n_tri + w - 1) / w; }
// entries (batches + 1) a BatchTable for n_tri triangles may need; 0: the scene takes uniform 64-triangle batches
// (room for one batch per wave slot of the lean kernel — 4096 — where that is more than one per wave of k_fused2)
inline uint32_t batch_table_capacity(uint32_t n_tri) { return fused_tpw(n_tri) < 64u ? (n_fused_waves(n_tri) > 4096u ? n_fused_waves(n_tri) : 4096u) + n_tri / 64u + 16u : 0u; }

}  // namespace m2s
