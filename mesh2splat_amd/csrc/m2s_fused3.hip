// m2s_fused3.hip — single-pass conversion kernel, the LEAN form of the team kernel (gfx950).
//
// k_fused2 (m2s_fused2.hip) is compiled for every scene the library accepts: triangles of up to 16 pixel rows expanded in the
// workgroup (a 30-register row walker), edge functions in 64 bits, three separately sized maps sampled in one round trip (75
// registers of taps and texels).  That generality is what its 157 vector registers — three waves per SIMD — pay for, and a
// scene like BASELINE config 3 uses none of it: every triangle fits an 8 x 8 pixel box, every material samples one interleaved
// ("combo") texture.  This file is the same protocol — one batch of triangles per wave, ONE entry stream per workgroup, strips
// of 64 fragments handed out by an LDS counter, one look-back per workgroup, records staged in LDS and written as coalesced
// non-temporal runs; the same bytes out — compiled for exactly that case:
//
//   * in the workgroup only triangles whose pixel box is at most 8 x 8 (coverage = one 64-bit mask); everything larger is
//     counted here (wave-cooperatively, one row per lane) and handed to k_emit_big through the deferred-triangle list, as
//     k_fused2 does with triangles of more than 16 rows.  The host uses this kernel only while such triangles are rare
//     (run_pass: a launch that deferred many switches the scene back to k_fused2 at that R);
//   * fragment constants as TriShadeS (64 B: 16-bit edge coefficients, 32-bit edge values — exact for such boxes), barycentrics
//     in 32-bit integers; entries are ONE byte (bit of the mask | first << 6, `first` = first fragment of its triangle): the owner
//     wave follows from the stream position, the triangle from the wave's prefix sums `cum` (below);
//   * only meshes that sample their combo texture or no map at all (decided at upload: SceneDev has no other mesh);
//   * fragment constants are computed and stored BEFORE the wave waits for anything: across the waits a lane keeps its mask,
//     its counts and its triangle index, nothing else; the strip loop re-reads the workgroup's protocol words from LDS;
//   * the texture coordinates a strip needs — (uv0, uv1 - uv0, uv2 - uv0) per triangle — are stored next to the fragment constants:
//     the triangle phase has the B planes in registers anyway, and a strip computes its texel addresses without a global round trip
//     in front of them (and without fetching the two planes a second time).
//
// Four instances (template <bool kIndexed, bool kGeo>; launch_fused3 picks by what the upload left: a vertex table, m2s_ctx::vt_use, and
// geometry planes, m2s_ctx::geo_use; one of them runs per scene).  kIndexed — where the STRIPS gather a triangle's attributes:
//   * k_fused3<false, *>, the plane instance: a strip gathers its triangle's positions, normals and tangents from the per-corner SoA planes
//     (A, C, D: 120 B per triangle, every vertex once per corner that uses it);
//   * k_fused3<true, *>, the indexed instance: the upload deduplicated the shard's corners into a table of distinct vertices (m2s_vdedup.hip;
//     rows of three float4: (p.xyz, u), (n.xyz, v), (t.xyzw); config 3: 501 128 rows for 3 006 756 corners) and left three row ids per
//     triangle, packed in 8 bytes (VtIds, m2s_vtable.h).  The triangle phase reads them with the B planes (one coalesced 8-byte load)
//     and stores them in the 8 bytes of the fragment constants that otherwise hold the combo texture's two level offsets (TriShadeSI:
//     the strips re-derive the offsets from the level nibbles in mesh[31:24] and the mesh's wave-uniform combo.coff[]); F3Lds does not
//     grow.  A strip then takes nine row loads through the ids it has in LDS — no dependent global read in front of them — in place of
//     the nine plane loads: the same operand bits from another address, the interpolation text unchanged, the records byte for byte
//     those of the plane instance.  Neighbouring triangles read the same rows, so a workgroup's gathers touch ~48 B per triangle
//     instead of 120.  k_emit_big (deferred triangles) and every other kernel read planes only.
// kGeo — what the TRIANGLE PHASE starts from:
//   * k_fused3<*, false>: the positions (planes A, 36 B per triangle) and the mesh's box: geo_setup (three roots, a reciprocal, two
//     normalisations, six quotients, the axis selection) in front of the raster setup, geo_flat (yAxis, quat_cast, the 2 x 2 inverse, the
//     Jacobian, two roots) for every covered triangle;
//   * k_fused3<*, true>: the scene's geometry planes (GeoPlanes, m2s_device.h; built once per upload by k_geo_planes, m2s_geoplanes.hip, with
//     the same device functions): three coalesced 16-byte loads per lane — Quaternion; Scale.xy, ou[0], ov[0]; ou[1], ov[1], ou[2], ov[2] —
//     in place of the A planes.  Geo::ou / ov are all raster_head and raster_setup read, Scale and Quaternion go unchanged into the
//     triangle's fragment constants; nothing of this depends on R.  The phase has no positions at all: neither geo_setup nor geo_flat
//     runs (static vector instructions of the indexed instance 2802 -> 1942), 48 B in for 36 B out per triangle.  The coordinates (planes
//     B), the ids, the raster setup, coverage, the levels of detail and everything behind the phase are the other instance's text; the
//     records are the same bytes (tests/test_gpu_fused3_geoplanes.py).  The kGeo = false instances are what runs when a scene has no
//     planes (more than 2^22 resident triangles, or no memory for them).
//
// LDS per workgroup (F3Lds, 40 824 of the 40 960 bytes that four workgroups per CU leave each):
//     tri      16 384   TriShadeS / TriShadeSI, [wave][lane]
//     uv        6 144   float2[3], [wave][lane]
//     tskip     1 024   [wave][lane]; read only by strips of a workgroup with deferred triangles
//     cum         512   uint16 [wave][slot]: inclusive prefix of the entry counts over the wave's COVERED triangles (slot = rank of the
//                       triangle among those with entries; unused slots hold 0xFFFF)
//     lane_of     256   uint8 [wave][slot]: the lane (triangle of the batch) of that slot
//     entries   4 096   one byte each
//     stage    12 288   32 records per wave
//     ctl         120
// Decoding a strip: for every owner wave in it, lane l reads cum[ow][l] and the wave ballots cum <= q0 (q0 = the strip's first
// position inside that wave's entries): the popcount is the slot at that position; a lane's slot is that plus the `first` flags
// between the wave's first lane in the strip and itself.
//
// kLeanWaves waves per SIMD (M2S_FUSED3_WAVES, default 4: 128 registers, 40 KB of LDS per workgroup).  Registers: this file is compiled with
// -fno-slp-vectorize (its Makefile rule): plain -O3 packs neighbouring f32 operations into v_pk_*_f32, which have no higher rate than the
// scalar forms on gfx950 and whose register pairs cost 14 registers and ~100 moves — both instances 110 -> 96 registers, no scratch, the
// same roundings per component (explicit fma_, contraction off); config 3: step about 2-3 % shorter at the same four workgroups per CU.
// Five workgroups per CU: 96 registers allow them, and a 32 768 B layout of the indexed instance (no uv: coordinates from the vertex
// rows; tskip inside the staging area; 3 200 entries) compiled without spills, got 5 from the occupancy query, and was no faster than
// the four-workgroup build beside it (0.0952 against 0.0948 ms) — but its wave cycles per kernel time were those of four workgroups,
// so nothing shows that a fifth was ever alive.  Not shipped, and not settled: DESIGN 6.3, profiles/r10.
// Measurement-only switches (compile time; the A/B tables of DESIGN 6): M2S_FUSED3_UV_GLOBAL — the strips load the B planes as they
// did before the coordinates moved to LDS; M2S_FUSED3_NT_ATTR — normals / tangents of the plane instance as non-temporal loads;
// M2S_FUSED3_TRI_PRIO — 0: every wave at one priority throughout, 2: phase classes (below), with M2S_FUSED3_PRIO_FLOOR.
//
// Priority.  A wave runs its triangle phase — no wait after its loads — at priority 1 and drops to 0 when
// its counts are published: the waits and the strips run at 0.  From the second generation of workgroups on, a wave in the triangle phase
// shares its SIMD with three waves in strips, which issue a few instructions between long waits; ahead of them it leaves the phase ~1 us
// sooner (mean 6.8 -> 5.7 us on config 3) and its workgroup's texel requests start that much earlier.  Priority only orders issue — nothing a
// workgroup writes, or where, depends on it.  Measured and NOT shipped: a priority per "phase class" of the workgroup
// (f3_class: which of the four dispatch slots of its CU it took), to make the waves of one SIMD leave the phase one after another — the
// first generation's triangle phase is not issue-bound (8 us at any priority), so the classes order nothing.
#include "m2s_fused_common.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace m2s {

#ifndef M2S_FUSED3_WAVES
#define M2S_FUSED3_WAVES 4                 // waves per SIMD the kernel is compiled for (= workgroups per CU)
#endif
#ifndef M2S_FUSED3_ENTRIES
#define M2S_FUSED3_ENTRIES 1024            // entry-stream capacity per wave of the team (x1 byte x 4 of LDS)
#endif
#ifndef M2S_FUSED3_STAGE
#define M2S_FUSED3_STAGE (M2S_FUSED3_WAVES >= 5 ? 16 : 32)   // records staged per wave and round (32 = half a strip)
#endif
constexpr int kL3Team = 4;                 // waves (= batches) per workgroup
constexpr int kL3Threads = kL3Team * 64;
constexpr uint32_t kL3Entries = (uint32_t)M2S_FUSED3_ENTRIES * kL3Team;
constexpr int kL3Stage = M2S_FUSED3_STAGE;
constexpr uint32_t kL3Wait = 1u << 24;     // LDS polls before giving up
constexpr uint32_t kL3Stop = 1u << 28;     // added to the strip counter by a wave that gives up: nobody draws a strip after that

struct F3Ctl {
    unsigned long long base;               // record index of stream position 0
    unsigned long long total_w[kL3Team];   // fragments (all kinds) per batch
    uint32_t total_c[kL3Team];             // entries per batch
    uint32_t counted[kL3Team];             // 1: total_w / total_c of that wave are valid
    uint32_t expanded[kL3Team];            // 1: that wave's TriShadeS, tskip and entries are in place
    uint32_t t0[kL3Team];                  // first triangle of each wave's batch
    uint32_t claimed;                      // next strip to hand out
    uint32_t base_state;                   // 0 unknown, 1 being resolved, 2 known
    uint32_t flags;                        // bits 0-7: error (1 a wait gave up, 2 entries do not fit); bit 8: deferred triangles
                                           // somewhere in this workgroup (record index != base + stream position after them)
    uint32_t pad_;
};
struct F3Lds {
    float4 tri[kL3Team][64 * 4];           // TriShadeS of the four batches
    uint32_t tskip[kL3Team][64];           // per triangle: (record index - stream position) of its fragments
    float2 uv[kL3Team][64 * 3];            // per triangle: uv0, uv1 - uv0, uv2 - uv0 (shade_from_tri's `uvl`)
    uint16_t cum[kL3Team][64];             // per slot (= covered triangle of the batch, in order): entries of the batch up to and with it
    uint8_t lane_of[kL3Team][64];          // per slot: its triangle's lane
    uint8_t entries[kL3Entries];           // bit of the 8 x 8 mask | first << 6  (the owning wave follows from the stream position)
    float4 stage[kL3Team][kL3Stage * 6];   // record staging, one per wave
    F3Ctl ctl;
};
static_assert(sizeof(F3Lds) * M2S_FUSED3_WAVES <= 163840, "M2S_FUSED3_WAVES workgroups per CU must fit the 160 KB of LDS");
static_assert((uint32_t)M2S_FUSED3_ENTRIES * kL3Team < 0xFFFFu && 64u * 64u < 0xFFFFu, "cum is 16 bits wide, 0xFFFF marks an unused slot");
#ifdef M2S_FUSED3_NT_ATTR
constexpr bool kF3StreamAttr = true;
#else
constexpr bool kF3StreamAttr = false;
#endif
constexpr uint32_t kF3Irregular = 1u << 8;
#ifndef M2S_FUSED3_TRI_PRIO
#define M2S_FUSED3_TRI_PRIO 1              // 1: the triangle phase at priority 1; 0: no priorities; 2: a priority per phase class (A/B)
#endif
#ifndef M2S_FUSED3_PRIO_FLOOR
#define M2S_FUSED3_PRIO_FLOOR 0            // phase classes: lowest priority of a triangle phase (classes at or below it share it)
#endif
// An XCD hands its workgroups (blockIdx.x >> 3 = 0, 1, 2, ...) to its 32 CUs in turn, so the workgroups that share a CU are 32 apart:
// the class is the index of that group of 32 — on a launch in runs of 32 units (config 3) the dispatch slot of the run.  (Timeline build:
// all 256 CUs of config 3's first generation hold four distinct classes.)
constexpr uint32_t kF3ClassShift = 5;
__device__ __forceinline__ uint32_t f3_class(uint32_t round) { return (round >> kF3ClassShift) & 3u; }

__device__ __forceinline__ uint32_t l3_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void l3_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
// a wave-uniform word, re-read where it is used (relaxed atomic: not hoisted out of the strip loop), into a scalar register
__device__ __forceinline__ uint32_t l3_uniform(const uint32_t* p) {
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
// a wave gives up: remember why, and stop the strip counter
__device__ __forceinline__ void l3_fail(F3Ctl& C, uint32_t why, int lane) {
    if (lane == 0) {
        __hip_atomic_fetch_or(&C.flags, why, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&C.claimed, kL3Stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// The workgroup's base: sum of the totals of all batches before its first one.  Whoever needs it first resolves it.
__device__ __forceinline__ bool f3_get_base(F3Ctl& C, unsigned long long* chain, uint32_t b0, int lane, uint32_t epoch, uint32_t* status,
                                            unsigned long long& base) {
    uint32_t st = l3_load(&C.base_state);
    if (st != 2) {
        uint32_t got = 1;
        if (lane == 0) {
            uint32_t expect = 0;
            got = __hip_atomic_compare_exchange_strong(&C.base_state, &expect, 1u, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) ? 0u : 1u;
        }
        got = __builtin_amdgcn_readfirstlane(got);
        if (got == 0) {   // this wave resolves
            const unsigned long long b = b0 == 0 ? 0ull : lookback(chain, b0, lane, epoch, status);
            if (lane == 0) {
                C.base = b;
                // the first batch's inclusive prefix: successors' look-backs stop here
                chain_store(&chain[b0], kFlagPrefix | ((unsigned long long)epoch << kEpochShift) | ((b + C.total_w[0]) & kValMask));
            }
            l3_store(&C.base_state, 2u);
        } else {
            uint32_t spins = 0;
            while (l3_load(&C.base_state) != 2) {
                if (++spins > kL3Wait) { l3_fail(C, 1u, lane); return false; }
                __builtin_amdgcn_s_sleep(2);
            }
        }
    }
    base = C.base;
    return true;
}

#ifdef M2S_TIMELINE
// measurement build only (tools/timeline_probe.py): 100 MHz timestamps per wave — start, counts known, entries expanded, first strip,
// last strip done, end — and the strips the wave shaded
__device__ unsigned long long g_tl_f3[16384 * 4 * 8];
constexpr int kTlHwId = 4 | (31 << 11);      // s_getreg operand: HW_REG_HW_ID, all 32 bits (wave 3:0, SIMD 5:4, CU 11:8, SH 12, SE 15:13)
constexpr int kTlXccId = 20 | (3 << 11);     // HW_REG_XCC_ID, bits 3:0
#define TLF(k) do { __builtin_amdgcn_sched_barrier(0); if (lane == 0 && blockIdx.x < 16384u) g_tl_f3[((size_t)blockIdx.x * 4 + wave) * 8 + (k)] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define TLFV(k, v) do { if (lane == 0 && blockIdx.x < 16384u) g_tl_f3[((size_t)blockIdx.x * 4 + wave) * 8 + (k)] = (v); } while (0)
#else
#define TLF(k) do { } while (0)
#define TLFV(k, v) do { } while (0)
#endif

struct VtNone { };   // the plane instance takes no table
struct GeoNone { };  // the instances that compute their geometry take no geometry planes
template <bool kIndexed, bool kGeo>
__global__ void __launch_bounds__(kL3Threads, M2S_FUSED3_WAVES) k_fused3(SceneDev sc, uint32_t R, unsigned long long* __restrict__ chain,
                                                      unsigned long long limit, float4* __restrict__ out,
                                                      unsigned long long* __restrict__ total_out,
                                                      uint32_t* __restrict__ status /* [0]=any big, [1]=error */, uint32_t epoch,
                                                      BigItem* __restrict__ biglist, uint32_t* __restrict__ bigmeta,
                                                      uint32_t tpw /* triangles per wave: 64 .. 8 (fused_tpw) */,
                                                      RunInfo runs, BatchTable bt,
                                                      std::conditional_t<kIndexed, VtxTable, VtNone> vt,
                                                      std::conditional_t<kGeo, GeoPlanes, GeoNone> gp) {
    using TS = std::conditional_t<kIndexed, TriShadeSI, TriShadeS>;   // what the strips read from S.tri
    __shared__ F3Lds S;
    F3Ctl& C = S.ctl;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // batches, units, XCD runs: exactly as in k_fused2 (the two kernels share the run tables of a scene)
    const uint32_t n_batches = bt.first ? bt.n : (sc.n_tri + tpw - 1u) / tpw;
    const uint32_t hb = blockIdx.x, xcd = hb & 7u, round = hb >> 3;
    const bool in_runs = runs.base != nullptr;
    const uint32_t rmask = (1u << runs.shift) - 1u;
    const unsigned long long etag = (unsigned long long)epoch << kEpochShift;
    uint32_t lb = hb;
    if (in_runs) {
        uint32_t rr = ((round >> runs.shift) << 3) + xcd;          // dispatch slot of the run ...
        if (runs.order) rr = ((const __attribute__((address_space(4))) uint32_t*)runs.order)[rr];   // ... heaviest runs first
        lb = (rr << runs.shift) + (round & rmask);
    }
    const bool band_first = in_runs && (round & rmask) == 0u;     // first unit of its run: its base is the run's, known
    if (lb * (uint32_t)kL3Team >= n_batches) return;
#if M2S_FUSED3_TRI_PRIO == 1
    __builtin_amdgcn_s_setprio(1);         // the triangle phase ahead of other waves' strips (file header)
#elif M2S_FUSED3_TRI_PRIO == 2
    switch (f3_class(round)) {             // (the priority is an immediate operand)
        case 0: __builtin_amdgcn_s_setprio(3); break;
        case 1: __builtin_amdgcn_s_setprio(2); break;
        case 2: __builtin_amdgcn_s_setprio(M2S_FUSED3_PRIO_FLOOR > 1 ? M2S_FUSED3_PRIO_FLOOR : 1); break;
        default: __builtin_amdgcn_s_setprio(M2S_FUSED3_PRIO_FLOOR); break;
    }
#endif
    TLF(0);
    // LDS is not zero on entry: one barrier at the very start makes the flags trustworthy (see k_fused2)
    if (lane == 0) { C.counted[wave] = 0; C.expanded[wave] = 0; }
    if (wave == 0 && lane == 0) {
        C.claimed = 0; C.flags = 0;
        C.base_state = (lb == 0 || band_first) ? 2u : 0u;
        C.base = band_first ? runs.base[lb >> runs.shift] : 0ull;
    }
    __syncthreads();
    const uint32_t b0 = lb * kL3Team;
    const uint32_t nb_here = min((uint32_t)kL3Team, n_batches - b0);
    const uint32_t b = b0 + wave;
    const bool has_batch = wave < nb_here;
    const unsigned long long band_base = band_first ? C.base : 0ull;

    // ======================= triangle phase: one batch per wave =======================
    uint32_t t0 = b * tpw, nt = tpw;
    if (bt.first && has_batch) {
        const __attribute__((address_space(4))) uint32_t* q = (const __attribute__((address_space(4))) uint32_t*)bt.first;
        t0 = q[b];
        nt = q[b + 1] - t0;
    }
    const uint32_t t = t0 + lane;
    const bool valid = has_batch && (uint32_t)lane < nt && t < sc.n_tri;
    if (lane == 0) C.t0[wave] = t0;        // (read by other waves only after this wave's `expanded` flag)
    int kind = kNone;
    unsigned long long mask = 0;
    uint32_t cnt = 0;
    {
        [[maybe_unused]] float p[9];   // (kGeo: no positions in the phase — g.ou / g.ov, Scale and Quaternion come from the geometry planes)
        Geo g;
        [[maybe_unused]] float4 grot = make_float4(0, 0, 0, 0);
        [[maybe_unused]] float gsx = 0, gsy = 0;
        RasterHead h;
        h.x0 = h.y0 = 0; h.x1 = h.y1 = -1; h.ext = 0;
        bool box = false;
        uint32_t m = 0;
        float4 uvb0 = make_float4(0, 0, 0, 0);
        float2 uvb1 = make_float2(0, 0);
        [[maybe_unused]] uint2 vid = make_uint2(0, 0);   // indexed: the triangle's three row ids, packed at upload (VtIds)
        bool uniform_mesh = false;     // the wave's batch lies inside one mesh (m0): mesh uniforms through scalar loads
        uint32_t m0 = 0;
        if (has_batch) {
            const uint32_t lastT = min(t0 + nt, sc.n_tri) - 1;
            m0 = mesh_of_range(sc, t0, lastT, uniform_mesh);
            m = m0;
            if (valid) {
                [[maybe_unused]] float4 q0, q1, q2;
                if constexpr (kGeo) { q0 = ld_plane(gp.G0, t); q1 = ld_plane(gp.G1, t); q2 = ld_plane(gp.G2, t); }
                else load_positions(sc.tri, t, p);
                uvb0 = sc.tri.B0[t];
                uvb1 = sc.tri.B1[t];
                if constexpr (kIndexed) vid = ld_plane(reinterpret_cast<const uint2*>(vt.ids), t);
                if constexpr (kGeo) {
                    grot = q0; gsx = q1.x; gsy = q1.y;
                    g.ou[0] = q1.z; g.ov[0] = q1.w; g.ou[1] = q2.x; g.ov[1] = q2.y; g.ou[2] = q2.z; g.ov[2] = q2.w;
                    if (!uniform_mesh) m = find_mesh(sc, sc.tri_first + t);
                }
                else if (uniform_mesh) geo_setup_mp(p, kConstMesh(sc.meshes + m0), g);
                else { m = find_mesh(sc, sc.tri_first + t); geo_setup_mp(p, sc.meshes + m, g); }
                box = raster_head(g, R, h);
            }
        }
        const int w = h.x1 - h.x0 + 1, rows = h.y1 - h.y0 + 1;
        // small: shaded in this workgroup, all of its integer setup in 32 bits (raster_small)
        RasterSmall rs;
        bool small = box && w <= 8 && rows <= 8 && h.ext <= 2304;
        if (small) small = raster_small(h, rs);
        else if (box) kind = kBig;         // (unless it has no area: decided where the wave counts it, below)
        {   // coverage of the small triangles, the wave walking rows and columns together (small_coverage, m2s_devfn.h)
            uint32_t mlo = 0, mhi = 0;
            small_coverage(small, w, rows, rs, mlo, mhi);
            mask = (unsigned long long)mlo | ((unsigned long long)mhi << 32);
            cnt = (uint32_t)__popc(mlo) + (uint32_t)__popc(mhi);
            if (small) kind = kSmall;
        }
        // fragment constants of the triangles this workgroup shades itself: in place before any wait (see the file header)
        if (cnt != 0 && kind == kSmall) {
            TriShadeS c;
            if (uniform_mesh) tri_shade_small<!kGeo>(p, g, h, rs, kConstMesh(sc.meshes + m0), uvb0, uvb1, m, c);
            else tri_shade_small<!kGeo>(p, g, h, rs, sc.meshes + m, uvb0, uvb1, m, c);
            if constexpr (kGeo) { c.sx = gsx; c.sy = gsy; c.rot = grot; }   // the upload's geo_flat (m2s_geoplanes.hip)
            const float4* src = reinterpret_cast<const float4*>(&c);
#pragma unroll
            for (int k = 0; k < 3; ++k) S.tri[wave][lane * 4 + k] = src[k];
            // (indexed: the ids take the place of the two level offsets, which the strips re-derive — TriShadeSI)
            if constexpr (kIndexed) S.tri[wave][lane * 4 + 3] = make_float4(__uint_as_float(vid.x), __uint_as_float(vid.y), src[3].z, src[3].w);
            else S.tri[wave][lane * 4 + 3] = src[3];
            // ... and its texture coordinates in the form the strips interpolate (the subtractions shade_from_tri would do itself)
            float2* const uvs = &S.uv[wave][lane * 3];
            uvs[0] = make_float2(uvb0.x, uvb0.y);
            uvs[1] = make_float2(uvb0.z - uvb0.x, uvb0.w - uvb0.y);
            uvs[2] = make_float2(uvb1.x - uvb0.x, uvb1.y - uvb0.y);
        }
        if (__ballot(kind == kBig) != 0ull) {   // larger triangles (rare): the whole wave counts one of them, a pixel row per lane
            // (inline on purpose: as a non-inlined function this path gave the kernel a stack — 64 bytes of scratch per lane — and the
            //  FIRST launch of a kernel that uses scratch pays the runtime's scratch allocation: first conversion 0.19 -> 0.31 ms)
            Raster rb;                           // their full (64-bit) setup, only here
            rb.x0 = rb.y0 = 0; rb.x1 = rb.y1 = -1; rb.ext = 0; rb.bias = 0; rb.area2 = 1;
#pragma unroll
            for (int i = 0; i < 3; i++) { rb.a[i] = rb.b[i] = 0; rb.c[i] = 0; }
            if (kind == kBig && !raster_setup(g, R, rb)) kind = kNone;
            unsigned long long bigm = __ballot(kind == kBig);
            while (bigm) {
                const int src = __ffsll((long long)bigm) - 1;
                bigm &= bigm - 1;
                const Raster br = shfl_raster(rb, src);
                uint32_t part = 0;
                for (int y = br.y0 + lane; y <= br.y1; y += 64) {
                    int xa, xb;
                    row_span(br, y, xa, xb);
                    part += (uint32_t)max(xb - xa + 1, 0);
                }
                part = wave_sum(part);
                if (lane == src) cnt = part;
            }
        }
    }
    if (cnt == 0) kind = kNone;
    const uint32_t cntc = kind == kSmall ? cnt : 0;
    const bool anybig = __ballot(kind == kBig) != 0ull;

    // (a triangle has at most 4096^2 = 2^24 fragments, so the wave's 64 counts sum to < 2^31: 32-bit scans)
    const uint32_t incl = wave_incl_scan(cnt, lane);
    const uint32_t inclc = wave_incl_scan(cntc, lane);
    const unsigned long long total_w = __builtin_amdgcn_readlane(incl, 63);
    const uint32_t total_c = __builtin_amdgcn_readlane(inclc, 63);
    const uint32_t toff = incl - cnt;
    const uint32_t ctoff = inclc - cntc;

    // publish: the chain word of this batch (global batch 0 and the first batch of a run know their prefix) and the counts
    if (has_batch && lane == 0) {
        const bool knows = b == 0 || (band_first && wave == 0);
        chain_store(&chain[b], (knows ? kFlagPrefix : kFlagAgg) | etag | (((knows ? band_base : 0ull) + total_w) & kValMask));
    }
    if (lane == 0) {
        C.total_w[wave] = total_w; C.total_c[wave] = total_c;
        // the "deferred triangles" flag travels WITH the counts (see k_fused2: a strip of another wave's entries must see it)
        if (anybig) __hip_atomic_fetch_or(&C.flags, kF3Irregular, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#if M2S_FUSED3_TRI_PRIO
    __builtin_amdgcn_s_setprio(0);         // the phase is over: the waits and the strips run at the common priority
#endif
    l3_store(&C.counted[wave], 1u);
    TLF(1);

    // ======================= where do my entries go?  counts of the waves before me =======================
    uint32_t stream0 = 0;              // stream position of my first entry
    unsigned long long out0 = 0;       // fragments (all kinds) of the batches before mine in this workgroup
    bool alive = true;
    for (uint32_t k = 0; k < wave && alive; ++k) {
        uint32_t spins = 0;
        while (l3_load(&C.counted[k]) == 0) {
            if (++spins > kL3Wait) { alive = false; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        stream0 += C.total_c[k];
        out0 += C.total_w[k];
    }
    if (!alive) l3_fail(C, 1u, lane);
    if (alive && (unsigned long long)stream0 + total_c > kL3Entries) {   // does not fit the LDS stream
        alive = false;
        l3_fail(C, 2u, lane);
    }
    // the look-back is taken by the LAST wave, before its own expansion: its entries are the last ones a strip asks for
    unsigned long long base = 0;
    bool have_base = false;
    if (alive && wave == (uint32_t)kL3Team - 1 && (l3_load(&C.flags) & 0xFFu) == 0) {
        have_base = f3_get_base(C, chain, b0, lane, epoch, status, base);
        if (!have_base) alive = false;
    }

    // ======================= my tskip and entries =======================
    if (alive) {
        if (cntc) S.tskip[wave][lane] = (uint32_t)((out0 + toff) - ((unsigned long long)stream0 + ctoff));
        {   // the wave's prefix sums over its covered triangles, and which lane each of them is
            const unsigned long long cov = __ballot(cntc != 0);
            const uint32_t ncov = (uint32_t)__popcll(cov);
            if ((uint32_t)lane >= ncov) S.cum[wave][lane] = 0xFFFFu;
            if (cntc) {
                const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(cov >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cov, 0u));
                S.cum[wave][slot] = (uint16_t)inclc;
                S.lane_of[wave][slot] = (uint8_t)lane;
            }
        }
        if (anybig) {   // deferred triangles: reserve their slice of the output, list them for k_emit_big
            unsigned long long bb;
            if (f3_get_base(C, chain, b0, lane, epoch, status, bb)) {
                if (kind == kBig) {
                    const uint32_t slot = atomicAdd(&bigmeta[0], 1u);
                    atomicMax(&bigmeta[1], cnt);
                    atomicAdd(&bigmeta[2], cnt);
                    BigItem it2;
                    it2.t = t; it2.cnt = cnt; it2.off = bb + out0 + toff;
                    biglist[slot] = it2;
                }
                if (lane == 0) __hip_atomic_store(&status[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            } else alive = false;
        }
        if (kind == kSmall) {
            unsigned long long mm = mask;
            uint32_t ci = stream0 + ctoff;
            uint32_t first = 64u;
            while (mm) {
                const int bit = __ffsll((long long)mm) - 1;
                mm &= mm - 1;
                S.entries[ci++] = (uint8_t)(first | (uint32_t)bit);
                first = 0u;
            }
        }
    }
    l3_store(&C.expanded[wave], 1u);   // release: TriShadeS, uv, tskip, cum, lane_of, entries (set even on error so that nobody waits for it)
    TLF(2);
    [[maybe_unused]] unsigned long long tl_strips = 0;

    // ======================= fragment phase: strips of the workgroup's stream =======================
    // the stream's length needs every wave's count
    for (uint32_t k = 0; k < (uint32_t)kL3Team && alive; ++k) {
        uint32_t spins = 0;
        while (l3_load(&C.counted[k]) == 0) {
            if (++spins > kL3Wait) { alive = false; l3_fail(C, 1u, lane); break; }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    float4* const stage = S.stage[wave];
    uint32_t exp_seen = 0;             // bit k: wave k's expansion has been seen (after that its flag is not polled again)
    TLF(3);
    while (alive) {
        uint32_t s = 0;
        if (lane == 0) s = __hip_atomic_fetch_add(&C.claimed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        s = __builtin_amdgcn_readfirstlane(s);
        // the workgroup's protocol words are re-read from LDS for every strip (wave-uniform: they live in scalar registers for the
        // length of one strip instead of in vector registers for the whole loop)
        const uint32_t c1 = l3_uniform(&C.total_c[0]), c2 = c1 + l3_uniform(&C.total_c[1]), c3 = c2 + l3_uniform(&C.total_c[2]),
                       stream_total = c3 + l3_uniform(&C.total_c[3]);
        const uint32_t pos0 = s * 64u;
        if (s >= kL3Stop / 64u || pos0 >= stream_total) break;
#ifdef M2S_TIMELINE
        ++tl_strips;
#endif
        const uint32_t n = min(64u, stream_total - pos0);
        const uint32_t lo[4] = { 0u, c1, c2, c3 }, hi[4] = { c1, c2, c3, stream_total };
        if (exp_seen != 15u) {   // the waves whose entries this strip contains must have expanded them
#pragma unroll
            for (int k = 0; k < kL3Team; ++k) {
                if ((exp_seen >> k) & 1u) continue;
                if (hi[k] <= pos0 || lo[k] >= pos0 + n) continue;
                uint32_t spins = 0;
                while (l3_load(&C.expanded[k]) == 0) {
                    if (++spins > kL3Wait) { alive = false; l3_fail(C, 1u, lane); break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                exp_seen |= 1u << k;
            }
            if (!alive) break;
        }
#ifdef M2S_FUSED3_PRIO
        __builtin_amdgcn_s_setprio(M2S_FUSED3_PRIO);       // A/B: the front of a strip (up to its texel requests) ahead of other waves' arithmetic
#endif
        const uint32_t pos = pos0 + (uint32_t)lane;
        const bool have = (uint32_t)lane < n;
        uint32_t en = 0;
        if (have) en = S.entries[pos];
        const uint32_t ow = (pos >= c1 ? 1u : 0u) + (pos >= c2 ? 1u : 0u) + (pos >= c3 ? 1u : 0u);   // owner wave of my entry
        const uint32_t bit = en & 63u;
        // my triangle: the slot at the strip's first position inside my owner wave's entries + the `first` flags from there to me
        uint32_t slot = 0;
        {
            const unsigned long long fm = __ballot(have && (en & 64u) != 0u);
#pragma unroll
            for (int k = 0; k < kL3Team; ++k) {
                if (hi[k] <= pos0 || lo[k] >= pos0 + n || hi[k] == lo[k]) continue;   // (wave-uniform)
                const uint32_t p0 = max(pos0, lo[k]);
                const uint32_t q0 = p0 - lo[k], sl = p0 - pos0;   // position in that wave's entries / lane of the strip
                const uint32_t s0 = (uint32_t)__popcll(__ballot((uint32_t)S.cum[k][lane] <= q0));
                const unsigned long long fk = fm & ~((2ull << sl) - 1ull);      // flags above the wave's first lane in the strip
                const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(fk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fk, 0u));
                if (ow == (uint32_t)k) slot = s0 + below + (uint32_t)((fk >> lane) & 1ull);
            }
        }
        uint32_t tl = 0;
        if (have) tl = S.lane_of[ow][slot & 63u] & 63u;
        float4 rec[6];
        // fragments of one strip almost always belong to one mesh; if not, the meshes take turns (every turn shades through a
        // wave-uniform descriptor: scalar loads, one instantiation of the shader)
        uint32_t my_mesh = 0;
        if (have) my_mesh = reinterpret_cast<const uint32_t*>(&S.tri[ow][tl * 4 + 3])[3] & 0xFFFFFFu;
        unsigned long long todo = __ballot(have);
        while (todo) {
            const uint32_t m_now = __builtin_amdgcn_readlane(my_mesh, __ffsll((long long)todo) - 1);
            const bool mine = have && my_mesh == m_now;
            if (mine) {
                const TS& ts = *reinterpret_cast<const TS*>(&S.tri[ow][tl * 4]);
                const uint32_t tt = C.t0[ow] + tl;
                const uint32_t org = ts.org;
                const int x = (int)(org & 0xFFFu) + (int)(bit & 7u), y = (int)(org >> 12) + (int)(bit >> 3);
                // (readfirstlane, not m_now: inside this branch the optimiser knows my_mesh == m_now and substitutes the per-lane
                //  value — the descriptor loads then become vector loads through a per-lane pointer, the texel reads 64-bit addresses)
#ifdef M2S_FUSED3_UV_GLOBAL
                const float2* const uvl = nullptr;
#else
                const float2* const uvl = &S.uv[ow][tl * 3];
#endif
                const float4* vrows = nullptr;
                if constexpr (kIndexed) vrows = reinterpret_cast<const float4*>(vt.rows);
                shade_from_tri<ConstMeshPtr, TS, true, kF3StreamAttr>(sc.tri, tt, x, y, kConstMesh(sc.meshes + __builtin_amdgcn_readfirstlane(my_mesh)),
                                                                       ts, rec, nullptr, uvl, vrows);
            }
            todo &= ~__ballot(mine);
        }
        if (!have_base) {
            if (!f3_get_base(C, chain, b0, lane, epoch, status, base)) break;
            have_base = true;
        }
        const uint32_t fl = l3_load(&C.flags);
        if (fl & 0xFFu) break;
        // (the base, like the counts, is re-read per strip: two scalar registers for the length of the stores)
        const unsigned long long base_now = (unsigned long long)l3_uniform(reinterpret_cast<const uint32_t*>(&C.base)) |
                                            ((unsigned long long)l3_uniform(reinterpret_cast<const uint32_t*>(&C.base) + 1) << 32);
        if ((fl & kF3Irregular) == 0) {
            const unsigned long long o0 = base_now + pos0;
            uint32_t nvalid = n;
            if (o0 + 64ull > limit) {
                if (o0 >= limit) nvalid = 0;
                else if (limit - o0 < nvalid) nvalid = (uint32_t)(limit - o0);
            }
#pragma unroll 1
            for (int part = 0; part < 64 / kL3Stage; ++part) {
                if (have && (lane / kL3Stage) == part) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) stage[(lane % kL3Stage) * 6 + k] = rec[k];
                }
                wave_lds_sync();
                float4* __restrict__ dsto = out + (o0 + (uint32_t)kL3Stage * part) * 6;
                const uint32_t nv = nvalid > (uint32_t)kL3Stage * part ? min((uint32_t)kL3Stage, nvalid - (uint32_t)kL3Stage * part) : 0u;
#pragma unroll
                for (int j = 0; j < (kL3Stage * 6 + 63) / 64; ++j) {
                    const uint32_t q = (uint32_t)lane + 64u * j;
                    const uint32_t r = q / 6u;
                    if (r < nv) nt_store(&dsto[q], stage[q]);
                }
                wave_lds_sync();
            }
        } else if (have) {
            const unsigned long long oidx = base_now + S.tskip[ow][tl] + pos;
            if (oidx < limit) {
                float4* __restrict__ dsto = out + oidx * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) nt_store(&dsto[k], rec[k]);
            }
        }
    }
    TLF(4);
    // (the upper halves of words 6 and 7: where the wave ran — XCC, then the hardware id register with its SE / CU / SIMD fields — and its class)
    TLFV(6, tl_strips | ((unsigned long long)(__builtin_amdgcn_s_getreg(kTlXccId) | (f3_class(round) << 8)) << 32));
    // ======================= epilogue: the workgroup's inclusive prefix / the counter =======================
    // (by the wave of the last batch; the base is resolved here if no strip needed it, e.g. a workgroup without fragments)
    const uint32_t err = l3_load(&C.flags) & 0xFFu;
    if (alive && wave == nb_here - 1 && err == 0) {
        if (!have_base) have_base = f3_get_base(C, chain, b0, lane, epoch, status, base);
        if (have_base && lane == 0) {
            const unsigned long long out_total = (C.total_w[0] + C.total_w[1]) + (C.total_w[2] + C.total_w[3]);
            chain_store(&chain[b0 + nb_here - 1], kFlagPrefix | etag | ((base + out_total) & kValMask));
            if (b0 + nb_here == n_batches) *total_out = base + out_total;
            // by-product of a launch without runs: where every run's output starts (the table of the NEXT launches at this R)
            if (runs.out && (lb & rmask) == 0u) runs.out[lb >> runs.shift] = base;
        }
    }
    // status[1] != 0 is what the host acts on; 2 = "a workgroup's entries do not fit", 1 = a bounded wait gave up
    if (err && lane == 0) __hip_atomic_store(&status[1], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    TLF(5);
    TLFV(7, (unsigned long long)lb | ((unsigned long long)__builtin_amdgcn_s_getreg(kTlHwId) << 32));
}

void launch_fused3(const SceneDev& sc, uint32_t R, unsigned long long* chain, uint64_t limit, float4* out,
                   unsigned long long* total, uint32_t* status, uint32_t epoch, BigItem* biglist, uint32_t* bigmeta,
                   const RunInfo& runs, const BatchTable& bt, hipStream_t st, const VtxTable* vt, const GeoPlanes* gp) {
    const uint32_t tpw = fused_tpw(sc.n_tri);
    const uint32_t n_batches = bt.first ? bt.n : n_fused_waves(sc.n_tri);
    if (!n_batches) return;
    uint32_t nb = (n_batches + kL3Team - 1) / kL3Team;
    RunInfo r = runs;
    if (tpw != 64u || bt.first) r = RunInfo{ nullptr, nullptr, 0u, nullptr };
    if (r.base) r.out = nullptr;
    if (r.base) nb = ((nb + (8u << r.shift) - 1u) / (8u << r.shift)) * (8u << r.shift);   // whole groups of eight runs; surplus workgroups exit at once
    else nb = (nb + 7u) & ~7u;
    const bool indexed = vt && vt->rows && vt->ids, geo = gp && gp->G0 && gp->G1 && gp->G2;
    auto go = [&](auto kernel, auto table, auto planes) {
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(kL3Threads), 0, st, sc, R, chain, (unsigned long long)limit, out, total, status,
                           epoch & 0xFFFFu, biglist, bigmeta, tpw, r, bt, table, planes);
    };
    if (indexed && geo) go(k_fused3<true, true>, *vt, *gp);
    else if (indexed) go(k_fused3<true, false>, *vt, GeoNone{});
    else if (geo) go(k_fused3<false, true>, VtNone{}, *gp);
    else go(k_fused3<false, false>, VtNone{}, GeoNone{});
}

#ifdef M2S_TIMELINE
}  // namespace m2s
extern "C" int m2s_debug_timeline_f3(void* dst, size_t bytes) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(m2s::g_tl_f3), std::min(bytes, sizeof(m2s::g_tl_f3))) == hipSuccess ? 0 : 1;
}
extern "C" int m2s_debug_timeline_f3_clear() {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(m2s::g_tl_f3)) != hipSuccess) return 1;
    return hipMemset(p, 0, sizeof(m2s::g_tl_f3)) == hipSuccess ? 0 : 2;
}
namespace m2s {
#endif
// (all instances are compiled for the same registers and LDS: one answer)
uint32_t fused3_resident_workgroups() { return resident_workgroups(reinterpret_cast<const void*>(&k_fused3<false, false>), kL3Threads); }
hipError_t preload_fused3() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_fused3<false, false>)); }

}  // namespace m2s
