/*
 * m2s.h — C ABI of the MI355X-native mesh -> 3D-Gaussian-splat conversion pass.
 *
 * This is the drop-in boundary for the ONE hot path of electronicarts/mesh2splat: the
 * per-triangle UV-space rasterisation conversion,
 *     class ConversionPass : IRenderPass { void execute(RenderContext&); }
 *     (src/renderer/renderPasses/ConversionPass.{hpp,cpp}, RenderPass.hpp:11-29)
 * whose device side is the GLSL program converter{VS,GS,FS}.glsl.  The reference has no
 * FFI layer (it is a C++ virtual call inside one executable); the entry points below are
 * what a binding for that call would need — the inputs ConversionPass reads from
 * RenderContext, the outputs it leaves there — with every GL object replaced by plain
 * pointers and sizes.  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: status-code returns, no exceptions cross the ABI, caller-owned input memory
 * is only borrowed for the duration of a call, device memory is owned by the context unless
 * the *_into variant is used, one context per host thread (like the single GL context).
 * All functions are implemented by hand-written HIP kernels for gfx950; there is NO CPU
 * fallback: on a machine without a usable device m2s_create fails with M2S_ERR_NO_DEVICE.
 */
#ifndef M2S_H
#define M2S_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M2S_ABI_VERSION 1

typedef enum m2s_status {
    M2S_OK = 0,
    M2S_ERR_INVALID = 1,   /* bad argument                                              */
    M2S_ERR_NO_DEVICE = 2, /* no HIP device / device index out of range                 */
    M2S_ERR_HIP = 3,       /* a HIP runtime call failed (m2s_last_error has the string) */
    M2S_ERR_OOM = 4,       /* device or host allocation failed                          */
    M2S_ERR_CAPACITY = 5,  /* destination too small                                     */
    M2S_ERR_IO = 6,        /* file could not be written                                 */
    M2S_ERR_STATE = 7      /* call order violated (e.g. convert before upload)          */
} m2s_status;

typedef struct m2s_ctx m2s_ctx;

/* One RGBA8 image as tiny_gltf leaves it (always 4 components, tiny_gltf.h:2609; row 0 first,
 * no flip) == utils::TextureDataGl (utils.hpp:190-211).  rgba8 == NULL means "map absent"
 * (ConversionPass.cpp:77-99 leaves has*Map = 0). */
typedef struct m2s_texture {
    const uint8_t* rgba8;
    uint32_t width, height;
} m2s_texture;

enum { M2S_TEX_ALBEDO = 0, M2S_TEX_NORMAL = 1, M2S_TEX_METALLIC_ROUGHNESS = 2 }; /* tex units 0,1,2 */

/* One glTF primitive == one std::pair<utils::Mesh, utils::GLMesh> of
 * RenderContext::dataMeshAndGlMesh (RenderContext.hpp:86).
 *   vertices      : the VBO built by SceneManager::setupMeshBuffers (SceneManager.cpp:483-512),
 *                   de-indexed, 3 vertices per triangle; per vertex
 *                   pos3 normal3 tangent4 uv2 [normalizedUv2 scale3].  stride_floats is 17 for
 *                   the reference layout, 12 for the live attributes only (the trailing 5 floats
 *                   are never read: converterGS.glsl uses neither normalizedUv nor scale).
 *   bbox_min/max  : Mesh::bbox == u_bboxMin/u_bboxMax (ConversionPass.cpp:111-112).  NOTE the
 *                   reference computes it cumulatively over the mesh list (SceneManager.cpp:476-527).
 *   base_color    : material.baseColorFactor == u_materialFactor (ConversionPass.cpp:110).
 *   tex           : meshToTextureData[mesh.name][BASE_COLOR|NORMAL|METALLIC_ROUGHNESS]. */
typedef struct m2s_mesh {
    const float* vertices;
    uint32_t n_vertices;
    uint32_t stride_floats;
    float bbox_min[3];
    float bbox_max[3];
    float base_color[4];
    m2s_texture tex[3];
} m2s_mesh;

/* == utils::GaussianDataSSBO (utils.hpp:145-152) == GLSL GaussianVertex (converterFS.glsl:21-28):
 * position (P,1) | color rgba*factor | scale (|Ju|,|Jv|,1e-7,0) | normal (n,0) | rotation (w,x,y,z) |
 * pbr (metallic, roughness, 0, 1).  96 bytes, std430. */
typedef struct m2s_gaussian {
    float position[4];
    float color[4];
    float scale[4];
    float normal[4];
    float rotation[4];
    float pbr[4];
} m2s_gaussian;

/* ---- lifetime -------------------------------------------------------------------------------- */
uint32_t m2s_abi_version(void);
/* Creates a context on HIP device `device` (>= 0). */
m2s_status m2s_create(int device, m2s_ctx** out_ctx);
void m2s_destroy(m2s_ctx* ctx);
/* Message of the last failure on this context (never NULL).  ctx == NULL: last create failure. */
const char* m2s_last_error(const m2s_ctx* ctx);

/* ---- scene upload == SceneManager::setupMeshBuffers + glUtils::generateTextures ---------------- */
/* Restricts the context to triangles [first, first+count) of the flattened (mesh-major, draw-order)
 * triangle list of the NEXT m2s_upload_scene: the multi-GPU shard of this rank.  count ==
 * UINT64_MAX (default) means "to the end".  Mesh uniforms and textures are always complete. */
m2s_status m2s_set_triangle_range(m2s_ctx* ctx, uint64_t first, uint64_t count);
/* Copies vertices to HBM (re-laid out as 144 B/triangle SoA planes), uploads the mesh table and the
 * RGBA8 textures and generates mip levels 1..4 (glUtils.cpp:292-313).  Replaces any previous scene. */
m2s_status m2s_upload_scene(m2s_ctx* ctx, const m2s_mesh* meshes, uint32_t n_meshes);

/* Optional: allocate now what the first upload (M2S_PREPARE_UPLOAD: pinned + device staging chunks) and the first export
 * (M2S_PREPARE_EXPORT: pinned chunks for the device-to-host copies) would otherwise allocate on their own critical path;
 * M2S_PREPARE_KERNELS: have the HIP runtime load the code objects of every kernel now instead of inside the first conversion /
 * export / viewer pass of the process (m2s_upload_scene does it for the conversion pipeline it chooses in any case). */
enum { M2S_PREPARE_UPLOAD = 1, M2S_PREPARE_EXPORT = 2, M2S_PREPARE_KERNELS = 4 };
m2s_status m2s_prepare(m2s_ctx* ctx, uint32_t flags);

/* Wall-clock breakdown (ms) of the last m2s_upload_scene: [0] whole call, [1] geometry (pinned staging + re-layout kernel),
 * [2] textures (staging, mip and combo kernels, final sync), [3] device / pinned allocations. */
m2s_status m2s_last_upload_ms(const m2s_ctx* ctx, float out_ms[4]);

/* The resolutionTarget the NEXT m2s_upload_scene prepares the scene for (0, the default: the R this context last converted at,
 * else 1024).  The reference converts right after SceneManager::loadModel, at RenderContext::resolutionTarget
 * (guiRendererConcreteMediator.cpp:11-29, RenderContext.hpp:64) — and never twice at the same (scene, R), so its FIRST
 * conversion is the one a user waits for.  The upload therefore ends with one exact fragment count at this R behind its own
 * kernels (in [0] of m2s_last_upload_ms; m2s_last_warm_ms alone) and leaves behind what that first conversion needs: the
 * pipeline decision, the XCD band table, the record pool.  A conversion at any other R needs none of it (fragments scale with
 * R^2; its first launch runs without bands). */
m2s_status m2s_set_resolution_hint(m2s_ctx* ctx, uint32_t R);
float m2s_last_warm_ms(const m2s_ctx* ctx);

/* ---- the pass == ConversionPass::execute ------------------------------------------------------- */
/* u_maxGaussians policy (converterFS.glsl:46-51): -1 (default) = the reference formula
 * min(R*R*6*max(1,meshes), 7'000'000) in 32-bit unsigned arithmetic (ConversionPass.cpp:21-24);
 * 0 = unlimited; > 0 = explicit cap.  Records with index >= cap are not stored. */
m2s_status m2s_set_max_gaussians(m2s_ctx* ctx, int64_t cap);
/* Runs the conversion at resolutionTarget R into the context-owned record buffer (re-allocated when
 * its size changes, ConversionPass.cpp:25-33).  Synchronous like execute() (glFinish + counter
 * read-back, ConversionPass.cpp:54-59).  *out_total = value of the fragment counter, i.e. the number
 * of fragments generated — NOT clamped to the cap, exactly like renderContext.numberOfGaussians. */
m2s_status m2s_convert(m2s_ctx* ctx, uint32_t R, uint64_t* out_total);
/* Same, but records go to caller-owned DEVICE memory (e.g. a torch tensor feeding an RCCL gather),
 * kernels are enqueued on `hip_stream` (a hipStream_t, NULL = default stream) and the call returns
 * after that stream has drained.  capacity_records additionally bounds what is stored. */
m2s_status m2s_convert_into(m2s_ctx* ctx, uint32_t R, void* d_records, uint64_t capacity_records,
                            void* hip_stream, uint64_t* out_total);
/* Asynchronous form for back-to-back conversions (a frame loop, one rank of a multi-GPU job): submit enqueues one
 * conversion and returns without waiting; wait blocks until the OLDEST submitted conversion has finished and returns
 * its counter (it then becomes "the last conversion" for m2s_num_stored / m2s_download / m2s_export_ply ...).
 * At most M2S_MAX_IN_FLIGHT conversions may be in flight; they execute in submission order.  d_records == NULL uses
 * the context-owned buffer and the context's stream; otherwise the caller's buffer and `hip_stream`, as in
 * m2s_convert_into.  Conversions that write the same buffer overwrite each other in order, like repeated draws into
 * one SSBO.  The reference's execute() is synchronous (glFinish, ConversionPass.cpp:54): this pair is an extension
 * that removes the launch + completion round trip (16 us of the 197 us a C3 conversion takes) from the critical path.
 * The first conversion of a scene at a given R, and any conversion that needs the second stage or the multi-pass
 * pipeline, is executed synchronously inside submit (same results, no overlap). */
#define M2S_MAX_IN_FLIGHT 4
/* lanes = 2: context-owned submissions alternate between two streams, each with its own look-back chain and record
 * buffer, so consecutive single-kernel conversions OVERLAP (the tail of one, where the GPU drains, with the head of the
 * next: C3 0.132 -> 0.108 ms per conversion at three in flight) instead of running back to back with ~8 us between
 * dependent kernels; multi-pass conversions likewise — the second lane has its own offsets / slice starts / per-triangle
 * setup records, so k_count_scan of one conversion runs beside k_emit2 of the one before.  Records then alternate between two buffers; m2s_device_records / m2s_download / m2s_export_ply
 * follow the conversion last waited for.  Default 1 (one stream, one buffer). */
m2s_status m2s_set_async_lanes(m2s_ctx* ctx, int lanes);
m2s_status m2s_convert_submit(m2s_ctx* ctx, uint32_t R, void* d_records, uint64_t capacity_records, void* hip_stream);
m2s_status m2s_convert_wait(m2s_ctx* ctx, uint64_t* out_total);
/* Number of records actually stored by the last convert: min(total, cap[, capacity]). */
uint64_t m2s_num_stored(const m2s_ctx* ctx);
/* Device pointer of the context-owned records of the last m2s_convert (zero-copy consumers). */
const void* m2s_device_records(const m2s_ctx* ctx);
/* == glGetBufferSubData in SceneManager::exportPly (SceneManager.cpp:659-664). */
m2s_status m2s_download(m2s_ctx* ctx, m2s_gaussian* dst, uint64_t capacity_records);
/* Per-triangle fragment counts of the last convert (shard balancing / diagnostics); n = triangles in range. */
m2s_status m2s_download_triangle_counts(m2s_ctx* ctx, uint32_t* dst, uint64_t n);

/* ---- export == SceneManager::exportPly + parsers::savePlyVector -------------------------------- */
/* format 0 standard 3DGS (62 floats/row), 1 PBR (19 floats/row), 2 compressed PBR (48 B/row); any
 * other value behaves like 0 (parsers.cpp:646-648).  scale_multiplier = gaussianStd / R. */
m2s_status m2s_write_ply(const char* path, const m2s_gaussian* records, uint64_t n, uint32_t format,
                         float scale_multiplier);
/* Downloads the last convert's records and writes them: scaleMultiplier = gaussian_std / R
 * (SceneManager.cpp:668). */
m2s_status m2s_export_ply(m2s_ctx* ctx, const char* path, uint32_t format, float gaussian_std);

/* Several writers, one file (one per GPU rank of a sharded conversion: no record gather needed): writes n host records as
 * rows [first_row, first_row + n) of a .ply whose header announces total_rows.  The file is created if absent and never
 * truncated below its final size; the writer of row 0 also writes the header and sets the file's length.  Writers may run
 * concurrently (different processes); the result is byte-identical to m2s_write_ply of the concatenated records. */
m2s_status m2s_write_ply_slice(const char* path, const m2s_gaussian* records, uint64_t n, uint32_t format, float scale_multiplier,
                               uint64_t first_row, uint64_t total_rows);
/* Same for the first n_rows records of the context's last conversion (n_rows <= m2s_num_stored). */
m2s_status m2s_export_ply_slice(m2s_ctx* ctx, const char* path, uint32_t format, float gaussian_std, uint64_t first_row,
                                uint64_t n_rows, uint64_t total_rows);

/* ---- multi-GPU: triangle-range shards, one process per GPU, RCCL over xGMI ------------------------------------------
 * The reference is a single-GPU program; this block implements BASELINE.json's sharding: every triangle is independent
 * (no depth test, no blending: ConversionPass.cpp:45-48), the reference's one shared word — the append cursor,
 * converterFS.glsl:46 — becomes one counter per rank, and concatenating the per-rank record blocks in rank order
 * reproduces the single-GPU output byte for byte (the device emits in canonical (triangle, row, column) order).
 * Per rank: m2s_dist_shard_ranges -> m2s_set_triangle_range + m2s_upload_scene (cap lifted: m2s_set_max_gaussians(0)) ->
 * m2s_convert* -> m2s_dist_all_gather_counts (8 bytes per rank) -> either m2s_export_ply_slice at the rank's offset (no
 * record leaves its GPU) or m2s_dist_gather_records (every block to every rank / to one root, exact sizes, one RCCL
 * group of sends and receives).  librccl is opened at run time; without it these calls fail with M2S_ERR_STATE. */
#define M2S_DIST_ID_BYTES 128
typedef struct m2s_dist m2s_dist;
/* Rank 0 obtains the communicator id (== ncclGetUniqueId) and hands the 128 bytes to the other ranks by any means. */
m2s_status m2s_dist_unique_id(uint8_t out_id[M2S_DIST_ID_BYTES]);
/* Collective over all ranks (== ncclCommInitRank) on HIP device `device`. */
m2s_status m2s_dist_create(int device, const uint8_t id[M2S_DIST_ID_BYTES], int rank, int world, m2s_dist** out);
/* The same exchange with the ranks as THREADS of one process (the shape of the reference: one executable), one context and
 * one GPU each; no RCCL involved: counts go through a table of the group, records through hipMemcpyPeerAsync (the same xGMI
 * links).  The id of a new group of `world` ranks; every rank then calls m2s_dist_create with it, every m2s_dist_* call
 * below works unchanged, and the group is released by its last m2s_dist_destroy. */
m2s_status m2s_dist_local_id(int world, uint8_t out_id[M2S_DIST_ID_BYTES]);
void m2s_dist_destroy(m2s_dist* d);
int m2s_dist_rank(const m2s_dist* d);
int m2s_dist_world(const m2s_dist* d);
/* What moves the bytes of this communicator: "in-process", "rccl", or "rccl:<path>" when the environment variable M2S_RCCL_PATH
 * named the library (it takes precedence over an RCCL already in the process and over the system's). */
const char* m2s_dist_transport(const m2s_dist* d);
/* d == NULL: message of the last failed m2s_dist_unique_id / _create / _shard_ranges on this thread. */
const char* m2s_dist_last_error(const m2s_dist* d);
/* Host only, deterministic (every rank computes the same plan): cuts the flattened triangle list into `world` contiguous
 * ranges of about equal cost = estimated fragments at density R (projected area on the dominant axis plane, in pixels)
 * + 0.25 per triangle.  first[r], count[r] feed m2s_set_triangle_range on rank r. */
m2s_status m2s_dist_shard_ranges(const m2s_mesh* meshes, uint32_t n_meshes, uint32_t R, int world, uint64_t* first, uint64_t* count);
/* The one mandatory exchange: every rank learns every rank's counter.  counts[world]; offsets[world + 1] (may be NULL) =
 * exclusive prefix = where each rank's block starts in the merged buffer.  publish/collect is the non-blocking form for
 * back-to-back conversions (up to 8 exchanges in flight, completed in order, on a stream of their own). */
m2s_status m2s_dist_all_gather_counts(m2s_dist* d, uint64_t my_total, uint64_t* counts, uint64_t* offsets);
m2s_status m2s_dist_publish_count(m2s_dist* d, uint64_t my_total);
m2s_status m2s_dist_collect_counts(m2s_dist* d, uint64_t* counts, uint64_t* offsets);
/* Global cap semantics of a sharded conversion (converterFS.glsl:46-51): the merged buffer keeps the first `cap` records
 * in rank order (0 = unlimited); keep[r] = how many records rank r contributes. */
void m2s_dist_clamp_to_cap(const uint64_t* counts, int world, uint64_t cap, uint64_t* keep);
/* Record exchange: rank r's block (counts[r] records at d_mine on rank r) lands at record offset sum(counts[0..r)) of
 * d_merged on every rank (root < 0) or on `root` only (d_merged may be NULL elsewhere).  Device pointers; enqueued on
 * hip_stream (the stream the conversion ran on); returns without waiting for it. */
m2s_status m2s_dist_gather_records(m2s_dist* d, const void* d_mine, const uint64_t* counts, void* d_merged, int root, void* hip_stream);
/* Depth sort (== m2s_sort_by_depth == RadixSortPass.cpp:8-90) of records spread over the ranks — BASELINE config 5's "final
 * radix sort of the merged splat buffer" without merging it on one GPU: sample sort with one exact-size record exchange.
 * Collective.  In: every rank's context holds its block (its last conversion, or m2s_set_records).  Out: the context's sorted
 * buffer (m2s_device_sorted_records, m2s_download_sorted) holds this rank's contiguous slice of the globally sorted sequence —
 * *out_n records starting at position *out_offset; the slices in rank order are bit-identical to one GPU sorting the
 * rank-major concatenation (stable: ties keep rank, then original position).  The context's current records become the
 * received, not yet sorted ones. */
m2s_status m2s_dist_sort_by_depth(m2s_dist* d, m2s_ctx* ctx, const float world_to_view[16], uint64_t* out_n, uint64_t* out_offset);
/* Blocks until everything enqueued on hip_stream (the record exchange) has completed. */
m2s_status m2s_dist_wait(m2s_dist* d, void* hip_stream);

/* ---- depth sort == RadixSortPass::execute (RadixSortPass.cpp:8-90) ------------------------------------ */
/* Sorts the records stored by the last m2s_convert by key = floatBitsToUint(view-space z), ascending on the
 * raw bits (radixSortPrepass.glsl:23-33; z = row 2 of world_to_view * (P,1), world_to_view column-major like
 * glm), stable, and gathers the 96-byte records into a second context-owned buffer (radixSortGather.glsl).
 * *out_n = number of records sorted. */
m2s_status m2s_sort_by_depth(m2s_ctx* ctx, const float world_to_view[16], uint64_t* out_n);
/* A caller that is going to sort what it converts (BASELINE config 5: "final radix sort of the merged splat buffer") says so before
 * converting: where the conversion kernel can (k_sparse: the scenes of tens of millions of records), it then also leaves the records'
 * positions behind as a compact 16-byte plane, and the first m2s_sort_by_depth of those records builds its keys from 16 B per record
 * instead of touching every 128-byte line of the 96-byte records (RadixSortPass.cpp:16-90 sorts every frame; this is the first frame).
 * Costs the conversion 16 more bytes written per record; changes no record.  Default: off. */
m2s_status m2s_set_keep_positions(m2s_ctx* ctx, int enabled);
/* 1 if the position plane of the CURRENT records exists (left by their conversion, or by an earlier m2s_sort_by_depth of them). */
int m2s_positions_ready(const m2s_ctx* ctx);
const void* m2s_device_sorted_records(const m2s_ctx* ctx);
const void* m2s_device_sorted_keys(const m2s_ctx* ctx);      /* uint32[n], ascending: the keys of those records */
uint64_t m2s_num_sorted(const m2s_ctx* ctx);
uint32_t m2s_last_resolution(const m2s_ctx* ctx);            /* R of the current records (0: none / uploaded records) */
m2s_status m2s_download_sorted(m2s_ctx* ctx, m2s_gaussian* dst, uint64_t capacity_records);
/* Duration (ms) of the last profiled sort (key build + radix sort + gather). */
float m2s_last_sort_ms(const m2s_ctx* ctx);
/* The three stages of the last m2s_sort_by_depth, ms (m2s_set_profiling on): [0] keys, [1] radix sort, [2] gather of the 96-byte
 * records.  The first sort after the records changed reads the positions out of the records (every line of the buffer) and leaves
 * them behind as a compact plane; later sorts of the same records — the reference sorts every frame — build their keys from that. */
m2s_status m2s_last_sort_stage_ms(const m2s_ctx* ctx, float out_ms[3]);

/* ---- records from elsewhere == Renderer::updateGaussianBuffer after SceneManager::loadPly --------------- */
/* Makes `n` host records (e.g. the output of m2s_read_ply) the context's current records, as the reference does with a
 * loaded .ply (guiRendererConcreteMediator.cpp:30-34 -> glUtils::fillGaussianBufferSsbo, glUtils.cpp:676-684):
 * m2s_num_stored / m2s_device_records / m2s_download / m2s_prepass / m2s_sort_by_depth then refer to them.  The next
 * conversion replaces them.  (The viewer treats such records as format 1: set m2s_prepass_params.format accordingly.) */
m2s_status m2s_upload_records(m2s_ctx* ctx, const m2s_gaussian* records, uint64_t n);

/* Records that already live in device memory (e.g. the merged buffer of m2s_dist_gather_records) become the context's current
 * records without a copy: m2s_num_stored / m2s_download / m2s_export_ply (scale multiplier = std / R) / m2s_prepass /
 * m2s_sort_by_depth then refer to them.  The memory stays the caller's and must outlive those calls.
 * The context caches what it derives from the current records (m2s_sort_by_depth: the plane of positions its keys are built from)
 * under (pointer, n, a counter bumped by every conversion / m2s_upload_records / m2s_set_records).  A caller that REWRITES a buffer
 * in place — the one adopted here, or one handed to m2s_convert_into by a kernel of its own — must call m2s_set_records again
 * afterwards: without it later sorts would order the new records by the old positions. */
m2s_status m2s_set_records(m2s_ctx* ctx, const void* d_records, uint64_t n, uint32_t R);
/* Room for n records in the context-owned pool (grow-only, like the conversion's own allocation); *out_ptr = device address. */
m2s_status m2s_reserve_records(m2s_ctx* ctx, uint64_t n, void** out_ptr);

/* ---- viewer prepass == GaussiansPrepass::execute (GaussiansPrepass.cpp:8-56) ---------------------------- */
/* What the reference's compute shader gaussianSplattingPrepassCS.glsl:58-204 (+ common.glsl) does to every Gaussian
 * before it is drawn: transform, frustum cull (1.05 * w guard band), optional test against the mesh depth texture,
 * 3D covariance -> 2D covariance (+0.3 low-pass) -> conic and the two quad axes in NDC, debug colour modes; survivors
 * are appended to a QuadNdcTransformation array and a view-space depth array (the RadixSortPass key source).
 * Fields mirror the RenderContext members the pass reads (RenderContext.hpp:34-111).  Matrices are column-major (glm). */
typedef struct m2s_prepass_params {
    float world_to_view[16];     /* viewMat   -> u_worldToView                                              */
    float view_to_clip[16];      /* projMat   -> u_viewToClip                                               */
    float model_to_world[16];    /* modelMat  -> u_modelToWorld                                             */
    int32_t resolution[2];       /* rendererResolution (glm::ivec2) -> u_resolution                         */
    float near_far[2];           /* nearPlane, farPlane -> u_nearFar                                        */
    float gaussian_std;          /* gaussianStd;  u_stdDev = gaussianStd / float(resolutionTarget)          */
    uint32_t resolution_target;  /* resolutionTarget                                                        */
    int32_t render_mode;         /* renderMode: 0 colour, 1 depth, 2 normal, 3 geometry (per-invocation hash), 6 as 0; else black */
    uint32_t format;             /* 0 mesh2splat, 1 classic 3DGS .ply, 2 compressed PBR (3 treated like 0)  */
    uint32_t ply_has_pbr;        /* plyHasPbr                                                               */
    uint32_t depth_test_mesh;    /* performMeshDepthTest: 1 = cull opaque (alpha > .95) format-0 Gaussians behind `depth` */
    const float* depth;          /* meshDepthTexture: depth_w x depth_h window-space depth in [0,1], row 0 = bottom of the
                                    window (GL texture orientation), sampled GL_NEAREST / CLAMP_TO_EDGE (renderer.cpp:290-296).
                                    HOST memory unless depth_on_device; read only when depth_test_mesh == 1               */
    uint32_t depth_w, depth_h;
    uint32_t depth_on_device;    /* 1: `depth` is a device pointer on the context's device (no copy)        */
    uint32_t arrival_order;      /* 0: survivors in input order (reproducible).  1: in arrival order, as the reference's atomic
                                    append leaves them (same set, nondeterministic order; ~1.4x faster)                  */
} m2s_prepass_params;

/* == QuadNdcTransformation (gaussianSplattingPrepassCS.glsl:17-24), 96 bytes */
typedef struct m2s_quad {
    float mean2d_ndc[4];     /* clip position, xyz divided by w; w kept                   */
    float quad_scale_ndc[4]; /* major axis xy, minor axis xy, in NDC units                */
    float color[4];          /* per render mode                                           */
    float conic[4];          /* inverse 2D covariance (xx, xy, yy), view depth (-z)       */
    float normal[4];         /* encoded normal xyz, metallic                              */
    float ws_pos[4];         /* world position xyz, roughness                             */
} m2s_quad;

/* Runs the prepass over `n` records at device pointer `d_records` (96-byte m2s_gaussian each), or over the records of the
 * context's last conversion when d_records is NULL (n ignored).  Survivors are stored in context-owned buffers in INPUT
 * order (the reference appends through an atomic counter, i.e. in arrival order; RadixSortPass reorders them anyway).
 * Synchronous, like the reference's dispatch + the counter read-back that follows it (RadixSortPass.cpp:18-22).
 * *out_visible = number of survivors (the reference's atomic counter). */
m2s_status m2s_prepass(m2s_ctx* ctx, const m2s_prepass_params* params, const void* d_records, uint64_t n, uint64_t* out_visible);
const void* m2s_device_quads(const m2s_ctx* ctx);            /* m2s_quad[visible]  (perQuadTransformationsBuffer)   */
const void* m2s_device_prepass_depths(const m2s_ctx* ctx);   /* float[visible]     (gaussianDepthPostFiltering)     */
m2s_status m2s_download_prepass(m2s_ctx* ctx, m2s_quad* dst_quads, float* dst_depths, uint64_t capacity);
/* Duration (ms) of the last profiled prepass kernel. */
float m2s_last_prepass_ms(const m2s_ctx* ctx);

/* == RadixSortPass::execute (RadixSortPass.cpp:8-90) on the output of the last m2s_prepass: key = the raw bits of the
 * view-space depths (radixSortPrepass.glsl:23-33), ascending, stable (LSD radix like glu::RadixSort); the quads are gathered
 * into a second context-owned buffer in that order (radixSortGather.glsl:30-49).  *out_n = number sorted = what the
 * reference writes to drawElementsIndirectCommand.instanceCount (count = 6, first = baseInstance = 0). */
m2s_status m2s_sort_prepass(m2s_ctx* ctx, uint64_t* out_n);
const void* m2s_device_sorted_quads(const m2s_ctx* ctx);     /* m2s_quad[n]  (perQuadTransformationBufferSorted) */
m2s_status m2s_download_sorted_quads(m2s_ctx* ctx, m2s_quad* dst, uint64_t capacity);
/* Duration (ms) of the last profiled m2s_sort_prepass (radix sort + gather). */
float m2s_last_sort_prepass_ms(const m2s_ctx* ctx);
/* One frame's GaussiansPrepass::execute + RadixSortPass::execute (GaussiansPrepass.cpp:8-56, RadixSortPass.cpp:8-90) as ONE pass over the
 * records of the context (its last conversion, or m2s_set_records / m2s_upload_records): the depth sort is taken FIRST — keys = the bits of
 * the view-space depth the prepass is about to store (from the 16-byte position plane the context keeps of its current records), stable
 * radix sort of (key, record index) — and the prepass then reads the records THROUGH that permutation and appends its survivors in that
 * order: the 96-byte gather of RadixSortPass::gatherPost (radixSortGather.glsl:30-49) and the prepass's own read become one pass.  Without a depth
 * image (depth_test_mesh == 0, or format != 0) the sort applies the prepass's frustum test itself — it depends on the position alone — and the
 * prepass runs over the survivors only.  The shader's last test (lambda2 < 0, gaussianSplattingPrepassCS.glsl:183: it removes stretched
 * splats whose screen-space covariance is numerically of rank 1, as a loaded .ply can hold) depends on scale and rotation and is not
 * known to the sort.  A frame in which a record passes the frustum test and fails that one is detected by the prepass and taken a second
 * time, every record sorted and the prepass compacting as with a depth image: same result, but such a frame pays a second sort and a
 * second prepass (2.74 M records + 2000 needles, 1920 x 1080, one blocking call: 0.72 ms against 0.44 ms for m2s_prepass + m2s_sort_prepass
 * and 0.34 ms for the call on a frame without such records — for records like these the two calls are the faster route).  The stage times
 * are then those of the second attempt.
 * Result: m2s_device_sorted_quads / m2s_download_sorted_quads hold exactly what m2s_prepass (input order) followed by m2s_sort_prepass
 * leaves there, byte for byte; *out_visible = their number.  params->arrival_order is ignored (the order IS the result); the unsorted quads
 * of m2s_prepass are not produced.  m2s_last_sort_stage_ms: [0] keys, [1] radix sort, [2] the prepass through the permutation. */
m2s_status m2s_prepass_sorted(m2s_ctx* ctx, const m2s_prepass_params* params, uint64_t* out_visible);
/* uint32[visible] after m2s_prepass_sorted: entry i = the index, in the context's current records, of the record sorted quad i was made
 * from.  Valid until the next prepass or sort of the context.  NULL after any other producer of sorted quads (m2s_sort_prepass,
 * m2s_upload_quads), once the records changed, and when there are no sorted quads. */
const void* m2s_device_sorted_sources(const m2s_ctx* ctx);
/* Copies them to the host, as m2s_download_sorted_quads copies the quads.  M2S_ERR_STATE when there are none; M2S_ERR_CAPACITY when
 * dst holds fewer entries than there are sorted quads. */
m2s_status m2s_download_sorted_sources(m2s_ctx* ctx, uint32_t* dst, uint64_t capacity);
/* The counterpart of m2s_upload_quads for the sources: n host indices become the sources of the context's sorted quads.
 * M2S_ERR_INVALID unless n is the number of sorted quads and every index is below m2s_num_stored. */
m2s_status m2s_upload_quad_sources(m2s_ctx* ctx, const uint32_t* host_sources, uint64_t n);

/* ---- splat pass == GaussianSplattingPass::execute (GaussianSplattingPass.cpp:50-95) ----------------------- */
/* Draws one quad per entry of perQuadTransformationBufferSorted (gaussianSplattingVS.glsl:31-40) and blends the fragment shader's
 * five outputs (gaussianSplattingPS.glsl:29-45) into the G-buffer of renderer.cpp:325-380.  GL semantics restated for a compute
 * pass; these choices are the pin (tests/splat_ref.py restates them operation for operation, fp32 without contraction):
 *  - Quads are blended in ARRAY order, quad 0 first (the depth sort's ascending keys put the nearest Gaussian first).
 *  - Targets, all cleared to 0 at the start of the call (GaussianSplattingPass.cpp:59-60), W x H pixels, row 0 = the BOTTOM row
 *    (GL orientation, as m2s_prepass_params.depth): attachment 0 position, 1 normal, 3 depth: RGBA16F (half4 per pixel);
 *    2 albedo, 4 metallic-roughness: RGBA8 unorm (uchar4 per pixel).
 *  - Geometry: vertices mean.xy + (vx * scale.xy + vy * scale.zw), (vx, vy) in {(-1,-1), (-1,1), (1,1), (1,-1)}, triangles (0,1,2)
 *    and (0,2,3); the sum of the two axis terms rounds, then the addition of the mean.  Viewport xw = (W/2) x + W/2, yw = (H/2) y + H/2,
 *    then the project's pinned rasteriser (the conversion's, with a W x H viewport): snap to 1/256 px (RNE), int64 edge functions,
 *    both windings (GL_CULL_FACE off), top-left rule, pixel centres (x + 0.5, y + 0.5).  A pixel centre on the shared diagonal
 *    belongs to exactly one of the two triangles.
 *  - A quad with a non-finite value in any field the pass reads (mean.xy, scale, color, conic, normal, ws_pos) or with a vertex
 *    beyond the +-16384 px guard band is SKIPPED and counted (*out_skipped) — GL would clip it instead.  Quads made by m2s_prepass
 *    never get there for W, H <= 8192: their means lie inside the 1.05 w frustum and their axes are capped at 1024 px
 *    (gaussianSplattingPrepassCS.glsl:185-186).
 *  - Fragment (VS:34-40, PS:30-45): screen = ((mean.xy + 1) * 0.5) * (W, H); d = screen - fragcoord;
 *    alpha = ((-0.5 cx) * (dx dx) + (-0.5 cz) * (dy dy)) + (-cy) * (dx dy) with conic = (cx, cy, cz); g = exp(alpha) (the device's
 *    fast exp: the one step allowed to differ from the restatement).  Sources: albedo ((rgb * a) * g, a * g) — in render mode 4
 *    (overdraw) the constant (0.01, 0.005, 0, 0.01) —; position (ws.xyz * g, g); normal (normal.xyz * g, a * g);
 *    depth (conic.w * g x 3, a * g); metallic-roughness (normal.w * g, ws.w * g, 0, g).
 *  - Blend (GaussianSplattingPass.cpp:63-66), per attachment with its own destination alpha: t = 1 - dst.a, r = src * t + dst, each
 *    operation rounded to fp32; render mode 4: r = src + dst.  RGBA16F: no clamp, r rounded to half (RNE, subnormals kept, overflow
 *    to +-inf) after EVERY fragment.  RGBA8: the source is clamped to [0, 1] first, q = rint(clamp(r, 0, 1) * 255), read back as q / 255.
 *  - A pixel whose five alphas are exactly 1.0 stops early only where that leaves its bytes unchanged.
 * Synchronous.  Errors: M2S_ERR_INVALID for a resolution outside 1..8192, a render mode outside 0..6, reserved != 0, or d_quads NULL
 * while the context holds no sorted quads.  n = 0 with a non-NULL d_quads: five cleared planes. */
typedef struct m2s_splat_params {
    int32_t resolution[2];  /* rendererResolution == u_resolution == viewport, 1..8192 each: the W x H the quads were made for */
    int32_t render_mode;    /* u_renderMode 0..6: 4 = overdraw (constant albedo, blend ONE/ONE); any other ONE_MINUS_DST_ALPHA/ONE */
    uint32_t reserved;      /* 0 */
} m2s_splat_params;
/* d_quads == NULL: the context's sorted quads (m2s_sort_prepass / m2s_prepass_sorted / m2s_upload_quads), n ignored; else n m2s_quad
 * at a device pointer on the context's device.  *out_skipped (may be NULL) = quads skipped by the rule above. */
m2s_status m2s_splat(m2s_ctx* ctx, const m2s_splat_params* params, const void* d_quads, uint64_t n, uint64_t* out_skipped);
/* n host quads become the context's sorted quads (what m2s_device_sorted_quads returns and m2s_splat draws with d_quads == NULL). */
m2s_status m2s_upload_quads(m2s_ctx* ctx, const m2s_quad* host_quads, uint64_t n);
/* Attachment 0..4 of the last m2s_splat: 0, 1, 3: half4[W * H]; 2, 4: uchar4[W * H]; row 0 = bottom.  NULL before any splat. */
const void* m2s_device_gbuffer(const m2s_ctx* ctx, uint32_t attachment);
m2s_status m2s_download_gbuffer(m2s_ctx* ctx, uint32_t attachment, void* dst, uint64_t capacity_bytes);
/* Duration (ms) of the last profiled m2s_splat (sum of its three stages), and the stages: [0] setup + bin, [1] grouping by tile
 * (radix sort, tile ranges, tile order), [2] blend. */
float m2s_last_splat_ms(const m2s_ctx* ctx);
m2s_status m2s_last_splat_stage_ms(const m2s_ctx* ctx, float out_ms[3]);
/* What the last m2s_splat did: [0] (tile, quad) pairs, [1] fragments blended (after the early exit), [2] quads skipped. */
m2s_status m2s_last_splat_counts(const m2s_ctx* ctx, uint64_t out[3]);

/* ---- contribution pass and pruning (no counterpart in the reference: it shows every Gaussian it keeps) ------------------------ */
/* What every record of the context adds to the picture of a view, recorded instead of the picture.  The pin:
 *  - For render modes other than 4, m2s_splat updates the albedo attachment's alpha per fragment as A3 <- unorm8(sA3 * tA + A3) with
 *    sA3 = clamp01(a * g) and tA = 1 - A3 (the RGBA8 rule above).  The WEIGHT of a fragment is the fp32 product w = sA3 * tA of
 *    exactly that update: what the fragment adds to the pixel's coverage before quantisation, with A3 evolving byte-quantised exactly
 *    as in m2s_splat.
 *  - Geometry, coverage, quad order, skipped quads and g = exp(alpha) (the device's fast exp) are all those of m2s_splat; a pixel
 *    covered by both triangles of a quad yields two fragments.
 *  - w is never NaN: clamp01 is fmin(fmax(x, 0), 1), which returns the other operand for a NaN, so sA3 lies in [0, 1]; tA lies in
 *    [0, 1] because A3 is one of q / 255.  Hence 0 <= w <= 1, and non-negative floats order as their bits do as unsigned integers.
 *  - Two accumulators per record, uint32[m2s_num_stored] each: wmax = the bits of the largest w of any fragment of any quad made from
 *    that record; npix = the number of fragments with w > count_weight (strict: a fragment on a saturated pixel, w = 0, never counts).
 *    An integer maximum and an integer sum: independent of the order of evaluation, identical from run to run.  They keep accumulating
 *    over calls (views).  npix cannot overflow within 256 views: a quad's axes are capped at 1024 px by the prepass, so a quad covers at
 *    most 2048^2 = 2^22 pixels of a view, and 256 * 2^22 = 2^30.
 *  - A record whose every fragment has w = 0 adds nothing to the ALPHA of the albedo attachment.  It adds nothing to its colour
 *    either — m2s_splat adds clamp01(colour * g) * tA there, and tA = 0 wherever a positive opacity gave w = 0 — with one exception:
 *    a record whose opacity is exactly 0 (or NaN, or negative) has sA3 = 0 and w = 0 on pixels that are not saturated, where its
 *    colour term is still added.  Such a record is invisible to the weight and is dropped by m2s_prune at min_weight = 0, which
 *    then changes the colour of that plane.  The conversion writes the material's alpha; a .ply can hold anything.
 * m2s_contrib_begin sizes both accumulators to the context's current records, zeroes them and ties them to those records.
 * m2s_contrib_accumulate runs over the context's sorted quads and their sources (m2s_prepass_sorted; m2s_device_sorted_sources) at
 * params->resolution.  It touches neither the G-buffer nor the frame.  Synchronous.  M2S_ERR_INVALID for render mode 4 (the weight is
 * not defined there), a render mode outside 0..6, reserved != 0, a resolution outside 1..8192, missing sorted quads or sources, no
 * m2s_contrib_begin, records that changed since it, a count_weight that is negative or not finite. */
m2s_status m2s_contrib_begin(m2s_ctx* ctx);
m2s_status m2s_contrib_accumulate(m2s_ctx* ctx, const m2s_splat_params* params, float count_weight);
/* which = 0: wmax, 1: npix.  uint32[m2s_num_stored]; NULL without valid accumulators. */
const void* m2s_device_contrib(const m2s_ctx* ctx, uint32_t which);
/* Either destination may be NULL.  M2S_ERR_STATE without valid accumulators. */
m2s_status m2s_download_contrib(m2s_ctx* ctx, uint32_t* dst_wmax, uint32_t* dst_npix, uint64_t capacity);
/* Duration (ms) of the last profiled m2s_contrib_accumulate and its stages: [0] setup + bin, [1] grouping (both m2s_splat's own),
 * [2] the contribution blend. */
float m2s_last_contrib_ms(const m2s_ctx* ctx);
m2s_status m2s_last_contrib_stage_ms(const m2s_ctx* ctx, float out_ms[3]);
/* Keeps record i iff wmax[i] > min_weight (compared as floats) and npix[i] >= min_pixels: a stable compaction on the device into the
 * context-owned pool.  The survivors become the context's current records, in their previous order, with the resolutionTarget kept
 * (records adopted through m2s_set_records are compacted into the pool; the caller's memory is not written).  Cached positions, sorted
 * quads, sources and the accumulators are invalidated.  A baked plane of these records (m2s_bake_light) is compacted with the same
 * flags, so that m2s_export_ply_sh still matches.  *out_kept (may be NULL) = survivors.  M2S_ERR_INVALID for a NaN min_weight or
 * reserved != 0; M2S_ERR_STATE without accumulators of the current records or with conversions in flight. */
typedef struct m2s_prune_params {
    float min_weight;
    uint32_t min_pixels;
    uint32_t reserved;      /* 0 */
} m2s_prune_params;
m2s_status m2s_prune(m2s_ctx* ctx, const m2s_prune_params* params, uint64_t* out_kept);
/* The last m2s_prune: [0] records before, [1] kept, [2] dropped by weight, [3] dropped by pixels alone. */
m2s_status m2s_last_prune_counts(const m2s_ctx* ctx, uint64_t out[4]);
float m2s_last_prune_ms(const m2s_ctx* ctx);

/* ---- pruning to a budget (no counterpart in the reference: its cap keeps whatever arrives first, RenderPass.hpp:9) ------------- */
/* Of the records that pass the thresholds, keeps the max_records with the largest importance.  m2s_set_max_gaussians truncates in
 * canonical (mesh, triangle, row, column) order — the last meshes go, the first stay at full density —; this chooses which records go.
 * The pin (tests/budget_ref.py restates it):
 *  - Candidates.  M2S_IMPORTANCE_VIEWS: the records m2s_prune keeps with the same min_weight / min_pixels — wmax > min_weight compared
 *    as floats, and npix >= min_pixels —; it needs valid accumulators of the current records exactly as m2s_prune does.
 *    M2S_IMPORTANCE_AREA: every record; it needs records only (converted, uploaded, adopted or already pruned) and reads neither
 *    threshold.
 *  - Key, a uint32 per candidate.  VIEWS: the bits of the fp32 product (float)npix * wmax — the conversion uint32 -> float rounds to
 *    nearest even, once; the multiply rounds once; wmax lies in [0, 1] and npix < 2^30, so the product is finite and non-negative.
 *    AREA: a = fminf(fmaxf(color[3], 0), 1), s = fabsf(scale[0]) * fabsf(scale[1]), p = s * a, key = the bits of fmaxf(p, 0.0f) with a
 *    zero of either sign read as +0 (key = p > 0 ? bits(p) : 0): a NaN anywhere, or inf * 0, gives key 0; +inf is the largest key.  (A
 *    .ply can hold anything; conversion records are tame.)  Non-negative floats order as their bits do as unsigned integers: from
 *    here on everything is integer arithmetic, identical from run to run.
 *  - Selection.  At most max_records candidates: the candidates are kept.  Otherwise let T be the max_records-th largest key among
 *    the candidates; kept are every candidate with key > T and, of the candidates with key == T, the first
 *    max_records - #{key > T} in index order.  Exactly max_records survive.  This equals: stable-sort the candidates by key
 *    descending, take the first max_records, restore index order.  (A radix select over the keys, four rounds of eight bits; the
 *    96-byte records are not sorted.)
 *  - Effect, as m2s_prune: a stable compaction into the context-owned pool, order and resolutionTarget kept; a caller's adopted memory
 *    is not written; a baked SH plane of these records is compacted with the same flags; cached positions, sorted quads, sources and
 *    the accumulators are invalidated and the records epoch advances.
 * *out_kept (may be NULL) = survivors.  Synchronous.  M2S_ERR_INVALID: max_records == 0, reserved != 0, an unknown importance, a NaN
 * min_weight (VIEWS).  M2S_ERR_STATE: VIEWS without accumulators of the current records, no records at all, conversions in flight.
 * M2S_ERR_CAPACITY: 2^32 records or more. */
enum { M2S_IMPORTANCE_VIEWS = 0, M2S_IMPORTANCE_AREA = 1 };
typedef struct m2s_budget_params {
    uint64_t max_records;   /* >= 1 */
    float    min_weight;    /* VIEWS: m2s_prune's test; AREA: not read */
    uint32_t min_pixels;    /* VIEWS: m2s_prune's test; AREA: not read */
    uint32_t importance;    /* M2S_IMPORTANCE_* */
    uint32_t reserved;      /* 0 */
} m2s_budget_params;        /* 24 bytes; offsets 0, 8, 12, 16, 20 */
m2s_status m2s_prune_budget(m2s_ctx* ctx, const m2s_budget_params* params, uint64_t* out_kept);
/* The last m2s_prune_budget: [0] records before, [1] candidates, [2] kept, [3] T (0 when nothing had to be selected), [4] kept with
 * key == T, [5] candidates with key == T. */
m2s_status m2s_last_budget_counts(const m2s_ctx* ctx, uint64_t out[6]);
/* Stages (ms) of the last profiled m2s_prune_budget: [0] keys + the four histogram / pick rounds, [1] flags + scans, [2] compaction. */
m2s_status m2s_last_budget_stage_ms(const m2s_ctx* ctx, float out_ms[3]);
/* The counterpart of m2s_upload_quad_sources for the accumulators: after m2s_contrib_begin, host arrays of n == m2s_num_stored words
 * become wmax and npix (either may be NULL: that accumulator stays as it is), so that a caller with an importance measure of its own
 * — or a test — drives the selection without rendering views.  M2S_ERR_INVALID for another n or a wmax word above 0x3F800000 (not
 * the bits of a weight in [0, 1]); M2S_ERR_STATE without accumulators of the current records. */
m2s_status m2s_upload_contrib(m2s_ctx* ctx, const uint32_t* host_wmax, const uint32_t* host_npix, uint64_t n);

/* ---- colour refit (no counterpart in the reference: its Gaussians keep the one texture sample the conversion gave them) -------- */
/* Carries the per-pixel colour error of the splat picture against the mesh picture of the same camera back to the records, over any
 * number of views, and applies it: one SART step dc_i = step * sum_p(w_i(p) e(p)) / sum_p(w_i(p)).  The pin (tests/refit_ref.py
 * restates it):
 *  - Planes.  Two uchar4[W * H] device images, row 0 = bottom: the target (NULL: attachment 2 of the mesh G-buffer, m2s_mesh_render)
 *    and the render (NULL: attachment 2 of the splat G-buffer, m2s_splat).  THE CALLER must have rendered the render plane from the
 *    context's current sorted quads in a colour mode (render mode 0 or 6): the pass recomputes the fragment weights from those quads
 *    and takes the picture they produced from the plane.  It does not read quad colours.
 *  - Pixel participation.  A pixel takes part iff the target's alpha byte is non-zero and the render's alpha byte sa >= min_cover
 *    (1..255).
 *  - Per-pixel error, integers only, per channel k with m the target byte and s the render byte: n = 4096 * (m * sa - 255 * s) (fits
 *    int32), d = 255 * sa, eq_k = floor((2 n + d) / (2 d)) — a floor division — clamped to [-4096, 4096]: e = m / 255 - s / sa, the
 *    error of the un-premultiplied splat colour, in steps of 1 / 4096, |e| <= 1 by the clamp.
 *  - Fragment weight.  Geometry, coverage, quad order, skipped quads, g = exp(alpha) (the device's fast exp) and w = sA3 * tA are those
 *    of m2s_contrib_accumulate, with A3 evolving byte-quantised exactly as there; a pixel under both triangles of a quad yields two
 *    fragments.  wq = (uint32)rintf(w * 65536.0f), 0..65536; the scaling by a power of two is exact.
 *  - Accumulation.  Four 64-bit words per record, num[3] (signed) and den (unsigned).  Per fragment on a participating pixel, for the
 *    record the quad was made from: num[k] += (int64)wq * eq_k, den += wq.  A pixel that does not take part adds nothing.  Integer sums:
 *    independent of the order of evaluation, identical from run to run.  A product is at most 2^28 in magnitude; a record has at most
 *    2^30 fragments over 256 views (m2s_contrib_accumulate's bound), so |num| < 2^58 and den < 2^46.  The words keep adding over calls
 *    (views).  Behind a saturated pixel w = +0 and wq = 0: the accumulators receive exactly nothing.
 * m2s_refit_begin sizes the accumulators to the context's current records, zeroes them and ties them to those records, exactly as
 * m2s_contrib_begin does, with its error cases.
 * m2s_refit_accumulate runs over the context's sorted quads and their sources at params->resolution.  out_counts (may be NULL):
 * [0] participating pixels, [1] (tile, quad) pairs.  Synchronous.  M2S_ERR_INVALID as m2s_contrib_accumulate — no m2s_refit_begin,
 * records that changed since it, missing sorted quads or sources, a resolution outside 1..8192, reserved != 0 — and for min_cover
 * outside 1..255; M2S_ERR_STATE for a NULL plane whose G-buffer is missing or not W x H (as m2s_score_frames). */
typedef struct m2s_refit_params {
    int32_t  resolution[2];
    uint32_t min_cover;     /* 1..255 */
    uint32_t reserved;      /* 0 */
} m2s_refit_params;         /* 16 bytes */
m2s_status m2s_refit_begin(m2s_ctx* ctx);
m2s_status m2s_refit_accumulate(m2s_ctx* ctx, const m2s_refit_params* params, const void* d_target, const void* d_render, uint64_t out_counts[2]);
/* dst_num: int64[3 * capacity_records], three words per record; dst_den: uint64[capacity_records]; either may be NULL.
 * M2S_ERR_STATE without valid accumulators, M2S_ERR_CAPACITY for fewer than m2s_num_stored records. */
m2s_status m2s_download_refit(m2s_ctx* ctx, int64_t* dst_num, uint64_t* dst_den, uint64_t capacity_records);
/* The counterpart of m2s_upload_contrib: after m2s_refit_begin, host arrays for n == m2s_num_stored records become num (3 n words) and
 * den (either may be NULL: it stays as it is), so that a caller with an error measure of its own — or a test — drives m2s_refit_apply
 * without rendering.  M2S_ERR_INVALID for another n; M2S_ERR_STATE without accumulators of the current records. */
m2s_status m2s_upload_refit(m2s_ctx* ctx, const int64_t* host_num, const uint64_t* host_den, uint64_t n);
/* which = 0: num, int64[3 * m2s_num_stored]; 1: den, uint64[m2s_num_stored].  NULL without valid accumulators. */
const void* m2s_device_refit(const m2s_ctx* ctx, uint32_t which);
/* The update, one lane per record.  D = llrint((double)min_weight_sum * 65536) on the host (saturating at 2^64 - 1).  A record with
 * den < D or den == 0 is left untouched; so is a channel whose colour is not finite.  Otherwise, per channel k, every operation in
 * fp64 and correctly rounded: dlt = (double)num_k / ((double)den * 4096.0) — the product is exact, the conversions round once —,
 * c' = (float)fmin(fmax((double)c + (double)step * dlt, 0.0), 1.0).  Only color[0..2] of the 96-byte record change: alpha and every
 * other field keep their bits.
 * Effect on the context, as m2s_prune: the records live in the context-owned pool afterwards (records adopted through
 * m2s_set_records are copied there first; the caller's memory is not written), the records epoch advances, and cached positions,
 * sorted quads, sources, the contribution accumulators, the refit accumulators and a baked SH plane (it was baked from the old albedo)
 * are invalidated.  out_counts (may be NULL): [0] records, [1] updated, [2] updated with at least one channel clamped, [3] left for
 * lack of weight.  Synchronous.  M2S_ERR_INVALID: a step that is not finite, a min_weight_sum that is negative or not finite,
 * reserved != 0; M2S_ERR_STATE without accumulators of the current records or with conversions in flight. */
typedef struct m2s_refit_apply_params {
    float    step;             /* the SART relaxation: converges for the linearised blend in (0, 2) */
    float    min_weight_sum;   /* in units of one fully weighted fragment */
    uint32_t reserved[2];      /* 0 */
} m2s_refit_apply_params;      /* 16 bytes */
m2s_status m2s_refit_apply(m2s_ctx* ctx, const m2s_refit_apply_params* params, uint64_t out_counts[4]);
/* Stages (ms) of the last profiled m2s_refit_accumulate: [0] setup + bin, [1] grouping (both m2s_splat's own), [2] the refit blend;
 * and the duration of the last profiled m2s_refit_apply. */
m2s_status m2s_last_refit_stage_ms(const m2s_ctx* ctx, float out_ms[3]);
float m2s_last_refit_apply_ms(const m2s_ctx* ctx);

/* ---- merge pass (no counterpart in the reference: its density is chosen once, before the conversion) ---------------------------- */
/* Replaces groups of neighbouring records by one record that covers what they covered: level of detail without holes, for records of
 * any origin (converted, pruned, refitted, uploaded, adopted).  A record is read as what the conversion made it, a flat rectangular
 * texel footprint with edges scale[0], scale[1] along axes 1 and 2 of its rotation, uniform density, second moment
 * diag(sx^2 / 12, sy^2 / 12, 0) in its own axes; the parent is the moment-matched rectangle of the union (four h x h tiles in a
 * 2 x 2 block give the 2h x 2h record that half the density would have produced).  The axes are the viewer's: r_1, r_2, r_3 = the rows
 * of castQuatToMat3 of the stored four floats (x, y, z, w) = rotation[0..3], no normalisation,
 *    r_1 = (1 - 2(zz + ww), 2(yz + xw), 2(yw - xz)), r_2 = (2(yz - xw), 1 - 2(yy + ww), 2(zw + xy)), r_3 = (2(yw + xz), 2(zw - xy), 1 - 2(yy + zz)),
 * so that the viewer's covariance is sum_i s_i^2 r_i r_i^T; for a conversion's record r_3 is its normal and r_1, r_2 run along the
 * triangle's Ju, Jv.  The pin (tests/merge_ref.py restates it):
 *  1. Order.  Validity, box, key and the stable sort are pins 1 - 4 of the compact export (below), the same functions.  Invalid records
 *     carry the key 2^30 and sort behind every valid record, in index order.  The sorted sequence is j = 0 .. n-1 with perm[j].
 *  2. Runs.  Position j starts a run iff j == 0, or record j or j-1 is invalid, or key_j >> (3 level) != key_{j-1} >> (3 level), or
 *     !(d >= min_axis_dot) with d = ((a0 b0) + a1 b1) + a2 b2 in fp32 without contraction, a and b the r_3 of the two records evaluated
 *     in fp32 exactly as written above (one rounding per operation).  A NaN breaks the run.
 *  3. Segments.  A run is cut every max_group members: j is a segment head iff (j - run_start) % max_group == 0.  The number of heads
 *     is the number of records afterwards; segment s becomes record s.  (Integer logic and exact fp32: reproducible bit for bit.)
 *  4. A segment of one member is copied byte for byte; every invalid record is such a segment, so they are kept, at the end, unchanged.
 *  5. A segment of members i = 1..m >= 2, in sorted order, all arithmetic in fp64 (the r_k above evaluated in fp64 from the stored
 *     floats), every field rounded to fp32 once:
 *       w_i = sx_i sy_i, or 1 for every member where their sum is 0; W = sum w_i;  d_i = p_i - p_1, mu = sum w_i d_i / W;
 *       position = p_1 + mu, position[3] = the first member's;
 *       nb = sum w_i r3_i, or the first member's r_3 where |nb|^2 is 0 or not finite; normalised ((0, 0, 1) where that fails too);
 *       t1 = the first member's r_1 minus its component along nb, normalised — its r_2 instead where less than 1e-12 |r_1|^2 of the
 *       squared length is left —, t2 = nb x t1;
 *       M = sum w_i (A_i + (d_i - mu)(d_i - mu)^T) / W with A_i = (sx_i^2 / 12) r1 r1^T + (sy_i^2 / 12) r2 r2^T;
 *       a = t1^T M t1, b = t1^T M t2, c = t2^T M t2;  dl = sqrt((a - c)^2 + 4 b^2), l1 = (a + c + dl) / 2, l2 = max((a + c - dl) / 2, 0);
 *       e1 = t1 where dl == 0, else the normalised one of (b, l1 - a) and (l1 - c, b) (coordinates along t1, t2) with the larger squared
 *       length, the first on a tie; e2 = nb x e1;
 *       scale = (sqrt(12 l1), sqrt(12 l2), the first member's scale[2], scale[3]);
 *       rotation = the quaternion of the matrix with columns e1, e2, nb by the branch selection of the conversion's quat_cast
 *       (converterGS.glsl:131-183), stored (w, x, y, z) as the conversion stores it, negated as a whole where w < 0;
 *       alpha = sum w_i alpha_i / W;  rgb = sum w_i alpha_i c_i / sum w_i alpha_i, or sum w_i c_i / W where that denominator is 0;
 *       normal.xyz = the normalised sum w_i normal_i, all zeros where the sum is zero or not finite; normal[3], pbr[2], pbr[3] are the
 *       first member's; pbr[0..1] = sum w_i pbr_i / W.
 *     (Plain moment matching of the rendered Gaussians' covariances is NOT this: it shrinks a 2 x 2 block to 0.82 h where 1.3 h is needed.)
 *  5s. The baked SH plane (tests/merge_sh_ref.py restates it).  With m2s_set_carry_sh on, a call that is no dry run, and a plane of
 *     exactly the current n records (a bake of them, m2s_upload_sh, or what an earlier call under this pin left):
 *     5s.1 Segments are pin 3's (pin 2u's with M2S_MERGE_UNSIGNED_AXIS), unchanged: the plane is never read by the heads.  SH has no axis
 *          sign to lose, so 5s is the same under both rules.
 *     5s.2 A segment of one member: its 48 floats are copied bit for bit.  Invalid records are such segments.
 *     5s.3 A segment of members i = 1..m >= 2 in sorted order, every product and sum in fp64 from the stored floats, in member order:
 *          w_i = sx_i sy_i, W = sum w_i; where W == 0, w_i = 1 for every member and W = m (pin 5's own test, the same value);
 *          a_i = w_i alpha_i, A = sum a_i; for k = 0..47: sh'_k = (float)(sum a_i sh_ik / A) where A != 0, else
 *          (float)(sum w_i sh_ik / W) — the selector pin 5 uses for rgb; one rounding to fp32 per coefficient.  All 48 columns are
 *          merged whatever the bake's degree: those above it are zero and stay zero for finite weights.  The colour 0.5 + sum_k sh_k
 *          B_k(dir) is linear in the coefficients, so the parent's colour in every direction is the same weighted mean of its
 *          members' colours in that direction that pin 5 takes of rgb.
 *     5s.4 Afterwards the context is as pin 7 leaves it, except for the plane: it is the parents' plane, in segment order, valid for the
 *          n' parents, its degree kept, its tap counts gone (as after a prune that compacts a plane).
 *     5s.5 Switch off, no such plane, or a dry run: nothing of this happens — the bytes, the invalidation and the plane dropped are pin 7's.
 *  6. Output order is segment order: the canonical (mesh, triangle, row, column) order of a conversion is gone afterwards.
 *  7. Effect on the context, as m2s_prune: the parents are written into the context-owned pool (through a staging buffer where the
 *     sources live there; adopted memory is never written), the resolutionTarget is kept, the records epoch advances; cached positions,
 *     sorted quads, sources, the contribution and refit accumulators and a baked SH plane (as by m2s_refit_apply: it is not merged
 *     — unless pin 5s applies) are invalidated.  With M2S_MERGE_DRY_RUN nothing of the context changes: only the counts are produced.
 *  8. out_counts (may be NULL): [0] records before, [1] records after, [2] segments with two members or more, [3] invalid records
 *     carried.  The counts are monotone in level (a coarser cell only removes run breaks).
 * With M2S_MERGE_UNSIGNED_AXIS the sign of r_3 carries no meaning, as it carries none for the viewer (its covariance is
 * sum s_i^2 r_i r_i^T) and as the conversion leaves it: the two triangles of a flat quad may store r_3 = +n and -n (tests/
 * merge_unsigned_ref.py restates these two pins; DESIGN 5.18 has what the signed rule does to a conversion).  Off by default.
 *  2u. Runs.  d is pin 2's, the same fp32 expression; position j starts a run iff one of pin 2's other conditions holds or
 *     !(fabsf(d) >= min_axis_dot).  A NaN still breaks the run; min_axis_dot <= 0 still never breaks on the axis.  The breaks are a
 *     subset of pin 2's on the same input, so records after is never larger than without the flag.
 *  5u. In the walk over a segment's members in sorted order their third rows are oriented one after the other: o_1 = r3_1, and for
 *     i >= 2 o_i = -r3_i where dot(r3_i, o_{i-1}) < 0, else r3_i (a zero or a NaN does not flip), the dot in fp64 from the fp64 rows
 *     above as (x x + y y) + z z without contraction.  o_i takes the place of r3_i in nb's sum, with either weighting; everything else
 *     of pin 5 is as it is (A_i is made of r_1, r_2, which have no sign to lose; the fallback is still the first member's r_3).  The
 *     parent's r_3 lies on the first member's side, so a chain of merges is well defined.  The orientation goes against the member
 *     before, not the first: the run rule bounds the angle between neighbours, not across a group of 64.
 *     Segments, pins 3, 4, 6, 7, 8, the map, the dry run and the monotonicity in level are unchanged.
 * Synchronous.  M2S_ERR_INVALID: level > 10, max_group outside 2..64, a NaN min_axis_dot, unknown flag bits, reserved != 0.
 * M2S_ERR_STATE: no records, or conversions in flight.  M2S_ERR_CAPACITY: 2^32 records or more. */
/* The valid flags are 0, 1, 4, 5.  Bit 1 (value 2) names nothing and stays refused: flags 2 and 3 were M2S_ERR_INVALID before the second
 * flag existed and callers may rely on it, so the second flag took bit 2. */
enum { M2S_MERGE_DRY_RUN = 1, M2S_MERGE_UNSIGNED_AXIS = 4 };
typedef struct m2s_merge_params {
    uint32_t level;          /* 0..10: cell = key >> (3 * level) */
    uint32_t max_group;      /* 2..64: members per parent, at most */
    float    min_axis_dot;   /* a run breaks where !(dot(r3_j, r3_prev) >= min_axis_dot); NaN refused */
    uint32_t flags;          /* M2S_MERGE_DRY_RUN = 1 | M2S_MERGE_UNSIGNED_AXIS = 4; other bits 0 */
    uint32_t reserved[2];    /* 0 */
} m2s_merge_params;          /* 24 bytes */
m2s_status m2s_merge(m2s_ctx* ctx, const m2s_merge_params* params, uint64_t out_counts[4]);
/* The counts of the last m2s_merge (a dry run included), and its stages (ms): [0] keys + sort, [1] heads + scans, [2] reduce + adopt
 * (0 for a dry run). */
m2s_status m2s_last_merge_counts(const m2s_ctx* ctx, uint64_t out[4]);
m2s_status m2s_last_merge_stage_ms(const m2s_ctx* ctx, float out_ms[3]);
/* The switch of pins 5s (m2s_merge), 4s (m2s_lod_build) and 3s (the cuts): a baked SH plane of the records is carried through them
 * instead of dropped.  Off by default; with it off every entry point behaves as it did before the switch existed.  m2s_carry_sh: 1 / 0.
 * m2s_last_merge_sh_ms: the SH reduction of the last m2s_merge (ms; 0 where none ran); it lies inside stage [2] above. */
m2s_status m2s_set_carry_sh(m2s_ctx* ctx, int enabled);
int m2s_carry_sh(const m2s_ctx* ctx);
float m2s_last_merge_sh_ms(const m2s_ctx* ctx);
/* The map of the last merge that was not a dry run: a uint32 per record of the order before it, the index of its parent in the order
 * after it.  Valid until the records change again (NULL / M2S_ERR_STATE then); the maps of a chain of merges compose into a hierarchy.
 * m2s_download_merge_map: *out_n (may be NULL) = its entries; dst NULL with capacity 0 only asks for that; M2S_ERR_CAPACITY for a
 * smaller destination. */
const void* m2s_device_merge_map(const m2s_ctx* ctx);
m2s_status m2s_download_merge_map(m2s_ctx* ctx, uint32_t* dst, uint64_t capacity, uint64_t* out_n);
/* The record model of m2s_merge, m2s_lod_build and everything built on them.  M2S_MERGE_MODEL_FOOTPRINT (the default) is the pin above:
 * right for what the conversion emits.  M2S_MERGE_MODEL_GAUSSIAN reads a record as the viewer draws one of any other origin
 * (m2s_read_ply, m2s_upload_records, m2s_prepass_params.format = 1): a 3D Gaussian with three standard deviations sigma |scale[k]| along
 * r_1, r_2, r_3 and covariance C = sigma^2 sum_k s_k^2 r_k r_k^T.  sigma multiplies every stored scale before it is read as a standard
 * deviation in the units of the positions: 1 for a .ply (it holds the drawn deviations), gaussian_std for a conversion behind
 * m2s_records_to_world_units.  A parent's covariance is the sum of a term that scales with sigma^2 and the spread of the members'
 * positions, which does not: the merge must know sigma.  Under FOOTPRINT every entry point behaves as it did before the switch existed
 * and sigma is not read.  The switch invalidates nothing; a tree remembers the model and sigma it was built under.  No flag bit is
 * involved: the valid flag words of m2s_merge and m2s_lod_build are what they were.
 * M2S_ERR_INVALID: a model other than 0 or 1, a sigma that is NaN, infinite or <= 0.  M2S_ERR_STATE: conversions in flight.
 * Under M2S_MERGE_MODEL_GAUSSIAN pins 1, 3, 4, 6, 7, 8 of m2s_merge hold unchanged and (tests/merge_gauss_ref.py restates these):
 *  2g. Runs.  The axis of a record is the row r_k whose |scale[k]| is smallest: k = 0; k = 1 where |scale[1]| < |scale[0]|; k = 2 where
 *     |scale[2]| < |scale[k]| — the lower k on a tie (m2s_prepass's choice for format 1, except that a tie of the two smaller scales
 *     goes to the lower of THEM; a flat record, scale[2] = 0, has its r_3).  The rows in fp32 exactly as written in front of pin 1, one
 *     rounding per operation.  Position j starts a run iff one of pin 2's other conditions holds or !(fabsf(d) >= min_axis_dot), d the
 *     fp32 dot of the two axes as in pin 2.  The rule is always sign-free: M2S_MERGE_UNSIGNED_AXIS is accepted and changes nothing.
 *  5g. A segment of members i = 1..m >= 2 in sorted order, all arithmetic in fp64 from the stored floats without contraction, every
 *     field rounded to fp32 once:
 *       a_i = the product of the two largest of |s_i1|, |s_i2|, |s_i3| (the splat's area measure; |sx sy| for a flat record);
 *       w_i = a_i, or 1 for every member where their sum is 0;  W, d_i, mu, position as in pin 5;
 *       C_i = sigma^2 ((s_i1^2 r1 r1^T + s_i2^2 r2 r2^T) + s_i3^2 r3 r3^T), sigma the float widened, sigma^2 its fp64 square;
 *       M = sum w_i (C_i + (d_i - mu)(d_i - mu)^T) / W, symmetric, held as six doubles m00, m01, m02, m11, m12, m22.
 *       Eigenpairs by cyclic Jacobi rotations.  V = the identity.  A sweep visits the pairs (p, q) = (0, 1), (0, 2), (1, 2) in this
 *       order; the iteration stops in front of a sweep where m01, m02, m12 are all exactly 0, and after 16 sweeps.  A pair with
 *       m_pq == 0 is skipped; otherwise, with r the third index,
 *         theta = (m_qq - m_pp) / (2 m_pq);  t = sgn / (|theta| + sqrt(theta^2 + 1)), sgn = -1 where theta < 0, else 1;
 *         c = 1 / sqrt(t^2 + 1), s = t c;  m_pp -= t m_pq, m_qq += t m_pq (both with the old m_pq), then m_pq = 0 exactly;
 *         (m_rp, m_rq) = (c m_rp - s m_rq, s m_rp + c m_rq);  for k = 0..2: (V_kp, V_kq) = (c V_kp - s V_kq, s V_kp + c V_kq)
 *       (a theta that overflows gives t = 0: the element is dropped).  l_k = max(m_kk, 0) with eigenvector column k of V.  The pairs
 *       are sorted descending in l, the lower original index first on a tie (three compare-and-swaps of neighbours, (0,1), (1,2),
 *       (0,1), each only where the later one is strictly larger); e1, e2 = the first two eigenvectors, e3 = e1 x e2;
 *       scale = (sqrt(l1) / sigma, sqrt(l2) / sigma, sqrt(l3) / sigma, the first member's scale[3]);
 *       rotation = pin 5's quat_cast of the matrix with columns e1, e2, e3, stored the same way;
 *       rgb, normal, pbr, normal[3], pbr[2..3]: pin 5's rules with these w_i;
 *       alpha = min(1, sum a_i alpha_i / a_p) — alpha-weighted area is conserved — with a_p = (sqrt(l1) / sigma)(sqrt(l2) / sigma) in
 *       fp64; where a_p is 0 or not finite, pin 5's mean sum w_i alpha_i / W.  (The a_i here are the areas themselves: under the
 *       unit weights every one of them is 0 and so is alpha, where a_p > 0.)
 *     Valid records are finite and their squares fit fp64, so M is finite: there is no other fallback.  Two coincident identical records
 *     give their own scales and twice their alpha; a 2 x 2 block of flat records of deviation s at spacing h gives in-plane variance
 *     s^2 + h^2 / 4 and thickness 0.
 *  5sg. The SH plane: pin 5s with w_i = a_i of pin 5g (and 1 where their sum is 0).  Everything else of 5s is unchanged.
 *  4g. Tree bounds (m2s_lod_build): e = sigma * fmaxf(fmaxf(|scale[0]|, |scale[1]|), |scale[2]|) in fp32, one rounding for the product:
 *     tau_px counts one standard deviation in pixels.  The cuts read only bounds and parents and are what they were.  m2s_lod_blend on
 *     a tree built under this model returns M2S_ERR_STATE: its eight frame turns and its axis-by-axis lerp assume the footprint's axis
 *     order (scale[2] a thickness along r_3), which pin 5g's descending order does not keep. */
enum { M2S_MERGE_MODEL_FOOTPRINT = 0, M2S_MERGE_MODEL_GAUSSIAN = 1 };
m2s_status m2s_set_merge_model(m2s_ctx* ctx, uint32_t model, float sigma);
uint32_t m2s_merge_model(const m2s_ctx* ctx);
float m2s_merge_sigma(const m2s_ctx* ctx);

/* ---- level-of-detail tree and its per-camera cut (no counterpart in the reference, which draws every Gaussian it converted) ------- */
/* m2s_lod_build keeps a chain of m2s_merge steps resident and linked; m2s_lod_select takes a cut through it for one camera: each part
 * of the surface exactly once, as coarse as the camera allows.  Integer logic and exact fp32 throughout: reproducible bit for bit
 * (tests/lod_ref.py restates it).  The tree, pinned:
 *  1. Leaves.  The context's current records are the leaves, tree level 0, copied in their own order into a node pool the tree owns.
 *  2. Steps.  Step s = 0 .. n_steps-1 runs m2s_merge's own code with (levels[s], max_group, min_axis_dot, flags) on what the previous step
 *     left.  Its parents are appended to the pool as the next tree level, in segment order; for a node i of the level below,
 *     parent[i] = first[next] + map[i - first[this]] with map the merge's map.  Nodes of the last level have M2S_LOD_NO_PARENT.
 *  3. A step that merges nothing — its merge would leave as many records as it found — is not applied (as M2S_MERGE_DRY_RUN): it adds
 *     no level, is counted, and the records stay in the order of the level below.  (Applied, it would only permute them: the stable
 *     sort of the next step arrives at the same sequence either way, so the levels above are the same bytes.)
 *  4. Bounds.  Every node also has a 16-byte entry (x, y, z, e): position[0..2] and e = fmaxf(fabsf(scale[0]), fabsf(scale[1])), the
 *     longer edge of the flat footprint m2s_merge reads a record as.  The cut reads this plane, never the 96-byte records.
 *  4s. The SH plane.  With m2s_set_carry_sh on and a baked plane of the current records at the build, the tree also owns
 *     float[nodes][48]: the leaves' rows copied in leaf order, and behind them the rows pin 5s of m2s_merge made for every step that
 *     merged (a step that merges nothing adds none); the tree remembers the plane's degree.  Afterwards the context's plane is the last
 *     level's, or untouched where no step merged.  A tree built otherwise has no plane.  The plane costs 192 bytes per node beside the
 *     116 of the other three: 2.4 GB for a tree of 12.68 M nodes, 0.8 GB for one of 4.23 M.
 *  5. Afterwards.  Where a step merged, the context's current records are the last level — what the chain left, in the context-owned
 *     pool — with everything m2s_merge invalidates invalid; where none did they are untouched.  The tree is a copy: it stays valid until
 *     the next m2s_lod_build (one refused for its arguments or the context's state leaves it; one that fails later leaves no tree),
 *     m2s_lod_release or m2s_destroy, whatever happens to the current records.  The resolutionTarget of the leaves is remembered.
 *     m2s_last_merge_counts reports the last step.  Scales are read as stored, as by m2s_merge: a conversion's are in units the
 *     viewer divides by the resolutionTarget (Limits) until m2s_records_to_world_units has divided them.
 *  6. out_counts (may be NULL): [0] leaves, [1] nodes, [2] tree levels (the leaves included), [3] steps that added no level.
 * Synchronous.  M2S_ERR_INVALID: n_steps outside 1..16, a level above 10, levels that decrease, a level past n_steps that is not 0,
 * max_group outside 2..64, a NaN min_axis_dot, flags other than 0 or M2S_MERGE_UNSIGNED_AXIS (M2S_MERGE_DRY_RUN too: a build is no dry
 * run).  M2S_ERR_STATE: no records, or conversions in flight.  M2S_ERR_CAPACITY:
 * 2^32 - 1 nodes or more.  Zero records build an empty tree of one level. */
#define M2S_LOD_MAX_STEPS 16
#define M2S_LOD_NO_PARENT 0xFFFFFFFFu
typedef struct m2s_lod_build_params {
    uint32_t n_steps;                    /* 1..16 */
    uint32_t levels[M2S_LOD_MAX_STEPS];  /* merge level of step s: 0..10, non-decreasing; entries past n_steps are 0 */
    uint32_t max_group;                  /* 2..64, as m2s_merge */
    float    min_axis_dot;               /* as m2s_merge; NaN refused */
    union {                              /* one word; `reserved` is the name it had while its only value was 0, kept for existing callers */
        uint32_t flags;                  /* 0 or M2S_MERGE_UNSIGNED_AXIS (every step merges with pins 2u, 5u); any other value refused */
        uint32_t reserved;
    };
} m2s_lod_build_params;                  /* 80 bytes */
m2s_status m2s_lod_build(m2s_ctx* ctx, const m2s_lod_build_params* params, uint64_t out_counts[4]);
/* The tree's levels: first[l] is the first node of level l = 0 .. *out_levels - 1, first[*out_levels] and every entry behind it the
 * node count (either pointer may be NULL).  M2S_ERR_STATE without a tree. */
m2s_status m2s_lod_levels(const m2s_ctx* ctx, uint32_t* out_levels, uint64_t first[M2S_LOD_MAX_STEPS + 2]);
/* which = 0: the node records (96 bytes each), 1: parent, a uint32 per node, 2: the bounds, a float4 per node.  m2s_device_lod: NULL
 * without a tree, for an empty one and for another `which`.  m2s_download_lod: M2S_ERR_STATE without a tree, M2S_ERR_CAPACITY for a
 * destination of fewer bytes than the plane. */
const void* m2s_device_lod(const m2s_ctx* ctx, uint32_t which);
m2s_status m2s_download_lod(m2s_ctx* ctx, uint32_t which, void* dst, uint64_t capacity_bytes);
/* The tree's SH plane (pin 4s), float[nodes][48] in node order.  m2s_device_lod_sh: NULL without a tree, without a plane, for an empty
 * tree.  m2s_download_lod_sh: the errors of m2s_download_lod (capacity in rows), M2S_ERR_STATE for a tree without a plane;
 * *out_degree (may be NULL) = the plane's degree. */
const void* m2s_device_lod_sh(const m2s_ctx* ctx);
m2s_status m2s_download_lod_sh(m2s_ctx* ctx, float* dst, uint64_t capacity_rows, uint32_t* out_degree);
/* Frees the tree, its SH plane included (M2S_OK without one too).  The current records are not touched. */
m2s_status m2s_lod_release(m2s_ctx* ctx);
/* Duration (ms) of the last m2s_lod_build, its merges and host round trips included. */
float m2s_last_lod_build_ms(const m2s_ctx* ctx);

/* The cut, pinned:
 *  1. Per node, all in fp32, one rounding per operation, no contraction, no division, no root, with (cx, cy, cz) = camera_position:
 *       dx = x - cx, dy = y - cy, dz = z - cz;  d2 = fmaxf((dx*dx + dy*dy) + dz*dz, near*near);  s = e * focal_px;
 *       refine = (s * s > (tau_px * tau_px) * d2).
 *     The comparison is false for any NaN; equality does not refine; fmaxf returns its other operand for a NaN (a node whose position
 *     is NaN is taken to be `near` away).  The distance is to the camera POSITION, not the view depth: turning the camera changes no
 *     cut, and nodes behind it are not refined to the leaves.
 *  2. A node is selected iff it is a leaf or does not refine, and every proper ancestor refines.  Walking from a node of the last level
 *     towards any leaf, the first node that is a leaf or does not refine is the selected one: every leaf has exactly one selected
 *     ancestor-or-self, whatever the sizes do along the chain — no holes, nothing drawn twice.  Invalid records, which m2s_merge
 *     carries through every level as byte-identical singletons, come out once.
 *  3. Output: the stable compaction of the selected nodes, in node-index order (the leaves in their own order, then level 1, ...),
 *     into the context-owned pool.  They become the context's current records at the leaves' resolutionTarget; the records epoch
 *     advances, everything m2s_prune invalidates is invalid, and a baked SH plane is dropped.  Memory adopted through m2s_set_records
 *     is not written.  The tree is not changed.
 *  3s. Where the tree has an SH plane (pin 4s of the tree) and the call is no dry run, the rows of the selected nodes go into the
 *     context's plane instead, compacted in the same node-index order by the same flags and offsets as the records: the plane is valid
 *     for the selected records, its degree is the tree's, it has no tap counts.  Zero selected nodes under a frustum give an empty
 *     plane, which is valid.  m2s_lod_select, m2s_lod_select_budget and their _frustum forms behave alike.  The tree's property
 *     decides, not m2s_set_carry_sh at the time of the cut; a tree without a plane cuts exactly as pin 3 says.
 *  4. out_counts (may be NULL): [0] nodes, [1] selected, [2] selected leaves, [3] nodes with `refine` (whatever their ancestors do).
 *     Integer sums, identical from run to run.
 *  5. With M2S_LOD_DRY_RUN only the counts are produced: nothing of the context changes.
 * Synchronous.  M2S_ERR_INVALID: a camera position, focal_px, tau_px or near that is not finite, focal_px <= 0, tau_px < 0, near <= 0,
 * unknown flag bits, reserved != 0.  M2S_ERR_STATE: no tree, or conversions in flight.  No frustum culling here: m2s_lod_select_frustum
 * (below) takes the same cut over the nodes a camera can see. */
enum { M2S_LOD_DRY_RUN = 1 };
typedef struct m2s_lod_select_params {
    float    camera_position[3];  /* world space, finite */
    float    focal_px;            /* view_to_clip[5] * H / 2; finite, > 0 */
    float    tau_px;              /* finite, >= 0: the longer edge of a drawn node projects to at most this many pixels */
    float    near;                /* finite, > 0: distances below it count as it */
    uint32_t flags;               /* M2S_LOD_DRY_RUN; other bits 0 */
    uint32_t reserved;            /* 0 */
} m2s_lod_select_params;          /* 32 bytes */
m2s_status m2s_lod_select(m2s_ctx* ctx, const m2s_lod_select_params* params, uint64_t out_counts[4]);
/* The selected nodes per tree level of the last m2s_lod_select (a dry run included; levels the tree does not have: 0), and the stages
 * (ms) of the last profiled one: [0] the sweep over the levels, [1] scan + node indices, [2] compaction (the round trip of the counts
 * included); [1] and [2] are 0 for a dry run. */
m2s_status m2s_last_lod_level_counts(const m2s_ctx* ctx, uint64_t out[M2S_LOD_MAX_STEPS + 1]);
m2s_status m2s_last_lod_select_stage_ms(const m2s_ctx* ctx, float out_ms[3]);
/* The node index of every record the last m2s_lod_select that was not a dry run left, a uint32 each, in their order.  Valid until the
 * records change again (NULL / M2S_ERR_STATE then).  m2s_download_lod_nodes: as m2s_download_merge_map. */
const void* m2s_device_lod_nodes(const m2s_ctx* ctx);
m2s_status m2s_download_lod_nodes(m2s_ctx* ctx, uint32_t* dst, uint64_t capacity, uint64_t* out_n);

/* The cut that fits a budget: the finest cut of m2s_lod_select that holds at most max_records records for this camera, found on the
 * device in a handful of passes over the bounds (tests/lod_budget_ref.py restates it).  Pinned:
 *  1. Keys.  A key k is the bits of a non-negative finite float, 0 .. 0x7F7FFFFF; "at key k" means m2s_lod_select's comparison (pin 1
 *     of the cut) evaluated with tau_px = the float whose bits are k.  tau_px * tau_px and its product with d2 do not decrease with k,
 *     roundings included, so per node the comparison is true below one key and false from it on.
 *  2. T(i) is the smallest key at which node i does not refine (at 0x7F7FFFFF none does: tau_px * tau_px is +inf, the product +inf or
 *     NaN).  H(i) is the minimum of T over the proper ancestors of i, 0xFFFFFFFF on the last level.  L(i) is 0 for a leaf, else T(i).
 *     Pin 2 of the cut then reads: node i is selected at key k iff L(i) <= k < H(i), and
 *       count(k) = #{i: L(i) < H(i), L(i) <= k} - #{i: L(i) < H(i), H(i) <= k}
 *     is the number of records the cut at key k holds.  It does not increase with k; count(0x7F7FFFFF) is the size of the last level.
 *  3. Result.  N_eff = max(max_records, nodes of the last level); key* = the smallest key with count(key) <= N_eff, raised to the key
 *     of tau_min_px where that is larger; tau_px = the float of key*; met = (count(key*) <= max_records); selected_finer =
 *     count(key* - 1), the cut that did not fit, or count(key*) where key* is 0 or the floor decided.
 *  4. Every effect on the context is m2s_lod_select's at that tau_px: out_counts, m2s_last_lod_level_counts, m2s_device_lod_nodes, the
 *     record bytes and their order, what is invalidated, the resolutionTarget handed back, the tree untouched, and with M2S_LOD_DRY_RUN
 *     nothing of the context changes.  A caller who passes the returned tau_px to m2s_lod_select gets the same bytes.
 *  5. An empty tree gives tau_px = tau_min_px, met = 1 and 0 selected.
 * Integer sums throughout: the same result from run to run.  Synchronous.  Errors as m2s_lod_select; in addition max_records == 0 and
 * a tau_min_px that is negative or not finite are M2S_ERR_INVALID.  `out` may be NULL. */
typedef struct m2s_lod_budget_params {
    float    camera_position[3];  /* as m2s_lod_select_params */
    float    focal_px;            /* finite, > 0 */
    float    near;                /* finite, > 0 */
    float    tau_min_px;          /* finite, >= 0: never cut finer than this, even where the budget allows (0: no floor) */
    uint32_t max_records;         /* >= 1 */
    uint32_t flags;               /* M2S_LOD_DRY_RUN; other bits 0 */
} m2s_lod_budget_params;          /* 32 bytes */
typedef struct m2s_lod_budget_result {
    float    tau_px;              /* the tau the cut was taken at */
    uint32_t met;                 /* 1: selected <= max_records */
    uint64_t selected_finer;      /* count at the next smaller key (the cut that did not fit); = selected where key* is 0 or the floor decided */
} m2s_lod_budget_result;          /* 16 bytes */
m2s_status m2s_lod_select_budget(m2s_ctx* ctx, const m2s_lod_budget_params* params, m2s_lod_budget_result* out, uint64_t out_counts[4]);
/* The stages (ms) of the last profiled m2s_lod_select_budget: [0] thresholds + ancestor minima, [1] the four select rounds, [2] the cut
 * (m2s_lod_select's three stages summed). */
m2s_status m2s_last_lod_budget_stage_ms(const m2s_ctx* ctx, float out_ms[3]);

/* The two cuts over what a camera sees: nodes with no leaf inside the view frustum are not selected, so they are neither compacted,
 * keyed and sorted only for m2s_prepass to discard them, nor charged to a record budget (tests/lod_frustum_ref.py restates it).  Pinned:
 *  1. Leaf test.  For leaf i with bound (x, y, z, e), in fp32, one rounding per operation, mat4 * vec4 as (m0*x + m1*y) + (m2*z + m3*w):
 *       ws = model_to_world * (x, y, z, 1);  vs = world_to_view * (ws.xyz, 1);  c = view_to_clip * vs;  clip = guard_band * c.w;
 *       inside = !(c.z < -clip || c.x < -clip || c.x > clip || c.y < -clip || c.y > clip).
 *     Every comparison is false for a NaN: such a leaf is inside, as in the viewer's shader.  With guard_band == 1.05f this is
 *     m2s_prepass's own test operation for operation: the leaves outside are exactly the records m2s_prepass culls with the same
 *     three matrices and no depth image.
 *  2. Visibility.  vis(i) = inside(i) for a leaf; for a node above the leaves vis is the OR of vis over the nodes whose parent word
 *     names it.  A node is visible iff a leaf below it is inside; the position of a node above the leaves is never tested.  (Testing
 *     each node's own position instead would let the number of selected nodes rise with tau_px, and the budget search has no answer
 *     then: DESIGN 5.22.)
 *  3. The cut.  A node is selected iff pin 2 of m2s_lod_select selects it and vis(i).  Every inside leaf has exactly one selected
 *     ancestor-or-self; every selected node has an inside leaf below it; `refine` is evaluated exactly as by m2s_lod_select.
 *  4. Everything else is m2s_lod_select's: output order, adoption, what is invalidated, m2s_device_lod_nodes, M2S_LOD_DRY_RUN, the tree
 *     untouched.  out_counts: [0] nodes, [1] selected, [2] selected leaves, [3] nodes with `refine` (unmasked).
 *     m2s_last_lod_level_counts reports the counts after masking.  Zero selected is a valid result: the context then holds 0 records,
 *     as after an m2s_prune that kept none.
 *  5. The budget.  Pin 2 of m2s_lod_select_budget with "L(i) < H(i)" read as "L(i) < H(i) and vis(i)": count(0x7F7FFFFF) is the number
 *     of visible nodes of the last level, N_eff the larger of max_records and that number; key*, the floor, met and selected_finer are
 *     as there, and the cut is pin 3 above at that tau_px.  With no leaf inside: key* = 0 raised to the floor, 0 selected, met 1,
 *     selected_finer 0.
 *  6. camera_position is, as for the plain cuts, in the records' own space.  Keeping it consistent with the matrices is the caller's
 *     business and is not checked.
 *  7. Errors: those of m2s_lod_select / m2s_lod_select_budget, and M2S_ERR_INVALID for a NULL frustum, a matrix entry that is not
 *     finite, a guard_band that is not finite or below 1, a reserved word that is not 0.
 * Where the two rules part from m2s_prepass, which tests the selected node's own position afterwards: a node above the leaves whose
 * own position passes but none of whose leaves do is not selected, and one whose position fails but which has a leaf inside is
 * selected and culled by the prepass.  Both sit at the guard band's border; a larger guard_band widens the test. */
typedef struct m2s_lod_frustum {
    float    model_to_world[16];  /* as m2s_prepass_params, column-major; finite */
    float    world_to_view[16];
    float    view_to_clip[16];
    float    guard_band;          /* finite, >= 1; 1.05f is the prepass's own */
    uint32_t reserved[3];         /* 0 */
} m2s_lod_frustum;                /* 208 bytes */
m2s_status m2s_lod_select_frustum(m2s_ctx* ctx, const m2s_lod_select_params* params, const m2s_lod_frustum* frustum, uint64_t out_counts[4]);
m2s_status m2s_lod_select_budget_frustum(m2s_ctx* ctx, const m2s_lod_budget_params* params, const m2s_lod_frustum* frustum,
                                         m2s_lod_budget_result* out, uint64_t out_counts[4]);
/* Of the last of the two calls above (a dry run included): [0] leaves inside, [1] nodes the plain cut selects at that tau_px and this
 * one dropped.  m2s_last_lod_frustum_ms: the visibility stage (ms) of the last profiled one. */
m2s_status m2s_last_lod_frustum_counts(const m2s_ctx* ctx, uint64_t out[2]);
float      m2s_last_lod_frustum_ms(const m2s_ctx* ctx);

/* The two frustum cuts behind an occluder: a leaf counts as inside only if it passes the frustum test AND is not behind a depth image
 * under m2s_prepass's own depth test, so that the leaves on the far side of a closed mesh are neither selected nor charged to a record
 * budget (tests/lod_occlusion_ref.py restates it).  Pinned, on top of the pins of the frustum cuts above:
 *  1. Leaf test.  For leaf i with bound (x, y, z, e) and alpha = color[3] of its node record (tree plane 0): c and inside_frustum exactly
 *     as in pin 1 above.  Where inside_frustum holds, in fp32, one rounding per operation, IEEE division:
 *       u = (c.x / c.w) * 0.5f + 0.5f;  v = (c.y / c.w) * 0.5f + 0.5f;
 *       ti = clamp(floorf(u * (float)depth_w));  tj = clamp(floorf(v * (float)depth_h));   (m2s_prepass's clamp: below 0 and NaN give 0,
 *                                                                                            at or above the size gives size - 1)
 *       d = depth[tj * depth_w + ti];  my = (c.z / c.w) * 0.5f + 0.5f;  behind = (my > d + depth_bias);
 *       occluded = behind && alpha > .95f;  inside = inside_frustum && !occluded.
 *     Every comparison is false for a NaN: a NaN position, a NaN texel and a NaN alpha all leave the leaf inside.  With guard_band ==
 *     1.05f and depth_bias == 0.00002f the leaves that are not inside are exactly the records m2s_prepass culls with the same matrices,
 *     format 0, depth_test_mesh 1 and the same image: the two share one definition of the test.
 *  2. Pins 2 to 6 of the frustum cuts apply word for word with this `inside`: positions above the leaves are never tested, masking is
 *     L := H, N_eff is the larger of max_records and the visible part of the last level, zero selected is a valid result, `refine` is
 *     unmasked, m2s_last_lod_level_counts reports the counts after masking; order, adoption, invalidation, m2s_device_lod_nodes,
 *     M2S_LOD_DRY_RUN and the SH plane (pin 3s) are m2s_lod_select's.
 *  3. Counts.  m2s_last_lod_occlusion_counts (a dry run included): [0] leaves inside the frustum, [1] of those, occluded, [2] of those
 *     inside the frustum, behind the image but kept because alpha <= .95 or is NaN, [3] nodes the plain cut selects at that tau_px and
 *     this one dropped.  After an occluded call m2s_last_lod_frustum_counts reports [0] and [3] of these and m2s_last_lod_frustum_ms the
 *     visibility stage.  Integer sums: identical from run to run.
 *  4. Errors: those of the frustum forms; M2S_ERR_INVALID for a NULL occluder, a depth_bias that is not finite or negative, a reserved
 *     word that is not 0, a depth_w or depth_h of 0 with a depth that is not NULL, a size that disagrees with the context's image where
 *     depth is NULL; M2S_ERR_STATE where depth is NULL and no m2s_mesh_depth has run.  An empty tree behaves as in the frustum forms and
 *     reads no image.
 *  5. The m2s_prepass that follows an occluded cut is run with depth_test_mesh = 0: a selected node above the leaves is the mean of
 *     points on a curved surface, lies under the surface its leaves lie on and would be culled by its own position where its leaves
 *     pass.  A node is drawn whole as soon as one leaf below it is visible: the rule is conservative, it never removes visible surface. */
typedef struct m2s_lod_occluder {
    const float* depth;        /* depth_w x depth_h window-space depth in [0,1], row 0 = bottom: m2s_prepass_params.depth's layout.
                                  NULL: the image of the context's last m2s_mesh_depth (depth_w / depth_h must then be 0 or equal to its size) */
    uint32_t depth_w, depth_h;
    uint32_t depth_on_device;  /* as m2s_prepass_params: 1 = device pointer on the context's device, 0 = host memory (copied) */
    float    depth_bias;       /* finite, >= 0; 0.00002f is the prepass's own */
    uint32_t reserved[2];      /* 0 */
} m2s_lod_occluder;            /* 32 bytes */
m2s_status m2s_lod_select_occluded(m2s_ctx* ctx, const m2s_lod_select_params* params, const m2s_lod_frustum* frustum,
                                   const m2s_lod_occluder* occluder, uint64_t out_counts[4]);
m2s_status m2s_lod_select_budget_occluded(m2s_ctx* ctx, const m2s_lod_budget_params* params, const m2s_lod_frustum* frustum,
                                          const m2s_lod_occluder* occluder, m2s_lod_budget_result* out, uint64_t out_counts[4]);
m2s_status m2s_last_lod_occlusion_counts(const m2s_ctx* ctx, uint64_t out[4]);

/* The blend: after any of the six cuts, every record of the cut is moved towards its node's parent as tau_px approaches the value at
 * which the parent takes over, so that the records just before a switch are, up to rounding, the parent just after it — the cut no
 * longer pops between levels (tests/lod_blend_ref.py restates it).  Which nodes are drawn does not change: counts, order,
 * node indices and the tree stay as the cut left them.  All arithmetic is fp32, one rounding per operation, no contraction; every `/`
 * is the IEEE division; no root.  Pinned:
 *  1. Precondition.  The context's current records are what the last cut that was no dry run left (m2s_device_lod_nodes is valid for
 *     them) and the tree that cut went through exists; M2S_ERR_STATE otherwise.  Record j is node i = ids[j]; p = parent[i].
 *  2. Weight.  For a node n with bound (x, y, z, e): d2 and s exactly as in pin 1 of the cut, q(n) = (s * s) / d2.
 *       t = 0 where p == M2S_LOD_NO_PARENT; otherwise
 *       den = q(p) - q(i);  num = tau_px * tau_px - q(i);  t_raw = num / den;
 *       t = fminf(fmaxf((t_raw - (1.0f - band)) / band, 0.0f), 1.0f);   t = 0 where !(den > 0).
 *     A NaN anywhere gives 0 (fmaxf returns its other operand), a parent that projects no larger than its child gives 0, invalid
 *     records — byte-identical singletons on every level, den == 0 — give 0.  t is linear in tau_px squared: the comparison's own
 *     operands, no root.  For a fixed node and camera t does not decrease as the bits of tau_px increase.
 *  3. Copy.  t == 0: the 96 bytes of tree node i, bit for bit.  The source of every record is the TREE (planes 0, 1 and the bounds),
 *     never the context's records: the pass is idempotent and may be called again with another band.
 *  4. Lerp.  u = 1.0f - t;  lerp(a, b) = u * a + t * b (two products, one sum; exactly b at t == 1 for finite a).  Lerped between node i
 *     and node p: position[0..2], color[0..3], scale[2], normal[0..2], pbr[0..1].  The child's own bits are kept in position[3],
 *     scale[3], normal[3], pbr[2..3].  The normal is not renormalised (the relighting and bake shaders normalise it).
 *  5. Frame.  A flat record's covariance does not change when its frame turns by 90 degrees about r_3 with the two edges swapped, or by
 *     180 degrees about r_1, and m2s_merge picks a parent's e1 by eigen-decomposition: child and parent frames may differ by such a
 *     turn.  With the stored quaternion (w, x, y, z) = rotation[0..3] of the PARENT, eight candidates raw_k, each component one fp32 sum
 *     or a copy (right-multiplication turns the body axes):
 *       k = 0  none          ( w,       x,      y,      z     )
 *       k = 1  Rz 90         ( w - z,   x + y,  y - x,  z + w )   scaled by kC, edges swapped
 *       k = 2  Rz 180        (-z,       y,     -x,      w     )
 *       k = 3  Rz 270        ( w + z,   x - y,  y + x,  z - w )   scaled by kC, edges swapped
 *       k = 4  Rx 180        (-x,       w,      z,     -y     )
 *       k = 5  diagonal      (-(x + y), w - z,  w + z,  x - y )   scaled by kC, edges swapped
 *       k = 6  Ry 180        (-y,      -z,      w,      x     )
 *       k = 7  antidiagonal  ( y - x,   w + z,  z - w, -(x + y))  scaled by kC, edges swapped
 *     kC = 0.70710678118654752f.  With the child's quaternion c: d_k = (c0 r0 + c1 r1) + (c2 r2 + c3 r3) over raw_k; the score is
 *     d_k * d_k, times 0.5f for odd k; the candidate is the first k with the strictly greatest score (a NaN score never wins over
 *     k = 0).  Candidates 1 .. 7 are considered only where the parent is unit, fabsf(((w w + x x) + (y y + z z)) - 1.0f) <= 0x1p-10f
 *     (the viewer does not normalise a quaternion: the turns of a non-unit frame do not preserve its covariance); other parents take
 *     k = 0.  cand = raw_k, times kC per component for odd k, negated as a whole where d_k < 0; the target edges are the parent's
 *     (scale[0], scale[1]), swapped for odd k.  rotation = lerp(c, cand) per component, not normalised; scale[0..1] = lerp(own, target).
 *  6. SH rows.  Where the tree has an SH plane and the context's plane holds for these records: row j = lerp of tree rows i and p in
 *     all 48 columns, copied at t == 0; the plane stays valid with its degree.  A tree without a plane touches none.
 *  7. Effect on the context: m2s_lod_select's own — the records epoch advances, what a cut invalidates is invalid —, after which
 *     m2s_device_lod_nodes is valid again and m2s_device_lod_blend_t holds the weights.  Zero records: a valid no-op.
 *  8. out_counts (may be NULL): [0] records, [1] records with t > 0, [2] records with t == 1, [3] records with t > 0 and k != 0.
 *     Integer sums, identical from run to run.
 * Known limit: alpha is lerped like the colour, and near t = 1 the m children of a parent are m coincident copies of it; front-to-back
 * blending of m copies is 1 - (1 - a g)^m against a g, so a change in edge softness remains at the switch.
 * Synchronous.  M2S_ERR_INVALID: as m2s_lod_select, a band that is not finite or outside (0, 1], reserved != 0.  M2S_ERR_STATE: no tree,
 * conversions in flight, records that are not the last cut's, a tree built under M2S_MERGE_MODEL_GAUSSIAN (m2s_set_merge_model, pin
 * 4g: the eight turns and the axis-by-axis lerp assume the footprint's axis order; the model is the tree's, whatever the switch says now). */
typedef struct m2s_lod_blend_params {
    float    camera_position[3];  /* as m2s_lod_select_params: the values the cut was taken with */
    float    focal_px;            /* finite, > 0 */
    float    tau_px;              /* finite, >= 0: the cut's tau (for a budget cut: the returned tau_px) */
    float    near;                /* finite, > 0 */
    float    band;                /* finite, 0 < band <= 1: the upper share of a node's tau^2 interval over which it moves to its parent */
    uint32_t reserved;            /* 0 */
} m2s_lod_blend_params;           /* 32 bytes */
m2s_status m2s_lod_blend(m2s_ctx* ctx, const m2s_lod_blend_params* params, uint64_t out_counts[4]);
/* The weight t of every record of the last m2s_lod_blend, a float each, in their order.  Valid until the records change again (NULL /
 * M2S_ERR_STATE then; NULL for zero records too).  m2s_download_lod_blend_t: as m2s_download_lod_nodes. */
const void* m2s_device_lod_blend_t(const m2s_ctx* ctx);
m2s_status  m2s_download_lod_blend_t(m2s_ctx* ctx, float* dst, uint64_t capacity, uint64_t* out_n);
/* The counts of the last m2s_lod_blend; its duration on the device (ms, measured whatever m2s_set_profiling says) and its stages:
 * [0] weights, [1] records, [2] SH rows (0 without a plane). */
m2s_status m2s_last_lod_blend_counts(const m2s_ctx* ctx, uint64_t out[4]);
float       m2s_last_lod_blend_ms(const m2s_ctx* ctx);
m2s_status  m2s_last_lod_blend_stage_ms(const m2s_ctx* ctx, float out_ms[3]);

/* ---- world units (no counterpart in the reference, which keeps the resolutionTarget beside its records) ---------------------------- */
/* Brings the context's current records to world units: scale[k] = scale[k] / (float)R for k = 0, 1, 2, with R the records'
 * resolutionTarget; afterwards the records' resolutionTarget is 1.  A conversion stores scale = (|Ju|, |Jv|, 1e-7) and leaves the
 * division by R to the viewer (std / R times the stored scale); m2s_merge, m2s_lod_build and m2s_lod_select read scale[0..1] as world
 * lengths, which holds for uploaded records and for these, not for a conversion's as stored: run this pass between the conversion and
 * them, and tau_px of the cut counts screen pixels.  The pin (tests/worldunits_ref.py restates it):
 *  1. Arithmetic.  Each of scale[0], scale[1], scale[2] is replaced by the correctly rounded (IEEE, round to nearest even) fp32 quotient
 *     by (float)R; every other word of the 96-byte record keeps its bits, scale[3] included.  This holds for invalid records, NaN
 *     (a NaN stays a NaN; its payload is the division's), infinities, zeros and negative scales (the sign is kept) and for quotients
 *     that are subnormal (not flushed).
 *  2. No-op cases.  With R = 0 (uploaded records, taken as R = 1) or R = 1 the call succeeds and nothing of the context changes: the
 *     records stay where they are and the records epoch does not advance.
 *  3. Effect on the context, otherwise as m2s_refit_apply: the records live in the context-owned pool afterwards (records adopted
 *     through m2s_set_records are divided on their way there; the caller's memory is not written), the records epoch advances, and
 *     cached positions, sorted quads, sources, the contribution and refit accumulators, the maps of m2s_merge and m2s_lod_select and a
 *     baked SH plane are invalidated.  m2s_last_resolution reports 1.  A level-of-detail tree built earlier is a copy: it is not
 *     touched and keeps its leaves' resolutionTarget, which m2s_lod_select hands back to the records it selects.
 *     m2s_download_triangle_counts and the preparation of the next m2s_upload_scene still see the R of the conversion.
 *  4. *out_previous_R (may be NULL): the resolutionTarget the records had, also in the no-op cases (0 or 1) — 0 where the call fails.
 *  5. For the viewer.  For a power-of-two R the division and the viewer's std / R are both exact scalings (short of underflow), so
 *     every consumer that takes its resolution_target from m2s_last_resolution produces the same bytes before and after: the quads of
 *     m2s_prepass and the rows of m2s_export_ply in formats 0, 1 and 2.  For another R the results differ by the one rounding: here
 *     the stored scale is rounded after the division and std is used as it is, there std / R is rounded and the product after it.
 * Synchronous.  M2S_ERR_INVALID for a NULL context; M2S_ERR_STATE without records or with conversions in flight; M2S_ERR_CAPACITY for
 * more than 2^32 - 1 records. */
m2s_status m2s_records_to_world_units(m2s_ctx* ctx, uint32_t* out_previous_R);
/* Duration (ms) of the last m2s_records_to_world_units that was not a no-op; 0 where it ran with profiling off. */
float m2s_last_world_units_ms(const m2s_ctx* ctx);

/* ---- shadow pass == GaussianShadowPass::execute (GaussianShadowPass.cpp:83-236) ---------------------------- */
/* The point light of the frame (RenderContext::pointLightData) and what the two lighting passes read from RenderContext. */
typedef struct m2s_light_params {
    float light_position[3];     /* pointLightModel[3].xyz -> u_lightPos / u_LightPosition                                       */
    float light_color[3];        /* pointLightData.lightColor -> u_lightColor                                                   */
    float light_intensity;       /* pointLightData.lightIntensity -> u_lightIntensity                                           */
    float camera_position[3];    /* camera position -> u_camPos                                                                 */
    float near_far[2];           /* nearPlane, farPlane: the cube's glm::perspective and u_farPlane of both passes               */
    int32_t render_mode;         /* renderMode 0..6 (m2s_relight: 5 = metallic-roughness view, 6 = lit, any other = albedo)      */
    int32_t resolution[2];       /* rendererResolution: the W x H of the G-buffer m2s_relight lights (m2s_shadow does not read it:
                                    its u_resolution is m2s_prepass_params.resolution, the same RenderContext member)            */
    uint32_t shadow_resolution;  /* S, the side of a cube face: 1..4096; 0 = 1024, the reference's SHADOW_CUBEMAP_SIZE           */
    uint32_t want_shadow_counts; /* m2s_relight, mode 6: also keep the per-pixel count of shadowed PCF taps (0..20)              */
    uint32_t reserved;           /* 0 */
} m2s_light_params;

/* == QuadNdcTransformation of gaussianPointShadowMappingCS.glsl:26-30, 48 bytes */
typedef struct m2s_shadow_quad {
    float mean2d_ndc[4];     /* clip position through the face's camera, xyz divided by w; w kept */
    float quad_scale_ndc[4]; /* major axis xy, minor axis xy, in NDC units of the RENDERER's window (see below) */
    float ws_pos[4];         /* u_modelToWorld * (P, 1) */
} m2s_shadow_quad;

/* Stage A == gaussianPointShadowMappingCS.glsl:58-207 over `n` records at `d_records` (or the context's records when d_records is
 * NULL, n ignored — as m2s_prepass): world position; cube face by the dominant axis of normalize(ws - light) with the shader's `if`
 * chain (|x| >= |y| and |x| >= |z|: x > 0 ? 0 : 1; else |y| >= |x| and |y| >= |z|: y > 0 ? 2 : 3; else z > 0 ? 4 : 5 — every test is
 * false for NaN, so a NaN direction lands on face 5); that face's camera; the 1.05 w cull; 3D covariance -> 2D covariance (+0.3) ->
 * eigenvalues; cull on lambda2 < 0; the two axes capped at 1024; appended to the face's list.  fp32 in the shader's operation
 * order, one rounding per operation — the covariance code is the viewer prepass's own (shared device functions).  Per-record inputs
 * come from `prepass` (model_to_world, gaussian_std, resolution_target, format, resolution, near_far -> u_nearFar); its two camera
 * matrices, render mode, depth test and ordering fields are not read.
 *  - Cameras: glm::lookAt(light, light + axis, up) for (+X, up -Y), (-X, -Y), (+Y, +Z), (-Y, -Z), (+Z, -Y), (-Z, -Y)
 *    (GaussianShadowPass.cpp:91-108) and glm::perspective(90 degrees, 1, near, far), built in double and rounded to float, with
 *    `light + axis - light` taken as the axis itself and 1 / tan(45 degrees) as 1: the rotation part is an exact signed permutation
 *    (no negative zeros), the translation the permuted, negated light position.
 *  - normalize in determineFaceIndex is v / sqrt((x x + y y) + z z) with correctly rounded root and division: a record exactly at the
 *    light gives 0 / 0 = NaN, goes to face 5, and is then culled or kept by the tests that follow, as written.
 * Oddities of the shader carried over as written, because they change pixels:
 *  - u_resolution is the RENDERER's resolution (GaussianShadowPass.cpp:123) — it scales the Jacobian and converts the axes to NDC —
 *    while the faces are S x S: quads on the cube are sized for the window, not for the face.
 *  - modelScale = (|M[0]|, |M[0]|, |M[1]|) (:97).
 *  - the colour / normal / depth-colour code of :114-151 writes nothing that leaves the shader: not computed.
 *  - the reference appends through one atomic per record into fixed regions of 7 000 000 quads per face and overruns silently beyond
 *    that.  Here the six lists are exact-size (grow-only buffer) and each is in INPUT order, like m2s_prepass.
 * Stage B == drawToCubeMapFaces + gaussianPointLightCubeMapShadow{VS,PS}.glsl: every quad of a face's list drawn as two triangles,
 * depth test GL_LESS against a cube cleared to 1.0, blending off, gl_FragDepth = length(ws - light) / farPlane (constant over the
 * quad).  A texel therefore ends as min(1.0, min over the covering quads of d): order-independent and idempotent.  The pin:
 *  - Geometry exactly as m2s_splat: vertices mean.xy + (vx * scale.xy + vy * scale.zw), (vx, vy) in {(-1,-1), (-1,1), (1,1), (1,-1)},
 *    triangles (0,1,2) and (0,2,3), the same rounding order, viewport S x S, the project's pinned rasteriser (24.8 snap RNE, int64
 *    edge functions, both windings, top-left rule, texel centres (x + 0.5, y + 0.5)).  A quad with a non-finite value in mean.xy,
 *    scale or ws_pos, or with a vertex beyond the +-16384 px guard band, is SKIPPED and counted (*out_skipped).
 *  - d: (dx, dy, dz) = ws - light; sqrt((dx dx + dy dy) + dz dz) / farPlane, every operation rounded to fp32, root and division
 *    correctly rounded; clamped to [0, 1] (a NaN d never passes the depth test).
 *  - Storage: fp32 (the reference asks for an unsized GL_DEPTH_COMPONENT and leaves the bit depth to the driver; fp32 is what it
 *    uploads and what texture().r returns unchanged): float[6][S][S], faces in GL order +X, -X, +Y, -Y, +Z, -Z, row 0 = window
 *    row 0 of that face's framebuffer = t = 0 of the face image.
 * Synchronous.  out_per_face (may be NULL): the six list lengths.  Errors: M2S_ERR_INVALID for a shadow resolution outside 1..4096,
 * a renderer resolution outside 1..8192, a render mode outside 0..6, reserved != 0, resolution_target == 0; M2S_ERR_STATE without
 * records; M2S_ERR_CAPACITY beyond 2^31-1 (tile, quad) pairs.  n = 0 with a non-NULL d_records: six empty lists, a cube of 1.0. */
m2s_status m2s_shadow(m2s_ctx* ctx, const m2s_prepass_params* prepass, const m2s_light_params* light, const void* d_records, uint64_t n,
                      uint64_t out_per_face[6], uint64_t* out_skipped);
/* Stage B alone on quad lists made elsewhere (the counterpart of m2s_upload_quads + m2s_splat): `host_quads` holds the six lists back to
 * back, per_face[f] quads for face f, in face order.  They become the context's lists (m2s_download_shadow_quads) and are drawn into a
 * cleared cube exactly as m2s_shadow draws its own; `light` gives the light position, farPlane (near_far[1]) and S.  Same errors as
 * m2s_shadow where they apply; host_quads may be NULL only when every per_face[f] is 0 (a cube of 1.0). */
m2s_status m2s_shadow_from_quads(m2s_ctx* ctx, const m2s_light_params* light, const m2s_shadow_quad* host_quads, const uint64_t per_face[6],
                                 uint64_t* out_skipped);
/* The cube of the last m2s_shadow / m2s_shadow_from_quads / m2s_upload_shadow_cubemap: float[6][S][S] on the device.  NULL before any. */
const void* m2s_device_shadow_cubemap(const m2s_ctx* ctx);
m2s_status m2s_download_shadow_cubemap(m2s_ctx* ctx, float* dst, uint64_t capacity_floats);
/* The list of face 0..5 of the last m2s_shadow, in input order. */
m2s_status m2s_download_shadow_quads(m2s_ctx* ctx, uint32_t face, m2s_shadow_quad* dst, uint64_t capacity_quads);
/* A cube made elsewhere (host float[6][S][S], S in 1..4096) becomes the context's cube: what m2s_relight samples. */
m2s_status m2s_upload_shadow_cubemap(m2s_ctx* ctx, const float* host, uint32_t S);
/* Duration (ms) of the last profiled m2s_shadow (sum of its stages), and the stages: [0] stage A (count, scan, emit), [1] stage B
 * setup + binning (tile counts, pairs, radix sort), [2] stage B raster. */
float m2s_last_shadow_ms(const m2s_ctx* ctx);
m2s_status m2s_last_shadow_stage_ms(const m2s_ctx* ctx, float out_ms[3]);
/* What the last m2s_shadow did: [0..5] quads per face, [6] (tile, quad) pairs, [7] texel updates sent, [8] quads skipped. */
m2s_status m2s_last_shadow_counts(const m2s_ctx* ctx, uint64_t out[9]);

/* ---- relighting pass == GaussianRelightingPass::execute without split screen (GaussianRelightingPass.cpp:136-143) -------------- */
/* One full-screen draw of gaussianSplattingDeferredPS.glsl over the G-buffer of the last m2s_splat / m2s_upload_gbuffer and the cube
 * of the last m2s_shadow / m2s_upload_shadow_cubemap into a W x H RGBA8 frame (uchar4 per pixel, row 0 = bottom, like the G-buffer).
 *  - The G-buffer textures are GL_LINEAR but sampled at texel centres at 1:1: a texel fetch of pixel (x, y).
 *  - Mode 5: (mr.r, mr.g, 0, 255); every mode other than 5 and 6: (albedo.rgb, 255).  Byte copies: exact.
 *  - Mode 6: the shader as written, including what looks like mistakes: PI is the MACRO 22.0f/7.0f, so `PI * denom * denom` is
 *    ((22/7) denom) denom and `kD * albedo / PI` is ((kD albedo) / 22) / 7; metallic = pbr.b (which m2s_splat always leaves 0); ao,
 *    gDepth, u_isLightingEnalbed, u_worldToView and u_resolution are unused (the depth plane is not read); position and normal are
 *    taken without dividing by the accumulated alpha; background pixels are lit like any other.
 *  - computeShadowFactor is decision arithmetic, fp32 operation by operation without contraction: lightDir = pos - light;
 *    currentDepth = sqrt((x x + y y) + z z); sampleDir = lightDir / currentDepth (component-wise, correctly rounded); for each of the
 *    20 offsets o (in the shader's order) v = sampleDir + o * 0.025f; the cube texel of v by the GL rule (OpenGL 4.6 core, table 8.19:
 *    major axis x if |x| >= |y| and |x| >= |z|, else y if |y| >= |z|, else z; negative face when the major coordinate is < 0;
 *    (sc, tc) = +X (-z, -y), -X (z, -y), +Y (x, z), -Y (x, -z), +Z (x, -y), -Z (-x, -y); s = 0.5 (sc / |ma| + 1), same for t;
 *    GL_NEAREST, clamp to edge: texel min(max(floor(s S), 0), S - 1); a NaN s or t reads texel (0, 0) of face 5);
 *    closest = texel * farPlane; the tap counts when currentDepth - 0.05f > closest.  shadow = count / 20.
 *  - The rest of mode 6 (three pow, the normalisations, GGX, the tone map) is value arithmetic: fp32 without contraction, with the
 *    device's fast exp2 / log2 / reciprocal square root / square root (as exp is in m2s_splat); max(x, 0.0) keeps a NaN.
 *  - Output: rint(clamp(c, 0, 1) * 255), NaN -> 0, alpha 255.
 * Synchronous.  Errors: M2S_ERR_INVALID for a render mode outside 0..6, reserved != 0, a shadow resolution outside 1..4096 or (when
 * not 0) different from the cube's, `resolution` different from the G-buffer's, or when no G-buffer or no cube exists yet. */
m2s_status m2s_relight(m2s_ctx* ctx, const m2s_light_params* light);
/* Five host planes (layouts of m2s_device_gbuffer; a NULL plane is zero-filled; attachment 3 is never read by m2s_relight) become
 * the context's G-buffer, as if m2s_splat had left them: the counterpart of m2s_upload_quads.  W, H in 1..8192. */
m2s_status m2s_upload_gbuffer(m2s_ctx* ctx, const void* const planes[5], int32_t W, int32_t H);
/* The frame of the last m2s_relight: uchar4[W * H], row 0 = bottom.  NULL before any. */
const void* m2s_device_frame(const m2s_ctx* ctx);
m2s_status m2s_download_frame(m2s_ctx* ctx, void* dst, uint64_t capacity_bytes);
/* uint8[W * H]: the 20-tap counts of the last m2s_relight (mode 6 with want_shadow_counts); M2S_ERR_STATE otherwise. */
m2s_status m2s_download_shadow_counts(m2s_ctx* ctx, uint8_t* dst, uint64_t capacity_bytes);
/* Duration (ms) of the last profiled m2s_relight. */
float m2s_last_relight_ms(const m2s_ctx* ctx);

/* ---- mesh depth prepass == DepthPrepass::execute (DepthPrepass.cpp:8-50, depthPrepass{VS,PS}.glsl) ------------------------------- */
/* Draws the opaque meshes of the UPLOADED SCENE (not records) with the camera of the frame, depth only, depth test GL_LESS, into a
 * W x H image cleared to 1.0: the reference's meshDepthTexture (renderer.cpp:281-309), which the viewer prepass tests its Gaussians
 * against (m2s_prepass_params.depth_test_mesh).  Under m2s_set_triangle_range it draws the uploaded range only (the image of a whole
 * scene is the texel-wise min of its shards' images).  GL semantics restated for a compute pass; these choices are the pin
 * (tests/meshdepth_ref.py restates them operation for operation).  All of it is decision arithmetic: fp32, no contraction, divisions
 * correctly rounded.
 *  - Which meshes: base_color[3] == 1.0f exactly (DepthPrepass.cpp:33).  Both windings: the pass does not enable culling.
 *  - Vertex: gl_Position = ((P V) M) (p, 1).  The two mat4 x mat4 products are taken once per call in glm's order — element (i, j) =
 *    ((A[0][i] B[j][0] + A[1][i] B[j][1]) + A[2][i] B[j][2]) + A[3][i] B[j][3] — then one mat4 x vec4 per vertex as
 *    (m0 x + m1 y) + (m2 z + m3 w).  (Last-bit differences from the prepass's step-by-step transform, as in the reference.)  A vertex
 *    shared by several triangles gets the same clip coordinates in each: watertight.
 *  - A triangle with a non-finite clip coordinate is SKIPPED and counted ([2]).
 *  - Clipping: five planes in the fixed order near (d = z + w), +x (d = 2w - x), -x (2w + x), +y (2w - y), -y (2w + y); a vertex
 *    is inside a plane when d >= 0.  A triangle whose three vertices are outside ONE plane is rejected.  One whose vertices are
 *    inside all five is not clipped at all.  Any other goes through Sutherland-Hodgman, plane by plane over the polygon's edges
 *    (cur, next): emit cur when inside; where the edge crosses, emit in + t (out - in) for the four clip coordinates with
 *    t = d_in / (d_in - d_out), always from the INSIDE vertex (both triangles at a shared edge get the same point).  The polygon
 *    (at most 8 vertices) is fanned from its first vertex.  The factor 2 keeps every vertex that reaches the snap inside the
 *    +-16384 px guard band for W, H <= 8192; the edges it introduces lie outside the window.  No far clip: see z_w.
 *  - Per piece (the triangle, or one triangle of the fan): x_n = x / w, y_n = y / w, z_w = (z / w) * 0.5 + 0.5 per vertex.  A piece
 *    none of whose z_w is < 1.0 is rejected (it cannot pass GL_LESS against the clear value).  Viewport xw = (W/2) x_n + W/2,
 *    yw = (H/2) y_n + H/2, then the project's pinned rasteriser as m2s_splat uses it: snap to 1/256 px (RNE), +-16384 px guard band
 *    (beyond it, or NaN: rejected), int64 edge functions, both windings, top-left rule, pixel centres (x + 0.5, y + 0.5); zero
 *    area: rejected.
 *    The three vertices of a piece are then put in ascending (Y, X) order of their snapped coordinates, so that neither the winding
 *    nor the order in which a triangle's vertices are stored changes a bit of the image.
 *  - Depth of a fragment: with E_i the int64 edge function opposite vertex i at the pixel centre (interior positive) and
 *    inv = 1.0f / (float)|area2|:  b_i = (float)E_i * inv;  z = (b_0 z_w0 + b_1 z_w1) + b_2 z_w2;  clamped to [0, 1]; a NaN never
 *    passes.  (z_w is affine in window space; these are the conversion's barycentrics.)
 *  - Storage: fp32 (the reference asks for an unsized GL_DEPTH_COMPONENT; the prepass's eps of 2e-5 is far above either choice):
 *    float[H][W], row 0 = the BOTTOM row — exactly the layout m2s_prepass_params.depth expects, so m2s_device_mesh_depth() can be
 *    passed straight back with depth_on_device = 1, depth_w = W, depth_h = H.  A texel ends as min(1.0, min over covering fragments):
 *    order-independent and idempotent.
 * Counts (out_counts may be NULL): [0] triangles drawn (opaque, finite, at least one piece not rejected), [1] triangles that went
 * through the clipper, [2] triangles skipped for a non-finite vertex, [3] (tile, piece) pairs of the binned path, [4] texel updates
 * sent ([3] and [4] depend on how the work was split, not on the scene alone: [4] also on timing).
 * Synchronous.  Errors: M2S_ERR_INVALID for a resolution outside 1..8192 or reserved != 0; M2S_ERR_STATE without a scene;
 * M2S_ERR_CAPACITY beyond 2^31-1 pairs.  A scene with no opaque mesh gives an image of 1.0. */
typedef struct m2s_mesh_depth_params {
    float world_to_view[16], view_to_clip[16], model_to_world[16];  /* column-major, as m2s_prepass_params */
    int32_t resolution[2];      /* rendererResolution, 1..8192 each */
    uint32_t reserved[2];       /* 0 */
} m2s_mesh_depth_params;
m2s_status m2s_mesh_depth(m2s_ctx* ctx, const m2s_mesh_depth_params* params, uint64_t out_counts[5]);
/* The image of the last m2s_mesh_depth: float[H][W] on the device, row 0 = bottom (context-owned, grow-only).  NULL before any. */
const void* m2s_device_mesh_depth(const m2s_ctx* ctx);
m2s_status m2s_download_mesh_depth(m2s_ctx* ctx, float* dst, uint64_t capacity_floats);
/* Duration (ms) of the last profiled m2s_mesh_depth (sum of its stages), and the stages: [0] clear + setup + triangles covered in
 * place, [1] clipper + binning (records, tile counts, pairs, radix sort), [2] tile raster. */
float m2s_last_mesh_depth_ms(const m2s_ctx* ctx);
m2s_status m2s_last_mesh_depth_stage_ms(const m2s_ctx* ctx, float out_ms[3]);
m2s_status m2s_last_mesh_depth_counts(const m2s_ctx* ctx, uint64_t out[5]);
/* Test hook: an unclipped triangle whose pixel box is at most max_box pixels wide and high is covered by its own lane instead of
 * being binned (default 4; -1 restores it).  0 sends every triangle through the binned path, 8192 every unclipped one through the
 * in-place path.  The image does not depend on it. */
m2s_status m2s_debug_set_mesh_depth_inplace(m2s_ctx* ctx, int32_t max_box);

/* ---- mesh render pass == MeshRenderPass::execute (MeshRenderPass.cpp:8-73, meshRender{VS,PS}.glsl) ----------------------------- */
/* Draws EVERY mesh of the uploaded scene (no alpha filter) with the camera of the frame into a second five-target G-buffer (the
 * targets of renderer.cpp:473-539, layouts and orientation of m2s_device_gbuffer): what m2s_relight_split shows left of the divider.
 * GL semantics restated for a compute pass in two stages; these choices are the pin (tests/meshrender_ref.py restates them).
 * Stage 1, visibility — decision arithmetic, exact:
 *  - Vertex transform, finite test, five-plane clipper, fan, division, z_w, snap, guard band and the depth of a fragment are exactly
 *    those of m2s_mesh_depth.  In particular gl_Position = ((P V) M) (p, 1): the reference's mesh vertex shader multiplies step by
 *    step (P (V (M p))) and differs from that in last bits; sharing the depth pass's transform keeps the two passes' depths identical.
 *  - GL_CULL_FACE is on (front = CCW, cull back): a piece is drawn only if the int64 doubled area of its snapped vertices, taken in
 *    the STORED vertex order — (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0), before the canonical (Y, X) reorder, window with y up — is
 *    > 0.  Zero area is rejected as before.  The test comes after the z_w, guard-band and empty-box rejections.
 *  - GL_LESS in draw order: per pixel the winner is the minimum of the 64-bit key (bits of z) << 32 | global triangle index, z in
 *    [0, 1] after the clamp; fragments with z >= 1.0 or NaN never compete; an empty pixel holds (bits of 1.0f) << 32 | 0xFFFFFFFF.
 *    The lowest index wins a depth tie: the triangle GL drew first.  The index is global under m2s_set_triangle_range, so the
 *    visibility images of shards combine by 64-bit min.
 * Stage 2, shading, per pixel — an empty pixel gets zeros in all five planes (the pass's clear).  Otherwise, for the winner:
 *  - Barycentrics of the ORIGINAL triangle (clipped or not) in homogeneous form, in fp64 from the fp32 clip coordinates
 *    c_i = (x_i, y_i, w_i): with (j, k) = (i + 1, i + 2) mod 3, A_i = y_j w_k - w_j y_k, B_i = x_j w_k - w_j x_k, C_i = x_j y_k - y_j x_k,
 *    n = ((2 x + 1) / W - 1, (2 y + 1) / H - 1) at the centre of pixel (x, y): e_i = (n.x A_i - n.y B_i) + C_i (= det[n; c_j; c_k]);
 *    lambda_i = e_i / ((e_0 + e_1) + e_2), rounded to fp32.  Coverage was decided on SNAPPED vertices, so a covered centre may get a
 *    slightly negative lambda: accepted (an extrapolation by less than 1/256 px).
 *  - Varyings as the vertex shader makes them, per corner, fp32: v_worldPos = (M (p, 1)).xyz; v_normal = normalize(N n);
 *    v_tangent = (normalize(N t.xyz), t.w); v_uv; v_viewDepth = -(V (M (p, 1))).z, step by step; N = mat3(transpose(inverse(M))) taken
 *    once on the host in float64 from the fp32 matrix and rounded to fp32.  Interpolation: (lambda_0 a_0 + lambda_1 a_1) + lambda_2 a_2.
 *  - Texture LOD: the implicit derivatives a helper invocation would see: dUV/dx = uv(x + 1, y) - uv(x, y), dUV/dy = uv(x, y + 1) -
 *    uv(x, y), uv(.) being the winner's own interpolation (fp64 barycentrics, as above) at the neighbouring centre; then the
 *    conversion's sampler unchanged per map (0.5 log2(max(|dx|^2, |dy|^2)) in texels, levels 0..4, REPEAT, trilinear, fp32 weights).
 *    A non-finite gradient selects the last level.
 *  - The fragment shader as written: albedo = baseColorFactor (x texture); N = normalize(v_normal), with a normal map
 *    normalize(TBN normalize(2 s - 1)), T = normalize(v_tangent.xyz), B = normalize(cross(N, T)) * v_tangent.w; encodeNormal = 0.5 N +
 *    0.5; metallic-roughness (0.1, 0.5), or the map's (b, g); computeExponentialDepth(v_viewDepth, near_far) =
 *    clamp(exp(-20 clamp((d - near) / (far - near)))).  Render modes 0 / 6 / 5 (and any not named here) albedo, 1 depth, 2 encoded
 *    normal, 4 the constant (0.01, 0.005, 0), 3 the per-triangle hash (fract(sin(id 311.7) 43758.5453), fract(sin(id 269.5 + 1.3) ..),
 *    fract(sin(id 183.3 + 2.7) ..)) with id = gl_PrimitiveID = the triangle's index within its mesh; the argument is an fp32 product
 *    (and sum), its sine is taken in fp64 and rounded to fp32 (the factor 43758.5453 amplifies any error of it), the rest is fp32.
 *  - Outputs: 0 position (v_worldPos, 1), 1 normal (encoded, 1), 3 depth (d, d, d, 1): half4, RNE; 2 albedo (rgb of the mode's colour),
 *    4 metallic-roughness (metallic, roughness, 0): uchar4 = rint(clamp(c, 0, 1) * 255), NaN -> 0, alpha 255.
 *  - Arithmetic: the normalisations, exp and log2 are value arithmetic with the device's fast forms; everything else is fp32
 *    operation by operation without contraction.
 * Counts (out_counts may be NULL): [0]..[4] as m2s_mesh_depth (over every mesh), [5] triangles culled as back-facing (a piece reached
 * the area test with a negative area and no piece was drawn).
 * Synchronous.  Errors: M2S_ERR_INVALID for a resolution outside 1..8192, a render mode outside 0..6 or reserved != 0; M2S_ERR_STATE
 * without a scene; M2S_ERR_CAPACITY beyond 2^31-1 pairs.  An empty scene gives five planes of zeros. */
typedef struct m2s_mesh_render_params {
    float world_to_view[16], view_to_clip[16], model_to_world[16];  /* column-major, as m2s_prepass_params */
    int32_t resolution[2];      /* rendererResolution, 1..8192 each */
    float near_far[2];          /* u_nearFar */
    int32_t render_mode;        /* u_renderMode 0..6 */
    uint32_t reserved;          /* 0 */
} m2s_mesh_render_params;
m2s_status m2s_mesh_render(m2s_ctx* ctx, const m2s_mesh_render_params* params, uint64_t out_counts[6]);
/* Attachment 0..4 of the last m2s_mesh_render (layouts of m2s_device_gbuffer; context-owned, grow-only).  NULL before any. */
const void* m2s_device_mesh_gbuffer(const m2s_ctx* ctx, uint32_t attachment);
m2s_status m2s_download_mesh_gbuffer(m2s_ctx* ctx, uint32_t attachment, void* dst, uint64_t capacity_bytes);
/* The visibility image of the last m2s_mesh_render: uint64[H][W], row 0 = bottom (for tests and for merging shards). */
m2s_status m2s_download_mesh_visibility(m2s_ctx* ctx, uint64_t* dst, uint64_t capacity_pixels);
/* Duration (ms) of the last profiled m2s_mesh_render (sum of its stages), and the stages: [0] clear + visibility setup + triangles
 * covered in place, [1] clipper + binning, [2] tile raster, [3] shading.  [0] + [1] + [2] is the work of m2s_mesh_depth with an 8-byte
 * payload.  m2s_debug_set_mesh_depth_inplace moves this pass's in-place threshold too. */
float m2s_last_mesh_render_ms(const m2s_ctx* ctx);
m2s_status m2s_last_mesh_render_stage_ms(const m2s_ctx* ctx, float out_ms[4]);
m2s_status m2s_last_mesh_render_counts(const m2s_ctx* ctx, uint64_t out[6]);

/* == GaussianRelightingPass::execute with split screen (GaussianRelightingPass.cpp:90-135): m2s_relight, except that pixels with
 * x < splitPixelX = (int)(split_position * W) (an fp32 product, truncated) are lit from the mesh G-buffer of the last m2s_mesh_render
 * instead of the splat G-buffer — same shader, cube and light — and that the columns [dividerX, dividerX + 2) n [0, W),
 * dividerX = max(0, splitPixelX - 1), are (255, 255, 255, 255).  Errors as m2s_relight, and M2S_ERR_INVALID for a split_position
 * outside [0, 1], M2S_ERR_STATE without a mesh G-buffer of the G-buffer's W x H. */
m2s_status m2s_relight_split(m2s_ctx* ctx, const m2s_light_params* light, float split_position);

/* ---- fidelity score: the mesh frame against the splat frame (no counterpart in the reference, where a person looks at the split screen) */
/* m2s_relight over the MESH G-buffer of the last m2s_mesh_render, every pixel, no divider: the shader, cube and light m2s_relight_split
 * uses left of the divider, into a SECOND frame buffer (m2s_device_mesh_frame; uchar4[W * H], row 0 = bottom).  m2s_device_frame and the
 * shadow counts of the last m2s_relight stay untouched (want_shadow_counts is not read).  By definition its bytes are those of
 * m2s_upload_gbuffer(the mesh G-buffer's five planes) followed by m2s_relight.  Errors as m2s_relight (`resolution` is compared with the
 * mesh G-buffer's), and M2S_ERR_STATE without a mesh G-buffer.  m2s_last_relight_ms is this call's time when it was the last profiled. */
m2s_status m2s_relight_mesh(m2s_ctx* ctx, const m2s_light_params* light);
/* The frame of the last m2s_relight_mesh.  NULL / M2S_ERR_STATE before any. */
const void* m2s_device_mesh_frame(const m2s_ctx* ctx);
m2s_status m2s_download_mesh_frame(m2s_ctx* ctx, void* dst, uint64_t capacity_bytes);

/* Compares image B (under test: the splats) with image A (the reference: the mesh) in one pass over the device images.  All four images
 * are uchar4[W * H] device pointers, row 0 = bottom.  A NULL pointer means the context's own buffer — d_a: m2s_device_mesh_frame, d_b:
 * m2s_device_frame, d_cover_a: attachment 2 of the mesh G-buffer, d_cover_b: attachment 2 of the splat G-buffer — and M2S_ERR_STATE when
 * that buffer does not exist or is not W x H.  Every output is an integer; the pin (tests/score_ref.py restates it in numpy):
 *  - Coverage: a pixel is covered by A when the alpha byte (bits 24..31) of cover_a is non-zero (m2s_mesh_render leaves 255 or 0 there),
 *    by B when the alpha byte of cover_b is non-zero (the accumulated alpha m2s_splat leaves in the albedo attachment).  With
 *    M2S_SCORE_NO_COVER the planes are not read and every pixel counts as covered by both.  cover[] = pixels covered by neither, A only,
 *    B only, both — over the WHOLE image, whatever the mask.
 *  - Mask: mode 0 every pixel, 1 covered by A, 2 by A or B, 3 by A and B.  pixels = pixels that pass.
 *  - Colour, over the pixels that pass, per channel R, G, B (bytes 0, 1, 2) of the frames; frame alpha ignored: sse = sum of (a - b)^2,
 *    sad = sum of |a - b|, max_abs = max of |a - b|.  (PSNR is left to the caller: 10 log10(255^2 * 3 * pixels / (sse_r + sse_g + sse_b)).)
 *  - Luma: Y = (77 R + 150 G + 29 B + 128) >> 8, 0..255.
 *  - SSIM, the integer block form: windows of 8 x 8 pixels with origins (4 i, 4 j), 4 i + 8 <= W, 4 j + 8 <= H.  A window is COUNTED when
 *    at least 32 of its 64 pixels pass the mask; all 64 pixels enter its sums either way.  s1 = sum Ya, s2 = sum Yb, ssq = sum Ya^2 + sum
 *    Yb^2, s12 = sum Ya Yb (each < 2^32); c1 = 26634, c2 = 239708 (= (0.01 * 255)^2 * 64^2 and (0.03 * 255)^2 * 64^2, truncated); in int64
 *    num = (2 s1 s2 + c1) (128 s12 - 2 s1 s2 + c2), den = (s1^2 + s2^2 + c1) (64 ssq - s1^2 - s2^2 + c2) (|num|, den < 2^59, den > 0);
 *    ssim = (double)num / (double)den, the two conversions and the division correctly rounded (fp64, the one floating-point step);
 *    q = llrint(ssim * 2^32) (ties to even; the product is exact).  windows = windows counted, ssim_q32 = sum of their q in 64-bit
 *    integer arithmetic (below 2^55 at 8192 x 8192).  Identical windows give exactly 2^32.  W < 8 or H < 8: no window.
 *  - Every output is a sum, count or maximum of integers: it does not depend on the order of the reduction, two calls give the same
 *    bits, and so does the numpy restatement.  No floating-point atomics.
 *  - M2S_SCORE_WANT_MAP: the context also keeps the error map, uchar4[W * H]: (|dR|, |dG|, |dB|, 255) where the pixel passes the mask,
 *    zeros elsewhere (m2s_device_score_map / m2s_download_score_map: NULL / M2S_ERR_STATE when the LAST call kept none).
 * Synchronous.  Errors: M2S_ERR_INVALID for a resolution outside 1..8192, mask_mode > 3, an unknown flag, reserved != 0, a NULL
 * params / out; M2S_ERR_STATE as above. */
enum { M2S_SCORE_NO_COVER = 1, M2S_SCORE_WANT_MAP = 2 };
typedef struct m2s_score_params {      /* 24 bytes */
    int32_t  resolution[2];  /* W, H, 1..8192 each */
    uint32_t mask_mode;      /* 0 every pixel, 1 covered by A, 2 by A or B, 3 by A and B */
    uint32_t flags;          /* M2S_SCORE_* */
    uint32_t reserved[2];    /* 0 */
} m2s_score_params;
typedef struct m2s_score_result {      /* 120 bytes */
    uint64_t pixels;         /* pixels that pass the mask */
    uint64_t cover[4];       /* over the WHOLE image: neither, A only, B only, both */
    uint64_t sse[3], sad[3]; /* R, G, B over the pixels that pass: sum of (a - b)^2, sum of |a - b| */
    uint32_t max_abs[3], pad;
    uint64_t windows;        /* SSIM windows counted */
    int64_t  ssim_q32;       /* sum over the counted windows of llrint(ssim * 2^32) */
} m2s_score_result;
m2s_status m2s_score_frames(m2s_ctx* ctx, const m2s_score_params* params, const void* d_a, const void* d_b, const void* d_cover_a,
                            const void* d_cover_b, m2s_score_result* out);
const void* m2s_device_score_map(const m2s_ctx* ctx);
m2s_status m2s_download_score_map(m2s_ctx* ctx, void* dst, uint64_t capacity_bytes);
/* Duration (ms) of the last profiled m2s_score_frames kernel. */
float m2s_last_score_ms(const m2s_ctx* ctx);

/* ---- the point light baked into spherical harmonics: the lit result in a standard 3DGS .ply ------------------------------------- */
/* The format-0 .ply carries the flat albedo in f_dc and zeros in its 45 f_rest slots, so a standard 3DGS viewer shows an unlit object.
 * m2s_bake_light evaluates the deferred shader of m2s_relight (mode 6) per GAUSSIAN instead of per pixel, for a fixed set of view
 * directions, and projects the view-dependent colour onto the 16 real harmonics the format stores.  No counterpart in the reference.
 * The pin (tests/bake_ref.py restates it in numpy):
 *  - Directions: a product quadrature of n_theta Gauss-Legendre nodes in z = cos(theta) (descending) times n_phi azimuths
 *    phi_j = 2 pi (j + 0.5) / n_phi; row t * n_phi + j holds d = (sin(theta) cos(phi), sin(theta) sin(phi), z) and the weight
 *    w = w_GL 2 pi / n_phi (sum of w = 4 pi).  n_theta in {4, 8}, n_phi in {8, 16}, 0 = the default 8 x 16: every allowed pair
 *    integrates a product of two degree-3 harmonics exactly (degree 6 <= 2 n_theta - 1 in z, |m| <= 6 < n_phi in phi).  Nodes, weights
 *    and the products w B_i(d) are built on the host in double by a fixed sequence of + - * / and sqrt (Newton's iteration on P_n
 *    from literal starting values, a fixed number of steps; the azimuths' cosines are literals), then rounded to float once:
 *    m2s_bake_directions returns the rows (20 floats each: d.xyz, w, w B_0..15), mesh2splat_amd/bake.py builds the same bits.
 *  - Basis, the 3DGS convention colour(dir) = 0.5 + sum_i sh_i B_i(dir), dir = normalize(ws - camera): B_0 = C0; B_1..3 = -C1 y,
 *    C1 z, -C1 x; B_4..8 = C2[0] xy, C2[1] yz, C2[2] ((2zz - xx) - yy), C2[3] xz, C2[4] (xx - yy); B_9..15 = C3[0] y (3xx - yy),
 *    C3[1] (xy) z, C3[2] y ((4zz - xx) - yy), C3[3] z ((2zz - 3xx) - 3yy), C3[4] x ((4zz - xx) - yy), C3[5] z (xx - yy),
 *    C3[6] x (xx - 3yy); C0 = 0.28209479177387814, C1 = 0.4886025119029199, C2 = {1.0925484305920792, -1.0925484305920792,
 *    0.31539156525252005, -1.0925484305920792, 0.5462742152960396}, C3 = {-0.5900435899266435, 2.890611442640554,
 *    -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277, -0.5900435899266435}.
 *  - Coefficient: sh_i[c] = sum_k (w_k B_i(d_k)) (L_c(V = -d_k) - 0.5), fp32, one rounding per operation, in table order.  A colour
 *    that does not depend on V gives sh_0 = (c - 0.5) / C0 — what m2s_write_ply writes — and zeros (to rounding) above it.
 *  - Per record: ws = model_to_world * (P, 1); N = normalize(normalWs), normalWs = (transpose(inverse(model_to_world)) * vec4(normal.xyz,
 *    1)).xyz exactly as m2s_prepass computes it (gaussianSplattingPrepassCS.glsl:119, including the vec4's w of 1); albedo =
 *    min(max(color.rgb, 0), 1) (a NaN channel becomes 0); roughness = pbr[1]; metallic = pbr[0], or 0 with viewer_metallic (what the
 *    viewer's frame shows: its shader reads the G-buffer's always-zero B channel, see m2s_relight).
 *  - L(V): mode 6 of m2s_relight as written — the 22/7 macro, 0.3 albedo ambient, c / (c + 1) and the 1 / 2.2 power — with position
 *    ws, normal N and V from the table instead of normalize(cam - p); value arithmetic with the device's fast log2 / exp2 / reciprocal
 *    square root / square root.  Left as float: not clamped, not quantised.
 *  - Shadow factor: decision arithmetic, the 20 taps, cube-texel rule and comparison of m2s_relight taken ONCE per record from ws
 *    (count / 20); with use_shadows = 0 the factor is 0 and no cube is read.
 *  - degree 0..3: the coefficients i >= (degree + 1)^2 are written as +0.0; the others are the same bits at every degree.
 *  - One lane per record, no atomics: two calls give the same bytes.
 * The result is the context's coefficient plane float[n][48], per record f_dc[3], then f_rest[45] channel-major as the .ply orders
 * them (f_rest_{15 c + i - 1} for channel c, coefficient i = 1..15); with want_shadow_counts also uint8[n], the tap counts.
 * d_records == NULL: the context's records (n ignored), as m2s_shadow.  `light`: light_position, light_color, light_intensity and
 * near_far[1] are read; the cube is the context's (m2s_shadow / m2s_upload_shadow_cubemap), whatever its S.
 * Synchronous.  Errors: M2S_ERR_INVALID for degree > 3, a node count not listed above, reserved != 0; M2S_ERR_STATE without records,
 * or without a cube when use_shadows is set; M2S_ERR_CAPACITY beyond 2^32-1 records. */
typedef struct m2s_bake_params {
    float model_to_world[16];    /* column-major, as m2s_prepass_params */
    uint32_t degree;             /* 0..3 */
    uint32_t n_theta, n_phi;     /* 4 | 8, 8 | 16; 0 = the default 8 x 16 */
    uint32_t use_shadows;        /* 0: shadow factor 0, no cube needed */
    uint32_t viewer_metallic;    /* != 0: metallic 0, as the viewer's frame */
    uint32_t want_shadow_counts; /* also keep the per-record count of shadowed taps (0..20) */
    uint32_t reserved;           /* 0 */
} m2s_bake_params;
m2s_status m2s_bake_light(m2s_ctx* ctx, const m2s_bake_params* params, const m2s_light_params* light, const void* d_records, uint64_t n);
/* The table of an allowed (n_theta, n_phi) (0 = default): n_theta * n_phi rows of 20 floats.  Host only. */
m2s_status m2s_bake_directions(uint32_t n_theta, uint32_t n_phi, float* out, uint64_t capacity_floats);
/* The plane of the last m2s_bake_light: float[n][48] on the device.  NULL before any. */
const void* m2s_device_sh(const m2s_ctx* ctx);
m2s_status m2s_download_sh(m2s_ctx* ctx, float* dst, uint64_t capacity_records);
/* A plane made elsewhere (host float[n][48], the layout of m2s_download_sh, of this degree 0..3) becomes the context's plane of its
 * current records, without tap counts: what loaded records need in front of m2s_merge / m2s_lod_build with m2s_set_carry_sh.
 * M2S_ERR_INVALID: degree > 3, n != the stored records, NULL with n > 0.  M2S_ERR_STATE: no records, stale records, conversions in flight. */
m2s_status m2s_upload_sh(m2s_ctx* ctx, const float* host, uint64_t n, uint32_t degree);
/* The rows and the degree of the context's plane (either pointer may be NULL), whoever left it: a bake, m2s_upload_sh, a prune, and with
 * m2s_set_carry_sh a merge or a cut.  M2S_ERR_STATE without a plane. */
m2s_status m2s_sh_plane_info(const m2s_ctx* ctx, uint64_t* rows, uint32_t* degree);
/* uint8[n]: the tap counts of the last m2s_bake_light (want_shadow_counts); M2S_ERR_STATE otherwise. */
m2s_status m2s_download_bake_shadow_counts(m2s_ctx* ctx, uint8_t* dst, uint64_t capacity_bytes);
/* Duration (ms) of the last profiled m2s_bake_light kernel. */
float m2s_last_bake_ms(const m2s_ctx* ctx);
/* What a standard 3DGS viewer shows of the baked records from `camera_position`: record i of d_records (NULL: the context's, n ignored;
 * n must be the plane's) is copied to d_dst[i] (96 bytes each, a device buffer of the caller's) with color.rgb replaced by
 * max(0, ((0.5 + sh_0 B_0) + sh_1 B_1) + ... + sh_15 B_15) per channel — fp32, one rounding per operation, B(dir) with
 * dir = (ws - camera) * rsq(|ws - camera|^2) (the device's fast reciprocal square root), max keeps a NaN (a record AT the camera
 * gives NaN).  color.a and every other field are copied bit for bit.  M2S_ERR_STATE without a plane of n records. */
m2s_status m2s_sh_shade_records(m2s_ctx* ctx, const float model_to_world[16], const float camera_position[3], const void* d_records,
                                uint64_t n, void* d_dst);
/* Format-0 rows as m2s_write_ply writes them, except that the 48 floats f_dc_0..2, f_rest_0..44 of row i are sh[48 i .. 48 i + 47] as
 * given.  Host only. */
m2s_status m2s_write_ply_sh(const char* path, const m2s_gaussian* records, const float* sh, uint64_t n, float scale_multiplier);
/* The context's records and its baked plane as such a file (scale multiplier gaussian_std / R, as m2s_export_ply).  M2S_ERR_STATE
 * when no conversion has run, no plane exists or the plane's n is not the records'. */
m2s_status m2s_export_ply_sh(m2s_ctx* ctx, const char* path, float gaussian_std);

/* ---- compact export: Morton-ordered, chunk-quantised rows of 16 bytes ----------------------------------------------------------
 * A delivery format of 16.3 bytes per Gaussian instead of format 0's 248, laid out after the "compressed PLY" of the PlayCanvas /
 * SuperSplat tools as remembered — NOT verified against their reader: the header text and the bit layout below are this project's
 * definition.  All arithmetic is fp32, one rounding per operation, no contraction; `/` and sqrtf are IEEE; the logarithm is the C
 * library's logf (on the device: logf_glibc, m2s_logf.h).  Every min / max below is taken in the order of the real line with -0 below
 * +0, so that it does not depend on the order of a reduction.  mesh2splat_amd/csrc/m2s_compactmath.h states every step once, for the
 * host writer, the device encoder and the reader; tests/compact_ref.py restates it in numpy.
 *  1. A record is valid iff position.xyz, color.rgba, scale.xyz and rotation are finite, scale.xyz >= 0 and
 *     n2 = ((w*w + x*x) + y*y) + z*z is finite and > 0.  Invalid records are not written and are counted in `skipped`; N = valid records.
 *  2. bmin / bmax: per-axis min / max of position.xyz over the valid records.
 *  3. Per axis ext = bmax - bmin, i = ext > 0 ? min(1023, (uint)floorf(((p - bmin) / ext) * 1024.0f)) : 0 (0 too where that value is
 *     a NaN, i.e. ext overflowed); key = part1by2(ix) | part1by2(iy) << 1 | part1by2(iz) << 2 (30 bits).
 *  4. The valid records are sorted by key, stably (equal keys keep record order).  Chunk c = sorted rows [256 c, min(256 c + 256, N)),
 *     C = ceil(N / 256).
 *  5. Row values: p = position.xyz; ls_a = min(max(logf(scale_a * sm), -20), 20) with sm = the scale multiplier; col = color.rgb, or
 *     with a baked plane col_c = sh[row][c] * 0.28209479177387814f + 0.5f; alpha = color.a; a = (w, x, y, z) / sqrtf(n2).
 *  6. Chunk table, 18 floats per chunk: min_x min_y min_z max_x max_y max_z min_scale_x min_scale_y min_scale_z max_scale_x
 *     max_scale_y max_scale_z min_r min_g min_b max_r max_g max_b — min / max over the chunk's rows of p, ls and col.
 *  7. unorm(v, b), t = 2^b - 1: (uint)min(max(floorf(v * t + 0.5f), 0), t), 0 for a NaN.  nrm(v, lo, hi) = (hi - lo < 0.00001f) ? 0 :
 *     (v - lo) / (hi - lo).  packed_position = unorm(nx, 11) << 21 | unorm(ny, 10) << 11 | unorm(nz, 11); packed_scale the same on ls;
 *     packed_color = unorm(nr, 8) << 24 | unorm(ng, 8) << 16 | unorm(nb, 8) << 8 | unorm(alpha, 8) (alpha is not chunk-normalised);
 *     packed_rotation: L = the first index with the largest |a_i| (a later one replaces it only if strictly larger); if a_L < 0 every
 *     component is negated; word = L, then for i = 0..3, i != L, in order: word = word << 10 | unorm(a_i * 0.70710678f + 0.5f, 10).
 *  8. SH element, written iff a baked plane of degree d >= 1 is given: K = (d + 1)^2 - 1, properties uchar f_rest_0 .. f_rest_{3K-1},
 *     f_rest_{c K + i - 1} = coefficient i of channel c = word 3 + 15 c + i - 1 of the plane's float[48] row;
 *     byte = (uint)min(max(truncf((v / 8.0f + 0.5f) * 256.0f), 0), 255), 0 for a NaN.  Rows in the order of the vertex rows.
 *  9. File: the header has no comment lines and is exactly `ply`, `format binary_little_endian 1.0`, `element chunk C`, the 18
 *     `property float` lines, `element vertex N`, `property uint packed_position`, `property uint packed_rotation`,
 *     `property uint packed_scale`, `property uint packed_color`, with an SH element `element sh N` and its properties, `end_header`;
 *     then the chunk table, the vertex rows, the SH rows.  N = 0: a valid header with C = 0 and no data.
 * m2s_read_ply recognises the layout (a `chunk` element and the four packed_* properties) and decodes it: position = lo + t (hi - lo),
 * scale = exp(ls) (the multiplier stays in it; z as decoded), colour and alpha, the quaternion with its largest component rebuilt as
 * sqrt(max(0, 1 - a^2 - b^2 - c^2)); normal and pbr zero, has_pbr = 0; the sh element is bounds-checked and ignored. */
/* Host only, the pin in plain C++ and the yardstick of the device path.  sh (or NULL): float[n][48] as m2s_download_sh gives it, of
 * degree sh_degree (0..3; 0: the colour comes from the plane, no SH element).  out_counts (may be NULL) = { rows, chunks, skipped }.
 * M2S_ERR_CAPACITY beyond 2^32-1 records. */
m2s_status m2s_write_ply_compact(const char* path, const m2s_gaussian* records, const float* sh, uint32_t sh_degree, uint64_t n,
                                 float scale_multiplier, uint64_t out_counts[3]);
/* The context's records — converted, pruned, uploaded or adopted — as such a file; everything up to the file's bytes is computed on the
 * device.  sm = gaussian_std / R as m2s_export_ply; records without a resolutionTarget (m2s_upload_records) are taken as R = 1.
 * use_baked_sh: colour and SH element from the plane of the last m2s_bake_light, at its degree.  Leaves the records, the position plane,
 * the sorted quads and their sources, the contribution accumulators and the SH plane as they are.  Synchronous.
 * M2S_ERR_STATE without records, or with use_baked_sh without a plane of the records' count; M2S_ERR_CAPACITY beyond 2^32-1 records;
 * M2S_ERR_INVALID for a gaussian_std that is not finite or <= 0. */
m2s_status m2s_export_ply_compact(m2s_ctx* ctx, const char* path, float gaussian_std, int use_baked_sh, uint64_t out_counts[3]);
/* Stages (ms) of the last m2s_export_ply_compact: box + keys, sort, pack (device events), download + write (host clock). */
m2s_status m2s_last_compact_stage_ms(const m2s_ctx* ctx, float out_ms[4]);

/* ---- scene I/O == SceneManager::loadModel (minus GL) and parsers::loadPlyFile ------------------------ */
/* Host-side scene loaded from a binary glTF file: scene-graph transforms applied, de-indexed 17-float
 * vertex buffers, fallback normals/tangents, cumulative bboxes, RGBA8 textures (PNG) — exactly what
 * SceneManager::parseGltfFile/setupMeshBuffers/loadTextures leave in RenderContext
 * (SceneManager.cpp:195-649).  The returned m2s_mesh array can be passed to m2s_upload_scene and stays
 * valid until m2s_free_host_scene. */
typedef struct m2s_host_scene m2s_host_scene;
m2s_status m2s_load_glb(const char* path, m2s_host_scene** out_scene);
void m2s_free_host_scene(m2s_host_scene* scene);
uint32_t m2s_host_scene_num_meshes(const m2s_host_scene* scene);
const m2s_mesh* m2s_host_scene_meshes(const m2s_host_scene* scene);
const char* m2s_host_scene_mesh_name(const m2s_host_scene* scene, uint32_t i);   /* "<mesh name>_<counter>" */
const char* m2s_host_scene_warnings(const m2s_host_scene* scene);                 /* skipped primitives etc. */
/* Reads a binary .ply written by format 0 or 1 back into records (parsers.cpp:516-629): scale = exp,
 * alpha = sigmoid, colour = SH -> RGB, quaternion normalised; or a compact .ply ("compact export" above).  Free with m2s_free_records. */
m2s_status m2s_read_ply(const char* path, m2s_gaussian** out_records, uint64_t* out_n, int* out_has_pbr);
void m2s_free_records(m2s_gaussian* records);
/* m2s_read_ply that keeps the view-dependent colour.  Records, *out_n and *out_has_pbr are m2s_read_ply's, bit for bit.  For a file
 * with f_dc (every layout above but the compact one) *out_sh = float[n][48] in the layout of the baked plane (m2s_upload_sh,
 * m2s_write_ply_sh): f_dc_0..2, then 15 coefficients per colour channel.  *out_degree comes from the number of f_rest properties:
 * 0, 9, 24, 45 -> 0..3; a file of 45 has its row copied across, one of 3 c per channel c < 15 has channel k's c coefficients at
 * 3 + 15 k and +0 above them.  Any other number, an f_rest_* that is not a float or not one of f_rest_0 .. f_rest_{count-1}:
 * M2S_ERR_IO with m2s_io_last_error.  A compact .ply and a file of zero rows: *out_sh = NULL (degree 0, resp. the header's).  On
 * failure nothing is allocated.  out_sh and out_degree must not be NULL.  Free the plane with m2s_free_sh (NULL is fine). */
m2s_status m2s_read_ply_sh(const char* path, m2s_gaussian** out_records, uint64_t* out_n, int* out_has_pbr, float** out_sh, uint32_t* out_degree);
void m2s_free_sh(float* sh);
/* Message of the last failed scene-I/O call on this thread. */
const char* m2s_io_last_error(void);

/* ---- pipeline selection ------------------------------------------------------------------------ */
/* AUTO (default) decides once per (scene, R), from an exact fragment count taken at the first conversion:
 *   - fewer than 11 fragments per triangle on average: the SINGLE-PASS kernel (k_fused2 / its lean form k_fused3; the multi-pass
 *     pipeline from an R on at which a workgroup's fragments do not fit the kernel's LDS stream).  It emits every triangle of <= 16 pixel rows and <= 96 fragments
 *     itself; larger triangles only reserve their slice of the ordered output there and are emitted by a second
 *     kernel (k_emit_big, one workgroup per 1024-fragment chunk); a scene DOMINATED by such triangles falls through
 *     to the multi-pass pipeline;
 *   - otherwise the MULTI-PASS pipeline count -> scan -> offsets -> emit (output-range balanced, any triangle size).
 *   - a mesh far finer than the density asked for (BASELINE config 5) — fewer than 1.75 fragments per triangle on average
 *     in a scene of at least 2 M triangles, fewer than 0.5 in a smaller one (measured crossovers): the SPARSE form of the
 *     single-pass kernel (k_sparse): a cheap conservative test drops the triangles that cannot cover a pixel centre before
 *     the exact per-triangle phase runs on the survivors; k_fused2 where a workgroup does not fit.
 * MULTIPASS forces the multi-pass pipeline, TEAM / LEAN / SPARSE force the single-pass kernel in one of its forms.  Every
 * setting produces bit-identical output.  Changing the setting forgets the remembered decisions. */
enum { M2S_PIPELINE_AUTO = 0, M2S_PIPELINE_MULTIPASS = 1,
       /* 2: the one-wave-per-batch kernel of rounds 1-5 (k_fused), removed in round 6: m2s_set_pipeline rejects the value */
       M2S_PIPELINE_TEAM = 3 /* always the single-pass kernel, workgroup-cooperative form (k_fused2); the multi-pass pipeline where a
                                workgroup does not fit its LDS stream */,
       M2S_PIPELINE_SPARSE = 4 /* always the sparse form of the single-pass kernel (k_sparse) where the scene is large enough for
                                  it (>= ~172 k triangles), k_fused2 / the multi-pass pipeline where a workgroup does not fit its LDS stream */,
       M2S_PIPELINE_LEAN = 5 /* the team kernel in its lean form (k_fused3: four waves per SIMD; shades triangles of at most 8 x 8
                                pixels itself and defers the rest to k_emit_big) where the scene allows it — every mesh samples
                                three equally sized maps or none —, else as TEAM.  AUTO prefers it to k_fused2 under the same
                                condition and returns to k_fused2 at an R where many triangles were deferred */ };
m2s_status m2s_set_pipeline(m2s_ctx* ctx, int pipeline);
/* Which pipeline the last conversion actually ran: M2S_PIPELINE_MULTIPASS, _TEAM (k_fused2), _LEAN (k_fused3) or _SPARSE (k_sparse); 0 before any. */
int m2s_last_pipeline(const m2s_ctx* ctx);
/* The vertex table of the last m2s_upload_scene: *out_rows = distinct vertices among the resident triangles' corners (all 12 attribute
 * floats compared bitwise; 0 when the scene was not counted: it cannot take the LEAN form, or has more than 2^22 triangles);
 * *out_in_use = 1 when conversions in the LEAN form gather vertex attributes from that table (the indexed instance of k_fused3: fewer
 * than 2^21 rows and at most half as many rows as corners), 0 when they read the per-corner planes.  m2s_last_pipeline says
 * M2S_PIPELINE_LEAN for both; the records are the same bytes.  Either pointer may be NULL. */
m2s_status m2s_vertex_table(const m2s_ctx* ctx, uint64_t* out_rows, int* out_in_use);
/* The geometry planes of the last m2s_upload_scene: per resident triangle the Quaternion, the Scale and the box-normalised orthogonal
 * UVs of the triangle setup (48 bytes), which depend on the positions and the mesh's box but not on the resolution.  Built once per
 * upload for scenes that can take the LEAN form and have at most 2^22 resident triangles, where memory allows; conversions in the LEAN
 * form then read them instead of recomputing the setup.  *out_bytes = their size (0: not built), *out_in_use = 1 when LEAN conversions
 * read them.  The records are the same bytes either way.  Either pointer may be NULL. */
m2s_status m2s_geo_planes(const m2s_ctx* ctx, uint64_t* out_bytes, int* out_in_use);

/* ---- measurement ------------------------------------------------------------------------------- */
enum { M2S_K_COUNT = 0, M2S_K_SCAN = 1, M2S_K_OFFSETS = 2, M2S_K_EMIT = 3, M2S_K_FUSED = 4, M2S_K_N = 5 };
/* When enabled every convert brackets each kernel with hipEvents on its stream. */
m2s_status m2s_set_profiling(m2s_ctx* ctx, int enabled);
/* Kernel durations (ms) of the last profiled convert, indexed by M2S_K_*. */
m2s_status m2s_last_kernel_ms(const m2s_ctx* ctx, float out_ms[M2S_K_N]);
/* Scene facts for roofline accounting: triangles in range, meshes. */
uint64_t m2s_num_triangles(const m2s_ctx* ctx);
/* Test hook: sets the counter of single-pass launches (its low 16 bits tag the look-back chain words), so that a test
 * can walk a context across the wrap of that tag without issuing 65 536 conversions.  Requires an idle context. */
m2s_status m2s_debug_set_launch_counter(m2s_ctx* ctx, uint32_t value);

#ifdef __cplusplus
}
#endif
#endif /* M2S_H */
