// mesh2splat — headless command-line converter.  The reference has no CLI (src/utils/argparser.hpp is
// dead code and main() ignores argv); its workflows are the GUI's LoadModel -> RunConversion -> SavePLY event
// sequence (src/renderer/guiRendererConcreteMediator.cpp:11-29,51-57,111-115) and the batch state machine
// Idle -> Loading -> Converting -> Exporting per file (:134-251).  This tool runs both through the C ABI (include/m2s.h).
//
//   mesh2splat in.glb out.ply [options]                      one file
//   mesh2splat --batch in_dir --out out_dir [options]        every *.glb of in_dir -> out_dir/<name>.ply
//
//   --density R | --quality q [--max-res 1024|2048|4096]     defaults are the GUI's: quality 0.5, max-res 1024 ->
//                                                            R = int(16 + q*(maxRes-16)) = 520 (ImGuiUI.cpp:512, main.cpp:26)
//   --std s        gaussian std, default 0.65 (main.cpp:26)   --format 0|1|2   standard 3DGS / PBR / compressed PBR
//   --cap n        0 = unlimited, default: the reference formula        --pipeline auto|multipass
//   --device d     first HIP device to use                     --timing  per-stage wall clock
//   --gpus N       one process per GPU (devices d .. d+N-1):
//                    one file : the triangle list is cut into N fragment-balanced ranges (m2s_dist_shard_ranges), every
//                               rank converts its range, the N counters are exchanged (8 bytes each: through the shared
//                               mapping the forked ranks inherit) and every rank writes ITS rows of the one output file at
//                               their final offset (m2s_export_ply_slice) — no record leaves its GPU, no RCCL needed.
//                               --gather: instead, the counters go through RCCL (m2s_dist_all_gather_counts) and the blocks
//                               are concatenated on rank 0 over xGMI (m2s_dist_gather_records), which writes the file.
//                               --threads: the N ranks are THREADS of this process instead of forked processes (the reference's
//                               shape: one executable); with --gather the exchange then runs on the in-process transport
//                               (m2s_dist_local_id: hipMemcpyPeer over the same links, no RCCL).
//                    --batch  : file k goes to GPU k mod N (independent replicas, no exchange).
// One GPU, --batch: load(k+1) | upload + convert(k) | export(k-1) overlap (a loader thread, an exporter thread, two
// contexts used alternately so that file k's records stay intact while file k+1 converts).
#include <dirent.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../include/m2s.h"

namespace {

struct Options {
    std::string in, out, batch_dir, out_dir;
    double quality = 0.5, std_dev = 0.65;
    long max_res = 1024, density = -1, device = 0, cap = -1, format = 0, gpus = 1;
    int pipeline = M2S_PIPELINE_AUTO;
    bool timing = false, gather = false, force_sharded = false;   // force_sharded: the --gpus code path with one rank (tests)
    bool one_device = false;                                       // tests: every rank on --device (several processes share one GPU)
    bool threads = false;                                          // ranks as threads of this process
    std::string preview;                                           // --preview view.png: prepass + depth sort + splat of the result
    int preview_w = 1280, preview_h = 720;
    bool mesh_depth_test = false;                                  // --mesh-depth-test: the preview uses the mesh as occluder (m2s_mesh_depth)
    double split_screen = -1.0;                                    // --split-screen POS: the preview is the split screen, mesh left of POS * W (m2s_mesh_render + m2s_relight_split)
    int preview_mode = 0;                                          // --preview-mode N: 0..4 the albedo plane (as before), 5 / 6 the relit frame
    bool has_light = false;                                        // --light x,y,z[,intensity]
    bool bake_light = false;                                       // --bake-light: shadow + m2s_bake_light, the .ply carries the lit result (m2s_export_ply_sh)
    int bake_degree = 3;                                           // --bake-degree 0..3
    double light[4] = { 0, 0, 0, 0 };
    int score_views = 0;                                           // --score K: the fidelity score through K cameras round the scene (m2s_score_frames)
    double score_elevation = 0.0;                                  // --score-elevation deg
    int score_mask = 2;                                            // --score-mask 0..3
    std::string score_map;                                         // --score-map prefix: the error maps as prefix_k.png
    bool compact = false;                                          // --compact: out.ply in the compact layout (m2s_export_ply_compact) instead of --format's
    int prune_views = 0;                                           // --prune K: K cameras round the scene per elevation; drop the Gaussians none of them sees (m2s_prune)
    std::vector<double> prune_elevations = { -35.0, 0.0, 35.0 };   // --prune-elevations e1,e2,...
    double prune_weight = 1.0 / 255.0;                             // --prune-weight w: keep wmax > w
    long prune_pixels = 1;                                         // --prune-pixels n: keep npix >= n
    double prune_count_weight = 1.0 / 255.0;                       // --prune-count-weight c: a fragment counts with weight > c
    int refit_views = 0;                                           // --refit K: K cameras round the scene per elevation; refit the colours to the mesh render (m2s_refit_*)
    int refit_iters = 2;                                           // --refit-iters n (a guess nobody has tuned, like the two constants below)
    double refit_step = 1.0;                                       // --refit-step s
    std::vector<double> refit_elevations = { -35.0, 0.0, 35.0 };   // --refit-elevations e1,e2,...
    static constexpr uint32_t kRefitMinCover = 128;                // a pixel takes part from this splat alpha on
    static constexpr float kRefitMinWeightSum = 1.0f;              // a record is updated from this much accumulated weight on
    int merge_level = -1;                                          // --merge-level L (0..10): replace neighbouring Gaussians by their moment-matched parent (m2s_merge); -1: off
    long long merge_to = 0;                                        // --merge-to N: the same at the finest level that leaves at most N; 0: off
    int merge_group = 4;                                           // --merge-group g (2..64; 4 and the 0.5 below are guesses nobody has tuned)
    double merge_dot = 0.5;                                        // --merge-dot d
    bool merging() const { return merge_level >= 0 || merge_to > 0; }
    std::vector<uint32_t> lod_levels;                              // --lod-levels a,b,...: the merge levels of the level-of-detail tree's steps (m2s_lod_build); empty: off
    double lod_pixels = -1.0;                                      // --lod-pixels t: every --preview / --score camera takes its cut at tau_px = t first (m2s_lod_select)
    double view_distance = 1.0;                                    // --view-distance f (0.25..64): the --preview / --score eyes at f x the preview rule's distance, the far plane f x as far
    long long lod_budget = 0;                                      // --lod-budget N: every camera takes the finest cut of at most N records (m2s_lod_select_budget); --lod-pixels is then its floor
    double lod_guard = -1.0;                                       // --lod-frustum [--lod-guard g]: the cuts select only what their camera sees (m2s_lod_select_frustum,
    bool lod_occlusion = false;                                    // --lod-occlusion [--lod-depth-bias b]: ... and that the mesh does not hide (m2s_mesh_depth per camera, then
    double lod_depth_bias = -1.0;                                  //   m2s_lod_select_occluded, m2s_lod_select_budget_occluded); implies --lod-frustum; b >= 0, 0.00002 without --lod-depth-bias
    bool lod_frustum = false;                                      //   m2s_lod_select_budget_frustum), the frustum test widened by g (>= 1; 1.05, the prepass's own, without --lod-guard)
    double lod_blend = -1.0;                                       // --lod-blend b (0 < b <= 1): every cut is blended towards its nodes' parents over this band (m2s_lod_blend)
    std::string lod_ply;                                           // --lod-ply cut.ply: the --preview camera's cut as a .ply (with --bake-light: its carried SH plane, m2s_set_carry_sh)
    bool lod() const { return !lod_levels.empty(); }
    bool conversion_flag = false;                                  // one of --density / --quality / --max-res / --std / --cap / --pipeline was given: refused with a .ply input, which is not converted
    int merge_model = -1;                                          // --merge-model footprint|gaussian (m2s_set_merge_model) for --merge-level / --merge-to / --lod-levels; -1: not given
    double merge_sigma = -1.0;                                     // --merge-sigma s (> 0), with --merge-model: what a stored scale is multiplied with to be a standard deviation; < 0: 1
    bool merge_unsigned_axis = false;                              // --merge-unsigned-axis: M2S_MERGE_UNSIGNED_AXIS for --merge-level / --merge-to / --lod-levels
    bool world_units = false;                                      // --world-units: the scales divided by the density right after the conversion (m2s_records_to_world_units)
    long long budget = 0;                                          // --budget N: keep the N most important Gaussians (m2s_prune_budget); 0: off
    bool cap_set = false;                                          // an explicit --cap (without one, --budget converts with the cap lifted)
    long conversion_cap() const { return budget > 0 && !cap_set ? 0 : cap; }
    bool preview_mode_set = false;                                 // (--score lights its frames in mode 6 unless --preview-mode says otherwise)
    uint32_t R() const { return density > 0 ? (uint32_t)density : (uint32_t)(int)(16 + quality * (double)(max_res - 16)); }  // ImGuiUI.cpp:512
};

void usage() {
    std::fprintf(stderr,
                 "usage: mesh2splat in.glb|in.ply out.ply [options]\n"
                 "       mesh2splat --batch in_dir --out out_dir [options]\n"
                 "options: [--density R | --quality q [--max-res M]] [--std s] [--format 0|1|2] [--device d] [--gpus N [--gather]]\n"
                 "         [--cap n (0 = unlimited, default: reference formula)] [--pipeline auto|multipass] [--timing]\n"
                 "         [--preview view.png [--preview-size WxH (default 1280x720)] [--mesh-depth-test] [--split-screen POS (0..1)]]\n"
                 "         [--preview-mode N (0..6; 5 = metallic-roughness view, 6 = lit)] [--light x,y,z[,intensity]]\n"
                 "         [--score K [--score-elevation deg] [--score-mask 0..3] [--score-map prefix]]\n"
                 "         [--prune K [--prune-elevations e1,e2,...] [--prune-weight w] [--prune-pixels n] [--prune-count-weight c]]\n"
                 "         [--budget N] [--bake-light [--bake-degree 0..3]] [--compact]\n"
                 "         [--refit K [--refit-iters n] [--refit-step s] [--refit-elevations e1,e2,...]]\n"
                 "         [--merge-level L | --merge-to N] [--merge-group g] [--merge-dot d]\n"
                 "         [--lod-levels a,b,... --lod-pixels t | --lod-budget N [--lod-frustum [--lod-guard g]] [--lod-occlusion [--lod-depth-bias b]] [--lod-blend b] [--lod-ply cut.ply]] [--merge-unsigned-axis] [--view-distance f] [--world-units]\n"
                 "--preview: after the conversion, m2s_prepass (render mode 0) + m2s_sort_prepass + m2s_splat, and the albedo plane\n"
                 "  (top row first) as an 8-bit RGBA PNG.  Camera (double precision, matrices rounded to float; glm::lookAt / perspective):\n"
                 "  box = cumulative bounding box of the meshes, centre = (min + max) / 2, radius = |max - min| / 2,\n"
                 "  dist = 1.1 * radius / tan(radians(22.5)), eye = centre + (0, 0, dist), up = (0, 1, 0), looking at centre,\n"
                 "  45 deg vertical field of view, aspect W / H, near = dist / 100, far = dist * 10.\n"
                 "--split-screen POS: the preview is the reference's split screen (m2s_mesh_render + m2s_relight_split): the source mesh left\n"
                 "  of column (int)(POS * W), the splats right of it, two white divider columns; with --preview-mode 0..4 both sides show albedo.\n"
                 "--score K [--score-elevation deg (-90 < deg < 90, default 0)] [--score-mask 0..3 (default 2)] [--score-map prefix]: how close the\n"
                 "  splats look to the mesh.  K frames at --preview-size, lit with --preview-mode (default 6 here) and --light; per view the splat\n"
                 "  frame is compared on the device with the mesh-lit frame of the same camera (m2s_relight_mesh, m2s_score_frames) and ONE line\n"
                 "  `score: {...}` of JSON is printed: per view the eye and the integers of m2s_score_result, pooled (integers added) psnr_db, ssim,\n"
                 "  coverage_iou (null where undefined or infinite).  Camera rule: view 0 is the --preview camera; view k keeps its centre, distance,\n"
                 "  near, far and field of view, with the eye at centre + dist * (cos(el) sin(t), sin(el), cos(el) cos(t)), t = 2 pi k / K,\n"
                 "  el = the elevation.  Mask: 0 every pixel, 1 covered by the mesh, 2 by mesh or splats, 3 by both.\n"
                 "  --score-map: the error maps (|dR|, |dG|, |dB|, 255 on masked pixels) as prefix_k.png, top row first.\n"
                 "--bake-light [--bake-degree 0..3 (default 3)]: --format 0 only, one GPU, one file.  After the conversion the shadow pass\n"
                 "  (cube 1024, quads sized for --preview-size, the --preview camera's near / far) and m2s_bake_light with --light (default: the\n"
                 "  preview light); the .ply's f_dc / f_rest carry the lit, shadowed colour as spherical harmonics (m2s_export_ply_sh), so a\n"
                 "  standard 3DGS viewer shows the light.\n"
                 "--compact: out.ply is written in the compact layout instead of --format's (m2s_export_ply_compact: Morton-ordered chunks of\n"
                 "  256 rows, 16 bytes per row, laid out after the PlayCanvas compressed PLY; not verified against their reader).  It runs after\n"
                 "  --prune; with --bake-light the file carries the SH element.  Prints ONE line `compact: {...}` of JSON per file: rows, chunks,\n"
                 "  skipped, bytes, stage_ms (box + keys, sort, pack, download + write).  Not with --gpus N > 1 (the Morton order is global: slice\n"
                 "  writers do not apply), hence not with --batch together with --gpus; --batch alone works.\n"
                 "--budget N (>= 1): keep the N most important Gaussians (m2s_prune_budget), ties by index; fewer when fewer exist.  With\n"
                 "  --prune K the importance is npix * wmax over the K cameras' views and --prune's thresholds select the candidates; without\n"
                 "  it |scale x| * |scale y| * alpha of every record, right after the conversion (also with --batch).  It runs where --prune\n"
                 "  runs: before --bake-light, --compact, the export, --preview and --score.  --cap truncates in canonical order (the last\n"
                 "  meshes go first): without an explicit --cap the conversion runs with the cap lifted, an explicit one is honoured.  Prints\n"
                 "  ONE line `budget: {...}` of JSON per file: importance, max_records, before, candidates, kept, threshold_key, ties_kept,\n"
                 "  ties, cap_lifted.  Not with --gpus N > 1.  With --prune the `prune:` line changes its keys: it carries before, kept,\n"
                 "  dropped_thresholds (failed --prune's thresholds) and dropped_budget (passed them, cut by the budget) in place of\n"
                 "  dropped_weight / dropped_pixels, which a budget does not tell apart.  With --batch the per-file report times the selection\n"
                 "  as `budget`, apart from `convert`.\n"
                 "--refit K [--refit-iters n (default 2)] [--refit-step s (default 1)] [--refit-elevations e1,e2,... (default -35,0,35)]: refit the\n"
                 "  Gaussians' colours to the mesh render.  Per iteration, through K cameras round the scene at each elevation (the --score camera\n"
                 "  rule) at --preview-size: m2s_prepass_sorted, m2s_splat and m2s_mesh_render in mode 0, m2s_refit_accumulate over the two albedo\n"
                 "  planes; then m2s_refit_apply (one SART step; min_cover 128, min_weight_sum 1 and the two iterations are untuned guesses).  It\n"
                 "  runs after --prune / --budget and before --bake-light, --score, --preview, --compact and the export.  Prints ONE line\n"
                 "  `refit: {...}` of JSON: iterations, views, size, density, step, sse (the albedo planes' pooled squared error over the pixels\n"
                 "  both cover, before and after every iteration), pixels, and per iteration updated, clamped, no_weight.  Those are the TRAINING\n"
                 "  cameras: --score with other elevations (--score-elevation) is the held-out check.  Not with --gpus N > 1; with --batch the\n"
                 "  per-file report times it as `refit`.\n"
                 "--merge-level L (0..10) | --merge-to N (>= 1) [--merge-group g (2..64, default 4)] [--merge-dot d (default 0.5)]: level of detail\n"
                 "  without holes (m2s_merge): Gaussians that share a Morton cell of 2^L per axis are replaced, at most g at a time, by the\n"
                 "  moment-matched rectangle of their union; a group ends where two neighbours' normals have a dot product below d.  --merge-to\n"
                 "  takes the finest level whose count is at most N (dry runs, a bisection; level 10 where none is).  g = 4 and d = 0.5 are untuned\n"
                 "  guesses.  It runs after --prune / --budget and before --refit (which then corrects the parents' colours), --bake-light,\n"
                 "  --score, --preview, --compact and the export; the canonical record order is gone afterwards.  Prints ONE line `merge: {...}`\n"
                 "  of JSON per file: level, max_group, min_axis_dot, target, met, before, after, merged, invalid, stage_ms.  Not with\n"
                 "  --gpus N > 1.  With --batch the per-file report times it as `merge`.\n"
                 "--lod-levels a,b,... (1 to 16 merge levels, each 0..10, non-decreasing) --lod-pixels t (>= 0), with --preview and / or --score:\n"
                 "  level of detail per camera.  After the export (the file keeps the full records) the resident tree is built (m2s_lod_build,\n"
                 "  with --merge-group and --merge-dot), and the --preview camera and every --score camera first take their cut through it\n"
                 "  (m2s_lod_select at the eye, focal = view_to_clip[5] * H / 2, tau_px = t, near = the camera's near plane): each part of the\n"
                 "  surface once, as coarse as t pixels allow; the frame is drawn from the cut.  Prints ONE line `lod: {...}` of JSON per file:\n"
                 "  levels, nodes, per_level_nodes, skipped, tau_px, build_ms, views (per camera, the preview's first: selected, per_level).\n"
                 "  With --batch, which draws no frames, --score K names the cameras and every cut is a dry run.  Not with --gpus N > 1.\n"
                 "--lod-budget N (1 .. 2^32-1), with --lod-levels, in place of --lod-pixels or together with it: every camera takes the finest cut\n"
                 "  of at most N records instead (m2s_lod_select_budget; the tau_px is found on the device), never finer than t pixels where\n"
                 "  --lod-pixels t is given too.  A budget below the size of the coarsest level gets that level.  Every entry of `views` then also\n"
                 "  has tau_px (the tau the cut was taken at), met and selected_finer (the records of the next finer cut, the one that did not\n"
                 "  fit), and the line has \"budget\": N; its own tau_px is the floor (0 without --lod-pixels).\n"
                 "--lod-frustum [--lod-guard g] (g >= 1, default 1.05), with --lod-levels: every cut selects only nodes with a leaf inside its\n"
                 "  camera's frustum (m2s_lod_select_frustum, m2s_lod_select_budget_frustum), and a budget is spent on those alone.  The `lod:`\n"
                 "  line then has \"frustum\": g, and every entry of `views` \"visible_leaves\" and \"culled\" (nodes the plain cut selects\n"
                 "  and this one dropped).\n"
                 "--lod-occlusion [--lod-depth-bias b] (b >= 0, default 0.00002), with --lod-levels; implies --lod-frustum: in front of every cut the\n"
                 "  mesh is drawn depth-only through that cut's camera at --preview-size (m2s_mesh_depth), and a leaf behind that image under the\n"
                 "  prepass's own depth test is not inside either (m2s_lod_select_occluded, m2s_lod_select_budget_occluded): the far side of a\n"
                 "  closed mesh is neither selected nor charged to a budget.  The `lod:` line then has \"depth_bias\": b, and every entry of `views`\n"
                 "  \"occluded\" and \"translucent_kept\" (leaves behind the image kept for an alpha <= .95).  Not with --mesh-depth-test: a merged\n"
                 "  node lies under the surface its leaves lie on, and the prepass's depth test of its own position would cull it.\n"
                 "--lod-blend b (0 < b <= 1), with --lod-levels: every --preview / --score / --lod-ply cut is blended afterwards (m2s_lod_blend with\n"
                 "  the cut's camera and tau_px, a budget's being the one it found): each record moves towards its node's parent over the upper\n"
                 "  share b of its interval of tau_px^2, so that retaking the cut for a moving camera does not pop between levels.  The `lod:`\n"
                 "  line then has \"blend\": b and every entry of `views` \"blended\" (records with a weight above 0) and \"blend_ms\".  With\n"
                 "  --batch the cuts are dry runs: nothing is blended and only \"blend\": b is reported.  Not with --gpus N > 1.\n"
                 "--lod-ply cut.ply, with --lod-levels and --preview (one file, one GPU): right after the --preview camera's cut its records are\n"
                 "  written to cut.ply, in --format (m2s_export_ply).  With --bake-light the baked plane is carried through the tree and the cut\n"
                 "  (m2s_set_carry_sh, switched on in front of the bake) and cut.ply carries the SH element (m2s_export_ply_sh).  The `lod:` line\n"
                 "  gains \"cut_ply\", and with a carried plane \"sh_degree\".\n"
                 "--merge-unsigned-axis, with --merge-level, --merge-to or --lod-levels: the sign of a record's third axis carries no meaning\n"
                 "  (M2S_MERGE_UNSIGNED_AXIS: a group ends where |dot| is below d, and the members' axes are turned onto one side before they\n"
                 "  are averaged).  A conversion stores the two triangles of a flat quad with opposite signs, which the viewer does not see; with\n"
                 "  this flag they merge.  The `merge:` and `lod:` lines then carry \"unsigned_axis\": true.  Works with --batch; not with\n"
                 "  --gpus N > 1.\n"
                 "--view-distance f (0.25..64, default 1: what it was): the --preview and --score eyes stand at f x the camera rule's distance\n"
                 "  and the far plane is f x as far; near stays.\n"
                 "--merge-model footprint|gaussian [--merge-sigma s (> 0, default 1)], with --merge-level, --merge-to or --lod-levels: how those\n"
                 "  passes read a record (m2s_set_merge_model).  footprint, the default: the flat texel rectangle the conversion emits.  gaussian:\n"
                 "  a 3D Gaussian with standard deviations s * scale[0..2], what a .ply of another origin holds (s = 1) or a conversion behind\n"
                 "  --world-units (s = --std).  The `merge:` and `lod:` lines gain \"model\" and \"sigma\".  Not with --lod-blend under gaussian.\n"
                 "in.ply in place of in.glb: the file's Gaussians are read (m2s_read_ply_sh) and uploaded, nothing is converted.  --budget N (by\n"
                 "  area), --merge-level / --merge-to [--merge-model ...], --format, --compact and the export follow as after a conversion; a file\n"
                 "  with f_rest coefficients keeps them through all of these (--format 0 or --compact).  Prints ONE line `ply_in: {...}`: rows,\n"
                 "  has_pbr, sh_degree.  Everything that needs the mesh, a camera or a conversion is a usage error: --preview, --score, --refit,\n"
                 "  --prune, --bake-light, --split-screen, --mesh-depth-test, every --lod-*, --world-units, --density, --quality, --max-res, --std,\n"
                 "  --cap, --pipeline, --gpus N > 1, --batch.\n"
                 "--world-units: right after the conversion, in front of --prune, --budget, --merge-*, --refit, --bake-light, --score, --preview,\n"
                 "  --compact, the export and --lod-*, the records' scales are divided by the density and their resolutionTarget becomes 1\n"
                 "  (m2s_records_to_world_units); every later stage takes the divisor from the context.  --merge-* and --lod-* read scales as\n"
                 "  world lengths: with it their parents grow as a quadtree's and --lod-pixels counts screen pixels, without it density-ths of a\n"
                 "  pixel.  For a power-of-two density the export and the frames are the same bytes with and without it.  Prints ONE line\n"
                 "  `world_units: {\"records\": n, \"previous_R\": R, \"ms\": t}` of JSON per file (t: the call on the host's clock).  Works with\n"
                 "  --batch; not with --gpus N > 1.\n");
}

// ---- --preview: the albedo plane as a PNG (stored deflate blocks: no compression library needed) ----------------------------
uint32_t crc32_of(const uint8_t* p, size_t n, uint32_t crc = 0) {
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

bool write_png_rgba(const char* path, const uint8_t* rgba_bottom_up, int W, int H) {
    std::vector<uint8_t> raw;                         // filter byte 0 + the row, top row first
    raw.reserve((size_t)H * (1 + 4 * (size_t)W));
    for (int y = H - 1; y >= 0; --y) {
        raw.push_back(0);
        const uint8_t* row = rgba_bottom_up + (size_t)y * 4 * W;
        raw.insert(raw.end(), row, row + 4 * (size_t)W);
    }
    std::vector<uint8_t> z = { 0x78, 0x01 };          // zlib header, then stored blocks of at most 65535 bytes
    uint32_t s1 = 1, s2 = 0;
    for (size_t off = 0; off < raw.size() || off == 0;) {
        const size_t len = std::min<size_t>(65535, raw.size() - off);
        const bool last = off + len == raw.size();
        z.push_back(last ? 1 : 0);
        z.push_back(len & 0xFF); z.push_back(len >> 8);
        z.push_back(~len & 0xFF); z.push_back((~len >> 8) & 0xFF);
        for (size_t i = off; i < off + len; ++i) { s1 = (s1 + raw[i]) % 65521u; s2 = (s2 + s1) % 65521u; }
        z.insert(z.end(), raw.begin() + off, raw.begin() + off + len);
        off += len;
        if (last) break;
    }
    const uint32_t adler = (s2 << 16) | s1;
    for (int k = 3; k >= 0; --k) z.push_back((adler >> (8 * k)) & 0xFF);
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    auto be32 = [](std::vector<uint8_t>& v, uint32_t x) { for (int k = 3; k >= 0; --k) v.push_back((x >> (8 * k)) & 0xFF); };
    auto chunk = [&](const char* type, const std::vector<uint8_t>& body) {
        std::vector<uint8_t> c;
        be32(c, (uint32_t)body.size());
        c.insert(c.end(), type, type + 4);
        c.insert(c.end(), body.begin(), body.end());
        be32(c, crc32_of(c.data() + 4, c.size() - 4));
        std::fwrite(c.data(), 1, c.size(), f);
    };
    static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n' };
    std::fwrite(sig, 1, 8, f);
    std::vector<uint8_t> ihdr;
    be32(ihdr, (uint32_t)W); be32(ihdr, (uint32_t)H);
    ihdr.insert(ihdr.end(), { 8, 6, 0, 0, 0 });       // 8 bits, RGBA, deflate, no filter method, no interlace
    chunk("IHDR", ihdr);
    chunk("IDAT", z);
    chunk("IEND", {});
    return std::fclose(f) == 0;
}

// The preview camera rule: the cumulative bounding box's centre, the distance that fits its sphere into a 45 degree view, the planes.
void preview_rule(const m2s_mesh* meshes, uint32_t n_meshes, double ctr[3], double* dist, double* near_p, double* far_p) {
    double mn[3] = { 1e300, 1e300, 1e300 }, mx[3] = { -1e300, -1e300, -1e300 };
    for (uint32_t i = 0; i < n_meshes; ++i)
        for (int k = 0; k < 3; ++k) { mn[k] = std::min(mn[k], (double)meshes[i].bbox_min[k]); mx[k] = std::max(mx[k], (double)meshes[i].bbox_max[k]); }
    double d2 = 0;
    for (int k = 0; k < 3; ++k) { ctr[k] = (mn[k] + mx[k]) / 2; d2 += (mx[k] - mn[k]) * (mx[k] - mn[k]); }
    const double radius = std::sqrt(d2) / 2;
    *dist = 1.1 * radius / std::tan(22.5 * (M_PI / 180.0));
    *near_p = *dist / 100;
    *far_p = *dist * 10;
}

// glm::lookAt(eye, ctr, (0, 1, 0)) / glm::perspective(45 degrees, W / H, near, far) in double, column-major (m[c * 4 + r]), rounded to
// float (tests/camera.py and mesh2splat_amd/score.py: camera_from_eye do the same)
void camera_matrices(const double eye[3], const double ctr[3], double near_p, double far_p, int W, int H, float view[16], float proj[16]) {
    // lookAt: f = normalize(ctr - eye), s = normalize(cross(f, up)), u = cross(s, f)
    double f[3] = { ctr[0] - eye[0], ctr[1] - eye[1], ctr[2] - eye[2] };
    double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (double& v : f) v /= fl;
    const double up[3] = { 0, 1, 0 };
    double s[3] = { f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0] };
    double sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (double& v : s) v /= sl;
    const double u[3] = { s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0] };
    double m[16] = { 0 };
    m[15] = 1;
    for (int k = 0; k < 3; ++k) { m[k * 4 + 0] = s[k]; m[k * 4 + 1] = u[k]; m[k * 4 + 2] = -f[k]; }
    m[12] = -(s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2]);
    m[13] = -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]);
    m[14] = f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2];
    for (int k = 0; k < 16; ++k) view[k] = (float)m[k];
    const double t = std::tan(45.0 * (M_PI / 180.0) / 2.0), aspect = (double)W / (double)H;
    for (int k = 0; k < 16; ++k) proj[k] = 0.0f;
    proj[0] = (float)(1.0 / (aspect * t));
    proj[5] = (float)(1.0 / t);
    proj[10] = (float)(-(far_p + near_p) / (far_p - near_p));
    proj[11] = -1.0f;
    proj[14] = (float)(-(2.0 * far_p * near_p) / (far_p - near_p));
}

void preview_camera(const m2s_mesh* meshes, uint32_t n_meshes, int W, int H, float view[16], float proj[16], double eye[3], double ctr[3],
                    double* near_p, double* far_p, double view_distance = 1.0) {
    double dist;
    preview_rule(meshes, n_meshes, ctr, &dist, near_p, far_p);
    dist *= view_distance;                // (--view-distance; a factor of 1 changes no bit)
    *far_p *= view_distance;
    for (int k = 0; k < 3; ++k) eye[k] = ctr[k];
    eye[2] += dist;
    camera_matrices(eye, ctr, *near_p, *far_p, W, H, view, proj);
}

// The default point light of --preview-mode 5 / 6 (tests/light_ref.py: default_light mirrors it), in double: above and to the right of the
// preview camera's side of the scene, 1.5 bounding-sphere radii in front of the centre; intensity 4 radius^2.
void preview_light(const m2s_mesh* meshes, uint32_t n_meshes, double pos[3], double* intensity) {
    double mn[3] = { 1e300, 1e300, 1e300 }, mx[3] = { -1e300, -1e300, -1e300 };
    for (uint32_t i = 0; i < n_meshes; ++i)
        for (int k = 0; k < 3; ++k) { mn[k] = std::min(mn[k], (double)meshes[i].bbox_min[k]); mx[k] = std::max(mx[k], (double)meshes[i].bbox_max[k]); }
    double ctr[3], d2 = 0;
    for (int k = 0; k < 3; ++k) { ctr[k] = (mn[k] + mx[k]) / 2; d2 += (mx[k] - mn[k]) * (mx[k] - mn[k]); }
    const double radius = std::sqrt(d2) / 2;
    pos[0] = ctr[0] + 0.75 * radius; pos[1] = ctr[1] + 0.75 * radius; pos[2] = ctr[2] + 1.5 * radius;
    *intensity = 4.0 * radius * radius;
}

// --merge-model / --merge-sigma: the context's record model for the merges and the tree (nothing is set without the flag), and the
// two keys the `merge:` and `lod:` lines gain with it
m2s_status apply_merge_model(m2s_ctx* ctx, const Options& o) {
    return o.merge_model < 0 ? M2S_OK : m2s_set_merge_model(ctx, (uint32_t)o.merge_model, o.merge_sigma > 0.0 ? (float)o.merge_sigma : 1.0f);
}
std::string merge_model_json(const Options& o) {
    if (o.merge_model < 0) return "";
    char b[96];
    std::snprintf(b, sizeof b, ", \"model\": \"%s\", \"sigma\": %.9g", o.merge_model == M2S_MERGE_MODEL_GAUSSIAN ? "gaussian" : "footprint",
                  (double)(o.merge_sigma > 0.0 ? (float)o.merge_sigma : 1.0f));
    return b;
}

// --lod-levels / --lod-pixels / --lod-budget: the tree over the context's records (Converter.lod_build), then one cut per camera (Converter.lod_select / .lod_select_budget)
// in front of its frame; the views collect in `views` for the one `lod:` line
struct LodReport { uint64_t build[4] = {}; std::vector<uint64_t> first; float build_ms = 0; std::string views; std::string cut_ply; };   // cut_ply: the keys of --lod-ply

int lod_build(m2s_ctx* ctx, const Options& o, LodReport* rep) {
    m2s_lod_build_params bp;
    std::memset(&bp, 0, sizeof(bp));
    bp.n_steps = (uint32_t)o.lod_levels.size();
    for (size_t s = 0; s < o.lod_levels.size(); ++s) bp.levels[s] = o.lod_levels[s];
    bp.max_group = (uint32_t)o.merge_group;
    bp.min_axis_dot = (float)o.merge_dot;
    bp.flags = o.merge_unsigned_axis ? (uint32_t)M2S_MERGE_UNSIGNED_AXIS : 0u;
    uint32_t levels = 0;
    uint64_t first[M2S_LOD_MAX_STEPS + 2] = {};
    if (m2s_lod_build(ctx, &bp, rep->build) != M2S_OK || m2s_lod_levels(ctx, &levels, first) != M2S_OK) return 1;
    rep->first.assign(first, first + levels + 1);
    rep->build_ms = m2s_last_lod_build_ms(ctx);
    return 0;
}

int lod_cut(m2s_ctx* ctx, const Options& o, const double eye[3], const float world_to_view[16], const float view_to_clip[16], int H, double near_p,
            bool dry, LodReport* rep) {
    m2s_lod_select_params sp;
    std::memset(&sp, 0, sizeof(sp));
    for (int k = 0; k < 3; ++k) sp.camera_position[k] = (float)eye[k];
    sp.focal_px = view_to_clip[5] * (float)H / 2.0f;
    sp.tau_px = (float)o.lod_pixels;
    sp.near = (float)near_p;
    sp.flags = dry ? (uint32_t)M2S_LOD_DRY_RUN : 0u;
    uint64_t c[4] = {}, per[M2S_LOD_MAX_STEPS + 1] = {};
    std::string budget;
    float blend_tau = sp.tau_px;
    m2s_lod_frustum fr;                                                 // --lod-frustum: the camera's matrices, the records' space being the world's
    std::memset(&fr, 0, sizeof(fr));
    for (int k = 0; k < 4; ++k) fr.model_to_world[k * 5] = 1.0f;
    std::memcpy(fr.world_to_view, world_to_view, sizeof(fr.world_to_view));
    std::memcpy(fr.view_to_clip, view_to_clip, sizeof(fr.view_to_clip));
    fr.guard_band = (float)o.lod_guard;
    m2s_lod_occluder oc;                                                // --lod-occlusion: the mesh through this camera, the context's own image (depth NULL)
    std::memset(&oc, 0, sizeof(oc));
    oc.depth_on_device = 1;
    oc.depth_bias = (float)o.lod_depth_bias;
    if (o.lod_occlusion) {
        m2s_mesh_depth_params mp;
        std::memset(&mp, 0, sizeof(mp));
        std::memcpy(mp.world_to_view, fr.world_to_view, sizeof(mp.world_to_view));
        std::memcpy(mp.view_to_clip, fr.view_to_clip, sizeof(mp.view_to_clip));
        std::memcpy(mp.model_to_world, fr.model_to_world, sizeof(mp.model_to_world));
        mp.resolution[0] = o.preview_w; mp.resolution[1] = o.preview_h;
        if (m2s_mesh_depth(ctx, &mp, nullptr) != M2S_OK) return 1;
    }
    if (o.lod_budget > 0) {                                             // the cut that fits: --lod-pixels, where given, is its floor
        m2s_lod_budget_params bp;
        std::memset(&bp, 0, sizeof(bp));
        std::memcpy(bp.camera_position, sp.camera_position, sizeof(bp.camera_position));
        bp.focal_px = sp.focal_px;
        bp.near = sp.near;
        bp.tau_min_px = o.lod_pixels >= 0.0 ? (float)o.lod_pixels : 0.0f;
        bp.max_records = (uint32_t)o.lod_budget;
        bp.flags = sp.flags;
        m2s_lod_budget_result res;
        if ((o.lod_occlusion ? m2s_lod_select_budget_occluded(ctx, &bp, &fr, &oc, &res, c)
             : o.lod_frustum ? m2s_lod_select_budget_frustum(ctx, &bp, &fr, &res, c) : m2s_lod_select_budget(ctx, &bp, &res, c)) != M2S_OK) return 1;
        blend_tau = res.tau_px;
        char tau[40];
        std::snprintf(tau, sizeof tau, "%.9g", (double)res.tau_px);
        budget =std::string(", \"tau_px\": ") + tau + ", \"met\": " + (res.met ? "true" : "false") + ", \"selected_finer\": " +
                 std::to_string((unsigned long long)res.selected_finer);
    } else if ((o.lod_occlusion ? m2s_lod_select_occluded(ctx, &sp, &fr, &oc, c)
                : o.lod_frustum ? m2s_lod_select_frustum(ctx, &sp, &fr, c) : m2s_lod_select(ctx, &sp, c)) != M2S_OK) {
        return 1;
    }
    if (o.lod_frustum) {
        uint64_t fc[2] = {};
        if (m2s_last_lod_frustum_counts(ctx, fc) != M2S_OK) return 1;
        budget += ", \"visible_leaves\": " + std::to_string((unsigned long long)fc[0]) + ", \"culled\": " + std::to_string((unsigned long long)fc[1]);
    }
    if (o.lod_occlusion) {
        uint64_t ocn[4] = {};
        if (m2s_last_lod_occlusion_counts(ctx, ocn) != M2S_OK) return 1;
        budget += ", \"occluded\": " + std::to_string((unsigned long long)ocn[1]) + ", \"translucent_kept\": " + std::to_string((unsigned long long)ocn[2]);
    }
    if (o.lod_blend > 0.0 && !dry) {                                    // --lod-blend: the cut just taken, with its own camera and tau (a budget's: the one it found)
        m2s_lod_blend_params bl;
        std::memset(&bl, 0, sizeof(bl));
        std::memcpy(bl.camera_position, sp.camera_position, sizeof(bl.camera_position));
        bl.focal_px = sp.focal_px;
        bl.tau_px = blend_tau;
        bl.near = sp.near;
        bl.band = (float)o.lod_blend;
        uint64_t bc[4] = {};
        if (m2s_lod_blend(ctx, &bl, bc) != M2S_OK) return 1;
        char ms[40];
        std::snprintf(ms, sizeof ms, "%.4f", (double)m2s_last_lod_blend_ms(ctx));
        budget += ", \"blended\": " + std::to_string((unsigned long long)bc[1]) + ", \"blend_ms\": " + ms;
    }
    if (m2s_last_lod_level_counts(ctx, per) != M2S_OK) return 1;
    std::string levels;
    for (size_t l = 0; l + 1 < rep->first.size(); ++l) levels += std::string(l ? ", " : "") + std::to_string((unsigned long long)per[l]);
    rep->views += std::string(rep->views.empty() ? "" : ", ") + "{\"selected\": " + std::to_string((unsigned long long)c[1]) + ", \"per_level\": [" + levels + "]" +
                  budget + "}";
    return 0;
}

void lod_print(const Options& o, const LodReport& rep) {
    std::string levels, per;
    for (size_t s = 0; s < o.lod_levels.size(); ++s) levels += std::string(s ? ", " : "") + std::to_string(o.lod_levels[s]);
    for (size_t l = 0; l + 1 < rep.first.size(); ++l) per += std::string(l ? ", " : "") + std::to_string((unsigned long long)(rep.first[l + 1] - rep.first[l]));
    char tau[40];
    std::snprintf(tau, sizeof tau, "%.9g", o.lod_pixels >= 0.0 ? (double)(float)o.lod_pixels : 0.0);
    std::string budget = o.lod_budget > 0 ? ", \"budget\": " + std::to_string(o.lod_budget) : std::string();
    if (o.lod_frustum) {
        char g[40];
        std::snprintf(g, sizeof g, "%.9g", (double)(float)o.lod_guard);
        budget += std::string(", \"frustum\": ") + g;
    }
    if (o.lod_occlusion) {
        char b[40];
        std::snprintf(b, sizeof b, "%.9g", (double)(float)o.lod_depth_bias);
        budget += std::string(", \"depth_bias\": ") + b;
    }
    if (o.lod_blend > 0.0) {
        char b[40];
        std::snprintf(b, sizeof b, "%.9g", (double)(float)o.lod_blend);
        budget += std::string(", \"blend\": ") + b;
    }
    std::printf("lod: {\"levels\": [%s], \"nodes\": %llu, \"per_level_nodes\": [%s], \"skipped\": %llu, \"tau_px\": %s, \"build_ms\": %.4f, \"views\": [%s]%s%s%s}\n",
                levels.c_str(), (unsigned long long)rep.build[1], per.c_str(), (unsigned long long)rep.build[3], tau, rep.build_ms, rep.views.c_str(),
                (budget + rep.cut_ply).c_str(), o.merge_unsigned_axis ? ", \"unsigned_axis\": true" : "", merge_model_json(o).c_str());
}

// --lod-ply: the records the preview camera's cut left, as a .ply — with --bake-light the plane the tree carried (m2s_set_carry_sh) through
// m2s_export_ply_sh, else --format through m2s_export_ply
int lod_write_cut(m2s_ctx* ctx, const Options& o, LodReport* rep) {
    std::string path;
    for (char ch : o.lod_ply) { if (ch == '"' || ch == '\\') path += '\\'; path += ch; }
    rep->cut_ply = ", \"cut_ply\": \"" + path + "\"";
    if (!o.bake_light) return m2s_export_ply(ctx, o.lod_ply.c_str(), (uint32_t)o.format, (float)o.std_dev) == M2S_OK ? 0 : 1;
    uint64_t rows = 0;
    uint32_t degree = 0;
    if (m2s_sh_plane_info(ctx, &rows, &degree) != M2S_OK || rows != m2s_num_stored(ctx)) return 1;
    rep->cut_ply += ", \"sh_degree\": " + std::to_string(degree);
    return m2s_export_ply_sh(ctx, o.lod_ply.c_str(), (float)o.std_dev) == M2S_OK ? 0 : 1;
}

// GaussiansPrepass -> RadixSortPass -> GaussianSplattingPass of the converted records; the albedo attachment to `path` — with
// --preview-mode 5 / 6 followed by GaussianShadowPass -> GaussianRelightingPass, and the relit frame to `path`
int write_preview(m2s_ctx* ctx, const m2s_mesh* meshes, uint32_t n_meshes, uint32_t R, const Options& o, LodReport* lod) {
    const int W = o.preview_w, H = o.preview_h;
    m2s_prepass_params pp;
    std::memset(&pp, 0, sizeof(pp));
    double eye[3], ctr[3], near_p, far_p;
    preview_camera(meshes, n_meshes, W, H, pp.world_to_view, pp.view_to_clip, eye, ctr, &near_p, &far_p, o.view_distance);
    if (lod && lod_cut(ctx, o, eye, pp.world_to_view, pp.view_to_clip, H, near_p, false, lod) != 0) return 1;
    if (lod && !o.lod_ply.empty() && lod_write_cut(ctx, o, lod) != 0) return 1;
    for (int k = 0; k < 4; ++k) pp.model_to_world[k * 5] = 1.0f;
    pp.resolution[0] = W; pp.resolution[1] = H;
    pp.near_far[0] = (float)near_p; pp.near_far[1] = (float)far_p;
    pp.gaussian_std = (float)o.std_dev;
    pp.resolution_target = m2s_last_resolution(ctx);          // (the density; 1 behind --world-units)
    pp.render_mode = 0;
    pp.format = 0;
    std::printf("preview camera: eye=%.17g,%.17g,%.17g centre=%.17g,%.17g,%.17g near=%.17g far=%.17g\n", eye[0], eye[1], eye[2], ctr[0],
                ctr[1], ctr[2], near_p, far_p);
    uint64_t visible = 0, n = 0, skipped = 0;
    if (o.mesh_depth_test) {
        // the mesh as occluder: DepthPrepass with the preview camera, then the Gaussian prepass against its image (on the device)
        m2s_mesh_depth_params mp;
        std::memset(&mp, 0, sizeof(mp));
        std::memcpy(mp.world_to_view, pp.world_to_view, sizeof(mp.world_to_view));
        std::memcpy(mp.view_to_clip, pp.view_to_clip, sizeof(mp.view_to_clip));
        std::memcpy(mp.model_to_world, pp.model_to_world, sizeof(mp.model_to_world));
        mp.resolution[0] = W; mp.resolution[1] = H;
        uint64_t mc[5] = {};
        if (m2s_mesh_depth(ctx, &mp, mc) != M2S_OK) return 1;
        pp.depth_test_mesh = 1;
        pp.depth = static_cast<const float*>(m2s_device_mesh_depth(ctx));
        pp.depth_w = (uint32_t)W; pp.depth_h = (uint32_t)H;
        pp.depth_on_device = 1;
        if (m2s_prepass_sorted(ctx, &pp, &visible) != M2S_OK) return 1;
        n = visible;
        std::printf("mesh depth test: %llu triangles drawn (%llu clipped), %llu Gaussians pass\n", (unsigned long long)mc[0], (unsigned long long)mc[1],
                    (unsigned long long)visible);
        pp.depth_test_mesh = 0;          // (the shadow pass below reads the per-record fields only)
        pp.depth = nullptr;
        pp.depth_on_device = 0;
    } else {
        if (m2s_prepass(ctx, &pp, nullptr, 0, &visible) != M2S_OK) return 1;
        if (m2s_sort_prepass(ctx, &n) != M2S_OK) return 1;
    }
    std::vector<uint8_t> img((size_t)W * H * 4, 0);
    const bool split = o.split_screen >= 0.0;
    const bool relit = o.preview_mode == 5 || o.preview_mode == 6 || split;       // (the split screen is composed by the relighting pass)
    if (n || relit) {
        m2s_splat_params sp = { { W, H }, 0, 0 };
        static const m2s_quad none = {};
        if (m2s_splat(ctx, &sp, n ? nullptr : &none, 0, &skipped) != M2S_OK) return 1;      // (n = 0: cleared planes)
        if (!relit && m2s_download_gbuffer(ctx, 2, img.data(), img.size()) != M2S_OK) return 1;
    }
    if (relit) {
        m2s_light_params lp;
        std::memset(&lp, 0, sizeof(lp));
        double lpos[3], inten;
        preview_light(meshes, n_meshes, lpos, &inten);
        if (o.has_light) { for (int k = 0; k < 3; ++k) lpos[k] = o.light[k]; if (o.light[3] > 0) inten = o.light[3]; }
        for (int k = 0; k < 3; ++k) { lp.light_position[k] = (float)lpos[k]; lp.light_color[k] = 1.0f; lp.camera_position[k] = (float)eye[k]; }
        lp.light_intensity = (float)inten;
        lp.near_far[0] = (float)near_p; lp.near_far[1] = (float)far_p;
        lp.render_mode = o.preview_mode;
        lp.resolution[0] = W; lp.resolution[1] = H;
        lp.shadow_resolution = 1024;
        std::printf("preview light: position=%.17g,%.17g,%.17g intensity=%.17g colour=1,1,1 shadow=1024\n", lpos[0], lpos[1], lpos[2], inten);
        uint64_t per_face[6], sh_skipped = 0;
        if (m2s_shadow(ctx, &pp, &lp, nullptr, 0, per_face, &sh_skipped) != M2S_OK) return 1;
        if (split) {
            // MeshRenderPass with the preview camera, then the relighting pass with the mesh G-buffer left of the divider
            m2s_mesh_render_params mr;
            std::memset(&mr, 0, sizeof(mr));
            std::memcpy(mr.world_to_view, pp.world_to_view, sizeof(mr.world_to_view));
            std::memcpy(mr.view_to_clip, pp.view_to_clip, sizeof(mr.view_to_clip));
            std::memcpy(mr.model_to_world, pp.model_to_world, sizeof(mr.model_to_world));
            mr.resolution[0] = W; mr.resolution[1] = H;
            mr.near_far[0] = pp.near_far[0]; mr.near_far[1] = pp.near_far[1];
            mr.render_mode = pp.render_mode;
            uint64_t mc[6] = {};
            if (m2s_mesh_render(ctx, &mr, mc) != M2S_OK) return 1;
            std::printf("split screen at %.17g: %llu triangles drawn (%llu clipped, %llu culled as back-facing)\n", o.split_screen,
                        (unsigned long long)mc[0], (unsigned long long)mc[1], (unsigned long long)mc[5]);
            if (m2s_relight_split(ctx, &lp, (float)o.split_screen) != M2S_OK) return 1;
        } else if (m2s_relight(ctx, &lp) != M2S_OK) return 1;
        if (m2s_download_frame(ctx, img.data(), img.size()) != M2S_OK) return 1;
    }
    if (!write_png_rgba(o.preview.c_str(), img.data(), W, H)) { std::fprintf(stderr, "cannot write %s\n", o.preview.c_str()); return 2; }
    std::printf("preview %dx%d: %llu quads splatted -> %s\n", W, H, (unsigned long long)n, o.preview.c_str());
    return 0;
}

// --bake-light: GaussianShadowPass of the converted records (per-record fields as --preview's: identity model matrix, quads sized for
// --preview-size, the preview camera's near / far), then m2s_bake_light; the plane stays in the context for m2s_export_ply_sh
int bake_light(m2s_ctx* ctx, const m2s_mesh* meshes, uint32_t n_meshes, uint32_t R, const Options& o) {
    const int W = o.preview_w, H = o.preview_h;
    m2s_prepass_params pp;
    std::memset(&pp, 0, sizeof(pp));
    double eye[3], ctr[3], near_p, far_p;
    preview_camera(meshes, n_meshes, W, H, pp.world_to_view, pp.view_to_clip, eye, ctr, &near_p, &far_p);
    for (int k = 0; k < 4; ++k) pp.model_to_world[k * 5] = 1.0f;
    pp.resolution[0] = W; pp.resolution[1] = H;
    pp.near_far[0] = (float)near_p; pp.near_far[1] = (float)far_p;
    pp.gaussian_std = (float)o.std_dev;
    pp.resolution_target = m2s_last_resolution(ctx);          // (the density; 1 behind --world-units)
    m2s_light_params lp;
    std::memset(&lp, 0, sizeof(lp));
    double lpos[3], inten;
    preview_light(meshes, n_meshes, lpos, &inten);
    if (o.has_light) { for (int k = 0; k < 3; ++k) lpos[k] = o.light[k]; if (o.light[3] > 0) inten = o.light[3]; }
    for (int k = 0; k < 3; ++k) { lp.light_position[k] = (float)lpos[k]; lp.light_color[k] = 1.0f; lp.camera_position[k] = (float)eye[k]; }
    lp.light_intensity = (float)inten;
    lp.near_far[0] = (float)near_p; lp.near_far[1] = (float)far_p;
    lp.render_mode = 6;
    lp.resolution[0] = W; lp.resolution[1] = H;
    lp.shadow_resolution = 1024;
    uint64_t per_face[6], sh_skipped = 0;
    if (m2s_shadow(ctx, &pp, &lp, nullptr, 0, per_face, &sh_skipped) != M2S_OK) return 1;
    m2s_bake_params bp;
    std::memset(&bp, 0, sizeof(bp));
    for (int k = 0; k < 4; ++k) bp.model_to_world[k * 5] = 1.0f;
    bp.degree = (uint32_t)o.bake_degree;
    bp.use_shadows = 1;
    if (m2s_bake_light(ctx, &bp, &lp, nullptr, 0) != M2S_OK) return 1;
    std::printf("bake light: position=%.17g,%.17g,%.17g intensity=%.17g near=%.17g far=%.17g size=%dx%d shadow=1024 degree=%d\n", lpos[0], lpos[1],
                lpos[2], inten, near_p, far_p, W, H, o.bake_degree);
    return 0;
}

// --score K: per view GaussiansPrepass -> RadixSortPass -> GaussianSplattingPass -> GaussianShadowPass -> GaussianRelightingPass for the
// splats, MeshRenderPass -> m2s_relight_mesh for the mesh, m2s_score_frames over the context's own buffers (Converter.score does the same)
std::string json_num(double v) {
    if (!std::isfinite(v)) return "null";
    char b[40];
    std::snprintf(b, sizeof b, "%.17g", v);
    return b;
}

int write_score(m2s_ctx* ctx, const m2s_mesh* meshes, uint32_t n_meshes, uint32_t R, const Options& o, LodReport* lod) {
    const int W = o.preview_w, H = o.preview_h, K = o.score_views;
    const int mode = o.preview_mode_set ? o.preview_mode : 6;
    double ctr[3], dist, near_p, far_p, lpos[3], inten;
    preview_rule(meshes, n_meshes, ctr, &dist, &near_p, &far_p);
    dist *= o.view_distance;              // (--view-distance; a factor of 1 changes no bit)
    far_p *= o.view_distance;
    preview_light(meshes, n_meshes, lpos, &inten);
    if (o.has_light) { for (int k = 0; k < 3; ++k) lpos[k] = o.light[k]; if (o.light[3] > 0) inten = o.light[3]; }
    auto u64 = [](uint64_t v) { return std::to_string((unsigned long long)v); };
    auto three = [&](const uint64_t* v) { return "[" + u64(v[0]) + ", " + u64(v[1]) + ", " + u64(v[2]) + "]"; };
    auto integers = [&](const m2s_score_result& r) {
        const uint64_t mx[3] = { r.max_abs[0], r.max_abs[1], r.max_abs[2] };
        return "\"pixels\": " + u64(r.pixels) + ", \"cover\": [" + u64(r.cover[0]) + ", " + u64(r.cover[1]) + ", " + u64(r.cover[2]) + ", " + u64(r.cover[3]) +
               "], \"sse\": " + three(r.sse) + ", \"sad\": " + three(r.sad) + ", \"max_abs\": " + three(mx) + ", \"windows\": " + u64(r.windows) +
               ", \"ssim_q32\": " + std::to_string((long long)r.ssim_q32);
    };
    m2s_score_result pooled;
    std::memset(&pooled, 0, sizeof(pooled));
    std::string views;
    std::vector<uint8_t> map;
    for (int v = 0; v < K; ++v) {
        const double th = 2.0 * M_PI * v / K, el = o.score_elevation * (M_PI / 180.0);
        const double eye[3] = { ctr[0] + dist * std::cos(el) * std::sin(th), ctr[1] + dist * std::sin(el), ctr[2] + dist * std::cos(el) * std::cos(th) };
        m2s_prepass_params pp;
        std::memset(&pp, 0, sizeof(pp));
        camera_matrices(eye, ctr, near_p, far_p, W, H, pp.world_to_view, pp.view_to_clip);
        if (lod && lod_cut(ctx, o, eye, pp.world_to_view, pp.view_to_clip, H, near_p, false, lod) != 0) return 1;
        for (int k = 0; k < 4; ++k) pp.model_to_world[k * 5] = 1.0f;
        pp.resolution[0] = W; pp.resolution[1] = H;
        pp.near_far[0] = (float)near_p; pp.near_far[1] = (float)far_p;
        pp.gaussian_std = (float)o.std_dev;
        pp.resolution_target = m2s_last_resolution(ctx);          // (the density; 1 behind --world-units)
        m2s_light_params lp;
        std::memset(&lp, 0, sizeof(lp));
        for (int k = 0; k < 3; ++k) { lp.light_position[k] = (float)lpos[k]; lp.light_color[k] = 1.0f; lp.camera_position[k] = (float)eye[k]; }
        lp.light_intensity = (float)inten;
        lp.near_far[0] = (float)near_p; lp.near_far[1] = (float)far_p;
        lp.render_mode = mode;
        lp.resolution[0] = W; lp.resolution[1] = H;
        lp.shadow_resolution = 1024;
        uint64_t visible = 0, n = 0, skipped = 0, per_face[6], sh_skipped = 0;
        if (m2s_prepass(ctx, &pp, nullptr, 0, &visible) != M2S_OK || m2s_sort_prepass(ctx, &n) != M2S_OK) return 1;
        m2s_splat_params sp = { { W, H }, 0, 0 };
        static const m2s_quad none = {};
        if (m2s_splat(ctx, &sp, n ? nullptr : &none, 0, &skipped) != M2S_OK) return 1;        // (n = 0: cleared planes)
        if (m2s_shadow(ctx, &pp, &lp, nullptr, 0, per_face, &sh_skipped) != M2S_OK || m2s_relight(ctx, &lp) != M2S_OK) return 1;
        m2s_mesh_render_params mr;
        std::memset(&mr, 0, sizeof(mr));
        std::memcpy(mr.world_to_view, pp.world_to_view, sizeof(mr.world_to_view));
        std::memcpy(mr.view_to_clip, pp.view_to_clip, sizeof(mr.view_to_clip));
        std::memcpy(mr.model_to_world, pp.model_to_world, sizeof(mr.model_to_world));
        mr.resolution[0] = W; mr.resolution[1] = H;
        mr.near_far[0] = pp.near_far[0]; mr.near_far[1] = pp.near_far[1];
        mr.render_mode = pp.render_mode;
        if (m2s_mesh_render(ctx, &mr, nullptr) != M2S_OK || m2s_relight_mesh(ctx, &lp) != M2S_OK) return 1;
        m2s_score_params sc = { { W, H }, (uint32_t)o.score_mask, o.score_map.empty() ? 0u : (uint32_t)M2S_SCORE_WANT_MAP, { 0, 0 } };
        m2s_score_result r;
        if (m2s_score_frames(ctx, &sc, nullptr, nullptr, nullptr, nullptr, &r) != M2S_OK) return 1;
        if (!o.score_map.empty()) {
            map.resize((size_t)W * H * 4);
            if (m2s_download_score_map(ctx, map.data(), map.size()) != M2S_OK) return 1;
            const std::string path = o.score_map + "_" + std::to_string(v) + ".png";
            if (!write_png_rgba(path.c_str(), map.data(), W, H)) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 2; }
        }
        pooled.pixels += r.pixels; pooled.windows += r.windows; pooled.ssim_q32 += r.ssim_q32;
        for (int k = 0; k < 4; ++k) pooled.cover[k] += r.cover[k];
        for (int k = 0; k < 3; ++k) { pooled.sse[k] += r.sse[k]; pooled.sad[k] += r.sad[k]; pooled.max_abs[k] = std::max(pooled.max_abs[k], r.max_abs[k]); }
        views += std::string(v ? ", " : "") + "{\"eye\": [" + json_num(eye[0]) + ", " + json_num(eye[1]) + ", " + json_num(eye[2]) + "], \"quads\": " + u64(n) +
                 ", " + integers(r) + "}";
    }
    const double sse = (double)pooled.sse[0] + (double)pooled.sse[1] + (double)pooled.sse[2];
    const double psnr = pooled.pixels == 0 ? NAN : sse == 0 ? INFINITY : 10.0 * std::log10(65025.0 * 3.0 * (double)pooled.pixels / sse);
    const double ssim = pooled.windows ? (double)pooled.ssim_q32 / 4294967296.0 / (double)pooled.windows : NAN;
    const uint64_t uni = pooled.cover[1] + pooled.cover[2] + pooled.cover[3];
    const double iou = uni ? (double)pooled.cover[3] / (double)uni : NAN;
    std::printf("score: {\"views\": %d, \"size\": [%d, %d], \"density\": %u, \"mask\": %d, \"mode\": %d, \"elevation\": %s, \"centre\": [%s, %s, %s], \"near\": %s, "
                "\"far\": %s, \"light\": {\"position\": [%s, %s, %s], \"intensity\": %s}, \"per_view\": [%s], \"pooled\": {\"psnr_db\": %s, \"ssim\": %s, "
                "\"coverage_iou\": %s, %s}}\n",
                K, W, H, R, o.score_mask, mode, json_num(o.score_elevation).c_str(), json_num(ctr[0]).c_str(), json_num(ctr[1]).c_str(), json_num(ctr[2]).c_str(),
                json_num(near_p).c_str(), json_num(far_p).c_str(), json_num(lpos[0]).c_str(), json_num(lpos[1]).c_str(), json_num(lpos[2]).c_str(),
                json_num(inten).c_str(), views.c_str(), json_num(psnr).c_str(), json_num(ssim).c_str(), json_num(iou).c_str(), integers(pooled).c_str());
    return 0;
}

// --compact: the context's records as a compact .ply; prints one JSON line
int export_compact(m2s_ctx* ctx, const std::string& out, const Options& o, bool baked) {
    uint64_t c[3] = { 0, 0, 0 };
    float ms[4] = { 0, 0, 0, 0 };
    if (m2s_export_ply_compact(ctx, out.c_str(), (float)o.std_dev, baked ? 1 : 0, c) != M2S_OK || m2s_last_compact_stage_ms(ctx, ms) != M2S_OK) return 1;
    long long bytes = -1;
    if (FILE* f = std::fopen(out.c_str(), "rb")) { if (std::fseek(f, 0, SEEK_END) == 0) bytes = std::ftell(f); std::fclose(f); }
    std::printf("compact: {\"rows\": %llu, \"chunks\": %llu, \"skipped\": %llu, \"bytes\": %lld, \"stage_ms\": [%.4f, %.4f, %.4f, %.4f]}\n",
                (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], bytes, ms[0], ms[1], ms[2], ms[3]);
    return 0;
}

// --budget N: m2s_prune_budget over the context's records (VIEWS: the accumulators of run_prune); prints one JSON line
int run_budget(m2s_ctx* ctx, uint32_t importance, float min_weight, uint32_t min_pixels, const Options& o) {
    m2s_budget_params bp = { (uint64_t)o.budget, min_weight, min_pixels, importance, 0 };
    uint64_t kept = 0, c[6] = { 0, 0, 0, 0, 0, 0 };
    if (m2s_prune_budget(ctx, &bp, &kept) != M2S_OK || m2s_last_budget_counts(ctx, c) != M2S_OK) return 1;
    std::printf("budget: {\"importance\": \"%s\", \"max_records\": %lld, \"before\": %llu, \"candidates\": %llu, \"kept\": %llu, "
                "\"threshold_key\": %llu, \"ties_kept\": %llu, \"ties\": %llu, \"cap_lifted\": %s}\n",
                importance == M2S_IMPORTANCE_VIEWS ? "views" : "area", o.budget, (unsigned long long)c[0], (unsigned long long)c[1],
                (unsigned long long)c[2], (unsigned long long)c[3], (unsigned long long)c[4], (unsigned long long)c[5], o.cap_set ? "false" : "true");
    return 0;
}

// --merge-level L / --merge-to N: m2s_merge over the context's records (Converter.merge / .merge_to_budget do the same); prints one JSON line
int run_merge(m2s_ctx* ctx, const Options& o) {
    m2s_merge_params mp = { 0, (uint32_t)o.merge_group, (float)o.merge_dot, o.merge_unsigned_axis ? (uint32_t)M2S_MERGE_UNSIGNED_AXIS : 0u, { 0, 0 } };
    uint64_t c[4] = {};
    bool met = true;
    if (o.merge_to > 0) {
        auto count = [&](uint32_t level, uint64_t* after) {
            m2s_merge_params dry = mp;
            dry.level = level; dry.flags |= M2S_MERGE_DRY_RUN;
            uint64_t d[4] = {};
            if (m2s_merge(ctx, &dry, d) != M2S_OK) return false;
            *after = d[1];
            return true;
        };
        uint32_t lo = 0, hi = 10;                                  // the finest level in [lo, hi] that leaves at most N, if hi does
        uint64_t after = 0;
        if (!count(hi, &after)) return 1;
        met = after <= (uint64_t)o.merge_to;
        while (met && lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (!count(mid, &after)) return 1;
            if (after <= (uint64_t)o.merge_to) hi = mid; else lo = mid + 1;
        }
        mp.level = hi;
    } else {
        mp.level = (uint32_t)o.merge_level;
    }
    float ms[3] = {};
    if (m2s_merge(ctx, &mp, c) != M2S_OK || m2s_last_merge_stage_ms(ctx, ms) != M2S_OK) return 1;
    char target[32] = "null";
    if (o.merge_to > 0) std::snprintf(target, sizeof(target), "%lld", o.merge_to);
    std::printf("merge: {\"level\": %u, \"max_group\": %u, \"min_axis_dot\": %s, \"target\": %s, \"met\": %s, \"before\": %llu, \"after\": %llu, "
                "\"merged\": %llu, \"invalid\": %llu, \"stage_ms\": [%.4f, %.4f, %.4f]%s%s}\n",
                mp.level, mp.max_group, json_num((double)mp.min_axis_dot).c_str(), target, met ? "true" : "false", (unsigned long long)c[0],
                (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3], ms[0], ms[1], ms[2],
                o.merge_unsigned_axis ? ", \"unsigned_axis\": true" : "", merge_model_json(o).c_str());
    return 0;
}

// --world-units: m2s_records_to_world_units over the context's records (Converter.to_world_units does the same); prints one JSON line
int run_world_units(m2s_ctx* ctx) {
    uint32_t prev = 0;
    const auto a = std::chrono::steady_clock::now();
    if (m2s_records_to_world_units(ctx, &prev) != M2S_OK) return 1;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    std::printf("world_units: {\"records\": %llu, \"previous_R\": %u, \"ms\": %.4f}\n", (unsigned long long)m2s_num_stored(ctx), prev, ms);
    return 0;
}

// --refit K: K cameras round the scene at each elevation, at --preview-size; per iteration and camera m2s_prepass_sorted -> m2s_splat ->
// m2s_mesh_render -> m2s_refit_accumulate, then m2s_refit_apply (Converter.refit_views does the same).  Prints one JSON line.
int run_refit(m2s_ctx* ctx, const m2s_mesh* meshes, uint32_t n_meshes, uint32_t R, const Options& o) {
    const int W = o.preview_w, H = o.preview_h, K = o.refit_views;
    double ctr[3], dist, near_p, far_p;
    preview_rule(meshes, n_meshes, ctr, &dist, &near_p, &far_p);
    std::string sse, pixels, updated, clamped, starved;
    auto add = [](std::string& list, unsigned long long v) { list += std::string(list.empty() ? "" : ", ") + std::to_string(v); };
    for (int it = 0; it <= o.refit_iters; ++it) {
        const bool last = it == o.refit_iters;                     // (the pass behind the last iteration only measures)
        if (!last && m2s_refit_begin(ctx) != M2S_OK) return 1;
        unsigned long long sse_sum = 0, px_sum = 0;
        for (size_t e = 0; e < o.refit_elevations.size(); ++e) {
            for (int v = 0; v < K; ++v) {
                const double th = 2.0 * M_PI * v / K, el = o.refit_elevations[e] * (M_PI / 180.0);
                const double eye[3] = { ctr[0] + dist * std::cos(el) * std::sin(th), ctr[1] + dist * std::sin(el), ctr[2] + dist * std::cos(el) * std::cos(th) };
                m2s_prepass_params pp;
                std::memset(&pp, 0, sizeof(pp));
                camera_matrices(eye, ctr, near_p, far_p, W, H, pp.world_to_view, pp.view_to_clip);
                for (int k = 0; k < 4; ++k) pp.model_to_world[k * 5] = 1.0f;
                pp.resolution[0] = W; pp.resolution[1] = H;
                pp.near_far[0] = (float)near_p; pp.near_far[1] = (float)far_p;
                pp.gaussian_std = (float)o.std_dev;
                pp.resolution_target = m2s_last_resolution(ctx);          // (the density; 1 behind --world-units)
                uint64_t visible = 0, skipped = 0;
                if (m2s_prepass_sorted(ctx, &pp, &visible) != M2S_OK) return 1;
                m2s_splat_params sp = { { W, H }, 0, 0 };
                static const m2s_quad none = {};
                if (m2s_splat(ctx, &sp, visible ? nullptr : &none, 0, &skipped) != M2S_OK) return 1;          // (no quads: cleared planes)
                m2s_mesh_render_params mr;
                std::memset(&mr, 0, sizeof(mr));
                std::memcpy(mr.world_to_view, pp.world_to_view, sizeof(mr.world_to_view));
                std::memcpy(mr.view_to_clip, pp.view_to_clip, sizeof(mr.view_to_clip));
                std::memcpy(mr.model_to_world, pp.model_to_world, sizeof(mr.model_to_world));
                mr.resolution[0] = W; mr.resolution[1] = H;
                mr.near_far[0] = pp.near_far[0]; mr.near_far[1] = pp.near_far[1];
                mr.render_mode = 0;
                if (m2s_mesh_render(ctx, &mr, nullptr) != M2S_OK) return 1;
                m2s_score_params sc = { { W, H }, 3u, 0u, { 0, 0 } };
                m2s_score_result r;
                if (m2s_score_frames(ctx, &sc, m2s_device_mesh_gbuffer(ctx, 2), m2s_device_gbuffer(ctx, 2), nullptr, nullptr, &r) != M2S_OK) return 1;
                sse_sum += r.sse[0] + r.sse[1] + r.sse[2];
                px_sum += r.pixels;
                m2s_refit_params rp = { { W, H }, Options::kRefitMinCover, 0 };
                if (!last && visible && m2s_refit_accumulate(ctx, &rp, nullptr, nullptr, nullptr) != M2S_OK) return 1;
            }
        }
        add(sse, sse_sum);
        add(pixels, px_sum);
        if (last) break;
        m2s_refit_apply_params ap = { (float)o.refit_step, Options::kRefitMinWeightSum, { 0, 0 } };
        uint64_t c[4] = { 0, 0, 0, 0 };
        if (m2s_refit_apply(ctx, &ap, c) != M2S_OK) return 1;
        add(updated, c[1]); add(clamped, c[2]); add(starved, c[3]);
    }
    std::string els;
    for (size_t e = 0; e < o.refit_elevations.size(); ++e) els += std::string(e ? ", " : "") + json_num(o.refit_elevations[e]);
    std::printf("refit: {\"iterations\": %d, \"views\": %d, \"elevations\": [%s], \"size\": [%d, %d], \"density\": %u, \"step\": %s, \"min_cover\": %u, "
                "\"min_weight_sum\": %s, \"sse\": [%s], \"pixels\": [%s], \"updated\": [%s], \"clamped\": [%s], \"no_weight\": [%s]}\n",
                o.refit_iters, K * (int)o.refit_elevations.size(), els.c_str(), W, H, R, json_num((double)(float)o.refit_step).c_str(), Options::kRefitMinCover,
                json_num((double)Options::kRefitMinWeightSum).c_str(), sse.c_str(), pixels.c_str(), updated.c_str(), clamped.c_str(), starved.c_str());
    return 0;
}

// --prune K: K cameras round the scene at each elevation, at --preview-size; per camera m2s_prepass_sorted -> m2s_contrib_accumulate, then
// m2s_prune (Converter.prune_views does the same) — with --budget: m2s_prune_budget with the same thresholds, whose line follows; what the
// thresholds dropped is then not split into weight and pixels.  Prints one JSON line.
int run_prune(m2s_ctx* ctx, const m2s_mesh* meshes, uint32_t n_meshes, uint32_t R, const Options& o) {
    const int W = o.preview_w, H = o.preview_h, K = o.prune_views;
    double ctr[3], dist, near_p, far_p;
    preview_rule(meshes, n_meshes, ctr, &dist, &near_p, &far_p);
    if (m2s_contrib_begin(ctx) != M2S_OK) return 1;
    std::string eyes, els;
    for (size_t e = 0; e < o.prune_elevations.size(); ++e) {
        els += std::string(e ? ", " : "") + json_num(o.prune_elevations[e]);
        for (int v = 0; v < K; ++v) {
            const double th = 2.0 * M_PI * v / K, el = o.prune_elevations[e] * (M_PI / 180.0);
            const double eye[3] = { ctr[0] + dist * std::cos(el) * std::sin(th), ctr[1] + dist * std::sin(el), ctr[2] + dist * std::cos(el) * std::cos(th) };
            m2s_prepass_params pp;
            std::memset(&pp, 0, sizeof(pp));
            camera_matrices(eye, ctr, near_p, far_p, W, H, pp.world_to_view, pp.view_to_clip);
            for (int k = 0; k < 4; ++k) pp.model_to_world[k * 5] = 1.0f;
            pp.resolution[0] = W; pp.resolution[1] = H;
            pp.near_far[0] = (float)near_p; pp.near_far[1] = (float)far_p;
            pp.gaussian_std = (float)o.std_dev;
            pp.resolution_target = m2s_last_resolution(ctx);          // (the density; 1 behind --world-units)
            uint64_t visible = 0;
            if (m2s_prepass_sorted(ctx, &pp, &visible) != M2S_OK) return 1;
            m2s_splat_params sp = { { W, H }, 0, 0 };
            if (visible && m2s_contrib_accumulate(ctx, &sp, (float)o.prune_count_weight) != M2S_OK) return 1;
            eyes += std::string(eyes.empty() ? "" : ", ") + "[" + json_num(eye[0]) + ", " + json_num(eye[1]) + ", " + json_num(eye[2]) + "]";
        }
    }
    m2s_prune_params pr = { (float)o.prune_weight, (uint32_t)o.prune_pixels, 0 };
    uint64_t kept = 0, c[4] = { 0, 0, 0, 0 };
    if (o.budget > 0) {
        uint64_t b[6] = { 0, 0, 0, 0, 0, 0 };
        if (run_budget(ctx, M2S_IMPORTANCE_VIEWS, pr.min_weight, pr.min_pixels, o) != 0 || m2s_last_budget_counts(ctx, b) != M2S_OK) return 1;
        std::printf("prune: {\"views\": %d, \"elevations\": [%s], \"size\": [%d, %d], \"density\": %u, \"min_weight\": %s, \"min_pixels\": %ld, "
                    "\"count_weight\": %s, \"eyes\": [%s], \"before\": %llu, \"kept\": %llu, \"dropped_thresholds\": %llu, \"dropped_budget\": %llu}\n",
                    K, els.c_str(), W, H, R, json_num((double)pr.min_weight).c_str(), o.prune_pixels, json_num((double)(float)o.prune_count_weight).c_str(),
                    eyes.c_str(), (unsigned long long)b[0], (unsigned long long)b[2], (unsigned long long)(b[0] - b[1]), (unsigned long long)(b[1] - b[2]));
        return 0;
    }
    if (m2s_prune(ctx, &pr, &kept) != M2S_OK || m2s_last_prune_counts(ctx, c) != M2S_OK) return 1;
    std::printf("prune: {\"views\": %d, \"elevations\": [%s], \"size\": [%d, %d], \"density\": %u, \"min_weight\": %s, \"min_pixels\": %ld, "
                "\"count_weight\": %s, \"eyes\": [%s], \"before\": %llu, \"kept\": %llu, \"dropped_weight\": %llu, \"dropped_pixels\": %llu}\n",
                K, els.c_str(), W, H, R, json_num((double)pr.min_weight).c_str(), o.prune_pixels, json_num((double)(float)o.prune_count_weight).c_str(), eyes.c_str(),
                (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3]);
    return 0;
}

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// ---- one file on one GPU ---------------------------------------------------------------------------------------------
int convert_one(const Options& o) {
    const auto t0 = Clock::now();
    // the HIP runtime and the context come up on a second thread while the .glb is parsed and its images decoded
    m2s_ctx* ctx = nullptr;
    m2s_status create_status = M2S_OK;
    double create_ms = 0;
    std::thread init([&] {
        const auto a = Clock::now();
        create_status = m2s_create((int)o.device, &ctx);
        if (create_status == M2S_OK) (void)m2s_prepare(ctx, M2S_PREPARE_UPLOAD | M2S_PREPARE_EXPORT | M2S_PREPARE_KERNELS);   // pinned buffers, code objects: off the critical path
        create_ms = ms_between(a, Clock::now());
    });
    m2s_host_scene* scene = nullptr;
    const m2s_status ls = m2s_load_glb(o.in.c_str(), &scene);
    const auto t1 = Clock::now();
    init.join();
    if (ls != M2S_OK) { std::fprintf(stderr, "%s\n", m2s_io_last_error()); if (ctx) m2s_destroy(ctx); return 1; }
    if (*m2s_host_scene_warnings(scene)) std::fprintf(stderr, "%s", m2s_host_scene_warnings(scene));
    if (create_status != M2S_OK) { std::fprintf(stderr, "%s\n", m2s_last_error(nullptr)); m2s_free_host_scene(scene); return 1; }
    const auto t1b = Clock::now();
    auto die = [&](const char* what) { std::fprintf(stderr, "%s: %s\n", what, m2s_last_error(ctx)); m2s_destroy(ctx); m2s_free_host_scene(scene); return 1; };
    if (m2s_set_pipeline(ctx, o.pipeline) != M2S_OK) return die("set_pipeline");
    if (m2s_set_max_gaussians(ctx, o.conversion_cap()) != M2S_OK) return die("set_max_gaussians");
    if (apply_merge_model(ctx, o) != M2S_OK) return die("merge model");
    (void)m2s_set_resolution_hint(ctx, o.R());   // the upload prepares for the conversion below
    if (m2s_upload_scene(ctx, m2s_host_scene_meshes(scene), m2s_host_scene_num_meshes(scene)) != M2S_OK) return die("upload");
    const auto t2 = Clock::now();
    uint64_t total = 0;
    const uint32_t R = o.R();
    if (m2s_convert(ctx, R, &total) != M2S_OK) return die("convert");
    const auto t3 = Clock::now();
    if (o.world_units && run_world_units(ctx) != 0) return die("world units");
    if (o.prune_views > 0 && run_prune(ctx, m2s_host_scene_meshes(scene), m2s_host_scene_num_meshes(scene), R, o) != 0) return die("prune");
    if (o.budget > 0 && o.prune_views == 0 && run_budget(ctx, M2S_IMPORTANCE_AREA, 0.0f, 0, o) != 0) return die("budget");
    if (o.merging() && run_merge(ctx, o) != 0) return die("merge");
    if (o.refit_views > 0 && run_refit(ctx, m2s_host_scene_meshes(scene), m2s_host_scene_num_meshes(scene), R, o) != 0) return die("refit");
    if (o.bake_light) {
        if (!o.lod_ply.empty() && m2s_set_carry_sh(ctx, 1) != M2S_OK) return die("carry sh");   // (the tree below then carries the baked plane into its cuts)
        if (bake_light(ctx, m2s_host_scene_meshes(scene), m2s_host_scene_num_meshes(scene), R, o) != 0) return die("bake");
        if (o.compact) { if (export_compact(ctx, o.out, o, true) != 0) return die("export"); }
        else if (m2s_export_ply_sh(ctx, o.out.c_str(), (float)o.std_dev) != M2S_OK) return die("export");
    } else if (o.compact) { if (export_compact(ctx, o.out, o, false) != 0) return die("export"); }
    else if (m2s_export_ply(ctx, o.out.c_str(), (uint32_t)o.format, (float)o.std_dev) != M2S_OK) return die("export");
    LodReport lod;
    if (o.lod() && lod_build(ctx, o, &lod) != 0) return die("lod");       // (after the export: the file keeps the full records)
    if (!o.preview.empty()) {
        const int pr = write_preview(ctx, m2s_host_scene_meshes(scene), m2s_host_scene_num_meshes(scene), R, o, o.lod() ? &lod : nullptr);
        if (pr == 1) return die("preview");
        if (pr) { m2s_destroy(ctx); m2s_free_host_scene(scene); return 1; }
    }
    if (o.score_views > 0) {
        const int sr = write_score(ctx, m2s_host_scene_meshes(scene), m2s_host_scene_num_meshes(scene), R, o, o.lod() ? &lod : nullptr);
        if (sr == 1) return die("score");
        if (sr) { m2s_destroy(ctx); m2s_free_host_scene(scene); return 1; }
    }
    if (o.lod()) lod_print(o, lod);
    const auto t4 = Clock::now();
    std::printf("%s: %u mesh(es), %llu triangles, density %u -> %llu Gaussians (%llu stored) -> %s (format %ld)\n", o.in.c_str(),
                m2s_host_scene_num_meshes(scene), (unsigned long long)m2s_num_triangles(ctx), R, (unsigned long long)total,
                (unsigned long long)m2s_num_stored(ctx), o.out.c_str(), o.format);
    if (o.timing) {
        float up[4] = { 0, 0, 0, 0 };
        (void)m2s_last_upload_ms(ctx, up);
        std::printf("load %.2f ms (HIP runtime + context %.2f ms, on a second thread; waited %.2f ms for it) | upload %.2f ms (geometry %.2f, textures %.2f, "
                    "allocations %.2f) | convert %.3f ms (first call, incl. buffer allocation) | export %.2f ms | total %.2f ms\n",
                    ms_between(t0, t1), create_ms, ms_between(t1, t1b), ms_between(t1b, t2), up[1], up[2], up[3], ms_between(t2, t3),
                    ms_between(t3, t4), ms_between(t0, t4));
    }
    m2s_destroy(ctx);
    m2s_free_host_scene(scene);
    return 0;
}

// ---- a .ply in place of a .glb: no conversion ----------------------------------------------------------------------------
// The file's Gaussians (m2s_read_ply_sh) become the context's records; --budget (AREA), --merge-* and the export follow as after a
// conversion.  A plane of degree >= 1 is uploaded with them and carried (m2s_set_carry_sh) into a standard-layout or compact file.
// Uploaded records carry no resolutionTarget, which m2s_export_ply and m2s_export_ply_sh divide by: the records come back to the
// host and the host writers take them with scale multiplier 1 (a .ply holds the drawn deviations); the compact export takes 0 as 1.
int convert_ply(const Options& o) {
    m2s_gaussian* rec = nullptr;
    float* sh = nullptr;
    uint64_t n = 0;
    int has_pbr = 0;
    uint32_t degree = 0;
    if (m2s_read_ply_sh(o.in.c_str(), &rec, &n, &has_pbr, &sh, &degree) != M2S_OK) { std::fprintf(stderr, "%s: %s\n", o.in.c_str(), m2s_io_last_error()); return 1; }
    m2s_ctx* ctx = nullptr;
    if (m2s_create((int)o.device, &ctx) != M2S_OK) { std::fprintf(stderr, "%s\n", m2s_last_error(nullptr)); m2s_free_records(rec); m2s_free_sh(sh); return 1; }
    auto die = [&](const char* what) { std::fprintf(stderr, "%s: %s\n", what, m2s_last_error(ctx)); m2s_destroy(ctx); m2s_free_records(rec); m2s_free_sh(sh); return 1; };
    const bool carried = sh && degree >= 1;
    if (apply_merge_model(ctx, o) != M2S_OK) return die("merge model");
    if (m2s_upload_records(ctx, rec, n) != M2S_OK) return die("upload");
    if (carried && (m2s_set_carry_sh(ctx, 1) != M2S_OK || m2s_upload_sh(ctx, sh, n, degree) != M2S_OK)) return die("upload sh");
    std::printf("ply_in: {\"rows\": %llu, \"has_pbr\": %s, \"sh_degree\": %u}\n", (unsigned long long)n, has_pbr ? "true" : "false", degree);
    m2s_free_records(rec); rec = nullptr;
    m2s_free_sh(sh); sh = nullptr;
    if (o.budget > 0 && run_budget(ctx, M2S_IMPORTANCE_AREA, 0.0f, 0, o) != 0) return die("budget");
    if (o.merging() && run_merge(ctx, o) != 0) return die("merge");
    const uint64_t stored = m2s_num_stored(ctx);
    if (o.compact) {
        Options one = o;
        one.std_dev = 1.0;
        if (export_compact(ctx, o.out, one, carried) != 0) return die("export");
    } else {
        std::vector<m2s_gaussian> out((size_t)std::max<uint64_t>(stored, 1));
        std::vector<float> plane;
        if (m2s_download(ctx, out.data(), stored) != M2S_OK) return die("download");
        if (carried && o.format == 0) {
            plane.resize((size_t)std::max<uint64_t>(stored, 1) * 48);
            if (m2s_download_sh(ctx, plane.data(), stored) != M2S_OK) return die("download sh");
        }
        const m2s_status ws = plane.empty() ? m2s_write_ply(o.out.c_str(), out.data(), stored, (uint32_t)o.format, 1.0f)
                                            : m2s_write_ply_sh(o.out.c_str(), out.data(), plane.data(), stored, 1.0f);
        if (ws != M2S_OK) { std::fprintf(stderr, "cannot write %s\n", o.out.c_str()); m2s_destroy(ctx); return 1; }
    }
    std::printf("%s: %llu Gaussians (%llu stored) -> %s (%s)\n", o.in.c_str(), (unsigned long long)n, (unsigned long long)stored, o.out.c_str(),
                o.compact ? "compact" : ("format " + std::to_string(o.format)).c_str());
    m2s_destroy(ctx);
    return 0;
}

// ---- one file on N GPUs: fork N ranks AFTER the (CPU-only) load so that they share the host scene copy-on-write -----------
struct Shared {
    std::atomic<int> id_ready;
    uint8_t id[M2S_DIST_ID_BYTES];
    std::atomic<int> failed;
    // the counters of a sharded conversion whose ranks write their own rows: N x 8 bytes through this mapping (the ranks
    // are forked children of one process on one node); RCCL is only brought up when records have to move (--gather)
    std::atomic<int> arrived;
    std::atomic<unsigned long long> counts[64];
    std::atomic<int> stage[64];   // --gather: how far each rank has got (see rendezvous below)
};

int rank_main(const Options& o, const m2s_host_scene* scene, Shared* sh, int rank, int world) {
    const m2s_mesh* meshes = m2s_host_scene_meshes(scene);
    const uint32_t n_meshes = m2s_host_scene_num_meshes(scene);
    const uint32_t R = o.R();
    const int device = (int)o.device + (o.one_device ? 0 : rank);
    auto fail = [&](const char* what, const char* msg) { std::fprintf(stderr, "[rank %d] %s: %s\n", rank, what, msg); sh->failed.store(1); return 1; };
    // --gather: RCCL calls are collectives — a rank that fails before one must not leave the others blocked inside it
    // (ncclCommInitRank, the counter all-gather, the record exchange).  Before each of them every rank reports, through the
    // shared mapping, that it got there in one piece; a rank that sees `failed` leaves instead of entering.
    auto rendezvous = [&](int stage) -> bool {
        sh->stage[rank].store(stage);
        for (;;) {
            if (sh->failed.load()) return false;
            int behind = 0;
            for (int r = 0; r < world; ++r) behind += sh->stage[r].load() < stage;
            if (!behind) return true;
            usleep(100);
        }
    };
    const auto t0 = Clock::now();
    std::vector<uint64_t> first((size_t)world), count((size_t)world);
    if (m2s_dist_shard_ranges(meshes, n_meshes, R, world, first.data(), count.data()) != M2S_OK) return fail("shard_ranges", m2s_dist_last_error(nullptr));
    m2s_ctx* ctx = nullptr;
    if (m2s_create(device, &ctx) != M2S_OK) return fail("create", m2s_last_error(nullptr));
    m2s_dist* d = nullptr;
    if (o.gather) {   // records will move between GPUs: one RCCL communicator per rank, id through the shared mapping
        if (rank == 0 && !o.threads) {   // (with --threads the parent made the in-process group's id before starting the ranks)
            if (m2s_dist_unique_id(sh->id) != M2S_OK) return fail("unique_id", m2s_dist_last_error(nullptr));
            sh->id_ready.store(1);
        } else {
            while (!sh->id_ready.load()) { if (sh->failed.load()) return 1; usleep(200); }
        }
        if (!rendezvous(1)) return 1;                 // every rank has a context and the id: nobody is left alone in ncclCommInitRank
        if (m2s_dist_create(device, sh->id, rank, world, &d) != M2S_OK) return fail("dist_create", m2s_dist_last_error(nullptr));
    }
    const auto t1 = Clock::now();
    // the merged scene may exceed the reference's cap envelope: every rank stores all of its records, the global cap is
    // applied to the row ranges below (the merged buffer keeps the first `cap` records in canonical order)
    (void)m2s_set_pipeline(ctx, o.pipeline);
    (void)m2s_set_max_gaussians(ctx, 0);
    (void)m2s_set_triangle_range(ctx, first[(size_t)rank], count[(size_t)rank]);
    (void)m2s_set_resolution_hint(ctx, R);
    if (m2s_upload_scene(ctx, meshes, n_meshes) != M2S_OK) return fail("upload", m2s_last_error(ctx));
    const auto t2 = Clock::now();
    uint64_t total = 0;
    if (m2s_convert(ctx, R, &total) != M2S_OK) return fail("convert", m2s_last_error(ctx));
    std::vector<uint64_t> counts((size_t)world), keep((size_t)world), offs((size_t)world + 1);
    if (d) {
        if (!rendezvous(2)) return 1;                 // every rank has uploaded and converted
        if (m2s_dist_all_gather_counts(d, total, counts.data(), nullptr) != M2S_OK) return fail("all_gather_counts", m2s_dist_last_error(d));
    } else {
        sh->counts[rank].store(total);
        sh->arrived.fetch_add(1);
        while (sh->arrived.load() < world) { if (sh->failed.load()) return 1; usleep(50); }
        for (int r = 0; r < world; ++r) counts[(size_t)r] = sh->counts[r].load();
    }
    uint64_t cap = 0;
    if (o.cap > 0) cap = (uint64_t)o.cap;
    else if (o.cap < 0) { const uint32_t mx = R * R * 6u * std::max<uint32_t>(1u, n_meshes); cap = std::min<uint32_t>(mx, 7000000u); }   // ConversionPass.cpp:21-24
    m2s_dist_clamp_to_cap(counts.data(), world, cap, keep.data());
    offs[0] = 0;
    for (int r = 0; r < world; ++r) offs[(size_t)r + 1] = offs[(size_t)r] + keep[(size_t)r];
    const auto t3 = Clock::now();
    uint64_t all = 0;
    for (int r = 0; r < world; ++r) all += counts[(size_t)r];
    if (!o.gather) {
        if (m2s_export_ply_slice(ctx, o.out.c_str(), (uint32_t)o.format, (float)o.std_dev, offs[(size_t)rank], keep[(size_t)rank], offs[(size_t)world]) != M2S_OK)
            return fail("export_slice", m2s_last_error(ctx));
    } else {
        // north-star variant: one RCCL exchange concatenates the blocks on rank 0, which then writes the whole file
        m2s_ctx* sink = nullptr;
        void* merged = nullptr;
        if (rank == 0) {
            if (m2s_create(device, &sink) != M2S_OK) return fail("create", m2s_last_error(nullptr));
            if (m2s_reserve_records(sink, offs[(size_t)world], &merged) != M2S_OK) return fail("reserve", m2s_last_error(sink));
        }
        if (!rendezvous(3)) return 1;                 // rank 0 has its receive buffer
        if (m2s_dist_gather_records(d, m2s_device_records(ctx), keep.data(), merged, 0, nullptr) != M2S_OK) return fail("gather_records", m2s_dist_last_error(d));
        if (m2s_dist_wait(d, nullptr) != M2S_OK) return fail("gather_records", m2s_dist_last_error(d));   // sends / receives have completed
        if (rank == 0) {
            if (m2s_set_records(sink, merged, offs[(size_t)world], R) != M2S_OK) return fail("set_records", m2s_last_error(sink));
            if (m2s_export_ply(sink, o.out.c_str(), (uint32_t)o.format, (float)o.std_dev) != M2S_OK) return fail("export", m2s_last_error(sink));
            m2s_destroy(sink);
        }
    }
    const auto t4 = Clock::now();
    if (rank == 0)
        std::printf("%s: %u mesh(es), density %u, %d GPUs -> %llu Gaussians (%llu stored) -> %s (format %ld, %s)\n", o.in.c_str(), n_meshes, R, world,
                    (unsigned long long)all, (unsigned long long)offs[(size_t)world], o.out.c_str(), o.format,
                    o.gather ? (o.threads ? "gathered on rank 0, in-process transport" : "gathered on rank 0 over RCCL") : "every rank wrote its rows");
    if (o.timing)
        std::printf("[rank %d] triangles [%llu, +%llu) -> %llu Gaussians | init (HIP%s) %.2f ms | upload %.2f ms | convert + counter exchange %.3f ms | export %.2f ms\n",
                    rank, (unsigned long long)first[(size_t)rank], (unsigned long long)count[(size_t)rank], (unsigned long long)total, o.gather ? " + RCCL" : "", ms_between(t0, t1),
                    ms_between(t1, t2), ms_between(t2, t3), ms_between(t3, t4));
    if (d) m2s_dist_destroy(d);
    m2s_destroy(ctx);
    return 0;
}

template <class F>
int fork_ranks(int world, F body) {
    std::fflush(stdout); std::fflush(stderr);
    std::vector<pid_t> pids;
    for (int r = 0; r < world; ++r) {
        const pid_t p = fork();
        if (p < 0) { std::perror("fork"); return 1; }
        if (p == 0) { const int rc = body(r); std::fflush(stdout); std::fflush(stderr); _exit(rc); }
        pids.push_back(p);
    }
    // a rank that dies (a signal, an abort inside a library) cannot tell the others: when one exits abnormally or non-zero the
    // parent gives the rest two seconds to notice `failed` by themselves and then ends them, so that nobody waits for ever
    int rc = 0;
    size_t left = pids.size();
    std::vector<char> done(pids.size(), 0);
    int grace_polls = -1;
    while (left) {
        bool progressed = false;
        for (size_t i = 0; i < pids.size(); ++i) {
            if (done[i]) continue;
            int st = 0;
            const pid_t w = waitpid(pids[i], &st, WNOHANG);
            if (w == 0) continue;
            done[i] = 1; --left; progressed = true;
            if (w < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) { rc = 1; if (grace_polls < 0) grace_polls = 2000; }
        }
        if (!left) break;
        if (grace_polls == 0) { for (size_t i = 0; i < pids.size(); ++i) if (!done[i]) kill(pids[i], SIGKILL); grace_polls = -2; }
        else if (grace_polls > 0) --grace_polls;
        if (!progressed) usleep(1000);
    }
    return rc;
}

int convert_sharded(const Options& o) {
    // NO HIP call in this process before the fork (a forked HIP runtime is unusable): the load is CPU-only
    m2s_host_scene* scene = nullptr;
    if (m2s_load_glb(o.in.c_str(), &scene) != M2S_OK) { std::fprintf(stderr, "%s\n", m2s_io_last_error()); return 1; }
    if (*m2s_host_scene_warnings(scene)) std::fprintf(stderr, "%s", m2s_host_scene_warnings(scene));
    Shared* sh = (Shared*)mmap(nullptr, sizeof(Shared), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (sh == MAP_FAILED) { std::perror("mmap"); return 1; }
    new (sh) Shared();
    sh->id_ready.store(0); sh->failed.store(0); sh->arrived.store(0);
    for (auto& st : sh->stage) st.store(0);
    std::remove(o.out.c_str());
    const int world = (int)o.gpus;
    int rc = 0;
    if (o.threads) {
        if (o.gather) {
            if (m2s_dist_local_id(world, sh->id) != M2S_OK) { std::fprintf(stderr, "local_id: %s\n", m2s_dist_last_error(nullptr)); return 1; }
            sh->id_ready.store(1);
        }
        std::vector<int> rcs((size_t)world, 1);
        std::vector<std::thread> ranks;
        for (int r = 0; r < world; ++r) ranks.emplace_back([&, r] { rcs[(size_t)r] = rank_main(o, scene, sh, r, world); });
        for (auto& t : ranks) t.join();
        for (int r = 0; r < world; ++r) rc |= rcs[(size_t)r];
    } else
        rc = fork_ranks(world, [&](int r) { return rank_main(o, scene, sh, r, world); });
    munmap(sh, sizeof(Shared));
    m2s_free_host_scene(scene);
    return rc;
}

// ---- batch -----------------------------------------------------------------------------------------------------------
template <class T>
class Channel {   // bounded blocking queue; close() ends the stream
public:
    explicit Channel(size_t cap) : cap_(cap) {}
    void push(T v) { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return q_.size() < cap_; }); q_.push_back(std::move(v)); cv_.notify_all(); }
    bool pop(T& v) { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return !q_.empty() || closed_; }); if (q_.empty()) return false; v = std::move(q_.front()); q_.pop_front(); cv_.notify_all(); return true; }
    void close() { std::lock_guard<std::mutex> l(m_); closed_ = true; cv_.notify_all(); }
private:
    std::mutex m_; std::condition_variable cv_; std::deque<T> q_; size_t cap_; bool closed_ = false;
};

struct Loaded { std::string in, out; m2s_host_scene* scene = nullptr; double load_ms = 0; };
struct Converted { std::string in, out; int slot = 0; uint64_t total = 0; double load_ms = 0, upload_ms = 0, convert_ms = 0, budget_ms = -1, merge_ms = -1, refit_ms = -1;   // budget_ms / merge_ms / refit_ms < 0: no --budget / --merge-* / --refit
                   double ctr[3] = {}, dist = 0, near_p = 0, far_p = 0; };   // the camera rule of its scene (--lod-*: the scene is gone by then)

int batch_on_device(const Options& o, const std::vector<std::pair<std::string, std::string>>& files, int device, int tag) {
    const auto t_begin = Clock::now();
    m2s_ctx* ctx[2] = { nullptr, nullptr };
    for (auto& c : ctx)
        if (m2s_create(device, &c) != M2S_OK) { std::fprintf(stderr, "%s\n", m2s_last_error(nullptr)); return 1; }
    for (auto c : ctx) { (void)m2s_set_pipeline(c, o.pipeline); (void)m2s_set_max_gaussians(c, o.conversion_cap()); (void)apply_merge_model(c, o); }
    Channel<Loaded> loaded(2);
    Channel<Converted> converted(1);
    std::mutex slot_m; std::condition_variable slot_cv; bool slot_busy[2] = { false, false };   // a context's records are being exported
    std::atomic<int> failures{ 0 };
    std::thread loader([&] {
        for (const auto& f : files) {
            Loaded l; l.in = f.first; l.out = f.second;
            const auto a = Clock::now();
            if (m2s_load_glb(l.in.c_str(), &l.scene) != M2S_OK) { std::fprintf(stderr, "%s: %s\n", l.in.c_str(), m2s_io_last_error()); ++failures; continue; }
            l.load_ms = ms_between(a, Clock::now());
            loaded.push(std::move(l));
        }
        loaded.close();
    });
    std::thread exporter([&] {
        Converted c;
        while (converted.pop(c)) {
            const auto a = Clock::now();
            if (o.compact ? export_compact(ctx[c.slot], c.out, o, false) != 0
                          : m2s_export_ply(ctx[c.slot], c.out.c_str(), (uint32_t)o.format, (float)o.std_dev) != M2S_OK) {
                std::fprintf(stderr, "%s: export: %s\n", c.in.c_str(), m2s_last_error(ctx[c.slot])); ++failures;
            }
            const double ex = ms_between(a, Clock::now());
            if (o.lod()) {
                // the tree over the exported records, and a dry-run cut per --score camera (a batch draws no frames)
                LodReport rep;
                bool ok = lod_build(ctx[c.slot], o, &rep) == 0;
                for (int v = 0; ok && v < o.score_views; ++v) {
                    const double th = 2.0 * M_PI * v / o.score_views, el = o.score_elevation * (M_PI / 180.0), dist = c.dist * o.view_distance;
                    const double eye[3] = { c.ctr[0] + dist * std::cos(el) * std::sin(th), c.ctr[1] + dist * std::sin(el), c.ctr[2] + dist * std::cos(el) * std::cos(th) };
                    float view[16], proj[16];
                    camera_matrices(eye, c.ctr, c.near_p, c.far_p * o.view_distance, o.preview_w, o.preview_h, view, proj);
                    ok = lod_cut(ctx[c.slot], o, eye, view, proj, o.preview_h, c.near_p, true, &rep) == 0;
                }
                if (ok) lod_print(o, rep);
                else { std::fprintf(stderr, "%s: lod: %s\n", c.in.c_str(), m2s_last_error(ctx[c.slot])); ++failures; }
            }
            char budget[48] = "";
            if (c.budget_ms >= 0) std::snprintf(budget, sizeof(budget), ", budget %.2f ms", c.budget_ms);
            char merge[48] = "";
            if (c.merge_ms >= 0) std::snprintf(merge, sizeof(merge), ", merge %.2f ms", c.merge_ms);
            char refit[48] = "";
            if (c.refit_ms >= 0) std::snprintf(refit, sizeof(refit), ", refit %.2f ms", c.refit_ms);
            std::printf("[gpu %d] %s -> %s: %llu Gaussians | load %.1f ms, upload %.1f ms, convert %.2f ms%s%s%s, export %.1f ms\n", tag, c.in.c_str(), c.out.c_str(),
                        (unsigned long long)c.total, c.load_ms, c.upload_ms, c.convert_ms, budget, merge, refit, ex);
            { std::lock_guard<std::mutex> l(slot_m); slot_busy[c.slot] = false; }
            slot_cv.notify_all();
        }
    });
    Loaded l;
    int k = 0, done = 0;
    while (loaded.pop(l)) {
        const int slot = k++ & 1;
        { std::unique_lock<std::mutex> lk(slot_m); slot_cv.wait(lk, [&] { return !slot_busy[slot]; }); slot_busy[slot] = true; }
        Converted c; c.in = l.in; c.out = l.out; c.slot = slot; c.load_ms = l.load_ms;
        auto a = Clock::now();
        (void)m2s_set_resolution_hint(ctx[slot], o.R());
        bool ok = m2s_upload_scene(ctx[slot], m2s_host_scene_meshes(l.scene), m2s_host_scene_num_meshes(l.scene)) == M2S_OK;
        c.upload_ms = ms_between(a, Clock::now());
        a = Clock::now();
        ok = ok && m2s_convert(ctx[slot], o.R(), &c.total) == M2S_OK;
        c.convert_ms = ms_between(a, Clock::now());
        if (ok && o.world_units) ok = run_world_units(ctx[slot]) == 0;                              // (its lines come in file order)
        if (ok && o.budget > 0) {                                                                   // (its lines come in file order)
            a = Clock::now();
            ok = run_budget(ctx[slot], M2S_IMPORTANCE_AREA, 0.0f, 0, o) == 0;
            c.budget_ms = ms_between(a, Clock::now());
        }
        if (ok && o.merging()) {
            a = Clock::now();
            ok = run_merge(ctx[slot], o) == 0;
            c.merge_ms = ms_between(a, Clock::now());
        }
        if (ok && o.refit_views > 0) {
            a = Clock::now();
            ok = run_refit(ctx[slot], m2s_host_scene_meshes(l.scene), m2s_host_scene_num_meshes(l.scene), o.R(), o) == 0;
            c.refit_ms = ms_between(a, Clock::now());
        }
        if (o.lod()) preview_rule(m2s_host_scene_meshes(l.scene), m2s_host_scene_num_meshes(l.scene), c.ctr, &c.dist, &c.near_p, &c.far_p);
        m2s_free_host_scene(l.scene);
        if (!ok) {
            std::fprintf(stderr, "%s: %s\n", l.in.c_str(), m2s_last_error(ctx[slot])); ++failures;
            { std::lock_guard<std::mutex> lk(slot_m); slot_busy[slot] = false; }
            slot_cv.notify_all();
            continue;
        }
        converted.push(std::move(c));
        ++done;
    }
    converted.close();
    loader.join();
    exporter.join();
    const double total_s = ms_between(t_begin, Clock::now()) * 1e-3;
    std::printf("[gpu %d] %d file(s) in %.3f s = %.2f meshes/s (load | upload + convert | export overlapped)\n", tag, done, total_s, done / std::max(total_s, 1e-9));
    for (auto c : ctx) m2s_destroy(c);
    return failures.load() ? 1 : 0;
}

int convert_batch(const Options& o) {
    std::vector<std::pair<std::string, std::string>> files;
    DIR* dir = opendir(o.batch_dir.c_str());
    if (!dir) { std::perror(o.batch_dir.c_str()); return 1; }
    while (dirent* e = readdir(dir)) {
        const std::string n = e->d_name;
        if (n.size() > 4 && n.compare(n.size() - 4, 4, ".glb") == 0)
            files.emplace_back(o.batch_dir + "/" + n, o.out_dir + "/" + n.substr(0, n.size() - 4) + ".ply");
    }
    closedir(dir);
    std::sort(files.begin(), files.end());
    if (files.empty()) { std::fprintf(stderr, "no .glb files in %s\n", o.batch_dir.c_str()); return 1; }
    if (o.gpus <= 1) return batch_on_device(o, files, (int)o.device, (int)o.device);
    // one process per GPU, file k on GPU k mod N: independent replicas (fork before any HIP call)
    const int world = (int)o.gpus;
    return fork_ranks(world, [&](int r) {
        std::vector<std::pair<std::string, std::string>> mine;
        for (size_t k = (size_t)r; k < files.size(); k += (size_t)world) mine.push_back(files[k]);
        return mine.empty() ? 0 : batch_on_device(o, mine, (int)o.device + r, (int)o.device + r);
    });
}

}  // namespace

int main(int argc, char** argv) {
    // --gpus N: one process per GPU over RCCL.  The host driver only supports dmabuf IPC; say so before any HIP runtime call of this
    // process or its forks (without it RCCL's bring-up fails with `hipIpcGetMemHandle: invalid argument`).  Never overrides the caller's value.
    setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);
    Options o;
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        if (a == "--density" || a == "--quality" || a == "--max-res" || a == "--std" || a == "--cap" || a == "--pipeline") o.conversion_flag = true;
        if (a == "--density") o.density = std::atol(next());
        else if (a == "--quality") o.quality = std::atof(next());
        else if (a == "--max-res") o.max_res = std::atol(next());
        else if (a == "--std") o.std_dev = std::atof(next());
        else if (a == "--format") o.format = std::atol(next());
        else if (a == "--device") o.device = std::atol(next());
        else if (a == "--cap") { o.cap = std::atol(next()); o.cap_set = true; }
        else if (a == "--budget") { o.budget = std::atoll(next()); if (o.budget < 1) { usage(); return 2; } }
        else if (a == "--gpus") o.gpus = std::atol(next());
        else if (a == "--gather") o.gather = true;
        else if (a == "--force-sharded") o.force_sharded = true;
        else if (a == "--one-device") o.one_device = true;
        else if (a == "--threads") o.threads = true;
        else if (a == "--batch") o.batch_dir = next();
        else if (a == "--out") o.out_dir = next();
        else if (a == "--pipeline") o.pipeline = std::string(next()) == "multipass" ? M2S_PIPELINE_MULTIPASS : M2S_PIPELINE_AUTO;
        else if (a == "--timing") o.timing = true;
        else if (a == "--preview") o.preview = next();
        else if (a == "--mesh-depth-test") o.mesh_depth_test = true;
        else if (a == "--split-screen") { o.split_screen = std::atof(next()); if (!(o.split_screen >= 0.0 && o.split_screen <= 1.0)) { usage(); return 2; } }
        else if (a == "--preview-mode") { o.preview_mode = std::atoi(next()); o.preview_mode_set = true; if (o.preview_mode < 0 || o.preview_mode > 6) { usage(); return 2; } }
        else if (a == "--score") { o.score_views = std::atoi(next()); if (o.score_views < 1 || o.score_views > 4096) { usage(); return 2; } }
        else if (a == "--merge-level") { o.merge_level = std::atoi(next()); if (o.merge_level < 0 || o.merge_level > 10) { usage(); return 2; } }
        else if (a == "--merge-to") { o.merge_to = std::atoll(next()); if (o.merge_to < 1) { usage(); return 2; } }
        else if (a == "--merge-group") { o.merge_group = std::atoi(next()); if (o.merge_group < 2 || o.merge_group > 64) { usage(); return 2; } }
        else if (a == "--merge-dot") { o.merge_dot = std::atof(next()); if (std::isnan(o.merge_dot)) { usage(); return 2; } }
        else if (a == "--lod-pixels") { o.lod_pixels = std::atof(next()); if (!(o.lod_pixels >= 0.0) || !std::isfinite(o.lod_pixels)) { usage(); return 2; } }
        else if (a == "--lod-frustum") o.lod_frustum = true;
        else if (a == "--lod-occlusion") o.lod_occlusion = true;
        else if (a == "--lod-depth-bias") { o.lod_depth_bias = std::atof(next()); if (!(o.lod_depth_bias >= 0.0) || !std::isfinite(o.lod_depth_bias)) { usage(); return 2; } }
        else if (a == "--lod-ply") o.lod_ply = next();
        else if (a == "--lod-blend") { o.lod_blend = std::atof(next()); if (!(o.lod_blend > 0.0) || !(o.lod_blend <= 1.0) || !((float)o.lod_blend > 0.0f)) { usage(); return 2; } }
        else if (a == "--lod-guard") { o.lod_guard = std::atof(next()); if (!(o.lod_guard >= 1.0) || !std::isfinite(o.lod_guard)) { usage(); return 2; } }
        else if (a == "--lod-budget") {
            const std::string v = next();
            char* end = nullptr;
            o.lod_budget = std::strtoll(v.c_str(), &end, 10);
            if (v.empty() || *end || o.lod_budget < 1 || o.lod_budget > 0xFFFFFFFFll) { usage(); return 2; }
        }
        else if (a == "--view-distance") { o.view_distance = std::atof(next()); if (!(o.view_distance >= 0.25 && o.view_distance <= 64.0)) { usage(); return 2; } }
        else if (a == "--lod-levels") {
            o.lod_levels.clear();
            const std::string v = next();
            size_t at = 0;
            while (at <= v.size()) {
                const size_t c = std::min(v.find(',', at), v.size());
                char* end = nullptr;
                const std::string tok = v.substr(at, c - at);
                const long lv = std::strtol(tok.c_str(), &end, 10);
                if (tok.empty() || *end || lv < 0 || lv > 10 || (!o.lod_levels.empty() && (uint32_t)lv < o.lod_levels.back())) { usage(); return 2; }
                o.lod_levels.push_back((uint32_t)lv);
                at = c + 1;
            }
            if (o.lod_levels.size() > M2S_LOD_MAX_STEPS) { usage(); return 2; }
        }
        else if (a == "--prune") { o.prune_views = std::atoi(next()); if (o.prune_views < 1 || o.prune_views > 4096) { usage(); return 2; } }
        else if (a == "--refit") { o.refit_views = std::atoi(next()); if (o.refit_views < 1 || o.refit_views > 4096) { usage(); return 2; } }
        else if (a == "--refit-iters") { o.refit_iters = std::atoi(next()); if (o.refit_iters < 1 || o.refit_iters > 64) { usage(); return 2; } }
        else if (a == "--refit-step") { o.refit_step = std::atof(next()); if (!std::isfinite(o.refit_step)) { usage(); return 2; } }
        else if (a == "--prune-elevations" || a == "--refit-elevations") {
            std::vector<double>& list = a == "--prune-elevations" ? o.prune_elevations : o.refit_elevations;
            list.clear();
            std::string v = next();
            size_t at = 0;
            while (at <= v.size()) {
                const size_t c = std::min(v.find(',', at), v.size());
                char* end = nullptr;
                const std::string tok = v.substr(at, c - at);
                const double e = std::strtod(tok.c_str(), &end);
                if (tok.empty() || *end || !(e > -90.0 && e < 90.0)) { usage(); return 2; }
                list.push_back(e);
                at = c + 1;
            }
            if (list.empty() || list.size() > 64) { usage(); return 2; }
        }
        else if (a == "--prune-weight") { o.prune_weight = std::atof(next()); if (!(o.prune_weight >= 0.0 && o.prune_weight <= 1.0)) { usage(); return 2; } }
        else if (a == "--prune-pixels") { o.prune_pixels = std::atol(next()); if (o.prune_pixels < 0 || o.prune_pixels > 0x7FFFFFFFl) { usage(); return 2; } }
        else if (a == "--prune-count-weight") { o.prune_count_weight = std::atof(next()); if (!(o.prune_count_weight >= 0.0 && o.prune_count_weight <= 1.0)) { usage(); return 2; } }
        else if (a == "--score-elevation") { o.score_elevation = std::atof(next()); if (!(o.score_elevation > -90.0 && o.score_elevation < 90.0)) { usage(); return 2; } }
        else if (a == "--score-mask") { o.score_mask = std::atoi(next()); if (o.score_mask < 0 || o.score_mask > 3) { usage(); return 2; } }
        else if (a == "--score-map") o.score_map = next();
        else if (a == "--bake-light") o.bake_light = true;
        else if (a == "--compact") o.compact = true;
        else if (a == "--world-units") o.world_units = true;
        else if (a == "--merge-unsigned-axis") o.merge_unsigned_axis = true;
        else if (a == "--merge-model") {
            const std::string v = next();
            o.merge_model = v == "footprint" ? (int)M2S_MERGE_MODEL_FOOTPRINT : v == "gaussian" ? (int)M2S_MERGE_MODEL_GAUSSIAN : -1;
            if (o.merge_model < 0) { usage(); return 2; }
        }
        else if (a == "--merge-sigma") { o.merge_sigma = std::atof(next()); if (!(o.merge_sigma > 0.0) || !std::isfinite(o.merge_sigma) || !((float)o.merge_sigma > 0.0f) || !std::isfinite((float)o.merge_sigma)) { usage(); return 2; } }
        else if (a == "--bake-degree") { o.bake_degree = std::atoi(next()); if (o.bake_degree < 0 || o.bake_degree > 3) { usage(); return 2; } }
        else if (a == "--light") {
            const int got = std::sscanf(next(), "%lf,%lf,%lf,%lf", &o.light[0], &o.light[1], &o.light[2], &o.light[3]);
            if (got < 3) { usage(); return 2; }
            o.has_light = true;
        }
        else if (a == "--preview-size") {
            if (std::sscanf(next(), "%dx%d", &o.preview_w, &o.preview_h) != 2 || o.preview_w < 1 || o.preview_h < 1 || o.preview_w > 8192 ||
                o.preview_h > 8192) { usage(); return 2; }
        }
        else if (!a.empty() && a[0] == '-') { usage(); return 2; }
        else pos.push_back(a);
    }
    if (o.gpus < 1 || o.gpus > 64) { usage(); return 2; }
    // --bake-light writes the standard layout only, from the one context that holds the records, the cube and the plane
    if (o.prune_views > 0 && (o.gpus > 1 || o.force_sharded || !o.batch_dir.empty())) { usage(); return 2; }   // (multi-rank pruning: out of scope)
    if (o.budget > 0 && (o.gpus > 1 || o.force_sharded)) { usage(); return 2; }   // (multi-rank budgets: out of scope)
    if (o.merging() && (o.gpus > 1 || o.force_sharded || (o.merge_level >= 0 && o.merge_to > 0))) { usage(); return 2; }   // (multi-rank merges: out of scope)
    if (o.merge_unsigned_axis && !o.merging() && !o.lod()) { usage(); return 2; }   // (a mode of those passes, refused with --gpus N > 1 as they are)
    if ((o.merge_model >= 0 && !o.merging() && !o.lod()) || (o.merge_sigma > 0.0 && o.merge_model < 0)) { usage(); return 2; }   // (--merge-model: a mode of those passes; --merge-sigma: of --merge-model)
    if (o.merge_model == M2S_MERGE_MODEL_GAUSSIAN && o.lod_blend > 0.0) { usage(); return 2; }   // (m2s_lod_blend refuses a tree built under the Gaussian model)
    if (o.refit_views > 0 && (o.gpus > 1 || o.force_sharded)) { usage(); return 2; }   // (the refit reads one context's records and scene)
    if (o.world_units && (o.gpus > 1 || o.force_sharded)) { usage(); return 2; }   // (a rank's slice writer and the gather hand on the density)
    if (o.compact && (o.gpus > 1 || o.force_sharded)) { usage(); return 2; }   // (the Morton order is global: no slice writers)
    // --lod-*: the levels with a bound in pixels, a budget or both, or none of them; the cuts need cameras (--preview / --score; a batch
    // draws no preview) and one context
    if (o.lod() != (o.lod_pixels >= 0.0 || o.lod_budget > 0)) { usage(); return 2; }
    // (--lod-occlusion: a mode of the frustum cuts; --lod-depth-bias: of --lod-occlusion; not beside the prepass's own depth test, which
    //  would cull a merged node by its own position under the surface; the mesh depth image is one context's)
    if ((o.lod_occlusion && (!o.lod() || o.mesh_depth_test || o.gpus > 1)) || (o.lod_depth_bias >= 0.0 && !o.lod_occlusion)) { usage(); return 2; }
    if (o.lod_occlusion) { o.lod_frustum = true; if (o.lod_depth_bias < 0.0) o.lod_depth_bias = 0.00002; }
    if ((o.lod_frustum && !o.lod()) || (o.lod_guard >= 0.0 && !o.lod_frustum)) { usage(); return 2; }   // (--lod-frustum: a mode of the cuts; --lod-guard: of --lod-frustum)
    if (o.lod_frustum && o.lod_guard < 0.0) o.lod_guard = 1.05;
    if (o.lod_blend > 0.0 && (!o.lod() || o.gpus > 1)) { usage(); return 2; }                          // (--lod-blend: a mode of the cuts)
    if (o.lod() && (o.gpus > 1 || o.force_sharded || (o.score_views == 0 && (o.preview.empty() || !o.batch_dir.empty())))) { usage(); return 2; }
    if (!o.lod_ply.empty() && (!o.lod() || o.preview.empty() || !o.batch_dir.empty() || o.gpus > 1 || o.force_sharded)) { usage(); return 2; }
    if (o.bake_light && (o.format != 0 || o.gpus > 1 || o.force_sharded || !o.batch_dir.empty())) { usage(); return 2; }
    if (!o.batch_dir.empty()) {
        if (o.out_dir.empty() || !pos.empty()) { usage(); return 2; }
        return convert_batch(o);
    }
    if (pos.size() != 2) { usage(); return 2; }
    o.in = pos[0]; o.out = pos[1];
    if (o.in.size() > 4 && o.in.compare(o.in.size() - 4, 4, ".ply") == 0) {
        // a .ply has no mesh and no camera rule: everything that needs one, or a conversion, is a usage error
        if (!o.preview.empty() || o.score_views > 0 || o.refit_views > 0 || o.prune_views > 0 || o.bake_light || o.split_screen >= 0.0 || o.mesh_depth_test ||
            o.lod() || o.lod_pixels >= 0.0 || o.lod_budget > 0 || o.lod_frustum || o.lod_occlusion || o.lod_blend > 0.0 || !o.lod_ply.empty() || o.world_units ||
            o.conversion_flag || o.gpus > 1 || o.force_sharded) { usage(); return 2; }
        return convert_ply(o);
    }
    return (o.gpus > 1 || o.force_sharded) ? convert_sharded(o) : convert_one(o);
}
