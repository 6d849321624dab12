"""The level-of-detail tree and its per-camera cut (`Converter.lod_build` / `.lod_select` / `.lod_select_budget` / `.lod_levels` /
`.download_lod` / `.download_lod_nodes` / `.lod_release`, m2s_lod_build, m2s_lod_select, m2s_lod_select_budget and the _frustum and
_occluded forms of the two cuts, and m2s_lod_blend behind them: `Converter.lod_blend`): the ctypes mirrors of their parameters and the two numbers a cut takes from a camera.  The pins are in include/m2s.h.

The default chain of merge levels (1 .. 8), like max_group = 4 and min_axis_dot = 0.5, is a guess: nothing in the repository has
tuned it (tools/lod_probe.py reports what it does on one scene)."""
from __future__ import annotations

import ctypes as C

import numpy as np

MAX_STEPS = 16                                               # M2S_LOD_MAX_STEPS
NO_PARENT = 0xFFFFFFFF                                       # M2S_LOD_NO_PARENT
DRY_RUN = 1                                                  # M2S_LOD_DRY_RUN
UNSIGNED_AXIS = 4                                            # M2S_MERGE_UNSIGNED_AXIS: the one value m2s_lod_build_params.flags takes beside 0
DEFAULT_LEVELS = (1, 2, 3, 4, 5, 6, 7, 8)
BUILD_COUNTS = ("leaves", "nodes", "levels", "skipped")      # m2s_lod_build's out_counts, in order
SELECT_COUNTS = ("nodes", "selected", "selected_leaves", "refine")   # m2s_lod_select's
FRUSTUM_COUNTS = ("visible_leaves", "culled")                # m2s_last_lod_frustum_counts', in order
BLEND_COUNTS = ("records", "blended", "saturated", "turned")   # m2s_lod_blend's out_counts, in order
OCCLUSION_COUNTS = ("visible_leaves", "occluded_leaves", "translucent_kept", "culled")   # m2s_last_lod_occlusion_counts', in order
PLANES = {0: (np.float32, 24), 1: (np.uint32, None), 2: (np.float32, 4)}    # m2s_download_lod: which -> (dtype, row length)


class LodBuildParamsC(C.Structure):
    """== m2s_lod_build_params (include/m2s.h).  The last word is the header's `flags`; it keeps the name it had while it was reserved,
    and `flags` reads and writes the same word."""
    _fields_ = [("n_steps", C.c_uint32), ("levels", C.c_uint32 * MAX_STEPS), ("max_group", C.c_uint32), ("min_axis_dot", C.c_float),
                ("reserved", C.c_uint32)]

    @property
    def flags(self) -> int:
        return int(self.reserved)

    @flags.setter
    def flags(self, value: int) -> None:
        self.reserved = int(value)


class LodSelectParamsC(C.Structure):
    """== m2s_lod_select_params (include/m2s.h)."""
    _fields_ = [("camera_position", C.c_float * 3), ("focal_px", C.c_float), ("tau_px", C.c_float), ("near", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class LodBudgetParamsC(C.Structure):
    """== m2s_lod_budget_params (include/m2s.h)."""
    _fields_ = [("camera_position", C.c_float * 3), ("focal_px", C.c_float), ("near", C.c_float), ("tau_min_px", C.c_float),
                ("max_records", C.c_uint32), ("flags", C.c_uint32)]


class LodBudgetResultC(C.Structure):
    """== m2s_lod_budget_result (include/m2s.h)."""
    _fields_ = [("tau_px", C.c_float), ("met", C.c_uint32), ("selected_finer", C.c_uint64)]


class LodFrustumC(C.Structure):
    """== m2s_lod_frustum (include/m2s.h)."""
    _fields_ = [("model_to_world", C.c_float * 16), ("world_to_view", C.c_float * 16), ("view_to_clip", C.c_float * 16),
                ("guard_band", C.c_float), ("reserved", C.c_uint32 * 3)]


class LodOccluderC(C.Structure):
    """== m2s_lod_occluder (include/m2s.h)."""
    _fields_ = [("depth", C.c_void_p), ("depth_w", C.c_uint32), ("depth_h", C.c_uint32), ("depth_on_device", C.c_uint32),
                ("depth_bias", C.c_float), ("reserved", C.c_uint32 * 2)]


class LodBlendParamsC(C.Structure):
    """== m2s_lod_blend_params (include/m2s.h)."""
    _fields_ = [("camera_position", C.c_float * 3), ("focal_px", C.c_float), ("tau_px", C.c_float), ("near", C.c_float),
                ("band", C.c_float), ("reserved", C.c_uint32)]


def blend_to_c(camera_position, focal_px: float, tau_px: float, near: float = 1e-3, band: float = 1.0) -> LodBlendParamsC:
    """The camera, focal and tau_px the cut was taken with (for a budget cut: the tau_px it returned) and the band: the upper share of
    a node's tau^2 interval over which it moves to its parent, 0 < band <= 1."""
    band = float(band)
    if not 0.0 < band <= 1.0:                                # (a NaN too)
        raise ValueError("band outside (0, 1]")
    c = LodBlendParamsC()
    c.camera_position[:] = [float(v) for v in camera_position]
    c.focal_px, c.tau_px, c.near, c.band = float(focal_px), float(tau_px), float(near), band
    return c


def build_to_c(levels=DEFAULT_LEVELS, max_group: int = 4, min_axis_dot: float = 0.5, unsigned_axis: bool = False) -> LodBuildParamsC:
    levels = [int(v) for v in levels]
    if len(levels) > MAX_STEPS:
        raise ValueError(f"at most {MAX_STEPS} steps")
    c = LodBuildParamsC()
    c.n_steps = len(levels)
    c.levels[:len(levels)] = levels
    c.max_group, c.min_axis_dot = int(max_group), float(min_axis_dot)
    c.flags = UNSIGNED_AXIS if unsigned_axis else 0
    return c


def select_to_c(camera_position, focal_px: float, tau_px: float = 1.0, near: float = 1e-3, dry_run: bool = False) -> LodSelectParamsC:
    c = LodSelectParamsC()
    c.camera_position[:] = [float(v) for v in camera_position]
    c.focal_px, c.tau_px, c.near, c.flags = float(focal_px), float(tau_px), float(near), DRY_RUN if dry_run else 0
    return c


def budget_to_c(camera_position, focal_px: float, max_records: int, tau_min_px: float = 0.0, near: float = 1e-3,
                dry_run: bool = False) -> LodBudgetParamsC:
    max_records = int(max_records)
    if not 0 <= max_records <= 0xFFFFFFFF:
        raise ValueError("max_records outside 0..2^32-1")
    c = LodBudgetParamsC()
    c.camera_position[:] = [float(v) for v in camera_position]
    c.focal_px, c.near, c.tau_min_px = float(focal_px), float(near), float(tau_min_px)
    c.max_records, c.flags = max_records, DRY_RUN if dry_run else 0
    return c


def frustum_to_c(model_to_world, world_to_view, view_to_clip, guard_band: float = 1.05) -> LodFrustumC:
    """The three matrices of a PrepassParams (glm's memory order, 16 floats each) and the guard band of the frustum test; 1.05 is the
    prepass's own."""
    c = LodFrustumC()
    for name, m in (("model_to_world", model_to_world), ("world_to_view", world_to_view), ("view_to_clip", view_to_clip)):
        a = np.ascontiguousarray(m, np.float32).reshape(-1)
        if a.size != 16:
            raise ValueError(f"{name}: 16 floats expected")
        getattr(c, name)[:] = a.tolist()
    c.guard_band = float(np.float32(guard_band))
    return c


def occluder_to_c(depth_hw_float32, depth_bias: float = 2e-5) -> LodOccluderC:
    """A host depth image (H, W) float32, window-space depth in [0, 1], row 0 = the bottom row (the layout of PrepassParams' depth
    image), as the occluder of lod_select / lod_select_budget; 2e-5 is the prepass's own bias.  The array is kept alive by the
    returned structure."""
    a = np.ascontiguousarray(depth_hw_float32, np.float32)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("depth image: a non-empty (H, W) array expected")
    c = LodOccluderC()
    c.depth = a.ctypes.data
    c.depth_h, c.depth_w = int(a.shape[0]), int(a.shape[1])
    c.depth_on_device, c.depth_bias = 0, float(np.float32(depth_bias))
    c._keep = a
    return c


def occluder_on_device(pointer: int, depth_w: int, depth_h: int, depth_bias: float = 2e-5) -> LodOccluderC:
    """A depth image that already lies on the context's device (depth_h rows of depth_w floats, row 0 = bottom), not copied."""
    c = LodOccluderC()
    c.depth, c.depth_w, c.depth_h = int(pointer), int(depth_w), int(depth_h)
    c.depth_on_device, c.depth_bias = 1, float(np.float32(depth_bias))
    return c


def occluder_of_mesh_depth(conv=None, depth_bias: float = 2e-5) -> LodOccluderC:
    """The image of the context's last mesh_depth() as occluder: a NULL image, which the library reads as the context's own.  `conv`
    (the Converter the cut will run on) is not read; it documents whose image is meant."""
    c = LodOccluderC()
    c.depth, c.depth_w, c.depth_h = None, 0, 0
    c.depth_on_device, c.depth_bias = 1, float(np.float32(depth_bias))
    return c


def frustum_of(prepass_params, guard_band: float = 1.05) -> LodFrustumC:
    """The frustum of a mesh2splat_amd.prepass.PrepassParams: its model, view and projection matrices."""
    return frustum_to_c(prepass_params.model_mat, prepass_params.view_mat, prepass_params.proj_mat, guard_band)


def focal_px(view_to_clip, H: int) -> float:
    """Pixels per unit of tan(angle) of a perspective projection on a viewport H pixels high: view_to_clip[5] * H / 2 (glm's memory
    order: element [1][1]), in float32."""
    p = np.asarray(view_to_clip, np.float32).reshape(-1)
    return float(np.float32(p[5] * np.float32(H)) / np.float32(2))


def camera_position(world_to_view) -> tuple:
    """The eye of a rigid world-to-view matrix (glm's memory order, m[4 c + r]): -R^T t, in float64, rounded to float32 once."""
    m = np.asarray(world_to_view, np.float64).reshape(-1)
    t = m[12:15]
    return tuple(float(np.float32(-(m[4 * k + 0] * t[0] + m[4 * k + 1] * t[1] + m[4 * k + 2] * t[2]))) for k in range(3))
