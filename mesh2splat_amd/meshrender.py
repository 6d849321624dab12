"""Parameters of the mesh render pass (`Converter.mesh_render`, m2s_mesh_render): MeshRenderPass::execute (MeshRenderPass.cpp:8-73),
named after the RenderContext members it reads (viewMat, projMat, modelMat, rendererResolution, nearPlane / farPlane, renderMode)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from .prepass import PrepassParams, _eye

COUNT_NAMES = ("drawn", "clipped", "non_finite", "pairs", "texel_updates", "culled")
STAGE_NAMES = ("setup", "bin", "raster", "shade")
EMPTY = np.uint64((0x3F800000 << 32) | 0xFFFFFFFF)          # an empty pixel of the visibility image


@dataclass
class MeshRenderParams:
    """Matrices are 4x4 float32 arrays in glm's memory order (m[c] is column c), as in PrepassParams."""
    view_mat: np.ndarray = field(default_factory=_eye)
    proj_mat: np.ndarray = field(default_factory=_eye)
    model_mat: np.ndarray = field(default_factory=_eye)
    renderer_resolution: tuple = (1280, 720)
    near_far: tuple = (0.01, 100.0)
    render_mode: int = 0

    @classmethod
    def from_prepass(cls, p: PrepassParams) -> "MeshRenderParams":
        """The camera, model matrix, window, planes and render mode of the frame `p` describes."""
        return cls(p.view_mat, p.proj_mat, p.model_mat, tuple(int(v) for v in p.renderer_resolution),
                   (float(np.float32(p.near_plane)), float(np.float32(p.far_plane))), int(p.render_mode))


class MeshRenderParamsC(C.Structure):
    """== m2s_mesh_render_params (include/m2s.h)."""
    _fields_ = [("world_to_view", C.c_float * 16), ("view_to_clip", C.c_float * 16), ("model_to_world", C.c_float * 16),
                ("resolution", C.c_int32 * 2), ("near_far", C.c_float * 2), ("render_mode", C.c_int32), ("reserved", C.c_uint32)]


def to_c(p) -> MeshRenderParamsC:
    if isinstance(p, PrepassParams):
        p = MeshRenderParams.from_prepass(p)
    c = MeshRenderParamsC()
    for name, m in (("world_to_view", p.view_mat), ("view_to_clip", p.proj_mat), ("model_to_world", p.model_mat)):
        getattr(c, name)[:] = np.ascontiguousarray(m, np.float32).reshape(16).tolist()
    c.resolution[:] = [int(p.renderer_resolution[0]), int(p.renderer_resolution[1])]
    c.near_far[:] = [float(p.near_far[0]), float(p.near_far[1])]
    c.render_mode = int(p.render_mode)
    c.reserved = 0
    return c
