"""Parameters of the mesh depth prepass (`Converter.mesh_depth`, m2s_mesh_depth): DepthPrepass::execute (DepthPrepass.cpp:8-50), named
after the RenderContext members it reads (viewMat, projMat, modelMat, rendererResolution)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from .prepass import PrepassParams, _eye

COUNT_NAMES = ("drawn", "clipped", "non_finite", "pairs", "texel_updates")


@dataclass
class MeshDepthParams:
    """Matrices are 4x4 float32 arrays in glm's memory order (m[c] is column c), as in PrepassParams."""
    view_mat: np.ndarray = field(default_factory=_eye)
    proj_mat: np.ndarray = field(default_factory=_eye)
    model_mat: np.ndarray = field(default_factory=_eye)
    renderer_resolution: tuple = (1280, 720)

    @classmethod
    def from_prepass(cls, p: PrepassParams) -> "MeshDepthParams":
        """The camera, model matrix and window of the frame `p` describes."""
        return cls(p.view_mat, p.proj_mat, p.model_mat, tuple(int(v) for v in p.renderer_resolution))


class MeshDepthParamsC(C.Structure):
    """== m2s_mesh_depth_params (include/m2s.h)."""
    _fields_ = [("world_to_view", C.c_float * 16), ("view_to_clip", C.c_float * 16), ("model_to_world", C.c_float * 16),
                ("resolution", C.c_int32 * 2), ("reserved", C.c_uint32 * 2)]


def to_c(p) -> MeshDepthParamsC:
    if isinstance(p, PrepassParams):
        p = MeshDepthParams.from_prepass(p)
    c = MeshDepthParamsC()
    for name, m in (("world_to_view", p.view_mat), ("view_to_clip", p.proj_mat), ("model_to_world", p.model_mat)):
        getattr(c, name)[:] = np.ascontiguousarray(m, np.float32).reshape(16).tolist()
    c.resolution[:] = [int(p.renderer_resolution[0]), int(p.renderer_resolution[1])]
    c.reserved[:] = [0, 0]
    return c
