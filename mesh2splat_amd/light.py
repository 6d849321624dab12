"""Parameters of the shadow and relighting passes (`Converter.shadow`, `Converter.relight`, m2s_shadow / m2s_relight):
GaussianShadowPass::execute (GaussianShadowPass.cpp:83-236) and GaussianRelightingPass::execute (GaussianRelightingPass.cpp:136-143),
named after the RenderContext members they read (RenderContext::pointLightData, nearPlane, farPlane, renderMode, rendererResolution)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

FACES = ("+X", "-X", "+Y", "-Y", "+Z", "-Z")      # GL order of the cube's faces
SHADOW_CUBEMAP_SIZE = 1024                        # GaussianShadowPass.cpp:14


@dataclass
class LightParams:
    light_position: tuple = (0.0, 2.0, 2.0)       # pointLightModel[3].xyz
    light_color: tuple = (1.0, 1.0, 1.0)
    light_intensity: float = 10.0
    camera_position: tuple = (0.0, 0.0, 3.0)      # u_camPos
    near_plane: float = 0.01
    far_plane: float = 100.0
    render_mode: int = 6                          # 5 metallic-roughness view, 6 lit, any other: albedo
    renderer_resolution: tuple = (1280, 720)      # the W x H of the G-buffer relight() lights
    shadow_resolution: int = SHADOW_CUBEMAP_SIZE  # side of a cube face, 1..4096
    want_shadow_counts: bool = False              # relight(), mode 6: keep the per-pixel count of shadowed PCF taps


class LightParamsC(C.Structure):
    """== m2s_light_params (include/m2s.h)."""
    _fields_ = [("light_position", C.c_float * 3), ("light_color", C.c_float * 3), ("light_intensity", C.c_float),
                ("camera_position", C.c_float * 3), ("near_far", C.c_float * 2), ("render_mode", C.c_int32),
                ("resolution", C.c_int32 * 2), ("shadow_resolution", C.c_uint32), ("want_shadow_counts", C.c_uint32),
                ("reserved", C.c_uint32)]


def to_c(p: LightParams) -> LightParamsC:
    c = LightParamsC()
    c.light_position[:] = [float(np.float32(v)) for v in p.light_position]
    c.light_color[:] = [float(np.float32(v)) for v in p.light_color]
    c.light_intensity = float(np.float32(p.light_intensity))
    c.camera_position[:] = [float(np.float32(v)) for v in p.camera_position]
    c.near_far[:] = [float(np.float32(p.near_plane)), float(np.float32(p.far_plane))]
    c.render_mode = int(p.render_mode)
    c.resolution[:] = [int(p.renderer_resolution[0]), int(p.renderer_resolution[1])]
    c.shadow_resolution = int(p.shadow_resolution)
    c.want_shadow_counts = 1 if p.want_shadow_counts else 0
    c.reserved = 0
    return c
