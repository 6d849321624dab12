"""Parameters and result of the splat pass (`Converter.splat`, m2s_splat): GaussianSplattingPass::execute
(GaussianSplattingPass.cpp:50-95) over the sorted quads into the five-target G-buffer of renderer.cpp:325-380."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

# attachments in GL order: (name, dtype) — 0, 1, 3 RGBA16F, 2, 4 RGBA8 unorm
ATTACHMENTS = (("position", np.float16), ("normal", np.float16), ("albedo", np.uint8), ("depth", np.float16),
               ("metallic_roughness", np.uint8))


@dataclass
class SplatParams:
    renderer_resolution: tuple = (1280, 720)   # RenderContext::rendererResolution == u_resolution == viewport (W, H)
    render_mode: int = 0                       # RenderContext::renderMode (u_renderMode): 4 = overdraw


class SplatParamsC(C.Structure):
    """== m2s_splat_params (include/m2s.h)."""
    _fields_ = [("resolution", C.c_int32 * 2), ("render_mode", C.c_int32), ("reserved", C.c_uint32)]


def to_c(p: SplatParams) -> SplatParamsC:
    c = SplatParamsC()
    c.resolution[:] = [int(p.renderer_resolution[0]), int(p.renderer_resolution[1])]
    c.render_mode = int(p.render_mode)
    c.reserved = 0
    return c
