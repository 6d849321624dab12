"""The fidelity score (`Converter.score_frames`, `Converter.score`, m2s_score_frames): the mesh-lit frame against the splat frame of the
same camera, compared on the device.  The reference has no counterpart: there a person looks at the split screen.  The pin is in
include/m2s.h; the device returns integers only and the ratios (PSNR, mean SSIM, coverage IoU) are derived here in float64."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

NO_COVER, WANT_MAP = 1, 2                 # M2S_SCORE_*
MASK_ALL, MASK_A, MASK_A_OR_B, MASK_A_AND_B = 0, 1, 2, 3


@dataclass
class ScoreParams:
    resolution: tuple = (1280, 720)       # W, H of the four images
    mask_mode: int = MASK_A_OR_B          # 0 every pixel, 1 covered by A (the mesh), 2 by A or B, 3 by A and B
    no_cover: bool = False                # the coverage planes are not read: every pixel counts as covered by both
    want_map: bool = False                # keep the error map on the device


class ScoreParamsC(C.Structure):
    """== m2s_score_params (include/m2s.h)."""
    _fields_ = [("resolution", C.c_int32 * 2), ("mask_mode", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ScoreResultC(C.Structure):
    """== m2s_score_result (include/m2s.h)."""
    _fields_ = [("pixels", C.c_uint64), ("cover", C.c_uint64 * 4), ("sse", C.c_uint64 * 3), ("sad", C.c_uint64 * 3),
                ("max_abs", C.c_uint32 * 3), ("pad", C.c_uint32), ("windows", C.c_uint64), ("ssim_q32", C.c_int64)]


def to_c(p: ScoreParams) -> ScoreParamsC:
    c = ScoreParamsC()
    c.resolution[:] = [int(p.resolution[0]), int(p.resolution[1])]
    c.mask_mode = int(p.mask_mode)
    c.flags = (NO_COVER if p.no_cover else 0) | (WANT_MAP if p.want_map else 0)
    c.reserved[:] = [0, 0]
    return c


@dataclass
class ScoreResult:
    """The integers of m2s_score_result, and the ratios derived from them."""
    pixels: int = 0
    cover: tuple = (0, 0, 0, 0)           # over the whole image: neither, A only, B only, both
    sse: tuple = (0, 0, 0)
    sad: tuple = (0, 0, 0)
    max_abs: tuple = (0, 0, 0)
    windows: int = 0
    ssim_q32: int = 0
    error_map: object = field(default=None, compare=False)   # (H, W, 4) uint8, row 0 = bottom (download_map=True)

    @classmethod
    def from_c(cls, r: ScoreResultC) -> "ScoreResult":
        return cls(int(r.pixels), tuple(int(v) for v in r.cover), tuple(int(v) for v in r.sse), tuple(int(v) for v in r.sad),
                   tuple(int(v) for v in r.max_abs), int(r.windows), int(r.ssim_q32))

    def integers(self) -> dict:
        return {"pixels": self.pixels, "cover": list(self.cover), "sse": list(self.sse), "sad": list(self.sad), "max_abs": list(self.max_abs),
                "windows": self.windows, "ssim_q32": self.ssim_q32}

    @property
    def psnr(self) -> float:
        """10 log10(255^2 * 3 * pixels / (sse_r + sse_g + sse_b)) in dB; inf at zero error, NaN when no pixel passed the mask."""
        if self.pixels == 0:
            return math.nan
        sse = sum(self.sse)
        return math.inf if sse == 0 else 10.0 * math.log10(65025.0 * 3.0 * self.pixels / sse)

    @property
    def ssim(self) -> float:
        """Mean SSIM over the counted windows; NaN when none was counted."""
        return self.ssim_q32 / 4294967296.0 / self.windows if self.windows else math.nan

    @property
    def coverage_iou(self) -> float:
        """both / (A only + B only + both); NaN when neither image covers a pixel."""
        union = self.cover[1] + self.cover[2] + self.cover[3]
        return self.cover[3] / union if union else math.nan


def pool(results: Sequence[ScoreResult]) -> ScoreResult:
    """Several views as one: the integers add (max_abs: the maximum) and the ratios follow from the sums."""
    add = lambda name, n: tuple(sum(getattr(r, name)[i] for r in results) for i in range(n))
    return ScoreResult(sum(r.pixels for r in results), add("cover", 4), add("sse", 3), add("sad", 3),
                       tuple(max([r.max_abs[i] for r in results], default=0) for i in range(3)),
                       sum(r.windows for r in results), sum(r.ssim_q32 for r in results))


# ---- cameras round the scene --------------------------------------------------------------------------------------------------------
@dataclass
class OrbitCamera:
    eye: tuple
    centre: tuple
    near: float
    far: float
    resolution: tuple
    view_mat: np.ndarray                  # glm's memory order (m[c] is column c), float32
    proj_mat: np.ndarray

    def frame_params(self, resolution_target: int, light_position, light_intensity: float, gaussian_std: float = 0.65, render_mode: int = 6,
                     shadow_resolution: int = 1024, light_color=(1.0, 1.0, 1.0)):
        """-> (PrepassParams, LightParams) of the frame this camera sees, as the command line's --score builds them: the prepass and the
        mesh render pass in render mode 0, the relighting pass in `render_mode`."""
        from .light import LightParams
        from .prepass import PrepassParams
        pp = PrepassParams(view_mat=self.view_mat, proj_mat=self.proj_mat, renderer_resolution=tuple(self.resolution), near_plane=self.near,
                           far_plane=self.far, gaussian_std=gaussian_std, resolution_target=int(resolution_target), render_mode=0)
        lp = LightParams(tuple(light_position), tuple(light_color), float(light_intensity), tuple(self.eye), self.near, self.far, int(render_mode),
                         tuple(self.resolution), int(shadow_resolution), False)
        return pp, lp


def _bbox(scene_or_bbox):
    if hasattr(scene_or_bbox, "meshes"):
        ms = scene_or_bbox.meshes
        return [min(float(m.bbox_min[k]) for m in ms) for k in range(3)], [max(float(m.bbox_max[k]) for m in ms) for k in range(3)]
    mn, mx = scene_or_bbox
    return [float(v) for v in mn], [float(v) for v in mx]


def preview_rule(scene_or_bbox):
    """The command line's preview camera rule, in double: box = cumulative bounding box of the meshes, centre = (min + max) / 2,
    radius = |max - min| / 2, dist = 1.1 radius / tan(22.5 deg), near = dist / 100, far = dist * 10.  -> (centre, dist, near, far)"""
    mn, mx = _bbox(scene_or_bbox)
    ctr = [(mn[k] + mx[k]) / 2 for k in range(3)]
    d2 = 0.0
    for k in range(3):
        d2 += (mx[k] - mn[k]) * (mx[k] - mn[k])
    radius = math.sqrt(d2) / 2
    dist = 1.1 * radius / math.tan(22.5 * (math.pi / 180.0))
    return ctr, dist, dist / 100, dist * 10


def camera_from_eye(eye, centre, near: float, far: float, W: int, H: int) -> OrbitCamera:
    """glm::lookAt(eye, centre, (0, 1, 0)) and glm::perspective(45 deg, W / H, near, far) in double, operation for operation as
    tools/mesh2splat_cli.cpp takes them, rounded to float."""
    eye, ctr = [float(v) for v in eye], [float(v) for v in centre]
    f = [ctr[k] - eye[k] for k in range(3)]
    fl = math.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])
    f = [v / fl for v in f]
    up = (0.0, 1.0, 0.0)
    s = [f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]]
    sl = math.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
    s = [v / sl for v in s]
    u = [s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]]
    m = np.zeros(16, np.float64)
    m[15] = 1
    for k in range(3):
        m[k * 4 + 0], m[k * 4 + 1], m[k * 4 + 2] = s[k], u[k], -f[k]
    m[12] = -(s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2])
    m[13] = -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2])
    m[14] = f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2]
    t, aspect = math.tan(45.0 * (math.pi / 180.0) / 2.0), float(W) / float(H)
    p = np.zeros(16, np.float64)
    p[0] = 1.0 / (aspect * t)
    p[5] = 1.0 / t
    p[10] = -(far + near) / (far - near)
    p[11] = -1.0
    p[14] = -(2.0 * far * near) / (far - near)
    return OrbitCamera(tuple(eye), tuple(ctr), float(near), float(far), (int(W), int(H)), m.astype(np.float32).reshape(4, 4),
                       p.astype(np.float32).reshape(4, 4))


def orbit_eye(centre, dist: float, k: int, K: int, elevation_deg: float = 0.0):
    """Eye of view k of K: on the sphere of radius dist round the centre, rotated about the vertical axis through the centre by
    2 pi k / K from the +z side and raised by the elevation.  k = 0 at elevation 0 is centre + (0, 0, dist) exactly."""
    if not -90.0 < elevation_deg < 90.0:
        raise ValueError("elevation must lie strictly between -90 and 90 degrees (the up vector is the vertical)")
    th, el = 2.0 * math.pi * k / K, elevation_deg * (math.pi / 180.0)
    return [centre[0] + dist * math.cos(el) * math.sin(th), centre[1] + dist * math.sin(el), centre[2] + dist * math.cos(el) * math.cos(th)]


def orbit_cameras(scene_or_bbox, K: int, W: int, H: int, elevation_deg: float = 0.0):
    """K cameras round the scene (a Scene, or (bbox_min, bbox_max)).  View 0 is the command line's preview camera — same centre, distance,
    near, far and field of view, in double with the matrices rounded to float —; view k has the eye rotated about the vertical axis through
    the centre by 2 pi k / K and raised by the elevation (orbit_eye)."""
    if K < 1:
        raise ValueError("K must be at least 1")
    ctr, dist, near, far = preview_rule(scene_or_bbox)
    return [camera_from_eye(orbit_eye(ctr, dist, k, K, elevation_deg), ctr, near, far, W, H) for k in range(K)]
