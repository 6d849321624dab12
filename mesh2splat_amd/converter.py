"""Host-side mirror of the reference's operator interface for the conversion path.

Reference                                             | here
------------------------------------------------------+--------------------------------------------
IRenderPass / ConversionPass::execute(RenderContext&) | ConversionPass.execute(RenderContext)
  (RenderPass.hpp:11-29, ConversionPass.cpp:9-68)     |
RenderContext fields the pass reads / writes          | RenderContext (same names)
  (RenderContext.hpp:64,73,83,86,90)                  |
SceneManager::exportPly(outputFile, exportFormat)     | SceneManager.exportPly
  (SceneManager.cpp:651-678)                          |
parsers::savePlyVector                                | write_ply

All compute happens in the HIP library behind include/m2s.h; this file only marshals arguments.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _lib
from .scene import RECORD_FLOATS, TEXTURE_SLOTS, Scene


def marshal_scene(scene: Scene):
    """Scene -> (m2s_mesh[] for the C ABI, objects that must stay alive while it is used)."""
    n = scene.n_meshes
    arr = (_lib.MeshC * max(1, n))()
    keep = []
    for i, m in enumerate(scene.meshes):
        v = np.ascontiguousarray(m.vertices, np.float32)
        keep.append(v)
        arr[i].vertices = v.ctypes.data
        arr[i].n_vertices = v.shape[0]
        arr[i].stride_floats = v.shape[1]
        for k in range(3):
            arr[i].bbox_min[k] = float(m.bbox_min[k])
            arr[i].bbox_max[k] = float(m.bbox_max[k])
        for k in range(4):
            arr[i].base_color[k] = float(m.base_color[k])
        for k, key in enumerate(TEXTURE_SLOTS):
            t = m.textures.get(key)
            if t is None:
                continue
            keep.append(t)
            arr[i].tex[k].rgba8 = t.ctypes.data
            arr[i].tex[k].width = t.shape[1]
            arr[i].tex[k].height = t.shape[0]
    return arr, keep


class _DeviceImage:
    """A (h, w) float32 image at a device address, in the shape mesh2splat_amd.prepass.to_c reads a CUDA tensor."""

    def __init__(self, ptr: int, h: int, w: int):
        self._ptr, self.shape = int(ptr), (int(h), int(w))

    def data_ptr(self) -> int:
        return self._ptr

    def contiguous(self):
        return self

    def float(self):
        return self


class Converter:
    """Thin owner of one m2s_ctx (one per host thread / per GPU rank)."""

    def __init__(self, device: int = 0):
        self._L = _lib.load()
        h = C.c_void_p()
        st = self._L.m2s_create(int(device), C.byref(h))
        if st != _lib.M2S_OK:
            raise _lib.M2SError(st, self._L.m2s_last_error(None).decode())
        self._h = h
        self.device = int(device)
        self._keep = None
        self._last_splat_wh = (0, 0)

    # -- helpers ------------------------------------------------------------------------------------
    _nonnull = C.c_uint64(0)      # a non-NULL address for "n = 0 records at this pointer"
    _last_shadow_S = 0            # side of the context's shadow cube (0: none yet)
    _last_splat_wh = (0, 0)       # W x H of the context's G-buffer
    _last_bake_n = 0              # records of the context's baked plane

    def _check(self, st: int):
        if st != _lib.M2S_OK:
            raise _lib.M2SError(st, self._L.m2s_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.m2s_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- scene ------------------------------------------------------------------------------------
    def set_triangle_range(self, first: int, count: Optional[int]):
        self._check(self._L.m2s_set_triangle_range(self._h, int(first), (1 << 64) - 1 if count is None else int(count)))

    PREPARE_UPLOAD, PREPARE_EXPORT, PREPARE_KERNELS = 1, 2, 4

    def prepare(self, flags: int = 7):
        """m2s_prepare: staging buffers (upload / export) and the kernels' code objects now, not inside the first upload /
        export / conversion of the process (the command line does this on a second thread while it parses the file)."""
        self._check(self._L.m2s_prepare(self._h, int(flags)))

    def set_resolution_hint(self, R: int):
        """The resolutionTarget the next upload_scene prepares for (0: the last R converted at, else 1024)."""
        self._check(self._L.m2s_set_resolution_hint(self._h, int(R)))

    def upload_scene(self, scene: Scene):
        arr, keep = marshal_scene(scene)
        self._check(self._L.m2s_upload_scene(self._h, arr, scene.n_meshes))
        del keep

    def last_upload_ms(self) -> dict:
        """Wall-clock breakdown of the last upload_scene (ms)."""
        ms = (C.c_float * 4)()
        self._check(self._L.m2s_last_upload_ms(self._h, ms))
        return {"total": float(ms[0]), "geometry": float(ms[1]), "textures": float(ms[2]), "alloc": float(ms[3]),
                "warm": float(self._L.m2s_last_warm_ms(self._h))}

    # -- the pass ---------------------------------------------------------------------------------
    def set_max_gaussians(self, cap: int):
        """-1 reference formula (default), 0 unlimited, >0 explicit."""
        self._check(self._L.m2s_set_max_gaussians(self._h, int(cap)))

    def convert(self, R: int) -> int:
        total = C.c_uint64()
        self._check(self._L.m2s_convert(self._h, int(R), C.byref(total)))
        return int(total.value)

    def convert_into(self, R: int, device_ptr: int, capacity_records: int, stream: int = 0) -> int:
        total = C.c_uint64()
        self._check(self._L.m2s_convert_into(self._h, int(R), C.c_void_p(device_ptr), int(capacity_records),
                                             C.c_void_p(stream), C.byref(total)))
        return int(total.value)

    def submit(self, R: int, device_ptr: int = 0, capacity_records: int = 0, stream: int = 0) -> None:
        """Enqueue one conversion without waiting (m2s_convert_submit); device_ptr == 0 uses the context's buffer."""
        self._check(self._L.m2s_convert_submit(self._h, int(R), C.c_void_p(device_ptr or None), int(capacity_records),
                                               C.c_void_p(stream or None)))

    def wait(self) -> int:
        """Counter of the oldest submitted conversion, once it has finished (m2s_convert_wait)."""
        total = C.c_uint64()
        self._check(self._L.m2s_convert_wait(self._h, C.byref(total)))
        return int(total.value)

    @property
    def num_stored(self) -> int:
        return int(self._L.m2s_num_stored(self._h))

    @property
    def num_triangles(self) -> int:
        return int(self._L.m2s_num_triangles(self._h))

    @property
    def device_records(self) -> int:
        return int(self._L.m2s_device_records(self._h) or 0)

    def download(self) -> np.ndarray:
        n = self.num_stored
        out = np.empty((n, RECORD_FLOATS), np.float32)
        self._check(self._L.m2s_download(self._h, out.ctypes.data, n))
        return out

    def download_triangle_counts(self) -> np.ndarray:
        n = self.num_triangles
        out = np.empty(n, np.uint32)
        self._check(self._L.m2s_download_triangle_counts(self._h, out.ctypes.data, n))
        return out

    def export_ply(self, path: str, fmt: int = 0, gaussian_std: float = 0.65):
        self._check(self._L.m2s_export_ply(self._h, os.fsencode(path), int(fmt), float(gaussian_std)))

    def export_ply_slice(self, path: str, fmt: int, gaussian_std: float, first_row: int, n_rows: int, total_rows: int):
        """This rank's rows of a .ply that several ranks write together (m2s_export_ply_slice)."""
        self._check(self._L.m2s_export_ply_slice(self._h, os.fsencode(path), int(fmt), float(gaussian_std), int(first_row),
                                                 int(n_rows), int(total_rows)))

    def reserve_records(self, n: int) -> int:
        """Room for n records in the context-owned pool; its device address (m2s_reserve_records)."""
        p = C.c_void_p()
        self._check(self._L.m2s_reserve_records(self._h, int(n), C.byref(p)))
        return int(p.value or 0)

    def set_records(self, device_ptr: int, n: int, R: int):
        """Device-resident records from elsewhere (e.g. the merged buffer of a multi-GPU exchange) become the context's
        current records, zero copy (m2s_set_records)."""
        self._check(self._L.m2s_set_records(self._h, C.c_void_p(device_ptr or None), int(n), int(R)))

    def set_keep_positions(self, on: bool):
        """Say before converting that the records will be depth-sorted: the sparse kernel then also writes the 16-byte position plane."""
        self._check(self._L.m2s_set_keep_positions(self._h, 1 if on else 0))

    @property
    def positions_ready(self) -> bool:
        """the 16-byte position plane of the current records exists (left by their conversion or by an earlier depth sort)"""
        return bool(self._L.m2s_positions_ready(self._h))

    def sort_by_depth(self, world_to_view, download: bool = True):
        """RadixSortPass: sort the last conversion's records by floatBitsToUint(view-space z); returns them (or, with
        download=False, their number: the sorted records stay on the device).
        world_to_view: 4x4, applied as M @ (P,1) (stored column-major for the ABI, like glm)."""
        m = np.ascontiguousarray(np.asarray(world_to_view, np.float32).T.reshape(16))   # column-major
        n = C.c_uint64()
        self._check(self._L.m2s_sort_by_depth(self._h, m.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n)))
        if not download:
            return int(n.value)
        out = np.empty((n.value, RECORD_FLOATS), np.float32)
        self._check(self._L.m2s_download_sorted(self._h, out.ctypes.data, n.value))
        return out

    def download_sorted(self) -> np.ndarray:
        """The context's sorted buffer (after sort_by_depth(download=False) or RcclExchange.sort_by_depth)."""
        n = int(self._L.m2s_num_sorted(self._h))
        out = np.empty((n, RECORD_FLOATS), np.float32)
        if n:
            self._check(self._L.m2s_download_sorted(self._h, out.ctypes.data, n))
        return out

    @property
    def last_sort_ms(self) -> float:
        return float(self._L.m2s_last_sort_ms(self._h))

    @property
    def last_sort_stage_ms(self) -> dict:
        """keys | radix sort | gather of the last sort_by_depth (profiling on)."""
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_sort_stage_ms(self._h, ms))
        return {"keys": float(ms[0]), "radix_sort": float(ms[1]), "gather": float(ms[2])}

    def upload_records(self, records: np.ndarray):
        """Renderer::updateGaussianBuffer after LoadPly: (n, 24) float32 host records become the context's current records."""
        r = np.ascontiguousarray(records, np.float32).reshape(-1, RECORD_FLOATS)
        self._check(self._L.m2s_upload_records(self._h, r.ctypes.data, r.shape[0]))

    def prepass(self, params, records=None, download: bool = True):
        """GaussiansPrepass: cull + covariance projection of the last conversion's records (or of `records`, a CUDA torch
        tensor of shape (n, 24) float32).  `params`: mesh2splat_amd.prepass.PrepassParams.
        -> (visible, quads (visible,24) f32, depths (visible,) f32) in input order; with download=False only `visible`
        (the results stay on the device: device_quads / device_prepass_depths)."""
        from . import prepass as _pp
        pc, keep = _pp.to_c(params)
        ptr, n = None, 0
        if records is not None:
            if not (hasattr(records, "data_ptr") and records.is_cuda and records.is_contiguous()):
                raise ValueError("records must be a contiguous CUDA tensor (n, 24) float32")
            ptr, n = records.data_ptr(), int(records.shape[0])
            if n == 0:                       # (a NULL pointer would mean "the last conversion" to the C entry point)
                return (0, np.empty((0, 24), np.float32), np.empty(0, np.float32)) if download else 0
        vis = C.c_uint64()
        self._check(self._L.m2s_prepass(self._h, C.byref(pc), ptr, n, C.byref(vis)))
        del keep
        if not download:
            return vis.value
        quads = np.empty((vis.value, 24), np.float32)
        depths = np.empty(vis.value, np.float32)
        self._check(self._L.m2s_download_prepass(self._h, quads.ctypes.data, depths.ctypes.data, vis.value))
        return vis.value, quads, depths

    @property
    def device_quads(self) -> int:
        return int(self._L.m2s_device_quads(self._h) or 0)

    @property
    def device_prepass_depths(self) -> int:
        return int(self._L.m2s_device_prepass_depths(self._h) or 0)

    @property
    def last_prepass_ms(self) -> float:
        return float(self._L.m2s_last_prepass_ms(self._h))

    def sort_prepass(self, download: bool = True):
        """RadixSortPass on the last prepass: quads ordered by the raw bits of their view-space depth (ascending, stable).
        -> (n, 24) float32 quads, or just n with download=False."""
        n = C.c_uint64()
        self._check(self._L.m2s_sort_prepass(self._h, C.byref(n)))
        if not download:
            return n.value
        out = np.empty((n.value, 24), np.float32)
        self._check(self._L.m2s_download_sorted_quads(self._h, out.ctypes.data, n.value))
        return out

    def prepass_sorted(self, params, download: bool = True):
        """GaussiansPrepass + RadixSortPass of one frame in one pass over the context's records (m2s_prepass_sorted): the depth sort first,
        as a permutation; the prepass through it.  -> (visible, 24) float32 quads in depth order == prepass() then sort_prepass(), byte
        for byte; or just `visible` with download=False."""
        from . import prepass as _pp
        pc, keep = _pp.to_c(params)
        vis = C.c_uint64()
        self._check(self._L.m2s_prepass_sorted(self._h, C.byref(pc), C.byref(vis)))
        del keep
        if not download:
            return vis.value
        out = np.empty((vis.value, 24), np.float32)
        self._check(self._L.m2s_download_sorted_quads(self._h, out.ctypes.data, vis.value))
        return out

    @property
    def last_sort_prepass_ms(self) -> float:
        return float(self._L.m2s_last_sort_prepass_ms(self._h))

    def upload_quads(self, quads: np.ndarray):
        """(n, 24) float32 host quads (m2s_quad) become the context's sorted quads: what splat() draws without `quads`."""
        q = np.ascontiguousarray(quads, np.float32).reshape(-1, 24)
        self._check(self._L.m2s_upload_quads(self._h, q.ctypes.data if q.shape[0] else None, q.shape[0]))

    def splat(self, params, quads=None, download: bool = True):
        """GaussianSplattingPass (m2s_splat): blend the context's sorted quads (or `quads`, a contiguous CUDA torch tensor (n, 24)
        float32) in array order into the five-target G-buffer.  `params`: mesh2splat_amd.splat.SplatParams.
        -> (planes, skipped): planes = five (H, W, 4) arrays (float16 for attachments 0, 1, 3, uint8 for 2, 4), row 0 = the bottom
        row; with download=False just `skipped` (the planes stay on the device: device_gbuffer(k))."""
        from . import splat as _sp
        pc = _sp.to_c(params)
        ptr, n = None, 0
        if quads is not None:
            if not (hasattr(quads, "data_ptr") and quads.is_cuda and quads.is_contiguous()):
                raise ValueError("quads must be a contiguous CUDA tensor (n, 24) float32")
            n = int(quads.shape[0])
            ptr = quads.data_ptr() if n else 1          # n = 0: cleared planes (a NULL pointer would mean "the sorted quads")
        skipped = C.c_uint64()
        self._check(self._L.m2s_splat(self._h, C.byref(pc), ptr, n, C.byref(skipped)))
        self._last_splat_wh = (int(pc.resolution[0]), int(pc.resolution[1]))
        if not download:
            return skipped.value
        return self.download_gbuffer(), skipped.value

    def download_gbuffer(self):
        """The five planes of the last splat as (H, W, 4) arrays."""
        from . import splat as _sp
        W, H = self._last_splat_wh
        out = []
        for k, (_, dt) in enumerate(_sp.ATTACHMENTS):
            a = np.empty((H, W, 4), dt)
            self._check(self._L.m2s_download_gbuffer(self._h, k, a.ctypes.data, a.nbytes))
            out.append(a)
        return out

    def device_gbuffer(self, attachment: int) -> int:
        return int(self._L.m2s_device_gbuffer(self._h, int(attachment)) or 0)

    @property
    def last_splat_ms(self) -> float:
        return float(self._L.m2s_last_splat_ms(self._h))

    def last_splat_stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_splat_stage_ms(self._h, ms))
        return {"setup_bin": float(ms[0]), "grouping": float(ms[1]), "blend": float(ms[2])}

    def last_splat_counts(self) -> dict:
        v = (C.c_uint64 * 3)()
        self._check(self._L.m2s_last_splat_counts(self._h, v))
        return {"pairs": int(v[0]), "fragments": int(v[1]), "skipped": int(v[2])}

    def shadow(self, prepass_params, light_params, records=None, download: bool = True):
        """GaussianShadowPass (m2s_shadow): every record of the context (or of `records`, a contiguous CUDA torch tensor (n, 24)
        float32) through the six cameras of the light into per-face quad lists, those drawn depth-only into the cube.
        `prepass_params`: mesh2splat_amd.prepass.PrepassParams (its per-record fields), `light_params`: mesh2splat_amd.light.LightParams.
        -> (per_face, skipped, cube): six list lengths, quads skipped, cube (6, S, S) float32 (faces in GL order, row 0 = t = 0);
        with download=False (per_face, skipped) — the cube stays on the device (device_shadow_cubemap)."""
        from . import light as _li, prepass as _pp
        pc, keep = _pp.to_c(prepass_params)
        lc = _li.to_c(light_params)
        ptr, n = None, 0
        if records is not None:
            if not (hasattr(records, "data_ptr") and records.is_cuda and records.is_contiguous()):
                raise ValueError("records must be a contiguous CUDA tensor (n, 24) float32")
            n = int(records.shape[0])
            # n = 0: a cube of 1.0.  An empty tensor's data_ptr() is 0, which the C entry point reads as "the context's records": pass the
            # address of a host word instead — with n = 0 the pointer is only compared with NULL, never dereferenced (include/m2s.h)
            ptr = records.data_ptr() if n else C.addressof(self._nonnull)
        per_face = (C.c_uint64 * 6)()
        skipped = C.c_uint64()
        self._check(self._L.m2s_shadow(self._h, C.byref(pc), C.byref(lc), ptr, n, per_face, C.byref(skipped)))
        del keep
        self._last_shadow_S = int(lc.shadow_resolution) or _li.SHADOW_CUBEMAP_SIZE
        if not download:
            return list(per_face), skipped.value
        return list(per_face), skipped.value, self.download_shadow_cubemap()

    def shadow_from_quads(self, lists, light_params, download: bool = True):
        """Stage B of the shadow pass alone (m2s_shadow_from_quads): `lists` = six (n_f, 12) float32 host arrays of shadow quads (mean,
        axes, world position), one per cube face, drawn depth-only into a cleared cube.  -> (skipped, cube) or, download=False, skipped."""
        from . import light as _li
        lc = _li.to_c(light_params)
        arrs = [np.ascontiguousarray(q, np.float32).reshape(-1, 12) for q in lists]
        assert len(arrs) == 6
        allq = np.ascontiguousarray(np.concatenate(arrs, 0))
        per_face = (C.c_uint64 * 6)(*[a.shape[0] for a in arrs])
        skipped = C.c_uint64()
        self._check(self._L.m2s_shadow_from_quads(self._h, C.byref(lc), allq.ctypes.data if allq.shape[0] else None, per_face, C.byref(skipped)))
        self._last_shadow_S = int(lc.shadow_resolution) or _li.SHADOW_CUBEMAP_SIZE
        return (skipped.value, self.download_shadow_cubemap()) if download else skipped.value

    def download_shadow_cubemap(self) -> np.ndarray:
        S = self._last_shadow_S or 1                  # (before any cube: the library answers M2S_ERR_STATE)
        cube = np.empty((6, S, S), np.float32)
        self._check(self._L.m2s_download_shadow_cubemap(self._h, cube.ctypes.data, cube.size))
        return cube

    def download_shadow_quads(self, face: int, count: int) -> np.ndarray:
        """(count, 12) float32: the list of `face` of the last shadow() in input order (m2s_shadow_quad: mean, axes, world position)."""
        q = np.empty((int(count), 12), np.float32)
        self._check(self._L.m2s_download_shadow_quads(self._h, int(face), q.ctypes.data if count else None, int(count)))
        return q

    def upload_shadow_cubemap(self, cube: np.ndarray):
        """(6, S, S) float32 host cube becomes the context's: what relight() samples."""
        c = np.ascontiguousarray(cube, np.float32)
        assert c.ndim == 3 and c.shape[0] == 6 and c.shape[1] == c.shape[2]
        self._check(self._L.m2s_upload_shadow_cubemap(self._h, c.ctypes.data, c.shape[1]))
        self._last_shadow_S = int(c.shape[1])

    @property
    def device_shadow_cubemap(self) -> int:
        return int(self._L.m2s_device_shadow_cubemap(self._h) or 0)

    def upload_gbuffer(self, planes):
        """Five (H, W, 4) host planes (float16 for attachments 0, 1, 3, uint8 for 2, 4; None = zeros; row 0 = bottom) become the
        context's G-buffer, as if splat() had left them."""
        from . import splat as _sp
        shape = next(p.shape for p in planes if p is not None)
        H, W = int(shape[0]), int(shape[1])
        keep, ptrs = [], (C.c_void_p * 5)()
        for k, (_, dt) in enumerate(_sp.ATTACHMENTS):
            if planes[k] is None:
                ptrs[k] = None
                continue
            a = np.ascontiguousarray(planes[k], dt)
            assert a.shape == (H, W, 4)
            keep.append(a)
            ptrs[k] = a.ctypes.data
        self._check(self._L.m2s_upload_gbuffer(self._h, ptrs, W, H))
        self._last_splat_wh = (W, H)

    def relight(self, light_params, download: bool = True):
        """GaussianRelightingPass (m2s_relight) over the context's G-buffer and cube.  -> frame (H, W, 4) uint8, row 0 = bottom (with
        want_shadow_counts in mode 6: (frame, counts (H, W) uint8)); download=False: None (device_frame)."""
        from . import light as _li
        lc = _li.to_c(light_params)
        self._check(self._L.m2s_relight(self._h, C.byref(lc)))
        return self._download_relit(lc) if download else None

    def _download_relit(self, lc):
        """The frame of the last relight / relight_split (and its shadow counts, where `lc` asked for them)."""
        W, H = int(lc.resolution[0]), int(lc.resolution[1])
        frame = np.empty((H, W, 4), np.uint8)
        self._check(self._L.m2s_download_frame(self._h, frame.ctypes.data, frame.nbytes))
        if lc.want_shadow_counts and lc.render_mode == 6:
            counts = np.empty((H, W), np.uint8)
            self._check(self._L.m2s_download_shadow_counts(self._h, counts.ctypes.data, counts.nbytes))
            return frame, counts
        return frame

    @property
    def device_frame(self) -> int:
        return int(self._L.m2s_device_frame(self._h) or 0)

    def relight_split(self, light_params, split_position: float, download: bool = True):
        """GaussianRelightingPass with the split screen (m2s_relight_split): pixels left of int(split_position * W) are lit from the mesh
        G-buffer of the last mesh_render(), the others from the splat G-buffer; two white divider columns.  Returns what relight() does."""
        from . import light as _li
        lc = _li.to_c(light_params)
        self._check(self._L.m2s_relight_split(self._h, C.byref(lc), float(split_position)))
        return self._download_relit(lc) if download else None

    def mesh_render(self, params, download: bool = True):
        """MeshRenderPass (m2s_mesh_render): every mesh of the uploaded scene drawn through the camera of `params` (a
        mesh2splat_amd.meshrender.MeshRenderParams, or a PrepassParams whose camera, model matrix, resolution, planes and render mode
        are taken) into the mesh G-buffer.  -> (five planes as splat() returns them, counts dict); download=False: counts alone (the
        planes stay on the device: device_mesh_gbuffer, where relight_split() reads them)."""
        from . import meshrender as _mr
        mc = _mr.to_c(params)
        v = (C.c_uint64 * 6)()
        self._check(self._L.m2s_mesh_render(self._h, C.byref(mc), v))
        self._last_mr_wh = (int(mc.resolution[0]), int(mc.resolution[1]))
        counts = {k: int(v[i]) for i, k in enumerate(_mr.COUNT_NAMES)}
        if not download:
            return counts
        return self.download_mesh_gbuffer(), counts

    def download_mesh_gbuffer(self):
        """The five planes of the last mesh_render(): (H, W, 4) float16 for attachments 0, 1, 3, uint8 for 2, 4; row 0 = bottom."""
        from . import splat as _sp
        W, H = self._last_mr_wh
        planes = []
        for k, (_, dt) in enumerate(_sp.ATTACHMENTS):
            a = np.empty((max(H, 1), max(W, 1), 4), dt)             # (before any: the library answers M2S_ERR_STATE)
            self._check(self._L.m2s_download_mesh_gbuffer(self._h, k, a.ctypes.data, a.nbytes))
            planes.append(a)
        return planes

    def download_mesh_visibility(self) -> np.ndarray:
        """(H, W) uint64 of the last mesh_render(): (bits of z) << 32 | global triangle index; meshrender.EMPTY where nothing was drawn."""
        W, H = self._last_mr_wh
        vis = np.empty((max(H, 1), max(W, 1)), np.uint64)
        self._check(self._L.m2s_download_mesh_visibility(self._h, vis.ctypes.data, vis.size))
        return vis

    def device_mesh_gbuffer(self, attachment: int) -> int:
        return int(self._L.m2s_device_mesh_gbuffer(self._h, int(attachment)) or 0)

    @property
    def last_mesh_render_ms(self) -> float:
        return float(self._L.m2s_last_mesh_render_ms(self._h))

    def last_mesh_render_stage_ms(self) -> dict:
        from . import meshrender as _mr
        ms = (C.c_float * 4)()
        self._check(self._L.m2s_last_mesh_render_stage_ms(self._h, ms))
        return {k: float(ms[i]) for i, k in enumerate(_mr.STAGE_NAMES)}

    def mesh_depth(self, params, download: bool = True):
        """DepthPrepass (m2s_mesh_depth): the opaque meshes of the uploaded scene drawn depth-only through the camera of `params`
        (a mesh2splat_amd.meshdepth.MeshDepthParams, or a PrepassParams whose camera, model matrix and resolution are taken).
        -> (image (H, W) float32 window-space depth, row 0 = bottom, 1.0 = nothing drawn; counts dict); download=False: counts alone
        (the image stays on the device: device_mesh_depth, ready to be handed to prepass() as a device image)."""
        from . import meshdepth as _md
        mc = _md.to_c(params)
        v = (C.c_uint64 * 5)()
        self._check(self._L.m2s_mesh_depth(self._h, C.byref(mc), v))
        self._last_md_wh = (int(mc.resolution[0]), int(mc.resolution[1]))
        counts = {k: int(v[i]) for i, k in enumerate(_md.COUNT_NAMES)}
        if not download:
            return counts
        return self.download_mesh_depth(), counts

    _last_md_wh = (0, 0)
    _last_mr_wh = (0, 0)                 # resolution of the last mesh_render()

    def download_mesh_depth(self) -> np.ndarray:
        W, H = self._last_md_wh
        img = np.empty((max(H, 1), max(W, 1)), np.float32)          # (before any image: the library answers M2S_ERR_STATE)
        self._check(self._L.m2s_download_mesh_depth(self._h, img.ctypes.data, img.size))
        return img

    @property
    def device_mesh_depth(self) -> int:
        return int(self._L.m2s_device_mesh_depth(self._h) or 0)

    def debug_set_mesh_depth_inplace(self, max_box: int):
        """Test hook (m2s_debug_set_mesh_depth_inplace): pixel-box side up to which a triangle is covered in place; -1: default."""
        self._check(self._L.m2s_debug_set_mesh_depth_inplace(self._h, int(max_box)))

    @property
    def last_mesh_depth_ms(self) -> float:
        return float(self._L.m2s_last_mesh_depth_ms(self._h))

    def last_mesh_depth_stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_mesh_depth_stage_ms(self._h, ms))
        return {"setup": float(ms[0]), "bin": float(ms[1]), "raster": float(ms[2])}

    def _with_device_mesh_depth(self, prepass_params):
        """A copy of `prepass_params` that tests against the context's mesh depth image in place (depth_on_device)."""
        import dataclasses
        W, H = self._last_md_wh
        return dataclasses.replace(prepass_params, perform_mesh_depth_test=True, mesh_depth=_DeviceImage(self.device_mesh_depth, H, W))

    def render_frame(self, prepass_params, light_params, mesh_depth_test: bool = False, split_screen: Optional[float] = None,
                     download: bool = True):
        """One viewer frame of the context's records (renderer.cpp:129-138): prepass + depth sort + splat + shadow + relight.
        split_screen (None: off, the frame is what it was without the argument; else a position in [0, 1]): the mesh render pass of the
        uploaded scene runs with the frame's camera and render mode (mesh_render) and the relighting pass composes the reference's
        split screen (relight_split): mesh left of the divider, splats right.  (Both of those frames carry the white divider; the fidelity
        figure of a conversion is score(), which compares the splat frame with a mesh frame that has none.)  (m2s_prepass + m2s_sort_prepass rather than the fused m2s_prepass_sorted: the benchmark reads the two calls' stage times.)  `light_params`'s
        renderer_resolution must equal `prepass_params`'s.  mesh_depth_test: the frame starts with the mesh depth prepass of the uploaded
        scene (mesh_depth) and the Gaussian prepass — then m2s_prepass_sorted — tests against its image on the device, the reference's
        "use the mesh as occluder in depth prepass".  -> what relight() returns (download=False: None, the frame stays on the device)."""
        from .splat import SplatParams
        res = tuple(int(v) for v in prepass_params.renderer_resolution)
        if tuple(int(v) for v in light_params.renderer_resolution) != res:
            raise ValueError("light_params.renderer_resolution differs from prepass_params.renderer_resolution")
        if mesh_depth_test:
            self.mesh_depth(prepass_params, download=False)
            visible = self.prepass_sorted(self._with_device_mesh_depth(prepass_params), download=False)
        else:
            self.prepass(prepass_params, download=False)
            visible = self.sort_prepass(download=False)
        if visible:
            self.splat(SplatParams(res, int(prepass_params.render_mode)), download=False)
        else:
            import torch
            self.splat(SplatParams(res, int(prepass_params.render_mode)), quads=torch.empty((0, 24), dtype=torch.float32, device="cuda"), download=False)
        self.shadow(prepass_params, light_params, download=False)
        if split_screen is not None:
            self.mesh_render(prepass_params, download=False)
            return self.relight_split(light_params, split_screen, download=download)
        return self.relight(light_params, download=download)

    # -- the light baked into spherical harmonics -----------------------------------------------------
    def _records_arg(self, records):
        """(pointer, n) of `records` (None: the context's; else a contiguous CUDA torch tensor (n, 24) float32) for the C entry points."""
        if records is None:
            return None, 0
        if not (hasattr(records, "data_ptr") and records.is_cuda and records.is_contiguous()):
            raise ValueError("records must be a contiguous CUDA tensor (n, 24) float32")
        n = int(records.shape[0])
        return (records.data_ptr() if n else C.addressof(self._nonnull)), n

    def bake_light(self, bake_params, light_params, records=None, download: bool = True):
        """m2s_bake_light: the deferred shader per Gaussian over a fixed table of view directions, projected onto the 16 harmonics of
        the standard .ply.  `bake_params`: mesh2splat_amd.bake.BakeParams, `light_params`: mesh2splat_amd.light.LightParams (position,
        colour, intensity, far plane); the cube is the context's (shadow() / upload_shadow_cubemap()).  -> the plane (n, 48) float32
        (with want_shadow_counts: (plane, counts (n,) uint8)); download=False: None (device_sh)."""
        from . import bake as _bk, light as _li
        bc, lc = _bk.to_c(bake_params), _li.to_c(light_params)
        ptr, n = self._records_arg(records)
        self._check(self._L.m2s_bake_light(self._h, C.byref(bc), C.byref(lc), ptr, n))
        self._last_bake_n = n if records is not None else self.num_stored
        if not download:
            return None
        sh = self.download_sh()
        if bc.want_shadow_counts:
            counts = np.empty(self._last_bake_n, np.uint8)
            self._check(self._L.m2s_download_bake_shadow_counts(self._h, counts.ctypes.data if counts.size else None, counts.size))
            return sh, counts
        return sh

    def download_sh(self) -> np.ndarray:
        """The context's SH plane: (n, 48) float32 — f_dc[3], then f_rest[45] channel-major.  It is the last bake_light()'s, or what
        upload_sh(), a prune and, with carry_sh, a merge or a cut have made of it since (sized by sh_plane_info())."""
        rows = C.c_uint64()
        if self._L.m2s_sh_plane_info(self._h, C.byref(rows), None) == _lib.M2S_OK:
            n = int(rows.value)
        else:
            n = self._last_bake_n
        sh = np.empty((n, 48), np.float32)
        self._check(self._L.m2s_download_sh(self._h, sh.ctypes.data if sh.size else None, sh.shape[0]))
        return sh

    @property
    def carry_sh(self) -> bool:
        """m2s_set_carry_sh: merge(), lod_build() and the cuts carry a baked SH plane of the records instead of dropping it.  Off by
        default."""
        return bool(self._L.m2s_carry_sh(self._h))

    @carry_sh.setter
    def carry_sh(self, on: bool):
        self._check(self._L.m2s_set_carry_sh(self._h, 1 if on else 0))

    @property
    def merge_model(self) -> tuple:
        """m2s_merge_model / m2s_merge_sigma -> ("footprint" | "gaussian", sigma): the record model merge(), merge_count(),
        merge_to_budget() and lod_build() act under (include/m2s.h, pins 2g, 5g, 5sg, 4g)."""
        from . import merge as _mg
        return _mg.MODELS[int(self._L.m2s_merge_model(self._h))], float(self._L.m2s_merge_sigma(self._h))

    def set_merge_model(self, model: str = "footprint", sigma: float = 1.0):
        """m2s_set_merge_model.  "footprint" (the default): a record is the flat texel footprint the conversion emits.  "gaussian": a 3D
        Gaussian with standard deviations sigma * scale[0..2], what a loaded .ply holds (sigma = 1) or a conversion behind
        records_to_world_units (sigma = gaussian_std).  lod_blend() refuses a tree built under "gaussian"."""
        from . import merge as _mg
        if model not in _mg.MODELS:
            raise ValueError(f"merge model {model!r}: one of {_mg.MODELS}")
        self._check(self._L.m2s_set_merge_model(self._h, _mg.MODELS.index(model), float(sigma)))

    def upload_sh(self, sh, degree: int = 3):
        """m2s_upload_sh: `sh` (n, 48) float32, n the context's stored records, becomes their SH plane of this degree (no tap counts)."""
        sh = np.ascontiguousarray(sh, np.float32)
        if sh.ndim != 2 or sh.shape[1] != 48:
            raise ValueError("sh must be (n, 48) float32")
        self._check(self._L.m2s_upload_sh(self._h, sh.ctypes.data if sh.size else None, sh.shape[0], int(degree)))

    def sh_plane_info(self) -> dict:
        """m2s_sh_plane_info -> {"rows", "degree"} of the context's SH plane; M2SError (M2S_ERR_STATE) without one."""
        rows, degree = C.c_uint64(), C.c_uint32()
        st = self._L.m2s_sh_plane_info(self._h, C.byref(rows), C.byref(degree))
        if st:
            raise _lib.M2SError(st, "the context has no SH plane (bake_light, upload_sh)")
        return {"rows": int(rows.value), "degree": int(degree.value)}

    @property
    def device_sh(self) -> int:
        return int(self._L.m2s_device_sh(self._h) or 0)

    @property
    def last_bake_ms(self) -> float:
        return float(self._L.m2s_last_bake_ms(self._h))

    def sh_shade_records(self, model_mat, camera_position, records=None, out=None):
        """m2s_sh_shade_records: the records (None: the context's) with color.rgb replaced by what a standard 3DGS viewer shows of the
        baked plane from `camera_position`.  -> a CUDA torch tensor (n, 24) float32 (`out`, when given)."""
        import torch
        ptr, n = self._records_arg(records)
        if records is None:
            n = self.num_stored
        if out is None:
            out = torch.empty((n, RECORD_FLOATS), dtype=torch.float32, device="cuda")
        if not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n * RECORD_FLOATS):
            raise ValueError("out must be a contiguous CUDA float32 tensor of n x 24 floats")
        torch.cuda.current_stream().synchronize()          # the context's stream does not wait for torch's
        m = (C.c_float * 16)(*np.ascontiguousarray(model_mat, np.float32).reshape(16).tolist())
        cam = (C.c_float * 3)(*[float(np.float32(v)) for v in camera_position])
        self._check(self._L.m2s_sh_shade_records(self._h, m, cam, ptr, n, out.data_ptr() if n else None))
        return out

    def export_ply_sh(self, path: str, gaussian_std: float = 0.65):
        """m2s_export_ply_sh: the context's records with the baked plane as a standard (format 0) .ply."""
        self._check(self._L.m2s_export_ply_sh(self._h, os.fsencode(path), float(gaussian_std)))

    def export_ply_compact(self, path: str, gaussian_std: float = 0.65, baked_sh: bool = False) -> dict:
        """m2s_export_ply_compact: the context's records as a compact .ply (Morton-ordered chunks of 256, 16 bytes per row; with baked_sh the
        colour and the SH element come from the plane of the last bake_light()).  -> {"rows", "chunks", "skipped", "bytes", "stage_ms"}."""
        counts = (C.c_uint64 * 3)()
        self._check(self._L.m2s_export_ply_compact(self._h, os.fsencode(path), float(gaussian_std), 1 if baked_sh else 0, counts))
        return {"rows": int(counts[0]), "chunks": int(counts[1]), "skipped": int(counts[2]), "bytes": os.path.getsize(path),
                "stage_ms": self.last_compact_stage_ms()}

    def last_compact_stage_ms(self) -> dict:
        ms = (C.c_float * 4)()
        self._check(self._L.m2s_last_compact_stage_ms(self._h, ms))
        return {"box_keys": float(ms[0]), "sort": float(ms[1]), "pack": float(ms[2]), "download_write": float(ms[3])}

    def render_baked(self, prepass_params, download: bool = True):
        """What a standard 3DGS viewer shows of the baked records through `prepass_params`'s camera: sh_shade_records() from the camera
        position (the view matrix inverted), the viewer prepass in render mode 0 over the shaded copy, depth sort, splat.  -> the albedo
        attachment (H, W, 4) uint8, row 0 = bottom (download=False: None; it stays on the device: device_gbuffer(2))."""
        import dataclasses
        from .splat import SplatParams
        V = np.asarray(prepass_params.view_mat, np.float64).reshape(4, 4).T           # glm's memory order -> math order
        cam = -(V[:3, :3].T @ V[:3, 3])                                               # rigid view matrix: eye = -R^T t
        shaded = self.sh_shade_records(prepass_params.model_mat, cam)
        pp = dataclasses.replace(prepass_params, render_mode=0)
        res = tuple(int(v) for v in pp.renderer_resolution)
        self.prepass(pp, records=shaded, download=False)
        if self.sort_prepass(download=False):
            self.splat(SplatParams(res, 0), download=False)
        else:                                                                         # nothing visible: cleared planes
            import torch
            self.splat(SplatParams(res, 0), quads=torch.empty((0, 24), dtype=torch.float32, device="cuda"), download=False)
        del shaded
        if not download:
            return None
        alb = np.empty((res[1], res[0], 4), np.uint8)
        self._check(self._L.m2s_download_gbuffer(self._h, 2, alb.ctypes.data, alb.nbytes))
        return alb

    def score_baked(self, prepass_params, light_params):
        """How close the baked export looks to the viewer's own lit frame through one camera: m2s_score_frames between the lit splat
        frame of render_frame() (image A) and render_baked()'s albedo attachment used as a frame (image B), over the pixels the splats
        cover (the attachment's accumulated alpha; both renders draw the same quads).  Nothing but the result leaves the device.
        -> ScoreResult (mean squared error per channel value: sum(sse) / (3 * pixels))."""
        from . import score as _sc
        res = tuple(int(v) for v in prepass_params.renderer_resolution)
        self.render_frame(prepass_params, light_params, download=False)               # the frame has its own buffer ...
        self.render_baked(prepass_params, download=False)                             # ... so this splat leaves it as it is
        W, H = res
        baked = _DeviceImage(self.device_gbuffer(2), H, W)
        return self.score_frames(_sc.ScoreParams(res, _sc.MASK_A_AND_B, False, False),
                                 a=_DeviceImage(self.device_frame, H, W), b=baked, cover_a=baked, cover_b=baked)

    # -- fidelity score ----------------------------------------------------------------------------
    def relight_mesh(self, light_params, download: bool = True):
        """m2s_relight_mesh: the relighting pass over the MESH G-buffer of the last mesh_render(), every pixel, no divider, into a second
        frame buffer (device_mesh_frame); device_frame is left as it was.  -> frame (H, W, 4) uint8, row 0 = bottom; download=False: None."""
        from . import light as _li
        lc = _li.to_c(light_params)
        self._check(self._L.m2s_relight_mesh(self._h, C.byref(lc)))
        return self.download_mesh_frame(int(lc.resolution[0]), int(lc.resolution[1])) if download else None

    def download_mesh_frame(self, W: int, H: int) -> np.ndarray:
        """The frame of the last relight_mesh(): (H, W, 4) uint8, row 0 = bottom."""
        frame = np.empty((int(H), int(W), 4), np.uint8)
        self._check(self._L.m2s_download_mesh_frame(self._h, frame.ctypes.data, frame.nbytes))
        return frame

    @property
    def device_mesh_frame(self) -> int:
        return int(self._L.m2s_device_mesh_frame(self._h) or 0)

    @staticmethod
    def _image_ptr(img, what: str, nbytes: int):
        """Device address of `img`: None (the context's own buffer), a contiguous CUDA torch tensor of W * H * 4 bytes, or a _DeviceImage."""
        if img is None:
            return None, False
        if isinstance(img, _DeviceImage):
            return img.data_ptr(), False
        if not (hasattr(img, "data_ptr") and img.is_cuda and img.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous CUDA tensor of W x H uchar4 pixels, or a _DeviceImage")
        if img.numel() * img.element_size() != nbytes:
            raise ValueError(f"{what} holds {img.numel() * img.element_size()} bytes, W x H x 4 is {nbytes}")
        return img.data_ptr(), True

    def score_frames(self, params, a=None, b=None, cover_a=None, cover_b=None, download_map: bool = False):
        """m2s_score_frames: image `b` (under test: the splats) against image `a` (the reference: the mesh), with their coverage planes.
        Each is None (the context's own: the mesh frame, the frame, the albedo attachments of the mesh and splat G-buffers), a contiguous
        CUDA torch tensor of W x H uchar4 pixels (row 0 = bottom), or a _DeviceImage.  `params`: mesh2splat_amd.score.ScoreParams.
        -> ScoreResult; with download_map (and params.want_map) its error_map is the (H, W, 4) uint8 map."""
        from . import score as _sc
        pc = _sc.to_c(params)
        W, H = int(pc.resolution[0]), int(pc.resolution[1])
        ptrs, tensors = [], False
        for img, what in ((a, "a"), (b, "b"), (cover_a, "cover_a"), (cover_b, "cover_b")):
            ptr, is_tensor = self._image_ptr(img, what, max(W, 0) * max(H, 0) * 4)
            ptrs.append(ptr)
            tensors = tensors or is_tensor
        if tensors:                                     # the context's stream does not wait for torch's
            import torch
            torch.cuda.current_stream().synchronize()
        out = _sc.ScoreResultC()
        self._check(self._L.m2s_score_frames(self._h, C.byref(pc), ptrs[0], ptrs[1], ptrs[2], ptrs[3], C.byref(out)))
        res = _sc.ScoreResult.from_c(out)
        if download_map:
            res.error_map = self.download_score_map(W, H)
        return res

    def download_score_map(self, W: int, H: int) -> np.ndarray:
        """The error map of the last score_frames (params.want_map): (H, W, 4) uint8, row 0 = bottom."""
        m = np.empty((int(H), int(W), 4), np.uint8)
        self._check(self._L.m2s_download_score_map(self._h, m.ctypes.data, m.nbytes))
        return m

    @property
    def device_score_map(self) -> int:
        return int(self._L.m2s_device_score_map(self._h) or 0)

    @property
    def last_score_ms(self) -> float:
        return float(self._L.m2s_last_score_ms(self._h))

    def score(self, prepass_params, light_params, mask_mode: int = 2, mesh_depth_test: bool = False, want_map: bool = False):
        """How close the splats of the context's records look to the uploaded mesh through one camera: the frame of render_frame() for
        the splats, mesh_render() + relight_mesh() for the mesh, and score_frames() over the context's own buffers (coverage: the albedo
        attachments of the two G-buffers).  Nothing but the result leaves the device.  -> ScoreResult (want_map: with its error_map)."""
        from . import score as _sc
        self.render_frame(prepass_params, light_params, mesh_depth_test=mesh_depth_test, download=False)
        self.mesh_render(prepass_params, download=False)
        self.relight_mesh(light_params, download=False)
        res = tuple(int(v) for v in prepass_params.renderer_resolution)
        return self.score_frames(_sc.ScoreParams(res, int(mask_mode), False, bool(want_map)), download_map=bool(want_map))

    def score_views(self, cameras, resolution_target: int, light_position, light_intensity: float, gaussian_std: float = 0.65,
                    render_mode: int = 6, shadow_resolution: int = 1024, mask_mode: int = 2, mesh_depth_test: bool = False):
        """score() through each of `cameras` (mesh2splat_amd.score.OrbitCamera, e.g. orbit_cameras(scene, K, W, H)), the frames built as the
        command line's --score builds them (OrbitCamera.frame_params).  -> (per-view ScoreResults, the pooled ScoreResult: the integers
        added, the ratios derived from the sums).  `resolution_target` divides the records' scales: pass `self.resolution` (the R of
        the conversion, 1 after to_world_units())."""
        from . import score as _sc
        views = [self.score(*cam.frame_params(resolution_target, light_position, light_intensity, gaussian_std, render_mode, shadow_resolution),
                            mask_mode=mask_mode, mesh_depth_test=mesh_depth_test) for cam in cameras]
        return views, _sc.pool(views)

    # ---- contribution pass and pruning (m2s_contrib_*, m2s_prune) ---------------------------------------------------------------------
    @property
    def device_sorted_sources(self) -> int:
        """Device address of uint32[visible], the record every sorted quad of the last prepass_sorted() was made from; 0 when the sorted
        quads carry none (m2s_device_sorted_sources)."""
        return int(self._L.m2s_device_sorted_sources(self._h) or 0)

    def download_sorted_sources(self, n: int) -> np.ndarray:
        """-> uint32[n], the sources of the context's n sorted quads (m2s_download_sorted_sources)."""
        out = np.empty(int(n), np.uint32)
        self._check(self._L.m2s_download_sorted_sources(self._h, out.ctypes.data, out.size))
        return out

    def upload_quad_sources(self, sources):
        """The counterpart of upload_quads() for the sources: one record index per sorted quad (m2s_upload_quad_sources)."""
        s = np.ascontiguousarray(sources, np.uint32).reshape(-1)
        self._check(self._L.m2s_upload_quad_sources(self._h, s.ctypes.data if s.size else None, s.size))

    def contrib_begin(self):
        """Size the two per-record accumulators to the context's current records and zero them (m2s_contrib_begin)."""
        self._check(self._L.m2s_contrib_begin(self._h))

    def contrib_accumulate(self, params, count_weight: float = 1.0 / 255.0):
        """What every record adds to the picture of the context's sorted quads (prepass_sorted()) at `params` (SplatParams), added to the
        accumulators: wmax, the largest fragment weight, and npix, the fragments with weight > count_weight (m2s_contrib_accumulate)."""
        from . import splat as _sp
        pc = _sp.to_c(params)
        self._check(self._L.m2s_contrib_accumulate(self._h, C.byref(pc), C.c_float(count_weight)))

    def download_contrib(self):
        """-> (wmax, npix): float32[n] (the weights themselves; .view(np.uint32) gives the accumulated bits) and uint32[n]."""
        n = self.num_stored
        w = np.empty(n, np.float32)
        k = np.empty(n, np.uint32)
        self._check(self._L.m2s_download_contrib(self._h, w.ctypes.data, k.ctypes.data, n))
        return w, k

    def device_contrib(self, which: int) -> int:
        return int(self._L.m2s_device_contrib(self._h, int(which)) or 0)

    @property
    def last_contrib_ms(self) -> float:
        return float(self._L.m2s_last_contrib_ms(self._h))

    def last_contrib_stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_contrib_stage_ms(self._h, ms))
        return {"setup_bin": float(ms[0]), "grouping": float(ms[1]), "blend": float(ms[2])}

    def prune(self, min_weight: float = 0.0, min_pixels: int = 0) -> dict:
        """Keep the records with wmax > min_weight and npix >= min_pixels (m2s_prune): the survivors become the context's records, in
        order.  -> {"before", "kept", "dropped_weight", "dropped_pixels"}."""
        from . import prune as _pr
        pc = _pr.PruneParamsC(float(min_weight), int(min_pixels), 0)
        kept = C.c_uint64()
        had_plane = bool(self.device_sh)
        self._check(self._L.m2s_prune(self._h, C.byref(pc), C.byref(kept)))
        counts = self.last_prune_counts()
        if had_plane and getattr(self, "_last_bake_n", None) == counts["before"]:
            self._last_bake_n = counts["kept"]          # (the baked plane of these records was compacted with them)
        return counts

    def last_prune_counts(self) -> dict:
        v = (C.c_uint64 * 4)()
        self._check(self._L.m2s_last_prune_counts(self._h, v))
        return {"before": int(v[0]), "kept": int(v[1]), "dropped_weight": int(v[2]), "dropped_pixels": int(v[3])}

    @property
    def last_prune_ms(self) -> float:
        return float(self._L.m2s_last_prune_ms(self._h))

    def upload_contrib(self, wmax=None, npix=None):
        """After contrib_begin(): the two accumulators from host arrays of num_stored words each (m2s_upload_contrib) — wmax as float32
        weights in [0, 1] or as their uint32 bits, npix as uint32; None leaves that accumulator as it is.  wmax of a floating type is
        rounded to float32 and its bits are taken; any other array must be of an unsigned integer type that fits 32 bits (TypeError
        otherwise: a weight must not silently become the word 0)."""
        def words(a, weights: bool):
            if a is None:
                return None
            a = np.asarray(a)
            if weights and a.dtype.kind == "f":
                a = np.ascontiguousarray(a, np.float32).view(np.uint32)
            elif a.dtype.kind != "u" or a.dtype.itemsize > 4:
                raise TypeError(("wmax takes float weights or uint32 bits" if weights else "npix takes unsigned integers of at most 32 bits") +
                                f", not {a.dtype}")
            return np.ascontiguousarray(a, np.uint32).reshape(-1)
        w, k = words(wmax, True), words(npix, False)
        for a in (w, k):
            if a is not None and a.size != self.num_stored:
                raise ValueError("an accumulator has one word per record")
        self._check(self._L.m2s_upload_contrib(self._h, w.ctypes.data if w is not None and w.size else None,
                                               k.ctypes.data if k is not None and k.size else None, self.num_stored))

    def prune_budget(self, max_records: int, importance: str = "views", min_weight: float = 0.0, min_pixels: int = 0) -> dict:
        """Of the records that pass the thresholds, keep the max_records with the largest importance, ties by index (m2s_prune_budget;
        the pin is in include/m2s.h).  "views": importance npix * wmax over the accumulated views, the thresholds are prune()'s; "area":
        |scale x| * |scale y| * alpha of every record, no accumulators needed, the thresholds are not read.  The survivors become the
        context's records, in order.  -> {"before", "candidates", "kept", "threshold_key", "ties_kept", "ties"}."""
        from . import prune as _pr
        pc = _pr.BudgetParamsC(int(max_records), float(min_weight), int(min_pixels), _pr.IMPORTANCE[importance], 0)
        kept = C.c_uint64()
        had_plane = bool(self.device_sh)
        self._check(self._L.m2s_prune_budget(self._h, C.byref(pc), C.byref(kept)))
        counts = self.last_budget_counts()
        if had_plane and getattr(self, "_last_bake_n", None) == counts["before"]:
            self._last_bake_n = counts["kept"]          # (the baked plane of these records was compacted with them)
        return counts

    def last_budget_counts(self) -> dict:
        from . import prune as _pr
        v = (C.c_uint64 * 6)()
        self._check(self._L.m2s_last_budget_counts(self._h, v))
        return {name: int(v[k]) for k, name in enumerate(_pr.BUDGET_COUNTS)}

    def last_budget_stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_budget_stage_ms(self._h, ms))
        return {"select": float(ms[0]), "flags_scans": float(ms[1]), "compact": float(ms[2])}

    def prune_views(self, cameras, resolution_target: int, size=None, gaussian_std: float = 0.65, count_weight: float = 1.0 / 255.0,
                    min_weight: float = 1.0 / 255.0, min_pixels: int = 1, budget=None) -> dict:
        """prepass_sorted() -> contrib_accumulate() through each of `cameras` (mesh2splat_amd.prune.orbit_cameras), then prune().
        `size`: (W, H) at which every view is taken instead of the camera's own resolution (the cameras' projections are kept, so keep their
        aspect ratio; default: each camera's resolution).  -> the counts of prune().  `budget`: an integer makes the final call
        prune_budget(budget, "views") with the same thresholds -> its counts.  `resolution_target` divides the records' scales: pass
        `self.resolution` (the R of the conversion, 1 after to_world_units())."""
        import dataclasses
        from . import splat as _sp
        if size is not None:
            size = (int(size[0]), int(size[1]))
        self.contrib_begin()
        for cam in cameras:
            pp, _ = cam.frame_params(resolution_target, (0.0, 0.0, 0.0), 0.0, gaussian_std)
            if size is not None:
                pp = dataclasses.replace(pp, renderer_resolution=size)
            if self.prepass_sorted(pp, download=False):
                self.contrib_accumulate(_sp.SplatParams(tuple(pp.renderer_resolution), 0), count_weight)
        if budget is not None:
            return self.prune_budget(int(budget), "views", min_weight, min_pixels)
        return self.prune(min_weight, min_pixels)

    # ---- merge pass (m2s_merge) ----------------------------------------------------------------------------------------------------------
    def merge(self, level: int, max_group: int = 4, min_axis_dot: float = 0.5, dry_run: bool = False, unsigned_axis: bool = False) -> dict:
        """Replace every group of neighbouring records by its moment-matched parent (m2s_merge; the pin is in include/m2s.h): neighbours
        share a Morton cell of 2^level per axis (level 0..10), a parent takes at most max_group (2..64) members, and a run of members
        breaks where the third axes of two neighbours have a dot product below min_axis_dot.  The parents become the context's
        records, in segment order; sorted quads, accumulators and a baked SH plane are invalid.  dry_run: nothing changes, only the
        counts are produced.  max_group = 4 and min_axis_dot = 0.5 are untuned guesses.  unsigned_axis (M2S_MERGE_UNSIGNED_AXIS): the sign
        of the third axis carries no meaning, as for the viewer — a run breaks where |dot| is below min_axis_dot and the members' axes
        are turned onto one side before they are averaged; a conversion stores the two triangles of a flat quad with opposite signs.
        With carry_sh on and an SH plane of the records, the plane is merged too (pin 5s: the alpha-and-area-weighted mean of every
        coefficient, the rule of the colour) and stays valid for the parents; last_merge_sh_ms is what that cost.
        -> {"before", "after", "merged": parents of two members or more, "invalid": invalid records carried}."""
        from . import merge as _mg
        pc = _mg.to_c(level, max_group, min_axis_dot, dry_run, unsigned_axis)
        v = (C.c_uint64 * 4)()
        self._check(self._L.m2s_merge(self._h, C.byref(pc), v))
        return {name: int(v[k]) for k, name in enumerate(_mg.COUNTS)}

    def merge_count(self, level: int, max_group: int = 4, min_axis_dot: float = 0.5, unsigned_axis: bool = False) -> int:
        """The number of records merge() with these parameters would leave (a dry run)."""
        return self.merge(level, max_group, min_axis_dot, dry_run=True, unsigned_axis=unsigned_axis)["after"]

    def merge_to_budget(self, max_records: int, max_group: int = 4, min_axis_dot: float = 0.5, unsigned_axis: bool = False) -> dict:
        """merge() at the finest level whose dry-run count is <= max_records (the counts are monotone in level: a bisection over
        0..10; records that fit already are merged at level 0, where only records of one 1 / 1024 cell meet).  Where even level 10
        leaves more, level 10 is merged and "met" is False.  -> merge()'s counts + {"level", "met"}."""
        from . import merge as _mg
        max_records = int(max_records)
        if max_records < 1:
            raise ValueError("max_records must be at least 1")
        lo, hi = 0, _mg.MAX_LEVEL                         # the finest level in [lo, hi] that meets the budget, if hi does
        met = self.merge_count(hi, max_group, min_axis_dot, unsigned_axis) <= max_records
        if met:
            while lo < hi:
                mid = (lo + hi) // 2
                if self.merge_count(mid, max_group, min_axis_dot, unsigned_axis) <= max_records:
                    hi = mid
                else:
                    lo = mid + 1
        out = self.merge(hi, max_group, min_axis_dot, unsigned_axis=unsigned_axis)
        out.update(level=hi, met=met)
        return out

    def last_merge_counts(self) -> dict:
        from . import merge as _mg
        v = (C.c_uint64 * 4)()
        self._check(self._L.m2s_last_merge_counts(self._h, v))
        return {name: int(v[k]) for k, name in enumerate(_mg.COUNTS)}

    def last_merge_stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_merge_stage_ms(self._h, ms))
        return {"keys_sort": float(ms[0]), "heads_scans": float(ms[1]), "reduce": float(ms[2])}

    @property
    def last_merge_sh_ms(self) -> float:
        """The SH reduction of the last merge() (ms; 0.0 where none ran): a part of last_merge_stage_ms()["reduce"]."""
        return float(self._L.m2s_last_merge_sh_ms(self._h))

    @property
    def device_merge_map(self) -> int:
        return int(self._L.m2s_device_merge_map(self._h) or 0)

    def download_merge_map(self) -> np.ndarray:
        """uint32 per record of the order before the last merge(): the index of its parent afterwards (m2s_download_merge_map).  Valid
        until the records change again."""
        n = C.c_uint64()
        self._check(self._L.m2s_download_merge_map(self._h, None, 0, C.byref(n)))
        out = np.empty(int(n.value), np.uint32)
        if out.size:
            self._check(self._L.m2s_download_merge_map(self._h, out.ctypes.data, out.size, None))
        return out

    # ---- level-of-detail tree and its cut (m2s_lod_*) ------------------------------------------------------------------------------------
    def lod_build(self, levels=(1, 2, 3, 4, 5, 6, 7, 8), max_group: int = 4, min_axis_dot: float = 0.5, unsigned_axis: bool = False) -> dict:
        """Build the resident level-of-detail tree over the context's current records (m2s_lod_build; the pin is in include/m2s.h): they
        are the leaves, and step s merges what the previous step left at merge level levels[s] (0..10, non-decreasing, at most 16) with
        merge()'s max_group, min_axis_dot and unsigned_axis; every step that merges something adds a tree level.  The coarsest level is the context's
        records afterwards; the tree is a copy and outlives them.  The default chain is an untuned guess, like max_group and min_axis_dot.
        With carry_sh on and an SH plane of the records, the tree also owns a plane of its nodes (download_lod_sh; 192 bytes per node)
        and every cut through it leaves the selected nodes' rows as the context's plane; a tree built otherwise has none.
        -> {"leaves", "nodes", "levels": tree levels, the leaves included, "skipped": steps that merged nothing, "first": first node of
        every level and the node count behind them}."""
        from . import lod as _ld
        pc = _ld.build_to_c(levels, max_group, min_axis_dot, unsigned_axis)
        v = (C.c_uint64 * 4)()
        self._check(self._L.m2s_lod_build(self._h, C.byref(pc), v))
        out = {name: int(v[k]) for k, name in enumerate(_ld.BUILD_COUNTS)}
        out["first"] = self.lod_levels()
        return out

    def lod_levels(self) -> list:
        """First node of every tree level, then the node count: len() - 1 levels (m2s_lod_levels)."""
        from . import lod as _ld
        n = C.c_uint32()
        first = (C.c_uint64 * (_ld.MAX_STEPS + 2))()
        st = self._L.m2s_lod_levels(self._h, C.byref(n), first)
        if st:
            raise _lib.M2SError(st, "no level-of-detail tree (lod_build)")
        return [int(first[k]) for k in range(n.value + 1)]

    def _lod_frustum_counts(self, out: dict) -> None:
        from . import lod as _ld
        fc = (C.c_uint64 * 2)()
        self._check(self._L.m2s_last_lod_frustum_counts(self._h, fc))
        out.update({name: int(fc[k]) for k, name in enumerate(_ld.FRUSTUM_COUNTS)})

    def last_lod_occlusion_counts(self) -> dict:
        """Of the last lod_select() / lod_select_budget() with an occluder, a dry run included (m2s_last_lod_occlusion_counts):
        {"visible_leaves": leaves inside the frustum, "occluded_leaves": of those, hidden by the depth image, "translucent_kept": of
        those inside, behind the image but kept for an alpha <= .95 or NaN, "culled": nodes the plain cut selects and this one dropped}."""
        from . import lod as _ld
        oc = (C.c_uint64 * 4)()
        self._check(self._L.m2s_last_lod_occlusion_counts(self._h, oc))
        return {name: int(oc[k]) for k, name in enumerate(_ld.OCCLUSION_COUNTS)}

    def lod_select(self, camera_position, focal_px: float, tau_px: float = 1.0, near: float = 1e-3, dry_run: bool = False,
                   frustum=None, occluder=None, blend=None) -> dict:
        """Take the cut through the tree for a camera at `camera_position` (world space) whose projection has `focal_px` pixels per unit
        of tan(angle) (mesh2splat_amd.lod.focal_px, .camera_position): walking down from the coarsest level, a node is drawn as soon as
        its longer edge projects to at most tau_px pixels at its distance from the camera (at least `near`), or it is a leaf
        (m2s_lod_select; the pin is in include/m2s.h).  Every leaf is covered exactly once.  The selected nodes become the context's
        records, in node order; sorted quads, accumulators and a baked SH plane are invalid — unless the tree was built with carry_sh
        and has a plane: the selected nodes' rows are then the context's SH plane (download_sh, render_baked, export_ply_sh work on
        the cut), whatever carry_sh says at the time of the cut.  dry_run: only the counts.
        -> {"nodes", "selected", "selected_leaves", "refine", "per_level": selected nodes of every tree level}.
        frustum (a mesh2splat_amd.lod.LodFrustumC: lod.frustum_to_c, lod.frustum_of): only nodes with a leaf inside it are selected
        (m2s_lod_select_frustum), possibly none; the dict then also has "visible_leaves" and "culled", the nodes the plain cut selects
        and this one dropped.
        occluder (a mesh2splat_amd.lod.LodOccluderC: lod.occluder_to_c, lod.occluder_of_mesh_depth; needs a frustum): a leaf behind
        this depth image under the prepass's own depth test is not inside either (m2s_lod_select_occluded); the dict then also has
        "occluded_leaves" and "translucent_kept", and "visible_leaves" stays the leaves inside the frustum.  Run the prepass that
        follows with depth_test_mesh = 0: a merged node lies under the surface its leaves lie on.
        blend (a band, 0 < blend <= 1; None: none): after a cut that is no dry run, lod_blend() with the same camera, this tau_px and
        this band; the dict then also has "blend": lod_blend()'s dict."""
        from . import lod as _ld
        if occluder is not None and frustum is None:
            raise ValueError("an occluder needs a frustum")
        if blend is not None:
            _ld.blend_to_c(camera_position, focal_px, tau_px, near, blend)           # (a band outside (0, 1]: refused before the cut)
        pc = _ld.select_to_c(camera_position, focal_px, tau_px, near, dry_run)
        v = (C.c_uint64 * 4)()
        if frustum is None:
            self._check(self._L.m2s_lod_select(self._h, C.byref(pc), v))
        elif occluder is not None:
            self._check(self._L.m2s_lod_select_occluded(self._h, C.byref(pc), C.byref(frustum), C.byref(occluder), v))
        else:
            self._check(self._L.m2s_lod_select_frustum(self._h, C.byref(pc), C.byref(frustum), v))
        out = {name: int(v[k]) for k, name in enumerate(_ld.SELECT_COUNTS)}
        per = (C.c_uint64 * (_ld.MAX_STEPS + 1))()
        self._check(self._L.m2s_last_lod_level_counts(self._h, per))
        out["per_level"] = [int(per[k]) for k in range(len(self.lod_levels()) - 1)]
        if frustum is not None:
            self._lod_frustum_counts(out)
        if occluder is not None:
            out.update(self.last_lod_occlusion_counts())
        if blend is not None and not dry_run:
            out["blend"] = self.lod_blend(camera_position, focal_px, tau_px, near, blend)
        return out

    def lod_select_budget(self, camera_position, focal_px: float, max_records: int, tau_min_px: float = 0.0, near: float = 1e-3,
                          dry_run: bool = False, frustum=None, occluder=None, blend=None) -> dict:
        """Take the finest cut of lod_select() that holds at most `max_records` records for this camera, never finer than tau_min_px: the
        tau_px is found on the device, without a bisection on the host (m2s_lod_select_budget; the pin is in include/m2s.h).  A budget
        below the size of the coarsest level returns that level, with "met" False.  Everything else is lod_select()'s at the returned
        tau_px, the SH plane of a tree built with carry_sh included.  -> lod_select()'s dict plus {"tau_px": the float32 the cut was taken at, "met", "selected_finer": the records of the
        next finer cut, the one that did not fit (= "selected" where there is none or tau_min_px decided)}.
        frustum: as for lod_select(); the budget is then spent on the nodes the camera sees (m2s_lod_select_budget_frustum).
        occluder: as for lod_select(); ... and that no mesh hides (m2s_lod_select_budget_occluded).
        blend: as for lod_select(), with the tau_px the search returned."""
        from . import lod as _ld
        if occluder is not None and frustum is None:
            raise ValueError("an occluder needs a frustum")
        if blend is not None:
            _ld.blend_to_c(camera_position, focal_px, 0.0, near, blend)
        pc = _ld.budget_to_c(camera_position, focal_px, max_records, tau_min_px, near, dry_run)
        res = _ld.LodBudgetResultC()
        v = (C.c_uint64 * 4)()
        if frustum is None:
            self._check(self._L.m2s_lod_select_budget(self._h, C.byref(pc), C.byref(res), v))
        elif occluder is not None:
            self._check(self._L.m2s_lod_select_budget_occluded(self._h, C.byref(pc), C.byref(frustum), C.byref(occluder), C.byref(res), v))
        else:
            self._check(self._L.m2s_lod_select_budget_frustum(self._h, C.byref(pc), C.byref(frustum), C.byref(res), v))
        out = {name: int(v[k]) for k, name in enumerate(_ld.SELECT_COUNTS)}
        per = (C.c_uint64 * (_ld.MAX_STEPS + 1))()
        self._check(self._L.m2s_last_lod_level_counts(self._h, per))
        out["per_level"] = [int(per[k]) for k in range(len(self.lod_levels()) - 1)]
        out["tau_px"], out["met"], out["selected_finer"] = float(res.tau_px), bool(res.met), int(res.selected_finer)
        if frustum is not None:
            self._lod_frustum_counts(out)
        if occluder is not None:
            out.update(self.last_lod_occlusion_counts())
        if blend is not None and not dry_run:
            out["blend"] = self.lod_blend(camera_position, focal_px, out["tau_px"], near, blend)
        return out

    def lod_blend(self, camera_position, focal_px: float, tau_px: float, near: float = 1e-3, band: float = 1.0) -> dict:
        """Rewrite the records of the last cut (lod_select / lod_select_budget, any form, no dry run) in place so that they do not pop
        between levels: every record becomes its node at weight 1 - t and its node's parent at weight t, with t rising from 0 to 1
        over the upper `band` share of the node's interval of tau_px^2, and reaching 1 where the parent takes over (m2s_lod_blend; the
        pin is in include/m2s.h).  Pass the camera, focal_px and near of the cut and its tau_px (a budget cut: the "tau_px" it
        returned).  Which nodes are drawn, their order and download_lod_nodes() do not change; the SH plane of a tree built with
        carry_sh is blended with the records.  The source is the tree: calling it again, with another band too, starts afresh.
        -> {"records", "blended": t > 0, "saturated": t == 1, "turned": t > 0 and the parent's frame was turned to the child's}."""
        from . import lod as _ld
        pc = _ld.blend_to_c(camera_position, focal_px, tau_px, near, band)
        v = (C.c_uint64 * 4)()
        self._check(self._L.m2s_lod_blend(self._h, C.byref(pc), v))
        return {name: int(v[k]) for k, name in enumerate(_ld.BLEND_COUNTS)}

    def download_lod_blend_t(self) -> np.ndarray:
        """float32 per record the last lod_blend() left: its weight t (m2s_download_lod_blend_t).  Valid until the records change again."""
        n = C.c_uint64()
        self._check(self._L.m2s_download_lod_blend_t(self._h, None, 0, C.byref(n)))
        out = np.empty(int(n.value), np.float32)
        if out.size:
            self._check(self._L.m2s_download_lod_blend_t(self._h, out.ctypes.data, out.size, None))
        return out

    @property
    def device_lod_blend_t(self) -> int:
        return int(self._L.m2s_device_lod_blend_t(self._h) or 0)

    def last_lod_blend_ms(self) -> float:
        """The last lod_blend() on the device (ms)."""
        return float(self._L.m2s_last_lod_blend_ms(self._h))

    def last_lod_blend_stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_lod_blend_stage_ms(self._h, ms))
        return {"weights": float(ms[0]), "records": float(ms[1]), "sh": float(ms[2])}

    def download_lod(self, which: int) -> np.ndarray:
        """A plane of the tree (m2s_download_lod): 0 the node records (nodes, 24) float32, 1 parent (nodes,) uint32 with 0xFFFFFFFF on the
        last level, 2 the bounds (nodes, 4) float32: position and longer edge."""
        from . import lod as _ld
        dtype, row = _ld.PLANES[int(which)]
        nodes = self.lod_levels()[-1]
        out = np.empty((nodes, row) if row else (nodes,), dtype)
        self._check(self._L.m2s_download_lod(self._h, int(which), out.ctypes.data if out.size else None, out.nbytes))
        return out

    def device_lod(self, which: int) -> int:
        return int(self._L.m2s_device_lod(self._h, int(which)) or 0)

    def download_lod_sh(self):
        """The tree's SH plane (m2s_download_lod_sh) -> ((nodes, 48) float32 in node order, degree).  M2SError (M2S_ERR_STATE) for a tree
        built without carry_sh or without a plane."""
        nodes = self.lod_levels()[-1]
        out = np.empty((nodes, 48), np.float32)
        degree = C.c_uint32()
        self._check(self._L.m2s_download_lod_sh(self._h, out.ctypes.data if out.size else None, nodes, C.byref(degree)))
        return out, int(degree.value)

    @property
    def device_lod_sh(self) -> int:
        return int(self._L.m2s_device_lod_sh(self._h) or 0)

    @property
    def device_lod_nodes(self) -> int:
        return int(self._L.m2s_device_lod_nodes(self._h) or 0)

    def download_lod_nodes(self) -> np.ndarray:
        """uint32 per record the last lod_select() left: its node index in the tree (m2s_download_lod_nodes).  Valid until the records
        change again."""
        n = C.c_uint64()
        self._check(self._L.m2s_download_lod_nodes(self._h, None, 0, C.byref(n)))
        out = np.empty(int(n.value), np.uint32)
        if out.size:
            self._check(self._L.m2s_download_lod_nodes(self._h, out.ctypes.data, out.size, None))
        return out

    def lod_release(self):
        """Free the tree (m2s_lod_release); the context's records stay."""
        self._check(self._L.m2s_lod_release(self._h))

    @property
    def last_lod_build_ms(self) -> float:
        return float(self._L.m2s_last_lod_build_ms(self._h))

    def last_lod_select_stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_lod_select_stage_ms(self._h, ms))
        return {"sweep": float(ms[0]), "scan_ids": float(ms[1]), "compact": float(ms[2])}

    @property
    def last_lod_budget_stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_lod_budget_stage_ms(self._h, ms))
        return {"thresholds": float(ms[0]), "select": float(ms[1]), "cut": float(ms[2])}

    def last_lod_frustum_ms(self) -> float:
        """The visibility stage (ms) of the last profiled lod_select() / lod_select_budget() with a frustum."""
        return float(self._L.m2s_last_lod_frustum_ms(self._h))

    # ---- world units (m2s_records_to_world_units) ----------------------------------------------------------------------------------------
    @property
    def resolution(self) -> int:
        """The resolutionTarget of the context's current records, the divisor of their scales (m2s_last_resolution): the R of the
        conversion, 1 after to_world_units(), 0 for uploaded records (taken as 1).  The one place to take `resolution_target` from for
        prepass parameters, prune_views(), refit_views() and score_views()."""
        return int(self._L.m2s_last_resolution(self._h))

    def to_world_units(self) -> dict:
        """scale[0..2] of every record divided by the records' resolutionTarget R (correctly rounded fp32; every other word keeps its
        bits), after which `resolution` is 1 (m2s_records_to_world_units; the pin is in include/m2s.h).  merge(), lod_build() and
        lod_select() read scales as world lengths: on a conversion run this first, and tau_px counts screen pixels.  With R <= 1 nothing
        changes.  Otherwise the records live in the context's pool afterwards; sorted quads, accumulators, maps and a baked SH plane are
        invalid; a tree built earlier stays as it is.  -> {"records", "previous_R", "ms" (0 unless profiling is on)}."""
        prev = C.c_uint32(0)
        self._check(self._L.m2s_records_to_world_units(self._h, C.byref(prev)))
        ms = float(self._L.m2s_last_world_units_ms(self._h)) if prev.value > 1 else 0.0
        return {"records": self.num_stored, "previous_R": int(prev.value), "ms": ms}

    # ---- colour refit (m2s_refit_*) ---------------------------------------------------------------------------------------------------
    def refit_begin(self):
        """Size the four 64-bit accumulators per record (num[3], den) to the context's current records and zero them (m2s_refit_begin)."""
        self._check(self._L.m2s_refit_begin(self._h))

    def refit_accumulate(self, params, target=None, render=None) -> dict:
        """The colour error of `render` against `target` carried back to the records of the context's sorted quads (prepass_sorted()) at
        `params` (mesh2splat_amd.refit.RefitParams), added to the accumulators (m2s_refit_accumulate; the pin is in include/m2s.h).  Each
        plane is None (the albedo attachment of the mesh G-buffer / of the splat G-buffer), a contiguous CUDA torch tensor of W x H uchar4
        pixels (row 0 = bottom), or a _DeviceImage; `render` must have been splatted from these same quads in render mode 0 or 6.
        -> {"pixels": participating pixels, "pairs": (tile, quad) pairs}."""
        from . import refit as _rf
        pc = _rf.to_c(params)
        W, H = int(pc.resolution[0]), int(pc.resolution[1])
        ptrs, tensors = [], False
        for img, what in ((target, "target"), (render, "render")):
            ptr, is_tensor = self._image_ptr(img, what, max(W, 0) * max(H, 0) * 4)
            ptrs.append(ptr)
            tensors = tensors or is_tensor
        if tensors:                                     # the context's stream does not wait for torch's
            import torch
            torch.cuda.current_stream().synchronize()
        v = (C.c_uint64 * 2)()
        self._check(self._L.m2s_refit_accumulate(self._h, C.byref(pc), ptrs[0], ptrs[1], v))
        return {"pixels": int(v[0]), "pairs": int(v[1])}

    def download_refit(self):
        """-> (num, den): int64 (n, 3) and uint64 (n,) (m2s_download_refit)."""
        n = self.num_stored
        num = np.empty((n, 3), np.int64)
        den = np.empty(n, np.uint64)
        self._check(self._L.m2s_download_refit(self._h, num.ctypes.data, den.ctypes.data, n))
        return num, den

    def upload_refit(self, num=None, den=None):
        """After refit_begin(): the accumulators from host arrays — num int64 (n, 3), den uint64 (n,) for n = num_stored; None leaves
        that accumulator as it is (m2s_upload_refit)."""
        n = self.num_stored
        a = None if num is None else np.ascontiguousarray(num, np.int64).reshape(-1)
        d = None if den is None else np.ascontiguousarray(den, np.uint64).reshape(-1)
        if (a is not None and a.size != 3 * n) or (d is not None and d.size != n):
            raise ValueError("num holds three words per record and den one")
        self._check(self._L.m2s_upload_refit(self._h, a.ctypes.data if a is not None and a.size else None,
                                             d.ctypes.data if d is not None and d.size else None, n))

    def device_refit(self, which: int) -> int:
        return int(self._L.m2s_device_refit(self._h, int(which)) or 0)

    def refit_apply(self, step: float = 1.0, min_weight_sum: float = 1.0) -> dict:
        """color[0..2] += step * num / (den * 4096), clamped to [0, 1], for every record with den >= min_weight_sum * 65536
        (m2s_refit_apply).  The records live in the context's pool afterwards; sorted quads, accumulators and a baked SH plane are
        invalid.  -> {"records", "updated", "clamped", "no_weight"}."""
        from . import refit as _rf
        pc = _rf.RefitApplyParamsC(float(step), float(min_weight_sum))
        v = (C.c_uint64 * 4)()
        self._check(self._L.m2s_refit_apply(self._h, C.byref(pc), v))
        return {name: int(v[k]) for k, name in enumerate(_rf.APPLY_COUNTS)}

    def last_refit_stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_refit_stage_ms(self._h, ms))
        return {"setup_bin": float(ms[0]), "grouping": float(ms[1]), "blend": float(ms[2]), "apply": float(self._L.m2s_last_refit_apply_ms(self._h))}

    def refit_views(self, cameras, resolution_target: int, iterations: int = 2, step: float = 1.0, size=None, gaussian_std: float = 0.65,
                    min_cover: int = 128, min_weight_sum: float = 1.0) -> dict:
        """Refit the records' colours to the mesh render through `cameras` (mesh2splat_amd.prune.orbit_cameras).  Per iteration:
        refit_begin(), then per camera prepass_sorted() -> splat() in mode 0 -> mesh_render() in mode 0 -> refit_accumulate() over the
        two albedo attachments, then refit_apply(step, min_weight_sum).  Before every iteration and after the last the albedo error is
        pooled over the cameras: score_frames() over the two albedo attachments, mask 3 (covered by both).  `size`: as prune_views().
        The defaults min_cover = 128, min_weight_sum = 1.0 and iterations = 2 are guesses that nothing has tuned.  `resolution_target`
        divides the records' scales: pass `self.resolution` (the R of the conversion, 1 after to_world_units()).
        -> {"iterations", "views", "sse": [before, after iteration 1, ...] (the three channels added), "pixels": the same for the
        pixels compared, "updated", "clamped", "no_weight": per iteration}."""
        import dataclasses
        from . import refit as _rf
        from . import score as _sc
        from . import splat as _sp
        if size is not None:
            size = (int(size[0]), int(size[1]))
        cameras = list(cameras)
        out = {"iterations": int(iterations), "views": len(cameras), "sse": [], "pixels": [], "updated": [], "clamped": [], "no_weight": []}

        def view(cam, accumulate: bool):
            pp, _ = cam.frame_params(resolution_target, (0.0, 0.0, 0.0), 0.0, gaussian_std)
            if size is not None:
                pp = dataclasses.replace(pp, renderer_resolution=size)
            res = tuple(int(v) for v in pp.renderer_resolution)
            if not self.prepass_sorted(pp, download=False):
                return _sc.ScoreResult()                # (no splat covers a pixel: nothing passes mask 3, nothing to carry back)
            self.splat(_sp.SplatParams(res, 0), download=False)
            self.mesh_render(pp, download=False)
            r = self.score_frames(_sc.ScoreParams(res, _sc.MASK_A_AND_B), a=_DeviceImage(self.device_mesh_gbuffer(2), res[1], res[0]),
                                  b=_DeviceImage(self.device_gbuffer(2), res[1], res[0]))
            if accumulate:
                self.refit_accumulate(_rf.RefitParams(res, int(min_cover)))
            return r

        def pooled(results):
            p = _sc.pool(results)
            out["sse"].append(sum(p.sse))
            out["pixels"].append(p.pixels)

        for _ in range(int(iterations)):
            self.refit_begin()
            pooled([view(cam, True) for cam in cameras])
            counts = self.refit_apply(step, min_weight_sum)
            for k in ("updated", "clamped", "no_weight"):
                out[k].append(counts[k])
        pooled([view(cam, False) for cam in cameras])
        return out

    @property
    def last_shadow_ms(self) -> float:
        return float(self._L.m2s_last_shadow_ms(self._h))

    def last_shadow_stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self._L.m2s_last_shadow_stage_ms(self._h, ms))
        return {"quads": float(ms[0]), "bin": float(ms[1]), "raster": float(ms[2])}

    def last_shadow_counts(self) -> dict:
        v = (C.c_uint64 * 9)()
        self._check(self._L.m2s_last_shadow_counts(self._h, v))
        return {"quads_per_face": [int(v[k]) for k in range(6)], "pairs": int(v[6]), "texel_updates": int(v[7]), "skipped": int(v[8])}

    @property
    def last_relight_ms(self) -> float:
        return float(self._L.m2s_last_relight_ms(self._h))

    def set_pipeline(self, name: str):
        """'auto' (single-pass kernel or multi-pass pipeline, chosen per scene and R), 'multipass', or the single-pass
        kernel forced in one of its forms: 'team' (k_fused2, workgroup-cooperative), 'lean' (k_fused3), 'sparse' (k_sparse)."""
        self._check(self._L.m2s_set_pipeline(self._h, {"auto": 0, "multipass": 1, "team": 3, "sparse": 4, "lean": 5}[name]))

    def set_async_lanes(self, lanes: int):
        """2: context-owned submissions alternate between two streams / chains / record buffers and overlap."""
        self._check(self._L.m2s_set_async_lanes(self._h, int(lanes)))

    @property
    def last_pipeline(self) -> str:
        """What the last conversion ran: 'multipass', 'team' (k_fused2), 'lean' (k_fused3) or 'sparse' (k_sparse)."""
        return {0: "none", 1: "multipass", 3: "team", 4: "sparse", 5: "lean"}[self._L.m2s_last_pipeline(self._h)]

    def vertex_table(self) -> dict:
        """The last upload's vertex table: {'rows': distinct vertices among the resident corners (0: not counted), 'in_use': whether
        conversions in the lean form gather from it (the indexed instance of k_fused3) instead of the per-corner planes}."""
        rows, used = C.c_uint64(0), C.c_int(0)
        self._check(self._L.m2s_vertex_table(self._h, C.byref(rows), C.byref(used)))
        return {"rows": int(rows.value), "in_use": bool(used.value)}

    def geo_planes(self) -> dict:
        """The last upload's geometry planes (Quaternion, Scale and orthogonal UVs per resident triangle, 48 bytes): {'bytes': their size
        (0: not built), 'in_use': whether conversions in the lean form read them (the kGeo instances of k_fused3) instead of computing
        the triangle setup from the positions}."""
        nbytes, used = C.c_uint64(0), C.c_int(0)
        self._check(self._L.m2s_geo_planes(self._h, C.byref(nbytes), C.byref(used)))
        return {"bytes": int(nbytes.value), "in_use": bool(used.value)}

    # -- measurement --------------------------------------------------------------------------------
    def set_profiling(self, on: bool):
        self._check(self._L.m2s_set_profiling(self._h, 1 if on else 0))

    def last_kernel_ms(self) -> dict:
        ms = (C.c_float * len(_lib.KERNEL_NAMES))()
        self._check(self._L.m2s_last_kernel_ms(self._h, ms))
        return {k: float(ms[i]) for i, k in enumerate(_lib.KERNEL_NAMES)}


def write_ply(path: str, records: np.ndarray, fmt: int, scale_multiplier: float):
    """parsers::savePlyVector (parsers.cpp:631-651) on a host array of 96-byte records."""
    r = np.ascontiguousarray(records, np.float32)
    if r.ndim != 2 or r.shape[1] != RECORD_FLOATS:
        raise ValueError("records must be (n, 24) float32")
    st = _lib.load().m2s_write_ply(os.fsencode(path), r.ctypes.data, r.shape[0], int(fmt), float(scale_multiplier))
    if st != _lib.M2S_OK:
        raise _lib.M2SError(st, f"could not write {path}")


def write_ply_compact(path: str, records: np.ndarray, scale_multiplier: float, sh: np.ndarray | None = None, sh_degree: int = 0) -> dict:
    """m2s_write_ply_compact: the compact .ply of a host array of 96-byte records, on the CPU.  sh: (n, 48) float32 as download_sh() gives
    it, of degree sh_degree.  -> {"rows", "chunks", "skipped"}."""
    r = np.ascontiguousarray(records, np.float32).reshape(-1, RECORD_FLOATS)
    p = None
    if sh is not None:
        p = np.ascontiguousarray(sh, np.float32)
        if p.shape != (r.shape[0], 48):
            raise ValueError("sh must be (n, 48) float32")
    counts = (C.c_uint64 * 3)()
    st = _lib.load().m2s_write_ply_compact(os.fsencode(path), r.ctypes.data if r.size else None, p.ctypes.data if p is not None else None,
                                           int(sh_degree), r.shape[0], float(scale_multiplier), counts)
    if st != _lib.M2S_OK:
        raise _lib.M2SError(st, f"could not write {path}")
    return {"rows": int(counts[0]), "chunks": int(counts[1]), "skipped": int(counts[2])}


def write_ply_slice(path: str, records: np.ndarray, fmt: int, scale_multiplier: float, first_row: int, total_rows: int):
    """One of several writers of one .ply (m2s_write_ply_slice): rows [first_row, first_row + len(records))."""
    r = np.ascontiguousarray(records, np.float32).reshape(-1, RECORD_FLOATS)
    st = _lib.load().m2s_write_ply_slice(os.fsencode(path), r.ctypes.data, r.shape[0], int(fmt), float(scale_multiplier),
                                         int(first_row), int(total_rows))
    if st != _lib.M2S_OK:
        raise _lib.M2SError(st, f"could not write {path}")


# ---------------------------------------------------------------------------------------------------
# reference-shaped interface
# ---------------------------------------------------------------------------------------------------
class RenderContext:
    """The slice of RenderContext (RenderContext.hpp:28-124) that the conversion path touches."""

    def __init__(self, scene: Optional[Scene] = None, resolutionTarget: int = 520, gaussianStd: float = 0.65,
                 device: int = 0):
        self.scene = scene                        # dataMeshAndGlMesh + meshToTextureData
        self.resolutionTarget = int(resolutionTarget)  # main.cpp:26 default quality 0.5 -> 520
        self.gaussianStd = float(gaussianStd)     # main.cpp:26
        self.numberOfGaussians = 0                # written by ConversionPass::execute
        self.device = int(device)
        self.converter: Optional[Converter] = None  # owns gaussianBuffer (the SSBO equivalent)
        self.rendererResolution = (1280, 720)     # RenderContext::rendererResolution (GaussianSplattingPass)
        self.renderMode = 0                       # RenderContext::renderMode
        self.gBuffer = None                       # written by GaussianSplattingPass::execute: the five planes
        self.splatSkipped = 0
        self.prepassParams = None                 # what GaussiansPrepass read: a mesh2splat_amd.prepass.PrepassParams (the shadow pass's per-record inputs)
        self.lightParams = None                   # RenderContext::pointLightData + camera: a mesh2splat_amd.light.LightParams
        self.shadowCubemap = None                 # written by GaussianShadowPass::execute: (6, S, S) float32
        self.mesh_depth = None                    # written by DepthPrepass::execute: (H, W) float32 window-space depth, row 0 = bottom
        self.frame = None                         # written by GaussianRelightingPass::execute: (H, W, 4) uint8, row 0 = bottom
        self.meshGBuffer = None                   # written by MeshRenderPass::execute: five planes, as gBuffer
        self.splitScreenEnabled = False           # RenderContext::splitScreenEnabled / splitScreenPosition (GaussianRelightingPass)
        self.splitScreenPosition = 0.5
        self._uploaded_scene = None


class IRenderPass:
    """RenderPass.hpp:11-29."""

    def __init__(self):
        self._enabled = False

    def execute(self, context: RenderContext):
        raise NotImplementedError

    def isEnabled(self) -> bool:
        return self._enabled

    def setIsEnabled(self, enabled: bool):
        self._enabled = bool(enabled)


class ConversionPass(IRenderPass):
    """ConversionPass::execute (ConversionPass.cpp:9-68): synchronous; leaves the Gaussians in the
    context's device buffer and their count in context.numberOfGaussians (not clamped to the cap)."""

    def execute(self, context: RenderContext):
        if context.scene is None:
            raise ValueError("RenderContext.scene is not set (SceneManager::loadModel has not run)")
        if context.converter is None:
            context.converter = Converter(context.device)
        if context._uploaded_scene is not context.scene:
            context.converter.set_resolution_hint(context.resolutionTarget)   # the upload prepares for the conversion below
            context.converter.upload_scene(context.scene)
            context._uploaded_scene = context.scene
        context.numberOfGaussians = context.converter.convert(context.resolutionTarget)


class DepthPrepass(IRenderPass):
    """DepthPrepass::execute (DepthPrepass.cpp:8-50): the opaque meshes of the uploaded scene drawn depth-only with the camera of
    context.prepassParams.  The image ends up in context.mesh_depth ((H, W) float32, row 0 = bottom) and, when
    context.prepassParams.perform_mesh_depth_test is set, in context.prepassParams.mesh_depth — where Converter.prepass picks it up."""

    def execute(self, context: RenderContext):
        if context.converter is None or context.prepassParams is None or context._uploaded_scene is None:
            raise RuntimeError("needs an uploaded scene (ConversionPass) and context.prepassParams")
        context.mesh_depth, _ = context.converter.mesh_depth(context.prepassParams)
        if context.prepassParams.perform_mesh_depth_test:
            context.prepassParams.mesh_depth = context.mesh_depth


class MeshRenderPass(IRenderPass):
    """MeshRenderPass::execute (MeshRenderPass.cpp:8-73): every mesh of the uploaded scene drawn with the camera of
    context.prepassParams (its render mode and planes included) into the mesh G-buffer; the planes end up in context.meshGBuffer."""

    def execute(self, context: RenderContext):
        if context.converter is None or context.prepassParams is None or context._uploaded_scene is None:
            raise RuntimeError("needs an uploaded scene (ConversionPass) and context.prepassParams")
        context.meshGBuffer, _ = context.converter.mesh_render(context.prepassParams)


class GaussianSplattingPass(IRenderPass):
    """GaussianSplattingPass::execute (GaussianSplattingPass.cpp:50-95): blends the sorted quads (what RadixSortPass left in the
    context: Converter.sort_prepass / prepass_sorted / upload_quads) into the G-buffer at context.rendererResolution with
    context.renderMode.  The five planes end up in context.gBuffer as (H, W, 4) arrays, row 0 = bottom, in attachment order
    position, normal, albedo, depth, metallic-roughness (renderer.cpp:325-380)."""

    def execute(self, context: RenderContext):
        from .splat import SplatParams
        if context.converter is None:
            raise RuntimeError("no quads: run the conversion, the prepass and the depth sort first")
        res = getattr(context, "rendererResolution", (1280, 720))
        mode = getattr(context, "renderMode", 0)
        context.gBuffer, context.splatSkipped = context.converter.splat(SplatParams(renderer_resolution=tuple(res), render_mode=int(mode)))


class GaussianShadowPass(IRenderPass):
    """GaussianShadowPass::execute (GaussianShadowPass.cpp:83-236): the context's records through the six cameras of
    context.lightParams into the shadow cube (context.shadowCubemap, (6, S, S) float32).  context.prepassParams carries the
    per-record inputs (model matrix, gaussianStd, resolutionTarget, format, rendererResolution)."""

    def execute(self, context: RenderContext):
        if context.converter is None or context.prepassParams is None or context.lightParams is None:
            raise RuntimeError("needs converted records, context.prepassParams and context.lightParams")
        _, _, context.shadowCubemap = context.converter.shadow(context.prepassParams, context.lightParams)


class GaussianRelightingPass(IRenderPass):
    """GaussianRelightingPass::execute (GaussianRelightingPass.cpp:83-143): lights the G-buffer of GaussianSplattingPass with the
    cube of GaussianShadowPass; the RGBA8 frame ends up in context.frame (row 0 = bottom).  With context.splitScreenEnabled and a mesh
    G-buffer (MeshRenderPass has run) the left of context.splitScreenPosition is lit from the mesh G-buffer, as in the reference."""

    def execute(self, context: RenderContext):
        if context.converter is None or context.lightParams is None:
            raise RuntimeError("needs a G-buffer, a shadow cube and context.lightParams")
        if context.splitScreenEnabled and context.meshGBuffer is not None:
            r = context.converter.relight_split(context.lightParams, context.splitScreenPosition)
        else:
            r = context.converter.relight(context.lightParams)
        context.frame = r[0] if isinstance(r, tuple) else r


class SceneManager:
    """The export half of SceneManager (SceneManager.cpp:651-678)."""

    def __init__(self, context: RenderContext):
        self.renderContext = context

    def exportPly(self, outputFile: str, exportFormat: int = 0):
        ctx = self.renderContext
        if ctx.converter is None:
            raise RuntimeError("nothing converted yet")
        ctx.converter.export_ply(outputFile, exportFormat, ctx.gaussianStd)
