"""Python mirror of the reference's ``Renderer`` (tp2/projets/renderer/renderer.h:20-355)
and of ``render(Renderer&)`` (tp2/projets/utils/mainUtils.cpp:6-21), backed by the
HIP library through its C ABI (include/rt_mi355x.h).  Method names, argument
meaning and call order follow the reference; errors raise :class:`RtError`
instead of asserting or invoking undefined behaviour.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import RtSettings, RtStats, check, f32, ptr
from .scene import RenderSettings, SceneData, SHAPE_SPHERE, TEX_AO, TEX_DIFFUSE, TEX_NORMAL, TEX_DISPLACEMENT, \
    TEX_ROUGHNESS, TEX_SKYSPHERE

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)


def _to_c(st: RenderSettings) -> RtSettings:
    c = RtSettings()
    _lib.lib().rt_default_settings(C.byref(c))
    for name, typ in RtSettings._fields_:
        if hasattr(st, name):
            v = getattr(st, name)
            setattr(c, name, float(v) if typ is C.c_float else int(v))
    return c


def _from_c(c: RtSettings) -> RenderSettings:
    st = RenderSettings()
    for name, typ in RtSettings._fields_:
        if hasattr(st, name):
            v = getattr(c, name)
            cur = getattr(st, name)
            setattr(st, name, bool(v) if isinstance(cur, bool) else (float(v) if typ is C.c_float else int(v)))
    return st


class Renderer:
    """One renderer on one GPU (HIP device ordinal ``device``)."""

    def __init__(self, device: int = 0, settings: Optional[RenderSettings] = None):
        L = _lib.lib()
        self._h = L.rt_create(int(device))
        if not self._h:
            raise RuntimeError(f"rt_create({device}): {L.rt_last_error().decode()}")
        self.device = device
        if settings is not None:
            self.set_render_settings(settings)

    # -- lifetime -------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        return check(getattr(_lib.lib(), name)(self._h, *args), name)

    # -- settings (renderer.h:46, 118) ----------------------------------------------
    def render_settings(self) -> RenderSettings:
        c = RtSettings()
        self._call("rt_get_settings", C.byref(c))
        return _from_c(c)

    def set_render_settings(self, st: RenderSettings):
        c = _to_c(st)
        self._call("rt_set_settings", C.byref(c))

    def change_render_size(self, width: int, height: int):
        self._call("rt_change_render_size", int(width), int(height))

    def set_devices(self, ids):
        """rt_set_devices: render() uses every device in ids (ids[0] = this renderer's device),
        bands gathered to ids[0] with RCCL; an empty list returns to one device."""
        a = np.ascontiguousarray(list(ids), np.int32)
        self._call("rt_set_devices", ptr(a, _i32p) if len(a) else None, len(a))

    def finish_accel(self):
        """rt_finish_accel: wait for the background build of the leaf cones / slabs and the wide
        BVH (frames before it take the exact octree path)."""
        self._call("rt_finish_accel")

    def set_exact(self, on: bool = True):
        """Exact mode: every query walks the octree over the whole line, as
        the reference does, instead of the certified wide BVH."""
        self._call("rt_set_exact", 1 if on else 0)

    def set_device_build(self, on: bool = True):
        """rt_set_device_build: the octree of the next geometry changes is built on the
        GPU (the host build's bytes; inputs the device builder does not take build on the host)."""
        self._call("rt_set_device_build", 1 if on else 0)

    def device_builds(self) -> int:
        """rt_get_device_builds: device octree builds since the renderer was created."""
        n = C.c_int64()
        self._call("rt_get_device_builds", C.byref(n))
        return int(n.value)

    def device_wide_builds(self) -> int:
        """rt_get_device_wide_builds: quick wide BVHs built on the GPU (from a device-built octree) since the
        renderer was created."""
        n = C.c_int64()
        self._call("rt_get_device_wide_builds", C.byref(n))
        return int(n.value)

    # -- geometry (renderer.h:57-62) ------------------------------------------------
    def set_triangles(self, tri9, mat, uv6=None):
        tri9 = f32(tri9).reshape(-1, 9)
        mat = np.ascontiguousarray(mat, np.int32)
        uv = None if uv6 is None else f32(uv6).reshape(-1, 6)
        self._call("rt_set_triangles", ptr(tri9, _f32p), ptr(mat, _i32p), ptr(uv, _f32p), tri9.shape[0])

    @staticmethod
    def _stream_ptr(stream, device):
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(device)
        return C.c_void_p(int(stream.cuda_stream))

    def set_triangles_device(self, verts, mat, uv6=None, indices=None, stream=None):
        """rt_set_triangles_device: set_triangles with the positions read from GPU memory.  verts: a
        contiguous float32 torch tensor on this renderer's GPU, [n, 9], or [nv, 3] with indices int32
        [n, 3]; mat / uv6 host arrays as in set_triangles.  The copy runs in the order of ``stream`` (a
        torch stream; default the current one): verts and indices may be overwritten on it as soon as
        the call returns.  A non-finite coordinate or a bad index raises at the next frame."""
        vp, nv, ip, n = _lib.device_geometry_args(verts, indices, self.device)
        mat = np.ascontiguousarray(mat, np.int32).reshape(-1)
        uv = None if uv6 is None else f32(uv6).reshape(-1, 6)
        if mat.shape[0] != n or (uv is not None and uv.shape[0] != n):
            raise ValueError(f"set_triangles_device: {n} triangles but {mat.shape[0]} materials"
                             + ("" if uv is None else f" and {uv.shape[0]} texture coordinates"))
        self._call("rt_set_triangles_device", C.c_void_p(vp), nv, C.c_void_p(ip), ptr(mat, _i32p), ptr(uv, _f32p), n,
                   self._stream_ptr(stream, self.device))

    def update_vertices_device(self, verts, indices=None, stream=None):
        """rt_update_vertices_device: new positions for the current triangles from GPU memory (tensors
        and stream as in set_triangles_device); materials and texture coordinates stay."""
        vp, nv, ip, _ = _lib.device_geometry_args(verts, indices, self.device)
        self._call("rt_update_vertices_device", C.c_void_p(vp), nv, C.c_void_p(ip),
                   self._stream_ptr(stream, self.device))

    def device_ingests(self) -> int:
        """rt_get_device_ingests: launches of the geometry-input kernel since the renderer was created."""
        n = C.c_int64()
        self._call("rt_get_device_ingests", C.byref(n))
        return int(n.value)

    def set_accel_deferred(self, on: bool = True):
        """rt_set_accel_deferred: geometry changes build the octree and the quick wide BVH
        only; finish_accel, or the first frame after the switch is off, starts the background build."""
        self._call("rt_set_accel_deferred", 1 if on else 0)

    def accel_builds(self) -> int:
        """rt_get_accel_builds: background builds started since the renderer was created."""
        n = C.c_int64()
        self._call("rt_get_accel_builds", C.byref(n))
        return int(n.value)

    def add_sphere(self, center: Sequence[float], radius: float, mat_index: int = 0):
        self._call("rt_add_sphere", float(center[0]), float(center[1]), float(center[2]), float(radius), int(mat_index))

    def add_plane(self, point: Sequence[float], normal: Sequence[float], mat_index: int = 0):
        self._call("rt_add_plane", *[float(x) for x in point], *[float(x) for x in normal], int(mat_index))

    def clear_geometry(self):
        self._call("rt_clear_geometry")

    def set_materials(self, mats16):
        m = f32(mats16).reshape(-1, 16)
        self._call("rt_set_materials", ptr(m, _f32p), m.shape[0])

    def get_material_count(self) -> int:
        n = C.c_int32()
        self._call("rt_get_material_count", C.byref(n))
        return n.value

    # -- camera / light (renderer.h:72-75, 96-98) -----------------------------------
    def change_camera_fov(self, fov: float):
        self._call("rt_change_camera_fov", float(fov))

    def change_camera_aspect_ratio(self, aspect: float):
        self._call("rt_change_camera_aspect_ratio", float(aspect))

    def set_light_position(self, p: Sequence[float]):
        self._call("rt_set_light_position", float(p[0]), float(p[1]), float(p[2]))

    def set_camera_transform(self, m):
        m = f32(m)
        self._call("rt_set_camera_transform", ptr(m, _f32p))

    def apply_transformation_to_camera(self, m):
        m = f32(m)
        self._call("rt_apply_transformation_to_camera", ptr(m, _f32p))

    def set_camera_matrices(self, pos, proj_inv, cam_to_world):
        pos, pi, cw = f32(pos), f32(proj_inv), f32(cam_to_world)
        self._call("rt_set_camera_matrices", ptr(pos, _f32p), ptr(pi, _f32p), ptr(cw, _f32p))

    def set_camera_projection(self, proj, world_to_cam):
        """Camera::_perspective_proj_mat / _world_to_camera_mat, used by raster_trace."""
        pr, wc = f32(proj), f32(world_to_cam)
        self._call("rt_set_camera_projection", ptr(pr, _f32p), ptr(wc, _f32p))

    def set_camera_lens(self, fov: float, aspect: float):
        """Camera::_fov / _aspect_ratio without touching the matrices (read by SSAO)."""
        self._call("rt_set_camera_lens", float(fov), float(aspect))

    def get_camera_matrices(self):
        pos, pi, cw = np.zeros(3, np.float32), np.zeros(16, np.float32), np.zeros(16, np.float32)
        self._call("rt_get_camera_matrices", ptr(pos, _f32p), ptr(pi, _f32p), ptr(cw, _f32p))
        return pos, pi, cw

    def set_object_transform(self, m):
        m = f32(m)
        self._call("rt_set_object_transform", ptr(m, _f32p))

    def reset_previous_transform(self):
        self._call("rt_reset_previous_transform")

    def get_triangles(self):
        """rt_get_triangles: the world-space positions [n, 9] in caller order, after every
        set_object_transform so far (object edits queued for the device are applied first)."""
        n = C.c_int64()
        self._call("rt_get_triangles", None, C.byref(n))
        tri9 = np.zeros((n.value, 9), np.float32)
        self._call("rt_get_triangles", ptr(tri9, _f32p), C.byref(n))
        return tri9

    def device_transforms(self) -> int:
        """rt_get_device_transforms: object transforms applied by the GPU kernel since the renderer was
        created (the device build on, RT_GPU_XFORM not 0)."""
        n = C.c_int64()
        self._call("rt_get_device_transforms", C.byref(n))
        return int(n.value)

    # -- textures (renderer.h:77-90) ------------------------------------------------
    def _set_tex(self, slot, img):
        if img is None:
            self._call("rt_set_texture", slot, 0, 0, ptr(None, _f32p))
            return
        a = f32(img)
        h, w = a.shape[0], a.shape[1]
        self._call("rt_set_texture", slot, w, h, ptr(a, _f32p))

    def set_ao_map(self, img): self._set_tex(TEX_AO, img)
    def set_diffuse_map(self, img): self._set_tex(TEX_DIFFUSE, img)
    def set_normal_map(self, img): self._set_tex(TEX_NORMAL, img)
    def set_displacement_map(self, img): self._set_tex(TEX_DISPLACEMENT, img)
    def set_roughness_map(self, img): self._set_tex(TEX_ROUGHNESS, img)
    def set_skysphere(self, img): self._set_tex(TEX_SKYSPHERE, img)
    def clear_ao_map(self): self._set_tex(TEX_AO, None)
    def clear_diffuse_map(self): self._set_tex(TEX_DIFFUSE, None)
    def clear_normal_map(self): self._set_tex(TEX_NORMAL, None)
    def clear_displacement_map(self): self._set_tex(TEX_DISPLACEMENT, None)
    def clear_roughness_map(self): self._set_tex(TEX_ROUGHNESS, None)

    def set_skybox(self, faces):
        """faces: right, left, top, bottom, back, front (skybox.h:12-16), each (h, w, 4) float32."""
        arrs = [f32(f) for f in faces]
        w = (C.c_int32 * 6)(*[a.shape[1] for a in arrs])
        h = (C.c_int32 * 6)(*[a.shape[0] for a in arrs])
        p = (_f32p * 6)(*[ptr(a, _f32p) for a in arrs])
        self._keep_sky = arrs
        self._call("rt_set_skybox", w, h, p)

    # -- BVH (renderer.h:104-109) ---------------------------------------------------
    def reconstruct_bvh_new(self):
        self._call("rt_reconstruct_bvh_new")

    def destroy_bvh(self):
        self._call("rt_destroy_bvh")

    # -- rendering (renderer.h:149-154) ---------------------------------------------
    def ray_trace(self):
        self._call("rt_ray_trace")

    def raster_trace(self):
        """Renderer::raster_trace (renderer.cpp:869-1006): the hybrid raster + trace path."""
        self._call("rt_raster_trace")

    def post_process(self):
        self._call("rt_post_process")

    def get_image(self, out=None) -> np.ndarray:
        """Renderer::get_image: the current ARGB32 image as (h, w) uint32 (row 0 = bottom).
        Safe from a display thread while another thread renders (progressive readback): the
        size query and the copy run under the image lock.  ``out``: a (h, w) uint32 array to
        fill (a display that keeps its image buffer, as a QImage); a new one when it does not
        match the image's size."""
        w, h = C.c_int32(), C.c_int32()
        self.lock_image()
        try:
            self._call("rt_get_image", ptr(None, _u32p), C.byref(w), C.byref(h))
            if out is None or out.shape != (h.value, w.value) or out.dtype != np.uint32 or not out.flags.c_contiguous:
                out = np.empty((h.value, w.value), np.uint32)
            self._call("rt_get_image", ptr(out, _u32p), C.byref(w), C.byref(h))
        finally:
            self.unlock_image()
        return out

    def lock_image(self):
        """Renderer::lock_image_mutex (renderer.h:41)."""
        self._call("rt_lock_image")

    def unlock_image(self):
        """Renderer::unlock_image_mutex (renderer.h:42)."""
        self._call("rt_unlock_image")

    def request_aux(self, rgba=False, hit=False, shadow=False):
        self._call("rt_request_aux", int(rgba), int(hit), int(shadow))

    def get_internal(self, argb=True, rgba=False, hit=False, shadow=False):
        st = self.stats()
        n = st["render_width"] * st["render_height"]
        out = {}
        a = np.zeros(n, np.uint32) if argb else None
        r = np.zeros((n, 4), np.float32) if rgba else None
        hid = np.zeros(n, np.int32) if hit else None
        ht = np.zeros(n, np.float32) if hit else None
        sh = np.zeros(n, np.uint8) if shadow else None
        self._call("rt_get_internal", ptr(a, _u32p), ptr(r, _f32p), ptr(hid, _i32p), ptr(ht, _f32p), ptr(sh, _u8p))
        for k, v in (("argb", a), ("rgba", r), ("hit_id", hid), ("hit_t", ht), ("shadow", sh)):
            if v is not None:
                out[k] = v
        return out

    def get_ssao_buffers(self, ao=True):
        """(z, normals (n, 3), occlusion counts or None) of the last frame / SSAO pass."""
        st = self.stats()
        n = st["render_width"] * st["render_height"]
        z = np.zeros(n, np.float32)
        n4 = np.zeros((n, 4), np.float32)
        a = np.zeros(n, np.int32) if ao else None
        self._call("rt_get_ssao_buffers", ptr(z, _f32p), ptr(n4, _f32p), ptr(a, _i32p))
        return z, np.ascontiguousarray(n4[:, :3]), a

    def tile_costs(self):
        """The last frame's per-tile shader cycles, shape (tiles_y, tiles_x) (rt_tile_costs)."""
        tx, ty = C.c_int32(0), C.c_int32(0)
        self._call("rt_tile_costs", None, 0, C.byref(tx), C.byref(ty))
        out = np.zeros(tx.value * ty.value, np.uint32)
        self._call("rt_tile_costs", out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(tx), C.byref(ty))
        return out.reshape(ty.value, tx.value)

    def ocone_read(self):
        """The resident origin-cone grid (rt_ocone_read): (cells uint32 [n, 2], dims int32 [3], lo_ih float32 [4])."""
        dims = np.zeros(3, np.int32)
        lo_ih = np.zeros(4, np.float32)
        i32 = C.POINTER(C.c_int32)
        f32p = C.POINTER(C.c_float)
        self._call("rt_ocone_read", None, 0, dims.ctypes.data_as(i32), lo_ih.ctypes.data_as(f32p))
        cells = np.zeros((int(np.prod(dims.astype(np.int64))), 2), np.uint32)
        self._call("rt_ocone_read", cells.ctypes.data_as(C.POINTER(C.c_uint32)), cells.size, dims.ctypes.data_as(i32),
                   lo_ih.ctypes.data_as(f32p))
        return cells, dims, lo_ih

    def debug_read(self, n):
        """Diagnostic builds: the last frame's per-wave records (rt_debug_read)."""
        out = np.zeros(n, np.uint64)
        self._call("rt_debug_read", out.ctypes.data_as(C.POINTER(C.c_uint64)), n)
        return out

    def stats(self) -> dict:
        s = RtStats()
        self._call("rt_get_stats", C.byref(s))
        return s.as_dict()

    # -- image strips (multi-GPU) ---------------------------------------------------
    def local_rows(self, band_rows, rank, nranks) -> int:
        n = C.c_int32()
        self._call("rt_local_rows", int(band_rows), int(rank), int(nranks), C.byref(n))
        return n.value

    def render_bands_device(self, band_rows, rank, nranks, d_out_ptr: int, stream_ptr: int = 0):
        self._call("rt_render_bands_device", int(band_rows), int(rank), int(nranks), C.c_void_p(d_out_ptr),
                   C.c_void_p(stream_ptr))

    def render_band_list_device(self, band_rows, bands, d_out_ptr: int, stream_ptr: int = 0):
        """rt_render_band_list_device: the listed output bands into consecutive local bands of d_out
        (cost-balanced strips, strips.assign_bands)."""
        b = np.ascontiguousarray(bands, np.int32)
        self._call("rt_render_band_list_device", int(band_rows), ptr(b, _i32p), int(b.size), C.c_void_p(d_out_ptr),
                   C.c_void_p(stream_ptr))

    def band_costs(self, nbands: int, stream_ptr: int = 0, out=None) -> np.ndarray:
        """rt_band_costs: the cost (tile shader cycles) of each output band of the last band launch on the
        stream; the bands it did not render stay as in ``out`` (zeros by default)."""
        c = np.zeros(nbands, np.float64) if out is None else np.ascontiguousarray(out, np.float64)
        self._call("rt_band_costs", C.c_void_p(stream_ptr), c.ctypes.data_as(C.POINTER(C.c_double)), int(nbands))
        return c

    def trace_rays(self, orig, dirs):
        """BVH::intersect for a batch of rays -> (tri_id, t, u, v, ret)."""
        o = f32(orig).reshape(-1, 3)
        d = f32(dirs).reshape(-1, 3)
        if d.shape != o.shape:
            raise ValueError(f"trace_rays: {o.shape[0]} origins but {d.shape[0]} directions")
        n = o.shape[0]
        ids = np.zeros(n, np.int32)
        t, u, v = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        ret = np.zeros(n, np.uint8)
        self._call("rt_trace_rays", ptr(o, _f32p), ptr(d, _f32p), n, ptr(ids, _i32p), ptr(t, _f32p), ptr(u, _f32p),
                   ptr(v, _f32p), ptr(ret, _u8p))
        return ids, t, u, v, ret

    # -- ray queries on GPU memory (include/rt_mi355x.h "Ray queries on device memory") --------
    _RAY_OUT = (("tri_id", "int32"), ("t", "float32"), ("u", "float32"), ("v", "float32"), ("ret", "uint8"))

    def _ray_stream(self, stream):
        import torch
        return torch.cuda.current_stream(self.device) if stream is None else stream

    def trace_rays_device(self, orig, dirs, out=None, counts=None, stream=None):
        """rt_trace_rays_device: trace_rays for rays in GPU memory, through the frames' wide-BVH query, in
        the order of ``stream`` (a torch stream; default the current one) and without a host wait
        -> dict(tri_id int32, t, u, v float32, ret uint8) of torch tensors [n], bit for bit trace_rays'
        answers.  orig, dirs: contiguous float32 [n, 3] tensors on this renderer's GPU.  out: such a dict to
        write into (tensors of at least n elements; the rest is left alone), else new tensors.  counts: an
        int64 [2] tensor the kernel adds to: [0] rays the certified wide query answered, [1] rays traced
        through the octree (or the brute-force loop)."""
        import torch
        op, dp, n = _lib.device_ray_args(orig, dirs, self.device, ("orig", "dirs"))
        if n > 1 << 30:
            raise ValueError(f"trace_rays_device: {n} rays, at most 2^30 are taken")
        stream = self._ray_stream(stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = {k: torch.empty(n, dtype=getattr(torch, dt), device=orig.device) for k, dt in self._RAY_OUT}
        ptrs = [_lib.device_ray_out(out[k], k, getattr(torch, dt), n, self.device) for k, dt in self._RAY_OUT]
        cp = None if counts is None else _lib.device_ray_out(counts, "counts", torch.int64, 2, self.device)
        self._call("rt_trace_rays_device", C.c_void_p(op), C.c_void_p(dp), n, *[C.c_void_p(p) for p in ptrs],
                   C.c_void_p(cp), self._stream_ptr(stream, self.device))
        return out

    def is_shadowed_device(self, points, normals, light=None, out=None, stream=None):
        """rt_is_shadowed_device: Renderer::is_shadowed(point, normal, light) for (point, normal) pairs in GPU
        memory -> a uint8 torch tensor [n], 1 where the point is shadowed (all 0 with compute_shadows off).
        points, normals, stream as in trace_rays_device; light: 3 floats, None = the scene's light; out: a
        uint8 tensor of at least n elements to write into."""
        import torch
        pp, np_, n = _lib.device_ray_args(points, normals, self.device, ("points", "normals"))
        if n > 1 << 30:
            raise ValueError(f"is_shadowed_device: {n} pairs, at most 2^30 are taken")
        stream = self._ray_stream(stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty(n, dtype=torch.uint8, device=points.device)
        sp = _lib.device_ray_out(out, "out", torch.uint8, n, self.device)
        lp = None if light is None else f32(light).reshape(3)
        self._call("rt_is_shadowed_device", C.c_void_p(pp), C.c_void_p(np_), n, ptr(lp, _f32p), C.c_void_p(sp),
                   self._stream_ptr(stream, self.device))
        return out

    def device_ray_queries(self):
        """rt_get_device_ray_queries -> (calls, rays): launches of the closest-hit and the shadow kernel
        since the renderer was created, and the rays given to them (two ints each)."""
        calls, rays = np.zeros(2, np.int64), np.zeros(2, np.int64)
        i64p = C.POINTER(C.c_int64)
        self._call("rt_get_device_ray_queries", ptr(calls, i64p), ptr(rays, i64p))
        return (int(calls[0]), int(calls[1])), (int(rays[0]), int(rays[1]))

    # -- ray-segment queries on GPU memory (include/rt_mi355x.h "Ray-segment queries on device memory") ------
    def occluded_device(self, orig, dirs, tmax=None, out=None, counts=None, stream=None):
        """rt_occluded_device: is anything hit before tmax[i] along ray i -> a uint8 torch tensor [n], 1 where
        trace_rays_device's answer for the ray has ret != 0 and t < tmax[i] (float32, strict, false for a NaN).
        orig, dirs, counts, stream as in trace_rays_device; tmax: a contiguous float32 [n] tensor on this
        renderer's GPU, None = +inf for every ray; out: a uint8 tensor of at least n elements to write into."""
        import torch
        op, dp, tp, n = _lib.device_segment_args(orig, dirs, tmax, self.device)
        if n > 1 << 30:
            raise ValueError(f"occluded_device: {n} rays, at most 2^30 are taken")
        stream = self._ray_stream(stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty(n, dtype=torch.uint8, device=orig.device)
        sp = _lib.device_ray_out(out, "out", torch.uint8, n, self.device)
        cp = None if counts is None else _lib.device_ray_out(counts, "counts", torch.int64, 2, self.device)
        self._call("rt_occluded_device", C.c_void_p(op), C.c_void_p(dp), C.c_void_p(tp), n, C.c_void_p(sp),
                   C.c_void_p(cp), self._stream_ptr(stream, self.device))
        return out

    def trace_segments_device(self, orig, dirs, tmax=None, out=None, counts=None, stream=None):
        """rt_trace_segments_device: trace_rays_device's dict where the ray's answer has ret != 0 and
        t < tmax[i], bit for bit, and (-1, -1.0, 1.0, 0.0, 0) everywhere else.  tmax as in occluded_device, the
        other arguments as in trace_rays_device."""
        import torch
        op, dp, tp, n = _lib.device_segment_args(orig, dirs, tmax, self.device)
        if n > 1 << 30:
            raise ValueError(f"trace_segments_device: {n} rays, at most 2^30 are taken")
        stream = self._ray_stream(stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = {k: torch.empty(n, dtype=getattr(torch, dt), device=orig.device) for k, dt in self._RAY_OUT}
        ptrs = [_lib.device_ray_out(out[k], k, getattr(torch, dt), n, self.device) for k, dt in self._RAY_OUT]
        cp = None if counts is None else _lib.device_ray_out(counts, "counts", torch.int64, 2, self.device)
        self._call("rt_trace_segments_device", C.c_void_p(op), C.c_void_p(dp), C.c_void_p(tp), n,
                   *[C.c_void_p(p) for p in ptrs], C.c_void_p(cp), self._stream_ptr(stream, self.device))
        return out

    def device_segment_queries(self):
        """rt_get_device_segment_queries -> (calls, rays): launches of occluded_device and of
        trace_segments_device since the renderer was created, and the rays given to them (two ints each)."""
        calls, rays = np.zeros(2, np.int64), np.zeros(2, np.int64)
        i64p = C.POINTER(C.c_int64)
        self._call("rt_get_device_segment_queries", ptr(calls, i64p), ptr(rays, i64p))
        return (int(calls[0]), int(calls[1])), (int(rays[0]), int(rays[1]))

    def visibility_device(self, out=None, stream=None):
        """rt_visibility_device: the visibility buffer of the current camera, in the order of ``stream`` (a torch
        stream; default the current one) and without a host wait -> dict(tri_id int32 [rh, rw], t float32 [rh, rw],
        uv float32 [rh, rw, 2]) of torch tensors on this renderer's GPU, rh x rw the internal image (SSAA applied):
        per pixel the hit_id and hit_t ray_trace leaves for get_internal, and the hit's barycentrics where tri_id
        >= 0 (else 0, 0).  Nothing is shaded.  out: such a dict to write into, any non-empty subset of the keys:
        only those are written and returned; else three new tensors."""
        import torch
        st = self.stats()
        rw, rh = st["render_width"], st["render_height"]
        stream = self._ray_stream(stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = {k: torch.empty((rh, rw) if c is None else (rh, rw, c), dtype=getattr(torch, dt),
                                      device=torch.device("cuda", self.device))
                       for k, dt, c in _lib.VISIBILITY_OUT}
        ptrs = _lib.device_visibility_outs(out, rw, rh, self.device)
        self._call("rt_visibility_device", *[C.c_void_p(p) for p in ptrs], self._stream_ptr(stream, self.device))
        return out

    def device_visibility(self):
        """rt_get_device_visibility -> (calls, pixels, used): visibility_device's launches of the fast [0] and the
        generic [1] kernel instance since the renderer was created and their pixels; used: the launches that were
        given a tile mask [0] and entry sets [1]."""
        calls, pixels, used = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(2, np.int64)
        i64p = C.POINTER(C.c_int64)
        self._call("rt_get_device_visibility", ptr(calls, i64p), ptr(pixels, i64p), ptr(used, i64p))
        return tuple(int(c) for c in calls), tuple(int(p) for p in pixels), tuple(int(u) for u in used)

    def trace_ray_device(self, orig, dirs, current_recursion_depth=0, first_ray=0, out=None, counts=None, stream=None):
        """rt_trace_ray_device: trace_ray (shaded) for rays in GPU memory, in the order of ``stream`` (a torch
        stream; default the current one) and without a host wait -> dict(rgba float32 [n, 4], hit_src int32,
        t float32, intersection_found uint8, shadowed uint8) of torch tensors, trace_ray's answers.  orig, dirs:
        contiguous float32 [n, 3] tensors on this renderer's GPU.  first_ray: ray i draws the rough-reflection
        stream of pixel first_ray + i.  out: such a dict to write into, any subset of the keys that holds rgba
        (tensors of at least n rows; the rest is left alone): only those are written and returned; else five new
        tensors.  counts: an int64 [2] tensor the kernel adds to: [0] the call's shadow rays, [1] its reflection
        rays (what stats() reports after trace_ray)."""
        return self._shade_device("rt_trace_ray_device", "trace_ray_device", orig, dirs, current_recursion_depth,
                                  first_ray, out, counts, stream)

    def _shade_device(self, fn, name, orig, dirs, depth, first_ray, out, counts, stream):
        """The two shaded device queries' common form: the tensors' checks, new outputs on ``stream``, the call."""
        import torch
        op, dp, n = _lib.device_ray_args(orig, dirs, self.device, ("orig", "dirs"))
        if n > 1 << 30:
            raise ValueError(f"{name}: {n} rays, at most 2^30 are taken")
        stream = self._ray_stream(stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = {k: torch.empty((n, c) if c else n, dtype=getattr(torch, dt), device=orig.device)
                       for k, dt, c in _lib.SHADE_OUT}
        ptrs = _lib.device_shade_outs(out, n, self.device)
        cp = None if counts is None else _lib.device_ray_out(counts, "counts", torch.int64, 2, self.device)
        self._call(fn, C.c_void_p(op), C.c_void_p(dp), n, int(depth), int(first_ray), *[C.c_void_p(p) for p in ptrs],
                   C.c_void_p(cp), self._stream_ptr(stream, self.device))
        return out

    def trace_ray_batch_device(self, orig, dirs, current_recursion_depth=0, first_ray=0, out=None, counts=None,
                               stream=None):
        """rt_trace_ray_batch_device: trace_ray_device's arguments and answers, shaded by the frame engine where the
        scene has a reflective material (level by level, as the frames; else it is trace_ray_device).  The work is
        ordered on ``stream``, but the host blocks while the engine reads its counts, the call may allocate, and
        the stream first waits for band launches and queries in flight.  hit_src, t, the flags and the counts are
        trace_ray_device's bit for bit; rgba is the engine's colour (a frame's, for its camera rays)."""
        return self._shade_device("rt_trace_ray_batch_device", "trace_ray_batch_device", orig, dirs,
                                  current_recursion_depth, first_ray, out, counts, stream)

    def device_shaded_batches(self):
        """rt_get_device_shaded_batches -> (calls, rays): trace_ray_batch_device's calls the engine shaded [0] and
        those handed to trace_ray_device's code [1] since the renderer was created, and their rays."""
        calls, rays = np.zeros(2, np.int64), np.zeros(2, np.int64)
        i64p = C.POINTER(C.c_int64)
        self._call("rt_get_device_shaded_batches", ptr(calls, i64p), ptr(rays, i64p))
        return tuple(int(c) for c in calls), tuple(int(r) for r in rays)

    def device_shaded_queries(self):
        """rt_get_device_shaded_queries -> (calls, rays): launches of trace_ray_device's plain, generic and
        reflective kernel instance since the renderer was created, and the rays given to them (three ints
        each)."""
        calls, rays = np.zeros(3, np.int64), np.zeros(3, np.int64)
        i64p = C.POINTER(C.c_int64)
        self._call("rt_get_device_shaded_queries", ptr(calls, i64p), ptr(rays, i64p))
        return tuple(int(c) for c in calls), tuple(int(r) for r in rays)

    def wide_query(self, orig, dirs, kind=1):
        """rt_wide_query: the frames' wide-BVH query on the GPU with its status -> dict(o, d, status,
        id, t, u, v, shadowed); kind 0 plain rays, 1 camera rays, 2 (hit point, normal) pairs as
        is_shadowed's rays towards the light."""
        o = f32(orig).reshape(-1, 3)
        d = f32(dirs).reshape(-1, 3)
        if d.shape != o.shape:
            raise ValueError(f"wide_query: {o.shape[0]} origins but {d.shape[0]} directions")
        n = o.shape[0]
        out = dict(o=np.zeros((n, 3), np.float32), d=np.zeros((n, 3), np.float32), status=np.zeros(n, np.int32),
                   id=np.zeros(n, np.int32), t=np.zeros(n, np.float32), u=np.zeros(n, np.float32),
                   v=np.zeros(n, np.float32), shadowed=np.zeros(n, np.uint8))
        self._call("rt_wide_query", ptr(o, _f32p), ptr(d, _f32p), n, int(kind), ptr(out["o"], _f32p),
                   ptr(out["d"], _f32p), ptr(out["status"], _i32p), ptr(out["id"], _i32p), ptr(out["t"], _f32p),
                   ptr(out["u"], _f32p), ptr(out["v"], _f32p), ptr(out["shadowed"], _u8p))
        return out

    def risk_words(self, src=0):
        """rt_risk_words: the current camera / light risk words, src 0 the GPU's, 1 the host walk's
        -> (words, violations of check_risk_words)."""
        n, bad = C.c_int64(), C.c_int64()
        self._call("rt_risk_words", int(src), None, 0, C.byref(n), None)
        out = np.zeros(n.value, np.uint64)
        self._call("rt_risk_words", int(src), out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size, C.byref(n),
                   C.byref(bad))
        return out, bad.value

    def trace_ray(self, orig, dirs, current_recursion_depth=0):
        """Renderer::trace_ray (shaded) for a batch of rays, each with a fresh HitInfo
        -> (rgba [n,4], hit_src, t, intersection_found, shadowed)."""
        o = f32(orig).reshape(-1, 3)
        d = f32(dirs).reshape(-1, 3)
        if d.shape != o.shape:
            raise ValueError(f"trace_ray: {o.shape[0]} origins but {d.shape[0]} directions")
        n = o.shape[0]
        rgba = np.zeros((n, 4), np.float32)
        src = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        found = np.zeros(n, np.uint8)
        shadowed = np.zeros(n, np.uint8)
        self._call("rt_trace_ray", ptr(o, _f32p), ptr(d, _f32p), n, int(current_recursion_depth), ptr(rgba, _f32p),
                   ptr(src, _i32p), ptr(t, _f32p), ptr(found, _u8p), ptr(shadowed, _u8p))
        return rgba, src, t, found, shadowed

    def kernel_times(self, n):
        ms = np.zeros(n, np.float32)
        self._call("rt_kernel_times", ptr(ms, _f32p), int(n))
        return ms

    def band_counters(self):
        a, b = C.c_int64(), C.c_int64()
        self._call("rt_band_counters", C.byref(a), C.byref(b))
        return a.value, b.value

    def tile_mask(self, src=0):
        """The last frame launch's tile mask (rt_tile_mask) -> (covered [block rows, blocks per row] bool, dict):
        covered[by, bx] False: the 8 x 8 block was written as background without a ray.  src 0: the device's
        mask, 1: the host's recomputation.  dict: 'on' (False: the launch had no mask), 'cut' entries."""
        info = np.zeros(5, np.int32)
        self._call("rt_tile_mask", int(src), None, 0, ptr(info, _i32p))
        bw, bh, wpr = int(info[0]), int(info[1]), int(info[2])
        words = np.zeros(bh * wpr, np.uint32)
        self._call("rt_tile_mask", int(src), ptr(words, _u32p), words.size, ptr(info, _i32p))
        bits = (words.reshape(bh, wpr)[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
        return bits.reshape(bh, wpr * 32)[:, :bw].astype(bool), {"on": bool(info[3]), "cut": int(info[4])}

    def tile_starts(self, src=0):
        """The last frame launch's entry sets (rt_tile_starts) -> (sets [block rows, blocks per row, 4] uint32,
        on): the wide-BVH nodes each 8 x 8 block's camera rays start at (0xFFFFFFFF: unused slot; [0, ...]: the
        root).  src 0: the device's, 1: the host's recomputation.  on False: the launch had no entry sets."""
        info = np.zeros(3, np.int32)
        self._call("rt_tile_starts", int(src), None, 0, ptr(info, _i32p))
        sets = np.zeros((int(info[1]), int(info[0]), 4), np.uint32)
        self._call("rt_tile_starts", int(src), ptr(sets, _u32p), sets.size, ptr(info, _i32p))
        return sets, bool(info[2])

    def tile_lists(self, src=0):
        """The last frame launch's tile lists (rt_tile_lists) -> (covered, clear, dict): the launch's 8 x 8 tiles
        (row-major over its local rows) that the queue handed out and those filled with the background at the
        waves' exit, each ascending.  src 0: the device's lists, 1: the host's recomputation from the mask
        words.  dict: 'on' (False: the launch had no lists), 'tiles_x', 'tiles_y'."""
        info = np.zeros(5, np.int32)
        self._call("rt_tile_lists", int(src), None, 0, ptr(info, _i32p))
        tiles = np.zeros(max(1, int(info[2]) + int(info[3])), np.int32)
        self._call("rt_tile_lists", int(src), ptr(tiles, _i32p), tiles.size, ptr(info, _i32p))
        nc, nk = int(info[2]), int(info[3])
        return tiles[:nc].copy(), tiles[nc:nc + nk].copy(), {"on": bool(info[4]), "tiles_x": int(info[0]),
                                                             "tiles_y": int(info[1])}

    # -- convenience ----------------------------------------------------------------
    def load_scene(self, sc: SceneData, st: RenderSettings):
        """Settings, camera, light, materials, geometry and textures of a SceneData."""
        self.set_render_settings(st)
        self.change_render_size(st.image_width, st.image_height)
        self.set_camera_matrices(sc.cam_pos, sc.proj_inv, sc.cam_to_world)
        if sc.proj is not None and sc.world_to_cam is not None:
            self.set_camera_projection(sc.proj, sc.world_to_cam)
        self.set_camera_lens(*sc.lens(st))
        self.set_light_position(sc.light)
        self.set_materials(sc.materials)
        self.clear_geometry()
        for k in range(len(sc.shape_kind)):
            s = sc.shape[k]
            if sc.shape_kind[k] == SHAPE_SPHERE:
                self.add_sphere(s[:3], s[3], int(sc.shape_mat[k]))
            else:
                self.add_plane(s[:3], s[3:6], int(sc.shape_mat[k]))
        self.set_triangles(sc.tri, sc.tri_mat, sc.tri_uv)
        for slot in range(6):
            self._set_tex(slot, sc.textures.get(slot) if sc.textures else None)
        if sc.skybox is not None:
            self.set_skybox(sc.skybox)


def render(renderer: Renderer) -> float:
    """render(Renderer&) (utils/mainUtils.cpp:6-21): ray_trace + post_process; returns ms."""
    ms = C.c_float()
    check(_lib.lib().rt_render(renderer._h, C.byref(ms)), "rt_render")
    return float(ms.value)
