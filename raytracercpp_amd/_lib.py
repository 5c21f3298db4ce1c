"""ctypes binding of librt_mi355x.so (include/rt_mi355x.h).

The product path is this HIP library; there is no CPU fallback.  Loading fails
loudly when the in-tree .so is missing (build it with ``__graft_entry__.build()``
or ``make -C raytracercpp_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librt_mi355x.so")
# development only (tools/variants.py): benchmark an alternative build of the same library
if os.environ.get("RT_LIB_PATH"):
    LIB_PATH = os.environ["RT_LIB_PATH"]

RT_OK = 0
ERRORS = {-1: "RT_EINVAL", -2: "RT_EHIP", -3: "RT_ENOMEM", -4: "RT_ESTATE", -5: "RT_EUNSUPPORTED", -6: "RT_EIO"}

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)
_i64p = C.POINTER(C.c_int64)


class RtSettings(C.Structure):
    _fields_ = [
        ("image_width", C.c_int32), ("image_height", C.c_int32),
        ("enable_ssaa", C.c_int32), ("ssaa_factor", C.c_int32),
        ("enable_clipping", C.c_int32), ("hybrid_rasterization_tracing", C.c_int32),
        ("shading_method", C.c_int32), ("compute_shadows", C.c_int32), ("max_recursion_depth", C.c_int32),
        ("enable_bvh", C.c_int32), ("bvh_max_depth", C.c_int32), ("bvh_leaf_object_count", C.c_int32),
        ("enable_ssao", C.c_int32), ("ssao_sample_count", C.c_int32),
        ("ssao_radius", C.c_float), ("ssao_amount", C.c_float),
        ("enable_ambient", C.c_int32), ("enable_diffuse", C.c_int32), ("enable_specular", C.c_int32),
        ("enable_emissive", C.c_int32), ("rough_reflections_sample_count", C.c_int32),
        ("enable_ao_mapping", C.c_int32), ("enable_diffuse_mapping", C.c_int32),
        ("enable_normal_mapping", C.c_int32), ("enable_displacement_mapping", C.c_int32),
        ("displacement_mapping_strength", C.c_float), ("parallax_mapping_steps", C.c_int32),
        ("enable_roughness_mapping", C.c_int32), ("enable_skysphere", C.c_int32), ("enable_skybox", C.c_int32),
        ("rng_seed", C.c_uint32),
    ]


class RtStats(C.Structure):
    _fields_ = [
        ("primary_rays", C.c_int64), ("shadow_rays", C.c_int64), ("reflection_rays", C.c_int64),
        ("kernel_ms", C.c_float), ("post_ms", C.c_float), ("build_ms", C.c_float),
        ("octree_inner", C.c_int64), ("octree_leaves", C.c_int64), ("octree_empty_leaves", C.c_int64),
        ("octree_max_leaf", C.c_int64), ("octree_max_depth", C.c_int64),
        ("gpu_nodes", C.c_int64), ("gpu_tris", C.c_int64),
        ("render_width", C.c_int32), ("render_height", C.c_int32), ("seg_scale", C.c_float),
        ("work", C.c_int64 * 4), ("work_wide", C.c_int64 * 4), ("uncertified", C.c_int64 * 6),
        ("wave_steps", C.c_int64 * 6), ("build_split_ms", C.c_float * 4), ("host_builds", C.c_int64),
        ("wide_tree", C.c_int32),
    ]

    def as_dict(self):
        def conv(n, t):
            v = getattr(self, n)
            if t is C.c_float:
                return float(v)
            if isinstance(v, C.Array):
                return [float(x) if n == "build_split_ms" else int(x) for x in v]
            return int(v)
        return {n: conv(n, t) for n, t in self._fields_}


class RtEntryProbe(C.Structure):
    """rt_entry_probe (include/rt_mi355x_diag.h): rt_wbvh_query_ex's camera rays start at their blocks' entry sets."""
    _fields_ = [
        ("proj_inv", C.c_float * 16), ("cam_to_world", C.c_float * 16), ("rw", C.c_int32), ("rh", C.c_int32),
        ("k", C.c_int32), ("fan", C.c_int32), ("depth", C.c_int32), ("quick", C.c_int32),
        ("pixel", _i32p), ("sets", _u32p), ("info", C.c_int64 * 4), ("depth_hist", C.c_int64 * 16),
        ("no_cull", C.c_int32), ("reserved", C.c_int32), ("close_hist", C.c_int64 * 4),
    ]


# every exported symbol and its ctypes signature (restype, argtypes); tests check
# that the .so exports exactly what include/rt_mi355x.h declares.
_H = C.c_void_p
SIGNATURES = {
    "rt_default_settings": (None, [C.POINTER(RtSettings)]),
    "rt_create": (_H, [C.c_int]),
    "rt_destroy": (None, [_H]),
    "rt_last_error": (C.c_char_p, []),
    "rt_get_settings": (C.c_int, [_H, C.POINTER(RtSettings)]),
    "rt_set_settings": (C.c_int, [_H, C.POINTER(RtSettings)]),
    "rt_change_render_size": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "rt_set_exact": (C.c_int, [_H, C.c_int]),
    "rt_finish_accel": (C.c_int, [_H]),
    "rt_set_devices": (C.c_int, [_H, _i32p, C.c_int32]),
    "rt_set_triangles": (C.c_int, [_H, _f32p, _i32p, _f32p, C.c_int64]),
    "rt_add_sphere": (C.c_int, [_H, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32]),
    "rt_add_plane": (C.c_int, [_H] + [C.c_float] * 6 + [C.c_int32]),
    "rt_clear_geometry": (C.c_int, [_H]),
    "rt_set_materials": (C.c_int, [_H, _f32p, C.c_int32]),
    "rt_get_material_count": (C.c_int, [_H, _i32p]),
    "rt_change_camera_fov": (C.c_int, [_H, C.c_float]),
    "rt_change_camera_aspect_ratio": (C.c_int, [_H, C.c_float]),
    "rt_set_light_position": (C.c_int, [_H, C.c_float, C.c_float, C.c_float]),
    "rt_set_camera_transform": (C.c_int, [_H, _f32p]),
    "rt_apply_transformation_to_camera": (C.c_int, [_H, _f32p]),
    "rt_set_camera_matrices": (C.c_int, [_H, _f32p, _f32p, _f32p]),
    "rt_set_camera_projection": (C.c_int, [_H, _f32p, _f32p]),
    "rt_set_camera_lens": (C.c_int, [_H, C.c_float, C.c_float]),
    "rt_get_ssao_buffers": (C.c_int, [_H, _f32p, _f32p, _i32p]),
    "rt_get_camera_matrices": (C.c_int, [_H, _f32p, _f32p, _f32p]),
    "rt_set_object_transform": (C.c_int, [_H, _f32p]),
    "rt_reset_previous_transform": (C.c_int, [_H]),
    "rt_get_triangles": (C.c_int, [_H, _f32p, _i64p]),
    "rt_get_device_transforms": (C.c_int, [_H, _i64p]),
    "rt_transform_points_device": (C.c_int, [C.c_int32, _f32p, _f32p, C.c_int64, _f32p, _i32p, _f32p]),
    "rt_set_triangles_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, _i32p, _f32p, C.c_int64, C.c_void_p]),
    "rt_update_vertices_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "rt_get_device_ingests": (C.c_int, [_H, _i64p]),
    "rt_gather_triangles_device": (C.c_int, [C.c_int32, _f32p, C.c_int64, _i32p, C.c_int64, _f32p, _i32p, _f32p]),
    "rt_set_accel_deferred": (C.c_int, [_H, C.c_int]),
    "rt_get_accel_builds": (C.c_int, [_H, _i64p]),
    "rt_set_texture": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, _f32p]),
    "rt_set_skybox": (C.c_int, [_H, _i32p, _i32p, C.POINTER(_f32p)]),
    "rt_reconstruct_bvh_new": (C.c_int, [_H]),
    "rt_destroy_bvh": (C.c_int, [_H]),
    "rt_ray_trace": (C.c_int, [_H]),
    "rt_raster_trace": (C.c_int, [_H]),
    "rt_post_process": (C.c_int, [_H]),
    "rt_get_image": (C.c_int, [_H, _u32p, _i32p, _i32p]),
    "rt_render": (C.c_int, [_H, _f32p]),
    "rt_lock_image": (C.c_int, [_H]),
    "rt_unlock_image": (C.c_int, [_H]),
    "rt_request_aux": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32]),
    "rt_get_internal": (C.c_int, [_H, _u32p, _f32p, _i32p, _f32p, _u8p]),
    "rt_get_stats": (C.c_int, [_H, C.POINTER(RtStats)]),
    "rt_local_rows": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, _i32p]),
    "rt_render_bands_device": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rt_render_band_list_device": (C.c_int, [_H, C.c_int32, _i32p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rt_band_costs": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    "rt_trace_rays": (C.c_int, [_H, _f32p, _f32p, C.c_int64, _i32p, _f32p, _f32p, _f32p, _u8p]),
    "rt_trace_rays_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_is_shadowed_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, _f32p, C.c_void_p, C.c_void_p]),
    "rt_get_device_ray_queries": (C.c_int, [_H, _i64p, _i64p]),
    "rt_occluded_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "rt_trace_segments_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_get_device_segment_queries": (C.c_int, [_H, _i64p, _i64p]),
    "rt_trace_ray_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_get_device_shaded_queries": (C.c_int, [_H, _i64p, _i64p]),
    "rt_trace_ray_batch_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_get_device_shaded_batches": (C.c_int, [_H, _i64p, _i64p]),
    "rt_visibility_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_get_device_visibility": (C.c_int, [_H, _i64p, _i64p, _i64p]),
    "rt_trace_ray":(C.c_int, [_H, _f32p, _f32p, C.c_int64, C.c_int32, _f32p, _i32p, _f32p, _u8p, _u8p]),
    "rt_wide_query": (C.c_int, [_H, _f32p, _f32p, C.c_int64, C.c_int32, _f32p, _f32p, _i32p, _i32p, _f32p, _f32p, _f32p,
                                _u8p]),
    "rt_risk_words": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_uint64), C.c_int64, _i64p, _i64p]),
    "rt_kernel_times": (C.c_int, [_H, _f32p, C.c_int32]),
    "rt_band_counters": (C.c_int, [_H, _i64p, _i64p]),
    "rt_tile_mask": (C.c_int, [_H, C.c_int32, _u32p, C.c_int64, _i32p]),
    "rt_tile_starts": (C.c_int, [_H, C.c_int32, _u32p, C.c_int64, _i32p]),
    "rt_tile_lists": (C.c_int, [_H, C.c_int32, _i32p, C.c_int64, _i32p]),
    "rt_make_transform": (None, [C.c_int32, C.c_float, C.c_float, C.c_float, _f32p]),
    "rt_compose": (None, [_f32p, _f32p, _f32p]),
    "rt_inverse": (None, [_f32p, _f32p]),
    "rt_perspective": (None, [C.c_float, C.c_float, C.c_float, C.c_float, _f32p]),
    "rt_transform_points": (None, [_f32p, _f32p, C.c_int64, _f32p]),
    "rt_obj_open": (_H, [C.c_char_p, _f32p, C.c_int32]),
    "rt_obj_counts": (C.c_int, [_H, _i64p, _i32p, _i32p]),
    "rt_obj_fetch": (C.c_int, [_H, _f32p, _i32p, _f32p, _f32p]),
    "rt_obj_close": (None, [_H]),
    "rt_octree_digest": (C.c_int, [_f32p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint64), _i64p,
                                   _f32p]),
    "rt_octree_build_device": (C.c_int, [C.c_int32, _f32p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64),
                                         _i64p, _f32p]),
    "rt_set_device_build": (C.c_int, [_H, C.c_int]),
    "rt_get_device_builds": (C.c_int, [_H, _i64p]),
    "rt_get_device_wide_builds": (C.c_int, [_H, _i64p]),
    "rt_wbvh_quick_digest": (C.c_int, [_f32p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64), _i64p, _f32p]),
    "rt_wbvh_quick_build_device": (C.c_int, [C.c_int32, _f32p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64),
                                             _i64p, _i64p, _f32p]),
    "rt_debug_read": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_int64]),
    "rt_tile_costs": (C.c_int, [_H, C.POINTER(C.c_uint32), C.c_int64, _i32p, _i32p]),
    "rt_wbvh_query": (C.c_int, [_f32p, C.c_int64, C.c_int32, C.c_int32, _f32p, _f32p, C.c_int64, _i32p, _i32p, _f32p,
                                _f32p, _f32p, _i64p, _f32p]),
    "rt_wbvh_query_ex": (C.c_int, [_f32p, C.c_int64, C.c_int32, C.c_int32, _f32p, _f32p, C.c_int64, _f32p, _f32p,
                                   C.c_int32, _f32p, _f32p, _i32p, _i32p, _f32p, _f32p, _f32p, _i64p, _f32p, _i32p,
                                   C.c_int32, _i64p, C.POINTER(RtEntryProbe)]),
    "rt_ocone_check": (C.c_int, [_f32p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _f32p, _f32p, C.c_int64, _i32p,
                                 _i64p, C.POINTER(C.c_uint32), _i32p, _f32p, C.POINTER(C.c_uint32)]),
    "rt_ocone_read": (C.c_int, [_H, C.POINTER(C.c_uint32), C.c_int64, _i32p, _f32p]),
    "rt_risk_cap_check": (C.c_int, [_f32p, C.c_int64, C.c_int32, C.c_int32, _f32p, _f32p, C.c_int64, C.c_float, _i32p,
                                    _i64p]),
}

# the geometry-input entry points: an older build named by RT_LIB_PATH (development, tools/deform_time.py's
# row against another commit's library) may lack them; the in-tree library must have every symbol
GEOMETRY_INPUT = ("rt_set_triangles_device", "rt_update_vertices_device", "rt_get_device_ingests",
                  "rt_gather_triangles_device", "rt_set_accel_deferred", "rt_get_accel_builds")
# the device ray queries, likewise (tools/ray_query_time.py skips their rows for such a library)
RAY_QUERIES = ("rt_trace_rays_device", "rt_is_shadowed_device", "rt_get_device_ray_queries")
# the shaded device query, likewise
SHADED_QUERIES = ("rt_trace_ray_device", "rt_get_device_shaded_queries")
# the shaded batches through the frame engine, likewise
SHADED_BATCHES = ("rt_trace_ray_batch_device", "rt_get_device_shaded_batches")
# the tile lists' read-back, likewise (an A/B run against the parent commit's library)
TILE_LISTS = ("rt_tile_lists",)
# the visibility buffer on device memory, likewise
VISIBILITY = ("rt_visibility_device", "rt_get_device_visibility")
# the ray-segment queries, likewise
SEGMENT_QUERIES = ("rt_occluded_device", "rt_trace_segments_device", "rt_get_device_segment_queries")

_lib = None


def has(name):
    """Whether the loaded library exports ``name`` (see GEOMETRY_INPUT)."""
    return hasattr(lib(), name)


def lib():
    """The loaded librt_mi355x.so (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: the HIP library must be built "
                               "(python -c 'import __graft_entry__ as g; g.build()')")
        # torch bundles its own libamdhip64.so.7 (same soname as ROCm's): load it first
        # so that a process using both (device buffers, RCCL) runs ONE HIP runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if (name in GEOMETRY_INPUT + RAY_QUERIES + SHADED_QUERIES + SHADED_BATCHES + TILE_LISTS + VISIBILITY +
                    SEGMENT_QUERIES and os.environ.get("RT_LIB_PATH") and not hasattr(L, name)):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class RtError(RuntimeError):
    def __init__(self, code, where):
        msg = lib().rt_last_error()
        super().__init__(f"{where}: {ERRORS.get(code, code)}: {msg.decode() if msg else ''}")
        self.code = code


def check(rc, where):
    if rc != RT_OK:
        raise RtError(rc, where)
    return rc


def ptr(a, t):
    if a is None:
        return C.cast(None, t)
    return a.ctypes.data_as(t)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- mat.cpp helpers -----------------------------------------------------------
_KINDS = {"translation": 0, "rx": 1, "ry": 2, "rz": 3, "scale": 4, "identity": 5}


def make_transform(kind, x=0.0, y=0.0, z=0.0):
    out = np.zeros(16, np.float32)
    lib().rt_make_transform(_KINDS[kind], x, y, z, ptr(out, _f32p))
    return out


def compose(a, b):
    a, b = f32(a), f32(b)
    out = np.zeros(16, np.float32)
    lib().rt_compose(ptr(a, _f32p), ptr(b, _f32p), ptr(out, _f32p))
    return out


def inverse(m):
    m = f32(m)
    out = np.zeros(16, np.float32)
    lib().rt_inverse(ptr(m, _f32p), ptr(out, _f32p))
    return out


def perspective(fov, aspect, znear=0.1, zfar=1000.0):
    out = np.zeros(16, np.float32)
    lib().rt_perspective(fov, aspect, znear, zfar, ptr(out, _f32p))
    return out


def camera_matrices(fov, aspect, znear=0.1, zfar=1000.0):
    """Camera::set_aspect_ratio (camera.cpp:5-11): (Perspective, Perspective.inverse())."""
    p = perspective(fov, aspect, znear, zfar)
    return p, inverse(p)


def transform_points(m, pts):
    m = f32(m)
    pts = f32(pts).reshape(-1, 3)
    out = np.zeros_like(pts)
    lib().rt_transform_points(ptr(m, _f32p), ptr(pts, _f32p), pts.shape[0], ptr(out, _f32p))
    return out


def transform_points_device(m, pts, device=0):
    """rt_transform_points_device: (points, nonfinite flag, (kernel ms by HIP events, whole call ms)) of
    the object-edit kernel alone on the GPU; against transform_points the bytes differ only where both
    are NaN.  Raises RtError (RT_EHIP: no usable device)."""
    m = f32(m)
    pts = f32(pts).reshape(-1, 3)
    out = np.zeros_like(pts)
    flag = C.c_int32()
    ms = np.zeros(2, np.float32)
    check(lib().rt_transform_points_device(device, ptr(m, _f32p), ptr(pts, _f32p), pts.shape[0], ptr(out, _f32p),
                                           C.byref(flag), ptr(ms, _f32p)), "rt_transform_points_device")
    return out, int(flag.value), (float(ms[0]), float(ms[1]))


def gather_triangles_device(verts, indices=None, device=0):
    """rt_gather_triangles_device: (tri9 [n, 9], flags, (kernel ms by HIP events, whole call ms)) of the
    geometry-input kernel alone on host arrays: verts [nv, 3] gathered through indices [n, 3] (int32), or
    with indices None verts is the flat [n, 9].  flags bit 0: a written coordinate is not finite; bit 1: an
    index outside [0, nv) (zeros written).  Raises RtError (RT_EHIP: no usable device)."""
    verts = f32(verts)
    if indices is None:
        verts = verts.reshape(-1, 9)
        n, nv, idx = verts.shape[0], 3 * verts.shape[0], None
    else:
        verts = verts.reshape(-1, 3)
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
        n, nv = idx.shape[0], verts.shape[0]
    out = np.zeros((n, 9), np.float32)
    flags = C.c_int32()
    ms = np.zeros(2, np.float32)
    check(lib().rt_gather_triangles_device(device, ptr(verts, _f32p), nv, ptr(idx, _i32p), n, ptr(out, _f32p),
                                           C.byref(flags), ptr(ms, _f32p)), "rt_gather_triangles_device")
    return out, int(flags.value), (float(ms[0]), float(ms[1]))


def device_geometry_args(verts, indices, device):
    """The checks of Renderer.set_triangles_device / update_vertices_device on their torch tensors:
    (verts pointer, nv, indices pointer or None, n).  verts: float32 [n, 9] (indices None) or [nv, 3] with
    indices int32 [n, 3]; both contiguous tensors on the GPU with index ``device``.  TypeError for a
    non-tensor or a wrong dtype, ValueError for the wrong place, layout or shape."""
    import torch

    def form(t, name, dtype, cols):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a torch tensor on the GPU is needed, not {type(t).__name__}")
        if t.dtype != dtype:
            raise TypeError(f"{name}: dtype {t.dtype}, {dtype} is needed")
        if t.dim() != 2 or t.shape[1] != cols:
            raise ValueError(f"{name}: shape {tuple(t.shape)}, [n, {cols}] is needed")

    def place(t, name):
        if not t.is_cuda:
            raise ValueError(f"{name}: the tensor is on {t.device}, not on a GPU")
        if t.device.index != int(device):
            raise ValueError(f"{name}: the tensor is on GPU {t.device.index}, the renderer on GPU {int(device)}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: the tensor is not contiguous")

    # (what each tensor is before where it lies: the first kind of mistake shows without a GPU)
    form(verts, "verts", torch.float32, 9 if indices is None else 3)
    if indices is not None:
        form(indices, "indices", torch.int32, 3)
    place(verts, "verts")
    if indices is None:
        return verts.data_ptr(), 3 * verts.shape[0], None, verts.shape[0]
    place(indices, "indices")
    return verts.data_ptr(), verts.shape[0], indices.data_ptr(), indices.shape[0]


def device_ray_args(a, b, device, names=("orig", "dirs")):
    """The checks of Renderer.trace_rays_device / is_shadowed_device on their two torch tensors (origins and
    directions, or points and normals): (a pointer, b pointer, n).  Both float32 [n, 3] with the same n,
    contiguous, on the GPU with index ``device``.  TypeError for a non-tensor or a wrong dtype, ValueError for
    the wrong place, layout, shape or count."""
    # (what each tensor is, its layout included, before where it lies: a [3, n] tensor transposed has the right
    # shape and would be read as other rays, and the mistake shows without a GPU)
    _ray_pair_form(a, b, names)
    for t, name in zip((a, b), names):
        _device_place(t, name, device)
    return a.data_ptr(), b.data_ptr(), a.shape[0]


def _ray_pair_form(a, b, names):
    import torch

    for t, name in zip((a, b), names):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a torch tensor on the GPU is needed, not {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: dtype {t.dtype}, torch.float32 is needed")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name}: shape {tuple(t.shape)}, [n, 3] is needed")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"{names[0]} has {a.shape[0]} rows, {names[1]} {b.shape[0]}")
    for t, name in zip((a, b), names):
        _contiguous(t, name)


def device_segment_args(orig, dirs, tmax, device):
    """The checks of Renderer.occluded_device / trace_segments_device on their input tensors: (orig pointer, dirs
    pointer, tmax pointer or None, n).  orig, dirs as device_ray_args takes them; tmax: None (+inf for every ray)
    or a float32 tensor of one dimension and exactly n elements, contiguous, on the GPU with index ``device``.
    What every tensor is (layout included) before where any lies, so those mistakes show without a GPU."""
    import torch

    _ray_pair_form(orig, dirs, ("orig", "dirs"))
    n = orig.shape[0]
    if tmax is not None:
        if not isinstance(tmax, torch.Tensor):
            raise TypeError(f"tmax: a torch tensor on the GPU is needed, not {type(tmax).__name__}")
        if tmax.dtype != torch.float32:
            raise TypeError(f"tmax: dtype {tmax.dtype}, torch.float32 is needed")
        if tmax.dim() != 1 or tmax.shape[0] != n:
            raise ValueError(f"tmax: shape {tuple(tmax.shape)}, [{n}] is needed (one length per ray)")
        _contiguous(tmax, "tmax")
    for t, name in ((orig, "orig"), (dirs, "dirs")) + (() if tmax is None else ((tmax, "tmax"),)):
        _device_place(t, name, device)
    return orig.data_ptr(), dirs.data_ptr(), None if tmax is None else tmax.data_ptr(), n


def _contiguous(t, name):
    if not t.is_contiguous():
        raise ValueError(f"{name}: the tensor is not contiguous")


def _device_place(t, name, device):
    if not t.is_cuda:
        raise ValueError(f"{name}: the tensor is on {t.device}, not on a GPU")
    if t.device.index != int(device):
        raise ValueError(f"{name}: the tensor is on GPU {t.device.index}, the renderer on GPU {int(device)}")


def device_ray_out(t, name, dtype, n, device, cols=None):
    """An output tensor of a device ray query: ``dtype``, one dimension and at least n elements (cols: two
    dimensions, at least n rows of ``cols``), contiguous, placed as the inputs; its pointer."""
    _ray_out_form(t, name, dtype, n, cols)
    _device_place(t, name, device)
    return t.data_ptr()


def _ray_out_form(t, name, dtype, n, cols):
    import torch

    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a torch tensor on the GPU is needed, not {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: dtype {t.dtype}, {dtype} is needed")
    if cols is not None:
        if t.dim() != 2 or t.shape[1] != cols or t.shape[0] < n:
            raise ValueError(f"{name}: shape {tuple(t.shape)}, [>= {n}, {cols}] is needed")
    elif t.dim() != 1 or t.shape[0] < n:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, [>= {n}] is needed")
    _contiguous(t, name)


# the outputs of Renderer.trace_ray_device in the C call's order: (key, dtype, columns; None: [n])
SHADE_OUT = (("rgba", "float32", 4), ("hit_src", "int32", None), ("t", "float32", None),
             ("intersection_found", "uint8", None), ("shadowed", "uint8", None))


def device_shade_outs(out, n, device):
    """The checks of Renderer.trace_ray_device on its ``out`` dict: any subset of SHADE_OUT's keys that holds
    rgba, each tensor checked as device_ray_out checks it (rgba: [>= n, 4]), what every tensor is before where any
    lies; the five pointers, None for a key left out."""
    import torch

    if not isinstance(out, dict):
        raise TypeError(f"out: a dict of torch tensors is needed, not {type(out).__name__}")
    unknown = sorted(set(out) - {k for k, _, _ in SHADE_OUT})
    if unknown:
        raise ValueError(f"out: unknown key {unknown[0]!r}")
    if "rgba" not in out:
        raise ValueError("out: rgba is needed (the other outputs may be left out)")
    given = [(k, dt, c) for k, dt, c in SHADE_OUT if k in out]
    for k, dt, c in given:
        _ray_out_form(out[k], k, getattr(torch, dt), n, c)
    for k, _, _ in given:
        _device_place(out[k], k, device)
    return [out[k].data_ptr() if k in out else None for k, _, _ in SHADE_OUT]


# the outputs of Renderer.visibility_device in the C call's order: (key, dtype, trailing dimension; None: [rh, rw])
VISIBILITY_OUT = (("tri_id", "int32", None), ("t", "float32", None), ("uv", "float32", 2))


def device_visibility_outs(out, rw, rh, device):
    """The checks of Renderer.visibility_device on its ``out`` dict: any non-empty subset of VISIBILITY_OUT's keys,
    each a contiguous torch tensor of exactly [rh, rw] (uv: [rh, rw, 2]) and its dtype on the GPU with index
    ``device``; what every tensor is (layout included) before where any lies, so those mistakes show without a
    GPU; the three pointers, None for a key left out."""
    import torch

    if not isinstance(out, dict):
        raise TypeError(f"out: a dict of torch tensors is needed, not {type(out).__name__}")
    unknown = sorted(set(out) - {k for k, _, _ in VISIBILITY_OUT})
    if unknown:
        raise ValueError(f"out: unknown key {unknown[0]!r}")
    given = [(k, getattr(torch, dt), c) for k, dt, c in VISIBILITY_OUT if k in out]
    if not given:
        raise ValueError("out: at least one of tri_id, t, uv is needed")
    for k, dtype, c in given:
        t = out[k]
        shape = (rh, rw) if c is None else (rh, rw, c)
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{k}: a torch tensor on the GPU is needed, not {type(t).__name__}")
        if t.dtype != dtype:
            raise TypeError(f"{k}: dtype {t.dtype}, {dtype} is needed")
        if tuple(t.shape) != shape:
            raise ValueError(f"{k}: shape {tuple(t.shape)}, {list(shape)} is needed")
        _contiguous(t, k)
    for k, _, _ in given:
        _device_place(out[k], k, device)
    return [out[k].data_ptr() if k in out else None for k, _, _ in VISIBILITY_OUT]


def load_obj(path, xform, mat_offset=0):
    """read_meshio_data + create_triangles -> (tri9, mat, uv6 or None, mats16)."""
    xform = f32(xform)
    L = lib()
    h = L.rt_obj_open(path.encode(), ptr(xform, _f32p), mat_offset)
    if not h:
        raise RuntimeError(f"rt_obj_open({path}): {L.rt_last_error().decode()}")
    try:
        n = C.c_int64()
        nm = C.c_int32()
        has_uv = C.c_int32()
        check(L.rt_obj_counts(h, C.byref(n), C.byref(nm), C.byref(has_uv)), "rt_obj_counts")
        tri = np.zeros((n.value, 9), np.float32)
        mat = np.zeros(n.value, np.int32)
        uv = np.zeros((n.value, 6), np.float32) if has_uv.value else None
        mats = np.zeros((nm.value, 16), np.float32)
        check(L.rt_obj_fetch(h, ptr(tri, _f32p), ptr(mat, _i32p), ptr(uv, _f32p), ptr(mats, _f32p)), "rt_obj_fetch")
        return tri, mat, uv, mats
    finally:
        L.rt_obj_close(h)


def wbvh_query(tri9, orig, dirs, max_depth=12, leaf=40, cam=None, light=None, shadow_rays=False, rays_out=False,
               ray_nodes=None, ocone_dim=0, oc_stats=None, entry=None):
    """rt_wbvh_query(_ex): the wide-BVH certified closest hit on the host (no GPU).  Returns
    (status, id, t, u, v, stats dict, (octree ms, wide-BVH ms)); status 0 certified miss,
    1 certified hit, 2 not certified.  cam / light: the frame's grazing-risk points (rays from cam
    read the camera's bits); shadow_rays: orig / dirs are hit points and normals, traced as
    is_shadowed's rays towards light.  rays_out: (o, d) of the queried rays are appended.
    entry: dict(proj_inv, cam_to_world, rw, rh, pixel [n, 2][, k, fan, depth, quick, no_cull]) -- the camera rays
    start at their blocks' entry sets; it receives 'sets' [block rows, blocks per row, 4],
    'has_mask', 'covered', 'depth_hist' and 'close_hist'."""
    tri9 = f32(tri9).reshape(-1, 9)
    o = f32(orig).reshape(-1, 3)
    d = f32(dirs).reshape(-1, 3)
    n = o.shape[0]
    st = np.zeros(n, np.int32)
    ids = np.zeros(n, np.int32)
    t, u, v = (np.zeros(n, np.float32) for _ in range(3))
    stats = np.zeros(8, np.int64)
    ms = np.zeros(2, np.float32)
    oo = np.zeros((n, 3), np.float32)
    do = np.zeros((n, 3), np.float32)
    c = None if cam is None else f32(cam).reshape(3)
    li = None if light is None else f32(light).reshape(3)
    ep = None
    if entry is not None:
        ep = RtEntryProbe()
        ep.proj_inv[:] = [float(x) for x in f32(entry["proj_inv"]).ravel()]
        ep.cam_to_world[:] = [float(x) for x in f32(entry["cam_to_world"]).ravel()]
        ep.rw, ep.rh = int(entry["rw"]), int(entry["rh"])
        ep.k, ep.fan, ep.depth = (int(entry.get(x, 0)) for x in ("k", "fan", "depth"))
        ep.quick = int(entry.get("quick", 0))
        ep.no_cull = int(entry.get("no_cull", 0))
        pix = np.ascontiguousarray(entry["pixel"], np.int32).reshape(-1, 2)
        assert pix.shape[0] == n
        sets = np.zeros(((ep.rh + 7) // 8, (ep.rw + 7) // 8, 4), np.uint32)
        ep.pixel = ptr(pix, _i32p)
        ep.sets = ptr(sets, _u32p)
    check(lib().rt_wbvh_query_ex(ptr(tri9, _f32p), tri9.shape[0], max_depth, leaf, ptr(o, _f32p), ptr(d, _f32p), n,
                                 None if c is None else ptr(c, _f32p), None if li is None else ptr(li, _f32p),
                                 1 if shadow_rays else 0, ptr(oo, _f32p), ptr(do, _f32p),
                                 ptr(st, _i32p), ptr(ids, _i32p), ptr(t, _f32p), ptr(u, _f32p), ptr(v, _f32p),
                                 ptr(stats, _i64p), ptr(ms, _f32p),
                                 None if ray_nodes is None else ptr(ray_nodes, _i32p), int(ocone_dim),
                                 None if oc_stats is None else ptr(oc_stats, _i64p),
                                 None if ep is None else C.byref(ep)), "rt_wbvh_query")
    if ep is not None:
        entry.update(sets=sets, has_mask=bool(ep.info[2]), covered=int(ep.info[3]), depth_hist=[int(x) for x in ep.depth_hist],
                     close_hist=[int(x) for x in ep.close_hist])
    keys = ("nodes", "leaves", "max_leaf", "depth", "node_visits", "tri_tests", "violations", "sah_x1000")
    out = (st, ids, t, u, v, dict(zip(keys, map(int, stats))), (float(ms[0]), float(ms[1])))
    return out + (oo, do) if rays_out else out


def ocone_check(tri9, orig, dirs, max_depth=12, leaf=40, ocone_dim=64, grid=None, want_cells=False):
    """rt_ocone_check: (skip flags, dict[, cells]) -- the origin cones' brute-force soundness check (no
    GPU).  grid: (cells uint32 [n, 2], dims, lo_ih) to check instead of building one (Renderer.ocone_read);
    want_cells: also return the built grid's words."""
    tri9 = f32(tri9).reshape(-1, 9)
    o = f32(orig).reshape(-1, 3)
    d = f32(dirs).reshape(-1, 3)
    skip = np.zeros(o.shape[0], np.int32)
    out = np.zeros(6, np.int64)
    _u32p = C.POINTER(C.c_uint32)
    cells = dims = lo_ih = None
    if grid is not None:
        cells = np.ascontiguousarray(grid[0], np.uint32)
        dims = np.ascontiguousarray(grid[1], np.int32)
        lo_ih = f32(grid[2])
    built = None
    if want_cells:
        # the grid's size: the renderer's frame (ocone_dim + 2 cells at most per axis)
        built = np.zeros(((ocone_dim + 2) ** 3, 2), np.uint32)
    check(lib().rt_ocone_check(ptr(tri9, _f32p), tri9.shape[0], max_depth, leaf, ocone_dim, ptr(o, _f32p),
                               ptr(d, _f32p), o.shape[0], ptr(skip, _i32p), ptr(out, _i64p),
                               None if cells is None else ptr(cells, _u32p), None if dims is None else ptr(dims, _i32p),
                               None if lo_ih is None else ptr(lo_ih, _f32p), None if built is None else ptr(built, _u32p)),
          "rt_ocone_check")
    keys = ("violations", "skipping", "grazing_tests", "cells", "empty_cells", "noskip_cells")
    res = (skip, dict(zip(keys, map(int, out))))
    return res + (built,) if want_cells else res


def risk_cap_check(tri9, cam, dirs, max_depth=12, leaf=40, cap_override=-1.0):
    """rt_risk_cap_check: (skip flags, dict) -- the camera risk cap's brute-force soundness check (no GPU)."""
    tri9 = f32(tri9).reshape(-1, 9)
    c = f32(cam).reshape(3)
    d = f32(dirs).reshape(-1, 3)
    skip = np.zeros(d.shape[0], np.int32)
    out = np.zeros(4, np.int64)
    check(lib().rt_risk_cap_check(ptr(tri9, _f32p), tri9.shape[0], max_depth, leaf, ptr(c, _f32p), ptr(d, _f32p),
                                  d.shape[0], float(cap_override), ptr(skip, _i32p), ptr(out, _i64p)), "rt_risk_cap_check")
    return skip, {"violations": int(out[0]), "skipping": int(out[1]), "grazing_tests": int(out[2]),
                  "cap": float(out[3]) * 1e-9 if out[3] >= 0 else None}


def octree_digest(tri9, max_depth=12, leaf=40, builder=0):
    """rt_octree_digest: (digest, stats dict, build ms) of the flattened host octree (no GPU)."""
    tri9 = f32(tri9).reshape(-1, 9)
    dg = C.c_uint64()
    st = np.zeros(7, np.int64)
    ms = C.c_float()
    check(lib().rt_octree_digest(ptr(tri9, _f32p), tri9.shape[0], max_depth, leaf, builder, C.byref(dg),
                                 ptr(st, _i64p), C.byref(ms)), "rt_octree_digest")
    keys = ("inner", "leaves", "empty_leaves", "max_leaf", "max_depth", "nodes", "levels")
    return int(dg.value), dict(zip(keys, map(int, st))), float(ms.value)


_WQ_STATS = ("nodes", "leaves", "tris", "max_leaf", "depth")


def wbvh_quick_digest(tri9, max_depth=12, leaf=40):
    """rt_wbvh_quick_digest: (six digests, stats dict, build ms) of the quick wide BVH built on the host
    (no GPU).  Digests: exact node fields, slabs, conditioning bytes, transcendental bytes (cone code,
    sth), slot maps, links."""
    tri9 = f32(tri9).reshape(-1, 9)
    dg = (C.c_uint64 * 6)()
    st = np.zeros(5, np.int64)
    ms = C.c_float()
    check(lib().rt_wbvh_quick_digest(ptr(tri9, _f32p), tri9.shape[0], max_depth, leaf, dg, ptr(st, _i64p),
                                     C.byref(ms)), "rt_wbvh_quick_digest")
    return tuple(int(x) for x in dg), dict(zip(_WQ_STATS, map(int, st))), float(ms.value)


def wbvh_quick_build_device(tri9, max_depth=12, leaf=40, device=0):
    """rt_wbvh_quick_build_device: (six digests, stats dict, check dict, (device quick build ms, whole call
    ms)) of the quick wide BVH built on the GPU from the device-built octree.  check: violations
    (check_wbvh of the downloaded tree), trans_diff / trans_max (transcendental bytes differing from the
    host tree's, the largest code difference), other_diff (differing bytes elsewhere)."""
    tri9 = f32(tri9).reshape(-1, 9)
    dg = (C.c_uint64 * 6)()
    st = np.zeros(5, np.int64)
    ck = np.zeros(4, np.int64)
    ms = np.zeros(2, np.float32)
    check(lib().rt_wbvh_quick_build_device(device, ptr(tri9, _f32p), tri9.shape[0], max_depth, leaf, dg,
                                           ptr(st, _i64p), ptr(ck, _i64p), ptr(ms, _f32p)),
          "rt_wbvh_quick_build_device")
    keys = ("violations", "trans_diff", "trans_max", "other_diff")
    return (tuple(int(x) for x in dg), dict(zip(_WQ_STATS, map(int, st))), dict(zip(keys, map(int, ck))),
            (float(ms[0]), float(ms[1])))


def octree_build_device(tri9, max_depth=12, leaf=40, device=0):
    """rt_octree_build_device: (digest, stats dict, (device build ms, whole call ms)) of the octree built on
    the GPU, digested as octree_digest does.  Raises RtError (RT_EUNSUPPORTED: the builder does not take the
    input; RT_EHIP: no usable device)."""
    tri9 = f32(tri9).reshape(-1, 9)
    dg = C.c_uint64()
    st = np.zeros(7, np.int64)
    ms = np.zeros(2, np.float32)
    check(lib().rt_octree_build_device(device, ptr(tri9, _f32p), tri9.shape[0], max_depth, leaf, C.byref(dg),
                                       ptr(st, _i64p), ptr(ms, _f32p)), "rt_octree_build_device")
    keys = ("inner", "leaves", "empty_leaves", "max_leaf", "max_depth", "nodes", "levels")
    return int(dg.value), dict(zip(keys, map(int, st))), (float(ms[0]), float(ms[1]))
