"""The device ray queries (rt_trace_rays_device, rt_is_shadowed_device, rt_get_device_ray_queries) where no
GPU is needed: the exported symbols and their declarations, the error returns on a null handle, and the
Python mirror's checks of its tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytracercpp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_trace_rays_device", "rt_is_shadowed_device", "rt_get_device_ray_queries")


def test_symbols_exported_and_declared():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by the library"
        assert re.search(r"^int %s\(rt_renderer \*r," % name, header, re.M), f"{name} is not declared in rt_mi355x.h"
        assert name in _lib.SIGNATURES and _lib.has(name)


def test_null_handles():
    L = _lib.lib()
    v = C.c_void_p(4096)   # (never read: the handle is checked first)
    calls, rays = np.zeros(2, np.int64), np.zeros(2, np.int64)
    light = np.zeros(3, np.float32)
    assert L.rt_trace_rays_device(None, v, v, 4, v, v, v, v, v, v, None) == -1   # RT_EINVAL
    assert L.rt_trace_rays_device(None, None, None, 0, None, None, None, None, None, None, None) == -1
    assert L.rt_is_shadowed_device(None, v, v, 4, _lib.ptr(light, _lib._f32p), v, None) == -1
    assert L.rt_is_shadowed_device(None, v, v, 4, None, v, None) == -1
    assert L.rt_get_device_ray_queries(None, _lib.ptr(calls, _lib._i64p), _lib.ptr(rays, _lib._i64p)) == -1
    assert L.rt_get_device_ray_queries(None, None, None) == -1
    assert L.rt_last_error().decode() == "null renderer handle"


# ---- the Python mirror's checks (no renderer, no GPU: every case fails before a pointer is taken) ----

def test_helper_rejects_what_is_not_a_tensor():
    torch = pytest.importorskip("torch")
    check = _lib.device_ray_args
    good = torch.zeros(4, 3)
    with pytest.raises(TypeError, match="orig: a torch tensor"):
        check(np.zeros((4, 3), np.float32), good, 0)
    with pytest.raises(TypeError, match="dirs: a torch tensor"):
        check(good, np.zeros((4, 3), np.float32), 0)
    with pytest.raises(TypeError, match="points: a torch tensor"):
        check([[0.0, 0.0, 0.0]], good, 0, ("points", "normals"))


def test_helper_rejects_wrong_dtype_shape_and_count():
    """(What a tensor is comes before where it lies, so CPU tensors show each kind of mistake.)"""
    torch = pytest.importorskip("torch")
    check = _lib.device_ray_args
    good = torch.zeros(4, 3)
    for bad in (torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float16)):
        with pytest.raises(TypeError, match="orig: dtype"):
            check(bad, good, 0)
        with pytest.raises(TypeError, match="dirs: dtype"):
            check(good, bad, 0)
    for bad in (torch.zeros(12), torch.zeros(4, 4), torch.zeros(3, 4)):
        with pytest.raises(ValueError, match="orig: shape"):
            check(bad, good, 0)
        with pytest.raises(ValueError, match="normals: shape"):
            check(good, bad, 0, ("points", "normals"))
    # a wrong dtype shows before a wrong shape, a wrong shape before unequal counts
    with pytest.raises(TypeError, match="orig: dtype"):
        check(torch.zeros(4, 4, dtype=torch.float64), torch.zeros(5, 3), 0)
    with pytest.raises(ValueError, match="dirs: shape"):
        check(good, torch.zeros(5, 4), 0)
    with pytest.raises(ValueError, match="orig has 4 rows, dirs 5"):
        check(good, torch.zeros(5, 3), 0)


def test_helper_rejects_cpu_tensors_and_views():
    torch = pytest.importorskip("torch")
    check = _lib.device_ray_args
    # unequal counts show before the place
    with pytest.raises(ValueError, match="rows"):
        check(torch.zeros(4, 3), torch.zeros(5, 3), 0)
    with pytest.raises(ValueError, match="orig: the tensor is on cpu, not on a GPU"):
        check(torch.zeros(4, 3), torch.zeros(4, 3), 0)
    # a non-contiguous view ([3, n] transposed, a strided slice) has the right shape and would be read as other
    # rays: the layout is checked before the place, so the mistake shows here
    view = torch.zeros(3, 4).t()
    assert tuple(view.shape) == (4, 3) and not view.is_contiguous()
    with pytest.raises(ValueError, match="orig: the tensor is not contiguous"):
        check(view, torch.zeros(4, 3), 0)
    with pytest.raises(ValueError, match="dirs: the tensor is not contiguous"):
        check(torch.zeros(4, 3), torch.zeros(8, 3)[::2], 0)
    with pytest.raises(ValueError, match="normals: the tensor is not contiguous"):
        check(torch.zeros(4, 3), view, 0, ("points", "normals"))
    with pytest.raises(ValueError, match="t: the tensor is not contiguous"):
        _lib.device_ray_out(torch.zeros(8)[::2], "t", torch.float32, 4, 0)


def test_output_helper():
    torch = pytest.importorskip("torch")
    out = _lib.device_ray_out
    with pytest.raises(TypeError, match="t: a torch tensor"):
        out(np.zeros(4, np.float32), "t", torch.float32, 4, 0)
    with pytest.raises(TypeError, match="tri_id: dtype"):
        out(torch.zeros(4, dtype=torch.int64), "tri_id", torch.int32, 4, 0)
    with pytest.raises(ValueError, match="ret: shape"):
        out(torch.zeros(3, dtype=torch.uint8), "ret", torch.uint8, 4, 0)
    with pytest.raises(ValueError, match="ret: shape"):
        out(torch.zeros(4, 1, dtype=torch.uint8), "ret", torch.uint8, 4, 0)
    with pytest.raises(ValueError, match="not on a GPU"):
        out(torch.zeros(8, dtype=torch.uint8), "ret", torch.uint8, 4, 0)
