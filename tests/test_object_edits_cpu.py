"""The object-edit entry points (rt_get_triangles, rt_get_device_transforms, rt_transform_points_device)
where no GPU is needed: their error returns."""
import ctypes as C

import numpy as np
import pytest

from raytracercpp_amd import _lib


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def _args(n=5):
    m = _lib.make_transform("ry", 25)
    pts = np.random.default_rng(3).uniform(-1, 1, (max(n, 1), 3)).astype(np.float32)
    out = np.zeros_like(pts)
    flag = C.c_int32(7)
    ms = np.zeros(2, np.float32)
    return m, pts, out, flag, ms


def _call(m, pts, n, out, flag, ms):
    p = _lib.ptr
    return _lib.lib().rt_transform_points_device(0, p(m, _lib._f32p), p(pts, _lib._f32p), n, p(out, _lib._f32p),
                                                 None if flag is None else C.byref(flag), p(ms, _lib._f32p))


def test_null_handles():
    L = _lib.lib()
    n = C.c_int64()
    tri = np.zeros((4, 9), np.float32)
    assert L.rt_get_triangles(None, _lib.ptr(tri, _lib._f32p), C.byref(n)) == -1   # RT_EINVAL
    assert L.rt_get_triangles(None, None, None) == -1
    assert L.rt_get_device_transforms(None, C.byref(n)) == -1
    assert L.rt_get_device_transforms(None, None) == -1
    assert L.rt_last_error().decode() == "null renderer handle"


@pytest.mark.parametrize("missing", ["m", "pts", "out", "nonfinite"])
def test_transform_points_device_null_pointers(missing):
    m, pts, out, flag, ms = _args()
    a = {"m": m, "pts": pts, "out": out, "nonfinite": flag}
    a[missing] = None
    assert _call(a["m"], a["pts"], 5, a["out"], a["nonfinite"], ms) == -1
    assert _lib.lib().rt_last_error().decode().startswith("rt_transform_points_device:")
    # (also with nothing to do)
    assert _call(a["m"], a["pts"], 0, a["out"], a["nonfinite"], ms) == -1


def test_transform_points_device_negative_count():
    m, pts, out, flag, ms = _args()
    assert _call(m, pts, -1, out, flag, ms) == -1
    assert _call(m, pts, -(1 << 40), out, flag, None) == -1


def test_transform_points_device_empty_needs_no_device():
    """n == 0: RT_OK without a launch (and without touching a device), the flag cleared."""
    m, pts, out, flag, ms = _args(0)
    assert _call(m, pts, 0, out, flag, ms) == 0
    assert flag.value == 0
    got, f, _ = _lib.transform_points_device(m, np.zeros((0, 3), np.float32))
    assert got.shape == (0, 3) and f == 0


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the call transforms")
def test_transform_points_device_without_gpu_is_an_error_not_a_crash():
    m, pts, out, flag, ms = _args(100)
    assert _call(m, pts, 100, out, flag, ms) == -2   # RT_EHIP
    assert _lib.lib().rt_last_error().decode().startswith("rt_transform_points_device:")
    with pytest.raises(_lib.RtError, match="RT_EHIP"):
        _lib.transform_points_device(m, pts)
