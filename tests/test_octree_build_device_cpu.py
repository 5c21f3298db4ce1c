"""The device octree build's entry points where no GPU is needed: their error returns."""
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


def _call(tri, depth, leaf):
    tri = _lib.f32(tri).reshape(-1, 9)
    dg = C.c_uint64()
    st = np.zeros(7, np.int64)
    ms = np.zeros(2, np.float32)
    return _lib.lib().rt_octree_build_device(0, _lib.ptr(tri, _lib._f32p), tri.shape[0], depth, leaf, C.byref(dg),
                                             _lib.ptr(st, _lib._i64p), _lib.ptr(ms, _lib._f32p))


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the call builds")
def test_build_device_without_gpu_is_an_error_not_a_crash():
    tri = np.random.default_rng(1).uniform(-1, 1, (100, 9)).astype(np.float32)
    assert _call(tri, 12, 40) == -2   # RT_EHIP
    assert _lib.lib().rt_last_error().decode().startswith("rt_octree_build_device:")
    with pytest.raises(_lib.RtError, match="RT_EHIP"):
        _lib.octree_build_device(tri, 12, 40)


def test_build_device_unsupported_inputs():
    """Outside the builder's range the answer is RT_EUNSUPPORTED before any device is touched."""
    tri = np.random.default_rng(2).uniform(-1, 1, (10, 9)).astype(np.float32)
    assert _call(tri, 31, 40) == -5
    assert _call(tri, -1, 40) == -5
    bad = tri.copy()
    bad[3, 4] = np.nan
    assert _call(bad, 12, 40) == -5


def test_device_build_switch_rejects_null_handle():
    L = _lib.lib()
    assert L.rt_set_device_build(None, 1) == -1   # RT_EINVAL
    n = C.c_int64()
    assert L.rt_get_device_builds(None, C.byref(n)) == -1
    assert L.rt_octree_build_device(0, None, 5, 12, 40, None, None, None) == -1
