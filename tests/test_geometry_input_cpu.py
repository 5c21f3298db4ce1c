"""The geometry-input entry points (rt_set_triangles_device, rt_update_vertices_device, rt_get_device_ingests,
rt_gather_triangles_device, rt_set_accel_deferred, rt_get_accel_builds) where no GPU is needed: their error
returns, and the Python mirror's checks of its tensors."""
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


def _args(n=4, indexed=True):
    rng = np.random.default_rng(5)
    nv = 7 if indexed else 3 * n
    verts = rng.uniform(-1, 1, (max(nv, 1), 3)).astype(np.float32)
    idx = rng.integers(0, nv, (max(n, 1), 3)).astype(np.int32) if indexed else None
    out = np.full((max(n, 1), 9), 7.0, np.float32)
    return verts, nv, idx, out, C.c_int32(7), np.zeros(2, np.float32)


def _call(verts, nv, idx, n, out, flags, ms):
    p = _lib.ptr
    return _lib.lib().rt_gather_triangles_device(0, p(verts, _lib._f32p), nv, p(idx, _lib._i32p), n, p(out, _lib._f32p),
                                                 None if flags is None else C.byref(flags), p(ms, _lib._f32p))


def test_null_handles():
    L = _lib.lib()
    n = C.c_int64()
    mat = np.zeros(4, np.int32)
    v = C.c_void_p(4096)   # (never read: the handle is checked first)
    assert L.rt_set_triangles_device(None, v, 12, None, _lib.ptr(mat, _lib._i32p), None, 4, None) == -1   # RT_EINVAL
    assert L.rt_update_vertices_device(None, v, 12, None, None) == -1
    assert L.rt_get_device_ingests(None, C.byref(n)) == -1
    assert L.rt_get_device_ingests(None, None) == -1
    assert L.rt_set_accel_deferred(None, 1) == -1
    assert L.rt_get_accel_builds(None, C.byref(n)) == -1
    assert L.rt_get_accel_builds(None, None) == -1
    assert L.rt_last_error().decode() == "null renderer handle"


@pytest.mark.parametrize("missing", ["verts", "out", "flags"])
@pytest.mark.parametrize("indexed", [True, False], ids=["indexed", "flat"])
def test_gather_null_pointers(missing, indexed):
    verts, nv, idx, out, flags, ms = _args(4, indexed)
    a = {"verts": verts, "out": out, "flags": flags}
    a[missing] = None
    assert _call(a["verts"], nv, idx, 4, a["out"], a["flags"], ms) == -1
    assert _lib.lib().rt_last_error().decode().startswith("rt_gather_triangles_device:")


def test_gather_negative_counts_and_flat_mismatch():
    verts, nv, idx, out, flags, ms = _args()
    assert _call(verts, nv, idx, -1, out, flags, ms) == -1
    assert _call(verts, -1, idx, 4, out, flags, ms) == -1
    assert _call(verts, nv, idx, -(1 << 40), out, flags, None) == -1
    # the flat form is [n][9]: nv == 3 n
    assert _call(verts, nv, None, 4, out, flags, ms) == -1
    assert np.all(out == 7.0)


@pytest.mark.parametrize("indexed", [True, False], ids=["indexed", "flat"])
def test_gather_empty_needs_no_device(indexed):
    """n == 0: RT_OK without a launch (and without touching a device), the flags cleared."""
    verts, nv, idx, out, flags, ms = _args(0, indexed)
    assert _call(verts, nv, idx, 0, out, flags, ms) == 0
    assert flags.value == 0 and np.all(out == 7.0)
    # (the pointers are not read)
    flags = C.c_int32(7)
    assert _call(None, 0, None, 0, None, flags, None) == 0 and flags.value == 0
    got, f, _ = _lib.gather_triangles_device(np.zeros((0, 9), np.float32))
    assert got.shape == (0, 9) and f == 0
    got, f, _ = _lib.gather_triangles_device(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32))
    assert got.shape == (0, 9) and f == 0


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the call gathers")
def test_gather_without_gpu_is_an_error_not_a_crash():
    verts, nv, idx, out, flags, ms = _args(4)
    assert _call(verts, nv, idx, 4, out, flags, ms) == -2   # RT_EHIP
    assert _lib.lib().rt_last_error().decode().startswith("rt_gather_triangles_device:")
    with pytest.raises(_lib.RtError, match="RT_EHIP"):
        _lib.gather_triangles_device(verts, idx)


# ---- the Python mirror's checks (no renderer, no GPU: every case fails before a pointer is taken) ----

def test_helper_rejects_what_is_not_a_gpu_tensor():
    torch = pytest.importorskip("torch")
    check = _lib.device_geometry_args
    with pytest.raises(TypeError, match="torch tensor"):
        check(np.zeros((4, 9), np.float32), None, 0)
    with pytest.raises(TypeError, match="torch tensor"):
        check([[0.0] * 9], None, 0)
    with pytest.raises(ValueError, match="not on a GPU"):
        check(torch.zeros(4, 9), None, 0)
    with pytest.raises(ValueError, match="not on a GPU"):
        check(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), 0)


def test_helper_rejects_wrong_dtype_and_shape():
    """(dtype and shape are checked before the tensor's place, so CPU tensors show them.)"""
    torch = pytest.importorskip("torch")
    check = _lib.device_geometry_args
    for bad in (torch.zeros(4, 9, dtype=torch.float64), torch.zeros(4, 9, dtype=torch.float16),
                torch.zeros(4, 9, dtype=torch.int32)):
        with pytest.raises(TypeError, match="verts: dtype"):
            check(bad, None, 0)
    for bad in (torch.zeros(4, 8), torch.zeros(36), torch.zeros(4, 3), torch.zeros(2, 2, 9)):
        with pytest.raises(ValueError, match="verts: shape"):
            check(bad, None, 0)
    # the indexed form: verts [nv, 3], indices int32 [n, 3]
    with pytest.raises(ValueError, match="verts: shape"):
        check(torch.zeros(4, 9), torch.zeros(2, 3, dtype=torch.int32), 0)
    with pytest.raises(TypeError, match="indices: a torch tensor"):
        check(torch.zeros(4, 3), np.zeros((2, 3), np.int32), 0)
    with pytest.raises(TypeError, match="indices: dtype"):
        check(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="indices: shape"):
        check(torch.zeros(4, 3), torch.zeros(6, dtype=torch.int32), 0)
