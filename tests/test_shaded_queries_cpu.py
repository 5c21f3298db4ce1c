"""The shaded device query (rt_trace_ray_device, rt_get_device_shaded_queries) where no GPU is needed: the
exported symbols and their declarations, the error returns on a null handle, and the Python mirror's checks of
its tensors (what a tensor is, its layout included, before where it lies: CPU tensors show each mistake)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytracercpp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_trace_ray_device", "rt_get_device_shaded_queries")
KEYS = ("rgba", "hit_src", "t", "intersection_found", "shadowed")


def test_symbols_exported_and_declared():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by the library"
        assert re.search(r"^int %s\(rt_renderer \*r," % name, header, re.M), f"{name} is not declared in rt_mi355x.h"
        assert name in _lib.SIGNATURES and _lib.has(name)
    # the declaration's parameters, in the order the mirror passes them
    decl = re.search(r"^int rt_trace_ray_device\((.*?)\);", header, re.M | re.S).group(1)
    names = [p.split()[-1].lstrip("*") for p in decl.split(",")]
    assert names == ["r", "d_orig", "d_dir", "n", "current_recursion_depth", "first_ray", "d_rgba", "d_hit_src", "d_t",
                     "d_found", "d_shadowed", "d_counts", "hip_stream"]
    assert len(_lib.SIGNATURES["rt_trace_ray_device"][1]) == len(names)


def test_null_handles():
    L = _lib.lib()
    v = C.c_void_p(4096)   # (never read: the handle is checked first)
    calls, rays = np.zeros(3, np.int64), np.zeros(3, np.int64)
    assert L.rt_trace_ray_device(None, v, v, 4, 0, 0, v, v, v, v, v, v, None) == -1   # RT_EINVAL
    assert L.rt_last_error().decode() == "null renderer handle"
    assert L.rt_trace_ray_device(None, None, None, 0, 0, 0, None, None, None, None, None, None, None) == -1
    assert L.rt_get_device_shaded_queries(None, _lib.ptr(calls, _lib._i64p), _lib.ptr(rays, _lib._i64p)) == -1
    assert L.rt_get_device_shaded_queries(None, None, None) == -1
    assert L.rt_last_error().decode() == "null renderer handle"


def _out(torch, n=4):
    return dict(rgba=torch.zeros(n, 4), hit_src=torch.zeros(n, dtype=torch.int32), t=torch.zeros(n),
                intersection_found=torch.zeros(n, dtype=torch.uint8), shadowed=torch.zeros(n, dtype=torch.uint8))


def test_outputs_are_checked_by_name():
    torch = pytest.importorskip("torch")
    check = _lib.device_shade_outs
    assert [k for k, _, _ in _lib.SHADE_OUT] == list(KEYS)
    # a numpy array
    for k in KEYS:
        out = _out(torch)
        out[k] = out[k].numpy()
        with pytest.raises(TypeError, match=f"{k}: a torch tensor"):
            check(out, 4, 0)
    with pytest.raises(TypeError, match="out: a dict"):
        check(np.zeros((4, 4), np.float32), 4, 0)
    # a wrong dtype
    for k, bad in (("rgba", torch.float64), ("hit_src", torch.int64), ("t", torch.float16),
                   ("intersection_found", torch.bool), ("shadowed", torch.int32)):
        out = _out(torch)
        out[k] = out[k].to(bad)
        with pytest.raises(TypeError, match=f"{k}: dtype"):
            check(out, 4, 0)
    # [n, 3] given for rgba, and the other shapes that are not [n, 4]
    for bad in (torch.zeros(4, 3), torch.zeros(16), torch.zeros(4, 4, 1), torch.zeros(4, 5)):
        with pytest.raises(ValueError, match=r"rgba: shape .* \[>= 4, 4\] is needed"):
            check(dict(_out(torch), rgba=bad), 4, 0)
    with pytest.raises(ValueError, match="t: shape"):
        check(dict(_out(torch), t=torch.zeros(4, 1)), 4, 0)
    # fewer than n rows
    with pytest.raises(ValueError, match="rgba: shape"):
        check(dict(_out(torch), rgba=torch.zeros(3, 4)), 4, 0)
    with pytest.raises(ValueError, match="shadowed: shape"):
        check(dict(_out(torch), shadowed=torch.zeros(3, dtype=torch.uint8)), 4, 0)
    # a transposed or strided rgba has the right shape and would be written between the caller's elements
    transposed = torch.zeros(4, 4).t()
    strided = torch.zeros(8, 4)[::2]
    columns = torch.zeros(4, 8)[:, :4]
    for bad in (transposed, strided, columns):
        assert tuple(bad.shape) == (4, 4)
    for bad in (strided, columns):
        with pytest.raises(ValueError, match="rgba: the tensor is not contiguous"):
            check(dict(_out(torch), rgba=bad), 4, 0)
    t5 = torch.zeros(4, 5).t()[:4]   # [4, 4] rows of a transposed [5, 4]
    assert tuple(t5.shape) == (4, 4) and not t5.is_contiguous()
    with pytest.raises(ValueError, match="rgba: the tensor is not contiguous"):
        check(dict(_out(torch), rgba=t5), 4, 0)
    with pytest.raises(ValueError, match="hit_src: the tensor is not contiguous"):
        check(dict(_out(torch), hit_src=torch.zeros(8, dtype=torch.int32)[::2]), 4, 0)
    # an out without rgba, and a key the call does not know
    for k in KEYS[1:]:
        with pytest.raises(ValueError, match="out: rgba is needed"):
            check({k: _out(torch)[k]}, 4, 0)
    with pytest.raises(ValueError, match="out: rgba is needed"):
        check({}, 4, 0)
    with pytest.raises(ValueError, match="out: unknown key 'tri_id'"):
        check(dict(_out(torch), tri_id=torch.zeros(4, dtype=torch.int32)), 4, 0)
    # every check of what the tensors are passes: where they lie comes last
    with pytest.raises(ValueError, match="rgba: the tensor is on cpu, not on a GPU"):
        check(_out(torch), 4, 0)
    with pytest.raises(ValueError, match="rgba: the tensor is on cpu, not on a GPU"):
        check(dict(rgba=torch.zeros(9, 4)), 4, 0)


def test_square_transposed_rgba_is_caught_by_its_strides():
    """A transposed [4, 4] is the one shape whose transpose has the same shape; torch calls it non-contiguous."""
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="rgba: the tensor is not contiguous"):
        _lib.device_shade_outs(dict(rgba=torch.zeros(4, 4).t()), 4, 0)
