"""Shaded ray batches through the frame engine (rt_trace_ray_batch_device, rt_get_device_shaded_batches) where no
GPU is needed: the exported symbols and their declarations, the parameter order against rt_trace_ray_device's, the
error returns on a null handle, and the Python mirror's checks of its tensors, which must refuse by name what
trace_ray_device refuses (CPU tensors show each mistake: what a tensor is comes before where it lies)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from raytracercpp_amd import _lib
from raytracercpp_amd.renderer import Renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_trace_ray_batch_device", "rt_get_device_shaded_batches")
KEYS = ("rgba", "hit_src", "t", "intersection_found", "shadowed")


def _params(header, name):
    decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
    return [" ".join(p.split()) for p in decl.split(",")]


def test_symbols_exported_and_declared():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by the library"
        assert re.search(r"^int %s\(rt_renderer \*r," % name, header, re.M), f"{name} is not declared in rt_mi355x.h"
        assert name in _lib.SIGNATURES and _lib.has(name)
    # the arguments are rt_trace_ray_device's: the same types and names in the same order, in the header and the mirror
    batch, single = _params(header, "rt_trace_ray_batch_device"), _params(header, "rt_trace_ray_device")
    assert batch == single
    assert [p.split()[-1].lstrip("*") for p in batch] == [
        "r", "d_orig", "d_dir", "n", "current_recursion_depth", "first_ray", "d_rgba", "d_hit_src", "d_t", "d_found",
        "d_shadowed", "d_counts", "hip_stream"]
    assert _lib.SIGNATURES["rt_trace_ray_batch_device"] == _lib.SIGNATURES["rt_trace_ray_device"]
    assert _params(header, "rt_get_device_shaded_batches") == ["rt_renderer *r", "int64_t calls[2]", "int64_t rays[2]"]
    assert (inspect.signature(Renderer.trace_ray_batch_device).parameters.keys() ==
            inspect.signature(Renderer.trace_ray_device).parameters.keys())
    assert str(inspect.signature(Renderer.trace_ray_batch_device)) == str(inspect.signature(Renderer.trace_ray_device))


def test_null_handles():
    L = _lib.lib()
    v = C.c_void_p(4096)   # (never read: the handle is checked first)
    calls, rays = np.zeros(2, np.int64), np.zeros(2, np.int64)
    assert L.rt_trace_ray_batch_device(None, v, v, 4, 0, 0, v, v, v, v, v, v, None) == -1   # RT_EINVAL
    assert L.rt_last_error().decode() == "null renderer handle"
    assert L.rt_trace_ray_batch_device(None, None, None, 0, 0, 0, None, None, None, None, None, None, None) == -1
    assert L.rt_get_device_shaded_batches(None, _lib.ptr(calls, _lib._i64p), _lib.ptr(rays, _lib._i64p)) == -1
    assert L.rt_get_device_shaded_batches(None, None, None) == -1
    assert L.rt_last_error().decode() == "null renderer handle"


class _NoHandle(Renderer):
    """The mirror's methods without a library handle (no rt_create, so no GPU): the C calls are recorded."""

    def __init__(self):
        self.device = 0
        self.calls = []

    def _ray_stream(self, stream):
        return None

    @staticmethod
    def _stream_ptr(stream, device):
        return None

    def _call(self, name, *a):
        self.calls.append((name, len(a)))

    def close(self):
        pass


def _out(torch, n=4):
    return dict(rgba=torch.zeros(n, 4), hit_src=torch.zeros(n, dtype=torch.int32), t=torch.zeros(n),
                intersection_found=torch.zeros(n, dtype=torch.uint8), shadowed=torch.zeros(n, dtype=torch.uint8))


def _refusals(torch):
    """(what, exception, the message's pattern, orig, dirs, out): what trace_ray_device refuses by name."""
    o, d = torch.zeros(4, 3), torch.zeros(4, 3)
    cases = [("a numpy array for orig", TypeError, "orig: a torch tensor", o.numpy(), d, None),
             ("a numpy array for dirs", TypeError, "dirs: a torch tensor", o, d.numpy(), None),
             ("a wrong dtype for orig", TypeError, "orig: dtype", o.double(), d, None),
             ("a transposed orig", ValueError, "orig: ", torch.zeros(3, 4).t(), d, None),
             ("a strided dirs", ValueError, "dirs: ", o, torch.zeros(8, 3)[::2], None)]
    for k in KEYS:
        out = _out(torch)
        out[k] = out[k].numpy()
        cases.append((f"a numpy array for {k}", TypeError, f"{k}: a torch tensor", o, d, out))
    for k, bad in (("rgba", torch.float64), ("hit_src", torch.int64), ("t", torch.float16),
                   ("intersection_found", torch.bool), ("shadowed", torch.int32)):
        out = _out(torch)
        out[k] = out[k].to(bad)
        cases.append((f"a wrong dtype for {k}", TypeError, f"{k}: dtype", o, d, out))
    cases.append(("[n, 3] for rgba", ValueError, r"rgba: shape .* \[>= 4, 4\] is needed", o, d,
                  dict(_out(torch), rgba=torch.zeros(4, 3))))
    cases.append(("a transposed rgba", ValueError, "rgba: the tensor is not contiguous", o, d,
                  dict(_out(torch), rgba=torch.zeros(4, 4).t())))
    cases.append(("a strided rgba", ValueError, "rgba: the tensor is not contiguous", o, d,
                  dict(_out(torch), rgba=torch.zeros(8, 4)[::2])))
    cases.append(("columns of a wider rgba", ValueError, "rgba: the tensor is not contiguous", o, d,
                  dict(_out(torch), rgba=torch.zeros(4, 8)[:, :4])))
    cases.append(("a strided hit_src", ValueError, "hit_src: the tensor is not contiguous", o, d,
                  dict(_out(torch), hit_src=torch.zeros(8, dtype=torch.int32)[::2])))
    cases.append(("fewer than n rows of rgba", ValueError, "rgba: shape", o, d, dict(_out(torch), rgba=torch.zeros(3, 4))))
    cases.append(("fewer than n elements of shadowed", ValueError, "shadowed: shape", o, d,
                  dict(_out(torch), shadowed=torch.zeros(3, dtype=torch.uint8))))
    cases.append(("an out without rgba", ValueError, "out: rgba is needed", o, d, dict(t=torch.zeros(4))))
    cases.append(("an empty out", ValueError, "out: rgba is needed", o, d, {}))
    cases.append(("an out that is no dict", TypeError, "out: a dict", o, d, np.zeros((4, 4), np.float32)))
    cases.append(("an unknown key", ValueError, "out: unknown key 'tri_id'", o, d,
                  dict(_out(torch), tri_id=torch.zeros(4, dtype=torch.int32))))
    return cases


def test_wrapper_refuses_by_name_what_trace_ray_device_refuses(monkeypatch):
    torch = pytest.importorskip("torch")
    r = _NoHandle()
    o, d = torch.zeros(4, 3), torch.zeros(4, 3)
    # where a tensor lies is checked last; CPU tensors stop both wrappers there, before any call
    for out in (None, _out(torch)):
        for call in (r.trace_ray_device, r.trace_ray_batch_device):
            with pytest.raises(ValueError, match="orig: the tensor is on cpu, not on a GPU"):
                call(o, d, out=out)
    assert r.calls == []
    # with that one check out of the way (a run without a GPU has none to put them on), everything else about the tensors
    # is refused by the same name and in the same words as by trace_ray_device, and no call is made
    monkeypatch.setattr(_lib, "_device_place", lambda t, name, device: None)
    for what, exc, pattern, o_, d_, out in _refusals(torch):
        messages = []
        for call in (r.trace_ray_device, r.trace_ray_batch_device):
            with pytest.raises(exc, match=pattern) as err:
                call(o_, d_, out=out)
            messages.append(str(err.value))
        assert messages[0] == messages[1], what
    with pytest.raises(ValueError, match="counts: shape"):
        r.trace_ray_batch_device(o, d, out=_out(torch), counts=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError, match="counts: dtype"):
        r.trace_ray_batch_device(o, d, out=_out(torch), counts=torch.zeros(2, dtype=torch.int32))
    assert r.calls == []
    # good tensors reach the C call, the new entry point with rt_trace_ray_device's twelve arguments after the handle
    out = _out(torch)
    assert r.trace_ray_batch_device(o, d, 1, 5, out=out, counts=torch.zeros(2, dtype=torch.int64)) is out
    assert r.calls == [("rt_trace_ray_batch_device", 12)]
    assert len(_lib.SIGNATURES["rt_trace_ray_batch_device"][1]) == 13
