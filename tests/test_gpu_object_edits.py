"""Object edits on the device (geom_gpu.hip; rt_transform_points_device, rt_get_triangles,
rt_get_device_transforms): the kernel against rt_transform_points bit for bit, then renderers with the
device build on against host-mode renderers given the same calls -- frames, positions, the host readers
of the positions after a device edit, and non-finite results."""
import ctypes as C

import numpy as np
import pytest

from raytracercpp_amd import _lib, scenes
from test_gpu_octree_build import (assert_same_frame, bits, edge_soup, frame, make_renderer,  # noqa: F401
                                   robot_small)

pytestmark = pytest.mark.gpu


def assert_same_points(got, ref, what=""):
    """Bits everywhere (infinities, signed zeros, denormals), except where both are NaN: x86 and the GPU
    give a NaN different signs and payloads."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, what
    both_nan = np.isnan(got) & np.isnan(ref)
    assert np.array_equal(bits(got)[~both_nan], bits(ref)[~both_nan]), what


# ---- 1. the kernel alone -----------------------------------------------------------------------------

WAVE, BLOCK, GRID = 64, 256, 2048   # geom_gpu.hip: one lane per point; at most GRID blocks, then a grid stride
COUNTS = (0, 1, 2, 3, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 1, 3 * 65537,
          GRID * BLOCK + 1)
SCALES = (1.0, 1e-13, 1e13)


def _with_bottom_row(row):
    m = _lib.make_transform("identity")
    m[12:16] = np.asarray(row, np.float32)
    return m


MATRICES = {
    "identity": lambda: _lib.make_transform("identity"),               # wt == 1: no divide
    "ry25": lambda: _lib.make_transform("ry", 25),
    "scale1e-30": lambda: _lib.make_transform("scale", 1e-30, 1e-30, 1e-30),   # denormal results are kept
    "projective": lambda: _with_bottom_row((0.1, 0.2, 0.3, 1.5)),      # the divide path (wt >= 0.9 at scale 1)
    "wt0": lambda: _with_bottom_row((1.0, 0.0, 0.0, 0.0)),             # wt = x: 0 for point 0 and every x = +-0
}

_soup = {}


def soup_points(n, scale):
    """The edge soup's values (signed zeros, quarter-rounded values) as n points; point 0 has x = +0."""
    if "base" not in _soup:
        p = edge_soup((max(COUNTS) + 2) // 3 + 1).reshape(-1, 3)
        p[0] = (0.0, 0.5, -0.25)
        p.setflags(write=False)
        _soup["base"] = p
    return (_soup["base"][:n] * np.float32(scale)).astype(np.float32)


@pytest.mark.parametrize("mat", list(MATRICES))
@pytest.mark.parametrize("n", COUNTS)
def test_kernel_equals_host_transform(n, mat):
    m = MATRICES[mat]()
    for scale in SCALES:
        pts = soup_points(n, scale)
        ref = _lib.transform_points(m, pts)
        got, flag, ms = _lib.transform_points_device(m, pts)
        what = f"{mat}, n = {n}, scale {scale}"
        assert_same_points(got, ref, what)
        if n == max(COUNTS):
            print(f"{what}: kernel {ms[0]:.3f} ms (HIP events), whole call {ms[1]:.2f} ms")
        assert flag == int(not np.isfinite(ref).all()), what
        assert flag == int(mat == "wt0" and n > 0), what


def test_kernel_keeps_denormals():
    """(The case above at scale 1e-13 holds them; this states it.)"""
    m = MATRICES["scale1e-30"]()
    pts = soup_points(1000, 1e-13)
    got, flag, _ = _lib.transform_points_device(m, pts)
    tiny = np.abs(got[got != 0])
    assert tiny.size and tiny.max() < np.finfo(np.float32).tiny and flag == 0


# ---- 2. edits through the renderer -------------------------------------------------------------------

EDITS = [_lib.make_transform("ry", 25), _lib.make_transform("scale", 1.5, 0.75, 1.25),
         _lib.make_transform("translation", 1e3, 0.0, 0.0)]   # (test_renderer_edits')
FOURTH = _lib.make_transform("rz", 10)


def pair(make_renderer, sc, st, **dev_env):
    host = make_renderer()
    dev = make_renderer(**dev_env)
    dev.set_device_build(True)
    for r in (host, dev):
        r.load_scene(sc, st)
    return host, dev


def both(host, dev, f):
    f(host)
    f(dev)


@pytest.mark.parametrize("knob", [None, 0], ids=["device_xform", "RT_GPU_XFORM=0"])
def test_edits_through_the_renderer(make_renderer, knob):
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st, **({} if knob is None else {"RT_GPU_XFORM": knob}))
    on = knob is None
    assert_same_frame(frame(host), frame(dev), "before the edits")
    assert np.array_equal(bits(dev.get_triangles()), bits(sc.tri))
    pos = sc.tri.reshape(-1, 3).copy()
    prev = _lib.make_transform("identity")
    for k, m in enumerate(EDITS + [None, FOURTH]):
        if m is None:
            both(host, dev, lambda r: r.reset_previous_transform())
            prev = _lib.make_transform("identity")
            continue
        both(host, dev, lambda r: r.set_object_transform(m))
        assert_same_frame(frame(host), frame(dev), f"edit {k}")
        th, td = host.get_triangles(), dev.get_triangles()
        assert np.array_equal(bits(th), bits(td)), f"edit {k}"
        pos = _lib.transform_points(_lib.compose(m, _lib.inverse(prev)), pos)
        prev = m
        assert np.array_equal(bits(td), bits(pos.reshape(-1, 9))), f"edit {k}"
    assert dev.device_transforms() == (4 if on else 0) and host.device_transforms() == 0
    assert dev.stats()["host_builds"] == 0 and dev.device_builds() == 5
    # two edits with no frame between them: two matrices queued, applied in order (get_triangles runs them)
    a, b = _lib.make_transform("rx", -40), _lib.make_transform("scale", 0.5, 2.0, 1.0)
    both(host, dev, lambda r: (r.set_object_transform(a), r.set_object_transform(b)))
    th, td = host.get_triangles(), dev.get_triangles()
    assert np.array_equal(bits(th), bits(td))
    assert dev.device_transforms() == (6 if on else 0)
    assert_same_frame(frame(host), frame(dev), "two edits, one frame")
    both(host, dev, lambda r: (r.set_object_transform(b), r.set_object_transform(a)))
    assert_same_frame(frame(host), frame(dev), "two more edits, the frame first")
    assert np.array_equal(bits(host.get_triangles()), bits(dev.get_triangles()))
    assert dev.device_transforms() == (8 if on else 0) and dev.stats()["host_builds"] == 0


def test_get_triangles_arguments(make_renderer):
    sc, st = robot_small()
    r = make_renderer()
    r.load_scene(sc, st)
    L = _lib.lib()
    n = C.c_int64(-1)
    assert L.rt_get_triangles(r._h, None, C.byref(n)) == 0 and n.value == sc.tri.shape[0]   # only n
    assert L.rt_get_triangles(r._h, None, None) == -1   # RT_EINVAL
    assert L.rt_get_device_transforms(r._h, None) == -1
    assert np.array_equal(bits(r.get_triangles()), bits(sc.tri))   # before any frame


# ---- 3. host readers of the positions after a device edit --------------------------------------------

def edited_pair(make_renderer):
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st)
    assert_same_frame(frame(host), frame(dev), "before the edit")
    both(host, dev, lambda r: r.set_object_transform(EDITS[0]))
    return sc, st, host, dev


def test_host_build_after_device_edit_max_depth_31(make_renderer):
    sc, st, host, dev = edited_pair(make_renderer)
    both(host, dev, lambda r: r.set_render_settings(st.copy(bvh_max_depth=31)))
    assert_same_frame(frame(host), frame(dev), "max_depth 31")
    assert dev.device_transforms() == 1 and dev.stats()["host_builds"] == 1


def test_brute_force_after_device_edit(make_renderer):
    sc, st, host, dev = edited_pair(make_renderer)
    both(host, dev, lambda r: r.set_render_settings(st.copy(enable_bvh=False)))
    assert_same_frame(frame(host), frame(dev), "brute force")
    assert dev.device_transforms() == 1


def test_raster_frame_after_device_edit(make_renderer):
    sc, st, host, dev = edited_pair(make_renderer)
    both(host, dev, lambda r: r.set_render_settings(st.copy(hybrid_rasterization_tracing=True)))

    def raster(r):
        r.request_aux(rgba=True, hit=True, shadow=True)
        r.raster_trace()
        return r.get_internal(argb=True, rgba=True, hit=True, shadow=True)
    assert_same_frame(raster(host), raster(dev), "raster frame on the resident positions")
    both(host, dev, lambda r: r.set_object_transform(EDITS[1]))
    assert_same_frame(raster(host), raster(dev), "raster frame after a second edit")
    assert dev.device_transforms() == 2 and dev.stats()["host_builds"] == 0


def test_mode_off_then_another_edit(make_renderer):
    """The first edit is still queued when the mode goes off: the host-path edit applies it, downloads the
    positions and transforms them on the host."""
    sc, st, host, dev = edited_pair(make_renderer)
    dev.set_device_build(False)
    both(host, dev, lambda r: r.set_object_transform(EDITS[1]))
    assert_same_frame(frame(host), frame(dev), "edit after the mode went off")
    assert np.array_equal(bits(host.get_triangles()), bits(dev.get_triangles()))
    assert dev.device_transforms() == 1 and dev.stats()["host_builds"] == 1


def test_set_devices_after_device_edit(make_renderer):
    from raytracercpp_amd.renderer import render
    sc, st = robot_small()
    one, multi = pair(make_renderer, sc, st)
    both(one, multi, render)
    both(one, multi, lambda r: r.set_object_transform(EDITS[0]))
    multi.set_devices([0, 0])
    both(one, multi, render)
    assert np.array_equal(multi.get_image().ravel(), one.get_image().ravel())
    both(one, multi, lambda r: r.set_object_transform(EDITS[1]))
    both(one, multi, render)
    assert np.array_equal(multi.get_image().ravel(), one.get_image().ravel())
    assert np.array_equal(bits(one.get_triangles()), bits(multi.get_triangles()))
    assert multi.device_transforms() == 2 and multi.stats()["host_builds"] == 0


# ---- 4. non-finite geometry --------------------------------------------------------------------------

def test_non_finite_geometry(make_renderer):
    """scale 1e30 twice, the previous transform reset in between (without the reset the second call's
    matrix is scale x scale^-1, the identity): 1e60 overflows to infinities."""
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st)
    assert_same_frame(frame(host), frame(dev), "before")
    big = _lib.make_transform("scale", 1e30, 1e30, 1e30)
    both(host, dev, lambda r: (r.set_object_transform(big), r.reset_previous_transform(), r.set_object_transform(big)))
    for r in (host, dev):
        for _ in range(2):   # the geometry stays poisoned
            with pytest.raises(_lib.RtError, match="non-finite vertex coordinate") as ei:
                frame(r)
            assert ei.value.code == -1   # RT_EINVAL
    th, td = host.get_triangles(), dev.get_triangles()
    assert not np.isfinite(th).all()
    assert_same_points(td, th)
    assert dev.device_transforms() == 2
    both(host, dev, lambda r: r.set_triangles(sc.tri, sc.tri_mat, sc.tri_uv))
    assert_same_frame(frame(host), frame(dev), "after set_triangles")
    both(host, dev, lambda r: r.set_object_transform(EDITS[0]))
    assert_same_frame(frame(host), frame(dev), "an edit of the new geometry")
    assert dev.device_transforms() == 3


# ---- 5. sphere1m -------------------------------------------------------------------------------------

def test_sphere1m_edit(make_renderer):
    sc, st = scenes.sphere1m()
    host, dev = pair(make_renderer, sc, st)
    m = _lib.make_transform("rz", 3.0)
    out = {}
    for name, r in (("host", host), ("device", dev)):
        frame(r)
        r.set_object_transform(m)
        out[name] = (frame(r), r.get_triangles())
    assert_same_frame(out["host"][0], out["device"][0], "sphere1m after rz")
    assert np.array_equal(bits(out["host"][1]), bits(out["device"][1]))
    assert dev.device_transforms() == 1 and dev.stats()["host_builds"] == 0
    _, flag, ms = _lib.transform_points_device(m, sc.tri.reshape(-1, 3))
    print(f"sphere1m, {3 * sc.tri.shape[0]} points: kernel {ms[0]:.3f} ms (HIP events), whole call {ms[1]:.1f} ms")
    assert flag == 0
