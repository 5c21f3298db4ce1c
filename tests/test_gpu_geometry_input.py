"""Geometry input on the device (geom_gpu.hip gather_points_kernel; rt_gather_triangles_device,
rt_set_triangles_device, rt_update_vertices_device, rt_get_device_ingests) and deferred refinement
(rt_set_accel_deferred, rt_get_accel_builds): the kernel against numpy's gather bit for bit, then renderers
given torch tensors against renderers given the same bytes from the host -- frames, positions, edits, the
host readers of the positions, rejections, stream order -- and frames of a renderer that defers its
background build against one that does not."""
import ctypes as C

import numpy as np
import pytest
import torch

from raytracercpp_amd import _lib, scenes
from raytracercpp_amd.scene import TEX_DIFFUSE
from test_gpu_octree_build import (assert_same_frame, bits, edge_soup, frame, make_renderer,  # noqa: F401
                                   robot_small)

pytestmark = pytest.mark.gpu


# ---- 1. the kernel alone -----------------------------------------------------------------------------

BLOCK, GRID = 256, 2048   # geom_gpu.hip: one lane per point; at most GRID blocks, then a grid stride
# triangles: 3 n = 63 / 66 / 255 / 258 points around a wave and a block, and one point past the grid
COUNTS = (0, 1, 21, 22, 85, 86, (GRID * BLOCK) // 3 + 1)
assert 3 * COUNTS[-1] > GRID * BLOCK >= 3 * (COUNTS[-1] - 1)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31

_cache = {}


def soup_verts(nv):
    """nv vertices of the edge soup's values (signed zeros, quarter-rounded values) with denormals among them."""
    if "base" not in _cache:
        p = edge_soup(COUNTS[-1] + 1).reshape(-1, 3)
        flat = p.reshape(-1)
        tiny = np.arange(flat.size) % 11 == 3
        flat[tiny] = (flat[tiny] * np.float32(1e-40)).astype(np.float32)   # denormals of both signs
        assert np.any((flat != 0) & (np.abs(flat) < np.finfo(np.float32).tiny))
        assert np.any(np.signbit(flat) & (flat == 0))
        p.setflags(write=False)
        _cache["base"] = p
    return _cache["base"][:nv].copy()


def indices(pattern, n, nv):
    if pattern == "identity":
        return np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    if pattern == "reversed":
        return np.arange(3 * n, dtype=np.int32)[::-1].reshape(n, 3).copy()
    if pattern == "same":
        return np.full((n, 3), nv // 2, np.int32)
    if pattern == "random":   # (with repeats: nv is smaller than 3 n)
        return np.random.default_rng(n + 17).integers(0, nv, (n, 3)).astype(np.int32)
    raise KeyError(pattern)


def reference(verts, idx):
    """numpy's gather: verts[idx].reshape(n, 9) (fancy indexing copies the words)."""
    if idx is None:
        return verts.reshape(-1, 9)
    return verts.reshape(-1, 3)[idx.reshape(-1)].reshape(-1, 9)


def run(verts, idx):
    got, flags, ms = _lib.gather_triangles_device(verts, idx)
    ref = reference(verts, idx)
    assert got.shape == ref.shape
    assert np.array_equal(bits(got), bits(ref))
    return got, flags, ms


@pytest.mark.parametrize("pattern", ["flat", "identity", "reversed", "same", "random", "nv1"])
@pytest.mark.parametrize("n", COUNTS)
def test_kernel_equals_numpy_gather(n, pattern):
    if pattern == "flat":
        verts, idx = soup_verts(3 * n).reshape(n, 9), None
    elif pattern == "nv1":
        verts, idx = soup_verts(1), np.zeros((n, 3), np.int32)
    else:
        nv = 3 * n if pattern in ("identity", "reversed") else max(1, n // 2 + 1)
        verts = soup_verts(max(nv, 1))
        idx = indices(pattern, n, verts.shape[0])
    got, flags, ms = run(verts, idx)
    assert flags == 0, f"{pattern}, n = {n}"
    if n == COUNTS[-1]:
        print(f"{pattern}, n = {n}: kernel {ms[0]:.3f} ms (HIP events), whole call {ms[1]:.2f} ms")


def special_words():
    """+-inf, and NaNs with distinct payloads and signs (quiet and signalling)"""
    return np.array([0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fc12345, 0xffabcdef,
                     0x7fffffff], np.uint32)


@pytest.mark.parametrize("n", [1, 22, 86, COUNTS[-1]])
@pytest.mark.parametrize("indexed", [False, True], ids=["flat", "indexed"])
def test_kernel_moves_non_finite_words_bit_for_bit(n, indexed):
    sp = special_words()
    nv = 3 * n
    verts = soup_verts(nv)
    w = bits(verts).reshape(-1)
    where = (np.arange(sp.size) * 7919) % w.size   # spread over the array, the first word included
    w[where] = sp[:where.size]
    idx = indices("reversed", n, nv) if indexed else None
    got, flags, _ = run(verts.reshape(n, 9) if idx is None else verts, idx)
    assert flags == 1
    assert np.isin(sp[:1], bits(got)).all()


@pytest.mark.parametrize("word", [0x7f800000, 0xffc00001], ids=["inf", "nan"])
@pytest.mark.parametrize("n", [22, COUNTS[-1]])
def test_flag_bit0_only_for_referenced_vertices(n, word):
    nv = 3 * n + 1
    for pos in (0, 3 * n - 1):   # the first and the last output point
        verts = soup_verts(nv)
        idx = indices("identity", n, nv)
        bits(verts)[idx.reshape(-1)[pos], 1] = word
        _, flags, _ = run(verts, idx)
        assert flags == 1, pos
        flat = reference(verts, idx).copy()
        _, flags, _ = run(flat, None)
        assert flags == 1, pos
    # the one vertex no index refers to
    verts = soup_verts(nv)
    bits(verts)[nv - 1, :] = word
    _, flags, _ = run(verts, indices("identity", n, nv))
    assert flags == 0


@pytest.mark.parametrize("bad", [-1, "nv", INT32_MAX, INT32_MIN], ids=["-1", "nv", "INT32_MAX", "INT32_MIN"])
@pytest.mark.parametrize("n", [1, 22, COUNTS[-1]])
def test_flag_bit1_and_zeros_for_an_index_out_of_range(n, bad):
    nv = n + 2
    verts = soup_verts(nv)
    for pos in (0, 3 * n - 1):
        idx = indices("random", n, nv)
        idx.reshape(-1)[pos] = nv if bad == "nv" else bad
        got, flags, _ = _lib.gather_triangles_device(verts, idx)
        assert flags == 2, (pos, flags)
        ok = idx.copy()
        ok.reshape(-1)[pos] = 0
        ref = reference(verts, ok).copy().reshape(-1, 3)
        ref[pos] = 0.0
        assert np.array_equal(bits(got.reshape(-1, 3)[pos]), np.zeros(3, np.uint32))   # +0, not the vertex, not -0
        assert np.array_equal(bits(got), bits(ref.reshape(-1, 9)))
    # both bits: a bad index and, elsewhere, a referenced infinity
    if n > 1:
        idx = indices("random", n, nv)
        idx.reshape(-1)[0] = -1
        v = verts.copy()
        v[idx.reshape(-1)[-1], 2] = np.inf
        assert _lib.gather_triangles_device(v, idx)[1] == 3


# ---- renderers ---------------------------------------------------------------------------------------

def gpu(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def textured_small():
    """A small textured scene: texture coordinates on every triangle and a diffuse map."""
    sc, st = scenes.uv_sphere_scene(24, 12, 1.2, 0.05, 64, 36, texcoords=True, enable_diffuse_mapping=True)
    tex = np.random.default_rng(4).uniform(0, 1, (16, 16, 4)).astype(np.float32)
    tex[..., 3] = 1.0
    sc.textures = {TEX_DIFFUSE: tex}
    assert sc.tri_uv is not None
    return sc, st


def indexed_form(tri9):
    """(verts [nv, 3], idx [n, 3]) with every distinct vertex once (distinct as words: -0 is not +0)."""
    w = bits(np.ascontiguousarray(tri9, np.float32).reshape(-1, 3))
    uw, inv = np.unique(w, axis=0, return_inverse=True)
    verts = np.ascontiguousarray(uw).view(np.float32)
    idx = np.ascontiguousarray(inv.reshape(-1, 3).astype(np.int32))
    assert verts.shape[0] < w.shape[0]
    assert np.array_equal(bits(verts[idx.reshape(-1)].reshape(-1, 9)), bits(tri9))
    return verts, idx


def deform(base, k):
    """Step k of a deformation made on the device: every coordinate moves, finite for the small scenes."""
    return (base + 0.03 * torch.sin(7.0 * base.roll(1, 1) + float(k))).contiguous()


def pair(make_renderer, sc, st, build, **dev_env):
    host = make_renderer()
    dev = make_renderer(**dev_env)
    for r in (host, dev):
        r.set_device_build(build)
        r.load_scene(sc, st)
    return host, dev


def give(host, dev, sc, t, form="flat", update=False):
    """The same bytes to both: from the host array downloaded from t, and from the device."""
    tri = t.cpu().numpy()
    host.set_triangles(tri, sc.tri_mat, sc.tri_uv)
    if form == "flat":
        v, i = t, None
    else:
        hv, hi = indexed_form(tri)
        v, i = gpu(hv), gpu(hi)
    if update:
        dev.update_vertices_device(v, indices=i)
    else:
        dev.set_triangles_device(v, sc.tri_mat, sc.tri_uv, indices=i)
    return tri


def same(host, dev, what):
    assert_same_frame(frame(host), frame(dev), what)
    th, td = host.get_triangles(), dev.get_triangles()
    assert np.array_equal(bits(th), bits(td)), what
    return td


@pytest.mark.parametrize("build", [True, False], ids=["device_build", "host_build"])
@pytest.mark.parametrize("form", ["flat", "indexed"])
def test_renderer_equality(make_renderer, form, build):
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st, build)
    base = gpu(sc.tri)
    tri = give(host, dev, sc, deform(base, 0), form)
    assert dev.device_ingests() == 1 and host.device_ingests() == 0
    assert np.array_equal(bits(same(host, dev, "first input")), bits(tri))
    tri = give(host, dev, sc, deform(base, 1), form)
    assert np.array_equal(bits(same(host, dev, "second input")), bits(tri))
    assert dev.device_ingests() == 2
    if build:
        assert dev.stats()["host_builds"] == 0 and dev.device_builds() == 2
    else:
        assert dev.stats()["host_builds"] == 2 and dev.device_builds() == 0
    # another triangle count, then none
    m = sc.tri.shape[0] // 3
    half = deform(base, 2)[:m].contiguous()
    host.set_triangles(half.cpu().numpy(), sc.tri_mat[:m], None)
    dev.set_triangles_device(half, sc.tri_mat[:m])
    assert same(host, dev, "fewer triangles, no texture coordinates").shape == (m, 9)
    host.set_triangles(np.zeros((0, 9), np.float32), np.zeros(0, np.int32))
    dev.set_triangles_device(torch.zeros((0, 9), device="cuda"), np.zeros(0, np.int32))
    assert same(host, dev, "no triangles").shape == (0, 9)
    assert dev.device_ingests() == 3   # (n == 0: no launch)


@pytest.mark.parametrize("scene", [robot_small, textured_small], ids=["robot", "textured"])
def test_animation(make_renderer, scene):
    sc, st = scene()
    host, dev = pair(make_renderer, sc, st, True)
    base = gpu(sc.tri)
    same(host, dev, "before")
    for k in range(4):
        give(host, dev, sc, deform(base, k), "indexed" if k == 2 else "flat", update=True)
        same(host, dev, f"step {k}")
    assert dev.device_ingests() == 4 and dev.stats()["host_builds"] == 0 and dev.device_builds() == 5


EDITS = [_lib.make_transform("ry", 25), _lib.make_transform("scale", 1.5, 0.75, 1.25),
         _lib.make_transform("rz", 10), _lib.make_transform("translation", 0.1, -0.2, 0.05)]


def both(host, dev, f):
    f(host)
    f(dev)


@pytest.mark.parametrize("build", [True, False], ids=["device_build", "host_build"])
def test_with_edits(make_renderer, build):
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st, build)
    base = gpu(sc.tri)
    give(host, dev, sc, deform(base, 0))
    same(host, dev, "input")
    for k in (0, 1):
        both(host, dev, lambda r: r.set_object_transform(EDITS[k]))
        same(host, dev, f"edit {k} after a device input")
    # new positions keep the previous transform: the next matrix is EDITS[2] x EDITS[1]^-1 on both
    give(host, dev, sc, deform(base, 1), update=True)
    same(host, dev, "update after the edits")
    both(host, dev, lambda r: r.set_object_transform(EDITS[2]))
    same(host, dev, "edit after the update")
    # an edit queued, then replaced before any frame: dropped, as on the host
    both(host, dev, lambda r: r.set_object_transform(EDITS[3]))
    tri = give(host, dev, sc, deform(base, 2), update=True)
    assert np.array_equal(bits(same(host, dev, "edit replaced by an update")), bits(tri))
    both(host, dev, lambda r: r.set_object_transform(EDITS[0]))
    same(host, dev, "edit after the replaced one")
    assert dev.device_transforms() == (4 if build else 0) and dev.device_ingests() == 3


def given_pair(make_renderer, **dev_env):
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st, True, **dev_env)
    give(host, dev, sc, deform(gpu(sc.tri), 0), "indexed")
    return sc, st, host, dev


def test_brute_force_after_device_input(make_renderer):
    sc, st, host, dev = given_pair(make_renderer)
    both(host, dev, lambda r: r.set_render_settings(st.copy(enable_bvh=False)))
    same(host, dev, "brute force")


def test_raster_frame_after_device_input(make_renderer):
    sc, st, host, dev = given_pair(make_renderer)
    both(host, dev, lambda r: r.set_render_settings(st.copy(hybrid_rasterization_tracing=True)))

    def raster(r):
        r.request_aux(rgba=True, hit=True, shadow=True)
        r.raster_trace()
        return r.get_internal(argb=True, rgba=True, hit=True, shadow=True)
    assert_same_frame(raster(host), raster(dev), "raster frame on the given positions")
    give(host, dev, sc, deform(gpu(sc.tri), 1), update=True)
    assert_same_frame(raster(host), raster(dev), "raster frame after an update")
    assert dev.stats()["host_builds"] == 0


def test_set_devices_after_device_input(make_renderer):
    from raytracercpp_amd.renderer import render
    sc, st, one, multi = given_pair(make_renderer)
    multi.set_devices([0, 0])
    both(one, multi, render)
    assert np.array_equal(multi.get_image().ravel(), one.get_image().ravel())
    give(one, multi, sc, deform(gpu(sc.tri), 1), update=True)
    both(one, multi, render)
    assert np.array_equal(multi.get_image().ravel(), one.get_image().ravel())
    assert np.array_equal(bits(one.get_triangles()), bits(multi.get_triangles()))


def test_host_path_transform_after_device_input(make_renderer):
    sc, st, host, dev = given_pair(make_renderer, RT_GPU_XFORM=0)
    both(host, dev, lambda r: r.set_object_transform(EDITS[0]))
    same(host, dev, "RT_GPU_XFORM=0: the edit on the host")
    assert dev.device_transforms() == 0


# ---- rejections --------------------------------------------------------------------------------------

def poisoned(r, message):
    for _ in range(2):   # the geometry stays refused
        with pytest.raises(_lib.RtError, match=message) as ei:
            frame(r)
        assert ei.value.code == -1   # RT_EINVAL


@pytest.mark.parametrize("build", [True, False], ids=["device_build", "host_build"])
def test_non_finite_and_bad_index_are_refused_at_the_frame(make_renderer, build):
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st, build)
    base = gpu(sc.tri)
    same(host, dev, "before")
    t = deform(base, 0)
    t[t.shape[0] // 2, 4] = float("inf")
    dev.update_vertices_device(t)
    poisoned(dev, "non-finite vertex coordinate")
    give(host, dev, sc, deform(base, 1), update=True)
    same(host, dev, "a clean update after the infinity")
    hv, hi = indexed_form(deform(base, 2).cpu().numpy())
    hi[-1, 2] = hv.shape[0]
    dev.update_vertices_device(gpu(hv), indices=gpu(hi))
    poisoned(dev, "vertex index out of range")
    if not build:   # (the host-path edit reads the positions: the state survives it)
        dev.set_object_transform(EDITS[0])
        poisoned(dev, "vertex index out of range")
        dev.set_object_transform(_lib.make_transform("identity"))
    give(host, dev, sc, deform(base, 3), update=True)
    same(host, dev, "a clean update after the bad index")
    # both at once: the first message
    hi[0, 0] = -1
    hv[hi[5, 1], 0] = np.nan
    dev.set_triangles_device(gpu(hv), sc.tri_mat, sc.tri_uv, indices=gpu(hi))
    poisoned(dev, "non-finite vertex coordinate")
    give(host, dev, sc, deform(base, 1))
    same(host, dev, "a clean input after both")


def test_pointers_that_are_not_this_devices_memory(make_renderer):
    sc, st = robot_small()
    r = make_renderer()
    r.set_device_build(True)
    r.load_scene(sc, st)
    before, tri = frame(r), r.get_triangles()
    L = _lib.lib()
    n = sc.tri.shape[0]
    host_v = np.ascontiguousarray(sc.tri + 1.0)
    host_i = np.arange(3 * n, dtype=np.int32)
    good = gpu(sc.tri + 2.0)
    mat = np.ascontiguousarray(sc.tri_mat, np.int32)
    vp, ip = C.c_void_p(host_v.ctypes.data), C.c_void_p(host_i.ctypes.data)
    gp = C.c_void_p(good.data_ptr())
    assert L.rt_update_vertices_device(r._h, vp, 3 * n, None, None) == -1   # RT_EINVAL
    assert "geometry input" in L.rt_last_error().decode()
    assert L.rt_update_vertices_device(r._h, gp, 3 * n, ip, None) == -1     # (the indices on the host)
    assert L.rt_set_triangles_device(r._h, vp, 3 * n, None, _lib.ptr(mat, _lib._i32p), None, n, None) == -1
    assert L.rt_set_triangles_device(r._h, None, 3 * n, None, _lib.ptr(mat, _lib._i32p), None, n, None) == -1
    assert L.rt_set_triangles_device(r._h, gp, 3 * n, None, None, None, n, None) == -1
    assert L.rt_set_triangles_device(r._h, gp, 3 * n - 3, None, _lib.ptr(mat, _lib._i32p), None, n, None) == -1
    assert L.rt_update_vertices_device(r._h, None, 3 * n, None, None) == -1
    if torch.cuda.device_count() > 1:   # memory of another device
        other = torch.zeros((n, 9), device="cuda:1")
        assert L.rt_update_vertices_device(r._h, C.c_void_p(other.data_ptr()), 3 * n, None, None) == -1
        with pytest.raises(ValueError, match="the renderer on GPU 0"):
            r.update_vertices_device(other)
    # the flat form with another count, and the mirror's own checks on GPU tensors
    assert L.rt_update_vertices_device(r._h, gp, 3 * n - 3, None, None) == -4   # RT_ESTATE
    with pytest.raises(_lib.RtError, match="RT_ESTATE"):
        r.update_vertices_device(good[:-1])
    with pytest.raises(ValueError, match="not contiguous"):
        r.update_vertices_device(gpu(np.zeros((9, n), np.float32)).t())
    with pytest.raises(TypeError, match="dtype"):
        r.update_vertices_device(good.double())
    with pytest.raises(ValueError, match="materials"):
        r.set_triangles_device(good, sc.tri_mat[:-1])
    assert r.device_ingests() == 0
    assert_same_frame(frame(r), before, "after the refused calls")
    assert np.array_equal(bits(r.get_triangles()), bits(tri))
    assert r.device_builds() == 1   # (nothing was marked changed)
    # the sticky HIP error of the unknown pointer was cleared: the next call works
    r.update_vertices_device(good)
    assert np.array_equal(bits(r.get_triangles()), bits(good.cpu().numpy()))


def test_update_without_geometry(make_renderer):
    r = make_renderer()
    with pytest.raises(_lib.RtError, match="RT_ESTATE"):
        r.update_vertices_device(torch.zeros((4, 9), device="cuda"))
    with pytest.raises(_lib.RtError, match="RT_ESTATE"):
        r.update_vertices_device(torch.zeros((4, 3), device="cuda"), indices=torch.zeros((0, 3), dtype=torch.int32,
                                                                                         device="cuda"))


# ---- stream order ------------------------------------------------------------------------------------

def test_stream_order(make_renderer):
    """The tensor is made on a side stream behind long-running work and overwritten on it right after the
    call: the renderer holds the values in between.  (This exercises the two waits; a race could still
    pass by luck.)"""
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st, True)
    base = gpu(sc.tri)
    want = (base * 0.75 + 0.125).cpu().numpy()
    a = torch.rand((2048, 2048), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = a
        for _ in range(24):
            b = (b @ a) * (1.0 / 2048)
        t = base * 0.75 + 0.125
        dev.update_vertices_device(t, stream=side)
        t.fill_(float("nan"))
    host.set_triangles(want, sc.tri_mat, sc.tri_uv)
    assert np.array_equal(bits(same(host, dev, "values between the producer and the overwrite")), bits(want))
    # and with the current stream taken by default
    with torch.cuda.stream(side):
        t2 = base * 0.5 - 0.25
        dev.update_vertices_device(t2)
        t2.zero_()
    torch.cuda.current_stream().wait_stream(side)
    host.set_triangles((base * 0.5 - 0.25).cpu().numpy(), sc.tri_mat, sc.tri_uv)
    same(host, dev, "the current stream by default")
    torch.cuda.synchronize()
    del b


# ---- deferred refinement -----------------------------------------------------------------------------

def wide_tree(r):
    return r.stats()["wide_tree"]


@pytest.mark.parametrize("build", [True, False], ids=["device_build", "host_build"])
def test_deferred_refinement(make_renderer, build):
    sc, st = robot_small()
    # (the suite's renderers finish their background build inside the frame that starts it: wide_tree 2)
    ref, d = pair(make_renderer, sc, st, build, RT_ASYNC_ACCEL=1)
    d.set_accel_deferred(True)
    base = gpu(sc.tri)
    same(ref, d, "first frame")
    assert wide_tree(ref) == 2 and wide_tree(d) == 1
    assert ref.accel_builds() == 1 and d.accel_builds() == 0
    for k in range(5):
        give(ref, d, sc, deform(base, k), update=True)
        same(ref, d, f"deferred, step {k}")
        assert wide_tree(ref) == 2 and wide_tree(d) == 1
        assert d.accel_builds() == 0 and ref.accel_builds() == k + 2   # default off: one per change
    last = frame(d)
    d.finish_accel()
    assert d.accel_builds() == 1
    assert_same_frame(frame(d), last, "the refined tree, the same frame")
    assert wide_tree(d) == 2
    d.finish_accel()
    assert d.accel_builds() == 1   # (refined already)
    # still deferred: the next change is back on the quick tree
    give(ref, d, sc, deform(base, 5), update=True)
    same(ref, d, "deferred again")
    assert wide_tree(d) == 1 and d.accel_builds() == 1
    # off: the next frame starts this geometry's build
    d.set_accel_deferred(False)
    same(ref, d, "after the switch went off")
    assert d.accel_builds() == 2
    d.finish_accel()
    assert wide_tree(d) == 2 and d.accel_builds() == 2
    same(ref, d, "refined after the switch went off")
    give(ref, d, sc, deform(base, 6), update=True)
    same(ref, d, "not deferred")
    assert d.accel_builds() == 3


def test_deferred_without_the_quick_tree(make_renderer):
    sc, st = robot_small()
    ref, d = pair(make_renderer, sc, st, True, RT_ACCEL_DEFER=1, RT_WBVH_QUICK_FIRST=0, RT_ASYNC_ACCEL=1)
    base = gpu(sc.tri)
    for k in range(2):
        give(ref, d, sc, deform(base, k), update=True)
        same(ref, d, f"on the octree, step {k}")
        assert wide_tree(d) == 0 and d.accel_builds() == 0
    d.finish_accel()
    assert wide_tree(d) == 2 and d.accel_builds() == 1
    same(ref, d, "refined")
