"""The visibility buffer on device memory (rt_visibility_device, rt_get_device_visibility; kernels.hip
visibility_kernel).

Per pixel of the internal image the call must write what a frame leaves for rt_get_internal (hit_id, hit_t, bit for
bit) and, where a triangle was hit, the barycentrics rt_trace_rays_device answers for that pixel's camera ray.  The
references are the reference-generated golden frames, ray_trace + get_internal of the same renderer state, and
trace_rays_device on test_trace_ray.camera_rays."""
import ctypes as C

import numpy as np
import pytest
import torch

from golden_cases import Case
from raytracercpp_amd import _lib, scenes
from raytracercpp_amd._lib import RtError
from test_gpu_octree_build import bits, make_renderer  # noqa: F401
from test_trace_ray import TRACE_CASES, camera_rays

pytestmark = pytest.mark.gpu

KEYS = ("tri_id", "t", "uv")
# the golden cases the frames render with their plain pixel (no texture, sky, analytic shape, debug shading or
# reflective material): the tile mask is the frames' there too
PLAIN_CASES = ("c2_cube", "robot", "c3_bumpy70k", "c4_sphere1m", "ssaa3_cube")
NO_TRIANGLES = ("c1_sphere256",)


@pytest.fixture(scope="module")
def R():
    from raytracercpp_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(out):
    """The outputs on the host, flat per pixel (the copy waits for the kernel)."""
    return {"tri_id": out["tri_id"].cpu().numpy().ravel(), "t": out["t"].cpu().numpy().ravel(),
            "uv": out["uv"].cpu().numpy().reshape(-1, 2)}


def vis(r, stream=None, **kw):
    out = r.visibility_device(stream=stream, **kw)
    if stream is not None:
        stream.synchronize()   # (the copy to the host runs on the current stream)
    return host(out)


def internal(r):
    """(hit_id, hit_t) of a frame of r's current state."""
    r.request_aux(hit=True)
    r.ray_trace()
    g = r.get_internal(argb=False, hit=True)
    return g["hit_id"], g["hit_t"]


def same_hits(got, hit_id, hit_t, what):
    assert np.array_equal(got["tri_id"], hit_id), f"{what}: {int((got['tri_id'] != hit_id).sum())} ids differ"
    assert np.array_equal(bits(got["t"]), bits(hit_t)), f"{what}: t differs in its bits"


def same_all(a, b, what):
    same_hits(a, b["tri_id"], b["t"], what)
    assert np.array_equal(bits(a["uv"]), bits(b["uv"])), f"{what}: uv differs in its bits"


def uv_checked(r, got, sc, st, what):
    """uv against trace_rays_device on the camera rays where a triangle is visible, zero elsewhere; the count."""
    o, d = camera_rays(sc, st)
    q = r.trace_rays_device(gpu(o), gpu(d))
    u, v = q["u"].cpu().numpy(), q["v"].cpu().numpy()
    tri = got["tri_id"] >= 0
    assert np.array_equal(bits(got["uv"][tri, 0]), bits(u[tri])), f"{what}: u differs in its bits"
    assert np.array_equal(bits(got["uv"][tri, 1]), bits(v[tri])), f"{what}: v differs in its bits"
    assert np.array_equal(q["tri_id"].cpu().numpy()[tri], got["tri_id"][tri]), what
    assert not bits(got["uv"][~tri]).any(), f"{what}: uv is not (0, 0) where no triangle is visible"
    return int(tri.sum())


# ---- 1, 2. the golden frames, and u / v ------------------------------------------------------------------

@pytest.mark.parametrize("name", TRACE_CASES)
def test_golden_frames_and_barycentrics(R, name):
    c = Case(name)
    R.load_scene(c.scene, c.settings)
    exp = c.expected()
    calls0, pixels0, used0 = R.device_visibility()
    got = vis(R)
    rw, rh = c.settings.render_size()
    assert got["tri_id"].shape == (rw * rh,) and got["uv"].shape == (rw * rh, 2)
    same_hits(got, exp["hit_id"], exp["hit_t"], name)
    calls, pixels, used = R.device_visibility()
    assert sum(calls) == sum(calls0) + 1 and sum(pixels) == sum(pixels0) + rw * rh
    if name in PLAIN_CASES:
        assert calls[0] == calls0[0] + 1 and used[0] == used0[0] + 1, f"{name}: no tile mask: {calls}, {used}"
    if len(c.scene.shape_kind) or not c.settings.enable_bvh:
        assert calls[1] == calls0[1] + 1, f"{name}: shapes or the brute-force loop take the generic instance"
    n = uv_checked(R, got, c.scene, c.settings, name)
    print(f"{name}: {rw}x{rh}, {n} pixels show a triangle, {int((got['tri_id'] < -1).sum())} a shape; instance calls "
          f"{calls}, mask / entry sets {used}")
    if name in NO_TRIANGLES:
        assert n == 0 and (got["tri_id"] < -1).any()
    else:
        assert n >= 200
    # the same bytes from the second launch (entry sets where the fast instance runs) and after the SAH tree
    if name != "c4_sphere1m":
        R.finish_accel()
    again = vis(R)
    same_all(again, got, f"{name}: second launch")


# ---- 3. both trees, the mask, the entry sets ---------------------------------------------------------------

@pytest.mark.parametrize("tree", ["sah", "quick"])
def test_trees_mask_and_entry_sets(make_renderer, tree):
    c = Case("c3_bumpy70k")
    sc, st = c.scene, c.settings
    env = {"RT_ACCEL_HOLD": 1} if tree == "quick" else {}
    rs = {k: make_renderer(**dict(env, **e)) for k, e in
          (("on", {}), ("mask_off", {"RT_TILE_MASK": 0}), ("starts_off", {"RT_TILE_START": 0}))}
    for r in rs.values():
        r.load_scene(sc, st)
        r.ray_trace()
        if tree == "sah":
            r.finish_accel()
        assert r.stats()["wide_tree"] == (2 if tree == "sah" else 1)
    r = rs["on"]
    side = torch.cuda.Stream()
    moves = [None, ("translation", 0.4, -0.2, 0.8), ("ry", 9)]
    for mi, move in enumerate(moves):
        for q in rs.values():
            if move:
                q.set_camera_transform(_lib.make_transform(*move))
        hit_id, hit_t = internal(r)
        ref = None
        for stream in ((None,) if mi == 0 else (side, None)):
            used0 = r.device_visibility()[2]
            for k in range(3):
                got = vis(r, stream=stream)
                what = f"{tree} tree, camera {mi}, launch {k}"
                same_hits(got, hit_id, hit_t, what)
                if ref is None:
                    ref = got
                    assert uv_checked(r, got, _with_camera(sc, r), st, what) >= 200
                same_all(got, ref, what)
            used = r.device_visibility()[2]
            assert used[0] == used0[0] + 3, f"camera {mi}: a mask at every launch ({used0} -> {used})"
            assert used[1] >= used0[1] + 1, f"camera {mi}: the third launch in a row had no entry sets ({used0} -> {used})"
        for k in ("mask_off", "starts_off"):
            u0 = rs[k].device_visibility()[2]
            for _ in range(3):
                same_all(vis(rs[k]), ref, f"{tree} tree, camera {mi}: {k}")
            u1 = rs[k].device_visibility()[2]
            assert (u1[0] == u0[0], u1[1] == u0[1]) == ((True, True) if k == "mask_off" else (False, True)), (k, u0, u1)
    calls, pixels, used = r.device_visibility()
    assert calls[1] == 0 and calls[0] == 3 + 2 * 6 and pixels[0] == calls[0] * len(hit_id)


def _with_camera(sc, r):
    import dataclasses
    pos, pinv, c2w = r.get_camera_matrices()
    return dataclasses.replace(sc, cam_pos=pos, proj_inv=pinv, cam_to_world=c2w)


# ---- 4. modes --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["exact", "RT_WBVH=0", "no_wide_tree", "enable_bvh_0"])
@pytest.mark.parametrize("name", ["robot", "mirror"])
def test_modes_take_the_generic_instance(make_renderer, name, mode):
    c = Case(name)
    sc, st = c.scene, c.settings
    if mode == "enable_bvh_0":
        st = st.copy(enable_bvh=False)
    r = make_renderer(**({"RT_WBVH": 0} if mode == "RT_WBVH=0" else
                         {"RT_WBVH_QUICK_FIRST": 0, "RT_ACCEL_HOLD": 1} if mode == "no_wide_tree" else {}))
    if mode == "exact":
        r.set_exact(True)
    r.load_scene(sc, st)
    got = vis(r)
    calls, pixels, used = r.device_visibility()
    assert calls == (0, 1) and used == (0, 0), f"{name}, {mode}: {calls}, {used}"
    hit_id, hit_t = internal(r)
    same_hits(got, hit_id, hit_t, f"{name}, {mode}")
    assert uv_checked(r, got, sc, st, f"{name}, {mode}") >= 200
    exp = c.expected()
    same_hits(got, exp["hit_id"], exp["hit_t"], f"{name}, {mode}: the golden frame")
    # the default renderer's bytes (the fast instance where the scene has no shapes)
    d = make_renderer()
    d.load_scene(c.scene, c.settings)
    same_all(vis(d), got, f"{name}: default against {mode}")
    assert d.device_visibility()[0] == ((1, 0) if name == "robot" else (0, 1))


# ---- 5. sizes --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (7, 5), (8, 8), (9, 9), (65, 9), (64, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_guards_and_outputs_left_out(R, size):
    w, h = size
    c = Case("c2_cube")
    st = c.settings.copy(image_width=w, image_height=h, enable_ssaa=False)
    R.load_scene(c.scene, st)
    hit_id, hit_t = internal(R)
    assert len(hit_id) == w * h
    pad = 8   # (floats: uv stays 8-byte aligned)
    shapes = {"tri_id": (h, w), "t": (h, w), "uv": (h, w, 2)}
    dts = {"tri_id": torch.int32, "t": torch.float32, "uv": torch.float32}

    def guarded():
        flat = {k: torch.full((int(np.prod(shapes[k])) + 2 * pad,), 77, dtype=dts[k], device="cuda") for k in KEYS}
        return flat, {k: flat[k][pad:flat[k].numel() - pad].view(shapes[k]) for k in KEYS}

    flat, out = guarded()
    assert R.visibility_device(out=out) is out
    full = host(out)
    same_hits(full, hit_id, hit_t, f"{w}x{h}")
    uv_checked(R, full, c.scene, st, f"{w}x{h}")
    for k in KEYS:
        assert bool((flat[k][:pad] == 77).all()) and bool((flat[k][-pad:] == 77).all()), f"{w}x{h}: {k}'s guards"
    for left_out in KEYS:
        flat, out = guarded()
        sub = {k: v for k, v in out.items() if k != left_out}
        ret = R.visibility_device(out=sub)
        assert set(ret) == set(sub)
        torch.cuda.synchronize()
        assert bool((flat[left_out] == 77).all()), f"{w}x{h}: {left_out} was left out and written"
        for k in sub:
            a = sub[k].cpu().numpy().reshape(full[k].shape)
            assert np.array_equal(bits(a), bits(full[k])), (k, left_out)
            assert bool((flat[k][:pad] == 77).all()) and bool((flat[k][-pad:] == 77).all())


# ---- 6. animated geometry ----------------------------------------------------------------------------------

def test_animated_geometry_on_the_quick_tree(make_renderer):
    sc, st = scenes.bumpy70k(width=96, height=54)
    r = make_renderer()
    r.set_device_build(True)
    r.set_accel_deferred(True)
    r.load_scene(sc, st)
    verts = gpu(sc.tri.reshape(-1, 9))
    r.set_triangles_device(verts, sc.tri_mat, sc.tri_uv)
    builds0 = r.accel_builds()
    for step in (1, 2):
        moved = (verts * (1.0 + 0.03 * step)).contiguous()
        r.update_vertices_device(moved)
        got = vis(r)
        got2 = vis(r)
        same_all(got2, got, f"step {step}: second launch")
        h = make_renderer()
        h.load_scene(sc, st)
        h.set_triangles(moved.cpu().numpy(), sc.tri_mat, sc.tri_uv)
        hit_id, hit_t = internal(h)
        same_hits(got, hit_id, hit_t, f"step {step}: against the host-input renderer's frame")
        same_all(vis(h), got, f"step {step}: against the host-input renderer")
        assert (got["tri_id"] >= 0).sum() >= 200
    assert r.accel_builds() == builds0 and r.stats()["wide_tree"] == 1
    assert r.device_visibility()[0] == (4, 0)


# ---- 7. stream order -----------------------------------------------------------------------------------------

def test_stream_order(R):
    """The outputs are filled with a sentinel on a side stream behind long-running work, the call follows on that
    stream and a consumer on it reads them; the host is back while the stream's earlier work still runs.  (This
    exercises the order; a race could still pass by luck.)"""
    c = Case("robot")
    R.load_scene(c.scene, c.settings)
    rw, rh = c.settings.render_size()
    ref = vis(R)   # (the scene is resident: the call below has nothing to build)
    a = torch.rand((4096, 4096), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    busy = torch.cuda.Event()
    with torch.cuda.stream(side):
        b = a
        for _ in range(60):
            b = (b @ a) * (1.0 / 4096)
        busy.record(side)
        out = {"tri_id": torch.empty((rh, rw), dtype=torch.int32, device="cuda"),
               "t": torch.empty((rh, rw), dtype=torch.float32, device="cuda"),
               "uv": torch.empty((rh, rw, 2), dtype=torch.float32, device="cuda")}
        for v in out.values():
            v.fill_(77)
        R.visibility_device(out=out, stream=side)
        back_early = not busy.query()
        seen = {k: v.clone() for k, v in out.items()}
        for v in out.values():
            v.fill_(55)
    side.synchronize()
    same_all(host(seen), ref, "the consumer on the side stream")
    assert back_early, "the call returned only after the stream's earlier work had ended"
    with torch.cuda.stream(side):   # the current stream by default
        seen2 = {k: v.clone() for k, v in R.visibility_device().items()}
    side.synchronize()
    same_all(host(seen2), ref, "the current stream by default")
    torch.cuda.synchronize()
    del b


# ---- 8. fences -------------------------------------------------------------------------------------------

def test_scene_changes_and_close_wait_for_the_launch(make_renderer):
    scb, stb = scenes.bumpy70k(width=320, height=180)
    scr, str_ = scenes.robot1080(width=320, height=180)
    r = make_renderer()
    r.load_scene(scb, stb)
    before = vis(r)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = r.visibility_device(stream=side)
    r.load_scene(scr, str_)          # the geometry and the materials are replaced, no wait in between
    hit_id, hit_t = internal(r)
    side.synchronize()
    same_all(host(out), before, "the launch in flight while the geometry was replaced")
    robot = vis(r)
    same_hits(robot, hit_id, hit_t, "the robot after the change")
    out = r.visibility_device(stream=side)
    r.set_materials(scr.materials)
    side.synchronize()
    same_all(host(out), robot, "the launch in flight while the materials were replaced")
    from raytracercpp_amd.renderer import Renderer
    r3 = Renderer(0)
    r3.load_scene(scb, stb)
    out3 = r3.visibility_device(stream=side)
    r3.close()
    side.synchronize()
    torch.cuda.synchronize()
    same_all(host(out3), before, "the launch in flight at close()")


# ---- 9. frames undisturbed ---------------------------------------------------------------------------------

def test_frames_are_undisturbed(make_renderer):
    c = Case("c3_bumpy70k")
    sc, st = c.scene, c.settings
    rw, rh = st.render_size()
    seen = []
    for with_visibility in (False, True):
        r = make_renderer()
        r.load_scene(sc, st)
        r.ray_trace()
        r.finish_accel()
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        img = torch.zeros((r.local_rows(8, 0, 1), st.image_width), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rec = []
        for k in range(3):
            r.render_bands_device(8, 0, 1, img.data_ptr(), a.cuda_stream)
            if with_visibility:
                stats0 = r.stats()
                out = r.visibility_device(stream=b)
                assert r.stats() == stats0, "rt_get_stats moved with the visibility call"
            torch.cuda.synchronize()
            cov, minfo = r.tile_mask(0)
            sets, son = r.tile_starts(0)
            covered, clear, linfo = r.tile_lists(0)
            rec.append((img.cpu().numpy().copy(), r.band_counters(), cov, minfo, sets, son, covered, clear, linfo))
        if with_visibility:
            hit_id, hit_t = internal(r)
            same_hits(host(out), hit_id, hit_t, "the visibility launch between band launches")
            assert r.device_visibility()[0] == (3, 0)
        seen.append(rec)
    for k, (x, y) in enumerate(zip(*seen)):
        assert np.array_equal(x[0], y[0]), f"band launch {k}: the image"
        assert x[1] == y[1], f"band launch {k}: rt_band_counters {x[1]} | {y[1]}"
        assert np.array_equal(x[2], y[2]) and x[3] == y[3], f"band launch {k}: rt_tile_mask"
        assert np.array_equal(x[4], y[4]) and x[5] == y[5], f"band launch {k}: rt_tile_starts"
        assert np.array_equal(x[6], y[6]) and np.array_equal(x[7], y[7]) and x[8] == y[8], f"band launch {k}: rt_tile_lists"
    assert seen[0][2][5], "the third band launch had no entry sets: the comparison shows nothing about them"


# ---- 10. refusals ------------------------------------------------------------------------------------------

def _raw(r, p, stream=None):
    return _lib.lib().rt_visibility_device(r._h, C.c_void_p(p[0]), C.c_void_p(p[1]), C.c_void_p(p[2]), stream)


def test_refusals(R):
    c = Case("robot")
    R.load_scene(c.scene, c.settings)
    rw, rh = c.settings.render_size()
    ref = vis(R)
    n = rw * rh
    good = {"tri_id": torch.full((rh, rw), 77, dtype=torch.int32, device="cuda"),
            "t": torch.full((rh, rw), 77, dtype=torch.float32, device="cuda"),
            "uv": torch.full((rh, rw, 2), 77, dtype=torch.float32, device="cuda")}
    host_arrays = [np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(2 * n, np.float32)]
    pinned = [torch.from_numpy(a.copy()).pin_memory() for a in host_arrays]
    before = R.device_visibility()

    def unchanged():
        torch.cuda.synchronize()
        assert R.device_visibility() == before
        assert all(bool((t == 77).all()) for t in good.values())

    ptrs = [good[k].data_ptr() for k in KEYS]
    for i in range(3):
        for what, bad in (("host", host_arrays[i].ctypes.data), ("pinned", pinned[i].data_ptr())):
            p = list(ptrs)
            p[i] = bad
            assert _raw(R, p) == -1, f"output {i} in {what} memory"   # RT_EINVAL
            unchanged()
    assert _raw(R, [None, None, None]) == -1
    unchanged()
    assert _raw(R, [ptrs[0], ptrs[1], ptrs[2] + 4]) == -1, "a misaligned d_uv"
    assert _raw(R, [None, None, ptrs[2] + 4]) == -1
    unchanged()
    # the Python mirror, by name: what each tensor is (its layout included) before where it lies
    with pytest.raises(TypeError, match="tri_id: a torch tensor"):
        R.visibility_device(out={"tri_id": host_arrays[0].reshape(rh, rw)})
    with pytest.raises(TypeError, match="t: dtype"):
        R.visibility_device(out={"t": good["tri_id"]})
    with pytest.raises(ValueError, match="uv: shape"):
        R.visibility_device(out={"uv": good["uv"].view(rh, 2 * rw)})
    with pytest.raises(ValueError, match="t: shape"):
        R.visibility_device(out={"t": good["t"][:-1]})
    with pytest.raises(ValueError, match="tri_id: the tensor is not contiguous"):
        R.visibility_device(out={"tri_id": torch.full((rw, rh), 77, dtype=torch.int32, device="cuda").t()})
    with pytest.raises(ValueError, match="t: the tensor is not contiguous"):
        R.visibility_device(out={"t": torch.full((rh, 2 * rw), 77, dtype=torch.float32, device="cuda")[:, ::2]})
    with pytest.raises(ValueError, match="tri_id: the tensor is on cpu"):
        R.visibility_device(out={"tri_id": pinned[0].view(rh, rw)})
    with pytest.raises(ValueError, match="unknown key"):
        R.visibility_device(out={"depth": good["t"]})
    with pytest.raises(ValueError, match="at least one"):
        R.visibility_device(out={})
    misaligned = torch.full((2 * n + 2,), 77, dtype=torch.float32, device="cuda")[1:-1].view(rh, rw, 2)
    with pytest.raises(RtError, match="8-byte aligned"):
        R.visibility_device(out={"uv": misaligned})
    assert bool((misaligned == 77).all())
    unchanged()
    # and the good arguments pass
    assert _raw(R, ptrs) == 0
    same_all(host(good), ref, "after the refusals")


def test_without_geometry_and_with_shapes_only(make_renderer):
    """A frame renders a renderer without geometry (the background): so does the call, with a frame's answers.
    Analytic shapes alone are geometry enough."""
    c = Case("robot")
    r = make_renderer()
    r.set_render_settings(c.settings)
    r.change_render_size(c.settings.image_width, c.settings.image_height)
    r.set_materials(c.scene.materials)
    hit_id, hit_t = internal(r)
    got = vis(r)
    same_hits(got, hit_id, hit_t, "no geometry")
    assert (got["tri_id"] == -1).all() and not bits(got["uv"]).any()
    r.add_sphere((0.0, 0.0, -3.0), 1.0, 0)
    hit_id, hit_t = internal(r)
    got = vis(r)
    same_hits(got, hit_id, hit_t, "a sphere alone")
    assert (got["tri_id"] == -2).any() and not bits(got["uv"]).any()
    assert r.device_visibility()[0] == (0, 2)
