"""The shaded query on device memory (rt_trace_ray_device, rt_get_device_shaded_queries; kernels.hip
shade_rays_kernel).

trace_ray_device must write, per ray, what Renderer.trace_ray (rt_trace_ray, pinned to the oracle and the golden
frames by tests/test_trace_ray.py) writes for that ray in the same renderer state: sources, t and flags bit for
bit, the counts rt_get_stats reports after the host call, and the colour bit for bit where the generic or the
reflective instance runs.  Where the plain instance runs (a scene the frames render with their plain pixel, over
a resident wide BVH) the colour is held to the oracle's within RGBA_TOL and, for camera rays, to the float RGBA
of a frame of the same renderer bit for bit.  rt_trace_ray stages its arrays and runs the generic or the reflective
instance itself, so every instance is also held to the oracle directly, on every 10th ray."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from golden_cases import Case
from oracle.bindings import Oracle
from raytracercpp_amd import _lib
from test_gpu_octree_build import assert_same_frame, bits, frame, make_renderer  # noqa: F401
from test_trace_ray import RGBA_TOL, SMALL_CASES, camera_rays

pytestmark = pytest.mark.gpu

BLOCK = 256   # lanes per block of shade_rays_kernel: 64 * WAVES_PER_BLOCK (kernels.hip:57)
KEYS = ("rgba", "hit_src", "t", "intersection_found", "shadowed")
DTYPES = (torch.float32, torch.int32, torch.float32, torch.uint8, torch.uint8)
N = 20000
PLAIN, GENERIC, REFL = 0, 1, 2   # rt_get_device_shaded_queries' order
PLAIN_CASE = "c3_bumpy70k"       # no map, sky, shape, debug shading or reflective material: KParams::plain holds


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(out):
    return tuple(out[k].cpu().numpy() for k in KEYS)


def zeros2():
    return torch.zeros(2, dtype=torch.int64, device="cuda")


def dev(r, o, d, depth=0, **kw):
    """trace_ray_device on the current stream, its outputs on the host (the copy waits for the kernel)."""
    return host(r.trace_ray_device(gpu(o), gpu(d), depth, **kw))


def ref_of(r, o, d, depth=0):
    """rt_trace_ray's answers and the (shadow, reflection) ray counts rt_get_stats reports after it."""
    out = r.trace_ray(o, d, depth)
    st = r.stats()
    return out, (st["shadow_rays"], st["reflection_rays"])


def same(got, ref, what, rgba=True):
    assert np.array_equal(got[1], ref[1]), f"{what}: {int((got[1] != ref[1]).sum())} sources differ"
    assert np.array_equal(bits(got[2]), bits(ref[2])), f"{what}: t differs in its bits"
    assert np.array_equal(got[3], ref[3]), f"{what}: intersection_found differs"
    assert np.array_equal(got[4], ref[4]), f"{what}: shadowed differs"
    if rgba:
        nd = int((bits(got[0]) != bits(ref[0])).any(axis=-1).sum())
        assert nd == 0, f"{what}: the colours of {nd} rays differ in their bits"


def random_rays(c, n=N, seed=17):
    """tests/test_trace_ray.py's random rays around the camera of case c."""
    rng = np.random.default_rng(seed)
    cam = np.asarray(c.scene.cam_pos, np.float32)
    o = (cam + rng.uniform(-1.5, 1.5, (n, 3))).astype(np.float32)
    d = rng.standard_normal((n, 3))
    d[: n // 2, 2] = -np.abs(d[: n // 2, 2]) * 3   # half of them roughly down the view axis
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def reflective(c):
    """KParams::has_reflection of case c: RT_SHADING with a material whose reflection is positive."""
    return c.settings.shading_method == 0 and bool((np.asarray(c.scene.materials).reshape(-1, 16)[:, 12] > 0).any())


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope="module")
def R():
    from raytracercpp_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rough(R):
    """The rough case's random rays and rt_trace_ray's answers to them, computed once."""
    c = case("rough")
    o, d = random_rays(c)
    R.load_scene(c.scene, c.settings)
    ref, cnt = ref_of(R, o, d)
    for a in ref:
        a.setflags(write=False)
    return c, o, d, ref, cnt


@pytest.fixture(scope="module")
def plain_ref():
    """The plain case's camera rays followed by N random rays, and the oracle's trace_ray of them, computed once."""
    c = case(PLAIN_CASE)
    oc, dc = camera_rays(c.scene, c.settings)
    orr, drr = random_rays(c)
    o, d = np.concatenate([oc, orr]), np.concatenate([dc, drr])
    e = Oracle(c.scene, c.settings).trace_ray(o, d, 0)
    for a in e[:5]:
        a.setflags(write=False)
    return c, o, d, len(oc), e


# ---- 1. equality with rt_trace_ray ------------------------------------------------------------------------

@pytest.mark.parametrize("name", SMALL_CASES)
def test_equals_trace_ray(R, name):
    c = case(name)
    R.load_scene(c.scene, c.settings)
    o, d = random_rays(c)
    od, dd = gpu(o), gpu(d)
    # every 10th ray, from both halves of the set, for the oracle (a call of its own: ray j draws pixel j's stream)
    o10, d10 = np.ascontiguousarray(o[::10]), np.ascontiguousarray(d[::10])
    assert len(o10) == 2000
    orc, oracle = Oracle(c.scene, c.settings), {}   # (its answers by depth, computed once each)
    for depth in (0, 1, c.settings.max_recursion_depth + 1):
        ref, cnt = ref_of(R, o, d, depth)
        calls0, rays0 = R.device_shaded_queries()
        counts = zeros2()
        got = host(R.trace_ray_device(od, dd, depth, counts=counts))
        calls, rays = R.device_shaded_queries()
        inst = [k for k in range(3) if calls[k] != calls0[k]]
        print(f"{name}, depth {depth}: instance {inst}, counts {counts.tolist()}, rt_get_stats {cnt}")
        # (the plain instance's colour is held to the oracle's, as in test_plain_instance)
        same(got, ref, f"{name}, depth {depth}", rgba=inst != [PLAIN])
        if inst == [PLAIN]:
            e = Oracle(c.scene, c.settings).trace_ray(o, d, depth)
            assert float(np.abs(got[0] - e[0]).max()) <= RGBA_TOL, f"{name}, depth {depth}"
        assert tuple(counts.tolist()) == cnt, f"{name}, depth {depth}: counts"
        if depth > c.settings.max_recursion_depth:
            assert inst == [] and rays == rays0, "the fill past the limit counts in no instance"
            assert np.all(got[0] == np.array([0, 0, 0, 1], np.float32)) and np.all(got[1] == -1)
            assert np.all(got[2] == -1.0) and not got[3].any() and not got[4].any()
        else:
            assert len(inst) == 1 and rays[inst[0]] == rays0[inst[0]] + N
            assert (inst == [REFL]) == reflective(c)
            if name in ("textured", "diffuse_map_skysphere", "shading_3"):
                assert inst == [GENERIC]
        # rt_trace_ray runs the same kernel in the generic and the reflective instance: every instance is also
        # held to the oracle itself, at depths 0 and 1
        if depth <= 1 and depth not in oracle:
            e = oracle[depth] = orc.trace_ray(o10, d10, depth)
            counts10 = zeros2()
            got10 = host(R.trace_ray_device(gpu(o10), gpu(d10), depth, counts=counts10))
            same(got10, e, f"{name}, depth {depth}, against the oracle", rgba=False)
            err = float(np.abs(got10[0] - e[0]).max())
            print(f"{name}, depth {depth}: max |RGBA - oracle| {err:.3g} over {len(o10)} rays, counts {counts10.tolist()}")
            assert err <= RGBA_TOL, f"{name}, depth {depth}"
            assert tuple(counts10.tolist()) == (e[5]["shadow_rays"], e[5]["reflection_rays"]), f"{name}, depth {depth}"


# ---- 2. the plain instance --------------------------------------------------------------------------------

PLAIN_STATES = {
    # name: (environment, rt_finish_accel first, the wide tree rt_get_stats names, the instance that runs)
    "sah_tree": (dict(RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1), True, 2, PLAIN),
    "quick_tree": (dict(RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1), False, 1, PLAIN),
    "no_wide_tree": (dict(RT_WBVH_QUICK_FIRST=0, RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1), False, 0, GENERIC),
    "RT_SHADE_PLAIN=0": (dict(RT_SHADE_PLAIN=0, RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1), True, 2, GENERIC),
}


@pytest.mark.parametrize("state", list(PLAIN_STATES))
def test_plain_instance(make_renderer, plain_ref, state):
    c, o, d, ncam, e = plain_ref
    env, finish, tree, inst = PLAIN_STATES[state]
    r = make_renderer(**env)
    r.load_scene(c.scene, c.settings)
    fr = frame(r)   # (the first frame starts the background build)
    if finish:
        r.finish_accel()
        fr = frame(r)
    assert r.stats()["wide_tree"] == tree
    ref, cnt = ref_of(r, o, d)
    counts = zeros2()
    got = dev(r, o, d, counts=counts)
    assert r.stats()["wide_tree"] == tree
    calls, rays = r.device_shaded_queries()
    want_calls = [0, 0, 0]
    want_calls[inst] = 1
    assert list(calls) == want_calls and rays[inst] == len(o), f"{state}: instance {inst} was to run, calls {calls}"
    same(got, ref, state, rgba=False)
    assert tuple(counts.tolist()) == cnt
    err = float(np.abs(got[0] - e[0]).max())
    nbits = int((bits(got[0]) != bits(ref[0])).any(axis=-1).sum())
    nframe = int((bits(got[0][:ncam]) != bits(fr["rgba"].reshape(-1, 4))).any(axis=-1).sum())
    print(f"{state}: max |RGBA - oracle| {err:.3g}; {nbits} of {len(o)} colours differ from rt_trace_ray's in their "
          f"bits; {nframe} of {ncam} camera rays differ from the frame's float RGBA")
    assert np.array_equal(got[1], e[1]) and np.array_equal(bits(got[2]), bits(e[2]))
    assert err <= RGBA_TOL
    if state == "RT_SHADE_PLAIN=0":
        # the generic instance is the one rt_trace_ray runs on this scene: its expressions, so its bits
        assert nbits == 0, f"{state}: the colours of {nbits} rays differ from rt_trace_ray's in their bits"
    assert nframe == 0, f"{state}: the colours of {nframe} camera rays differ from the frame's"
    assert np.array_equal(np.where(got[3][:ncam] == 1, got[1][:ncam], -1), fr["hit_id"])
    assert np.array_equal(bits(got[2][:ncam]), bits(fr["hit_t"])) and np.array_equal(got[4][:ncam], fr["shadow"])


# ---- 3. sizes ---------------------------------------------------------------------------------------------

def _guarded(n, pad=7):
    return {k: torch.full((n + pad, 4) if k == "rgba" else (n + pad,), 77, dtype=dt, device="cuda")
            for k, dt in zip(KEYS, DTYPES)}


_size_refs = {}


@pytest.mark.parametrize("name,inst", [("rough", REFL), (PLAIN_CASE, PLAIN), ("textured", GENERIC)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_sizes_and_counts(R, name, inst, n):
    """A partial wave and a partial block in each instance (the plain one parks its pixel in LDS)."""
    c = case(name)
    R.load_scene(c.scene, c.settings)
    if name not in _size_refs:
        o, d = random_rays(c, BLOCK + 1)
        oracle_rgba = Oracle(c.scene, c.settings).trace_ray(o, d, 0)[0] if inst == PLAIN else None
        _size_refs[name] = (o, d, R.trace_ray(o, d, 0), oracle_rgba)
    o, d, ref, oracle_rgba = _size_refs[name]
    _, cnt = ref_of(R, o[:n], d[:n])
    out = _guarded(n)
    counts = zeros2()
    calls0, rays0 = R.device_shaded_queries()
    od, dd = gpu(o[:n]), gpu(d[:n])
    ret = R.trace_ray_device(od, dd, out=out, counts=counts)
    assert ret is out
    got = host(out)
    # (the plain instance's colour came out rt_trace_ray's too, but only its other outputs are held to it here)
    same(tuple(a[:n] for a in got), tuple(a[:n] for a in ref), f"{name}, n = {n}", rgba=inst != PLAIN)
    for k, a in zip(KEYS, got):
        assert np.all(a[n:] == 77), f"{name}, n = {n}: {k} was written past n"
    if inst == PLAIN:
        assert float(np.abs(got[0][:n] - oracle_rgba[:n]).max()) <= RGBA_TOL
    assert tuple(counts.tolist()) == cnt
    R.trace_ray_device(od, dd, out=out, counts=counts)
    assert tuple(counts.tolist()) == (2 * cnt[0], 2 * cnt[1]), "the counts accumulate over two calls"
    calls, rays = R.device_shaded_queries()
    want_calls, want_rays = list(calls0), list(rays0)
    want_calls[inst] += 2
    want_rays[inst] += 2 * n
    assert list(calls) == want_calls and list(rays) == want_rays, f"{name}: instance {inst} was to run"


@pytest.mark.parametrize("name", ["rough", PLAIN_CASE, "textured"])
def test_optional_outputs(R, name):
    """Each optional output left out in turn, then all four: the others are what the full call writes."""
    c = case(name)
    R.load_scene(c.scene, c.settings)
    R.ray_trace()
    R.finish_accel()
    n = 1000
    o, d = random_rays(c, n)
    od, dd = gpu(o), gpu(d)
    full = dict(zip(KEYS, host(R.trace_ray_device(od, dd))))
    for leave in [(k,) for k in KEYS[1:]] + [KEYS[1:]]:
        out = {k: t for k, t in _guarded(n).items() if k not in leave}
        counts = zeros2()
        ret = R.trace_ray_device(od, dd, out=out, counts=counts)
        assert ret is out and set(ret) == set(KEYS) - set(leave)
        for k in out:
            a = out[k].cpu().numpy()
            assert np.array_equal(bits(a[:n]) if a.dtype == np.float32 else a[:n],
                                  bits(full[k]) if a.dtype == np.float32 else full[k]), f"{name}: {k} without {leave}"
            assert np.all(a[n:] == 77)
        assert int(counts[0]) > 0


def test_empty_call_launches_nothing(R, rough):
    c, o, d, ref, _ = rough
    R.load_scene(c.scene, c.settings)
    out = _guarded(0, 5)
    counts = torch.full((2,), 5, dtype=torch.int64, device="cuda")
    before = R.device_shaded_queries()
    e = torch.zeros((0, 3), device="cuda")
    R.trace_ray_device(e, e.clone(), out=out, counts=counts)
    torch.cuda.synchronize()
    assert R.device_shaded_queries() == before
    assert all(bool((out[k] == 77).all()) for k in KEYS) and bool((counts == 5).all())
    # (the pointers are not read: null ones pass with n == 0)
    assert _lib.lib().rt_trace_ray_device(R._h, None, None, 0, 0, 0, None, None, None, None, None, None, None) == 0
    assert R.device_shaded_queries() == before
    assert R.trace_ray_device(e, e.clone())["rgba"].shape == (0, 4)


@pytest.mark.parametrize("name", ["rough", "textured"])
def test_host_queries_leave_device_counters_alone(R, name):
    """rt_trace_ray runs the device query's kernel over a staged copy of its arrays, one block and a lane here; it
    is no device query, and neither are rt_trace_rays and rt_wide_query."""
    c = case(name)
    R.load_scene(c.scene, c.settings)
    o, d = random_rays(c, BLOCK + 1)

    def counters():
        return R.device_ray_queries(), R.device_shaded_queries(), R.device_shaded_batches()

    before = counters()
    rgba = R.trace_ray(o, d, 0)[0]
    assert rgba.shape == (BLOCK + 1, 4) and counters() == before, "trace_ray at depth 0"
    past = R.trace_ray(o, d, c.settings.max_recursion_depth + 1)
    st = R.stats()
    assert (st["shadow_rays"], st["reflection_rays"]) == (0, 0)
    assert np.all(past[0] == np.array([0, 0, 0, 1], np.float32)) and np.all(past[1] == -1)
    assert np.all(past[2] == -1.0) and not past[3].any() and not past[4].any()
    assert counters() == before, "trace_ray past the depth limit"
    assert len(R.trace_rays(o, d)[0]) == BLOCK + 1 and counters() == before, "trace_rays"
    assert len(R.wide_query(o, d, kind=0)["status"]) == BLOCK + 1 and counters() == before, "wide_query"


# ---- 4. first_ray -----------------------------------------------------------------------------------------

def test_first_ray_keys_the_rough_streams(R, rough):
    c, o, d, ref, cnt = rough
    R.load_scene(c.scene, c.settings)
    od, dd = gpu(o), gpu(d)
    out = {k: torch.zeros((N, 4) if k == "rgba" else (N,), dtype=dt, device="cuda") for k, dt in zip(KEYS, DTYPES)}
    counts = zeros2()
    cut = 9000
    R.trace_ray_device(od[:cut].contiguous(), dd[:cut].contiguous(), first_ray=0,
                       out={k: t[:cut] for k, t in out.items()}, counts=counts)
    R.trace_ray_device(od[cut:].contiguous(), dd[cut:].contiguous(), first_ray=cut,
                       out={k: t[cut:] for k, t in out.items()}, counts=counts)
    same(host(out), ref, "two calls with first_ray 0 and 9000")
    assert tuple(counts.tolist()) == cnt
    # the same rays keyed five pixels on: the rough pixels draw other samples
    moved = dev(R, o, d, first_ray=5)
    same(moved, ref, "first_ray 5", rgba=False)
    changed = int((bits(moved[0]) != bits(ref[0])).any(axis=-1).sum())
    print(f"first_ray 5: the colours of {changed} of {N} rays change")
    assert changed > 0
    # ray i of a call with first_ray 5 is ray i + 5's stream: the same ray there gives the same colour
    o2, d2 = np.concatenate([o[:5], o[:N - 5]]), np.concatenate([d[:5], d[:N - 5]])
    shifted = dev(R, o2, d2, first_ray=0)
    assert np.array_equal(bits(shifted[0][5:]), bits(moved[0][:N - 5]))


# ---- 5. modes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,name", [("exact", PLAIN_CASE), ("exact", "rough"), ("RT_WBVH=0", PLAIN_CASE),
                                       ("RT_WBVH=0", "rough"), ("brute_force", "brute_force")])
def test_modes(make_renderer, mode, name):
    c = case(name)
    r = make_renderer(RT_WBVH=0) if mode == "RT_WBVH=0" else make_renderer()
    if mode == "exact":
        r.set_exact(True)
    if mode == "brute_force":
        assert not c.settings.enable_bvh
    r.load_scene(c.scene, c.settings)
    r.ray_trace()
    r.finish_accel()
    o, d = random_rays(c)
    for depth in (0, 1):
        ref, cnt = ref_of(r, o, d, depth)
        counts = zeros2()
        same(dev(r, o, d, depth, counts=counts), ref, f"{name}, {mode}, depth {depth}")
        assert tuple(counts.tolist()) == cnt
    # (no wide BVH is read in these modes: a plain scene takes the generic instance)
    calls, _ = r.device_shaded_queries()
    assert calls == ((0, 0, 2) if reflective(c) else (0, 2, 0))


# ---- 6. stream order --------------------------------------------------------------------------------------

def test_stream_order(R, rough):
    """The rays are produced on a side stream behind long-running work and overwritten on it right after the
    call; a consumer on that stream reads the outputs; no host wait in between, and the host is back from the
    call while that work is still pending.  (This exercises the order; a race could still pass by luck.)"""
    c, o, d, ref, cnt = rough
    R.load_scene(c.scene, c.settings)
    R.trace_ray(o[:1], d[:1])   # (the scene is resident: the call below has nothing to build)
    oc, dc = gpu(o), gpu(d)
    a = torch.rand((4096, 4096), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    before = torch.cuda.Event()
    with torch.cuda.stream(side):
        b = a
        for _ in range(24):
            b = (b @ a) * (1.0 / 4096)
        before.record(side)
        ot, dt = oc.clone(), dc.clone()
        counts = zeros2()
        out = R.trace_ray_device(ot, dt, counts=counts, stream=side)
        pending = not before.query()
        ot.fill_(float("nan"))
        dt.zero_()
        seen = {k: v.clone() for k, v in out.items()}
        seen_counts = counts.clone()
    assert pending, "the call returned only after the work queued before it had finished"
    side.synchronize()
    same(host(seen), ref, "the consumer on the side stream")
    assert tuple(seen_counts.tolist()) == cnt
    # and with the current stream taken by default
    with torch.cuda.stream(side):
        ot2, dt2 = oc.clone(), dc.clone()
        out2 = R.trace_ray_device(ot2, dt2)
        ot2.zero_()
        seen2 = {k: v.clone() for k, v in out2.items()}
    side.synchronize()
    same(host(seen2), ref, "the current stream by default")
    torch.cuda.synchronize()
    del b


# ---- 7. scene changes wait --------------------------------------------------------------------------------

def _changed(c, what):
    """(scene, settings) of case c after one change, and how to apply it to a renderer that holds c."""
    sc = c.scene
    if what == "materials":
        m = np.array(sc.materials, np.float32).reshape(-1, 16).copy()
        m[:, :9] = m[:, :9][:, ::-1] * 0.5 + 0.125   # the ambient, diffuse and specular colours
        new = dataclasses.replace(sc, materials=m)
        return new, lambda r: r.set_materials(m)
    if what == "texture":
        slot = sorted(sc.textures)[0]
        img = np.ascontiguousarray(np.asarray(sc.textures[slot], np.float32)[::-1]) * np.float32(0.5)
        tex = dict(sc.textures)
        tex[slot] = img
        new = dataclasses.replace(sc, textures=tex)
        return new, lambda r: r._set_tex(slot, img)
    assert what == "geometry"
    tri = (np.asarray(sc.tri, np.float32).reshape(-1, 3) * np.float32(0.75) + np.array([0.1, -0.05, 0.0], np.float32))
    tri = tri.reshape(-1, 9).astype(np.float32)
    new = dataclasses.replace(sc, tri=tri)
    return new, lambda r: r.set_triangles(tri, sc.tri_mat, sc.tri_uv)


@pytest.mark.parametrize("what", ["materials", "texture", "geometry", "close"])
def test_scene_changes_and_close_wait_for_queries(make_renderer, what):
    c = case("diffuse_map_skysphere")
    n = 1 << 19
    o, d = random_rays(c, n, seed=3)
    od, dd = gpu(o), gpu(d)
    r = make_renderer()
    r.load_scene(c.scene, c.settings)
    old = host(r.trace_ray_device(od, dd))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    if what == "close":
        from raytracercpp_amd.renderer import Renderer
        r3 = Renderer(0)
        r3.load_scene(c.scene, c.settings)
        out3 = r3.trace_ray_device(od, dd, stream=side)
        r3.close()
        side.synchronize()
        torch.cuda.synchronize()
        same(host(out3), old, "the query in flight at close()")
        return
    new_scene, apply = _changed(c, what)
    fresh = make_renderer()
    fresh.load_scene(new_scene, c.settings)
    want = fresh.trace_ray(o, d, 0)
    assert (bits(want[0]) != bits(old[0])).any(), "the change is visible in the colours"
    out = r.trace_ray_device(od, dd, stream=side)
    # no wait: the scene is changed and asked again while the first query may still run
    apply(r)
    out2 = r.trace_ray_device(od, dd)
    side.synchronize()
    same(host(out), old, f"the query in flight while the {what} changed")
    same(host(out2), want, f"the query after the {what} changed")


# ---- 8. nothing shared with band launches -------------------------------------------------------------------

@pytest.mark.parametrize("name", [PLAIN_CASE, "rough"])
def test_band_launch_beside_a_query(make_renderer, name):
    c = case(name)
    st = c.settings
    r = make_renderer()
    r.load_scene(c.scene, st)
    r.ray_trace()
    r.finish_accel()
    W, rows = st.image_width, r.local_rows(8, 0, 1)
    alone = torch.zeros((rows, W), dtype=torch.int32, device="cuda")
    for _ in range(2):   # (the second launch has its heavy list, as the one below)
        r.render_bands_device(8, 0, 1, alone.data_ptr(), 0)
        torch.cuda.synchronize()
    want_counters = r.band_counters()
    n = 1 << 18
    o, d = random_rays(c, n, seed=4)
    od, dd = gpu(o), gpu(d)
    ref, cnt = ref_of(r, o[:N], d[:N])
    r.render_bands_device(8, 0, 1, alone.data_ptr(), 0)   # (a launch after the host call counts what the one before it did)
    torch.cuda.synchronize()
    assert r.band_counters() == want_counters
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    img = torch.zeros((rows, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    counts = zeros2()
    with torch.cuda.stream(s2):
        out_a = r.trace_ray_device(od, dd, stream=s2)
    r.render_bands_device(8, 0, 1, img.data_ptr(), s1.cuda_stream)
    with torch.cuda.stream(s2):
        out_b = r.trace_ray_device(od[:N].contiguous(), dd[:N].contiguous(), counts=counts, stream=s2)
    torch.cuda.synchronize()
    assert r.band_counters() == want_counters, "the frame's counters hold the frame's counts alone"
    assert torch.equal(img, alone), "the image equals an undisturbed frame"
    same(host(out_b), ref, "the query beside the band launch")
    assert tuple(counts.tolist()) == cnt
    assert out_a["rgba"].shape == (n, 4)


# ---- 9. refusals ------------------------------------------------------------------------------------------

def _raw(r, p, n, depth=0, first=0):
    v = [C.c_void_p(x) for x in p]
    return _lib.lib().rt_trace_ray_device(r._h, v[0], v[1], n, depth, first, v[2], v[3], v[4], v[5], v[6], v[7], None)


def test_refusals(R, rough):
    c, o, d, ref, _ = rough
    R.load_scene(c.scene, c.settings)
    n = 64
    good = [gpu(o[:n]), gpu(d[:n])] + [t[:n] for t in _guarded(n, 0).values()] + \
           [torch.full((2,), 5, dtype=torch.int64, device="cuda")]
    host_arrays = [np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32),
                   np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8),
                   np.zeros(2, np.int64)]
    pinned = [torch.from_numpy(a.copy()).pin_memory() for a in host_arrays]
    before = R.device_shaded_queries()

    def unchanged():
        torch.cuda.synchronize()
        assert R.device_shaded_queries() == before
        assert all(bool((t == 77).all()) for t in good[2:7]) and bool((good[7] == 5).all())

    ptrs = [t.data_ptr() for t in good]
    for i in range(8):
        for what, bad in (("host", host_arrays[i].ctypes.data), ("pinned", pinned[i].data_ptr())):
            p = list(ptrs)
            p[i] = bad
            if i == 2 and bad % 16:
                continue   # (an unaligned host d_rgba is refused for its alignment: below)
            rc = _raw(R, p, n)
            assert rc == -1, f"argument {i} in {what} memory: {rc}"   # RT_EINVAL
            unchanged()
    if torch.cuda.device_count() > 1:
        for i in range(8):
            p = list(ptrs)
            other = torch.zeros(4 * n, dtype=torch.float32, device="cuda:1")
            p[i] = other.data_ptr()
            assert _raw(R, p, n) == -1, f"argument {i} in another device's memory"
            unchanged()
    # a null d_orig / d_dir / d_rgba with n > 0 (the other outputs and the counts may be null)
    for i in range(3):
        p = list(ptrs)
        p[i] = None
        assert _raw(R, p, n) == -1
        unchanged()
    # d_rgba not 16-byte aligned
    wide = torch.full((4 * n + 4,), 77, dtype=torch.float32, device="cuda")
    for off in (1, 2, 3):
        p = list(ptrs)
        p[2] = wide.data_ptr() + 4 * off
        assert _raw(R, p, n) == -1 and b"16-byte aligned" in _lib.lib().rt_last_error()
        torch.cuda.synchronize()
        assert bool((wide == 77).all())
    unchanged()
    # counts, depths and first rays out of range
    for bad_n in ((1 << 30) + 1, -1, 1 << 40):
        assert _raw(R, ptrs, bad_n) == -1
    assert _raw(R, ptrs, n, depth=-1) == -1
    # (the last three: first_ray + n does not fit 64 bits; no sum may wrap back into range)
    for first in (-1, (1 << 32) - n + 1, 1 << 32, 1 << 40, (1 << 63) - 1, (1 << 63) - n, (1 << 63) - n + 1, -(1 << 63)):
        assert _raw(R, ptrs, n, first=first) == -1, first
    assert _raw(R, ptrs, 1 << 30, first=(1 << 32) - (1 << 30) + 1) == -1
    assert _raw(R, ptrs, -1, first=(1 << 63) - 1) == -1 and _raw(R, ptrs, 1 << 40, first=(1 << 63) - 1) == -1
    unchanged()
    with pytest.raises(_lib.RtError):
        R.trace_ray_device(good[0], good[1], -1)
    with pytest.raises(_lib.RtError):
        R.trace_ray_device(good[0], good[1], first_ray=-1)
    # the Python mirror refuses the same before any pointer is taken
    with pytest.raises(ValueError, match="not on a GPU"):
        R.trace_ray_device(pinned[0], pinned[1])
    with pytest.raises(ValueError, match="rgba: shape"):
        R.trace_ray_device(good[0], good[1], out=dict(rgba=good[2][: n - 1]))
    with pytest.raises(ValueError, match="rgba: the tensor is not contiguous"):
        R.trace_ray_device(good[0], good[1], out=dict(rgba=torch.zeros((n, 8), device="cuda")[:, :4]))
    with pytest.raises(ValueError, match="out: rgba is needed"):
        R.trace_ray_device(good[0], good[1], out=dict(t=good[4]))
    unchanged()
    # the largest first_ray, and the good arguments, pass
    assert _raw(R, ptrs, n, first=(1 << 32) - n) == 0
    assert _raw(R, ptrs, n) == 0
    same(host(dict(zip(KEYS, good[2:7]))), tuple(a[:n] for a in ref), "after the refusals")


def test_invalid_scene_is_refused_as_by_trace_ray(make_renderer):
    """An enabled map that is missing: the code rt_trace_ray returns, and no launch."""
    c = case("diffuse_map_skysphere")
    r = make_renderer()
    r.load_scene(c.scene, c.settings)
    r._set_tex(sorted(c.scene.textures)[0], None)
    o, d = random_rays(c, 64)
    with pytest.raises(_lib.RtError) as host_err:
        r.trace_ray(o, d, 0)
    with pytest.raises(_lib.RtError) as dev_err:
        r.trace_ray_device(gpu(o), gpu(d))
    assert dev_err.value.code == host_err.value.code == -1   # RT_EINVAL
    assert "invalid scene" in str(dev_err.value)
    assert r.device_shaded_queries() == ((0, 0, 0), (0, 0, 0))


# ---- 10. ray index past 2^31 --------------------------------------------------------------------------------

def test_ray_index_past_2_31(R):
    """n = 715,827,883 + 1,141 rays: from ray 715,827,883 on, 3 i does not fit 32 bits.  Every ray points away from
    the scene except the last 2,048, the textured case's rays, whose answers rt_trace_ray gives for them alone
    (the case draws no rough-reflection sample, so a ray's index does not key its colour).  rgba and t only:
    the inputs take 8.6 GB each, the outputs 11.5 and 2.9 GB."""
    c = case("textured")
    R.load_scene(c.scene, c.settings)
    tail = 2048
    o, d = random_rays(c, tail)
    ref = R.trace_ray(o, d, 0)
    assert ref[3].any() and not ref[3].all()
    n = 715_827_883 + 1141
    assert n == 715_829_024 and 3 * (n - tail) < 2 ** 31 < 3 * (n - tail + 1024)
    cam = np.asarray(c.scene.cam_pos, np.float32)
    away_o, away_d = (cam + np.array([0, 0, 100], np.float32))[None], np.array([[0, 0, 1]], np.float32)
    head = R.trace_ray(away_o, away_d, 0)
    assert head[3][0] == 0
    od = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    dd = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    od[:] = gpu(away_o)
    dd[:] = gpu(away_d)
    od[n - tail:] = gpu(o[:tail])
    dd[n - tail:] = gpu(d[:tail])
    out = R.trace_ray_device(od, dd, out=dict(rgba=torch.empty((n, 4), device="cuda"), t=torch.empty(n, device="cuda")))
    assert set(out) == {"rgba", "t"}
    assert np.array_equal(bits(out["rgba"][n - tail:].cpu().numpy()), bits(ref[0][:tail]))
    assert np.array_equal(bits(out["t"][n - tail:].cpu().numpy()), bits(ref[2][:tail]))
    assert bool((out["rgba"][:n - tail].view(torch.int32) == gpu(head[0]).view(torch.int32)).all())
    assert bool((out["t"][:n - tail].view(torch.int32) == gpu(head[2]).view(torch.int32)).all())
    del out, od, dd
    torch.cuda.empty_cache()
