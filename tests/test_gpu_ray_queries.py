"""The ray queries on device memory (rt_trace_rays_device, rt_is_shadowed_device, rt_get_device_ray_queries;
kernels.hip closest_rays_kernel / shadow_points_kernel).

trace_rays_device answers through the frames' certified wide-BVH query and must write, bit for bit, what
Renderer.trace_rays (trace_rays_kernel: the exact octree walk, pinned to the oracle by
tests/test_gpu_parity.py::test_trace_rays_match_oracle) writes for the same rays in the same renderer state,
and what the oracle's bvh_query answers.  is_shadowed_device is compared with the recipe of
tests/test_gpu_wide.py::_shadow_decisions (the ray the kernel builds, the oracle's record of it, the float32
distance test) on every pair, and with known answers on analytic shapes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import test_gpu_wide as tg
import test_wbvh as tw
from oracle.bindings import Oracle
from raytracercpp_amd import _lib, scenes
from raytracercpp_amd.scene import RenderSettings
from test_gpu_octree_build import assert_same_frame, bits, frame, make_renderer  # noqa: F401
from test_gpu_parity import _random_rays, _voxel_scene

pytestmark = pytest.mark.gpu

BLOCK = 256   # lanes per block of both kernels: 64 * WAVES_PER_BLOCK (kernels.hip:57)
KEYS = ("tri_id", "t", "u", "v", "ret")
DTYPES = (torch.int32, torch.float32, torch.float32, torch.float32, torch.uint8)
N = 20000


@pytest.fixture(scope="module")
def R():
    from raytracercpp_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(out):
    return tuple(out[k].cpu().numpy() for k in KEYS)


def dev(r, o, d, **kw):
    """trace_rays_device on the current stream, its outputs on the host (the copy waits for the kernel)."""
    return host(r.trace_rays_device(gpu(o), gpu(d), **kw))


def same(got, ref, what):
    assert np.array_equal(got[0], ref[0]), f"{what}: {int((got[0] != ref[0]).sum())} triangle indices differ"
    assert np.array_equal(got[4], ref[4]), f"{what}: {int((got[4] != ref[4]).sum())} return values differ"
    for k in (1, 2, 3):
        assert np.array_equal(bits(got[k]), bits(ref[k])), f"{what}: {KEYS[k]} differs in its bits"


def with_specials(o, d, rng, count=240):
    """Rays with a NaN or an infinite component in the origin or the direction among the others."""
    o, d = o.copy(), d.copy()
    k = rng.choice(len(o), count, replace=False)
    vals = np.array([np.nan, np.inf, -np.inf], np.float32)
    for j, i in enumerate(k):
        (o if j % 2 else d)[i, rng.integers(0, 3)] = vals[j % 3]
    return o, d


_cache = {}


def stress(name):
    """(scene, settings, origins, directions) of one stress input, N rays each (the cases' own counts)."""
    if name in _cache:
        return _cache[name]
    rng = np.random.default_rng(5)
    if name in ("robot", "robot_nonfinite"):
        sc, st = scenes.robot1080(width=64, height=36)
        o, d = _random_rays(rng, N, np.array([0, 0, -4], np.float32), 3.0)
        if name == "robot_nonfinite":
            # (a set of its own: for most non-finite rays the oracle's bvh_query names a triangle beside its
            # NaN record where rt_trace_rays writes -1, so the sets compared with the oracle hold finite rays
            # only, as in tests/test_gpu_parity.py::test_trace_rays_match_oracle)
            o, d = with_specials(o, d, rng)
    elif name == "voxels":
        sc = _voxel_scene()
        st = RenderSettings(bvh_max_depth=12, bvh_leaf_object_count=8)
        o, d = _random_rays(rng, N, np.zeros(3, np.float32), 2.5)
        d[:10000] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 10000)] * rng.choice([-1, 1], (10000, 1))
    elif name == "grazing":
        sc, st = scenes.robot1080(width=64, height=36)
        o, d = _random_rays(rng, N, np.array([0, 0, -4], np.float32), 3.0)
        tiny = rng.choice(np.array([0.0, 1e-13, -1e-13, 1e-30, -1e-41], np.float32), (N,))
        d[np.arange(N), rng.integers(0, 3, N)] = tiny
    elif name in ("tiny", "huge"):
        f = np.float32(1e-13 if name == "tiny" else 1e13)
        sc, st = scenes.robot1080(width=64, height=36)
        sc.tri = (sc.tri * f).astype(np.float32)
        o, d = _random_rays(rng, N, np.array([0, 0, -4], np.float32) * f, 3.0 * f)
    elif name == "grazing_plane":
        tri, o, d = tw.grazing_plane_case()
        sc, st = tg._scene(tri)
    elif name == "grazing_sphere":
        tri, o, d = tw.grazing_sphere_case()[:3]
        sc, st = tg._scene(tri)
    else:
        raise KeyError(name)
    assert len(o) == N
    _cache[name] = (sc, st, o, d)
    return _cache[name]


@pytest.fixture(scope="module")
def robot(R):
    """The robot's rays, non-finite ones among them, and trace_rays' answers to them, computed once."""
    sc, st, o, d = stress("robot_nonfinite")
    R.load_scene(sc, st)
    ref = R.trace_rays(o, d)
    for a in ref:
        a.setflags(write=False)
    return sc, st, o, d, ref


# ---- 1. equality on the stress inputs ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["robot", "robot_nonfinite", "voxels", "grazing", "tiny", "huge", "grazing_plane",
                                  "grazing_sphere"])
def test_equals_trace_rays_on_stress_inputs(R, name):
    sc, st, o, d = stress(name)
    R.load_scene(sc, st)
    ref = R.trace_rays(o, d)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = dev(R, o, d, counts=counts)
    c = counts.cpu().numpy()
    print(f"{name}: wide_tree {R.stats()['wide_tree']}, {int(c[0])} rays by the wide query, {int(c[1])} by the octree walk")
    same(got, ref, name)
    assert int(c.sum()) == N
    if name in ("robot", "grazing_plane"):
        oi, ot, ou, ov, orr, _ = Oracle(sc, st).bvh_query(o, d)
        same(got, (oi, ot, ou, ov, orr), name + " against the oracle")


# ---- 2. sizes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, N])
def test_sizes_and_counts(R, robot, n):
    sc, st, o, d, ref = robot
    R.load_scene(sc, st)
    pad = 7
    out = {k: torch.full((n + pad,), 77, dtype=dt, device="cuda") for k, dt in zip(KEYS, DTYPES)}
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    calls0, rays0 = R.device_ray_queries()
    od, dd = gpu(o[:n]), gpu(d[:n])
    ret = R.trace_rays_device(od, dd, out=out, counts=counts)
    assert ret is out
    got = host(out)
    same(tuple(a[:n] for a in got), tuple(a[:n] for a in ref), f"n = {n}")
    for k, a in zip(KEYS, got):
        assert np.all(a[n:] == 77), f"n = {n}: {k} was written past n"
    c1 = counts.cpu().numpy().copy()
    assert int(c1.sum()) == n
    R.trace_rays_device(od, dd, out=out, counts=counts)
    c2 = counts.cpu().numpy()
    assert np.array_equal(c2, 2 * c1), "the counts accumulate over two calls"
    calls, rays = R.device_ray_queries()
    assert calls == (calls0[0] + 2, calls0[1]) and rays == (rays0[0] + 2 * n, rays0[1])


def test_empty_call_launches_nothing(R, robot):
    sc, st, o, d, ref = robot
    R.load_scene(sc, st)
    out = {k: torch.full((5,), 77, dtype=dt, device="cuda") for k, dt in zip(KEYS, DTYPES)}
    counts = torch.full((2,), 5, dtype=torch.int64, device="cuda")
    before = R.device_ray_queries()
    e = torch.zeros((0, 3), device="cuda")
    R.trace_rays_device(e, e.clone(), out=out, counts=counts)
    sh = torch.full((5,), 77, dtype=torch.uint8, device="cuda")
    R.is_shadowed_device(e, e.clone(), out=sh)
    torch.cuda.synchronize()
    assert R.device_ray_queries() == before
    assert all(bool((out[k] == 77).all()) for k in KEYS) and bool((sh == 77).all()) and bool((counts == 5).all())
    # (the pointers are not read: null ones pass with n == 0)
    L = _lib.lib()
    assert L.rt_trace_rays_device(R._h, None, None, 0, None, None, None, None, None, None, None) == 0
    assert L.rt_is_shadowed_device(R._h, None, None, 0, None, None, None) == 0
    assert R.device_ray_queries() == before
    assert R.trace_rays_device(e, e.clone())["t"].shape == (0,)


# ---- 3. the fast path is taken -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grazing_sphere", "robot"])
def test_wide_query_answers_what_it_certifies(R, name):
    sc, st, o, d = stress(name)
    R.load_scene(sc, st)
    ref = R.trace_rays(o, d)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = dev(R, o, d, counts=counts)
    assert R.stats()["wide_tree"] in (1, 2)
    same(got, ref, name)
    fin = np.isfinite(o).all(1) & np.isfinite(d).all(1)   # (rt_wide_query is given the finite rays)
    certified = int((R.wide_query(o[fin], d[fin], kind=0)["status"] != 2).sum())
    c = counts.cpu().numpy()
    print(f"{name}: {int(c[0])} of {N} rays by the wide query, rt_wide_query certifies {certified}")
    assert certified > 0.5 * N
    assert c[0] >= 0.9 * certified and int(c.sum()) == N


@pytest.mark.parametrize("mode", ["RT_WBVH=0", "exact", "brute_force"])
@pytest.mark.parametrize("name", ["robot", "grazing_sphere"])
def test_modes_without_the_wide_query(make_renderer, name, mode):
    sc, st, o, d = stress(name)
    if mode == "brute_force":
        st = st.copy(enable_bvh=False)
        o, d = o[:2000], d[:2000]   # (every ray tests every triangle)
    r = make_renderer(RT_WBVH=0) if mode == "RT_WBVH=0" else make_renderer()
    if mode == "exact":
        r.set_exact(True)
    r.load_scene(sc, st)
    ref = r.trace_rays(o, d)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = dev(r, o, d, counts=counts)
    same(got, ref, f"{name}, {mode}")
    c = counts.cpu().numpy()
    assert c[0] == 0 and c[1] == len(o)
    if mode != "brute_force":
        # the same answers as the default renderer's (the octree's record is the wide query's)
        r2 = make_renderer()
        r2.load_scene(sc, st)
        same(dev(r2, o, d), got, f"{name}, default against {mode}")


def test_quick_tree_then_sah_tree(make_renderer, robot):
    sc, st, o, d, ref = robot
    r = make_renderer(RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1)
    r.load_scene(sc, st)
    for tree in (1, 2):
        if tree == 2:
            r.finish_accel()
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        got = dev(r, o, d, counts=counts)
        assert r.stats()["wide_tree"] == tree
        same(got, ref, f"wide_tree {tree}")
        assert int(counts[0]) > 0.5 * N


# ---- 4. camera rays ------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", [0.0, 1e-7, 1e-4, 1e-1])
def test_camera_rays(R, h):
    """Rays from the camera position read the camera's risk words, its risk cap and the scene bound; the same
    rays after the camera has moved are ordinary rays."""
    tri, o, d, cam = tw._plane_frame(23, h)
    sc, st = tg._scene(tri, cam=cam, light=cam + np.float32(7.0))
    R.load_scene(sc, st)
    assert np.array_equal(o, np.repeat(np.asarray(cam, np.float32)[None], len(o), 0))
    ref = R.trace_rays(o, d)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    same(dev(R, o, d, counts=counts), ref, f"camera at {h}")
    pos, pinv, c2w = R.get_camera_matrices()
    assert np.array_equal(pos, np.asarray(cam, np.float32))
    R.set_camera_matrices(pos + np.array([0.5, -0.25, 1.0], np.float32), pinv, c2w)
    counts2 = torch.zeros(2, dtype=torch.int64, device="cuda")
    same(dev(R, o, d, counts=counts2), ref, f"camera moved away from the rays' origin ({h})")
    print(f"camera at {h}: {int(counts[0])} rays by the wide query as camera rays, {int(counts2[0])} as ordinary rays")


# ---- 5. is_shadowed_device, triangles ------------------------------------------------------------------

def _terminator():
    """The sphere-terminator pairs of tests/test_gpu_wide.py::test_device_light_sphere_terminator."""
    rng = np.random.default_rng(8)
    sc, _ = scenes.bumpy70k(width=8, height=8)
    tri = sc.tri
    T = tri.reshape(-1, 3, 3).astype(np.float64)
    L = np.array([5.0, 0.5, 1.0], np.float32)
    nn = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    area = np.linalg.norm(nn, axis=1)
    nn /= np.maximum(area, 1e-30)[:, None]
    toL = L - T.mean(1)
    toL /= np.linalg.norm(toL, axis=1, keepdims=True)
    key = np.where(area > 1e-12, np.abs((nn * toL).sum(1)), np.inf)
    k = np.argsort(key)[:N]
    uv = rng.uniform(0, 1, (len(k), 2))
    uv[uv.sum(1) > 1] = 1 - uv[uv.sum(1) > 1]
    p = (T[k, 0] + (T[k, 1] - T[k, 0]) * uv[:, :1] + (T[k, 2] - T[k, 0]) * uv[:, 1:]).astype(np.float32)
    return tri, p, nn[k].astype(np.float32), L, np.array([0.0, 0.0, 6.0], np.float32)


def _shadow_case(name):
    if name == "terminator":
        return _terminator()
    tri, p, nrm, L = tg._light_plane(float(name))
    return tri, p, nrm, L, np.array([0.0, 30.0, 0.0], np.float32)


def _shadow_reference(r, oracle, p, nrm, light):
    """tests/test_gpu_wide.py::_shadow_decisions' reference for every pair: the ray (o, d) the kernel builds
    (rt_wide_query kind 2 returns it), the oracle's record of it, then is_shadowed's distance test in float32
    in its operation order.  (r's scene light is `light`; the oracle holds the triangles only.)"""
    g = r.wide_query(p, nrm, kind=2)
    oi, ot, ou, ov, orr, _ = oracle.bvh_query(g["o"], g["d"])
    q = g["o"] + g["d"] * ot[:, None]
    pq = p - q
    pl = p - np.asarray(light, np.float32)[None]
    l2 = lambda v: (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]   # noqa: E731
    return ((orr != 0) & (l2(pq) < l2(pl))).astype(np.uint8)


@pytest.mark.parametrize("name", ["0.0", "1e-06", "0.001", "terminator"])
def test_is_shadowed_triangles(R, name):
    tri, p, nrm, L, cam = _shadow_case(name)
    assert len(p) == N
    sc, st = tg._scene(tri, cam, L)
    R.load_scene(sc, st)
    oracle = tg._oracle_for(sc)
    ref = _shadow_reference(R, oracle, p, nrm, L)
    pd, nd = gpu(p), gpu(nrm)
    calls0, rays0 = R.device_ray_queries()
    got = R.is_shadowed_device(pd, nd).cpu().numpy()
    print(f"light case {name}: {int(ref.sum())} of {N} pairs shadowed, {int((got != ref).sum())} differ")
    assert got.dtype == np.uint8 and np.array_equal(got, ref)
    # the scene's light given explicitly takes the same path
    assert np.array_equal(R.is_shadowed_device(pd, nd, light=L).cpu().numpy(), ref)
    for n in (1, 65):
        out = torch.full((n + 3,), 77, dtype=torch.uint8, device="cuda")
        R.is_shadowed_device(pd[:n].contiguous(), nd[:n].contiguous(), out=out)
        o = out.cpu().numpy()
        assert np.array_equal(o[:n], ref[:n]) and np.all(o[n:] == 77), n
    calls, rays = R.device_ray_queries()
    assert calls == (calls0[0], calls0[1] + 4) and rays == (rays0[0], rays0[1] + 2 * N + 66)
    # another light: the answers of a renderer whose scene light it is (and that renderer's reference)
    L2 = (L + np.array([0.75, 1.5, -0.5], np.float32)).astype(np.float32)
    got2 = R.is_shadowed_device(pd, nd, light=L2).cpu().numpy()
    R.set_light_position(L2)
    exp2 = R.is_shadowed_device(pd, nd).cpu().numpy()
    assert np.array_equal(got2, exp2), f"{int((got2 != exp2).sum())} differ from the renderer lit from there"
    assert np.array_equal(exp2, _shadow_reference(R, oracle, p, nrm, L2))
    print(f"light case {name}, the light moved: {int(exp2.sum())} of {N} pairs shadowed")
    # compute_shadows off: is_shadowed returns false
    R.set_render_settings(st.copy(compute_shadows=False))
    assert not R.is_shadowed_device(pd, nd).cpu().numpy().any()


# ---- 6. is_shadowed_device, analytic shapes (known answers) ---------------------------------------------

@pytest.mark.parametrize("with_triangles", [False, True], ids=["shapes", "shapes_and_cube"])
def test_is_shadowed_analytic_shapes(R, with_triangles):
    """A plane y = 0 under a sphere of radius 1 at (0, 2, 0), lit from (0, 6, 0): the sphere's shadow on the
    plane is the disc of radius 6 tan(asin(1 / 4)) = 1.549.  Points within 0.5 of its centre are shadowed,
    points beyond 3 are lit; the ring between is left out."""
    base, st = scenes.sphere256()
    tri = np.zeros((0, 9), np.float32)
    if with_triangles:
        # the cube's triangles far from the light's rays: the whole-line BVH branch runs before the shapes
        tri = (scenes.cube1080(width=64, height=36)[0].tri.reshape(-1, 3) + np.array([40.0, 1.0, 0.0], np.float32))
        tri = tri.reshape(-1, 9).astype(np.float32)
    sc = dataclasses.replace(base, tri=tri, tri_mat=np.zeros(len(tri), np.int32), tri_uv=None,
                             shape_kind=np.array([1, 0], np.int32),
                             shape=np.array([[0, 0, 0, 0, 1, 0], [0, 2, 0, 1, 0, 0]], np.float32),
                             shape_mat=np.zeros(2, np.int32), light=np.array([0.0, 6.0, 0.0], np.float32))
    R.load_scene(sc, st.copy(compute_shadows=True))
    rng = np.random.default_rng(12)
    n = 4001
    rad = np.where(np.arange(n) % 2 == 0, rng.uniform(0.0, 0.5, n), rng.uniform(3.0, 8.0, n))
    az = rng.uniform(0, 2 * np.pi, n)
    p = np.stack([rad * np.cos(az), np.zeros(n), rad * np.sin(az)], 1).astype(np.float32)
    nrm = np.repeat(np.array([[0.0, 1.0, 0.0]], np.float32), n, 0)
    got = R.is_shadowed_device(gpu(p), gpu(nrm)).cpu().numpy()
    want = (np.hypot(p[:, 0], p[:, 2]) < 1.0).astype(np.uint8)
    assert want.sum() == (n + 1) // 2
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {n} known answers differ"


# ---- 7. stream order -----------------------------------------------------------------------------------

def test_stream_order(R, robot):
    """The rays are produced on a side stream behind long-running work and overwritten on it right after the
    call; a consumer on that stream reads the outputs; no host wait in between.  (This exercises the order; a
    race could still pass by luck.)"""
    sc, st, o, d, ref = robot
    R.load_scene(sc, st)
    R.trace_rays(o[:1], d[:1])   # (the scene is resident: the call below has nothing to build)
    oc, dc = gpu(o), gpu(d)
    a = torch.rand((2048, 2048), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = a
        for _ in range(24):
            b = (b @ a) * (1.0 / 2048)
        ot, dt = oc.clone(), dc.clone()
        out = R.trace_rays_device(ot, dt, stream=side)
        ot.fill_(float("nan"))
        dt.zero_()
        seen = {k: v.clone() for k, v in out.items()}
    side.synchronize()
    same(host(seen), ref, "the consumer on the side stream")
    # and with the current stream taken by default
    with torch.cuda.stream(side):
        ot2, dt2 = oc.clone(), dc.clone()
        out2 = R.trace_rays_device(ot2, dt2)
        ot2.zero_()
        seen2 = {k: v.clone() for k, v in out2.items()}
    side.synchronize()
    same(host(seen2), ref, "the current stream by default")
    torch.cuda.synchronize()
    del b


# ---- 8. scene changes wait -----------------------------------------------------------------------------

def test_scene_changes_and_close_wait_for_queries(make_renderer):
    n = 1 << 20
    rng = np.random.default_rng(3)
    scb, stb = scenes.bumpy70k(width=64, height=36)
    scr, str_ = scenes.robot1080(width=64, height=36)
    o, d = _random_rays(rng, n, np.array([0, 0, -3], np.float32), 2.0)
    od, dd = gpu(o), gpu(d)
    r = make_renderer()
    r.load_scene(scb, stb)
    before = host(r.trace_rays_device(od, dd))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = r.trace_rays_device(od, dd, stream=side)
    # no wait: the geometry is replaced and a frame rendered while the query may still run
    r.load_scene(scr, str_)
    got_frame = frame(r)
    side.synchronize()
    same(host(out), before, "the query in flight while the geometry was replaced")
    fresh = make_renderer()
    fresh.load_scene(scr, str_)
    assert_same_frame(got_frame, frame(fresh), "the robot's frame after the query")
    # close() right after a launch
    from raytracercpp_amd.renderer import Renderer
    r3 = Renderer(0)
    r3.load_scene(scb, stb)
    out3 = r3.trace_rays_device(od, dd, stream=side)
    sh3 = r3.is_shadowed_device(od, dd, stream=side)
    r3.close()
    side.synchronize()
    torch.cuda.synchronize()
    same(host(out3), before, "the query in flight at close()")
    assert sh3.shape == (n,)


# ---- 9. refusals ---------------------------------------------------------------------------------------

def _raw_trace(r, p, n):
    v = [C.c_void_p(x) for x in p]
    return _lib.lib().rt_trace_rays_device(r._h, v[0], v[1], n, v[2], v[3], v[4], v[5], v[6], v[7], None)


def test_refusals(R, robot):
    sc, st, o, d, ref = robot
    R.load_scene(sc, st)
    n = 64
    L = _lib.lib()
    good = [gpu(o[:n]), gpu(d[:n])] + [torch.full((n,), 77, dtype=dt, device="cuda") for dt in DTYPES] + \
           [torch.full((2,), 5, dtype=torch.int64, device="cuda")]
    host_arrays = [np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32),
                   np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8),
                   np.zeros(2, np.int64)]
    pinned = [torch.from_numpy(a.copy()).pin_memory() for a in host_arrays]
    before = R.device_ray_queries()

    def unchanged():
        torch.cuda.synchronize()
        assert R.device_ray_queries() == before
        assert all(bool((t == 77).all()) for t in good[2:7]) and bool((good[7] == 5).all())

    ptrs = [t.data_ptr() for t in good]
    for i in range(8):
        for what, bad in (("host", host_arrays[i].ctypes.data), ("pinned", pinned[i].data_ptr())):
            p = list(ptrs)
            p[i] = bad
            rc = _raw_trace(R, p, n)
            assert rc == -1, f"argument {i} in {what} memory: {rc}"   # RT_EINVAL
            unchanged()
    # a null pointer with n > 0 (the counts may be null)
    for i in range(7):
        p = list(ptrs)
        p[i] = None
        assert _raw_trace(R, p, n) == -1
    sh = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    sp = [ptrs[0], ptrs[1], sh.data_ptr()]
    sbad = [(host_arrays[0], pinned[0]), (host_arrays[1], pinned[1]), (host_arrays[6], pinned[6])]
    for i in range(3):
        for bad in (sbad[i][0].ctypes.data, sbad[i][1].data_ptr(), None):
            p = list(sp)
            p[i] = bad
            rc = L.rt_is_shadowed_device(R._h, C.c_void_p(p[0]), C.c_void_p(p[1]), n, None, C.c_void_p(p[2]), None)
            assert rc == -1, f"is_shadowed_device argument {i}: {rc}"
            unchanged()
            assert bool((sh == 77).all())
    # counts out of range, before anything is read or allocated
    for bad_n in ((1 << 30) + 1, -1, 1 << 40):
        assert _raw_trace(R, ptrs, bad_n) == -1
        assert L.rt_is_shadowed_device(R._h, C.c_void_p(sp[0]), C.c_void_p(sp[1]), bad_n, None, C.c_void_p(sp[2]), None) == -1
    unchanged()
    # the Python mirror refuses the same before any pointer is taken
    with pytest.raises(ValueError, match="not on a GPU"):
        R.trace_rays_device(pinned[0], pinned[1])
    with pytest.raises(ValueError, match="shape"):
        R.trace_rays_device(good[0], good[1], out={k: t[: n - 1] for k, t in zip(KEYS, good[2:7])})
    unchanged()
    # and the good arguments pass
    assert _raw_trace(R, ptrs, n) == 0
    same(host(dict(zip(KEYS, good[2:7]))), tuple(a[:n] for a in ref), "after the refusals")


def test_renderer_without_geometry(make_renderer, robot):
    """Before any geometry is set the call answers what trace_rays answers in that state."""
    sc, st, o, d, ref = robot
    r = make_renderer()
    want = r.trace_rays(o[:300], d[:300])
    got = dev(r, o[:300], d[:300])
    same(got, want, "no geometry")
    assert not got[4].any() and np.all(got[0] == -1)
    sh = r.is_shadowed_device(gpu(o[:300]), gpu(d[:300])).cpu().numpy()
    assert not sh.any()


def test_non_contiguous_views_are_refused(R, robot):
    """A [3, n] tensor transposed and a strided view have the right shape on the GPU too; read as they lie in
    memory they would be other rays, or outputs written between the caller's elements."""
    sc, st, o, d, ref = robot
    R.load_scene(sc, st)
    n = 64
    od, dd = gpu(o[:n]), gpu(d[:n])
    before = R.device_ray_queries()
    transposed = gpu(np.ascontiguousarray(o[:n].T)).t()
    strided = gpu(o[:2 * n])[::2]
    assert tuple(transposed.shape) == tuple(strided.shape) == (n, 3)
    for bad in (transposed, strided):
        with pytest.raises(ValueError, match="orig: the tensor is not contiguous"):
            R.trace_rays_device(bad, dd)
        with pytest.raises(ValueError, match="dirs: the tensor is not contiguous"):
            R.trace_rays_device(od, bad)
        with pytest.raises(ValueError, match="points: the tensor is not contiguous"):
            R.is_shadowed_device(bad, dd)
        with pytest.raises(ValueError, match="normals: the tensor is not contiguous"):
            R.is_shadowed_device(od, bad)
    for k, dt in zip(KEYS, DTYPES):
        out = {kk: torch.full((n,), 77, dtype=dd_, device="cuda") for kk, dd_ in zip(KEYS, DTYPES)}
        out[k] = torch.full((2 * n,), 77, dtype=dt, device="cuda")[::2]
        with pytest.raises(ValueError, match=f"{k}: the tensor is not contiguous"):
            R.trace_rays_device(od, dd, out=out)
        assert all(bool((t == 77).all()) for t in out.values())
    with pytest.raises(ValueError, match="out: the tensor is not contiguous"):
        R.is_shadowed_device(od, dd, out=torch.zeros(2 * n, dtype=torch.uint8, device="cuda")[::2])
    with pytest.raises(ValueError, match="counts: the tensor is not contiguous"):
        R.trace_rays_device(od, dd, counts=torch.zeros(4, dtype=torch.int64, device="cuda")[::2])
    assert R.device_ray_queries() == before
    # the same values in contiguous tensors pass
    same(host(R.trace_rays_device(transposed.contiguous(), dd)), tuple(a[:n] for a in ref), "contiguous copy")


def test_ray_index_past_2_31(R, robot):
    """n = 715,827,883 + 1,141 rays: from ray 715,827,883 on, 3 i does not fit 32 bits (a 32-bit index turns
    negative there and reads in front of the arrays).  The rays are one ray that leaves the scene behind it, answered
    at the root, except the last 2,048: the robot's rays, whose answers are known.  The inputs take 8.6 GB
    each and the outputs 12.2 GB."""
    sc, st, o, d, ref = robot
    R.load_scene(sc, st)
    tail = 2048
    n = 715_827_883 + 1141
    assert 3 * (n - tail) < 2 ** 31 < 3 * (n - tail + 1024)   # the tail straddles the first index past 2^31
    od = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    dd = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    od[:, 2] = 100.0
    dd[:, 2] = 1.0
    od[n - tail:] = gpu(o[:tail])
    dd[n - tail:] = gpu(d[:tail])
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = R.trace_rays_device(od, dd, counts=counts)
    got = tuple(out[k][n - tail:].cpu().numpy() for k in KEYS)
    same(got, tuple(a[:tail] for a in ref), "the rays around index 2^31 / 3")
    assert int(counts.sum()) == n
    head = R.trace_rays(np.array([[0, 0, 100]], np.float32), np.array([[0, 0, 1]], np.float32))
    assert head[4][0] == 0
    for k, a in zip(KEYS, head):
        assert bool((out[k][:n - tail].view(torch.uint8 if out[k].dtype == torch.uint8 else torch.int32) ==
                     torch.from_numpy(a).cuda().view(torch.uint8 if a.dtype == np.uint8 else torch.int32)).all()), k
    del out
    sh = R.is_shadowed_device(od, dd)
    want = R.is_shadowed_device(od[n - tail:].contiguous(), dd[n - tail:].contiguous())
    assert torch.equal(sh[n - tail:], want)
    assert torch.equal(sh[:n - tail], sh[:1].expand(n - tail))
    del sh, od, dd
    torch.cuda.empty_cache()
