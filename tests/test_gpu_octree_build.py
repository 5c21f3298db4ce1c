"""The device octree build (octree_gpu.hip; rt_octree_build_device, rt_set_device_build) against the
host builds: the flattened nodes, triangle records and slot map byte for byte (the digest
rt_octree_digest computes) and the tree's statistics, then whole frames of a renderer built either way."""
import os

import numpy as np
import pytest

from golden_cases import Case
from raytracercpp_amd import _lib, scenes
from test_octree_build import CASES, soup  # noqa: F401  (the host build's cases)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_tree(tri, depth, leaf, builder=1):
    ref = _lib.octree_digest(tri, depth, leaf, builder=builder)
    got = _lib.octree_build_device(tri, depth, leaf)
    assert got[1] == ref[1]
    assert got[0] == ref[0], "the device-built arrays differ from the host's"
    return got


# ---- 1. digest parity --------------------------------------------------------------------------------

PARITY = list(CASES)
if not any(c[0] == "bumpy70k" for c in PARITY):
    PARITY.append(("bumpy70k", lambda: scenes.bumpy70k()[0].tri, 12, 40))
PARITY.append(("empty", lambda: np.zeros((0, 9), np.float32), 12, 40))


@pytest.mark.parametrize("name,make,depth,leaf", PARITY, ids=[c[0] for c in PARITY])
def test_device_build_equals_insertion_order_build(name, make, depth, leaf):
    assert_same_tree(make(), depth, leaf, builder=1)


# ---- 2. edge soup ------------------------------------------------------------------------------------

EDGE_N = (1, 2, 63, 64, 65, 257, 1025, 65537)
EDGE_PARAMS = ((12, 40), (12, 4), (3, 1), (0, 40), (5, 0), (12, -1))


def edge_soup(n, seed=20261019):
    """Signed zeros, centroids on cell planes, and a run of identical triangles (a max-depth leaf
    larger than any block beside seven empty siblings per level)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    flat = t.reshape(-1)
    i = np.arange(flat.size)
    five = i % 5 == 0
    flat[five & (i % 2 == 1)] = np.float32(0.0)
    flat[five & (i % 2 == 0)] = np.float32(-0.0)
    seven = ~five & (i % 7 == 0)
    flat[seven] = np.round(flat[seven] * 4) / 4
    t[:n // 4] = t[0]
    return t


_edge_cache = {}


def edge_case(n):
    if n not in _edge_cache:
        _edge_cache[n] = edge_soup(n)
    return _edge_cache[n]


@pytest.mark.parametrize("depth,leaf", EDGE_PARAMS, ids=[f"d{d}_l{l}" for d, l in EDGE_PARAMS])
@pytest.mark.parametrize("n", EDGE_N)
def test_edge_soup(n, depth, leaf):
    tri = edge_case(n)
    h0 = _lib.octree_digest(tri, depth, leaf, builder=0)
    h1 = _lib.octree_digest(tri, depth, leaf, builder=1)
    assert h0[0] == h1[0] and h0[1] == h1[1], "the two host builders disagree (a host finding)"
    got = _lib.octree_build_device(tri, depth, leaf)
    assert got[1] == h1[1]
    assert got[0] == h1[0]


# ---- 3. sphere1m -------------------------------------------------------------------------------------

def test_sphere1m_device_build():
    sc, _ = scenes.sphere1m()
    ref = _lib.octree_digest(sc.tri, 12, 40, builder=0)
    got = _lib.octree_build_device(sc.tri, 12, 40)
    print("sphere1m device build ms (HIP events, whole call):", got[2], "host build ms:", ref[2])
    assert got[1] == ref[1]
    assert got[0] == ref[0]


# ---- renderer ----------------------------------------------------------------------------------------

@pytest.fixture
def make_renderer():
    """Renderers created with switches in the environment (read once at rt_create), closed afterwards."""
    from raytracercpp_amd.renderer import Renderer
    made = []

    def make(**env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update({k: str(v) for k, v in env.items()})
        try:
            r = Renderer(0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def frame(r):
    r.request_aux(rgba=True, hit=True, shadow=True)
    r.ray_trace()
    return r.get_internal(argb=True, rgba=True, hit=True, shadow=True)


def assert_same_frame(a, b, what):
    assert np.array_equal(a["argb"], b["argb"]), what
    assert np.array_equal(bits(a["rgba"]), bits(b["rgba"])), what
    assert np.array_equal(a["hit_id"], b["hit_id"]), what
    assert np.array_equal(bits(a["hit_t"]), bits(b["hit_t"])), what
    assert np.array_equal(a["shadow"], b["shadow"]), what


def robot_small():
    sc, st = scenes.robot1080(width=64, height=36)
    return sc, st.copy(compute_shadows=True)


def cube_golden():
    c = Case("c2_cube")
    return c.scene, c.settings.copy(compute_shadows=True)


@pytest.mark.parametrize("scene", [robot_small, cube_golden], ids=["robot", "c2_cube"])
def test_renderer_same_frame(make_renderer, scene):
    """Mode off and on: the same frame on the quick tree (before rt_finish_accel) and on the SAH tree."""
    sc, st = scene()
    host = make_renderer(RT_ASYNC_ACCEL=1)
    dev = make_renderer(RT_ASYNC_ACCEL=1)
    dev.set_device_build(True)
    frames = {}
    for name, r in (("host", host), ("device", dev)):
        r.load_scene(sc, st)
        quick = frame(r)
        r.finish_accel()
        frames[name] = (quick, frame(r))
    assert_same_frame(frames["host"][0], frames["device"][0], "first frame")
    assert_same_frame(frames["host"][1], frames["device"][1], "frame after finish_accel")
    assert dev.device_builds() == 1 and dev.stats()["host_builds"] == 0
    assert host.device_builds() == 0 and host.stats()["host_builds"] == 1
    # the statistics the device build brought back are the host build's
    hs, ds = host.stats(), dev.stats()
    for k in ("octree_inner", "octree_leaves", "octree_empty_leaves", "octree_max_leaf", "octree_max_depth",
              "gpu_nodes", "gpu_tris"):
        assert hs[k] == ds[k], k


def test_renderer_env_switch(make_renderer):
    """RT_GPU_BUILD=1 at rt_create turns the mode on."""
    sc, st = robot_small()
    r = make_renderer(RT_GPU_BUILD=1)
    r.load_scene(sc, st)
    frame(r)
    assert r.device_builds() == 1 and r.stats()["host_builds"] == 0


def test_renderer_edits(make_renderer):
    """Three set_object_transform calls (each rebuilds the octree), a frame after each."""
    sc, st = robot_small()
    host = make_renderer()
    dev = make_renderer()
    dev.set_device_build(True)
    edits = [_lib.make_transform("ry", 25), _lib.make_transform("scale", 1.5, 0.75, 1.25),
             _lib.make_transform("translation", 1e3, 0.0, 0.0)]
    for r in (host, dev):
        r.load_scene(sc, st)
    assert_same_frame(frame(host), frame(dev), "before the edits")
    for k, m in enumerate(edits):
        host.set_object_transform(m)
        dev.set_object_transform(m)
        assert_same_frame(frame(host), frame(dev), f"edit {k}")
    assert dev.device_builds() == 4 and dev.stats()["host_builds"] == 0
    assert host.device_builds() == 0 and host.stats()["host_builds"] == 4


def test_renderer_set_devices(make_renderer):
    """Two renderers on one device: the helper copies the lead's device-built tables."""
    from raytracercpp_amd.renderer import render
    sc, st = robot_small()
    one = make_renderer()
    one.load_scene(sc, st)
    render(one)
    ref = one.get_image().ravel().copy()
    multi = make_renderer()
    multi.set_device_build(True)
    multi.load_scene(sc, st)
    multi.set_devices([0, 0])
    render(multi)
    assert np.array_equal(multi.get_image().ravel(), ref)
    assert multi.device_builds() == 1 and multi.stats()["host_builds"] == 0
    tri = (sc.tri * np.float32(0.9)).astype(np.float32)
    for r in (one, multi):
        r.set_triangles(tri, sc.tri_mat, sc.tri_uv)
        render(r)
    assert np.array_equal(multi.get_image().ravel(), one.get_image().ravel())
    assert multi.device_builds() == 2 and multi.stats()["host_builds"] == 0


def test_fallback_max_depth_31(make_renderer):
    """bvh_max_depth = 31 is outside the device builder's range: the host builds, the frame is the same."""
    sc, st = robot_small()
    st31 = st.copy(bvh_max_depth=31)
    host = make_renderer()
    host.load_scene(sc, st31)
    ref = frame(host)
    dev = make_renderer()
    dev.set_device_build(True)
    dev.load_scene(sc, st)
    frame(dev)
    assert dev.device_builds() == 1 and dev.stats()["host_builds"] == 0
    dev.set_render_settings(st31)
    assert_same_frame(frame(dev), ref, "max_depth 31")
    assert dev.device_builds() == 1 and dev.stats()["host_builds"] == 1
    with pytest.raises(_lib.RtError) as ei:
        _lib.octree_build_device(sc.tri, 31, 40)
    assert ei.value.code == -5   # RT_EUNSUPPORTED
