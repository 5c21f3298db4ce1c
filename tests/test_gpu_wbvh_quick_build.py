"""The quick wide BVH built on the device from the device-built octree (wbvh_quick_gpu.hip;
rt_wbvh_quick_build_device, rt_set_device_build) against the host's build_wbvh_quick: the same tree byte
for byte in every class that involves no transcendental (digests 0, 1, 2, 4, 5 and the statistics), the
cone code and sth at most one step apart, 0 structural violations; then renderers built either way, with
the SAH tree held back (RT_ACCEL_HOLD=1) so that frames and queries run on the quick tree."""
import os

import numpy as np
import pytest

from golden_cases import Case
from oracle.bindings import Oracle
from raytracercpp_amd import _lib, scenes
from test_gpu_octree_build import edge_soup
from test_octree_build import soup

pytestmark = pytest.mark.gpu

EXACT = (0, 1, 2, 4, 5)   # the digest classes without a transcendental


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_tree(tri, depth, leaf, what=""):
    ref = _lib.wbvh_quick_digest(tri, depth, leaf)
    dg, st, ck, ms = _lib.wbvh_quick_build_device(tri, depth, leaf)
    print(f"{what} n={len(tri)} ({depth}, {leaf}): {st}, check {ck}, ms {ms}")
    assert st == ref[1]
    for k in EXACT:
        assert dg[k] == ref[0][k], f"digest class {k} differs from the host tree's"
    assert ck["violations"] == 0
    assert ck["other_diff"] == 0
    assert ck["trans_max"] <= 1
    if ck["trans_diff"] == 0:
        assert dg[3] == ref[0][3]
    return dg, st, ck, ms


# ---- 1. structure: every branch of the planner ------------------------------------------------------

ONE = np.array([0.1, 0.2, -3.0, 1.1, 0.3, -3.2, 0.4, 1.5, -2.9], np.float32)


def copies(n):
    return np.repeat(ONE[None], n, 0)


@pytest.mark.parametrize("n", [1, 8, 9])
def test_root_leaf_runs(n):
    """A root leaf with one run, then two."""
    assert_same_tree(soup(7, n, 0), 12, 40, "root leaf")


@pytest.mark.parametrize("n", [40, 41])
def test_root_leaf_of_five_runs_then_the_first_split(n):
    assert_same_tree(soup(8, n, 0), 12, 40, "five runs / first split")


@pytest.mark.parametrize("n", [500, 2])
def test_max_depth_pile(n):
    """Copies of one triangle: a chain to the maximum depth, runs trees three deep."""
    _, st, _, _ = assert_same_tree(copies(n), 12, 40, "pile")
    if n == 500:
        assert st["leaves"] == 63


@pytest.mark.parametrize("depth,leaf", [(3, 1), (0, 40)])
def test_soup_shallow(depth, leaf):
    assert_same_tree(soup(2, 5000), depth, leaf, "soup")


def octant_soup(octants, heavy):
    """One small triangle per listed octant of [-1, 1]^3 (0 and 7 always among them: the root box is the
    cube), the triangles of the first 'heavy' octants repeated past the leaf size 3 (6 copies: a chain to a
    leaf child; 20: a runs tree)."""
    rows = []
    for i, o in enumerate(octants):
        c = np.array([0.5 if o & 1 else -0.5, 0.5 if o & 2 else -0.5, 0.5 if o & 4 else -0.5], np.float32)
        t = np.concatenate([c + np.float32([0.0, 0.0, 0.0]), c + np.float32([0.02, 0.0, 0.01]),
                            c + np.float32([0.0, 0.02, 0.01])]).astype(np.float32)
        if o == 0:
            t[0:3] = [-1.0, -1.0, -1.0]
            t[3:9] = [-0.98, -1.0, -0.99, -1.0, -0.98, -0.99]
        if o == 7:
            t[0:3] = [0.98, 1.0, 0.99]
            t[3:9] = [1.0, 0.98, 0.99, 1.0, 1.0, 1.0]
        rows += [t] * ((6, 20)[i % 2] if i < heavy else 1)
    return np.stack(rows)


@pytest.mark.parametrize("octants", [(0, 7, 1, 2), (0, 7, 1, 2, 4), (0, 7, 1, 2, 4, 5, 6), (0, 7, 1, 2, 3, 4, 5, 6)],
                         ids=["4", "5", "7", "8"])
@pytest.mark.parametrize("heavy", [0, 3])
def test_root_with_k_octants(octants, heavy):
    """No group, one group, one group of 4, two groups."""
    tri = octant_soup(octants, heavy)
    _, ost, _ = _lib.octree_digest(tri, 12, 3, builder=0)
    if heavy == 0:
        assert ost["inner"] == 1 and ost["leaves"] - ost["empty_leaves"] == len(octants)
    _, st, _, _ = assert_same_tree(tri, 12, 3, f"{len(octants)} octants")
    if heavy == 0:   # the root, its group nodes, and leaf children only
        assert st["nodes"] == 1 + (0, 0, 0, 0, 0, 1, 1, 1, 2)[len(octants)]
        assert st["leaves"] == len(octants)


def test_degenerate_triangles():
    """Zero area (nosth, s2 = 0), and a zero stored normal with non-zero edges (collinear vertices)."""
    t = soup(9, 300, 0).reshape(-1, 3, 3)
    t[0:40, 1] = t[0:40, 0]
    t[0:40, 2] = t[0:40, 0]                                   # a point
    t[40:80, 2] = t[40:80, 0] + 2 * (t[40:80, 1] - t[40:80, 0])   # collinear: edges, no normal
    t[80:90] = 0.0
    t[90:100] *= np.float32(1e-20)                            # normals below the cone's range
    assert_same_tree(t.reshape(-1, 9), 12, 40, "degenerate")
    assert_same_tree(t.reshape(-1, 9), 12, 4, "degenerate")


_edge_cache = {}


@pytest.mark.parametrize("depth,leaf", [(12, 40), (12, 4)], ids=["d12_l40", "d12_l4"])
@pytest.mark.parametrize("n", [63, 64, 65, 257, 1025, 65537])
def test_edge_soup(n, depth, leaf):
    if n not in _edge_cache:
        _edge_cache[n] = edge_soup(n)
    assert_same_tree(_edge_cache[n], depth, leaf, "edge soup")


def test_robot():
    assert_same_tree(scenes.robot1080()[0].tri, 12, 40, "robot")


def test_sphere1m():
    sc, _ = scenes.sphere1m()
    _, _, ck, ms = assert_same_tree(sc.tri, 12, 40, "sphere1m")
    print(f"sphere1m: device quick build {ms[0]:.2f} ms (HIP events), whole call {ms[1]:.1f} ms; "
          f"{ck['trans_diff']} transcendental bytes differ from the host's")


def test_empty_scene():
    dg, st, ck, _ = _lib.wbvh_quick_build_device(np.zeros((0, 9), np.float32), 12, 40)
    assert st == {"nodes": 0, "leaves": 0, "tris": 0, "max_leaf": 0, "depth": 0}
    assert ck == {"violations": 0, "trans_diff": 0, "trans_max": 0, "other_diff": 0}
    assert dg == _lib.wbvh_quick_digest(np.zeros((0, 9), np.float32), 12, 40)[0]


def test_depth_31_is_unsupported():
    with pytest.raises(_lib.RtError) as ei:
        _lib.wbvh_quick_build_device(soup(6, 50), 31, 40)
    assert ei.value.code == -5   # RT_EUNSUPPORTED


# ---- 2. renderers, the SAH tree held back ------------------------------------------------------------

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


HOLD = dict(RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1)


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


def pair(make_renderer, sc, st):
    host = make_renderer(**HOLD)
    dev = make_renderer(**HOLD)
    dev.set_device_build(True)
    for r in (host, dev):
        r.load_scene(sc, st)
    return host, dev


@pytest.mark.parametrize("scene", [robot_small, cube_golden], ids=["robot", "c2_cube"])
def test_frame_parity_on_the_held_quick_tree(make_renderer, scene):
    sc, st = scene()
    host, dev = pair(make_renderer, sc, st)
    fh, fd = frame(host), frame(dev)
    assert_same_frame(fh, fd, "first frame")
    assert host.stats()["wide_tree"] == 1 and dev.stats()["wide_tree"] == 1
    assert dev.device_wide_builds() == 1 and host.device_wide_builds() == 0
    assert dev.device_builds() == 1 and dev.stats()["host_builds"] == 0
    fh2, fd2 = frame(host), frame(dev)   # still held
    assert host.stats()["wide_tree"] == 1 and dev.stats()["wide_tree"] == 1
    assert_same_frame(fh2, fd2, "second frame")
    host.finish_accel()
    dev.finish_accel()
    fh3, fd3 = frame(host), frame(dev)
    assert host.stats()["wide_tree"] == 2 and dev.stats()["wide_tree"] == 2
    assert_same_frame(fh3, fd3, "frame after finish_accel")
    assert_same_frame(fh, fh3, "quick tree against SAH tree")


def robot_rays(sc, kind, rng, n=20000, ngraze=2000):
    """Random rays of the kind at the robot's triangles plus rays at the triangles most nearly edge-on to
    the kind's point (the camera's silhouette, the light's terminator)."""
    T = sc.tri.reshape(-1, 3, 3).astype(np.float64)
    P = np.asarray(sc.cam_pos if kind == 1 else sc.light, np.float64)
    nn = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    area = np.linalg.norm(nn, axis=1)
    nn /= np.maximum(area, 1e-30)[:, None]
    to = P - T.mean(1)
    to /= np.linalg.norm(to, axis=1, keepdims=True)
    key = np.where(area > 1e-12, np.abs((nn * to).sum(1)), np.inf)
    k = np.concatenate([rng.integers(0, len(T), n), rng.choice(np.argsort(key)[:max(ngraze, 1)], ngraze)])
    uv = rng.uniform(0, 1, (len(k), 2))
    uv[uv.sum(1) > 1] = 1 - uv[uv.sum(1) > 1]
    p = T[k, 0] + (T[k, 1] - T[k, 0]) * uv[:, :1] + (T[k, 2] - T[k, 0]) * uv[:, 1:]
    if kind == 1:
        d = p - P
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return np.repeat(P[None].astype(np.float32), len(k), 0), d.astype(np.float32)
    return p.astype(np.float32), nn[k].astype(np.float32)


@pytest.mark.parametrize("kind", [1, 2], ids=["camera", "shadow"])
def test_wide_queries_on_the_held_quick_tree(make_renderer, kind):
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st)
    o, d = robot_rays(sc, kind, np.random.default_rng(5 + kind))
    assert np.isfinite(o).all() and np.isfinite(d).all()
    gh, gd = host.wide_query(o, d, kind), dev.wide_query(o, d, kind)
    assert host.stats()["wide_tree"] == 1 and dev.stats()["wide_tree"] == 1
    assert dev.device_wide_builds() == 1
    assert np.array_equal(bits(gh["o"]), bits(gd["o"])) and np.array_equal(bits(gh["d"]), bits(gd["d"]))
    both = (gh["status"] != 2) & (gd["status"] != 2)
    print(f"kind {kind}: certified host {float((gh['status'] != 2).mean()):.4f}, device "
          f"{float((gd['status'] != 2).mean()):.4f}, statuses equal {float((gh['status'] == gd['status']).mean()):.4f}")
    assert both.mean() > 0.5
    assert np.array_equal(gh["status"][both], gd["status"][both])
    hit = both & (gh["status"] == 1)
    assert np.array_equal(gh["id"][hit], gd["id"][hit])
    assert np.array_equal(bits(gh["t"])[hit], bits(gd["t"])[hit])
    oi, ot, ou, ov, orr, _ = Oracle(sc, st).bvh_query(gh["o"], gh["d"])
    for r in (host, dev):
        ids, t, u, v, ret = r.trace_rays(gh["o"], gh["d"])
        assert np.array_equal(ret != 0, orr != 0)
        h = orr != 0
        assert np.array_equal(ids[h], oi[h])
        assert np.array_equal(bits(t)[h], bits(ot)[h])
        assert np.array_equal(bits(u)[h], bits(ou)[h]) and np.array_equal(bits(v)[h], bits(ov)[h])
    for g in (gh, gd):   # and every certified answer is the oracle's
        c = g["status"] != 2
        assert np.array_equal((g["status"] == 1)[c], (orr != 0)[c])
        hh = (g["status"] == 1) & (orr != 0)
        assert np.array_equal(g["id"][hh], oi[hh]) and np.array_equal(bits(g["t"])[hh], bits(ot)[hh])


def test_risk_words_on_the_device_built_tree(make_renderer):
    """rt_risk_words reads the tree on the host: the lazy download of the device-built one."""
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st)
    gw, gbad = dev.risk_words(0)
    hw, hbad = dev.risk_words(1)
    assert dev.stats()["wide_tree"] == 1 and dev.device_wide_builds() == 1
    assert gbad == 0 and hbad == 0
    rw, rbad = host.risk_words(1)
    assert rbad == 0 and rw.shape == hw.shape
    assert_same_frame(frame(host), frame(dev), "frame after the download")


def test_edits_under_hold(make_renderer):
    sc, st = robot_small()
    host, dev = pair(make_renderer, sc, st)
    edits = [_lib.make_transform("ry", 25), _lib.make_transform("scale", 1.5, 0.75, 1.25),
             _lib.make_transform("translation", 1e3, 0.0, 0.0)]
    assert_same_frame(frame(host), frame(dev), "before the edits")
    for k, m in enumerate(edits):
        host.set_object_transform(m)
        dev.set_object_transform(m)
        assert_same_frame(frame(host), frame(dev), f"edit {k}")
        assert dev.stats()["wide_tree"] == 1
    assert dev.device_wide_builds() == 4 and dev.device_builds() == 4 and dev.stats()["host_builds"] == 0
    assert host.device_wide_builds() == 0


def test_set_devices_copies_the_device_built_tree(make_renderer):
    from raytracercpp_amd.renderer import render
    sc, st = robot_small()
    one = make_renderer(**HOLD)
    one.load_scene(sc, st)
    render(one)
    ref = one.get_image().ravel().copy()
    multi = make_renderer(**HOLD)
    multi.set_device_build(True)
    multi.load_scene(sc, st)
    multi.set_devices([0, 0])
    render(multi)
    assert np.array_equal(multi.get_image().ravel(), ref)
    assert multi.device_wide_builds() == 1 and multi.stats()["wide_tree"] == 1


def test_fallback_max_depth_31(make_renderer):
    sc, st = robot_small()
    st31 = st.copy(bvh_max_depth=31)
    host = make_renderer(**HOLD)
    host.load_scene(sc, st31)
    ref = frame(host)
    dev = make_renderer(**HOLD)
    dev.set_device_build(True)
    dev.load_scene(sc, st)
    frame(dev)
    assert dev.device_wide_builds() == 1
    dev.set_render_settings(st31)
    assert_same_frame(frame(dev), ref, "max_depth 31")
    assert dev.device_wide_builds() == 1 and dev.device_builds() == 1 and dev.stats()["host_builds"] == 1
    assert dev.stats()["wide_tree"] == 1


def test_without_the_hold_knob_frames_adopt_the_sah_tree(make_renderer):
    sc, st = robot_small()
    r = make_renderer(RT_ASYNC_ACCEL=1)
    r.set_device_build(True)
    r.load_scene(sc, st)
    first = frame(r)
    assert r.stats()["wide_tree"] in (1, 2)
    r.finish_accel()
    assert_same_frame(first, frame(r), "after finish_accel")
    assert r.stats()["wide_tree"] == 2
    assert r.device_wide_builds() == 1
