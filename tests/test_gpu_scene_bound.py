"""The scene bound on the GPU (DESIGN.md 5.6 "The scene bound"; kernels.hip wide_closest): camera rays whose
line misses the widened box of the resident wide BVH's root are answered as misses without a node load.
Every frame (bumpy70k, at most 64 x 48 at ssaa_factor 2) is compared with the oracle bit for bit -- image,
hit id, hit t and shadow buffers: cameras that leave whole background tiles and tiles the bound's edge cuts,
a camera inside the bound, the camera moving between three frames in flight on three streams (a stale bound),
an object transform on the held quick tree and then the SAH tree (the wrong tree's bound), RT_SCENE_BOUND=0
against the default, and rt_wide_query's camera rays.  Reference path: Renderer::ray_trace
(renderer.cpp:1068-1116) through BVH::intersect (bvh.h:212-287)."""
import os

import numpy as np
import pytest

import tools.wbvh_probe as wp
from oracle.bindings import Oracle
from raytracercpp_amd import _lib, scenes
from raytracercpp_amd.scene import SceneData
from scene_bound_tool import scene_bound_check

pytestmark = pytest.mark.gpu

W, H = 64, 48


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


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


def _scene():
    return scenes.bumpy70k(width=W, height=H, enable_ssaa=True, ssaa_factor=2)


def _with_camera(sc, R, tri=None):
    sc2 = SceneData(**{**vars(sc), **({} if tri is None else {"tri": tri})})
    sc2.cam_pos, sc2.proj_inv, sc2.cam_to_world = R.get_camera_matrices()
    return sc2


def _frame(R):
    R.request_aux(hit=True, shadow=True)
    R.ray_trace()
    return R.get_internal(argb=True, hit=True, shadow=True)


def _assert_oracle(g, o, what):
    assert np.array_equal(g["hit_id"], o.hit_id), what
    assert np.array_equal(bits(g["hit_t"]), bits(o.hit_t)), what
    assert np.array_equal(g["shadow"], o.shadow), what
    assert np.array_equal(g["argb"], o.argb), what


def _rejected_tiles(sc2, st):
    """Per 8 x 8 tile of the internal image, how many of its primary rays the bound rejects (host checker)."""
    o, d = wp.camera_rays(sc2, st, 1)
    rej, res = scene_bound_check(sc2.tri, sc2.cam_pos, d)
    assert res["violations"] == 0
    rw, rh = st.render_size()
    t = rej.reshape(rh // 8, 8, rw // 8, 8).sum((1, 3))
    return t, res


CAMERAS = {
    "default": None,
    "back": ("translation", 0.5, 0.3, 1.5),
    "inside": ("translation", 1.2, 1.2, -1.9),   # inside the bound's box, outside the mesh
}


@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_frames_match_oracle(make_renderer, camera):
    sc, st = _scene()
    R = make_renderer()
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    if CAMERAS[camera]:
        R.set_camera_transform(_lib.make_transform(*CAMERAS[camera]))
    g = _frame(R)
    sc2 = _with_camera(sc, R)
    _assert_oracle(g, Oracle(sc2, st).render_rows(), camera)
    tiles, res = _rejected_tiles(sc2, st)
    print(f"{camera}: {res}; tiles wholly rejected {(tiles == 64).sum()}, cut {((tiles > 0) & (tiles < 64)).sum()} of {tiles.size}")
    assert res["valid"]
    if camera == "inside":
        assert res["rejected"] == 0
    else:   # whole background tiles, and tiles the bound's edge cuts through
        assert (tiles == 64).sum() > 0 and ((tiles > 0) & (tiles < 64)).sum() > 0


def test_moving_camera_three_frames_in_flight(make_renderer):
    """set_camera_transform before every launch, three launches in flight on three streams: each frame is
    the oracle's for its own camera (each launch carries its own bound)."""
    import torch
    sc, st = _scene()
    rw, rh = st.render_size()
    R = make_renderer()
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    streams = [torch.cuda.Stream("cuda:0") for _ in range(3)]
    outs = [torch.zeros((R.local_rows(8, 0, 1), W), dtype=torch.int32, device="cuda:0") for _ in range(3)]
    moves = [("translation", 0.9, 0.0, 1.0), ("translation", -0.9, 0.2, 0.5), ("ry", 14), ("translation", 0.0, -0.8, 1.5),
             ("rx", -11), ("translation", 0.4, 0.4, 0.0)]
    torch.cuda.synchronize()
    for base in (0, 3):
        cams = []
        for i in range(3):
            R.set_camera_transform(_lib.make_transform(*moves[base + i]))
            cams.append(_with_camera(sc, R))
            R.render_bands_device(8, 0, 1, outs[i].data_ptr(), streams[i].cuda_stream)
        torch.cuda.synchronize()
        for i in range(3):
            o = Oracle(cams[i], st).render_rows()
            exp = Oracle.downscale(o.argb, rw, rh, 2)
            got = outs[i].cpu().numpy().view(np.uint32)[:H].ravel()
            assert np.array_equal(got, exp), f"frame {base + i}: {int((got != exp).sum())} pixels differ"


def test_object_transform_on_the_quick_tree_then_the_sah_tree(make_renderer):
    """RT_ACCEL_HOLD=1: after set_object_transform the frames run on the quick tree of the moved mesh, after
    rt_finish_accel on its SAH tree; each tree's root gives its own bound."""
    sc, st = _scene()
    R = make_renderer(RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1)
    R.load_scene(sc, st)
    _assert_oracle(_frame(R), Oracle(sc, st).render_rows(), "first frame")
    m = _lib.compose(_lib.make_transform("translation", 1.4, 0.3, -1.0), _lib.make_transform("scale", 0.6, 0.6, 0.6))
    R.set_object_transform(m)
    tri = _lib.transform_points(m, sc.tri.reshape(-1, 3)).reshape(-1, 9)
    sc2 = _with_camera(sc, R, tri)
    o = Oracle(sc2, st).render_rows()
    _assert_oracle(_frame(R), o, "moved mesh, quick tree")
    assert R.stats()["wide_tree"] == 1
    _assert_oracle(_frame(R), o, "moved mesh, quick tree, second frame")
    R.finish_accel()
    _assert_oracle(_frame(R), o, "moved mesh, SAH tree")
    assert R.stats()["wide_tree"] == 2
    tiles, res = _rejected_tiles(sc2, st)
    assert res["valid"] and (tiles == 64).sum() > 0


def test_knob_off_gives_identical_buffers(make_renderer):
    sc, st = _scene()
    frames = []
    for env in ({}, {"RT_SCENE_BOUND": 0}):
        R = make_renderer(**env)
        R.load_scene(sc, st)
        R.ray_trace()
        R.finish_accel()
        R.set_camera_transform(_lib.make_transform(*CAMERAS["back"]))
        frames.append(_frame(R))
    a, b = frames
    for k in ("argb", "hit_id", "shadow"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(bits(a["hit_t"]), bits(b["hit_t"]))


def test_wide_query_rejected_camera_rays_are_misses(make_renderer):
    """rt_wide_query kind 1: status 0 for every camera ray the bound rejects; the others as without the bound."""
    sc, st = _scene()
    rng = np.random.default_rng(2)
    d = rng.standard_normal((20000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = np.repeat(np.asarray(sc.cam_pos, np.float32)[None], len(d), 0)
    rej, res = scene_bound_check(sc.tri, sc.cam_pos, d)
    assert res["valid"] and res["violations"] == 0 and res["rejected"] > 1000
    out = []
    for env in ({}, {"RT_SCENE_BOUND": 0}):
        R = make_renderer(**env)
        R.load_scene(sc, st)
        out.append(R.wide_query(o, d, 1))
    on, off = out
    assert (on["status"][rej == 1] == 0).all()
    assert np.array_equal(on["status"], off["status"])
    assert np.array_equal(on["id"], off["id"]) and np.array_equal(bits(on["t"]), bits(off["t"]))
