"""The tile mask on the GPU (kernels.hip wide_cut_kernel / wide_mask_kernel and the plain frame
kernel's masked tiles): a 64 x 32-segment UV sphere and the cube at 256 x 144, ssaa_factor 2.  Frames with the
mask against RT_TILE_MASK=0 and against the oracle, bit for bit (image, hit id, hit t, shadow): whole masked
tiles, partly covered tiles, the camera inside the bound, three frames in flight with the camera moving, band
layouts whose tiles straddle mask blocks, the held quick tree and the SAH tree after an object transform, the
non-fused SSAA and rgba paths; the device's mask against the host's, word for word.  Reference path:
Renderer::ray_trace (renderer.cpp:1068-1116) through BVH::intersect (bvh.h:212-287)."""
import os

import numpy as np
import pytest

from oracle.bindings import Oracle
from raytracercpp_amd import _lib, scenes
from raytracercpp_amd.scene import SceneData

pytestmark = pytest.mark.gpu

W, H = 256, 144


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


def _sphere(**kw):
    return scenes.uv_sphere_scene(64, 32, 1.0, 0.0, W, H, texcoords=False, enable_ssaa=True, ssaa_factor=2, **kw)


def _cube():
    return scenes.cube1080(width=W, height=H, enable_ssaa=True, ssaa_factor=2)


SCENES = {"sphere": _sphere, "cube": _cube}


def _with_camera(sc, R, tri=None):
    sc2 = SceneData(**{**vars(sc), **({} if tri is None else {"tri": tri})})
    sc2.cam_pos, sc2.proj_inv, sc2.cam_to_world = R.get_camera_matrices()
    return sc2


def _frame(R, rgba=False):
    R.request_aux(rgba=rgba, hit=True, shadow=True)
    R.ray_trace()
    return R.get_internal(argb=True, rgba=rgba, hit=True, shadow=True)


def _assert_same(a, b, what):
    for k in a:
        assert np.array_equal(bits(a[k]) if a[k].dtype == np.float32 else a[k], bits(b[k]) if b[k].dtype == np.float32 else b[k]), \
            f"{what}: {k}"


def _assert_oracle(g, o, what):
    assert np.array_equal(g["hit_id"], o.hit_id), what
    assert np.array_equal(bits(g["hit_t"]), bits(o.hit_t)), what
    assert np.array_equal(g["shadow"], o.shadow), what
    assert np.array_equal(g["argb"], o.argb), what


_ORACLE = {}


def _oracle(name, key, sc2, st):
    """The oracle's frame of a scene and camera, computed once and shared."""
    if (name, key) not in _ORACLE:
        _ORACLE[(name, key)] = Oracle(sc2, st).render_rows()
    return _ORACLE[(name, key)]


CAMERAS = {
    "default": None,                               # partly covered tiles around the object, masked ones beyond
    "far": ("translation", 0.5, 0.3, 4.0),         # most of the image is background
    "inside": ("translation", 0.85, 0.85, -2.15),  # inside the sphere's bounding box, outside the mesh
}


@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_frames_match_oracle_and_knob_off(make_renderer, scene, camera):
    sc, st = SCENES[scene]()
    frames, info = [], None
    for env in ({}, {"RT_TILE_MASK": 0}):
        R = make_renderer(**env)
        R.load_scene(sc, st)
        R.ray_trace()
        R.finish_accel()
        if CAMERAS[camera]:
            R.set_camera_transform(_lib.make_transform(*CAMERAS[camera]))
        frames.append(_frame(R, rgba=True))
        if not env:
            sc2 = _with_camera(sc, R)
            dev, info = R.tile_mask(0)
            host, _ = R.tile_mask(1)
            assert np.array_equal(dev, host), "device mask != host mask"
            # a clear block holds no hit
            rw, rh = st.render_size()
            hit = (frames[0]["hit_id"].reshape(rh // 8, 8, rw // 8, 8) >= 0).any((1, 3))
            assert not (hit & ~dev).any()
            print(f"{scene} / {camera}: mask {info}, {int((~dev).sum())} of {dev.size} blocks clear, {int(hit.sum())} hit")
            if scene == "sphere":
                assert info["on"] and info["cut"] > 4
                if camera == "far":
                    assert (~dev).sum() > dev.size // 2
                if camera == "default":
                    assert (~dev).any() and (dev & ~hit).any()
        else:
            _, off = R.tile_mask(0)
            assert not off["on"]
    _assert_same(frames[0], frames[1], f"{scene} / {camera}: mask on against off")
    _assert_oracle(frames[0], _oracle(scene, camera, sc2, st), f"{scene} / {camera}")


def test_tile_mask_before_a_frame_is_a_state_error(make_renderer):
    R = make_renderer()
    with pytest.raises(Exception):
        R.tile_mask(0)


def test_general_camera_has_no_mask(make_renderer):
    """A projection inverse whose w row depends on x (proj_mode 0) takes the general path: no mask, and the
    frame is the knob-off frame."""
    sc, st = _sphere()
    frames = []
    for env in ({}, {"RT_TILE_MASK": 0}):
        R = make_renderer(**env)
        R.load_scene(sc, st)
        R.ray_trace()
        R.finish_accel()
        pos, pinv, c2w = R.get_camera_matrices()
        pinv = pinv.copy()
        pinv[12] = np.float32(0.05)
        R.set_camera_matrices(pos, pinv, c2w)
        frames.append(_frame(R))
        cov, info = R.tile_mask(0)
        assert not info["on"] and cov.all()
    _assert_same(frames[0], frames[1], "general camera")


def test_moving_camera_three_frames_in_flight(make_renderer):
    """set_camera_transform before every launch, three launches in flight on three streams: each frame is the
    oracle's for its own camera (a launch waits for the launches that read the previous mask)."""
    import torch
    sc, st = _sphere()
    rw, rh = st.render_size()
    R = make_renderer()
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    streams = [torch.cuda.Stream("cuda:0") for _ in range(3)]
    outs = [torch.zeros((R.local_rows(8, 0, 1), W), dtype=torch.int32, device="cuda:0") for _ in range(3)]
    moves = [("translation", 0.9, 0.0, 1.0), ("translation", -0.9, 0.2, 2.5), ("ry", 14)]
    torch.cuda.synchronize()
    cams = []
    for i in range(3):
        R.set_camera_transform(_lib.make_transform(*moves[i]))
        cams.append(_with_camera(sc, R))
        R.render_bands_device(8, 0, 1, outs[i].data_ptr(), streams[i].cuda_stream)
    torch.cuda.synchronize()
    assert R.tile_mask(0)[1]["on"]
    for i in range(3):
        o = _oracle("sphere", ("move", i), cams[i], st)
        exp = Oracle.downscale(o.argb, rw, rh, 2)
        got = outs[i].cpu().numpy().view(np.uint32)[:H].ravel()
        assert np.array_equal(got, exp), f"frame {i}: {int((got != exp).sum())} pixels differ"


# (band rows, ranks): 8 output rows = 16 internal, whole tiles; 3 output rows = 6 internal: with three ranks a
# tile of 8 local rows holds rows of two bands, which lie in different mask blocks
LAYOUTS = [(8, 1), (8, 3), (3, 1), (3, 3)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"rows{l[0]}x{l[1]}ranks")
def test_band_layouts(make_renderer, layout):
    import torch
    br, nranks = layout
    sc, st = _sphere()
    rw, rh = st.render_size()
    R = make_renderer()
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    exp = Oracle.downscale(_oracle("sphere", "default", _with_camera(sc, R), st).argb, rw, rh, 2).reshape(H, W)
    nb = (H + br - 1) // br
    for rank in range(nranks):
        lrows = R.local_rows(br, rank, nranks)
        out = torch.zeros((lrows, W), dtype=torch.int32, device="cuda:0")
        R.render_bands_device(br, rank, nranks, out.data_ptr(), 0)
        torch.cuda.synchronize()
        assert R.tile_mask(0)[1]["on"]
        got = out.cpu().numpy().view(np.uint32)
        for i, b in enumerate(range(rank, nb, nranks)):
            rows = min(br, H - b * br)
            assert np.array_equal(got[i * br:i * br + rows], exp[b * br:b * br + rows]), f"rank {rank}, band {b}"
    if nranks == 3:   # a band list: the bands of rank 1 in reverse order
        bands = list(range(1, nb, nranks))[::-1]
        out = torch.zeros((len(bands) * br, W), dtype=torch.int32, device="cuda:0")
        R.render_band_list_device(br, bands, out.data_ptr(), 0)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        for i, b in enumerate(bands):
            rows = min(br, H - b * br)
            assert np.array_equal(got[i * br:i * br + rows], exp[b * br:b * br + rows]), f"band list, band {b}"


def test_object_transform_on_the_quick_tree_then_the_sah_tree(make_renderer):
    """RT_ACCEL_HOLD=1: after set_object_transform the frames run on the quick tree of the moved mesh, after
    rt_finish_accel on its SAH tree; each tree has its own cut and mask."""
    sc, st = _sphere()
    R = make_renderer(RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1)
    R.load_scene(sc, st)
    _assert_oracle(_frame(R), _oracle("sphere", "default", sc, st), "first frame")
    m = _lib.compose(_lib.make_transform("translation", 1.4, 0.3, -1.0), _lib.make_transform("scale", 0.6, 0.6, 0.6))
    R.set_object_transform(m)
    tri = _lib.transform_points(m, sc.tri.reshape(-1, 3)).reshape(-1, 9)
    o = _oracle("sphere", "moved", _with_camera(sc, R, tri), st)
    masks = []
    for what, tree in (("quick tree", 1), ("quick tree, second frame", 1), ("SAH tree", 2)):
        if tree == 2:
            R.finish_accel()
        _assert_oracle(_frame(R), o, "moved mesh, " + what)
        assert R.stats()["wide_tree"] == tree
        dev, info = R.tile_mask(0)
        host, _ = R.tile_mask(1)
        assert info["on"] and (~dev).any() and np.array_equal(dev, host), what
        masks.append((dev, info["cut"]))
    print("cut entries (quick, quick, SAH):", [m[1] for m in masks])


def test_non_fused_ssaa_matches(make_renderer):
    """RT_FUSED_SSAA=0: the masked tiles write the internal image and downscale_kernel filters it."""
    import torch
    sc, st = _sphere()
    rw, rh = st.render_size()
    R = make_renderer(RT_FUSED_SSAA=0)
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    exp = Oracle.downscale(_oracle("sphere", "default", _with_camera(sc, R), st).argb, rw, rh, 2)
    out = torch.zeros((R.local_rows(8, 0, 1), W), dtype=torch.int32, device="cuda:0")
    R.render_bands_device(8, 0, 1, out.data_ptr(), 0)
    torch.cuda.synchronize()
    assert R.tile_mask(0)[1]["on"]
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:H].ravel(), exp)
