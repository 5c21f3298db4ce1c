"""The entry search's back-face test on the GPU (wbvh.hpp wbvh_entry_backfacing through kernels.hip
wide_entry_kernel): tests/test_gpu_tile_starts.py's shapes, a 64 x 32-segment UV sphere and the cube at 256 x 144,
ssaa_factor 2.  The device's sets against the host's, word for word, with the test on; frames with it on against
RT_ENTRY_CULL=0, against the camera's first frame (no sets yet) and against the oracle, bit for bit (image, rgba,
hit id, hit t, shadow); a camera inside the sphere; split tiles; three frames in flight with the camera moving and
then at rest; the held quick tree, then the SAH tree after an object transform.  Reference path:
Renderer::ray_trace (renderer.cpp:1068-1116) through BVH::intersect (bvh.h:212-287)."""
import numpy as np
import pytest

from oracle.bindings import Oracle
from raytracercpp_amd import _lib
from test_gpu_frames import _heavy_tiles
from test_gpu_tile_mask import (CAMERAS, H, SCENES, W, _assert_oracle, _assert_same, _frame, _oracle, _sphere,
                                _with_camera, make_renderer)  # noqa: F401  (make_renderer: the fixture)
from test_gpu_tile_starts import EMPTY, _sets_checked

pytestmark = pytest.mark.gpu


def _second_frame(R, camera, what):
    """The camera's second frame (its first computes the mask only), checked against the first."""
    if camera is not None:
        R.set_camera_transform(_lib.make_transform(*camera))
    first = _frame(R, rgba=True)
    second = _frame(R, rgba=True)
    _assert_same(first, second, f"{what}: the camera's first frame against its second")
    return second


@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_frames_match_oracle_and_cull_off(make_renderer, scene, camera):
    sc, st = SCENES[scene]()
    frames, sets = [], []
    for env in ({}, {"RT_ENTRY_CULL": 0}):
        R = make_renderer(**env)
        R.load_scene(sc, st)
        R.ray_trace()
        R.finish_accel()
        frames.append(_second_frame(R, CAMERAS[camera], f"{scene} / {camera} / {env}"))
        sc2 = _with_camera(sc, R)
        # (the host's sets are computed with the launch's own camera, its switch included)
        sets.append(_sets_checked(R, f"{scene} / {camera} / {env}", scene == "sphere" and camera != "inside")[0])
    changed = int((sets[0] != sets[1]).any(2).sum())
    nl = [(s != EMPTY).sum(2)[s[:, :, 0] != 0] for s in sets]
    print(f"{scene} / {camera}: {changed} blocks' sets change with the test; blocks below the root {len(nl[0])} (off: "
          f"{len(nl[1])}), links per such block {nl[0].mean() if len(nl[0]) else 0:.2f} (off: {nl[1].mean() if len(nl[1]) else 0:.2f})")
    if scene == "sphere" and camera == "default":
        assert changed > 0   # (the test does change sets here)
    _assert_same(frames[0], frames[1], f"{scene} / {camera}: the back-face test on against off")
    _assert_oracle(frames[0], _oracle(scene, camera, sc2, st), f"{scene} / {camera}")


def test_camera_inside_the_sphere(make_renderer):
    """The camera at the sphere's centre: every triangle faces away from every ray, so the search drops every child
    it examines that has a cone (the blocks' sets are printed: the children without one keep them below the root).
    No pixel is hit, and the frame is the oracle's."""
    sc, st = _sphere()
    centre = sc.tri.reshape(-1, 3).astype(np.float64).mean(0).astype(np.float32)
    frames = []
    for env in ({}, {"RT_ENTRY_CULL": 0}):
        R = make_renderer(**env)
        R.load_scene(sc, st)
        R.ray_trace()
        R.finish_accel()
        pos, pinv, c2w = R.get_camera_matrices()
        c2w = c2w.copy()
        c2w[3], c2w[7], c2w[11] = centre
        R.set_camera_matrices(centre.copy(), pinv, c2w)
        _frame(R, rgba=True)
        frames.append(_frame(R, rgba=True))
        sc2 = _with_camera(sc, R)
        dev, below = _sets_checked(R, f"inside the sphere / {env}", False)
        print(f"inside the sphere / {env}: {int(below.sum())} of {below.size} blocks start below the root")
    _assert_same(frames[0], frames[1], "inside the sphere: the back-face test on against off")
    assert (frames[0]["hit_id"] < 0).all()
    _assert_oracle(frames[0], _oracle("sphere", "centre", sc2, st), "inside the sphere")


def test_split_tiles(make_renderer):
    """A low RT_HEAVY_SPLIT: the costliest tiles are split into parts whose lane groups start at the culled sets."""
    sc, st = _sphere()
    frames = []
    for env in ({}, {"RT_ENTRY_CULL": 0}):
        R = make_renderer(RT_HEAVY_SPLIT=0.01, **env)
        R.load_scene(sc, st)
        R.ray_trace()
        R.finish_accel()
        _frame(R, rgba=True)
        c = R.tile_costs()
        assert _heavy_tiles(c, nwaves=c.size, split=0.01) > 0, "no tile would be split"
        frames.append(_frame(R, rgba=True))
        _sets_checked(R, f"split frame / {env}", True)
    _assert_same(frames[0], frames[1], "split tiles: the back-face test on against off")
    _assert_oracle(frames[0], _oracle("sphere", "default", sc, st), "split tiles")


def test_moving_camera_then_at_rest_three_frames_in_flight(make_renderer):
    """Three launches in flight on three streams with a camera that moves before each (no sets), then the camera at
    rest while each stream launches twice more, the second time from the culled sets in its own buffer."""
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
    assert not R.tile_starts(0)[1]
    for i in range(3):
        exp = Oracle.downscale(_oracle("sphere", ("move", i), cams[i], st).argb, rw, rh, 2)
        got = outs[i].cpu().numpy().view(np.uint32)[:H].ravel()
        assert np.array_equal(got, exp), f"frame {i}: {int((got != exp).sum())} pixels differ"
    exp = Oracle.downscale(_oracle("sphere", ("move", 2), cams[2], st).argb, rw, rh, 2)
    for rnd in range(2):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        for i in range(3):
            R.render_bands_device(8, 0, 1, outs[i].data_ptr(), streams[i].cuda_stream)
        torch.cuda.synchronize()
        for i in range(3):
            got = outs[i].cpu().numpy().view(np.uint32)[:H].ravel()
            assert np.array_equal(got, exp), f"camera at rest, round {rnd}, stream {i}"
    _sets_checked(R, "the last launch of the camera at rest", True)


def test_object_transform_on_the_quick_tree_then_the_sah_tree(make_renderer):
    """RT_ACCEL_HOLD=1: the moved mesh's quick tree, then its SAH tree, each with its own culled sets; the frames
    are the oracle's and the same with RT_ENTRY_CULL=0."""
    sc, st = _sphere()
    m = _lib.compose(_lib.make_transform("translation", 1.4, 0.3, -1.0), _lib.make_transform("scale", 0.6, 0.6, 0.6))
    tri = _lib.transform_points(m, sc.tri.reshape(-1, 3)).reshape(-1, 9)
    frames = {}
    for env in ({}, {"RT_ENTRY_CULL": 0}):
        R = make_renderer(RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1, **env)
        R.load_scene(sc, st)
        _frame(R)
        R.set_object_transform(m)
        o = _oracle("sphere", "moved", _with_camera(sc, R, tri), st)
        for what, tree in (("quick tree", 1), ("quick tree, second frame", 1), ("SAH tree", 2), ("SAH tree, second frame", 2)):
            if what == "SAH tree":
                R.finish_accel()
            g = _frame(R)
            _assert_oracle(g, o, f"moved mesh, {what} / {env}")
            assert R.stats()["wide_tree"] == tree
            if "frame" in what:
                sets = _sets_checked(R, f"{what} / {env}", True)[0]
                if env:
                    _assert_same(g, frames[what][0], f"{what}: the back-face test on against off")
                else:
                    frames[what] = (g, sets)
            else:
                assert not R.tile_starts(0)[1], what
