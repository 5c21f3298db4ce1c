"""Entry nodes on the GPU (kernels.hip wide_entry_kernel and the plain frame kernel's primary
queries started at their blocks' entry sets): the shapes of tests/test_gpu_tile_mask.py, a 64 x 32-segment UV
sphere and the cube at 256 x 144, ssaa_factor 2.  A stream computes its entry sets at its second launch in a row
with the same camera and tree.  Frames with entry sets against RT_TILE_START=0, against the camera's first
frame and against the oracle, bit for bit (image, rgba, hit id, hit t, shadow); the device's entry sets against the host's, word for
word; band layouts whose tiles straddle blocks; three frames in flight with the camera moving; the held quick
tree, then the SAH tree after an object transform; split tiles (trace_split_part); a general camera (no mask, no
entry sets).  Reference path: Renderer::ray_trace (renderer.cpp:1068-1116) through BVH::intersect
(bvh.h:212-287)."""
import numpy as np
import pytest

from oracle.bindings import Oracle
from raytracercpp_amd import _lib
from test_gpu_frames import _heavy_tiles
from test_gpu_tile_mask import (CAMERAS, H, LAYOUTS, SCENES, W, _assert_oracle, _assert_same, _frame, _oracle, _sphere,
                                _with_camera, make_renderer)  # noqa: F401  (make_renderer: the fixture)

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF


def _sets_checked(R, what, expect_below_root):
    """The launch's entry sets, device against host; (sets, blocks that start below the root)."""
    dev, on = R.tile_starts(0)
    host, _ = R.tile_starts(1)
    assert on, what
    assert np.array_equal(dev, host), f"{what}: device entry sets != host entry sets"
    cov, _ = R.tile_mask(0)
    below = dev[:, :, 0] != 0
    # a clear block keeps the root; a set is packed to the front, its links are inner nodes
    assert not (below & ~cov).any(), what
    used = dev != EMPTY
    assert used[:, :, 0].all() and (used[:, :, :-1] >= used[:, :, 1:]).all(), what
    assert (dev[used] < 0x80000000).all(), what
    if expect_below_root:
        assert below.any(), what
    return dev, below


@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_frames_match_oracle_and_knob_off(make_renderer, scene, camera):
    sc, st = SCENES[scene]()
    frames = []
    for env in ({}, {"RT_TILE_START": 0}):
        R = make_renderer(**env)
        R.load_scene(sc, st)
        R.ray_trace()
        R.finish_accel()
        if CAMERAS[camera]:
            R.set_camera_transform(_lib.make_transform(*CAMERAS[camera]))
            # a stream's first launch with a new camera computes its mask only; the entry sets come with the second
            first = _frame(R, rgba=True)
            assert not R.tile_starts(0)[1]
        frames.append(_frame(R, rgba=True))
        if CAMERAS[camera]:
            _assert_same(first, frames[-1], f"{scene} / {camera}: the camera's first frame against its second")
        if not env:
            sc2 = _with_camera(sc, R)
            dev, below = _sets_checked(R, f"{scene} / {camera}", scene == "sphere" and camera != "inside")
            nl = (dev != EMPTY).sum(2)
            print(f"{scene} / {camera}: {int(below.sum())} of {below.size} blocks start below the root; links per such "
                  f"block 1/2/3/4: {[int(((nl == k) & below).sum()) for k in (1, 2, 3, 4)]}")
        else:
            dev, on = R.tile_starts(0)
            assert not on and (dev[:, :, 0] == 0).all() and (dev[:, :, 1:] == EMPTY).all()
    _assert_same(frames[0], frames[1], f"{scene} / {camera}: entry sets on against off")
    _assert_oracle(frames[0], _oracle(scene, camera, sc2, st), f"{scene} / {camera}")


def test_tile_starts_before_a_frame_is_a_state_error(make_renderer):
    R = make_renderer()
    with pytest.raises(Exception):
        R.tile_starts(0)


def test_general_camera_has_no_entry_sets(make_renderer):
    """A projection inverse whose w row depends on x (proj_mode 0): no mask, no entry sets, the knob-off frame."""
    sc, st = _sphere()
    frames = []
    for env in ({}, {"RT_TILE_START": 0}):
        R = make_renderer(**env)
        R.load_scene(sc, st)
        R.ray_trace()
        R.finish_accel()
        pos, pinv, c2w = R.get_camera_matrices()
        pinv = pinv.copy()
        pinv[12] = np.float32(0.05)
        R.set_camera_matrices(pos, pinv, c2w)
        frames.append(_frame(R))
        dev, on = R.tile_starts(0)
        assert not on and (dev[:, :, 0] == 0).all() and (dev[:, :, 1:] == EMPTY).all()
    _assert_same(frames[0], frames[1], "general camera")


def test_moving_camera_three_frames_in_flight(make_renderer):
    """set_camera_transform before every launch, three launches in flight on three streams: a camera that moves
    every launch gets no entry sets.  Then the camera rests while each stream launches twice more, the second
    time from the entry sets in its own buffer.  Each frame is the oracle's for its camera."""
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
    assert not R.tile_starts(0)[1] and R.tile_mask(0)[1]["on"]
    for i in range(3):
        o = _oracle("sphere", ("move", i), cams[i], st)
        exp = Oracle.downscale(o.argb, rw, rh, 2)
        got = outs[i].cpu().numpy().view(np.uint32)[:H].ravel()
        assert np.array_equal(got, exp), f"frame {i}: {int((got != exp).sum())} pixels differ"
    # the camera at rest (the last one): stream 2 has seen it once, streams 0 and 1 not yet
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


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"rows{l[0]}x{l[1]}ranks")
def test_band_layouts(make_renderer, layout):
    """Band rows 3: a tile of 8 local rows holds rows of two blocks; each lane reads its own block's set."""
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
    for n, rank in enumerate(list(range(nranks)) * 2):   # (the stream's first band launch computes its mask only)
        lrows = R.local_rows(br, rank, nranks)
        out = torch.zeros((lrows, W), dtype=torch.int32, device="cuda:0")
        R.render_bands_device(br, rank, nranks, out.data_ptr(), 0)
        torch.cuda.synchronize()
        assert R.tile_starts(0)[1] == (n > 0)
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
    rt_finish_accel on its SAH tree; each tree has its own entry sets (node links of the old tree would name
    other nodes: the sets are recomputed with the cut)."""
    sc, st = _sphere()
    R = make_renderer(RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1)
    R.load_scene(sc, st)
    _assert_oracle(_frame(R), _oracle("sphere", "default", sc, st), "first frame")
    m = _lib.compose(_lib.make_transform("translation", 1.4, 0.3, -1.0), _lib.make_transform("scale", 0.6, 0.6, 0.6))
    R.set_object_transform(m)
    tri = _lib.transform_points(m, sc.tri.reshape(-1, 3)).reshape(-1, 9)
    o = _oracle("sphere", "moved", _with_camera(sc, R, tri), st)
    sets = {}
    for what, tree in (("quick tree", 1), ("quick tree, second frame", 1), ("quick tree, third frame", 1), ("SAH tree", 2),
                       ("SAH tree, second frame", 2)):
        if what == "SAH tree":
            R.finish_accel()
        _assert_oracle(_frame(R), o, "moved mesh, " + what)
        assert R.stats()["wide_tree"] == tree
        if "frame" in what:
            sets[what] = _sets_checked(R, what, True)[0]
        else:   # a new tree: a new cut and mask, no entry sets yet (the old tree's links name other nodes)
            assert not R.tile_starts(0)[1], what
    assert np.array_equal(sets["quick tree, second frame"], sets["quick tree, third frame"])
    assert not np.array_equal(sets["quick tree, third frame"], sets["SAH tree, second frame"])


def test_split_tiles_start_at_their_entry_sets(make_renderer):
    """A second frame of the same view with a low RT_HEAVY_SPLIT: heavy_prep_kernel splits the costliest tiles
    into parts, whose lane groups start at the entry sets (group lane 0 holds the links)."""
    sc, st = _sphere()
    frames = []
    for env in ({}, {"RT_TILE_START": 0}):
        R = make_renderer(RT_HEAVY_SPLIT=0.01, **env)
        R.load_scene(sc, st)
        R.ray_trace()
        R.finish_accel()
        _frame(R, rgba=True)
        c = R.tile_costs()
        nsplit = _heavy_tiles(c, nwaves=c.size, split=0.01)
        assert nsplit > 0, "no tile would be split"
        frames.append(_frame(R, rgba=True))
        if not env:
            _sets_checked(R, "split frame", True)
    print("split tiles:", nsplit)
    _assert_same(frames[0], frames[1], "split tiles: entry sets on against off")
    _assert_oracle(frames[0], _oracle("sphere", "default", sc, st), "split tiles")
