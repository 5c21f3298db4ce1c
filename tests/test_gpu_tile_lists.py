"""The tile lists on the GPU (kernels.hip tile_class_kernel / tile_list_kernel, the plain frame
kernel's queue over 'covered' and its exit fill of 'clear'): the shapes of tests/test_gpu_tile_mask.py, a 64 x
32-segment UV sphere and the cube at 256 x 144, ssaa_factor 2.  Frames with lists against RT_TILE_LIST=0 and
against the oracle, bit for bit: rt_ray_trace with every auxiliary output (the generic fill), band launches with
fused SSAA (the packed fill) into poisoned buffers, band rows 8 and 3 at one and three ranks and a band list,
a camera that sees no geometry (the kernel only fills), one inside the bound (nothing to fill), three frames in
flight with the camera moving and nearly every heavy tile split (stale heavy and split lists), the non-fused
SSAA path and a general camera (no mask, no lists); the device's lists against the host's, word for word; a
cost above 0 for every on-image tile.  Reference path: Renderer::ray_trace (renderer.cpp:1068-1116)."""
import numpy as np
import pytest

from oracle.bindings import Oracle
from raytracercpp_amd import _lib
from test_gpu_tile_mask import (CAMERAS, H, LAYOUTS, SCENES, W, _assert_oracle, _assert_same, _frame, _oracle, _sphere,
                                _with_camera, make_renderer)  # noqa: F401  (make_renderer: a fixture)

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xDEADBEEF)


def _lists(R, on=True):
    """The last launch's device lists, checked against the host's recomputation and against each other."""
    cov, clr, info = R.tile_lists(0)
    assert info["on"] == on
    if not on:
        assert cov.size == 0 and clr.size == 0
        return cov, clr, info
    hcov, hclr, _ = R.tile_lists(1)
    assert np.array_equal(cov, hcov) and np.array_equal(clr, hclr), "device lists != host lists"
    ntiles = info["tiles_x"] * info["tiles_y"]
    both = np.concatenate([cov, clr])
    assert (np.diff(cov) > 0).all() and (np.diff(clr) > 0).all() and np.unique(both).size == both.size
    assert both.size <= ntiles and (both >= 0).all() and (both < ntiles).all()
    return cov, clr, info


def _costs_follow_the_lists(R, cov, clr, info):
    """tile_costs() > 0 exactly on the on-image tiles (the lists' union)."""
    c = R.tile_costs().ravel()
    assert c.size == info["tiles_x"] * info["tiles_y"]
    on = np.zeros(c.size, bool)
    on[cov] = True
    on[clr] = True
    assert (c[on] > 0).all(), f"{int((c[on] == 0).sum())} on-image tiles without a cost"
    assert (c[~on] == 0).all()


def _poisoned(rows):
    import torch
    return torch.full((rows, W), int(POISON.view(np.int32)), dtype=torch.int32, device="cuda:0")


@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_frames_match_oracle_and_knob_off(make_renderer, scene, camera):
    """rt_ray_trace with rgba, hit id, t and shadow requested: the exit fill goes through fill_masked_tile."""
    sc, st = SCENES[scene]()
    frames = []
    for env in ({}, {"RT_TILE_LIST": 0}):
        R = make_renderer(**env)
        R.load_scene(sc, st)
        # the warm-up frame under another camera: what it leaves in the internal buffers is not this frame's, so a
        # clear tile that nobody filled shows
        R.set_camera_transform(_lib.make_transform("translation", 0.7, -0.5, 1.5))
        R.ray_trace()
        R.finish_accel()
        R.set_camera_matrices(sc.cam_pos, sc.proj_inv, sc.cam_to_world)
        if CAMERAS[camera]:
            R.set_camera_transform(_lib.make_transform(*CAMERAS[camera]))
        frames.append(_frame(R, rgba=True))
        mask, minfo = R.tile_mask(0)
        if not env:
            sc2 = _with_camera(sc, R)
            cov, clr, info = _lists(R, on=minfo["on"])
            if minfo["on"]:
                # whole frame, 8-aligned size: a tile is a mask block
                assert np.array_equal(np.flatnonzero(mask.ravel()), cov) and np.array_equal(np.flatnonzero(~mask.ravel()), clr)
                _costs_follow_the_lists(R, cov, clr, info)
                print(f"{scene} / {camera}: {cov.size} covered, {clr.size} clear of {mask.size} tiles")
                if scene == "sphere" and camera == "far":
                    assert clr.size > mask.size // 2
                if mask.all():
                    assert clr.size == 0   # (the camera inside the bound: nothing to fill)
        else:
            _lists(R, on=False)
    _assert_same(frames[0], frames[1], f"{scene} / {camera}: lists on against off")
    _assert_oracle(frames[0], _oracle(scene, camera, sc2, st), f"{scene} / {camera}")


def test_camera_at_the_centre_has_nothing_to_fill(make_renderer):
    """A camera inside the bound: every block is covered and 'clear' is empty."""
    sc, st = _sphere()
    R = make_renderer()
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    pos, pinv, c2w = R.get_camera_matrices()
    c2w = np.array(c2w, np.float32).copy()
    p = sc.tri.reshape(-1, 3)
    centre = (0.5 * (p.min(0) + p.max(0))).astype(np.float32)
    c2w[[3, 7, 11]] = centre   # the translation column
    R.set_camera_matrices(centre, pinv, c2w)
    g = _frame(R)
    mask, minfo = R.tile_mask(0)
    cov, clr, info = _lists(R, on=minfo["on"])
    assert minfo["on"] and mask.all() and clr.size == 0 and cov.size == mask.size
    _assert_oracle(g, _oracle("sphere", "centre", _with_camera(sc, R), st), "camera at the centre")


def test_camera_turned_away_only_fills(make_renderer):
    """The camera pitched until the sphere has left the frustum: 'covered' is empty, the queue hands out
    nothing and the kernel only fills -- the whole frame and a band launch (the packed fill)."""
    import torch
    sc, st = _sphere()
    rw, rh = st.render_size()
    R = make_renderer()
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    # turned through 90 degrees the cut's boxes straddle the camera's plane and every block is set; the frustum is
    # narrower vertically, so the camera pitches: the first of these angles at which the mask is empty
    base = R.get_camera_matrices()
    chosen = None
    for move in (("rx", 65), ("rx", -65), ("rx", 58), ("rx", -58)):
        R.set_camera_matrices(*base)
        R.set_camera_transform(_lib.make_transform(*move))
        R.ray_trace()
        mask, minfo = R.tile_mask(0)
        print(f"{move}: mask on {minfo['on']}, {int(mask.sum())} of {mask.size} blocks set")
        if minfo["on"] and not mask.any():
            chosen = move
            break
    assert chosen is not None, "no camera with an empty mask"
    sc2 = _with_camera(sc, R)
    o = _oracle("sphere", chosen, sc2, st)
    assert (o.hit_id < 0).all()
    for _ in range(2):   # (the second launch has a heavy list from the first)
        g = _frame(R, rgba=True)
        cov, clr, info = _lists(R)
        assert cov.size == 0 and clr.size == info["tiles_x"] * info["tiles_y"]
        _costs_follow_the_lists(R, cov, clr, info)
        _assert_oracle(g, o, "turned away")
    exp = Oracle.downscale(o.argb, rw, rh, 2)
    for _ in range(2):
        out = _poisoned(R.local_rows(8, 0, 1))
        R.render_bands_device(8, 0, 1, out.data_ptr(), 0)
        torch.cuda.synchronize()
        cov, clr, info = _lists(R)
        assert cov.size == 0 and clr.size > 0
        got = out.cpu().numpy().view(np.uint32)[:H].ravel()
        assert not (got == POISON).any() and np.array_equal(got, exp)
        _costs_follow_the_lists(R, cov, clr, info)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"rows{l[0]}x{l[1]}ranks")
def test_band_layouts_into_poisoned_buffers(make_renderer, layout):
    """Band launches (8 output rows: fused SSAA, the packed fill; 3: the separate downscale) and a band list: no
    poisoned pixel survives in a band's rows, every band is the oracle's."""
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

    def check(out, bands, what):
        cov, clr, info = _lists(R)
        assert cov.size > 0 and clr.size > 0
        _costs_follow_the_lists(R, cov, clr, info)
        got = out.cpu().numpy().view(np.uint32)
        for i, b in enumerate(bands):
            rows = min(br, H - b * br)
            assert not (got[i * br:i * br + rows] == POISON).any(), f"{what}, band {b}: poisoned pixels"
            assert np.array_equal(got[i * br:i * br + rows], exp[b * br:b * br + rows]), f"{what}, band {b}"

    for rank in range(nranks):
        for launch in range(2):   # (the second: the same lists, and a heavy list)
            out = _poisoned(R.local_rows(br, rank, nranks))
            R.render_bands_device(br, rank, nranks, out.data_ptr(), 0)
            torch.cuda.synchronize()
            check(out, list(range(rank, nb, nranks)), f"rank {rank}, launch {launch}")
    if nranks == 3:   # band lists on the same stream: the layout changes, the mask does not
        for bands in (list(range(1, nb, nranks))[::-1], list(range(0, nb, 2))):
            out = _poisoned(len(bands) * br)
            R.render_band_list_device(br, bands, out.data_ptr(), 0)
            torch.cuda.synchronize()
            check(out, bands, "band list")


def test_moving_camera_three_in_flight_with_stale_heavy_and_split_lists(make_renderer):
    """Three launches in flight on three streams, the camera set before each, two rounds; RT_HEAVY_SPLIT=0.01
    splits nearly every heavy tile.  In the second round a stream's heavy and split lists come from its previous
    camera: they name tiles that are clear now (filled in the tile loop, skipped by the exit fill) and leave out
    tiles that are covered now.  Every frame is the oracle's for its own camera."""
    import torch
    sc, st = _sphere()
    rw, rh = st.render_size()
    R = make_renderer(RT_HEAVY_SPLIT=0.01)
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    streams = [torch.cuda.Stream("cuda:0") for _ in range(3)]
    moves = [("translation", 0.9, 0.0, 1.0), ("translation", -0.9, 0.2, 2.5), ("ry", 14)]
    torch.cuda.synchronize()
    # the cameras of tests/test_gpu_tile_mask.py's moving camera: each move is applied to the previous camera
    cams, outs = [], []
    for i in range(3):
        R.set_camera_transform(_lib.make_transform(*moves[i]))
        cams.append((_with_camera(sc, R), R.get_camera_matrices()))
        outs.append(_poisoned(R.local_rows(8, 0, 1)))
        R.render_bands_device(8, 0, 1, outs[-1].data_ptr(), streams[i].cuda_stream)
    # second round: stream i renders camera (i + 1) % 3
    outs2 = []
    for i in range(3):
        R.set_camera_matrices(*cams[(i + 1) % 3][1])
        outs2.append(_poisoned(R.local_rows(8, 0, 1)))
        R.render_bands_device(8, 0, 1, outs2[-1].data_ptr(), streams[i].cuda_stream)
    torch.cuda.synchronize()
    _lists(R)
    # what the second round's lists were stale about: each camera alone, its tile costs and clear tiles; a tile
    # that heavy_prep_kernel's bar (max(4 x mean, max / 8)) lists after camera i and that camera i + 1 leaves clear
    # was named by a stale heavy or split list and filled in the tile loop
    cost, clear = [], []
    for k in range(3):
        R.set_camera_matrices(*cams[k][1])
        out = _poisoned(R.local_rows(8, 0, 1))
        R.render_bands_device(8, 0, 1, out.data_ptr(), 0)
        torch.cuda.synchronize()
        cov, clr, info = _lists(R)
        c = R.tile_costs().ravel().astype(np.float64)
        cost.append(c)
        m = np.zeros(c.size, bool)
        m[clr] = True
        clear.append(m)
    stale = []
    for i in range(3):
        c = cost[i]
        listed = (c > 0) & (c >= max(4 * c.sum() / c.size, c.max() / 8))
        stale.append(int((listed & clear[(i + 1) % 3]).sum()))
    print("heavy tiles of a stream's previous camera that are clear under its next one:", stale)
    assert sum(stale) > 0
    for rnd, bufs in enumerate((outs, outs2)):
        for i in range(3):
            k = (i + rnd) % 3
            exp = Oracle.downscale(_oracle("sphere", ("move", k), cams[k][0], st).argb, rw, rh, 2)
            got = bufs[i].cpu().numpy().view(np.uint32)[:H].ravel()
            assert not (got == POISON).any(), f"round {rnd}, stream {i}: poisoned pixels"
            assert np.array_equal(got, exp), f"round {rnd}, stream {i}: {int((got != exp).sum())} pixels differ"


def test_fewer_covered_tiles_than_a_round_of_tickets(make_renderer):
    """The far camera in three ranks of 8-row bands: a launch has fewer covered tiles than the eight shards hand
    out in one round of batches (32); then one band at the sphere's edge: fewer covered tiles than shards, so
    some shards own one tile and some none."""
    import torch
    sc, st = _sphere()
    rw, rh = st.render_size()
    R = make_renderer()
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    R.set_camera_transform(_lib.make_transform(*CAMERAS["far"]))
    exp = Oracle.downscale(_oracle("sphere", "far", _with_camera(sc, R), st).argb, rw, rh, 2).reshape(H, W)
    nb, small = (H + 7) // 8, []
    for rank in range(3):
        out = _poisoned(R.local_rows(8, rank, 3))
        R.render_bands_device(8, rank, 3, out.data_ptr(), 0)
        torch.cuda.synchronize()
        cov, clr, info = _lists(R)
        small.append(cov.size)
        _costs_follow_the_lists(R, cov, clr, info)
        got = out.cpu().numpy().view(np.uint32)
        for i, b in enumerate(range(rank, nb, 3)):
            assert not (got[i * 8:i * 8 + 8] == POISON).any() and np.array_equal(got[i * 8:i * 8 + 8], exp[b * 8:b * 8 + 8]), \
                f"rank {rank}, band {b}"
    print("covered tiles per rank:", small)
    assert all(0 < n < 32 for n in small)
    # fewer covered tiles than shards: the far camera moved sideways until the image's edge cuts the covered square
    # (it is eight or nine tiles wide), one band of 4 output rows (one tile row) through it, as a band list
    edge = []
    for x in (2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5):
        R.set_camera_matrices(sc.cam_pos, sc.proj_inv, sc.cam_to_world)
        R.set_camera_transform(_lib.make_transform("translation", x, 0.3, 4.0))
        R.ray_trace()
        cov, clr, info = _lists(R, on=R.tile_mask(0)[1]["on"])
        per_band = np.bincount(cov // max(1, info["tiles_x"]), minlength=H // 4)
        edge = [b for b in range(H // 4) if 0 < per_band[b] < 8]
        print(f"x {x}: covered tiles per tile row of the whole frame:", per_band[per_band > 0])
        if edge:
            break
    assert edge, "no tile row with fewer than eight covered tiles"
    exp = Oracle.downscale(_oracle("sphere", ("far", x), _with_camera(sc, R), st).argb, rw, rh, 2).reshape(H, W)
    out = _poisoned(4)
    R.render_band_list_device(4, [edge[0]], out.data_ptr(), 0)
    torch.cuda.synchronize()
    cov, clr, info = _lists(R)
    assert cov.size == per_band[edge[0]] and clr.size == info["tiles_x"] * info["tiles_y"] - cov.size
    _costs_follow_the_lists(R, cov, clr, info)
    got = out.cpu().numpy().view(np.uint32)
    assert not (got == POISON).any() and np.array_equal(got, exp[edge[0] * 4:edge[0] * 4 + 4])


def test_non_fused_ssaa_matches(make_renderer):
    """RT_FUSED_SSAA=0: the exit fill writes the internal band and downscale_kernel filters it."""
    import torch
    sc, st = _sphere()
    rw, rh = st.render_size()
    R = make_renderer(RT_FUSED_SSAA=0)
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    exp = Oracle.downscale(_oracle("sphere", "default", _with_camera(sc, R), st).argb, rw, rh, 2)
    out = _poisoned(R.local_rows(8, 0, 1))
    R.render_bands_device(8, 0, 1, out.data_ptr(), 0)
    torch.cuda.synchronize()
    cov, clr, _ = _lists(R)
    assert cov.size > 0 and clr.size > 0
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:H].ravel(), exp)


def test_general_camera_has_no_mask_and_no_lists(make_renderer):
    sc, st = _sphere()
    frames = []
    for env in ({}, {"RT_TILE_LIST": 0}):
        R = make_renderer(**env)
        R.load_scene(sc, st)
        R.ray_trace()
        R.finish_accel()
        pos, pinv, c2w = R.get_camera_matrices()
        pinv = pinv.copy()
        pinv[12] = np.float32(0.05)
        R.set_camera_matrices(pos, pinv, c2w)
        frames.append(_frame(R))
        assert not R.tile_mask(0)[1]["on"]
        _lists(R, on=False)
    _assert_same(frames[0], frames[1], "general camera")


def test_tile_lists_before_a_frame_is_a_state_error(make_renderer):
    R = make_renderer()
    with pytest.raises(_lib.RtError):
        R.tile_lists(0)
