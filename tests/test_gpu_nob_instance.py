"""The wide query's instance without case (b) in the frame kernels (kernels.hip wide_run's NOBF):
a wave whose active lanes all skip case (b) runs wbvh_closest<.., NOB = true>, every other wave the general instance.
A 64 x 32-segment UV sphere at 128 x 72, ssaa_factor 2: the tiles inside the silhouette are all-nob, the tiles on it
mixed (tests/test_nob_instance.py prints the host's figures for such views).  Frames against the oracle and against
the exact octree mode, bit for bit (image, rgba, hit id, hit t, shadow): the default camera; the camera at the
sphere's centre; a mesh whose at-risk set holds a degenerate record, so that the camera has no cap; split tiles
(lane groups); band rows 8 and 3 at one and three ranks; three frames in flight with the camera moving, then at rest.
Reference path: Renderer::ray_trace (renderer.cpp:1068-1116) through BVH::intersect (bvh.h:212-287)."""
import numpy as np
import pytest

from oracle.bindings import Oracle
from raytracercpp_amd import _lib, scenes
from raytracercpp_amd.scene import SceneData
from test_gpu_frames import _heavy_tiles
from test_gpu_tile_mask import _assert_oracle, _assert_same, _frame, _oracle, _with_camera, make_renderer  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 128, 72


def _sphere():
    return scenes.uv_sphere_scene(64, 32, 1.0, 0.0, W, H, texcoords=False, enable_ssaa=True, ssaa_factor=2)


def _wide_and_exact(R, what):
    """The camera's first and second frame on the wide BVH (the second starts at the blocks' entry sets) and the
    frame of the exact octree mode, which must be the same; the wide frame."""
    first = _frame(R, rgba=True)
    second = _frame(R, rgba=True)
    _assert_same(first, second, f"{what}: the camera's first frame against its second")
    R.set_exact(True)
    exact = _frame(R, rgba=True)
    R.set_exact(False)
    _assert_same(second, exact, f"{what}: the wide BVH against the exact octree mode")
    return second


def _ready(make_renderer, sc, st, **env):
    R = make_renderer(**env)
    R.load_scene(sc, st)
    R.ray_trace()
    R.finish_accel()
    return R


def test_sphere_frames_match_oracle_and_exact_mode(make_renderer):
    sc, st = _sphere()
    R = _ready(make_renderer, sc, st)
    g = _wide_and_exact(R, "sphere")
    hit = g["hit_id"] >= 0
    print(f"sphere: {int(hit.sum())} of {hit.size} rays hit, {int(g['shadow'].sum())} shadowed")
    # (the silhouette crosses the image: 8 x 8 tiles wholly inside it, tiles on it and tiles outside)
    tiles = hit.reshape(2 * H // 8, 8, 2 * W // 8, 8)
    assert tiles.all((1, 3)).any() and (tiles.any((1, 3)) & ~tiles.all((1, 3))).any() and g["shadow"].any()
    _assert_oracle(g, _oracle("nob_sphere", "default", _with_camera(sc, R), st), "sphere")


def test_camera_at_the_sphere_centre(make_renderer):
    sc, st = _sphere()
    R = _ready(make_renderer, sc, st)
    centre = sc.tri.reshape(-1, 3).astype(np.float64).mean(0).astype(np.float32)
    pos, pinv, c2w = R.get_camera_matrices()
    c2w = c2w.copy()
    c2w[3], c2w[7], c2w[11] = centre
    R.set_camera_matrices(centre.copy(), pinv, c2w)
    g = _wide_and_exact(R, "the camera at the centre")
    assert (g["hit_id"] < 0).all()
    _assert_oracle(g, _oracle("nob_sphere", "centre", _with_camera(sc, R), st), "the camera at the centre")


def test_a_degenerate_record_at_risk_leaves_no_cap(make_renderer):
    """The sphere with a zero-area triangle and a sliver on its surface towards the camera: the degenerate record is
    at risk for every origin and bounds no cap (wbvh.hpp risk_cap_tri: 0), so no camera ray skips case (b) while the
    shadow rays still may (the origin cones)."""
    sc, st = _sphere()
    p = sc.tri.reshape(-1, 3).astype(np.float64)
    c = p.mean(0)
    r = float(np.linalg.norm(p - c, axis=1).max())
    to_cam = (sc.cam_pos.astype(np.float64) - c) / np.linalg.norm(sc.cam_pos.astype(np.float64) - c)
    a = c + to_cam * r * 1.01
    side = np.cross(to_cam, [0.0, 1.0, 0.0])
    side /= np.linalg.norm(side)
    degenerate = np.concatenate([a, a + 0.2 * side, a + 0.4 * side])                      # collinear vertices
    sliver = np.concatenate([a + 0.1 * to_cam, a + 0.1 * to_cam + 0.3 * side, a + 0.1 * to_cam + 0.3 * side + 1e-5 * to_cam])
    tri = np.concatenate([sc.tri, np.float32([degenerate, sliver])]).astype(np.float32)
    sc2 = SceneData(**{**vars(sc), "tri": tri, "tri_mat": np.concatenate([sc.tri_mat, sc.tri_mat[:2]]), "tri_uv": None})
    R = _ready(make_renderer, sc2, st)
    g = _wide_and_exact(R, "the sphere with a degenerate record")
    _assert_oracle(g, _oracle("nob_sphere", "degenerate", _with_camera(sc2, R), st), "the sphere with a degenerate record")


def test_split_tiles(make_renderer):
    """A low RT_HEAVY_SPLIT: the costliest tiles are split into parts traced by lane groups, which take the instance
    when no lane of the wave needs case (b)."""
    sc, st = _sphere()
    R = _ready(make_renderer, sc, st, RT_HEAVY_SPLIT=0.01)
    _frame(R, rgba=True)
    cost = R.tile_costs()
    assert _heavy_tiles(cost, nwaves=cost.size, split=0.01) > 0, "no tile would be split"
    g = _wide_and_exact(R, "split tiles")
    _assert_oracle(g, _oracle("nob_sphere", "default", _with_camera(sc, R), st), "split tiles")


@pytest.mark.parametrize("layout", [(8, 1), (8, 3), (3, 1), (3, 3)], ids=lambda l: f"rows{l[0]}x{l[1]}ranks")
def test_band_layouts(make_renderer, layout):
    import torch
    br, nranks = layout
    sc, st = _sphere()
    rw, rh = st.render_size()
    R = _ready(make_renderer, sc, st)
    exp = Oracle.downscale(_oracle("nob_sphere", "default", _with_camera(sc, R), st).argb, rw, rh, 2).reshape(H, W)
    nb = (H + br - 1) // br
    for rnd in range(2):   # (the camera's second launch starts at the entry sets)
        for rank in range(nranks):
            out = torch.zeros((R.local_rows(br, rank, nranks), W), dtype=torch.int32, device="cuda:0")
            R.render_bands_device(br, rank, nranks, out.data_ptr(), 0)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            for i, b in enumerate(range(rank, nb, nranks)):
                rows = min(br, H - b * br)
                assert np.array_equal(got[i * br:i * br + rows], exp[b * br:b * br + rows]), f"round {rnd}, rank {rank}, band {b}"


def test_moving_camera_then_at_rest_three_frames_in_flight(make_renderer):
    import torch
    sc, st = _sphere()
    rw, rh = st.render_size()
    R = _ready(make_renderer, sc, st)
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
    for i in range(3):
        exp = Oracle.downscale(_oracle("nob_sphere", ("move", i), cams[i], st).argb, rw, rh, 2)
        got = outs[i].cpu().numpy().view(np.uint32)[:H].ravel()
        assert np.array_equal(got, exp), f"frame {i}: {int((got != exp).sum())} pixels differ"
    exp = Oracle.downscale(_oracle("nob_sphere", ("move", 2), cams[2], st).argb, rw, rh, 2)
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
