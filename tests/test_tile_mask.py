"""The tile mask (wbvh.hpp wbvh_cut_host / wbvh_mask_cam / wbvh_mask_rect) on the host, through
tests/c/tile_mask_check.cpp (tile_mask_tool): every pixel-centre ray of every block the mask leaves clear,
its direction by the frame kernel's own float arithmetic, runs the unmodified wide query with and without the
camera's risk words and must end as a miss without a triangle test.  CPU only."""
import numpy as np
import pytest

import test_wbvh as tw
from test_scene_bound import MESHES, _box
from tile_mask_tool import camera, camera_towards, tile_mask_check

SIZES = [(128, 72), (96, 96)]


def _cameras(tri, aspect):
    """name -> (camera, a block must be clear)"""
    lo, hi = _box(tri)
    c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    u = np.array([0.48, 0.36, 0.8])
    far = c + u * 3.5 * diag
    near = np.array([c[0] + 0.1, c[1] - 0.05, hi[2] + 1e-3])
    face = np.array([c[0] + 0.1, c[1] - 0.05, hi[2]])
    side = c + np.array([1.0, 0.2, 0.1]) * 1.5 * diag
    return {
        "far": (camera_towards(far, c, 80.0, aspect), True),
        "near": (camera(near, 80.0, aspect), False),      # 1e-3 off a face, looking at it
        "face": (camera(face, 80.0, aspect), False),      # on a face
        "inside": (camera(c, 80.0, aspect), False),       # inside the bound: nothing can be masked
        "away": (camera_towards(far, 2 * far - c, 80.0, aspect), True),   # the scene behind: the line test
        # (a mesh of a few large triangles, the cube, has boxes and reaches too wide to clear a block from here)
        "rolled": (camera_towards(side, c, 80.0, aspect, roll=33.0, yaw_off=17.0), False),
        "fov20": (camera_towards(far, c, 20.0, aspect, yaw_off=4.0), False),
        "fov120": (camera_towards(side, c, 120.0, aspect, roll=-10.0), False),
    }


CAMERAS = ["far", "near", "face", "inside", "away", "rolled", "fov20", "fov120"]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("quick", [False, True], ids=["sah", "quick"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_rays_of_clear_blocks_miss_without_a_triangle_test(mesh, quick, size):
    tri = MESHES[mesh]
    rw, rh = size
    for name in CAMERAS:
        cam, must_mask = _cameras(tri, rw / rh)[name]
        for nudge in ((0, 3, -4) if name in ("far", "rolled") else (0,)):
            res = tile_mask_check(tri, cam, rw, rh, quick=quick, nudge=nudge)
            clear = ~res["covered"]
            print(f"{mesh} / {'quick' if quick else 'sah'} / {name} / nudge {nudge}: cut {res['cut']}, "
                  f"{int(clear.sum())} of {clear.size} blocks clear, {int(res['hit'].sum())} hit, "
                  f"violations {res['violations']}")
            assert res["violations"] == 0
            assert not (clear & res["hit"]).any()
            if must_mask:
                assert res["valid"] and clear.any()
            if name == "inside":
                assert not clear.any()
            if name == "away":
                # the scene lies behind the camera: the blocks its mirror image covers stay set (case (b)
                # accepts any t: a ray there may test a triangle)
                assert res["covered"].any()


def _dilate(a, r):
    p = np.pad(a, r)
    out = np.zeros_like(a)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + a.shape[0], dx:dx + a.shape[1]]
    return out


@pytest.mark.parametrize("quick", [False, True], ids=["sah", "quick"])
def test_far_sphere_mask_is_the_hit_blocks_and_a_ring(quick):
    """The ring: a cut box is widened by W >= 2 rho + step, rho the reach of the octree leaves its triangles
    share with their neighbours.  An octree leaf holds up to 40 of the sphere's 4,096 triangles, a hundredth
    of its surface, so it is about a fifth of the sphere's 48-pixel diameter across: W is at most some 16
    pixels of the 256 x 144 image, two blocks, and a covered block lies within two blocks of a hit one.  Of the
    all-miss blocks the mask must clear a larger share than the scene bound's box rejects."""
    tri = MESHES["sphere"]
    lo, hi = _box(tri)
    c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    cam = camera_towards(c + np.array([0.48, 0.36, 0.8]) * 1.2 * diag, c, 80.0, 256 / 144)
    res = tile_mask_check(tri, cam, 256, 144, quick=quick)
    assert res["valid"] and res["sb_valid"] and res["violations"] == 0
    assert res["hit"].sum() > 20
    assert not (res["covered"] & ~_dilate(res["hit"], 2)).any()
    miss = ~res["hit"]
    mask_share = (miss & ~res["covered"]).sum() / miss.sum()
    sb_share = (miss & res["sb_rejects"]).sum() / miss.sum()
    print(f"far sphere ({'quick' if quick else 'sah'}): cut {res['cut']}, all-miss blocks cleared by the mask "
          f"{mask_share:.3f}, rejected whole by the scene bound {sb_share:.3f}")
    assert mask_share > sb_share
    assert mask_share > 0.9


def test_cut_sizes_nest():
    """A larger budget refines the cut: its mask is a subset of the smaller one's."""
    tri = MESHES["bumpy"]
    lo, hi = _box(tri)
    c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    cam = camera_towards(c + np.array([0.48, 0.36, 0.8]) * 1.2 * diag, c, 80.0, 16 / 9)
    prev = None
    for budget in (4, 64, 1024, 16384):
        res = tile_mask_check(tri, cam, 128, 72, budget=budget)
        assert res["violations"] == 0 and res["cut"] <= budget
        if prev is not None:
            assert res["cut"] >= prev["cut"] and not (res["covered"] & ~prev["covered"]).any()
        prev = res


def test_shrunk_boxes_and_negative_guard_are_caught():
    """The checker has teeth: cut boxes at half their size, or a guard of -6 pixels, clear blocks that are hit
    (from 0.6 box diagonals the sphere is 130 pixels across: a box is larger than a block)."""
    tri = MESHES["sphere"]
    lo, hi = _box(tri)
    c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    cam = camera_towards(c + np.array([0.48, 0.36, 0.8]) * 0.6 * diag, c, 80.0, 256 / 144)
    assert tile_mask_check(tri, cam, 256, 144)["violations"] == 0
    assert tile_mask_check(tri, cam, 256, 144, scale_override=0.5)["violations"] > 0
    assert tile_mask_check(tri, cam, 256, 144, guard_override=-6.0)["violations"] > 0


def test_sliver_soup_and_out_of_gate_scale_have_no_mask():
    soup = tw._soup(np.random.default_rng(11))
    big = (MESHES["sphere"] * np.float32(1e13)).astype(np.float32)
    small = (MESHES["sphere"] * np.float32(1e-13)).astype(np.float32)
    for tri in (soup, big, small):
        lo, hi = _box(tri)
        c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
        cam = camera_towards(c + np.array([0.48, 0.36, 0.8]) * 3.5 * diag, c, 80.0, 16 / 9)
        res = tile_mask_check(tri, cam, 128, 72)
        assert not res["valid"] and res["covered"].all() and res["violations"] == 0
