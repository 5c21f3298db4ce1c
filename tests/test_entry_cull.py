"""The entry search's back-face test (wbvh.hpp wbvh_entry_backfacing) on the host, through
tests/c/entry_cull_check.cpp (entry_cull_tool) and tests/c/tile_starts_check.cpp (tile_starts_tool, whose camera has
the test on, as every camera of wbvh_mask_cam has).  A child the block's test drops must be skipped by every ray of
the block through the query's own float cone test; the queries from the culled sets must give the root queries'
answers after the fallback; with the test off the sets are those of the search before it had one
(tests/golden/entry_sets_before_cull.npz: the sets its tile_starts_check wrote for these meshes and cameras at
128 x 72); a mesh without cones is not touched.  CPU only."""
import os

import numpy as np
import pytest

from entry_cull_tool import FAN, entry_cull_check
from test_scene_bound import MESHES, _box
from test_tile_mask import CAMERAS, SIZES, _cameras
from test_tile_starts import _final, _oracle
from tile_mask_tool import camera_towards
from tile_starts_tool import tile_starts_check

EMPTY = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entry_sets_before_cull.npz")
# the UV sphere and the bumpy sphere from far away, from near and from inside (tests/test_tile_mask.py _cameras)
VIEWS = ["far", "near", "inside"]


def _wide_cam(tri):
    """A wide field of view from close by: a block of the 64 x 32 image spans many degrees."""
    lo, hi = _box(tri)
    c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    return camera_towards(c + np.array([0.48, 0.36, 0.8]) * 0.45 * diag, c, 140.0, 2.0)


def _line(what, r):
    return (f"{what}: {r['covered']} covered blocks, {r['below_root']} below the root, {r['examined']} nodes examined, "
            f"{r['dropped']} children dropped, violations {r['violations']}")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mesh", ["sphere", "bumpy"])
def test_a_dropped_child_is_skipped_by_every_ray_of_the_block(mesh, size):
    tri = MESHES[mesh]
    rw, rh = size
    for quick in (False, True):
        for name in VIEWS:
            cam, _ = _cameras(tri, rw / rh)[name]
            for nudge in ((0, 3, -4) if name == "far" else (0,)):
                r = entry_cull_check(tri, cam, rw, rh, quick=quick, nudge=nudge)
                print(_line(f"{mesh} / {'quick' if quick else 'sah'} / {name} / nudge {nudge}", r))
                assert r["valid"] and r["structural"] == 0
                assert r["violations"] == 0
                # (the test is not vacuous.  From inside every triangle faces away: what the search reaches is dropped
                # unless it has no cone, and an emptied frontier is stored as the root)
                assert r["dropped"] > 0


def test_the_cube_and_a_wide_field_of_view():
    for quick in (False, True):
        for name in CAMERAS:
            cam, _ = _cameras(MESHES["cube"], 128 / 72)[name]
            r = entry_cull_check(MESHES["cube"], cam, 128, 72, quick=quick)
            print(_line(f"cube / {'quick' if quick else 'sah'} / {name}", r))
            assert r["violations"] == 0 and r["structural"] == 0
            if name in ("far", "rolled", "fov20", "fov120") and not quick:
                assert r["dropped"] > 0   # (the quick tree of the 12 triangles has one child with a cone)
        for mesh in ("sphere", "bumpy"):
            r = entry_cull_check(MESHES[mesh], _wide_cam(MESHES[mesh]), 64, 32, quick=quick)
            print(_line(f"{mesh} / {'quick' if quick else 'sah'} / wide field of view at 64 x 32", r))
            assert r["valid"] and r["violations"] == 0 and r["structural"] == 0 and r["dropped"] > 0


def test_the_centre_direction_alone_is_caught():
    """The checker has teeth: a block test that looks at the block's centre direction only (WMaskCam::cull = 2, set
    by the check program alone) drops children that rays near the block's corners still enter."""
    tri = MESHES["sphere"]
    good = entry_cull_check(tri, _wide_cam(tri), 64, 32, cull=1)
    bad = entry_cull_check(tri, _wide_cam(tri), 64, 32, cull=2)
    print(_line("the four corners", good))
    print(_line("the centre alone", bad))
    assert good["violations"] == 0 and good["dropped"] > 0
    assert bad["violations"] > 0


@pytest.mark.parametrize("quick", [False, True], ids=["sah", "quick"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_queries_from_the_culled_sets_agree_with_root_queries(mesh, quick):
    """tests/test_tile_starts.py's scenes, both trees: every pixel-centre ray from the root and from its block's
    culled entry set (the sets are checked to be the cull's: entry_cull_check's with the test on)."""
    tri = MESHES[mesh]
    changed = 0
    for rw, rh in SIZES:
        for name in CAMERAS:
            cam, _ = _cameras(tri, rw / rh)[name]
            res = tile_starts_check(tri, cam, rw, rh, quick=quick, fan=FAN)
            on = entry_cull_check(tri, cam, rw, rh, quick=quick, cull=1)
            off = entry_cull_check(tri, cam, rw, rh, quick=quick, cull=0)
            assert np.array_equal(res["sets"], on["sets"])
            changed += int((on["sets"] != off["sets"]).any(2).sum())
            _, differ = _final(res, _oracle(mesh, tri))
            print(f"{mesh} / {'quick' if quick else 'sah'} / {rw} x {rh} / {name}: {res['below_root']} blocks start below "
                  f"the root, certified from the root but not from the entry set: {res['extra_fallbacks']}, answers that "
                  f"differ {differ}")
            assert res["violations"] == 0
            assert res["certified_differ"] == 0 and differ == 0
    if mesh in ("sphere", "bumpy"):
        assert changed > 0   # (the cull does change sets here)


def test_knob_off_gives_the_sets_of_the_search_before_the_cull():
    gold = np.load(GOLDEN)
    differ = 0
    for key in gold.files:
        mesh, name, tree = key.split("_")
        cam, _ = _cameras(MESHES[mesh], 128 / 72)[name]
        off = entry_cull_check(MESHES[mesh], cam, 128, 72, quick=tree == "quick", cull=0)
        assert np.array_equal(off["sets"], gold[key]), key
        on = entry_cull_check(MESHES[mesh], cam, 128, 72, quick=tree == "quick", cull=1)
        differ += int((on["sets"] != gold[key]).any(2).sum())
    assert len(gold.files) == 24 and differ > 0


def test_a_mesh_without_cones_keeps_its_sets():
    """The UV sphere with every triangle twice, once per winding: a child that holds both copies of a triangle has
    no cone (code 255), and only a few leaf children hold a single copy (printed).  Nothing is dropped, and the sets
    are the same words with the test on and off, although blocks do start below the root."""
    tri = MESHES["sphere"].reshape(-1, 3, 3)
    both = np.stack([tri, tri[:, [0, 2, 1]]], 1).reshape(-1, 9)
    lo, hi = _box(both)
    c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    below = 0
    for dist in (3.5, 0.6):
        cam = camera_towards(c + np.array([0.48, 0.36, 0.8]) * dist * diag, c, 80.0, 16 / 9)
        for quick in (False, True):
            on = entry_cull_check(both, cam, 128, 72, quick=quick, cull=1, fan=FAN)
            off = entry_cull_check(both, cam, 128, 72, quick=quick, cull=0, fan=FAN)
            print(_line(f"two-sided sphere / {'quick' if quick else 'sah'} / {dist}: children with a cone {on['cones']}", on))
            assert on["valid"] and on["dropped"] == 0 and on["violations"] == 0
            assert np.array_equal(on["sets"], off["sets"])
            below += on["below_root"]
    assert below > 0
