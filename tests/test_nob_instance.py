"""The wide query's instance without case (b) (wbvh.hpp wbvh_closest<.., NOB = true>) on the host,
through tests/c/nob_instance_check.cpp (nob_instance_tool).  For every camera ray (the camera's risk words and cap)
and every shadow ray of a certified hit (the light's words and cap, the origin cones): the frame kernels' general
query (risk words loaded only where nob does not hold) and the general query as every other caller runs it, both
with nob as computed, and for the rays whose nob holds also the general query with nob true and no risk words and
the instance, must agree in status, triangle, the bits of t, u and v, the reasons word and the work counters for
nodes, triangles and loop iterations.  Both trees.  The checker has teeth: rays whose nob does not hold, sent
through the instance, differ.  CPU only."""
import numpy as np
import pytest

import test_wbvh as tw
from nob_instance_tool import nob_instance_check
from test_scene_bound import MESHES, _box
from test_tile_mask import SIZES, _cameras
from tile_mask_tool import camera_towards

TREES = [False, True]


def _light(tri):
    lo, hi = _box(tri)
    return 0.5 * (lo + hi) + np.array([-0.6, 0.9, 0.7]) * 1.2 * float(np.linalg.norm(hi - lo))


def _views(tri, aspect):
    """From far, from close enough that the silhouette crosses the image, from near a face and from inside."""
    lo, hi = _box(tri)
    c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    cams = _cameras(tri, aspect)
    return {"far": cams["far"][0], "mid": camera_towards(c + np.array([0.48, 0.36, 0.8]) * 0.8 * diag, c, 80.0, aspect),
            "near": cams["near"][0], "inside": cams["inside"][0]}


def _line(what, r):
    return (f"{what}: camera rays {r['cam_rays']} (nob {r['cam_nob']}, their share of node visits "
            f"{r['cam_visits_nob'] / max(1, r['cam_visits']):.3f}), shadow rays {r['shadow_rays']} (nob {r['shadow_nob']}, "
            f"share {r['shadow_visits_nob'] / max(1, r['shadow_visits']):.3f}), all-nob tiles {r['tiles_all_nob']} of "
            f"{r['tiles']}, differing: no words {r['cam_bad_b']} + {r['shadow_bad_b']}, instance {r['cam_bad_c']} + "
            f"{r['shadow_bad_c']}")


def _agree(r):
    assert r["cam_bad_b"] == 0 and r["cam_bad_c"] == 0
    assert r["shadow_bad_b"] == 0 and r["shadow_bad_c"] == 0


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mesh", ["sphere", "bumpy"])
def test_the_instance_is_the_general_query_of_a_nob_ray(mesh, size):
    tri = MESHES[mesh]
    rw, rh = size
    mixed = cam_nob = shadow_nob = 0
    for quick in TREES:
        for name, cam in _views(tri, rw / rh).items():
            r = nob_instance_check(tri, cam, _light(tri), rw, rh, quick=quick)
            print(_line(f"{mesh} / {'quick' if quick else 'sah'} / {name}", r))
            _agree(r)
            assert r["cam_cap"] and r["light_cap"] and r["cones"]
            assert r["cam_rays"] == rw * rh and r["nob"].sum() == r["cam_nob"]
            cam_nob += r["cam_nob"]
            shadow_nob += r["shadow_nob"]
            mixed += 0 < r["cam_nob"] < r["cam_rays"]
    # (not vacuous: rays of both kinds skip case (b), and some views have rays that do and rays that do not)
    assert cam_nob > 0 and shadow_nob > 0 and mixed > 0


def test_the_cube_the_sliver_soup_and_a_mesh_without_a_cap():
    cube = MESHES["cube"]
    soup = tw._soup(np.random.default_rng(11))
    for quick in TREES:
        for name, cam in _views(cube, 128 / 72).items():
            r = nob_instance_check(cube, cam, _light(cube), 128, 72, quick=quick)
            print(_line(f"cube / {'quick' if quick else 'sah'} / {name}", r))
            _agree(r)
        # the soup's degenerate records leave no cap that lets a ray skip: no camera ray has nob
        r = nob_instance_check(soup, _views(soup, 128 / 72)["far"], _light(soup), 128, 72, quick=quick)
        print(_line(f"soup / {'quick' if quick else 'sah'} / far", r))
        _agree(r)
        assert r["cam_nob"] == 0 and r["cam_at_risk"] > 0
        # no cap at all: the shadow rays skip by the origin cones alone
        sphere = MESHES["sphere"]
        r = nob_instance_check(sphere, _views(sphere, 128 / 72)["mid"], _light(sphere), 128, 72, quick=quick, no_cap=True)
        print(_line(f"sphere without caps / {'quick' if quick else 'sah'} / mid", r))
        _agree(r)
        assert not r["cam_cap"] and r["cam_nob"] == 0 and r["shadow_nob"] > 0


def test_rays_that_need_case_b_differ_in_the_instance():
    """The checker has teeth: the rays whose nob does not hold go through the instance as well.  On the sphere's
    grazing rays (its silhouette, where the at-risk triangles are) answers or work counters then differ; the
    comparison of the nob rays still passes."""
    differ = 0
    for mesh in ("sphere", "bumpy"):
        tri = MESHES[mesh]
        for name in ("far", "mid"):
            r = nob_instance_check(tri, _views(tri, 128 / 72)[name], _light(tri), 128, 72, teeth=True)
            print(f"{mesh} / {name}: rays without nob sent through the instance {r['cam_teeth']} + {r['shadow_teeth']}, "
                  f"differing {r['cam_teeth_differ']} + {r['shadow_teeth_differ']}")
            _agree(r)
            assert r["cam_teeth"] == r["cam_rays"] - r["cam_nob"]
            differ += r["cam_teeth_differ"] + r["shadow_teeth_differ"]
    assert differ > 0
