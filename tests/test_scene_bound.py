"""The scene bound (DESIGN.md 5.6 "The scene bound"; wbvh.hpp wbvh_scene_bound / scene_bound_rejects) on the
host, through tests/c/scene_bound_check.cpp (scene_bound_tool): every camera ray the bound rejects runs the unmodified wide query, with
and without the camera's risk words, and must end as a certified miss after its root step (at most one
node visit).  CPU only."""
import numpy as np
import pytest

import test_wbvh as tw
from raytracercpp_amd import scenes
from scene_bound_tool import scene_bound_check


def _meshes():
    sphere, _ = scenes.uv_sphere_triangles(64, 32, texcoords=False)          # pole slivers
    bumpy, _ = scenes.uv_sphere_triangles(66, 33, bump=0.08, texcoords=False)
    shift = np.tile(np.float32([0.25, -0.5, -3.0]), 3)
    return {
        "sphere": (sphere + shift).astype(np.float32),
        "cube": scenes.cube1080(width=8, height=8)[0].tri,
        "robot": scenes.robot1080(width=8, height=8)[0].tri,
        "bumpy": (bumpy * np.float32(1.2) + shift).astype(np.float32),
    }


MESHES = _meshes()


def _box(tri):
    p = tri.reshape(-1, 3).astype(np.float64)
    return p.min(0), p.max(0)


def _cameras(tri):
    lo, hi = _box(tri)
    c, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    u = np.array([0.48, 0.36, 0.8])
    return {
        "far": c + u * 3.5 * diag,                                  # >= 3 box diagonals away
        "near": np.array([c[0] + 0.1, c[1] - 0.05, hi[2] + 1e-3]),   # 1e-3 from a face
        "face": np.array([c[0] + 0.1, c[1] - 0.05, hi[2]]),          # on a face
        "inside": c,
    }


def _nudge(d, k):
    """Each component moved by k float32 ulps (k of either sign)."""
    out = d.copy()
    for _ in range(abs(k)):
        out = np.nextafter(out, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return out


def _rays(rng, cam, lo, hi):
    """Directions from cam: random; through the faces, edges and corners of the box [lo, hi] and the same
    nudged by 1..4 ulps; axis-parallel; zero, tiny (< 2^-100) and denormal components; NaN / inf."""
    cam = np.float32(cam).astype(np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    d = rng.standard_normal((4000, 3))
    out = [d / np.linalg.norm(d, axis=1, keepdims=True)]
    # box points: per axis a coordinate at lo / hi / in between; corners (3 fixed), edges (2), faces (1)
    sel = rng.integers(0, 3, (3000, 3))
    sel[:8] = [[(i >> a) & 1 for a in range(3)] for i in range(8)]
    sel[8:600][:, :] = np.where(rng.random((592, 3)) < 0.7, rng.integers(0, 2, (592, 3)), 2)
    mid = lo + (hi - lo) * rng.random((3000, 3))
    pts = np.where(sel == 0, lo, np.where(sel == 1, hi, mid))
    through = (pts - cam).astype(np.float32)
    through = through[np.abs(through).max(1) > 0]
    out.append(through)
    for k in (-4, -3, -2, -1, 1, 2, 3, 4):
        out.append(_nudge(through[:800], k))
        g = through[800:1600].copy()
        ax = rng.integers(0, 3, len(g))
        g[np.arange(len(g)), ax] = _nudge(g[np.arange(len(g)), ax], k)   # one component only
        out.append(g)
    eye = np.eye(3, dtype=np.float32)
    out.append(np.concatenate([eye, -eye, eye * np.float32(1e-20), -eye * np.float32(3e37)]))
    sp = through[:1500].copy()
    vals = np.array([0.0, -0.0, 1e-31, -1e-31, 1e-38, -1e-41, 1e-45], np.float32)
    sp[np.arange(len(sp)), rng.integers(0, 3, len(sp))] = rng.choice(vals, len(sp))
    sp[np.arange(200), (np.arange(200) + 1) % 3] = rng.choice(vals, 200)   # (some with two such components)
    out.append(sp)
    out.append(np.zeros((1, 3), np.float32))
    bad = through[:600].copy()
    bad[np.arange(len(bad)), rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(bad))
    out.append(bad)
    return np.ascontiguousarray(np.concatenate([np.asarray(o, np.float32) for o in out]), np.float32)


def _run(tri, cam, seed=5, **kw):
    rng = np.random.default_rng(seed)
    # the bound's own planes (or, when it is invalid, the mesh's box) are what the directions aim at
    _, info = scene_bound_check(tri, cam, np.zeros((0, 3), np.float32), **kw)
    lo, hi = (info["lo"], info["hi"]) if info["valid"] else _box(tri)
    d = _rays(rng, cam, lo, hi)
    rej, res = scene_bound_check(tri, cam, d, **kw)
    assert res["valid"] == info["valid"]
    finite = np.isfinite(d).all(1)
    assert not rej[~finite].any(), "a NaN / inf direction was rejected"
    return d, rej, res


@pytest.mark.parametrize("camera", ["far", "near", "face", "inside"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_rejected_rays_end_after_the_root_step(mesh, camera):
    tri = MESHES[mesh]
    cam = _cameras(tri)[camera]
    d, rej, res = _run(tri, cam)
    print(f"{mesh} / {camera}: {len(d)} rays, {res}")
    assert res["valid"], "a well-conditioned mesh has a bound"
    assert res["violations"] == 0
    if camera == "inside":
        assert res["rejected"] == 0
    if camera == "far":
        assert res["rejected"] > 0


def test_far_camera_rejects_most_misses():
    """From 3.5 box diagonals the widened box subtends a few per cent of the directions: of the uniformly
    random rays the full query answers as misses, the bound must reject at least half."""
    tri = MESHES["sphere"]
    cam = _cameras(tri)["far"]
    rng = np.random.default_rng(9)
    d = rng.standard_normal((20000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rej, res = scene_bound_check(tri, cam, d)
    print(f"sphere / far, random rays: {res}")
    assert res["valid"] and res["violations"] == 0
    assert res["misses"] > 10000
    assert res["rejected"] >= 0.5 * res["misses"]


def test_sliver_soup_has_no_bound():
    """A root child holding degenerate triangles has no finite reach: the bound is invalid, nothing is rejected."""
    tri = tw._soup(np.random.default_rng(11))
    for camera, cam in _cameras(tri).items():
        d, rej, res = _run(tri, cam)
        print(f"soup / {camera}: {res}")
        assert not res["valid"] and res["rejected"] == 0 and res["violations"] == 0


@pytest.mark.parametrize("factor", [1e-13, 1e13])
def test_scene_scale_outside_the_gate_has_no_bound(factor):
    tri = (MESHES["sphere"] * np.float32(factor)).astype(np.float32)
    cam = _cameras(tri)["far"]
    d, rej, res = _run(tri, cam)
    assert not res["valid"] and res["rejected"] == 0 and res["violations"] == 0


def test_shrunk_bound_is_caught():
    """The checker has teeth: the bound shrunk to half its size rejects rays that hit the sphere."""
    tri = MESHES["sphere"]
    cam = _cameras(tri)["far"]
    d, rej, res = _run(tri, cam, scale_override=0.5)
    print(f"sphere / far, bound x 0.5: {res}")
    assert res["valid"] and res["violations"] > 0
    # rays at the triangles' centroids: those outside the half-size box are rejected although they hit
    aim = (tri.reshape(-1, 3, 3).mean(1) - np.float32(cam)).astype(np.float32)
    rej, res = scene_bound_check(tri, cam, aim, scale_override=0.5)
    print(f"sphere / far, bound x 0.5, rays at the triangles: {res}")
    assert res["violations"] > len(aim) // 10
    rej, res = scene_bound_check(tri, cam, aim)
    assert res["violations"] == 0
