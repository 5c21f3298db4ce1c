"""The host quick wide BVH by its digests (rt_wbvh_quick_digest; the per-node arithmetic shared with the
device builder, wbvh_quick.hpp): the same bytes at any thread count, the statistics the host probe sees,
the runs trees' closed-form size, and the stand-alone builder (tests/c/wbvh_quick_host.cpp).  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from raytracercpp_amd import _lib, scenes
from test_octree_build import soup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    ("robot", lambda: scenes.robot1080()[0].tri, 12, 40),
    ("soup", lambda: soup(1, 20000), 12, 4),
]


@pytest.mark.parametrize("name,make,depth,leaf", CASES, ids=[c[0] for c in CASES])
def test_digest_is_thread_count_independent(name, make, depth, leaf, monkeypatch):
    tri = make()
    got = {}
    for threads in ("1", "3", "8"):
        monkeypatch.setenv("RT_BUILD_THREADS", threads)
        got[threads] = _lib.wbvh_quick_digest(tri, depth, leaf)[:2]
    assert got["1"] == got["3"] == got["8"]
    assert len(got["1"][0]) == 6 and len(set(got["1"][0])) == 6


@pytest.mark.parametrize("name,make,depth,leaf", CASES, ids=[c[0] for c in CASES])
def test_stats_equal_the_host_probes(name, make, depth, leaf, monkeypatch):
    """rt_wbvh_query with RT_WBVH_QUICK=1 builds the same tree: the same statistics, 0 violations."""
    tri = make()
    _, st, _ = _lib.wbvh_quick_digest(tri, depth, leaf)
    monkeypatch.setenv("RT_WBVH_QUICK", "1")
    o = np.zeros((1, 3), np.float32)
    d = np.array([[0, 0, -1]], np.float32)
    *_, q, _ = _lib.wbvh_query(tri, o, d, depth, leaf)
    assert q["violations"] == 0
    for k in ("nodes", "leaves", "max_leaf", "depth"):
        assert st[k] == q[k], k
    assert st["tris"] == len(tri)


def test_empty_scene_and_bad_arguments():
    dg, st, _ = _lib.wbvh_quick_digest(np.zeros((0, 9), np.float32))
    assert st == {"nodes": 0, "leaves": 0, "tris": 0, "max_leaf": 0, "depth": 0}
    assert len(set(dg)) == 1   # six empty digests
    L = _lib.lib()
    assert L.rt_wbvh_quick_digest(None, 5, 12, 40, None, None, None) == -1   # RT_EINVAL
    assert L.rt_wbvh_quick_build_device(0, None, 5, 12, 40, None, None, None, None) == -1
    import ctypes as C
    n = C.c_int64()
    assert L.rt_get_device_wide_builds(None, C.byref(n)) == -1


def test_device_builder_refuses_without_device_or_outside_its_range():
    """Depth 31 is RT_EUNSUPPORTED before any HIP call; in range, no usable device is RT_EHIP."""
    import torch
    tri = soup(6, 50)
    with pytest.raises(_lib.RtError) as ei:
        _lib.wbvh_quick_build_device(tri, 31, 40)
    assert ei.value.code == -5   # RT_EUNSUPPORTED
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RtError) as ei:
            _lib.wbvh_quick_build_device(tri, 12, 40)
        assert ei.value.code == -2   # RT_EHIP
        assert _lib.lib().rt_last_error().decode().startswith("rt_wbvh_quick_build_device:")


def test_standalone_host_builder(tmp_path):
    """tests/c/wbvh_quick_host.cpp against the library's host builders: piles, soups with degenerate
    records and a sphere, 0 violations each."""
    lib = os.path.join(ROOT, "raytracercpp_amd")
    exe = str(tmp_path / "wbvh_quick_host")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-x", "hip",
                        "--offload-arch=gfx950", "-o", exe, os.path.join(ROOT, "tests", "c", "wbvh_quick_host.cpp"),
                        "-L" + lib, "-lrt_mi355x", "-Wl,-rpath," + lib],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
