"""wbvh_scene_bound after its per-child reach was factored out (wbvh.hpp wbvh_bound_ctx / wbvh_child_reach,
DESIGN.md 5.12): the bound of every mesh and camera of tests/test_scene_bound.py is bit for bit the one
recorded from the code before the change (tests/golden/scene_bound_parent.npz: lo, hi, valid).  CPU only."""
import os

import numpy as np
import pytest

from scene_bound_tool import scene_bound_check
from test_scene_bound import MESHES, _cameras

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_bound_parent.npz"))


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_scene_bound_is_bit_identical(mesh):
    for cam, pos in _cameras(MESHES[mesh]).items():
        _, info = scene_bound_check(MESHES[mesh], pos, np.zeros((0, 3), np.float32))
        got = np.concatenate([info["lo"], info["hi"], np.float32([info["valid"]])]).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), GOLDEN[f"{mesh}/{cam}"].view(np.uint32)), f"{mesh} / {cam}"
