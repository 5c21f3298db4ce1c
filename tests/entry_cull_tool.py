"""The back-face test's host checker (tests/c/entry_cull_check.cpp) for tests/test_entry_cull.py: builds the program
against the in-tree library (as tests/tile_starts_tool.py builds its own) and runs it on a mesh and a camera."""
import os
import struct
import subprocess
import tempfile

import numpy as np

from tile_mask_tool import proj_shortcut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "entry_cull_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "entry_cull_check")
LIBDIR = os.path.join(ROOT, "raytracercpp_amd")
FAN, FAN_UNCULLED = 4, 3   # wbvh.hpp W_ENTRY_FAN, W_ENTRY_FAN_UNCULLED


def build_program(out=EXE):
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-x", "hip",
           "--offload-arch=gfx950", "-o", out, SRC, "-L" + LIBDIR, "-lrt_mi355x", "-Wl,-rpath," + LIBDIR, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _program():
    """The built program (__graft_entry__.build() rebuilds it with the library); built here when it is missing."""
    if not os.path.exists(EXE):
        build_program()
    return EXE


def entry_cull_check(tri9, cam, rw, rh, quick=False, budget=4096, nudge=0, k=4, fan=None, cull=1, max_depth=12, leaf=40):
    """dict: the entry sets of the camera (pos, proj_inv, cam_to_world) over a rw x rh image with WMaskCam::cull =
    cull, and every child the block test drops checked against the per-ray cone test of the block's rays (no GPU).
    fan None: the renderer's (wbvh.hpp W_ENTRY_FAN with the test, W_ENTRY_FAN_UNCULLED without it)."""
    fan = (FAN if cull else FAN_UNCULLED) if fan is None else fan
    tri9 = np.ascontiguousarray(tri9, np.float32).reshape(-1, 9)
    pos, pinv, c2w = (np.ascontiguousarray(x, np.float32) for x in cam)
    mode, pw = proj_shortcut(pinv)
    affine = int(c2w[12] == 0 and c2w[13] == 0 and c2w[14] == 0 and c2w[15] == 1)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<q12if", tri9.shape[0], max_depth, leaf, rw, rh, int(quick), budget, nudge, mode, affine,
                                k, fan, cull, float(pw)))
            f.write(pos.tobytes() + pinv.tobytes() + c2w.tobytes() + tri9.tobytes())
        r = subprocess.run([_program(), fin, fout], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fout, "rb").read()
    out = np.frombuffer(raw, np.int64, 10)
    bw, bh = int(out[1]), int(out[2])
    sets = np.frombuffer(raw, np.uint32, bw * bh * 4, 80).reshape(bh, bw, 4)
    keys = ("valid", "bw", "bh", "covered", "below_root", "examined", "dropped", "violations", "cones", "structural")
    res = dict(zip(keys, map(int, out)))
    res.update(valid=bool(out[0]), sets=sets)
    return res
