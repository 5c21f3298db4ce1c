"""The host checker of the wide query's instance without case (b) (tests/c/nob_instance_check.cpp) for
tests/test_nob_instance.py: builds the program against the in-tree library (as tests/entry_cull_tool.py builds its own)
and runs it on a mesh, a camera and a light."""
import os
import struct
import subprocess
import tempfile

import numpy as np

from tile_mask_tool import proj_shortcut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "nob_instance_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "nob_instance_check")
LIBDIR = os.path.join(ROOT, "raytracercpp_amd")
# per ray kind: rays, those with nob, rays whose general query as every other caller runs it (and, with nob, without
# risk words: B) / nob rays whose NOB instance (C) differs from the frame kernels' general query (A), node visits,
# those of nob rays, the teeth mode's rays and those that differ
KIND = ("rays", "nob", "bad_b", "bad_c", "visits", "visits_nob", "teeth", "teeth_differ")
KEYS = tuple("cam_" + k for k in KIND) + tuple("shadow_" + k for k in KIND) + (
    "tiles", "tiles_all_nob", "cam_cap", "light_cap", "cam_at_risk", "light_at_risk", "nodes", "cones")


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


def nob_instance_check(tri9, cam, light, rw, rh, quick=False, teeth=False, ocone_dim=24, no_cap=False, max_depth=12,
                       leaf=40):
    """dict (KEYS, and 'nob': bool [rh, rw] of the camera rays): every pixel-centre ray of the camera (pos, proj_inv,
    cam_to_world) and the shadow ray of every certified hit towards light, each through the general query and, where
    its nob holds (teeth: where it does not), the instance without case (b) (no GPU)."""
    tri9 = np.ascontiguousarray(tri9, np.float32).reshape(-1, 9)
    pos, pinv, c2w = (np.ascontiguousarray(x, np.float32) for x in cam)
    light = np.ascontiguousarray(light, np.float32).reshape(3)
    mode, pw = proj_shortcut(pinv)
    affine = int(c2w[12] == 0 and c2w[13] == 0 and c2w[14] == 0 and c2w[15] == 1)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<q10if", tri9.shape[0], max_depth, leaf, rw, rh, int(quick), int(teeth), mode, affine,
                                ocone_dim, int(no_cap), float(pw)))
            f.write(pos.tobytes() + light.tobytes() + pinv.tobytes() + c2w.tobytes() + tri9.tobytes())
        r = subprocess.run([_program(), fin, fout], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fout, "rb").read()
    res = dict(zip(KEYS, map(int, np.frombuffer(raw, np.int64, len(KEYS)))))
    res["nob"] = np.frombuffer(raw, np.uint8, rw * rh, 8 * len(KEYS)).reshape(rh, rw).astype(bool)
    return res
