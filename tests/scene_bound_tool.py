"""The scene bound's host checker (tests/c/scene_bound_check.cpp) for tests/test_scene_bound.py and
tests/test_gpu_scene_bound.py: builds the program against the in-tree library (as tests/test_soundness.py
builds wbvh_mutation.cpp; __graft_entry__.build() builds it ahead) and runs it on a mesh, a camera and rays."""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "scene_bound_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "scene_bound_check")
LIBDIR = os.path.join(ROOT, "raytracercpp_amd")


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


def scene_bound_check(tri9, cam, dirs, max_depth=12, leaf=40, scale_override=0.0):
    """(rejected flags, dict): every ray the bound rejects through the unmodified host query (no GPU)."""
    tri9 = np.ascontiguousarray(tri9, np.float32).reshape(-1, 9)
    c = np.ascontiguousarray(cam, np.float32).reshape(3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<qqiif", tri9.shape[0], d.shape[0], max_depth, leaf, float(scale_override)))
            f.write(c.tobytes() + tri9.tobytes() + d.tobytes())
        r = subprocess.run([_program(), fin, fout], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fout, "rb").read()
    out = np.frombuffer(raw, np.int64, 4)
    box = np.frombuffer(raw, np.float32, 6, 32)
    rej = np.frombuffer(raw, np.int32, d.shape[0], 56).copy()
    return rej, {"violations": int(out[0]), "rejected": int(out[1]), "misses": int(out[2]), "valid": bool(out[3]),
                 "lo": box[:3].copy(), "hi": box[3:].copy()}
