"""The layouts of the device-resident wide BVH's packed buffers (raytracercpp_amd/csrc/wide_layout.hpp: the
risk buffer, the slot maps, the risk walk's links) are the expressions their users computed by hand before the
header owned them, over (nodes, triangle records) in {1, 2, 7, 4096} x {1, 3, 5}: tests/c/accel_layout.cpp, a
host program that includes the header alone.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_functions_return_the_hand_written_offsets(tmp_path):
    exe = str(tmp_path / "accel_layout")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-x", "hip", "--offload-arch=gfx950", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "accel_layout.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    # 12 (nodes, records) pairs, 20 checks each
    assert int(out.stdout.split()[1]) == 12 * 20
