"""The closed-form reach of well-conditioned children (wbvh.hpp wq_fast / wq_fast_eta, DESIGN.md 5.6
"Closed-form reach") is never below the bounds it replaces (wq_reach, wq_split, wq_eta), over every smin
code from the threshold up, every finite L code, qa from W_FAST_Q to 1 and D over 2^-20 .. 2^20, and is not
taken one step below either threshold: tests/c/wq_fast_bound.cpp, built with the closed form on.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_closed_form_reach_dominates_the_exact_bounds(tmp_path):
    exe = str(tmp_path / "wq_fast_bound")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-x", "hip",
                        "--offload-arch=gfx950", "-DW_FAST_REACH=1", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "wq_fast_bound.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    f = out.stdout.split()
    print(out.stdout.strip())
    assert int(f[1]) > 10_000_000
    # the constants are the corner's values rounded up: each closed form is within 1% of its bound there
    assert all(1.0 <= float(x) < 1.01 for x in f[2:6])
