"""The tile lists (raytracercpp_amd/csrc/tile_lists.hpp) on the host, through
tests/c/tile_lists_check.cpp: over all-clear, all-set, one-bit, disc and random masks at 64 x 32, 96 x 96 and
128 x 72 internal pixels, the whole frame, band rows 8 and 3 at 1 and 3 ranks and permuted band lists, the lists
are ascending, disjoint, cover exactly the on-image tiles and agree with the frame kernel's predicate evaluated
lane by lane; the queue's eight shard ranges partition 'covered' (also for fewer than eight entries and for
none).  The program needs the header alone (no library, no GPU) and is also built with the address and
undefined-behaviour sanitizers, as a stand-alone program.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "tile_lists_check.cpp")
HIPCC = "/opt/rocm/bin/hipcc"


def build_program(out, extra=()):
    cmd = [HIPCC, "-std=c++17", "-O2", "-x", "hip", "--cuda-host-only", *extra, "-o", out, SRC]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1].startswith("OK ")


def test_lists_match_the_lane_predicate_and_shards_partition(tmp_path):
    _run(build_program(str(tmp_path / "tile_lists_check")))   # (always from the current header)


def test_the_same_under_asan_and_ubsan(tmp_path):
    exe = build_program(str(tmp_path / "tile_lists_check_san"),
                        ("-g", "-O1", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    _run(exe)
