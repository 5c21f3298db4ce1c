"""Geometry that changes on every frame, on the C4 scene (sphere1m, default BVH settings, device build on),
on the GPU: after rt_finish_accel, `steps` steps, each with new positions made by torch on the device and
one frame.  Per step: set_ms (the call that gives the positions, alone), rt_stats build_ms,
build_split_ms (octree; quick wide BVH and upload) and the wall time from the call to the image.
Four rows in one process:
  host             set_triangles from a host array (downloaded outside the timed part), rt_finish_accel
                   between the steps, outside the timed part
  device           update_vertices_device from the tensor, rt_finish_accel between the steps likewise
  device_deferred  the same with rt_set_accel_deferred: no background build is started
  device_joined    as `device` without rt_finish_accel between the steps: each change waits for the
                   background build of the one before
The image checksums of all rows must agree at each step.  Rows whose calls the loaded library lacks are
skipped (RT_LIB_PATH naming an older build: the host row alone).
Usage: python tools/deform_time.py [steps [row,row,...]]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracercpp_amd import _lib, scenes
from raytracercpp_amd.renderer import Renderer, render

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
sc, st = scenes.sphere1m()
base = torch.from_numpy(sc.tri.copy()).cuda()
KEYS = ("set_ms", "build_ms", "octree_ms", "upload_ms", "wall_ms")
ROWS = {"host": (), "device": ("rt_update_vertices_device",),
        "device_deferred": ("rt_update_vertices_device", "rt_set_accel_deferred"),
        "device_joined": ("rt_update_vertices_device",)}
only = sys.argv[2].split(",") if len(sys.argv) > 2 else list(ROWS)
rows = {}
for mode, needs in ROWS.items():
    if mode not in only:
        continue
    if not all(_lib.has(name) for name in needs):
        print(f"{mode}: skipped (the library lacks {', '.join(n for n in needs if not _lib.has(n))})", flush=True)
        continue
    r = Renderer(0)
    r.set_device_build(True)
    if mode == "device_deferred":
        r.set_accel_deferred(True)
    r.load_scene(sc, st)
    render(r)
    r.finish_accel()
    render(r)
    samples = []
    for k in range(steps):
        t = (base + 0.01 * torch.sin(5.0 * base.roll(1, 1) + float(k))).contiguous()
        host = t.cpu().numpy() if mode == "host" else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "host":
            r.set_triangles(host, sc.tri_mat, sc.tri_uv)
        else:
            r.update_vertices_device(t)
        t1 = time.perf_counter()
        render(r)
        img = r.get_image()
        wall = (time.perf_counter() - t0) * 1e3
        s = r.stats()
        samples.append({"mode": mode, "step": k, "set_ms": (t1 - t0) * 1e3, "build_ms": s["build_ms"],
                        "octree_ms": s["build_split_ms"][0], "upload_ms": s["build_split_ms"][3], "wall_ms": wall,
                        "wide_tree": s["wide_tree"], "checksum": int(img.sum(dtype="uint64"))})
        print(json.dumps(samples[-1]), flush=True)
        if mode in ("host", "device"):
            r.finish_accel()
    rows[mode] = {k: statistics.median(x[k] for x in samples) for k in KEYS}
    rows[mode]["range"] = {k: [min(x[k] for x in samples), max(x[k] for x in samples)] for k in KEYS}
    rows[mode]["host_builds"], rows[mode]["device_builds"] = r.stats()["host_builds"], r.device_builds()
    if _lib.has("rt_get_device_ingests"):
        rows[mode]["device_ingests"], rows[mode]["accel_builds"] = r.device_ingests(), r.accel_builds()
    rows[mode]["checksums"] = [x["checksum"] for x in samples]
    r.finish_accel()
    r.close()
sums = [rows[mode].pop("checksums") for mode in rows]
assert all(s == sums[0] for s in sums), "the rows' images differ"
print(json.dumps({"checksums": sums[0]}), flush=True)
print(json.dumps({"medians": rows}), flush=True)
