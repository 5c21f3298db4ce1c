"""The blocking part of a geometry change on the C4 scene (sphere1m, default BVH settings), host octree
build against the device build (rt_set_device_build), on the GPU: after rt_finish_accel,
set_object_transform `repeats` times with a frame after each; per row the medians of edit_ms (the
set_object_transform call alone), rt_stats build_ms, build_split_ms[0] (octree; a device build: with its
readback), build_split_ms[3] (the quick wide BVH and the upload; in device mode the quick tree is built on
the device too, rt_get_device_wide_builds counts it) and the wall time from the call to the image.  The
background build of the frame before is waited for outside the timed part.  Three rows in one process:
mode off, mode on (the edits run on the device, rt_get_device_transforms counts them), and mode on with
RT_GPU_XFORM=0 (the edits on the host, the positions uploaded again).  The images of all three must agree.
Usage: python tools/rebuild_time.py [repeats]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracercpp_amd import _lib, scenes
from raytracercpp_amd.renderer import Renderer, render

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 10
sc, st = scenes.sphere1m()
rows = {}
KEYS = ("edit_ms", "build_ms", "octree_ms", "upload_ms", "wall_ms")
for mode in ("host", "device", "device_host_xform"):
    if mode == "device_host_xform":   # (read at rt_create)
        os.environ["RT_GPU_XFORM"] = "0"
    try:
        r = Renderer(0)
    finally:
        os.environ.pop("RT_GPU_XFORM", None)
    r.set_device_build(mode != "host")
    r.load_scene(sc, st)
    render(r)
    r.finish_accel()
    render(r)
    samples = []
    for k in range(repeats):
        m = _lib.make_transform("rz", 1.0 + k)
        t0 = time.perf_counter()
        r.set_object_transform(m)
        t1 = time.perf_counter()
        render(r)
        img = r.get_image()
        wall = (time.perf_counter() - t0) * 1e3
        s = r.stats()
        samples.append({"mode": mode, "edit": k, "edit_ms": (t1 - t0) * 1e3, "build_ms": s["build_ms"],
                        "octree_ms": s["build_split_ms"][0], "upload_ms": s["build_split_ms"][3], "wall_ms": wall,
                        "checksum": int(img.sum(dtype="uint64"))})
        print(json.dumps(samples[-1]), flush=True)
        r.finish_accel()
    rows[mode] = {k: statistics.median(x[k] for x in samples) for k in KEYS}
    rows[mode]["spread"] = {k: max(x[k] for x in samples) - min(x[k] for x in samples) for k in KEYS}
    rows[mode]["host_builds"], rows[mode]["device_builds"] = r.stats()["host_builds"], r.device_builds()
    rows[mode]["device_wide_builds"] = r.device_wide_builds()
    rows[mode]["device_transforms"] = r.device_transforms()
    rows[mode]["checksums"] = [x["checksum"] for x in samples]
    print(f"{mode}: device_transforms {rows[mode]['device_transforms']}", flush=True)
    r.close()
sums = [rows[mode].pop("checksums") for mode in rows]
assert sums[0] == sums[1] == sums[2], "the three rows' images differ"
print(json.dumps({"medians": rows}), flush=True)
