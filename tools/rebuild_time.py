"""The blocking part of a geometry change on the C4 scene (sphere1m, default BVH settings), host octree
build against the device build (rt_set_device_build), on the GPU: after rt_finish_accel,
set_object_transform `repeats` times with a frame after each; per mode the medians of rt_stats build_ms,
build_split_ms[0] (octree; a device build: with its readback), build_split_ms[3] (the quick wide BVH and
the upload; in device mode the quick tree is built on the device too, rt_get_device_wide_builds counts it)
and the wall time from the call to the image.  The background build of the frame before is waited for
outside the timed part.  Mode off runs first, then mode on, in one process.
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
for mode in ("host", "device"):
    r = Renderer(0)
    r.set_device_build(mode == "device")
    r.load_scene(sc, st)
    render(r)
    r.finish_accel()
    render(r)
    samples = []
    for k in range(repeats):
        m = _lib.make_transform("rz", 1.0 + k)
        t0 = time.perf_counter()
        r.set_object_transform(m)
        render(r)
        img = r.get_image()
        wall = (time.perf_counter() - t0) * 1e3
        s = r.stats()
        samples.append({"mode": mode, "edit": k, "build_ms": s["build_ms"], "octree_ms": s["build_split_ms"][0],
                        "upload_ms": s["build_split_ms"][3], "wall_ms": wall, "checksum": int(img.sum(dtype="uint64"))})
        print(json.dumps(samples[-1]), flush=True)
        r.finish_accel()
    builds = (r.stats()["host_builds"], r.device_builds())
    wide_builds = r.device_wide_builds()
    rows[mode] = {k: statistics.median(x[k] for x in samples) for k in ("build_ms", "octree_ms", "upload_ms", "wall_ms")}
    rows[mode]["host_builds"], rows[mode]["device_builds"] = builds
    rows[mode]["device_wide_builds"] = wide_builds
    rows[mode]["checksums"] = [x["checksum"] for x in samples]
    r.close()
assert rows["host"].pop("checksums") == rows["device"].pop("checksums"), "the two modes' images differ"
print(json.dumps({"medians": rows}), flush=True)
