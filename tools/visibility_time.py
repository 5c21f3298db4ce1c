"""The visibility buffer of the current camera in GPU memory (rt_visibility_device), timed on the C4 scene
(sphere1m, 1920 x 1080, SSAA 2: 3840 x 2160 = 8,294,400 pixels of the internal image) after rt_finish_accel, on one
GPU.  Rows, all in one process:
  a  visibility_device of the default renderer from the third launch on (tile mask and entry sets)
  b  the same with RT_TILE_START=0 (the mask, every query from the root)
  c  the same with RT_TILE_MASK=0 (neither)
  d  trace_rays_device of the default renderer on the same 8,294,400 camera rays, lying in GPU memory in pixel
     order (they are made by the reference's float32 expressions, tests/test_trace_ray.py camera_rays' recipe: the
     rays must be the kernel's bit for bit for the rows to be comparable)
  e  rt_ray_trace's kernel_ms with the hit buffers requested (the frame kernel: primary query, shading, shadow query)
  f  row a on the quick tree (RT_ACCEL_DEFER=1: no refinement, the state an animated mesh runs in)
  g  row a's launches with three in flight: 30 launches round-robin over three streams between one event pair, ms
     per launch (what bench.py's ms per step is for frames, which also keeps three in flight)
Each call of rows a-d and f is timed with a torch.cuda.Event pair on the call's stream after three warm-up launches;
row e is the library's own event pair around the frame kernel.  The median and the range of the repetitions are
reported, with Mpixels/s from the median.  Rows a, b, c (and f) must agree bit for bit in id, t, u, v, and with row d
where a ray hits (id where t > 0.1, t, u, v; elsewhere the visibility rows hold -1, the fresh record's t, 0, 0):
else the tool exits with status 1.
Usage: python tools/visibility_time.py [repetitions]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracercpp_amd import scenes
from raytracercpp_amd.renderer import Renderer, render

reps = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 10
dev = torch.device("cuda", 0)   # (no GPU: this raises at the first tensor)
sc, st = scenes.sphere1m()
rw, rh = st.render_size()
npx = rw * rh


def make(env=None, finish=True):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        r = Renderer(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    r.load_scene(sc, st)
    render(r)
    if finish:
        r.finish_accel()
        render(r)
    return r


def camera_rays():
    """Every pixel's primary ray (renderer.cpp:1086-1098) in float32, the reference's operation order."""
    f32 = np.float32

    def xform(m, x, y, z):
        m = np.asarray(m, np.float32)
        xt = m[0] * x + m[1] * y + m[2] * z + m[3]
        yt = m[4] * x + m[5] * y + m[6] * z + m[7]
        zt = m[8] * x + m[9] * y + m[10] * z + m[11]
        wt = m[12] * x + m[13] * y + m[14] * z + m[15]
        w = f32(1) / wt
        keep = wt == f32(1)
        return np.where(keep, xt, xt * w), np.where(keep, yt, yt * w), np.where(keep, zt, zt * w)

    py, px = np.meshgrid(np.arange(rh, dtype=np.float32), np.arange(rw, dtype=np.float32), indexing="ij")
    yw = (py + f32(0.5)) / f32(rh) * f32(2) - f32(1)
    xw = (px + f32(0.5)) / f32(rw) * f32(2) - f32(1)
    ws = xform(sc.cam_to_world, *xform(sc.proj_inv, xw, yw, np.full_like(xw, -1)))
    cam = np.asarray(sc.cam_pos, np.float32)
    d = np.stack([ws[0] - cam[0], ws[1] - cam[1], ws[2] - cam[2]], axis=-1).reshape(-1, 3)
    l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    d = (d * (f32(1) / np.sqrt(l2))[:, None]).astype(np.float32)
    o = np.broadcast_to(cam, d.shape).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(o)).to(dev), torch.from_numpy(d).to(dev)


def timed(call, warm=3):
    for _ in range(warm):
        res = call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return res, ms


lines = {}


def report(row, what, ms, **extra):
    med = statistics.median(ms)
    line = dict({"row": row, "what": what, "pixels": npx, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                 "ms_max": round(max(ms), 4), "reps": len(ms), "mpixels_per_s": round(npx / med / 1e3, 1)}, **extra)
    lines[row] = line
    print(json.dumps(line), flush=True)


def as_bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


ok = True


def compare(row, out, ref):
    global ok
    for k in ("tri_id", "t", "uv"):
        if not torch.equal(as_bits(out[k]), as_bits(ref[k])):
            ok = False
            print(f"row {row}: {k} differs from row a in {int((as_bits(out[k]) != as_bits(ref[k])).sum())} elements", flush=True)


def visibility_row(row, what, r):
    out = {"tri_id": torch.empty((rh, rw), dtype=torch.int32, device=dev),
           "t": torch.empty((rh, rw), dtype=torch.float32, device=dev),
           "uv": torch.empty((rh, rw, 2), dtype=torch.float32, device=dev)}
    c0 = r.device_visibility()
    _, ms = timed(lambda: r.visibility_device(out=out))
    c1 = r.device_visibility()
    n = len(ms) + 3
    report(row, what, ms, wide_tree=r.stats()["wide_tree"], launches_fast_generic=[b - a for a, b in zip(c0[0], c1[0])],
           launches_with_mask_entry_sets=[b - a for a, b in zip(c0[2], c1[2])], launches=n)
    return out


ra = make()
a = visibility_row("a", "visibility_device, mask and entry sets", ra)
print(json.dumps({"scene": "sphere1m", "triangles": int(sc.ntri), "internal_image": [rw, rh], "repetitions": reps,
                  "pixels_showing_a_triangle": int((a["tri_id"] >= 0).sum())}), flush=True)
for row, what, env in (("b", "visibility_device, RT_TILE_START=0", {"RT_TILE_START": "0"}),
                       ("c", "visibility_device, RT_TILE_MASK=0", {"RT_TILE_MASK": "0"})):
    r = make(env)
    compare(row, visibility_row(row, what, r), a)
    r.close()

# g: row a's launches, three in flight: 30 launches round-robin over three streams between one event pair (the
# figure to hold against bench.py's ms per step, which has three frames in flight: a launch's tail overlaps the next)
streams = [torch.cuda.Stream(dev) for _ in range(3)]
outs = [{"tri_id": torch.empty((rh, rw), dtype=torch.int32, device=dev), "t": torch.empty((rh, rw), dtype=torch.float32, device=dev),
         "uv": torch.empty((rh, rw, 2), dtype=torch.float32, device=dev)} for _ in streams]
main = torch.cuda.current_stream(dev)
ms = []
for rep in range(reps + 1):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(main)
    for s in streams:
        s.wait_event(e0)
    for k in range(30):
        ra.visibility_device(out=outs[k % 3], stream=streams[k % 3])
    for s in streams:
        main.wait_stream(s)
    e1.record(main)
    e1.synchronize()
    if rep:   # (the first round is the streams' warm-up: their slots, masks and entry sets)
        ms.append(e0.elapsed_time(e1) / 30)
report("g", "visibility_device, three launches in flight, ms per launch", ms)
for o_ in outs:
    compare("g", o_, a)
del outs

# d: the ray query on the same rays
o, d = camera_rays()
q = {k: torch.empty(npx, dtype=dt, device=dev) for k, dt in
     (("tri_id", torch.int32), ("t", torch.float32), ("u", torch.float32), ("v", torch.float32), ("ret", torch.uint8))}
_, ms = timed(lambda: ra.trace_rays_device(o, d, out=q))
report("d", "trace_rays_device on the camera rays", ms)
hit = (q["ret"] != 0) & (q["t"] > 0.1)
va = {k: a[k].reshape(-1, 2) if k == "uv" else a[k].reshape(-1) for k in a}
checks = {"id": torch.equal(va["tri_id"], torch.where(hit, q["tri_id"], torch.full_like(q["tri_id"], -1))),
          "t": torch.equal(as_bits(va["t"])[hit], as_bits(q["t"])[hit]) and bool((va["t"][~hit] == -1).all()),
          "u": torch.equal(as_bits(va["uv"][:, 0])[hit], as_bits(q["u"])[hit]),
          "v": torch.equal(as_bits(va["uv"][:, 1])[hit], as_bits(q["v"])[hit]),
          "uv elsewhere": not bool(as_bits(va["uv"])[~hit].any())}
for k, good in checks.items():
    if not good:
        ok = False
        print(f"row d: {k} differs from row a", flush=True)
del o, d, q

# e: the frame kernel with the hit buffers requested
ra.request_aux(hit=True)
for _ in range(3):
    ra.ray_trace()
ms = []
for _ in range(reps):
    ra.ray_trace()
    ms.append(ra.stats()["kernel_ms"])
report("e", "rt_ray_trace kernel_ms, hit buffers requested", ms)
g = ra.get_internal(argb=False, hit=True)
if not (np.array_equal(g["hit_id"], va["tri_id"].cpu().numpy()) and
        np.array_equal(g["hit_t"].view(np.uint32), va["t"].cpu().numpy().view(np.uint32))):
    ok = False
    print("row e: the frame's hit buffers differ from row a", flush=True)
ra.close()

# f: the quick tree
rf = make({"RT_ACCEL_DEFER": "1"}, finish=False)
compare("f", visibility_row("f", "visibility_device on the quick tree (RT_ACCEL_DEFER=1)", rf), a)
rf.close()

L = lines
print(json.dumps({"equal": ok,
                  "a_range_below_d_range": L["a"]["ms_max"] < L["d"]["ms_min"],
                  "a_range_below_e_range": L["a"]["ms_max"] < L["e"]["ms_min"],
                  "d_over_a_medians": round(L["d"]["ms_median"] / L["a"]["ms_median"], 2),
                  "e_over_a_medians": round(L["e"]["ms_median"] / L["a"]["ms_median"], 2)}), flush=True)
sys.exit(0 if ok else 1)
