"""Ray-segment queries for rays that lie in GPU memory (rt_occluded_device, rt_trace_segments_device) against
what a caller did before them, on the C4 scene (sphere1m, default BVH settings) after rt_finish_accel, 2^22 rays
made on the GPU from tools/ray_query_time.py's seed, all rows in one process:
  set b  uniformly random origins in the scene's box, uniformly random directions (that tool's set (b)), with
         tmax = f x the box's diagonal for f = 1/64, 1/8 and +inf
  rows   closest+compare  trace_rays_device and then the torch expression (ret != 0) & (t < tmax), both inside
                          the timed pair: the detour through the whole-line query
         segments         trace_segments_device
         occluded         occluded_device
Every row of a set must agree with the definition (the expression above over trace_rays_device's outputs) bit
for bit, else the tool exits with status 1.  The bars, against the existing call in the same process:
  f = 1/64, 1/8  the occluded row's whole range lies below the closest+compare row's whole range
  f = +inf       the occluded row's median is no higher than the closest+compare row's maximum
Each is printed with the ratio of the medians; a bar that does not hold is printed as such and the tool goes on.
Informational, no bar: the shadow pairs of that tool's set (c) (the hit points of its camera rays (a) with their
geometric normals) written as segments towards the scene's light (origin p + 1e-4 n, tmax = |L - p|), beside
is_shadowed_device on the pairs; the two are different expressions and their answers are only counted.
Each call is timed with a torch.cuda.Event pair after a warm-up of the same shape; median and range of the
repetitions, Mrays/s from the median, and the counts the kernel adds up per call (wide query, octree walk).
Usage: python tools/segment_query_time.py [repetitions [log2 rays]]"""
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
n = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 22)
KEYS = ("tri_id", "t", "u", "v", "ret")
DTYPES = (torch.int32, torch.float32, torch.float32, torch.float32, torch.uint8)
MISS = (-1, -1.0, 1.0, 0.0, 0)
dev = torch.device("cuda", 0)   # (no GPU: this raises at the first tensor)
gen = torch.Generator(device=dev)
gen.manual_seed(20261020)
sc, st = scenes.sphere1m()


def unit(v):
    return v / v.norm(dim=1, keepdim=True)


def rays_camera():
    ndc = torch.rand((n, 2), generator=gen, device=dev) * 2.0 - 1.0
    p = torch.cat([ndc, -torch.ones((n, 1), device=dev), torch.ones((n, 1), device=dev)], 1)
    pinv = torch.from_numpy(np.asarray(sc.proj_inv, np.float32).reshape(4, 4)).to(dev)
    c2w = torch.from_numpy(np.asarray(sc.cam_to_world, np.float32).reshape(4, 4)).to(dev)
    q = p @ pinv.T
    q = (q / q[:, 3:]) @ c2w.T
    cam = torch.from_numpy(np.asarray(sc.cam_pos, np.float32)).to(dev)
    d = unit(q[:, :3] / q[:, 3:] - cam)
    return cam.repeat(n, 1).contiguous(), d.contiguous()


def box():
    v = torch.from_numpy(sc.tri.reshape(-1, 3)).to(dev)
    return v.min(0).values, v.max(0).values


def rays_box():
    lo, hi = box()
    o = lo + (hi - lo) * torch.rand((n, 3), generator=gen, device=dev)
    d = unit(torch.randn((n, 3), generator=gen, device=dev))
    return o.contiguous(), d.contiguous()


def shadow_pairs(o, d, out):
    hit = out["ret"] != 0
    tri = torch.from_numpy(sc.tri.reshape(-1, 3, 3)).to(dev)[out["tri_id"][hit].long()]
    nrm = unit(torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1))
    nrm = torch.where(((nrm * d[hit]).sum(1, keepdim=True) > 0), -nrm, nrm)
    ok = torch.isfinite(nrm).all(1)   # (the sphere's zero-area pole triangles have no normal)
    p = (o[hit] + d[hit] * out["t"][hit][:, None])[ok]
    return p.contiguous(), nrm[ok].contiguous()


def timed(call):
    """The call's results and its durations in ms (one warm-up, then the repetitions between event pairs)."""
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


def report(ray_set, row, count, ms, counts=None, **more):
    med = statistics.median(ms)
    line = {"set": ray_set, "row": row, "rays": count, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "reps": len(ms), "mrays_per_s": round(count / med / 1e3, 1)}
    if counts is not None:
        line["counts"] = [int(x) // (reps + 1) for x in counts.cpu()]   # (the warm-up and the repetitions added up)
    line.update(more)
    print(json.dumps(line), flush=True)
    return line


def as_bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def new_out(count):
    return {k: torch.empty(count, dtype=dt, device=dev) for k, dt in zip(KEYS, DTYPES)}


r = Renderer(0)
r.load_scene(sc, st)
render(r)
r.finish_accel()
render(r)
print(json.dumps({"scene": "sphere1m", "triangles": int(sc.ntri), "rays": n, "repetitions": reps,
                  "wide_tree": r.stats()["wide_tree"]}), flush=True)
ok = True
bars = True
cam_o, cam_d = rays_camera()   # (drawn first, as tools/ray_query_time.py draws them: set (b) is that tool's)
o, d = rays_box()
lo, hi = box()
diag = float((hi - lo).norm())
for name, f in (("1/64", 1.0 / 64), ("1/8", 1.0 / 8), ("inf", float("inf"))):
    ray_set = f"b, tmax = {name} x diagonal"
    tm = torch.full((n,), f * diag if f != float("inf") else f, dtype=torch.float32, device=dev)
    whole, cw = new_out(n), torch.zeros(2, dtype=torch.int64, device=dev)

    def closest_compare():
        r.trace_rays_device(o, d, out=whole, counts=cw)
        return (whole["ret"] != 0) & (whole["t"] < tm)

    hit, ms_cc = timed(closest_compare)
    report(ray_set, "closest+compare", n, ms_cc, cw, occluded=int(hit.sum()), hits=int((whole["ret"] != 0).sum()))
    seg, cs = new_out(n), torch.zeros(2, dtype=torch.int64, device=dev)
    _, ms_seg = timed(lambda: r.trace_segments_device(o, d, tm, out=seg, counts=cs))
    report(ray_set, "segments", n, ms_seg, cs)
    occ, co = torch.empty(n, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    _, ms_occ = timed(lambda: r.occluded_device(o, d, tm, out=occ, counts=co))
    report(ray_set, "occluded", n, ms_occ, co)
    # the definition, from the whole-line row
    if not torch.equal(occ, hit.to(torch.uint8)):
        ok = False
        print(f"set {ray_set}, row occluded: {int((occ != hit.to(torch.uint8)).sum())} rays differ from the definition", flush=True)
    for k, miss in zip(KEYS, MISS):
        want = hit.to(torch.uint8) if k == "ret" else torch.where(hit, whole[k], torch.full_like(whole[k], miss))
        if not torch.equal(as_bits(seg[k]), as_bits(want)):
            ok = False
            print(f"set {ray_set}, row segments: {k} differs from the definition in "
                  f"{int((as_bits(seg[k]) != as_bits(want)).sum())} rays", flush=True)
    med_cc, med_occ, med_seg = (statistics.median(m) for m in (ms_cc, ms_occ, ms_seg))
    if f != float("inf"):
        holds = max(ms_occ) < min(ms_cc)
        rule = "the occluded row's whole range lies below the closest+compare row's whole range"
    else:
        holds = med_occ <= max(ms_cc)
        rule = "the occluded row's median is no higher than the closest+compare row's maximum"
    bars = bars and holds
    print(json.dumps({"set": ray_set, "bar": rule, "holds": bool(holds),
                      "closest_compare_over_occluded_medians": round(med_cc / med_occ, 3),
                      "closest_compare_over_segments_medians": round(med_cc / med_seg, 3)}), flush=True)

# informational: set (c) as segments beside is_shadowed_device
out_a = new_out(n)
r.trace_rays_device(cam_o, cam_d, out=out_a)
p, nrm = shadow_pairs(cam_o, cam_d, out_a)
L = torch.from_numpy(np.asarray(sc.light, np.float32)).to(dev)
so = (p + nrm * 1.0e-4).contiguous()
sd = unit(L - p).contiguous()
stm = (L - p).norm(dim=1).contiguous()
m = int(p.shape[0])
sh, ms = timed(lambda: r.is_shadowed_device(p, nrm))
report("c", "is_shadowed_device", m, ms, shadowed=int(sh.sum()))
c = torch.zeros(2, dtype=torch.int64, device=dev)
oc, ms = timed(lambda: r.occluded_device(so, sd, stm, counts=c))
report("c as segments", "occluded", m, ms, c, occluded=int(oc.sum()), differ_from_is_shadowed=int((oc != sh).sum()))
r.close()
print(json.dumps({"equal": ok, "bars_hold": bars}), flush=True)
sys.exit(0 if ok else 1)
