"""Closest-hit and shadow queries for rays that lie in GPU memory, on the C4 scene (sphere1m, default BVH
settings) after rt_finish_accel, 2^22 rays per set, made on the GPU from a seed:
  a  camera rays: from the camera position through uniformly random points of the 1920 x 1080 frame
  b  uniformly random origins in the scene's box, uniformly random directions
  c  shadow pairs: the hit points of (a) with their triangles' geometric normals (towards the camera)
Rows, all in one process:
  host           Renderer.trace_rays from numpy arrays (the copy to numpy is outside the timed part; the
                 upload, the download and the host wait are inside it: they are part of that call)
  device_octree  trace_rays_device / is_shadowed_device of a second renderer created with RT_WBVH=0
  device         the same calls of the default renderer
Shaded rows on sets (a) and (b), likewise (rt_trace_ray / rt_trace_ray_device):
  host            Renderer.trace_ray from numpy arrays
  device_generic  trace_ray_device of a renderer created with RT_SHADE_PLAIN=0 (the generic instance)
  device          trace_ray_device of the default renderer (C4 is a plain scene: the plain instance)
and, on C5's settings (sphere1m_refl: rough reflections, 16 samples, depth 5), 2^18 camera rays of set (a): host
against device (the reflective instance, the per-lane recursion).  Their counts are the call's shadow and
reflection rays.
Batch rows (rt_trace_ray_batch_device, the frame engine), one per shaded ray set, against the device row run in
the same call:
  batch           trace_ray_batch_device of the default renderer (C4 has no reflective material: the call is
                  trace_ray_device's code there)
On C5's settings the same 2^18 camera rays (section c5: device and batch alone, without the host row), then the
sweep (section sweep): 2^10, 2^14 and 2^22 of set (a)'s rays on C5's settings (the device row only up to 2^14 and
with 3 repetitions where one call takes more than 5 s: 2^22 rays would take it minutes per call), and 2^10 ...
2^22 rays on the mirror golden's settings (roughness 0: one sample per hit, depth 5, no maps) over the same
geometry, both rows.  A batch row must agree with its device row in sources, t, flags and counts bit for bit and
in RGBA within RGBA_TOL; the rays whose RGBA bits differ are counted, and each pair of rows reports the ratio of
the medians and whether the batch row's whole range lies below the device row's.  The shaded rows of one set must agree in sources, t and flags bit for bit and in RGBA within
RGBA_TOL (the plain instance shades through the frames' expressions), and the counts must be the host row's.
Each call is timed with a torch.cuda.Event pair on the call's stream, after a warm-up of the same shape;
the median and the range of the repetitions are reported, with Mrays/s from the median and the counts
trace_rays_device adds up (rays answered by the wide query, rays traced through the octree).  The outputs
of all rows of one set must be equal bit for bit, else the tool exits with status 1.  Rows whose calls the
loaded library lacks are skipped (RT_LIB_PATH naming an older build: the host row alone).
Usage: python tools/ray_query_time.py [repetitions [log2 rays [sections]]]
sections: a comma list of c4 (sets a, b, c), c5host (C5 with the host row), c5, sweep; default all of them."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracercpp_amd import _lib, scenes
from raytracercpp_amd.renderer import Renderer, render

reps = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 10
n = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 22)
SECTIONS = ("c4", "c5host", "c5", "sweep")
sections = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else SECTIONS
if set(sections) - set(SECTIONS):
    sys.exit("sections: a comma list of " + ", ".join(SECTIONS))
KEYS = ("tri_id", "t", "u", "v", "ret")
SHADE_KEYS = ("rgba", "hit_src", "t", "intersection_found", "shadowed")
RGBA_TOL = 1e-4   # the project's (tests/test_trace_ray.py)
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


def rays_box():
    v = torch.from_numpy(sc.tri.reshape(-1, 3)).to(dev)
    lo, hi = v.min(0).values, v.max(0).values
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


def timed(call, reps=reps, slow_ms=None, slow_reps=3):
    """The call's results and its durations in ms (one warm-up, then `reps` repetitions between event pairs;
    slow_ms: `slow_reps` repetitions when the warm-up took longer than that)."""
    t0 = time.perf_counter()
    res = call()
    torch.cuda.synchronize()
    if slow_ms is not None and (time.perf_counter() - t0) * 1e3 > slow_ms:
        reps = slow_reps
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return res, ms


def report(ray_set, row, count, ms, counts=None):
    med = statistics.median(ms)
    rate = count / med / 1e3   # (one decimal, or four digits of a rate below 100: the C5 rows run at 0.016)
    line = {"set": ray_set, "row": row, "rays": count, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "reps": len(ms), "mrays_per_s": round(rate, 1) if rate >= 100 else float("%.4g" % rate)}
    if counts is not None:
        line["counts"] = counts
    print(json.dumps(line), flush=True)
    return line


def make(env=None, scene=None):
    sc, st = scene or (globals()["sc"], globals()["st"])
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        r = Renderer(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    r.load_scene(sc, st)
    render(r)
    r.finish_accel()
    render(r)
    return r


def as_bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


have = all(_lib.has(s) for s in _lib.RAY_QUERIES) if hasattr(_lib, "RAY_QUERIES") else False
if not have:
    print("device, device_octree: skipped (the library lacks the device ray queries)", flush=True)
have_shaded = have and all(_lib.has(s) for s in getattr(_lib, "SHADED_QUERIES", ("missing",)))
have_batches = have_shaded and all(_lib.has(s) for s in getattr(_lib, "SHADED_BATCHES", ("missing",)))
renderers = {}
if "c4" in sections:
    renderers["device"] = make()
    if have:
        renderers["device_octree"] = make({"RT_WBVH": "0"})
    if have_shaded:
        renderers["device_generic"] = make({"RT_SHADE_PLAIN": "0"})
    else:
        print("shaded rows: skipped (the library lacks the shaded device query)", flush=True)
    if not have_batches:
        print("batch rows: skipped (the library lacks the shaded batches)", flush=True)
    print(json.dumps({"scene": "sphere1m", "triangles": int(sc.ntri), "rays_per_set": n, "repetitions": reps,
                      "wide_tree": {k: r.stats()["wide_tree"] for k, r in renderers.items()}}), flush=True)


def batch_rows(ray_set, r, o, d, device=True, ref=None, slow_ms=None):
    """The device row (trace_ray_device; device False: none, the batch row alone) and the batch row
    (trace_ray_batch_device) of renderer r over one ray set, compared with each other (ref: the device row's
    outputs and counts when shaded_rows has run it already; slow_ms: the device row takes 3 repetitions when
    one call takes longer than that)."""
    global ok
    count = int(o.shape[0])
    new = lambda: {k: torch.empty((count, 4) if k == "rgba" else count, dtype=dt, device=dev)   # noqa: E731
                   for k, dt in zip(SHADE_KEYS, (torch.float32, torch.int32, torch.float32, torch.uint8, torch.uint8))}
    dms = None
    if device and ref is None:
        out, counts = new(), torch.zeros(2, dtype=torch.int64, device=dev)
        _, dms = timed(lambda: r.trace_ray_device(o, d, out=out, counts=counts), slow_ms=slow_ms)
        ref = (out, [int(x) // (len(dms) + 1) for x in counts.cpu()], dms)
        lines.append(report(ray_set, "shaded device", count, dms, ref[1]))
    elif ref is not None:
        dms = ref[2]
    out, counts = new(), torch.zeros(2, dtype=torch.int64, device=dev)
    before = r.device_shaded_batches()
    _, ms = timed(lambda: r.trace_ray_batch_device(o, d, out=out, counts=counts))
    c = [int(x) // (len(ms) + 1) for x in counts.cpu()]
    lines.append(report(ray_set, "shaded batch", count, ms, c))
    after = r.device_shaded_batches()
    note = {"set": ray_set, "row": "shaded batch",
            "calls_engine_delegated": [b - a for a, b in zip(before[0], after[0])]}
    if ref is not None:
        err = float((out["rgba"] - ref[0]["rgba"]).abs().max())
        note["max_abs_rgba_diff_from_device"] = err
        note["rays_whose_rgba_bits_differ_from_device"] = int(
            (out["rgba"].view(torch.int32) != ref[0]["rgba"].view(torch.int32)).any(1).sum())
        note["device_over_batch_medians"] = round(statistics.median(dms) / statistics.median(ms), 2)
        note["batch_range_below_device_range"] = max(ms) < min(dms)
        if c != ref[1]:
            ok = False
            print(f"set {ray_set}, row shaded batch: counts {c}, the device row's {ref[1]}", flush=True)
        if not err <= RGBA_TOL:
            ok = False
            print(f"set {ray_set}, row shaded batch: RGBA differs from the device row by {err}", flush=True)
        for k in SHADE_KEYS[1:]:
            if not torch.equal(as_bits(out[k]), as_bits(ref[0][k])):
                ok = False
                print(f"set {ray_set}, row shaded batch: {k} differs from the device row in "
                      f"{int((as_bits(out[k]) != as_bits(ref[0][k])).sum())} rays", flush=True)
    print(json.dumps(note), flush=True)


def shaded_rows(ray_set, rows, o, d):
    """The shaded rows of one ray set: rows = [(name, renderer)], the host row from the first renderer."""
    global ok
    count = int(o.shape[0])
    oh, dh = o.cpu().numpy(), d.cpu().numpy()
    torch.cuda.synchronize()
    host = rows[0][1]
    ref, ms = timed(lambda: host.trace_ray(oh, dh, 0))
    hs = host.stats()
    want = [hs["shadow_rays"], hs["reflection_rays"]]
    lines.append(report(ray_set, "shaded host", count, ms, want))
    ref = [torch.from_numpy(a).to(dev) for a in ref]
    last = None
    for row, r in rows:
        out = {k: torch.empty_like(a) for k, a in zip(SHADE_KEYS, ref)}
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        calls0 = r.device_shaded_queries()[0]
        _, ms = timed(lambda: r.trace_ray_device(o, d, out=out, counts=counts))
        total = [int(x) for x in counts.cpu()]   # (the warm-up and the repetitions added to it)
        c = [x // (reps + 1) for x in total]
        line = report(ray_set, "shaded " + row, count, ms, c)
        last = (out, c, ms)
        inst = [b - a for a, b in zip(calls0, r.device_shaded_queries()[0])]
        err = float((out["rgba"] - ref[0]).abs().max())
        nbits = int((out["rgba"].view(torch.int32) != ref[0].view(torch.int32)).any(1).sum())
        print(json.dumps({"set": ray_set, "row": "shaded " + row, "launches_plain_generic_reflective": inst,
                          "max_abs_rgba_diff_from_host": err, "rays_whose_rgba_bits_differ_from_host": nbits}), flush=True)
        lines.append(line)
        if total != [w * (reps + 1) for w in want]:
            ok = False
            print(f"set {ray_set}, row shaded {row}: counts {total} over {reps + 1} calls, the host row's {want} per call",
                  flush=True)
        if not err <= RGBA_TOL:
            ok = False
            print(f"set {ray_set}, row shaded {row}: RGBA differs from the host row by {err}", flush=True)
        for k, a in zip(SHADE_KEYS[1:], ref[1:]):
            if not torch.equal(as_bits(out[k]), as_bits(a)):
                ok = False
                print(f"set {ray_set}, row shaded {row}: {k} differs from the host row in "
                      f"{int((as_bits(out[k]) != as_bits(a)).sum())} rays", flush=True)
    if have_batches:   # (the batch row against the last row above, the default renderer's)
        batch_rows(ray_set, rows[-1][1], o, d, ref=last)


ok = True
lines = []
pairs = None
cam_all = None
for ray_set, maker in (("a", rays_camera), ("b", rays_box)):
    o, d = maker()
    if ray_set == "a":
        cam_all = (o, d)
        cam_rays = (o[: 1 << 18].contiguous(), d[: 1 << 18].contiguous())
    if "c4" not in sections:
        continue
    oh, dh = o.cpu().numpy(), d.cpu().numpy()
    torch.cuda.synchronize()
    if have_shaded:
        shaded_rows(ray_set, [("device_generic", renderers["device_generic"]), ("device", renderers["device"])], o, d)
    ref, ms = timed(lambda: renderers["device"].trace_rays(oh, dh))
    lines.append(report(ray_set, "host", n, ms))
    ref = [torch.from_numpy(a).to(dev) for a in ref]
    for row in ("device_octree", "device"):
        if not have:
            continue
        r = renderers[row]
        out = {k: torch.empty(n, dtype=a.dtype, device=dev) for k, a in zip(KEYS, ref)}
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        _, ms = timed(lambda: r.trace_rays_device(o, d, out=out, counts=counts))
        c = [int(x) // (reps + 1) for x in counts.cpu()]
        lines.append(report(ray_set, row, n, ms, c))
        for k, a in zip(KEYS, ref):
            if not torch.equal(as_bits(out[k]), as_bits(a)):
                ok = False
                print(f"set {ray_set}, row {row}: {k} differs from the host row in "
                      f"{int((as_bits(out[k]) != as_bits(a)).sum())} rays", flush=True)
        if ray_set == "a" and row == "device":
            pairs = shadow_pairs(o, d, out)
if pairs is not None:
    p, nrm = pairs
    first = None
    for row in ("device_octree", "device"):
        sh, ms = timed(lambda: renderers[row].is_shadowed_device(p, nrm))
        lines.append(report("c", row, int(p.shape[0]), ms))
        print(json.dumps({"set": "c", "row": row, "shadowed": int(sh.sum())}), flush=True)
        if first is None:
            first = sh.clone()
        elif not torch.equal(first, sh):
            ok = False
            print(f"set c: the rows differ in {int((first != sh).sum())} pairs", flush=True)
for r in renderers.values():
    r.close()
if have_shaded and set(sections) & {"c5host", "c5", "sweep"}:
    r5 = make(scene=scenes.sphere1m_refl())
    print(json.dumps({"scene": "sphere1m_refl", "rays": 1 << 18, "wide_tree": {"device": r5.stats()["wide_tree"]}}), flush=True)
    if "c5host" in sections:
        # C5's settings: the reflective instance (the per-lane recursion) against the host call, then the batch row
        shaded_rows("a, C5 settings", [("device", r5)], *cam_rays)
    elif "c5" in sections and have_batches:
        batch_rows("a, C5 settings", r5, *cam_rays)
    if "sweep" in sections and have_batches:
        for lg in (10, 14, 22):
            if (1 << lg) <= n:
                batch_rows(f"a, C5 settings, 2^{lg} rays", r5, cam_all[0][: 1 << lg].contiguous(),
                           cam_all[1][: 1 << lg].contiguous(), device=lg <= 14, slow_ms=5000.0)
    r5.close()
    if "sweep" in sections and have_batches:
        # the mirror golden's settings over C5's geometry: roughness 0 (one sample per reflective hit), depth 5, no maps
        scm, stm = scenes.sphere1m_refl()
        scm.materials[0, 13] = 0.0
        stm = stm.copy(rough_reflections_sample_count=3, max_recursion_depth=5, enable_normal_mapping=False,
                       enable_displacement_mapping=False)
        rm = make(scene=(scm, stm))
        print(json.dumps({"scene": "sphere1m_refl as a mirror", "wide_tree": {"device": rm.stats()["wide_tree"]}}), flush=True)
        for lg in (10, 14, 18, 22):
            if (1 << lg) <= n:
                batch_rows(f"a, mirror settings, 2^{lg} rays", rm, cam_all[0][: 1 << lg].contiguous(),
                           cam_all[1][: 1 << lg].contiguous())
        rm.close()
print(json.dumps({"equal": ok}), flush=True)
sys.exit(0 if ok else 1)
