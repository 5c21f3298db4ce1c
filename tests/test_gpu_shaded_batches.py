"""Shaded ray batches through the frame engine (rt_trace_ray_batch_device, rt_get_device_shaded_batches; kernels.hip
refl_rays_level0_kernel).

On a scene with a reflective material trace_ray_batch_device must write, per ray, what trace_ray_device (the
per-lane recursion, pinned to rt_trace_ray and the oracle by tests/test_gpu_shaded_queries.py) writes for that ray
in the same renderer state: sources, t, both flags and the counts bit for bit, the colour within RGBA_TOL of the
oracle's and, for a frame's camera rays, bit for bit the float RGBA of an engine frame of the same renderer.  On
any other scene the call is trace_ray_device's code, and the bytes are its bytes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle.bindings import Oracle
from raytracercpp_amd import _lib
from test_gpu_octree_build import bits, frame, make_renderer  # noqa: F401
from test_gpu_shaded_queries import DTYPES, KEYS, _guarded, case, gpu, host, random_rays, same, zeros2
from test_trace_ray import RGBA_TOL, camera_rays

pytestmark = pytest.mark.gpu

BLOCK = 256   # lanes per block of refl_rays_level0_kernel: 64 * WAVES_PER_BLOCK (kernels.hip:57)
NRANDOM = 2000
FILL = (np.array([0, 0, 0, 1], np.float32), -1, -1.0, 0, 0)   # what trace_ray returns past max_recursion_depth


def batch(r, o, d, depth=0, **kw):
    """trace_ray_batch_device on the current stream, its outputs on the host."""
    return host(r.trace_ray_batch_device(gpu(o), gpu(d), depth, **kw))


def single(r, o, d, depth=0, **kw):
    return host(r.trace_ray_device(gpu(o), gpu(d), depth, **kw))


def same_bytes(got, ref, what):
    same(got, ref, what, rgba=True)


@pytest.fixture(scope="module")
def R():
    from raytracercpp_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


_rays = {}


def rays_of(name):
    """The case's camera rays followed by NRANDOM of random_rays, made once."""
    if name not in _rays:
        c = case(name)
        oc, dc = camera_rays(c.scene, c.settings)
        orr, drr = random_rays(c, NRANDOM)
        o, d = np.concatenate([oc, orr]), np.concatenate([dc, drr])
        _rays[name] = (c, o, d, len(oc))
    return _rays[name]


def moved(r, before):
    """(batches' calls, batches' rays, shaded queries' calls) since ``before`` = counters(r)."""
    now = counters(r)
    return tuple(tuple(int(x) - int(y) for x, y in zip(a, b)) for a, b in zip(now, before))


def counters(r):
    bc, br = r.device_shaded_batches()
    qc, _ = r.device_shaded_queries()
    return bc, br, qc


# ---- 1. equality with rt_trace_ray_device -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["mirror", "rough"])
def test_equals_trace_ray_device(R, name):
    c, o, d, _ = rays_of(name)
    R.load_scene(c.scene, c.settings)
    orc = Oracle(c.scene, c.settings)
    od, dd = gpu(o), gpu(d)
    n, limit = len(o), c.settings.max_recursion_depth
    for depth in (0, 1, limit, limit + 1):
        cref, cgot = zeros2(), zeros2()
        ref = host(R.trace_ray_device(od, dd, depth, counts=cref))
        before = counters(R)
        got = host(R.trace_ray_batch_device(od, dd, depth, counts=cgot))
        same(got, ref, f"{name}, depth {depth}", rgba=False)
        assert cgot.tolist() == cref.tolist(), f"{name}, depth {depth}: counts {cgot.tolist()} against {cref.tolist()}"
        e = orc.trace_ray(o, d, depth)
        err = float(np.abs(got[0] - e[0]).max())
        nbits = int((bits(got[0]) != bits(ref[0])).any(axis=-1).sum())
        print(f"{name}, depth {depth}: counts {cgot.tolist()}; max |RGBA - oracle| {err:.3g}; the colours of {nbits} of "
              f"{n} rays differ from rt_trace_ray_device's in their bits")
        assert np.array_equal(got[1], e[1]) and np.array_equal(bits(got[2]), bits(e[2]))
        assert cgot.tolist() == [e[5]["shadow_rays"], e[5]["reflection_rays"]]
        assert err <= RGBA_TOL, f"{name}, depth {depth}"
        if depth > limit:
            assert moved(R, before) == ((0, 0), (0, 0), (0, 0, 0)), "the fill past the limit counts nowhere"
            for a, v in zip(got, FILL):
                assert np.all(a == v)
        else:
            assert moved(R, before) == ((1, 0), (n, 0), (0, 0, 0)), "an engine-routed call moves slot 0 only"


# ---- 2. camera rays against a frame ------------------------------------------------------------------------

def test_camera_rays_equal_an_engine_frame(R):
    c, o, d, ncam = rays_of("rough")
    R.load_scene(c.scene, c.settings)
    fr = frame(R)
    got = batch(R, o[:ncam], d[:ncam])
    nframe = int((bits(got[0]) != bits(fr["rgba"].reshape(-1, 4))).any(axis=-1).sum())
    assert nframe == 0, f"the colours of {nframe} of {ncam} camera rays differ from the frame's float RGBA"
    assert np.array_equal(np.where(got[3] == 1, got[1], -1), fr["hit_id"].ravel())
    assert np.array_equal(bits(got[2]), bits(fr["hit_t"].ravel()))
    assert np.array_equal(got[4], fr["shadow"].ravel())
    assert got[3].any() and not got[3].all() and got[4].any()


# ---- 3. sizes around a wave and a block ----------------------------------------------------------------------

_size_ref = {}


@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_sizes(R, n):
    c = case("rough")
    R.load_scene(c.scene, c.settings)
    if not _size_ref:
        o, d = random_rays(c, BLOCK + 1)
        _size_ref["rays"] = (o, d, batch(R, o, d))
    o, d, ref = _size_ref["rays"]
    out = _guarded(n)
    counts, cref = zeros2(), zeros2()
    od, dd = gpu(o[:n]), gpu(d[:n])
    ret = R.trace_ray_batch_device(od, dd, out=out, counts=counts)
    assert ret is out
    got = host(out)
    same_bytes(tuple(a[:n] for a in got), tuple(a[:n] for a in ref), f"n = {n}: the first n of a larger call")
    for k, a in zip(KEYS, got):
        assert np.all(a[n:] == 77), f"n = {n}: {k} was written past n"
    R.trace_ray_device(od, dd, counts=cref)
    assert counts.tolist() == cref.tolist()
    if n >= 63:   # (the first ray alone misses the scene)
        assert int(counts[0]) > 0 and int(counts[1]) > 0


# ---- 4. several batches and several chunks -------------------------------------------------------------------

def test_batches_and_chunks(R, make_renderer):
    c = case("rough")
    n = 2500
    o, d = random_rays(c, n, seed=5)
    R.load_scene(c.scene, c.settings)
    cref = zeros2()
    ref = batch(R, o, d, counts=cref)
    small = make_renderer(RT_SHADE_BATCH_LOG2=10, RT_REFL_CHUNK_LOG2=10)   # three batches, the last one of 452 rays
    small.load_scene(c.scene, c.settings)
    cgot = zeros2()
    same_bytes(batch(small, o, d, counts=cgot), ref, "batches of 2^10 rays and chunks of 2^10 slots")
    assert cgot.tolist() == cref.tolist()
    assert small.device_shaded_batches() == ((1, 0), (n, 0))
    # the same rays split by the caller, first_ray continued
    for r in (R, small):
        od, dd = gpu(o), gpu(d)
        out = {k: torch.zeros((n, 4) if k == "rgba" else (n,), dtype=dt, device="cuda") for k, dt in zip(KEYS, DTYPES)}
        counts = zeros2()
        cut = 1100
        r.trace_ray_batch_device(od[:cut].contiguous(), dd[:cut].contiguous(), first_ray=0,
                                 out={k: t[:cut] for k, t in out.items()}, counts=counts)
        r.trace_ray_batch_device(od[cut:].contiguous(), dd[cut:].contiguous(), first_ray=cut,
                                 out={k: t[cut:] for k, t in out.items()}, counts=counts)
        same_bytes(host(out), ref, "two calls with first_ray 0 and 1100")
        assert counts.tolist() == cref.tolist()
    # first_ray keys the rough streams: other samples on rough, the same colours on a mirror
    keyed = batch(small, o, d, first_ray=7)
    same(keyed, ref, "rough, first_ray 7", rgba=False)
    changed = int((bits(keyed[0]) != bits(ref[0])).any(axis=-1).sum())
    print(f"rough, first_ray 7: the colours of {changed} of {n} rays change")
    assert changed > 0
    m = case("mirror")
    om, dm = random_rays(m, n, seed=5)
    small.load_scene(m.scene, m.settings)
    same_bytes(batch(small, om, dm, first_ray=7), batch(small, om, dm, first_ray=0), "mirror, first_ray 7 against 0")


# ---- 5. optional outputs ---------------------------------------------------------------------------------------

def test_optional_outputs(R):
    c = case("rough")
    R.load_scene(c.scene, c.settings)
    n = 1000
    o, d = random_rays(c, n)
    od, dd = gpu(o), gpu(d)
    full = dict(zip(KEYS, host(R.trace_ray_batch_device(od, dd))))
    for leave in [(k,) for k in KEYS[1:]] + [KEYS[1:]]:
        out = {k: t for k, t in _guarded(n).items() if k not in leave}
        ret = R.trace_ray_batch_device(od, dd, out=out)   # (and no counts)
        assert ret is out and set(ret) == set(KEYS) - set(leave) and "rgba" in ret
        for k in out:
            a = out[k].cpu().numpy()
            assert np.array_equal(bits(a[:n]) if a.dtype == np.float32 else a[:n],
                                  bits(full[k]) if a.dtype == np.float32 else full[k]), f"{k} without {leave}"
            assert np.all(a[n:] == 77)


# ---- 6. delegation ---------------------------------------------------------------------------------------------

DELEGATED = {
    # name: (case, environment, settings changed)
    "textured": ("textured", {}, {}),
    "c3_bumpy70k": ("c3_bumpy70k", {}, {}),
    "RT_REFL_ENGINE=0": ("rough", dict(RT_REFL_ENGINE=0), {}),
    "enable_bvh=0": ("rough", {}, dict(enable_bvh=False)),
}


@pytest.mark.parametrize("which", list(DELEGATED))
def test_delegation(make_renderer, which):
    name, env, change = DELEGATED[which]
    c = case(name)
    st = c.settings.copy(**change) if change else c.settings
    r = make_renderer(**env)
    r.load_scene(c.scene, st)
    r.ray_trace()
    r.finish_accel()   # (the tree is settled: the same instance of rt_trace_ray_device's kernel runs every time)
    n = NRANDOM
    o, d = random_rays(c, n)
    cref, cgot = zeros2(), zeros2()
    ref = single(r, o, d, counts=cref)
    before = counters(r)
    got = batch(r, o, d, counts=cgot)
    same_bytes(got, ref, f"{which}: rt_trace_ray_device's bytes")
    assert cgot.tolist() == cref.tolist()
    bc, br, qc = moved(r, before)
    assert (bc, br) == ((0, 1), (0, n)), f"{which}: a delegated call moves slot 1"
    assert sorted(qc) == [0, 0, 1], f"{which}: rt_trace_ray_device's own counters move, in one instance: {qc}"
    # the instance that ran is the one rt_trace_ray_device itself runs
    again = counters(r)
    single(r, o, d)
    assert moved(r, again)[2] == qc
    # a call past the depth limit and an empty call move nothing
    again = counters(r)
    past = batch(r, o, d, st.max_recursion_depth + 1)
    for a, v in zip(past, FILL):
        assert np.all(a == v)
    e = torch.zeros((0, 3), device="cuda")
    assert r.trace_ray_batch_device(e, e.clone())["rgba"].shape == (0, 4)
    assert moved(r, again) == ((0, 0), (0, 0), (0, 0, 0))


def test_empty_call_launches_nothing(R):
    c = case("rough")
    R.load_scene(c.scene, c.settings)
    out = _guarded(0, 5)
    counts = torch.full((2,), 5, dtype=torch.int64, device="cuda")
    before = counters(R)
    e = torch.zeros((0, 3), device="cuda")
    R.trace_ray_batch_device(e, e.clone(), out=out, counts=counts)
    torch.cuda.synchronize()
    assert moved(R, before) == ((0, 0), (0, 0), (0, 0, 0))
    assert all(bool((out[k] == 77).all()) for k in KEYS) and bool((counts == 5).all())
    # (the pointers are not read: null ones pass with n == 0)
    assert _lib.lib().rt_trace_ray_batch_device(R._h, None, None, 0, 0, 0, None, None, None, None, None, None, None) == 0
    assert moved(R, before) == ((0, 0), (0, 0), (0, 0, 0))


# ---- 7. C5 small -----------------------------------------------------------------------------------------------

def test_c5_small_matches_oracle(make_renderer):
    """C5's features (rough reflections, normal and parallax maps, 1 M triangles) at a reduced size: the 64 x 36 case
    at depth 3 that tests/test_gpu_frames.py renders.  It renders at SSAA 2, so its camera rays are the 128 x 72
    internal image's, 9,216 of them."""
    from raytracercpp_amd import scenes
    sc, st = scenes.sphere1m_refl(width=64, height=36, samples=4)
    st = st.copy(max_recursion_depth=3)
    o, d = camera_rays(sc, st)
    n = len(o)
    assert n == 4 * 2304
    e = Oracle(sc, st).trace_ray(o, d, 0)
    r = make_renderer()
    r.load_scene(sc, st)
    counts = zeros2()
    got = batch(r, o, d, counts=counts)
    same(got, e[:5], "C5 small against the oracle", rgba=False)
    assert counts.tolist() == [e[5]["shadow_rays"], e[5]["reflection_rays"]]
    err = float(np.abs(got[0] - e[0]).max())
    print(f"C5 small: counts {counts.tolist()}, max |RGBA - oracle| {err:.3g}")
    assert err <= RGBA_TOL
    assert r.device_shaded_batches() == ((1, 0), (n, 0))


# ---- 8. stream order -------------------------------------------------------------------------------------------

def test_stream_order(R):
    """The rays are produced on a side stream behind queued matrix products and overwritten on it right after the
    call; a consumer on that stream reads the outputs.  (This exercises the order; a race could still pass by
    luck.)"""
    c, o, d, _ = rays_of("rough")
    R.load_scene(c.scene, c.settings)
    cref = zeros2()
    ref = batch(R, o, d, counts=cref)
    torch.cuda.synchronize()
    oc, dc = gpu(o), gpu(d)
    a = torch.rand((2048, 2048), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = a
        for _ in range(16):
            b = (b @ a) * (1.0 / 2048)
        ot, dt = oc + 0 * b[0, 0], dc + 0 * b[0, 0]   # (the rays depend on the products)
        counts = zeros2()
        out = R.trace_ray_batch_device(ot, dt, counts=counts, stream=side)
        ot.fill_(float("nan"))
        dt.fill_(float("nan"))
        seen = {k: v.clone() for k, v in out.items()}
        seen_counts = counts.clone()
    side.synchronize()
    assert bool(torch.isfinite(b).all())
    same_bytes(host(seen), ref, "the consumer on the side stream")
    assert seen_counts.tolist() == cref.tolist()
    torch.cuda.synchronize()


# ---- 9. around band launches -----------------------------------------------------------------------------------

def test_band_launch_then_a_batch(make_renderer):
    c, o, d, _ = rays_of("rough")
    st = c.settings
    r = make_renderer()
    r.load_scene(c.scene, st)
    r.ray_trace()
    r.finish_accel()
    W, rows = st.image_width, r.local_rows(8, 0, 1)
    alone = torch.zeros((rows, W), dtype=torch.int32, device="cuda")
    for _ in range(2):   # (the second launch has its heavy list, as the one below)
        r.render_bands_device(8, 0, 1, alone.data_ptr(), 0)
        torch.cuda.synchronize()
    want_counters = r.band_counters()
    cref = zeros2()
    ref = batch(r, o, d, counts=cref)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    img = torch.zeros((rows, W), dtype=torch.int32, device="cuda")
    od, dd = gpu(o), gpu(d)
    torch.cuda.synchronize()
    r.render_bands_device(8, 0, 1, img.data_ptr(), sa.cuda_stream)
    stats = r.stats()
    counts = zeros2()
    with torch.cuda.stream(sb):
        out = r.trace_ray_batch_device(od, dd, counts=counts, stream=sb)
    assert r.stats() == stats, "rt_get_stats reports what it reported before the batch"
    assert r.band_counters() == want_counters, "the frame's counters hold the frame's counts alone"
    torch.cuda.synchronize()
    assert torch.equal(img, alone), "the image equals an undisturbed frame"
    same_bytes(host(out), ref, "the batch behind the band launch")
    assert counts.tolist() == cref.tolist()
    # and a band launch behind the batch
    img.zero_()
    with torch.cuda.stream(sb):
        out = r.trace_ray_batch_device(od, dd, stream=sb)
    r.render_bands_device(8, 0, 1, img.data_ptr(), sa.cuda_stream)
    torch.cuda.synchronize()
    assert r.band_counters() == want_counters and torch.equal(img, alone)
    same_bytes(host(out), ref, "the batch in front of the band launch")


# ---- 10. scene changes and close() right behind a call ---------------------------------------------------------

def _reflective_textured():
    """diffuse_map_skysphere with every material a rough mirror: the engine's passes read a texture and the sky."""
    c = case("diffuse_map_skysphere")
    m = np.array(c.scene.materials, np.float32).reshape(-1, 16).copy()
    m[:, 12] = 0.5    # reflection
    m[:, 13] = 0.25   # roughness
    return dataclasses.replace(c.scene, materials=m), c.settings.copy(max_recursion_depth=2)


def _changed(sc, what):
    if what == "materials":
        m = np.array(sc.materials, np.float32).reshape(-1, 16).copy()
        m[:, :9] = m[:, :9][:, ::-1] * 0.5 + 0.125   # the ambient, diffuse and specular colours
        return dataclasses.replace(sc, materials=m), lambda r: r.set_materials(m)
    if what == "texture":
        slot = sorted(sc.textures)[0]
        img = np.ascontiguousarray(np.asarray(sc.textures[slot], np.float32)[::-1]) * np.float32(0.5)
        tex = dict(sc.textures)
        tex[slot] = img
        return dataclasses.replace(sc, textures=tex), lambda r: r._set_tex(slot, img)
    assert what == "geometry"
    tri = (np.asarray(sc.tri, np.float32).reshape(-1, 3) * np.float32(0.75) + np.array([0.1, -0.05, 0.0], np.float32))
    tri = tri.reshape(-1, 9).astype(np.float32)
    return dataclasses.replace(sc, tri=tri), lambda r: r.set_triangles(tri, sc.tri_mat, sc.tri_uv)


@pytest.mark.parametrize("what", ["materials", "texture", "geometry", "close"])
def test_scene_changes_and_close_wait_for_batches(make_renderer, what):
    sc, st = _reflective_textured()
    n = 1 << 16
    o, d = random_rays(case("diffuse_map_skysphere"), n, seed=3)
    od, dd = gpu(o), gpu(d)
    r = make_renderer()
    r.load_scene(sc, st)
    old = host(r.trace_ray_batch_device(od, dd))
    assert r.device_shaded_batches() == ((1, 0), (n, 0))
    same(old, single(r, o, d), "the reflective textured scene", rgba=False)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    if what == "close":
        from raytracercpp_amd.renderer import Renderer
        r3 = Renderer(0)
        r3.load_scene(sc, st)
        out3 = r3.trace_ray_batch_device(od, dd, stream=side)
        r3.close()
        side.synchronize()
        torch.cuda.synchronize()
        same_bytes(host(out3), old, "the batch in flight at close()")
        return
    new_scene, apply = _changed(sc, what)
    fresh = make_renderer()
    fresh.load_scene(new_scene, st)
    want = host(fresh.trace_ray_batch_device(od, dd))
    assert (bits(want[0]) != bits(old[0])).any(), "the change is visible in the colours"
    out = r.trace_ray_batch_device(od, dd, stream=side)
    # no wait: the scene is changed and asked again while the first call's last pass may still run
    apply(r)
    out2 = r.trace_ray_batch_device(od, dd)
    side.synchronize()
    same_bytes(host(out), old, f"the batch in flight while the {what} changed")
    same_bytes(host(out2), want, f"the batch after the {what} changed")


# ---- 11. refusals ----------------------------------------------------------------------------------------------

def _raw(r, p, n, depth=0, first=0):
    v = [C.c_void_p(x) for x in p]
    return _lib.lib().rt_trace_ray_batch_device(r._h, v[0], v[1], n, depth, first, v[2], v[3], v[4], v[5], v[6], v[7], None)


def test_refusals(R):
    c = case("rough")
    R.load_scene(c.scene, c.settings)
    n = 64
    o, d = random_rays(c, n)
    ref = batch(R, o, d)
    good = [gpu(o), gpu(d)] + [t[:n] for t in _guarded(n, 0).values()] + \
           [torch.full((2,), 5, dtype=torch.int64, device="cuda")]
    host_arrays = [np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32),
                   np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8),
                   np.zeros(2, np.int64)]
    pinned = [torch.from_numpy(a.copy()).pin_memory() for a in host_arrays]
    before = counters(R)

    def unchanged():
        torch.cuda.synchronize()
        assert moved(R, before) == ((0, 0), (0, 0), (0, 0, 0))
        assert all(bool((t == 77).all()) for t in good[2:7]) and bool((good[7] == 5).all())

    ptrs = [t.data_ptr() for t in good]
    for i in range(8):
        for what, bad in (("host", host_arrays[i].ctypes.data), ("pinned", pinned[i].data_ptr())):
            p = list(ptrs)
            p[i] = bad
            if i == 2 and bad % 16:
                continue   # (an unaligned host d_rgba is refused for its alignment: below)
            rc = _raw(R, p, n)
            assert rc == -1, f"argument {i} in {what} memory: {rc}"   # RT_EINVAL
            unchanged()
    if torch.cuda.device_count() > 1:
        for i in range(8):
            p = list(ptrs)
            other = torch.zeros(4 * n, dtype=torch.float32, device="cuda:1")
            p[i] = other.data_ptr()
            assert _raw(R, p, n) == -1, f"argument {i} in another device's memory"
            unchanged()
    # a null d_orig / d_dir / d_rgba with n > 0 (the other outputs and the counts may be null)
    for i in range(3):
        p = list(ptrs)
        p[i] = None
        assert _raw(R, p, n) == -1
        unchanged()
    # d_rgba not 16-byte aligned
    wide = torch.full((4 * n + 4,), 77, dtype=torch.float32, device="cuda")
    for off in (1, 2, 3):
        p = list(ptrs)
        p[2] = wide.data_ptr() + 4 * off
        assert _raw(R, p, n) == -1 and b"16-byte aligned" in _lib.lib().rt_last_error()
        torch.cuda.synchronize()
        assert bool((wide == 77).all())
    unchanged()
    # counts, depths and first rays out of range
    for bad_n in ((1 << 30) + 1, -1, 1 << 40):
        assert _raw(R, ptrs, bad_n) == -1
    assert _raw(R, ptrs, n, depth=-1) == -1
    for first in (-1, (1 << 32) - n + 1, 1 << 32, 1 << 40, (1 << 63) - 1, (1 << 63) - n, (1 << 63) - n + 1, -(1 << 63)):
        assert _raw(R, ptrs, n, first=first) == -1, first
    assert _raw(R, ptrs, 1 << 30, first=(1 << 32) - (1 << 30) + 1) == -1
    unchanged()
    with pytest.raises(_lib.RtError):
        R.trace_ray_batch_device(good[0], good[1], -1)
    with pytest.raises(_lib.RtError):
        R.trace_ray_batch_device(good[0], good[1], first_ray=-1)
    with pytest.raises(ValueError, match="not on a GPU"):
        R.trace_ray_batch_device(pinned[0], pinned[1])
    with pytest.raises(ValueError, match="out: rgba is needed"):
        R.trace_ray_batch_device(good[0], good[1], out=dict(t=good[4]))
    unchanged()
    # the largest first_ray, and the good arguments, pass
    cref = zeros2()   # (what the recursive call counts for the same two keyings)
    R.trace_ray_device(good[0], good[1], first_ray=(1 << 32) - n, counts=cref)
    R.trace_ray_device(good[0], good[1], counts=cref)
    assert _raw(R, ptrs, n, first=(1 << 32) - n) == 0
    assert _raw(R, ptrs, n) == 0
    same_bytes(host(dict(zip(KEYS, good[2:7]))), ref, "after the refusals")
    assert good[7].tolist() == [5 + int(x) for x in cref.tolist()], "the two good calls added their counts"


def test_invalid_scene_is_refused_as_by_trace_ray_device(make_renderer):
    """An enabled map that is missing, and reflective materials with max_recursion_depth > 15: validate()'s and
    check_frame()'s codes, and no launch."""
    sc, st = _reflective_textured()
    r = make_renderer()
    r.load_scene(sc, st)
    r._set_tex(sorted(sc.textures)[0], None)
    o, d = random_rays(case("diffuse_map_skysphere"), 64)
    codes = []
    for call in (r.trace_ray_device, r.trace_ray_batch_device):
        with pytest.raises(_lib.RtError) as err:
            call(gpu(o), gpu(d))
        assert "invalid scene" in str(err.value)
        codes.append(err.value.code)
    assert codes == [-1, -1]   # RT_EINVAL
    c = case("rough")
    r.load_scene(c.scene, c.settings.copy(max_recursion_depth=16))
    codes = []
    for call in (r.trace_ray_device, r.trace_ray_batch_device):
        with pytest.raises(_lib.RtError) as err:
            call(gpu(o), gpu(d))
        codes.append(err.value.code)
    assert codes[0] == codes[1] and "max_recursion_depth > 15" in str(err.value)
    assert counters(r) == ((0, 0), (0, 0), (0, 0, 0))
