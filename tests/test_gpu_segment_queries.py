"""The ray-segment queries on device memory (rt_occluded_device, rt_trace_segments_device,
rt_get_device_segment_queries; kernels.hip segment_rays_kernel).

The definition goes through the call that exists: with (id, t, u, v, ret) what the whole-line query writes for
ray i, hit_i = ret != 0 && t < tmax[i] in float32 (strict, false for a NaN); occluded_device writes hit_i,
trace_segments_device the record where hit_i holds and (-1, -1, 1, 0, 0) elsewhere.  The expected answers are that
expression in numpy over Renderer.trace_rays (trace_rays_kernel: the exact octree walk, pinned to the oracle by
tests/test_gpu_parity.py::test_trace_rays_match_oracle) and, on the finite sets, over the oracle's bvh_query.
The lengths come from one recipe by i % 8 around each ray's own hit, so every set holds rays cut off in front of
their hit, exactly at it, one ulp to either side, and behind it."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_wide as tg
import test_wbvh as tw
from golden_cases import Case
from oracle.bindings import Oracle
from raytracercpp_amd import _lib, scenes
from test_gpu_octree_build import assert_same_frame, bits, frame, make_renderer  # noqa: F401
from test_gpu_parity import _random_rays
from test_gpu_ray_queries import BLOCK, DTYPES, KEYS, N, gpu, host, same, stress
from test_trace_ray import camera_rays

pytestmark = pytest.mark.gpu

F32 = np.float32
SPECIAL = np.array([0.0, -1.0, np.nan, -np.inf, 1e-45, np.finfo(np.float32).max], np.float32)
SETS = ["robot", "robot_nonfinite", "voxels", "grazing", "tiny", "huge", "grazing_plane", "grazing_sphere"]


@pytest.fixture(scope="module")
def R():
    from raytracercpp_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


def hit_pos(ref):
    """The rays that hit with a finite t > 0."""
    return (ref[4] != 0) & np.isfinite(ref[1]) & (ref[1] > 0)


def make_tmax(ref, seed=7):
    """The class recipe: a length per ray by i % 8, around base = the ray's own t where it hit with a finite
    t > 0, else 1."""
    n = len(ref[1])
    rng = np.random.default_rng(seed)
    hp = hit_pos(ref)
    base = np.where(hp, ref[1], F32(1)).astype(np.float32)
    med = F32(np.median(ref[1][hp])) if hp.any() else F32(1)
    pick = SPECIAL[rng.integers(0, len(SPECIAL), n)]
    uni = rng.uniform(0.0, 2.0 * float(med), n).astype(np.float32)
    with np.errstate(over="ignore"):
        by_class = [np.full(n, np.inf, np.float32), F32(0.5) * base, base, np.nextafter(base, F32(np.inf)),
                    np.nextafter(base, F32(0)), F32(2) * base, pick, uni]
    cls = np.arange(n) % 8
    tm = np.choose(cls, by_class).astype(np.float32)
    assert tm.dtype == np.float32
    return tm, cls


def expected(ref, tm):
    """The definition in numpy float32: (occluded bytes, the five segment outputs)."""
    ids, t, u, v, ret = ref
    assert t.dtype == np.float32 and tm.dtype == np.float32
    with np.errstate(invalid="ignore"):
        hit = (ret != 0) & (t < tm)
    seg = (np.where(hit, ids, -1).astype(np.int32), np.where(hit, t, F32(-1)), np.where(hit, u, F32(1)),
           np.where(hit, v, F32(0)), hit.astype(np.uint8))
    return hit.astype(np.uint8), seg


def run_both(r, o, d, tm, counts=None, **kw):
    """Both calls on the current stream, their outputs on the host: (occluded bytes, the five segment outputs)."""
    od, dd = gpu(o), gpu(d)
    td = None if tm is None else gpu(tm)
    occ = r.occluded_device(od, dd, td, counts=None if counts is None else counts[0], **kw)
    seg = r.trace_segments_device(od, dd, td, counts=None if counts is None else counts[1], **kw)
    return occ.cpu().numpy(), host(seg)


def check(got, want, what):
    occ, seg = got
    eocc, eseg = want
    assert occ.dtype == np.uint8 and np.array_equal(occ, eocc), f"{what}: {int((occ != eocc).sum())} occlusion bytes differ"
    same(seg, eseg, what)


def zeros2():
    return torch.zeros(2, dtype=torch.int64, device="cuda")


_refs = {}


def stress_ref(R, name):
    """A stress set, trace_rays' answers to it and the recipe's lengths, computed once; R holds the set's scene."""
    sc, st, o, d = stress(name)
    R.load_scene(sc, st)
    if name not in _refs:
        ref = R.trace_rays(o, d)
        tm, cls = make_tmax(ref)
        for a in ref + (tm, cls):
            a.setflags(write=False)
        _refs[name] = (ref, tm, cls)
    return (sc, st, o, d) + _refs[name]


# ---- 1. the definition on the stress inputs ----------------------------------------------------------------

@pytest.mark.parametrize("name", SETS)
def test_definition_on_stress_inputs(R, name):
    sc, st, o, d, ref, tm, cls = stress_ref(R, name)
    want = expected(ref, tm)
    counts = (zeros2(), zeros2())
    cw = zeros2()
    R.trace_rays_device(gpu(o), gpu(d), counts=cw)
    got = run_both(R, o, d, tm, counts)
    hp = hit_pos(ref)
    with np.errstate(invalid="ignore"):
        beyond = int(((ref[4] != 0) & (ref[1] >= tm)).sum())
    per_class = [int((hp & (cls == c)).sum()) for c in range(8)]
    print(f"{name}: wide_tree {R.stats()['wide_tree']}; {int((ref[4] != 0).sum())} hits, {int(want[0].sum())} occluded, "
          f"{beyond} hit beyond tmax; hit rays per class {per_class}; counts (wide, octree): occluded "
          f"{counts[0].tolist()}, segments {counts[1].tolist()}, trace_rays_device {cw.tolist()}")
    check(got, want, name)
    for c in counts:
        assert int(c.sum()) == N
    # the test cannot pass on misses alone
    assert int(want[0].sum()) >= 600 and beyond >= 800, name
    assert all(per_class[c] >= 150 for c in range(1, 6)), name
    # strictness: a length equal to the hit's t does not occlude, one ulp more does
    assert not want[0][hp & (cls == 2)].any() and want[0][hp & (cls == 3)].all()
    if name != "robot_nonfinite":
        # (for most non-finite rays the oracle names a triangle beside its NaN record: finite sets only)
        oi, ot, ou, ov, orr, _ = Oracle(sc, st).bvh_query(o, d)
        check(got, expected((oi, ot, ou, ov, orr), tm), name + " against the oracle")


# ---- 2. shapes at which indexing goes wrong ----------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_sizes_with_guards(R, n):
    sc, st, o, d, ref, tm, cls = stress_ref(R, "robot_nonfinite")
    pad = 7
    od, dd, td = gpu(o[:n]), gpu(d[:n]), gpu(tm[:n])
    refn = tuple(a[:n] for a in ref)
    for what, t_arg, t_np in (("recipe", td, tm[:n]), ("tmax None", None, np.full(n, np.inf, np.float32)),
                              ("tmax all inf", torch.full((n,), float("inf"), device="cuda"), np.full(n, np.inf, np.float32))):
        eocc, eseg = expected(refn, t_np)
        buf = {k: torch.full((n + 2 * pad,), 77, dtype=dt, device="cuda") for k, dt in zip(KEYS, DTYPES)}
        out = {k: b[pad:pad + n] for k, b in buf.items()}
        obuf = torch.full((n + 2 * pad,), 77, dtype=torch.uint8, device="cuda")
        c0, c1 = zeros2(), zeros2()
        assert R.trace_segments_device(od, dd, t_arg, out=out, counts=c0) is out
        oview = obuf[pad:pad + n]
        assert R.occluded_device(od, dd, t_arg, out=oview, counts=c1) is oview
        same(host(out), eseg, f"n = {n}, {what}")
        assert np.array_equal(oview.cpu().numpy(), eocc), f"n = {n}, {what}"
        for k, b in list(buf.items()) + [("occluded", obuf)]:
            a = b.cpu().numpy()
            assert np.all(a[:pad] == 77) and np.all(a[pad + n:] == 77), f"n = {n}, {what}: {k} was written outside [0, n)"
        assert int(c0.sum()) == n and int(c1.sum()) == n
    # tmax = None is the whole-line query where it returned true
    whole = host(R.trace_rays_device(od, dd))
    same(host(R.trace_segments_device(od, dd)), expected(whole, np.full(n, np.inf, np.float32))[1],
         f"n = {n}: tmax None against trace_rays_device")


# ---- 3. modes ----------------------------------------------------------------------------------------------

MODES = {
    # name: (environment, rt_finish_accel first, the wide tree rt_get_stats names or None, counts[0] > 0)
    "sah_tree": (dict(RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1), True, 2, True),
    "quick_tree": (dict(RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1), False, 1, True),
    "no_wide_tree": (dict(RT_WBVH_QUICK_FIRST=0, RT_ACCEL_HOLD=1, RT_ASYNC_ACCEL=1), False, 0, False),
    "exact": ({}, False, None, False),
    "RT_WBVH=0": (dict(RT_WBVH=0), False, None, False),
    "RT_SEG=0": (dict(RT_SEG=0), False, None, True),
    # (the octree's segment form, off by default: every ray through bvh_closest_seg over [-m, tmax + m])
    "RT_SEG_OCTREE=1 RT_WBVH=0": (dict(RT_SEG_OCTREE=1, RT_WBVH=0), False, None, False),
    "brute_force": ({}, False, None, False),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_modes(R, make_renderer, mode):
    sc, st, o, d, ref, tm, cls = stress_ref(R, "robot")
    env, finish, tree, wide = MODES[mode]
    if mode == "brute_force":
        st = st.copy(enable_bvh=False)
        o, d, tm = o[:2000], d[:2000], tm[:2000]   # (every ray tests every triangle)
    r = make_renderer(**env)
    if mode == "exact":
        r.set_exact(True)
    r.load_scene(sc, st)
    if finish:
        r.occluded_device(gpu(o[:64]), gpu(d[:64]))   # (the first query starts the held build on the quick tree)
        assert r.stats()["wide_tree"] == 1
        r.finish_accel()
    # the definition from this renderer's own whole-line answers; with the tree they are the module renderer's
    own = r.trace_rays(o, d)
    if mode != "brute_force":
        same(own, ref, f"{mode}: trace_rays")
    counts = (zeros2(), zeros2())
    got = run_both(r, o, d, tm, counts)
    if tree is not None:
        assert r.stats()["wide_tree"] == tree
    print(f"{mode}: wide_tree {r.stats()['wide_tree']}; counts (wide, octree): "
          f"occluded {counts[0].tolist()}, segments {counts[1].tolist()}")
    check(got, expected(own, tm), mode)
    for c in counts:
        assert int(c.sum()) == len(o)
        assert (int(c[0]) > 0) == wide, f"{mode}: {c.tolist()}"


@pytest.mark.parametrize("name", ["voxels"])
def test_octree_segment_form(R, make_renderer, name):
    """RT_SEG_OCTREE=1 without the wide query: every ray takes the octree walk over its segment (test_modes does
    the same on the robot).  The switch is off by default because the form assumes that no grazing report falls
    outside its triangle's volumes near a segment's end; the grazing sets are built to
    break that premise and the recipe puts segment ends on their hits, so they are not part of this test: with
    the switch on, 14 of grazing_plane's 20,000 occlusion bytes differ from the definition."""
    sc, st, o, d, ref, tm, cls = stress_ref(R, name)
    r = make_renderer(RT_SEG_OCTREE=1, RT_WBVH=0)
    r.load_scene(sc, st)
    counts = (zeros2(), zeros2())
    check(run_both(r, o, d, tm, counts), expected(ref, tm), name)
    assert counts[0].tolist() == [0, N] and counts[1].tolist() == [0, N]


def test_scene_with_analytic_shapes(R):
    """The shapes are not part of BVH::intersect: the calls equal the definition from trace_rays."""
    c = Case("mirror")
    assert len(c.scene.shape_kind) > 0 and len(c.scene.tri) > 0
    R.load_scene(c.scene, c.settings)
    P = c.scene.tri.reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    rng = np.random.default_rng(11)
    o, d = _random_rays(rng, N, ((lo + hi) / 2).astype(np.float32), float((hi - lo).max()))
    ref = R.trace_rays(o, d)
    tm, cls = make_tmax(ref)
    want = expected(ref, tm)
    counts = (zeros2(), zeros2())
    got = run_both(R, o, d, tm, counts)
    print(f"mirror: {int((ref[4] != 0).sum())} hits, {int(want[0].sum())} occluded; "
          f"counts {counts[0].tolist()} {counts[1].tolist()}")
    assert int(want[0].sum()) >= 600
    check(got, want, "mirror")


# ---- 4. camera-origin rays ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["robot", "plane_0.0001", "plane_0.0"])
def test_camera_rays(R, case):
    """Rays from the camera position read the camera's risk words; the same rays after the camera has moved are
    ordinary rays.  The answers are the same either way and so, on these inputs, are the counts: this shows that
    the path with the risk words is not wrong, not that it was taken (the condition is the kernel's comparison
    of the origin with P.cam_pos, read in kernels.hip)."""
    if case == "robot":
        c = Case("robot")
        sc, st = c.scene, c.settings
        o, d = camera_rays(sc, st)
    else:
        tri, o, d, cam = tw._plane_frame(23, float(case.split("_")[1]))
        sc, st = tg._scene(tri, cam=cam, light=cam + np.float32(7.0))
    R.load_scene(sc, st)
    assert np.array_equal(o, np.repeat(np.asarray(sc.cam_pos, np.float32)[None], len(o), 0))
    ref = R.trace_rays(o, d)
    tm, cls = make_tmax(ref)
    want = expected(ref, tm)
    assert int(want[0].sum()) >= 100 and int(((ref[4] != 0) & (want[0] == 0)).sum()) >= 100
    counts = (zeros2(), zeros2())
    check(run_both(R, o, d, tm, counts), want, f"{case}: camera rays")
    pos, pinv, c2w = R.get_camera_matrices()
    assert np.array_equal(pos, np.asarray(sc.cam_pos, np.float32))
    R.set_camera_matrices(pos + np.array([0.5, -0.25, 1.0], np.float32), pinv, c2w)
    counts2 = (zeros2(), zeros2())
    check(run_both(R, o, d, tm, counts2), want, f"{case}: the camera moved away from the rays' origin")
    print(f"{case}: {len(o)} rays, {int(want[0].sum())} occluded; by the wide query as camera rays "
          f"{int(counts[0][0])} / {int(counts[1][0])}, as ordinary rays {int(counts2[0][0])} / {int(counts2[1][0])}")


# ---- 5. counts ---------------------------------------------------------------------------------------------

def test_counts(R, make_renderer):
    sc, st, o, d, ref, tm, cls = stress_ref(R, "robot")
    od, dd, td = gpu(o), gpu(d), gpu(tm)
    assert R.stats()["wide_tree"] in (1, 2)
    c_occ, c_seg, c_whole = zeros2(), zeros2(), zeros2()
    R.occluded_device(od, dd, td, counts=c_occ)
    R.trace_segments_device(od, dd, td, counts=c_seg)
    R.trace_rays_device(od, dd, counts=c_whole)
    print(f"robot, counts (wide, octree): occluded {c_occ.tolist()}, segments {c_seg.tolist()}, "
          f"trace_rays_device {c_whole.tolist()}")
    for c in (c_occ, c_seg):
        assert int(c.sum()) == N and int(c[0]) > 0
    # they accumulate
    R.occluded_device(od, dd, td, counts=c_occ)
    assert int(c_occ.sum()) == 2 * N
    r = make_renderer(RT_WBVH=0)
    r.load_scene(sc, st)
    c_occ, c_seg = zeros2(), zeros2()
    r.occluded_device(od, dd, td, counts=c_occ)
    r.trace_segments_device(od, dd, td, counts=c_seg)
    assert c_occ.tolist() == [0, N] and c_seg.tolist() == [0, N]


# ---- 6. the contract ---------------------------------------------------------------------------------------

def test_stream_order(R):
    """The rays and lengths are produced on a side stream behind long-running work and overwritten on it right
    after the calls; a consumer on that stream reads the outputs.  The host is back from both calls while the
    stream's earlier work still runs: an event recorded behind that work has not completed when they return
    (tests/test_gpu_visibility.py's form and amount of queued work).  (This exercises the order; a race could
    still pass by luck.)"""
    sc, st, o, d, ref, tm, cls = stress_ref(R, "robot")
    want = expected(ref, tm)
    R.trace_rays(o[:1], d[:1])   # (the scene is resident: the calls below have nothing to build)
    oc, dc, tc = gpu(o), gpu(d), gpu(tm)
    a = torch.rand((4096, 4096), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    busy = torch.cuda.Event()
    with torch.cuda.stream(side):
        b = a
        for _ in range(60):
            b = (b @ a) * (1.0 / 4096)
        busy.record(side)
        ot, dt, tt = oc.clone(), dc.clone(), tc.clone()
        seg = R.trace_segments_device(ot, dt, tt, stream=side)
        back_early_seg = not busy.query()
        occ = R.occluded_device(ot, dt, tt)   # (the current stream by default)
        back_early = not busy.query()
        ot.fill_(float("nan"))
        dt.zero_()
        tt.fill_(-1.0)
        seen = {k: v.clone() for k, v in seg.items()}
        seen_occ = occ.clone()
    side.synchronize()
    check((seen_occ.cpu().numpy(), host(seen)), want, "the consumer on the side stream")
    assert back_early_seg, "trace_segments_device returned only after the stream's earlier work had ended"
    assert back_early, "occluded_device returned only after the stream's earlier work had ended"
    torch.cuda.synchronize()
    del b


def test_scene_changes_and_close_wait_for_queries(make_renderer):
    n = 1 << 20
    rng = np.random.default_rng(3)
    scb, stb = scenes.bumpy70k(width=64, height=36)
    scr, str_ = scenes.robot1080(width=64, height=36)
    o, d = _random_rays(rng, n, np.array([0, 0, -3], np.float32), 2.0)
    od, dd = gpu(o), gpu(d)
    td = torch.full((n,), 2.5, device="cuda")
    r = make_renderer()
    r.load_scene(scb, stb)
    before = host(r.trace_segments_device(od, dd, td))
    before_occ = r.occluded_device(od, dd, td).cpu().numpy()
    assert np.array_equal(before_occ, before[4]) and 1000 < int(before_occ.sum()) < n - 1000
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = r.trace_segments_device(od, dd, td, stream=side)
    occ = r.occluded_device(od, dd, td, stream=side)
    # no wait: the geometry is replaced and a frame rendered while the queries may still run
    r.load_scene(scr, str_)
    got_frame = frame(r)
    side.synchronize()
    same(host(out), before, "the query in flight while the geometry was replaced")
    assert np.array_equal(occ.cpu().numpy(), before_occ)
    fresh = make_renderer()
    fresh.load_scene(scr, str_)
    assert_same_frame(got_frame, frame(fresh), "the robot's frame after the queries")
    # close() right after a launch
    from raytracercpp_amd.renderer import Renderer
    r3 = Renderer(0)
    r3.load_scene(scb, stb)
    out3 = r3.trace_segments_device(od, dd, td, stream=side)
    occ3 = r3.occluded_device(od, dd, td, stream=side)
    r3.close()
    side.synchronize()
    torch.cuda.synchronize()
    same(host(out3), before, "the query in flight at close()")
    assert np.array_equal(occ3.cpu().numpy(), before_occ)


def _raw_seg(r, p, n):
    v = [C.c_void_p(x) for x in p]
    return _lib.lib().rt_trace_segments_device(r._h, v[0], v[1], v[2], n, v[3], v[4], v[5], v[6], v[7], v[8], None)


def _raw_occ(r, p, n):
    v = [C.c_void_p(x) for x in p]
    return _lib.lib().rt_occluded_device(r._h, v[0], v[1], v[2], n, v[3], v[4], None)


def test_refusals_and_counters(R):
    sc, st, o, d, ref, tm, cls = stress_ref(R, "robot")
    n = 64
    # orig, dirs, tmax, the five outputs, counts; and the occlusion query's: orig, dirs, tmax, occluded, counts
    good = [gpu(o[:n]), gpu(d[:n]), gpu(tm[:n])] + [torch.full((n,), 77, dtype=dt, device="cuda") for dt in DTYPES] + \
           [torch.full((2,), 5, dtype=torch.int64, device="cuda")]
    host_arrays = [np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.ones(n, np.float32), np.zeros(n, np.int32),
                   np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8),
                   np.zeros(2, np.int64)]
    pinned = [torch.from_numpy(a.copy()).pin_memory() for a in host_arrays]
    occ = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    seg_before = R.device_segment_queries()
    others = (R.device_ray_queries(), R.device_shaded_queries(), R.device_visibility())

    def unchanged():
        torch.cuda.synchronize()
        assert R.device_segment_queries() == seg_before
        assert all(bool((t == 77).all()) for t in good[3:8]) and bool((good[8] == 5).all()) and bool((occ == 77).all())

    ptrs = [t.data_ptr() for t in good]
    optrs = [ptrs[0], ptrs[1], ptrs[2], occ.data_ptr(), ptrs[8]]
    omap = [0, 1, 2, 7, 8]   # the occlusion query's arguments among host_arrays
    for i in range(9):
        for what, bad in (("host", host_arrays[i].ctypes.data), ("pinned", pinned[i].data_ptr())):
            p = list(ptrs)
            p[i] = bad
            rc = _raw_seg(R, p, n)
            assert rc == -1, f"trace_segments_device argument {i} in {what} memory: {rc}"   # RT_EINVAL
            unchanged()
    for j, i in enumerate(omap):
        for what, bad in (("host", host_arrays[i].ctypes.data), ("pinned", pinned[i].data_ptr())):
            p = list(optrs)
            p[j] = bad
            rc = _raw_occ(R, p, n)
            assert rc == -1, f"occluded_device argument {j} in {what} memory: {rc}"
            unchanged()
    # a null pointer with n > 0 (tmax and the counts may be null)
    for i in (0, 1, 3, 4, 5, 6, 7):
        p = list(ptrs)
        p[i] = None
        assert _raw_seg(R, p, n) == -1, i
    for j in (0, 1, 3):
        p = list(optrs)
        p[j] = None
        assert _raw_occ(R, p, n) == -1, j
    # counts out of range, before anything is read
    for bad_n in ((1 << 30) + 1, -1, 1 << 40):
        assert _raw_seg(R, ptrs, bad_n) == -1 and _raw_occ(R, optrs, bad_n) == -1
    unchanged()
    # the Python mirror refuses the same before any pointer is taken
    with pytest.raises(ValueError, match="tmax: the tensor is on cpu, not on a GPU"):
        R.occluded_device(good[0], good[1], pinned[2])
    with pytest.raises(ValueError, match="tmax: shape"):
        R.trace_segments_device(good[0], good[1], good[2][: n - 1])
    with pytest.raises(ValueError, match="tmax: the tensor is not contiguous"):
        R.occluded_device(good[0], good[1], gpu(tm[:2 * n])[::2])
    with pytest.raises(ValueError, match="out: shape"):
        R.occluded_device(good[0], good[1], good[2], out=occ[: n - 1])
    unchanged()
    # n == 0: RT_OK, nothing launched, the pointers unread
    e = torch.zeros((0, 3), device="cuda")
    R.occluded_device(e, e.clone(), torch.zeros(0, device="cuda"), out=occ, counts=good[8])
    R.trace_segments_device(e, e.clone(), None, out=dict(zip(KEYS, good[3:8])), counts=good[8])
    L = _lib.lib()
    assert L.rt_occluded_device(R._h, None, None, None, 0, None, None, None) == 0
    assert L.rt_trace_segments_device(R._h, None, None, None, 0, None, None, None, None, None, None, None) == 0
    unchanged()
    assert R.occluded_device(e, e.clone()).shape == (0,) and R.trace_segments_device(e, e.clone())["t"].shape == (0,)
    unchanged()
    # and the good arguments pass: the segment counters move, the other queries' do not
    eocc, eseg = expected(tuple(a[:n] for a in ref), tm[:n])
    assert _raw_seg(R, ptrs, n) == 0 and _raw_occ(R, optrs, n) == 0
    same(host(dict(zip(KEYS, good[3:8]))), eseg, "after the refusals")
    assert np.array_equal(occ.cpu().numpy(), eocc)
    assert int(good[8].sum()) == 5 + 5 + 2 * n
    assert _raw_occ(R, optrs[:2] + [None] + optrs[3:], n) == 0   # (tmax null: +inf)
    assert np.array_equal(occ.cpu().numpy(), expected(tuple(a[:n] for a in ref), np.full(n, np.inf, np.float32))[0])
    calls, rays = R.device_segment_queries()
    assert calls == (seg_before[0][0] + 2, seg_before[0][1] + 1) and rays == (seg_before[1][0] + 2 * n, seg_before[1][1] + n)
    assert (R.device_ray_queries(), R.device_shaded_queries(), R.device_visibility()) == others


def test_renderer_without_geometry(make_renderer):
    """Before any geometry is set nothing is hit."""
    rng = np.random.default_rng(2)
    o, d = _random_rays(rng, 300, np.zeros(3, np.float32), 1.0)
    r = make_renderer()
    occ, seg = run_both(r, o, d, None)
    want = r.trace_rays(o, d)
    assert not want[4].any()
    check((occ, seg), expected(want, np.full(300, np.inf, np.float32)), "no geometry")
