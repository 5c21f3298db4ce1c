"""Where the triangle positions are (host only, host and device, device only) across every ordered pair of
position writers, each pair followed by every reader of the positions, with the device build on and off: a
renderer driven through the device paths against a host-only renderer given the same bytes.  Frames and aux
buffers bit for bit, rt_get_triangles word for word, and the counters by rule: one ingest per device input,
one device transform per matrix taken (and applied) on the device path, one octree build per frame that
follows a change.

The 12-triangle c2_cube golden scene at its golden size.  Each (build, first writer, second writer) is one
test on a fresh pair of renderers; the two writers run again before each of the four readers, so every reader
meets the state the pair leaves (what the reader before it left behind is the pair's starting state).

The host-path transform is set_object_transform on a renderer created under RT_GPU_XFORM=0.  A pair that
mixes it with the device-path transform needs both on one renderer: there the renderer is created with device
transforms and the host-path call is made with the device build switched off around it, which selects the
same path (Renderer::set_object_transform's choice reads both switches)."""
import itertools

import numpy as np
import pytest

from test_gpu_geometry_input import EDITS, bits, both, gpu, indexed_form
from test_gpu_octree_build import assert_same_frame, cube_golden, frame, make_renderer  # noqa: F401

pytestmark = pytest.mark.gpu

WRITERS = ("set_triangles", "set_triangles_device", "update_vertices_device", "xform_device", "xform_host",
           "clear_then_set")
READERS = ("ray_frame", "raster_frame", "brute_frame", "get_triangles")


class Run:
    """The two renderers of one sequence and the model the counters are predicted from."""

    def __init__(self, make_renderer, build, host_xform_env):
        self.sc, self.st = cube_golden()
        self.build = build
        self.gpu_xform = not host_xform_env
        self.host = make_renderer()
        self.dev = make_renderer(**({"RT_GPU_XFORM": 0} if host_xform_env else {}))
        self.dev.set_device_build(build)   # (the host-only renderer builds on the host throughout)
        for r in (self.host, self.dev):
            r.load_scene(self.sc, self.st)
        self.step = 0
        self.edit = 0
        # the model: the device copy is current; matrices queued for it; a frame has to build
        self.resident = False
        self.queued = 0
        self.dirty = True
        self.ingests = self.xforms = self.builds = 0

    def tri(self):
        """New positions for every input: the cube scaled and moved a little (the shared vertices stay shared)."""
        self.step += 1
        k = np.float32(1.0 + 0.03125 * (self.step % 7))
        return np.ascontiguousarray(self.sc.tri * k + np.float32(0.015625 * (self.step % 3)), np.float32)

    def replaced(self, resident):
        self.resident, self.queued, self.dirty = resident, 0, True

    def apply_queue(self):
        self.xforms += self.queued
        self.queued = 0

    def write(self, w):
        sc, host, dev = self.sc, self.host, self.dev
        if w in ("set_triangles", "clear_then_set"):
            if w == "clear_then_set":
                both(host, dev, lambda r: r.clear_geometry())
            t = self.tri()
            both(host, dev, lambda r: r.set_triangles(t, sc.tri_mat, sc.tri_uv))
            self.replaced(False)
        elif w == "set_triangles_device":
            t = self.tri()
            host.set_triangles(t, sc.tri_mat, sc.tri_uv)
            dev.set_triangles_device(gpu(t), sc.tri_mat, sc.tri_uv)
            self.ingests += 1
            self.replaced(True)
        elif w == "update_vertices_device":
            t = self.tri()
            host.set_triangles(t, sc.tri_mat, sc.tri_uv)
            hv, hi = indexed_form(t)
            dev.update_vertices_device(gpu(hv), indices=gpu(hi))
            self.ingests += 1
            self.replaced(True)
        else:
            m = EDITS[self.edit % len(EDITS)]
            self.edit += 1
            host.set_object_transform(m)
            forced = w == "xform_host" and self.gpu_xform   # (a mixed pair: see the module's docstring)
            if forced:
                dev.set_device_build(False)
            dev.set_object_transform(m)
            if forced:
                dev.set_device_build(self.build)
            if self.build and self.gpu_xform and not forced and self.resident:
                self.queued += 1
            else:   # the host path reads the positions (the queue runs first) and leaves them on the host
                self.apply_queue()
                self.resident = False
            self.dirty = True

    def settle(self, bvh, raster):
        """What a frame does to the model."""
        if self.dirty:
            self.apply_queue()
            self.builds += 1
            self.dirty = False
            if self.build and bvh:
                self.resident = True   # (the device build stages the positions)
        if raster:
            self.resident = True

    def read(self, rd, what):
        host, dev, st = self.host, self.dev, self.st
        if rd == "ray_frame":
            assert_same_frame(frame(host), frame(dev), what)
            self.settle(True, False)
        elif rd == "raster_frame":
            both(host, dev, lambda r: r.set_render_settings(st.copy(hybrid_rasterization_tracing=True)))

            def raster(r):
                r.request_aux(rgba=True, hit=True, shadow=True)
                r.raster_trace()
                return r.get_internal(argb=True, rgba=True, hit=True, shadow=True)
            assert_same_frame(raster(host), raster(dev), what)
            both(host, dev, lambda r: r.set_render_settings(st))
            self.settle(True, True)
        elif rd == "brute_frame":
            both(host, dev, lambda r: r.set_render_settings(st.copy(enable_bvh=False)))
            self.dirty = True
            assert_same_frame(frame(host), frame(dev), what)
            self.settle(False, False)
            both(host, dev, lambda r: r.set_render_settings(st))
            self.dirty = True
        else:
            th, td = host.get_triangles(), dev.get_triangles()
            assert th.shape == td.shape == (self.sc.tri.shape[0], 9), what
            assert np.array_equal(bits(th), bits(td)), what
            self.apply_queue()
        self.check_counters(what)

    def check_counters(self, what):
        dev, host = self.dev, self.host
        assert dev.device_ingests() == self.ingests and host.device_ingests() == 0, what
        assert dev.device_transforms() == self.xforms and host.device_transforms() == 0, what
        assert dev.stats()["host_builds"] + dev.device_builds() == self.builds, what
        assert host.stats()["host_builds"] == self.builds and host.device_builds() == 0, what
        if not self.build:
            assert dev.device_builds() == 0, what


SEQUENCES = list(itertools.product(WRITERS, WRITERS))
assert len(SEQUENCES) == 36


@pytest.mark.parametrize("build", [True, False], ids=["device_build", "host_build"])
@pytest.mark.parametrize("first,second", SEQUENCES, ids=[f"{a}-{b}" for a, b in SEQUENCES])
def test_writer_pair_then_every_reader(make_renderer, first, second, build):
    pair = {first, second}
    run = Run(make_renderer, build, host_xform_env="xform_host" in pair and "xform_device" not in pair)
    for rd in READERS:
        run.write(first)
        run.write(second)
        run.read(rd, f"{first}, {second}, then {rd}")
    # and the state the last reader left is whole: one more frame, nothing to build
    run.read("ray_frame", f"{first}, {second}: a last frame")
