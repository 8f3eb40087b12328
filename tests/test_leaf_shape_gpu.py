"""The leaf kernel's instances with a launch shape compiled in (DESIGN.md 5.2 "Launch shapes") perform the operations of the instance
that reads the shape at run time, on the same values: every frame is the same with SKR_LEAF_SHAPE unset and =0, byte for byte and bit
for bit, with the same ray, hit, shadow-ray and test counts.  64x36 frames, at the smallest shapes at which a compiled-in fact can be
wrong: both kinds of units (depth 2: level-0 nodes; depth 3, 4: records), an odd N (the last round has no second child), one and two
lights — and the launches that break a fact (three lights, an exponent of 8 bits, 32-bit GI masks), which must run the run-time
instance.  Which instance ran is asked of the renderer (skr_renderer_last_leaf_shape, internal): no case passes because the run-time
instance ran twice."""
import ctypes as C
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path
from test_leaf_shape_host import POINT1, POINT2, RUNTIME, SWITCHES, write_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def frame(gpu, monkeypatch, scene, opt, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = skr.Renderer(scene)
    r.work(reset=True)
    rgb, rgbf = r.render(opt, want_float=True)
    gpu.cuda.synchronize()
    fn = skr.lib().skr_renderer_last_leaf_shape
    fn.argtypes, fn.restype = [C.c_void_p], C.c_int
    return rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), r.work(reset=True), r.kernel_variant(), fn(r.h)


def same_with_and_without(gpu, monkeypatch, scene, opt, shape, env=None):
    """The frame with the shaped instance (`shape`: the one the launch must get) and with SKR_LEAF_SHAPE=0."""
    env = dict({"SKR_FLAT": "0"}, **(env or {}))  # (the persistent leaf kernel, on so small a launch)
    got = frame(gpu, monkeypatch, scene, opt, env)
    ref = frame(gpu, monkeypatch, scene, opt, dict(env, SKR_LEAF_SHAPE="0"))
    assert got[3] == ref[3] == "node_levels_v5", (got[3], ref[3])
    assert got[4] == shape and ref[4] == RUNTIME, (got[4], ref[4], shape)
    assert got[2]["radiance_rays"] > 0 and got[2]["shadow_rays"] > 0, got[2]
    assert got[2] == ref[2], (got[2], ref[2])
    assert np.array_equal(got[0], ref[0]), "bytes differ at %d pixels" % int((got[0] != ref[0]).any(-1).sum())
    assert np.array_equal(got[1], ref[1]), "float image differs at %d values" % int((got[1] != ref[1]).sum())


def spheres2():
    return skr.parse_scene(scene_path("spheres2.scn"))


def generated(tmp_path, **kw):
    return skr.parse_scene(write_scene(os.path.join(str(tmp_path), "s.scn"), **kw))


@pytest.mark.parametrize("kw", [
    dict(gillum=4, depth=3),             # records of level 1
    dict(gillum=4, depth=2),             # FIRST: the units are the level-0 nodes, the pixels are written by the leaf kernel
    dict(gillum=3, depth=3),             # odd N: the last round has no second child
    dict(gillum=4, depth=4),             # activate + leaf
    dict(gillum=4, depth=3, jsample=2),  # AA: four passes, no replay of the level-0 stage
], ids=["depth3", "depth2", "odd_n", "depth4", "jsample2"])
def test_spheres2_two_light_shape(gpu, monkeypatch, kw):
    same_with_and_without(gpu, monkeypatch, spheres2(), skr.Options(64, 36, shadow=True, seed=11, **kw), POINT2)


@pytest.mark.parametrize("depth", [2, 3])
def test_one_point_light(gpu, monkeypatch, tmp_path, depth):
    same_with_and_without(gpu, monkeypatch, generated(tmp_path, lights=1), skr.Options(64, 36, gillum=4, depth=depth, shadow=True, seed=12), POINT1)


def test_two_lights_sixteen_spheres(gpu, monkeypatch, tmp_path):
    """The largest scene of the shape: every bit of a 16-bit GI mask names a sphere."""
    same_with_and_without(gpu, monkeypatch, generated(tmp_path, spheres=16), skr.Options(64, 36, gillum=4, depth=3, shadow=True, seed=13), POINT2)


@pytest.mark.parametrize("kw", [dict(lights=3), dict(power=128), dict(spheres=17)], ids=["three_lights", "exponent_128", "17_spheres"])
def test_a_broken_fact_runs_the_run_time_instance(gpu, monkeypatch, tmp_path, kw):
    same_with_and_without(gpu, monkeypatch, generated(tmp_path, **kw), skr.Options(64, 36, gillum=4, depth=3, shadow=True, seed=14), RUNTIME)


def test_flat_schedule_runs_no_leaf_kernel(gpu, monkeypatch):
    """The flat schedule's kernels have no shaped instances: the switch changes nothing there, and the renderer says so."""
    got = frame(gpu, monkeypatch, spheres2(), skr.Options(64, 36, gillum=4, depth=3, shadow=True, seed=11), {"SKR_FLAT": "1"})
    assert got[4] == -1, got[4]
