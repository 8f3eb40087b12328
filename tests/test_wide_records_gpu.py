"""A hit record of the node pipeline is 32 bytes and carries the ray that found the hit with its b and D for the sphere it hit
(csrc/launch.h SKR_WIDE_RECORDS; csrc/render_nodes.hip trace_round, activate_record): whoever shades the hit reads them instead of
forming them again from the record's draws.  They are the values it used to form, so every frame here is held against the CPU oracle bit
for bit — bytes, float image and the four work counts — at the smallest launches that reach every writer and every reader of a record:
all three trace instances (GI masks, none, triangles), the leaf kernel's unit begin and unit end (the shaped and the run-time instance),
skr_activate_kernel (depth 4), skr_shade_leaf_kernel (the flat schedule), an odd N whose last round has no second child, and a launch
that the doubled table cuts into two bands (the plan's side of it: tests/test_record_tables_host.py).  A launch of which not even
one 16x16 block fits its budget with 32-byte records runs the instances with 16-byte records instead of being refused: the last
tests render such launches — asked of the plan, not assumed — through every kernel that has both forms."""
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path
from test_leaf_shape_host import write_scene
from test_record_tables_host import narrow_budget, plan

pytestmark = pytest.mark.gpu

SWITCHES = ("SKR_FLAT", "SKR_PIPELINE", "SKR_GI_MASK", "SKR_GI_SURFACE", "SKR_SHADOW_MASK", "SKR_SHADOW_SURFACE", "SKR_LEVELS_BUDGET_MB",
            "SKR_PRIMARY_CACHE", "SKR_LEAF_SHAPE")
W, H = 64, 36
SCHEDULES = [("0", "node_levels_v5"), ("1", "node_levels_v5_flat")]
_ORACLE = {}  # one oracle frame per (scene file, size, options, rows), shared by the schedules and the frames of a renderer


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """Scene files by name: the golden ones, and the generated ones (tests/test_leaf_shape_host.py write_scene)."""
    d = str(tmp_path_factory.mktemp("wide_records"))
    return {"spheres2": scene_path("spheres2.scn"), "spheres1": scene_path("spheres1.scn"),
            "generated": write_scene(os.path.join(d, "five.scn")), "three_lights": write_scene(os.path.join(d, "three.scn"), lights=3)}


def want(oracle, path, w, h, kw, rows=None):
    key = (path, w, h, tuple(sorted(kw.items())), rows)
    if key not in _ORACLE:
        ykw = {} if rows is None else dict(y0=rows[0], y1=rows[1])
        rgb, f, st = oracle.render(path, w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **dict(kw, **ykw))
        _ORACLE[key] = (rgb, f.view(np.uint32), tuple(int(v) for v in st[:4]))
    return _ORACLE[key]


def frame(gpu, r, opt):
    r.work(reset=True)
    rgb, rgbf = r.render(opt, want_float=True)
    gpu.cuda.synchronize()
    wk = r.work(reset=True)
    return rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), (wk["radiance_rays"], wk["sphere_hits"], wk["shadow_rays"], wk["sphere_tests"])


def assert_oracle(got, exp, what):
    assert got[0].shape == exp[0].shape, (what, got[0].shape, exp[0].shape)
    assert np.array_equal(got[1].reshape(-1), exp[1].reshape(-1)), "%s: %d float words differ" % (what, int((got[1].reshape(-1) != exp[1].reshape(-1)).sum()))
    assert np.array_equal(got[0], exp[0]), "%s: bytes differ at %d pixels" % (what, int((got[0] != exp[0]).any(-1).sum()))
    assert got[2] == exp[2], (what, got[2], exp[2])
    assert exp[2][0] > 0 and exp[2][1] > 0


def check(gpu, oracle, monkeypatch, flat, variant, path, w, h, kw, env=None):
    monkeypatch.setenv("SKR_FLAT", flat)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = skr.Renderer(skr.parse_scene(path))
    got = frame(gpu, r, skr.Options(w, h, **kw))
    assert r.kernel_variant() == variant, r.kernel_variant()
    assert_oracle(got, want(oracle, path, w, h, kw), "%s %s flat=%s" % (os.path.basename(path), kw, flat))
    return r


@pytest.mark.parametrize("flat,variant", SCHEDULES)
@pytest.mark.parametrize("scene", ["spheres2", "generated"])
@pytest.mark.parametrize("kw", [
    dict(gillum=4, depth=3),  # records of level 1: the leaf kernel's unit begin and end / skr_shade_leaf_kernel
    dict(gillum=4, depth=4),  # skr_activate_kernel reads the records and writes nodes that are traced again
    dict(gillum=3, depth=3),  # odd N: the last round has no second child, so no second record
], ids=["depth3", "depth4", "odd_n"])
def test_frames_with_records(gpu, oracle, monkeypatch, scenes, kw, scene, flat, variant):
    check(gpu, oracle, monkeypatch, flat, variant, scenes[scene], W, H, dict(kw, shadow=True, seed=41))


@pytest.mark.parametrize("flat,variant", SCHEDULES)
def test_three_lights_run_the_run_time_shape(gpu, oracle, monkeypatch, scenes, flat, variant):
    """No shape of the leaf kernel has three lights (launch.h skr_leaf_shape): the instance that reads the launch at run time."""
    check(gpu, oracle, monkeypatch, flat, variant, scenes["three_lights"], W, H, dict(gillum=4, depth=3, shadow=True, seed=42))


@pytest.mark.parametrize("flat,variant", SCHEDULES)
def test_the_triangle_instance(gpu, oracle, monkeypatch, scenes, flat, variant):
    """spheres1.scn has two triangles: skr_trace_kernel<true, false> writes the records, classify_child's walk sits between the walk that
    formed b, D and the store."""
    check(gpu, oracle, monkeypatch, flat, variant, scenes["spheres1"], W, H, dict(gillum=4, depth=3, shadow=True, seed=43))


def test_no_gi_masks_instance(gpu, oracle, monkeypatch, scenes):
    """SKR_GI_MASK=0: skr_trace_kernel<false, false> and the leaf kernel without the masked walk."""
    check(gpu, oracle, monkeypatch, "0", "node_levels_v5", scenes["spheres2"], W, H, dict(gillum=4, depth=3, shadow=True, seed=41), env={"SKR_GI_MASK": "0"})


def test_two_bands_where_16_byte_records_took_one(gpu, oracle, monkeypatch, scenes):
    """--gillum 16 under a budget of 2 MiB: the 12 blocks' tables are 2.27 MiB with 32-byte records (1.52 MiB with 16-byte ones:
    tests/test_record_tables_host.py asks the plan), so the frame is two bands — two block rows, then rows 32 .. 35 — and keeps no
    level-0 stage."""
    kw = dict(gillum=16, depth=3, shadow=True, seed=44)
    r = check(gpu, oracle, monkeypatch, "0", "node_levels_v5", scenes["spheres2"], W, H, kw, env={"SKR_LEVELS_BUDGET_MB": "2"})
    last = want(oracle, scenes["spheres2"], W, H, dict(depth=1), rows=(32, 36))[2][1]  # the primary hits of the last band's rows
    assert 0 < last < want(oracle, scenes["spheres2"], W, H, dict(depth=1))[2][1] and r.last_parent_count() == last
    assert r.primary_cache_stats() == (0, 0)


@pytest.mark.parametrize("scene,kw,flat,variant", [
    ("spheres2", dict(gillum=97, depth=3), "0", "node_levels_v5"),      # the shaped leaf instance and the GI-mask trace instance
    ("spheres2", dict(gillum=8, depth=4), "0", "node_levels_v5"),       # skr_activate_kernel
    ("spheres2", dict(gillum=33, depth=3), "1", "node_levels_v5_flat"), # skr_shade_leaf_kernel
    ("spheres1", dict(gillum=97, depth=3), "0", "node_levels_v5"),      # the triangle instances
    ("three_lights", dict(gillum=97, depth=3), "0", "node_levels_v5"),  # the run-time shape
], ids=["leaf", "activate", "flat", "triangles", "three_lights"])
def test_16_byte_records_where_one_block_needs_them(gpu, oracle, monkeypatch, scenes, scene, kw, flat, variant):
    """16x36 under the budget at which the plan keeps 16-byte records (one block's tables fit it with them and not with 32-byte ones):
    the launch is rendered, in bands of one block, by the instances that form the ray again from the record's draws."""
    w, h = 16, 36
    mb = narrow_budget(w, h, kw["gillum"], kw["depth"], flat == "1")
    assert mb is not None, "no whole number of MiB between the two forms: choose another N"
    pl = plan(w, h, kw["gillum"], kw["depth"], flat == "1", budget_mb=mb)
    assert pl["rec_bytes"] == 16 and plan(w, h, kw["gillum"], kw["depth"], flat == "1", nblk=1)["banded"] > mb << 20
    r = check(gpu, oracle, monkeypatch, flat, variant, scenes[scene], w, h, dict(kw, shadow=True, seed=45), env={"SKR_LEVELS_BUDGET_MB": str(mb)})
    if pl["band_nblk"] < 3:
        assert r.primary_cache_stats() == (0, 0)  # several bands: no stage is kept
