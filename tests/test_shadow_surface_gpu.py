"""The shadow masks' surface patches (DESIGN.md "Shadow surface patches") change which mask a lane's shadow pair walk takes, never
what the walk finds: with SKR_SHADOW_SURFACE=1 (a sphere hit reads its patch's word), =0 (the two direction masks) and
SKR_SHADOW_MASK=0 (the loop over every sphere) every frame is the same, byte for byte and bit for bit, with the same four work
counts — and the oracle's where it is compared.  The shapes are the smallest that reach every caller of direct_light<false>: the leaf
kernel's batches on records and on level-0 nodes, the flat schedule's shade kernel, the activate kernel of a deeper tree, bands, an
odd N, an odd light count with masks above 16 bits, and the general pipeline's fallback on a scene with triangles."""
import ctypes as C
import os

import numpy as np
import pytest

import camera_poses as cp
import skele_raytracer_amd as skr
from conftest import scene_path

pytestmark = pytest.mark.gpu

SWITCHES = ("SKR_FLAT", "SKR_PIPELINE", "SKR_GI_MASK", "SKR_GI_SURFACE", "SKR_SHADOW_MASK", "SKR_SHADOW_SURFACE", "SKR_LEVELS_BUDGET_MB", "SKR_PRIMARY_CACHE")
THREE_WAYS = [{"SKR_SHADOW_SURFACE": "1"}, {"SKR_SHADOW_SURFACE": "0"}, {"SKR_SHADOW_MASK": "0"}]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def patch_pairs(scene):
    """The number of pair tables of the scene's surface patches (skr_scene_get_shadow_surface, internal); 0 = none."""
    fn = skr.lib().skr_scene_get_shadow_surface
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    n, stride = C.c_int32(), C.c_int32()
    assert fn(scene.h, C.byref(n), C.byref(stride), None, None) == 0
    return n.value


def frame(gpu, monkeypatch, scene, opt, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = skr.Renderer(scene)
    r.work(reset=True)
    rgb, rgbf = r.render(opt, want_float=True)
    gpu.cuda.synchronize()
    return rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), r.work(reset=True), r.kernel_variant()


def same_three_ways(gpu, monkeypatch, scene, opt, env, variant, pairs):
    """The frame under the three switch settings; returns the first (bytes, float words, work counts, variant)."""
    assert patch_pairs(scene) == pairs
    ref = None
    for sw in THREE_WAYS:
        got = frame(gpu, monkeypatch, scene, opt, dict(env, **sw))
        assert got[3] == variant, (got[3], variant, sw)
        assert got[2]["radiance_rays"] > 0 and got[2]["shadow_rays"] > 0
        if ref is None:
            ref = got
            continue
        assert got[2] == ref[2], (sw, got[2], ref[2])
        assert np.array_equal(got[0], ref[0]), "%r: bytes differ at %d pixels" % (sw, int((got[0] != ref[0]).any(-1).sum()))
        assert np.array_equal(got[1], ref[1]), "%r: float image differs at %d values" % (sw, int((got[1] != ref[1]).sum()))
    return ref


def assert_oracle(oracle, path, w, h, kw, got):
    o_rgb, o_f, st = oracle.render(path, w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw)
    assert np.array_equal(got[1], o_f.view(np.uint32)), "float image differs from the oracle at %d values" % int((got[1] != o_f.view(np.uint32)).sum())
    assert np.array_equal(got[0], o_rgb)
    assert [got[2]["radiance_rays"], got[2]["sphere_hits"], got[2]["shadow_rays"]] == [int(x) for x in st[:3]]


# name, options, switches, variant
SPHERES2 = [
    ("leaf_records_gi4_d3", dict(gillum=4, depth=3, shadow=True, seed=11), {"SKR_FLAT": "0"}, "node_levels_v5"),
    ("flat_gi5_d3", dict(gillum=5, depth=3, shadow=True, seed=12), {"SKR_FLAT": "1"}, "node_levels_v5_flat"),
    ("leaf_level0_gi4_d2", dict(gillum=4, depth=2, shadow=True, seed=13), {"SKR_FLAT": "0"}, "node_levels_v5"),
    ("flat_gi5_d2", dict(gillum=5, depth=2, shadow=True, seed=14), {"SKR_FLAT": "1"}, "node_levels_v5_flat"),
    ("activate_gi4_d4", dict(gillum=4, depth=4, shadow=True, seed=15), {"SKR_FLAT": "0"}, "node_levels_v5"),
    ("bands_gi5_d3", dict(gillum=5, depth=3, shadow=True, seed=16), {"SKR_FLAT": "0", "SKR_LEVELS_BUDGET_MB": "1"}, "node_levels_v5"),
]


@pytest.mark.parametrize("case", SPHERES2, ids=[c[0] for c in SPHERES2])
def test_spheres2_is_unchanged_and_the_oracles(gpu, oracle, monkeypatch, case):
    _, kw, env, variant = case
    path = scene_path("spheres2.scn")
    got = same_three_ways(gpu, monkeypatch, skr.parse_scene(path), skr.Options(96, 54, **kw), env, variant, 1)
    assert_oracle(oracle, path, 96, 54, kw, got)


def test_seventeen_spheres_three_lights(gpu, oracle, monkeypatch, tmp_path):
    """An odd light count (the last pair is single) and masks above 16 bits."""
    rng = np.random.default_rng(9417)
    lines = ["camera 0 2 -10 0 -.1 .9 0 1 0 30", "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1", "sphere 0 -40 0 40"]
    for i in range(16):
        c, rad = rng.uniform(-6, 6, 3) + [0, 2, 3], 10.0 ** rng.uniform(-1.5, 0.2)
        lines.append("material %g %g %g %g %g %g .2 .2 .2 8 0 0 0 1" % (*rng.random(3), *rng.random(3)))
        lines.append("sphere %.7g %.7g %.7g %.7g" % (*c, rad))
    lines += ["point_light .8 .8 .8 2 9 -1", "point_light .5 .6 .7 -5 4 2", "point_light .7 .5 .4 1 3 8"]
    path = os.path.join(str(tmp_path), "s.scn")
    open(path, "w").write("\n".join(lines) + "\n")
    kw = dict(gillum=4, depth=3, shadow=True, seed=17)
    got = same_three_ways(gpu, monkeypatch, skr.parse_scene(path), skr.Options(96, 54, **kw), {"SKR_FLAT": "0"}, "node_levels_v5", 2)
    assert_oracle(oracle, path, 96, 54, kw, got)


@pytest.mark.parametrize("shade", [False, True], ids=["black_triangles", "shade_triangles"])
def test_triangle_scene(gpu, oracle, monkeypatch, shade):
    """spheres1.scn (4 spheres, 2 triangles).  Triangles as black holes: the node pipeline, whose shaded hits are all sphere hits.
    --shade-triangles: the general level pipeline shades triangle hits too and has no sphere to key a hit to, so every lane takes
    the two direction masks."""
    path = scene_path("spheres1.scn")
    kw = dict(gillum=4, depth=3, shadow=True, seed=18, shade_triangles=shade)
    got = same_three_ways(gpu, monkeypatch, skr.parse_scene(path), skr.Options(96, 54, **kw), {}, "level_pipeline_g1" if shade else "node_levels_v5_flat", 1)
    assert_oracle(oracle, path, 96, 54, kw, got)


@pytest.mark.parametrize("name", ["s2_long", "s2_in_ground"])
def test_poses_away_from_the_small_spheres(gpu, oracle, monkeypatch, name):
    """Hits far out on the ground (s2_long) and on the inside of the ground sphere (s2_in_ground: P on the surface, the sphere around it)."""
    pose = cp.BY_NAME[name]
    path = scene_path(cp.scene_file(pose))
    kw = dict(pose.kw, gillum=4, depth=3, shadow=True, seed=19)
    got = same_three_ways(gpu, monkeypatch, skr.parse_scene(path), skr.Options(96, 72, **kw), {"SKR_FLAT": "0"}, "node_levels_v5", 1)
    assert_oracle(oracle, path, 96, 72, kw, got)
