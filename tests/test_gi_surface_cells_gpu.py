"""The GI masks' surface patches (DESIGN.md "GI surface patches") change which row of masks a leaf-kernel lane takes, never what
its closest-hit walk finds: with SKR_GI_SURFACE=0 (the grids' rows) and =1 (the patches' rows) every frame is the same, byte for
byte and bit for bit, with the same ray, hit, shadow-ray and test counts — and the same as the loop over every sphere
(SKR_GI_MASK=0) on the headline frame — on spheres2 and on random scenes of 1, 16, 17 and 32 spheres (uint16_t and uint32_t masks)."""
import ctypes as C
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def patch_words(scene):
    """The number of words of the scene's surface patches (skr_scene_get_gi_surface, internal); 0 = none."""
    fn = skr.lib().skr_scene_get_gi_surface
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]
    n = C.c_int32()
    assert fn(scene.h, C.byref(n), None, None, None) == 0
    return n.value


def frame(gpu, monkeypatch, scene, opt, env):
    for k in ("SKR_FLAT", "SKR_PIPELINE", "SKR_GI_MASK", "SKR_GI_SURFACE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = skr.Renderer(scene)
    r.work(reset=True)
    rgb, rgbf = r.render(opt, want_float=True)
    gpu.cuda.synchronize()
    return rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), r.work(reset=True), r.kernel_variant()


def same_every_way(gpu, monkeypatch, scene, opt, env, variant, switches):
    assert patch_words(scene) > 0, "the scene has no surface patches"
    ref = None
    for sw in switches:
        got = frame(gpu, monkeypatch, scene, opt, dict(env, **sw))
        assert got[3] == variant, (got[3], variant, sw)
        assert got[2]["radiance_rays"] > 0
        if ref is None:
            ref = got
            continue
        assert got[2] == ref[2], (sw, got[2], ref[2])
        assert np.array_equal(got[0], ref[0]), "%r: bytes differ at %d pixels" % (sw, int((got[0] != ref[0]).any(-1).sum()))
        assert np.array_equal(got[1], ref[1]), "%r: float image differs at %d values" % (sw, int((got[1] != ref[1]).sum()))


def test_headline_frame_is_unchanged(gpu, monkeypatch):
    """bench.py --config 3: spheres2.scn 1920x1080 --gillum 16 --shadow, the persistent leaf kernel: patches, grids, every sphere."""
    same_every_way(gpu, monkeypatch, skr.parse_scene(scene_path("spheres2.scn")), skr.Options(1920, 1080, gillum=16, shadow=True, seed=20261004),
                   {}, "node_levels_v5", [{"SKR_GI_SURFACE": "1"}, {"SKR_GI_SURFACE": "0"}, {"SKR_GI_MASK": "0"}])


def test_deeper_tree_is_unchanged(gpu, monkeypatch):
    """depth 4: the leaf kernel's units are records of level 2, activated by the trace kernel's levels."""
    same_every_way(gpu, monkeypatch, skr.parse_scene(scene_path("spheres2.scn")), skr.Options(480, 270, gillum=8, depth=4, shadow=True, seed=3),
                   {"SKR_FLAT": "0"}, "node_levels_v5", [{"SKR_GI_SURFACE": "1"}, {"SKR_GI_SURFACE": "0"}])


@pytest.mark.parametrize("n", [1, 16, 17, 32])
def test_random_sphere_scenes_are_unchanged(gpu, monkeypatch, tmp_path, n):
    """n spheres of mixed sizes over a ground sphere (n = 1: the ground alone), one light."""
    rng = np.random.default_rng(9300 + n)
    lines = ["camera 0 2 -10 0 -.1 .9 0 1 0 30", "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1", "sphere 0 -40 0 40"]
    for i in range(n - 1):
        c, rad = rng.uniform(-6, 6, 3) + [0, 2, 3], 10.0 ** rng.uniform(-1.5, 0.2)
        lines.append("material %g %g %g %g %g %g .2 .2 .2 8 0 0 0 1" % (*rng.random(3), *rng.random(3)))
        lines.append("sphere %.7g %.7g %.7g %.7g" % (*c, rad))
    lines.append("point_light .8 .8 .8 2 9 -1")
    path = os.path.join(str(tmp_path), "s.scn")
    open(path, "w").write("\n".join(lines) + "\n")
    scene = skr.parse_scene(path)
    same_every_way(gpu, monkeypatch, scene, skr.Options(240, 136, gillum=8, depth=3, shadow=True, seed=n), {"SKR_FLAT": "0"}, "node_levels_v5",
                   [{"SKR_GI_SURFACE": "1"}, {"SKR_GI_SURFACE": "0"}])
