"""The GI masks (DESIGN.md "GI masks") change which spheres the node pipeline's closest-hit walk of a GI child visits, never what it
finds: with SKR_GI_MASK=0 (every sphere) and =1 (the masked walk) every frame is the same, byte for byte and bit for bit, with the
same ray, hit, shadow-ray and test counts — on the headline frame, a deeper tree, the flat schedule, and random scenes of 1, 16, 17
and 32 spheres (uint16_t and uint32_t masks)."""
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


def frame(gpu, monkeypatch, scene, opt, env, mask):
    for k in ("SKR_FLAT", "SKR_PIPELINE", "SKR_GI_MASK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env, SKR_GI_MASK=str(mask)).items():
        monkeypatch.setenv(k, v)
    r = skr.Renderer(scene)
    r.work(reset=True)
    rgb, rgbf = r.render(opt, want_float=True)
    gpu.cuda.synchronize()
    return rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), r.work(reset=True), r.kernel_variant()


def same_both_ways(gpu, monkeypatch, scene, opt, env, variant):
    assert len(scene.gi_masks()[0]) > 0, "the scene has no GI masks"
    a_rgb, a_f, a_w, a_v = frame(gpu, monkeypatch, scene, opt, env, 0)
    b_rgb, b_f, b_w, b_v = frame(gpu, monkeypatch, scene, opt, env, 1)
    assert a_v == b_v == variant, (a_v, b_v, variant)
    assert a_w == b_w, (a_w, b_w)
    assert a_w["radiance_rays"] > 0
    assert np.array_equal(a_rgb, b_rgb), "bytes differ at %d pixels" % int((a_rgb != b_rgb).any(-1).sum())
    assert np.array_equal(a_f, b_f), "float image differs at %d values" % int((a_f != b_f).sum())


def test_headline_frame_is_unchanged(gpu, monkeypatch):
    """bench.py --config 3: spheres2.scn 1920x1080 --gillum 16 --shadow, the persistent leaf kernel."""
    same_both_ways(gpu, monkeypatch, skr.parse_scene(scene_path("spheres2.scn")), skr.Options(1920, 1080, gillum=16, shadow=True, seed=20261004),
                   {}, "node_levels_v5")


@pytest.mark.parametrize("kw,env,variant", [
    (dict(gillum=8, depth=4, shadow=True, seed=3), {"SKR_FLAT": "0"}, "node_levels_v5"),       # trace kernel levels + activate
    (dict(gillum=6, depth=3, shadow=True, seed=4), {"SKR_FLAT": "1"}, "node_levels_v5_flat"),  # the last level through the trace kernel
])
def test_deeper_and_flat_are_unchanged(gpu, monkeypatch, kw, env, variant):
    same_both_ways(gpu, monkeypatch, skr.parse_scene(scene_path("spheres2.scn")), skr.Options(480, 270, **kw), env, variant)


@pytest.mark.parametrize("n", [1, 16, 17, 32])
def test_random_sphere_scenes_are_unchanged(gpu, monkeypatch, tmp_path, n):
    """n spheres of mixed sizes over a ground sphere (n = 1: the ground alone), one light."""
    rng = np.random.default_rng(9100 + n)
    lines = ["camera 0 2 -10 0 -.1 .9 0 1 0 30", "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1", "sphere 0 -40 0 40"]
    for i in range(n - 1):
        c, rad = rng.uniform(-6, 6, 3) + [0, 2, 3], 10.0 ** rng.uniform(-1.5, 0.2)
        lines.append("material %g %g %g %g %g %g .2 .2 .2 8 0 0 0 1" % (*rng.random(3), *rng.random(3)))
        lines.append("sphere %.7g %.7g %.7g %.7g" % (*c, rad))
    lines.append("point_light .8 .8 .8 2 9 -1")
    path = os.path.join(str(tmp_path), "s.scn")
    open(path, "w").write("\n".join(lines) + "\n")
    scene = skr.parse_scene(path)
    assert scene.gi_masks()[2] == (1 if n > 16 else 0)
    for env, variant in (({"SKR_FLAT": "0"}, "node_levels_v5"), ({"SKR_FLAT": "1"}, "node_levels_v5_flat")):
        same_both_ways(gpu, monkeypatch, scene, skr.Options(240, 136, gillum=8, depth=3, shadow=True, seed=n), env, variant)
