"""The shadow masks (DESIGN.md "Shadow masks") change which spheres the level pipelines' shadow walk visits, never what it finds:
with SKR_SHADOW_MASK=0 (every sphere) and =1 (the masked walk) every frame is the same, byte for byte and bit for bit, with the same
ray, hit, shadow-ray and shadow-test counts — on the headline frame, through both schedules of the node pipeline and through the
general level pipeline (triangles, --shade-triangles, fog)."""
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
    for k in ("SKR_FLAT", "SKR_PIPELINE", "SKR_SHADOW_MASK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env, SKR_SHADOW_MASK=str(mask)).items():
        monkeypatch.setenv(k, v)
    r = skr.Renderer(scene)
    r.work(reset=True)
    rgb, rgbf = r.render(opt, want_float=True)
    gpu.cuda.synchronize()
    return rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), r.work(reset=True), r.kernel_variant()


def same_both_ways(gpu, monkeypatch, scene, opt, env, variant=None):
    a_rgb, a_f, a_w, a_v = frame(gpu, monkeypatch, scene, opt, env, 0)
    b_rgb, b_f, b_w, b_v = frame(gpu, monkeypatch, scene, opt, env, 1)
    assert a_v == b_v and (variant is None or a_v == variant), (a_v, b_v, variant)
    assert a_w == b_w, (a_w, b_w)
    assert a_w["shadow_rays"] > 0
    assert np.array_equal(a_rgb, b_rgb), "bytes differ at %d pixels" % int((a_rgb != b_rgb).any(-1).sum())
    assert np.array_equal(a_f, b_f), "float image differs at %d values" % int((a_f != b_f).sum())


def test_headline_frame_is_unchanged(gpu, monkeypatch):
    """bench.py --config 3: spheres2.scn 1920x1080 --gillum 16 --shadow, the persistent leaf kernel."""
    same_both_ways(gpu, monkeypatch, skr.parse_scene(scene_path("spheres2.scn")), skr.Options(1920, 1080, gillum=16, shadow=True, seed=20261004),
                   {}, "node_levels_v5")


@pytest.mark.parametrize("kw,env,variant", [
    (dict(gillum=4, shadow=True, seed=3), {"SKR_FLAT": "1"}, "node_levels_v5_flat"),
    (dict(gillum=3, depth=5, shadow=True, seed=4), {"SKR_FLAT": "0"}, "node_levels_v5"),       # activate kernel levels
    (dict(gillum=4, depth=4, shadow=True, seed=5), {"SKR_PIPELINE": "generic"}, "level_pipeline_g1"),
])
def test_node_and_general_pipelines_are_unchanged(gpu, monkeypatch, kw, env, variant):
    same_both_ways(gpu, monkeypatch, skr.parse_scene(scene_path("spheres2.scn")), skr.Options(480, 270, **kw), env, variant)


@pytest.mark.parametrize("name,kw", [("test.scn", dict(gillum=4, shadow=True, seed=6)),
                                     ("test.scn", dict(gillum=2, depth=3, shadow=True, shade_triangles=True, seed=7)),
                                     ("spheres1.scn", dict(gillum=4, depth=3, shadow=True, legacy_reflect=True, seed=8)),
                                     ("bear.scn", dict(gillum=4, shadow=True, seed=9))])
def test_other_scenes_and_modes_are_unchanged(gpu, monkeypatch, name, kw):
    same_both_ways(gpu, monkeypatch, skr.parse_scene(scene_path(name)), skr.Options(320, 180, **kw), {})


def test_fog_frame_is_unchanged(gpu, monkeypatch):
    same_both_ways(gpu, monkeypatch, skr.parse_scene(scene_path("spheres2.scn"), fog=True), skr.Options(320, 180, gillum=4, shadow=True, seed=10),
                   {}, "level_pipeline_g1")


@pytest.mark.parametrize("seed", range(4))
def test_random_sphere_scenes_are_unchanged(gpu, monkeypatch, tmp_path, seed):
    """Up to 32 spheres of any size, one or two lights, sometimes inside a sphere."""
    rng = np.random.default_rng(7000 + seed)
    lines = ["camera 0 2 -10 0 -.1 .9 0 1 0 30", "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1", "sphere 0 -40 0 40"]
    lights = [rng.uniform(-6, 6, 3) + [0, 6, 0] for _ in range(int(rng.integers(1, 3)))]
    for i in range(int(rng.integers(1, 32))):
        c, rad = rng.uniform(-6, 6, 3) + [0, 2, 3], 10.0 ** rng.uniform(-1.5, 0.2)
        if i == 0 and seed % 2:
            c, rad = lights[0] + rng.normal(size=3) * 0.2, 0.8
        lines.append("material %g %g %g %g %g %g .2 .2 .2 8 0 0 0 1" % (*rng.random(3), *rng.random(3)))
        lines.append("sphere %.7g %.7g %.7g %.7g" % (*c, rad))
    lines += ["point_light .8 .8 .8 %.7g %.7g %.7g" % tuple(lp) for lp in lights]
    path = os.path.join(str(tmp_path), "s.scn")
    open(path, "w").write("\n".join(lines) + "\n")
    scene = skr.parse_scene(path)
    assert scene.shadow_masks()[0].shape[0] == len(lights)
    for env in ({"SKR_FLAT": "0"}, {"SKR_PIPELINE": "generic"}):
        same_both_ways(gpu, monkeypatch, scene, skr.Options(240, 136, gillum=4, shadow=True, seed=seed), env)
