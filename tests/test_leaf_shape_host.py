"""Which launches get the leaf kernel's instance with their shape compiled in (csrc/launch.h skr_leaf_shape, DESIGN.md 5.2 "Launch
shapes") — no GPU.

A shape is a set of facts the instance holds as constants (csrc/shade_common.h PointLightShape<1 | 2>): one or two lights, all of them
point lights with their shadow masks, shadows on, integer Phong exponents below 128, 16-bit GI masks, no triangles.  The dispatch must
name a shape only where EVERY fact holds, since the instance no longer looks: each of the launches below that breaks exactly one fact
must get the instance that reads the facts at run time (0).  The entry, skr_scene_leaf_shape (internal), runs the host side of a
launch — the packed scene, the SKR_* switches of the environment, launch_params — and uploads nothing.
"""
import ctypes as C
import os

import pytest

import skele_raytracer_amd as skr
from conftest import scene_path

RUNTIME, POINT1, POINT2 = 0, 1, 2  # launch.h SkrLeafShape
SWITCHES = ("SKR_LEAF_SHAPE", "SKR_GI_MASK", "SKR_SHADOW_MASK", "SKR_GI_SURFACE", "SKR_SHADOW_SURFACE", "SKR_PIPELINE", "SKR_FLAT")


def write_scene(path, spheres=5, lights=2, power=32, directional=False, triangle=False):
    """A ground sphere and spheres - 1 small ones over it (fixed places: no randomness), `lights` point lights."""
    lines = ["camera 0 2 -10 0 -.1 .9 0 1 0 30", "ambient_light .3 .3 .3", "background .2 .3 .5",
             "material .6 .6 .6 .7 .7 .7 .2 .2 .2 %g 0 0 0 1" % power, "sphere 0 -40 0 40"]
    for i in range(spheres - 1):
        x, z = -4.5 + 3.0 * (i % 4), 1.0 + 2.5 * (i // 4)
        lines.append("material .5 .4 .%d .%d .6 .5 .3 .3 .3 %g 0 0 0 1" % (1 + i % 9, 9 - i % 9, power if i % 2 else 8))
        lines.append("sphere %g %g %g %g" % (x, 0.5 + 0.1 * (i % 3), z, 0.5 + 0.1 * (i % 3)))
    for l in range(lights):
        lines.append("point_light .8 .%d .7 %g 9 %g" % (8 - l, 2.0 - 3.0 * l, -1.0 - l))
    if directional:
        lines.append("directional_light .5 .5 .5 0 -1 .2")
    if triangle:
        lines += ["vertex -1 0 0", "vertex 1 0 0", "vertex 0 2 0", "triangle 0 1 2"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def leaf_shape(scene, opt):
    fn = skr.lib().skr_scene_leaf_shape
    fn.argtypes = [C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    got = fn(scene.h, C.byref(opt.c))
    assert got >= 0, "skr_scene_leaf_shape failed: %d" % got
    return got


@pytest.fixture
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def opts(**kw):
    return skr.Options(64, 36, **dict(dict(gillum=4, depth=3, shadow=True, seed=5), **kw))


def test_spheres2_gets_the_two_light_shape(clean_env):
    """The headline scene: 15 spheres, two point lights, exponents below 128."""
    assert leaf_shape(skr.parse_scene(scene_path("spheres2.scn")), opts(gillum=16)) == POINT2


def test_generated_scenes_get_their_shapes(clean_env, tmp_path):
    p = str(tmp_path)
    assert leaf_shape(skr.parse_scene(write_scene(os.path.join(p, "two.scn"), lights=2)), opts()) == POINT2
    assert leaf_shape(skr.parse_scene(write_scene(os.path.join(p, "one.scn"), lights=1)), opts()) == POINT1
    assert leaf_shape(skr.parse_scene(write_scene(os.path.join(p, "sixteen.scn"), spheres=16)), opts()) == POINT2  # (the last count with 16-bit masks)
    assert leaf_shape(skr.parse_scene(write_scene(os.path.join(p, "p127.scn"), power=127)), opts()) == POINT2     # (the last exponent of 7 bits)


@pytest.mark.parametrize("what, scene_kw, parse_kw, opt_kw", [
    ("three lights", dict(lights=3), {}, {}),
    ("a directional light", dict(lights=1, directional=True), dict(strict=True), {}),
    ("shadows off", {}, {}, dict(shadow=False)),
    ("pow_steps = 8", dict(power=128), {}, {}),
    ("17 spheres: 32-bit GI masks", dict(spheres=17), {}, {}),
    ("a triangle", dict(triangle=True), {}, {}),
])
def test_one_broken_fact_gets_the_run_time_instance(clean_env, tmp_path, what, scene_kw, parse_kw, opt_kw):
    scene = skr.parse_scene(write_scene(os.path.join(str(tmp_path), "s.scn"), **scene_kw), **parse_kw)
    assert leaf_shape(scene, opts(**opt_kw)) == RUNTIME, what
    # ... and the same scene without the broken fact is one the dispatch does take: the case tests that fact, not another
    base = skr.parse_scene(write_scene(os.path.join(str(tmp_path), "b.scn"), lights=min(scene_kw.get("lights", 2), 2)))
    assert leaf_shape(base, opts()) in (POINT1, POINT2), what


def test_the_directional_light_counts_only_under_strict(clean_env, tmp_path):
    """Without --strict-scn the loader drops the directional light (as the reference does): one point light, its shape."""
    scene = skr.parse_scene(write_scene(os.path.join(str(tmp_path), "s.scn"), lights=1, directional=True))
    assert leaf_shape(scene, opts()) == POINT1


@pytest.mark.parametrize("switch", ["SKR_GI_MASK", "SKR_LEAF_SHAPE", "SKR_SHADOW_MASK"])
def test_switches_force_the_run_time_instance(clean_env, switch):
    """SKR_GI_MASK=0: the kernels without the masked walk have no shaped instance; SKR_SHADOW_MASK=0: the shape compiles the masks
    in; SKR_LEAF_SHAPE=0: the A/B switch itself.  =1 is the default."""
    scene, opt = skr.parse_scene(scene_path("spheres2.scn")), opts()
    clean_env.setenv(switch, "0")
    assert leaf_shape(scene, opt) == RUNTIME
    clean_env.setenv(switch, "1")
    assert leaf_shape(scene, opt) == POINT2


def test_surface_patches_are_no_fact_of_the_shape(clean_env):
    """The shaped instances read at run time whether the launch has surface patches: without them the shape stays."""
    scene, opt = skr.parse_scene(scene_path("spheres2.scn")), opts()
    clean_env.setenv("SKR_GI_SURFACE", "0")
    clean_env.setenv("SKR_SHADOW_SURFACE", "0")
    assert leaf_shape(scene, opt) == POINT2
