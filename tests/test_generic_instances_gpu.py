"""The instance table of the general level pipeline (render_generic.hip with_pack, launch.h GenericFeatures), walked once: every tail
{plain, fog, sphere tree, sphere tree + fog, spot, soft, soft + spot} with and without triangle shadows renders a frame and answers the
query of that frame's camera rays — under the names skr_kernel_variant() has for them, bit for bit the same values, the same work
counters — and every combination the launch refuses is refused with its text."""
import numpy as np
import pytest

import skele_raytracer_amd as skr
from test_shade_query_gpu import assert_bitwise, frame_and_query

pytestmark = pytest.mark.gpu

W, H = 64, 32
CAMERA = [0, 0, -10, 0, 0, 1, 0, 1, 0]
# centre radius ambient diffuse specular power
SPHERES = np.array([
    [-1.6, 0.2, 0.5, 1.0, 0.05, 0.02, 0.02, 0.8, 0.3, 0.2, 0.5, 0.5, 0.5, 24],
    [0.3, -0.3, -0.4, 0.8, 0.02, 0.05, 0.02, 0.2, 0.8, 0.3, 0.3, 0.3, 0.3, 12],
    [1.8, 0.5, 1.0, 1.1, 0.02, 0.02, 0.05, 0.3, 0.3, 0.9, 0.0, 0.0, 0.0, 1],
], np.float32)
# a floor of two triangles under the spheres, one triangle between the lights and the spheres, one behind them
TRIANGLES = np.array([
    [-5, -1.4, -4, 5, -1.4, -4, 5, -1.4, 6],
    [-5, -1.4, -4, 5, -1.4, 6, -5, -1.4, 6],
    [-1.5, 2.2, -0.5, 0.5, 2.2, -0.5, -0.5, 2.2, 1.5],
    [-3, -1, 4, 3, -1, 4, 0, 3, 4],
], np.float32)
TRIANGLE_MATERIALS = np.array([[0.03, 0.03, 0.03, 0.6, 0.6, 0.6, 0.2, 0.2, 0.2, 8]] * 4, np.float32)
# position colour: an odd count, so the pair loops run their single tail
LIGHTS = np.array([
    [-4, 5, -3, 30, 28, 26],
    [0.5, 6, 0.5, 35, 35, 30],
    [4, 4, -4, 20, 24, 30],
], np.float32)
# light 1 as a spot light (colour position direction angle1 angle2): some of the scene inside its inner cone, some in the falloff, some outside
SPOT = np.array([[35, 35, 30, 0.5, 6, 0.5, -0.1, -1, -0.05, 12, 25]], np.float32)
RADIUS = 0.4  # of light 2
FOG = np.array([[-1.6, 0.2, 0.5, 1.6, 0.8, 0.8, 0.9, 0.4, 0.1]], np.float32)  # around sphere 0: centre radius albedo scattering absorption

# tail -> (what the scene switches on, the name's suffix); fog has no name of its own
TAILS = {
    "plain": (dict(), ""),
    "fog": (dict(fog=True), ""),
    "stree": (dict(stree=True), "_stree"),
    "stree_fog": (dict(stree=True, fog=True), "_stree"),
    "spot": (dict(spot=True), "_spot"),
    "soft": (dict(soft=True), "_soft"),
    "soft_spot": (dict(soft=True, spot=True), "_soft"),
}
ROWS = [(tail, False) for tail in TAILS] + [(tail, True) for tail in TAILS if "fog" not in tail]  # (fog excludes shade_triangles)


def scene(spot=False, soft=False, stree=False, fog=False, tshadow=False):
    """the three lights in shading order: point lights first, then the spot light"""
    points = LIGHTS[[0, 2]] if spot else LIGHTS
    sc = skr.Scene.from_arrays(SPHERES, TRIANGLES, points, CAMERA, background=(0.1, 0.1, 0.2), ambient=(1, 1, 1), triangle_materials=TRIANGLE_MATERIALS,
                               triangle_shadows=tshadow, sphere_tree=stree)
    if spot:
        sc.set_spot_lights(SPOT)
    if soft:  # (after the spot lights: setting those resets the radii)
        sc.set_light_radii([0, RADIUS, 0] if spot else [0, 0, RADIUS])
    if fog:
        sc.set_fog(FOG)
    return sc


def options(**kw):
    return skr.Options(W, H, gillum=2, depth=2, shadow=True, seed=29, **kw)


@pytest.mark.parametrize("tail,tshadow", ROWS, ids=["%s%s" % (t, "_tshadow" if ts else "") for t, ts in ROWS])
def test_every_instance_renders_and_answers_its_frame(tail, tshadow, monkeypatch):
    on, suffix = TAILS[tail]
    if not on and not tshadow:  # the plain row: nothing sends its few triangles to the general pipeline but the switch, read when the renderer is made
        monkeypatch.setenv("SKR_PIPELINE", "generic")
    r = skr.Renderer(scene(tshadow=tshadow, **on), 0)
    opt = options(shade_triangles=True) if tshadow else options()
    name = suffix + ("_tshadow" if tshadow else "")
    r.counters(reset=True)
    r.render(opt)
    assert skr.Renderer.kernel_variant() == "level_pipeline_g1" + name
    f, c, q, cq = frame_and_query(r, opt)
    assert skr.Renderer.kernel_variant() == "shade_rays_g1" + name
    assert_bitwise(q, f, "%s tshadow=%s" % (tail, tshadow))
    assert cq == c
    assert c["shadow_rays"] > 0 and (f.reshape(-1, 3) != f.reshape(-1, 3)[0]).any()  # (shadow rays were cast; not a flat image)


SPOT_TEXT = "spot lights (--scn-spot) cannot be combined with "
SOFT_TEXT = "light radii (--light-radius) cannot be combined with "
REFUSED = {
    "spot_stree": (dict(spot=True, stree=True), dict(), SPOT_TEXT + "the sphere tree (--sphere-tree)"),
    "spot_fog": (dict(spot=True, fog=True), dict(), SPOT_TEXT + "fog volumes (--scn-fog)"),
    "spot_legacy": (dict(spot=True), dict(legacy_reflect=True), SPOT_TEXT + "--legacy-reflect"),
    "soft_stree": (dict(soft=True, stree=True), dict(), SOFT_TEXT + "the sphere tree (--sphere-tree)"),
    "soft_fog": (dict(soft=True, fog=True), dict(), SOFT_TEXT + "fog volumes (--scn-fog)"),
    "soft_legacy": (dict(soft=True), dict(legacy_reflect=True), SOFT_TEXT + "--legacy-reflect"),
    "fog_shade_triangles": (dict(fog=True), dict(shade_triangles=True), "fog volumes (--scn-fog) cannot be combined with --legacy-reflect or --shade-triangles"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_combinations_keep_their_text(case):
    on, kw, text = REFUSED[case]
    r = skr.Renderer(scene(**on), 0)
    with pytest.raises(skr.SkrError) as frame:
        r.render(options(**kw))
    assert str(frame.value).split("): ", 1)[1] == text  # (behind the binding's "<call> failed (status N): ")
    with pytest.raises(skr.SkrError) as query:
        r.shade(r.camera_rays(options()).view(-1, 8), options(**kw), 0)
    assert str(query.value).split("): ", 1)[1] == text
