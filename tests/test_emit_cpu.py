"""Emissive spheres on the host (no GPU; include/skr.h skr_scene_set_sphere_emission): the CPU checker pinned to the
texture checker and the frozen oracle — an all-zero emission is their frame; without --gillum the frame is the emission-free one plus e
at the emitters' pixels and nowhere else; in a dark scene an emitter's pixels are e itself, and under --gillum the surfaces next to it
are lit — the reach conditions of every frame case tests/test_emit_gpu.py renders, and the host side: the ABI's errors and round trips,
the parser's `emission` lines, the refused combinations that need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import render_cli
from conftest import ROOT, scene_path
from emit_cases import CASES, GROUND, GROUND_MID, MID, SMALL_ALONE, checker_frame, load, scene_flags, scene_texts
from emit_check import build as build_checker, emission_scene_text, scene_text
from oracle import pyoracle

f32 = np.float32
W, H = 48, 36
MODES = [("shadow", dict(shadow=True)), ("gi2_d3", dict(gillum=2, depth=3, shadow=True, seed=5)), ("js2", dict(jsample=2, shadow=True, seed=3))]
# no lights, no ambient light, a black background: whatever is seen was emitted
DARK = "camera 0 1.5 -9 0 -0.1 1 0 1 0 30\nbackground 0 0 0\nambient_light 0 0 0\n" + "".join(
    ln + "\n" for ln in scene_text().split("\n") if ln.startswith(("material", "sphere")))


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("emitcheck")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="session")
def scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("emit_scenes")
    out = {}
    for name, text in dict(scene_texts(), dark=DARK).items():
        p = d / (name + ".scn")
        p.write_text(text)
        out[name] = str(p)
    return out


def emitters_of(e, winners):
    """bool per ray: its primary winner is a sphere with an emission component > 0"""
    glow = (np.asarray(e, f32).reshape(-1, 3) > 0).any(1)
    return (winners >= 0) & glow[np.clip(winners, 0, None)]


# ---- 1. the checker against the texture checker and the frozen oracle ----
@pytest.mark.parametrize("name,kw", MODES, ids=[m[0] for m in MODES])
def test_an_all_zero_emission_is_the_texture_checker_and_the_oracle_frame(checker, scenes, name, kw):
    o_rgb, o_f, o_st = pyoracle.render(scenes["three"], W, H, want_float=True, **kw)
    t_rgb, t_f, t_st = checker.without_the_add().render(scenes["three"], W, H, **kw)
    assert np.array_equal(bits(t_f), bits(o_f)) and t_st[:5].tolist() == o_st.tolist()
    for e in (None, np.zeros((4, 3), f32), np.full((4, 3), -0.0, f32)):  # none; zeros; -0: x + (-0) = x
        rgb, f, st = checker.render(scenes["three"], W, H, emission=e, **kw)
        assert np.array_equal(bits(f), bits(t_f)) and np.array_equal(rgb, t_rgb) and st[:8].tolist() == t_st.tolist() and st[8] == 0
        assert np.array_equal(bits(f), bits(o_f)) and np.array_equal(rgb, o_rgb) and st[:5].tolist() == o_st.tolist()
    tex = dict(textures=[np.full((2, 2, 3), 0.5, f32)], sphere_textures=[0, -1, 0, 0])  # ... and on textured spheres
    want = checker.without_the_add().render(scenes["three"], W, H, **tex, **kw)
    got = checker.render(scenes["three"], W, H, emission=np.zeros((4, 3), f32), **tex, **kw)
    assert np.array_equal(bits(got[1]), bits(want[1])) and got[2][:8].tolist() == want[2].tolist() and want[2][7] > 0


# ---- 2. what the add does to a frame ----
@pytest.mark.parametrize("name,kw", [MODES[0], MODES[2], ("plain", dict())], ids=["shadow", "js2", "plain"])
def test_without_gillum_only_the_emitters_pixels_change_and_by_exactly_e(checker, scenes, name, kw):
    e = np.array(GROUND_MID, f32)
    win = []
    rgb, f, st = checker.render(scenes["three"], W, H, emission=e, winners=win, **kw)
    _, f0, st0 = checker.render(scenes["three"], W, H, **kw)
    assert st[:8].tolist() == st0[:8].tolist() and st[8] > 0  # rays, hits, shadow rays, tests: all counters are equal
    if kw.get("jsample"):
        return  # (a pixel is a mean of samples: the per-sample statement below is made on the samples)
    w0 = win[0].reshape(H, W)
    glow = emitters_of(e, w0)
    assert glow.sum() * 10 >= W * H and (~glow).sum() > 0
    assert np.array_equal(bits(f[~glow]), bits(f0[~glow]))  # nothing else changes
    assert np.array_equal(bits(f[glow]), bits(f0[glow] + e[w0[glow]]))  # fl(base + e), one add per component
    assert (bits(f[glow]) != bits(f0[glow])).any(1).all()


def test_the_samples_of_an_antialiased_frame_change_by_exactly_e(checker, scenes):
    kw = dict(jsample=2, shadow=True, seed=3)
    e = np.array(GROUND_MID, f32)
    win = []
    with_e = checker.render_samples(scenes["three"], W, H, emission=e, winners=win, **kw)
    without = checker.render_samples(scenes["three"], W, H, **kw)
    assert len(with_e) == 4
    for (c, _), (c0, _), w0 in zip(with_e, without, win):
        glow = emitters_of(e, w0)
        assert np.array_equal(bits(c[~glow]), bits(c0[~glow])) and np.array_equal(bits(c[glow]), bits(c0[glow] + e[w0[glow]]))


def test_in_a_dark_scene_an_emitters_pixels_are_e_itself(checker, scenes):
    e = np.array([(0.25, 0, 3.5), (0, 0, 0), (1e-3, 7.0, 0.1), (0, 0, 0)], f32)
    win = []
    _, f, st = checker.render(scenes["dark"], W, H, emission=e, winners=win, depth=1)
    w0 = win[0].reshape(H, W)
    glow = emitters_of(e, w0)
    assert glow.sum() >= 40 and len(set(w0[glow].tolist())) == 2
    assert np.array_equal(bits(f[glow]), bits(e[w0[glow]]))
    assert (f[~glow] == 0).all()
    _, fg, _ = checker.render(scenes["dark"], W, H, emission=e, gillum=4, depth=1, seed=3)  # depth 1: the children are shade(depth 0) = 0, so (0 / pi + 0) * kd + e
    assert np.array_equal(bits(fg[glow]), bits(e[w0[glow]])) and (fg[~glow] == 0).all()


def test_under_gillum_an_emitter_lights_the_surfaces_next_to_it(checker, scenes):
    """a room lit only by its objects: the ground glows, the three spheres do not, and their pixels are strictly positive"""
    e = np.array([(0, 0, 0), (0, 0, 0), (0, 0, 0), (1.0, 0.5, 0.25)], f32)
    win = []
    kw = dict(gillum=8, depth=2, seed=2)
    _, f, st = checker.render(scenes["dark"], W, H, emission=e, winners=win, **kw)
    _, f0, st0 = checker.render(scenes["dark"], W, H, **kw)
    assert (f0 == 0).all() and st[:8].tolist() == st0[:8].tolist()
    w0 = win[0].reshape(H, W)
    balls = (w0 >= 0) & (w0 < 3)
    assert balls.sum() >= 40
    # lit through --gillum children that hit the ground.  A ball's top sees only the sky and stays black; at a normal with N.y <= 0 half the
    # hemisphere or more looks at the ground, so one of 8 children hits it but for a chance of 2^-8.  The camera stands a little above the
    # balls' centres, so such normals fill somewhat less than the lower half of each disc: more than a third of the balls' pixels.
    assert (f[balls] > 0).all(1).mean() >= 1 / 3
    near = np.zeros_like(balls)  # a ball's pixel with the ground as its left, right, upper or lower neighbour: next to the emitter
    near[:-1] |= balls[:-1] & (w0[1:] == 3)
    near[1:] |= balls[1:] & (w0[:-1] == 3)
    near[:, :-1] |= balls[:, :-1] & (w0[:, 1:] == 3)
    near[:, 1:] |= balls[:, 1:] & (w0[:, :-1] == 3)
    # (not all of them: a child starts at P + 0.00001 per component, raytrace.h:127, which under a normal that points down lies inside
    # the ball, and such a child ends on the ball's own inside at depth 0)
    assert near.sum() >= 10 and (f[near] > 0).all(1).sum() >= 5
    _, f1, _ = checker.render(scenes["dark"], W, H, emission=e, **dict(kw, gillum=None))  # and without --gillum they stay black
    assert (f1[balls] == 0).all() and (f1[w0 == 3] == e[3]).all()


def test_the_emission_moves_with_its_sphere(checker, scenes):
    e = np.array(MID, f32)
    v = np.zeros((4, 3), f32)
    v[1] = (3.0, 0.5, 0)
    win, still = [], []
    _, f, _ = checker.render(scenes["dark"], W, H, emission=e, winners=win, velocities=v, shutter=1.0, depth=1, seed=9)
    checker.render(scenes["dark"], W, H, emission=e, winners=still, depth=1, seed=9)
    w0, s0 = win[0].reshape(H, W), still[0].reshape(H, W)
    glow = w0 == 1
    assert (glow & (s0 != 1)).sum() >= 20 and ((s0 == 1) & ~glow).sum() >= 5  # the streak leaves the disc the sphere has at rest
    assert np.array_equal(bits(f[glow]), bits(np.broadcast_to(e[1], (int(glow.sum()), 3)))) and (f[~glow] == 0).all()


def test_a_textured_emitter_keeps_its_emission(checker, scenes):
    """the texture primes kd and the ambient row; e is added behind, untouched"""
    e = np.array(GROUND_MID, f32)
    tex = dict(textures=[np.full((2, 2, 3), 0.5, f32), np.random.default_rng(5).uniform(0.25, 2, (3, 3, 3)).astype(f32)], sphere_textures=[0, 1, -1, 0])
    kw = dict(shadow=True)
    win = []
    _, f, st = checker.render(scenes["three"], W, H, emission=e, winners=win, **tex, **kw)
    _, ft, stt = checker.without_the_add().render(scenes["three"], W, H, **tex, **kw)
    _, fe, _ = checker.render(scenes["three"], W, H, emission=e, **kw)
    w0 = win[0].reshape(H, W)
    glow = emitters_of(e, w0)
    assert st[:8].tolist() == stt.tolist() and st[7] > 0
    assert np.array_equal(bits(f[glow]), bits(ft[glow] + e[w0[glow]])) and np.array_equal(bits(f[~glow]), bits(ft[~glow]))
    assert (bits(f[glow]) != bits(fe[glow])).any()  # and the texture shows on the emitter


# ---- 3. the reach conditions of every frame case the GPU file renders ----
@pytest.mark.parametrize("name,scn,size,setup,kw", CASES, ids=[c[0] for c in CASES])
def test_the_gpu_cases_reach_their_emitters(checker, scenes, name, scn, size, setup, kw):
    w, h = size
    given, told = scene_flags(setup)
    sc = load(scenes, scn, **given)
    e = sc.emission
    win = []
    _, f, st = checker_frame(checker, scenes, sc, scn, w, h, winners=win, **told, **kw)
    _, f0, st0 = checker_frame(checker, scenes, sc, scn, w, h, emission=None, **told, **kw)
    assert st[:8].tolist() == st0[:8].tolist()
    share = np.mean([emitters_of(e, w0).mean() for w0 in win])
    differ = (bits(f) != bits(f0)).any(2).reshape(-1)
    other = np.all([(w0 != -1) & ~emitters_of(e, w0) for w0 in win], axis=0)  # pixels every sample of which wins on a surface that does not glow
    print("%s: primary share %.3f, pixels on other surfaces %d, of which differ %d" % (name, share, other.sum(), (differ & other).sum()))
    assert share >= 0.10, "at least a tenth of the primary rays win on an emitter"
    ground = sc.info.n_spheres == 4 and (e[3] > 0).any() and sc.info.n_triangles == 0
    if kw.get("gillum") and ground:
        assert other.sum() > 0 and (differ & other).sum() * 10 >= other.sum(), "a tenth of the pixels on non-emitting surfaces differ"
    if name == SMALL_ALONE:
        assert size == (64, 48) and kw["gillum"] == 4 and (e > 0).any(1).tolist() == [False, True, False, False]
        assert (differ & other).sum() >= 16, "16 pixels on non-emitting surfaces differ"


# ---- 4. the ABI ----
def test_the_abi_clause_by_clause():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    ns = sc.info.n_spheres
    L = skr.lib()
    assert sc.emission.shape == (ns, 3) and (sc.emission == 0).all()  # the default
    e = np.random.default_rng(1).uniform(0, 4, (ns, 3)).astype(f32)
    e[2] = (0.0, -0.0, 1e-30)
    sc.set_emission(e)
    assert np.array_equal(bits(sc.emission), bits(e)) and np.signbit(sc.emission[2, 1])  # a round trip; -0 is stored as given
    n = C.c_int32(-1)
    assert L.skr_scene_get_sphere_emission(sc.h, None, C.byref(n)) == 0 and n.value == ns  # null rgb: the count only
    for bad in (e[:-1], np.concatenate([e, e[:1]])):  # n != the sphere count
        with pytest.raises(skr.SkrError) as err:
            sc.set_emission(bad)
        assert "(status 2)" in str(err.value) and np.array_equal(bits(sc.emission), bits(e))
    assert L.skr_scene_set_sphere_emission(sc.h, e.ctypes.data, -1) == 2 and np.array_equal(bits(sc.emission), bits(e))
    for v in (np.nan, np.inf, -np.inf, -1.0, -1e-45):  # a value that is not finite, a negative value (the smallest denormal too)
        bad = e.copy()
        bad[ns - 1, 2] = v
        with pytest.raises(skr.SkrError) as err:
            sc.set_emission(bad)
        assert "(status 2)" in str(err.value) and np.array_equal(bits(sc.emission), bits(e)), v  # the scene is unchanged
    assert L.skr_scene_set_sphere_emission(None, e.ctypes.data, ns) == 2 and L.skr_scene_get_sphere_emission(None, None, None) == 2
    assert L.skr_scene_set_sphere_emission(sc.h, None, ns) == 0 and (sc.emission == 0).all() and not np.signbit(sc.emission).any()  # NULL clears
    sc.set_emission(e)
    assert L.skr_scene_set_sphere_emission(sc.h, e.ctypes.data, 0) == 0 and (sc.emission == 0).all()  # n == 0 clears
    sc.set_emission(e)
    sc.set_emission(None)
    assert (sc.emission == 0).all()
    cam = list(sc.info.camera)[:9]
    sa = skr.Scene.from_arrays(np.zeros((2, 14), f32), np.zeros((0, 9), f32), np.zeros((0, 6), f32), cam)
    assert (sa.emission == 0).all() and sa.emission.shape == (2, 3)  # scenes from arrays start with no emission
    sa = skr.Scene.from_arrays(np.zeros((2, 14), f32), np.zeros((0, 9), f32), np.zeros((0, 6), f32), cam, emission=[(1, 2, 3), (0, 0, 0.5)])
    assert sa.emission.tolist() == [[1, 2, 3], [0, 0, 0.5]]


def test_the_header_announces_the_addition():
    text = open(os.path.join(ROOT, "include", "skr.h")).read()
    assert "#define SKR_HAS_EMISSION 1" in text and "#define SKR_SCN_EMISSION 128u" in text
    for name in ("skr_scene_set_sphere_emission", "skr_scene_get_sphere_emission"):
        assert name in text and name in skr.EXPORTED_SYMBOLS
    assert skr.binding.SCN_EMISSION == 128


# ---- 5. the parser ----
def test_the_emission_line_is_stateful_and_zeros_end_it(tmp_path):
    scn = tmp_path / "s.scn"
    scn.write_text("sphere 0 0 0 1\nemission 1 0.5 0.25\nsphere 1 0 0 1\nmaterial .1 .1 .1 .2 .2 .2 0 0 0 1 0 0 0 1\nsphere 2 0 0 1\nemission 0 0 7\nsphere 3 0 0 1\n"
                   "emission 0 0 0\nsphere 4 0 0 1\nemission 2 2 2 trailing words\nsphere 5 0 0 1\n")
    sc = skr.parse_scene(str(scn), emission=True)
    assert sc.emission.tolist() == [[0, 0, 0], [1, 0.5, 0.25], [1, 0.5, 0.25], [0, 0, 7], [0, 0, 0], [2, 2, 2]] and sc.info.n_unknown == 0
    assert text_of(emission_scene_text(GROUND_MID), tmp_path).emission.tolist() == np.array(GROUND_MID, f32).tolist()


def text_of(text, tmp_path):
    p = tmp_path / "t.scn"
    p.write_text(text)
    return skr.parse_scene(str(p), emission=True)


def test_lines_that_are_skipped_are_counted_and_leave_the_emission_in_force(tmp_path, capfd):
    scn = tmp_path / "s.scn"
    scn.write_text("emission 1 2 3\nsphere 0 0 0 1\nemission\nsphere 1 0 0 1\nemission 1 2\nsphere 2 0 0 1\nemission 1 -2 3\nsphere 3 0 0 1\nemission nan 0 0\nemission 0 inf 0\n"
                   "emission a b c\nsphere 4 0 0 1\nemission 0 0 0\nsphere 5 0 0 1\nemission -1 0 0\nsphere 6 0 0 1\n")
    sc = skr.parse_scene(str(scn), emission=True)
    assert sc.info.n_unknown == 7
    assert sc.emission.tolist() == [[1, 2, 3]] * 5 + [[0, 0, 0]] * 2
    assert capfd.readouterr().err.count("WARNING. emission") == 7


def test_without_the_flag_the_line_is_an_unknown_command(tmp_path):
    body = "camera 0 0 -6 0 0 1 0 1 0 20\n%s 1 2 3\nsphere 0 0 0 1\n%s 0 0 0\nsphere 1 0 0 1\n%s\n"
    (tmp_path / "emit.scn").write_text(body % ("emission", "emission", "emission"))
    (tmp_path / "bogus.scn").write_text(body % ("emissiom", "emissiom", "emissiom"))
    sc = skr.parse_scene(str(tmp_path / "emit.scn"))
    assert sc.info.n_unknown == 3 and (sc.emission == 0).all()
    other = skr.parse_scene(str(tmp_path / "bogus.scn"))
    assert bytes(sc.info) == bytes(other.info)  # skr_scene_info is what it is for any unknown command
    code = "import sys, skele_raytracer_amd as skr; skr.parse_scene(sys.argv[1], echo=True)"
    outs = [subprocess.run([sys.executable, "-c", code, str(tmp_path / n)], cwd=ROOT, capture_output=True, timeout=120, check=True) for n in ("emit.scn", "bogus.scn")]
    assert outs[0].stdout.count(b"WARNING. Do not know command: emission\n") == 3
    assert outs[0].stdout == outs[1].stdout.replace(b"emissiom", b"emission") and outs[0].stderr == outs[1].stderr  # byte for byte an unknown command's output


def test_both_command_lines_parse_the_flag():
    base = ["--path", scene_path("spheres2.scn"), "--output", "out.ppm"]
    assert "scn_emission" not in render_cli._parse(base) and render_cli._parse(base + ["--scn-emission"])["scn_emission"] is True
    assert "--scn-emission" in open(os.path.join(ROOT, "skele_raytracer_amd", "csrc", "raytracer_main.cpp")).read()


# ---- 6. the refused combinations that the host alone decides (launch_params on the packed scene, nothing uploaded) ----
def plan(scene, **kw):
    fn = skr.lib().skr_scene_leaf_shape
    fn.argtypes = [C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    rc = fn(scene.h, C.byref(skr.Options(32, 24, **kw).c))
    return rc, (skr.lib().skr_last_error() or b"").decode()


def test_the_refused_combinations():
    fog_rows = np.array([[0, 0, 5, 3, .5, .5, .5, .1, .05]], f32)

    def cases():
        def glowing(**flags):
            sc = skr.parse_scene(scene_path("spheres2.scn"), **flags)
            e = sc.emission
            e[3, 1] = 0.5
            sc.set_emission(e)
            return sc
        fog = glowing(fog=True)
        fog.set_fog(fog_rows)
        return [(glowing(), dict(legacy_reflect=True), "--legacy-reflect"), (fog, dict(), "fog volumes"), (glowing(sphere_tree=True), dict(), "sphere tree")]

    for sc, kw, text in cases():
        rc, why = plan(sc, **kw)
        assert rc == -4 and "sphere emission (--scn-emission)" in why and text in why, (rc, why)
        sc.set_emission(np.full((sc.info.n_spheres, 3), -0.0, f32))  # none of them is refused once no component is > 0: the emission is not in force
        assert plan(sc, **kw)[0] >= 0
    ok = cases()[0][0]
    for kw in (dict(shadow=True), dict(gillum=2, depth=3), dict(jsample=2), dict(shade_triangles=True, shadow=True)):
        assert plan(ok, **kw)[0] >= 0
