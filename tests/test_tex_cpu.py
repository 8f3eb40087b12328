"""Sphere textures on the host (no GPU; include/skr.h skr_scene_add_texture): the CPU checker pinned to the frozen
oracle — a texture of ones is the untextured frame, a texture of 0.5 is the scene whose kd and ka are halved (exact only for a power of
two, which is the reason for the choice), E = 1, -0 texels, mixed textured and untextured spheres — and the host side: the ABI's errors
and round trips, the parser's `texture` lines, the refused combinations that need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import render_cli
from conftest import ROOT, scene_path
from oracle import pyoracle
from tex_check import TEX_MAX, TEX_MAX_EDGE, build as build_checker, debug_texture, decision_normals, scene_text

f32 = np.float32
W, H = 48, 36
MODES = [("shadow", dict(shadow=True)), ("gi2_d3", dict(gillum=2, depth=3, shadow=True, seed=5)), ("js2", dict(jsample=2, shadow=True, seed=3))]


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("texcheck")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="session")
def scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("tex_scenes")
    out = {}
    for name, scale in (("base", (1, 1, 1)), ("half", (0.5, 0.5, 0.5)), ("half_mid", (1, 0.5, 1)), ("black", (0, 0, 0))):
        p = d / (name + ".scn")
        p.write_text(scene_text(scale))
        out[name] = str(p)
    return out


def frames_equal(a, b):
    return np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[0], b[0]) and a[2][:7].tolist() == b[2][:7].tolist()


# ---- 1. the checker against the frozen oracle ----
@pytest.mark.parametrize("name,kw", MODES, ids=[m[0] for m in MODES])
def test_a_texture_of_ones_is_the_oracle_frame(checker, scenes, name, kw):
    o_rgb, o_f, o_st = pyoracle.render(scenes["base"], W, H, want_float=True, **kw)
    for E in (1, 3):
        rgb, f, st = checker.render(scenes["base"], W, H, textures=[np.ones((E, E, 3), f32)], sphere_textures=[0, 0, 0, 0], **kw)
        assert np.array_equal(bits(f), bits(o_f)) and np.array_equal(rgb, o_rgb) and st[:5].tolist() == o_st.tolist(), E
        assert st[7] == st[1] > 0  # every shaded hit looked its texture up
    rgb, f, st = checker.render(scenes["base"], W, H, **kw)  # and without textures the restated shade tree is the oracle's too
    assert np.array_equal(bits(f), bits(o_f)) and st[:5].tolist() == o_st.tolist() and st[7] == 0
    rgb, f, st = checker.render(scenes["base"], W, H, textures=[np.full((2, 2, 3), 7.0, f32)], sphere_textures=[-1, -1, -1, -1], **kw)  # a texture no sphere names
    assert np.array_equal(bits(f), bits(o_f)) and st[7] == 0


@pytest.mark.parametrize("name,kw", MODES, ids=[m[0] for m in MODES])
def test_a_texture_of_one_half_is_the_scene_with_kd_and_ka_halved(checker, scenes, name, kw):
    half = pyoracle.render(scenes["half"], W, H, want_float=True, **kw)
    base = pyoracle.render(scenes["base"], W, H, want_float=True, **kw)
    assert (bits(half[1]) != bits(base[1])).any()
    for E in (1, 2, 64):  # E = 1: every lookup is texel (0, 0)
        rgb, f, st = checker.render(scenes["base"], W, H, textures=[np.full((E, E, 3), 0.5, f32)], sphere_textures=[0, 0, 0, -1], **kw)
        assert np.array_equal(bits(f), bits(half[1])) and np.array_equal(rgb, half[0]) and st[:5].tolist() == half[2].tolist(), E


def test_mixed_textured_and_untextured_spheres(checker, scenes):
    kw = dict(gillum=2, depth=3, shadow=True, seed=5)
    want = pyoracle.render(scenes["half_mid"], W, H, want_float=True, **kw)
    tex = [np.full((3, 3, 3), 2.0, f32), np.full((2, 2, 3), 0.5, f32)]  # texture 0 is held and not used
    rgb, f, st = checker.render(scenes["base"], W, H, textures=tex, sphere_textures=[-1, 1, -1, -1], **kw)
    assert np.array_equal(bits(f), bits(want[1])) and np.array_equal(rgb, want[0]) and st[:5].tolist() == want[2].tolist()
    assert 0 < st[7] < st[1]


def test_texels_of_minus_zero_are_a_black_albedo(checker, scenes):
    """-0 texels look up as +0 (top = -0 + fx * (+0)), so kd' = ka' = +0: the scene whose spheres have kd = ka = 0"""
    kw = dict(gillum=2, depth=2, shadow=True, seed=4)
    want = pyoracle.render(scenes["black"], W, H, want_float=True, **kw)
    for E in (1, 2):
        rgb, f, st = checker.render(scenes["base"], W, H, textures=[np.full((E, E, 3), -0.0, f32)], sphere_textures=[0, 0, 0, -1], **kw)
        assert np.array_equal(bits(f), bits(want[1])) and st[:5].tolist() == want[2].tolist(), E
    assert not np.signbit(checker.colour(np.full((2, 2, 3), -0.0, f32), decision_normals(2)[:6])).any()


def test_the_colour_is_the_environment_lookup_with_a_fallback_of_ones(checker):
    for k in range(4):
        tex = debug_texture(k)
        N = decision_normals(tex.shape[0])
        got = checker.colour(tex, N)
        env = checker.lookup(tex, N, background=(1, 1, 1))
        assert np.array_equal(bits(got), bits(env))
        flags = checker.taps(N, tex.shape[0])[:, 0]
        assert flags.sum() >= 6 and np.array_equal(got[flags == 1], np.ones((int(flags.sum()), 3), f32))  # zero, NaN, inf, overflow
        assert (got[flags == 0, 0] >= 1).all() and (got[flags == 0, 0] <= tex.shape[0]).all()  # inside the texture's own range: no tap outside it
    one = checker.colour(debug_texture(0), decision_normals(1))
    assert np.array_equal(one[checker.taps(decision_normals(1), 1)[:, 0] == 0], np.broadcast_to(debug_texture(0)[0, 0], (int((checker.taps(decision_normals(1), 1)[:, 0] == 0).sum()), 3)))


def test_a_pattern_shows_where_the_rule_says(checker, tmp_path):
    """a sphere seen from the camera at -z: a texture red on the +x half and blue on the -x half colours the right and left halves of
    the disc (x grows to the right of this camera)"""
    scn = tmp_path / "lone.scn"
    scn.write_text("camera 0 0 -6 0 0 1 0 1 0 20\nbackground 0 0 0\nambient_light 1 1 1\nmaterial 1 1 1 1 1 1 0 0 0 1 0 0 0 1\nsphere 0 0 0 1.5\n")
    E = 16
    tex = np.zeros((E, E, 3), f32)
    tex[:, E // 2:] = (1, 0, 0)  # u > 0.5: qx > 0
    tex[:, :E // 2] = (0, 0, 1)
    _, f, st = checker.render(str(scn), 32, 32, fov=40.0, textures=[tex], sphere_textures=[0])
    sc = skr.parse_scene(str(scn))
    right = np.array(list(sc.info.camera)[9:12])  # the camera's right vector
    side = 1 if right[0] > 0 else -1
    halves = (f[12:20, 18:22], f[12:20, 10:14])[::side]
    assert (halves[0][..., 0] == 1).all() and (halves[0][..., 2] == 0).all() and (halves[1][..., 2] == 1).all() and (halves[1][..., 0] == 0).all()


# ---- 2. the ABI ----
def test_the_abi_clause_by_clause():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    ns = sc.info.n_spheres
    L = skr.lib()
    assert sc.textures == [] and L.skr_scene_texture_count(sc.h) == 0 and sc.sphere_textures.tolist() == [-1] * ns
    rng = np.random.default_rng(1)
    t0, t1 = rng.uniform(0, 2, (3, 3, 3)).astype(f32), rng.uniform(0, 2, (1, 1, 3)).astype(f32)
    assert sc.add_texture(t0) == 0 and sc.add_texture(t1) == 1
    got = sc.textures
    assert len(got) == 2 and np.array_equal(bits(got[0]), bits(t0)) and np.array_equal(bits(got[1]), bits(t1))
    for edge in (0, -1, TEX_MAX_EDGE + 1):  # a bad edge
        assert L.skr_scene_add_texture(sc.h, t0.ctypes.data, edge) == -2 and L.skr_scene_texture_count(sc.h) == 2
    assert L.skr_scene_add_texture(sc.h, None, 3) == -2
    for v in (np.nan, np.inf, -np.inf):  # a texel that is not finite
        bad = t0.copy()
        bad[2, 1, 0] = v
        with pytest.raises(skr.SkrError) as e:
            sc.add_texture(bad)
        assert "(status 2)" in str(e.value) and len(sc.textures) == 2
    with pytest.raises(ValueError):
        sc.add_texture(np.zeros((2, 3, 3), f32))
    e = C.c_int32(-1)
    assert L.skr_scene_get_texture(sc.h, 0, None, C.byref(e)) == 0 and e.value == 3  # null texels: the edge only
    for k in (-1, 2):
        assert L.skr_scene_get_texture(sc.h, k, None, C.byref(e)) == 2
    idx = np.full(ns, -1, np.int32)
    idx[1], idx[4] = 1, 0
    sc.set_sphere_textures(idx)
    assert sc.sphere_textures.tolist() == idx.tolist()
    n = C.c_int32(-1)
    assert L.skr_scene_get_sphere_textures(sc.h, None, C.byref(n)) == 0 and n.value == ns  # null idx: the count only
    for bad in (idx[:-1], np.append(idx, 0)):  # n != the sphere count
        with pytest.raises(skr.SkrError) as e2:
            sc.set_sphere_textures(bad)
        assert "(status 2)" in str(e2.value) and sc.sphere_textures.tolist() == idx.tolist()
    for v in (2, -2):  # an index outside [-1, n_tex)
        bad = idx.copy()
        bad[0] = v
        with pytest.raises(skr.SkrError):
            sc.set_sphere_textures(bad)
        assert sc.sphere_textures.tolist() == idx.tolist()  # the scene is unchanged
    sc.clear_textures()
    assert sc.sphere_textures.tolist() == [-1] * ns and len(sc.textures) == 2  # every index back to -1, the textures stay
    big = np.zeros((TEX_MAX_EDGE, TEX_MAX_EDGE, 3), f32)  # the largest edge is taken
    assert sc.add_texture(big) == 2
    for k in range(3, TEX_MAX):
        assert sc.add_texture(t1) == k
    with pytest.raises(skr.SkrError):  # a 17th
        sc.add_texture(t1)
    assert L.skr_scene_texture_count(sc.h) == TEX_MAX
    cam = list(sc.info.camera)[:9]
    sa = skr.Scene.from_arrays(np.zeros((2, 14), f32), np.zeros((0, 9), f32), np.zeros((0, 6), f32), cam, textures=[t0, t1], sphere_textures=[1, -1])
    assert len(sa.textures) == 2 and np.array_equal(sa.textures[1], t1) and sa.sphere_textures.tolist() == [1, -1]


def test_the_header_announces_the_addition():
    text = open(os.path.join(ROOT, "include", "skr.h")).read()
    assert "#define SKR_HAS_TEXTURES 1" in text and "#define SKR_TEX_MAX 16" in text and "#define SKR_TEX_MAX_EDGE 1024" in text and "#define SKR_SCN_TEXTURE 64u" in text
    for name in ("skr_scene_add_texture", "skr_scene_get_texture", "skr_scene_texture_count", "skr_scene_set_sphere_textures", "skr_scene_get_sphere_textures",
                 "skr_scene_clear_textures"):
        assert name in text and name in skr.EXPORTED_SYMBOLS
    assert (skr.binding.TEX_MAX, skr.binding.TEX_MAX_EDGE, skr.binding.SCN_TEXTURE) == (TEX_MAX, TEX_MAX_EDGE, 64)


# ---- 3. the parser ----
def write_textures(d, names, edge=2):
    for k, n in enumerate(names):
        p = os.path.join(str(d), n)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        skr.write_pfm(p, np.full((edge, edge, 3), k + 1, f32))


def test_the_texture_line_is_stateful_and_none_clears_it(tmp_path):
    write_textures(tmp_path, ["a.pfm", "sub/b.pfm"])
    absolute = str(tmp_path / "sub" / "b.pfm")
    scn = tmp_path / "s.scn"
    scn.write_text("sphere 0 0 0 1\ntexture a.pfm\nsphere 1 0 0 1\nsphere 2 0 0 1\ntexture sub/b.pfm\nsphere 3 0 0 1\ntexture none\nsphere 4 0 0 1\n"
                   "texture a.pfm\nsphere 5 0 0 1\ntexture %s\nsphere 6 0 0 1\n" % absolute)
    cwd = os.getcwd()
    os.chdir(ROOT)  # a relative name resolves against the scene's directory, not the working directory
    try:
        sc = skr.parse_scene(str(scn), texture=True)
    finally:
        os.chdir(cwd)
    assert sc.sphere_textures.tolist() == [-1, 0, 0, 1, -1, 0, 1]  # stateful; none clears; the same name twice, relative or absolute, is one texture
    assert len(sc.textures) == 2 and (sc.textures[0] == 1).all() and (sc.textures[1] == 2).all() and sc.info.n_unknown == 0


def test_lines_that_are_skipped_are_counted_and_leave_the_texture_in_force(tmp_path, capfd):
    write_textures(tmp_path, ["a.pfm"])
    skr.write_pfm(str(tmp_path / "wide.pfm"), np.zeros((2, 3, 3), f32))
    skr.write_pfm(str(tmp_path / "long.pfm"), np.zeros((TEX_MAX_EDGE + 1, TEX_MAX_EDGE + 1, 3), f32))  # square, an edge above the limit
    nf = np.ones((2, 2, 3), f32)
    nf[1, 1, 2] = np.inf
    skr.write_pfm(str(tmp_path / "inf.pfm"), nf)
    (tmp_path / "text.pfm").write_text("PF\nnot a map\n")
    scn = tmp_path / "s.scn"
    scn.write_text("texture a.pfm\nsphere 0 0 0 1\ntexture\nsphere 1 0 0 1\ntexture missing.pfm\nsphere 2 0 0 1\ntexture wide.pfm\nsphere 3 0 0 1\n"
                   "texture long.pfm\ntexture text.pfm\ntexture inf.pfm\nsphere 4 0 0 1\ntexture none\nsphere 5 0 0 1\ntexture missing.pfm\nsphere 6 0 0 1\n")
    sc = skr.parse_scene(str(scn), texture=True)
    assert sc.info.n_unknown == 7 and len(sc.textures) == 1
    assert sc.sphere_textures.tolist() == [0, 0, 0, 0, 0, -1, -1]
    assert capfd.readouterr().err.count("WARNING. texture") == 7


def test_a_seventeenth_texture_is_skipped_and_counted(tmp_path):
    names = ["t%02d.pfm" % k for k in range(TEX_MAX + 1)]
    write_textures(tmp_path, names, edge=1)
    scn = tmp_path / "s.scn"
    scn.write_text("".join("texture %s\nsphere %d 0 0 1\n" % (n, k) for k, n in enumerate(names)) + "texture t03.pfm\nsphere 99 0 0 1\n")
    sc = skr.parse_scene(str(scn), texture=True)
    assert len(sc.textures) == TEX_MAX and sc.info.n_unknown == 1
    assert sc.sphere_textures.tolist() == list(range(TEX_MAX)) + [TEX_MAX - 1, 3]  # the 17th is skipped, the 16th stays in force; a known name is still taken


def test_without_the_flag_the_line_is_an_unknown_command(tmp_path):
    write_textures(tmp_path, ["a.pfm"])
    body = "camera 0 0 -6 0 0 1 0 1 0 20\n%s a.pfm\nsphere 0 0 0 1\n%s none\nsphere 1 0 0 1\n%s\n"
    (tmp_path / "tex.scn").write_text(body % ("texture", "texture", "texture"))
    (tmp_path / "bogus.scn").write_text(body % ("texturf", "texturf", "texturf"))
    sc = skr.parse_scene(str(tmp_path / "tex.scn"))
    assert sc.info.n_unknown == 3 and sc.textures == [] and sc.sphere_textures.tolist() == [-1, -1]
    other = skr.parse_scene(str(tmp_path / "bogus.scn"))
    assert bytes(sc.info) == bytes(other.info)  # skr_scene_info is what it is for any unknown command
    code = "import sys, skele_raytracer_amd as skr; skr.parse_scene(sys.argv[1], echo=True)"
    outs = [subprocess.run([sys.executable, "-c", code, str(tmp_path / n)], cwd=ROOT, capture_output=True, timeout=120, check=True) for n in ("tex.scn", "bogus.scn")]
    assert outs[0].stdout.count(b"WARNING. Do not know command: texture\n") == 3
    assert outs[0].stdout == outs[1].stdout.replace(b"texturf", b"texture") and outs[0].stderr == outs[1].stderr  # byte for byte an unknown command's output


def test_both_command_lines_parse_the_flag():
    base = ["--path", scene_path("spheres2.scn"), "--output", "out.ppm"]
    assert "scn_texture" not in render_cli._parse(base) and render_cli._parse(base + ["--scn-texture"])["scn_texture"] is True
    assert "--scn-texture" in open(os.path.join(ROOT, "skele_raytracer_amd", "csrc", "raytracer_main.cpp")).read()


# ---- 4. the refused combinations that the host alone decides (launch_params on the packed scene, nothing uploaded) ----
def plan(scene, **kw):
    fn = skr.lib().skr_scene_leaf_shape
    fn.argtypes = [C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    rc = fn(scene.h, C.byref(skr.Options(32, 24, **kw).c))
    return rc, (skr.lib().skr_last_error() or b"").decode()


def test_the_refused_combinations():
    fog_rows = np.array([[0, 0, 5, 3, .5, .5, .5, .1, .05]], f32)

    def cases():
        def textured(**flags):
            sc = skr.parse_scene(scene_path("spheres2.scn"), **flags)
            k = sc.add_texture(np.full((2, 2, 3), 0.5, f32))
            idx = sc.sphere_textures
            idx[3] = k
            sc.set_sphere_textures(idx)
            return sc
        fog = textured(fog=True)
        fog.set_fog(fog_rows)
        return [(textured(), dict(legacy_reflect=True), "--legacy-reflect"), (fog, dict(), "fog volumes"), (textured(sphere_tree=True), dict(), "sphere tree")]

    for sc, kw, text in cases():
        rc, why = plan(sc, **kw)
        assert rc == -4 and "sphere textures (--scn-texture)" in why and text in why, (rc, why)
        sc.clear_textures()  # none of them is refused once no sphere has a texture: the textures a scene merely holds are not in force
        assert plan(sc, **kw)[0] >= 0
    ok = cases()[0][0]
    for kw in (dict(shadow=True), dict(gillum=2, depth=3), dict(jsample=2), dict(shade_triangles=True, shadow=True)):
        assert plan(ok, **kw)[0] >= 0
