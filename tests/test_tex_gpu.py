"""Sphere textures on the MI355X (include/skr.h skr_scene_add_texture): whole frames against the CPU checker
(tests/tex_checker.c) — bytes, float bits and the four work counters, no tolerance — in every mode that combines with textures, every
work counter against the same frame without textures, two tiles against one frame, a clone, shading queries, the debug op at the rule's
decision points, a frame through which the fold runs, the refused denoiser calls, both command lines.  Frames are 32 x 24 to 64 x 48,
the textures have the edges 1, 2, 3 and 64, random texels: a wrong tap or weight shows."""
import os
import subprocess

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding, render_cli
from conftest import ROOT, read_ppm_bytes, scene_path
from tex_check import DEBUG_EDGES, build as build_checker, debug_texture, decision_normals, records, scene_text

pytestmark = pytest.mark.gpu
f32 = np.float32
TEX_OP = 26  # include/skr.h skr_debug_eval
ST = dict(shade_triangles=True, shadow=True)
SPOT = "spot_light 30 30 30 0 9 -2 0 -1 0.2 15 35\n"


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("texcheck_gpu")))


@pytest.fixture(scope="session")
def scenes(tmp_path_factory):
    """the scene files the golden set lacks"""
    d = tmp_path_factory.mktemp("tex_gpu_scenes")
    text = {
        "three": scene_text(),                 # three small spheres over a large one, two point lights
        "three_spot": scene_text() + SPOT,     # ... and a spot light
        # the camera looks down -y at one sphere: the fold N.y = 0 is the sphere's outline, and the -y sheet shows in the floor's GI
        "down": "camera 0 7 0 0 -1 0 0 0 1 25\nbackground .2 .2 .2\nambient_light .3 .3 .3\npoint_light 30 30 30 3 9 2\nmaterial .5 .5 .5 .8 .8 .8 .3 .3 .3 8 0 0 0 1\n"
                "sphere 0 1.5 0 1.5\nmaterial .5 .5 .5 .5 .5 .5 0 0 0 1 0 0 0 1\nsphere 0 -1000 0 1000\n",
    }
    out = {}
    for k, t in text.items():
        p = d / (k + ".scn")
        p.write_text(t)
        out[k] = str(p)
    return out


def tex_map(E, seed):
    return np.random.default_rng(seed).uniform(0.25, 2.0, (E, E, 3)).astype(f32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def path_of(scenes, scn):
    return scenes[scn] if scn in scenes else scene_path(scn)


def load(scenes, scn, edges, *, skip=None, motion=False, radii=None, lens=None, env=None, **flags):
    """the scene with one random texture per edge, sphere i carrying texture i % len(edges) (sphere `skip`: none)"""
    sc = skr.parse_scene(path_of(scenes, scn), **flags)
    ns = sc.info.n_spheres
    for k, E in enumerate(edges):
        assert sc.add_texture(tex_map(E, 10 * E + k)) == k
    idx = np.arange(ns, dtype=np.int32) % len(edges)
    if skip is not None:
        idx[skip] = -1
    sc.set_sphere_textures(idx)
    if radii is not None:
        sc.set_light_radii(radii)
    if lens is not None:
        sc.set_lens(*lens)
    if motion:
        v = np.zeros((ns, 3), f32)
        v[0], v[min(1, ns - 1)] = (1.5, 0.25, 0), (0, 0.5, -1)
        sc.set_velocities(v)
    if env is not None:
        sc.set_environment(env)
    return sc


def gpu_frame(gpu, scene, w, h, **kw):
    """(bytes, floats, the four work counters, kernel variant) of a frame of the scene under its own renderer"""
    r = skr.Renderer(scene)
    try:
        rgb, rgbf = r.render(skr.Options(w, h, **kw), want_float=True)
        gpu.cuda.synchronize()
        c = r.work()
        return rgb.cpu().numpy(), rgbf.cpu().numpy(), [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"], c["sphere_tests"]], skr.Renderer.kernel_variant()
    finally:
        r.close()


def checker_frame(checker, scenes, sc, scn, w, h, *, strict=False, triangle_shadows=False, **kw):
    """the checker's frame of the scene file under the library scene's textures, environment, lens, velocities, spot lights and radii"""
    A, F = sc.lens
    return checker.render(path_of(scenes, scn), w, h, textures=sc.textures, sphere_textures=sc.sphere_textures, environment=sc.environment, aperture=A, focus=F,
                          velocities=sc.velocities, shutter=sc.shutter, spots=sc.spot_lights, cones=sc.spot_cones, radii=sc.light_radii, triangle_shadows=triangle_shadows,
                          strict=strict, **kw)


def same_as_checker(gpu, checker, scenes, scn, w, h, what, *, edges=(3,), skip=None, part="", motion=False, radii=None, lens=None, env=None, spot=False, strict=False,
                    triangle_shadows=False, **kw):
    sc = load(scenes, scn, edges, skip=skip, motion=motion, radii=radii, lens=lens, env=env, spot=spot, strict=strict, triangle_shadows=triangle_shadows)
    g_rgb, g_f, g_cnt, variant = gpu_frame(gpu, sc, w, h, **kw)
    c_rgb, c_f, c_st = checker_frame(checker, scenes, sc, scn, w, h, strict=strict, triangle_shadows=triangle_shadows, **kw)
    # the case is about something: at least 30 shaded hits look a texture up, and a tenth of all where no mesh takes most of them (triangles have no texture)
    assert int(c_st[7]) >= 30 and (sc.info.n_triangles > 0 or int(c_st[7]) * 10 >= int(c_st[1])), (what, c_st.tolist())
    nb = int((bits(g_f) != bits(c_f)).sum())
    assert nb == 0, "%s: %d float words differ" % (what, nb)
    assert np.array_equal(g_rgb, c_rgb), what
    assert g_cnt == [int(x) for x in c_st[:4]], what
    tsh = triangle_shadows and kw.get("shade_triangles") and kw.get("shadow") and sc.info.n_triangles > 0
    assert variant == "level_pipeline_g1" + part + ("_motion" if motion else "_lens" if lens else "") + ("_tshadow" if tsh else "") + ("_env" if env is not None else "") + "_tex", (what, variant)
    sc.clear_textures()  # the same scene without textures: every work counter is what it was, the picture is not
    p_rgb, p_f, p_cnt, p_variant = gpu_frame(gpu, sc, w, h, **kw)
    assert p_cnt == g_cnt and "_tex" not in p_variant and (bits(p_f) != bits(g_f)).any(), what
    return g_f


# ---- 1. GPU == checker, bit for bit, in every mode that combines with textures ----
MODES = [
    ("shadow", "three", (32, 24), dict(edges=(3, 1)), dict(shadow=True)),
    ("no_shadow_mixed", "three", (32, 24), dict(edges=(2,), skip=1), dict()),
    ("gi2_d2", "three", (40, 30), dict(edges=(2, 64), skip=3), dict(gillum=2, depth=2, shadow=True, seed=4)),  # the last-level arm at textured children
    ("gi2_d3", "three", (40, 30), dict(edges=(64, 3, 1, 2)), dict(gillum=2, depth=3, shadow=True, seed=5)),    # finalize's node_value
    ("js2", "three", (33, 25), dict(edges=(1, 3)), dict(jsample=2, shadow=True, seed=3)),
    ("strict", "three", (32, 24), dict(edges=(3,), strict=True), dict(shadow=True)),
    ("spot_radius", "three_spot", (40, 30), dict(edges=(2, 3), spot=True, radii=[0.4, 0.0, 0.25], part="_soft"), dict(gillum=2, depth=2, shadow=True, seed=2)),
    ("motion", "three", (40, 30), dict(edges=(64, 2), motion=True), dict(gillum=2, depth=2, shadow=True, seed=5)),  # N from the displaced centre
    ("lens", "three", (40, 30), dict(edges=(3, 64), lens=(0.3, 9.0)), dict(jsample=2, shadow=True, seed=3)),
    ("env", "three", (40, 30), dict(edges=(2, 3), env=tex_map(8, 99)), dict(gillum=2, depth=3, shadow=True, seed=6)),
    ("env_lens", "three", (32, 24), dict(edges=(1, 64), env=tex_map(4, 98), lens=(0.2, 8.0)), dict(gillum=2, depth=2, seed=8)),
    ("mesh_tshadow", "test.scn", (48, 36), dict(edges=(64, 2, 3), triangle_shadows=True), dict(**ST)),  # a mesh and textured spheres
    ("mesh_tshadow_gi", "test.scn", (32, 24), dict(edges=(3,), triangle_shadows=True), dict(gillum=2, depth=2, seed=5, **ST)),
    ("mesh_black", "test.scn", (32, 24), dict(edges=(2,)), dict(shadow=True)),
    ("fold", "down", (64, 48), dict(edges=(3, 2)), dict(gillum=2, depth=2, shadow=True, seed=7)),
]


@pytest.mark.parametrize("name,scn,size,flags,kw", MODES, ids=[m[0] for m in MODES])
def test_frames_match_the_checker_bit_for_bit(gpu, checker, scenes, name, scn, size, flags, kw):
    same_as_checker(gpu, checker, scenes, scn, *size, name, **flags, **kw)


def test_the_fold_runs_through_the_picture(gpu, checker, scenes):
    """the camera looks down -y: the sphere's outline is N.y = 0, and both sheets of the map are read (the lower one by GI children of the floor)"""
    w, h = 64, 48
    sc = load(scenes, "down", (3, 2))
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, shadow=True)
        hits = r.trace(r.camera_rays(opt).view(-1, 8))
        gpu.cuda.synchronize()
    finally:
        r.close()
    t = hits.t.cpu().numpy().reshape(h, w)
    assert np.isfinite(t[h // 2, w // 2]) and t[h // 2, w // 2] < 5  # the sphere's top is in the middle of the picture
    f = same_as_checker(gpu, checker, scenes, "down", w, h, "fold", edges=(3, 2), shadow=True)
    plain = skr.parse_scene(scenes["down"])
    p = gpu_frame(gpu, plain, w, h, shadow=True)[1]
    changed = (bits(f) != bits(p)).any(2)
    assert changed[h // 2, w // 2] and changed.sum() > w * h // 4  # the disc in the middle and the floor around it


# ---- 2. the other entry points ----
def test_two_tiles_a_clone_and_a_shading_query_are_the_frame(gpu, checker, scenes):
    torch = gpu
    w, h = 40, 32
    kw = dict(gillum=2, depth=2, shadow=True, seed=9)
    sc = load(scenes, "three", (3, 64))
    one = checker_frame(checker, scenes, sc, "three", w, h, **kw)
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, **kw)
        rows = h // 2  # two tiles against one frame
        for first in (0, 1):
            rgb, rgbf = r.render(opt, want_float=True, tile_rows=rows, first_tile=first, tile_stride=2)
            torch.cuda.synchronize()
            assert np.array_equal(bits(rgbf[:rows].cpu().numpy()), bits(one[1][first * rows:(first + 1) * rows])), first
            assert np.array_equal(rgb[:rows].cpu().numpy(), one[0][first * rows:(first + 1) * rows])
        clone = r.clone()  # a clone shares the textures
        try:
            assert np.array_equal(bits(clone.render(opt, want_float=True)[1].cpu().numpy()), bits(one[1]))
            torch.cuda.synchronize()
            assert skr.Renderer.kernel_variant() == "level_pipeline_g1_tex"
        finally:
            clone.close()
        rays = r.camera_rays(opt)  # Renderer.shade of the frame's camera rays against the frame
        keys = torch.arange(w * h, dtype=torch.int32, device=rays.device)
        got = r.shade(rays.view(-1, 8), opt, keys=keys)
        torch.cuda.synchronize()
        assert skr.Renderer.kernel_variant() == "shade_rays_g1_tex"
        assert np.array_equal(bits(got.cpu().numpy()), bits(one[1]).reshape(-1, 3))
    finally:
        r.close()
    m = binding.Multi(sc, 1)  # the frame step's renderer takes the textures with the scene
    try:
        rgb, _ = m.render_frame_host(skr.Options(w, h, **kw), tile_rows=8)
    finally:
        m.close()
    assert np.array_equal(rgb, one[0])


def test_progressive_and_adaptive_frames(gpu, checker, scenes):
    w, h = 32, 24
    K = 2
    kw = dict(gillum=2, depth=2, shadow=True, seed=9)
    sc = load(scenes, "three", (2, 3))
    A, F = sc.lens
    want = checker.render_progressive(scenes["three"], w, h, K, textures=sc.textures, sphere_textures=sc.sphere_textures, **kw)
    r = skr.Renderer(sc)
    try:
        rgb, rgbf, passes, _ = r.render_adaptive_host(skr.Options(w, h, **kw), threshold=-1.0, min_passes=1, max_passes=K, want_float=True)
        assert (passes == K).all() and np.array_equal(bits(rgbf), bits(want[1])) and np.array_equal(rgb, want[0])
        rgb, rgbf = r.render(skr.Options(w, h, progressive=K, **kw), want_float=True)
        gpu.cuda.synchronize()
        assert np.array_equal(bits(rgbf.cpu().numpy()), bits(want[1])) and np.array_equal(rgb.cpu().numpy(), want[0])
    finally:
        r.close()


# ---- 3. the debug op, at the rule's decision points ----
def test_the_colour_through_the_debug_op(gpu, checker):
    rng = np.random.default_rng(11)
    rand = (rng.normal(0, 1, (1024 + 37, 3)) * np.exp(rng.uniform(-20, 20, (1024 + 37, 1)))).astype(f32)
    rand[:300, 1] = -np.abs(rand[:300, 1]) * 1e3  # near the -y pole: the corners of the square
    for k, E in enumerate(DEBUG_EDGES):
        tex = debug_texture(k)
        for N in (decision_normals(E), rand):
            got = binding.debug_eval(TEX_OP, records(N, k), 3).view(np.float32)
            want = checker.colour(tex, N)
            assert np.array_equal(bits(got), bits(want)), (k, E)
            arm = checker.taps(N, E)[:, 0] == 1
            assert np.array_equal(got[arm], np.ones((int(arm.sum()), 3), f32))  # a zero vector, a NaN: the fallback
    N = decision_normals(3)
    for k in (4, 7, 0xFFFFFFFF):  # no texture: (1, 1, 1)
        assert np.array_equal(binding.debug_eval(TEX_OP, records(N, k), 3).view(np.float32), np.ones((len(N), 3), f32))


# ---- 4. the refused combinations ----
def test_the_refused_combinations(gpu, scenes):
    fog_rows = np.array([[0, 0, 5, 3, .5, .5, .5, .1, .05]], f32)
    cases = [(load(scenes, "three", (2,)), dict(legacy_reflect=True), "--legacy-reflect")]
    fog = load(scenes, "three", (2,), fog=True)
    fog.set_fog(fog_rows)
    cases += [(fog, dict(), "fog volumes"), (load(scenes, "three", (2,), sphere_tree=True), dict(), "sphere tree")]
    for sc, kw, text in cases:
        r = skr.Renderer(sc)
        try:
            with pytest.raises(skr.SkrError) as e:
                r.render(skr.Options(32, 24, **kw))
            assert "(status 4)" in str(e.value) and "sphere textures (--scn-texture)" in str(e.value) and text in str(e.value), str(e.value)
        finally:
            r.close()
        sc.clear_textures()  # none of them is refused once no sphere has a texture
        r = skr.Renderer(sc)
        try:
            r.render(skr.Options(32, 24, **kw))
            gpu.cuda.synchronize()
            assert "tex" not in skr.Renderer.kernel_variant()
        finally:
            r.close()
    opt = skr.Options(32, 24, shadow=True)
    sc = load(scenes, "three", (2,))
    r = skr.Renderer(sc)
    try:
        for call in (lambda: r.render_denoised(opt), lambda: r.render_adaptive_denoised(opt, min_passes=2, max_passes=2)):
            with pytest.raises(skr.SkrError) as e:
                call()
            assert "(status 4)" in str(e.value) and "sphere textures" in str(e.value) and "denoiser" in str(e.value), str(e.value)
        hits = r.trace(r.camera_rays(opt).view(-1, 8))  # skr_trace_rays is unaffected
        gpu.cuda.synchronize()
    finally:
        r.close()
    sc.clear_textures()
    r = skr.Renderer(sc)
    try:
        r.render_denoised(opt)
        hits2 = r.trace(r.camera_rays(opt).view(-1, 8))
        gpu.cuda.synchronize()
    finally:
        r.close()
    assert np.array_equal(bits(hits.raw.cpu().numpy()), bits(hits2.raw.cpu().numpy()))


# ---- 5. both command lines ----
def test_both_command_lines_take_the_flag(gpu, tmp_path):
    w, h = 40, 30
    rng = np.random.default_rng(3)
    tex = [rng.uniform(0.25, 2.0, (E, E, 3)).astype(f32) for E in (3, 64)]
    for k, t in enumerate(tex):
        skr.write_pfm(str(tmp_path / ("t%d.pfm" % k)), t)
    scn = tmp_path / "tex.scn"
    scn.write_text(scene_text(texture_lines=["texture t0.pfm\n", "texture t1.pfm\n", "texture none\n"]))
    sc = skr.parse_scene(str(scn), texture=True)
    assert sc.sphere_textures.tolist() == [0, 1, -1, -1] and np.array_equal(bits(sc.textures[1]), bits(tex[1]))
    kw = dict(gillum=2, depth=2, shadow=True, seed=3)
    want = gpu_frame(gpu, sc, w, h, **kw)
    assert want[3] == "level_pipeline_g1_tex"
    off = gpu_frame(gpu, skr.parse_scene(str(scn)), w, h, **kw)
    assert "tex" not in off[3] and (want[0] != off[0]).any()
    args = ["--path", str(scn), "--width", str(w), "--height", str(h), "--shadow", "--gillum", "2", "--depth", "2", "--seed", "3"]
    exe = os.path.join(ROOT, "bin", "raytracer")
    out1, out2, out3 = str(tmp_path / "native.ppm"), str(tmp_path / "py.ppm"), str(tmp_path / "noflag.ppm")
    subprocess.run([exe, *args, "--scn-texture", "--output", out1, "--quiet"], check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=300)
    assert render_cli.main([*args, "--scn-texture", "--output", out2]) == 0
    for o in (out1, out2):
        assert np.array_equal(read_ppm_bytes(open(o, "rb").read()), want[0]), o
    subprocess.run([exe, *args, "--output", out3, "--quiet"], check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=300)
    assert np.array_equal(read_ppm_bytes(open(out3, "rb").read()), off[0])
