"""Emissive spheres on the MI355X (include/skr.h skr_scene_set_sphere_emission): whole frames against the CPU checker
(tests/emit_checker.c) — bytes, float bits and the four work counters, no tolerance — in every mode that combines with emission
(tests/emit_cases.py, whose reach conditions tests/test_emit_cpu.py asserts), every work counter against the same frame without
emission, two tiles against one frame, a clone, skr_multi, shading queries, progressive and adaptive frames, the denoised-host call, an
all-zero emission on all three paths, the variant names, the refusals, both command lines.  Frames are 32 x 24 to 64 x 48."""
import os
import subprocess

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding, render_cli
from conftest import ROOT, read_ppm_bytes, scene_path
from emit_cases import CASES, GROUND_MID, checker_frame, load, scene_flags, scene_texts
from emit_check import build as build_checker, emission_scene_text

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("emitcheck_gpu")))


@pytest.fixture(scope="session")
def scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("emit_gpu_scenes")
    out = {}
    for k, t in scene_texts().items():
        p = d / (k + ".scn")
        p.write_text(t)
        out[k] = str(p)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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


# ---- 1. GPU == checker, bit for bit, in every mode that combines with emission ----
@pytest.mark.parametrize("name,scn,size,setup,kw", CASES, ids=[c[0] for c in CASES])
def test_frames_match_the_checker_bit_for_bit(gpu, checker, scenes, name, scn, size, setup, kw):
    w, h = size
    given, told = scene_flags(setup)
    sc = load(scenes, scn, **given)
    g_rgb, g_f, g_cnt, variant = gpu_frame(gpu, sc, w, h, **kw)
    c_rgb, c_f, c_st = checker_frame(checker, scenes, sc, scn, w, h, **told, **kw)
    assert int(c_st[8]) >= 30, (name, c_st.tolist())  # the case is about something: shaded hits on emitters
    nb = int((bits(g_f) != bits(c_f)).sum())
    assert nb == 0, "%s: %d float words differ" % (name, nb)
    assert np.array_equal(g_rgb, c_rgb), name
    assert g_cnt == [int(x) for x in c_st[:4]], name
    tsh = told["triangle_shadows"] and kw.get("shade_triangles") and kw.get("shadow") and sc.info.n_triangles > 0
    want = ("level_pipeline_g1" + setup.get("part", "") + ("_motion" if setup.get("motion") else "_lens" if setup.get("lens") else "") + ("_tshadow" if tsh else "")
            + ("_env" if setup.get("env") else "") + ("_tex" if setup.get("textures") else "") + "_emit")
    assert variant == want, (name, variant)
    sc.set_emission(None)  # the same scene without emission: every work counter is what it was, the picture is not
    p_rgb, p_f, p_cnt, p_variant = gpu_frame(gpu, sc, w, h, **kw)
    assert p_cnt == g_cnt and "_emit" not in p_variant and (bits(p_f) != bits(g_f)).any(), name


# ---- 2. the other entry points ----
def test_two_tiles_a_clone_skr_multi_and_a_shading_query_are_the_frame(gpu, checker, scenes):
    torch = gpu
    w, h = 40, 32
    kw = dict(gillum=2, depth=2, shadow=True, seed=9)
    sc = load(scenes, "three", emission=GROUND_MID)
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
        clone = r.clone()  # a clone shares the emission rows
        try:
            assert np.array_equal(bits(clone.render(opt, want_float=True)[1].cpu().numpy()), bits(one[1]))
            torch.cuda.synchronize()
            assert skr.Renderer.kernel_variant() == "level_pipeline_g1_emit"
        finally:
            clone.close()
        rays = r.camera_rays(opt).view(-1, 8)  # Renderer.shade of 257 of the frame's camera rays against the frame: more than one workgroup, the last one partial
        pick = torch.arange(257, device=rays.device) * ((w * h) // 257)
        got = r.shade(rays[pick].contiguous(), opt, keys=pick.to(torch.int32))
        torch.cuda.synchronize()
        assert skr.Renderer.kernel_variant() == "shade_rays_g1_emit"
        assert np.array_equal(bits(got.cpu().numpy()), bits(one[1]).reshape(-1, 3)[pick.cpu().numpy()])
    finally:
        r.close()
    m = binding.Multi(sc, 1)  # the frame step's renderer takes the emission with the scene
    try:
        rgb, _ = m.render_frame_host(skr.Options(w, h, **kw), tile_rows=8)
    finally:
        m.close()
    assert np.array_equal(rgb, one[0])


def test_progressive_and_adaptive_frames(gpu, checker, scenes):
    w, h = 32, 24
    K = 2
    kw = dict(gillum=2, depth=2, shadow=True, seed=9)
    sc = load(scenes, "three", emission=GROUND_MID)
    want = checker.render_progressive(scenes["three"], w, h, K, emission=sc.emission, **kw)
    r = skr.Renderer(sc)
    try:
        rgb, rgbf, passes, _ = r.render_adaptive_host(skr.Options(w, h, **kw), threshold=-1.0, min_passes=1, max_passes=K, want_float=True)
        assert (passes == K).all() and np.array_equal(bits(rgbf), bits(want[1])) and np.array_equal(rgb, want[0])
        rgb, rgbf = r.render(skr.Options(w, h, progressive=K, **kw), want_float=True)
        gpu.cuda.synchronize()
        assert np.array_equal(bits(rgbf.cpu().numpy()), bits(want[1])) and np.array_equal(rgb.cpu().numpy(), want[0])
    finally:
        r.close()


def test_the_denoised_host_call_is_the_denoiser_on_the_frame_and_its_guides(gpu, checker, scenes):
    w, h = 32, 24
    kw = dict(gillum=2, depth=2, shadow=True, seed=4)
    sc = load(scenes, "three", emission=GROUND_MID)
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, **kw)
        rgb, rgbf, _ = r.render_denoised(opt, want_float=True)  # not refused: emission is constant per sphere
        frame = r.render(opt, want_float=True)[1]
        gpu.cuda.synchronize()
        assert skr.Renderer.kernel_variant() == "level_pipeline_g1_emit"
        assert np.array_equal(bits(frame.cpu().numpy()), bits(checker_frame(checker, scenes, sc, "three", w, h, **kw)[1]))
        hits = r.trace(r.camera_rays(opt).view(-1, 8))
        d_rgb, d_f = r.denoise(frame, hits)
        gpu.cuda.synchronize()
        assert np.array_equal(bits(rgbf), bits(d_f.cpu().numpy())) and np.array_equal(rgb, d_rgb.cpu().numpy())
        a = r.render_adaptive_denoised(opt, min_passes=2, max_passes=2, want_float=True)  # nor is the adaptive one
        assert np.isfinite(a[1]).all()
    finally:
        r.close()


def test_an_all_zero_emission_changes_nothing_on_any_path(gpu):
    """the direct kernel, the node pipeline and the general level pipeline: the variant's name and the bytes of the scene without emission"""
    for kw, path in ((dict(shadow=True, depth=1), "direct"), (dict(gillum=4, shadow=True, seed=7), "node"), (dict(shade_triangles=True, shadow=True), "level_pipeline_g1")):
        plain = skr.parse_scene(scene_path("spheres2.scn"))
        want = gpu_frame(gpu, plain, 48, 36, **kw)
        for e in (0.0, -0.0):
            sc = skr.parse_scene(scene_path("spheres2.scn"))
            sc.set_emission(np.full((sc.info.n_spheres, 3), e, f32))
            got = gpu_frame(gpu, sc, 48, 36, **kw)
            assert got[3] == want[3] and "emit" not in got[3], (path, got[3])
            assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and got[2] == want[2], path
        sc.set_emission(np.full((sc.info.n_spheres, 3), 0.5, f32))  # and with it in force every one of them takes the general pipeline
        assert gpu_frame(gpu, sc, 48, 36, **kw)[3] == "level_pipeline_g1_emit"
    assert len({gpu_frame(gpu, skr.parse_scene(scene_path("spheres2.scn")), 48, 36, **kw)[3] for kw in (dict(shadow=True, depth=1), dict(gillum=4, shadow=True, seed=7))}) == 2


def test_the_emit_names(gpu, scenes):
    sc = load(scenes, "three_spot", emission=GROUND_MID, spot=True, radii=[0.4, 0.0, 0.25], lens=(0.3, 9.0), env=(4, 1), textures=(2,))
    assert gpu_frame(gpu, sc, 32, 24, shadow=True)[3] == "level_pipeline_g1_soft_lens_env_tex_emit"
    sc = load(scenes, "three_spot", emission=GROUND_MID, spot=True)
    assert gpu_frame(gpu, sc, 32, 24, shadow=True)[3] == "level_pipeline_g1_spot_emit"
    sc = load(scenes, "three", emission=GROUND_MID, env=(4, 1))
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(32, 24, shadow=True)
        r.shade(r.camera_rays(opt).view(-1, 8), opt)
        gpu.cuda.synchronize()
        assert skr.Renderer.kernel_variant() == "shade_rays_g1_env_emit"
    finally:
        r.close()


# ---- 3. the refused combinations ----
def test_the_refused_combinations(gpu, scenes):
    fog_rows = np.array([[0, 0, 5, 3, .5, .5, .5, .1, .05]], f32)
    cases = [(load(scenes, "three", emission=GROUND_MID), dict(legacy_reflect=True), "--legacy-reflect")]
    fog = load(scenes, "three", emission=GROUND_MID, fog=True)
    fog.set_fog(fog_rows)
    cases += [(fog, dict(), "fog volumes (--scn-fog)"), (load(scenes, "three", emission=GROUND_MID, sphere_tree=True), dict(), "the sphere tree (--sphere-tree)")]
    for sc, kw, text in cases:
        r = skr.Renderer(sc)
        try:
            with pytest.raises(skr.SkrError) as e:
                r.render(skr.Options(32, 24, **kw))
            assert "(status 4)" in str(e.value) and "sphere emission (--scn-emission) cannot be combined with " + text in str(e.value), str(e.value)
        finally:
            r.close()
        sc.set_emission(None)  # none of them is refused once no sphere glows
        r = skr.Renderer(sc)
        try:
            r.render(skr.Options(32, 24, **kw))
            gpu.cuda.synchronize()
            assert "emit" not in skr.Renderer.kernel_variant()
        finally:
            r.close()


# ---- 4. both command lines ----
def test_both_command_lines_take_the_flag(gpu, tmp_path):
    w, h = 40, 30
    scn = tmp_path / "emit.scn"
    scn.write_text(emission_scene_text(GROUND_MID))
    sc = skr.parse_scene(str(scn), emission=True)
    assert np.array_equal(bits(sc.emission), bits(np.array(GROUND_MID, f32)))
    kw = dict(gillum=2, depth=2, shadow=True, seed=3)
    want = gpu_frame(gpu, sc, w, h, **kw)
    assert want[3] == "level_pipeline_g1_emit"
    off = gpu_frame(gpu, skr.parse_scene(str(scn)), w, h, **kw)
    assert "emit" not in off[3] and (want[0] != off[0]).any()
    args = ["--path", str(scn), "--width", str(w), "--height", str(h), "--shadow", "--gillum", "2", "--depth", "2", "--seed", "3"]
    exe = os.path.join(ROOT, "bin", "raytracer")
    out1, out2, out3 = str(tmp_path / "native.ppm"), str(tmp_path / "py.ppm"), str(tmp_path / "noflag.ppm")
    subprocess.run([exe, *args, "--scn-emission", "--output", out1, "--quiet"], check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=300)
    assert render_cli.main([*args, "--scn-emission", "--output", out2]) == 0
    for o in (out1, out2):
        assert np.array_equal(read_ppm_bytes(open(o, "rb").read()), want[0]), o
    subprocess.run([exe, *args, "--output", out3, "--quiet"], check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=300)
    assert np.array_equal(read_ppm_bytes(open(out3, "rb").read()), off[0])
