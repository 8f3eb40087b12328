"""Triangle shadows on the MI355X (include/skr.h skr_scene_set_triangle_shadows): whole frames and shading queries
against the CPU checker (tests/triangle_shadow_checker.c) — bytes, float bits and the three work counters, no tolerance —, the
culling switches, what the switch leaves alone, inheritance by clones and the multi-GPU step, both command lines, the work counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding
from conftest import ROOT, read_ppm_bytes, scene_path
from test_shade_triangles import _write_mesh_scene
from triangle_shadow_check import build as build_checker

pytestmark = pytest.mark.gpu

ON = dict(shade_triangles=True, shadow=True)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("trishadowcheck_gpu")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_frame(gpu, path, w, h, *, triangle_shadows=True, strict=False, **kw):
    """(bytes, floats, the three counters, kernel variant) of a frame of the scene file under its own renderer"""
    r = skr.Renderer(skr.parse_scene(path, strict=strict, triangle_shadows=triangle_shadows))
    try:
        rgb, rgbf = r.render(skr.Options(w, h, **kw), want_float=True)
        gpu.cuda.synchronize()
        c = r.counters()
        return rgb.cpu().numpy(), rgbf.cpu().numpy(), [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]], skr.Renderer.kernel_variant()
    finally:
        r.close()


def same_as_checker(gpu, checker, path, w, h, what, *, strict=False, **kw):
    g_rgb, g_f, g_cnt, variant = gpu_frame(gpu, path, w, h, strict=strict, **kw)
    c_rgb, c_f, c_st = checker.render(path, w, h, triangle_shadows=True, strict=strict, **kw)
    nb = int((bits(g_f) != bits(c_f)).sum())
    assert nb == 0, "%s: %d float words differ" % (what, nb)
    assert np.array_equal(g_rgb, c_rgb), what
    assert g_cnt == [int(x) for x in c_st[:3]], what
    assert variant == "level_pipeline_g1_tshadow"
    return c_f


# name, scene, strict, w, h, options: 1 light (test.scn's point light), 2 (+ its directional light under the strict loader); --gillum with
# depth 2 .. 6, --jsample, --legacy-reflect; dragon.scn: a mesh that shadows itself and no sphere
FRAMES = [
    ("test_primary", "test.scn", False, 160, 120, dict()),
    ("test_gi4_d2", "test.scn", False, 80, 60, dict(gillum=4, depth=2, seed=3)),
    ("test_strict_gi3_d3", "test.scn", True, 64, 48, dict(gillum=3, depth=3, seed=5)),
    ("test_strict_js2", "test.scn", True, 96, 72, dict(jsample=2, seed=4)),
    ("test_strict_legacy_gi2_d3", "test.scn", True, 48, 36, dict(gillum=2, depth=3, legacy_reflect=True, seed=7)),
    ("test_gi2_d6", "test.scn", False, 32, 24, dict(gillum=2, depth=6, seed=9)),
    ("dragon_strict", "dragon.scn", True, 160, 120, dict()),
    ("dragon_strict_gi2_d4", "dragon.scn", True, 64, 48, dict(gillum=2, depth=4, seed=2)),
    ("dragon_strict_gi3_d2_js2", "dragon.scn", True, 48, 36, dict(gillum=3, depth=2, jsample=2, seed=6)),
]


@pytest.mark.parametrize("name,scn,strict,w,h,kw", FRAMES, ids=[c[0] for c in FRAMES])
def test_frames_match_the_checker_bit_for_bit(gpu, checker, name, scn, strict, w, h, kw):
    on = same_as_checker(gpu, checker, scene_path(scn), w, h, name, strict=strict, **ON, **kw)
    if name in ("test_primary", "dragon_strict"):  # the switch does something: the wall shadows the spheres, the dragon itself
        off = checker.render(scene_path(scn), w, h, triangle_shadows=False, strict=strict, **ON, **kw)[1]
        assert (bits(on) != bits(off)).any()


def _mesh_scene(path, n_tris, n_spheres, n_lights):
    """test_shade_triangles' random mesh (coincident triangle pairs included) under n_lights point lights"""
    _write_mesh_scene(path, np.random.default_rng(n_tris), n_tris, n_spheres)
    lines = [ln for ln in open(path).read().split("\n") if ln and not ln.startswith("point_light")]
    lights = ["point_light 30 30 30 6 8 -6", "point_light 10 25 40 -7 5 2", "point_light 20 12 12 1 9 4"]
    open(path, "w").write("\n".join(lines + lights[:n_lights]) + "\n")
    return path


@pytest.mark.parametrize("n_tris,n_spheres,n_lights,kw", [
    (60, 4, 3, dict(gillum=4, depth=3, seed=31)),                        # three lights: a full pair and the odd tail
    (300, 2, 1, dict(jsample=2, seed=32)),
    (120, 6, 2, dict(gillum=2, depth=5, legacy_reflect=True, seed=34)),
], ids=["mesh60_3lights_gi4_d3", "mesh300_1light_aa", "mesh120_2lights_legacy_d5"])
def test_random_meshes_with_spheres(gpu, checker, tmp_path, n_tris, n_spheres, n_lights, kw):
    scn = _mesh_scene(str(tmp_path / "mesh.scn"), n_tris, n_spheres, n_lights)
    same_as_checker(gpu, checker, scn, 96, 54, "mesh %d" % n_tris, **ON, **kw)


def test_culling_switches_change_nothing_at_1080p(gpu, monkeypatch):
    sc = skr.parse_scene(scene_path("dragon.scn"), strict=True, triangle_shadows=True)
    r = skr.Renderer(sc)
    opt = skr.Options(1920, 1080, **ON)
    try:
        frames = []
        for env in (None, "SKR_NO_CULL", "SKR_NO_CONES"):
            if env:
                monkeypatch.setenv(env, "1")
            rgb, rgbf = r.render(opt, want_float=True)
            gpu.cuda.synchronize()
            frames.append((rgb.cpu().numpy(), rgbf.cpu().numpy()))
            if env:
                monkeypatch.delenv(env)
        for rgb, f in frames[1:]:
            assert np.array_equal(bits(f), bits(frames[0][1])) and np.array_equal(rgb, frames[0][0])
    finally:
        r.close()


def test_shading_queries_follow_the_switch(gpu, checker):
    torch = gpu
    path, w, h = scene_path("test.scn"), 96, 72
    kw = dict(gillum=2, depth=3, seed=11, **ON)
    r = skr.Renderer(skr.parse_scene(path, strict=True, triangle_shadows=True))
    try:
        opt = skr.Options(w, h, **kw)
        frame = r.render(opt, want_float=True)[1]
        rays = r.camera_rays(opt).view(-1, 8)
        keys = torch.arange(w * h, dtype=torch.int32, device=rays.device)
        r.counters(reset=True)
        got = r.shade(rays, opt, keys=keys)
        torch.cuda.synchronize()
        assert skr.Renderer.kernel_variant() == "shade_rays_g1_tshadow"
        assert np.array_equal(bits(got.cpu().numpy()), bits(frame.cpu().numpy()).reshape(-1, 3))
        c = r.counters()
        want, st = checker.shade(path, rays.cpu().numpy(), triangle_shadows=True, keys=np.arange(w * h), strict=True, **kw)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        assert [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]] == [int(x) for x in st]
        # caller rays that start outside the trace tree's ball: the trace kernel's waves test every triangle
        ball = r.scene.trace_culling(0)[5]
        rng = np.random.default_rng(3)
        n = 4096 + 17
        dirs = rng.normal(size=(n, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        o = ball[:3] + dirs * float(ball[3]) * rng.uniform(1.5, 3.0, (n, 1))
        target = np.array([0, 0, 5.0]) + rng.uniform(-8, 8, (n, 3))
        far = np.zeros((n, 8), np.float32)
        far[:, 0:3] = o
        far[:, 3] = np.inf
        far[:, 4:7] = (target - o) / np.linalg.norm(target - o, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
        far[:, 7] = np.array([-1], np.int32).view(np.float32)[0]
        got = r.shade(torch.from_numpy(far).to(rays.device), opt, sample=0)
        torch.cuda.synchronize()
        want, _ = checker.shade(path, far, triangle_shadows=True, strict=True, **kw)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        off, _ = checker.shade(path, far, triangle_shadows=False, strict=True, **kw)
        assert (bits(want) != bits(off)).any()
    finally:
        r.close()


@pytest.mark.parametrize("scn", ["spheres2.scn", "test.scn"])
def test_without_shade_triangles_the_switch_is_a_no_op(gpu, scn):
    for kw in (dict(shadow=True), dict(gillum=3, depth=3, shadow=True, seed=4)):
        a = gpu_frame(gpu, scene_path(scn), 96, 54, triangle_shadows=True, **kw)
        b = gpu_frame(gpu, scene_path(scn), 96, 54, triangle_shadows=False, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
        assert a[3] == b[3] and "tshadow" not in a[3]
    # and with shade_triangles but without --shadow
    a = gpu_frame(gpu, scene_path(scn), 64, 36, triangle_shadows=True, shade_triangles=True, gillum=2, seed=3)
    b = gpu_frame(gpu, scene_path(scn), 64, 36, triangle_shadows=False, shade_triangles=True, gillum=2, seed=3)
    assert np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2] and a[3] == b[3] and "tshadow" not in a[3]


def test_a_clone_and_a_one_device_multi_inherit_the_switch(gpu, checker):
    path, w, h = scene_path("test.scn"), 64, 48
    kw = dict(gillum=2, depth=2, seed=5, **ON)
    want = checker.render(path, w, h, triangle_shadows=True, **kw)[0]
    off = checker.render(path, w, h, triangle_shadows=False, **kw)[0]
    assert (want != off).any()
    sc = skr.parse_scene(path, triangle_shadows=True)
    r = skr.Renderer(sc)
    try:
        sc.set_triangle_shadows(False)  # the renderer took the setting when it was made
        clone = r.clone()
        try:
            rgb = clone.render(skr.Options(w, h, **kw))[0]
            gpu.cuda.synchronize()
            assert np.array_equal(rgb.cpu().numpy(), want)
        finally:
            clone.close()
        assert np.array_equal(r.render(skr.Options(w, h, **kw))[0].cpu().numpy(), want)
    finally:
        r.close()
    sc.set_triangle_shadows(True)
    m = binding.Multi(sc, 1)
    try:
        rgb, _ = m.render_frame_host(skr.Options(w, h, **kw), tile_rows=8)
    finally:
        m.close()
    assert np.array_equal(rgb, want)


def test_both_command_lines_take_the_flag(gpu, checker, tmp_path):
    w, h = 96, 72
    args = ["--path", scene_path("test.scn"), "--width", str(w), "--height", str(h), "--gillum", "2", "--shadow", "--seed", "5", "--shade-triangles",
            "--triangle-shadows"]
    want = checker.render(scene_path("test.scn"), w, h, triangle_shadows=True, gillum=2, seed=5, **ON)[0]
    off = checker.render(scene_path("test.scn"), w, h, triangle_shadows=False, gillum=2, seed=5, **ON)[0]
    assert (want != off).any()
    out1, out2 = str(tmp_path / "native.ppm"), str(tmp_path / "py.ppm")
    exe = os.path.join(ROOT, "bin", "raytracer")
    subprocess.run([exe, *args, "--output", out1, "--quiet"], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL, timeout=300)
    subprocess.run([sys.executable, "-m", "skele_raytracer_amd.render_cli", *args, "--output", out2], check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=300)
    for out in (out1, out2):
        assert np.array_equal(read_ppm_bytes(open(out, "rb").read()), want), out


def test_triangle_work_counts_the_shadow_walk(gpu):
    """out[0] / out[1] (the walks' own counts) grow against the frame without the switch; out[2] (the reference's loop: every triangle for
    every radiance ray) does not: the reference has no shadow loop over triangles."""
    work = {}
    for switch in (False, True):
        r = skr.Renderer(skr.parse_scene(scene_path("dragon.scn"), strict=True, triangle_shadows=switch))
        try:
            r.count_triangle_work(True)
            r.triangle_work(reset=True)
            r.counters(reset=True)
            r.render(skr.Options(160, 120, **ON))
            gpu.cuda.synchronize()
            work[switch] = r.triangle_work(reset=False)
        finally:
            r.close()
    assert work[True]["cull_tests"] > work[False]["cull_tests"] and work[True]["triangle_tests"] > work[False]["triangle_tests"]
    assert work[True]["reference_triangle_tests"] == work[False]["reference_triangle_tests"] > 0
