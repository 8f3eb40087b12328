"""--scn-fog and --scn-fov on the MI355X (pytest -m gpu): the fog term, the exp form and whole fog frames against the CPU checker
(tests/fog_checker.c) bit for bit, the routing, the partitions and the errors (DESIGN.md "Spherical fog")."""
import os
import subprocess

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding
from conftest import ROOT, SCENES, scene_path
from fog_check import build as build_checker

pytestmark = pytest.mark.gpu
RNG = np.random.default_rng(2026)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("fogcheck")))


def render(scene, w, h, **kw):
    import torch
    r = skr.Renderer(scene)
    try:
        r.counters(reset=True)
        rgb, rgbf = r.render(skr.Options(w, h, **kw), want_float=True)
        torch.cuda.synchronize()
        return rgb.cpu().numpy(), rgbf.cpu().numpy(), r.counters(), r.kernel_variant()
    finally:
        r.close()


def same(g_rgb, g_f, c_rgb, c_f, what):
    nb = int((g_f.view(np.uint32) != c_f.view(np.uint32)).sum())
    assert nb == 0, "%s: %d float words differ, first at %s" % (what, nb, np.argwhere(g_f.view(np.uint32) != c_f.view(np.uint32))[:3])
    assert np.array_equal(g_rgb, c_rgb), what


def test_exp_spec_on_the_device(gpu, checker):
    x = np.concatenate([RNG.uniform(-746, 710, 4000), RNG.uniform(-2, 0, 4000), -RNG.exponential(5, 4000),
                        [0.0, -0.0, 1e-300, -745.5, 709.9, 800.0, -800.0, np.inf, -np.inf, np.nan]])
    out = binding.debug_eval(10, x.astype(np.float64).view(np.uint32).reshape(-1, 2), 2)
    got = out.reshape(-1).view(np.float64)
    want = np.array([checker.exp(v) for v in x])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_fog_term_on_the_device(gpu, checker):
    n = 8192
    rec = np.zeros((n, 40), np.uint32)
    f = rec.view(np.float32)
    f[:, 0] = RNG.uniform(0.5, 60, n)                          # radius
    f[:, 1] = RNG.choice([0.0, 0.001, 0.005, 0.02], n)         # absorption
    f[:, 2] = RNG.uniform(0.0, 0.04, n)                        # scattering
    f[:, 4:7] = RNG.uniform(0, 1, (n, 3))                      # albedo
    L = RNG.normal(size=(n, 3))
    f[:, 8:11] = L / np.linalg.norm(L, axis=1, keepdims=True)
    f[:, 11] = RNG.uniform(1e-4, 1e-2, n)                      # intensity
    f[:, 12:15] = RNG.uniform(0, 1, (n, 3))                    # light colour
    rec[:, 15] = RNG.integers(0, 2, n)                         # pass
    f[:, 16:19] = RNG.uniform(-50, 50, (n, 3))                 # sphere centre
    rec[:, 19] = RNG.integers(0, 64, n)                        # fog index
    f[:, 20:23] = RNG.uniform(-50, 50, (n, 3))                 # light position
    rec[:, 23] = RNG.integers(0, 8, n)                         # light index
    f[:, 24:27] = RNG.uniform(0, 1, (n, 3))                    # kd
    rec[:, 27] = RNG.integers(0, 1920 * 1080, n)               # pixel
    N = RNG.normal(size=(n, 3))
    f[:, 28:31] = N / np.linalg.norm(N, axis=1, keepdims=True)
    rec[:, 31] = RNG.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)  # node
    rec[:, 32] = RNG.integers(0, 25, n)                        # aa
    rec[:, 33:35] = RNG.integers(0, 2**32, (n, 2), dtype=np.uint64).astype(np.uint32)
    got = binding.debug_eval(11, rec, 4)
    want = checker.fog_term_records(rec)
    assert np.array_equal(got, want)
    # both branches of blinn_phong.h:29 were taken
    p = want[:, 3].view(np.float32)
    assert (p < 0.3).sum() > n // 10 and (p > 0.7).sum() > n // 10


SPHERES2_CASES = [
    ("d1", dict(depth=1), False),
    ("d1_shadow", dict(depth=1, shadow=True), False),
    ("jsample3", dict(jsample=3, shadow=True, seed=4), False),
    ("gillum4_depth3", dict(gillum=4, depth=3, shadow=True, seed=17), False),
    ("strict", dict(gillum=2, depth=2, shadow=True, seed=8), True),
]


@pytest.mark.parametrize("name,kw,strict", SPHERES2_CASES, ids=[c[0] for c in SPHERES2_CASES])
def test_spheres2_fog_frames_match_the_checker(gpu, checker, name, kw, strict):
    w, h = (96, 54) if "gillum" not in kw else (64, 36)
    scene = skr.parse_scene(scene_path("spheres2.scn"), strict=strict, fog=True)
    fog = scene.fog
    assert len(fog) == 1
    g_rgb, g_f, cnt, variant = render(scene, w, h, **kw)
    assert variant == "level_pipeline_g1"
    c_rgb, c_f, st = checker.render(scene_path("spheres2.scn"), w, h, fog, strict=strict, **kw)
    same(g_rgb, g_f, c_rgb, c_f, name)
    assert [cnt["radiance_rays"], cnt["sphere_hits"], cnt["shadow_rays"]] == st.tolist()
    # the fog changes the frame
    plain = render(skr.parse_scene(scene_path("spheres2.scn"), strict=strict), w, h, **kw)[1]
    assert not np.array_equal(plain, g_f)


def test_generated_scene_with_several_fogs(gpu, checker, tmp_path):
    rng = np.random.default_rng(77)
    lines = ["camera 0 0 30 0 0 -1 0 1 0 30", "background 0.1 0.1 0.2", "ambient_light 0.1 0.1 0.1"]
    spheres, lights = [], []
    for i in range(12):
        lines.append("material %g %g %g %g %g %g %g %g %g 16 0 0 0 1" % tuple(rng.uniform(0.1, 1, 9)))
        c = rng.uniform(-12, 12, 3) * [1, 1, 0.5] - [0, 0, 10]
        spheres.append(c)
        lines.append("sphere %g %g %g %g" % (*c, rng.uniform(1, 4)))
    for i in range(3):
        lp = rng.uniform(-20, 20, 3) + [0, 10, 0]
        lights.append(lp)
        lines.append("point_light %g %g %g %g %g %g" % (*rng.uniform(50, 200, 3), *lp))
    path = tmp_path / "fogs.scn"
    path.write_text("\n".join(lines) + "\n")
    # x y z radius r g b scattering absorption: p = exp(-min(|C - Lp|, 2 r) (a + s)) mostly in (0.1, 0.9)
    fog = np.array([[0, 0, 0, 40, 0.9, 0.6, 0.3, 0.02, 0.02],
                    [5, 5, 5, 4, 0.2, 0.8, 0.4, 0.15, 0.05],
                    [0, 0, 0, 30, 1.0, 1.0, 1.0, 0.5, -0.47],
                    [1, 2, 3, 10, 0.3, 0.3, 0.9, 0.05, 0.0]], np.float32)
    d = np.linalg.norm(np.array(spheres)[:, None, :] - np.array(lights)[None, :, :], axis=2)
    p = np.exp(-np.minimum(d[..., None], 2 * fog[:, 3]) * (fog[:, 7] + fog[:, 8]))
    assert ((p > 0.1) & (p < 0.9)).mean() > 0.6
    scene = skr.parse_scene(str(path))
    scene.set_fog(fog)
    for kw in (dict(depth=1, shadow=True), dict(gillum=3, depth=3, shadow=True, seed=23), dict(jsample=2, gillum=2, depth=2, seed=3)):
        g_rgb, g_f, cnt, variant = render(scene, 80, 60, **kw)
        assert variant == "level_pipeline_g1"
        c_rgb, c_f, st = checker.render(str(path), 80, 60, fog, **kw)
        same(g_rgb, g_f, c_rgb, c_f, str(kw))
        assert [cnt["radiance_rays"], cnt["sphere_hits"], cnt["shadow_rays"]] == st.tolist()


def test_full_size_headline_fog_frame_on_a_band(gpu, checker):
    scene = skr.parse_scene(scene_path("spheres2.scn"), fog=True)
    kw = dict(gillum=16, shadow=True, seed=20261015)
    g_rgb, g_f, _, variant = render(scene, 1920, 1080, **kw)
    assert variant == "level_pipeline_g1"
    y0, y1 = 600, 604
    c_rgb, c_f, _ = checker.render(scene_path("spheres2.scn"), 1920, 1080, scene.fog, y0=y0, y1=y1, **kw)
    same(g_rgb[y0:y1], g_f[y0:y1], c_rgb, c_f, "1080p band")


def test_fog_frame_is_partition_independent(gpu):
    import torch
    scene = skr.parse_scene(scene_path("spheres2.scn"), fog=True)
    opt = skr.Options(128, 72, gillum=3, depth=2, shadow=True, seed=6)
    r = skr.Renderer(scene)
    try:
        whole = r.render(opt, want_float=True)[1].cpu().numpy()
        tr, G = 8, 3
        frame = np.zeros_like(whole)
        for first in range(G):
            part = r.render(opt, want_float=True, tile_rows=tr, first_tile=first, tile_stride=G)[1].cpu().numpy()
            for k, t in enumerate(range(first, (72 + tr - 1) // tr, G)):
                frame[t * tr:(t + 1) * tr] = part[k * tr:(k + 1) * tr]
        torch.cuda.synchronize()
        assert np.array_equal(frame.view(np.uint32), whole.view(np.uint32))
        u8 = r.render(opt)[0].cpu().numpy()
    finally:
        r.close()
    m = binding.Multi(scene, 1)
    try:
        rgb, _ = m.render_frame_host(opt, tile_rows=8)
    finally:
        m.close()
    assert np.array_equal(rgb, u8)


def test_fog_with_legacy_reflect_or_shade_triangles_is_an_error(gpu):
    scene = skr.parse_scene(scene_path("spheres1.scn"), fog=True)
    scene.set_fog([[0, 0, 0, 10, 1, 1, 1, 0.1, 0.1]])
    r = skr.Renderer(scene)
    try:
        for kw in (dict(legacy_reflect=True), dict(shade_triangles=True)):
            with pytest.raises(skr.SkrError, match="cannot be combined"):
                r.render(skr.Options(32, 18, **kw))
    finally:
        r.close()


@pytest.mark.parametrize("scn", sorted(f for f in os.listdir(SCENES) if f.endswith(".scn")))
def test_cli_scn_fov_equals_fov_2h(gpu, tmp_path, scn):
    exe = os.path.join(ROOT, "bin", "raytracer")
    h = skr.parse_scene(scene_path(scn)).info.camera[12]
    fov = repr(float(np.float32(2) * np.float32(h)))
    base = [exe, "--path", scene_path(scn), "--width", "64", "--height", "36", "--quiet", "--shadow", "--gillum", "2", "--depth", "2"]

    def run(*extra):
        out = str(tmp_path / ("o%d.ppm" % len(os.listdir(tmp_path))))
        res = subprocess.run(base + ["--output", out, *extra], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and "WROTE TO PPM" in res.stdout, res.stderr
        return open(out, "rb").read()

    a, b = run("--scn-fov"), run("--fov", fov)
    assert a == b
    assert run("--scn-fov", "--fov", "37") == run("--fov", "37")  # an explicit --fov wins
