"""The denoiser on the MI355X (include/skr.h skr_denoise, skr_render_denoised_host): GPU == the CPU checker
(tests/denoise_checker.c) bit for bit on real frames with real guides and on synthetic ones, the camera-ray guides equal with and
without culling and against the ray-query checker, the quality bounds against a 256-pass mean, no side effects, and both command lines."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import skele_raytracer_amd as skr
from conftest import ROOT, read_ppm_bytes, scene_path
from denoise_check import build as build_checker, random_frame, random_guides
from ray_query_check import build as build_ray_checker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("denoise_gpu")))


def guide_options(opt):
    """opt with jsample 0: the pixel centres."""
    g = skr.Options(opt.width, opt.height)
    C.memmove(C.byref(g.c), C.byref(opt.c), C.sizeof(opt.c))
    g.c.grid_size = 0
    return g


def frame_and_guides(r, opt):
    """The float frame and its guides, by the documented recipe: trace(camera_rays(opt with jsample 0))."""
    _, rgbf = r.render(opt, want_float=True)
    hits = r.trace(r.camera_rays(guide_options(opt)).view(-1, 8))
    torch.cuda.synchronize()
    return rgbf, hits


def assert_same(gpu_rgb, gpu_f, ref_rgb, ref_f, what):
    gf, rf = gpu_f.cpu().numpy(), ref_f
    bad = gf.view(np.uint32) != rf.view(np.uint32)
    assert not bad.any(), "%s: %d float words differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[:3].tolist())
    assert np.array_equal(gpu_rgb.cpu().numpy(), ref_rgb), what


SCENES = {
    "spheres2": ("spheres2.scn", dict(gillum=16, shadow=True)),
    "bear": ("bear.scn", dict(gillum=8, shadow=True)),
    "test": ("test.scn", dict(gillum=4, shadow=True)),
    "dragon": ("dragon.scn", dict(gillum=16)),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_gpu_equals_checker_on_frames(chk, name):
    scn, kw = SCENES[name]
    r = skr.Renderer(skr.parse_scene(scene_path(scn)), 0)
    opt = skr.Options(640, 360, seed=3, **kw)
    rgbf, hits = frame_and_guides(r, opt)
    kinds = set(np.unique(hits.kind.cpu().numpy()).tolist())
    assert 0 in kinds and (1 in kinds or 2 in kinds), kinds
    c, g = rgbf.cpu().numpy(), hits.raw.cpu().numpy()
    for L in (0, 1, 5, 16):
        rgb, out = r.denoise(rgbf, hits, L)
        torch.cuda.synchronize()
        ref_rgb, ref_f = chk.denoise(c, g, L)
        assert_same(rgb, out, ref_rgb, ref_f, "%s L=%d" % (name, L))
        if L == 0:
            assert np.array_equal(out.cpu().numpy().view(np.uint32), c.view(np.uint32))


def test_gpu_equals_checker_on_the_headline_frame(chk):
    r = skr.Renderer(skr.parse_scene(scene_path("spheres2.scn")), 0)
    opt = skr.Options(1920, 1080, gillum=16, shadow=True)
    rgbf, hits = frame_and_guides(r, opt)
    rgb, out = r.denoise(rgbf, hits, 5)
    torch.cuda.synchronize()
    ref_rgb, ref_f = chk.denoise(rgbf.cpu().numpy(), hits.raw.cpu().numpy(), 5)
    assert_same(rgb, out, ref_rgb, ref_f, "headline L=5")


@pytest.mark.parametrize("h,w", [(1, 1), (1, 37), (17, 13), (40, 23), (33, 70)])
@pytest.mark.parametrize("L", [0, 1, 5, 16])
def test_gpu_equals_checker_on_synthetic_guides(chk, h, w, L):
    r = skr.Renderer(skr.parse_scene(scene_path("spheres2.scn")), 0)
    seed = 7 * h + w
    g, c = random_guides(h, w, seed), random_frame(h, w, seed)
    rgb, out = r.denoise(torch.from_numpy(c).cuda(), torch.from_numpy(g).cuda(), L)
    torch.cuda.synchronize()
    ref_rgb, ref_f = chk.denoise(c, g, L)
    assert_same(rgb, out, ref_rgb, ref_f, "%dx%d L=%d" % (h, w, L))


@pytest.mark.parametrize("scn", ["dragon.scn", "test.scn", "pose_dragon_rolled.scn", "pose_dragon_inside.scn"])  # + a rolled and a mesh-interior pose (tests/camera_poses.py)
def test_camera_guides_culled_equal_every_triangle_and_the_checker(scn):
    """Camera waves of skr_trace_rays walk the renderer's tree: the same bits as every triangle and as the ray-query checker."""
    import tempfile
    sc = skr.parse_scene(scene_path(scn))
    r = skr.Renderer(sc, 0)
    opt = skr.Options(1920, 1080)
    rays = r.camera_rays(opt).view(-1, 8)
    culled = r.trace(rays).raw.cpu().numpy()
    culled_any = r.trace(rays, any_hit=True).cpu().numpy()
    os.environ["SKR_NO_CULL"] = "1"
    try:
        r2 = skr.Renderer(sc, 0)
        brute = r2.trace(rays).raw.cpu().numpy()
        brute_any = r2.trace(rays, any_hit=True).cpu().numpy()
    finally:
        del os.environ["SKR_NO_CULL"]
    assert np.array_equal(culled.view(np.uint32), brute.view(np.uint32))
    assert np.array_equal(culled_any, brute_any)
    assert np.array_equal(culled_any, (culled[:, 1].view(np.int32) != 0).astype(np.int32))
    pick = np.random.default_rng(14).choice(len(culled), 1 << 14, replace=False)
    s, t, _ = sc.arrays()
    ray_chk = build_ray_checker(tempfile.mkdtemp(prefix="dn_raycheck"))
    want = ray_chk.trace(s, t, rays.cpu().numpy()[pick])[0]
    assert np.array_equal(culled[pick].view(np.uint32), want.view(np.uint32))
    for st in (False, True):  # the guides of either triangle rule's frame are the same rays
        g = r.trace(r.camera_rays(skr.Options(1920, 1080, shade_triangles=st)).view(-1, 8)).raw.cpu().numpy()
        assert np.array_equal(g[pick].view(np.uint32), want.view(np.uint32)), st


def _mse(x, ref):
    return float(np.mean((np.minimum(x, 1) - np.minimum(ref, 1)) ** 2))


@pytest.mark.parametrize("scn,kw,bound", [("spheres2.scn", dict(gillum=16, shadow=True, depth=3), 0.40), ("bear.scn", dict(gillum=8, shadow=True), 0.6)])
def test_quality_against_a_256_pass_mean(scn, kw, bound):
    r = skr.Renderer(skr.parse_scene(scene_path(scn)), 0)
    w, h = 480, 270
    ref = r.render(skr.Options(w, h, seed=1000, progressive=256, **kw), want_float=True)[1].cpu().numpy().astype(np.float64)
    opt = skr.Options(w, h, seed=1, **kw)
    rgbf, hits = frame_and_guides(r, opt)
    _, den = r.denoise(rgbf, hits, 5)
    raw = rgbf.cpu().numpy().astype(np.float64)
    ratio = _mse(den.cpu().numpy().astype(np.float64), ref) / _mse(raw, ref)
    print("%s denoised / raw mse = %.3f" % (scn, ratio))
    assert ratio <= bound, ratio


def test_denoise_changes_nothing_a_render_reads():
    r = skr.Renderer(skr.parse_scene(scene_path("spheres2.scn")), 0)
    opt = skr.Options(320, 180, gillum=4, shadow=True)
    r.counters(reset=True)
    a, af = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    ca, va = r.counters(reset=True), r.kernel_variant()
    g = skr.Options(320, 180)
    hits = r.trace(r.camera_rays(g).view(-1, 8))
    r.denoise(af, hits, 5)
    torch.cuda.synchronize()
    assert r.counters(reset=False) == {k: 0 for k in ca} and r.kernel_variant() == va
    b, bf = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    assert r.counters(reset=True) == ca and r.kernel_variant() == va
    assert torch.equal(a, b) and torch.equal(af.view(torch.int32), bf.view(torch.int32))


@pytest.mark.parametrize("progressive", [1, 4])
def test_render_denoised_host_equals_the_three_steps(progressive):
    r = skr.Renderer(skr.parse_scene(scene_path("spheres2.scn")), 0)
    opt = skr.Options(400, 224, gillum=4, shadow=True, jsample=2, progressive=progressive)
    _, rgbf = r.render(opt, want_float=True)
    rgb, out = r.denoise(rgbf, r.trace(r.camera_rays(guide_options(opt)).view(-1, 8)), 5)
    h_rgb, h_f, ms = r.render_denoised(opt, 5, want_float=True)
    assert ms > 0
    assert np.array_equal(h_rgb, rgb.cpu().numpy())
    assert np.array_equal(h_f.view(np.uint32), out.cpu().numpy().view(np.uint32))
    only_rgb, none, _ = r.render_denoised(opt, 5)
    assert none is None and np.array_equal(only_rgb, h_rgb)


def test_argument_errors():
    L = skr.lib()
    r = skr.Renderer(skr.parse_scene(scene_path("spheres2.scn")), 0)
    h, w = 8, 16
    c = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    g = torch.zeros((h * w, 8), dtype=torch.float32, device="cuda")
    o = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    b = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    big = torch.zeros(h * w * 16, dtype=torch.float32, device="cuda")
    ok = lambda *a: L.skr_denoise(r.h, *a, None)
    assert ok(w, h, c.data_ptr(), g.data_ptr(), 5, o.data_ptr(), b.data_ptr()) == 0
    assert ok(w, h, c.data_ptr(), g.data_ptr(), 5, o.data_ptr(), None) == 0
    assert ok(w, h, c.data_ptr(), g.data_ptr(), 5, None, b.data_ptr()) == 0
    bad = [
        (w, h, c.data_ptr(), g.data_ptr(), 5, None, None),                       # no output
        (w, h, None, g.data_ptr(), 5, o.data_ptr(), None),                       # no frame
        (w, h, c.data_ptr(), None, 5, o.data_ptr(), None),                       # no guides
        (w, h, c.data_ptr(), g.data_ptr() + 4, 5, o.data_ptr(), None),           # misaligned guides
        (w, h, c.data_ptr() + 2, g.data_ptr(), 5, o.data_ptr(), None),           # misaligned frame
        (w, h, c.data_ptr(), g.data_ptr(), 17, o.data_ptr(), None),              # iterations
        (0, h, c.data_ptr(), g.data_ptr(), 5, o.data_ptr(), None),               # size
        (w, 65537, c.data_ptr(), g.data_ptr(), 5, o.data_ptr(), None),
        (w, h, c.data_ptr(), g.data_ptr(), 5, c.data_ptr(), None),               # in place
        (w, h, big.data_ptr(), g.data_ptr(), 5, big.data_ptr() + 64, None),      # overlapping
        (w, h, c.data_ptr(), g.data_ptr(), 5, None, g.data_ptr() + 8),           # bytes over the guides
        (w, h, c.data_ptr(), g.data_ptr(), 5, o.data_ptr(), o.data_ptr() + 12),  # the two outputs
    ]
    for a in bad:
        assert ok(*a) == 2, a
    with pytest.raises(skr.SkrError):
        r.denoise(c, g[:-1], 5)
    torch.cuda.synchronize()


def _read_pfm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], "<f4", w * h * 3).reshape(h, w, 3)[::-1]


def test_both_command_lines_write_the_denoised_frame(tmp_path):
    scn = scene_path("spheres2.scn")
    W, H = 200, 120
    r = skr.Renderer(skr.parse_scene(scn), 0)
    want_rgb, want_f, _ = r.render_denoised(skr.Options(W, H, gillum=4, shadow=True, seed=5), 5, want_float=True)
    args = ["--path", scn, "--width", str(W), "--height", str(H), "--gillum", "4", "--shadow", "--seed", "5", "--denoise", "5"]
    exe = os.path.join(ROOT, "bin", "raytracer")
    native = lambda extra, out: subprocess.run([exe, *args, *extra, "--output", out, "--quiet"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    py = lambda extra, out: subprocess.run([sys.executable, "-m", "skele_raytracer_amd.render_cli", *args, *extra, "--output", out], cwd=ROOT, capture_output=True, text=True,
                                           timeout=300)
    for tag, run in (("native", native), ("py", py)):
        ppm, pfm = str(tmp_path / (tag + ".ppm")), str(tmp_path / (tag + ".pfm"))
        p = run([], ppm)
        assert p.returncode == 0, (tag, p.stderr)
        assert np.array_equal(read_ppm_bytes(open(ppm, "rb").read()), want_rgb), tag
        p = run(["--format", "pfm"], pfm)
        assert p.returncode == 0, (tag, p.stderr)
        assert np.array_equal(_read_pfm(pfm).view(np.uint32), want_f.view(np.uint32)), tag
        bad = run(["--progressive", "3", "--progressive-every", "1"], str(tmp_path / "x.ppm"))
        assert bad.returncode != 0 and "--denoise" in bad.stderr, (tag, bad.stderr)
        bad = run(["--denoise", "17"], str(tmp_path / "x.ppm"))
        assert bad.returncode != 0 and "--denoise" in bad.stderr, (tag, bad.stderr)
    bad = native(["--gpus", "2"], str(tmp_path / "x.ppm"))
    assert bad.returncode != 0 and "--denoise" in bad.stderr
    one = native(["--gpus", "1"], str(tmp_path / "one.ppm"))  # --gpus 1: the one device
    assert one.returncode == 0, one.stderr
    assert np.array_equal(read_ppm_bytes(open(str(tmp_path / "one.ppm"), "rb").read()), want_rgb)
