"""The thin-lens camera on the MI355X (include/skr.h skr_scene_set_lens): whole frames against the CPU checker
(tests/lens_checker.c) — bytes, float bits and the four work counters, no tolerance — in every mode that combines with a lens, the
camera rays and the debug op, culling, bands, tiles and rows, adaptive frames, the refused combinations, what a scene with aperture 0
leaves alone, both command lines.  Frames are 67 x 35 and 130 x 21: off the 64-lane and 16-pixel grids, a wave straddles rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding
from conftest import ROOT, read_ppm_bytes, scene_path
from oracle import pyoracle
from lens_check import build as build_checker
from test_lens_cpu import random_records

pytestmark = pytest.mark.gpu
f32 = np.float32
LENS_OP = 22  # include/skr.h skr_debug_eval
SIZES = [(67, 35), (130, 21)]
# the lens of each scene file: the focus at the t of its spheres, an aperture that moves the image by a few pixels
LENS = {"test.scn": (0.8, 25.0), "spheres2.scn": (0.3, 11.0), "dragon.scn": (0.01, 0.3)}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("lenscheck_gpu")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load(scn, lens=None, *, radii=None, **flags):
    sc = skr.parse_scene(scene_path(scn) if not os.path.isabs(scn) else scn, **flags)
    if radii is not None:
        sc.set_light_radii(radii)
    if lens is not None:
        sc.set_lens(*lens)
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


def checker_frame(checker, sc, scn, w, h, lens, *, strict=False, triangle_shadows=False, progressive=1, **kw):
    """the checker's frame of the scene file under the library scene's spot lights, cones and radii"""
    extra = dict(spots=sc.spot_lights, cones=sc.spot_cones, radii=sc.light_radii, triangle_shadows=triangle_shadows, strict=strict)
    path = scene_path(scn) if not os.path.isabs(scn) else scn
    if progressive > 1:
        return checker.render_progressive(path, w, h, progressive, aperture=lens[0], focus=lens[1], **extra, **kw)
    return checker.render(path, w, h, aperture=lens[0], focus=lens[1], **extra, **kw)


def same_as_checker(gpu, checker, scn, w, h, what, *, lens=None, part="", radii=None, spot=False, strict=False, triangle_shadows=False, **kw):
    lens = lens or LENS[os.path.basename(scn)]
    sc = load(scn, lens, radii=radii, spot=spot, strict=strict, triangle_shadows=triangle_shadows)
    g_rgb, g_f, g_cnt, variant = gpu_frame(gpu, sc, w, h, **kw)
    c_rgb, c_f, c_st = checker_frame(checker, sc, scn, w, h, lens, strict=strict, triangle_shadows=triangle_shadows, **kw)
    nb = int((bits(g_f) != bits(c_f)).sum())
    assert nb == 0, "%s: %d float words differ" % (what, nb)
    assert np.array_equal(g_rgb, c_rgb), what
    assert g_cnt == [int(x) for x in c_st[:4]], what
    in_force = triangle_shadows and kw.get("shade_triangles") and kw.get("shadow") and sc.info.n_triangles > 0  # (spheres2.scn has no triangle: the switch is a no-op)
    assert variant == "level_pipeline_g1" + part + "_lens" + ("_tshadow" if in_force else ""), (what, variant)
    return c_f


# ---- 1. GPU == checker, bit for bit, in every mode that combines with a lens ----
ST = dict(shade_triangles=True, shadow=True)
MODES = [
    ("direct", dict(), dict()),
    ("shadow", dict(), dict(shadow=True)),
    ("gi3_d3_shadow", dict(), dict(gillum=3, depth=3, shadow=True, seed=5)),
    ("js2", dict(), dict(jsample=2, seed=3)),
    ("gi2_js2", dict(), dict(gillum=2, jsample=2, seed=4)),
    ("strict", dict(strict=True), dict(shadow=True)),
    ("shade_triangles", dict(), dict(**ST)),
    ("triangle_shadows", dict(triangle_shadows=True), dict(**ST)),
    ("progressive3", dict(), dict(progressive=3, shadow=True, seed=7)),
]


@pytest.mark.parametrize("scn,size", [("test.scn", SIZES[0]), ("spheres2.scn", SIZES[1])], ids=["test", "spheres2"])
@pytest.mark.parametrize("name,flags,kw", MODES, ids=[m[0] for m in MODES])
def test_frames_match_the_checker_bit_for_bit(gpu, checker, scn, size, name, flags, kw):
    on = same_as_checker(gpu, checker, scn, *size, "%s %s" % (scn, name), **flags, **kw)
    if name == "shadow":  # the lens does something
        off = checker.render(scene_path(scn), *size, **kw)[1]
        assert (bits(on) != bits(off)).any()


LIGHTS = [
    ("spot", "_spot", dict(spot=True), dict(shadow=True)),
    ("radius", "_soft", dict(radii=0.4), dict(shadow=True, seed=2)),
    ("soft_spot", "_soft", dict(spot=True, radii=[0.4, 0.25]), dict(shadow=True, seed=3)),
    ("soft_spot_tshadow_gi", "_soft", dict(spot=True, radii=[0.4, 0.25], triangle_shadows=True), dict(gillum=2, depth=2, seed=6, **ST)),
    ("spot_tshadow", "_spot", dict(spot=True, triangle_shadows=True), dict(**ST)),
]


@pytest.mark.parametrize("name,part,flags,kw", LIGHTS, ids=[m[0] for m in LIGHTS])
def test_spot_lights_and_radii_under_the_lens(gpu, checker, name, part, flags, kw):
    """test.scn: its point light and, under --scn-spot, its spot light"""
    same_as_checker(gpu, checker, "test.scn", *SIZES[0], name, part=part, **flags, **kw)


def test_one_radius_on_spheres2(gpu, checker):
    same_as_checker(gpu, checker, "spheres2.scn", *SIZES[1], "one radius", part="_soft", radii=[0.5, 0.0], shadow=True, seed=8)


# ---- 2. aperture 0: nothing changes ----
@pytest.mark.parametrize("scn,kw,variant", [("spheres2.scn", dict(shadow=True), "direct_v3"), ("spheres2.scn", dict(gillum=3, depth=3, shadow=True, seed=4), "node_levels"),
                                            ("test.scn", dict(gillum=2, depth=2, seed=4), "level_pipeline_g1")], ids=["direct", "nodes", "generic"])
def test_aperture_zero_renders_as_a_scene_that_never_had_a_lens(gpu, scn, kw, variant):
    w, h = SIZES[0]
    zero = load(scn, (0.5, 3.0))
    zero.set_lens(0.0, 3.0)  # (set and taken back; the focus alone has no effect)
    a = gpu_frame(gpu, zero, w, h, **kw)
    b = gpu_frame(gpu, load(scn), w, h, **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
    assert a[3] == b[3] and a[3].startswith(variant) and "lens" not in a[3]
    o_rgb, o_f, o_st = pyoracle.render(scene_path(scn), w, h, want_float=True, **kw)
    assert np.array_equal(bits(a[1]), bits(o_f)) and np.array_equal(a[0], o_rgb) and a[2] == [int(x) for x in o_st[:4]]
    r = skr.Renderer(zero)
    try:  # and the camera rays are the pinhole's
        r2 = skr.Renderer(load(scn))
        try:
            a_rays, b_rays = (x.camera_rays(skr.Options(w, h, **kw)).cpu().numpy() for x in (r, r2))
            assert np.array_equal(bits(a_rays), bits(b_rays))
        finally:
            r2.close()
    finally:
        r.close()


# ---- 3. camera rays, shading queries of them, the debug op ----
@pytest.mark.parametrize("scn,kw", [("test.scn", dict(**ST)), ("spheres2.scn", dict(gillum=2, depth=3, shadow=True, seed=5))], ids=["test", "spheres2"])
def test_camera_rays_are_the_checkers_and_shade_to_the_frame(gpu, checker, scn, kw):
    torch = gpu
    w, h = SIZES[0]
    lens = LENS[scn]
    r = skr.Renderer(load(scn, lens))
    try:
        opt = skr.Options(w, h, **kw)
        rays = r.camera_rays(opt)
        want = checker.rays(scene_path(scn), w, h, aperture=lens[0], focus=lens[1], seed=kw.get("seed", 1))
        assert np.array_equal(bits(rays.cpu().numpy()).reshape(-1, 8), bits(want))
        js = skr.Options(w, h, jsample=3, **kw)
        want = checker.rays(scene_path(scn), w, h, aperture=lens[0], focus=lens[1], jsample=3, sample=4, seed=kw.get("seed", 1))
        assert np.array_equal(bits(r.camera_rays(js, sample=4).cpu().numpy()).reshape(-1, 8), bits(want))
        frame = r.render(opt, want_float=True)[1]
        torch.cuda.synchronize()
        assert "_lens" in skr.Renderer.kernel_variant()
        keys = torch.arange(w * h, dtype=torch.int32, device=rays.device)
        got = r.shade(rays.view(-1, 8), opt, keys=keys)
        torch.cuda.synchronize()
        assert "lens" not in skr.Renderer.kernel_variant()  # the rays are the caller's
        assert np.array_equal(bits(got.cpu().numpy()), bits(frame.cpu().numpy()).reshape(-1, 3))
    finally:
        r.close()


def test_the_sample_and_the_ray_through_the_debug_op(gpu, checker):
    rec = random_records(4096 + 37, 3)
    got = binding.debug_eval(LENS_OP, rec, 8)
    assert np.array_equal(got, bits(checker.samples(rec)))


# ---- 4. culling: dragon.scn under both triangle rules ----
@pytest.mark.parametrize("shade_triangles", [False, True], ids=["black", "surfaces"])
def test_culled_walks_give_what_every_triangle_gives(gpu, checker, shade_triangles):
    w, h = 48, 32
    kw = dict(shade_triangles=shade_triangles, shadow=True, strict=False)
    opt = {k: v for k, v in kw.items() if k != "strict"}
    want = same_as_checker(gpu, checker, "dragon.scn", w, h, "dragon culled", **opt)
    os.environ["SKR_NO_CULL"] = "1"
    try:
        flat = gpu_frame(gpu, load("dragon.scn", LENS["dragon.scn"]), w, h, **opt)
    finally:
        del os.environ["SKR_NO_CULL"]
    assert np.array_equal(bits(flat[1]), bits(want)) and "_lens" in flat[3]
    assert (bits(want) != bits(np.broadcast_to(want[0, 0], want.shape))).any()  # the dragon is in the picture
    # an aperture that puts lens points outside the trace tree's ball: those waves test every triangle
    sc = load("dragon.scn")
    ball = sc.trace_culling(0)[5].astype(np.float64)
    cam = np.array(list(sc.info.camera)[:3])
    A = float(2 * (ball[3] + np.linalg.norm(cam - ball[:3])))
    big = (A, A)  # (k = 1: |d'| stays under the trees' bounds, so it is the origins that decide)
    rays = checker.rays(scene_path("dragon.scn"), w, h, aperture=big[0], focus=big[1])
    outside = np.linalg.norm(rays[:, :3].astype(np.float64) - ball[:3], axis=1) > ball[3]
    assert outside.any() and not outside.all()
    same_as_checker(gpu, checker, "dragon.scn", w, h, "dragon, origins outside the ball", lens=big, **opt)


# ---- 5. bands, tiles, rows ----
@pytest.mark.parametrize("budget", ["16", "4"])  # two bands; and bands of a few rows (one row's tables are over 1 MB)
def test_a_banded_frame_is_the_frame(gpu, checker, budget):
    w, h = SIZES[1]
    kw = dict(gillum=5, depth=4, shadow=True, seed=6)  # 2730 x 125 rays at the last level: 15 MB of records, over a 16 MB budget with the levels above
    sc = load("spheres2.scn", LENS["spheres2.scn"])
    one = gpu_frame(gpu, sc, w, h, **kw)
    os.environ["SKR_LEVELS_BUDGET_MB"] = budget
    try:
        banded = gpu_frame(gpu, sc, w, h, **kw)
    finally:
        del os.environ["SKR_LEVELS_BUDGET_MB"]
    assert np.array_equal(bits(banded[1]), bits(one[1])) and np.array_equal(banded[0], one[0]) and banded[2] == one[2] and banded[3] == one[3]
    if budget == "16":
        c_rgb, c_f, c_st = checker_frame(checker, sc, "spheres2.scn", w, h, LENS["spheres2.scn"], **kw)
        assert np.array_equal(bits(one[1]), bits(c_f)) and np.array_equal(one[0], c_rgb) and one[2] == [int(x) for x in c_st[:4]]


def test_tiles_and_rows_give_the_frames_rows(gpu, checker):
    w, h = SIZES[0]
    kw = dict(gillum=2, depth=2, shadow=True, seed=5)
    sc = load("spheres2.scn", LENS["spheres2.scn"])
    want = checker_frame(checker, sc, "spheres2.scn", w, h, LENS["spheres2.scn"], **kw)
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, **kw)
        rows = 4
        for first in (0, 1):  # the two interleaved halves
            rgb, rgbf = r.render(opt, want_float=True, tile_rows=rows, first_tile=first, tile_stride=2)
            gpu.cuda.synchronize()
            for k in range(rgb.shape[0] // rows):
                y0 = (first + 2 * k) * rows
                n = min(rows, h - y0)
                assert np.array_equal(bits(rgbf[k * rows:k * rows + n].cpu().numpy()), bits(want[1][y0:y0 + n])), (first, k)
                assert np.array_equal(rgb[k * rows:k * rows + n].cpu().numpy(), want[0][y0:y0 + n])
        for y0, y1 in ((0, h), (5, 6), (9, 31)):
            rgb, rgbf = r.render_rows(opt, y0, y1, want_float=True)
            gpu.cuda.synchronize()
            assert np.array_equal(bits(rgbf.cpu().numpy()), bits(want[1][y0:y1])) and np.array_equal(rgb.cpu().numpy(), want[0][y0:y1])
        clone = r.clone()  # a clone carries the lens
        try:
            assert np.array_equal(bits(clone.render(opt, want_float=True)[1].cpu().numpy()), bits(want[1]))
        finally:
            clone.close()
    finally:
        r.close()
    m = binding.Multi(sc, 1)  # --gpus 1: the frame step's renderer takes the lens with the scene
    try:
        rgb, _ = m.render_frame_host(skr.Options(w, h, **kw), tile_rows=8)
    finally:
        m.close()
    assert np.array_equal(rgb, want[0])


# ---- 6. adaptive frames ----
def test_adaptive_frames_are_progressive_frames_through_both_round_paths(gpu, checker, monkeypatch):
    w, h = SIZES[0]
    K = 3
    kw = dict(gillum=2, depth=2, shadow=True, seed=9)
    sc = load("spheres2.scn", LENS["spheres2.scn"])
    want = checker_frame(checker, sc, "spheres2.scn", w, h, LENS["spheres2.scn"], progressive=K, **kw)
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, **kw)
        prog = r.render(skr.Options(w, h, progressive=K, **kw), want_float=True)
        gpu.cuda.synchronize()
        assert np.array_equal(bits(prog[1].cpu().numpy()), bits(want[1])) and np.array_equal(prog[0].cpu().numpy(), want[0])
        # min == max == K: K whole frames
        rgb, rgbf, passes, _ = r.render_adaptive_host(opt, threshold=-1.0, min_passes=K, max_passes=K, want_float=True)
        assert (passes == K).all()
        assert np.array_equal(bits(rgbf), bits(want[1])) and np.array_equal(rgb, want[0])
        # one whole frame, then K - 1 rounds in which nothing converges: as whole frames, and as shading queries of the lens rays
        for path in ("frame", "query"):
            monkeypatch.setenv("SKR_ADAPTIVE_PATH", path)
            rgb, rgbf, passes, _ = r.render_adaptive_host(opt, threshold=-1.0, min_passes=1, max_passes=K, want_float=True)
            assert (passes == K).all(), path
            assert np.array_equal(bits(rgbf), bits(want[1])) and np.array_equal(rgb, want[0]), path
        monkeypatch.delenv("SKR_ADAPTIVE_PATH")
        js = dict(jsample=2, shadow=True, seed=2)  # the query path per AA sample
        want = checker_frame(checker, sc, "spheres2.scn", w, h, LENS["spheres2.scn"], progressive=2, **js)
        monkeypatch.setenv("SKR_ADAPTIVE_PATH", "query")
        rgb, rgbf, passes, _ = r.render_adaptive_host(skr.Options(w, h, **js), threshold=-1.0, min_passes=1, max_passes=2, want_float=True)
        assert (passes == 2).all() and np.array_equal(bits(rgbf), bits(want[1])) and np.array_equal(rgb, want[0])
    finally:
        r.close()


# ---- 7. the refused combinations and the argument errors ----
def test_the_refused_combinations(gpu):
    lens = LENS["spheres2.scn"]
    cases = [(load("spheres2.scn", lens), dict(legacy_reflect=True), "--legacy-reflect")]
    fog = load("spheres2.scn", lens, fog=True)
    fog.set_fog(np.array([[0, 0, 5, 3, .5, .5, .5, .1, .05]], np.float32))
    cases.append((fog, dict(), "fog volumes"))
    cases.append((load("spheres2.scn", lens, sphere_tree=True), dict(), "sphere tree"))
    for sc, kw, text in cases:
        r = skr.Renderer(sc)
        try:
            with pytest.raises(skr.SkrError) as e:
                r.render(skr.Options(32, 24, **kw))
            assert "(status 4)" in str(e.value) and "a lens (--aperture)" in str(e.value) and text in str(e.value), str(e.value)
        finally:
            r.close()
    r = skr.Renderer(load("spheres2.scn", lens))
    try:
        opt = skr.Options(32, 24, shadow=True)
        for call in (lambda: r.render_denoised(opt), lambda: r.render_adaptive_denoised(opt, min_passes=2, max_passes=2)):
            with pytest.raises(skr.SkrError) as e:
                call()
            assert "(status 4)" in str(e.value) and "a lens (--aperture)" in str(e.value) and "denoiser" in str(e.value), str(e.value)
        # a shading query of caller rays is not the lens's business: legacy_reflect is not refused there
        rays = gpu.zeros((4, 8), dtype=gpu.float32, device="cuda:0")
        rays[:, 6] = 1
        rays[:, 3] = float("inf")
        r.shade(rays, skr.Options(32, 24, legacy_reflect=True))
        gpu.cuda.synchronize()
    finally:
        r.close()
    sc = load("spheres2.scn", lens)
    for a, f in ((np.nan, 1.0), (np.inf, 1.0), (-0.5, 1.0), (0.5, 0.0), (0.5, -1.0), (0.5, np.nan), (0.5, np.inf)):
        with pytest.raises(skr.SkrError):
            sc.set_lens(a, f)
        assert sc.lens == (f32(lens[0]), f32(lens[1]))


# ---- 8. both command lines ----
def test_both_command_lines_take_the_flags(gpu, tmp_path):
    w, h = SIZES[0]
    path, lens = scene_path("spheres2.scn"), LENS["spheres2.scn"]
    args = ["--path", path, "--width", str(w), "--height", str(h), "--shadow", "--seed", "3", "--progressive", "2", "--aperture", str(lens[0]), "--focus", str(lens[1])]
    want = gpu_frame(gpu, load("spheres2.scn", lens), w, h, shadow=True, seed=3, progressive=2)[0]
    off = gpu_frame(gpu, load("spheres2.scn"), w, h, shadow=True, seed=3, progressive=2)[0]
    assert (want != off).any()
    exe = os.path.join(ROOT, "bin", "raytracer")
    out1, out2, out3 = str(tmp_path / "native.ppm"), str(tmp_path / "py.ppm"), str(tmp_path / "focus_only.ppm")
    subprocess.run([exe, *args, "--output", out1, "--quiet"], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL, timeout=300)
    subprocess.run([sys.executable, "-m", "skele_raytracer_amd.render_cli", *args, "--output", out2], check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=300)
    for out in (out1, out2):
        assert np.array_equal(read_ppm_bytes(open(out, "rb").read()), want), out
    # --focus without --aperture is accepted and has no effect
    subprocess.run([exe, *args[:-4], "--focus", "4", "--output", out3, "--quiet"], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL, timeout=300)
    assert np.array_equal(read_ppm_bytes(open(out3, "rb").read()), off)
    bad = subprocess.run([exe, *args[:-4], "--aperture", "-1", "--output", str(tmp_path / "bad.ppm"), "--quiet"], cwd=str(tmp_path), capture_output=True, timeout=300)
    assert bad.returncode == 2 and b"--aperture" in bad.stderr and not os.path.exists(str(tmp_path / "bad.ppm"))
