"""Spot lights on the MI355X (include/skr.h SKR_SCN_SPOT): whole frames and shading queries against the CPU checker
(tests/spot_checker.c) — bytes, float bits and the four work counters, no tolerance —, the cone's decision boundaries through the
debug op, launch shapes, the refused combinations, what the flag leaves alone, both command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding
from conftest import ROOT, read_ppm_bytes, scene_path
from oracle import pyoracle
from spot_check import MIXED_POINTS, MIXED_SPOTS, OCCLUDER, build as build_checker, write_floor_scene
from test_scene_size_gpu import LIMIT, last_lights_within

pytestmark = pytest.mark.gpu
f32 = np.float32
SPOT_OP = 17  # include/skr.h skr_debug_eval


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("spotcheck_gpu")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load(path, *, strict=False, triangle_shadows=False, **flags):
    return skr.parse_scene(path, spot=True, strict=strict, triangle_shadows=triangle_shadows, **flags)


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


def same_as_checker(gpu, checker, path, w, h, what, *, strict=False, triangle_shadows=False, **kw):
    sc = load(path, strict=strict, triangle_shadows=triangle_shadows)
    rows, cones = sc.spot_lights, sc.spot_cones
    assert len(rows) >= 1, what
    g_rgb, g_f, g_cnt, variant = gpu_frame(gpu, sc, w, h, **kw)
    c_rgb, c_f, c_st = checker.render(path, w, h, spots=rows, cones=cones, triangle_shadows=triangle_shadows, strict=strict, **kw)
    nb = int((bits(g_f) != bits(c_f)).sum())
    assert nb == 0, "%s: %d float words differ" % (what, nb)
    assert np.array_equal(g_rgb, c_rgb), what
    assert g_cnt == [int(x) for x in c_st[:4]], what
    in_force = triangle_shadows and kw.get("shade_triangles") and kw.get("shadow")
    assert variant == ("level_pipeline_g1_spot_tshadow" if in_force else "level_pipeline_g1_spot"), what
    return c_f, c_st


# ---- 1. GPU == checker, bit for bit ----
ST = dict(shade_triangles=True, shadow=True)
TEST_SCN = [
    ("direct", 160, 120, False, False, dict()),
    ("shadow", 160, 120, False, False, dict(shadow=True)),
    ("shade_triangles", 160, 120, False, False, dict(**ST)),
    ("triangle_shadows", 160, 120, False, True, dict(**ST)),
    ("triangle_shadows_strict", 160, 120, True, True, dict(**ST)),
    ("js2_shadow", 64, 48, False, False, dict(jsample=2, shadow=True, seed=3)),
    ("gi2_d2", 64, 48, False, False, dict(gillum=2, depth=2, seed=4)),
    ("gi2_d3", 64, 48, False, False, dict(gillum=2, depth=3, seed=5)),
    ("shade_triangles_gi2_d2", 64, 48, False, False, dict(gillum=2, depth=2, seed=6, **ST)),
]


@pytest.mark.parametrize("name,w,h,strict,tshadow,kw", TEST_SCN, ids=[c[0] for c in TEST_SCN])
def test_test_scn_matches_the_checker_bit_for_bit(gpu, checker, name, w, h, strict, tshadow, kw):
    on, _ = same_as_checker(gpu, checker, scene_path("test.scn"), w, h, name, strict=strict, triangle_shadows=tshadow, **kw)
    if name == "shade_triangles":  # the blue cone on the wall: the light does something
        off = checker.render(scene_path("test.scn"), w, h, **kw)[1]
        more_blue = (on[:, :, 2] > off[:, :, 2]) & (on[:, :, 0] == off[:, :, 0])
        assert more_blue.sum() > 50


def test_the_mixed_floor_scene_matches_the_checker(gpu, checker, tmp_path):
    """one point light, a 180/180 spot, a 5/20 spot, a 30/30 spot, an occluder triangle: the pairs (point, wide) and (narrow, hard edge),
    the second with both lights inside, one outside and both outside; then three and four lights with a single tail"""
    scn = write_floor_scene(str(tmp_path / "mixed.scn"), points=MIXED_POINTS, spots=MIXED_SPOTS, tris=[OCCLUDER])
    for tshadow in (False, True):
        _, st = same_as_checker(gpu, checker, scn, 96, 72, "mixed tshadow=%s" % tshadow, triangle_shadows=tshadow, **ST)
        assert int(st[1]) * 2 < int(st[2]) < int(st[1]) * 4
    same_as_checker(gpu, checker, scn, 64, 48, "mixed gi", triangle_shadows=True, gillum=3, depth=3, seed=8, **ST)
    # an odd light count: the last spot light is the pair loop's single tail; and a directional light behind the spot lights
    odd = write_floor_scene(str(tmp_path / "odd.scn"), points=MIXED_POINTS, spots=MIXED_SPOTS[1:], tris=[OCCLUDER])
    same_as_checker(gpu, checker, odd, 96, 72, "odd", triangle_shadows=True, **ST)
    strict = write_floor_scene(str(tmp_path / "strict.scn"), points=MIXED_POINTS, spots=MIXED_SPOTS[1:], tris=[OCCLUDER], directional=True)
    same_as_checker(gpu, checker, strict, 96, 72, "strict", strict=True, triangle_shadows=True, **ST)


@pytest.mark.parametrize("points,spots", [(0, 1), (0, 2), (1, 1)], ids=["one_spot", "two_spots", "point_and_spot"])
def test_small_light_counts(gpu, checker, tmp_path, points, spots):
    scn = write_floor_scene(str(tmp_path / "few.scn"), points=MIXED_POINTS[:points], spots=MIXED_SPOTS[1:1 + spots])
    same_as_checker(gpu, checker, scn, 96, 72, "%d+%d" % (points, spots), shadow=True)
    same_as_checker(gpu, checker, scn, 48, 36, "%d+%d gi" % (points, spots), gillum=2, depth=2, shadow=True, seed=2)


def test_the_largest_light_count_half_of_them_spot_lights(gpu, checker, tmp_path):
    """the floor sphere under as many lights as the general pipeline's LDS holds, every other one a spot light (narrow cones at many
    positions: most are outside at most points); and one more light is refused as it is for point lights"""
    n = last_lights_within("prefix", LIMIT, 1)
    rng = np.random.default_rng(5)

    def lights(count):
        pos = np.c_[rng.uniform(-8, 8, count), rng.uniform(4, 12, count), rng.uniform(-4, 10, count)]
        col = rng.uniform(0.02, 0.08, (count, 3))
        pts = [(*col[i], *pos[i]) for i in range(0, count, 2)]
        sps = []
        for i in range(1, count, 2):  # narrow cones that point roughly down
            a1 = rng.uniform(3, 30)
            sps.append((*(col[i] * 40), *pos[i], rng.normal(0, 0.3), -1.0, rng.normal(0, 0.3), a1, a1 + rng.uniform(0, 25)))
        return pts, sps

    pts, sps = lights(n)
    scn = write_floor_scene(str(tmp_path / "many.scn"), points=pts, spots=sps)
    sc = load(scn)
    assert sc.info.n_point_lights + len(sc.spot_lights) == n and len(sc.spot_lights) == n // 2
    _, st = same_as_checker(gpu, checker, scn, 32, 24, "%d lights" % n, shadow=True)
    assert int(st[2]) < int(st[1]) * n * 3 // 4  # the narrow cones cast no shadow ray where they do not reach
    pts, sps = lights(n + 1)
    over = load(write_floor_scene(str(tmp_path / "over.scn"), points=pts, spots=sps))
    r = skr.Renderer(over)
    try:
        with pytest.raises(skr.SkrError) as e:
            r.render(skr.Options(32, 24, shadow=True))
        assert "LDS" in str(e.value) and "(status 4)" in str(e.value)
    finally:
        r.close()


# ---- 2. the decision boundaries through the debug op ----
def test_the_cone_boundaries_through_the_debug_op(gpu, checker):
    c1, c2 = f32(np.cos(np.radians(5.0))), f32(np.cos(np.radians(20.0)))
    up, down = (lambda x: np.nextafter(f32(x), f32(2))), (lambda x: np.nextafter(f32(x), f32(-2)))
    recs = []
    # a = (0, -1, 0) makes c = -((0 * Lx + -1 * Ly) + 0 * Lz) = Ly exactly: c at c1, c2 and one ulp either side of each, inside, between, outside
    for c in (c1, up(c1), down(c1), c2, up(c2), down(c2), f32(1), f32(0.97), f32(0.95), f32(0.5), f32(-1), f32(0)):
        recs.append([0, -1, 0, c1, c2, 0.25, c, -0.125])
    for c in (c1, up(c1), down(c1)):  # c1 == c2: a hard edge, no division
        recs.append([0, -1, 0, c1, c1, 0, c, 0])
    for bad in ((np.nan, 0.99, 0), (0, np.nan, 0), (0, 0.99, np.nan), (np.inf, 0.5, 0), (0, -np.inf, 0)):  # NaN (and inf - inf) anywhere: outside
        recs.append([0, -1, 0, c1, c2, *bad])
    rng = np.random.default_rng(4)
    for _ in range(40):  # a = L (c = -1: behind the light) and a = -L (c = 1: on the axis), on any axis; and cones of every width
        a = rng.normal(size=3)
        a = (a / np.linalg.norm(a)).astype(f32)
        k1, k2 = np.sort(rng.uniform(-1, 1, 2).astype(f32))[::-1]
        recs.append([*a, k1, k2, *a])
        recs.append([*a, k1, k2, *(-a)])
        recs.append([*a, f32(-1), f32(-1), *a])  # 180 / 180: never outside, f = 1
    for _ in range(400):  # random unit vectors against random cones
        a, L = rng.normal(size=3), rng.normal(size=3)
        k1, k2 = np.sort(rng.uniform(-1, 1, 2).astype(f32))[::-1]
        recs.append([*(a / np.linalg.norm(a)), k1, k2, *(L / np.linalg.norm(L))])
    recs = np.array(recs, np.float32)
    got = binding.debug_eval(SPOT_OP, recs, 2)
    kinds = set()
    for r, g in zip(recs, got):
        f, outside = checker.cone(r[0:3], r[3], r[4], r[5:8])
        assert (int(g[0]), int(g[1])) == (int(np.float32(f).view(np.uint32)), outside), r
        kinds.add("outside" if outside else "full" if f == 1 else "partial")
    assert kinds == {"outside", "full", "partial"}
    # the clauses at the boundaries themselves
    assert [int(x) for x in got[0:6, 1]] == [0, 0, 0, 1, 0, 1] and bits(got[0, 0].view(f32)) == bits(f32(1))
    assert got[4, 0].view(f32) >= 0 and got[4, 0].view(f32) < 1e-6
    assert [int(x) for x in got[12:15, 1]] == [0, 0, 1]
    assert (got[15:20, 1] == 1).all()


# ---- 3. shading queries ----
@pytest.mark.parametrize("name,tshadow,kw", [("shade_triangles", True, dict(**ST)), ("gi2_d3", False, dict(gillum=2, depth=3, shadow=True, seed=5))])
def test_camera_rays_give_the_frame(gpu, checker, name, tshadow, kw):
    torch = gpu
    path, w, h = scene_path("test.scn"), 64, 48
    sc = load(path, triangle_shadows=tshadow)
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, **kw)
        frame = r.render(opt, want_float=True)[1]
        rays = r.camera_rays(opt).view(-1, 8)
        keys = torch.arange(w * h, dtype=torch.int32, device=rays.device)
        r.counters(reset=True)
        got = r.shade(rays, opt, keys=keys)
        torch.cuda.synchronize()
        assert skr.Renderer.kernel_variant() == ("shade_rays_g1_spot_tshadow" if tshadow else "shade_rays_g1_spot")
        assert np.array_equal(bits(got.cpu().numpy()), bits(frame.cpu().numpy()).reshape(-1, 3))
        c = r.counters()
        want, st = checker.shade(path, rays.cpu().numpy(), spots=sc.spot_lights, cones=sc.spot_cones, triangle_shadows=tshadow, keys=np.arange(w * h), **kw)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        assert [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]] == [int(x) for x in st]
    finally:
        r.close()


def test_arbitrary_rays_match_the_checker(gpu, checker, tmp_path):
    torch = gpu
    scn = write_floor_scene(str(tmp_path / "mixed.scn"), points=MIXED_POINTS, spots=MIXED_SPOTS, tris=[OCCLUDER])
    sc = load(scn, triangle_shadows=True)
    kw = dict(gillum=2, depth=2, seed=9, **ST)
    rng = np.random.default_rng(6)
    n = 300 + 17
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = np.c_[rng.uniform(-6, 6, n), rng.uniform(3, 9, n), rng.uniform(-6, 8, n)]
    target = np.c_[rng.uniform(-8, 8, n), np.zeros(n), rng.uniform(-4, 10, n)]
    d = target - rays[:, 0:3]
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    rays[: n // 8, 4:7] *= -1  # some look away from the floor: misses
    rays[:, 3] = np.inf
    rays[:, 7] = np.array([-1], np.int32).view(np.float32)[0]
    r = skr.Renderer(sc)
    try:
        r.counters(reset=True)
        got = r.shade(torch.from_numpy(rays).to("cuda:0"), skr.Options(8, 8, **kw), sample=0)
        torch.cuda.synchronize()
        c = r.counters()
        want, st = checker.shade(scn, rays, spots=sc.spot_lights, cones=sc.spot_cones, triangle_shadows=True, **kw)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        assert [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]] == [int(x) for x in st]
        assert int(st[1]) > n // 2
    finally:
        r.close()


# ---- 4. launch shapes and the modes above a frame ----
def test_tiles_strides_and_a_one_device_multi_give_the_frame(gpu, checker):
    path, w, h = scene_path("test.scn"), 96, 72
    kw = dict(gillum=2, depth=2, seed=5, **ST)
    sc = load(path, triangle_shadows=True)
    want = checker.render(path, w, h, spots=sc.spot_lights, cones=sc.spot_cones, triangle_shadows=True, **kw)
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, **kw)
        full = r.render(opt, want_float=True)
        gpu.cuda.synchronize()
        assert np.array_equal(full[0].cpu().numpy(), want[0]) and np.array_equal(bits(full[1].cpu().numpy()), bits(want[1]))
        rows = 8
        for first, stride in ((0, 2), (1, 2), (2, 3)):
            rgb, rgbf = r.render(opt, want_float=True, tile_rows=rows, first_tile=first, tile_stride=stride)
            gpu.cuda.synchronize()
            for k in range(rgb.shape[0] // rows):
                t = first + k * stride
                assert np.array_equal(bits(rgbf[k * rows:(k + 1) * rows].cpu().numpy()), bits(want[1][t * rows:(t + 1) * rows])), (first, stride, k)
                assert np.array_equal(rgb[k * rows:(k + 1) * rows].cpu().numpy(), want[0][t * rows:(t + 1) * rows])
        clone = r.clone()
        try:
            assert np.array_equal(clone.render(opt)[0].cpu().numpy(), want[0])
        finally:
            clone.close()
    finally:
        r.close()
    m = binding.Multi(sc, 1)
    try:
        rgb, _ = m.render_frame_host(skr.Options(w, h, **kw), tile_rows=8)
    finally:
        m.close()
    assert np.array_equal(rgb, want[0])


def test_two_progressive_passes_are_the_mean_of_two_checker_frames(gpu, checker):
    path, w, h = scene_path("test.scn"), 64, 48
    kw = dict(gillum=2, depth=2, **ST)
    sc = load(path)
    frames = [checker.render(path, w, h, spots=sc.spot_lights, cones=sc.spot_cones, seed=11 + k, **kw)[1] for k in range(2)]
    assert (bits(frames[0]) != bits(frames[1])).any()
    mean = (frames[0] + frames[1]) / f32(2)
    r = skr.Renderer(sc)
    try:
        rgb, rgbf = r.render(skr.Options(w, h, seed=11, progressive=2, **kw), want_float=True)
        gpu.cuda.synchronize()
        assert np.array_equal(bits(rgbf.cpu().numpy()), bits(mean))
        assert np.array_equal(rgb.cpu().numpy(), pyoracle.quantise(mean))
    finally:
        r.close()


def test_adaptive_and_denoised_frames_sit_above_the_spot_frame(gpu, checker, monkeypatch):
    """the modes above a frame: min == max == 2 adaptive passes are the two-pass mean; the adaptive rounds give the same bits as whole
    frames and as shading queries of the active pixels; zero denoiser iterations hand the frame through"""
    path, w, h = scene_path("test.scn"), 64, 48
    kw = dict(gillum=2, depth=2, **ST)
    sc = load(path)
    frames = [checker.render(path, w, h, spots=sc.spot_lights, cones=sc.spot_cones, seed=11 + k, **kw)[1] for k in range(2)]
    mean = (frames[0] + frames[1]) / f32(2)
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, seed=11, **kw)
        rgb, rgbf, passes, _ = r.render_adaptive_host(opt, threshold=-1.0, min_passes=2, max_passes=2, want_float=True)
        assert (passes == 2).all() and np.array_equal(bits(rgbf), bits(mean)) and np.array_equal(rgb, pyoracle.quantise(mean))
        got = {}
        for how in ("frame", "query"):
            monkeypatch.setenv("SKR_ADAPTIVE_PATH", how)
            got[how] = r.render_adaptive_host(opt, threshold=0.05, min_passes=2, max_passes=6, want_float=True)
        monkeypatch.delenv("SKR_ADAPTIVE_PATH")
        assert np.array_equal(bits(got["frame"][1]), bits(got["query"][1])) and np.array_equal(got["frame"][2], got["query"][2])
        assert got["query"][2].min() == 2 and got["query"][2].max() > 2
        d_rgb, d_f, _ = r.render_denoised(opt, iterations=0, want_float=True)
        assert np.array_equal(bits(d_f), bits(frames[0])) and np.array_equal(d_rgb, pyoracle.quantise(frames[0]))
    finally:
        r.close()


# ---- 5. the refused combinations ----
def test_the_three_refused_combinations(gpu):
    path = scene_path("test.scn")
    cases = []
    cases.append((load(path), dict(legacy_reflect=True), "--legacy-reflect"))
    fog = skr.parse_scene(path, spot=True, fog=True)
    fog.set_fog(np.array([[0, 0, 5, 3, .5, .5, .5, .1, .05]], np.float32))
    cases.append((fog, dict(), "fog volumes"))
    cases.append((load(path, sphere_tree=True), dict(), "sphere tree"))
    for sc, kw, text in cases:
        r = skr.Renderer(sc)
        try:
            with pytest.raises(skr.SkrError) as e:
                r.render(skr.Options(32, 24, **kw))
            assert "(status 4)" in str(e.value) and "spot lights" in str(e.value) and text in str(e.value), str(e.value)
            rays = gpu.zeros((4, 8), dtype=gpu.float32, device="cuda:0")
            rays[:, 6] = 1
            with pytest.raises(skr.SkrError) as e:
                r.shade(rays, skr.Options(32, 24, **kw))
            assert "(status 4)" in str(e.value) and text in str(e.value), str(e.value)
        finally:
            r.close()


# ---- 6. no spot light, no change ----
@pytest.mark.parametrize("scn,kw", [("spheres2.scn", dict(shadow=True)), ("spheres2.scn", dict(gillum=3, depth=3, shadow=True, seed=4)),
                                    ("dragon.scn", dict(**ST))], ids=["direct", "nodes", "generic"])
def test_a_scene_without_spot_lights_renders_as_without_the_flag(gpu, scn, kw):
    a = gpu_frame(gpu, skr.parse_scene(scene_path(scn), spot=True), 96, 54, **kw)
    b = gpu_frame(gpu, skr.parse_scene(scene_path(scn)), 96, 54, **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
    assert a[3] == b[3] and "spot" not in a[3]


# ---- 7. both command lines ----
def test_both_command_lines_take_the_flag(gpu, checker, tmp_path):
    w, h = 160, 120
    path = scene_path("test.scn")
    args = ["--path", path, "--width", str(w), "--height", str(h), "--shadow", "--shade-triangles", "--scn-spot"]
    sc = load(path)
    want = checker.render(path, w, h, spots=sc.spot_lights, cones=sc.spot_cones, **ST)[0]
    off = checker.render(path, w, h, **ST)[0]
    assert (want != off).any()
    out1, out2 = str(tmp_path / "native.ppm"), str(tmp_path / "py.ppm")
    exe = os.path.join(ROOT, "bin", "raytracer")
    subprocess.run([exe, *args, "--output", out1, "--quiet"], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL, timeout=300)
    subprocess.run([sys.executable, "-m", "skele_raytracer_amd.render_cli", *args, "--output", out2], check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=300)
    for out in (out1, out2):
        assert np.array_equal(read_ppm_bytes(open(out, "rb").read()), want), out
