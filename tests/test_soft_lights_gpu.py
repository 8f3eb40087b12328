"""Lights with a radius on the MI355X (include/skr.h skr_scene_set_light_radii): whole frames and shading queries against the
CPU checker (tests/soft_light_checker.c) — bytes, float bits and the four work counters, no tolerance —, the sample through the debug
op, launch shapes, progressive frames, the refused combinations, what a scene without a radius leaves alone, both command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding
from conftest import ROOT, read_ppm_bytes, scene_path
from oracle import pyoracle
from soft_light_check import build as build_checker
from spot_check import MIXED_POINTS, MIXED_SPOTS, OCCLUDER, write_floor_scene
from test_scene_size_gpu import LIMIT, last_lights_within
from test_soft_lights_cpu import GRID, records, sample_rule

pytestmark = pytest.mark.gpu
f32 = np.float32
SAMPLE_OP = 18  # include/skr.h skr_debug_eval


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("softlightcheck_gpu")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load(path, radii, *, strict=False, triangle_shadows=False, **flags):
    sc = skr.parse_scene(path, spot=True, strict=strict, triangle_shadows=triangle_shadows, **flags)
    sc.set_light_radii(radii)
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


def same_as_checker(gpu, checker, path, radii, w, h, what, *, strict=False, triangle_shadows=False, **kw):
    sc = load(path, radii, strict=strict, triangle_shadows=triangle_shadows)
    rows, cones, rd = sc.spot_lights, sc.spot_cones, sc.light_radii
    assert (rd > 0).any(), what
    g_rgb, g_f, g_cnt, variant = gpu_frame(gpu, sc, w, h, **kw)
    c_rgb, c_f, c_st = checker.render(path, w, h, radii=rd, spots=rows, cones=cones, triangle_shadows=triangle_shadows, strict=strict, **kw)
    nb = int((bits(g_f) != bits(c_f)).sum())
    assert nb == 0, "%s: %d float words differ" % (what, nb)
    assert np.array_equal(g_rgb, c_rgb), what
    assert g_cnt == [int(x) for x in c_st[:4]], what
    in_force = triangle_shadows and kw.get("shade_triangles") and kw.get("shadow")
    assert variant == ("level_pipeline_g1_soft_tshadow" if in_force else "level_pipeline_g1_soft"), what
    return c_f, c_st


# ---- 1. GPU == checker, bit for bit ----
ST = dict(shade_triangles=True, shadow=True)
TEST_RADII = [0.4, 0.25]  # test.scn under --scn-spot: its point light, its spot light
TEST_SCN = [
    ("direct", 160, 120, False, dict()),
    ("shadow", 160, 120, False, dict(shadow=True)),
    ("shade_triangles_shadow", 160, 120, False, dict(**ST)),
    ("triangle_shadows", 160, 120, True, dict(**ST)),
    ("js2_shadow", 64, 48, False, dict(jsample=2, shadow=True, seed=3)),
    ("gi2_d2", 64, 48, False, dict(gillum=2, depth=2, seed=4)),
    ("gi2_d3", 64, 48, False, dict(gillum=2, depth=3, seed=5)),
    ("shade_triangles_gi2_d2", 64, 48, False, dict(gillum=2, depth=2, seed=6, **ST)),
]


@pytest.mark.parametrize("name,w,h,tshadow,kw", TEST_SCN, ids=[c[0] for c in TEST_SCN])
def test_test_scn_matches_the_checker_bit_for_bit(gpu, checker, name, w, h, tshadow, kw):
    on, _ = same_as_checker(gpu, checker, scene_path("test.scn"), TEST_RADII, w, h, name, triangle_shadows=tshadow, **kw)
    if name == "shadow":  # the radii do something
        sc = skr.parse_scene(scene_path("test.scn"), spot=True)
        off = checker.render(scene_path("test.scn"), w, h, spots=sc.spot_lights, cones=sc.spot_cones, **kw)[1]
        assert (bits(on) != bits(off)).any()


# three point lights and four spot lights: the pairs (soft, point), (soft, soft spot with a 5 / 20 cone: outside it for most of the floor),
# (point, point: a wide and a hard-edged spot light), and a single soft spot light as the tail of an odd count
FLOOR_POINTS = [MIXED_POINTS[0], (30, 30, 30, 3.0, 8.0, -2.0), (20, 40, 30, -1.0, 10.0, 5.0)]
FLOOR_SPOTS = [MIXED_SPOTS[1], MIXED_SPOTS[0], MIXED_SPOTS[2], (50, 50, 20, 2.0, 9.0, -1.0, -0.1, -1.0, 0.1, 10, 35)]
FLOOR_RADII = [0.5, 0.0, 0.3, 0.4, 0.0, 0.0, 0.6]


def test_the_floor_scene_matches_the_checker(gpu, checker, tmp_path):
    scn = write_floor_scene(str(tmp_path / "floor.scn"), points=FLOOR_POINTS, spots=FLOOR_SPOTS, tris=[OCCLUDER])
    for tshadow in (False, True):
        _, st = same_as_checker(gpu, checker, scn, FLOOR_RADII, 96, 72, "floor tshadow=%s" % tshadow, triangle_shadows=tshadow, **ST)
        assert int(st[1]) * 4 < int(st[2]) < int(st[1]) * 7  # the soft 5 / 20 spot light is outside its cone somewhere, inside elsewhere
    same_as_checker(gpu, checker, scn, FLOOR_RADII, 64, 48, "floor gi", triangle_shadows=True, gillum=3, depth=3, seed=8, **ST)
    # --strict-scn: a directional light behind the others (it pairs with the soft tail)
    strict = write_floor_scene(str(tmp_path / "strict.scn"), points=FLOOR_POINTS, spots=FLOOR_SPOTS, tris=[OCCLUDER], directional=True)
    for tshadow in (False, True):
        same_as_checker(gpu, checker, strict, FLOOR_RADII, 96, 72, "strict tshadow=%s" % tshadow, strict=True, triangle_shadows=tshadow, **ST)


@pytest.mark.parametrize("points,spots,radii", [(1, 0, [0.5]), (0, 1, [0.5]), (2, 0, [0.5, 0.0]), (1, 1, [0.0, 0.7])],
                         ids=["one_point", "one_spot", "soft_and_point", "point_and_soft_spot"])
def test_small_light_counts(gpu, checker, tmp_path, points, spots, radii):
    scn = write_floor_scene(str(tmp_path / "few.scn"), points=FLOOR_POINTS[:points], spots=FLOOR_SPOTS[3:3 + spots])
    same_as_checker(gpu, checker, scn, radii, 96, 72, "%d+%d" % (points, spots), shadow=True)
    same_as_checker(gpu, checker, scn, radii, 48, 36, "%d+%d gi" % (points, spots), gillum=2, depth=2, shadow=True, seed=2)


def test_the_largest_light_count_every_other_light_soft(gpu, checker, tmp_path):
    """the floor sphere under as many lights as the general pipeline's LDS holds, half of them spot lights, every other light with a radius"""
    n = last_lights_within("prefix", LIMIT, 1)
    rng = np.random.default_rng(5)
    pos = np.c_[rng.uniform(-8, 8, n), rng.uniform(4, 12, n), rng.uniform(-4, 10, n)]
    col = rng.uniform(0.02, 0.08, (n, 3))
    pts = [(*col[i], *pos[i]) for i in range(0, n // 2)]
    sps = []
    for i in range(n // 2, n):
        a1 = rng.uniform(3, 30)
        sps.append((*(col[i] * 40), *pos[i], rng.normal(0, 0.3), -1.0, rng.normal(0, 0.3), a1, a1 + rng.uniform(0, 25)))
    scn = write_floor_scene(str(tmp_path / "many.scn"), points=pts, spots=sps)
    radii = np.where(np.arange(n) % 2 == 0, rng.uniform(0.1, 1.0, n), 0.0).astype(np.float32)
    sc = load(scn, radii)
    assert sc.info.n_point_lights + len(sc.spot_lights) == n == len(sc.light_radii) and n > 5000
    same_as_checker(gpu, checker, scn, radii, 32, 24, "%d lights" % n, shadow=True)


# ---- 2. the sample through the debug op ----
def test_the_sample_through_the_debug_op(gpu, checker):
    recs = [records(Lp=(3.0, 9.5, -2.25), R=0.5, **GRID), records(Lp=(-1e3, 4e-3, 77.0), R=12.75, **GRID), records(Lp=(0.0, -0.0, 5.0), R=0.0, **GRID)]
    # u1 = 1 (z = -1) and u1 < 2^-26 (z = +1): found by a search over the pixel word; and l at the top of its range
    edge = records([16343396, 29818698], [1], [7], [3], [5], (1.0, 2.0, 3.0), 2.0)
    top = records([0, 5], [0, 3], [0, 9], [2 ** 22 - 1, 2 ** 22 - 2], [1, 2 ** 63 + 9], (1.0, 2.0, 3.0), 0.75)
    rec = np.concatenate(recs + [edge, top])
    _, u1, _ = sample_rule(edge)
    assert (f32(1) - f32(2) * u1).tolist() == [-1.0, 1.0]
    want = checker.samples(rec)
    got = binding.debug_eval(SAMPLE_OP, rec, 3)
    assert np.array_equal(got, bits(want))
    k = len(rec) - len(top) - len(edge)
    assert np.array_equal(got[k:k + 2], bits(np.array([[1.0, 0.0, 3.0], [1.0, 4.0, 3.0]], np.float32)))  # z = -1, +1: s = 0, the poles
    z0 = sum(len(r) for r in recs[:2])
    assert np.array_equal(got[z0:k], np.broadcast_to(bits(np.array([0.0, -0.0, 5.0], np.float32)), (k - z0, 3)))  # R == 0: Lp, bit for bit


# ---- 3. shading queries ----
@pytest.mark.parametrize("name,tshadow,kw", [("shade_triangles", True, dict(**ST)), ("gi2_d3", False, dict(gillum=2, depth=3, shadow=True, seed=5))])
def test_camera_rays_give_the_frame(gpu, checker, name, tshadow, kw):
    torch = gpu
    path, w, h = scene_path("test.scn"), 64, 48
    sc = load(path, TEST_RADII, triangle_shadows=tshadow)
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, **kw)
        frame = r.render(opt, want_float=True)[1]
        rays = r.camera_rays(opt).view(-1, 8)
        keys = torch.arange(w * h, dtype=torch.int32, device=rays.device)
        r.counters(reset=True)
        got = r.shade(rays, opt, keys=keys)
        torch.cuda.synchronize()
        assert skr.Renderer.kernel_variant() == ("shade_rays_g1_soft_tshadow" if tshadow else "shade_rays_g1_soft")
        assert np.array_equal(bits(got.cpu().numpy()), bits(frame.cpu().numpy()).reshape(-1, 3))
        c = r.counters()
        want, st = checker.shade(path, rays.cpu().numpy(), radii=TEST_RADII, spots=sc.spot_lights, cones=sc.spot_cones, triangle_shadows=tshadow, keys=np.arange(w * h), **kw)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        assert [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]] == [int(x) for x in st]
    finally:
        r.close()


def test_arbitrary_rays_with_caller_keys_match_the_checker(gpu, checker, tmp_path):
    torch = gpu
    scn = write_floor_scene(str(tmp_path / "floor.scn"), points=FLOOR_POINTS, spots=FLOOR_SPOTS, tris=[OCCLUDER])
    sc = load(scn, FLOOR_RADII, triangle_shadows=True)
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
    keys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)  # the counter RNG's pixel word: any 32 bits
    r = skr.Renderer(sc)
    try:
        r.counters(reset=True)
        got = r.shade(torch.from_numpy(rays).to("cuda:0"), skr.Options(8, 8, **kw), sample=3, keys=torch.from_numpy(keys.view(np.int32)).to("cuda:0"))
        torch.cuda.synchronize()
        c = r.counters()
        want, st = checker.shade(scn, rays, radii=FLOOR_RADII, spots=sc.spot_lights, cones=sc.spot_cones, triangle_shadows=True, sample=3, keys=keys, **kw)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        assert [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]] == [int(x) for x in st]
        assert int(st[1]) > n // 2
        other, _ = checker.shade(scn, rays, radii=FLOOR_RADII, spots=sc.spot_lights, cones=sc.spot_cones, triangle_shadows=True, sample=3, **kw)
        assert (bits(other) != bits(want)).any()  # the keys reach the draw
    finally:
        r.close()


# ---- 4. launch shapes and the modes above a frame ----
def test_tiles_strides_a_clone_and_a_one_device_multi_give_the_frame(gpu, checker):
    path, w, h = scene_path("test.scn"), 96, 72
    kw = dict(gillum=2, depth=2, seed=5, **ST)
    sc = load(path, TEST_RADII, triangle_shadows=True)
    want = checker.render(path, w, h, radii=TEST_RADII, spots=sc.spot_lights, cones=sc.spot_cones, triangle_shadows=True, **kw)
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
    kw = dict(**ST)  # (no GI: the two frames differ through the light samples alone)
    sc = load(path, TEST_RADII)
    frames = [checker.render(path, w, h, radii=TEST_RADII, spots=sc.spot_lights, cones=sc.spot_cones, seed=11 + k, **kw)[1] for k in range(2)]
    assert (bits(frames[0]) != bits(frames[1])).any()
    mean = (frames[0] + frames[1]) / f32(2)
    r = skr.Renderer(sc)
    try:
        rgb, rgbf = r.render(skr.Options(w, h, seed=11, progressive=2, **kw), want_float=True)
        gpu.cuda.synchronize()
        assert np.array_equal(bits(rgbf.cpu().numpy()), bits(mean))
        assert np.array_equal(rgb.cpu().numpy(), pyoracle.quantise(mean))
        # adaptive and denoised frames sit above the same frame: min == max == 2 passes are the mean, zero iterations hand it through
        opt = skr.Options(w, h, seed=11, **kw)
        a_rgb, a_f, passes, _ = r.render_adaptive_host(opt, threshold=-1.0, min_passes=2, max_passes=2, want_float=True)
        assert (passes == 2).all() and np.array_equal(bits(a_f), bits(mean)) and np.array_equal(a_rgb, pyoracle.quantise(mean))
        d_rgb, d_f, _ = r.render_denoised(opt, iterations=0, want_float=True)
        assert np.array_equal(bits(d_f), bits(frames[0])) and np.array_equal(d_rgb, pyoracle.quantise(frames[0]))
    finally:
        r.close()


# ---- 5. the refused combinations ----
def test_the_three_refused_combinations(gpu):
    path = scene_path("spheres2.scn")

    def soft(**flags):
        sc = skr.parse_scene(path, **flags)
        sc.set_light_radii(0.5)
        return sc

    cases = [(soft(), dict(legacy_reflect=True), "--legacy-reflect")]
    fog = soft(fog=True)
    fog.set_fog(np.array([[0, 0, 5, 3, .5, .5, .5, .1, .05]], np.float32))
    cases.append((fog, dict(), "fog volumes"))
    cases.append((soft(sphere_tree=True), dict(), "sphere tree"))
    for sc, kw, text in cases:
        r = skr.Renderer(sc)
        try:
            with pytest.raises(skr.SkrError) as e:
                r.render(skr.Options(32, 24, **kw))
            assert "(status 4)" in str(e.value) and "light radii" in str(e.value) and text in str(e.value), str(e.value)
            rays = gpu.zeros((4, 8), dtype=gpu.float32, device="cuda:0")
            rays[:, 6] = 1
            with pytest.raises(skr.SkrError) as e:
                r.shade(rays, skr.Options(32, 24, **kw))
            assert "(status 4)" in str(e.value) and "light radii" in str(e.value) and text in str(e.value), str(e.value)
        finally:
            r.close()


# ---- 6. no radius, no change ----
@pytest.mark.parametrize("scn", ["spheres2.scn", "test.scn"])
@pytest.mark.parametrize("kw", [dict(shadow=True), dict(gillum=3, depth=3, shadow=True, seed=4)], ids=["direct", "gillum"])
def test_a_scene_whose_radii_are_all_zero_renders_as_before(gpu, scn, kw):
    w, h = 96, 54
    zero = skr.parse_scene(scene_path(scn))
    zero.set_light_radii(0.5)
    zero.set_light_radii(0.0)  # (set and taken back)
    a = gpu_frame(gpu, zero, w, h, **kw)
    b = gpu_frame(gpu, skr.parse_scene(scene_path(scn)), w, h, **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
    assert a[3] == b[3] and "soft" not in a[3] and "spot" not in a[3]
    # and both are the frozen oracle's frame, the one every earlier build renders
    o_rgb, o_f, o_st = pyoracle.render(scene_path(scn), w, h, want_float=True, **kw)
    assert np.array_equal(bits(a[1]), bits(o_f)) and np.array_equal(a[0], o_rgb) and a[2] == [int(x) for x in o_st[:4]]


# ---- 7. both command lines ----
def test_both_command_lines_take_the_flag(gpu, checker, tmp_path):
    w, h = 160, 120
    path = scene_path("test.scn")
    args = ["--path", path, "--width", str(w), "--height", str(h), "--shadow", "--shade-triangles", "--scn-spot", "--light-radius", "0.4", "--seed", "3"]
    sc = skr.parse_scene(path, spot=True)
    want = checker.render(path, w, h, radii=0.4, spots=sc.spot_lights, cones=sc.spot_cones, seed=3, **ST)[0]
    off = checker.render(path, w, h, spots=sc.spot_lights, cones=sc.spot_cones, seed=3, **ST)[0]
    assert (want != off).any()
    out1, out2 = str(tmp_path / "native.ppm"), str(tmp_path / "py.ppm")
    exe = os.path.join(ROOT, "bin", "raytracer")
    subprocess.run([exe, *args, "--output", out1, "--quiet"], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL, timeout=300)
    subprocess.run([sys.executable, "-m", "skele_raytracer_amd.render_cli", *args, "--output", out2], check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=300)
    for out in (out1, out2):
        assert np.array_equal(read_ppm_bytes(open(out, "rb").read()), want), out
    # a bad value is answered as the other added flags answer one: a message, status 2, no image
    bad = subprocess.run([exe, *args[:-4], "--light-radius", "-1", "--output", str(tmp_path / "bad.ppm"), "--quiet"], cwd=str(tmp_path), capture_output=True, timeout=300)
    assert bad.returncode == 2 and b"--light-radius" in bad.stderr and not os.path.exists(str(tmp_path / "bad.ppm"))
