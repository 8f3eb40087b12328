"""Ray queries on the MI355X (include/skr.h skr_trace_rays, skr_camera_rays; DESIGN.md "Ray queries"): every result bit for bit
against the CPU checker (tests/ray_query_checker.c), the any-hit answer against the closest hit, the camera rays against the
oracle's primary directions, and a query leaving every render and counter as it was."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import skele_raytracer_amd as skr
from conftest import scene_path
from ray_query_check import build as build_checker, pack_rays

pytestmark = pytest.mark.gpu

N_RAYS = (1 << 16) - 13  # not a multiple of 64: the last wave is partial


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("raycheck_gpu")))


def random_rays(scene, n, seed):
    """Seeded rays that mix what callers send: origins across the scene, at the camera and ON triangles (with ignore_triangle set
    to that triangle), unnormalised directions, aimed at surfaces or not, a quarter with a finite tmax."""
    rng = np.random.default_rng(seed)
    s, t, _ = scene.arrays()
    cam = np.array(list(scene.info.camera)[:3], np.float32)
    pts = [cam[None, :]]
    if len(s):
        pts.append(s[:, :3])
    if len(t):
        pts.append(t.reshape(-1, 3))
    pts = np.concatenate(pts).astype(np.float64)
    lo, hi = pts.min(0), pts.max(0)
    span = float(np.max(hi - lo)) or 1.0
    o = rng.uniform(lo - 0.1 * span, hi + 0.1 * span, (n, 3))
    o[: n // 8] = cam  # from the camera
    ignore = np.full(n, -1, np.int32)
    if len(t):  # from a point of a triangle's accept region (v0, v0 - e1, v0 + e2), leaving it
        k = np.arange(n // 8, n // 4)
        which = rng.integers(0, len(t), len(k))
        v = t[which].reshape(-1, 3, 3).astype(np.float64)
        a, b = rng.uniform(0, 0.5, len(k)), rng.uniform(0, 0.5, len(k))
        o[k] = v[:, 0] - a[:, None] * (v[:, 1] - v[:, 0]) + b[:, None] * (v[:, 2] - v[:, 0])
        ignore[k] = which
    targets = pts[rng.integers(0, len(pts), n)] + rng.normal(scale=0.02 * span, size=(n, 3))
    d = np.where(rng.random((n, 1)) < 0.7, targets - o, rng.normal(size=(n, 3)))
    d *= rng.choice([0.25, 1.0, 3.0], n)[:, None] / np.maximum(np.linalg.norm(d, axis=1), 1e-6)[:, None]
    tmax = np.where(rng.random(n) < 0.25, rng.uniform(0.0, 4.0, n), np.inf)
    return pack_rays(o, d, tmax, ignore)


def gpu_trace(r, rays, any_hit=False):
    out = r.trace(torch.from_numpy(np.ascontiguousarray(rays)).cuda(), any_hit=any_hit)
    torch.cuda.synchronize()
    return (out if any_hit else out.raw).cpu().numpy()


def assert_bitwise(gpu, cpu, what):
    g, c = gpu.view(np.uint32), cpu.view(np.uint32)
    bad = np.nonzero((g != c).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d rays differ; first %d: gpu %s cpu %s" % (what, len(bad), len(g), bad[0], gpu[bad[0]], cpu[bad[0]])


def arrays_scene(spheres, triangles):
    return skr.Scene.from_arrays(spheres, triangles, np.zeros((0, 6), np.float32), [0, 0, -10, 0, 0, 1, 0, 1, 0])


def random_arrays(seed, ns, nt):
    rng = np.random.default_rng(seed)
    s = np.zeros((ns, 14), np.float32)
    s[:, :3] = rng.uniform(-4, 4, (ns, 3))
    s[:, 3] = rng.uniform(0.2, 1.2, ns)
    c = rng.uniform(-4, 4, (nt, 1, 3))
    t = (c + rng.normal(scale=0.6, size=(nt, 3, 3))).reshape(nt, 9).astype(np.float32)
    return s, t


SCENES = {
    "spheres2": lambda: skr.parse_scene(scene_path("spheres2.scn")),
    "bear": lambda: skr.parse_scene(scene_path("bear.scn")),
    "dragon": lambda: skr.parse_scene(scene_path("dragon.scn")),
    "test": lambda: skr.parse_scene(scene_path("test.scn")),
    "arrays_no_spheres": lambda: arrays_scene(*random_arrays(5, 0, 300)),
    "arrays_no_triangles": lambda: arrays_scene(*random_arrays(6, 40, 0)),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_closest_and_any_hit_match_the_checker(checker, name):
    sc = SCENES[name]()
    r = skr.Renderer(sc, 0)
    rays = random_rays(sc, N_RAYS, seed=sum(name.encode()))
    s, t, _ = sc.arrays()
    want, occ_want = checker.trace(s, t, rays)
    got = gpu_trace(r, rays)
    assert_bitwise(got, want, name)
    kind = got[:, 1].view(np.int32)
    assert (kind == 0).any() and (kind != 0).any(), "the rays must both hit and miss"
    if len(s):
        assert (kind == 1).any()
    if len(t):
        assert (kind == 2).any()
    occ = gpu_trace(r, rays, any_hit=True)
    assert np.array_equal(occ, (kind != 0).astype(np.int32))
    assert np.array_equal(occ, occ_want)


@pytest.mark.parametrize("name", ["spheres2", "test", "dragon", "arrays_no_spheres"])
def test_any_hit_at_the_hit_distance(checker, name):
    """tmax at exactly t, one ulp either side of it, and a few ulps out: any-hit agrees with closest hit on every one (a sphere's
    bracket straddles tmax there, so these take the exact root)."""
    sc = SCENES[name]()
    r = skr.Renderer(sc, 0)
    base = random_rays(sc, 1 << 14, seed=11)
    s, t, _ = sc.arrays()
    hits, _ = checker.trace(s, t, base)
    th = hits[:, 0]
    keep = np.isfinite(th)
    base, th = base[keep], th[keep]
    variants = [th, np.nextafter(th, np.float32(np.inf)), np.nextafter(th, np.float32(-np.inf)), th * np.float32(1 + 3e-7), th * np.float32(1 - 3e-7)]
    rays = np.concatenate([base.copy() for _ in variants])
    rays[:, 3] = np.concatenate(variants)
    got = gpu_trace(r, rays)
    want, occ_want = checker.trace(s, t, rays)
    assert_bitwise(got, want, name + " tmax at t")
    kind = got[:, 1].view(np.int32)
    assert not kind[: len(base)].any(), "tmax == t must be a miss"
    assert kind[len(base): 2 * len(base)].all(), "tmax just past t must be a hit"
    occ = gpu_trace(r, rays, any_hit=True)
    assert np.array_equal(occ, (kind != 0).astype(np.int32))
    assert np.array_equal(occ, occ_want)


def test_dragon_culled_walk_matches_brute_force(checker):
    """The trace tree (rays from inside its ball) against the same rays with culling off (SKR_NO_CULL: every triangle), and both
    against the checker: camera rays and rays from points of the mesh."""
    sc = SCENES["dragon"]()
    rays = np.concatenate([random_rays(sc, 1 << 15, seed=21), np.zeros((0, 8), np.float32)])
    r = skr.Renderer(sc, 0)
    cam = r.camera_rays(skr.Options(320, 180)).reshape(-1, 8).cpu().numpy()
    rays = np.concatenate([rays, cam])
    culled = gpu_trace(r, rays)
    os.environ["SKR_NO_CULL"] = "1"
    try:
        brute = gpu_trace(skr.Renderer(sc, 0), rays)
    finally:
        del os.environ["SKR_NO_CULL"]
    assert_bitwise(culled, brute, "dragon culled vs every triangle")
    s, t, _ = sc.arrays()
    assert_bitwise(culled, checker.trace(s, t, rays)[0], "dragon vs checker")
    assert (culled[:, 1].view(np.int32) == 2).mean() > 0.05


@pytest.mark.parametrize("jsample,sample", [(0, 0), (3, 0), (3, 5)])
@pytest.mark.parametrize("name", ["spheres2.scn", "dragon.scn"])
def test_camera_rays_are_the_primary_rays(checker, name, jsample, sample):
    sc = skr.parse_scene(scene_path(name))
    r = skr.Renderer(sc, 0)
    opt = skr.Options(320, 180, jsample=jsample, seed=9)
    got = r.camera_rays(opt, sample)
    torch.cuda.synchronize()
    want = checker.camera_rays(scene_path(name), 320, 180, jsample=jsample, seed=9, sample=sample)
    assert got.shape == (180, 320, 8)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_camera_ray_miss_mask_on_spheres2():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    r = skr.Renderer(sc, 0)
    opt = skr.Options(320, 180)
    hits = r.trace(r.camera_rays(opt).view(-1, 8))
    miss = (hits.kind == 0).view(180, 320).cpu().numpy()
    assert miss.shape == (180, 320) and miss.any() and not miss.all()
    # the frame's own background pixels are the misses (spheres2: no triangles, so a hit pixel is shaded)
    rgb, rgbf = r.render(opt, want_float=True)
    bg = np.array(list(sc.info.background), np.float32)
    is_bg = (rgbf.cpu().numpy() == bg).all(axis=2)
    assert np.array_equal(miss, miss & is_bg)


def test_a_query_changes_nothing_a_render_reads():
    sc = skr.parse_scene(scene_path("test.scn"))
    r = skr.Renderer(sc, 0)
    opt = skr.Options(160, 90, gillum=2, depth=2, shade_triangles=True)
    r.count_triangle_work(True)
    r.kernel_timing(True)
    r.work(reset=True)
    r.triangle_work(reset=True)
    rgb1, f1 = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    variant = skr.Renderer.kernel_variant()
    tw1, w1 = r.triangle_work(reset=False), r.work(reset=False)
    rays = torch.from_numpy(random_rays(sc, 5000, seed=4)).cuda()
    r.trace(rays)
    r.trace(rays, any_hit=True)
    r.trace(r.camera_rays(opt).view(-1, 8))
    torch.cuda.synchronize()
    assert skr.Renderer.kernel_variant() == variant
    assert r.triangle_work(reset=False) == tw1 and r.work(reset=False) == w1
    assert r.kernel_ms()[1] == 1  # the render's one timed kernel; the queries are not timed
    r.work(reset=True)
    r.triangle_work(reset=True)
    rgb2, f2 = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    assert torch.equal(rgb1, rgb2) and torch.equal(f1, f2)
    # (the culling-sphere tests of a --gillum level depend on how its rays fall into waves, which the level's atomics decide: not
    # compared across renders)
    assert r.work(reset=False) == w1


def test_argument_errors_and_empty_calls():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    r = skr.Renderer(sc, 0)
    L = skr.lib()
    rays = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    out = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    p, q = rays.data_ptr(), out.data_ptr()
    assert L.skr_trace_rays(r.h, None, 4, 0, q, None) == 2
    assert L.skr_trace_rays(r.h, p, 4, 0, None, None) == 2
    assert L.skr_trace_rays(None, p, 4, 0, q, None) == 2
    assert L.skr_trace_rays(r.h, p, 4, 2, q, None) == 2  # unknown flag
    assert L.skr_trace_rays(r.h, p + 4, 3, 0, q, None) == 2  # misaligned
    sentinel = torch.full((4, 8), 7.0, device="cuda")
    assert L.skr_trace_rays(r.h, p, 0, 0, sentinel.data_ptr(), None) == 0  # n == 0: nothing launched
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())
    opt = skr.Options(32, 16)
    assert L.skr_camera_rays(r.h, C.byref(opt.c), 1, p, None) == 2  # sample 1 without --jsample
    assert L.skr_camera_rays(r.h, None, 0, p, None) == 2
    assert L.skr_camera_rays(r.h, C.byref(skr.Options(32, 16, jsample=2).c), 4, p, None) == 2
    assert r.trace(torch.zeros((0, 8), dtype=torch.float32, device="cuda")).raw.shape == (0, 8)


@pytest.mark.parametrize("name", ["spheres2", "dragon", "test"])
def test_bad_rays_do_not_disturb_good_ones(checker, name):
    sc = SCENES[name]()
    r = skr.Renderer(sc, 0)
    rays = random_rays(sc, 4096, seed=31)
    bad = np.arange(5, 4096, 97)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    junk = [(nan, 0, 0, 1), (0, 0, 0, 0), (inf, 1, 0, 0), (0, nan, 1, 1), (0, 0, -inf, 1)]
    for j, i in enumerate(bad):
        o0, d0, d1, d2 = junk[j % len(junk)]
        rays[i, 0] = o0 if j % 2 else rays[i, 0]
        rays[i, 4:7] = (d0, d1, d2) if not (j % 2) else (0, 0, 0)
        if j % 3 == 0:
            rays[i, 3] = nan
    s, t, _ = sc.arrays()
    want, occ_want = checker.trace(s, t, rays)
    got = gpu_trace(r, rays)
    occ = gpu_trace(r, rays, any_hit=True)
    good = np.setdiff1d(np.arange(len(rays)), bad)
    assert_bitwise(got[good], want[good], name + " good rays beside bad ones")
    assert np.array_equal(occ[good], occ_want[good])
