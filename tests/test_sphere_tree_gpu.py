"""The sphere tree on the device (pytest -m gpu; include/skr.h skr_scene_set_sphere_tree): with the switch on every
frame and shading query is the oracle's (or the switch-off renderer's, where only a checker the existing tests already hold it to knows
the mode) bit for bit — bytes, floats and all four work counts —, at sphere counts the LDS path refuses, with SKR_NO_SPHERE_CULL=1 as the
second arm of every frame."""
import numpy as np
import pytest
import torch

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding
from adaptive_check import adaptive
from conftest import scene_path
from denoise_check import denoise_numpy
from ray_query_check import build as build_ray_checker
from shade_query_check import build as build_shade_checker
from sphere_tree_cases import RANDOM_KINDS, random_scene, write_case_scene
from test_adaptive_gpu import assert_same, run_adaptive
from test_gpu_parity import compare
from test_scene_size_gpu import MAX_N, assert_refused, check_ray_queries, write_scene

pytestmark = pytest.mark.gpu
W, H = 96, 54
SEED = 17


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def ray_checker(tmp_path_factory):
    return build_ray_checker(str(tmp_path_factory.mktemp("stree_raycheck")))


@pytest.fixture(scope="module")
def ts_checker(tmp_path_factory):
    from triangle_shadow_check import build
    return build(str(tmp_path_factory.mktemp("stree_ts")))


@pytest.fixture(scope="module")
def fog_checker(tmp_path_factory):
    from fog_check import build
    return build(str(tmp_path_factory.mktemp("stree_fog")))


@pytest.fixture(scope="module")
def shade_checker(tmp_path_factory):
    return build_shade_checker(str(tmp_path_factory.mktemp("stree_shadecheck")))


def frame(r, opt, monkeypatch=None, no_cull=False, **render_kw):
    """(bytes, floats, the four work counts, variant) of one frame"""
    if monkeypatch:
        if no_cull:
            monkeypatch.setenv("SKR_NO_SPHERE_CULL", "1")
        else:
            monkeypatch.delenv("SKR_NO_SPHERE_CULL", raising=False)
    r.work(reset=True)
    rgb, rgbf = r.render(opt, want_float=True, **render_kw)
    torch.cuda.synchronize()
    c = r.work(reset=True)
    return rgb.cpu().numpy(), rgbf.cpu().numpy(), (c["radiance_rays"], c["sphere_hits"], c["shadow_rays"], c["sphere_tests"]), r.kernel_variant()


def oracle_frame(oracle, path, w, h, kw, strict=False):
    extra = dict(strict=True) if strict else {}
    o_rgb, o_f, st = oracle.render(path, w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **extra, **kw)
    return o_rgb, o_f, tuple(int(v) for v in st[:4])


def same(a, b, what):
    assert np.array_equal(a[0], b[0]), "%s: u8 image differs" % what
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "%s: float image differs (%d words)" % (what, int((a[1].view(np.uint32) != b[1].view(np.uint32)).sum()))
    assert a[2] == b[2], "%s: work counts %s != %s" % (what, a[2], b[2])


def both_arms(r, opt, monkeypatch, ref, what, variant):
    got = frame(r, opt, monkeypatch)
    assert got[3] == variant, (what, got[3])
    same(got, ref, what + " [tree]")
    loop = frame(r, opt, monkeypatch, no_cull=True)
    assert loop[3] == variant
    same(loop, got, what + " [SKR_NO_SPHERE_CULL=1]")
    monkeypatch.delenv("SKR_NO_SPHERE_CULL", raising=False)
    return got


# every mode the general level pipeline has; (options, parse flags, the reference: the oracle or the triangle-shadow checker)
SMALL_MODES = {
    "direct": (dict(depth=1), {}, "oracle"),
    "shadow": (dict(shadow=True), {}, "oracle"),
    "jsample2_shadow": (dict(jsample=2, shadow=True, seed=SEED), {}, "oracle"),
    "gillum3_d2": (dict(gillum=3, depth=2, shadow=True, seed=SEED), {}, "oracle"),
    "gillum2_d4": (dict(gillum=2, depth=4, shadow=True, seed=SEED), {}, "oracle"),
    "strict_scn": (dict(gillum=2, depth=2, shadow=True, seed=SEED), dict(strict=True), "oracle"),
    "shade_triangles_tshadow": (dict(gillum=2, depth=3, shadow=True, shade_triangles=True, seed=SEED), dict(triangle_shadows=True), "ts_checker"),
    "legacy_reflect": (dict(depth=3, shadow=True, legacy_reflect=True), {}, "oracle"),
    "legacy_reflect_gillum": (dict(gillum=2, depth=3, shadow=True, legacy_reflect=True, seed=SEED), {}, "oracle"),
}


@pytest.mark.parametrize("mode", sorted(SMALL_MODES))
@pytest.mark.parametrize("scn", ["spheres1.scn", "spheres2.scn", "test.scn", "bear.scn"])
def test_small_scenes_every_mode(gpu, oracle, ts_checker, monkeypatch, scn, mode):
    kw, flags, ref_kind = SMALL_MODES[mode]
    w, h = (64, 36) if scn == "test.scn" else (W, H)
    sc = skr.parse_scene(scene_path(scn), sphere_tree=True, **flags)
    assert sc.info.n_spheres > 0
    r = skr.Renderer(sc)
    opt = skr.Options(w, h, **kw)
    in_force = bool(flags.get("triangle_shadows")) and sc.info.n_triangles > 0
    variant = "level_pipeline_g1_stree_tshadow" if in_force else "level_pipeline_g1_stree"
    if ref_kind == "oracle":
        ref = oracle_frame(oracle, scene_path(scn), w, h, kw, strict=bool(flags.get("strict")))
    else:
        c_rgb, c_f, st = ts_checker.render(scene_path(scn), w, h, triangle_shadows=True, **kw)
        ref = (c_rgb, c_f, tuple(int(v) for v in st[:4]))
    both_arms(r, opt, monkeypatch, ref, "%s %s" % (scn, mode), variant)
    r.close()


def test_fog_on_the_tree(gpu, fog_checker, tmp_path, monkeypatch):
    """against the fog checker (images and the three counts it keeps), and against the switch-off renderer for the fourth count"""
    path = write_scene(tmp_path / "fog.scn", 71, triangles=0, fog=True)
    kw = dict(gillum=2, depth=2, shadow=True, seed=SEED)
    sc = skr.parse_scene(path, fog=True, sphere_tree=True)
    c_rgb, c_f, st = fog_checker.render(path, W, H, sc.fog, **kw)
    off = skr.Renderer(skr.parse_scene(path, fog=True))
    ref = frame(off, skr.Options(W, H, **kw), monkeypatch)
    compare(ref[0], ref[1], c_rgb, c_f, "fog, switch off")
    r = skr.Renderer(sc)
    got = both_arms(r, skr.Options(W, H, **kw), monkeypatch, ref, "fog", "level_pipeline_g1_stree")
    compare(got[0], got[1], c_rgb, c_f, "fog, tree")
    assert got[2][:3] == tuple(int(v) for v in st[:3])


LARGE_MODES = {
    "direct": dict(depth=1),
    "shadow": dict(shadow=True),
    "jsample2_shadow": dict(jsample=2, shadow=True, seed=SEED),
    "gillum4_d3_shadow": dict(gillum=4, depth=3, shadow=True, seed=SEED),
}


@pytest.fixture(scope="module")
def large(tmp_path_factory):
    """n -> (path, renderer with the switch on), built once"""
    d = tmp_path_factory.mktemp("stree_large")
    cache = {}

    def get(n, triangles=0):
        if (n, triangles) not in cache:
            p = write_scene(d / ("n%d_t%d.scn" % (n, triangles)), n, triangles=triangles)
            cache[(n, triangles)] = (p, skr.Renderer(skr.parse_scene(p, sphere_tree=True, triangle_shadows=triangles > 0)))
        return cache[(n, triangles)]

    yield get
    for _, r in cache.values():
        r.close()


@pytest.mark.parametrize("mode", sorted(LARGE_MODES))
@pytest.mark.parametrize("n", [MAX_N + 1, 4000, 20000])
def test_large_scenes(gpu, oracle, large, monkeypatch, n, mode):
    path, r = large(n)
    kw = LARGE_MODES[mode]
    both_arms(r, skr.Options(W, H, **kw), monkeypatch, oracle_frame(oracle, path, W, H, kw), "n=%d %s" % (n, mode), "level_pipeline_g1_stree")


@pytest.mark.parametrize("n", [MAX_N + 1, 4000, 20000])
def test_large_scenes_with_triangle_surfaces_and_triangle_shadows(gpu, large, ts_checker, monkeypatch, n):
    """a few triangles in front of the grid, --shade-triangles with triangle shadows in force, against the triangle-shadow checker"""
    checker = ts_checker
    path, r = large(n, triangles=6)
    kw = dict(gillum=2, depth=3, shadow=True, shade_triangles=True, seed=SEED)
    c_rgb, c_f, st = checker.render(path, W, H, triangle_shadows=True, **kw)
    both_arms(r, skr.Options(W, H, **kw), monkeypatch, (c_rgb, c_f, tuple(int(v) for v in st[:4])), "n=%d triangle shadows" % n, "level_pipeline_g1_stree_tshadow")


def test_the_switch_off_still_refuses_the_same_scenes(gpu, tmp_path):
    for n in (MAX_N + 1, 4000):
        r = skr.Renderer(skr.parse_scene(write_scene(tmp_path / "off.scn", n)))
        assert_refused(lambda: r.render(skr.Options(W, H, shadow=True)), "switch off, n=%d" % n)
        assert_refused(lambda: r.shade(r.camera_rays(skr.Options(W, H)).view(-1, 8), skr.Options(W, H, gillum=2, depth=2)), "switch off, shading query n=%d" % n)
        r.close()


@pytest.mark.parametrize("kind", RANDOM_KINDS)
def test_random_scenes(gpu, oracle, tmp_path, monkeypatch, kind):
    """overlapping, nested, coincident spheres (the lower file index wins: every sphere has its own material), radii over 6 decades, the
    camera inside a sphere, no sphere, one sphere"""
    path = write_case_scene(tmp_path / "case.scn", random_scene(kind))
    sc = skr.parse_scene(path, sphere_tree=True)
    r = skr.Renderer(sc)
    for kw in (dict(shadow=True), dict(gillum=3, depth=3, shadow=True, seed=SEED)):
        ref = oracle_frame(oracle, path, W, H, kw)
        if kind == "zero":  # no sphere: the switch does not apply
            got = frame(r, skr.Options(W, H, **kw), monkeypatch)
            assert "stree" not in got[3]
            same(got, ref, "zero spheres")
        else:
            both_arms(r, skr.Options(W, H, **kw), monkeypatch, ref, "%s %s" % (kind, kw), "level_pipeline_g1_stree")
    r.close()


def query_rays(sc, tree, n, seed, where):
    """rays with origins inside the tree's ball, outside it, or inside with one non-finite direction in every wave of 64"""
    rng = np.random.default_rng(seed)
    ball = tree["ball"].astype(np.float64)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = ball[3] * (0.6 * rng.uniform(0, 1, n) ** (1 / 3) if where != "outside" else rng.uniform(1.05, 3.0, n))
    o = ball[:3] + u * rad[:, None]
    s = sc.arrays()[0].reshape(-1, 14)
    tgt = s[rng.integers(0, len(s), n), 0:3] + rng.normal(scale=0.3, size=(n, 3))
    d = (tgt - o) * (2.0 ** rng.uniform(-6, 6, n))[:, None]
    d = d.astype(np.float32)
    if where == "nonfinite":
        k = np.arange(7, n, 64)
        d[k, rng.integers(0, 3, len(k))] = rng.choice([np.inf, -np.inf, np.nan], len(k))
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = o
    rays[:, 3] = np.inf
    rays[:, 4:7] = d
    rays[:, 7] = np.array(-1, np.int32).view(np.float32)
    return rays


@pytest.mark.parametrize("where", ["inside", "outside", "nonfinite"])
@pytest.mark.parametrize("n", [71, 4000])
def test_shading_queries(gpu, shade_checker, large, tmp_path, monkeypatch, n, where):
    path, r = large(n)
    sc = r.scene
    rays = query_rays(sc, sc.sphere_tree_data(), 4093, 5 + n, where)
    kw = dict(gillum=2, depth=3, shadow=True, seed=SEED)
    want, st = shade_checker.shade(path, rays, **kw)
    tests = []
    for no_cull in (False, True):
        monkeypatch.setenv("SKR_NO_SPHERE_CULL", "1") if no_cull else monkeypatch.delenv("SKR_NO_SPHERE_CULL", raising=False)
        r.work(reset=True)
        got = r.shade(torch.from_numpy(rays).cuda(), skr.Options(W, H, **kw))
        torch.cuda.synchronize()
        c = r.work(reset=True)
        assert r.kernel_variant() == "shade_rays_g1_stree"
        g = got.cpu().numpy()
        ok = (g.view(np.uint32) == want.view(np.uint32)) | (np.isnan(g) & np.isnan(want))
        assert ok.all(), "n=%d %s no_cull=%s: %d of %d values differ" % (n, where, no_cull, int((~ok).sum()), ok.size)
        assert (c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]) == tuple(int(v) for v in st[:3]), (n, where, no_cull)
        tests.append(c["sphere_tests"])  # (the checker does not count them: the walk against occluded_pair's loop, which the frames hold to the oracle)
    assert tests[0] == tests[1], (n, where, tests)
    monkeypatch.delenv("SKR_NO_SPHERE_CULL", raising=False)


@pytest.mark.parametrize("where", ["inside", "outside", "nonfinite"])
@pytest.mark.parametrize("n,triangles", [(71, 0), (4000, 0), (4000, 6), (20000, 0)])
def test_ray_queries_walk_the_tree(gpu, ray_checker, large, monkeypatch, n, triangles, where):
    """closest and any-hit queries against tests/ray_query_checker.c, origins inside the ball (the walk), outside it and with one
    non-finite direction per wave (the loop), a quarter of the rays with a finite tmax; and the walk == SKR_NO_SPHERE_CULL=1 on every
    ray.  (A ray whose direction is not finite is held to the loop's answer: the checker is not asked about it.)"""
    _, r = large(n, triangles)
    sc = r.scene
    rays = query_rays(sc, sc.sphere_tree_data(), 4093, 11 + n, where)
    rng = np.random.default_rng(n)
    k = rng.random(len(rays)) < 0.25
    rays[k, 3] = rng.uniform(0.2, 3.0, int(k.sum())).astype(np.float32)
    s, t, _ = sc.arrays()
    finite = np.isfinite(rays[:, 4:7]).all(axis=1)
    safe = rays.copy()  # (what the checker sees in place of a ray it is not asked about)
    safe[~finite] = safe[finite][0]
    want, occ = ray_checker.trace(s, t, safe)
    d = torch.from_numpy(rays).cuda()
    res = {}
    for no_cull in (False, True):
        monkeypatch.setenv("SKR_NO_SPHERE_CULL", "1") if no_cull else monkeypatch.delenv("SKR_NO_SPHERE_CULL", raising=False)
        got, anyhit = r.trace(d), r.trace(d, any_hit=True)
        torch.cuda.synchronize()
        res[no_cull] = (got.raw.cpu().numpy().view(np.uint32), anyhit.cpu().numpy())
    monkeypatch.delenv("SKR_NO_SPHERE_CULL", raising=False)
    assert np.array_equal(res[False][0], res[True][0]) and np.array_equal(res[False][1], res[True][1]), "n=%d %s: the walk differs from the loop" % (n, where)
    bad = np.nonzero((res[False][0] != want.view(np.uint32)).any(axis=1) & finite)[0]
    assert len(bad) == 0, "n=%d %s: %d closest hits differ from the checker; first %d" % (n, where, len(bad), bad[0])
    assert np.array_equal(res[False][1][finite], occ[finite]), "n=%d %s: any-hit answers differ from the checker" % (n, where)
    kinds = res[False][0].view(np.int32)[:, 1]
    assert (kinds == 1).sum() > len(rays) // 20, "the rays hit too few spheres"


@pytest.mark.parametrize("n", [71, 4000])
def test_generic_ray_queries_still_pass(gpu, ray_checker, large, n):
    _, r = large(n)
    check_ray_queries(r, r.scene, ray_checker, 300 + n, "sphere tree on, n=%d" % n)


def test_shade_of_the_camera_rays_is_the_frame(gpu, large, monkeypatch):
    _, r = large(4000)
    opt = skr.Options(W, H, gillum=3, depth=3, shadow=True, seed=SEED)
    base = frame(r, opt, monkeypatch)
    rays = r.camera_rays(opt).view(-1, 8)
    keys = torch.arange(W * H, dtype=torch.int32, device=rays.device)
    r.work(reset=True)
    out = r.shade(rays, opt, 0, keys=keys)
    torch.cuda.synchronize()
    c = r.work(reset=True)
    assert np.array_equal(out.cpu().numpy().reshape(H, W, 3).view(np.uint32), base[1].view(np.uint32))
    assert (c["radiance_rays"], c["sphere_hits"], c["shadow_rays"], c["sphere_tests"]) == base[2]


def test_everything_built_on_frames_at_4000_spheres(gpu, oracle, large, monkeypatch):
    """render_adaptive (both round paths), render_denoised, --progressive 3, tiles with a stride, Multi on one device and a cloned
    renderer, each against the same construction from oracle frames"""
    path, r = large(4000)
    w, h, seed = 48, 27, 9
    kw = dict(gillum=2, depth=2, shadow=True)
    o_f = {}

    def o_frame(k):
        if k not in o_f:
            o_f[k] = oracle.render(path, w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, seed=seed + k, **kw)
        return o_f[k]

    # adaptive, both round paths
    lo, hi, t = 2, 5, 0.1
    mean, b, n = adaptive(lambda k: o_frame(k)[1].reshape(-1, 3), lo, hi, t)
    for path_name in ("frame", "query"):
        monkeypatch.setenv("SKR_ADAPTIVE_PATH", path_name)
        assert_same(run_adaptive(r, skr.Options(w, h, seed=seed, **kw), t, lo, hi), (b, mean, n), "adaptive, %s path" % path_name)
    monkeypatch.delenv("SKR_ADAPTIVE_PATH", raising=False)
    # --progressive 3: the binary32 sum of three frames in pass order, divided by 3 once
    acc = o_frame(0)[1].copy()
    for k in (1, 2):
        acc = acc + o_frame(k)[1]
    prog = (acc / np.float32(3)).astype(np.float32)
    rgb, rgbf = r.render(skr.Options(w, h, seed=seed, progressive=3, **kw), want_float=True)
    assert np.array_equal(rgbf.cpu().numpy().view(np.uint32), prog.view(np.uint32)), "--progressive 3"
    # the denoiser on the frame and its guides
    opt = skr.Options(w, h, seed=seed, **kw)
    hits = r.trace(r.camera_rays(skr.Options(w, h, seed=seed)).view(-1, 8)).raw.cpu().numpy()
    d_rgb, d_f = denoise_numpy(o_frame(0)[1], hits, 3)
    g_rgb, g_f, _ = r.render_denoised(opt, 3, want_float=True)
    assert np.array_equal(g_f.view(np.uint32), d_f.view(np.uint32)) and np.array_equal(g_rgb, d_rgb), "render_denoised"
    # tiles with a stride: tiles 1, 4, 7, ... of 4 rows
    rgb, rgbf = r.render(opt, want_float=True, tile_rows=4, first_tile=1, tile_stride=3)
    rows = np.concatenate([np.arange(4 * t, min(4 * t + 4, h)) for t in range(1, (h + 3) // 4, 3)])
    got = rgbf.cpu().numpy().reshape(-1, w, 3)
    assert np.array_equal(got[:len(rows)].view(np.uint32), o_frame(0)[1][rows].view(np.uint32)), "tiles with a stride"
    # Multi on one device, and a clone
    m = binding.Multi(r.scene, 1)
    assert np.array_equal(m.render_frame_host(opt, 8)[0], o_frame(0)[0]), "Multi"
    m.close()
    c = r.clone()
    got = frame(c, opt)
    assert got[3] == "level_pipeline_g1_stree"
    compare(got[0], got[1], o_frame(0)[0], o_frame(0)[1], "clone")
    c.close()


def test_executed_tests_at_20000_spheres_are_below_the_references(gpu, large):
    _, r = large(20000)
    r.count_triangle_work(True)
    r.sphere_tree_work(reset=True)
    r.work(reset=True)
    r.render(skr.Options(W, H, gillum=4, depth=3, shadow=True, seed=SEED))
    torch.cuda.synchronize()
    st = r.sphere_tree_work(reset=True)
    ref = r.work(reset=True)["sphere_tests"]
    r.count_triangle_work(False)
    print("20000 spheres: %d culling + %d sphere tests executed, the reference's loops run %d (ratio %.1f)"
          % (st["cull_tests"], st["sphere_tests"], ref, ref / max(1, st["cull_tests"] + st["sphere_tests"])))
    assert st["cull_tests"] > 0 and st["sphere_tests"] > 0
    assert st["cull_tests"] + st["sphere_tests"] < ref


def test_switch_on_and_off_renderers_alternate(gpu, tmp_path, monkeypatch):
    path = write_scene(tmp_path / "n71.scn", 71)
    on, off = skr.Renderer(skr.parse_scene(path, sphere_tree=True)), skr.Renderer(skr.parse_scene(path))
    opt = skr.Options(W, H, gillum=4, depth=3, shadow=True, seed=SEED)
    first = None
    for _ in range(3):
        a, b = frame(on, opt, monkeypatch), frame(off, opt, monkeypatch)
        assert a[3] == "level_pipeline_g1_stree" and b[3] in ("node_levels_v5", "node_levels_v5_flat")
        same(a, b, "on against off")
        first = first or a
        same(a, first, "frame after frame")
    on.close()
    off.close()
