"""Shading queries on the MI355X (include/skr.h skr_shade_rays): the radiance of caller-supplied rays bit for bit against
the CPU checkers (tests/shade_query_checker.c, shade_query_fog_checker.c), counts included; camera rays against the frame itself;
culling, banding, non-interference with renders, bad rays and argument errors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import skele_raytracer_amd as skr
from conftest import scene_path
from oracle import pyoracle
from shade_query_check import build as build_checker
from test_ray_query_gpu import random_rays

pytestmark = pytest.mark.gpu

N_RAYS = (1 << 14) - 13  # not a multiple of 64: the last wave is partial


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("shadecheck_gpu")))


def scn_text(spheres, triangles, camera=(0, 0, -10, 0, 0, 1, 0, 1, 0, 30)):
    """A .scn file of spheres [ns, 4] and triangles [nt, 9] under two point lights, so that the same scene loads in libskr and in the
    oracle."""
    lines = ["camera " + " ".join("%r" % float(v) for v in camera), "background .1 .15 .2", "ambient_light .3 .3 .3",
             "point_light 20 20 20 3 8 -6", "point_light 5 5 5 -6 2 -2"]
    rng = np.random.default_rng(len(spheres) + 7 * len(triangles))
    for s in spheres:
        c = rng.uniform(0.1, 1.0, 3)
        lines.append("material %f %f %f %f %f %f .3 .3 .3 %d .2 .2 .2 %f" % (*c, *c, int(rng.choice([8, 16, 32])), rng.uniform(1.1, 1.6)))
        lines.append("sphere %r %r %r %r" % tuple(float(v) for v in s[:4]))
    if len(triangles):
        lines.append("material .6 .5 .4 .6 .5 .4 .2 .2 .2 16 0 0 0 1")
        lines.append("max_vertices %d" % (3 * len(triangles)))
        for t in triangles:
            for k in range(3):
                lines.append("vertex %r %r %r" % tuple(float(v) for v in t[3 * k: 3 * k + 3]))
        for i in range(len(triangles)):
            lines.append("triangle %d %d %d" % (3 * i, 3 * i + 1, 3 * i + 2))
    return "\n".join(lines) + "\n"


def arrays_scene_file(tmp_dir, name, seed, ns, nt):
    rng = np.random.default_rng(seed)
    s = np.zeros((ns, 4), np.float32)
    s[:, :3] = rng.uniform(-4, 4, (ns, 3))
    s[:, 3] = rng.uniform(0.2, 1.2, ns)
    c = rng.uniform(-4, 4, (nt, 1, 3))
    t = (c + rng.normal(scale=0.6, size=(nt, 3, 3))).reshape(nt, 9).astype(np.float32)
    path = os.path.join(tmp_dir, name + ".scn")
    with open(path, "w") as f:
        f.write(scn_text(s, t))
    return path


@pytest.fixture(scope="session")
def scene_files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("shade_scenes"))
    return {"spheres2": scene_path("spheres2.scn"), "bear": scene_path("bear.scn"), "test": scene_path("test.scn"),
            "arrays_no_spheres": arrays_scene_file(d, "nosph", 5, 0, 300), "arrays_no_triangles": arrays_scene_file(d, "notri", 6, 40, 0)}


MODES = {
    "direct": dict(),
    "direct_shadow": dict(shadow=True),
    "gillum4_depth3_shadow": dict(gillum=4, depth=3, shadow=True),
    "strict_scn": dict(gillum=2, depth=2, shadow=True, strict=True),
    "shade_triangles_gillum2_depth3": dict(gillum=2, depth=3, shade_triangles=True),
    "legacy_reflect_depth3": dict(depth=3, legacy_reflect=True, shadow=True),
}


def options(width=320, height=180, **kw):
    kw = {k: v for k, v in kw.items() if k != "strict"}
    return skr.Options(width, height, seed=kw.pop("seed", 13), **kw)


def gpu_shade(r, rays, opt, sample=0, keys=None):
    """(float32 [n, 3], counter deltas [rays, hits, shadow rays])"""
    r.counters(reset=True)
    k = None if keys is None else torch.from_numpy(np.ascontiguousarray(keys, np.int64).astype(np.uint32).view(np.int32)).cuda()
    out = r.shade(torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda(), opt, sample, keys=k)
    torch.cuda.synchronize()
    c = r.counters(reset=True)
    return out.cpu().numpy(), [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]]


def assert_bitwise(got, want, what):
    g, w = got.reshape(-1, 3).view(np.uint32), want.reshape(-1, 3).view(np.uint32)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d rays differ; first %d: gpu %s cpu %s" % (what, len(bad), len(g), bad[0], got.reshape(-1, 3)[bad[0]],
                                                                                 want.reshape(-1, 3)[bad[0]])


def sparse_keys(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.permutation(n).astype(np.uint64) * 7919 + 12345) % (1 << 32)


def check_case(checker, path, mode_kw, n, seed, fog=None):
    kw = dict(mode_kw)
    strict = kw.pop("strict", False)
    sc = skr.parse_scene(path, strict=strict, fog=fog is not None)
    r = skr.Renderer(sc, 0)
    rays = random_rays(sc, n, seed)
    keys = sparse_keys(n, seed)
    got, cnt = gpu_shade(r, rays, options(**kw), sample=3, keys=keys)
    want, st = checker.shade(pyoracle.OracleScene(path, strict=strict), rays, sample=3, keys=keys, seed=13, fog=fog, **kw)
    assert_bitwise(got, want, "%s %s" % (os.path.basename(path), mode_kw))
    assert cnt == [int(x) for x in st]
    bg = np.array(list(sc.info.background), np.float32)
    assert (got != bg).any(axis=1).any() and (got == bg).all(axis=1).any(), "the rays must both hit and miss"
    return r, rays, got


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["spheres2", "bear", "test", "arrays_no_spheres", "arrays_no_triangles"])
def test_shade_matches_the_checker(checker, scene_files, name, mode):
    check_case(checker, scene_files[name], MODES[mode], N_RAYS, seed=sum(name.encode()) + len(mode))


def test_fog_matches_the_checker(checker):
    fog = skr.parse_scene(scene_path("spheres2.scn"), fog=True).fog
    check_case(checker, scene_path("spheres2.scn"), dict(gillum=2, depth=2, shadow=True), N_RAYS, seed=77, fog=fog)


@pytest.mark.parametrize("mode", ["direct_shadow", "shade_triangles_gillum2_depth3"])
def test_dragon_matches_the_checker(checker, mode):
    check_case(checker, scene_path("dragon.scn"), MODES[mode], 1 << 12, seed=99)


def frame_and_query(r, opt, sample=0):
    """the frame's float output and counter deltas; the query of its camera rays (keys y*W+x)"""
    r.counters(reset=True)
    _, f = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    c = r.counters(reset=True)
    rays = r.camera_rays(opt, sample).view(-1, 8)
    keys = torch.arange(opt.width * opt.height, dtype=torch.int32, device="cuda")
    q = r.shade(rays, opt, sample, keys=keys)
    torch.cuda.synchronize()
    cq = r.counters(reset=True)
    return f.cpu().numpy(), c, q.cpu().numpy(), cq


@pytest.mark.parametrize("case", ["config3", "config4", "spheres2_shade_triangles", "spheres2_fog_640", "spheres2_legacy_640"])
def test_camera_rays_are_the_frame(case):
    scn, fog, kw, wh = {
        "config3": ("spheres2.scn", False, dict(gillum=16, shadow=True, depth=3), (1920, 1080)),
        "config4": ("dragon.scn", False, dict(gillum=16, depth=3), (1920, 1080)),
        "spheres2_shade_triangles": ("spheres2.scn", False, dict(gillum=2, shade_triangles=True), (1920, 1080)),
        "spheres2_fog_640": ("spheres2.scn", True, dict(gillum=2, depth=2, shadow=True), (640, 360)),
        "spheres2_legacy_640": ("spheres2.scn", False, dict(depth=3, legacy_reflect=True, shadow=True), (640, 360)),
    }[case]
    r = skr.Renderer(skr.parse_scene(scene_path(scn), fog=fog), 0)
    opt = skr.Options(*wh, seed=21, **kw)
    f, c, q, cq = frame_and_query(r, opt)
    assert skr.Renderer.kernel_variant() == "shade_rays_g1"
    assert_bitwise(q, f, case)
    assert cq == c


def test_jittered_samples_sum_to_the_frame():
    r = skr.Renderer(skr.parse_scene(scene_path("spheres2.scn")), 0)
    opt = skr.Options(320, 180, jsample=3, gillum=2, depth=2, shadow=True, seed=4)
    r.counters(reset=True)
    _, f = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    c = r.counters(reset=True)
    keys = torch.arange(320 * 180, dtype=torch.int32, device="cuda")
    acc = np.zeros((320 * 180, 3), np.float32)
    for s in range(9):
        acc = acc + r.shade(r.camera_rays(opt, s).view(-1, 8), opt, s, keys=keys).cpu().numpy()
    assert_bitwise(acc / np.float32(9.0), f.cpu().numpy(), "--jsample 3")
    assert r.counters(reset=True) == c


def test_a_subset_of_pixels_with_their_own_keys():
    """adaptive sampling: some pixels re-shaded alone equal those pixels of the frame"""
    r = skr.Renderer(skr.parse_scene(scene_path("test.scn")), 0)
    opt = skr.Options(320, 180, gillum=4, depth=3, shadow=True, seed=6)
    _, f = r.render(opt, want_float=True)
    pick = torch.from_numpy(np.sort(np.random.default_rng(1).choice(320 * 180, 5000, replace=False))).cuda()
    rays = r.camera_rays(opt).view(-1, 8)[pick]
    q = r.shade(rays, opt, keys=pick.to(torch.int32))
    torch.cuda.synchronize()
    assert_bitwise(q.cpu().numpy(), f.view(-1, 3)[pick].cpu().numpy(), "pixel subset")


@pytest.mark.parametrize("shade_triangles", [False, True])
@pytest.mark.parametrize("name", ["dragon.scn", "test.scn"])
def test_culling_changes_nothing(name, shade_triangles):
    sc = skr.parse_scene(scene_path(name))
    r = skr.Renderer(sc, 0)
    opt = skr.Options(320, 180, gillum=2, depth=2, shade_triangles=shade_triangles, seed=2)
    rays = np.concatenate([random_rays(sc, 1 << 13, seed=5), r.camera_rays(opt).view(-1, 8).cpu().numpy()])
    culled, c1 = gpu_shade(r, rays, opt)
    os.environ["SKR_NO_CULL"] = "1"
    try:
        brute, c2 = gpu_shade(r, rays, opt)
    finally:
        del os.environ["SKR_NO_CULL"]
    assert_bitwise(culled, brute, "%s culled vs every triangle" % name)
    assert c1 == c2


def test_bands_equal_one_call():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    rays = random_rays(sc, 200_000, seed=8)
    opt = skr.Options(64, 64, gillum=4, depth=3, shadow=True)
    r = skr.Renderer(sc, 0)
    whole, c1 = gpu_shade(r, rays, opt, sample=1)
    os.environ["SKR_LEVELS_BUDGET_MB"] = "16"
    try:
        banded, c2 = gpu_shade(r, rays, opt, sample=1)
    finally:
        del os.environ["SKR_LEVELS_BUDGET_MB"]
    assert_bitwise(banded, whole, "banded vs one band")
    assert c1 == c2


def test_render_shade_render():
    sc = skr.parse_scene(scene_path("test.scn"))
    r = skr.Renderer(sc, 0)
    opt = skr.Options(320, 180, gillum=2, depth=2, shade_triangles=True)
    r.counters(reset=True)
    rgb1, f1 = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    c1 = r.counters(reset=True)
    r.shade(torch.from_numpy(random_rays(sc, 50_000, seed=3)).cuda(), opt)
    torch.cuda.synchronize()
    r.counters(reset=True)
    rgb2, f2 = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    assert torch.equal(rgb1, rgb2) and torch.equal(f1, f2)
    assert r.counters(reset=True) == c1


@pytest.mark.parametrize("name", ["spheres2.scn", "test.scn", "dragon.scn"])
def test_bad_rays_do_not_disturb_good_ones(name):
    sc = skr.parse_scene(scene_path(name))
    r = skr.Renderer(sc, 0)
    opt = skr.Options(64, 64, gillum=2, depth=2, shadow=True, shade_triangles=name != "spheres2.scn")
    rays = random_rays(sc, 4096, seed=31)
    clean, _ = gpu_shade(r, rays, opt)
    bad = np.arange(5, 4096, 97)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    junk = [(nan, 0, 0, 1), (0, 0, 0, 0), (inf, 1, 0, 0), (0, nan, 1, 1), (0, 0, -inf, 1)]
    for j, i in enumerate(bad):
        o0, d0, d1, d2 = junk[j % len(junk)]
        rays[i, 0] = o0 if j % 2 else rays[i, 0]
        rays[i, 4:7] = (d0, d1, d2) if not (j % 2) else (0, 0, 0)
        if j % 3 == 0:
            rays[i, 3] = nan
    dirty, _ = gpu_shade(r, rays, opt)
    good = np.setdiff1d(np.arange(len(rays)), bad)
    assert_bitwise(dirty[good], clean[good], name + " good rays beside bad ones")


def test_argument_errors_and_empty_calls():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    r = skr.Renderer(sc, 0)
    L = skr.lib()
    rays = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    out = torch.zeros((5, 3), dtype=torch.float32, device="cuda")
    keys = torch.zeros(5, dtype=torch.int32, device="cuda")
    opt = skr.Options(32, 16)
    o, p, q, k = C.byref(opt.c), rays.data_ptr(), out.data_ptr(), keys.data_ptr()
    assert L.skr_shade_rays(r.h, o, None, 4, 0, None, q, None) == 2
    assert L.skr_shade_rays(r.h, o, p, 4, 0, None, None, None) == 2
    assert L.skr_shade_rays(None, o, p, 4, 0, None, q, None) == 2
    assert L.skr_shade_rays(r.h, None, p, 4, 0, None, q, None) == 2
    assert L.skr_shade_rays(r.h, o, p + 4, 3, 0, None, q, None) == 2  # misaligned rays
    assert L.skr_shade_rays(r.h, o, p, 4, 0, None, q + 2, None) == 2  # misaligned output
    assert L.skr_shade_rays(r.h, o, p, 4, 0, k + 2, q, None) == 2  # misaligned keys
    assert L.skr_shade_rays(r.h, C.byref(skr.Options(32, 16, depth=0).c), p, 4, 0, None, q, None) == 2  # bad options
    sentinel = torch.full((4, 3), 7.0, device="cuda")
    assert L.skr_shade_rays(r.h, o, p, 0, 0, None, sentinel.data_ptr(), None) == 0  # n == 0: nothing launched
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())
    fog = skr.Renderer(skr.parse_scene(scene_path("spheres2.scn"), fog=True), 0)
    assert L.skr_shade_rays(fog.h, C.byref(skr.Options(32, 16, legacy_reflect=True).c), p, 4, 0, None, q, None) == 4
    assert L.skr_shade_rays(r.h, C.byref(skr.Options(32, 16, gillum=32767, depth=4).c), p, 4, 0, None, q, None) == 4  # > 2^32 node ids
    assert r.shade(torch.zeros((0, 8), dtype=torch.float32, device="cuda"), opt).shape == (0, 3)
    with pytest.raises(skr.SkrError):
        r.shade(rays[:, :7], opt)
    with pytest.raises(skr.SkrError):
        r.shade(rays, opt, keys=torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(skr.SkrError):
        r.shade(rays, opt, keys=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(skr.SkrError):
        r.shade(rays.cpu(), opt)
