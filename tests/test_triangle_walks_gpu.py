"""The triangle walks on the MI355X at their decision boundaries: the families of tests/triangle_cases.py through Renderer.trace
(closest hit and any-hit) against the CPU checker tests/ray_query_checker.c bit for bit, with the culling and the cones switched
off, in other wave compositions, and as frames against the oracle.  tests/test_triangle_cases_cpu.py shows on the host that the
families reach the decisions they are built for and pins the numpy classification used here to the checker."""
import os

import numpy as np
import pytest
import torch

import skele_raytracer_amd as skr
import triangle_cases as tc
from conftest import scene_path
from ray_query_check import build as build_checker
from test_gpu_parity import compare
from test_ray_query_gpu import assert_bitwise, gpu_trace

pytestmark = pytest.mark.gpu
f32 = np.float32
DRAGON_RAYS = 1 << 16   # at most, per call on dragon.scn
SMALL_RAYS = 1 << 18    # at most, per call on scenes under 2 000 triangles


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("triwalk")))


@pytest.fixture(scope="module")
def soup(tmp_path_factory):
    return tc.soup_path(tmp_path_factory.mktemp("soup"))


def thin(rays, limit):
    """Every k-th whole wave of 64, so that at most `limit` rays remain and the waves stay as built."""
    n = len(rays)
    if n <= limit:
        return rays
    waves = np.arange((n + 63) // 64)
    keep = waves[:: -(-len(waves) * 64 // limit)]
    idx = (keep[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
    return rays[idx[idx < n]]


def border_all(scene, n, levels=(0, 1, 2)):
    return scene, np.concatenate([tc.border(scene, level, n, tree=tree)[1] for level in levels for tree in ("renderer", "trace")])


FAMILIES = {
    "border_dragon": lambda soup: border_all(scene_path("dragon.scn"), 8192),
    "border_test": lambda soup: border_all(scene_path("test.scn"), 16384),
    "border_soup": lambda soup: border_all(soup, 16384),
    "border_decks": lambda soup: border_all(tc.decks(n=2)[0], 16384),
    "edges_plate": lambda soup: tc.edges("plate")[:2],
    "edges_dragon": lambda soup: tc.edges("dragon")[:2],
    "det_cut": lambda soup: tc.det_cut()[:2],
    "t_zero": lambda soup: tc.t_zero()[:2],
    "nests": lambda soup: tc.nests()[:2],
    "nests_pairs_only": lambda soup: tc.nests(third=False)[:2],
    "decks": lambda soup: tc.decks()[:2],
    "cone_edge_test_0": lambda soup: tc.cone_edge(scene_path("test.scn"), 0)[:2],
    "cone_edge_test_2": lambda soup: tc.cone_edge(scene_path("test.scn"), 2)[:2],
    "cone_edge_dragon": lambda soup: tc.cone_edge(scene_path("dragon.scn"), 0)[:2],
    "graze_behind": lambda soup: tc.graze_behind()[:2],
    "levels_dragon": lambda soup: tc.levels(scene_path("dragon.scn"))[:2],
    "levels_test": lambda soup: tc.levels(scene_path("test.scn"), n=8192)[:2],
}


def family(name, soup):
    scene, rays = FAMILIES[name](soup)
    sc, s, t = tc.load(scene)
    rays = thin(rays, DRAGON_RAYS if len(t) >= 2000 else SMALL_RAYS)
    return sc, s, t, np.ascontiguousarray(rays)


def under(env, sc):
    """A renderer created with the development switch `env` set (api.cpp load_switches reads it then)."""
    if env is None:
        return skr.Renderer(sc, 0)
    os.environ[env] = "1"
    try:
        return skr.Renderer(sc, 0)
    finally:
        del os.environ[env]


def trees_walked(sc, rays):
    """The tree each 64-ray wave picks (wave_common.h pick_query_tree), restated: 'renderer', 'trace' or 'none', and its level."""
    o, d, _, _ = tc.ray_parts(rays)
    dd = tc._dot(d, d)
    pad = (-len(rays)) % 64
    wave = lambda x, fill: np.concatenate([x, np.full(pad, fill, x.dtype)]).reshape(-1, 64)
    level = tc.query_level(wave(dd, f32(0))).max(axis=1)
    at_cam = wave(np.all(o.view(np.uint32) == tc.camera_of(sc).view(np.uint32), axis=1), True).all(axis=1)
    ball = wave(tc.in_ball(o, sc.trace_culling(0)[5]), True).all(axis=1)
    kind = np.where(level == 3, "none", np.where(at_cam, "renderer", np.where(ball, "trace", "none")))
    return kind, level


@pytest.mark.parametrize("name", list(FAMILIES))
def test_family_matches_the_checker_with_and_without_culling(checker, soup, name):
    sc, s, t, rays = family(name, soup)
    want, occ_want = checker.trace(s, t, rays)
    r = skr.Renderer(sc, 0)
    got = gpu_trace(r, rays)
    occ = gpu_trace(r, rays, any_hit=True)
    kind, level = trees_walked(sc, rays)
    print("%s: %d rays, %d triangles; waves on the renderer's tree %d, the trace tree %d, no tree %d; levels %s; triangle hits %d" % (
        name, len(rays), len(t), (kind == "renderer").sum(), (kind == "trace").sum(), (kind == "none").sum(),
        np.bincount(level, minlength=4).tolist(), (want[:, 1].view(np.int32) == 2).sum()))
    assert_bitwise(got, want, name)
    assert np.array_equal(occ, occ_want), name + " any-hit"
    assert (want[:, 1].view(np.int32) == 2).sum() >= 50
    if name.startswith(("border", "edges", "det_cut", "nests", "decks", "levels")):
        assert (kind == "renderer").any() and (kind == "trace").any()
    if name.startswith("levels"):
        assert all((level == k).any() for k in range(4)) and (kind == "none").any()
    for env in ("SKR_NO_CULL", "SKR_NO_CONES"):
        r2 = under(env, sc)
        assert_bitwise(gpu_trace(r2, rays), got, "%s under %s" % (name, env))
        assert np.array_equal(gpu_trace(r2, rays, any_hit=True), occ), "%s any-hit under %s" % (name, env)


def finite_tmax(rays, hits, rng):
    """The rays with tmax drawn around their own hit distance: at t, one ulp either side, and well before or behind."""
    out = rays.copy()
    t = hits[:, 0]
    pick = rng.integers(0, 5, len(rays))
    with np.errstate(invalid="ignore", over="ignore"):
        choice = [t, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf)), t * f32(0.5), t * f32(2)]
    out[:, 3] = np.choose(pick, choice)
    return out


@pytest.mark.parametrize("name", ["nests", "decks", "graze_behind", "edges_dragon", "t_zero"])
def test_any_hit_walk_at_tmax(checker, soup, name):
    """tree_walk_any prunes with the running best fixed at tmax and accepts 0 < t < tmax: tmax on and beside the hit distance."""
    sc, s, t, rays = family(name, soup)
    hits, _ = checker.trace(s, t, rays)
    rays = finite_tmax(rays, hits, np.random.default_rng(3))
    want, occ_want = checker.trace(s, t, rays)
    r = skr.Renderer(sc, 0)
    assert_bitwise(gpu_trace(r, rays), want, name + " with tmax")
    occ = gpu_trace(r, rays, any_hit=True)
    assert np.array_equal(occ, occ_want)
    assert occ.any() and not occ.all()
    assert np.array_equal(gpu_trace(under("SKR_NO_CULL", sc), rays, any_hit=True), occ)


# ---- wave composition -----------------------------------------------------------------------------------------------------------------
def outliers(sc, rays, rng):
    """Lane 0 of every wave replaced by a ray that changes the wave's tree: |d| = 300, an origin 10 ball radii away, an origin one ulp
    off the camera in x, a NaN direction (in turn)."""
    out = rays.copy()
    ball = sc.trace_culling(0)[5]
    cam = tc.camera_of(sc)
    lanes = np.arange(0, len(rays), 64)
    for j, i in enumerate(lanes):
        d = out[i, 4:7].astype(np.float64)
        kind = j % 4
        if kind == 0:
            out[i, 4:7] = d * 300.0 / max(np.linalg.norm(d), 1e-30)
        elif kind == 1:
            out[i, 0:3] = ball[:3] + f32(10) * ball[3] * np.array([0.6, 0.0, 0.8], f32)
        elif kind == 2:
            out[i, 0:3] = cam
            out[i, 0] = np.nextafter(cam[0], f32(np.inf))
        else:
            out[i, 4] = np.nan
    return out, lanes


@pytest.mark.parametrize("name", ["nests", "decks", "border_dragon"])
def test_wave_composition_changes_no_ray(checker, soup, name):
    """A lane's answer does not depend on the rays it shares a wave with: the tree is picked per wave and an entry is entered when any
    lane wants it."""
    sc, s, t, rays = family(name, soup)
    rng = np.random.default_rng(17)
    r = skr.Renderer(sc, 0)
    want, occ_want = checker.trace(s, t, rays)
    a = gpu_trace(r, rays)
    assert_bitwise(a, want, name + " as built")
    perm = rng.permutation(len(rays))
    b = gpu_trace(r, np.ascontiguousarray(rays[perm]))
    assert_bitwise(b, a[perm], name + " permuted")
    assert np.array_equal(gpu_trace(r, np.ascontiguousarray(rays[perm]), any_hit=True), occ_want[perm])
    mixed, lanes = outliers(sc, rays, rng)
    c = gpu_trace(r, mixed)
    rest = np.setdiff1d(np.arange(len(rays)), lanes)
    assert_bitwise(c[rest], a[rest], name + " beside outliers")
    finite = lanes[np.isfinite(mixed[lanes, 4])]  # the outliers themselves, but for the NaN directions
    assert_bitwise(c[finite], checker.trace(s, t, mixed[finite])[0], name + " outliers")
    kind_a, _ = trees_walked(sc, rays)
    kind_c, _ = trees_walked(sc, mixed)
    assert (kind_a != kind_c).mean() > 0.5, "the outliers must change the tree of most waves"
    occ_c = gpu_trace(r, mixed, any_hit=True)
    assert np.array_equal(occ_c[rest], occ_want[rest])
    # one live ray per wave: the other 63 can hit nothing (tmax = -inf)
    live = rng.permutation(len(rays))[:1024]
    alone = np.repeat(rays[live], 64, axis=0)
    alone[:, 3] = -np.inf
    at = np.arange(1024) * 64 + rng.integers(0, 64, 1024)
    alone[at] = rays[live]
    e = gpu_trace(r, alone)
    assert_bitwise(e[at], a[live], name + " alone in the wave")
    assert (e[np.setdiff1d(np.arange(len(alone)), at), 1].view(np.int32) == 0).all()
    assert np.array_equal(gpu_trace(r, alone, any_hit=True)[at], occ_want[live])


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
FRAME_SCENES = {"nests": lambda: tc.nests()[0], "decks": lambda: tc.decks(n=2)[0], "plate": lambda: tc.edges("plate")[0]}


@pytest.mark.parametrize("name", list(FRAME_SCENES))
def test_frames_match_the_oracle(oracle, tmp_path, name):
    """The families' meshes as scenes with three spheres and a point light, 96x54: closest_triangle at level 1 and on GI children
    (--shade-triangles), and HEAD's rule (any_triangle_closer) on the direct kernel and in the level pipeline."""
    scn = tc.write_scn(str(tmp_path / (name + ".scn")), FRAME_SCENES[name]())
    w, h = 96, 54
    for kw, variant in ((dict(shade_triangles=True, gillum=2, depth=3, shadow=True, seed=5), "level_pipeline_g1"),
                        (dict(shadow=True), "direct_v3"),
                        (dict(gillum=2, depth=3, shadow=True, seed=6), "level_pipeline_g1")):
        r = skr.Renderer(skr.parse_scene(scn))
        rgb, rgbf = r.render(skr.Options(w, h, **kw), want_float=True)
        torch.cuda.synchronize()
        assert skr.Renderer.kernel_variant() == variant, (name, kw, skr.Renderer.kernel_variant())
        o_rgb, o_f, st = oracle.render(scn, w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw)
        compare(rgb.cpu().numpy(), rgbf.cpu().numpy(), o_rgb, o_f, "%s %s" % (name, kw))
        cnt = r.counters()
        assert cnt["radiance_rays"] == int(st[0]) and cnt["sphere_hits"] == int(st[1]) and cnt["shadow_rays"] == int(st[2])


# ---- the shadow walk's far end --------------------------------------------------------------------------------------------------------
def test_shadow_walk_at_tmax(tmp_path):
    """tree_walk_shadow's 0 < t < tmax where t = tmax up to rounding (tests/test_triangle_cases_cpu.py test_shadow_rays_reach_tmax counts
    the decisions within 4 ulps): frames against tests/triangle_shadow_checker.c bit for bit, two lights (the pair instance), with the
    culling and the cones off, and the same through Renderer.shade on the frame's camera rays."""
    from triangle_shadow_check import build
    ck = build(str(tmp_path))
    scn = tc.write_lights_in_plane_scene(str(tmp_path / "inplane.scn"))
    w, h = 96, 54
    bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)
    for kw in (dict(), dict(gillum=2, depth=3, seed=3)):
        opt = dict(shade_triangles=True, shadow=True, **kw)
        c_rgb, c_f, c_st = ck.render(scn, w, h, triangle_shadows=True, **opt)
        off = ck.render(scn, w, h, triangle_shadows=False, **opt)[1]
        assert (bits(c_f) != bits(off)).any() and (bits(c_f) == bits(off)).all(axis=2).any()
        sc = skr.parse_scene(scn, triangle_shadows=True)
        for env in (None, "SKR_NO_CULL", "SKR_NO_CONES"):
            r = under(env, sc) if env else skr.Renderer(sc)
            o = skr.Options(w, h, **opt)
            rgb, rgbf = r.render(o, want_float=True)
            torch.cuda.synchronize()
            assert skr.Renderer.kernel_variant() == "level_pipeline_g1_tshadow"
            nb = int((bits(rgbf.cpu().numpy()) != bits(c_f)).sum())
            assert nb == 0, "%s %s: %d float words differ from the checker" % (kw, env, nb)
            assert np.array_equal(rgb.cpu().numpy(), c_rgb)
            c = r.counters()
            assert [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]] == [int(x) for x in c_st[:3]]
            if env is None:
                rays = r.camera_rays(o).view(-1, 8)
                keys = torch.arange(w * h, dtype=torch.int32, device=rays.device)
                got = r.shade(rays, o, keys=keys)
                torch.cuda.synchronize()
                assert skr.Renderer.kernel_variant() == "shade_rays_g1_tshadow"
                assert np.array_equal(bits(got.cpu().numpy()), bits(c_f).reshape(-1, 3))
