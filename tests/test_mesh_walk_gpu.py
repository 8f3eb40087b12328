"""The triangle walks (shade_common.h, trace_rays.hip) on the MI355X beside tests/test_triangle_walks_gpu.py: the counting instances of
the walks against the plain ones, meshes of 7 to 17
triangles on the tree and on the loop over every triangle, and the families of tests/triangle_cases.py with the development switches
SKR_NO_CULL and SKR_NO_CONES in force at the launch."""
import contextlib
import os

import numpy as np
import pytest
import torch

import skele_raytracer_amd as skr
import triangle_cases as tc
from conftest import scene_path
from ray_query_check import build as build_checker
from test_ray_query_gpu import assert_bitwise, gpu_trace
from test_triangle_walks_gpu import FAMILIES, family

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("meshwalk")))


@pytest.fixture(scope="module")
def soup(tmp_path_factory):
    return tc.soup_path(tmp_path_factory.mktemp("soup"))


@contextlib.contextmanager
def under(env, sc):
    """A renderer of `sc` while the development switch `env` is set (None: no switch).  The binding re-reads the switches before a launch
    whenever the environment has changed since the last one, so a switch that is set only while the renderer is made is dropped again
    at its first launch: the variable stays set for as long as the renderer is used.  (tests/test_triangle_walks_gpu.py `under` sets it
    only while the renderer is made: its SKR_NO_CULL / SKR_NO_CONES comparisons run with the defaults, and
    test_family_matches_the_checker_with_the_switches_in_force below is the one that holds them.)"""
    if env is not None:
        os.environ[env] = "1"
    try:
        r = skr.Renderer(sc, 0)
        try:
            yield r
        finally:
            r.close()
    finally:
        if env is not None:
            del os.environ[env]


@pytest.mark.parametrize("name", list(FAMILIES))
def test_family_matches_the_checker_with_the_switches_in_force(checker, soup, name):
    """Closest hit and any-hit of every family against the checker bit for bit while SKR_NO_CULL (every wave on the loop over every
    triangle) and SKR_NO_CONES (the tight radii dropped) hold at the launch itself."""
    sc, s, t, rays = family(name, soup)
    want, occ_want = checker.trace(s, t, rays)
    for env in ("SKR_NO_CULL", "SKR_NO_CONES"):
        with under(env, sc) as r:
            assert_bitwise(gpu_trace(r, rays), want, "%s under %s" % (name, env))
            assert np.array_equal(gpu_trace(r, rays, any_hit=True), occ_want), "%s any-hit under %s" % (name, env)


# ---- the counting instances -----------------------------------------------------------------------------------------------------------
def light_scene(triangles):
    """`triangles` alone under ARRAY_CAMERA with a point light and triangle shadows switched on (Scene.from_arrays: no sphere, so chunks of
    4 triangles)."""
    t = np.asarray(triangles, f32).reshape(-1, 9)
    mats = np.tile(np.array([.3, .3, .3, .6, .6, .6, .2, .2, .2, 6], f32), (len(t), 1))
    return skr.Scene.from_arrays(np.zeros((0, 14), f32), t, np.array([[2, 6, -7, 30, 30, 30]], f32), tc.ARRAY_CAMERA, background=(.1, .2, .3),
                                 ambient=(.3, .3, .3), triangle_materials=mats, triangle_shadows=True)


COUNTED = {
    # closest_triangle at every level and shadow_triangles
    "test_shaded": (lambda: skr.parse_scene(scene_path("test.scn"), triangle_shadows=True), 96, 64, dict(shade_triangles=True)),
    # any_triangle_closer at every level
    "test_black": (lambda: skr.parse_scene(scene_path("test.scn"), triangle_shadows=True), 96, 64, dict()),
    "decks_shaded": (lambda: light_scene(tc.decks(n=2)[0]), 64, 64, dict(shade_triangles=True)),
}


@pytest.mark.parametrize("name", list(COUNTED))
def test_counting_changes_no_bit_and_counts_the_walks(name):
    """The counting instances of the triangle walks (count_triangle_work: mesh_walk under any_triangle_closer and shadow_triangles,
    tree_walk_closest) give the frame of the plain ones byte for byte, u8 and float, and count
    entries and triangles; without a tree (SKR_NO_CULL) the same frame again, no entry counted."""
    make, w, h, kw = COUNTED[name]
    sc = make()
    opt = skr.Options(w, h, gillum=2, depth=2, shadow=True, seed=5, **kw)
    frames = {}
    for env, count in ((None, False), (None, True), ("SKR_NO_CULL", True)):
        with under(env, sc) as r:
            r.count_triangle_work(count)
            r.triangle_work(reset=True)
            rgb, rgbf = r.render(opt, want_float=True)
            torch.cuda.synchronize()
            frames[env, count] = (rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), r.triangle_work(reset=False))
    plain, counted, brute = frames[None, False], frames[None, True], frames["SKR_NO_CULL", True]
    print("%s: counted %s, without a tree %s" % (name, counted[2], brute[2]))
    for other, what in ((counted, "counting"), (brute, "counting without a tree")):
        assert np.array_equal(other[0], plain[0]), "%s: the u8 frame changes with %s" % (name, what)
        assert np.array_equal(other[1], plain[1]), "%s: the float frame changes with %s" % (name, what)
    assert counted[2]["cull_tests"] > 0 and counted[2]["triangle_tests"] > 0
    assert brute[2]["cull_tests"] == 0


# ---- the loop over every triangle past a multiple of eight ----------------------------------------------------------------------------
SMALL = {"decks": lambda: tc.decks(n=2)[0], "nests": lambda: tc.nests(per_pair=2)[0]}


def small_case(kind, nt):
    """The first `nt` triangles of a family's mesh and 4096 border rays on them, half for each tree."""
    mesh = np.ascontiguousarray(SMALL[kind]()[:nt])
    rays = np.concatenate([tc.border(mesh, 0, 2048, tree=tree)[1] for tree in ("renderer", "trace")])
    return mesh, np.ascontiguousarray(rays)


@pytest.mark.parametrize("nt", [7, 8, 9, 17])
@pytest.mark.parametrize("kind", list(SMALL))
def test_small_meshes_with_and_without_the_tree(checker, kind, nt):
    """The loops over every triangle look at the wave-wide exit every eighth triangle, and the prefetching ones read the pad triangle behind
    the last: meshes one short of,
    at and past a multiple of eight, closest hit and any-hit against the checker bit for bit, on the tree and on the loop."""
    mesh, rays = small_case(kind, nt)
    sc, s, t = tc.load(mesh)
    assert len(t) == nt and len(rays) == 4096
    want, occ_want = checker.trace(s, t, rays)
    hits = int((want[:, 1].view(np.int32) == 2).sum())
    print("%s %d triangles: %d rays, triangle hits %d, occluded %d" % (kind, nt, len(rays), hits, int(occ_want.sum())))
    assert hits >= 50
    for env in (None, "SKR_NO_CULL"):
        with under(env, sc) as r:
            assert_bitwise(gpu_trace(r, rays), want, "%s %d under %s" % (kind, nt, env))
            assert np.array_equal(gpu_trace(r, rays, any_hit=True), occ_want), "%s %d any-hit under %s" % (kind, nt, env)
