"""Ray queries on the host (no GPU): the CPU checker of include/skr.h skr_trace_rays pinned on hand-built scenes whose answers are
known, and the ABI the queries add (DESIGN.md "Ray queries")."""
import math
import os
import re

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import ROOT
from ray_query_check import build as build_checker, pack_rays

NO_SPHERES = np.zeros((0, 14), np.float32)
NO_TRIANGLES = np.zeros((0, 9), np.float32)


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("raycheck")))


def sphere(x, y, z, r):
    s = np.zeros(14, np.float32)
    s[:4] = (x, y, z, r)
    return s


def tri_at(z):
    """A triangle in the plane z whose accept region (v0, v0 - e1, v0 + e2: utils.h:181-213 flips the sign of u) covers (-1, 1)."""
    return np.array([0, 0, z, 4, 0, z, 0, 4, z], np.float32)


def one(checker, spheres, triangles, o, d, tmax=None, ignore=None):
    hits, occ = checker.trace(np.array(spheres, np.float32).reshape(-1, 14), np.array(triangles, np.float32).reshape(-1, 9),
                              pack_rays([o], [d], tmax, ignore))
    h = hits[0]
    return float(h[0]), int(h[1:2].view(np.int32)[0]), int(h[2:3].view(np.int32)[0]), h[3:6].copy(), int(occ[0]), h


def test_ray_through_a_sphere_centre(checker):
    t, kind, index, n, occ, h = one(checker, [sphere(5, 0, 0, 9), sphere(0, 0, 10, 1)], NO_TRIANGLES, (0, 0, 0), (0, 0, 1))
    # sphere 0 contains the origin: its near root is negative, so it is never accepted (raytrace.h:152-165); sphere 1 at t = 9
    assert (t, kind, index, occ) == (9.0, 1, 1, 1)
    assert n.tolist() == [0.0, 0.0, -1.0]
    assert h[6:8].view(np.int32).tolist() == [0, 0]
    # the direction need not be unit length: t is in units of d
    t2, kind2, index2, n2, _, _ = one(checker, [sphere(0, 0, 10, 1)], NO_TRIANGLES, (0, 0, 0), (0, 0, 2))
    assert (t2, kind2, index2) == (4.5, 1, 0) and n2.tolist() == [0.0, 0.0, -1.0]


def test_miss_layout(checker):
    t, kind, index, n, occ, h = one(checker, [sphere(0, 0, 10, 1)], [tri_at(5)], (0, 0, 0), (0, 0, -1))
    assert math.isinf(t) and t > 0 and (kind, index, occ) == (0, -1, 0)
    assert n.tolist() == [0.0, 0.0, 0.0] and h[6:8].view(np.int32).tolist() == [0, 0]


def test_near_sphere_hits_rejected_but_near_triangles_accepted(checker):
    # from (0, 0, 8.5) the near root of the sphere is t = 0.5 <= 1: rejected, and the far root is never taken -> a miss
    t, kind, _, _, occ, _ = one(checker, [sphere(-1, 1, 10, 1)], NO_TRIANGLES, (-1, 1, 8.5), (0, 0, 1))
    assert (kind, occ) == (0, 0)
    # a triangle at t = 0.5 is accepted (t > 0)
    t, kind, index, n, occ, _ = one(checker, [sphere(-1, 1, 10, 1)], [tri_at(9)], (-1, 1, 8.5), (0, 0, 1))
    assert (t, kind, index, occ) == (0.5, 2, 0, 1)
    assert n.tolist() == [0.0, 0.0, -1.0]  # the geometric normal (0, 0, 1) turned against the ray
    # but not one behind the origin (t < 0), nor at t = 0
    assert one(checker, NO_SPHERES, [tri_at(8)], (-1, 1, 8.5), (0, 0, 1))[1] == 0
    assert one(checker, NO_SPHERES, [tri_at(8.5)], (-1, 1, 8.5), (0, 0, 1))[1] == 0


def test_sphere_triangle_tie_goes_to_the_sphere(checker):
    o, d = (-1, 1, 0), (0, 0, 1)
    ts = one(checker, [sphere(-1, 1, 10, 1)], NO_TRIANGLES, o, d)[0]
    tt = one(checker, NO_SPHERES, [tri_at(9)], o, d)[0]
    assert ts == tt == 9.0
    t, kind, index, _, _, _ = one(checker, [sphere(-1, 1, 10, 1)], [tri_at(9)], o, d)
    assert (t, kind, index) == (9.0, 1, 0)
    # a triangle strictly nearer wins
    t, kind, index, _, _, _ = one(checker, [sphere(-1, 1, 10, 1)], [tri_at(9.5), tri_at(8.75)], o, d)
    assert (t, kind, index) == (8.75, 2, 1)


def test_triangle_triangle_tie_goes_to_the_lower_index(checker):
    o, d = (-1, 1, 0), (0, 0, 1)
    tris = [tri_at(12), tri_at(7), tri_at(7)]
    t, kind, index, _, _, _ = one(checker, NO_SPHERES, tris, o, d)
    assert (t, kind, index) == (7.0, 2, 1)
    # the ray may not hit the triangle it leaves: then the other of the two
    assert one(checker, NO_SPHERES, tris, o, d, ignore=1)[:3] == (7.0, 2, 2)
    assert one(checker, NO_SPHERES, tris, o, d, ignore=2)[:3] == (7.0, 2, 1)


def test_ignore_triangle(checker):
    o, d = (-1, 1, 0), (0, 0, 1)
    tris = [tri_at(5), tri_at(6)]
    assert one(checker, NO_SPHERES, tris, o, d)[:3] == (5.0, 2, 0)
    assert one(checker, NO_SPHERES, tris, o, d, ignore=0)[:3] == (6.0, 2, 1)
    t, kind, index, _, occ, _ = one(checker, NO_SPHERES, [tri_at(5)], o, d, ignore=0)
    assert (kind, index, occ) == (0, -1, 0)


def test_tmax_equal_to_the_hit_is_a_miss(checker):
    o, d = (0, 0, 0), (0, 0, 1)
    for spheres, tris in (([sphere(0, 0, 10, 1)], NO_TRIANGLES), (NO_SPHERES, [tri_at(9)])):
        o2 = (-1, 1, 0) if len(tris) else o
        t = one(checker, spheres, tris, o2, d)[0]
        assert t == 9.0
        assert one(checker, spheres, tris, o2, d, tmax=t)[1] == 0
        assert one(checker, spheres, tris, o2, d, tmax=t)[4] == 0
        assert one(checker, spheres, tris, o2, d, tmax=np.nextafter(np.float32(t), np.float32(np.inf)))[1] != 0
        assert one(checker, spheres, tris, o2, d, tmax=np.nextafter(np.float32(t), np.float32(np.inf)))[4] == 1
    # a nearer winner beyond tmax hides a farther surface too: the result is a miss, not the next hit
    assert one(checker, [sphere(-1, 1, 10, 1)], [tri_at(20)], (-1, 1, 0), d, tmax=5.0)[1] == 0


def test_any_hit_agrees_with_closest_hit_on_random_rays(checker):
    rng = np.random.default_rng(3)
    spheres = np.array([sphere(*rng.uniform(-3, 3, 3), rng.uniform(0.3, 1.5)) for _ in range(6)])
    tris = rng.uniform(-3, 3, (20, 9)).astype(np.float32)
    n = 4000
    rays = pack_rays(rng.uniform(-5, 5, (n, 3)), rng.normal(size=(n, 3)), rng.choice([np.inf, 2.0, 0.5], n), rng.integers(-1, 20, n))
    hits, occ = checker.trace(spheres, tris, rays)
    kind = hits[:, 1].view(np.int32)
    assert np.array_equal(occ, (kind != 0).astype(np.int32))
    assert 0 < (kind == 1).sum() and 0 < (kind == 2).sum() and 0 < (kind == 0).sum()


def test_abi_declares_the_ray_queries():
    header = open(os.path.join(ROOT, "include", "skr.h")).read()
    assert re.search(r"#define SKR_ABI_VERSION 7\b", header)
    assert "skr_trace_rays" in skr.EXPORTED_SYMBOLS and "skr_camera_rays" in skr.EXPORTED_SYMBOLS
    assert skr.TRACE_ANY_HIT == 1
    L = skr.lib()
    L.skr_trace_rays, L.skr_camera_rays


def test_trace_rejects_bad_arguments_without_a_device():
    L = skr.lib()
    # a null renderer is an argument error before any device is touched
    out = np.zeros(16, np.float32)
    assert L.skr_trace_rays(None, out.ctypes.data, 1, 0, out.ctypes.data, None) == 2
    assert L.skr_camera_rays(None, None, 0, out.ctypes.data, None) == 2
