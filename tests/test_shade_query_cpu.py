"""Shading queries on the host (no GPU; include/skr.h skr_shade_rays): the CPU checkers pinned to the frozen oracle
on a frame's own camera rays, bit for bit with counts, in every mode; the tmax rule on hand-built rays; and the ABI."""
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import ROOT, scene_path
from oracle import pyoracle
from ray_query_check import pack_rays
from shade_query_check import build as build_checker, camera_rays

W, H = 64, 36


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("shadecheck")))


MODES = {
    "direct": ("spheres2.scn", dict()),
    "direct_shadow": ("spheres2.scn", dict(shadow=True)),
    "gillum_depth3": ("spheres2.scn", dict(gillum=4, depth=3, shadow=True)),
    "strict_scn": ("spheres2.scn", dict(gillum=2, depth=2, shadow=True, strict=True)),
    "mesh_black": ("test.scn", dict(gillum=2, depth=3)),
    "shade_triangles": ("test.scn", dict(gillum=2, depth=3, shade_triangles=True)),
    "legacy_reflect": ("spheres2.scn", dict(depth=3, legacy_reflect=True, shadow=True)),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_camera_rays_reproduce_the_oracle_frame(checker, mode):
    name, kw = MODES[mode]
    strict = kw.pop("strict", False) if "strict" in kw else False
    kw = dict(kw, seed=5)
    sc = pyoracle.OracleScene(scene_path(name), strict=strict)
    _, want, st = pyoracle.render(sc, W, H, want_float=True, **kw)
    rays = camera_rays(sc, W, H, seed=5)
    keys = np.arange(W * H, dtype=np.uint32)
    got, stats = checker.shade(sc, rays, keys=keys, **kw)
    assert np.array_equal(got.view(np.uint32), want.reshape(-1, 3).view(np.uint32)), mode
    assert stats.tolist() == [int(st[0]), int(st[1]), int(st[2])]
    # keys = None is the ray index: the same keys here
    again, _ = checker.shade(sc, rays, **kw)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_camera_rays_reproduce_the_fog_frame(checker):
    from fog_check import build as build_fog
    fog = skr.parse_scene(scene_path("spheres2.scn"), fog=True).fog
    assert len(fog) == 1
    fc = build_fog(os.path.dirname(checker.plain._name))
    kw = dict(gillum=2, depth=2, shadow=True, seed=3)
    _, want, st = fc.render(scene_path("spheres2.scn"), W, H, fog, **kw)
    sc = pyoracle.OracleScene(scene_path("spheres2.scn"))
    got, stats = checker.shade(sc, camera_rays(sc, W, H, seed=3), keys=np.arange(W * H), fog=fog, **kw)
    assert np.array_equal(got.view(np.uint32), want.reshape(-1, 3).view(np.uint32))
    assert stats.tolist() == [int(x) for x in st]
    plain, _ = checker.shade(sc, camera_rays(sc, W, H, seed=3), keys=np.arange(W * H), **kw)
    assert not np.array_equal(plain, got), "the fog must change the frame"


def test_jittered_sample_and_keys(checker):
    """Sample s of a --jsample frame: the oracle's sum of its samples, in sample order, divided by g*g."""
    sc = pyoracle.OracleScene(scene_path("spheres2.scn"))
    kw = dict(gillum=2, depth=2, seed=8)
    _, want, st = pyoracle.render(sc, 24, 16, want_float=True, jsample=2, **kw)
    acc = np.zeros((24 * 16, 3), np.float32)
    rays_total = 0
    for s in range(4):
        v, stats = checker.shade(sc, camera_rays(sc, 24, 16, jsample=2, seed=8, sample=s), sample=s, keys=np.arange(24 * 16), **kw)
        acc = acc + v
        rays_total += int(stats[0])
    assert np.array_equal((acc / np.float32(4.0)).view(np.uint32), want.reshape(-1, 3).view(np.uint32))
    assert rays_total == int(st[0])


def test_tmax_cuts_the_first_segment_only(checker):
    sc = pyoracle.OracleScene(scene_path("spheres2.scn"))
    bg = np.array([sc.s.background.x, sc.s.background.y, sc.s.background.z], np.float32)
    # from the camera towards the green sphere (centre (0, 1.25, 0), radius 1): the near hit is at t = 9 for a unit direction
    o = np.array([[0, 1.25, -10]] * 4, np.float32)
    d = np.array([[0, 0, 1]] * 4, np.float32)
    tmax = np.array([np.inf, 9.0, np.nextafter(np.float32(9.0), np.float32(10)), 2.0], np.float32)
    out, stats = checker.shade(sc, pack_rays(o, d, tmax), keys=[7] * 4, gillum=2, depth=3, shadow=True)
    assert not np.array_equal(out[0], bg) and np.array_equal(out[2], out[0]), "tmax past the winner: the frame's value"
    assert np.array_equal(out[1], bg) and np.array_equal(out[3], bg), "the winner at or beyond tmax: a miss"
    # the two misses are one radiance ray each; the two hits trace their children as in a frame
    _, one = checker.shade(sc, pack_rays(o[:1], d[:1]), keys=[7], gillum=2, depth=3, shadow=True)
    assert int(stats[0]) == 2 * int(one[0]) + 2


def test_mesh_black_and_ignore_triangle(checker, tmp_path):
    """A triangle in front of a sphere blackens the ray (HEAD rule) unless tmax lies before it; under --shade-triangles the triangle the
    ray starts on is skipped."""
    scn = tmp_path / "wall.scn"
    scn.write_text("camera 0 0 -10 0 0 1 0 1 0 30\nbackground .1 .2 .3\nmaterial .5 .5 .5 .5 .5 .5 .2 .2 .2 16 0 0 0 1\n"
                   "sphere 0 0 10 1\npoint_light 10 10 10 0 5 0\nambient_light .3 .3 .3\nmax_vertices 3\nvertex 0 0 5\nvertex 4 0 5\n"
                   "vertex 0 4 5\ntriangle 0 1 2\n")
    sc = pyoracle.OracleScene(str(scn))
    assert sc.s.n_triangles == 1
    o = np.array([[-0.5, 0.5, 0]] * 3 + [[-0.5, 0.5, 5]], np.float32)
    d = np.array([[0, 0, 1]] * 4, np.float32)
    rays = pack_rays(o, d, [np.inf, 4.0, 6.0, np.inf], [-1, -1, -1, 0])
    out, _ = checker.shade(sc, rays)
    assert out[0].tolist() == [0, 0, 0]
    assert np.allclose(out[1], [0.1, 0.2, 0.3]) and out[2].tolist() == [0, 0, 0]
    tri, _ = checker.shade(sc, rays, shade_triangles=True)
    assert tri[0].tolist() != [0, 0, 0] and np.allclose(tri[1], [0.1, 0.2, 0.3])
    assert tri[3].tolist() != tri[0].tolist(), "from the wall, ignoring it, the sphere behind it is shaded"


def test_abi_declares_the_shading_query():
    header = open(os.path.join(ROOT, "include", "skr.h")).read()
    assert "int skr_shade_rays(skr_renderer *r, const skr_options *opt, const skr_ray *d_rays, uint32_t n," in header
    assert "skr_shade_rays" in skr.EXPORTED_SYMBOLS
    L = skr.lib()
    out = np.zeros(16, np.float32)
    opt = skr.Options(8, 8)
    import ctypes as C
    # a null renderer or array is an argument error before any device is touched
    assert L.skr_shade_rays(None, C.byref(opt.c), out.ctypes.data, 1, 0, None, out.ctypes.data, None) == 2
    assert L.skr_shade_rays(None, None, None, 0, 0, None, None, None) == 2
    assert callable(skr.Renderer.shade)
