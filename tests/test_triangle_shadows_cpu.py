"""Triangle shadows on the host (no GPU; include/skr.h skr_scene_set_triangle_shadows): the CPU checker pinned to the
frozen oracle while the switch is off, the ABI, the rule's clauses one by one on the checker, and the trace tree — the tree the shadow
walk runs on — held against shadow rays aimed at the borders of the accept regions."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import ROOT, scene_path
from oracle import pyoracle
from test_culling_host import sphere_culls, tree_parents, triangle_accepts
from test_shade_triangles import CASES, _write_mesh_scene
from triangle_shadow_check import LIGHT_POS, OCCLUDER, build as build_checker, moved, write_floor_scene

f32 = np.float32


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("trishadowcheck")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the checker is the oracle while the switch is off ----
def _same_as_the_oracle(checker, scn, w, h, kw):
    strict = kw.get("strict", False)
    sc = pyoracle.OracleScene(scn, strict=strict)
    opt = {k: v for k, v in kw.items() if k != "strict"}
    o_rgb, o_f, o_st = pyoracle.render(sc, w, h, want_float=True, shade_triangles=True, **opt)
    for switch in (False, True) if not opt.get("shadow") else (False,):  # (without --shadow the switch is a no-op: the same frame)
        rgb, f, st = checker.render(sc, w, h, triangle_shadows=switch, shade_triangles=True, **opt)
        assert np.array_equal(rgb, o_rgb) and np.array_equal(bits(f), bits(o_f))
        assert st.tolist() == o_st.tolist()
    return sc, opt, o_f, o_st


@pytest.mark.parametrize("name,scn,w,h,kw", CASES, ids=[c[0] for c in CASES])
def test_checker_is_the_oracle_while_the_switch_is_off(checker, name, scn, w, h, kw):
    sc, opt, o_f, o_st = _same_as_the_oracle(checker, scene_path(scn), w, h, kw)
    if name in ("test_gi4_shadow", "dragon_strict_gi2_d3"):  # and on caller rays: the frame's camera rays with keys y w + x
        from shade_query_check import camera_rays
        rays = camera_rays(sc, w, h, seed=opt.get("seed", 1))
        got, st = checker.shade(sc, rays, triangle_shadows=False, keys=np.arange(w * h), shade_triangles=True, **opt)
        assert np.array_equal(bits(got), bits(o_f).reshape(-1, 3)) and st.tolist() == o_st[:3].tolist()


@pytest.mark.parametrize("n_tris,n_spheres,kw", [(60, 4, dict(gillum=4, depth=3, shadow=True, seed=31)), (120, 6, dict(gillum=2, depth=6, shadow=True, seed=34))],
                         ids=["mesh60_gi4_d3", "mesh120_d6"])
def test_checker_is_the_oracle_on_random_meshes(checker, tmp_path, n_tris, n_spheres, kw):
    scn = str(tmp_path / "mesh.scn")
    _write_mesh_scene(scn, np.random.default_rng(n_tris), n_tris, n_spheres)
    _same_as_the_oracle(checker, scn, 96, 54, kw)


# ---- 2. header and library ----
def test_header_and_library():
    header = open(os.path.join(ROOT, "include", "skr.h")).read()
    assert re.search(r"#define SKR_HAS_TRIANGLE_SHADOWS 1\b", header) and re.search(r"#define SKR_SCN_TRIANGLE_SHADOWS 4u\b", header)
    assert re.search(r"#define SKR_ABI_VERSION 7\b", header)
    assert "int skr_scene_set_triangle_shadows(skr_scene *scene, int enable);" in header
    assert "int skr_scene_get_triangle_shadows(const skr_scene *scene, int *enabled);" in header
    out = subprocess.check_output(["nm", "-D", "--defined-only", skr.lib_path()], text=True)
    for name in ("skr_scene_set_triangle_shadows", "skr_scene_get_triangle_shadows", "skr_scene_get_trace_culling"):
        assert re.search(r" T %s\b" % name, out) and name in skr.EXPORTED_SYMBOLS
    assert C.sizeof(skr.binding.COptions) == 56
    assert skr.binding.SCN_TRIANGLE_SHADOWS == 4


def test_sizeof_options_from_the_header(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "skr.h"\n#include <stdio.h>\nint main(void) { printf("%zu %d %u %d", sizeof(skr_options), SKR_ABI_VERSION, SKR_SCN_TRIANGLE_SHADOWS, '
                   'SKR_HAS_TRIANGLE_SHADOWS); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    assert subprocess.check_output([exe], text=True).split() == ["56", "7", "4", "1"]


def test_loader_flag_setter_getter_and_from_arrays():
    assert skr.parse_scene(scene_path("test.scn")).triangle_shadows is False
    sc = skr.parse_scene(scene_path("test.scn"), triangle_shadows=True, strict=True)
    assert sc.triangle_shadows is True and sc.info.n_directional_lights == 1  # (the flags combine)
    sc.set_triangle_shadows(False)
    assert sc.triangle_shadows is False
    sc.set_triangle_shadows(True)
    assert sc.triangle_shadows is True
    spheres, tris, lights = sc.arrays()
    cam = list(sc.info.camera[:9])
    assert skr.Scene.from_arrays(spheres, tris, lights, cam).triangle_shadows is False
    assert skr.Scene.from_arrays(spheres, tris, lights, cam, triangle_shadows=True).triangle_shadows is True
    L = skr.lib()
    on = C.c_int(7)
    assert L.skr_scene_set_triangle_shadows(None, 1) == 2 and L.skr_scene_get_triangle_shadows(None, C.byref(on)) == 2
    assert L.skr_scene_get_triangle_shadows(sc.h, None) == 2


# ---- 3. the rule's clauses, on the checker ----
W, H = 64, 48
ON = dict(shade_triangles=True, shadow=True)


def _frames(checker, tmp_path, tris, light="point", materials=None, **kw):
    """the frame with the switch on, with it off, with the light removed, and without any triangle (floats)"""
    strict = light == "directional"
    opt = dict(ON, **kw)
    scn = write_floor_scene(str(tmp_path / "floor.scn"), tris, light=light, materials=materials)
    on = checker.render(scn, W, H, triangle_shadows=True, strict=strict, **opt)[1]
    off = checker.render(scn, W, H, triangle_shadows=False, strict=strict, **opt)[1]
    dark = checker.render(write_floor_scene(str(tmp_path / "dark.scn"), tris, light=None, materials=materials), W, H, triangle_shadows=False, **opt)[1]
    bare = checker.render(write_floor_scene(str(tmp_path / "bare.scn"), [], light=light), W, H, triangle_shadows=False, strict=strict, **opt)[1]
    return on, off, dark, bare


def _classes(on, off, dark, bare):
    """per pixel: equals the switch-off frame / equals the frame without the light; and the pixels that see the floor directly"""
    lit = (bits(on) == bits(off)).all(axis=2)
    unlit = (bits(on) == bits(dark)).all(axis=2)
    floor = (bits(off) == bits(bare)).all(axis=2) & (bare != np.array([.1, .2, .3], f32)).any(axis=2)
    return lit, unlit, floor


def test_every_pixel_is_lit_or_dark_and_both_occur(checker, tmp_path):
    """An occluded light adds nothing to sums that start at 0: the pixel is the one of the frame without the light, bit for bit."""
    for kw in (dict(), dict(gillum=None, jsample=0, depth=1)):
        lit, unlit, floor = _classes(*_frames(checker, tmp_path, [OCCLUDER], **kw))
        assert (lit | unlit).all()
        n = floor.sum()
        assert n > 0.5 * W * H
        only_lit, only_dark = (lit & ~unlit & floor).sum(), (unlit & ~lit & floor).sum()
        assert only_lit >= 0.05 * n and only_dark >= 0.05 * n, (only_lit, only_dark, n)


def test_a_triangle_beyond_the_light_or_behind_the_hit_casts_no_shadow(checker, tmp_path):
    above_light = moved(OCCLUDER, LIGHT_POS[1] + 5 - OCCLUDER[0][1])  # t >= dist for every shadow ray of the floor
    under_floor = moved(OCCLUDER, -8.0)                                # its plane lies behind every shading point: t <= 0
    for tri in (above_light, under_floor):
        on, off, dark, bare = _frames(checker, tmp_path, [tri])
        assert np.array_equal(bits(on), bits(off)) and not np.array_equal(bits(off), bits(dark))
    # a directional light has no far end: the triangle above where the point light was does shadow
    lit, unlit, floor = _classes(*_frames(checker, tmp_path, [above_light], light="directional"))
    assert (lit | unlit).all() and (unlit & ~lit & floor).sum() >= 0.05 * floor.sum() and (lit & ~unlit & floor).sum() >= 0.05 * floor.sum()


def test_a_triangle_does_not_shadow_itself(checker, tmp_path):
    """The own file index is excluded: a single triangle facing the light is lit, with the switch as without."""
    on, off, dark, bare = _frames(checker, tmp_path, [OCCLUDER])
    tri_pixels = (bits(off) != bits(bare)).any(axis=2) & (bits(off) != bits(dark)).any(axis=2)  # where the triangle is seen, and lit
    # (the floor pixels in its shadow differ from `bare` only with the switch on: they are not in `off != bare`)
    assert tri_pixels.sum() > 20
    assert np.array_equal(bits(on)[tri_pixels], bits(off)[tri_pixels])
    assert (on[tri_pixels] > dark[tri_pixels]).any(axis=1).all()


def test_coincident_triangles_follow_the_rule(checker, tmp_path):
    """Two coincident triangles under different materials (as test_shade_triangles._write_mesh_scene makes them): the earlier line is the
    surface, the later one an occluder candidate like any other triangle — at t = 0 up to rounding, so each shaded point is whatever
    `t > 0` gives for it.  The checker pins it (the GPU test compares whole frames against it); here: every pixel is in one of the
    two classes, and the floor's shadow is the single triangle's."""
    mats = ["material .5 .4 .3 .6 .5 .4 .3 .3 .3 4 0 0 0 1", "material .9 .1 .1 .9 .1 .1 .9 .9 .9 3 0 0 0 1"]
    on2, off2, dark2, bare = _frames(checker, tmp_path, [OCCLUDER, OCCLUDER], materials=mats)
    lit, unlit, floor = _classes(on2, off2, dark2, bare)
    assert (lit | unlit).all()
    on1, off1, dark1, _ = _frames(checker, tmp_path, [OCCLUDER])
    floor1 = _classes(on1, off1, dark1, bare)[2]
    assert np.array_equal(floor, floor1) and np.array_equal(bits(on2)[floor], bits(on1)[floor])


def test_the_switch_needs_shade_triangles_and_shadow(checker, tmp_path):
    scn = write_floor_scene(str(tmp_path / "floor.scn"), [OCCLUDER])
    for opt in (dict(shade_triangles=False, shadow=True), dict(shade_triangles=True, shadow=False), dict(shade_triangles=False, shadow=False, gillum=2, depth=2)):
        a = checker.render(scn, W, H, triangle_shadows=True, **opt)
        b = checker.render(scn, W, H, triangle_shadows=False, **opt)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2].tolist() == b[2].tolist()
    # counters: in force, the three of skr_renderer_read_counters and the sphere tests are what they are without the switch
    a = checker.render(scn, W, H, triangle_shadows=True, gillum=2, depth=3, **ON)
    b = checker.render(scn, W, H, triangle_shadows=False, gillum=2, depth=3, **ON)
    assert a[2].tolist() == b[2].tolist() and not np.array_equal(bits(a[1]), bits(b[1]))


# ---- 4. the trace tree holds for shadow rays ----
def _accept_region_hits(o, d, tris64, chunk=256):
    """For lines o + s d (float64 [n, 3]): s of their farthest crossing, on either side of o, of any accept region (v0, v0 - e1, v0 + e2);
    nan: none.  (Either side: the tree is about the line, and a hit point on the light's side of a triangle casts such a ray too.)"""
    v0, e1, e2 = tris64[:, 0, :3], -tris64[:, 1, :3], tris64[:, 2, :3]  # the region as an ordinary triangle (v0, v0 + e1', v0 + e2)
    best = np.full(o.shape[0], np.nan)
    for a in range(0, o.shape[0], chunk):
        oo, dd = o[a:a + chunk, None, :], d[a:a + chunk, None, :]
        p = np.cross(dd, e2[None])
        det = (e1[None] * p).sum(-1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = oo - v0[None]
            u = (tv * p).sum(-1) * inv
            q = np.cross(tv, e1[None])
            v = (dd * q).sum(-1) * inv
            s = (e2[None] * q).sum(-1) * inv
            ok = (np.abs(det) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (np.abs(s) > 1e-6)
        far = np.abs(np.where(ok, s, 0.0)).argmax(axis=1)
        s = np.where(ok, s, np.nan)[np.arange(s.shape[0]), far]
        best[a:a + chunk] = s
    return best


def _shadow_rays(rng, sc, tris, lights, n):
    """Shadow rays as the device forms them — o = P + 1e-6, L = normalize(Lp - P) (or the normalised direction of a directional light), in
    binary32 — aimed at points on or next to the border of randomly chosen accept regions: P is where the line from the light through
    the border point meets a surface of the scene (a sphere, else another accept region; behind the border point or in front of it), else
    a free point of that line inside the tree's ball.  lights: [n, 4] position | direction, w = 1 for a directional light.  Returns (triangle index, o, L, on a surface)."""
    nt = tris.shape[0]
    k = rng.integers(0, nt, n)
    t = tris[k].astype(np.float64)
    v0, e1, e2 = t[:, 0, :3], t[:, 1, :3], t[:, 2, :3]
    A, B, Cc = v0, v0 - e1, v0 + e2
    a = rng.random(n)[:, None]
    edge = rng.integers(0, 3, n)[:, None]
    X = np.where(edge == 0, A + a * (B - A), np.where(edge == 1, B + a * (Cc - B), Cc + a * (A - Cc)))
    centroid = (A + B + Cc) / 3
    off = (10.0 ** rng.uniform(-8, -0.3, n)) * rng.choice([-1.0, 1.0], n)
    X = X + off[:, None] * (centroid - X)
    lt = lights[rng.integers(0, lights.shape[0], n)].astype(np.float64)
    directional = lt[:, 3] != 0
    away = np.where(directional[:, None], -lt[:, :3], X - lt[:, :3])  # from the light through X
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    # where the line meets a surface behind X
    s_tri = _accept_region_hits(X, away, tris.astype(np.float64))
    s_sph = np.full(n, np.nan)
    spheres = sc.arrays()[0].astype(np.float64)
    for c in spheres:
        e = X - c[:3]
        b = (e * away).sum(1)
        disc = b * b - ((e * e).sum(1) - c[3] * c[3])
        with np.errstate(invalid="ignore"):
            s = -b - np.sqrt(disc)  # the crossing on the light's side: the lit side of the sphere
        s_sph = np.where((disc > 0) & (np.abs(s) > 1e-6) & ~np.isfinite(s_sph), s, s_sph)
    s_free = rng.uniform(0.01, 2.0, n) * np.maximum(np.linalg.norm(t[:, 1, :3], axis=1), 1e-3)
    surface = np.isfinite(s_sph) | np.isfinite(s_tri)
    s = np.where(np.isfinite(s_sph), s_sph, np.where(np.isfinite(s_tri), s_tri, s_free))
    P = (X + away * s[:, None]).astype(f32)
    o = P + f32(0.000001)
    with np.errstate(all="ignore"):
        to_l = np.where(directional[:, None], lt[:, :3].astype(f32), lt[:, :3].astype(f32) - P)
        ss = (to_l[:, 0] * to_l[:, 0] + to_l[:, 1] * to_l[:, 1]) + to_l[:, 2] * to_l[:, 2]
        L = to_l * (f32(1.0) / np.sqrt(ss))[:, None]
    return k, o, L.astype(f32), surface


def _directional_lights(path):
    return [[float(x) for x in ln.split()[4:7]] + [1.0] for ln in open(path) if ln.startswith("directional_light")]


@pytest.mark.parametrize("name", ["dragon.scn", "test.scn", "mesh"])
def test_no_accepted_shadow_pair_is_hidden_by_the_trace_tree(tmp_path, name):
    if name == "mesh":
        path = str(tmp_path / "mesh.scn")
        _write_mesh_scene(path, np.random.default_rng(60), 60, 4)
    else:
        path = scene_path(name)
    sc = skr.parse_scene(path, strict=True)
    cs, tris, sph, links, ch, ball = sc.trace_culling(0)
    cs0, tris0, _, links0, _ = sc.culling(0)
    assert cs == cs0 and np.array_equal(tris, tris0) and np.array_equal(links, links0)  # one topology, the radii of another origin class
    assert ball[3] > 0
    lights = np.array([list(l[3:6]) + [0.0] for l in sc.arrays()[2]] + _directional_lights(path), np.float64)
    assert len(lights) == sc.info.n_point_lights + sc.info.n_directional_lights > 0
    n = 20000
    k, o, L, surface = _shadow_rays(np.random.default_rng(11), sc, tris, lights, n)
    inside = ((o - ball[:3]).astype(np.float64) ** 2).sum(1) <= float(ball[3]) ** 2  # the wave walks the tree only for such origins
    assert inside.mean() > 0.9 and surface.mean() > 0.05, (inside.mean(), surface.mean())
    t = tris[k]
    acc = triangle_accepts(o, L, t[:, 0, :3], t[:, 1, :3], t[:, 2, :3]) & inside
    assert 0.05 * n < acc.sum() < 0.98 * n, "the sample must straddle the border (%d of %d accepted)" % (acc.sum(), n)
    assert (acc & surface).sum() > 0.01 * n
    parent, node_of_chunk = tree_parents(links)
    chunk = k // cs
    for cones in (True, False):
        hidden = acc & sphere_culls(o, L, ch[chunk], cones=cones)
        node = node_of_chunk[chunk]
        while np.any(node >= 0):
            live = node >= 0
            hidden[live] |= acc[live] & sphere_culls(o[live], L[live], sph[node[live]], cones=cones)
            node = np.where(live, parent[np.maximum(node, 0)], -1)
        assert not hidden.any(), "%d accepted (shadow ray, triangle) pairs would have been culled (cones=%s)" % (hidden.sum(), cones)
    if name == "dragon.scn":
        other = np.random.default_rng(3).integers(0, ch.shape[0], n)
        # not vacuous: the check above means something only if the spheres cull at all (the trace tree is looser than the renderer's —
        # its radii hold for an origin anywhere in the ball —, so no share is asked for beyond "a sizeable one")
        assert sphere_culls(o, L, ch[other]).mean() > 0.1, "the tree must actually cull"
