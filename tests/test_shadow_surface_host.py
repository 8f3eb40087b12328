"""Host logic of the shadow masks' surface patches (csrc/scene_host.cpp build_shadow_surface, DESIGN.md "Shadow surface patches") — no GPU.

A shading point P of the level pipelines is a hit point of some sphere s; the node pipeline keys it to the cell of e = P - C_s in a
cube map on that sphere when the device's fl(|e|^2) - r_s^2 is within the sphere's radial slack, and reads ONE word there: the union,
over the pair of lights, of the spheres that may be candidates of a shadow ray from that patch (shade_common.h shadow_cands).
Otherwise it takes the two direction masks.  These tests restate that lookup in numpy binary32 and check, on points at patch corners
and borders, at radial offsets across the slack, at the own sphere's terminator and aimed so that the shadow ray grazes another
sphere, that no candidate (D >= 0 and b < 0 in the device's test, either light of the pair) is ever missing from its word.
"""
import ctypes as C
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path
from test_gi_surface_cells_host import cube_cell_n
from test_shadow_masks_host import _dot, _perp, _unit, candidates, device_cell

f32 = np.float32
SLACK = f32(2.0 ** -7)  # shadow_cells.h SKR_SURFACE_SLACK


class Patches:
    """The pairs' tables and the spheres' header words (skr_scene_get_shadow_surface, internal), with the margins scaled where asked."""

    def __init__(self, sc, rho_scale=1.0, cone_scale=1.0):
        L = skr.lib()
        if (rho_scale, cone_scale) != (1.0, 1.0):
            fn = L.skr_scene_rebuild_shadow_surface
            fn.argtypes = [C.c_void_p, C.c_double, C.c_double]
            assert fn(sc.h, rho_scale, cone_scale) == 0
        s, _, l = sc.arrays()
        self.geom = np.array([[x[0], x[1], x[2], f32(x[3]) * f32(x[3])] for x in s], f32).reshape(-1, 4)
        self.lp = l[:, :3].astype(f32)
        ns = len(self.geom)
        fn = L.skr_scene_get_shadow_surface
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
        npairs, stride = C.c_int32(), C.c_int32()
        assert fn(sc.h, C.byref(npairs), C.byref(stride), None, None) == 0
        self.npairs, self.stride = npairs.value, stride.value
        head = np.zeros(max(ns, 1), np.uint32)
        self.t = np.zeros(self.npairs * self.stride, np.uint32)
        if self.npairs:
            assert fn(sc.h, None, None, head.ctypes.data, self.t.ctypes.data) == 0
        self.base, self.G = (head & 0xFFFFFF).astype(np.int64)[:ns], (head >> 24).astype(np.int64)[:ns]
        self.sc = sc

    def lookup(self, s, P, pair):
        """shade_common.h shadow_cands, the patch path: (the pair's word, whether the lane takes it)."""
        g = self.geom[s]
        with np.errstate(all="ignore"):
            e = P - g[:, :3]
            c = _dot(e, e) - g[:, 3]
            ok = (self.G[s] != 0) & (np.abs(c) <= g[:, 3] * SLACK)
        cell = cube_cell_n(np.where(ok[:, None], e, f32(1)), np.maximum(self.G[s], 1))
        return self.t[np.where(ok, pair * self.stride + self.base[s] + cell, 0)], ok

    def direction_masks(self, P, pair):
        """The union of the two direction masks of the pair (shade_common.h shadow_mask_of); every sphere outside the reach."""
        masks, reach2 = self.sc.shadow_masks()
        ns, nl = len(self.geom), len(self.lp)
        out = np.zeros(len(P), np.uint32)
        for l in (2 * pair, 2 * pair + 1):
            if l >= nl:
                continue
            v = self.lp[l] - P
            face, i, j = device_cell(v)
            vv = _dot(v, v)
            out |= np.where((vv <= f32(reach2)) & (vv >= f32(2.0 ** -98)), masks[l, face, i, j], np.uint32((1 << ns) - 1))
        return out


def check(pt, s, P, light, k, what):
    """Every candidate (P on sphere s, light, sphere k) of a lane that takes the patch path is named.  Returns (candidates checked, missing)."""
    P = P.astype(f32)
    cand, _, _ = candidates(P, pt.lp[light], pt.geom[k])
    word, used = pt.lookup(s, P, light >> 1)
    missing = cand & used & (((word >> k.astype(np.uint32)) & 1) == 0)
    return int((cand & used).sum()), missing, "%s: %d of %d candidates missing from their words" % (what, missing.sum(), (cand & used).sum())


def surface_points(pt, rng, n):
    """P on the spheres, for sphere s, light `light` and tested sphere k, of four kinds: (0) patch corners, borders and insides (face
    coordinates a few ulps either side of a border), (1) the own sphere's terminator for the light, (2) where a line through the light that
    grazes sphere k meets sphere s, (3) anywhere; then at radial offsets across the whole slack."""
    geom, lp = pt.geom.astype(np.float64), pt.lp.astype(np.float64)
    ns, nl = len(geom), len(lp)
    has = np.nonzero(pt.G > 0)[0]
    s = has[rng.integers(0, len(has), n)]
    light, k = rng.integers(0, nl, n), rng.integers(0, ns, n)
    kind = rng.integers(0, 4, n)
    k = np.where(kind == 1, s, k)
    Cs, rs = geom[s, :3], np.sqrt(geom[s, 3])
    # (0) cells of the cube map
    G = pt.G[s]
    face = rng.integers(0, 6, n)
    ij = rng.random((n, 2)) * G[:, None]
    border = rng.random((n, 2)) < 0.6
    ij = np.where(border, rng.integers(0, G[:, None] + 1, (n, 2)), ij)
    fc = ij * (2.0 / G[:, None]) - 1.0 + np.where(border, rng.integers(-6, 7, (n, 2)) * 2.0 ** -24, 0.0)
    ax = face >> 1
    u0 = np.zeros((n, 3))
    u0[np.arange(n), ax] = np.where(face & 1, -1.0, 1.0)
    u0[np.arange(n), np.where(ax == 0, 1, 0)] = fc[:, 0]
    u0[np.arange(n), np.where(ax == 2, 1, 2)] = fc[:, 1]
    u0 = _unit(u0)
    # (1) the terminator: the angle between u and the direction to the light is acos(r / |Lp - C|), +- a little
    to_l = lp[light] - Cs
    dl = np.linalg.norm(to_l, axis=1)
    ang = np.arccos(np.minimum(1.0, rs / np.maximum(dl, 1e-30))) + rng.normal(size=n) * 10.0 ** rng.uniform(-7, -2, n)
    u1 = _unit(to_l) * np.cos(ang)[:, None] + _perp(to_l, rng) * np.sin(ang)[:, None]
    # (2) a grazing line of sphere k through the light, cut with sphere s
    q = geom[k, :3] - lp[light]
    qn = np.linalg.norm(q, axis=1)
    ga = np.arcsin(np.minimum(1.0, np.sqrt(geom[k, 3]) / np.maximum(qn, 1e-30))) * (1 + rng.choice([-1, 1], n) * 2.0 ** -rng.integers(4, 30, n))
    w = _unit(q) * np.cos(ga)[:, None] + _perp(q, rng) * np.sin(ga)[:, None]
    m = lp[light] - Cs
    bq = np.einsum("ij,ij->i", m, w)
    disc = bq * bq - (np.einsum("ij,ij->i", m, m) - rs * rs)
    t = -bq + rng.choice([-1.0, 1.0], n) * np.sqrt(np.maximum(disc, 0.0))
    u2 = m + w * t[:, None]
    meets = (disc > 0) & (kind == 2) & (np.linalg.norm(u2, axis=1) > 0)
    u3 = _unit(rng.normal(size=(n, 3)))
    u = np.where((kind == 0)[:, None], u0, np.where((kind == 1)[:, None], u1, np.where(meets[:, None], _unit(np.where(meets[:, None], u2, 1.0)), u3)))
    tau = geom[s, 3] * float(SLACK)
    off = np.where(rng.random(n) < 0.5, rng.uniform(-1, 1, n), rng.choice([-1, 1], n) * (1 - 1e-3)) * 0.5 * tau / rs
    off = np.where(rng.random(n) < 0.5, 0.0, off)
    P = Cs + u * (rs + off)[:, None]
    return P.astype(f32), s, light, k


def sweep(sc, seed, n, what, rho_scale=1.0, cone_scale=1.0):
    """(the patches, candidates checked, candidates missing) over three draws of n points"""
    pt = Patches(sc, rho_scale, cone_scale)
    assert pt.npairs == (len(pt.lp) + 1) // 2 and pt.stride > 0, "%s: no surface patches" % what
    assert len(pt.t) * 4 <= 1 << 20
    rng = np.random.default_rng(seed)
    total = lost = 0
    msg = ""
    for _ in range(3):
        P, s, light, k = surface_points(pt, rng, n)
        for kk in (k, rng.integers(0, len(pt.geom), n)):
            nc, missing, m = check(pt, s, P, light, kk, what)
            total += nc
            if missing.any():
                lost += int(missing.sum())
                i = np.nonzero(missing)[0][0]
                msg = "%s, e.g. s=%d P=%r light %d sphere %d" % (m, s[i], P[i], light[i], kk[i])
    return pt, total, lost, msg


def test_patches_name_every_candidate_of_spheres2():
    pt, total, lost, msg = sweep(skr.parse_scene(scene_path("spheres2.scn")), 71, 60000, "spheres2")
    assert lost == 0, msg
    assert total > 10000, total  # (the points reach candidates)
    # the table is what the device reads: direct addressing, every sphere's cells behind the last one's, no word beyond the spheres' bits
    assert (pt.G >= 1).all() and pt.G[0] > pt.G[1:].max()  # (the ground's patches are its own size, not the small spheres')
    assert np.array_equal(pt.base, np.concatenate([[0], np.cumsum(6 * pt.G * pt.G)[:-1]])) and pt.stride == (6 * pt.G * pt.G).sum()
    assert (pt.t >> np.uint32(len(pt.geom))).max() == 0
    print("spheres2: G = %s, %d bytes" % (pt.G.tolist(), len(pt.t) * 4))


def _random_scene(path, rng, n, nl, light_inside=False):
    """A ground-like sphere and n - 1 spheres of mixed sizes over it, nl point lights (one of them inside a sphere where asked)."""
    lines = ["camera 0 2 -10 0 -.1 .9 0 1 0 30", "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1",
             "sphere %.7g %.7g %.7g %.7g" % (rng.uniform(-3, 3), -40 * rng.uniform(0.5, 2), rng.uniform(-3, 3), 40 * rng.uniform(0.5, 2))]
    spheres = []
    for _ in range(n - 1):
        spheres.append((rng.uniform(-5, 5), rng.uniform(0, 3), rng.uniform(-5, 5), 10.0 ** rng.uniform(-1.5, 0.3)))
        lines.append("sphere %.7g %.7g %.7g %.7g" % spheres[-1])
    for i in range(nl):
        lp = np.array([rng.uniform(-6, 6), rng.uniform(3, 10), rng.uniform(-6, 6)])
        if light_inside and i == 0:
            c = spheres[0]
            lp = np.array(c[:3]) + rng.normal(size=3) * 0.2 * c[3]
        lines.append("point_light .8 .8 .8 %.7g %.7g %.7g" % tuple(lp))
    open(path, "w").write("\n".join(lines) + "\n")


@pytest.mark.parametrize("nl", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 9, 16, 17, 32])
def test_random_scenes_patches_name_every_candidate(tmp_path, n, nl):
    rng = np.random.default_rng(5100 + 10 * n + nl)
    path = os.path.join(str(tmp_path), "s.scn")
    _random_scene(path, rng, n, nl)
    _, total, lost, msg = sweep(skr.parse_scene(path), 80 + n, 15000, "random %d spheres %d lights" % (n, nl))
    assert lost == 0, msg
    assert total > 1000, total


def test_light_inside_a_sphere(tmp_path):
    rng = np.random.default_rng(77)
    path = os.path.join(str(tmp_path), "s.scn")
    _random_scene(path, rng, 6, 2, light_inside=True)
    pt, total, lost, msg = sweep(skr.parse_scene(path), 78, 30000, "light inside a sphere")
    assert lost == 0, msg
    assert total > 1000, total
    # from the inside of that sphere's surface the light is seen through the sphere itself: some patch names its own sphere
    own = pt.t[pt.base[1]:pt.base[1] + 6 * pt.G[1] ** 2]
    assert ((own >> np.uint32(1)) & 1).any()


def test_no_patches_where_the_plain_loop_must_run(tmp_path):
    lines = ["camera 0 0 -8 0 0 1 0 1 0 30", "point_light 1 1 1 0 5 0"]
    lines += ["sphere %d 0 %d .3" % (i % 7, i // 7) for i in range(33)]
    path = str(tmp_path / "many.scn")
    open(path, "w").write("\n".join(lines) + "\n")
    assert Patches(skr.parse_scene(path)).npairs == 0  # more than 32 spheres
    assert Patches(skr.parse_scene(scene_path("spheres2.scn"), strict=True)).npairs == 0  # a directional light
    assert Patches(skr.parse_scene(scene_path("spheres2.scn"))).npairs == 1


@pytest.mark.parametrize("which", ["rho", "cone"])
def test_shrunk_margins_lose_candidates(which):
    """The margins are needed: with the patch ball, or the cone of light directions, at 0.8 of itself candidates go missing."""
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    _, total, lost, _ = sweep(sc, 71, 60000, "spheres2 shrunk", 0.8 if which == "rho" else 1.0, 0.8 if which == "cone" else 1.0)
    assert total > 10000 and lost > 0, (total, lost)


def hit_like_points(pt, rng, n):
    """Shading points of spheres2's tree, roughly: on the spheres' surfaces, half of them on the ground in front of the camera, the
    others on the upper halves of the small spheres (the hits a path from the camera and from the ground's hemisphere finds)."""
    geom = pt.geom.astype(np.float64)
    ns = len(geom)
    ground = rng.random(n) < 0.5
    s = np.where(ground, 0, rng.integers(1, ns, n))
    Cs, r = geom[s, :3], np.sqrt(geom[s, 3])
    u = _unit(rng.normal(size=(n, 3)))
    u[:, 1] = np.where(rng.random(n) < 0.8, np.abs(u[:, 1]), u[:, 1])
    gp = np.stack([rng.uniform(-14, 14, n), np.zeros(n), rng.uniform(-8, 14, n)], -1)
    u = np.where(ground[:, None], _unit(gp - Cs), u)
    return (Cs + u * r[:, None]).astype(f32), s


def test_headline_lanes_name_fewer_spheres():
    """The gate of the issue: for spheres2 hit-like points in random batches of 64, the spheres a lane's shadow pair walk names (lane
    mean) and the busiest lane's, for the direction masks and for the patches.  Measured: see the print; DESIGN.md records the pair."""
    pt = Patches(skr.parse_scene(scene_path("spheres2.scn")))
    rng = np.random.default_rng(23)
    n = 64 * 2000
    P, s = hit_like_points(pt, rng, n)
    zero = np.zeros(n, np.int64)
    word, used = pt.lookup(s, P, zero)
    dirs = pt.direction_masks(P, 0)
    pop = lambda m: np.array([bin(int(x)).count("1") for x in m]).reshape(-1, 64)
    out = {"direction masks": pop(dirs), "patches": pop(np.where(used, word, dirs))}
    res = {k: (float(v.mean()), float(v.max(-1).mean())) for k, v in out.items()}
    print("shadow pair walk, spheres per call (lane mean, busiest of 64): %r; lanes on the patch path %.4f" % (res, used.mean()))
    assert used.mean() > 0.99
    assert res["patches"][0] < res["direction masks"][0] and res["patches"][1] < res["direction masks"][1], res
