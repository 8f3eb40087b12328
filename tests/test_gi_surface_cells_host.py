"""Host logic of the GI masks' surface patches (csrc/scene_host.cpp build_gi_surface, DESIGN.md "GI surface patches") — no GPU.

A GI origin is a hit point of some sphere s; the node pipeline keys it to the cell of e = o - C_s in a cube map on that sphere when the
device's fl(|e|^2) - r_s^2 is within the sphere's radial slack, and to the grids' row otherwise (shade_common.h gi_surface_row).
These tests restate that lookup in numpy binary32 and check, on origins at patch corners and borders, at radial offsets up to the
slack, aimed at grazing lines (of the origin's own sphere too) and at direction-cell borders, on spheres2 and on random scenes of
1-32 spheres, that no candidate (D >= 0 and b < 0 in the device's test) is ever missing from its mask.  They also report, for
hit-point-like GI rays of spheres2, how many spheres a lane names and how many the busiest lane of 64 names, for both tables.
"""
import ctypes as C
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path
from test_gi_masks_host import Table, _dot, _perp, _random_scene, _unit, aimed_rays, candidates

f32 = np.float32
HEAD = 4  # shadow_cells.h SKR_GI_SURFACE_HEAD


def cube_cell_n(v, N):
    """shade_common.h cube_cell_n (exact division for v_rcp_f32: the host widens every cell by far more than the difference)."""
    a = np.abs(v)
    fx = (a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2])
    fy = ~fx & (a[:, 1] >= a[:, 2])
    m = np.where(fx, a[:, 0], np.where(fy, a[:, 1], a[:, 2]))
    lead = np.where(fx, v[:, 0], np.where(fy, v[:, 1], v[:, 2]))
    ca = np.where(fx, v[:, 1], v[:, 0])
    cb = np.where(fx | fy, v[:, 2], v[:, 1])
    face = np.where(fx, 0, np.where(fy, 2, 4)) + (lead < 0)
    h = (f32(0.5) * N.astype(f32)).astype(f32)
    with np.errstate(all="ignore"):
        inv = f32(1) / m
        i = np.fmin(np.fmax((ca * inv) * h + h, f32(0)), (N - 1).astype(f32)).astype(np.int64)
        j = np.fmin(np.fmax((cb * inv) * h + h, f32(0)), (N - 1).astype(f32)).astype(np.int64)
    return (face * N + i) * N + j


class Surface:
    """The grids (test_gi_masks_host.Table) and the surface patches behind them (skr_scene_get_gi_surface, internal)."""

    def __init__(self, sc):
        self.tab = Table(sc)
        L = skr.lib()
        fn = L.skr_scene_get_gi_surface
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
        nw, hw, fr = C.c_int32(), C.c_int32(), C.c_int32()
        assert fn(sc.h, C.byref(nw), C.byref(hw), C.byref(fr), None) == 0
        self.t = np.zeros(nw.value, np.uint32)
        assert fn(sc.h, None, None, None, self.t.ctypes.data) == 0
        self.first_row, self.hw = fr.value, hw.value
        ns = len(self.tab.geom)
        self.masks = self.t[:self.hw] if self.tab.wide else self.t[:self.hw].view(np.uint16)
        self.words = self.t[self.hw:]
        head = self.words[:HEAD * ns].reshape(ns, HEAD) if len(self.t) else np.zeros((ns, HEAD), np.uint32)
        self.at, self.G, self.tau = head[:, 0].astype(np.int64), head[:, 1].astype(np.int64), head[:, 2].view(np.float32)

    def row(self, s, o):
        """shade_common.h gi_surface_row: the patch row of origin o on sphere s, else the grids' row."""
        g = self.tab.geom[s]
        with np.errstate(all="ignore"):
            e = o - g[:, :3]
            c = _dot(e, e) - g[:, 3]
            ok = np.abs(c) <= self.tau[s]
        N = np.maximum(self.G[s], 1)
        cell = cube_cell_n(np.where(ok[:, None], e, f32(1)), N)
        rows = np.where(ok, self.words[np.where(ok, self.at[s] + cell, 0)].view(np.int32), -1)
        return np.where(rows >= 0, rows, self.tab.origin_row(o))

    def named(self, row, d, k):
        """Bit k of the mask of (row, d's direction cell): rows below first_row are the grids', the others the patches'."""
        tab = self.tab
        E = 6 * tab.G * tab.G
        cell = tab.dir_cell(d)
        grid = row < self.first_row
        m_grid = tab.masks[np.where(grid, row, 0) * E + cell].astype(np.uint32)
        m_patch = self.masks[np.where(grid, 0, row - self.first_row) * E + cell].astype(np.uint32)
        return (np.where(grid, m_grid, m_patch) >> k.astype(np.uint32)) & 1

    def count(self, row, d):
        """Spheres named by the mask of (row, d), every sphere where row = -1."""
        ns = len(self.tab.geom)
        n = np.zeros(len(row), np.int64)
        for k in range(ns):
            n += self.named(np.where(row >= 0, row, 0), d, np.full(len(row), k))
        return np.where(row >= 0, n, ns)


def check(sf, s, o, d, k, what):
    """Every candidate (o, d, sphere k) of an origin on sphere s whose row is a patch's or the grids' is named."""
    o, d = o.astype(f32), d.astype(f32)
    cand = candidates(o, d, sf.tab.geom[k])
    row = sf.row(s, o)
    with np.errstate(all="ignore"):
        a = _dot(d, d)
    used = (row >= 0) & (a >= f32(2.0 ** -40)) & (a <= f32(2.0 ** 40))
    missing = cand & used & (sf.named(np.where(used, row, 0), d, k) == 0)
    assert not missing.any(), "%s: %d of %d candidates missing from their masks, e.g. s=%d o=%r d=%r sphere %d" % (
        what, missing.sum(), cand.sum(), s[missing][0], o[missing][0], d[missing][0], k[missing][0])
    return int((cand & used & (row >= sf.first_row)).sum())


def patch_points(sf, rng, n):
    """Origins on the stored patches: their corners, borders and insides (face coordinates a few ulps either side of a border), at
    radial offsets across the whole slack, and hit-point-like ones (on the surface, + 1e-5 per component)."""
    geom = sf.tab.geom
    has = np.nonzero(sf.G > 0)[0]
    s = has[rng.integers(0, len(has), n)]
    G = sf.G[s]
    face = rng.integers(0, 6, n)
    ij = rng.random((n, 2)) * G[:, None]
    border = rng.random((n, 2)) < 0.6
    ij = np.where(border, rng.integers(0, G[:, None] + 1, (n, 2)), ij)
    fc = ij * (2.0 / G[:, None]) - 1.0
    fc = fc + np.where(border, rng.integers(-6, 7, (n, 2)) * 2.0 ** -24, 0.0)
    ax = face >> 1
    v = np.zeros((n, 3))
    v[np.arange(n), ax] = np.where(face & 1, -1.0, 1.0)
    v[np.arange(n), np.where(ax == 0, 1, 0)] = fc[:, 0]
    v[np.arange(n), np.where(ax == 2, 1, 2)] = fc[:, 1]
    r = np.sqrt(geom[s, 3].astype(np.float64))
    slack = np.sqrt(np.maximum(sf.tau[s].astype(np.float64), 0)) / np.maximum(r, 1e-30)  # (|c| <= tau: |o - C| - r up to about tau / 2r)
    off = np.where(rng.random(n) < 0.5, rng.uniform(-1, 1, n) * 0.5 * sf.tau[s] / r, rng.choice([-1, 1], n) * 0.5 * sf.tau[s] / r * (1 - 1e-3))
    off = np.where(rng.random(n) < 0.2, 0 * slack, off)
    o = geom[s, :3].astype(np.float64) + _unit(v) * (r + off)[:, None]
    o = np.where((rng.random(n) < 0.3)[:, None], o - (off[:, None] * _unit(v)) + 1e-5, o)
    return o.astype(f32), s


def own_rays(sf, rng, o, s):
    """Directions from an origin on sphere s near its own tangent plane (the own-sphere rule of the patches) and into the sphere."""
    n = len(o)
    C = sf.tab.geom[s, :3].astype(np.float64)
    u = _unit(o.astype(np.float64) - C)
    t = _perp(u, rng)
    ang = np.where(rng.random(n) < 0.7, rng.normal(size=n) * 1e-3, rng.uniform(-np.pi / 2, np.pi / 2, n))
    d = u * np.sin(ang)[:, None] + t * np.cos(ang)[:, None]
    return (d * rng.uniform(0.3, 3.0, n)[:, None]).astype(f32)


def sweep(sc, seed, n, what):
    sf = Surface(sc)
    assert len(sf.t) > 0, "%s: no surface patches" % what
    assert len(sf.t) * 4 <= 2 << 20
    rng = np.random.default_rng(seed)
    total = 0
    ns = len(sf.tab.geom)
    for _ in range(3):
        o, s = patch_points(sf, rng, n)
        d, k = aimed_rays(sf.tab, rng, o.astype(np.float64))
        total += check(sf, s, o, d, k, what)
        total += check(sf, s, o, d, rng.integers(0, ns, n), what + " (any sphere)")
        d = own_rays(sf, rng, o, s)
        total += check(sf, s, o, d, s, what + " (own sphere)")
    assert total > n, "%s: too few patch candidates exercised (%d)" % (what, total)
    return sf


def test_patches_name_every_candidate_of_spheres2():
    sf = sweep(skr.parse_scene(scene_path("spheres2.scn")), 61, 40000, "spheres2")
    # the table is what the device reads: rows behind the grids', every stored index word a row of the table
    idx = sf.words[HEAD * len(sf.G):].view(np.int32)
    rows = idx[idx >= 0]
    assert rows.min() == sf.first_row and rows.max() == sf.first_row + len(sf.masks) // (6 * sf.tab.G * sf.tab.G) - 1
    assert len(np.unique(rows)) == len(rows)
    assert (sf.G[1:] >= 1).all() and sf.G[0] > sf.G[1:].max()  # (the ground's patches are its own size, not the small spheres')


@pytest.mark.parametrize("n", [1, 2, 9, 16, 17, 32])
def test_random_sphere_scenes_patches_name_every_candidate(tmp_path, n):
    rng = np.random.default_rng(4300 + n)
    path = os.path.join(str(tmp_path), "s.scn")
    _random_scene(path, rng, n)
    sweep(skr.parse_scene(path), 70 + n, 20000, "random %d" % n)


def test_no_patches_without_grids(tmp_path):
    def words(sc):
        return Surface(sc).t

    assert len(words(skr.parse_scene(scene_path("test.scn")))) == 0  # triangles: no GI masks at all
    rng = np.random.default_rng(5)
    path = os.path.join(str(tmp_path), "s.scn")
    _random_scene(path, rng, 33)
    assert len(words(skr.parse_scene(path))) == 0  # more than 32 spheres


def headline_lanes(sf, rng, n):
    """GI rays of spheres2's tree, roughly: origins on the spheres' surfaces (+ 1e-5), half of them on the ground in front of the
    camera, directions in the cosine-weighted hemisphere of the normal (shade_common.h gi_direction_pair)."""
    geom = sf.tab.geom
    ns = len(geom)
    ground = rng.random(n) < 0.5
    s = np.where(ground, 0, rng.integers(1, ns, n))
    C, r = geom[s, :3].astype(np.float64), np.sqrt(geom[s, 3].astype(np.float64))
    u = _unit(rng.normal(size=(n, 3)))
    gp = np.stack([rng.uniform(-14, 14, n), np.zeros(n), rng.uniform(-8, 14, n)], -1)
    u = np.where(ground[:, None], _unit(gp - C), u)
    o = (C + u * r[:, None] + 1e-5).astype(f32)
    t = _perp(u, rng)
    b = np.cross(u, t)
    phi, q = rng.uniform(0, 2 * np.pi, n), rng.random(n)
    d = u * np.sqrt(1 - q)[:, None] + (t * np.cos(phi)[:, None] + b * np.sin(phi)[:, None]) * np.sqrt(q)[:, None]
    return o, s, d.astype(f32)


def test_headline_lanes_name_fewer_spheres():
    """The gate of the issue: for spheres2 GI rays from sphere hits, the lane mean and the busiest lane of 64 (a wave that has a lane
    without a row takes the full loop: every lane counts as ns)."""
    sf = Surface(skr.parse_scene(scene_path("spheres2.scn")))
    rng = np.random.default_rng(21)
    n = 64 * 1500
    o, s, d = headline_lanes(sf, rng, n)
    ns = len(sf.tab.geom)
    out = {}
    for name, row in (("grids", sf.tab.origin_row(o)), ("patches", sf.row(s, o))):
        cnt = sf.count(row, d).reshape(-1, 64)
        full = (row < 0).reshape(-1, 64).any(-1)
        walk = np.where(full[:, None], ns, cnt)
        out[name] = (float(walk.mean()), float(walk.max(-1).mean()), float(full.mean()))
    print("lane mean / busiest of 64 / full-loop waves:", out)
    g, p = out["grids"], out["patches"]
    assert p[0] < 0.8 * g[0] and p[1] < 0.85 * g[1], out


def test_hit_points_take_patch_rows():
    """The patches are what a hit point gets: origins formed as the device forms them (a binary32 point of the surface, + 1e-5 per
    component: render_nodes.hip activate_record) on every small sphere of spheres2 and on the ground under them resolve to a patch
    row (>= first_row), not to the grids' row — a table that no lane could reach would leave frames unchanged too."""
    sf = Surface(skr.parse_scene(scene_path("spheres2.scn")))
    rng = np.random.default_rng(33)
    n = 20000
    geom = sf.tab.geom
    lo, inv, nn, _ = sf.tab.grid(0)
    hi = lo.astype(np.float64) + nn / float(inv)
    for s in range(len(geom)):
        C, r = geom[s, :3].astype(np.float64), np.sqrt(float(geom[s, 3]))
        if s == 0:  # the ground: points of its top inside the fine grid's box
            x, z = rng.uniform(lo[0], hi[0], n), rng.uniform(lo[2], hi[2], n)
            u = _unit(np.stack([x, np.zeros(n), z], -1) - C)
        else:
            u = _unit(rng.normal(size=(n, 3)))
        P = (C + u * r).astype(f32)
        o = (P + f32(1e-5)).astype(f32)
        row = sf.row(np.full(n, s), o)
        assert (row >= sf.first_row).mean() > 0.99, (s, (row >= sf.first_row).mean())
