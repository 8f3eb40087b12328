"""Host logic of the GI masks (csrc/scene_host.cpp build_gi_masks, DESIGN.md "GI masks") — no GPU.

The node pipeline's closest-hit walk of a GI child (wave_common.h closest_pair) tests only the spheres named by the mask of (the
cell of its origin, the cell of its direction) (shade_common.h gi_origin_row, gi_cands).  That is exact only if every candidate
(D >= 0 and b < 0 in the device's binary32 test, device_math.h pair_bD) is named.  These tests restate the device's side in numpy
binary32, in its operation order, and check on rays aimed at grazing lines, origin-cell corners and direction-cell borders of the
shipped and of random sphere scenes that no candidate is ever missing.  A numpy restatement of the builder's margins reproduces the
shipped masks, and with the origin-cell radius or the direction-cell angle shrunk to 0.7 of it, candidates go missing.
"""
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path

f32 = np.float32


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


class Table:
    def __init__(self, sc):
        self.t, self.mw, self.wide, self.G, self.grids = sc.gi_masks()
        self.index = self.t[:self.mw].view(np.int32)
        self.masks = self.t[self.mw:] if self.wide else self.t[self.mw:].view(np.uint16)
        self.geom = np.array([[s[0], s[1], s[2], f32(s[3]) * f32(s[3])] for s in sc.arrays()[0]], f32)

    def grid(self, g):
        r = self.grids[g]
        return r[:3].astype(f32), f32(r[3]), r[4:7].astype(np.int64), int(r[7])

    def origin_row(self, o):
        """shade_common.h gi_origin_row: the fine grid's row, else the coarse one's; -1 = none."""
        rows = []
        for g in range(2):
            lo, inv, n, base = self.grid(g)
            with np.errstate(all="ignore"):
                f = (o - lo) * inv
                inside = ((f >= 0) & (f < n.astype(f32))).all(-1)
                fi = np.where(inside[:, None], f, 0).astype(np.int64)
            c = base + (fi[:, 2] * n[1] + fi[:, 1]) * n[0] + fi[:, 0]
            rows.append(np.where(inside, self.index[np.where(inside, c, 0)], -1))
        return np.where(rows[0] >= 0, rows[0], rows[1])

    def dir_cell(self, v):
        """shade_common.h cube_cell<G> (exact division for v_rcp_f32: the host widens every cell by far more than the difference)."""
        N = self.G
        a = np.abs(v)
        fx = (a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2])
        fy = ~fx & (a[:, 1] >= a[:, 2])
        m = np.where(fx, a[:, 0], np.where(fy, a[:, 1], a[:, 2]))
        lead = np.where(fx, v[:, 0], np.where(fy, v[:, 1], v[:, 2]))
        ca = np.where(fx, v[:, 1], v[:, 0])
        cb = np.where(fx | fy, v[:, 2], v[:, 1])
        face = np.where(fx, 0, np.where(fy, 2, 4)) + (lead < 0)
        h = f32(0.5 * N)
        with np.errstate(all="ignore"):
            inv = f32(1) / m
            i = np.fmin(np.fmax((ca * inv) * h + h, f32(0)), f32(N - 1)).astype(np.int64)
            j = np.fmin(np.fmax((cb * inv) * h + h, f32(0)), f32(N - 1)).astype(np.int64)
        return (face * N + i) * N + j


def candidates(o, d, sph):
    """closest_pair_deferred's test of the ray o + t d (float32 [n,3]) against sphere rows sph [n,4]: D >= 0 and b < 0."""
    with np.errstate(all="ignore"):
        e = o - sph[:, :3]
        c = _dot(e, e) - sph[:, 3]
        a = _dot(d, d)
        b = f32(2) * _dot(d, e)
        D = b * b - (f32(4) * a) * c
    return (D >= 0) & (b < 0)


def check(tab, o, d, k, what):
    """Every candidate (o, d, sphere k) of a lane that uses the masks is named.  Returns the number of candidates checked."""
    o, d = o.astype(f32), d.astype(f32)
    cand = candidates(o, d, tab.geom[k])
    row = tab.origin_row(o)
    with np.errstate(all="ignore"):
        a = _dot(d, d)
    used = (row >= 0) & (a >= f32(2.0 ** -40)) & (a <= f32(2.0 ** 40))
    e = np.where(used, row, 0) * (6 * tab.G * tab.G) + tab.dir_cell(d)
    named = (tab.masks[e].astype(np.uint32) >> k.astype(np.uint32)) & 1
    missing = cand & used & (named == 0)
    assert not missing.any(), "%s: %d of %d candidates missing from their masks, e.g. o=%r d=%r sphere %d" % (
        what, missing.sum(), cand.sum(), o[missing][0], d[missing][0], k[missing][0])
    return int((cand & used).sum())


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _perp(w, rng):
    p = np.cross(w, rng.normal(size=w.shape))
    return _unit(p)


def stored_cell_points(tab, rng, n):
    """Points of the stored origin cells: corners, face centres and random points, each nudged by a few ulps either way."""
    pts = []
    for g in range(2):
        lo, inv, nn, base = tab.grid(g)
        h = 1.0 / float(inv)
        rows = tab.index[base:base + int(np.prod(nn))]
        cells = np.nonzero(rows >= 0)[0]
        if len(cells) == 0:
            continue
        pick = cells[rng.integers(0, len(cells), n)]
        ijk = np.stack([pick % nn[0], (pick // nn[0]) % nn[1], pick // (nn[0] * nn[1])], -1).astype(np.float64)
        frac = np.where(rng.random((n, 3)) < 0.5, rng.integers(0, 2, (n, 3)).astype(np.float64), rng.random((n, 3)))
        p = (lo.astype(np.float64) + (ijk + frac) * h).astype(f32)
        # within a few ulps of the cell's faces either way (the 2^-18 n padding of the origin cells)
        steps = rng.integers(-4, 5, (n, 3))
        for s in range(1, 5):
            p = np.where(steps >= s, np.nextafter(p, f32(np.inf)), np.where(-steps >= s, np.nextafter(p, f32(-np.inf)), p))
        pts.append(p)
    return np.concatenate(pts).astype(f32)


def surface_points(tab, rng, n):
    """Hit-point-like origins: on a sphere's surface, offset by 1e-5 per component (render_nodes.hip activate_record)."""
    k = rng.integers(0, len(tab.geom), n)
    c, r = tab.geom[k, :3].astype(np.float64), np.sqrt(tab.geom[k, 3].astype(np.float64))
    return (c + _unit(rng.normal(size=(n, 3))) * r[:, None] + 1e-5).astype(f32)


def aimed_rays(tab, rng, o):
    """Directions from o at grazing lines of a random sphere, at its centre, at direction-cell borders, and at random; lengths in
    [0.3, 3] (GI directions are not unit: shade_common.h gi_direction_pair)."""
    n = len(o)
    k = rng.integers(0, len(tab.geom), n)
    C, r = tab.geom[k, :3].astype(np.float64), np.sqrt(tab.geom[k, 3].astype(np.float64))
    w = C - o
    kind = rng.integers(0, 4, n)
    # grazing lines: 1e-4 of the radius off the surface (the cell terms), or a few ulps off it (the discriminant slack)
    off = np.where(rng.random(n) < 0.5, rng.normal(size=n) * 1e-4, rng.integers(-8, 9, n) * 2.0 ** -23)
    graze = C + _perp(_unit(w), rng) * (r * (1 + off))[:, None] - o
    G = tab.G
    face_pt = np.zeros((n, 3))
    ax = rng.integers(0, 3, n)
    face_pt[np.arange(n), ax] = rng.choice([-1.0, 1.0], n)
    border = (rng.integers(0, G + 1, (n, 2)) * (2.0 / G) - 1.0) + np.where(rng.random((n, 2)) < 0.5, rng.normal(size=(n, 2)) * 1e-6,
                                                                           rng.integers(-4, 5, (n, 2)) * 2.0 ** -24)  # (the 2^-12 face padding)
    border[:, 1] = np.where(rng.random(n) < 0.5, border[:, 1], rng.uniform(-1, 1, n))
    o1, o2 = np.where(ax == 0, 1, 0), np.where(ax == 2, 1, 2)
    face_pt[np.arange(n), o1] = border[:, 0]
    face_pt[np.arange(n), o2] = border[:, 1]
    d = np.where((kind == 0)[:, None], graze, np.where((kind == 1)[:, None], w, np.where((kind == 2)[:, None], face_pt, rng.normal(size=(n, 3)))))
    d = _unit(d) * rng.uniform(0.3, 3.0, n)[:, None]
    return d.astype(f32), k


def sweep(sc, seed, n, what):
    tab = Table(sc)
    assert len(tab.t) > 0, "%s: no GI masks" % what
    assert len(tab.t) * 4 <= 2 << 20
    rng = np.random.default_rng(seed)
    total = 0
    for origins in (stored_cell_points(tab, rng, n), surface_points(tab, rng, n)):
        for _ in range(3):
            d, k = aimed_rays(tab, rng, origins.astype(np.float64))
            total += check(tab, origins, d, k, what)
            ks = rng.integers(0, len(tab.geom), len(origins))
            total += check(tab, origins, d, ks, what + " (any sphere)")
    assert total > n, "%s: too few candidates exercised (%d)" % (what, total)
    return tab


@pytest.mark.parametrize("name", ["spheres2.scn"])  # (spheres1.scn, test.scn, bear.scn: triangles, no masks)
def test_masks_name_every_candidate_of_the_shipped_scenes(name):
    sweep(skr.parse_scene(scene_path(name)), 31, 40000, name)


def _random_scene(path, rng, n):
    lines = ["camera 0 2 -10 0 -.1 .9 0 1 0 30", "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1",
             "sphere %.7g %.7g %.7g %.7g" % (rng.uniform(-3, 3), -40 * rng.uniform(0.5, 2), rng.uniform(-3, 3), 40 * rng.uniform(0.5, 2))]
    for _ in range(n - 1):
        c, rad = rng.uniform(-8, 8, 3) + [0, 2, 3], 10.0 ** rng.uniform(-2, 0.3)
        lines.append("sphere %.7g %.7g %.7g %.7g" % (*c, rad))
    lines.append("point_light .8 .8 .8 2 9 -1")
    open(path, "w").write("\n".join(lines) + "\n")


@pytest.mark.parametrize("n", [1, 2, 9, 16, 17, 32])
def test_random_sphere_scenes_masks_name_every_candidate(tmp_path, n):
    rng = np.random.default_rng(4200 + n)
    path = os.path.join(str(tmp_path), "s.scn")
    _random_scene(path, rng, n)
    tab = sweep(skr.parse_scene(path), 50 + n, 20000, "random %d" % n)
    assert tab.wide == (1 if n > 16 else 0)


def test_no_masks_where_the_plain_loop_must_run(tmp_path):
    assert len(skr.parse_scene(scene_path("test.scn")).gi_masks()[0]) == 0  # triangles
    rng = np.random.default_rng(5)
    path = os.path.join(str(tmp_path), "s.scn")
    _random_scene(path, rng, 33)
    assert len(skr.parse_scene(path).gi_masks()[0]) == 0  # more than 32 spheres


# ---- the builder's margins, restated: they reproduce the shipped masks, and shrinking either cell term loses candidates ----
def cube_cells(N):
    """scene_host.cpp cube_cells: centre directions [6 N N, 3] and angular radii of the cells, widened by 2^-12 in face coordinates."""
    f, i, j = np.meshgrid(np.arange(6), np.arange(N), np.arange(N), indexing="ij")
    f, i, j = f.ravel(), i.ravel(), j.ravel()
    ax, sg = f >> 1, np.where(f & 1, -1.0, 1.0)
    o1, o2 = np.where(ax == 0, 1, 0), np.where(ax == 2, 1, 2)
    wid, pad = 2.0 / N, 2.0 ** -12

    def dirs(a, b):
        w = np.zeros((len(f), 3))
        w[np.arange(len(f)), ax] = sg
        w[np.arange(len(f)), o1] = a
        w[np.arange(len(f)), o2] = b
        return _unit(w)
    a0, b0 = -1.0 + i * wid, -1.0 + j * wid
    wc = dirs(a0 + 0.5 * wid, b0 + 0.5 * wid)
    theta = np.zeros(len(f))
    for corner in range(4):
        w = dirs(np.where(corner & 1, a0 + wid + pad, a0 - pad), np.where(corner & 2, b0 + wid + pad, b0 - pad))
        theta = np.maximum(theta, np.arctan2(np.linalg.norm(np.cross(wc, w), axis=-1), _dot(wc, w)))
    return wc, theta * (1 + 2.0 ** -20) + 2.0 ** -40


def restated_row(tab, q, rho, wc, theta, ns):
    """scene_host.cpp build_gi_masks: the masks of the origin cell (q, rho) for every direction cell."""
    row = np.zeros(len(wc), np.uint32)
    ct, st = np.cos(theta), np.sin(theta)
    for k in range(ns):
        r2 = float(tab.geom[k, 3])
        v = tab.geom[k, :3].astype(np.float64) - q
        dist = np.linalg.norm(v)
        E = (dist + rho) * (1 + 2.0 ** -20)
        rk = np.sqrt(r2 + 2.0 ** -16 * (E * E + r2)) + 2.0 ** -20 * E
        tol = 2.0 ** -30 * (dist + rho + rk)
        behind, reach = rho + 2.0 ** -16 * E + tol, rk + rho + tol
        if dist <= reach:
            row |= np.uint32(1 << k)
            continue
        cp = (wc @ v) / dist
        sp = np.linalg.norm(np.cross(v[None, :], wc), axis=-1) / dist
        lo0, hipi = cp >= ct, cp <= -ct
        cos_lo = np.where(lo0, 1.0, cp * ct + sp * st)
        sin_lo = np.where(lo0, 0.0, sp * ct - cp * st)
        sin_hi = np.where(hipi, 0.0, sp * ct + cp * st)
        min_sin = np.maximum(0.0, np.minimum(sin_lo, sin_hi))
        row |= np.where((dist * cos_lo + behind >= 0) & (dist * min_sin <= reach), np.uint32(1 << k), np.uint32(0))
    return row


def test_restated_margins_reproduce_and_are_needed():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    tab = Table(sc)
    ns = len(tab.geom)
    wc, theta = cube_cells(tab.G)
    rng = np.random.default_rng(77)
    lo, inv, n, base = tab.grid(0)
    h = 1.0 / float(inv)
    pad = 2.0 ** -18 * n.max() * h
    rho = np.sqrt(3.0) * (0.5 * h + pad) * (1 + 2.0 ** -20)
    stored = np.nonzero(tab.index[base:base + int(np.prod(n))] >= 0)[0]
    lost = {"rho": 0, "theta": 0}
    for c in stored[rng.choice(len(stored), 24, replace=False)]:
        ijk = np.array([c % n[0], (c // n[0]) % n[1], c // (n[0] * n[1])], np.float64)
        q = lo.astype(np.float64) + (ijk + 0.5) * h
        row = tab.index[base + c]
        shipped = tab.masks[row * 6 * tab.G * tab.G:(row + 1) * 6 * tab.G * tab.G].astype(np.uint32)
        assert np.array_equal(restated_row(tab, q, rho, wc, theta, ns), shipped)
        # rays from the cell's corners (pulled in by a few ulps) grazing every sphere: the candidates a shrunk margin would not name
        corners = q + (np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * 0.5 * h) * (1 - 2.0 ** -20)
        o = np.repeat(corners, ns * 48, axis=0)
        k = np.tile(np.repeat(np.arange(ns), 48), 8)
        C, r = tab.geom[k, :3].astype(np.float64), np.sqrt(tab.geom[k, 3].astype(np.float64))
        d = C + _perp(_unit(C - o), rng) * (r * (1 - 1e-4))[:, None] - o
        o, d = o.astype(f32), (_unit(d) * rng.uniform(0.3, 3.0, len(d))[:, None]).astype(f32)
        keep = tab.origin_row(o) == row
        o, d, k = o[keep], d[keep], k[keep]
        cand = candidates(o, d, tab.geom[k])
        e = tab.dir_cell(d)
        for what, r_, t_ in (("rho", 0.7 * rho, theta), ("theta", rho, 0.7 * theta)):
            small = restated_row(tab, q, r_, wc, t_, ns)
            lost[what] += int((cand & (((small[e] >> k.astype(np.uint32)) & 1) == 0)).sum())
    assert lost["rho"] > 0 and lost["theta"] > 0, lost


def test_headline_waves_mostly_walk_their_masks():
    """The masked walk is what runs on the headline: origins on the spheres' surfaces (the hit points of a GI tree) with directions
    in the hemisphere of their normal, in groups of 64 lanes; a group runs the full loop only when one of its lanes has no mask
    (wave_common.h closest_pair_deferred).  The device's own figure (-DSKR_DIAG): 3.8 % of the calls."""
    tab = Table(skr.parse_scene(scene_path("spheres2.scn")))
    rng = np.random.default_rng(12)
    n = 64 * 2000
    k = rng.integers(1, len(tab.geom), n)  # hits on the small spheres, and on the ground near them
    c, r = tab.geom[k, :3].astype(np.float64), np.sqrt(tab.geom[k, 3].astype(np.float64))
    nrm = _unit(rng.normal(size=(n, 3)))
    o = np.where((rng.random(n) < 0.5)[:, None], c + nrm * r[:, None], np.stack([rng.uniform(-20, 20, n), np.zeros(n), rng.uniform(-10, 25, n)], -1))
    nrm = np.where((np.abs(o[:, 1]) < 1e-9)[:, None], [0.0, 1.0, 0.0], nrm)
    o = (o + 1e-5).astype(f32)
    d = _unit(rng.normal(size=(n, 3)))
    d = np.where((_dot(d, nrm) < 0)[:, None], -d, d).astype(f32)
    row = tab.origin_row(o)
    e = np.where(row >= 0, row, 0) * (6 * tab.G * tab.G) + tab.dir_cell(d)
    named = np.unpackbits(tab.masks[e].astype(np.uint16).view(np.uint8)).reshape(n, 16).sum(-1)
    fallback = (row < 0).reshape(-1, 64).any(-1)
    assert fallback.mean() < 0.1, fallback.mean()
    assert named[row >= 0].mean() < 5, named[row >= 0].mean()
