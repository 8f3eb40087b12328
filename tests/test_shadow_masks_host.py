"""Host logic of the shadow masks (csrc/scene_host.cpp build_shadow_masks, DESIGN.md "Shadow masks") — no GPU.

The level pipelines' shadow walk (shade_common.h occluded_pair) tests only the spheres named by the cell of v = Lp - P in the light's
table (shade_common.h shadow_mask_of).  That is exact only if every sphere that can stop the ray is named.  These tests restate the
device's side in numpy binary32, in its operation order — the light direction of light_term, the origin offset and the pair test
(device_math.h pair_bD: a sphere is a candidate iff D >= 0 and b < 0, which every occluder is) and the cell lookup — and check, on
points aimed at the borders of the grown spheres and of the cells, that no candidate (P, light, sphere) is ever missing from its mask.
"""
import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path
from scenegen import write_random_mesh_scene

f32 = np.float32


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def device_cell(v):
    """shade_common.h shadow_mask_of: (face, i, j) of the binary32 vectors v [n,3] (fmin/fmax as v_min/v_max: NaN -> 0; exact division in place of v_rcp_f32: the host
    widens every cell by far more than the difference)."""
    N = CELLS
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
    return face, i, j


CELLS = 32


def candidates(P, Lp, sph):
    """occluded_pair's test of the shadow ray from P (float32 [n,3]) towards the light at Lp against sphere rows sph [n,4] =
    {centre, r^2}: (candidate: D >= 0 and b < 0, occluder: the reference's t2 > 1 as well), and v = Lp - P."""
    with np.errstate(all="ignore"):
        v = Lp - P                                        # light_term: to_l
        L = v * (f32(1) / np.sqrt(_dot(v, v)))[:, None]   # len_terms: 1 / sqrt(|v|^2), bit for bit
        o = P + f32(0.000001)
        e = o - sph[:, :3]
        c = _dot(e, e) - sph[:, 3]
        a = _dot(L, L)
        b = f32(2) * _dot(L, e)
        D = b * b - (f32(4) * a) * c
        cand = (D >= 0) & (b < 0)
        t2 = ((-b.astype(np.float64)) - np.sqrt(D.astype(np.float64))) / (f32(2) * a).astype(np.float64)
        t2 = t2.astype(f32)
        occ = cand & (t2 > 1) & np.isfinite(t2)
    return cand, occ, v


def check(sc, P, light, k, what):
    """Every (P, light, sphere k) candidate within the masks' reach is named by its cell.  Returns (candidates, occluders) checked."""
    masks, reach2 = sc.shadow_masks()
    geom = np.array([[s[0], s[1], s[2], s[3] * s[3]] for s in sc.arrays()[0]], f32)
    lp = sc.arrays()[2][:, :3].astype(f32)
    P = P.astype(f32)
    cand, occ, v = candidates(P, lp[light], geom[k])
    inside = _dot(v, v) <= f32(reach2)
    face, i, j = device_cell(v)
    named = (masks[light, face, i, j] >> k.astype(np.uint32)) & 1
    missing = cand & inside & (named == 0)
    assert not missing.any(), "%s: %d of %d candidates missing from their masks, e.g. P=%r light %d sphere %d" % (
        what, missing.sum(), cand.sum(), P[missing][0], light[missing][0], k[missing][0])
    return int((cand & inside).sum()), int((occ & inside).sum())


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _perp(w, rng):
    t = _unit(np.cross(w, rng.normal(size=w.shape)))
    return t


def border_points(sc, rng, n):
    """P aimed at the borders: (1) on the sphere surfaces, (2) on lines through a light that graze a sphere (its grown disc, seen from
    the light, at +-2^-k relative), (3) on lines through a light along cell borders (face coordinates k/16 - 1, +- 1 ulp).  P lies at
    random distances, either side of the light, inside the masks' reach.  Returns P [n,3], light [n], sphere [n]."""
    s, _, l = sc.arrays()
    _, reach2 = sc.shadow_masks()
    reach = np.sqrt(reach2)
    ns, nl = len(s), len(l)
    C, r, Lp = s[:, :3].astype(np.float64), s[:, 3].astype(np.float64), l[:, :3].astype(np.float64)
    light = rng.integers(0, nl, n)
    k = rng.integers(0, ns, n)
    kind = rng.integers(0, 3, n)
    # (1) points on the spheres (any sphere; the tested sphere is k)
    h = rng.integers(0, ns, n)
    P1 = C[h] + _unit(rng.normal(size=(n, 3))) * r[h, None] * (1 + rng.normal(size=(n, 1)) * 1e-6)
    # (2) grazing lines through the light: angle asin(r / |C - Lp|) from the centre direction, times 1 +- 2^-j
    q = C[k] - Lp[light]
    qn = np.linalg.norm(q, axis=1)
    ang = np.arcsin(np.minimum(1.0, r[k] / np.maximum(qn, 1e-30)))
    ang = ang * (1 + rng.choice([-1, 1], n) * 2.0 ** -rng.integers(4, 30, n))
    w2 = _unit(q) * np.cos(ang)[:, None] + _perp(q, rng) * np.sin(ang)[:, None]
    # (3) cell borders: one face coordinate on a border, the other random
    ax = rng.integers(0, 3, n)
    w3 = rng.uniform(-1, 1, (n, 3))
    w3[np.arange(n), ax] = rng.choice([-1.0, 1.0], n)
    b = rng.integers(0, CELLS + 1, n) * (2.0 / CELLS) - 1.0
    o1 = np.where(ax == 0, 1, 0)
    w3[np.arange(n), o1] = np.nextafter(b, b + rng.choice([-1.0, 0.0, 1.0], n))
    w = np.where((kind == 1)[:, None], w2, w3)
    dist = rng.uniform(-1, 1, n) * reach * np.where(rng.random(n) < 0.5, 1.0, rng.random(n) ** 4)
    P23 = Lp[light] + w * dist[:, None]
    P = np.where((kind == 0)[:, None], P1, P23)
    return P, light, k


SHIPPED = ["spheres1.scn", "spheres2.scn", "bear.scn", "test.scn"]


@pytest.mark.parametrize("name", SHIPPED)
def test_masks_name_every_candidate_of_the_shipped_scenes(name):
    sc = skr.parse_scene(scene_path(name))
    masks, reach2 = sc.shadow_masks()
    if not masks.shape[0]:
        assert sc.info.n_spheres > 32 or sc.info.n_point_lights == 0 or sc.info.n_spheres == 0
        pytest.skip("no masks: %d spheres, %d point lights" % (sc.info.n_spheres, sc.info.n_point_lights))
    assert masks.shape[1:] == (6, CELLS, CELLS) and masks.shape[0] == sc.info.n_point_lights
    rng = np.random.default_rng(SHIPPED.index(name))
    P, light, k = border_points(sc, rng, 400000)
    nc, no = check(sc, P, light, k, name)
    assert nc > 10000 and no > 1000  # (the points reach both)


def test_headline_scene_masks_are_narrow():
    """The masks are worth having: on spheres2.scn a shadow ray from a sphere surface names few of the 15 spheres."""
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    masks, _ = sc.shadow_masks()
    s, _, l = sc.arrays()
    rng = np.random.default_rng(3)
    h = rng.integers(0, len(s), 50000)
    P = (s[h, :3] + _unit(rng.normal(size=(len(h), 3))) * s[h, 3:4]).astype(f32)
    counts = []
    for li in range(len(l)):
        face, i, j = device_cell(l[li, :3].astype(f32) - P)
        counts.append(np.array([bin(int(x)).count("1") for x in masks[li, face, i, j]]))
    assert np.mean(counts) < 5.0, np.mean(counts)


def _random_sphere_scene(path, rng):
    """Up to 32 spheres of any size (some tiny, some huge, a light inside some of them), 1-2 point lights, anywhere in a box that is
    sometimes far from the origin."""
    off = rng.choice([0.0, 1e3, -3e4]) * rng.uniform(0.5, 1, 3)
    scale = 10.0 ** rng.uniform(-2, 3)
    lines = ["camera %g %g %g 0 0 1 0 1 0 30" % tuple(off + [0, 0, -8 * scale])]
    ns = int(rng.integers(1, 33))
    lights = [off + rng.uniform(-6, 6, 3) * scale for _ in range(int(rng.integers(1, 3)))]
    for i in range(ns):
        c = off + rng.uniform(-6, 6, 3) * scale
        rad = scale * 10.0 ** rng.uniform(-3, 0.3)
        if i == 0 and rng.random() < 0.5:
            c, rad = lights[0] + rng.normal(size=3) * 0.1 * scale, 0.5 * scale   # the light inside a sphere
        lines.append("material .5 .5 .5 .5 .5 .5 .2 .2 .2 8 0 0 0 1")
        lines.append("sphere %.9g %.9g %.9g %.9g" % (*c, rad))
    for lp in lights:
        lines.append("point_light 1 1 1 %.9g %.9g %.9g" % tuple(lp))
    open(path, "w").write("\n".join(lines) + "\n")


@pytest.mark.parametrize("seed", range(10))
def test_random_sphere_scenes_masks_name_every_candidate(tmp_path, seed):
    path = str(tmp_path / "s.scn")
    _random_sphere_scene(path, np.random.default_rng(4000 + seed))
    sc = skr.parse_scene(path)
    assert sc.shadow_masks()[0].shape[0] == sc.info.n_point_lights
    P, light, k = border_points(sc, np.random.default_rng(seed), 200000)
    nc, _ = check(sc, P, light, k, "random sphere scene %d" % seed)
    assert nc > 1000


@pytest.mark.parametrize("seed", range(6))
def test_random_mesh_scenes_masks_name_every_candidate(tmp_path, seed):
    """The scenes of tests/test_gpu_parity.py's random meshes (0-3 spheres, 0-2 lights, triangles that widen the reach)."""
    path = str(tmp_path / "mesh.scn")
    write_random_mesh_scene(path, np.random.default_rng(1000 + seed))
    sc = skr.parse_scene(path)
    if not sc.shadow_masks()[0].shape[0]:
        assert sc.info.n_spheres == 0 or sc.info.n_point_lights == 0
        return
    P, light, k = border_points(sc, np.random.default_rng(seed), 100000)
    check(sc, P, light, k, "random mesh scene %d" % seed)


def test_no_masks_where_the_plain_loop_must_run(tmp_path):
    """More than 32 spheres, or a directional light (--strict-scn): no masks, the walk keeps its loop over every sphere."""
    lines = ["camera 0 0 -8 0 0 1 0 1 0 30", "point_light 1 1 1 0 5 0"]
    lines += ["sphere %d 0 %d .3" % (i % 7, i // 7) for i in range(33)]
    path = str(tmp_path / "many.scn")
    open(path, "w").write("\n".join(lines) + "\n")
    assert skr.parse_scene(path).shadow_masks()[0].shape[0] == 0
    assert skr.parse_scene(scene_path("spheres2.scn"), strict=True).shadow_masks()[0].shape[0] == 0
    assert skr.parse_scene(scene_path("spheres2.scn")).shadow_masks()[0].shape[0] == 2
