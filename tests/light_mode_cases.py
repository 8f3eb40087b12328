"""Scenes for spot lights, lights with a radius, triangle shadows under them and the thin lens, as data:
shared by tests/test_light_modes_cpu.py, tests/test_light_modes_gpu.py and tests/fuzz_light_modes.py.  Plain Python and numpy, no GPU.

All four modes end in one light loop (shade_common.h direct_light_cone): per pair of lights it decides who is inside its cone, whether
the pair's shadow masks are used, united or dropped, and where a sample puts the light and the far end of the triangle walk.  A case is

    build(family, index, folder) -> Case(family, index, name, scene, flags, radii, lens, w, h, kw, rays, keys, sample, meta)

    scene    the .scn file, written into `folder` (spot_light lines in the grammar of spot_check.write_floor_scene)
    flags    the loader's: spot, strict, triangle_shadows
    radii    one per point and spot light, in shading order (point lights, then spot lights)
    lens     (A, F) or None
    kw       option keywords (fov, seed, shadow, shade_triangles, gillum, depth, jsample, progressive)
    rays     257 query rays float32 [257, 8] (include/skr.h skr_ray), keys uint32 [257], sample > 0
    meta     what the case is, for the conditions tests/test_light_modes_cpu.py holds

and depends on (family, index) alone: every case draws from its own generator np.random.default_rng([seed, index]), no draw depends on
a render, and every draw is taken whether or not a branch uses it, so two variants of a case share their geometry.

The family "random" has RANDOM_CASES cases under SEED.  The edge families are hand-built, at most 64 x 48, and each aims at one
decision of direct_light_cone; EDGE lists what every case of them is.  NAN holds the ids of cases in which a NaN can reach the frame
(compared with any NaN standing for any NaN); it is empty: no edge below divides 0 by 0, and no other case may hold a NaN."""
import collections
import os

import numpy as np

from camera_poses import posed_text, random_camera
from scenegen import write_random_mesh_scene
from spot_check import CAMERA, FLOOR, OCCLUDER

SEED = 9
RANDOM_CASES = 64
N_RAYS = 257  # four waves and a tail of one
MODES = ("direct", "jsample", "gillum", "progressive")
ANGLES = (0, 5, 20, 45, 90, 120, 180)
SPREADS = (0, 10, 40, 90)
MAX_MASK_SPHERES = 32  # csrc/shadow_cells.h SKR_SHADOW_MAX_SPHERES: above it a scene has no shadow masks
NO_TRIANGLE = np.array([-1], np.int32).view(np.float32)[0]

Case = collections.namedtuple("Case", "family index name scene flags radii lens w h kw rays keys sample meta")

NAN = ()


def _fmt(values):
    return " ".join("%.9g" % v for v in values)


def _query_rays(rng, lo, hi):
    """N_RAYS rays with origins in the box [lo, hi], any direction and length, a finite tmax on a quarter of them, keys that are any 32
    bits (never y * w + x of a frame), and the sample index"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    rays = np.zeros((N_RAYS, 8), np.float32)
    rays[:, 0:3] = rng.uniform(lo, hi, (N_RAYS, 3))
    d = rng.normal(size=(N_RAYS, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (N_RAYS, 1))
    tmax = rng.uniform(0.5, 15.0, N_RAYS)
    rays[:, 3] = np.where(rng.random(N_RAYS) < 0.25, tmax, np.inf)
    rays[:, 7] = NO_TRIANGLE
    keys = rng.integers(0, 2 ** 32, N_RAYS, dtype=np.uint64).astype(np.uint32)
    return rays, keys, int(rng.integers(1, 4))


def _box(text):
    """the box of a scene's sphere centres (the ground and the floor apart) and vertices, a unit wider"""
    pts = []
    for ln in text.split("\n"):
        t = ln.split()
        if t[:1] == ["sphere"] and float(t[4]) < 30:
            pts.append([float(x) for x in t[1:4]])
        elif t[:1] == ["vertex"]:
            pts.append([float(x) for x in t[1:4]])
    pts = np.array(pts if pts else [[0.0, 1.0, 3.0]])
    return pts.min(0) - 1.0, pts.max(0) + 1.0


def _finish(family, index, name, folder, text, flags, radii, lens, w, h, kw, rng, meta, box=None):
    path = os.path.join(folder, "%s_%d.scn" % (family, index))
    with open(path, "w") as f:
        f.write(text)
    rays, keys, sample = _query_rays(rng, *(box or _box(text)))
    flags = dict(spot=bool(flags.get("spot")), strict=bool(flags.get("strict")), triangle_shadows=bool(flags.get("triangle_shadows")))
    return Case(family, index, name, path, flags, np.asarray(radii, np.float32), lens, w, h, kw, rays, keys, sample, meta)


# ---- the random family ----
def _sphere_scene_text(rng):
    """in the manner of fuzz_parity.write_sphere_scene: a radius-40 ground and 1 to 39 further spheres that may overlap each other and
    the ground; no light"""
    lines = ["camera %g %g %g 0 -.05 1 0 1 0 30" % (rng.uniform(-1, 1), rng.uniform(1, 2), rng.uniform(-10, -7)), "background %g %g %g" % tuple(rng.random(3) * .5),
             "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1.3", "sphere 0 -40 0 40"]
    n = int(rng.integers(1, 40))
    draws = [(rng.random(3), rng.random(3), rng.random(3) * rng.choice([0, .5]), float(rng.choice([1, 2, 2.5, 16, 60])), rng.uniform(.8, 1.8),
              rng.uniform(-6, 6), rng.uniform(-.5, 4), rng.uniform(-3, 8), rng.uniform(.3, 1.3)) for _ in range(39)]
    for ka, kd, ks, power, ior, x, y, z, r in draws[:n]:
        lines.append("material %g %g %g %g %g %g %g %g %g %g 0 0 0 %g" % (*ka, *kd, *ks, power, ior))
        lines.append("sphere %g %g %g %g" % (x, y, z, r))
    return "\n".join(lines) + "\n"


def _mesh_scene_text(rng, folder, name):
    """scenegen.write_random_mesh_scene without its lights"""
    path = os.path.join(folder, name)
    write_random_mesh_scene(path, rng)
    with open(path) as f:
        lines = f.read().split("\n")
    os.remove(path)
    return "\n".join(ln for ln in lines if ln.split()[:1] != ["point_light"])


def random_case(index, folder, seed=SEED):
    """Case `index` of the random family under `seed`."""
    rng = np.random.default_rng([seed, index])
    # what the case is: every draw taken, in this order, whatever the case then uses
    mesh = bool(rng.random() < 0.35)
    mode = MODES[index % len(MODES)]
    n_point, n_spot = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    has_radius = rng.random(6) < 0.5
    radius = rng.uniform(0.1, 3.0, 6)
    strict = bool(rng.random() < 0.5)
    with_directional, n_directional = bool(rng.random() < 0.3), int(rng.integers(1, 3))
    posed = bool(rng.random() < 0.5)
    shadow = bool(rng.random() < 0.75)
    triangle_shadows = bool(rng.random() < 0.5)
    with_lens = bool(rng.random() < 0.25)
    lens_scale, focus_scale = float(rng.choice([0.002, 0.02, 0.1, 0.5])), float(rng.uniform(0.5, 1.5))
    w, h = int(rng.integers(8, 97)), int(rng.integers(8, 65))
    gillum, depth = int(rng.choice([1, 2, 3, 5])), int(rng.integers(2, 4))
    opt_seed, fov = int(rng.integers(1, 2 ** 40)), float(rng.choice([30, 60, 90]))
    if n_point + n_spot == 0:
        n_spot = 1
    if n_spot == 0 and not has_radius[:n_point].any():
        has_radius[0] = True  # at least one spot light or one radius
    # the geometry, the camera, the lights and the rays: a generator each, since the draw count of the first two depends on what they make
    sub, cam_rng, light_rng, ray_rng = (np.random.default_rng([seed, index, k]) for k in (1, 2, 3, 4))
    text = _mesh_scene_text(sub, folder, "random_%d_mesh.tmp" % index) if mesh else _sphere_scene_text(sub)
    balls = [tuple(float(t) for t in ln.split()[1:5]) for ln in text.split("\n") if ln.split()[:1] == ["sphere"]]
    camera = random_camera(cam_rng, (0, 1.5, 3), balls)
    if posed:
        text = posed_text(text, camera)
    lines = text.rstrip("\n").split("\n")
    points = [(*light_rng.uniform(5, 40, 3), light_rng.uniform(-7, 7), light_rng.uniform(2, 9), light_rng.uniform(-6, 8)) for _ in range(3)]
    spots = []
    for _ in range(3):
        pos = np.array([light_rng.uniform(-7, 7), light_rng.uniform(2, 9), light_rng.uniform(-6, 8)])
        aim = np.array([light_rng.uniform(-4, 4), light_rng.uniform(-1, 2), light_rng.uniform(-1, 7)]) - pos
        axis = aim / np.linalg.norm(aim) * 10.0 ** light_rng.uniform(-2, 2)  # not unit
        a1, spread = float(light_rng.choice(ANGLES)), float(light_rng.choice(SPREADS))
        spots.append((*light_rng.uniform(20, 120, 3), *pos, *axis, a1, min(a1 + spread, 180.0)))
    directional = [(*light_rng.uniform(.1, .8, 3), light_rng.uniform(-1, 1), light_rng.uniform(-1, -.2), light_rng.uniform(-1, 1)) for _ in range(2)]
    lines += ["point_light " + _fmt(p) for p in points[:n_point]]
    lines += ["spot_light " + _fmt(s) for s in spots[:n_spot]]
    n_dir = n_directional if strict and with_directional else 0
    lines += ["directional_light " + _fmt(d) for d in directional[:n_dir]]
    text = "\n".join(lines) + "\n"
    radii = np.where(has_radius, radius, 0.0)[:n_point + n_spot]
    kw = dict(seed=opt_seed, fov=fov, shadow=shadow)
    if mesh:
        kw["shade_triangles"] = True
    if mode == "jsample":
        kw["jsample"] = 2
    elif mode == "gillum":
        assert gillum ** (depth - 1) * w * h <= 2e5  # (5^2 * 96 * 64 = 153600: every draw fits)
        kw.update(gillum=gillum, depth=depth)
    elif mode == "progressive":
        kw["progressive"] = 2
    # the lens scaled to the camera's distance from the scene: a lens point lies A |right| from the camera (right = cross(-direction, up)),
    # the focal plane F |direction| ahead; the largest apertures put lens points inside spheres
    cam = np.array([float(t) for t in next(ln for ln in lines if ln.split()[:1] == ["camera"]).split()[1:10]])
    dist = np.linalg.norm(np.array([0, 1.5, 3]) - cam[:3])
    right = np.linalg.norm(np.cross(-cam[3:6], cam[6:9]))
    lens = (float(np.float32(dist * lens_scale / max(right, 1e-9))), float(np.float32(dist * focus_scale / max(np.linalg.norm(cam[3:6]), 1e-9)))) if with_lens else None
    n_spheres = len(balls)
    meta = dict(mesh=mesh, mode=mode, n_spheres=n_spheres, n_point=n_point, n_spot=n_spot, n_directional=n_dir, posed=posed, seed=seed,
                tshadow_in_force=bool(mesh and triangle_shadows and shadow))
    flags = dict(spot=n_spot > 0, strict=strict, triangle_shadows=mesh and triangle_shadows)
    return _finish("random", index, "random-%d" % index, folder, text, flags, radii, lens, w, h, kw, ray_rng, meta)


# ---- the edge families: a floor sphere whose top is the plane y = 0 about the origin (spot_check.FLOOR) under spot_check.CAMERA ----
W, H = 64, 48
FLOOR_BOX = ((-6.0, 0.2, -4.0), (6.0, 8.0, 9.0))
FLOOR_MATERIAL = "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1"


def _floor_text(*, spheres=(), tris=(), points=(), spots=(), directional=(), camera=CAMERA, floor=FLOOR):
    lines = [camera, "background .1 .2 .3", "ambient_light .3 .3 .3", FLOOR_MATERIAL, "sphere %g %g %g %g" % floor]
    for s in spheres:
        lines += ["material .5 .5 .6 .6 .7 .6 .3 .3 .3 16 0 0 0 1", "sphere " + _fmt(s)]
    k = 0
    for t in tris:
        lines += ["vertex " + _fmt(v) for v in t]
        lines += ["material .5 .4 .3 .6 .5 .4 .3 .3 .3 4 0 0 0 1", "triangle %d %d %d" % (k, k + 1, k + 2)]
        k += 3
    lines += ["point_light " + _fmt(p) for p in points] + ["spot_light " + _fmt(s) for s in spots] + ["directional_light " + _fmt(d) for d in directional]
    return "\n".join(lines) + "\n"


# cone_edges: one spot light per case whose circles c == c1 and c == c2 cross the frame.  The last two pairs have angle1 just below
# angle2: by half a degree (a ring of partly lit pixels a fraction of a pixel wide), and by 1e-4 degree (c1 and c2 some 15 binary32
# steps apart: a ring no pixel centre need fall into)
CONE_PAIRS = ((0, 0), (0, 30), (30, 30), (90, 90), (0, 180), (180, 180), (29.5, 30), (29.9999, 30))
CONE_COLOUR = (90.0, 60.0, 30.0)
DOWN_POS, TILT_POS = (0.5, 8.0, 1.0), (-2.0, 7.0, 0.0)
LEVEL_AXIS, LEVEL_TILT = (1.0, -0.1, 0.2), (-0.6, -0.3, 1.0)  # for the 90-degree pair: under a steep axis the whole floor is inside


# the first query rays of the straight-down cases fall along the light's axis: the floor point under the light has L = (0, 1, 0) exactly
# (DOWN_POS's height is chosen so that d * (1 / d) == 1 in binary32 there), c == 1 == c1 of the pair (0, 0): the edge c == c1 itself
AXIS_RAYS = tuple((DOWN_POS[0], y, DOWN_POS[2], np.inf, 0.0, -dy, 0.0, NO_TRIANGLE) for y, dy in ((2.0, 1.0), (3.0, 0.5), (5.0, 2.0), (7.0, 1.0)))


def _cone_edges(index):
    n = len(CONE_PAIRS)
    if index < 2 * n:
        a1, a2 = CONE_PAIRS[index % n]
        tilted = index >= n
        if tilted:  # axis length 1e3, behind one point light: sp.first == 1, the pairs are (point, spot)
            axis = np.array(LEVEL_TILT if (a1, a2) == (90, 90) else (0.45, -1.0, 0.3)) * 1e3
            spot = (*CONE_COLOUR, *TILT_POS, *axis, a1, a2)
            points = [(30, 30, 30, 3.0, 9.0, -2.0)]
        else:  # axis length 1e-3, alone: sp.first == 0, a tail
            axis = np.array(LEVEL_AXIS if (a1, a2) == (90, 90) else (0.0, -1.0, 0.0)) * 1e-3
            spot = (*CONE_COLOUR, *DOWN_POS, *axis, a1, a2)
            points = []
        return dict(name="%s_%g_%g" % ("tilted" if tilted else "down", a1, a2), text=_floor_text(points=points, spots=[spot]), off=_floor_text(points=points),
                    radii=[0.0] * (len(points) + 1), kw=dict(shadow=True), meta=dict(pair=(a1, a2), tilted=tilted), head=None if tilted else AXIS_RAYS)
    if index == 2 * n:  # the light below the floor looks up: every floor point has N . L < 0, the cone still decides the shadow rays
        spot = (*CONE_COLOUR, 0.0, -3.0, 2.0, 0.0, 1.0, 0.0, 20, 40)
        return dict(name="below_the_floor", text=_floor_text(spots=[spot]), off=_floor_text(), radii=[0.0], kw=dict(shadow=True), meta=dict())
    if index == 2 * n + 1:
        spot = (*CONE_COLOUR, *DOWN_POS, 0.0, -1e-3, 0.0, 0, 30)
        return dict(name="lens", text=_floor_text(spots=[spot]), off=_floor_text(), radii=[0.0], kw=dict(shadow=True, jsample=2, seed=5), lens=(0.4, 11.0), meta=dict())
    return None


# pair_shapes: two narrow spot lights A and B whose floor discs overlap partly (all four in / out shapes of the pair in one frame), two
# small spheres on the floor inside the overlap, and a third one 4 above it: its shadows from A and from B fall 3 apart, both inside the
# overlap, so where A's shadow falls the sphere is in A's mask cell and not in B's — there the union of the masks matters (a shadow next
# to its sphere, as those of the two on the floor, lies in the same cell of both lights' tables)
PAIR_A = (90.0, 30.0, 30.0, -1.0, 8.0, 1.0, 0.0, -2.0, 0.0, 15, 25)
PAIR_B = (30.0, 30.0, 90.0, 2.0, 8.0, 1.5, 0.0, -0.5, 0.0, 15, 25)
PAIR_POINT = (30.0, 30.0, 30.0, -3.0, 9.0, -2.0)
PAIR_SPHERES = ((0.2, 0.4, 1.0, 0.4), (1.0, 0.3, 2.2, 0.3), (0.5, 4.0, 1.2, 0.5))
PAIR_R = 0.6
PAIR_RADII = ((0.0, 0.0), (PAIR_R, 0.0), (0.0, PAIR_R), (PAIR_R, PAIR_R))


# (under spot_check.FLOOR's radius of 1000 the masks' margins, which grow with the scene's extent, put every sphere into every cell:
# these scenes stand on a ground of radius 40, where a cell names the spheres near its direction alone)
PAIR_FLOOR = (0.0, -40.0, 0.0, 40.0)


def pair_text(a=True, b=True, point=False):
    return _floor_text(spheres=PAIR_SPHERES, points=[PAIR_POINT] if point else [], spots=([PAIR_A] if a else []) + ([PAIR_B] if b else []), floor=PAIR_FLOOR)


def _pair_shapes(index):
    if index < 16:
        point, shadow, ra = bool(index & 1), bool(index & 2), PAIR_RADII[index >> 2]
        name = "%s_%s_r%g_%g" % ("behind_a_point" if point else "spots_only", "shadow" if shadow else "lit", *ra)
        return dict(name=name, text=pair_text(point=point), off=pair_text(False, False, point), radii=([0.0] if point else []) + list(ra), kw=dict(shadow=shadow, seed=3 + index),
                    meta=dict(point=point))
    if index == 16:
        return dict(name="lens", text=pair_text(point=True), off=pair_text(False, False, True), radii=[0.0, PAIR_R, 0.0], kw=dict(shadow=True, jsample=2, seed=9), lens=(0.4, 11.0),
                    meta=dict(point=True))
    return None


# ball_meets_geometry: the ball of a light with a radius cuts, contains or touches geometry, and holds shaded points
TEN_SPHERES = tuple((-4.0 + 0.9 * k, 0.35, -1.0 + 0.6 * ((3 * k) % 5), 0.35) for k in range(10))


def _ball_meets_geometry(index):
    lit = (60.0, 60.0, 60.0)
    cases = [
        dict(name="ball_cuts_floor_and_sphere", spheres=[(1.2, 0.8, 1.5, 0.8)], points=[(*lit, 0.0, 0.5, 1.0)], radii=[1.0]),
        dict(name="centre_inside_a_smaller_sphere", spheres=[(0.0, 2.0, 1.0, 0.5)], points=[(*lit, 0.0, 2.0, 1.0)], radii=[1.5]),
        dict(name="centre_on_a_surface", spheres=[(0.0, 1.0, 1.0, 1.0)], points=[(*lit, 0.0, 2.0, 1.0)], radii=[0.7]),
        dict(name="shaded_points_inside_the_ball", spheres=[(2.5, 0.5, 2.0, 0.5)], spots=[(*lit, 0.0, 1.0, 1.0, 0.0, -1.0, 0.0, 60, 90)], radii=[2.5]),
        # pairs (soft, hard) and (hard spot, hard): 11 spheres, so the masks exist; the first pair must ignore them, the second use them
        dict(name="soft_and_hard_pairs_with_masks", spheres=TEN_SPHERES, points=[(*lit, -2.0, 6.0, 0.0), (40.0, 20.0, 20.0, 3.0, 5.0, 3.0)],
             spots=[(20.0, 60.0, 90.0, 0.0, 7.0, 2.0, 0.1, -1.0, 0.0, 30, 50), (50.0, 50.0, 20.0, -3.0, 4.0, 4.0, 0.5, -1.0, -0.3, 40, 60)], radii=[0.8, 0.0, 0.0, 0.0]),
        dict(name="soft_and_hard_pairs_with_masks_gi", spheres=TEN_SPHERES, points=[(*lit, -2.0, 6.0, 0.0), (40.0, 20.0, 20.0, 3.0, 5.0, 3.0)],
             spots=[(20.0, 60.0, 90.0, 0.0, 7.0, 2.0, 0.1, -1.0, 0.0, 30, 50), (50.0, 50.0, 20.0, -3.0, 4.0, 4.0, 0.5, -1.0, -0.3, 40, 60)], radii=[0.0, 0.0, 0.0, 0.6],
             kw=dict(gillum=2, depth=2)),
        dict(name="lens", spheres=[(1.2, 0.8, 1.5, 0.8)], points=[(*lit, 0.0, 0.5, 1.0)], radii=[1.0], kw=dict(jsample=2), lens=(0.4, 11.0)),
    ]
    if index >= len(cases):
        return None
    c = cases[index]
    text = _floor_text(spheres=c["spheres"], points=c.get("points", ()), spots=c.get("spots", ()), floor=PAIR_FLOOR if "masks" in c["name"] else FLOOR)
    return dict(name=c["name"], text=text, radii=c["radii"], kw=dict(shadow=True, seed=11 + index, **c.get("kw", {})), lens=c.get("lens"), meta=dict())


# far_light: |Lp - P|^2 ~ 1.2e30 lies outside len_terms' short range [2^-98, 2^98]: the correctly rounded fallback; a colour of 1e30 still shades
FAR_POS = (3e14, 1e15, -2e14)
FAR_COLOUR = (1.1e30, 0.9e30, 0.7e30)
NEAR_POINT = (30.0, 30.0, 30.0, -3.0, 9.0, -2.0)


def _far_light(index):
    sphere = [(0.0, 1.0, 1.0, 1.0)]
    dim = (5.0, 5.0, 5.0, 2.0, 6.0, 3.0, 0.0, -1.0, 0.0, 20, 40)  # a spot light as the tail, so that the far point light without a radius meets the cone loop too
    cases = [
        dict(name="point", points=[NEAR_POINT, (*FAR_COLOUR, *FAR_POS)], spots=[dim], off=dict(points=[NEAR_POINT], spots=[dim]), radii=[0.0, 0.0, 0.0], off_radii=[0.0, 0.0]),
        dict(name="point_with_a_radius", points=[(*FAR_COLOUR, *FAR_POS), NEAR_POINT], off=dict(points=[NEAR_POINT]), radii=[2e14, 0.0], off_radii=[0.0]),
        dict(name="spot", points=[NEAR_POINT], spots=[(*FAR_COLOUR, *FAR_POS, -3.0, -10.0, 2.0, 0, 90)], off=dict(points=[NEAR_POINT]), radii=[0.0, 0.0], off_radii=[0.0]),
        dict(name="spot_with_a_radius_gi", points=[NEAR_POINT], spots=[(*FAR_COLOUR, *FAR_POS, -3.0, -10.0, 2.0, 20, 120)], off=dict(points=[NEAR_POINT]), radii=[0.5, 1e14],
             off_radii=[0.5], kw=dict(gillum=2, depth=2)),
        dict(name="lens", points=[(*FAR_COLOUR, *FAR_POS), NEAR_POINT], off=dict(points=[NEAR_POINT]), radii=[2e14, 0.0], off_radii=[0.0], kw=dict(jsample=2), lens=(0.4, 11.0)),
    ]
    if index >= len(cases):
        return None
    c = cases[index]
    return dict(name=c["name"], text=_floor_text(spheres=sphere, points=c["points"], spots=c.get("spots", ())), off=_floor_text(spheres=sphere, **c["off"]), radii=c["radii"],
                kw=dict(shadow=True, seed=21 + index, **c.get("kw", {})), lens=c.get("lens"), meta=dict(off_radii=c["off_radii"]))


# sampled_far_end: triangle shadows under lights with a radius: the far end of the walk is the distance to the sample, drawn again.
# The accept region of a triangle (v0, v1, v2) is the mirrored triangle (v0, 2 v0 - v1, v2).
ABOVE_CENTRE = ((2.0, 5.7, -1.0), (5.0, 5.7, -1.0), (2.0, 5.7, 4.0))  # accepts over (-1..2, -1..4): 0.7 above the light at (0.8, 5, 0.5), inside its ball of 1.5
FAR_END_MESH_SEED = 12  # 244 triangles, several chunks; its triangle shadows show at some 900 of the 3072 pixels


def _sampled_far_end(index, folder):
    lit = (60.0, 60.0, 60.0)
    st = dict(shade_triangles=True, shadow=True)
    if index == 3:  # a random mesh large enough for a chunk tree, its own camera
        text = _mesh_scene_text(np.random.default_rng(FAR_END_MESH_SEED), folder, "sampled_far_end_mesh.tmp").rstrip("\n")
        text += "\npoint_light 40 40 40 1 6 2\nspot_light 90 60 60 -2 7 5 0.2 -1 -0.1 45 90\n"
        return dict(name="random_mesh", text=text, radii=[0.8, 0.5], kw=dict(seed=34, **st), meta=dict(), box=_box(text))
    cases = {
        0: dict(name="occluder_between", tris=[OCCLUDER], points=[(*lit, 4.0, 6.0, 1.0)], radii=[0.8]),
        1: dict(name="triangle_behind_the_centre_inside_the_ball", tris=[ABOVE_CENTRE], points=[(*lit, 0.8, 5.0, 0.5)], radii=[1.5]),
        2: dict(name="coincident_triangles", tris=[OCCLUDER, OCCLUDER], points=[(*lit, 4.0, 6.0, 1.0)], radii=[0.8]),
        4: dict(name="lens", tris=[OCCLUDER], points=[(*lit, 4.0, 6.0, 1.0)], radii=[0.8], kw=dict(jsample=2), lens=(0.4, 11.0)),
        5: dict(name="spot_behind_the_centre_inside_the_ball", tris=[ABOVE_CENTRE, OCCLUDER], points=[(20.0, 20.0, 20.0, -3.0, 9.0, -2.0)],
                spots=[(*lit, 0.8, 5.0, 0.5, 0.1, -1.0, 0.0, 40, 70), (30.0, 30.0, 60.0, 4.0, 6.0, 1.0, 0.0, -1.0, 0.0, 50, 80)], radii=[0.0, 1.5, 0.8]),
        6: dict(name="occluder_between_gi", tris=[OCCLUDER], points=[(*lit, 4.0, 6.0, 1.0), (20.0, 20.0, 20.0, -3.0, 9.0, -2.0)], radii=[0.8, 0.0], kw=dict(gillum=2, depth=2)),
    }
    if index not in cases:
        return None
    c = cases[index]
    return dict(name=c["name"], text=_floor_text(tris=c["tris"], points=c["points"], spots=c.get("spots", ())), radii=c["radii"], kw=dict(seed=31 + index, **st, **c.get("kw", {})),
                lens=c.get("lens"), meta=dict())


_FAMILIES = {"cone_edges": lambda i, folder: _cone_edges(i), "pair_shapes": lambda i, folder: _pair_shapes(i), "ball_meets_geometry": lambda i, folder: _ball_meets_geometry(i),
             "far_light": lambda i, folder: _far_light(i), "sampled_far_end": _sampled_far_end}
COUNTS = {"cone_edges": 2 * len(CONE_PAIRS) + 2, "pair_shapes": 17, "ball_meets_geometry": 7, "far_light": 5, "sampled_far_end": 7}
EDGE = [(family, i) for family, n in COUNTS.items() for i in range(n)]
RANDOM = [("random", i) for i in range(RANDOM_CASES)]


def build(family, index, folder, seed=SEED):
    """The case (family, index), its scene written into folder."""
    if family == "random":
        return random_case(index, folder, seed)
    c = _FAMILIES[family](index, folder)
    if c is None:
        raise KeyError((family, index))
    rng = np.random.default_rng([SEED, sorted(_FAMILIES).index(family) + 1000, index])
    text = c["text"]
    flags = dict(spot="spot_light" in text, strict=False, triangle_shadows=family == "sampled_far_end")
    meta = dict(c["meta"], off_text=c.get("off"))
    case = _finish(family, index, "%s-%d" % (family, index), folder, text, flags, c["radii"], c.get("lens"), W, H, c["kw"], rng, dict(meta, what=c["name"]), c.get("box", FLOOR_BOX))
    if c.get("head"):
        case.rays[:len(c["head"])] = np.array(c["head"], np.float32)
    return case


def case_id(fi):
    return "%s-%d" % fi


def variant_name(case, n_triangles):
    """Renderer.kernel_variant() of the case's frame, from its features"""
    part = "_soft" if (np.asarray(case.radii) > 0).any() else "_spot"
    in_force = case.flags["triangle_shadows"] and case.kw.get("shade_triangles") and case.kw.get("shadow") and n_triangles > 0
    return "level_pipeline_g1" + part + ("_lens" if case.lens else "") + ("_tshadow" if in_force else "")


def query_options(case):
    """the option keywords of the case's shading query: its frame's, without what makes a frame of samples"""
    return {k: v for k, v in case.kw.items() if k not in ("jsample", "progressive", "fov")}


def checker_frame(soft, lens, case, spots, cones, *, scene=None, radii=None, aperture=None, **over):
    """(bytes, floats, stats[5]) of the case's frame from the checkers: soft_light_check.Checker.render, or lens_check.Checker.render /
    render_progressive under a lens; two progressive passes without a lens are pyoracle.render_progressive's steps over the soft
    checker's frames.  spots, cones: the library's rows and cones of the scene.  scene, radii, aperture and the option keywords in
    `over` replace the case's (a lens checker frame at aperture 0 is asked for with aperture=0.0)."""
    from oracle import pyoracle
    kw = {**case.kw, **over}
    passes = kw.pop("progressive", 1)
    common = dict(radii=case.radii if radii is None else radii, spots=spots, cones=cones, triangle_shadows=case.flags["triangle_shadows"], strict=case.flags["strict"])
    path = scene or case.scene
    if case.lens is not None or aperture is not None:
        A, F = case.lens if case.lens is not None else (0.0, 1.0)
        A = A if aperture is None else aperture
        if passes > 1:
            return lens.render_progressive(path, case.w, case.h, passes, aperture=A, focus=F, **common, **kw)
        return lens.render(path, case.w, case.h, aperture=A, focus=F, **common, **kw)
    if passes == 1:
        return soft.render(path, case.w, case.h, **common, **kw)
    acc, stats = None, np.zeros(5, np.uint64)
    seed = kw.pop("seed", 1)
    for k in range(passes):
        _, f, st = soft.render(path, case.w, case.h, seed=(seed + k) & 0xFFFFFFFFFFFFFFFF, **common, **kw)
        acc = f.copy() if acc is None else acc + f
        stats += st
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = acc / np.float32(passes)
    return pyoracle.quantise(mean), mean, stats
