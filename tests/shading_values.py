"""Material, colour and light values the suite never rendered, shared by tests/test_shading_values_cpu.py (what each case reaches, on
the CPU oracle alone) and tests/test_shading_values_gpu.py (every render path against the oracle, bit for bit).  Seeded, numpy only.

The scene (scene()): the ground sphere, six small spheres near the camera, one large sphere in front of it with the key light close to
the view direction, so that a tight highlight covers pixels at 64x36 (SIZE, fov 40), and a fill light.  `power` is the Phong exponent
of the large sphere and of every other small one (the family), `other` that of the rest.  A case (CASES) is the keywords of scene(),
the option keywords and loader flags that belong to it, and what it must reach, held by tests/test_shading_values_cpu.py:

    family "exponent"   integer exponents 127 .. 1024.  For n >= 128 the oracle's bytes differ at >= 16 pixels from those of the same
                        scene with n & 127 (0 staying exponent 0: what seven squarings would render, device_math.h pow_int_flat<7>), and
                        at >= 1 pixel from those of n - 1 and of n + 1.
    family "cold"       exponents 0, 0.5, -2, 1e6, and 1025 beside 64 (pow_steps stays 7): device_math.h powf_spec_cold.  The float
                        frame differs from the exponent-8 frame at >= 16 pixels.
    family "triangle"   the scene's largest integer exponent on a triangle material only (spheres at 8), and the converse, under
                        --shade-triangles: api.cpp reads tri_mats for pow_steps.  The same conditions as "exponent".
    family "colour"     negative diffuse, diffuse and specular of 3, specular exactly 0 and -0 under --legacy-reflect (the != 0 gate:
                        both cast fewer rays than a specular of 1e-3, and the same number), ambient light 2 and -0.5, a background
                        outside [0, 1].
    family "light"      colour 0, negative, 1e38; a light at the camera (H = L); on the line camera -> large sphere's centre behind the
                        sphere (also without shadows, where that light is shaded: no pixel of an even-sized frame lies on the axis, so
                        H is near-degenerate, not NaN: |view + L| falls below 0.05 at a hit point, where it is about 2 elsewhere, and
                        H is the quotient of that cancellation); 0.01 above the large sphere and inside it;
                        2^49.4, 2^49.6 and 1e20 away along FAR_DIRECTION (|to_l|^2 inside len_terms' fast range [2^-98, 2^99), outside
                        it, and inf: L = 0); two coincident lights; under the strict loader a directional light of direction 0 and one
                        of length 1e-30 (L is NaN, max0 takes it to 0: the base frame with one more shadow ray per hit).
`reach` names the condition on the oracle's frame: "negative" (negative floats at >= 16 pixels, and there bytes that are neither 0 nor
255: the quantiser's wrap), "overflow" (+inf or NaN at >= 16 pixels), "bright" (values above 1 at >= 16 pixels), or None.

NaN.  A case with `nan` set has NaN in the oracle's frame (held on the CPU; no other case has).  The kernels' NaN words are compared
like every other word: the products that make them (inf * 0) give the same default NaN on both sides.

Unit records.  pow_records(): skr_debug_eval op 20 — every integer p in 1 .. 1024 against POW_X (64 values) and against 16 random x in
[0.97, 1] each, at steps = bit_length(p) and at steps = 11, and the exponents POW_COLD, which are not plain, at every steps in 1 .. 11.
In the 1 .. 1024 x [0.97, 1] block every reference result but those of x == 1 is neither 0, 1, inf nor NaN (0.97^1024 = 2.8e-14): the
share is asserted at >= 0.99.  quantise_values(): the negative numbers of the quantiser, every one below -2^31 / 255 returning 0 by
the oracle's own guard (no float-to-int cast out of range is asked of its C).
"""
import collections
import math

import numpy as np

f32 = np.float32
SIZE = (64, 36)
FOV = 40.0
CAMERA = (0.0, 2.0, -10.0, 0.0, -0.1, 0.9, 0.0, 1.0, 0.0)  # position, direction, up
BIG = (0.0, 0.7, 2.0, 5.0)                                  # the large sphere: centre, radius
SMALL = [(-2.2, 0.45, -4.5, 0.45), (2.2, 0.45, -4.5, 0.45), (-1.4, 0.4, -6.0, 0.4), (1.5, 0.4, -6.0, 0.4), (-3.0, 0.5, -3.0, 0.5), (3.0, 0.5, -3.0, 0.5)]
KEY_POSITION = (0.4, 2.6, -9.5)
KEY_COLOUR = (60.0, 55.0, 50.0)
FILL = ((20.0, 18.0, 15.0), (-6.0, 8.0, -4.0))
FAR_DIRECTION = (-0.3, 0.8, -0.52)
FAR_COLOUR = (2e30, 1.5e30, 1e30)  # times 1 / d^2 = 2^-98.8: a few units
# the triangle of the "triangle" family: what the frame shows of it (utils.h:181-213 accepts the triangle mirrored at v0) faces the
# camera around a point left of the view axis, so that the key light's highlight lies on it
TRI_CENTRE = (-1.3, 2.3, -5.0)


def _fmt(v):
    v = float(v)
    if v == 0.0 and math.copysign(1.0, v) < 0:
        return "-0"
    return "%.9g" % f32(v)


def _line(word, *vals):
    return word + " " + " ".join(_fmt(v) for v in vals)


def _material(ambient, diffuse, specular, power):
    return _line("material", *ambient, *diffuse, *specular, power, 0, 0, 0, 1)


def triangle_vertices():
    """The file's (v0, v1, v2) of the family's triangle: the shown triangle (v0, 2 v0 - v1, v2) is an equilateral one of circumradius
    1.1 around TRI_CENTRE in the plane that faces the camera."""
    q, cam = np.array(TRI_CENTRE), np.array(CAMERA[:3])
    n = (cam - q) / np.linalg.norm(cam - q)
    u = np.cross(n, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(u, n)
    a, b, c = (q + 1.1 * (math.cos(t) * u + math.sin(t) * v) for t in (math.pi / 2, math.pi * 7 / 6, math.pi * 11 / 6))
    return a, 2 * a - b, c


def scene(power=8.0, other=8.0, big_diffuse=(0.02, 0.015, 0.01), big_specular=(0.9, 0.8, 0.7), small_diffuse=(0.5, 0.4, 0.6), small_specular=(0.6, 0.5, 0.3),
          ambient=(0.3, 0.3, 0.3), background=(0.2, 0.3, 0.5), key_position=KEY_POSITION, key_colour=KEY_COLOUR, more_lights=(FILL,), directional=(),
          triangle=None, extra_triangle=False):
    """The scene's lines.  triangle: the exponent of the family's triangle (None: no triangle); extra_triangle: a small triangle at
    the right edge with an exponent of 8, for the paths that need a mesh in a case that has none."""
    lines = [_line("camera", *CAMERA, 30), _line("ambient_light", *ambient), _line("background", *background),
             "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1", "sphere 0 -40 0 40",
             _material((0.05, 0.05, 0.05), big_diffuse, big_specular, power), _line("sphere", *BIG)]
    for i, s in enumerate(SMALL):
        lines += [_material((0.1, 0.1, 0.05 * i), small_diffuse, small_specular, other if i % 2 else power), _line("sphere", *s)]
    nv = 0
    if triangle is not None:
        lines += [_line("vertex", *v) for v in triangle_vertices()]
        lines += [_material(*TRI_MATERIAL, triangle), "triangle 0 1 2"]
        nv = 3
    if extra_triangle:
        lines += ["vertex 2.6 2.2 -5", "vertex 1.8 2.2 -5", "vertex 2.6 3.2 -5", "material .1 .1 .1 .5 .4 .3 .4 .4 .4 8 0 0 0 1", "triangle %d %d %d" % (nv, nv + 1, nv + 2)]
    if key_colour is not None:
        lines.append(_line("point_light", *key_colour, *key_position))
    for colour, position in more_lights:
        lines.append(_line("point_light", *colour, *position))
    for colour, direction in directional:
        lines.append(_line("directional_light", *colour, *direction))
    return lines


TRI_MATERIAL = ((0.05, 0.05, 0.05), (0.02, 0.015, 0.01), (0.9, 0.8, 0.7))  # ambient, diffuse, specular of the family's triangle


def triangle_materials(case):
    """float32 [1, 10] = ambient diffuse specular power of the case's triangle, as Scene.from_arrays(triangle_materials=) takes them:
    the numbers of the `material` line scene() writes in front of it."""
    return np.array([[*TRI_MATERIAL[0], *TRI_MATERIAL[1], *TRI_MATERIAL[2], case.scene["triangle"]]], f32)


def text(case, **over):
    return "\n".join(scene(**dict(case.scene, **over))) + "\n"


def write(case, path, **over):
    """The case's scene into path; over: keywords of scene() that replace the case's (the reach tests' variations)."""
    with open(path, "w") as f:
        f.write(text(case, **over))
    return path


Case = collections.namedtuple("Case", "name family scene kw load reach nan mesh")


def _c(name, family, scene_kw=None, kw=None, load=None, reach=None, nan=False):
    scene_kw = dict(scene_kw or {})
    return Case(name, family, scene_kw, dict(dict(fov=FOV), **(kw or {})), dict(load or {}), reach, nan, scene_kw.get("triangle") is not None)


def _along(frm, to, dist_beyond):
    a, b = np.array(frm, np.float64), np.array(to, np.float64)
    d = (b - a) / np.linalg.norm(b - a)
    return tuple(b + d * dist_beyond)


def _far(dist):
    d = np.array(FAR_DIRECTION) / np.linalg.norm(FAR_DIRECTION)
    return tuple(d * dist)


EXPONENTS = (127, 128, 255, 256, 1000, 1023, 1024)
COLD = (0.0, 0.5, -2.0, 1e6)
_TOP = (BIG[0], BIG[1] + BIG[3] * 0.6, BIG[2] - BIG[3] * 0.8)  # a point of the large sphere's surface that the camera sees (3-4-5)

CASES = [_c("exp_%d" % n, "exponent", dict(power=float(n))) for n in EXPONENTS]
CASES += [_c("exp_%s" % ("%g" % p).replace("-", "m").replace(".", "_").replace("+", ""), "cold", dict(power=p)) for p in COLD]
CASES += [
    _c("exp_1025_beside_64", "cold", dict(power=1025.0, other=64.0)),
    _c("tri_256_spheres_8", "triangle", dict(triangle=256.0), kw=dict(shade_triangles=True)),
    _c("spheres_256_tri_8", "triangle", dict(power=256.0, triangle=8.0), kw=dict(shade_triangles=True)),
    # ---- colours
    _c("diffuse_negative", "colour", dict(big_diffuse=(-0.3, -0.2, -0.4), small_diffuse=(-0.5, 0.4, -0.1)), reach="negative"),
    _c("diffuse_specular_3", "colour", dict(big_diffuse=(3, 3, 3), big_specular=(3, 3, 3), small_diffuse=(3, 3, 3), small_specular=(3, 3, 3)), reach="bright"),
    _c("specular_zero_legacy", "colour", dict(big_specular=(0.0, 0.0, 0.0), small_specular=(0.0, 0.0, 0.0)), kw=dict(legacy_reflect=True)),
    _c("specular_negzero_legacy", "colour", dict(big_specular=(-0.0, -0.0, -0.0), small_specular=(-0.0, -0.0, -0.0)), kw=dict(legacy_reflect=True)),
    _c("ambient_2", "colour", dict(ambient=(2, 2, 2)), reach="bright"),
    _c("ambient_negative", "colour", dict(ambient=(-0.5, -0.5, -0.5)), reach="negative"),
    _c("background_outside", "colour", dict(background=(1.5, -0.25, 2.0)), reach="negative"),
    # ---- lights
    _c("light_zero", "light", dict(key_colour=(0.0, 0.0, 0.0))),
    _c("light_negative", "light", dict(key_colour=(-30.0, -20.0, -40.0)), reach="negative"),
    # (half a unit above the large sphere, whose colours are 3: 1 / d^2 up to 4 takes k * 1e38 to inf, and away from the highlight of an
    # exponent of 1000 the power is 0: inf * 0, NaN)
    _c("light_1e38", "light", dict(key_colour=(1e38, 1e38, 1e38), key_position=_along(BIG[:3], _TOP, 0.5), power=1000.0, big_diffuse=(3, 3, 3), big_specular=(3, 3, 3)),
       reach="overflow", nan=True),
    _c("light_at_camera", "light", dict(key_position=CAMERA[:3])),
    _c("light_behind_sphere", "light", dict(key_position=_along(CAMERA[:3], BIG[:3], BIG[3] + 2.0))),
    _c("light_behind_sphere_no_shadows", "light", dict(key_position=_along(CAMERA[:3], BIG[:3], BIG[3] + 2.0)), kw=dict(shadow=False)),
    _c("light_near_surface", "light", dict(key_position=_along(BIG[:3], _TOP, 0.01))),
    _c("light_inside_sphere", "light", dict(key_position=(BIG[0] + 0.5, BIG[1] + 1.0, BIG[2] - 2.0))),
    _c("light_far_2p49_4", "light", dict(key_position=_far(2.0 ** 49.4), key_colour=FAR_COLOUR)),
    _c("light_far_2p49_6", "light", dict(key_position=_far(2.0 ** 49.6), key_colour=FAR_COLOUR)),
    _c("light_far_1e20", "light", dict(key_position=_far(1e20), key_colour=FAR_COLOUR)),
    _c("lights_coincident", "light", dict(more_lights=(FILL, (KEY_COLOUR, KEY_POSITION)))),
    _c("directional_zero", "light", dict(directional=(((0.5, 0.4, 0.3), (0.0, 0.0, 0.0)),)), load=dict(strict=True)),
    _c("directional_1e_30", "light", dict(directional=(((0.5, 0.4, 0.3), (0.0, -1e-30, 2e-31)),)), load=dict(strict=True)),
]
BY_NAME = {c.name: c for c in CASES}
FAR = {"light_far_2p49_4": "inside", "light_far_2p49_6": "outside", "light_far_1e20": "inf"}
# the families rendered once each through the other copies of the Blinn-Phong term (shade_common.h: cones / soft lights, fog)
COPIES = [c for c in CASES if c.family in ("exponent", "cold")]


def integer_exponents(case, extra_triangle=False):
    """The integer exponents in [1, 1024] among the materials of the case's scene (api.cpp: the ones pow_steps looks at)."""
    s = dict(dict(power=8.0, other=8.0, triangle=None), **case.scene)
    ps = [8.0, s["power"], s["other"]] + ([s["triangle"]] if s["triangle"] is not None else []) + ([8.0] if extra_triangle else [])
    return [int(p) for p in ps if 1.0 <= p <= 1024.0 and p == round(p)]


def pow_steps(case):
    """api.cpp: the bit length of the scene's largest integer exponent."""
    return max(integer_exponents(case)).bit_length()


def leaf_shape(case):
    """launch.h skr_leaf_shape for the case under shadow=True, a gillum frame and the default switches: 1 or 2 = the instance with that
    many point lights compiled in, 0 = the one that reads the launch's facts at run time."""
    s = dict(dict(key_colour=KEY_COLOUR, more_lights=(FILL,), directional=(), triangle=None), **case.scene)
    lights = (s["key_colour"] is not None) + len(s["more_lights"])
    far = max(np.linalg.norm(np.array(s.get("key_position", KEY_POSITION), np.float64)), 100.0)
    if far >= 1e18:  # scene_host.cpp build_shadow_masks: no masks for a reach beyond binary32's square root, and no shape without masks
        return 0
    if s["triangle"] is not None or (case.load.get("strict") and s["directional"]) or pow_steps(case) > 7 or not 1 <= lights <= 2 or not case.kw.get("shadow", True):
        return 0
    return lights


def seven_step_exponent(n):
    """The exponent pow_int_flat<7> would raise to, were it handed n."""
    return float(int(n) & 127)


# -------------------------------------------------------------------------------------------------------------- unit records ----
def _ulps_below_one(k):
    return (np.array(0x3f800000 - k, np.uint32)).view(f32)


POW_X = np.concatenate([
    f32([0.0, -0.0, 1e-40, 2.0 ** -126, 1e-30, 1e-10, 1e-3, 0.25, 0.5, 0.75, 0.9, 0.97, 0.98, 0.99, 0.995, 0.999, 0.9995, 0.9999, 0.99999, 0.999999]),
    np.array([_ulps_below_one(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 16, 64, 256)], f32),
    f32([1.0, np.nextafter(f32(1), f32(2)), 1.0000002, 1.0000005, 1.000001, 1.0001, 1.01, 1.5, 2.0, 3.0, 1e10, 3.4028235e38, np.inf, np.nan, -0.5, -1.0, -np.inf]),
    np.linspace(0.9, 0.9999, 16).astype(f32),
])
POW_COLD = f32([0.0, -0.0, 0.5, 0.99999994, -2.0, 2.5, 127.5, np.nextafter(f32(1024), f32(np.inf)), 1025.0, 1e6, np.inf, np.nan, 1e-40])
POW_RANDOM_PER_P = 16


def pow_records():
    """(records uint32 [n, 3] = x, p, steps of skr_debug_eval op 20; le7 bool [n]: the LE7 word is asserted; block int [n]: 0 = the
    integers against POW_X, 1 = the integers against random x in [0.97, 1], 2 = POW_COLD)."""
    rng = np.random.default_rng(20)
    p = np.arange(1, 1025)
    bits = np.array([int(v).bit_length() for v in p])
    rows = []

    def block(x, pp, steps, tag):
        x, pp, steps = np.broadcast_arrays(f32(x), f32(pp), np.asarray(steps, np.uint32))
        rows.append((x.ravel().copy(), pp.ravel().copy(), steps.ravel().astype(np.uint32), np.full(x.size, tag)))

    for steps in (bits[:, None], 11):
        block(POW_X[None, :], p[:, None], steps, 0)
    xr = (0.97 + 0.03 * rng.random((1024, POW_RANDOM_PER_P))).astype(f32)
    for steps in (bits[:, None], 11):
        block(xr, p[:, None], steps, 1)
    block(POW_X[None, None, :], POW_COLD[None, :, None], np.arange(1, 12)[:, None, None], 2)
    x, pp, steps, tag = (np.concatenate(c) for c in zip(*rows))
    rec = np.stack([x.view(np.uint32), pp.view(np.uint32), steps], 1)
    with np.errstate(invalid="ignore"):
        le7 = (tag == 2) | (pp <= 127)
    return rec, le7, tag


QUANTISE_EDGES = f32([-0.0, -1.0 / 255, -0.5, -1.0, -1.004, -256.0 / 255, -1e3, -8421504.5, -8.5e6, -1e30, -np.inf])


def quantise_values():
    rng = np.random.default_rng(5)
    return np.concatenate([QUANTISE_EDGES, (-300.0 * rng.uniform(1e-6, 1.0 - 1e-6, 4096)).astype(f32)])
