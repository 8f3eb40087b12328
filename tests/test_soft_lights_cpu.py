"""Lights with a radius on the host (no GPU; include/skr.h skr_scene_set_light_radii): the CPU checker pinned to the frozen
oracle and to the spot checker while every radius is 0, the sample rule against a numpy restatement, the setter and getter clause by
clause, and the picture-level property of the rule — a penumbra — on the checker alone."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import ROOT, scene_path
from oracle import pyoracle
from soft_light_check import build as build_checker
from spot_check import CAMERA, FLOOR, MIXED_POINTS, MIXED_SPOTS, OCCLUDER, build as build_spot_checker, write_floor_scene
from test_spot_cpu import NO_SPOT

f32 = np.float32


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("softlightcheck")))


@pytest.fixture(scope="session")
def spot_checker(tmp_path_factory):
    return build_spot_checker(str(tmp_path_factory.mktemp("softlight_spotcheck")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. with every radius 0 the checker is the oracle, and the spot checker: only after this is it evidence ----
@pytest.mark.parametrize("name,scn,w,h,kw", NO_SPOT, ids=[c[0] for c in NO_SPOT])
def test_checker_is_the_oracle_with_all_radii_zero(checker, name, scn, w, h, kw):
    sc = pyoracle.OracleScene(scene_path(scn), strict=kw.get("strict", False))
    opt = {k: v for k, v in kw.items() if k != "strict"}
    o_rgb, o_f, o_st = pyoracle.render(sc, w, h, want_float=True, **opt)
    for radii in (None, 0.0):
        rgb, f, st = checker.render(sc, w, h, radii=radii, **opt)
        assert np.array_equal(rgb, o_rgb) and np.array_equal(bits(f), bits(o_f))
        assert st.tolist() == o_st.tolist()  # all five


@pytest.mark.parametrize("kw", [dict(shadow=True), dict(shade_triangles=True, shadow=True, triangle_shadows=True),
                                dict(gillum=2, depth=2, shadow=True, seed=4), dict(jsample=2, shadow=True, seed=9)],
                         ids=["shadow", "tshadow", "gi2", "js2"])
def test_checker_is_the_spot_checker_with_all_radii_zero(checker, spot_checker, tmp_path, kw):
    mixed = write_floor_scene(str(tmp_path / "mixed.scn"), points=MIXED_POINTS, spots=MIXED_SPOTS, tris=[OCCLUDER], directional=True)
    for scn, strict in ((mixed, True), (scene_path("test.scn"), False)):
        sc = skr.parse_scene(scn, spot=True, strict=strict)
        rows, cones = sc.spot_lights, sc.spot_cones
        assert len(rows) >= 1
        a = spot_checker.render(scn, 64, 48, spots=rows, cones=cones, strict=strict, **kw)
        b = checker.render(scn, 64, 48, spots=rows, cones=cones, radii=0.0, strict=strict, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2].tolist() == b[2].tolist()
    rays = np.zeros((40, 8), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2] = np.linspace(-6, 6, 40), 5.0, np.linspace(-3, 4, 40)
    rays[:, 3], rays[:, 5], rays[:, 7] = np.inf, -1.0, np.array([-1], np.int32).view(np.float32)[0]
    sc = skr.parse_scene(mixed, spot=True, strict=True)
    keys = np.arange(40, dtype=np.uint32) * 977
    a = spot_checker.shade(mixed, rays, spots=sc.spot_lights, cones=sc.spot_cones, strict=True, keys=keys, sample=2, **kw)
    b = checker.shade(mixed, rays, spots=sc.spot_lights, cones=sc.spot_cones, strict=True, keys=keys, sample=2, **kw)
    assert np.array_equal(bits(a[0]), bits(b[0])) and a[1].tolist() == b[1].tolist()


# ---- 2. the sample: sl_sample against the rule restated in numpy binary32 ----
def soft_ctr3(l):
    return (0x80000080 | (int(l) << 8)) & 0xFFFFFFFF


def philox7(ctr, key):
    """Philox4x32-7 (Salmon et al., SC'11) on uint32 [n, 4] counters and [n, 2] keys, in uint64 arithmetic."""
    c = [ctr[:, k].astype(np.uint64) for k in range(4)]
    k0, k1 = key[:, 0].astype(np.uint64), key[:, 1].astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(7):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, 1).astype(np.uint32)


def sincos_spec(phi):
    """the shared-math sin / cos of binary32 angles (oracle/skr_oracle.c sko_sincos_shared == device_math.h sincos_spec)"""
    L = pyoracle.lib()
    s, c = C.c_float(), C.c_float()
    out = np.zeros((len(phi), 2), np.float32)
    for i, p in enumerate(phi):
        L.sko_sincos_shared(C.c_float(float(p)), C.byref(s), C.byref(c))
        out[i] = s.value, c.value
    return out[:, 0], out[:, 1]


def sample_rule(rec):
    """The rule of include/skr.h on records uint32 [n, 10] = (pixel, aa, node, l, seed_lo, seed_hi, Lp(3) bits, R bits): every step one
    numpy float32 operation."""
    rec = np.ascontiguousarray(rec, np.uint32).reshape(-1, 10)
    fl = rec[:, 6:].copy().view(np.float32)
    Lp, R = fl[:, :3], fl[:, 3]
    ctr = np.stack([rec[:, 0], rec[:, 1], rec[:, 2], np.array([soft_ctr3(l) for l in rec[:, 3]], np.uint32)], 1)
    out = philox7(ctr, rec[:, 4:6])
    u1 = (out[:, 0] >> 1).astype(np.float32) * f32(2.0 ** -31)
    u2 = (out[:, 1] >> 1).astype(np.float32) * f32(2.0 ** -31)
    z = f32(1) - f32(2) * u1
    t = f32(1) - z * z
    s = np.sqrt(np.where(f32(0) < t, t, f32(0)))
    phi = f32(float.fromhex("0x1.921fb6p+2")) * u2
    sn, cs = sincos_spec(phi)
    got = np.stack([Lp[:, 0] + R * (s * cs), Lp[:, 1] + R * z, Lp[:, 2] + R * (s * sn)], 1)
    assert all(a.dtype == np.float32 for a in (u1, u2, z, t, s, phi, got))
    return np.where((R > 0)[:, None], got, Lp), u1, u2


def records(pixels, aas, nodes, ls, seeds, Lp, R):
    g = np.array(list(itertools.product(pixels, aas, nodes, ls, seeds)), dtype=np.uint64)  # (Python ints: 2^64 - 1 is no float)
    rec = np.zeros((len(g), 10), np.uint32)
    rec[:, :4] = g[:, :4].astype(np.uint32)
    rec[:, 4], rec[:, 5] = (g[:, 4] & np.uint64(0xFFFFFFFF)).astype(np.uint32), (g[:, 4] >> np.uint64(32)).astype(np.uint32)
    rec[:, 6:9] = bits(np.broadcast_to(np.asarray(Lp, np.float32), (len(g), 3)))
    rec[:, 9] = bits(np.broadcast_to(f32(R), (len(g),)))
    return rec


GRID = dict(pixels=[0, 1, 77, 160 * 120 - 1, 2 ** 32 - 1], aas=[0, 1, 3, 15], nodes=[0, 1, 2, 7, 85, 2 ** 31 + 5], ls=[0, 1, 2, 9, 5107, 2 ** 22 - 1],
            seeds=[0, 1, 7, 2 ** 32, 2 ** 64 - 1])


def test_the_sample_is_the_rule_in_numpy_binary32(checker):
    for Lp, R in (((0.0, 0.0, 0.0), 1.0), ((3.0, 9.5, -2.25), 0.5), ((-1e3, 4e-3, 77.0), 12.75), ((1.0, 2.0, 3.0), 1e-4)):
        rec = records(Lp=Lp, R=R, **GRID)
        want, u1, u2 = sample_rule(rec)
        got = checker.samples(rec)
        assert np.array_equal(bits(got), bits(want))
        assert 0 <= u1.min() and u1.max() <= 1 and 0 <= u2.min() and u2.max() <= 1
    # the single-record form agrees with the batch
    assert np.array_equal(bits(checker.sample(77, 3, 85, 9, 2 ** 32, (3.0, 9.5, -2.25), 0.5)),
                          bits(checker.samples(records([77], [3], [85], [9], [2 ** 32], (3.0, 9.5, -2.25), 0.5))[0]))


def test_the_sample_lies_on_the_sphere_within_six_roundings(checker):
    """About Lp = 0 the three additions are exact, so |Lp'| / R = sqrt(s^2 (cs^2 + sn^2) + z^2) but for the roundings, with e = 2^-24:
      s^2 = fl(sqrt(fl(1 - fl(z z))))^2 is within e z^2 + e (1 - z^2) + 2 e s^2 <= 3 e of 1 - z^2  (the product, the difference, the root);
      sn and cs are within 1.43 ulp <= 1.43 e of sin and cos (exhaustive), so cs^2 + sn^2 is within 2 * 1.43 e (|cs| + |sn|)
      <= 4.05 e of 1;
      the products s * cs, R * (.) and R * z add at most 2 e relative to each component, 4 e to the sum of squares.
    |Lp'|^2 / R^2 is within 3 e + 4.05 e + 4 e < 12 e of 1, |Lp'| / R within 6 e = 6 * 2^-24: three ulps of R at the least favourable
    R (just above a power of two), six at the most favourable."""
    for R in (1.0, 0.5, 12.75, 1e-4, 1.9999999, 3e4):
        rec = records(Lp=(0.0, 0.0, 0.0), R=R, **GRID)
        got = checker.samples(rec).astype(np.float64)
        r = np.sqrt((got ** 2).sum(1))
        assert np.abs(r / np.float64(f32(R)) - 1).max() <= 6 * 2.0 ** -24


def test_radius_zero_returns_the_position_bit_for_bit(checker):
    for Lp in ((3.0, 9.5, -2.25), (-0.0, 0.0, -0.0), (1e-40, -1e38, np.inf)):
        for R in (0.0, -0.0):
            rec = records(Lp=Lp, R=R, **GRID)
            assert np.array_equal(bits(checker.samples(rec)), np.broadcast_to(bits(np.asarray(Lp, np.float32)), (len(rec), 3)))


def test_every_word_of_the_node_reaches_the_draw(checker):
    """different l, node, aa, pixel and seed give different samples: change one word of a record at a time"""
    base = dict(pixels=[77], aas=[1], nodes=[7], ls=[2], seeds=[5])
    ref = checker.samples(records(Lp=(0, 0, 0), R=1.0, **base))[0]
    seen = {tuple(bits(ref))}
    for name, other in (("pixels", [78, 77 + 2 ** 31]), ("aas", [0, 2]), ("nodes", [6, 8, 7 + 2 ** 16]), ("ls", [0, 1, 3, 2 + 2 ** 21]), ("seeds", [4, 6, 5 + 2 ** 32])):
        for v in other:
            got = checker.samples(records(Lp=(0, 0, 0), R=1.0, **{**base, name: [v]}))[0]
            assert tuple(bits(got)) not in seen, (name, v)
            seen.add(tuple(bits(got)))


def test_the_counter_word_is_disjoint_from_the_other_draws():
    """over every l < 2^22: bit 31 set (the hemisphere draws' word child >> 1 is below 2^30), bit 7 set (fog_ctr3(l, j, pass) = 0x80000000 |
    l << 8 | j << 1 | pass with j < 64 leaves it clear), bits 0-6 clear (the jitter word is 0xFFFFFFFF), and distinct for distinct l"""
    l = np.arange(2 ** 22, dtype=np.uint64)
    w = (np.uint64(0x80000080) | (l << np.uint64(8))) & np.uint64(0xFFFFFFFF)
    assert w[0] == soft_ctr3(0) and w[-1] == soft_ctr3(2 ** 22 - 1) == 0xBFFFFF80
    assert ((w >> np.uint64(31)) == 1).all() and ((w >> np.uint64(7)) & np.uint64(1) == 1).all() and ((w & np.uint64(0x7F)) == 0).all()
    assert (w != np.uint64(0xFFFFFFFF)).all() and len(np.unique(w)) == len(w)
    fog_words = {0x80000000 | (li << 8) | (j << 1) | p for li in (0, 1, 2 ** 22 - 1) for j in range(64) for p in (0, 1)}
    assert all((x >> 7) & 1 == 0 for x in fog_words) and not fog_words & {int(x) for x in w[[0, 1, -1]]}
    assert ((w >> np.uint64(8)) & np.uint64(0x3FFFFF) == l).all()  # (l << 8 stays below bit 30: bit 31 is the constant's)


# ---- 3. the setter and the getter, clause by clause ----
def test_the_setter_and_getter_clause_by_clause():
    sc = skr.parse_scene(scene_path("test.scn"), spot=True, strict=True)  # 1 point light, 1 spot light, 1 directional light
    assert sc.info.n_point_lights == 1 and len(sc.spot_lights) == 1 and sc.info.n_directional_lights == 1
    r0 = sc.light_radii
    assert r0.dtype == np.float32 and r0.tolist() == [0.0, 0.0]  # default 0; the directional light has none
    sc.set_light_radii([0.25, 1.5])
    assert sc.light_radii.tolist() == [0.25, 1.5]
    L = skr.lib()
    for bad in ([0.5], [0.5, 0.5, 0.5], [], [-0.5, 1.0], [1.0, np.nan], [np.inf, 1.0], [1.0, -np.inf]):
        a = np.array(bad, np.float32)
        assert L.skr_scene_set_light_radii(sc.h, a.ctypes.data if len(a) else None, len(a)) == 2  # SKR_ERR_ARG
        with pytest.raises(skr.SkrError):
            sc.set_light_radii(a)
        assert sc.light_radii.tolist() == [0.25, 1.5]  # unchanged
    assert L.skr_scene_set_light_radii(None, r0.ctypes.data, 2) == 2 and L.skr_scene_set_light_radii(sc.h, None, 2) == 2
    sc.set_light_radii(0.75)  # a scalar: every point and spot light
    assert sc.light_radii.tolist() == [0.75, 0.75]
    n = C.c_int32(-1)
    assert L.skr_scene_get_light_radii(sc.h, None, C.byref(n)) == 0 and n.value == 2
    sc.set_light_radii([0.0, -0.0])
    assert bits(sc.light_radii).tolist() == [0, 0]
    # skr_scene_set_spot_lights changes the light count: every radius is 0 again
    sc.set_light_radii([0.25, 1.5])
    sc.set_spot_lights(np.concatenate([sc.spot_lights, sc.spot_lights]))
    assert sc.light_radii.tolist() == [0.0, 0.0, 0.0]
    sc.set_light_radii([1, 2, 3])
    sc.set_spot_lights(np.zeros((0, 11), np.float32))
    assert sc.light_radii.tolist() == [0.0]
    # a scene made from arrays takes the radii
    src = skr.parse_scene(scene_path("spheres2.scn"))
    a, cam = src.arrays(), list(src.info.camera)[:9]
    n_l = len(a[2])
    made = skr.Scene.from_arrays(a[0], a[1], a[2], cam, light_radii=0.5)
    assert n_l >= 1 and made.light_radii.tolist() == [0.5] * n_l
    assert skr.Scene.from_arrays(a[0], a[1], a[2], cam).light_radii.tolist() == [0.0] * n_l
    with pytest.raises(skr.SkrError):
        skr.Scene.from_arrays(a[0], a[1], a[2], cam, light_radii=[0.5] * (n_l + 1))


def test_the_header_announces_the_addition():
    h = open(ROOT + "/include/skr.h").read()
    assert re.search(r"#define SKR_HAS_SOFT_LIGHTS 1\b", h) and re.search(r"#define SKR_ABI_VERSION 7\b", h)
    L = skr.lib()
    for name in ("skr_scene_set_light_radii", "skr_scene_get_light_radii"):
        assert hasattr(L, name) and name in skr.binding.EXPORTED_SYMBOLS


def test_the_python_command_line_refuses_a_bad_radius(capsys):
    from skele_raytracer_amd import render_cli
    for bad in ("-1", "nan", "inf", "-inf"):
        assert render_cli.main(["--path", scene_path("spheres2.scn"), "--output", "/dev/null", "--light-radius", bad]) == 2
        assert "--light-radius takes a finite radius >= 0" in capsys.readouterr().err


# ---- 4. the picture: a penumbra ----
# One light 9 above a floor, one occluding sphere of radius 1 centred 3 above it (its lowest point 2 above the floor: beyond the t > 1 of
# the any-hit rule from every floor point), 64 x 48 direct frames with shadows.  Chosen from the checker's own output: the point light's
# shadow on the floor covers rows 20..28, columns 25..38; with R = 0.5 the band of partly lit pixels is a ring one to three pixels wide
# around it (rows 19..29, columns 24..39: about 80 pixels), the core rows 22..25, columns 28..35 stays dark, and every row from 34 down
# is floor that no sample's shadow reaches.  K = 16 seeds: a band pixel whose lit probability lies in [0.1, 0.9] shows both outcomes with
# probability 1 - 2 * 0.9^16 > 0.6, so at least 20 of the 80 is safe by a wide margin; the frames take a fraction of a second.
PEN_W, PEN_H, PEN_K, PEN_R = 64, 48, 16, 0.5
PEN_CORE = (slice(22, 26), slice(28, 36))
PEN_BAND = (slice(19, 30), slice(22, 42))
PEN_FAR = (slice(34, 48), slice(0, 64))


def _penumbra_scene(path, light=True):
    lines = [CAMERA, "background .1 .2 .3", "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1", "sphere %g %g %g %g" % FLOOR, "sphere 0 3 0 1"]
    if light:
        lines.append("point_light 60 60 60 0 9 0")
    open(path, "w").write("\n".join(lines) + "\n")
    return path


def test_a_radius_turns_the_shadow_edge_into_a_penumbra(checker, tmp_path):
    scn, dark_scn = _penumbra_scene(str(tmp_path / "lit.scn")), _penumbra_scene(str(tmp_path / "dark.scn"), light=False)
    dark = checker.render(dark_scn, PEN_W, PEN_H, shadow=True)[1]

    def lit_fraction(R):  # per pixel, over K seeds: the light adds something to the ambient term
        acc = np.zeros((PEN_H, PEN_W))
        for k in range(PEN_K):
            acc += checker.render(scn, PEN_W, PEN_H, radii=R, shadow=True, seed=100 + k)[1][..., 0] > dark[..., 0]
        return acc / PEN_K

    hard, soft = lit_fraction(0.0), lit_fraction(PEN_R)
    assert np.isin(hard, (0.0, 1.0)).all()  # a point light: every pixel lit or dark, whatever the seed
    assert (hard[PEN_CORE] == 0).all() and (hard[PEN_FAR] == 1).all()
    partly = (soft > 0) & (soft < 1)
    assert partly[PEN_BAND].sum() >= 20
    assert (soft[PEN_CORE] == 0).all()  # the umbra's core
    assert (soft[PEN_FAR] == 1).all()  # far from the shadow
    # the band replaces the edge: it holds pixels the point light lit and pixels it left dark
    assert (hard[partly] == 1).any() and (hard[partly] == 0).any()
