"""What the cases of tests/shading_values.py reach, on the CPU oracle alone (no GPU): a case that reaches nothing proves nothing.  The
conditions are stated in the catalogue's docstring; the frames are the ones tests/test_shading_values_gpu.py compares the kernels with
(64x36, shadow=True, the case's own keywords)."""
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
import shading_values as sv
from test_leaf_shape_host import SWITCHES, leaf_shape

f32 = np.float32
W, H = sv.SIZE


@pytest.fixture(scope="module")
def frames(oracle, tmp_path_factory):
    """frame(case, **over) -> (bytes, floats, stats) of the oracle, each scene rendered once"""
    folder, kept = str(tmp_path_factory.mktemp("shading_values_cpu")), {}

    def frame(case, **over):
        key = (case.name, tuple(sorted(over.items())))
        if key not in kept:
            path = sv.write(case, os.path.join(folder, "s%d.scn" % len(kept)), **over)
            kw = dict(dict(shadow=True), **case.kw)
            kept[key] = oracle.render(path, W, H, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, strict=case.load.get("strict", False), **kw)
        return kept[key]
    return frame


def pixels(mask):
    return int(mask.reshape(H, W, -1).any(-1).sum())


def differ_bytes(a, b):
    return pixels(a[0] != b[0])


def differ_floats(a, b):
    return pixels(a[1].view(np.uint32) != b[1].view(np.uint32))


def test_catalogue_names_are_unique_and_every_family_is_there():
    assert len(sv.BY_NAME) == len(sv.CASES)
    assert {c.family for c in sv.CASES} == {"exponent", "cold", "triangle", "colour", "light"}
    assert [c.scene["power"] for c in sv.CASES if c.family == "exponent"] == [float(n) for n in sv.EXPONENTS]


@pytest.mark.parametrize("n", [n for n in sv.EXPONENTS if n >= 128])
def test_an_exponent_of_eight_bits_or_more_shows_in_the_bytes(frames, n):
    case = sv.BY_NAME["exp_%d" % n]
    full, seven = frames(case), frames(case, power=sv.seven_step_exponent(n))
    below, above = frames(case, power=float(n - 1)), frames(case, power=float(n + 1))
    print("exponent %d: %d pixels differ from %g's, %d from n - 1, %d from n + 1" % (n, differ_bytes(full, seven), sv.seven_step_exponent(n), differ_bytes(full, below),
                                                                                   differ_bytes(full, above)))
    assert differ_bytes(full, seven) >= 16
    assert differ_bytes(full, below) >= 1 and differ_bytes(full, above) >= 1


@pytest.mark.parametrize("name,member", [("tri_256_spheres_8", "triangle"), ("spheres_256_tri_8", "power")])
def test_the_largest_exponent_on_one_kind_of_surface_shows_in_the_bytes(frames, name, member):
    case = sv.BY_NAME[name]
    n = int(case.scene[member])
    assert max(sv.integer_exponents(case)) == n == 256 and sorted(set(sv.integer_exponents(case))) == [8, 256]
    full = frames(case)
    assert full[2][1] > 0 and (full[1] != 0).any()
    assert differ_bytes(full, frames(case, **{member: sv.seven_step_exponent(n)})) >= 16
    assert differ_bytes(full, frames(case, **{member: float(n - 1)})) >= 1 and differ_bytes(full, frames(case, **{member: float(n + 1)})) >= 1
    # ... and it is the shaded triangle that carries the exponent's highlight: without --shade-triangles the frame differs
    plain = sv.Case(*case[:3], dict(case.kw, shade_triangles=False), *case[4:])._replace(name=name + "_plain")
    assert differ_bytes(full, frames(plain)) >= 16


@pytest.mark.parametrize("case", [c for c in sv.CASES if c.family == "cold"], ids=lambda c: c.name)
def test_exponents_of_the_cold_path_change_the_frame(frames, case):
    n = differ_floats(frames(case), frames(case, power=8.0))
    print("%s: %d pixels differ from the exponent-8 frame" % (case.name, n))
    assert n >= 16
    assert sv.pow_steps(case) == (7 if case.name == "exp_1025_beside_64" else 4)


@pytest.mark.parametrize("case", [c for c in sv.CASES if c.reach], ids=lambda c: c.name)
def test_negative_overflowing_and_bright_values_are_in_the_frame(frames, case):
    rgb, f, _ = frames(case)
    with np.errstate(invalid="ignore"):
        if case.reach == "negative":
            neg = f < 0
            assert pixels(neg) >= 16
            assert pixels(neg & (rgb != 0) & (rgb != 255)) >= 16  # the wrap: (uint8_t) (int32_t) of a negative product
        elif case.reach == "overflow":
            assert pixels(np.isnan(f) | (f == np.inf)) >= 16
        else:
            assert case.reach == "bright" and pixels(f > 1) >= 16


def test_nan_is_in_the_frames_that_say_so_and_in_no_other(frames):
    for case in sv.CASES:
        assert bool(np.isnan(frames(case)[1]).any()) == case.nan, case.name


def test_the_specular_gate_of_the_legacy_code_is_taken(frames):
    zero, negzero = frames(sv.BY_NAME["specular_zero_legacy"]), frames(sv.BY_NAME["specular_negzero_legacy"])
    some = frames(sv.BY_NAME["specular_zero_legacy"], big_specular=(1e-3, 1e-3, 1e-3), small_specular=(1e-3, 1e-3, 1e-3))
    assert int(zero[2][0]) == int(negzero[2][0]) < int(some[2][0]), (zero[2], negzero[2], some[2])
    assert "-0 -0 -0" in sv.text(sv.BY_NAME["specular_negzero_legacy"])


def test_light_cases_change_the_frame(frames):
    """Each light case's frame differs from the base scene's, and from its neighbours' where the case is one of a pair."""
    base = frames(sv.BY_NAME["exp_127"], power=8.0)
    for case in sv.CASES:
        if case.family in ("light", "colour") and not case.kw.get("legacy_reflect") and case.kw.get("shadow", True) and not case.load.get("strict"):
            assert differ_floats(frames(case), base) >= 16, case.name
    assert differ_floats(frames(sv.BY_NAME["light_behind_sphere_no_shadows"]), frames(sv.BY_NAME["light_behind_sphere"])) >= 16
    assert differ_floats(frames(sv.BY_NAME["light_far_2p49_4"]), frames(sv.BY_NAME["light_far_2p49_6"])) >= 16
    assert differ_floats(frames(sv.BY_NAME["light_far_2p49_6"]), frames(sv.BY_NAME["light_far_1e20"])) >= 16


@pytest.mark.parametrize("name", ["directional_zero", "directional_1e_30"])
def test_degenerate_directional_lights_are_shaded(frames, name):
    """normalize of a zero (or underflowing) direction is NaN; max0 takes every term of the light to 0, so the frame is the base scene's
    but for the shadow ray each hit casts at the light."""
    base, got = frames(sv.BY_NAME["exp_127"], power=8.0), frames(sv.BY_NAME[name])
    assert np.array_equal(base[1].view(np.uint32), got[1].view(np.uint32))
    assert int(got[2][1]) == int(base[2][1]) > 0 and int(got[2][2]) == int(base[2][2]) + int(base[2][1])


def surface_points():
    """Points on every sphere of the scene (hit points lie there), binary32."""
    rng = np.random.default_rng(49)
    out = []
    for x, y, z, r in [(0.0, -40.0, 0.0, 40.0), sv.BIG] + sv.SMALL:
        d = rng.normal(size=(256, 3))
        out.append(np.array([x, y, z]) + r * d / np.linalg.norm(d, axis=1, keepdims=True))
    return np.concatenate(out).astype(f32)


@pytest.mark.parametrize("name", sorted(sv.FAR))
def test_far_lights_sit_where_they_claim_about_the_fast_range(name):
    """shade_common.h light_term restated: to_l = Lp - P, ss = (x x + y y) + z z in binary32; device_math.h len_terms takes the short
    forms for ss in [2^-98, 2^99)."""
    lp = np.array([float(t) for t in sv.scene(**sv.BY_NAME[name].scene)[-2].split()[4:7]], f32)
    to_l = lp[None, :] - surface_points()
    with np.errstate(over="ignore"):
        sq = to_l * to_l
        ss = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    fast = (ss.view(np.uint32) - np.uint32(29 << 23)) < np.uint32(197 << 23)  # the kernel's own range test
    assert np.array_equal(fast, (ss >= f32(2.0 ** -98)) & (ss < f32(2.0 ** 99)))
    if sv.FAR[name] == "inside":
        assert fast.all() and (ss > f32(2.0 ** 98.5)).all()
    elif sv.FAR[name] == "outside":
        assert not fast.any() and np.isfinite(ss).all()
    else:
        assert np.isinf(ss).all()


def test_light_positions_are_where_the_cases_say():
    cam, big = np.array(sv.CAMERA[:3]), np.array(sv.BIG[:3])
    at = lambda name: np.array(sv.BY_NAME[name].scene["key_position"], np.float64)
    assert np.array_equal(at("light_at_camera"), cam)
    behind = at("light_behind_sphere")
    assert np.linalg.norm(behind - big) > sv.BIG[3] and np.linalg.norm(np.cross(behind - cam, big - cam)) < 1e-9 and np.dot(behind - big, big - cam) > 0
    assert abs(np.linalg.norm(at("light_near_surface") - big) - sv.BIG[3] - 0.01) < 1e-9
    assert np.linalg.norm(at("light_inside_sphere") - big) < sv.BIG[3]
    c = sv.BY_NAME["lights_coincident"].scene["more_lights"]
    assert c[1] == (sv.KEY_COLOUR, sv.KEY_POSITION)


def test_the_light_behind_the_sphere_nearly_cancels_the_view_vector(oracle, tmp_path):
    """blinn_phong.h:93-95 restated at the frame's own hit points: view = normalize(camera - P), L = normalize(Lp - P) in binary32.  No
    pixel centre of a 64x36 frame lies on the axis, so view + L is not 0 anywhere (H is not NaN); half a pixel off the axis it is about
    0.02 long — the bound of 0.05 is two to three pixels' worth —, a cancellation of two unit vectors, and H is its quotient by that length."""
    case = sv.BY_NAME["light_behind_sphere_no_shadows"]
    osc = oracle.OracleScene(sv.write(case, str(tmp_path / "s.scn")))
    cam, lp = np.array(sv.CAMERA[:3], f32), np.array(case.scene["key_position"], np.float64).astype(f32)
    spheres = np.array([(0.0, -40.0, 0.0, 40.0), sv.BIG] + sv.SMALL, np.float64)
    shortest, on_big = np.inf, 0
    for y in range(H):
        for x in range(W):
            d = oracle.primary_direction(osc, W, H, sv.FOV, x, y, False).astype(np.float64)
            e = cam.astype(np.float64) - spheres[:, :3]
            a, b, c = d @ d, 2 * (e @ d), (e * e).sum(1) - spheres[:, 3] ** 2
            disc = b * b - 4 * a * c
            with np.errstate(invalid="ignore"):
                t = np.where(disc >= 0, (-b - np.sqrt(disc)) / (2 * a), np.inf)
            t[t < 0] = np.inf
            if int(np.argmin(t)) != 1 or not np.isfinite(t[1]):
                continue  # the large sphere is not what this pixel shows
            on_big += 1
            p = (cam.astype(np.float64) + t[1] * d).astype(f32)
            unit = lambda v: v * (f32(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
            vl = unit(cam - p) + unit(lp - p)
            shortest = min(shortest, float(np.sqrt((vl.astype(np.float64) ** 2).sum())))
    print("|view + L| at its shortest over %d hit points of the large sphere: %.4f" % (on_big, shortest))
    assert on_big >= 200 and 0.0 < shortest < 0.05


@pytest.fixture
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("case", sv.CASES, ids=lambda c: c.name)
def test_the_dispatch_names_the_leaf_instance_the_catalogue_expects(clean_env, tmp_path, case):
    """launch.h skr_leaf_shape on the host side of the case's launch: an exponent of 8 bits or more must get the run-time instance (the
    shaped ones compile seven squarings in), 127 and the exponents of the cold path a shaped one — and each other fact the catalogue's
    restatement knows breaks the shape."""
    scene = skr.parse_scene(sv.write(case, str(tmp_path / "s.scn")), **case.load)
    opt = skr.Options(*sv.SIZE, **dict(dict(gillum=4, depth=3, shadow=True, seed=5), **{k: v for k, v in case.kw.items() if k in ("fov", "shadow")}))
    assert leaf_shape(scene, opt) == sv.leaf_shape(case)


def test_the_catalogue_expects_both_kinds_of_leaf_instance():
    assert [sv.pow_steps(sv.BY_NAME["exp_%d" % n]) for n in sv.EXPONENTS] == [7, 8, 8, 9, 10, 10, 11]
    assert [sv.leaf_shape(sv.BY_NAME["exp_%d" % n]) for n in sv.EXPONENTS] == [2, 0, 0, 0, 0, 0, 0]
    want = {"exp_0": 2, "exp_1025_beside_64": 2, "light_far_2p49_6": 2, "light_far_1e20": 0, "lights_coincident": 0, "light_behind_sphere_no_shadows": 0,
            "directional_zero": 0, "tri_256_spheres_8": 0, "spheres_256_tri_8": 0}
    assert {n: sv.leaf_shape(sv.BY_NAME[n]) for n in want} == want


# ------------------------------------------------------------------------------------------------------------ the unit records ----
def pow_reference(oracle, rec):
    """sko_powf_shared of every record (steps is no operand of the reference), computed once per distinct (x, p)."""
    L = oracle.lib()
    xp = rec[:, :2].copy()
    uniq, inverse = np.unique(xp.view(np.uint64).ravel(), return_inverse=True)
    pairs = uniq.view(np.uint32).reshape(-1, 2).view(f32)
    want = f32([L.sko_powf_shared(float(a), float(b)) for a, b in pairs])
    return want[inverse.ravel()]


def test_pow_records_are_mostly_not_trivial(oracle):
    rec, le7, block = sv.pow_records()
    assert len(rec) == 2 * 1024 * (len(sv.POW_X) + sv.POW_RANDOM_PER_P) + 11 * len(sv.POW_COLD) * len(sv.POW_X) and len(sv.POW_X) == 64
    want = pow_reference(oracle, rec)
    with np.errstate(invalid="ignore"):
        trivial = (want == 0) | (want == 1) | np.isinf(want) | np.isnan(want)
    share = [float(1 - trivial[block == b].mean()) for b in (0, 1, 2)]
    print("share of op-20 records whose reference result is neither 0, 1, inf nor NaN: integers x family %.3f, integers x [0.97, 1] %.3f, cold %.3f" % tuple(share))
    assert share[1] >= 0.99 and share[0] >= 0.4 and share[2] >= 0.2
    p, steps = rec[:, 1].copy().view(f32), rec[:, 2]
    plain = block < 2
    assert set(np.unique(p[plain]).tolist()) == set(range(1, 1025))
    assert ((steps[plain] == 11) | (2.0 ** steps[plain] > p[plain])).all() and (steps >= 1).all() and (steps <= 11).all()
    assert le7[block == 2].all() and np.array_equal(le7[plain], p[plain] <= 127)
    # a step count one too small drops the exponent's top bit: such a record would have another reference result almost everywhere
    b1 = block == 1
    dropped = f32([oracle.lib().sko_powf_shared(float(a), float(int(b) & ~(1 << (int(b).bit_length() - 1)))) for a, b in zip(rec[b1, 0].copy().view(f32)[::37], p[b1][::37])])
    assert (dropped != want[b1][::37]).mean() > 0.99


def test_quantise_records_wrap(oracle):
    v = sv.quantise_values()
    assert (v[len(sv.QUANTISE_EDGES):] < 0).all() and (v[len(sv.QUANTISE_EDGES):] > -300).all()
    want = np.array([oracle.lib().sko_quantise(float(x)) for x in v], np.uint8)
    assert np.array_equal(want, oracle.quantise(v))
    share = float(((want != 0) & (want != 1) & (want != 255)).mean())
    print("share of quantise records whose byte is neither 0, 1 nor 255: %.3f" % share)
    assert share >= 0.95
    edges = dict(zip(sv.QUANTISE_EDGES.tolist(), want.tolist()))
    assert edges[-0.5] == 256 - 127 and edges[-1.0] == 1 and edges[-1e3] == (-255000) & 0xff and edges[float(f32(-8421504.5))] == (-8421504 * 255) & 0xff
    assert edges[float(f32(-8.5e6))] == edges[float(f32(-1e30))] == edges[-np.inf] == 0  # below -2^31: the oracle's guard, no cast
