"""The thin-lens camera on the host (no GPU; include/skr.h skr_scene_set_lens): the CPU checker pinned to the frozen oracle
while the aperture is 0, the sample and the ray against a numpy restatement, the disk and the focus identity within derived bounds, the
setter and getter, and the picture-level property of the rule — depth of field — on the checker alone."""
import ctypes as C
import re

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import ROOT, scene_path
from oracle import pyoracle
import camera_poses
from lens_check import LENS_CTR3, TWO_PI_F, build as build_checker, records
from test_soft_lights_cpu import philox7, sincos_spec, soft_ctr3

f32 = np.float32
E = 2.0 ** -24  # the unit roundoff of binary32


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("lenscheck")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. with A = 0 the composed frame is the frozen oracle's, counts included: only after this is the checker evidence ----
W, H = 67, 35
PIN_MODES = [
    ("direct", dict()),
    ("shadow", dict(shadow=True)),
    ("gi3_d3", dict(gillum=3, depth=3, shadow=True, seed=5)),
    ("js2", dict(jsample=2, shadow=True, seed=3)),
    ("strict", dict(strict=True, shadow=True)),
    ("shade_triangles", dict(shade_triangles=True, shadow=True)),
]


@pytest.mark.parametrize("scn", ["test.scn", "spheres2.scn"])
@pytest.mark.parametrize("name,kw", PIN_MODES, ids=[m[0] for m in PIN_MODES])
def test_the_composed_frame_is_the_oracle_with_aperture_zero(checker, scn, name, kw):
    sc = pyoracle.OracleScene(scene_path(scn), strict=kw.get("strict", False))
    opt = {k: v for k, v in kw.items() if k != "strict"}
    o_rgb, o_f, o_st = pyoracle.render(sc, W, H, want_float=True, **opt)
    for focus in (1.0, 7.5):  # (A = 0: the focus has no effect)
        rgb, f, st = checker.render(sc, W, H, aperture=0.0, focus=focus, **opt)
        assert np.array_equal(bits(f), bits(o_f)) and np.array_equal(rgb, o_rgb)
        assert st.tolist() == o_st.tolist()  # all five


def test_aperture_zero_rays_are_the_pinhole_rays(checker):
    from shade_query_check import camera_rays
    sc = pyoracle.OracleScene(scene_path("spheres2.scn"))
    for js, sample in ((0, 0), (3, 5)):
        a = checker.rays(sc, 19, 11, aperture=0.0, focus=3.0, jsample=js, seed=9, sample=sample)
        b = camera_rays(sc, 19, 11, jsample=js, seed=9, sample=sample)
        assert np.array_equal(bits(a), bits(b))


# ---- 2. the sample and the ray: the rule restated in numpy binary32 ----
def lens_rule(rec):
    """include/skr.h on records uint32 [n, 18]: every step one numpy float32 operation.  Returns float32 [n, 8] and u1, u2."""
    rec = np.ascontiguousarray(rec, np.uint32).reshape(-1, 18)
    fl = rec[:, 4:].copy().view(np.float32)
    A, k, cam, right, up, d = fl[:, 0:1], fl[:, 1:2], fl[:, 2:5], fl[:, 5:8], fl[:, 8:11], fl[:, 11:14]
    n = len(rec)
    ctr = np.stack([rec[:, 0], rec[:, 1], np.zeros(n, np.uint32), np.full(n, LENS_CTR3, np.uint32)], 1)
    out = philox7(ctr, rec[:, 2:4])
    u1 = (out[:, 0] >> 1).astype(np.float32) * f32(2.0 ** -31)
    u2 = (out[:, 1] >> 1).astype(np.float32) * f32(2.0 ** -31)
    r = np.sqrt(u1)
    phi = TWO_PI_F * u2
    sn, cs = sincos_spec(phi)
    lx, ly = (r * cs)[:, None], (r * sn)[:, None]
    o2 = (cam + right * (A * lx)) + up * (A * ly)
    d2 = (d - right * (k * lx)) - up * (k * ly)
    assert all(a.dtype == np.float32 for a in (u1, u2, r, phi, lx, ly, o2, d2))
    return np.concatenate([lx, ly, o2, d2], 1), u1, u2


def random_records(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.01, 3.0, n).astype(np.float32)
    F = rng.uniform(0.5, 40.0, n).astype(np.float32)
    vec = lambda s: (rng.normal(0, s, (n, 3))).astype(np.float32)
    seeds = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    return records(rng.integers(0, 2 ** 32, n, dtype=np.uint64), rng.integers(0, 1024, n, dtype=np.uint64), seeds, A, A / F, vec(20.0), vec(2.0), vec(2.0), vec(1.5))


def test_sample_and_ray_are_the_rule_in_numpy_binary32(checker):
    rec = random_records(100000, 1)
    want, u1, u2 = lens_rule(rec)
    got = checker.samples(rec)
    assert np.array_equal(bits(got), bits(want))
    assert 0 <= u1.min() and u1.max() <= 1 and 0 <= u2.min() and u2.max() <= 1
    # the corners of the words: pixel, aa and seed at the ends of their ranges
    edge = records([0, 2 ** 32 - 1, 7, 7], [0, 0, 2 ** 20 - 1, 3], [0, 2 ** 64 - 1, 2 ** 32, 1], 0.5, 0.125, (1, 2, 3), (1, 0, 0), (0, 3, 0), (0.1, -0.2, 1))
    assert np.array_equal(bits(checker.samples(edge)), bits(lens_rule(edge)[0]))


def test_every_word_reaches_the_draw_and_the_word_is_disjoint(checker):
    base = dict(pixel=77, aa=1, seed=5)
    rest = (0.5, 0.25, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
    seen = {tuple(bits(checker.samples(records(base["pixel"], base["aa"], base["seed"], *rest))[0, :2]))}
    for name, other in (("pixel", [78, 77 + 2 ** 31]), ("aa", [0, 2]), ("seed", [4, 6, 5 + 2 ** 32])):
        for v in other:
            kw = {**base, name: v}
            got = tuple(bits(checker.samples(records(kw["pixel"], kw["aa"], kw["seed"], *rest))[0, :2]))
            assert got not in seen, (name, v)
            seen.add(got)
    # bit 31 set (the hemisphere draws' word is below 2^30), bit 7 set (the fog word's is clear), bit 6 set (the light samples' is clear), not the jitter word
    assert LENS_CTR3 >> 31 == 1 and (LENS_CTR3 >> 7) & 1 == 1 and (LENS_CTR3 >> 6) & 1 == 1 and LENS_CTR3 != 0xFFFFFFFF
    assert all((soft_ctr3(l) >> 6) & 1 == 0 and soft_ctr3(l) != LENS_CTR3 for l in (0, 1, 2 ** 22 - 1))
    assert all(((0x80000000 | (l << 8) | (j << 1) | p) >> 7) & 1 == 0 for l in (0, 2 ** 22 - 1) for j in (0, 63) for p in (0, 1))
    h = open(ROOT + "/include/skr.h").read()
    assert re.search(r"#define SKR_LENS_CTR3 0x800000C0u\b", h)


def test_every_sample_lies_in_the_disk(checker):
    """lx = fl(r cs), ly = fl(r sn) with r = fl(sqrt(u1)) <= 1 (the root is correctly rounded and u1 <= 1).  sn and cs are within 1.43 ulp
    of sin and cos (exhaustive over [0, 2 pi]: device_math.h, oracle/skr_oracle.c), an ulp of a binary32 below 2 being at most 2^-23:
    delta = 1.43 * 2^-23, so cs^2 + sn^2 <= 1 + 2 delta (|cos| + |sin|) + 2 delta^2 <= 1 + 2 sqrt(2) delta + 2 delta^2.  Each of the two
    products rounds once, a factor (1 + e) at most, e = 2^-24 (a product that underflows loses less than 2^-149 instead).  So
    lx^2 + ly^2 <= (1 + 2 sqrt(2) delta + 2 delta^2) (1 + e)^2 + 2^-140 = 1 + eps."""
    delta = 1.43 * 2.0 ** -23
    eps = (1 + 2 * np.sqrt(2.0) * delta + 2 * delta * delta) * (1 + E) ** 2 + 2.0 ** -140 - 1
    assert 5e-7 < eps < 7e-7
    got = checker.samples(random_records(100000, 2)).astype(np.float64)
    rr = got[:, 0] ** 2 + got[:, 1] ** 2
    assert rr.max() <= 1 + eps
    assert rr.max() > 0.99 and rr.min() < 0.01 and abs(rr.mean() - 0.5) < 0.01  # uniform over the disk: E r^2 = 1/2
    assert abs(got[:, 0].mean()) < 0.01 and abs(got[:, 1].mean()) < 0.01


# ---- 3. focus: the lens ray passes through the pinhole ray's point at t = F ----
FOCUS_POSES = [p for p in camera_poses.REGULAR if p.family in ("rolled", "long")]


@pytest.mark.parametrize("pose", FOCUS_POSES, ids=[p.name for p in FOCUS_POSES])
def test_the_lens_ray_meets_the_pinhole_ray_at_the_focus(checker, pose):
    """In exact arithmetic o' + F d' = cam_pos + F d.  Per component c, with e = 2^-24, a_r = A |right_c|, a_u = A |up_c| and |lx|, |ly| <= l:
      o'_c: A lx and its product with right_c round once each (2 e a_r l), so do A ly and its product (2 e a_u l); the two sums round once
            each: e (|cam_c| + a_r l) and e (|cam_c| + a_r l + a_u l).  Together e (2 |cam_c| + 4 a_r l + 3 a_u l).
      d'_c: k = fl(A / F), k lx and the product with right_c: 3 e a_r l / F, likewise 3 e a_u l / F; the two differences: e (|d_c| +
            a_r l / F) and e (|d_c| + a_r l / F + a_u l / F).  Together e (2 |d_c| + 5 a_r l / F + 4 a_u l / F).
    So |o'_c + F d'_c - (cam_c + F d_c)| <= e (2 |cam_c| + 2 F |d_c| + 9 a_r l + 7 a_u l), to first order in e; a factor 1 + 2^-18 covers
    the higher orders, l = 1 + 2^-20 the disk's eps, and the comparison itself runs in binary64."""
    sc = pyoracle.OracleScene(scene_path(camera_poses.scene_file(pose)))
    fov = pose.kw.get("fov", 60.0)
    cam, right, up = (np.array([v.x, v.y, v.z], np.float64) for v in (sc.s.cam_pos, sc.s.cam_right, sc.s.cam_up))
    for A, F, js, sample in ((0.3, 7.5, 0, 0), (2.0, 0.75, 3, 4), (0.05, 300.0, 0, 0)):
        pin = checker.rays(sc, W, H, aperture=0.0, fov=fov, jsample=js, seed=11, sample=sample).astype(np.float64)
        got = checker.rays(sc, W, H, aperture=A, focus=F, fov=fov, jsample=js, seed=11, sample=sample).astype(np.float64)
        A64, F64 = float(f32(A)), float(f32(F))
        d = pin[:, 4:7]
        assert np.array_equal(pin[:, 0:3], np.broadcast_to(cam, d.shape))
        lhs = got[:, 0:3] + F64 * got[:, 4:7]
        rhs = cam + F64 * d
        l = 1 + 2.0 ** -20
        bound = E * (2 * np.abs(cam) + 2 * F64 * np.abs(d) + 9 * A64 * np.abs(right) * l + 7 * A64 * np.abs(up) * l) * (1 + 2.0 ** -18)
        assert (np.abs(lhs - rhs) <= bound).all(), (A, F, float((np.abs(lhs - rhs) / bound).max()))
        if np.abs(right).max() > 0:
            assert (got[:, 0:3] != pin[:, 0:3]).any() and (got[:, 4:7] != d).any()  # the lens does something
        assert np.array_equal(got[:, 3], pin[:, 3]) and np.array_equal(bits(got[:, 7].astype(np.float32)), bits(pin[:, 7].astype(np.float32)))


# ---- 4. the setter and the getter ----
def test_the_setter_and_getter_clause_by_clause():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    assert sc.lens == (0.0, 1.0)  # the default: the pinhole
    sc.set_lens(0.25, 7.5)
    assert sc.lens == (0.25, 7.5)
    sc.set_lens(0.5)
    assert sc.lens == (0.5, 1.0)
    L = skr.lib()
    for a, f in ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, np.inf), (-np.inf, 1.0), (-0.5, 1.0), (0.5, 0.0), (0.5, -1.0), (0.5, -0.0)):
        assert L.skr_scene_set_lens(sc.h, C.c_float(a), C.c_float(f)) == 2  # SKR_ERR_ARG
        with pytest.raises(skr.SkrError):
            sc.set_lens(a, f)
        assert sc.lens == (0.5, 1.0)  # unchanged
    assert L.skr_scene_set_lens(None, C.c_float(0.5), C.c_float(1.0)) == 2 and L.skr_scene_get_lens(None, None, None) == 2
    a = C.c_float(-1)
    assert L.skr_scene_get_lens(sc.h, C.byref(a), None) == 0 and a.value == 0.5
    sc.set_lens(-0.0, 3.0)
    assert bits(np.array(sc.lens, np.float32)).tolist() == bits(np.array([0.0, 3.0], np.float32)).tolist()
    # a scene made from arrays takes the lens
    arr, cam = sc.arrays(), list(sc.info.camera)[:9]
    assert skr.Scene.from_arrays(arr[0], arr[1], arr[2], cam, lens=(0.3, 6.0)).lens == (f32(0.3), 6.0)
    assert skr.Scene.from_arrays(arr[0], arr[1], arr[2], cam).lens == (0.0, 1.0)
    with pytest.raises(skr.SkrError):
        skr.Scene.from_arrays(arr[0], arr[1], arr[2], cam, lens=(-1.0, 6.0))


def test_the_header_announces_the_addition():
    h = open(ROOT + "/include/skr.h").read()
    assert re.search(r"#define SKR_HAS_LENS 1\b", h) and re.search(r"#define SKR_ABI_VERSION 7\b", h)
    L = skr.lib()
    for name in ("skr_scene_set_lens", "skr_scene_get_lens"):
        assert hasattr(L, name) and name in skr.binding.EXPORTED_SYMBOLS


def test_the_python_command_line_refuses_a_bad_lens(capsys):
    from skele_raytracer_amd import render_cli
    for flags in (["--aperture", "-1"], ["--aperture", "nan"], ["--aperture", "inf"], ["--aperture", "0.3", "--focus", "0"], ["--aperture", "0.3", "--focus", "-2"]):
        assert render_cli.main(["--path", scene_path("spheres2.scn"), "--output", "/dev/null", *flags]) == 2
        assert "--aperture takes a finite radius >= 0 and --focus a finite distance > 0" in capsys.readouterr().err


# ---- 5. the picture: depth of field ----
# The camera at the origin looks along +z (d.z = 1: t is the depth), ambient light only, so a sphere is one flat value.  Sphere 1 sits on
# the focal plane z = F = 5 at x = -1.5 with radius 0.6; sphere 2 is sphere 1 scaled by 3 from the camera and mirrored in x (z = 15 = 3 F,
# x = +4.5, radius 1.8): equal image sizes.  160 x 25 at fov 20: the centre row has v = 0 exactly, a pixel is 2 tan(10 deg) / 25 = 0.0141
# of d, the discs are 8.5 pixels in radius around columns 58.7 and 101.3.  A point at depth z is spread over a disc of radius A |1/z - 1/F|
# in d: with A = 0.6 that is 0.08 = 5.7 pixels at z = 3 F (an edge band of about 11 pixels, the disc's centre still pure) and, at sphere
# 1's silhouette (depth about F - R^2 / F), 0.6 * 0.0029 = 0.12 pixels: at most one pixel an edge.  A pixel of the 64-pass mean is mixed
# when it is farther than 2/255 from both the background and the flat value.  Confirmed on the checker: see the asserts' margins below.
DOF_W, DOF_H, DOF_FOV, DOF_K, DOF_A, DOF_F = 160, 25, 20.0, 64, 0.6, 5.0
DOF_SCENE = ["camera 0 0 0 0 0 1 0 1 0 10", "background .1 .2 .3", "ambient_light .8 .8 .8", "material .9 .9 .9 .5 .5 .5 0 0 0 8 0 0 0 1",
             "sphere -1.5 0 5 0.6", "sphere 4.5 0 15 1.8"]


def mixed_pixels_per_edge(line, background, flat):
    """the mixed pixels of the scanline in the four half-windows left and right of the two discs' centres: [sphere][edge]"""
    far = lambda v: np.abs(line - np.asarray(v, np.float32)).max(1) > 2 / 255
    mixed = far(background) & far(flat)
    c1, c2 = 58.7, 101.3
    half = int((c2 - c1) / 2)
    out = []
    for c in (c1, c2):
        m = int(round(c))
        out.append((int(mixed[m - half:m].sum()), int(mixed[m:m + half].sum())))
    assert mixed.sum() == sum(map(sum, out))  # nothing mixed anywhere else on the line
    return out


def test_the_focal_plane_stays_sharp_and_the_far_sphere_blurs(checker, tmp_path):
    scn = str(tmp_path / "dof.scn")
    open(scn, "w").write("\n".join(DOF_SCENE) + "\n")
    row = DOF_H // 2
    pin = checker.render(scn, DOF_W, DOF_H, fov=DOF_FOV)[1][row]
    background, flat = pin[0], pin[59]
    assert np.allclose(background, (.1, .2, .3)) and np.allclose(flat, 0.72) and np.array_equal(pin[59], pin[101])
    assert mixed_pixels_per_edge(pin, background, flat) == [(0, 0), (0, 0)]  # the pinhole: every pixel one or the other
    assert abs(int((np.abs(pin - flat).max(1) == 0)[:80].sum()) - int((np.abs(pin - flat).max(1) == 0)[80:].sum())) <= 1  # equal image sizes
    mean = checker.render_progressive(scn, DOF_W, DOF_H, DOF_K, seed=40, aperture=DOF_A, focus=DOF_F, fov=DOF_FOV)[1][row]
    (s1l, s1r), (s2l, s2r) = mixed_pixels_per_edge(mean, background, flat)
    print("mixed pixels per edge: focused", (s1l, s1r), "far", (s2l, s2r))
    assert s1l <= 2 and s1r <= 2
    assert s2l >= 4 and s2r >= 4
    assert np.abs(mean[[59, 101]] - flat).max() < 64 * E  # both centres stay pure (the sum of 64 equal values rounds)
