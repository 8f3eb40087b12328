"""The environment map on the host (no GPU; include/skr.h skr_scene_set_environment): the CPU checker pinned to the
frozen oracle and to the motion, lens and soft-light checkers under a constant map, the lookup's index rule against an exact restatement
in fractions.Fraction, the round trip of every texel centre, the orientation of the octants, the picture-level property — a sphere lit
by a bright upper hemisphere alone is brighter on top — on the checker alone, and the reader, the setter, the getter and the command
lines."""
import os
import subprocess

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import render_cli
from conftest import ROOT, scene_path
from oracle import pyoracle
from env_check import ENV_MAX_EDGE, build as build_checker, edge_directions, exact_taps, octa_decode
import lens_check
import motion_check
import soft_light_check

f32 = np.float32
W, H = 67, 35


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("envcheck")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def constant_map(sc, E):
    bg = sc.s.background
    assert not any(np.signbit(f32(x)) and x == 0 for x in (bg.x, bg.y, bg.z))  # (a -0 texel looks up as +0: include/skr.h)
    return np.broadcast_to(np.array([bg.x, bg.y, bg.z], np.float32), (E, E, 3)).copy()


# ---- 1. a constant map equal to the background is the frozen oracle's frame, counts included: only after this is the checker evidence ----
PIN_MODES = [("gillum", dict(gillum=2, depth=3, shadow=True, seed=5), False), ("jsample", dict(jsample=2, shadow=True, seed=3), False), ("strict", dict(shadow=True), True)]


@pytest.mark.parametrize("scn", ["spheres2.scn", "test.scn", "bear.scn"])
@pytest.mark.parametrize("name,kw,strict", PIN_MODES, ids=[m[0] for m in PIN_MODES])
def test_a_constant_map_is_the_oracle(checker, scn, name, kw, strict):
    sc = pyoracle.OracleScene(scene_path(scn), strict=strict)
    o_rgb, o_f, o_st = pyoracle.render(sc, W, H, want_float=True, **kw)
    for E in (1, 4):
        rgb, f, st = checker.render(sc, W, H, environment=constant_map(sc, E), **kw)
        assert np.array_equal(bits(f), bits(o_f)) and np.array_equal(rgb, o_rgb), E
        assert st[:5].tolist() == o_st.tolist(), E  # all five
        assert st[5] > 0 and (st[6] > 0 or "gillum" not in kw), E  # the map was looked up, at every level the mode has
    rgb, f, st = checker.render(sc, W, H, environment=None, **kw)  # and with no environment the restated shade tree is the oracle's too
    assert np.array_equal(bits(f), bits(o_f)) and st[:5].tolist() == o_st.tolist() and st[5] == 0 and st[6] == 0


def test_a_constant_map_is_the_motion_lens_and_soft_checkers(checker, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("envcheck_chain"))
    path = scene_path("spheres2.scn")
    sc = pyoracle.OracleScene(path)
    ns = sc.s.n_spheres
    vel = np.zeros((ns, 3), np.float32)
    vel[1], vel[8], vel[13] = (1.5, 0, 0), (0, 1, 0.5), (0, 0.5, 0)
    kw = dict(gillum=2, depth=3, shadow=True, seed=5)
    m_rgb, m_f, m_st = motion_check.build(d).render(sc, W, H, velocities=vel, shutter=0.75, radii=0.3, **kw)
    l_rgb, l_f, l_st = lens_check.build(d).render(sc, W, H, aperture=0.3, focus=11.0, radii=0.3, jsample=2, **kw)
    s_rgb, s_f, s_st = soft_light_check.build(d).render(sc, W, H, radii=0.4, **kw)
    for E in (1, 4):
        env = constant_map(sc, E)
        rgb, f, st = checker.render(sc, W, H, environment=env, velocities=vel, shutter=0.75, radii=0.3, **kw)
        assert np.array_equal(bits(f), bits(m_f)) and np.array_equal(rgb, m_rgb) and st[:5].tolist() == m_st.tolist()
        rgb, f, st = checker.render(sc, W, H, environment=env, aperture=0.3, focus=11.0, radii=0.3, jsample=2, **kw)
        assert np.array_equal(bits(f), bits(l_f)) and np.array_equal(rgb, l_rgb) and st[:5].tolist() == l_st.tolist()
        rgb, f, st = checker.render(sc, W, H, environment=env, radii=0.4, **kw)
        assert np.array_equal(bits(f), bits(s_f)) and np.array_equal(rgb, s_rgb) and st[:5].tolist() == s_st.tolist()
        assert st[5] > 0 and st[6] > 0


# ---- 2. the rule: indices and weights against the exact restatement, rounded to nearest-even ----
EDGES_E = (1, 2, 3, 8, ENV_MAX_EDGE)


def random_directions(n, seed):
    """directions of every magnitude, a third of them snapped near an axis plane, a fold or the pole"""
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, (n, 3)) * np.exp(rng.uniform(-30, 30, (n, 1)))
    k = n // 3
    d[:k, rng.integers(0, 3, k)] *= 1e-7          # near a border of an octant
    d[k:2 * k, 1] = -np.abs(d[k:2 * k, 1]) * 1e3  # near the -y pole: the corners of the square
    return d.astype(np.float32)


def check_taps(checker, d, E):
    got = checker.taps(d, E)
    for row, dir_ in zip(got, d):
        want = exact_taps(dir_, E)
        mine = (int(row[0]), int(row[1]), int(row[2]), int(row[3]), int(row[4]), int(row[5]), int(row[6]))
        assert mine == (want[0], want[1], want[2], want[3], want[4], int(bits(want[5]).reshape(-1)[0]), int(bits(want[6]).reshape(-1)[0])), (dir_.tolist(), E, mine, want)
        if not want[0]:
            assert 0 <= mine[1] <= mine[2] <= E - 1 and 0 <= mine[3] <= mine[4] <= E - 1 and mine[2] - mine[1] <= 1 and mine[4] - mine[3] <= 1
            fx, fy = row[5:7].copy().view(np.float32)
            assert 0.0 <= fx < 1.0 and 0.0 <= fy < 1.0
    return got


def test_the_taps_of_random_directions_are_the_exact_rule(checker):
    d = random_directions(2000, 17)
    for k, E in enumerate(EDGES_E):
        check_taps(checker, d[k::len(EDGES_E)], E)


def test_the_taps_at_the_edges_of_the_rule(checker):
    d = edge_directions()
    for E in EDGES_E:
        got = check_taps(checker, d, E)
        flags = got[:, 0]
        bad = ~np.isfinite(d.astype(np.float64)).all(1) | (np.abs(d.astype(np.float64)).sum(1) == 0) | (np.abs(d.astype(np.float64)).sum(1) > 3.4028234663852886e38 * (1 + 2.0 ** -25))
        assert flags[bad].all() and flags.sum() >= 12  # zero, NaN, inf and s overflowing take the background arm ...
        assert not flags[np.isfinite(d).all(1) & (np.abs(d.astype(np.float64)).sum(1) < 3e38) & (np.abs(d.astype(np.float64)).sum(1) > 0)].any()  # ... and nothing else does: subnormals too
        # d and 2 d: the last eight rows come in pairs
        pairs = got[-8:].reshape(4, 2, 7)
        assert np.array_equal(pairs[:, 0], pairs[:, 1])
    one = checker.taps(d, 1)  # E = 1: every lookup is texel (0, 0)
    assert not one[one[:, 0] == 0][:, 1:5].any()
    # the axes land where the map's orientation says: +y at the centre of the square, -y at its corners, +-x and +-z at the edge midpoints
    E = 8
    taps = {tuple(v): checker.taps(np.array([v], np.float32), E)[0] for v in ((0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1))}
    assert taps[(0, 1, 0)][1:5].tolist() == [3, 4, 3, 4] and taps[(0, -1, 0)][1:5].tolist() == [7, 7, 7, 7]
    assert taps[(1, 0, 0)][1:5].tolist() == [7, 7, 3, 4] and taps[(-1, 0, 0)][1:5].tolist() == [0, 0, 3, 4]
    assert taps[(0, 0, 1)][1:5].tolist() == [3, 4, 7, 7] and taps[(0, 0, -1)][1:5].tolist() == [3, 4, 0, 0]


def test_the_lookup_is_step_six_in_binary32(checker):
    rng = np.random.default_rng(5)
    E = 8
    tex = rng.uniform(-2, 9, (E, E, 3)).astype(np.float32)
    d = np.concatenate([random_directions(300, 9), edge_directions()])
    got = checker.lookup(tex, d, background=(0.25, 0.5, 0.75))
    taps = checker.taps(d, E)
    for g, t in zip(got, taps):
        if t[0]:
            assert g.tolist() == [0.25, 0.5, 0.75]
            continue
        i0, i1, j0, j1 = (int(x) for x in t[1:5])
        fx, fy = t[5:7].copy().view(np.float32)
        top = tex[j0, i0] + fx * (tex[j0, i1] - tex[j0, i0])
        bot = tex[j1, i0] + fx * (tex[j1, i1] - tex[j1, i0])
        assert np.array_equal(bits(g), bits(top + fy * (bot - top)))
    const = np.broadcast_to(np.array([0.1, 7.5, 1e-3], np.float32), (E, E, 3)).copy()  # a constant map returns its colour exactly
    ok = taps[:, 0] == 0
    assert np.array_equal(bits(checker.lookup(const, d)[ok]), bits(np.broadcast_to(const[0, 0], (int(ok.sum()), 3))))


# ---- 3. the round trip: the float64 octahedral decode of a texel centre looks that texel up with weight 0 ----
def test_every_texel_centre_looks_up_its_texel(checker):
    E = 8
    d = np.array([octa_decode((i + 0.5) / E, (j + 0.5) / E) for j in range(E) for i in range(E)], np.float32)
    t = checker.taps(d, E)
    assert not t[:, 0].any() and not t[:, 5:7].any()  # fx = fy = +0
    assert t[:, 1].tolist() == [i for j in range(E) for i in range(E)] and t[:, 3].tolist() == [j for j in range(E) for i in range(E)]
    tex = np.arange(E * E * 3, dtype=np.float32).reshape(E, E, 3)
    assert np.array_equal(checker.lookup(tex, d), tex.reshape(-1, 3))


# ---- 4. orientation: one colour per octant ----
def octant_map(E):
    """texel (j, i) holds the colour (1 + [x > 0], 1 + [y > 0], 1 + [z > 0]) of the octant its centre decodes into"""
    tex = np.zeros((E, E, 3), np.float32)
    for j in range(E):
        for i in range(E):
            tex[j, i] = 1.0 + (octa_decode((i + 0.5) / E, (j + 0.5) / E) > 0)
    return tex


LONE = "camera 0 0 -6 0 0 1 0 1 0 20\nbackground 0 0 0\nambient_light 0 0 0\nmaterial 0 0 0 .8 .8 .8 0 0 0 1 0 0 0 1\nsphere 0 0 0 1.5\n"


def test_primary_rays_into_each_octant_return_its_colour(checker, tmp_path):
    scn = tmp_path / "lone.scn"
    scn.write_text(LONE.replace("sphere 0 0 0 1.5", "sphere 0 0 1000 1"))
    tex = octant_map(16)
    signs = np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    for scale in (1.0, 0.37, 250.0):  # (+-1, +-1, +-1): the centroid of each octant's triangle of the square, four texels from its borders
        rays = np.zeros((8, 8), np.float32)
        rays[:, 3] = np.inf
        rays[:, 4:7] = signs * scale
        rays[:, 7] = np.array([-1], np.int32).view(np.float32)[0]
        out, st = checker.shade(str(scn), rays, environment=tex)
        assert np.array_equal(out, 1.0 + (signs > 0)) and st[5] == 8 and st[6] == 0 and st[1] == 0


# ---- 5. lighting: the environment lights a surface through its --gillum children alone ----
def test_a_bright_upper_hemisphere_lights_the_top_of_a_sphere(checker, tmp_path):
    scn = tmp_path / "lone.scn"
    scn.write_text(LONE)
    E, w, h = 16, 32, 32
    tex = np.zeros((E, E, 3), np.float32)
    for j in range(E):
        for i in range(E):
            tex[j, i] = 4.0 if octa_decode((i + 0.5) / E, (j + 0.5) / E)[1] > 0 else 0.0
    sc = pyoracle.OracleScene(str(scn))
    acc = np.zeros((h, w, 3), np.float64)
    for seed in range(1, 65):
        _, f, st = checker.render(sc, w, h, fov=40.0, environment=tex, gillum=4, depth=2, seed=seed)
        assert st[5] > 0 and st[6] > 0 and st[2] == 0  # lookups at level 0 (the backdrop) and below it; no light, no shadow ray
        acc += f
    _, flat, st0 = checker.render(sc, w, h, fov=40.0, environment=None, gillum=4, depth=2, seed=1)
    hit = np.zeros((h, w), bool)
    hit[8:24, 8:24] = True  # the sphere's disc holds the central square (radius 1.5 at distance 6 under fov 40: 11 of 16 pixels each way)
    assert not flat[hit].any() and st0[5] == 0  # without the environment the sphere is black: nothing else lights it
    lum = (acc / 64).sum(2)
    upper, lower = lum[8:16, 8:24].mean(), lum[16:24, 8:24].mean()
    assert upper > 2 * lower and lower >= 0 and upper > 0.5, (upper, lower)


# ---- 6. the host: the reader, the setter and the getter, the command lines ----
def test_read_pfm_is_the_inverse_of_write_pfm_in_both_byte_orders(tmp_path):
    rng = np.random.default_rng(2)
    a = rng.normal(0, 3, (5, 7, 3)).astype(np.float32)
    a[0, 0] = (0.0, -0.0, 1e-42)
    a[4, 6] = (3e38, -3e38, np.inf)
    p = str(tmp_path / "a.pfm")
    skr.write_pfm(p, a)
    assert np.array_equal(bits(skr.read_pfm(p)), bits(a))
    head, body = open(p, "rb").read().split(b"-1.0\n", 1)
    big = str(tmp_path / "big.pfm")
    open(big, "wb").write(head + b"1.0\n" + np.frombuffer(body, "<u4").astype(">u4").tobytes())
    assert np.array_equal(bits(skr.read_pfm(big)), bits(a))
    w, h = skr.binding.C.c_uint32(0), skr.binding.C.c_uint32(0)  # null rgbf: the sizes only
    assert skr.lib().skr_read_pfm(os.fsencode(p), skr.binding.C.byref(w), skr.binding.C.byref(h), None) == 0 and (w.value, h.value) == (7, 5)
    bad = {"grey": b"Pf\n7 5\n-1.0\n" + body, "magic": b"P6\n7 5\n255\n" + body, "short": head + b"-1.0\n" + body[:-4], "zero": b"PF\n0 5\n-1.0\n", "scale": b"PF\n7 5\n0\n" + body,
           "nan": b"PF\n7 5\nnan\n" + body, "words": b"PF\nseven 5\n-1.0\n" + body, "header": b"PF\n7", "empty": b""}
    for name, data in bad.items():
        q = str(tmp_path / (name + ".pfm"))
        open(q, "wb").write(data)
        with pytest.raises(skr.SkrError) as e:
            skr.read_pfm(q)
        assert "(status 1)" in str(e.value) and name + ".pfm" in str(e.value), (name, str(e.value))
    with pytest.raises(skr.SkrError):
        skr.read_pfm(str(tmp_path / "missing.pfm"))


def test_the_setter_and_getter_clause_by_clause():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    assert sc.environment is None
    tex = np.random.default_rng(1).uniform(0, 2, (3, 3, 3)).astype(np.float32)
    sc.set_environment(tex)
    assert np.array_equal(bits(sc.environment), bits(tex))
    L, Cm = skr.lib(), skr.binding.C
    for bad_tex, edge in ((tex, -1), (tex, ENV_MAX_EDGE + 1)):
        assert L.skr_scene_set_environment(sc.h, bad_tex.ctypes.data, edge) == 2 and np.array_equal(bits(sc.environment), bits(tex))
    for v in (np.nan, np.inf, -np.inf):
        bad = tex.copy()
        bad[2, 1, 0] = v
        with pytest.raises(skr.SkrError) as e:
            sc.set_environment(bad)
        assert "(status 2)" in str(e.value) and np.array_equal(bits(sc.environment), bits(tex))  # the scene is unchanged
    with pytest.raises(ValueError):
        sc.set_environment(np.zeros((2, 3, 3), np.float32))
    e = Cm.c_int32(-1)
    assert L.skr_scene_get_environment(sc.h, None, Cm.byref(e)) == 0 and e.value == 3  # null texels: the edge only
    assert L.skr_scene_set_environment(sc.h, None, 3) == 0 and sc.environment is None  # null texels clear it
    sc.set_environment(tex[:1, :1])
    assert sc.environment.shape == (1, 1, 3)
    assert L.skr_scene_set_environment(sc.h, tex.ctypes.data, 0) == 0 and sc.environment is None  # so does edge 0
    sc.set_environment(tex)
    sc.set_environment(None)
    assert sc.environment is None
    one = np.full((1, 1, 3), 0.5, np.float32)
    sa = skr.Scene.from_arrays(np.zeros((0, 14), np.float32), np.zeros((0, 9), np.float32), np.zeros((0, 6), np.float32), list(sc.info.camera)[:9], environment=one)
    assert np.array_equal(sa.environment, one)
    big = np.zeros((ENV_MAX_EDGE, ENV_MAX_EDGE, 3), np.float32)  # the largest edge is taken
    sc.set_environment(big)
    assert sc.environment.shape == (ENV_MAX_EDGE, ENV_MAX_EDGE, 3)


def test_the_header_announces_the_addition():
    text = open(os.path.join(ROOT, "include", "skr.h")).read()
    assert "#define SKR_HAS_ENVIRONMENT 1" in text and "#define SKR_ENV_MAX_EDGE 4096" in text
    for name in ("skr_scene_set_environment", "skr_scene_get_environment", "skr_read_pfm"):
        assert name in text and name in skr.EXPORTED_SYMBOLS
    assert "#define SKR_ABI_VERSION" in text


def test_both_command_lines_parse_envmap_and_refuse_a_file_that_is_not_square(tmp_path, capsys):
    base = ["--path", scene_path("spheres2.scn"), "--output", str(tmp_path / "out.ppm"), "--width", "32", "--height", "24"]
    assert "envmap" not in render_cli._parse(base) and render_cli._parse(base + ["--envmap", "sky.pfm"])["envmap"] == "sky.pfm"
    assert render_cli.main(base + ["--envmap"]) == 0 and "envmap takes the path" in capsys.readouterr().err  # a missing value: a usage error
    wide, missing, text = str(tmp_path / "wide.pfm"), str(tmp_path / "none.pfm"), str(tmp_path / "text.pfm")
    skr.write_pfm(wide, np.zeros((4, 6, 3), np.float32))
    open(text, "w").write("PF\nnot a map\n")
    exe = os.path.join(ROOT, "bin", "raytracer")
    for f, word in ((wide, "square"), (missing, "cannot open"), (text, "not a colour PFM")):
        assert render_cli.main(base + ["--envmap", f]) == 2
        err = capsys.readouterr().err
        assert "--envmap" in err and f in err and word in err, err
        r = subprocess.run([exe, *base, "--envmap", f, "--quiet"], cwd=str(tmp_path), capture_output=True, timeout=120)
        assert r.returncode != 0 and b"--envmap" in r.stderr and f.encode() in r.stderr and word.encode() in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "out.ppm"))
