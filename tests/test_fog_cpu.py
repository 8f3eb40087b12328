"""--scn-fog and --scn-fov on the host (no GPU): the loader, the ABI, the option plumbing, and the fog checker pinned to the frozen
oracle (DESIGN.md "Spherical fog")."""
import math

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import render_cli
from conftest import scene_path
from fog_check import build as build_checker

SPHERES2_FOG = [0, -50, 0, 100, 1, 1, 1, 0.5, 0]  # spheres2.scn:64, 8 fields: absorption 0


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("fogcheck")))


def test_spheres2_fog_parsed_under_the_flag():
    plain = skr.parse_scene(scene_path("spheres2.scn"))
    fog = skr.parse_scene(scene_path("spheres2.scn"), fog=True)
    assert fog.fog.tolist() == [SPHERES2_FOG]
    assert fog.info.n_fog_skipped == 0
    # without the flag: exactly what the loader did before
    assert plain.fog.shape == (0, 9) and plain.info.n_fog_skipped == 1
    for a, b in zip(plain.arrays(), fog.arrays()):
        assert np.array_equal(a, b)
    both = skr.parse_scene(scene_path("spheres2.scn"), strict=True, fog=True)  # combines with --strict-scn
    assert both.fog.tolist() == [SPHERES2_FOG] and both.info.n_directional_lights == 2


def test_fog_lines_of_8_9_and_fewer_fields(tmp_path):
    p = tmp_path / "f.scn"
    p.write_text("camera 0 0 0 0 0 -1 0 1 0 30\n"
                 "spherical_fog 1 2 3 4 0.1 0.2 0.3 0.4\n"
                 "spherical_fog 5 6 7 8 0.5 0.6 0.7 0.8 0.9\n"
                 "spherical_fog 1 2 3 4 5 6 7\n"
                 "spherical_fog\n"
                 "spherical_fog 9 9 9 9 9 9 9 9 9 9\n")
    s = skr.parse_scene(str(p), fog=True)
    want = np.array([[1, 2, 3, 4, 0.1, 0.2, 0.3, 0.4, 0], [5, 6, 7, 8, 0.5, 0.6, 0.7, 0.8, 0.9], [9] * 9], np.float32)
    assert np.array_equal(s.fog, want)
    assert s.info.n_fog_skipped == 2
    assert skr.parse_scene(str(p)).info.n_fog_skipped == 5


def test_fog_abi_round_trip():
    s = skr.Scene.from_arrays(np.zeros((1, 14)), np.zeros((0, 9)), np.zeros((1, 6)), [0, 0, 0, 0, 0, -1, 0, 1, 0])
    assert s.fog.shape == (0, 9)
    rows = np.arange(27, dtype=np.float32).reshape(3, 9) / 7
    s.set_fog(rows)
    assert np.array_equal(s.fog, rows)
    s.set_fog(np.zeros((0, 9)))
    assert s.fog.shape == (0, 9)
    with pytest.raises(skr.SkrError):
        s.set_fog(np.zeros((skr.binding.FOG_MAX_VOLUMES + 1, 9)))


def test_scn_fov_option_plumbing():
    s = skr.parse_scene(scene_path("spheres2.scn"))
    h = s.info.camera[12]
    assert skr.scene_fov(s) == 2 * h and skr.Options(scn_fov=s).c.fov == np.float32(2 * h)
    assert skr.Options(fov=45.0, scn_fov=s).c.fov == 45.0  # an explicit --fov wins
    assert skr.Options().c.fov == 60.0
    o = render_cli._parse(["--path", "a.scn", "--output", "b.ppm", "--scn-fov", "--scn-fog"])
    assert o["scn_fov"] and o["scn_fog"] and "fov" not in o["_given"]
    assert "fov" in render_cli._parse(["--path", "a", "--output", "b", "--scn-fov", "--fov", "10"])["_given"]


def test_exp_spec_against_libm(checker):
    """Within 1 ulp of binary64 exp everywhere it is asked for; the exhaustive measure is tools/exp_exhaustive.c."""
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(-746, 709.7, 20000), rng.uniform(-1, 1, 20000), -rng.exponential(3, 20000), [0.0, -0.0, 1.0, -1.0]])
    for x in xs:
        got, want = checker.exp(x), math.exp(x)
        if want == 0.0 or not math.isfinite(want):
            continue
        assert abs(got - want) <= math.ulp(want), (x, got, want)
    assert checker.exp(0.0) == 1.0 and checker.exp(-1000.0) == 0.0 and checker.exp(1000.0) == math.inf and math.isnan(checker.exp(math.nan))


NOFOG_CASES = [
    ("direct", "spheres2.scn", 96, 54, dict(depth=1)),
    ("shadow", "spheres2.scn", 96, 54, dict(depth=1, shadow=True)),
    ("jsample", "spheres2.scn", 64, 36, dict(jsample=3, shadow=True, seed=11)),
    ("gillum", "spheres2.scn", 48, 27, dict(gillum=4, depth=3, shadow=True, seed=5)),
    ("strict", "spheres2.scn", 64, 36, dict(gillum=2, depth=2, shadow=True, strict=True, seed=9)),
    ("triangles", "spheres1.scn", 64, 36, dict(gillum=3, depth=2, seed=2)),
]


@pytest.mark.parametrize("name,scn,w,h,kw", NOFOG_CASES, ids=[c[0] for c in NOFOG_CASES])
def test_checker_equals_the_oracle_without_fog(checker, oracle, name, scn, w, h, kw):
    o_rgb, o_f, o_st = oracle.render(scene_path(scn), w, h, want_float=True, **kw)
    c_rgb, c_f, c_st = checker.render(scene_path(scn), w, h, None, **kw)
    assert np.array_equal(c_rgb, o_rgb)
    assert np.array_equal(c_f.view(np.uint32), o_f.view(np.uint32))
    assert c_st.tolist() == [int(o_st[0]), int(o_st[1]), int(o_st[2])]


def test_checker_fog_changes_the_frame(checker):
    a = checker.render(scene_path("spheres2.scn"), 48, 27, None, depth=1, shadow=True)[1]
    b = checker.render(scene_path("spheres2.scn"), 48, 27, [SPHERES2_FOG], depth=1, shadow=True)[1]
    assert not np.array_equal(a, b)
