"""Phong exponents, colours and light values the suite never rendered (tests/shading_values.py), on the MI355X (pytest -m gpu): the
Phong power as the kernels call it and len_terms through debug ops 20 and 21, the quantiser on negative numbers, and every case of the
catalogue on every render path that takes it, against the CPU oracle — float words, bytes and the ray, hit and shadow-ray counts, bit
for bit, NaN words included.  The kernel variant, and on the persistent node pipeline the leaf kernel's instance, are asserted, so that
no case passes on another path.  What each case reaches is held on the CPU by tests/test_shading_values_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
import shading_values as sv
from skele_raytracer_amd import binding
from fog_check import build as build_fog_checker
from soft_light_check import build as build_soft_checker
from spot_check import build as build_spot_checker
from test_shading_values_cpu import pow_reference

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = sv.SIZE
SWITCHES = ("SKR_LEAF_SHAPE", "SKR_GI_MASK", "SKR_SHADOW_MASK", "SKR_GI_SURFACE", "SKR_SHADOW_SURFACE", "SKR_PIPELINE", "SKR_FLAT", "SKR_LEVELS_BUDGET_MB",
            "SKR_PRIMARY_CACHE", "SKR_NO_CULL", "SKR_NO_CONES")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


# --------------------------------------------------------------------------------------------------------------- the unit level ----
def test_powf_spec_as_the_kernels_call_it(gpu, oracle):
    """Op 20 on every record of the catalogue: the instance that reads pow_steps equals sko_powf_shared at steps = bit_length(p) and
    at steps = 11, the instance with seven squarings compiled in wherever p <= 127, and an exponent that is not plain gives the same
    bits whatever `steps` says.

    The last block is no specification: launch.h never gives a launch with pow_steps > 7 the instance with seven squarings, so what
    that instance returns for p > 127 is out of contract.  It documents the mutation model the reach tests rest on (a step count too
    small renders the exponent's low bits, tests/test_shading_values_cpu.py) and may be dropped with a rewrite of pow_int_flat that
    behaves otherwise there."""
    rec, le7, block = sv.pow_records()
    want = pow_reference(oracle, rec).view(np.uint32)
    out = binding.debug_eval(20, rec, 2)
    bad = out[:, 0] != want
    assert not bad.any(), "%d records differ, first (x, p, steps) = %s" % (int(bad.sum()), [(float(a), float(b), int(s)) for a, b, s in
                                                                                          zip(rec[bad, 0].view(f32)[:3], rec[bad, 1].view(f32)[:3], rec[bad, 2][:3])])
    bad7 = le7 & (out[:, 1] != want)
    assert not bad7.any(), "LE7: %d records differ, first (x, p) = %s" % (int(bad7.sum()), [(float(a), float(b)) for a, b in zip(rec[bad7, 0].view(f32)[:3], rec[bad7, 1].view(f32)[:3])])
    # the seven squarings are what the reach tests say they are: handed a larger exponent they raise to its low seven bits
    wide = (block == 1) & ~le7
    p7 = rec[wide].copy()
    p7[:, 1] = (rec[wide, 1].view(f32).astype(np.int64) & 127).astype(f32).view(np.uint32)
    low = pow_reference(oracle, p7).view(np.uint32)
    assert np.array_equal(out[wide, 1], low)


def test_len_terms_on_every_float(gpu):
    """device_math.h len_terms — sqrt(ss), 1 / len and 1 / (len len) behind one range test [2^-98, 2^99) — against the correctly rounded
    expansions tests/test_gpu_units.py pins to IEEE, on each of the 2^32 binary32 operands (op 21, in the shape of op 9)."""
    hi = np.arange(65536, dtype=np.uint32).reshape(-1, 1)
    out = binding.debug_eval(21, hi, 4)
    assert out.sum(axis=0).tolist() == [0, 0, 0, 0], out.sum(axis=0)


def test_quantise_wraps_negative_numbers(gpu, oracle):
    v = sv.quantise_values()
    out = binding.debug_eval(5, v.reshape(-1, 1), 1)
    want = [oracle.lib().sko_quantise(float(x)) for x in v]
    assert out[:, 0].tolist() == want


# -------------------------------------------------------------------------------------------------------------- the frame level ----
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return str(tmp_path_factory.mktemp("shading_values_gpu"))


_scenes = {}


def scene_of(folder, case, extra_triangle=False, **flags):
    """(path, the library's scene) of a case, parsed once per loader flags"""
    key = (case.name, extra_triangle, tuple(sorted(flags.items())))
    if key not in _scenes:
        path = sv.write(case, os.path.join(folder, "%s%s.scn" % (case.name, "_t" if extra_triangle else "")), extra_triangle=extra_triangle)
        _scenes[key] = (path, skr.parse_scene(path, **dict(case.load, **flags)))
    return _scenes[key]


def frame(gpu, scene, **kw):
    """(bytes, floats, [rays, sphere hits, shadow rays], kernel variant, leaf instance) of a 64x36 frame of the scene under its own renderer"""
    r = skr.Renderer(scene)
    try:
        r.counters(reset=True)
        rgb, rgbf = r.render(skr.Options(W, H, **kw), want_float=True)
        gpu.cuda.synchronize()
        c = r.counters(reset=True)
        fn = skr.lib().skr_renderer_last_leaf_shape
        fn.argtypes, fn.restype = [C.c_void_p], C.c_int
        return rgb.cpu().numpy(), rgbf.cpu().numpy(), [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]], r.kernel_variant(), fn(r.h)
    finally:
        r.close()


def same_words(a, b):
    return np.ascontiguousarray(a, f32).view(np.uint32) == np.ascontiguousarray(b, f32).view(np.uint32)


def assert_frame(got, want, what):
    rgb, f, st = want
    eq = same_words(got[1], f)
    assert eq.all(), "%s: %d float words differ, first at %s" % (what, int((~eq).sum()), np.argwhere(~eq)[:3].tolist())
    assert np.array_equal(got[0], rgb), "%s: %d bytes differ" % (what, int((got[0] != rgb).sum()))
    assert got[2] == [int(x) for x in st[:3]], (what, got[2], [int(x) for x in st[:3]])


def oracle_frame(oracle, path, case, **kw):
    return oracle.render(path, W, H, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, strict=case.load.get("strict", False), **kw)


GI = dict(gillum=4, depth=3)
# name, switches, options, loader flags, with the extra triangle, kernel variant
PATHS = [
    ("direct", {}, dict(), {}, False, "direct_v3"),
    ("nodes_flat", {"SKR_PIPELINE": "nodes", "SKR_FLAT": "1"}, dict(GI, seed=3), {}, False, "node_levels_v5_flat"),
    ("nodes_persistent", {"SKR_PIPELINE": "nodes", "SKR_FLAT": "0"}, dict(GI, seed=4), {}, False, "node_levels_v5"),
    ("generic", {"SKR_PIPELINE": "generic"}, dict(GI, seed=5), {}, False, "level_pipeline_g1"),
    ("sphere_tree", {}, dict(gillum=3, depth=2, seed=6), dict(sphere_tree=True), False, "level_pipeline_g1_stree"),
    ("shade_triangles", {}, dict(gillum=3, depth=3, seed=7, shade_triangles=True), {}, True, "level_pipeline_g1"),
    ("legacy_reflect", {}, dict(depth=3, legacy_reflect=True), {}, False, "level_pipeline_g1"),
]
# the cases whose own keywords name a mode run on that mode's paths alone
MESH_PATHS = [
    ("shade_triangles_direct", {}, dict(), {}, False, "level_pipeline_g1"),
    ("shade_triangles_gi", {}, dict(gillum=3, depth=3, seed=7), {}, False, "level_pipeline_g1"),
    ("shade_triangles_legacy", {}, dict(depth=2, legacy_reflect=True), {}, False, "level_pipeline_g1"),
]
LEGACY_PATHS = [
    ("legacy_direct", {}, dict(depth=3), {}, False, "level_pipeline_g1"),
    ("legacy_gi", {}, dict(gillum=2, depth=2, seed=8), {}, False, "level_pipeline_g1"),
]


def paths_of(case):
    return MESH_PATHS if case.kw.get("shade_triangles") else LEGACY_PATHS if case.kw.get("legacy_reflect") else PATHS


RUNS = [(c, p) for c in sv.CASES for p in paths_of(c)]


@pytest.mark.parametrize("case,path", RUNS, ids=["%s-%s" % (c.name, p[0]) for c, p in RUNS])
def test_case_matches_the_oracle(gpu, oracle, monkeypatch, folder, case, path):
    name, env, kw, flags, extra, variant = path
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(dict(shadow=True), **dict(kw, **case.kw))
    scn, scene = scene_of(folder, case, extra, **flags)
    got = frame(gpu, scene, **kw)
    assert got[3] == variant, (case.name, name, got[3])
    if name == "nodes_persistent":  # the instance with the launch's shape compiled in (seven squarings), or the one that reads pow_steps
        assert got[4] == sv.leaf_shape(case), (case.name, got[4])
    assert_frame(got, oracle_frame(oracle, scn, case, **kw), "%s %s" % (case.name, name))


QUERIES = [("direct", dict()), ("gi4_d2", dict(gillum=4, depth=2, seed=19))]


@pytest.mark.parametrize("name,kw", QUERIES, ids=[q[0] for q in QUERIES])
@pytest.mark.parametrize("case", sv.CASES, ids=[c.name for c in sv.CASES])
def test_shade_of_the_camera_rays_is_the_oracles_frame(gpu, oracle, folder, case, name, kw):
    import torch
    kw = dict(dict(shadow=True), **dict(kw, **case.kw))
    scn, scene = scene_of(folder, case)
    r = skr.Renderer(scene)
    try:
        opt = skr.Options(W, H, **kw)
        rays = r.camera_rays(opt).view(-1, 8)
        keys = torch.arange(W * H, dtype=torch.int32, device=rays.device)
        got = r.shade(rays, opt, 0, keys=keys)
        gpu.cuda.synchronize()
        assert r.kernel_variant() == "shade_rays_g1"
    finally:
        r.close()
    want = oracle_frame(oracle, scn, case, **kw)[1]
    eq = same_words(got.cpu().numpy().reshape(H, W, 3), want)
    assert eq.all(), "%s %s: %d float words differ" % (case.name, name, int((~eq).sum()))


@pytest.mark.parametrize("path", [PATHS[0], PATHS[2], PATHS[3]], ids=["direct", "nodes_persistent", "generic"])
def test_the_scene_built_from_arrays(gpu, oracle, monkeypatch, folder, path):
    """api.cpp derives pow_steps from the packed materials, whatever built the scene: exponent 1000 through Scene.from_arrays."""
    name, env, kw, _, _, variant = path
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = sv.BY_NAME["exp_1000"]
    scn, parsed = scene_of(folder, case)
    s, t, l = parsed.arrays()
    info = parsed.info
    assert s[:, 13].max() == 1000.0
    built = skr.Scene.from_arrays(s, t, l, list(info.camera[:9]), tuple(info.background), tuple(info.ambient))
    kw = dict(dict(shadow=True), **dict(kw, **case.kw))
    got = frame(gpu, built, **kw)
    assert got[3] == variant and (name != "nodes_persistent" or got[4] == 0), (got[3], got[4])
    assert_frame(got, oracle_frame(oracle, scn, case, **kw), "from_arrays %s" % name)


@pytest.mark.parametrize("path", MESH_PATHS[:2], ids=[p[0] for p in MESH_PATHS[:2]])
@pytest.mark.parametrize("name", ["tri_256_spheres_8", "spheres_256_tri_8"])
def test_the_triangle_scenes_built_from_arrays(gpu, oracle, folder, name, path):
    """The scene whose largest exponent sits on a triangle material alone, and its converse, through Scene.from_arrays: the triangle
    materials come from the catalogue by skr_scene_set_triangle_materials, not from the parser, and api.cpp reads pow_steps from what
    that call packed.  Against the oracle's frame of the .scn file."""
    case = sv.BY_NAME[name]
    scn, parsed = scene_of(folder, case)
    s, t, l = parsed.arrays()
    info = parsed.info
    mats = sv.triangle_materials(case)
    assert len(t) == len(mats) == 1 and sorted({float(s[:, 13].max()), float(mats[0, 9])}) == [8.0, 256.0]
    built = skr.Scene.from_arrays(s, t, l, list(info.camera[:9]), tuple(info.background), tuple(info.ambient), triangle_materials=mats)
    kw = dict(dict(shadow=True), **dict(path[2], **case.kw))
    assert kw["shade_triangles"]
    got = frame(gpu, built, **kw)
    assert got[3] == path[5], got[3]
    want = oracle_frame(oracle, scn, case, **kw)
    assert_frame(got, want, "from_arrays %s %s" % (name, path[0]))
    # ... and the materials matter: with the defaults (material.h:9-17) in their place the frame is another
    plain = frame(gpu, skr.Scene.from_arrays(s, t, l, list(info.camera[:9]), tuple(info.background), tuple(info.ambient)), **kw)
    assert not np.array_equal(plain[1].view(np.uint32), want[1].view(np.uint32))


# ------------------------------------------------------------------------------ the other copies of the Blinn-Phong term ----
@pytest.fixture(scope="module")
def fog_checker(tmp_path_factory):
    return build_fog_checker(str(tmp_path_factory.mktemp("fogcheck_shading")))


@pytest.fixture(scope="module")
def spot_checker(tmp_path_factory):
    return build_spot_checker(str(tmp_path_factory.mktemp("spotcheck_shading")))


@pytest.fixture(scope="module")
def soft_checker(tmp_path_factory):
    return build_soft_checker(str(tmp_path_factory.mktemp("softcheck_shading")))


COPY_KW = dict(fov=sv.FOV, gillum=2, depth=2, shadow=True, seed=9)
FOG = np.array([[0.0, 1.5, -3.0, 6.0, 0.8, 0.7, 0.6, 0.05, 0.02]], f32)  # around the large sphere's near side and the small spheres
SPOT = np.array([[60.0, 55.0, 50.0, *sv.KEY_POSITION, 0.0, -0.1, 0.9, 12.0, 25.0]], f32)  # a second key light with a cone onto the large sphere


@pytest.mark.parametrize("case", sv.COPIES, ids=[c.name for c in sv.COPIES])
def test_exponents_through_the_fog_copy(gpu, fog_checker, folder, case):
    scn, _ = scene_of(folder, case)
    scene = skr.parse_scene(scn)
    scene.set_fog(FOG)
    got = frame(gpu, scene, **COPY_KW)
    assert got[3] == "level_pipeline_g1"
    rgb, f, st = fog_checker.render(scn, W, H, FOG, **COPY_KW)
    assert_frame(got, (rgb, f, st.tolist()), case.name + " fog")
    assert not np.array_equal(f, frame(gpu, scene_of(folder, case)[1], **COPY_KW)[1])  # the fog is in the picture


@pytest.mark.parametrize("soft", [False, True], ids=["spot", "soft"])
@pytest.mark.parametrize("case", sv.COPIES, ids=[c.name for c in sv.COPIES])
def test_exponents_through_the_cone_and_soft_light_copy(gpu, spot_checker, soft_checker, folder, case, soft):
    scn, _ = scene_of(folder, case)
    scene = skr.parse_scene(scn, spot=True)
    scene.set_spot_lights(SPOT)
    if soft:
        scene.set_light_radii([0.3, 0.0, 0.2])
    got = frame(gpu, scene, **COPY_KW)
    assert got[3] == ("level_pipeline_g1_soft" if soft else "level_pipeline_g1_spot")
    if soft:
        want = soft_checker.render(scn, W, H, radii=scene.light_radii, spots=scene.spot_lights, cones=scene.spot_cones, **COPY_KW)
    else:
        want = spot_checker.render(scn, W, H, spots=scene.spot_lights, cones=scene.spot_cones, **COPY_KW)
    assert_frame(got, want, case.name + (" soft" if soft else " spot"))
    inside = want[2][2] > 2 * want[2][1]  # more than the two point lights' shadow rays: the cone reaches hits
    assert inside
