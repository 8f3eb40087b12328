"""The environment map on the MI355X (include/skr.h skr_scene_set_environment): whole frames against the CPU checker
(tests/env_checker.c) — bytes, float bits and the four work counters, no tolerance — in every mode that combines with an environment,
a constant map against the frame without one on every path, shading queries, the lookup's index bounds, adaptive frames, tiles, bands,
clones and skr_multi, the debug op, the refused combinations, both command lines.  Frames are 67 x 35 and 130 x 21: off the 64-lane and
16-pixel grids, a wave straddles rows.  Every frame case is conditioned on the checker's own counts: at least a tenth of its primary
rays miss, and where it has GI some child ray looks the map up."""
import os
import subprocess
import sys

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding
from conftest import ROOT, read_ppm_bytes, scene_path
from oracle import pyoracle
from env_check import build as build_checker, edge_directions, records

pytestmark = pytest.mark.gpu
f32 = np.float32
ENV_OP = 25  # include/skr.h skr_debug_eval
SIZES = [(67, 35), (130, 21)]
ST = dict(shade_triangles=True, shadow=True)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("envcheck_gpu")))


@pytest.fixture(scope="session")
def scenes(tmp_path_factory):
    """the scene files the golden set lacks"""
    d = tmp_path_factory.mktemp("env_scenes")
    mat = "material 1 1 1 .6 .5 .4 .5 .5 .5 16 0 0 0 1.3\n"
    text = {
        # one light, one sphere, most of the frame the backdrop
        "one": "camera 0 1 -8 0 0 1 0 1 0 30\nbackground .1 .2 .3\n" + mat + "sphere 0 1 2 1\nambient_light .2 .2 .2\npoint_light 30 30 30 4 8 -2\n",
    }
    out = {}
    for k, t in text.items():
        p = d / (k + ".scn")
        p.write_text(t)
        out[k] = str(p)
    return out


def env_map(E, seed=1):
    """a random map: every texel its own colour, so a wrong tap or weight shows"""
    return np.random.default_rng(seed).uniform(0.0, 3.0, (E, E, 3)).astype(np.float32)


def velocities(name, ns):
    v = np.zeros((ns, 3), np.float32)
    if name == "spheres2.scn":
        v[1], v[8], v[9], v[10], v[13], v[14] = (1.5, 0, 0), (0, 1, 0.5), (-1, 0.5, 0), (0.75, 0, -1), (0, 0.5, 0), (-2, 0.25, 1)
    elif name == "test.scn":
        v[0], v[2], v[3] = (-3, 0, 0), (0, 2.5, -4), (1, 1, 1)
    else:
        v[0] = (2, 0.5, 0)
    return v


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def path_of(scenes, scn):
    return scenes[scn] if scn in scenes else scene_path(scn)


def load(scenes, scn, env, *, motion=False, radii=None, lens=None, **flags):
    sc = skr.parse_scene(path_of(scenes, scn), **flags)
    if radii is not None:
        sc.set_light_radii(radii)
    if lens is not None:
        sc.set_lens(*lens)
    if motion:
        sc.set_velocities(velocities(scn, sc.info.n_spheres))
    if env is not None:
        sc.set_environment(env)
    return sc


def gpu_frame(gpu, scene, w, h, **kw):
    """(bytes, floats, the four work counters, kernel variant) of a frame of the scene under its own renderer"""
    r = skr.Renderer(scene)
    try:
        rgb, rgbf = r.render(skr.Options(w, h, **kw), want_float=True)
        gpu.cuda.synchronize()
        c = r.work()
        return rgb.cpu().numpy(), rgbf.cpu().numpy(), [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"], c["sphere_tests"]], skr.Renderer.kernel_variant()
    finally:
        r.close()


def checker_frame(checker, scenes, sc, scn, w, h, *, strict=False, triangle_shadows=False, progressive=1, **kw):
    """the checker's frame of the scene file under the library scene's environment, lens, velocities, shutter, spot lights, cones and radii"""
    A, F = sc.lens
    extra = dict(environment=sc.environment, aperture=A, focus=F, velocities=sc.velocities, shutter=sc.shutter, spots=sc.spot_lights, cones=sc.spot_cones, radii=sc.light_radii,
                 triangle_shadows=triangle_shadows, strict=strict)
    if progressive > 1:
        return checker.render_progressive(path_of(scenes, scn), w, h, progressive, **extra, **kw)
    return checker.render(path_of(scenes, scn), w, h, **extra, **kw)


def the_case_is_about_something(c_st, w, h, kw):
    """the condition on every frame case, from the checker's counts alone: a tenth of the primary rays miss into the map; with GI a child does"""
    primaries = w * h * max(1, kw.get("jsample", 0)) ** 2 * kw.get("progressive", 1)
    assert int(c_st[5]) * 10 >= primaries, (int(c_st[5]), primaries)
    if kw.get("gillum"):
        assert int(c_st[6]) >= 1


def same_as_checker(gpu, checker, scenes, scn, w, h, what, *, E=8, part="", motion=False, radii=None, lens=None, spot=False, strict=False, triangle_shadows=False, **kw):
    sc = load(scenes, scn, env_map(E, seed=E), motion=motion, radii=radii, lens=lens, spot=spot, strict=strict, triangle_shadows=triangle_shadows)
    g_rgb, g_f, g_cnt, variant = gpu_frame(gpu, sc, w, h, **kw)
    c_rgb, c_f, c_st = checker_frame(checker, scenes, sc, scn, w, h, strict=strict, triangle_shadows=triangle_shadows, **kw)
    the_case_is_about_something(c_st, w, h, kw)
    nb = int((bits(g_f) != bits(c_f)).sum())
    assert nb == 0, "%s: %d float words differ" % (what, nb)
    assert np.array_equal(g_rgb, c_rgb), what
    assert g_cnt == [int(x) for x in c_st[:4]], what
    tsh = triangle_shadows and kw.get("shade_triangles") and kw.get("shadow") and sc.info.n_triangles > 0
    assert variant == "level_pipeline_g1" + part + ("_motion" if motion else "_lens" if lens else "") + ("_tshadow" if tsh else "") + "_env", (what, variant)
    return c_f


# ---- 1. GPU == checker, bit for bit, in every mode that combines with an environment ----
SPHERE_MODES = [
    ("shadow", dict(E=8), dict(shadow=True)),
    ("js2", dict(E=3), dict(jsample=2, shadow=True, seed=3)),
    ("gi2_d3", dict(E=64), dict(gillum=2, depth=3, shadow=True, seed=5)),
    ("gi4_d2", dict(E=2), dict(gillum=4, depth=2, shadow=True, seed=4)),
    ("gi2_d4", dict(E=8), dict(gillum=2, depth=4, seed=6)),
    ("strict", dict(E=1, strict=True), dict(shadow=True)),
    ("radius", dict(E=8, radii=0.4, part="_soft"), dict(shadow=True, seed=2)),
    ("motion_gi2_d3", dict(E=3, motion=True), dict(gillum=2, depth=3, shadow=True, seed=5)),
    ("lens_js2", dict(E=64, lens=(0.3, 11.0)), dict(jsample=2, shadow=True, seed=3)),
    ("lens_gi4_d3", dict(E=2, lens=(0.2, 9.0)), dict(gillum=4, depth=3, seed=8)),
    ("progressive2", dict(E=3), dict(progressive=2, gillum=2, depth=2, shadow=True, seed=7)),
]


@pytest.mark.parametrize("scn,size", [("spheres2.scn", SIZES[1]), ("one", SIZES[0])], ids=["spheres2", "one"])
@pytest.mark.parametrize("name,flags,kw", SPHERE_MODES, ids=[m[0] for m in SPHERE_MODES])
def test_sphere_scenes_match_the_checker_bit_for_bit(gpu, checker, scenes, scn, size, name, flags, kw):
    """spheres2.scn has two point lights and fifteen spheres, `one` has one light and one sphere in front of the backdrop"""
    on = same_as_checker(gpu, checker, scenes, scn, *size, "%s %s" % (scn, name), **flags, **kw)
    if name == "shadow":  # the environment does something
        off = checker.render(path_of(scenes, scn), *size, **kw)[1]
        assert (bits(on) != bits(off)).any()


MESH_MODES = [
    ("black_triangles", dict(E=8), dict(shadow=True)),
    ("gi2_d2_black", dict(E=3), dict(gillum=2, depth=2, shadow=True, seed=4)),
    ("shade_triangles", dict(E=64), dict(**ST)),
    ("triangle_shadows", dict(E=2, triangle_shadows=True), dict(**ST)),
    ("triangle_shadows_gi2_d3", dict(E=8, triangle_shadows=True), dict(gillum=2, depth=3, seed=5, **ST)),
    ("strict_js2", dict(E=1, strict=True), dict(jsample=2, seed=3, **ST)),
    ("spot", dict(E=8, spot=True, part="_spot"), dict(shadow=True)),
    ("soft_spot_tshadow_gi2", dict(E=3, spot=True, radii=[0.4, 0.25], triangle_shadows=True, part="_soft"), dict(gillum=2, depth=2, seed=6, **ST)),
    ("motion_tshadow", dict(E=8, motion=True, triangle_shadows=True), dict(**ST)),
]


@pytest.mark.parametrize("name,flags,kw", MESH_MODES, ids=[m[0] for m in MESH_MODES])
def test_a_mesh_scene_matches_the_checker_bit_for_bit(gpu, checker, scenes, name, flags, kw):
    """test.scn: 1800 triangles among four spheres.  Without --shade-triangles a triangle blackens the ray it stops: black, not the map."""
    same_as_checker(gpu, checker, scenes, "test.scn", *SIZES[0], name, **flags, **kw)


# ---- 2. a constant map equal to the background is the frame without an environment, on whichever path that frame takes ----
@pytest.mark.parametrize("scn,kw,variant", [("spheres2.scn", dict(shadow=True), "direct_v3"), ("spheres2.scn", dict(gillum=3, depth=3, shadow=True, seed=4), "node_levels"),
                                            ("test.scn", dict(gillum=2, depth=2, seed=4), "level_pipeline_g1")], ids=["direct", "nodes", "generic"])
def test_a_constant_map_equal_to_the_background_changes_nothing_but_the_path(gpu, scenes, scn, kw, variant):
    w, h = SIZES[0]
    plain = skr.parse_scene(scene_path(scn))
    b = gpu_frame(gpu, plain, w, h, **kw)
    assert b[3].startswith(variant) and "env" not in b[3]
    o_rgb, o_f, o_st = pyoracle.render(scene_path(scn), w, h, want_float=True, **kw)
    assert np.array_equal(bits(b[1]), bits(o_f)) and np.array_equal(b[0], o_rgb) and b[2] == [int(x) for x in o_st[:4]]
    bg = np.array(list(plain.info.background), np.float32)
    for E in (1, 4):
        sc = load(scenes, scn, np.broadcast_to(bg, (E, E, 3)).copy())
        a = gpu_frame(gpu, sc, w, h, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2], E
        assert a[3] == "level_pipeline_g1_env"
    sc.set_environment(None)  # cleared: the scene plans, names and renders as it did
    a = gpu_frame(gpu, sc, w, h, **kw)
    assert a[3] == b[3] and np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]


# ---- 3. shading queries ----
@pytest.mark.parametrize("scn,kw", [("test.scn", dict(**ST)), ("spheres2.scn", dict(gillum=2, depth=3, shadow=True, seed=5))], ids=["test", "spheres2"])
def test_camera_rays_shade_to_the_frame_per_sample(gpu, checker, scenes, scn, kw):
    torch = gpu
    w, h = SIZES[0]
    sc = load(scenes, scn, env_map(8))
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, **kw)
        rays = r.camera_rays(opt)
        frame = r.render(opt, want_float=True)[1]
        torch.cuda.synchronize()
        keys = torch.arange(w * h, dtype=torch.int32, device=rays.device)
        got = r.shade(rays.view(-1, 8), opt, keys=keys)
        torch.cuda.synchronize()
        assert skr.Renderer.kernel_variant() == "shade_rays_g1_env"
        assert np.array_equal(bits(got.cpu().numpy()), bits(frame.cpu().numpy()).reshape(-1, 3))
        js = skr.Options(w, h, jsample=2, **kw)  # per aa of a jittered frame: the checker's samples, which the frame sums
        samples = checker.render_samples(path_of(scenes, scn), w, h, jsample=2, environment=sc.environment, **kw)
        for aa in (0, 3):
            got = r.shade(r.camera_rays(js, sample=aa).view(-1, 8), js, sample=aa, keys=keys)
            torch.cuda.synchronize()
            assert np.array_equal(bits(got.cpu().numpy()), bits(samples[aa][0])), aa
    finally:
        r.close()


def corner_directions():
    """the -y pole from every side (the four corners of the square), the four borders, and the folds"""
    e = 1e-6
    rows = [(sx * a, -1.0, sz * b) for sx in (-1, 1) for sz in (-1, 1) for a, b in ((e, e), (0.0, 0.0), (e, 0.0), (0.0, e), (0.3, e), (e, 0.3))]
    rows += [(sx, -e, sz * 0.5) for sx in (-1, 1) for sz in (-1, 1)] + [(sx * 0.5, -e, sz) for sx in (-1, 1) for sz in (-1, 1)]
    rows += [(sx * 0.5, s, sz * 0.5) for sx in (-1, 1) for sz in (-1, 1) for s in (0.0, -0.0, e, -e)]
    return np.array(rows, np.float32)


def test_queries_that_miss_return_the_map_and_no_direction_reads_outside_it(gpu, checker, scenes):
    torch = gpu
    E = 3
    env = np.full((E, E, 3), 0.5, np.float32)  # the last row and column differ from the rest: a tap one past them would show
    env[E - 1, :] = (7.0, 1.0, 2.0)
    env[:, E - 1] = (3.0, 9.0, 4.0)
    env[E - 1, E - 1] = (11.0, 12.0, 13.0)
    env[0, 0] = (0.25, 0.125, 6.0)
    sc = load(scenes, "spheres2.scn", env)
    bg = np.array(list(sc.info.background), np.float32)
    d = np.concatenate([corner_directions(), edge_directions()])
    o = np.zeros_like(d) + np.array([0.0, 30.0, 0.0], np.float32)
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(*SIZES[0], shadow=True)
        # cut at tmax = 0.5 (no surface is accepted below t = 1): every ray is a miss, whatever lies along it
        rays = skr.make_rays(o, d, tmax=0.5)
        got = r.shade(rays, opt).cpu().numpy()
        torch.cuda.synchronize()
        want = checker.lookup(env, d, background=bg)
        assert np.array_equal(bits(got), bits(want))
        w2, st = checker.shade(scene_path("spheres2.scn"), rays.cpu().numpy(), environment=env, shadow=True)
        assert np.array_equal(bits(got), bits(w2)) and int(st[5]) == len(d) and int(st[1]) == 0
        taps = checker.taps(d, E)
        arm = taps[:, 0] == 1  # d = 0, NaN, inf, s overflowing: the background
        assert arm.sum() >= 12 and np.array_equal(bits(got[arm]), bits(np.broadcast_to(bg, (int(arm.sum()), 3))))
        for corner in ((0, 0), (0, E - 1), (E - 1, 0), (E - 1, E - 1)):  # all four corners are looked up, alone
            at = (~arm) & (taps[:, 1] == corner[1]) & (taps[:, 2] == corner[1]) & (taps[:, 3] == corner[0]) & (taps[:, 4] == corner[0])
            assert at.any() and np.array_equal(got[at], np.broadcast_to(env[corner], (int(at.sum()), 3))), corner
        # rays whose winner lies beyond tmax, against the same rays uncut: the cut ones are the map, the others the scene
        rays2 = r.camera_rays(opt).view(-1, 8).clone()
        hit = r.trace(rays2)
        torch.cuda.synchronize()
        rays2[:, 3] = 1.5
        got2 = r.shade(rays2, opt).cpu().numpy()
        torch.cuda.synchronize()
        want2, st2 = checker.shade(scene_path("spheres2.scn"), rays2.cpu().numpy(), environment=env, shadow=True)
        assert np.array_equal(bits(got2), bits(want2)) and int(st2[5]) > 0
    finally:
        r.close()


# ---- 4. the other entry points ----
def test_adaptive_frames_tiles_clones_and_multi(gpu, checker, scenes, monkeypatch):
    w, h = SIZES[0]
    K = 2
    kw = dict(gillum=2, depth=2, shadow=True, seed=9)
    sc = load(scenes, "spheres2.scn", env_map(8))
    want = checker_frame(checker, scenes, sc, "spheres2.scn", w, h, progressive=K, **kw)
    one = checker_frame(checker, scenes, sc, "spheres2.scn", w, h, **kw)
    r = skr.Renderer(sc)
    try:
        opt = skr.Options(w, h, **kw)
        # one whole frame, then a round in which nothing converges: as whole frames, and as shading queries keyed by pixel
        for path in ("frame", "query"):
            monkeypatch.setenv("SKR_ADAPTIVE_PATH", path)
            rgb, rgbf, passes, _ = r.render_adaptive_host(opt, threshold=-1.0, min_passes=1, max_passes=K, want_float=True)
            assert (passes == K).all(), path
            assert np.array_equal(bits(rgbf), bits(want[1])) and np.array_equal(rgb, want[0]), path
        monkeypatch.delenv("SKR_ADAPTIVE_PATH")
        rows = 4  # strided tiles: the two interleaved halves
        for first in (0, 1):
            rgb, rgbf = r.render(opt, want_float=True, tile_rows=rows, first_tile=first, tile_stride=2)
            gpu.cuda.synchronize()
            for k in range(rgb.shape[0] // rows):
                y0 = (first + 2 * k) * rows
                n = min(rows, h - y0)
                assert np.array_equal(bits(rgbf[k * rows:k * rows + n].cpu().numpy()), bits(one[1][y0:y0 + n])), (first, k)
                assert np.array_equal(rgb[k * rows:k * rows + n].cpu().numpy(), one[0][y0:y0 + n])
        clone = r.clone()  # a clone shares the environment
        try:
            assert np.array_equal(bits(clone.render(opt, want_float=True)[1].cpu().numpy()), bits(one[1]))
            gpu.cuda.synchronize()
            assert skr.Renderer.kernel_variant() == "level_pipeline_g1_env"
        finally:
            clone.close()
    finally:
        r.close()
    m = binding.Multi(sc, 1)  # the frame step's renderer takes the environment with the scene
    try:
        rgb, _ = m.render_frame_host(skr.Options(w, h, **kw), tile_rows=8)
    finally:
        m.close()
    assert np.array_equal(rgb, one[0])


def test_a_banded_frame_is_the_frame(gpu, checker, scenes):
    w, h = SIZES[1]
    kw = dict(gillum=5, depth=4, shadow=True, seed=6)  # (tests/test_lens_gpu.py: 15 MB of records at the last level, two bands under 16 MB)
    sc = load(scenes, "spheres2.scn", env_map(8))
    whole = gpu_frame(gpu, sc, w, h, **kw)
    os.environ["SKR_LEVELS_BUDGET_MB"] = "16"
    try:
        banded = gpu_frame(gpu, sc, w, h, **kw)
    finally:
        del os.environ["SKR_LEVELS_BUDGET_MB"]
    assert np.array_equal(bits(banded[1]), bits(whole[1])) and np.array_equal(banded[0], whole[0]) and banded[2] == whole[2] and banded[3] == whole[3]
    c_rgb, c_f, c_st = checker_frame(checker, scenes, sc, "spheres2.scn", w, h, **kw)
    the_case_is_about_something(c_st, w, h, kw)
    assert np.array_equal(bits(whole[1]), bits(c_f)) and np.array_equal(whole[0], c_rgb) and whole[2] == [int(x) for x in c_st[:4]]


# ---- 5. the debug op ----
def test_the_taps_through_the_debug_op(gpu, checker):
    rng = np.random.default_rng(11)
    d = (rng.normal(0, 1, (4096 + 37, 3)) * np.exp(rng.uniform(-30, 30, (4096 + 37, 1)))).astype(np.float32)
    d[:1000, 1] = -np.abs(d[:1000, 1]) * 1e3
    d[1000:2000, rng.integers(0, 3, 1000)] *= 1e-7
    for E in (1, 2, 3, 8, 4096):
        for dirs in (edge_directions(), d):
            got = binding.debug_eval(ENV_OP, records(dirs, E), 7)
            assert np.array_equal(got, checker.taps(dirs, E)), E


# ---- 6. the refused combinations ----
def test_the_refused_combinations(gpu, scenes):
    fog_rows = np.array([[0, 0, 5, 3, .5, .5, .5, .1, .05]], np.float32)

    def cases(env):
        out = [(load(scenes, "spheres2.scn", env), dict(legacy_reflect=True), "--legacy-reflect")]
        fog = load(scenes, "spheres2.scn", env, fog=True)
        fog.set_fog(fog_rows)
        out.append((fog, dict(), "fog volumes"))
        out.append((load(scenes, "spheres2.scn", env, sphere_tree=True), dict(), "sphere tree"))
        return out

    for sc, kw, text in cases(env_map(2)):
        r = skr.Renderer(sc)
        try:
            with pytest.raises(skr.SkrError) as e:
                r.render(skr.Options(32, 24, **kw))
            assert "(status 4)" in str(e.value) and "environment map (--envmap)" in str(e.value) and text in str(e.value), str(e.value)
        finally:
            r.close()
        sc.set_environment(None)  # none of them is refused once the environment is cleared
        r = skr.Renderer(sc)
        try:
            r.render(skr.Options(32, 24, **kw))
            gpu.cuda.synchronize()
            assert "env" not in skr.Renderer.kernel_variant()
        finally:
            r.close()
    opt = skr.Options(32, 24, shadow=True)
    sc = load(scenes, "spheres2.scn", env_map(2))
    r = skr.Renderer(sc)
    try:
        for call in (lambda: r.render_denoised(opt), lambda: r.render_adaptive_denoised(opt, min_passes=2, max_passes=2)):
            with pytest.raises(skr.SkrError) as e:
                call()
            assert "(status 4)" in str(e.value) and "environment map" in str(e.value) and "denoiser" in str(e.value), str(e.value)
        # skr_denoise on guides the caller supplies stays as it is
        rgbf = r.render(opt, want_float=True)[1]
        r.denoise(rgbf, r.trace(r.camera_rays(opt).view(-1, 8)), 2)
        gpu.cuda.synchronize()
    finally:
        r.close()
    sc.set_environment(None)
    r = skr.Renderer(sc)
    try:
        r.render_denoised(opt)
        r.render_adaptive_denoised(opt, min_passes=2, max_passes=2)
        gpu.cuda.synchronize()
    finally:
        r.close()


# ---- 7. both command lines ----
def test_both_command_lines_take_the_flag_and_a_frame_fed_back_as_the_map(gpu, tmp_path):
    w, h = SIZES[0]
    scn = scene_path("spheres2.scn")
    exe = os.path.join(ROOT, "bin", "raytracer")
    # a square frame written with --format pfm is the map of the frames that follow
    sky = str(tmp_path / "sky.pfm")
    subprocess.run([exe, "--path", scn, "--width", "24", "--height", "24", "--shadow", "--format", "pfm", "--output", sky, "--quiet"], check=True, cwd=str(tmp_path),
                   stdout=subprocess.DEVNULL, timeout=300)
    env = skr.read_pfm(sky)
    first = gpu_frame(gpu, skr.parse_scene(scn), 24, 24, shadow=True)
    assert env.shape == (24, 24, 3) and np.array_equal(bits(env), bits(first[1]))
    sc = skr.parse_scene(scn)
    sc.set_environment(env)
    kw = dict(gillum=2, depth=2, shadow=True, seed=3)
    want = gpu_frame(gpu, sc, w, h, **kw)
    assert want[3] == "level_pipeline_g1_env"
    off = gpu_frame(gpu, skr.parse_scene(scn), w, h, **kw)[0]
    assert (want[0] != off).any()
    args = ["--path", scn, "--width", str(w), "--height", str(h), "--shadow", "--gillum", "2", "--depth", "2", "--seed", "3", "--envmap", sky]
    out1, out2, out3 = str(tmp_path / "native.ppm"), str(tmp_path / "py.ppm"), str(tmp_path / "noflag.ppm")
    subprocess.run([exe, *args, "--output", out1, "--quiet"], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL, timeout=300)
    subprocess.run([sys.executable, "-m", "skele_raytracer_amd.render_cli", *args, "--output", out2], check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=300)
    for o in (out1, out2):
        assert np.array_equal(read_ppm_bytes(open(o, "rb").read()), want[0]), o
    subprocess.run([exe, *args[:-2], "--output", out3, "--quiet"], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL, timeout=300)
    assert np.array_equal(read_ppm_bytes(open(out3, "rb").read()), off)
    wide = str(tmp_path / "wide.pfm")
    skr.write_pfm(wide, np.zeros((4, 6, 3), np.float32))
    bad = subprocess.run([exe, *args[:-1], wide, "--output", str(tmp_path / "bad.ppm"), "--quiet"], cwd=str(tmp_path), capture_output=True, timeout=300)
    assert bad.returncode == 2 and b"--envmap" in bad.stderr and wide.encode() in bad.stderr and not os.path.exists(str(tmp_path / "bad.ppm"))
