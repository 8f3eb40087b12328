"""Motion blur on the MI355X (include/skr.h skr_scene_set_sphere_velocities): whole frames against the CPU checker
(tests/motion_checker.c) — bytes, float bits and the four work counters, no tolerance — in every mode that combines with motion, the
edges of the rule, what a scene at rest leaves alone, shading queries, adaptive frames, clones, ray queries, the debug op, the refused
combinations, both command lines.  Frames are 67 x 35 and 130 x 21: off the 64-lane and 16-pixel grids, a wave straddles rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding
from conftest import ROOT, read_ppm_bytes, scene_path
from oracle import pyoracle
from motion_check import build as build_checker, records

pytestmark = pytest.mark.gpu
f32 = np.float32
MOTION_OP = 24  # include/skr.h skr_debug_eval
SIZES = [(67, 35), (130, 21)]
ST = dict(shade_triangles=True, shadow=True)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("motioncheck_gpu")))


@pytest.fixture(scope="session")
def scenes(tmp_path_factory):
    """the scene files the golden set lacks"""
    d = tmp_path_factory.mktemp("motion_scenes")
    mat = "material 1 1 1 .6 .5 .4 .5 .5 .5 16 0 0 0 1.3\n"
    text = {
        # one light, one sphere: the pair loop with `second` false
        "one": "camera 0 1 -8 0 0 1 0 1 0 30\nbackground .1 .2 .3\n" + mat + "sphere 0 1 2 1\nambient_light .2 .2 .2\npoint_light 30 30 30 4 8 -2\n",
        # a sphere that sweeps through another
        "through": "camera 0 0 -10 0 0 1 0 1 0 30\nbackground .1 .2 .3\n" + mat + "sphere -3 0 4 1.2\nsphere 0 0 4 1.5\nsphere 0 -52 4 50\nambient_light .2 .2 .2\n"
                   "point_light 30 30 30 4 8 -2\npoint_light 20 20 40 -6 5 -4\n",
        # a sphere that sweeps over the camera: for part of the shutter the primary rays start inside it
        "over": "camera 0 0 -10 0 0 1 0 1 0 30\nbackground .1 .2 .3\n" + mat + "sphere -4 0 -10 1.5\nsphere 0 0 4 1.5\nsphere 0 -52 4 50\nambient_light .2 .2 .2\n"
                "point_light 30 30 30 4 8 -2\n",
    }
    out = {}
    for k, t in text.items():
        p = d / (k + ".scn")
        p.write_text(t)
        out[k] = str(p)
    return out


# the velocities of each scene: mixed zero and non-zero rows (spheres2: the ground and the large spheres stay, the small ones move)
def velocities(name, ns):
    v = np.zeros((ns, 3), np.float32)
    if name == "spheres2.scn":
        v[1], v[8], v[9], v[10], v[13], v[14] = (1.5, 0, 0), (0, 1, 0.5), (-1, 0.5, 0), (0.75, 0, -1), (0, 0.5, 0), (-2, 0.25, 1)
    elif name == "test.scn":
        v[0], v[2], v[3] = (-3, 0, 0), (0, 2.5, -4), (1, 1, 1)
    elif name == "one":
        v[0] = (2, 0.5, 0)
    elif name == "through":
        v[0] = (6, 0, 0)
    elif name == "over":
        v[0] = (8, 0, 0)
    return v


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def path_of(scenes, scn):
    return scenes[scn] if scn in scenes else scene_path(scn)


def load(scenes, scn, vel="default", shutter=None, *, radii=None, lens=None, **flags):
    sc = skr.parse_scene(path_of(scenes, scn), **flags)
    if radii is not None:
        sc.set_light_radii(radii)
    if lens is not None:
        sc.set_lens(*lens)
    if vel is not None:
        sc.set_velocities(velocities(scn, sc.info.n_spheres) if isinstance(vel, str) else vel)
    if shutter is not None:
        sc.set_shutter(shutter)
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
    """the checker's frame of the scene file under the library scene's velocities, shutter, spot lights, cones and radii"""
    extra = dict(velocities=sc.velocities, shutter=sc.shutter, spots=sc.spot_lights, cones=sc.spot_cones, radii=sc.light_radii, triangle_shadows=triangle_shadows, strict=strict)
    if progressive > 1:
        return checker.render_progressive(path_of(scenes, scn), w, h, progressive, **extra, **kw)
    return checker.render(path_of(scenes, scn), w, h, **extra, **kw)


def same_as_checker(gpu, checker, scenes, scn, w, h, what, *, vel="default", shutter=None, part="", radii=None, spot=False, strict=False, triangle_shadows=False, **kw):
    sc = load(scenes, scn, vel, shutter, radii=radii, spot=spot, strict=strict, triangle_shadows=triangle_shadows)
    g_rgb, g_f, g_cnt, variant = gpu_frame(gpu, sc, w, h, **kw)
    c_rgb, c_f, c_st = checker_frame(checker, scenes, sc, scn, w, h, strict=strict, triangle_shadows=triangle_shadows, **kw)
    nb = int((bits(g_f) != bits(c_f)).sum())
    assert nb == 0, "%s: %d float words differ" % (what, nb)
    assert np.array_equal(g_rgb, c_rgb), what
    assert g_cnt == [int(x) for x in c_st[:4]], what
    tsh = triangle_shadows and kw.get("shade_triangles") and kw.get("shadow") and sc.info.n_triangles > 0
    assert variant == "level_pipeline_g1" + part + "_motion" + ("_tshadow" if tsh else ""), (what, variant)
    return c_f


# ---- 1. GPU == checker, bit for bit, in every mode that combines with motion ----
SPHERE_MODES = [
    ("shadow", dict(), dict(shadow=True)),
    ("js2", dict(), dict(jsample=2, shadow=True, seed=3)),
    ("gi2_d3", dict(), dict(gillum=2, depth=3, shadow=True, seed=5)),
    ("strict", dict(strict=True), dict(shadow=True)),
    ("radius", dict(radii=0.4, part="_soft"), dict(shadow=True, seed=2)),
    ("progressive2", dict(), dict(progressive=2, shadow=True, seed=7)),
]


@pytest.mark.parametrize("scn,size", [("spheres2.scn", SIZES[1]), ("one", SIZES[0])], ids=["spheres2", "one"])
@pytest.mark.parametrize("name,flags,kw", SPHERE_MODES, ids=[m[0] for m in SPHERE_MODES])
def test_sphere_scenes_match_the_checker_bit_for_bit(gpu, checker, scenes, scn, size, name, flags, kw):
    """spheres2.scn has two point lights (the pair loop runs with `second` true), `one` has one light and one sphere"""
    on = same_as_checker(gpu, checker, scenes, scn, *size, "%s %s" % (scn, name), **flags, **kw)
    if name == "shadow":  # the motion does something
        off = checker.render(path_of(scenes, scn), *size, **kw)[1]
        assert (bits(on) != bits(off)).any()


MESH_MODES = [
    ("black_triangles", dict(), dict(shadow=True)),
    ("shade_triangles", dict(), dict(**ST)),
    ("triangle_shadows", dict(triangle_shadows=True), dict(**ST)),
    ("triangle_shadows_gi2_d3", dict(triangle_shadows=True), dict(gillum=2, depth=3, seed=5, **ST)),
    ("gi2_d2_black", dict(), dict(gillum=2, depth=2, shadow=True, seed=4)),
    ("strict_js2", dict(strict=True), dict(jsample=2, seed=3, **ST)),
    ("spot", dict(spot=True, part="_spot"), dict(shadow=True)),
    ("soft_spot_tshadow", dict(spot=True, radii=[0.4, 0.25], triangle_shadows=True, part="_soft"), dict(seed=6, **ST)),
    ("progressive2", dict(triangle_shadows=True), dict(progressive=2, seed=7, **ST)),
]


@pytest.mark.parametrize("name,flags,kw", MESH_MODES, ids=[m[0] for m in MESH_MODES])
def test_a_mesh_scene_matches_the_checker_bit_for_bit(gpu, checker, scenes, name, flags, kw):
    """test.scn: 1800 triangles among four spheres, three of which move"""
    same_as_checker(gpu, checker, scenes, "test.scn", *SIZES[0], name, **flags, **kw)


# ---- 2. the edges of the rule ----
@pytest.mark.parametrize("scn,kw", [("through", dict(shadow=True)), ("through", dict(gillum=2, depth=2, shadow=True, seed=3)), ("over", dict(shadow=True)),
                                    ("over", dict(jsample=2, shadow=True, seed=2))], ids=["through", "through_gi", "over_camera", "over_camera_js2"])
def test_spheres_that_sweep_through_each_other_and_over_the_camera(gpu, checker, scenes, scn, kw):
    same_as_checker(gpu, checker, scenes, scn, *SIZES[0], scn, **kw)
    if scn == "over":  # for part of the shutter the camera is inside the sphere ("origin inside a sphere => miss"), for part it is not
        v, c = velocities("over", 3)[0].astype(np.float64), np.array([-4.0, 0, -10])
        inside = [np.linalg.norm(c + t * v - np.array([0, 0, -10.0])) < 1.5 for t in np.linspace(0, 1, 101)]
        assert any(inside) and not all(inside)


def test_a_shutter_so_short_that_the_displacement_is_subnormal(gpu, checker, scenes):
    S = 1e-39  # tau * v <= 2e-39: below the smallest normal binary32
    on = same_as_checker(gpu, checker, scenes, "spheres2.scn", *SIZES[1], "subnormal", shutter=S, shadow=True)
    off = checker.render(scene_path("spheres2.scn"), *SIZES[1], shadow=True)[1]
    assert np.abs(on - off).max() < 1e-3  # (the picture is the still one to the eye; the launch is a motion launch all the same)


def test_surfaces_carried_outside_the_trace_ball_walk_every_triangle(gpu, checker, scenes):
    """A wave with a lane that starts outside the ball walks every triangle: correct and slower.  The frame is the checker's; and a
    shading query whose every hit lies on the sphere while it is outside the ball proves which arm ran: a tree walk counts a culling
    test at its root for every live ray, the every-triangle arm counts none."""
    w, h = SIZES[0]
    path = scene_path("test.scn")
    sc0 = skr.parse_scene(path)
    ball = sc0.trace_culling(0)[5].astype(np.float64)
    ns, nt = sc0.info.n_spheres, sc0.info.n_triangles
    vel = np.zeros((ns, 3), np.float32)
    vel[1] = (-6.0, 6.0, 3 * ball[3])  # sphere -4 4 5 2: away from the camera, up and to the left, three ball radii deep
    c1 = np.array([-4.0, 4, 5], np.float32)
    kw = dict(gillum=2, depth=2, seed=3, **ST)
    sc = load(scenes, "test.scn", vel, triangle_shadows=True)
    c_rgb, c_f, c_st = checker_frame(checker, scenes, sc, "test.scn", w, h, triangle_shadows=True, **kw)
    r = skr.Renderer(sc)
    try:
        rgb, rgbf = r.render(skr.Options(w, h, **kw), want_float=True)
        gpu.cuda.synchronize()
        c = r.work()
        assert np.array_equal(bits(rgbf.cpu().numpy()), bits(c_f)) and np.array_equal(rgb.cpu().numpy(), c_rgb)
        assert [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"], c["sphere_tests"]] == [int(x) for x in c_st[:4]]
        # the query: keys whose shutter time has carried the whole sphere out of the ball, each ray aimed at its sample's centre from 10 in front of it
        seed = 3
        keys = np.array([k for k in range(5000) if np.linalg.norm(checker.centres(checker.tau(k, 0, seed, 1.0), c1, vel[1])[0] - ball[:3]) > ball[3] + 2.5][:300], np.uint32)
        assert len(keys) == 300
        cen = np.stack([checker.centres(checker.tau(int(k), 0, seed, 1.0), c1, vel[1])[0] for k in keys])
        rays = skr.make_rays(cen + np.array([0, 0, -10], np.float32), np.broadcast_to(np.array([0, 0, 1], np.float32), cen.shape).copy())
        opt = skr.Options(w, h, seed=seed, **ST)
        r.count_triangle_work(True)
        r.triangle_work()
        got = r.shade(rays, opt, keys=gpu.as_tensor(keys.astype(np.int32), device=rays.device))
        gpu.cuda.synchronize()
        tw = r.triangle_work()
    finally:
        r.close()
    want, st = checker.shade(path, rays.cpu().numpy(), velocities=vel, shutter=1.0, triangle_shadows=True, keys=keys, seed=seed, **ST)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert int(st[1]) == len(keys)  # every ray hit its sphere, out there
    print("culling tests %d, triangle tests %d, triangles %d" % (tw["cull_tests"], tw["triangle_tests"], nt))
    assert tw["cull_tests"] == 0 and tw["triangle_tests"] > 0, tw


# ---- 3. planning: a scene at rest is a scene that never heard of motion ----
@pytest.mark.parametrize("scn,kw,variant", [("spheres2.scn", dict(shadow=True), "direct_v3"), ("spheres2.scn", dict(gillum=3, depth=3, shadow=True, seed=4), "node_levels"),
                                            ("test.scn", dict(gillum=2, depth=2, seed=4), "level_pipeline_g1")], ids=["direct", "nodes", "generic"])
def test_a_closed_shutter_or_zero_velocities_change_nothing(gpu, scenes, scn, kw, variant):
    w, h = SIZES[0]
    b = gpu_frame(gpu, skr.parse_scene(scene_path(scn)), w, h, **kw)
    ns = skr.parse_scene(scene_path(scn)).info.n_spheres
    for sc in (load(scenes, scn, "default", 0.0), load(scenes, scn, np.zeros((ns, 3), np.float32), 1.0), load(scenes, scn, np.full((ns, 3), -0.0, np.float32), 2.0)):
        a = gpu_frame(gpu, sc, w, h, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
        assert a[3] == b[3] and a[3].startswith(variant) and "motion" not in a[3]
    o_rgb, o_f, o_st = pyoracle.render(scene_path(scn), w, h, want_float=True, **kw)
    assert np.array_equal(bits(b[1]), bits(o_f)) and np.array_equal(b[0], o_rgb) and b[2] == [int(x) for x in o_st[:4]]
    moving = gpu_frame(gpu, load(scenes, scn), w, h, **kw)
    assert "_motion" in moving[3] and moving[3].startswith("level_pipeline_g1")


# ---- 4. shading queries, adaptive frames, clones, ray queries ----
@pytest.mark.parametrize("scn,kw", [("test.scn", dict(**ST)), ("spheres2.scn", dict(gillum=2, depth=3, shadow=True, seed=5))], ids=["test", "spheres2"])
def test_camera_rays_shade_to_the_frame_per_sample(gpu, checker, scenes, scn, kw):
    torch = gpu
    w, h = SIZES[0]
    sc = load(scenes, scn)
    r, still = skr.Renderer(sc), skr.Renderer(skr.parse_scene(scene_path(scn)))
    try:
        opt = skr.Options(w, h, **kw)
        rays = r.camera_rays(opt)
        assert np.array_equal(bits(rays.cpu().numpy()), bits(still.camera_rays(opt).cpu().numpy()))  # skr_camera_rays is unchanged
        frame = r.render(opt, want_float=True)[1]
        torch.cuda.synchronize()
        keys = torch.arange(w * h, dtype=torch.int32, device=rays.device)
        got = r.shade(rays.view(-1, 8), opt, keys=keys)
        torch.cuda.synchronize()
        assert "shade_rays_g1" in skr.Renderer.kernel_variant() and "_motion" in skr.Renderer.kernel_variant()
        assert np.array_equal(bits(got.cpu().numpy()), bits(frame.cpu().numpy()).reshape(-1, 3))
        # per aa of a jittered frame: the checker's samples, which the frame sums
        js = skr.Options(w, h, jsample=2, **kw)
        samples = checker.render_samples(path_of(scenes, scn), w, h, jsample=2, velocities=sc.velocities, shutter=sc.shutter, **kw)
        for aa in (0, 3):
            got = r.shade(r.camera_rays(js, sample=aa).view(-1, 8), js, sample=aa, keys=keys)
            torch.cuda.synchronize()
            assert np.array_equal(bits(got.cpu().numpy()), bits(samples[aa][0])), aa
        # a ray query answers for the scene at rest
        a, b = r.trace(rays.view(-1, 8)), still.trace(rays.view(-1, 8))
        torch.cuda.synchronize()
        assert np.array_equal(a.raw.cpu().numpy().view(np.uint32), b.raw.cpu().numpy().view(np.uint32))
    finally:
        r.close()
        still.close()


def test_adaptive_frames_bands_tiles_and_clones(gpu, checker, scenes, monkeypatch):
    w, h = SIZES[0]
    K = 2
    kw = dict(gillum=2, depth=2, shadow=True, seed=9)
    sc = load(scenes, "spheres2.scn")
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
        # strided tiles: the two interleaved halves
        rows = 4
        for first in (0, 1):
            rgb, rgbf = r.render(opt, want_float=True, tile_rows=rows, first_tile=first, tile_stride=2)
            gpu.cuda.synchronize()
            for k in range(rgb.shape[0] // rows):
                y0 = (first + 2 * k) * rows
                n = min(rows, h - y0)
                assert np.array_equal(bits(rgbf[k * rows:k * rows + n].cpu().numpy()), bits(one[1][y0:y0 + n])), (first, k)
                assert np.array_equal(rgb[k * rows:k * rows + n].cpu().numpy(), one[0][y0:y0 + n])
        clone = r.clone()  # a clone carries the motion
        try:
            assert np.array_equal(bits(clone.render(opt, want_float=True)[1].cpu().numpy()), bits(one[1]))
            gpu.cuda.synchronize()
            assert "_motion" in skr.Renderer.kernel_variant()
        finally:
            clone.close()
    finally:
        r.close()
    m = binding.Multi(sc, 1)  # the frame step's renderer takes the motion with the scene
    try:
        rgb, _ = m.render_frame_host(skr.Options(w, h, **kw), tile_rows=8)
    finally:
        m.close()
    assert np.array_equal(rgb, one[0])


def test_a_banded_frame_is_the_frame(gpu, checker, scenes):
    w, h = SIZES[1]
    kw = dict(gillum=5, depth=4, shadow=True, seed=6)  # (tests/test_lens_gpu.py: 15 MB of records at the last level, two bands under 16 MB)
    sc = load(scenes, "spheres2.scn")
    whole = gpu_frame(gpu, sc, w, h, **kw)
    os.environ["SKR_LEVELS_BUDGET_MB"] = "16"
    try:
        banded = gpu_frame(gpu, sc, w, h, **kw)
    finally:
        del os.environ["SKR_LEVELS_BUDGET_MB"]
    assert np.array_equal(bits(banded[1]), bits(whole[1])) and np.array_equal(banded[0], whole[0]) and banded[2] == whole[2] and banded[3] == whole[3]
    c_rgb, c_f, c_st = checker_frame(checker, scenes, sc, "spheres2.scn", w, h, **kw)
    assert np.array_equal(bits(whole[1]), bits(c_f)) and np.array_equal(whole[0], c_rgb) and whole[2] == [int(x) for x in c_st[:4]]


# ---- 5. the debug op ----
def test_the_shutter_time_and_the_centre_through_the_debug_op(gpu, checker):
    rng = np.random.default_rng(11)  # the cases of tests/test_motion_cpu.py, and as many again
    n = 4096 + 37
    px = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    aa = rng.integers(0, 1024, n, dtype=np.uint64)
    seed = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    S = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), n)).astype(np.float32)
    c = rng.normal(0, 20, (n, 3)).astype(np.float32)
    v = (rng.normal(0, 5, (n, 3)) * np.exp(rng.uniform(-8, 3, (n, 1)))).astype(np.float32)
    rec = records(px, aa, seed, S, c, v)
    edge = np.concatenate([
        records([0, 2 ** 32 - 1, 0, 2 ** 32 - 1], [0, 0, 2 ** 20 - 1, 3], [0, 1, 2 ** 64 - 1, 2 ** 32], 0.75, (1.5, -2.25, 1e-30), (3.0, -7.0, 11.0)),
        records(7, 1, 5, [0.0, 1.0, 1e-39, 1e-30, 1.0, 5.0], [(1.5, -2.25, 1e-30), (1.5, -2.25, 0.0), (0.0, 1e-39, -1e-38), (1.0, -1.0, 5.0), (-3.0, 2.1, -1.0), (1.0, 2.0, 3.0)],
                [(3.0, -7.0, 11.0), (0.0, -0.0, 0.0), (1e-10, -3e-12, 2e-9), (1e-10, -3e-12, 2e-9), (10.0, -7.0, 3.3333333), (3e37, -3e37, 1e36)]),
    ])
    for r in (rec, edge):
        got = binding.debug_eval(MOTION_OP, r, 4)
        assert np.array_equal(got, bits(checker.samples(r)))


# ---- 6. the refused combinations ----
def test_the_refused_combinations(gpu, scenes):
    fog_rows = np.array([[0, 0, 5, 3, .5, .5, .5, .1, .05]], np.float32)

    def cases(shutter):
        out = [(load(scenes, "spheres2.scn", shutter=shutter), dict(legacy_reflect=True), "--legacy-reflect")]
        fog = load(scenes, "spheres2.scn", shutter=shutter, fog=True)
        fog.set_fog(fog_rows)
        out.append((fog, dict(), "fog volumes"))
        out.append((load(scenes, "spheres2.scn", shutter=shutter, sphere_tree=True), dict(), "sphere tree"))
        out.append((load(scenes, "spheres2.scn", shutter=shutter, lens=(0.3, 11.0)), dict(), "a lens (--aperture)"))
        return out

    for sc, kw, text in cases(None):
        r = skr.Renderer(sc)
        try:
            with pytest.raises(skr.SkrError) as e:
                r.render(skr.Options(32, 24, **kw))
            assert "(status 4)" in str(e.value) and "motion blur" in str(e.value) and text in str(e.value), str(e.value)
        finally:
            r.close()
    for sc, kw, text in cases(0.0):  # none of them is refused while the shutter is closed
        r = skr.Renderer(sc)
        try:
            r.render(skr.Options(32, 24, **kw))
            gpu.cuda.synchronize()
            assert "motion" not in skr.Renderer.kernel_variant()
        finally:
            r.close()
    opt = skr.Options(32, 24, shadow=True)
    r = skr.Renderer(load(scenes, "spheres2.scn"))
    try:
        for call in (lambda: r.render_denoised(opt), lambda: r.render_adaptive_denoised(opt, min_passes=2, max_passes=2)):
            with pytest.raises(skr.SkrError) as e:
                call()
            assert "(status 4)" in str(e.value) and "motion blur" in str(e.value) and "denoiser" in str(e.value), str(e.value)
    finally:
        r.close()
    r = skr.Renderer(load(scenes, "spheres2.scn", shutter=0.0))
    try:
        r.render_denoised(opt)
        r.render_adaptive_denoised(opt, min_passes=2, max_passes=2)
        gpu.cuda.synchronize()
    finally:
        r.close()


# ---- 7. both command lines ----
def test_both_command_lines_take_the_flags(gpu, tmp_path):
    w, h = SIZES[0]
    text = open(scene_path("spheres2.scn")).read().split("\n")
    out, n = [], 0
    for ln in text:
        if ln.startswith("sphere"):
            n += 1
            if n == 2:
                out.append("velocity 1.5 0 0")
            if n == 3:
                out.append("velocity 0 0 0")
            if n == 9:
                out.append("velocity 0 1 0.5")
        out.append(ln)
    scn = tmp_path / "moving.scn"
    scn.write_text("\n".join(out))
    args = ["--path", str(scn), "--width", str(w), "--height", str(h), "--shadow", "--seed", "3", "--progressive", "2", "--scn-motion", "--shutter", "0.5"]
    sc = skr.parse_scene(str(scn), motion=True)
    assert sc.velocities[1].tolist() == [1.5, 0, 0] and not sc.velocities[2].any() and sc.velocities[8:].tolist() == [[0, 1, 0.5]] * (sc.info.n_spheres - 8)
    sc.set_shutter(0.5)
    want = gpu_frame(gpu, sc, w, h, shadow=True, seed=3, progressive=2)
    assert "_motion" in want[3]
    off = gpu_frame(gpu, skr.parse_scene(scene_path("spheres2.scn")), w, h, shadow=True, seed=3, progressive=2)[0]
    assert (want[0] != off).any()
    exe = os.path.join(ROOT, "bin", "raytracer")
    out1, out2, out3 = str(tmp_path / "native.ppm"), str(tmp_path / "py.ppm"), str(tmp_path / "noflag.ppm")
    subprocess.run([exe, *args, "--output", out1, "--quiet"], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL, timeout=300)
    subprocess.run([sys.executable, "-m", "skele_raytracer_amd.render_cli", *args, "--output", out2], check=True, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=300)
    for o in (out1, out2):
        assert np.array_equal(read_ppm_bytes(open(o, "rb").read()), want[0]), o
    # without --scn-motion the velocity lines are unknown commands and --shutter has no effect
    subprocess.run([exe, *[a for a in args if a != "--scn-motion"], "--output", out3, "--quiet"], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL, timeout=300)
    assert np.array_equal(read_ppm_bytes(open(out3, "rb").read()), off)
    bad = subprocess.run([exe, *args[:-1], "-1", "--output", str(tmp_path / "bad.ppm"), "--quiet"], cwd=str(tmp_path), capture_output=True, timeout=300)
    assert bad.returncode == 2 and b"--shutter" in bad.stderr and not os.path.exists(str(tmp_path / "bad.ppm"))
