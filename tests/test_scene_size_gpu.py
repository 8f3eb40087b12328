"""Scene sizes up to what the LDS holds (pytest -m gpu): every render path stages the scene table in LDS (launch.h
skr_scene_lds_bytes), and a frame is accepted wherever one of its paths fits the device's workgroup LDS.  These tests take the sphere
and light counts to the byte boundaries of each path (64 KiB, the device limit, the largest scene accepted at all and one past it),
computed from the same formulas the planner uses, and check every kernel family there bit for bit against the oracle and the
checkers, counts included; past the limit a frame is a clean SKR_ERR_UNSUPPORTED and ray queries (which read the scene from global
memory) still answer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import skele_raytracer_amd as skr
from fog_check import build as build_fog_checker
from ray_query_check import build as build_ray_checker
from test_gpu_parity import compare
from test_ray_query_gpu import random_rays

pytestmark = pytest.mark.gpu

# render_nodes.hip: the leaf kernel's per-wave rings and windows, LEAF2_WAVE_FLOATS = NQ_CAP * NQ_F + NWIN * WIN_FLOATS
LEAF2_WAVE_FLOATS = 176 * 5 + 4 * (2 * 3 * 64)
# the regions' prefix sums the activate and shade-leaf kernels keep in static LDS (uint32_t[SKR_PREFIX_WORDS], 16-byte aligned)
PREFIX_LDS = (65 * 4 + 15) & ~15
# workgroup LDS of each kernel family beyond the scene table
EXTRA = {
    "direct": 4 * 192,                          # render_kernel.hip direct_lds_bytes: the scene + the tile
    "scene": 32,                                # the dynamic LDS of the node pipeline's scene kernels and of the general pipeline
    "prefix": 32 + PREFIX_LDS,                  # + the static prefix sums: the flat schedule and the general pipeline (launch.h skr_scene_kernels_lds)
    "leaf": 32 + 4 * LEAF2_WAVE_FLOATS * 4,     # the node pipeline's persistent leaf kernel: 4 waves of rings
}
LIGHTS = 1
KIB64 = 65536
GFX950_LDS = 160 * 1024  # what gfx950 reports; only stands in for the query where no device answers it (collection on a CPU host)
SKR_ERR_UNSUPPORTED = 4


def device_lds_limit():
    """hipDeviceAttributeMaxSharedMemoryPerBlock of device 0 (the value skr_renderer_create reads as sharedMemPerBlock), or None."""
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        return None
    v = C.c_int(0)
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    return v.value if hip.hipDeviceGetAttribute(C.byref(v), 74, 0) == 0 and v.value > 0 else None  # 74: hipDeviceAttributeMaxSharedMemoryPerBlock


LIMIT = device_lds_limit() or GFX950_LDS


def scene_bytes(n, lights=LIGHTS):
    return (4 * n + 1 + 2 * lights) * 16


def path_bytes(path, n, lights=LIGHTS):
    return scene_bytes(n, lights) + EXTRA[path]


def last_spheres_within(path, budget, lights=LIGHTS):
    """the largest sphere count whose table, on `path`, takes at most `budget` bytes"""
    return ((budget - EXTRA[path]) // 16 - 1 - 2 * lights) // 4


def last_lights_within(path, budget, n):
    return ((budget - EXTRA[path]) // 16 - 1 - 4 * n) // 2


def fits(path, n, lights=LIGHTS):
    return path_bytes(path, n, lights) <= LIMIT


MAX_N = last_spheres_within("prefix", LIMIT)  # the largest scene the ABI accepts at all (the general pipeline's LDS)


def boundary_counts():
    c = {71: "ids_below_256", 255: "ids_to_255", 256: "ids_to_256", 257: "ids_to_257", 258: "ids_to_258"}
    for path in ("direct", "scene", "prefix", "leaf"):
        for budget, tag in ((KIB64, "64KiB"), (LIMIT, "limit")):
            last = last_spheres_within(path, budget)
            c.setdefault(last, "%s_last_within_%s" % (path, tag))
            c.setdefault(last + 1, "%s_first_over_%s" % (path, tag))
    c[MAX_N] = "largest_accepted"
    return sorted(c.items())


COUNTS = [n for n, _ in boundary_counts()]


def bytes_id(n, lights=LIGHTS):
    return "-".join("%s%dB" % (path, path_bytes(path, n, lights)) for path in EXTRA) + "-dev%dB" % LIMIT


COUNT_IDS = ["n%d-%s-%s" % (n, why, bytes_id(n)) for n, why in boundary_counts()]


def write_scene(path, n, *, lights=LIGHTS, triangles=0, fog=False, directional=0):
    """n spheres: sphere 0 a ground sphere, spheres 1 .. n-1 on a grid that fills the view in front of it, each with its own material
    derived from its index (a wrong sphere id is a wrong colour); `lights` point lights, `directional` directional lights (kept under
    --strict-scn), a few triangles in front of the grid, one spherical_fog volume."""
    lines = ["camera 0 0 -10 0 0 1 0 1 0 30", "background .05 .1 .15", "ambient_light .25 .25 .25",
             "material .3 .3 .3 .5 .5 .5 .1 .1 .1 4 0 0 0 1", "sphere 0 -1005.6 0 1000"]
    m = n - 1
    if m > 0:
        cols = max(1, math.ceil(math.sqrt(m * 19.0 / 10.6)))
        rows = math.ceil(m / cols)
        cell = min(19.0 / cols, 10.6 / rows)
        for i in range(1, n):
            k = i - 1
            x = (k % cols - (cols - 1) / 2) * cell
            y = ((rows - 1) / 2 - k // cols) * cell
            z = (i * 37 % 11) * cell * 0.1
            c = ((i * 97) % 251 / 250.0, (i * 57 + 90) % 241 / 240.0, (i * 151 + 30) % 239 / 238.0)
            lines.append("material %.4f %.4f %.4f %.4f %.4f %.4f .2 .2 .2 %d 0 0 0 1" % (*(0.3 * v for v in c), *c, (1, 2, 7, 16, 33)[i % 5]))
            lines.append("sphere %.6g %.6g %.6g %.6g" % (x, y, z, 0.45 * cell))
    for j in range(lights):
        a = 2 * math.pi * j / max(lights, 1)
        e = 1.5 / lights
        lines.append("point_light %.6g %.6g %.6g %.6g %.6g %.6g" % (e, 0.9 * e, 0.8 * e, 8 * math.cos(a), 9 + 2 * math.sin(a), -12 + j % 5))
    for j in range(directional):
        a = 2 * math.pi * j / directional
        e = 0.8 / directional
        lines.append("directional_light %.6g %.6g %.6g %.6g %.6g %.6g" % (e, e, 0.9 * e, 0.4 * math.cos(a), -1, 0.3 + 0.4 * math.sin(a)))
    if triangles:
        lines.append("material .5 .4 .3 .6 .5 .4 .2 .2 .2 16 0 0 0 1")
        for j in range(triangles):
            x, y = -8 + 16 * j / max(triangles - 1, 1), -4.5 + 9 * (j % 2)
            lines += ["vertex %g %g -2" % (x, y), "vertex %g %g -2" % (x + 1.2, y), "vertex %g %g -2.3" % (x, y + 1.2)]
        lines += ["triangle %d %d %d" % (3 * j, 3 * j + 1, 3 * j + 2) for j in range(triangles)]
    if fog:
        lines.append("spherical_fog 0 0 0 30 .8 .7 .6 .03 .01")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)


W, H = 96, 54
SEED = 17
MODES = {  # (options, scene variant: "plain" spheres and lights | "tris" + a few triangles | "fog" + a few triangles and a fog volume)
    "direct_js2": (dict(jsample=2, shadow=True, seed=SEED), "plain"),
    "gillum4_d3": (dict(gillum=4, depth=3, shadow=True, seed=SEED), "plain"),
    "shade_triangles": (dict(gillum=2, depth=3, shadow=True, shade_triangles=True, seed=SEED), "tris"),
    "legacy_reflect_d3": (dict(depth=3, shadow=True, legacy_reflect=True), "plain"),
    "fog": (dict(gillum=2, depth=2, shadow=True, seed=SEED), "fog"),
}
SWITCHES = ("SKR_FLAT", "SKR_PIPELINE", "SKR_SHADOW_MASK", "SKR_LEVELS_BUDGET_MB")


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert device_lds_limit() == LIMIT, "the boundary counts were computed for %d bytes of LDS" % LIMIT
    return torch


@pytest.fixture(scope="module")
def ray_checker(tmp_path_factory):
    return build_ray_checker(str(tmp_path_factory.mktemp("sizes_raycheck")))


@pytest.fixture(scope="module")
def fog_checker(tmp_path_factory):
    return build_fog_checker(str(tmp_path_factory.mktemp("sizes_fogcheck")))


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """(n, variant) -> (path, Scene, Renderer), built once per module"""
    d = tmp_path_factory.mktemp("sizes")
    cache = {}

    def get(n, variant):
        if (n, variant) not in cache:
            fog = variant == "fog"
            p = write_scene(d / ("n%d_%s.scn" % (n, variant)), n, triangles=0 if variant == "plain" else 6, fog=fog)
            sc = skr.parse_scene(p, fog=fog)
            cache[(n, variant)] = (p, sc, skr.Renderer(sc))
        return cache[(n, variant)]

    yield get
    for _, _, r in cache.values():
        r.close()


def set_switches(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def render(r, opt, monkeypatch, env=None):
    set_switches(monkeypatch, env or {})
    r.counters(reset=True)
    rgb, rgbf = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    c = r.counters(reset=True)
    return rgb.cpu().numpy(), rgbf.cpu().numpy(), (c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]), r.kernel_variant()


def oracle_frame(oracle, path, kw):
    o_rgb, o_f, st = oracle.render(path, W, H, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw)
    return o_rgb, o_f, tuple(int(v) for v in st[:3])


def same_frame(a, b, what):
    assert np.array_equal(a[0], b[0]), "%s: u8 image differs" % what
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "%s: float image differs" % what
    assert a[2] == b[2], "%s: counts %s != %s" % (what, a[2], b[2])


def assert_refused(fn, what):
    with pytest.raises(skr.SkrError) as e:
        fn()
    msg = str(e.value)
    assert "LDS" in msg and "(status %d)" % SKR_ERR_UNSUPPORTED in msg, "%s: %s" % (what, msg)


def expected_variants(n, mode, lights=LIGHTS):
    """what the planner must pick for each schedule a mode is rendered under, or None where no path fits: a frame is refused only
    when nothing fits; the persistent leaf kernel gives way to the flat schedule, the direct kernel to the general pipeline"""
    if not fits("prefix", n, lights):
        return None
    if mode == "direct_js2":
        return {"": "direct_v3" if fits("direct", n, lights) else "level_pipeline_g1", "generic": "level_pipeline_g1"}
    if mode == "gillum4_d3":
        return {"": "node_levels_v5_flat", "persistent": "node_levels_v5" if fits("leaf", n, lights) else "node_levels_v5_flat",
                "flat": "node_levels_v5_flat", "generic": "level_pipeline_g1"}
    return {"": "level_pipeline_g1"}


SCHEDULES = {"": {}, "persistent": {"SKR_FLAT": "0"}, "flat": {"SKR_FLAT": "1"}, "generic": {"SKR_PIPELINE": "generic"}}


def test_boundary_counts_are_where_the_formulas_put_them():
    # each boundary pair straddles its budget; the planner's byte counts in the ids are those the kernels launch with
    for path in EXTRA:
        for budget in (KIB64, LIMIT):
            n = last_spheres_within(path, budget)
            assert path_bytes(path, n) <= budget < path_bytes(path, n + 1)
            assert n in COUNTS and n + 1 in COUNTS
    assert MAX_N + 1 in COUNTS and not fits("prefix", MAX_N + 1) and fits("prefix", MAX_N)
    assert EXTRA["leaf"] == 32 + 38656 and PREFIX_LDS == 272


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", COUNTS, ids=COUNT_IDS)
def test_frames_at_sphere_count(gpu, oracle, fog_checker, ray_checker, scenes, monkeypatch, n, mode):
    """Every family at every boundary count, bit for bit against the oracle (the fog checker for fog), counts included; the other
    schedules of the mode against the checked frame; past the limit a clean refusal."""
    kw, variant = MODES[mode]
    path, sc, r = scenes(n, variant)
    assert sc.info.n_spheres == n
    opt = skr.Options(W, H, **kw)
    want = expected_variants(n, mode)
    if want is None:
        for env in SCHEDULES.values():
            set_switches(monkeypatch, env)
            assert_refused(lambda: r.render(opt, want_float=True), "n=%d %s %s" % (n, mode, env))
        set_switches(monkeypatch, {})
        if mode == "gillum4_d3":
            rays = r.camera_rays(opt).view(-1, 8)
            assert_refused(lambda: r.shade(rays, opt), "shading query n=%d" % n)
        return
    base = render(r, opt, monkeypatch)
    assert base[3] == want[""], (n, mode, base[3])
    if mode == "fog":
        c_rgb, c_f, st = fog_checker.render(path, W, H, sc.fog, **kw)
        ref = (c_rgb, c_f, tuple(int(v) for v in st))
    else:
        ref = oracle_frame(oracle, path, kw)
    what = "n=%d %s [%s]" % (n, mode, base[3])
    compare(base[0], base[1], ref[0], ref[1], what)
    assert base[2] == ref[2], "%s: counts %s, oracle %s" % (what, base[2], ref[2])
    for name, variant_want in want.items():
        if name:
            got = render(r, opt, monkeypatch, SCHEDULES[name])
            assert got[3] == variant_want, (n, mode, name, got[3])
            same_frame(got, base, "n=%d %s %s [%s]" % (n, mode, name, got[3]))
    set_switches(monkeypatch, {})
    if mode == "gillum4_d3":
        # shading queries: the frame's camera rays keyed y * W + x are the frame itself, counts included
        rays = r.camera_rays(opt).view(-1, 8)
        keys = torch.arange(W * H, dtype=torch.int32, device=rays.device)
        r.counters(reset=True)
        out = r.shade(rays, opt, 0, keys=keys)
        torch.cuda.synchronize()
        c = r.counters(reset=True)
        assert np.array_equal(out.cpu().numpy().reshape(H, W, 3).view(np.uint32), base[1].view(np.uint32)), "shading query n=%d" % n
        assert (c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]) == base[2]
        # and the coverage the test relies on: sphere ids of 256 and above are hit, and the last ones
        hits = r.trace(rays)
        torch.cuda.synchronize()
        ids = hits.index[hits.kind.eq(1)].cpu().numpy()  # kind 1: a sphere
        s, t, _ = sc.arrays()
        h_cpu, _ = ray_checker.trace(s, t, rays.cpu().numpy())
        assert np.array_equal(hits.raw.cpu().numpy().view(np.uint32), h_cpu.view(np.uint32)), "camera-ray trace n=%d" % n
        assert len(np.unique(ids)) > min(n, 256) // 2, "n=%d: %d spheres visible" % (n, len(np.unique(ids)))
        if n > 256:
            assert (ids >= 256).any(), "n=%d: no sphere id >= 256 is hit" % n
        assert (ids >= n - 9).any(), "n=%d: none of the last spheres is hit (largest id %d)" % (n, ids.max())


def check_ray_queries(r, sc, checker, seed, what):
    s, t, _ = sc.arrays()
    rays = random_rays(sc, 4093, seed)
    want, occ = checker.trace(s, t, rays)
    d = torch.from_numpy(rays).cuda()
    got = r.trace(d)
    anyhit = r.trace(d, any_hit=True)
    torch.cuda.synchronize()
    g = got.raw.cpu().numpy()
    bad = np.nonzero((g.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d closest hits differ; first %d: gpu %s cpu %s" % (what, len(bad), len(g), bad[0], g[bad[0]], want[bad[0]])
    assert np.array_equal(anyhit.cpu().numpy(), occ), "%s: any-hit answers differ" % what
    return g


@pytest.mark.parametrize("n", COUNTS + [4000], ids=COUNT_IDS + ["n4000-past_the_limit-" + bytes_id(4000)])
def test_ray_queries_at_sphere_count(gpu, ray_checker, scenes, n):
    _, sc, r = scenes(n, "plain")
    g = check_ray_queries(r, sc, ray_checker, 1000 + n, "n=%d" % n)
    ids = g.view(np.int32)[:, 2][g.view(np.int32)[:, 1] == 1]
    assert (n <= 256 or (ids >= 256).any()) and (ids >= n - 64).any(), "n=%d: the rays miss the high sphere ids" % n


def test_past_the_limit_is_refused_and_the_renderer_keeps_working(gpu, oracle, ray_checker, scenes, monkeypatch):
    """A table that cannot fit: every frame and shading query refused with SKR_ERR_UNSUPPORTED naming LDS; the same renderer still
    answers ray queries and renders correctly afterwards; a small scene renders correctly in the same process."""
    for n in (MAX_N + 1, 4000):
        _, sc, r = scenes(n, "plain")
        for mode, (kw, variant) in MODES.items():
            if variant != "plain":
                continue  # (the same tables and the same refusal)
            opt = skr.Options(W, H, **kw)
            assert_refused(lambda: r.render(opt), "n=%d %s" % (n, mode))
            assert_refused(lambda: r.shade(r.camera_rays(opt).view(-1, 8), opt), "shading query n=%d %s" % (n, mode))
        check_ray_queries(r, sc, ray_checker, 7, "after refusals, n=%d" % n)
        # and camera rays of the same renderer, traced
        cam = r.camera_rays(skr.Options(W, H)).view(-1, 8)
        s, t, _ = sc.arrays()
        assert np.array_equal(r.trace(cam).raw.cpu().numpy().view(np.uint32), ray_checker.trace(s, t, cam.cpu().numpy())[0].view(np.uint32))
    path, _, small = scenes(71, "plain")
    kw = MODES["gillum4_d3"][0]
    got = render(small, skr.Options(W, H, **kw), monkeypatch)
    ref = oracle_frame(oracle, path, kw)
    compare(got[0], got[1], ref[0], ref[1], "71 spheres after the refusals")
    assert got[2] == ref[2]
    set_switches(monkeypatch, {})


@pytest.mark.parametrize("n,lights", [(32, 33), (32, 64), (32, 256), (40, 64)], ids=["32s33l_masks", "32s64l_masks", "32s256l_masks", "40s64l_plain_loop"])
def test_many_lights(gpu, oracle, tmp_path, monkeypatch, n, lights):
    """Shadow masks (at most 32 spheres) against the plain loop and the oracle at light counts past a 32-bit word of lights, and the
    plain loop (more than 32 spheres) at 64 lights, on the node pipeline and the general pipeline."""
    path = write_scene(tmp_path / "lights.scn", n, lights=lights)
    sc = skr.parse_scene(path)
    masks, _ = sc.shadow_masks()
    assert (len(masks) == lights) == (n <= 32), (n, lights, len(masks))
    r = skr.Renderer(sc)
    for kw in (dict(gillum=3, depth=2, shadow=True, seed=3), dict(jsample=2, shadow=True, seed=4)):
        opt = skr.Options(W, H, **kw)
        ref = oracle_frame(oracle, path, kw)
        for env in ({}, {"SKR_SHADOW_MASK": "0"}, {"SKR_PIPELINE": "generic"}, {"SKR_PIPELINE": "generic", "SKR_SHADOW_MASK": "0"}):
            got = render(r, opt, monkeypatch, env)
            what = "%d spheres %d lights %s %s [%s]" % (n, lights, kw, env, got[3])
            compare(got[0], got[1], ref[0], ref[1], what)
            assert got[2] == ref[2], what
    r.close()
    set_switches(monkeypatch, {})


def light_counts():
    n = 4
    c = {}
    for path in ("leaf", "direct", "prefix"):
        last = last_lights_within(path, LIMIT, n)
        c.setdefault(last, "%s_last_within_limit" % path)
        c.setdefault(last + 1, "%s_first_over_limit" % path)
    return n, sorted(c.items())


@pytest.mark.parametrize("lights", [l for l, _ in light_counts()[1]],
                         ids=["4s%dl-%s-%s" % (l, why, bytes_id(4, l)) for l, why in light_counts()[1]])
def test_light_counts_near_the_limit(gpu, oracle, tmp_path, monkeypatch, lights):
    """A few spheres under thousands of lights: the light rows fill the table instead of the spheres."""
    n = light_counts()[0]
    path = write_scene(tmp_path / "lights.scn", n, lights=lights)
    r = skr.Renderer(skr.parse_scene(path))
    w, h = 48, 27
    for kw, mode in ((dict(jsample=0, shadow=True), "direct_js2"), (dict(gillum=2, depth=2, shadow=True, seed=5), "gillum4_d3")):
        opt = skr.Options(w, h, **kw)
        want = expected_variants(n, mode, lights)
        if want is None:
            set_switches(monkeypatch, {})
            assert_refused(lambda: r.render(opt), "%d lights %s" % (lights, kw))
            continue
        o_rgb, o_f, st = oracle.render(path, w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw)
        for name, variant_want in want.items():
            got = render(r, opt, monkeypatch, SCHEDULES[name])
            what = "%d lights %s %s [%s]" % (lights, kw, name, got[3])
            assert got[3] == variant_want, what
            compare(got[0], got[1], o_rgb, o_f, what)
            assert got[2] == tuple(int(v) for v in st[:3]), what
    r.close()
    set_switches(monkeypatch, {})


def test_many_directional_lights_under_strict_scn(gpu, oracle, tmp_path, monkeypatch):
    """--strict-scn: 300 directional lights behind 2 point lights in the light rows (no shadow masks: a directional light turns them off)."""
    path = write_scene(tmp_path / "directional.scn", 20, lights=2, directional=300)
    sc = skr.parse_scene(path, strict=True)
    assert sc.info.n_directional_lights == 300 and len(sc.shadow_masks()[0]) == 0
    r = skr.Renderer(sc)
    for kw in (dict(jsample=2, shadow=True, seed=2), dict(gillum=3, depth=3, shadow=True, seed=6)):
        opt = skr.Options(W, H, **kw)
        o_rgb, o_f, st = oracle.render(path, W, H, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, strict=True, **kw)
        for env in ({}, {"SKR_PIPELINE": "generic"}):
            got = render(r, opt, monkeypatch, env)
            what = "strict 300 directional %s %s [%s]" % (kw, env, got[3])
            compare(got[0], got[1], o_rgb, o_f, what)
            assert got[2] == tuple(int(v) for v in st[:3]), what
    plain = skr.Renderer(skr.parse_scene(path))
    assert not np.array_equal(render(plain, skr.Options(W, H, jsample=2, shadow=True, seed=2), monkeypatch)[1], render(r, skr.Options(W, H, jsample=2, shadow=True, seed=2), monkeypatch)[1])
    plain.close()
    r.close()
    set_switches(monkeypatch, {})
