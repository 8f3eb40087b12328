"""Every render path under the camera poses of tests/camera_poses.py (pytest -m gpu): rolled and oblique cameras, long direction and up
vectors that move a frame to another triangle culling set, cameras inside spheres and amid meshes, on surfaces, at a light, 1e4 units
away, and the degenerate ones (right = 0, direction = 0).  The kernels against the CPU oracle and its checkers, bit for bit — float
words, bytes, ray, hit and shadow-ray counts — with the kernel variant asserted, so that a case cannot drift to another path unnoticed;
the culling and mask switches change nothing; the brute-force fallback is taken at dmax >= 256 and not below; the ray and shading
queries agree with the frames; the kept level-0 stage of one pose never serves another.

What each pose reaches is held on the CPU by tests/test_camera_poses_cpu.py.  The degenerate poses (camera_poses.DEGENERATE: s2_up_parallel,
s2_zero_dir, s2_zero_up, test_up_parallel, test_zero_dir) run through the same cases; their float images are compared bit for bit with
any NaN standing for any NaN.  No pose is refused by the product: none is asserted as an error."""
import numpy as np
import pytest

import skele_raytracer_amd as skr
import camera_poses as cp
from conftest import scene_path
from fog_check import build as build_fog_checker
from ray_query_check import build as build_ray_checker
from triangle_shadow_check import build as build_shadow_checker

pytestmark = pytest.mark.gpu

SWITCHES = ("SKR_FLAT", "SKR_PIPELINE", "SKR_NO_CULL", "SKR_NO_CONES", "SKR_GI_MASK", "SKR_GI_SURFACE", "SKR_SHADOW_MASK", "SKR_LEVELS_BUDGET_MB",
            "SKR_PRIMARY_CACHE")
DIRECT_SIZE, GI_SIZE = (160, 120), (96, 72)       # degenerate poses: one row less, so that the centre row has v = 0
MESH_POSES = cp.MESH


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def ray_checker(tmp_path_factory):
    return build_ray_checker(str(tmp_path_factory.mktemp("raycheck_poses_gpu")))


@pytest.fixture(scope="module")
def fog_checker(tmp_path_factory):
    return build_fog_checker(str(tmp_path_factory.mktemp("fogcheck_poses")))


@pytest.fixture(scope="module")
def shadow_checker(tmp_path_factory):
    return build_shadow_checker(str(tmp_path_factory.mktemp("trishadowcheck_poses")))


def path_of(pose):
    return scene_path(cp.scene_file(pose))


def size_of(pose, size):
    return (size[0], size[1] - 1) if pose.family == "degenerate" else size


_renderers = {}


def renderer(pose, **flags):
    """One renderer per posed scene and loader flags, kept for the module (the dragon's tree is built once per pose)."""
    key = (pose.name, tuple(sorted(flags.items())))
    if key not in _renderers:
        sc = skr.parse_scene(path_of(pose), **flags)
        _renderers[key] = (sc, skr.Renderer(sc))
    return _renderers[key][1]


def frame(gpu, r, w, h, triangle_work=False, **kw):
    """(bytes, floats, [rays, sphere hits, shadow rays], kernel variant, triangle work or None) of one frame of r"""
    if triangle_work:
        r.triangle_work(reset=True)
    r.counters(reset=True)
    rgb, rgbf = r.render(skr.Options(w, h, **kw), want_float=True)
    gpu.cuda.synchronize()
    tw = r.triangle_work(reset=True) if triangle_work else None  # (read before the counters are reset: include/skr.h)
    c = r.counters(reset=True)
    return rgb.cpu().numpy(), rgbf.cpu().numpy(), [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]], r.kernel_variant(), tw


def same_words(a, b, nan_is_nan):
    """float arrays equal bit for bit; nan_is_nan: any NaN standing for any NaN (the degenerate poses)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    eq = a.view(np.uint32) == b.view(np.uint32)
    if nan_is_nan:
        eq |= np.isnan(a) & np.isnan(b)
    return eq


def assert_frame(got, want_rgb, want_f, want_counts, what, degenerate=False):
    eq = same_words(got[1], want_f, degenerate)
    assert eq.all(), "%s: %d float words differ, first at %s" % (what, int((~eq).sum()), np.argwhere(~eq)[:3].tolist())
    assert np.array_equal(got[0], want_rgb), "%s: %d bytes differ" % (what, int((got[0] != want_rgb).sum()))
    if want_counts is not None:
        assert got[2] == [int(x) for x in want_counts[:3]], (what, got[2], want_counts[:3])


def oracle_frame(oracle, pose, w, h, **kw):
    return oracle.render(path_of(pose), w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw)


# ------------------------------------------------------------------------------------------- every pose on every path that renders it ----
# name, switches, options, size, variant on a scene with spheres (dragon.scn has none: api.cpp folds --depth to 1 and the direct kernel
# renders the frame, unless the general pipeline is forced)
PATHS = [
    ("direct", {}, dict(), DIRECT_SIZE, "direct_v3"),
    ("direct_shadow", {}, dict(shadow=True), DIRECT_SIZE, "direct_v3"),
    ("direct_js2", {}, dict(jsample=2, seed=5), DIRECT_SIZE, "direct_v3"),
    ("direct_js2_shadow", {}, dict(jsample=2, shadow=True, seed=6), DIRECT_SIZE, "direct_v3"),
    ("nodes_flat_gi6_d3", {"SKR_PIPELINE": "nodes", "SKR_FLAT": "1"}, dict(gillum=6, depth=3, shadow=True, seed=7), GI_SIZE, "node_levels_v5_flat"),
    ("nodes_persistent_gi4_d4", {"SKR_PIPELINE": "nodes", "SKR_FLAT": "0"}, dict(gillum=4, depth=4, shadow=True, seed=8), GI_SIZE, "node_levels_v5"),
    ("generic_gi8_d2", {"SKR_PIPELINE": "generic"}, dict(gillum=8, depth=2, shadow=True, seed=9), GI_SIZE, "level_pipeline_g1"),
]


def variant_for(pose, env, variant):
    if pose.base == "dragon.scn" and env.get("SKR_PIPELINE") != "generic":
        return "direct_v3"
    return variant


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("pose", cp.POSES, ids=[p.name for p in cp.POSES])
def test_pose_matches_the_oracle(gpu, oracle, monkeypatch, pose, path):
    name, env, kw, size, variant = path
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    w, h = size_of(pose, size)
    kw = dict(pose.kw, **kw)
    got = frame(gpu, renderer(pose), w, h, **kw)
    assert got[3] == variant_for(pose, env, variant), (pose.name, name, got[3])
    o_rgb, o_f, st = oracle_frame(oracle, pose, w, h, **kw)
    assert_frame(got, o_rgb, o_f, st, "%s %s" % (pose.name, name), pose.family == "degenerate")


@pytest.mark.parametrize("tshadow", [False, True], ids=["shade_triangles", "triangle_shadows"])
@pytest.mark.parametrize("pose", MESH_POSES, ids=[p.name for p in MESH_POSES])
def test_mesh_pose_with_triangles_as_surfaces(gpu, oracle, shadow_checker, pose, tshadow):
    """--shade-triangles (a triangle hit needs t > 0 there, and recurses), without and with triangles casting shadows (the strict
    loader: dragon.scn's only light is directional)."""
    w, h = size_of(pose, (64, 48))
    kw = dict(pose.kw, shade_triangles=True, gillum=3, depth=3, shadow=True, seed=11)
    if tshadow:
        got = frame(gpu, renderer(pose, strict=True, triangle_shadows=True), w, h, **kw)
        assert got[3] == "level_pipeline_g1_tshadow"
        o_rgb, o_f, st = shadow_checker.render(path_of(pose), w, h, triangle_shadows=True, strict=True, **kw)
    else:
        got = frame(gpu, renderer(pose), w, h, **kw)
        assert got[3] == "level_pipeline_g1"
        o_rgb, o_f, st = oracle_frame(oracle, pose, w, h, **kw)
    assert_frame(got, o_rgb, o_f, st, pose.name, pose.family == "degenerate")


@pytest.mark.parametrize("kw", [dict(depth=3, shadow=True), dict(gillum=3, depth=3, shadow=True, seed=13)], ids=["d3", "gi3_d3"])
@pytest.mark.parametrize("name", ["s2_in_small", "s2_rolled"])
def test_legacy_reflect_under_a_pose(gpu, oracle, name, kw):
    pose = cp.BY_NAME[name]
    w, h = GI_SIZE
    kw = dict(kw, legacy_reflect=True)
    got = frame(gpu, renderer(pose), w, h, **kw)
    assert got[3] == "level_pipeline_g1"
    o_rgb, o_f, st = oracle_frame(oracle, pose, w, h, **kw)
    assert_frame(got, o_rgb, o_f, st, name)


@pytest.mark.parametrize("kw", [dict(depth=1, shadow=True), dict(gillum=4, depth=3, shadow=True, seed=17)], ids=["d1", "gi4_d3"])
@pytest.mark.parametrize("name", ["s2_rolled", "s2_in_ground", "s2_down", "s2_at_centre"])
def test_fog_with_the_camera_inside_the_volume(gpu, fog_checker, name, kw):
    pose = cp.BY_NAME[name]
    sc = skr.parse_scene(path_of(pose), fog=True)
    fog = sc.fog
    cam = np.array(list(sc.info.camera)[:3], np.float64)
    assert len(fog) == 1 and np.linalg.norm(cam - fog[0, :3]) < fog[0, 3], "the camera must stand inside the fog volume"
    w, h = (96, 72) if "gillum" not in kw else (64, 48)
    r = skr.Renderer(sc)
    try:
        got = frame(gpu, r, w, h, **kw)
    finally:
        r.close()
    assert got[3] == "level_pipeline_g1"
    c_rgb, c_f, st = fog_checker.render(path_of(pose), w, h, fog, **kw)
    assert_frame(got, c_rgb, c_f, st.tolist(), name + " fog")


@pytest.mark.parametrize("kw,variant", [(dict(shadow=True), "direct_v3"), (dict(gillum=4, shadow=True, seed=3), "node_levels_v5_flat")], ids=["direct", "gi4"])
def test_strict_loader_under_a_rolled_pose(gpu, oracle, kw, variant):
    pose = cp.BY_NAME["s2_rolled"]
    w, h = GI_SIZE
    got = frame(gpu, renderer(pose, strict=True), w, h, **kw)
    assert got[3] == variant
    o_rgb, o_f, st = oracle_frame(oracle, pose, w, h, strict=True, **kw)
    assert_frame(got, o_rgb, o_f, st, "strict")
    plain = frame(gpu, renderer(pose), w, h, **kw)
    assert not np.array_equal(plain[1].view(np.uint32), got[1].view(np.uint32))  # the directional lights do change the picture


# ----------------------------------------------------------------------------------------------------- the switches change nothing ----
@pytest.mark.parametrize("pose", MESH_POSES, ids=[p.name for p in MESH_POSES])
def test_culling_switches_change_nothing_under_a_mesh_pose(gpu, monkeypatch, pose):
    """SKR_NO_CULL (every triangle) and SKR_NO_CONES (general radii only): the camera frame and a --shade-triangles tree."""
    r = renderer(pose)
    for size, kw in ((DIRECT_SIZE, dict(pose.kw)), ((64, 48), dict(pose.kw, shade_triangles=True, gillum=3, depth=2, shadow=True, seed=4))):
        w, h = size_of(pose, size)
        outs = []
        for env in (None, "SKR_NO_CULL", "SKR_NO_CONES"):
            with monkeypatch.context() as m:
                if env:
                    m.setenv(env, "1")
                outs.append(frame(gpu, r, w, h, **kw))
        for other in outs[1:]:
            assert np.array_equal(other[0], outs[0][0]) and np.array_equal(other[1].view(np.uint32), outs[0][1].view(np.uint32)), (pose.name, kw)
            assert other[2] == outs[0][2] and other[3] == outs[0][3]
    frame(gpu, r, 16, 12)  # (the cached renderer re-reads its switches: back to the defaults)


MASKS = ("SKR_GI_MASK", "SKR_GI_SURFACE", "SKR_SHADOW_MASK")


@pytest.mark.parametrize("env,variant", [({"SKR_FLAT": "0"}, "node_levels_v5"), ({"SKR_FLAT": "1"}, "node_levels_v5_flat"), ({"SKR_PIPELINE": "generic"}, "level_pipeline_g1")],
                         ids=["persistent", "flat", "generic"])
@pytest.mark.parametrize("switch", MASKS)
@pytest.mark.parametrize("pose", cp.INSIDE, ids=[p.name for p in cp.INSIDE])
def test_mask_switches_change_nothing_inside_a_sphere(gpu, monkeypatch, pose, switch, env, variant):
    """The GI masks, the GI surface patches and the shadow masks cull by where a hit lies and where a ray goes; with the camera inside
    a sphere the primary hits lie where no other test puts them.  Off and on: the same frame and the same work."""
    sc = skr.parse_scene(path_of(pose))
    assert len(sc.gi_masks()[0]) > 0 and sc.shadow_masks()[0].shape[0] > 0
    outs = []
    for value in ("0", "1"):
        with monkeypatch.context() as m:
            for k, v in dict(env, **{switch: value}).items():
                m.setenv(k, v)
            r = skr.Renderer(sc)
            try:
                r.work(reset=True)
                rgb, rgbf = r.render(skr.Options(240, 136, gillum=6, depth=3, shadow=True, seed=21), want_float=True)
                gpu.cuda.synchronize()
                outs.append((rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), r.work(reset=True), r.kernel_variant()))
            finally:
                r.close()
    a, b = outs
    assert a[3] == b[3] == variant
    assert a[2] == b[2] and a[2]["radiance_rays"] > 0, (a[2], b[2])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["dragon_long4", "dragon_long32", "dragon_long256"])
def test_full_size_frame_of_each_culling_set_equals_every_triangle(gpu, monkeypatch, name):
    pose = cp.BY_NAME[name]
    r = renderer(pose)
    assert cp.cull_level(cp.dmax(list(r.scene.info.camera), 60.0, 1920, 1080)) == pose.level
    r.count_triangle_work(True)
    try:
        outs = []
        for env in (None, "SKR_NO_CULL"):
            with monkeypatch.context() as m:
                if env:
                    m.setenv(env, "1")
                got = frame(gpu, r, 1920, 1080, triangle_work=True)
                outs.append((got, got[4]))
    finally:
        r.count_triangle_work(False)
    (a, wa), (b, wb) = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2] == b[2]
    assert (a[0].reshape(-1, 3).sum(axis=1) == 0).mean() > 0.2  # the mesh covers a good part of the frame
    if pose.level == 3:
        assert wa == wb, (wa, wb)  # beyond the last bound the frame is the brute-force walk itself
    else:
        assert wa["triangle_tests"] < wb["triangle_tests"], (wa, wb)
    frame(gpu, r, 16, 12)


# ------------------------------------------------------------------------------------------------------------ the three bounds ----
def _bound_frame(gpu, oracle, monkeypatch, fov):
    """The frame of BOUND_POSE at fov against the oracle; returns its triangle work, culled and under SKR_NO_CULL."""
    pose = cp.BY_NAME[cp.BOUND_POSE]
    r = renderer(pose)
    w, h = cp.BOUND_ASPECT
    o_rgb, o_f, st = oracle_frame(oracle, pose, w, h, fov=fov)
    r.count_triangle_work(True)
    work = []
    try:
        for env in (None, "SKR_NO_CULL"):
            with monkeypatch.context() as m:
                if env:
                    m.setenv(env, "1")
                got = frame(gpu, r, w, h, triangle_work=True, fov=fov)
                assert got[3] == "direct_v3"
                assert_frame(got, o_rgb, o_f, st, "fov %r %s" % (fov, env))
                work.append(got[4])
    finally:
        r.count_triangle_work(False)
    frame(gpu, r, 16, 12)
    return work


@pytest.mark.parametrize("k", [0, 1, 2], ids=["bound4", "bound32", "bound256"])
def test_frames_either_side_of_a_bound(gpu, oracle, monkeypatch, k):
    """dmax within 1 % below and above the bound (tests/test_camera_poses_cpu.py): each frame equals the oracle, culled and not; the two
    walk different sets, so their counted work differs; and the brute-force fallback is taken from 256 on and not below."""
    (_, fov_lo, _), (_, fov_hi, _) = cp.BOUND_CASES[2 * k], cp.BOUND_CASES[2 * k + 1]
    lo, lo_all = _bound_frame(gpu, oracle, monkeypatch, fov_lo)
    hi, hi_all = _bound_frame(gpu, oracle, monkeypatch, fov_hi)
    print("bound %g: below %s (every triangle %s), above %s (every triangle %s)" % (cp.BOUNDS[k], lo, lo_all, hi, hi_all))
    assert lo["triangle_tests"] < lo_all["triangle_tests"], "the frame below the bound must cull"
    assert (lo["cull_tests"], lo["triangle_tests"]) != (hi["cull_tests"], hi["triangle_tests"])
    if k == 2:
        assert hi == hi_all, "at dmax >= 256 the frame is the brute-force walk: %s against %s" % (hi, hi_all)
    else:
        assert hi["triangle_tests"] < hi_all["triangle_tests"]


@pytest.mark.parametrize("name,fov,level", cp.WIDE_CASES, ids=[c[0] for c in cp.WIDE_CASES])
def test_widest_lenses(gpu, oracle, monkeypatch, name, fov, level):
    culled, brute = _bound_frame(gpu, oracle, monkeypatch, fov)
    assert culled == brute


# ------------------------------------------------------------------------------------------------------------------- the queries ----
def _gpu_rays(gpu, r, w, h, sample=0, **kw):
    rays = r.camera_rays(skr.Options(w, h, **kw), sample)
    gpu.cuda.synchronize()
    return rays


@pytest.mark.parametrize("pose", cp.POSES, ids=[p.name for p in cp.POSES])
def test_camera_rays_and_their_trace_match_the_checker(gpu, ray_checker, pose):
    r = renderer(pose)
    w, h = size_of(pose, GI_SIZE)
    fov = pose.kw.get("fov", 60.0)
    s, t, _ = r.scene.arrays()
    for sample, kw in ((0, dict()), (3, dict(jsample=2, seed=9))):
        rays = _gpu_rays(gpu, r, w, h, sample, fov=fov, **kw)
        want = ray_checker.camera_rays(path_of(pose), w, h, fov=fov, jsample=kw.get("jsample", 0), seed=kw.get("seed", 1), sample=sample)
        assert np.array_equal(rays.cpu().numpy().view(np.uint32), want.view(np.uint32)), (pose.name, sample)
        flat = rays.view(-1, 8)
        hits = r.trace(flat).raw.cpu().numpy()
        occ = r.trace(flat, any_hit=True).cpu().numpy()
        want_hits, want_occ = ray_checker.trace(s, t, want.reshape(-1, 8))
        eq = same_words(hits, want_hits, pose.family == "degenerate")
        assert eq.all(), "%s sample %d: %d rays differ" % (pose.name, sample, int((~eq).any(axis=1).sum()))
        assert np.array_equal(occ, want_occ) and np.array_equal(occ, (hits[:, 1].view(np.int32) != 0).astype(np.int32))


SHADE_POSES = [p for p in cp.POSES if p.family in ("long", "inside", "rolled", "interior")]


@pytest.mark.parametrize("kw", [dict(shadow=True), dict(gillum=4, depth=2, shadow=True, seed=19)], ids=["direct", "gi4_d2"])
@pytest.mark.parametrize("pose", SHADE_POSES, ids=[p.name for p in SHADE_POSES])
def test_shade_of_the_camera_rays_is_the_frame(gpu, pose, kw):
    """shade(camera_rays) picks its culling set per wave from the lanes' own d.d; on the long-vector frames that is another set than
    the frame's (tests/test_camera_poses_cpu.py).  The radiance must be the frame's, bit for bit."""
    import torch
    r = renderer(pose)
    w, h = (320, 72) if pose.name == "dragon_long256" else GI_SIZE
    opt = skr.Options(w, h, **dict(pose.kw, **kw))
    _, rgbf = r.render(opt, want_float=True)
    rays = r.camera_rays(opt).view(-1, 8)
    keys = torch.arange(w * h, dtype=torch.int32, device=rays.device)
    got = r.shade(rays, opt, 0, keys=keys)
    gpu.cuda.synchronize()
    a, b = got.cpu().numpy().reshape(h, w, 3), rgbf.cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %d words differ" % (pose.name, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


# ------------------------------------------------------------------------------------------------------- the kept primary stage ----
@pytest.mark.parametrize("flat", ["0", "1"], ids=["persistent", "flat"])
def test_kept_primary_stage_of_one_pose_never_serves_another(gpu, oracle, monkeypatch, flat):
    """Two renderers of one scene under two poses, alternating frames and seeds: each frame is the oracle's, and each renderer builds
    its level-0 stage once and replays it for every later seed."""
    monkeypatch.setenv("SKR_FLAT", flat)
    poses = [cp.BY_NAME["s2_rolled"], cp.BY_NAME["s2_in_small"]]
    rs = [skr.Renderer(skr.parse_scene(path_of(p))) for p in poses]
    w, h = 160, 90
    try:
        for k, seed in enumerate((31, 32, 33)):
            for pose, r in zip(poses, rs):
                kw = dict(gillum=4, depth=3, shadow=True, seed=seed)
                got = frame(gpu, r, w, h, **kw)
                assert got[3] == ("node_levels_v5" if flat == "0" else "node_levels_v5_flat")
                o_rgb, o_f, st = oracle_frame(oracle, pose, w, h, **kw)
                assert_frame(got, o_rgb, o_f, st, "%s seed %d" % (pose.name, seed))
                assert r.primary_cache_stats() == (1, k), (pose.name, seed, r.primary_cache_stats())
    finally:
        for r in rs:
            r.close()


def test_kept_stages_of_three_poses_visited_in_turn(gpu, oracle, monkeypatch):
    """The same options on the renderers of three poses in turn, twice round: the second visit replays that renderer's own stage and
    still gives that pose's frame."""
    monkeypatch.setenv("SKR_FLAT", "1")
    poses = [cp.BY_NAME[n] for n in ("s2_down", "s2_plus_x", "s2_at_centre")]
    kw = dict(gillum=5, depth=2, shadow=True, seed=2)
    w, h = GI_SIZE
    want = {p.name: oracle_frame(oracle, p, w, h, **kw) for p in poses}
    rs = {p.name: skr.Renderer(renderer(p).scene) for p in poses}
    try:
        for visit in range(2):
            for p in poses:
                got = frame(gpu, rs[p.name], w, h, **kw)
                assert_frame(got, *want[p.name], "%s visit %d" % (p.name, visit))
                assert rs[p.name].primary_cache_stats() == (1, visit)
    finally:
        for r in rs.values():
            r.close()
