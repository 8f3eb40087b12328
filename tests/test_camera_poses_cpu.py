"""The reach of the camera poses of tests/camera_poses.py, on the CPU: the posed scenes load as the reference's parseScene() loads them,
the long-vector and bound frames fall into the culling set they claim (api.cpp launch_params restated), the query waves of such a frame
would pick another set than the frame (wave_common.h pick_query_tree), every pose hits what it is meant to hit, the trees the posed mesh
scenes build hide no accepted (ray, triangle) pair, and the oracle in the GPU's mode (counter RNG, shared math) meets the bound
tests/test_gpu_parity.py::test_gpu_matches_reference_output_where_no_rng_is_involved asserts against every new golden."""
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
import camera_poses as cp
import test_abi
import test_culling_host as tch
import test_oracle_golden
from conftest import args_to_kwargs, manifest, read_golden_ppm, scene_path
from ray_query_check import build as build_checker

f32 = np.float32
POSE_SCENES = [cp.scene_file(p) for p in cp.POSES]
QUERY_SIZE = (96, 72)  # the frames tests/test_camera_poses_gpu.py hands to shade(camera_rays)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("raycheck_poses")))


def test_catalogue_is_what_the_golden_folder_holds():
    """tests/golden/scenes/pose_*.scn (written by build()) are the catalogue's scenes, byte for byte, and nothing else; every pose has its dump and every
    golden case of the catalogue its reference PPM (a degenerate pose only if the reference agreed with itself: README.md)."""
    have = sorted(f for f in os.listdir(cp.SCENES) if f.startswith("pose_"))
    assert have == sorted(POSE_SCENES)
    for p in cp.POSES:
        with open(os.path.join(cp.SCENES, p.base)) as f:
            assert open(scene_path(cp.scene_file(p))).read() == cp.posed_text(f.read(), p.camera), p.name
    m = manifest()
    assert all(s in m["scene_dumps"] for s in POSE_SCENES)
    for name, scn, args in cp.golden_cases():
        if name in m["cases"]:
            assert (m["cases"][name]["scene"], m["cases"][name]["args"]) == (scn, args)
        else:
            assert name in cp.DEGENERATE_GOLDENS, "%s has no golden" % name
    assert len(cp.REGULAR) + len(cp.DEGENERATE) == len(cp.POSES) and len({p.name for p in cp.POSES}) == len(cp.POSES)


@pytest.mark.parametrize("scn", POSE_SCENES)
def test_loaders_match_the_parseScene_dump_of_every_posed_scene(oracle, scn):
    """tests/test_abi.py and tests/test_oracle_golden.py's loader checks on the new list — every word of the scene, the camera's
    position, direction, up and right = cross(-direction, up) among them — and the half-angle, which the dump does not hold, against the
    file's own token."""
    test_abi.test_loader_matches_reference_parseScene_dump(scn)
    test_oracle_golden.test_oracle_loader_matches_parseScene_dump(oracle, scn)
    test_abi.test_loader_matches_oracle_loader(oracle, scn)
    pose = cp.BY_NAME[scn[len("pose_"):-len(".scn")]]
    words = pose.camera.split()[1:]
    info = skr.parse_scene(scene_path(scn)).info
    osc = oracle.OracleScene(scene_path(scn))
    assert f32(info.camera[12]) == f32(float(words[9])) == f32(osc.s.cam_half_angle)
    want = np.array([float(t) for t in words[:9]], f32)
    assert np.array_equal(np.array(list(info.camera)[:9], f32).view(np.uint32), want.view(np.uint32))
    # right, restated: glm::cross(-direction, up) in binary32
    d, u = -want[3:6], want[6:9]
    right = np.array([d[1] * u[2] - u[1] * d[2], d[2] * u[0] - u[2] * d[0], d[0] * u[1] - u[0] * d[1]], f32)
    got = np.array(list(info.camera)[9:12], f32)
    assert np.array_equal(got.view(np.uint32), right.view(np.uint32)), (got, right)


def _camera(pose):
    return list(skr.parse_scene(scene_path(cp.scene_file(pose))).info.camera)


@pytest.mark.parametrize("pose", cp.LONG, ids=[p.name for p in cp.LONG])
def test_long_vector_poses_fall_into_the_culling_set_they_claim(pose):
    cam = _camera(pose)
    for w, h in (cp.GOLDEN_SIZE, QUERY_SIZE, (1920, 1080)):
        d = cp.dmax(cam, pose.kw.get("fov", 60.0), w, h)
        assert cp.cull_level(d) == pose.level, (pose.name, w, h, d)
    lo = 0.0 if pose.level == 0 else cp.BOUNDS[pose.level - 1]
    hi = np.inf if pose.level == 3 else cp.BOUNDS[pose.level]
    assert lo <= cp.dmax(cam, pose.kw.get("fov", 60.0), *cp.GOLDEN_SIZE) < hi


def test_every_culling_set_and_the_fallback_has_a_long_vector_mesh_pose():
    assert sorted(p.level for p in cp.LONG if p.base == "dragon.scn") == [1, 2, 3]
    assert all(cp.cull_level(cp.dmax(_camera(p), p.kw.get("fov", 60.0), *cp.GOLDEN_SIZE)) == 0 for p in cp.INTERIOR)


def test_bound_frames_sit_within_one_percent_of_their_bounds():
    cam = _camera(cp.BY_NAME[cp.BOUND_POSE])
    for k, (name, fov, level) in enumerate(cp.BOUND_CASES):
        bound = cp.BOUNDS[k // 2]
        d = cp.dmax(cam, fov, *cp.BOUND_ASPECT)
        assert cp.cull_level(d) == level == k // 2 + k % 2, (name, d)
        assert (d >= bound) == bool(k % 2), (name, d)
        assert 0 < abs(d / bound - 1) < 0.01, (name, d)
    for name, fov, level in cp.WIDE_CASES:
        assert cp.cull_level(cp.dmax(cam, fov, *cp.BOUND_ASPECT)) == level == 3
    # fov 181: the tangent is negative, the bound takes its magnitude
    assert cp.dmax(cam, 181.0, *cp.BOUND_ASPECT) == pytest.approx(cp.dmax(cam, 179.0, *cp.BOUND_ASPECT), rel=1e-5)


def _primary_directions(oracle, pose, w, h, fov):
    sc = oracle.OracleScene(scene_path(cp.scene_file(pose)))
    return np.array([[oracle.primary_direction(sc, w, h, fov, x, y, False) for x in range(w)] for y in range(h)], f32)


@pytest.mark.parametrize("name", ["dragon_long32", "dragon_long256"])
def test_query_waves_of_a_long_vector_frame_pick_a_tighter_set_than_the_frame(oracle, name):
    """shade(camera_rays) walks, per 64-ray wave, the set its own lanes' d.d allow.  On these frames that differs from the frame's
    set, so the GPU test's `shade(camera_rays) == frame` compares two different walks."""
    pose = cp.BY_NAME[name]
    w, h = QUERY_SIZE if name == "dragon_long32" else (320, 72)
    d = _primary_directions(oracle, pose, w, h, pose.kw.get("fov", 60.0)).reshape(-1, 3)
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]  # dot3, binary32
    frame = cp.cull_level(cp.dmax(_camera(pose), pose.kw.get("fov", 60.0), w, h))
    assert frame == pose.level >= 2
    waves = cp.query_levels(dd)
    assert (waves < frame).any(), "no wave of %s would walk a lower set than the frame's %d" % (name, frame)
    assert (waves <= frame).all()


def _hit_share(oracle, pose, w, h):
    path = scene_path(cp.scene_file(pose))
    _, f, st = oracle.render(path, w, h, depth=1, want_float=True, **pose.kw)
    bg = np.array(list(skr.parse_scene(path).info.background), f32)
    return float((f.view(np.uint32) != bg.view(np.uint32)).any(axis=-1).mean()), int(st[1])


@pytest.mark.parametrize("pose", cp.REGULAR, ids=[p.name for p in cp.REGULAR])
def test_at_least_a_fifth_of_the_primary_rays_hit_geometry(oracle, pose):
    """From the oracle's frame: a pixel that is not the background's bits hit a sphere or a triangle (a condition on the pose)."""
    share, _ = _hit_share(oracle, pose, *cp.GOLDEN_SIZE)
    assert share >= 0.2, "%s: %.3f of the primary rays hit geometry" % (pose.name, share)


@pytest.mark.parametrize("name,fov,level", cp.BOUND_CASES + cp.WIDE_CASES, ids=[c[0] for c in cp.BOUND_CASES + cp.WIDE_CASES])
def test_bound_frames_hit_geometry_too(oracle, name, fov, level):
    pose = cp.BY_NAME[cp.BOUND_POSE]._replace(kw=dict(fov=fov))
    share, _ = _hit_share(oracle, pose, *cp.BOUND_ASPECT)
    assert share >= 0.2, "%s: %.3f" % (name, share)


@pytest.mark.parametrize("pose", cp.INSIDE, ids=[p.name for p in cp.INSIDE])
def test_inside_poses_put_the_camera_inside_their_sphere(oracle, checker, pose):
    """The camera row of the containing sphere has c = e.e - r^2 < 0 in binary32 (e = 0 at the centre), every primary line crosses that
    sphere (D > 0) — and utils.h:87-110 takes the near root alone, which is negative from within: the reference never hits a sphere
    from inside, so the frame shows the other spheres through it and not one hit lies on the containing sphere.  (Inner-surface hits
    do not exist in this renderer; what the pose reaches is the rejection of a sphere whose c is negative, on every ray.)"""
    path = scene_path(cp.scene_file(pose))
    sc = skr.parse_scene(path)
    s, t, _ = sc.arrays()
    cam = np.array(list(sc.info.camera)[:3], f32)
    C, r = s[pose.sphere, :3], s[pose.sphere, 3]
    e = cam - C
    c = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) - r * r
    assert c < 0 and np.linalg.norm(e.astype(np.float64)) < float(r)
    if pose.name == "s2_at_centre":
        assert not e.any()
    w, h = cp.GOLDEN_SIZE
    rays = checker.camera_rays(path, w, h, fov=pose.kw.get("fov", 60.0)).reshape(-1, 8)
    assert np.array_equal(rays[:, :3].view(np.uint32), np.broadcast_to(cam, (w * h, 3)).view(np.uint32))
    d = rays[:, 4:7].astype(np.float64)
    b = 2 * (d @ e.astype(np.float64))
    D = b * b - 4 * (d * d).sum(1) * float(c)
    assert (D > 0).all()
    hits, _ = checker.trace(s, t, rays)
    kind, index = hits[:, 1].view(np.int32), hits[:, 2].view(np.int32)
    on_sphere = kind == 1
    assert on_sphere.mean() >= 0.2 and not (index[on_sphere] == pose.sphere).any()
    _, n_hits = _hit_share(oracle, pose, w, h)
    assert n_hits == int(on_sphere.sum())  # the checker's primary sphere hits are the oracle's count


def test_surface_poses_stand_where_they_claim():
    """On a sphere's surface (c within a few ulps of r^2 of zero), 5e-4 from a sphere and from the wall, on the wall's plane, at a
    point light, 1e4 units away."""
    def load(name):
        sc = skr.parse_scene(scene_path(cp.scene_file(cp.BY_NAME[name])))
        s, t, l = sc.arrays()
        return np.array(list(sc.info.camera)[:3], f32), s, t, l
    cam, s, _, _ = load("s2_on_surface")
    e = cam - s[2, :3]
    c = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) - s[2, 3] * s[2, 3]
    assert abs(float(c)) <= 8 * np.spacing(s[2, 3] * s[2, 3]) and e.all()
    cam, s, _, _ = load("s2_near")
    gap = np.linalg.norm((cam - s[1, :3]).astype(np.float64)) - float(s[1, 3])
    assert 0 < gap < 1e-3
    cam, _, t, _ = load("test_near")
    assert np.all(t[:, 2::3] == 10) and 0 < 10 - float(cam[2]) < 1e-3
    cam, _, t, _ = load("test_on_plane")
    assert cam[2] == 10
    cam, _, _, l = load("s2_at_light")
    assert np.array_equal(cam, l[0, :3])
    for name in ("s2_far", "test_far"):
        cam, s, _, _ = load(name)
        assert np.linalg.norm(cam.astype(np.float64)) >= 1e4
        e = cam - s[0, :3]
        ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        assert np.spacing(ee) > 1  # e.e - r^2 loses the radius's low bits: one ulp of e.e is several units


def _accepted_pairs(cam, d, tris, block=64):
    """(ray, triangle, t) of every pair utils.h:181-213 accepts, in numpy binary32 (tests/test_culling_host.py triangle_accepts), for
    rays cam + t d against device triangles [n, 3, 4]."""
    v0, e1, e2 = tris[:, 0, :3], tris[:, 1, :3], tris[:, 2, :3]
    nt = len(tris)
    out = []
    for k in range(0, len(d), block):
        dd = np.broadcast_to(d[k:k + block, None, :], (len(d[k:k + block]), nt, 3))
        o = np.broadcast_to(cam, dd.shape)
        V0, E1, E2 = (np.broadcast_to(a, dd.shape) for a in (v0, e1, e2))
        acc = tch.triangle_accepts(o, dd, V0, E1, E2)
        with np.errstate(all="ignore"):
            q = tch._cross(o - V0, E1)
            t = tch._dot(E2, q) * (f32(1.0) / tch._dot(E1, tch._cross(dd, E2)))
        ray, tri = np.nonzero(acc)
        out.append((ray + k, tri, t[ray, tri]))
    return tuple(np.concatenate(c) for c in zip(*out))


def _hidden(o, d, chunk, ch, sph, parent, node_of_chunk):
    hidden = tch.sphere_culls(o, d, ch[chunk])
    node = node_of_chunk[chunk]
    while np.any(node >= 0):
        live = node >= 0
        hidden[live] |= tch.sphere_culls(o[live], d[live], sph[node[live]])
        node = np.where(live, parent[np.maximum(node, 0)], -1)
    return hidden


@pytest.mark.parametrize("pose", cp.INTERIOR, ids=[p.name for p in cp.INTERIOR])
def test_interior_poses_have_accepting_triangles_behind_the_camera(oracle, pose):
    sc = skr.parse_scene(scene_path(cp.scene_file(pose)))
    cam = np.array(list(sc.info.camera)[:3], f32)
    d = _primary_directions(oracle, pose, 48, 36, pose.kw.get("fov", 60.0)).reshape(-1, 3)
    _, _, t = _accepted_pairs(cam, d, sc.culling(0)[1])
    assert len(t) > 1000 and (t < 0).mean() >= 0.2, "%s: %d accepted pairs, %.3f of them at t < 0" % (pose.name, len(t), (t < 0).mean())


MESH_REGULAR = [p for p in cp.MESH if p.family != "degenerate"]


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("pose", MESH_REGULAR, ids=[p.name for p in MESH_REGULAR])
def test_posed_mesh_trees_hide_no_accepted_pair(oracle, pose, level):
    """tests/test_culling_host.py's check on the trees the posed scenes build (the camera position is part of the slack): rays from the
    posed camera and from the spheres to the borders of the accept regions, as long as the set allows — and the pose's own primary rays,
    the ones behind the camera included, at every set whose bound covers them."""
    sc = skr.parse_scene(scene_path(cp.scene_file(pose)))
    cs, tris, sph, links, ch = sc.culling(level)
    parent, node_of_chunk = tch.tree_parents(links)
    n = 60000
    k, o, d = tch._border_rays(np.random.default_rng(31 + level), sc, tris, n, level)
    t = tris[k]
    acc = tch.triangle_accepts(o, d, t[:, 0, :3], t[:, 1, :3], t[:, 2, :3])
    assert acc.sum() > 0.05 * n
    hidden = acc & _hidden(o, d, k // cs, ch, sph, parent, node_of_chunk)
    assert not hidden.any(), "%s level %d: %d accepted border pairs would have been culled" % (pose.name, level, hidden.sum())
    w, h = 48, 36
    fov = pose.kw.get("fov", 60.0)
    if cp.cull_level(cp.dmax(list(sc.info.camera), fov, w, h)) > level:
        return  # the frame's rays are longer than this set allows: launch_params never pairs them
    cam = np.array(list(sc.info.camera)[:3], f32)
    dirs = _primary_directions(oracle, pose, w, h, fov).reshape(-1, 3)
    ray, tri, _ = _accepted_pairs(cam, dirs, tris)
    assert len(ray) > 100
    o = np.broadcast_to(cam, (len(ray), 3))
    hidden = _hidden(o, dirs[ray], tri // cs, ch, sph, parent, node_of_chunk)
    assert not hidden.any(), "%s level %d: %d accepted primary pairs would have been culled" % (pose.name, level, hidden.sum())


POSE_GOLDENS = [(n, c) for n, c in sorted(manifest()["cases"].items()) if n.startswith("pose_")]


@pytest.mark.parametrize("name,case", POSE_GOLDENS, ids=[c[0] for c in POSE_GOLDENS])
def test_shared_math_oracle_meets_the_gpu_golden_bound(oracle, name, case):
    """The GPU golden test asserts max <= 1/255 and fewer than 1e-4 of the bytes differing (spec powf against libm).  The GPU equals
    the counter-RNG / shared-math oracle bit for bit, so that oracle must meet the same bound against every new golden, here."""
    kw = args_to_kwargs(case["args"])
    w, h = kw.pop("width"), kw.pop("height")
    gold = read_golden_ppm(case["file"]).astype(np.int32)
    rgb, _, _ = oracle.render(scene_path(case["scene"]), w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, **kw)
    d = np.abs(rgb.astype(np.int32) - gold)
    print("%s: max %d, share %.2e" % (name, d.max(), (d > 0).mean()))
    assert d.max() <= 1
    assert (d > 0).mean() < 1e-4


def test_degenerate_poses_are_enumerated():
    """The degenerate list, in full: none is left out silently, and each really degenerates (right = 0)."""
    assert [p.name for p in cp.DEGENERATE] == ["s2_up_parallel", "s2_zero_dir", "s2_zero_up", "test_up_parallel", "test_zero_dir"]
    for p in cp.DEGENERATE:
        cam = np.array(_camera(p), f32)
        assert not cam[9:12].any(), p.name
