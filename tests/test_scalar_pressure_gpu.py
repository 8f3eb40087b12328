"""The node pipeline's trace kernel reads its launch constants from the kernel-argument segment where it uses them, block by block,
and the leaf kernel forms the Philox key schedule again in every round (render_nodes.hip launch_args): neither may
change a bit.  Small spheres2 frames (64x36) against the oracle (counter RNG, shared math): the bytes, the float image bit for bit and
the four work counters, on the cases where a key schedule formed per round or a constant read again at its use could go wrong —

  seeds        the key bumps wrap in the low word, in the high word, in both, in neither
  sample counts  an odd N (the last sibling pair has no second child), N = 1 (one round of one ray), N = 16 (eight rounds: more
               than the four slot windows, so they are reused)
  depths       2 (the leaf kernel's FIRST instantiation), 3 (the headline path), 4 (the trace kernel on a deeper level beside
               skr_activate_kernel)
  schedules    SKR_FLAT=0 (persistent leaf kernel) and 1 (the last level through the trace kernel too)
  switches     SKR_GI_MASK=0, SKR_GI_SURFACE=0, SKR_PRIMARY_CACHE=0: the instantiations without GI masks, and the trace kernel
               looking its lanes' rows up itself
  camera       tests/camera_poses.py s2_far: primary hits outside both GI grids — such a lane names every sphere (the re-read gi_all)
               and its wave takes the loop over every sphere
"""
import numpy as np
import pytest

import camera_poses
import skele_raytracer_amd as skr
from conftest import scene_path

pytestmark = pytest.mark.gpu

W, H = 64, 36
SWITCHES = ("SKR_FLAT", "SKR_PIPELINE", "SKR_GI_MASK", "SKR_GI_SURFACE", "SKR_PRIMARY_CACHE", "SKR_SHADOW_MASK", "SKR_LEVELS_BUDGET_MB")
SCHEDULES = [("0", "node_levels_v5"), ("1", "node_levels_v5_flat")]
_ref, _scene = {}, {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def reference(oracle, scn, kw):
    """the oracle's frame of (scene, options): rendered once, shared by every test that needs it, never written to"""
    key = (scn, tuple(sorted(kw.items())))
    if key not in _ref:
        rgb, f, st = oracle.render(scene_path(scn), W, H, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw)
        rgb.setflags(write=False)
        f.setflags(write=False)
        _ref[key] = (rgb, f.view(np.uint32), tuple(int(v) for v in st[:4]))
    return _ref[key]


def check(gpu, oracle, monkeypatch, scn, kw, env, variant):
    o_rgb, o_f, o_work = reference(oracle, scn, kw)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if scn not in _scene:
        _scene[scn] = skr.parse_scene(scene_path(scn))
    r = skr.Renderer(_scene[scn])  # (a renderer reads the switches when it is made)
    r.work(reset=True)
    rgb, rgbf = r.render(skr.Options(W, H, **kw), want_float=True)
    gpu.cuda.synchronize()
    got = r.work(reset=True)
    tag = (scn, kw, env)
    assert r.kernel_variant() == variant, (r.kernel_variant(), tag)
    assert (got["radiance_rays"], got["sphere_hits"], got["shadow_rays"], got["sphere_tests"]) == o_work, tag
    f = rgbf.cpu().numpy().view(np.uint32)
    assert np.array_equal(f, o_f), "float image differs at %d words %r" % (int((f != o_f).sum()), tag)
    assert np.array_equal(rgb.cpu().numpy(), o_rgb), tag


@pytest.mark.parametrize("flat,variant", SCHEDULES)
@pytest.mark.parametrize("seed", [0, 1, 0xFFFFFFFF, 0xFFFFFFFF00000000, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15])
def test_seeds_whose_key_bumps_wrap(gpu, oracle, monkeypatch, seed, flat, variant):
    check(gpu, oracle, monkeypatch, "spheres2.scn", dict(gillum=4, shadow=True, depth=3, seed=seed), {"SKR_FLAT": flat}, variant)


@pytest.mark.parametrize("flat,variant", SCHEDULES)
@pytest.mark.parametrize("gillum", [3, 1, 16])
def test_sample_counts(gpu, oracle, monkeypatch, gillum, flat, variant):
    check(gpu, oracle, monkeypatch, "spheres2.scn", dict(gillum=gillum, shadow=True, depth=3, seed=11), {"SKR_FLAT": flat}, variant)


@pytest.mark.parametrize("flat,variant", SCHEDULES)
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_depths(gpu, oracle, monkeypatch, depth, flat, variant):
    check(gpu, oracle, monkeypatch, "spheres2.scn", dict(gillum=4, shadow=True, depth=depth, seed=5), {"SKR_FLAT": flat}, variant)


@pytest.mark.parametrize("flat,variant", SCHEDULES)
@pytest.mark.parametrize("switch", ["SKR_GI_MASK", "SKR_GI_SURFACE", "SKR_PRIMARY_CACHE"])
def test_mask_switches_off(gpu, oracle, monkeypatch, switch, flat, variant):
    check(gpu, oracle, monkeypatch, "spheres2.scn", dict(gillum=4, shadow=True, depth=3, seed=5), {"SKR_FLAT": flat, switch: "0"}, variant)


def primary_hits_outside_grids(scn, fov):
    """how many of the W x H primary rays of scene scn hit a sphere at a point outside both GI grids (binary64, main.cpp:140-182 and
    utils.h:87-110 restated: the near root, accepted when t > 1)"""
    import math
    scene = skr.parse_scene(scene_path(scn))
    grids = scene.gi_masks()[4].astype(np.float64)  # [2] x {lo.xyz, cells per unit, n.xyz, -}
    spheres, cam = [], None
    for ln in open(scene_path(scn)):
        t = ln.split()
        if t[:1] == ["sphere"]:
            spheres.append([float(v) for v in t[1:5]])
        if t[:1] == ["camera"]:
            cam = np.array([float(v) for v in t[1:10]])
    pos, d, up = cam[0:3], cam[3:6], cam[6:9]
    right, ang = np.cross(-d, up), math.tan(math.pi * 0.5 * fov / 180.0)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    u, v = (2 * ((xs + 0.5) / W) - 1) * ang * (W / H), (1 - 2 * ((ys + 0.5) / H)) * ang
    D = d + right * u[..., None] + up * v[..., None]
    best = np.full((H, W), np.inf)
    for x, y, z, r in spheres:
        e = pos - np.array([x, y, z])
        a, b, c = (D * D).sum(-1), 2 * (D * e).sum(-1), e @ e - r * r
        disc = b * b - 4 * a * c
        with np.errstate(invalid="ignore"):
            t = (-b - np.sqrt(disc)) / (2 * a)
        best = np.where((disc >= 0) & (t > 1) & (t < best), t, best)
    hit = np.isfinite(best)
    P = pos + D * np.where(hit, best, 0.0)[..., None]
    inside = np.zeros((H, W), bool)
    for g in grids:
        inside |= ((P >= g[0:3]) & (P < g[0:3] + g[4:7] / g[3])).all(-1)
    return int((hit & ~inside).sum())


@pytest.mark.parametrize("flat,variant", SCHEDULES)
@pytest.mark.parametrize("env", [{}, {"SKR_PRIMARY_CACHE": "0", "SKR_GI_SURFACE": "0"}], ids=["stored-rows", "rows-looked-up"])
def test_camera_whose_hits_leave_the_gi_grids(gpu, oracle, monkeypatch, env, flat, variant):
    """s2_far: from 1e4 units away some primary hits lie on the ground sphere outside both grids (held here on the host, from the
    scene's own grids): with the rows looked up by the trace kernel and no surface patches their lanes name every sphere."""
    pose = camera_poses.BY_NAME["s2_far"]
    scn = camera_poses.scene_file(pose)
    assert primary_hits_outside_grids(scn, pose.kw["fov"]) > 0
    check(gpu, oracle, monkeypatch, scn, dict(pose.kw, gillum=4, shadow=True, depth=3, seed=5), dict(env, SKR_FLAT=flat), variant)
