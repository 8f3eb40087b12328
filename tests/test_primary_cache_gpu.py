"""Frames of one camera share the node pipeline's level-0 stage (DESIGN.md 5.2 "level-0 cache"): a renderer keeps the primary hits, the
pixels of the rays that hit no sphere and the primary kernel's counted work from one frame, and the next frame under the same key starts
behind them.  Whatever a renderer did before, every frame must be the frame a FRESH renderer with SKR_PRIMARY_CACHE=0 makes of the same
options — bytes, float bits, every work counter, the level-0 and level-1 counts — and primary_cache_stats() must show which path it took:
a replay only where nothing the stage depends on has changed, a build everywhere else."""
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path

pytestmark = pytest.mark.gpu

SWITCHES = ("SKR_FLAT", "SKR_PIPELINE", "SKR_GI_MASK", "SKR_GI_SURFACE", "SKR_LEVELS_BUDGET_MB", "SKR_PRIMARY_CACHE", "SKR_ADAPTIVE_PATH")
W, H = 320, 180
BASE = dict(gillum=6, depth=3, shadow=True, seed=11)


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
def spheres2():
    return skr.parse_scene(scene_path("spheres2.scn"))


def opts(w=W, h=H, **kw):
    return skr.Options(w, h, **dict(BASE, **kw))


def observe(gpu, r, render):
    """What one frame of r leaves: (bytes, float bits, work counters, level-0 nodes, level-1 records, kernel variant)."""
    r.work(reset=True)
    rgb, rgbf = render(r)
    gpu.cuda.synchronize()
    return rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), r.work(reset=True), r.last_parent_count(), r.last_level1_count(), r.kernel_variant()


def frame_of(opt, **kw):
    return lambda r: r.render(opt, want_float=True, **kw)


def fresh(gpu, monkeypatch, scene, render, prepare=None):
    """The same frame from a new renderer that replays nothing."""
    with monkeypatch.context() as m:
        m.setenv("SKR_PRIMARY_CACHE", "0")
        r = skr.Renderer(scene)
        if prepare:
            prepare(r)
        got = observe(gpu, r, render)
        assert r.primary_cache_stats() == (0, 0)
        r.close()
    return got


def assert_same(got, want, what=""):
    assert got[5] == want[5], (what, got[5], want[5])
    assert np.array_equal(got[0], want[0]), "%s: bytes differ at %d pixels" % (what, int((got[0] != want[0]).any(-1).sum()))
    assert np.array_equal(got[1], want[1]), "%s: float image differs at %d values" % (what, int((got[1] != want[1]).sum()))
    assert got[2] == want[2], (what, got[2], want[2])
    assert got[3:5] == want[3:5], (what, got[3:5], want[3:5])
    assert want[2]["radiance_rays"] > 0


def check(gpu, monkeypatch, scene, r, render, stats, what=""):
    """r renders the frame; it is the fresh renderer's, and r's statistics are now `stats`."""
    got = observe(gpu, r, render)
    assert r.primary_cache_stats() == stats, (what, r.primary_cache_stats(), stats)
    assert_same(got, fresh(gpu, monkeypatch, scene, render), what)
    return got


@pytest.mark.parametrize("env,kw,variant", [
    ({"SKR_FLAT": "0"}, {}, "node_levels_v5"),
    ({"SKR_FLAT": "1"}, {}, "node_levels_v5_flat"),
    ({"SKR_FLAT": "0"}, {"depth": 2}, "node_levels_v5"),        # skr_leaf_kernel2<FIRST> on the kept rows
    ({"SKR_FLAT": "1"}, {"depth": 2}, "node_levels_v5_flat"),
    ({"SKR_FLAT": "0"}, {"depth": 4, "gillum": 4}, "node_levels_v5"),
    ({}, {"shadow": False}, "node_levels_v5_flat"),
])
def test_three_seeds_build_once_and_replay_twice(gpu, monkeypatch, spheres2, env, kw, variant):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = skr.Renderer(spheres2)
    for k in range(3):
        got = check(gpu, monkeypatch, spheres2, r, frame_of(opts(**dict(kw, seed=40 + k))), (1, k), "seed %d" % (40 + k))
        assert got[5] == variant
    # the bytes alone, the floats alone: the replay emits into whatever the frame names
    o = opts(**dict(kw, seed=43))
    want = fresh(gpu, monkeypatch, spheres2, frame_of(o))
    rgb, none = r.render(o)
    gpu.cuda.synchronize()
    assert none is None and np.array_equal(rgb.cpu().numpy(), want[0])
    assert r.primary_cache_stats() == (1, 3)


def test_replayed_frames_match_the_oracle(gpu, oracle, monkeypatch, spheres2):
    w, h = 160, 90
    r = skr.Renderer(spheres2)
    for k, seed in enumerate((7, 8)):
        kw = dict(gillum=4, shadow=True, seed=seed)
        r.work(reset=True)
        rgb, rgbf = r.render(skr.Options(w, h, **kw), want_float=True)
        gpu.cuda.synchronize()
        o_rgb, o_f, st = oracle.render(scene_path("spheres2.scn"), w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw)
        assert np.array_equal(rgbf.cpu().numpy().view(np.uint32), o_f.view(np.uint32))
        assert np.abs(rgb.cpu().numpy().astype(np.int32) - o_rgb.astype(np.int32)).max() <= 1
        assert r.counters()["radiance_rays"] == int(st[0])
        assert r.primary_cache_stats() == (1, k)


CHANGES = {
    "width": (frame_of(opts()), frame_of(opts(w=W + 16))),
    "height": (frame_of(opts()), frame_of(opts(h=H + 8))),
    "fov": (frame_of(opts()), frame_of(opts(fov=75.0))),
    "shadow": (frame_of(opts()), frame_of(opts(shadow=False))),
    "gillum": (frame_of(opts()), frame_of(opts(gillum=5))),
    "depth": (frame_of(opts()), frame_of(opts(depth=4))),
    "first_tile": (frame_of(opts(), tile_rows=4, first_tile=0, tile_stride=2), frame_of(opts(), tile_rows=4, first_tile=1, tile_stride=2)),
    "tile_stride": (frame_of(opts(), tile_rows=4, first_tile=0, tile_stride=2), frame_of(opts(), tile_rows=4, first_tile=0, tile_stride=3)),
    "tile_rows": (frame_of(opts(), tile_rows=4), frame_of(opts(), tile_rows=12)),
}


@pytest.mark.parametrize("what", sorted(CHANGES))
def test_a_changed_option_builds_again(gpu, monkeypatch, spheres2, what):
    a, b = CHANGES[what]
    r = skr.Renderer(spheres2)
    check(gpu, monkeypatch, spheres2, r, a, (1, 0), "first")
    check(gpu, monkeypatch, spheres2, r, a, (1, 1), "again")
    check(gpu, monkeypatch, spheres2, r, b, (2, 1), "changed " + what)
    check(gpu, monkeypatch, spheres2, r, b, (2, 2), "changed, again")
    check(gpu, monkeypatch, spheres2, r, a, (3, 2), "back")


def test_switching_the_schedule_builds_again(gpu, monkeypatch, spheres2):
    """SKR_FLAT through reload_switches: the flat schedule cuts the scratch differently."""
    r = skr.Renderer(spheres2)
    monkeypatch.setenv("SKR_FLAT", "0")
    check(gpu, monkeypatch, spheres2, r, frame_of(opts()), (1, 0))
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=12)), (1, 1))
    monkeypatch.setenv("SKR_FLAT", "1")
    got = check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=13)), (2, 1))
    assert got[5] == "node_levels_v5_flat"
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=14)), (2, 2))


def test_a_callers_tile_table_never_replays(gpu, monkeypatch, spheres2):
    """skr_render_tile_list with caller memory: the same pointer may hold other tiles."""
    o, tile_rows = opts(), 4
    dev = gpu.device("cuda", 0)
    table = gpu.tensor([0, 5, 9, 0xFFFFFFFF, 30], dtype=gpu.int64, device=dev).to(gpu.uint32)
    n = int(table.numel())

    def listed(r):
        rgb = gpu.zeros((n * tile_rows, o.width, 3), dtype=gpu.uint8, device=dev)
        rgbf = gpu.zeros((n * tile_rows, o.width, 3), dtype=gpu.float32, device=dev)
        r.render_tile_list_into(o, tile_rows, table.data_ptr(), n, rgb.data_ptr(), rgbf.data_ptr(), gpu.cuda.current_stream(dev).cuda_stream)
        return rgb, rgbf

    r = skr.Renderer(spheres2)
    a = observe(gpu, r, listed)
    assert_same(a, fresh(gpu, monkeypatch, spheres2, listed), "first contents")
    table.copy_(gpu.tensor([2, 3, 0xFFFFFFFF, 17, 44], dtype=gpu.int64, device=dev).to(gpu.uint32))
    gpu.cuda.synchronize()
    b = observe(gpu, r, listed)
    assert_same(b, fresh(gpu, monkeypatch, spheres2, listed), "rewritten contents")
    assert not np.array_equal(a[0], b[0])
    assert r.primary_cache_stats()[1] == 0


def test_other_users_of_the_scratch_forget_the_stage(gpu, monkeypatch, spheres2):
    r = skr.Renderer(spheres2)
    node = lambda seed: frame_of(opts(seed=seed))
    check(gpu, monkeypatch, spheres2, r, node(1), (1, 0))
    check(gpu, monkeypatch, spheres2, r, node(2), (1, 1))
    # the general level pipeline
    got = check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=3, legacy_reflect=True)), (1, 1), "legacy-reflect")
    assert got[5] == "level_pipeline_g1"
    check(gpu, monkeypatch, spheres2, r, node(4), (2, 1), "behind the general pipeline")
    check(gpu, monkeypatch, spheres2, r, node(5), (2, 2))
    # a shading query
    o = opts(seed=6)
    rays = r.camera_rays(o).view(-1, 8)
    r.shade(rays[:4096].contiguous(), o)
    gpu.cuda.synchronize()
    check(gpu, monkeypatch, spheres2, r, node(6), (3, 2), "behind shade()")
    check(gpu, monkeypatch, spheres2, r, node(7), (3, 3))
    # a larger frame grows the scratch; then the first size again
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(w=2 * W, h=2 * H, seed=8)), (4, 3), "larger")
    check(gpu, monkeypatch, spheres2, r, node(9), (5, 3), "the first size again")
    check(gpu, monkeypatch, spheres2, r, node(10), (5, 4))


def test_adaptive_rounds_between_frames(gpu, monkeypatch, spheres2):
    """The query path of the adaptive sampler takes the scratch for its shading queries: the frame behind it builds."""
    r = skr.Renderer(spheres2)
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=21)), (1, 0))
    monkeypatch.setenv("SKR_ADAPTIVE_PATH", "query")
    r.render_adaptive(opts(seed=30), threshold=0.0, min_passes=2, max_passes=4)
    gpu.cuda.synchronize()
    monkeypatch.delenv("SKR_ADAPTIVE_PATH")
    builds, replays = r.primary_cache_stats()
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=22)), (builds + 1, replays), "behind the query rounds")
    # whole-frame rounds are frames like any other
    monkeypatch.setenv("SKR_ADAPTIVE_PATH", "frame")
    r.render_adaptive(opts(seed=30), threshold=0.0, min_passes=2, max_passes=4)
    gpu.cuda.synchronize()
    monkeypatch.delenv("SKR_ADAPTIVE_PATH")
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=23)), (builds + 1, replays + 5), "behind the frame rounds")


def test_a_renderer_and_its_clone_alternate(gpu, monkeypatch, spheres2):
    """The pipelined frame step's pattern: each has its own scratch, hence its own stage; they share the work counters."""
    r = skr.Renderer(spheres2)
    c = r.clone()
    for k in range(6):
        who = (r, c)[k & 1]
        got = observe(gpu, who, frame_of(opts(seed=60 + k)))
        assert_same(got, fresh(gpu, monkeypatch, spheres2, frame_of(opts(seed=60 + k))), "frame %d" % k)
        assert who.primary_cache_stats() == (1, k // 2)
    c.close()
    r.close()


@pytest.mark.parametrize("case", ["jsample", "bands", "triangle_work"])
def test_where_it_does_not_apply_nothing_is_kept(gpu, monkeypatch, spheres2, case):
    scene, kw, prepare = spheres2, {}, None
    if case == "jsample":
        kw = dict(jsample=2)
    elif case == "bands":
        monkeypatch.setenv("SKR_LEVELS_BUDGET_MB", "8")
    else:
        scene = skr.parse_scene(scene_path("spheres1.scn"))
        monkeypatch.setenv("SKR_PIPELINE", "nodes")
        prepare = lambda x: x.count_triangle_work(True)
    r = skr.Renderer(scene)
    if prepare:
        prepare(r)
    for k in range(3):
        render = frame_of(opts(**dict(kw, seed=70 + k)))
        got = observe(gpu, r, render)
        assert got[5].startswith("node_levels_v5")
        assert r.primary_cache_stats() == (0, 0)
        assert_same(got, fresh(gpu, monkeypatch, scene, render, prepare), "%s frame %d" % (case, k))


def test_progressive_and_adaptive_passes_replay(gpu, monkeypatch, spheres2):
    o = opts(seed=80, progressive=4)
    r = skr.Renderer(spheres2)
    got = check(gpu, monkeypatch, spheres2, r, frame_of(o), (1, 3), "progressive 4")
    r2 = skr.Renderer(spheres2)
    rgb, rgbf, passes = r2.render_adaptive(opts(seed=80), min_passes=4, max_passes=4, want_float=True)
    gpu.cuda.synchronize()
    assert r2.primary_cache_stats() == (1, 3)
    assert int(passes.cpu().numpy().view(np.uint32).min()) == 4 == int(passes.cpu().numpy().view(np.uint32).max())
    assert np.array_equal(rgb.cpu().numpy(), got[0]) and np.array_equal(rgbf.cpu().numpy().view(np.uint32), got[1])


def triangle_frames(gpu, oracle, monkeypatch, path):
    monkeypatch.setenv("SKR_PIPELINE", "nodes")
    scene = skr.parse_scene(path)
    w, h = 200, 120
    r = skr.Renderer(scene)
    for k in range(3):
        kw = dict(gillum=4, depth=3, shadow=True, seed=90 + k)
        got = check(gpu, monkeypatch, scene, r, frame_of(skr.Options(w, h, **kw)), (1, k), "seed %d" % (90 + k))
        assert got[5].startswith("node_levels_v5")
        o_rgb, o_f, st = oracle.render(path, w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw)
        assert np.array_equal(got[1], o_f.view(np.uint32).reshape(got[1].shape))
        assert got[2]["radiance_rays"] == int(st[0])
    return got


def test_a_scene_with_triangles_on_the_node_pipeline(gpu, oracle, monkeypatch):
    """spheres1.scn has two triangles (degenerate ones: no ray ends on them, but every kernel takes its triangle instance)."""
    triangle_frames(gpu, oracle, monkeypatch, scene_path("spheres1.scn"))


def test_pixels_a_triangle_took(gpu, oracle, monkeypatch, tmp_path):
    """spheres1.scn with a triangle in front of the camera: its pixels are black, final, no node and not the background."""
    lines = [ln for ln in open(scene_path("spheres1.scn")).read().split("\n") if not ln.startswith(("vertex", "triangle"))]
    lines += ["vertex -3.5 1.2 -1.2", "vertex -2.3 1.2 -1.9", "vertex -2.9 3.0 -1.5", "triangle 0 1 2", "triangle 0 2 1"]
    path = os.path.join(str(tmp_path), "tri.scn")
    open(path, "w").write("\n".join(lines) + "\n")
    got = triangle_frames(gpu, oracle, monkeypatch, path)
    assert (got[1] == 0).all(-1).any(), "no primary ray ends on the triangle"


@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("env", [{"SKR_GI_SURFACE": "0"}, {"SKR_GI_SURFACE": "1"}, {"SKR_GI_MASK": "0"}, {"SKR_GI_MASK": "1"}])
def test_gi_mask_switches_with_kept_stage(gpu, monkeypatch, spheres2, env, depth):
    """The masks are conservative either way: frames and counts under every setting are those of the default switches."""
    kw = dict(depth=depth, gillum=4 if depth == 4 else 6)
    monkeypatch.setenv("SKR_FLAT", "0")
    want = [fresh(gpu, monkeypatch, spheres2, frame_of(opts(**dict(kw, seed=100 + k)))) for k in range(2)]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = skr.Renderer(spheres2)
    for k in range(2):
        got = observe(gpu, r, frame_of(opts(**dict(kw, seed=100 + k))))
        assert r.primary_cache_stats() == (1, k)
        for i in (0, 1, 2, 3, 4):
            assert np.array_equal(got[i], want[k][i]) if i < 2 else got[i] == want[k][i], (env, depth, k, i)


def test_switching_the_gi_masks_builds_again(gpu, monkeypatch, spheres2):
    """The stage holds each node's row of GI masks: other masks (SKR_GI_SURFACE, SKR_GI_MASK through reload_switches), other rows."""
    monkeypatch.setenv("SKR_FLAT", "0")
    r = skr.Renderer(spheres2)
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=1)), (1, 0))
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=2)), (1, 1))
    monkeypatch.setenv("SKR_GI_SURFACE", "0")
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=3)), (2, 1), "grids only")
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=4)), (2, 2))
    monkeypatch.setenv("SKR_GI_MASK", "0")
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=5)), (3, 2), "no masks")
    monkeypatch.delenv("SKR_GI_MASK")
    monkeypatch.delenv("SKR_GI_SURFACE")
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=6)), (4, 2), "patches again")
    check(gpu, monkeypatch, spheres2, r, frame_of(opts(seed=7)), (4, 3))
