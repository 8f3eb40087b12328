"""The node pipeline's trace kernel holds one NODE per lane and loops over its sibling pairs (csrc/render_nodes.hip skr_trace_kernel,
csrc/launch.h skr_trace_header_row): a wave is a block of 64 consecutive nodes and its header for pair j is row
(node >> 6) * PP + j.  Every frame here is small enough for the CPU oracle and is held against it bit for
bit — bytes, float image, and the four work counts — at the shapes where that indexing can go wrong: one sibling pair, a lone last
child, a full run of pairs, a last node block that is partial, a node block of one node, nodes that skr_activate_kernel wrote, several
bands, several AA samples, a replayed level-0 stage, and the triangle row of the headers.  Both schedules (SKR_FLAT=0 / 1) run every shape.
"""
import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path

pytestmark = pytest.mark.gpu

SWITCHES = ("SKR_FLAT", "SKR_PIPELINE", "SKR_GI_MASK", "SKR_GI_SURFACE", "SKR_LEVELS_BUDGET_MB", "SKR_PRIMARY_CACHE", "SKR_LEAF_SHAPE")
W, H = 64, 36
SCHEDULES = [("0", "node_levels_v5"), ("1", "node_levels_v5_flat")]
_ORACLE = {}  # one oracle frame per (scene, size, options, rows), shared by the schedules


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def want(oracle, scn, w, h, kw, rows=None):
    key = (scn, w, h, tuple(sorted(kw.items())), rows)
    if key not in _ORACLE:
        ykw = {} if rows is None else dict(y0=rows[0], y1=rows[1])
        rgb, f, st = oracle.render(scene_path(scn), w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **dict(kw, **ykw))
        _ORACLE[key] = (rgb, f.view(np.uint32), tuple(int(v) for v in st[:4]))
    return _ORACLE[key]


def primary_hits(oracle, scn, w, h, rows=None, fov=60.0):
    """Sphere hits of the primary rays of the rows: the level-0 nodes of a --gillum frame of them."""
    return want(oracle, scn, w, h, dict(depth=1, fov=fov), rows)[2][1]


def frame(gpu, r, opt, **tiles):
    r.work(reset=True)
    rgb, rgbf = r.render(opt, want_float=True, **tiles)
    gpu.cuda.synchronize()
    wk = r.work(reset=True)
    return rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), (wk["radiance_rays"], wk["sphere_hits"], wk["shadow_rays"], wk["sphere_tests"])


def assert_oracle(got, exp, what):
    assert got[0].shape == exp[0].shape, (what, got[0].shape, exp[0].shape)
    assert np.array_equal(got[1].reshape(-1), exp[1].reshape(-1)), "%s: %d float words differ" % (what, int((got[1].reshape(-1) != exp[1].reshape(-1)).sum()))
    assert np.array_equal(got[0], exp[0]), "%s: bytes differ at %d pixels" % (what, int((got[0] != exp[0]).any(-1).sum()))
    assert got[2] == exp[2], (what, got[2], exp[2])
    assert exp[2][0] > 0


def check(gpu, oracle, monkeypatch, flat, variant, scn, w, h, kw, env=None, rows=None):
    monkeypatch.setenv("SKR_FLAT", flat)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = skr.Renderer(skr.parse_scene(scene_path(scn)))
    tiles = {} if rows is None else dict(tile_rows=rows[1] - rows[0], first_tile=rows[0] // (rows[1] - rows[0]), tile_stride=h)
    got = frame(gpu, r, skr.Options(w, h, **kw), **tiles)
    assert r.kernel_variant() == variant
    assert_oracle(got, want(oracle, scn, w, h, kw, rows), "%s %s flat=%s" % (scn, kw, flat))
    return r


@pytest.mark.parametrize("flat,variant", SCHEDULES)
@pytest.mark.parametrize("gillum", [1, 2, 3, 5, 16])
def test_pairs_per_node_and_a_partial_last_node_block(gpu, oracle, monkeypatch, gillum, flat, variant):
    """PP = 1 (one round, a lone child), 1 (both children), 2 and 3 with a lone last child, 8: a full run."""
    kw = dict(gillum=gillum, depth=3, shadow=True, seed=20 + gillum)
    r = check(gpu, oracle, monkeypatch, flat, variant, "spheres2.scn", W, H, kw)
    n0 = r.last_parent_count()
    assert n0 == primary_hits(oracle, "spheres2.scn", W, H) and n0 > 64 and n0 % 64 != 0  # several node blocks, the last one partial


@pytest.mark.parametrize("flat,variant", SCHEDULES)
@pytest.mark.parametrize("gillum", [3, 4])
def test_nodes_of_the_activate_kernel(gpu, oracle, monkeypatch, gillum, flat, variant):
    """Depth 4: the second trace launch takes its node count from the prefix word and its nodes from skr_activate_kernel."""
    check(gpu, oracle, monkeypatch, flat, variant, "spheres2.scn", W, H, dict(gillum=gillum, depth=4, shadow=True, seed=5))


@pytest.mark.parametrize("flat,variant", SCHEDULES)
def test_depth_two(gpu, oracle, monkeypatch, flat, variant):
    """No trace launch on the persistent schedule (the FIRST leaf kernel), one on the flat schedule: the plan holds for both."""
    check(gpu, oracle, monkeypatch, flat, variant, "spheres2.scn", W, H, dict(gillum=5, depth=2, shadow=True, seed=6))


def test_three_bands(gpu, oracle, monkeypatch):
    """A frame one 16x16 block wide and three high under a budget of 1 MiB.  --gillum 97 (PP = 49, a lone last child): one block's 256
    nodes are 4 node blocks x 49 header rows = 196 rows, four at most per region, so a region holds 512 records and the level
    64 x 512 = 32 768 of them: 0.9 MiB of record (16 B) and result (12 B) tables.  Two blocks' 392 rows make it 7 x 128 x 64 = 57 344
    records, 1.5 MiB.  So a band is one block and the frame three bands, the last one rows 32..35: its level-0 nodes are the primary
    hits of those rows, and no level-0 stage is kept."""
    w, h = 16, 36
    kw = dict(gillum=97, depth=3, shadow=True, seed=8)
    r = check(gpu, oracle, monkeypatch, "0", "node_levels_v5", "spheres2.scn", w, h, kw, env={"SKR_LEVELS_BUDGET_MB": "1"})
    last = primary_hits(oracle, "spheres2.scn", w, h, rows=(32, 36))
    assert 0 < last < primary_hits(oracle, "spheres2.scn", w, h) and r.last_parent_count() == last
    assert r.primary_cache_stats() == (0, 0)


@pytest.mark.parametrize("flat,variant", SCHEDULES)
def test_aa_samples(gpu, oracle, monkeypatch, flat, variant):
    """--jsample 2: four passes, no replay; aa_index reaches the trace kernel's Philox."""
    check(gpu, oracle, monkeypatch, flat, variant, "spheres2.scn", 48, 27, dict(gillum=5, jsample=2, depth=3, shadow=True, seed=7))


@pytest.mark.parametrize("flat,variant", SCHEDULES)
def test_triangle_row_of_the_headers(gpu, oracle, monkeypatch, flat, variant):
    """spheres1.scn has two triangles: the TRIS instances, the third header row, classify_child's walk."""
    r = check(gpu, oracle, monkeypatch, flat, variant, "spheres1.scn", W, H, dict(gillum=5, depth=3, shadow=True, seed=21))
    assert r.last_parent_count() % 64 != 0


@pytest.mark.parametrize("flat,variant", SCHEDULES)
@pytest.mark.parametrize("fov,row,nodes", [(60.0, 4, 4), (70.0, 6, 1)])
def test_a_crop_of_less_than_one_node_block(gpu, oracle, monkeypatch, fov, row, nodes, flat, variant):
    """One image row whose primary rays hit a sphere 4 times, and one where exactly one does: a single, partial node block."""
    assert primary_hits(oracle, "spheres2.scn", W, H, rows=(row, row + 1), fov=fov) == nodes
    r = check(gpu, oracle, monkeypatch, flat, variant, "spheres2.scn", W, H, dict(gillum=5, depth=3, shadow=True, seed=9, fov=fov), rows=(row, row + 1))
    assert r.last_parent_count() == nodes


@pytest.mark.parametrize("flat,variant", SCHEDULES)
def test_a_second_frame_replays_the_level_0_stage(gpu, oracle, monkeypatch, flat, variant):
    """Build, then replay: the second frame's trace kernel reads the kept nodes and their stored rows of GI masks (gi_row0)."""
    monkeypatch.setenv("SKR_FLAT", flat)
    r = skr.Renderer(skr.parse_scene(scene_path("spheres2.scn")))
    for k, seed in enumerate((31, 32)):
        kw = dict(gillum=6, depth=3, shadow=True, seed=seed)
        got = frame(gpu, r, skr.Options(W, H, **kw))
        assert r.kernel_variant() == variant
        assert_oracle(got, want(oracle, "spheres2.scn", W, H, kw), "frame %d flat=%s" % (k, flat))
        assert r.primary_cache_stats() == (1, k)
