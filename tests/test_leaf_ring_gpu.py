"""The leaf kernel's hit ring and slot windows at their edges (csrc/render_nodes.hip skr_leaf_kernel2: NQ_CAP, NWIN and the batch rule),
on the MI355X (pytest -m gpu), against the CPU oracle bit for bit — float words, bytes and the four work counts — with SKR_FLAT=0 and
the variant asserted, so that the persistent leaf kernel is what ran.

  slab scene     the camera, the lights and six small spheres in a narrow gap between two large spheres (no sphere can enclose the
                 camera: a ray that starts inside a sphere never hits it): more than nine children of ten hit, a round of a full unit
                 pushes about 120 hits, and the ring stands near its bound round after round (NQ_PRE waiting + the 128 a round can add)
  window edges   --gillum 1, 2, 5, 6, 7, 8, 9: fewer rounds than windows, an odd last round (no second child), and the first reuse of
                 a window, with the four windows of today (round 4) and with the three of tools/experiments/leaf_full_batches.patch (round 3)
  short unit     fewer than 64 records in a launch's last unit, and in its only one
each at depth 2 (the units are the level-0 nodes) and at depth 3 (records)."""
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path
from pow_plan_cases import SWITCHES, last_leaf, write_slab_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SKR_FLAT", "0")


@pytest.fixture(scope="module")
def slab(tmp_path_factory):
    return write_slab_scene(os.path.join(str(tmp_path_factory.mktemp("leaf_ring")), "slab.scn"))


def check(gpu, oracle, path, w, h, kw):
    """-> (the four counts, the level-0 nodes of the launch)"""
    rgb_o, f_o, st = oracle.render(path, w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw)
    r = skr.Renderer(skr.parse_scene(path))
    try:
        r.work(reset=True)
        rgb, rgbf = r.render(skr.Options(w, h, **kw), want_float=True)
        gpu.cuda.synchronize()
        wk = r.work(reset=True)
        assert r.kernel_variant() == "node_levels_v5", r.kernel_variant()
        assert last_leaf(r)[0] >= 0  # a leaf kernel ran
        got = rgbf.cpu().numpy().view(np.uint32).reshape(-1)
        exp = f_o.view(np.uint32).reshape(-1)
        assert np.array_equal(got, exp), "%s %s: %d float words differ" % (os.path.basename(path), kw, int((got != exp).sum()))
        assert np.array_equal(rgb.cpu().numpy(), rgb_o)
        counts = (wk["radiance_rays"], wk["sphere_hits"], wk["shadow_rays"], wk["sphere_tests"])
        assert counts == tuple(int(v) for v in st[:4]), (counts, st)
        return counts, r.last_parent_count()
    finally:
        r.close()


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("gillum", [2, 16])
def test_slab_scene_nearly_every_child_hits(gpu, oracle, slab, gillum, depth):
    w, h = 32, 18
    counts, nodes = check(gpu, oracle, slab, w, h, dict(gillum=gillum, depth=depth, shadow=True, seed=71))
    # a child leaves only within 4.4 degrees of the tangent plane: 7.7 % of a uniform hemisphere; primary rays only through the rim too
    assert nodes > 0.85 * w * h and counts[1] > 0.9 * counts[0], (counts, nodes)


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("gillum", [1, 2, 5, 6, 7, 8, 9])
def test_window_edges(gpu, oracle, gillum, depth):
    check(gpu, oracle, scene_path("spheres2.scn"), 64, 36, dict(gillum=gillum, depth=depth, shadow=True, seed=72))


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("size", [(8, 5), (24, 11)], ids=["8x5", "24x11"])
def test_short_units(gpu, oracle, slab, size, depth):
    """8x5: the launch's only unit of level-0 nodes holds at most 40; 24x11: up to 264 nodes, the last unit not full.  (At depth 3 the
    records spread over 64 regions: every unit is short.)"""
    _, nodes = check(gpu, oracle, slab, size[0], size[1], dict(gillum=9, depth=depth, shadow=True, seed=73))
    assert 0 < nodes <= size[0] * size[1] and nodes % 64 != 0, nodes
