"""skr_tile_costs borrows a renderer for one small render per tile and leaves no mark on it: with kernel timing on, the probe's launches
are not among those skr_renderer_kernel_ms averages, the caller's work counters are what they were, and the next frame is the frame."""
import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import scene_path

pytestmark = pytest.mark.gpu


def test_tile_costs_leaves_timing_counters_and_frames_alone():
    import torch
    assert torch.cuda.is_available(), "this test needs the MI355X"
    r = skr.Renderer(skr.parse_scene(scene_path("spheres2.scn")))
    opt = skr.Options(64, 48, gillum=2, depth=3, shadow=True)
    r.kernel_timing(True)
    before, _ = r.render(opt)
    torch.cuda.synchronize()
    assert r.kernel_ms()[1] == 1
    w0 = r.work(reset=False)
    assert w0["radiance_rays"] > 0
    cost = r.tile_costs(opt, 16)  # three tiles
    assert len(cost) == 3 and cost.min() > 0
    assert r.kernel_ms()[1] == 0  # (the probe's three launches were timed before the fix)
    assert r.work(reset=False) == w0
    after, _ = r.render(opt)
    torch.cuda.synchronize()
    assert np.array_equal(after.cpu().numpy(), before.cpu().numpy())
    assert r.kernel_ms()[1] == 1  # (timing is still on for the caller's own launches)
    r.close()
