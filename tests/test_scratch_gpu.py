"""One renderer through every user of its scratch in turn (the level tables and the AA image, the progressive and adaptive buffers, the
device frame of the *_host entries, the denoiser's buffers), at frame sizes that grow and shrink: every result equals the same call on a
fresh renderer, bit for bit.  Then a clone runs most of the sequence while its source renders other sizes in between."""
import numpy as np
import pytest
import torch

import skele_raytracer_amd as skr
from conftest import scene_path

pytestmark = pytest.mark.gpu

KW = dict(gillum=4, depth=3, shadow=True, seed=5)
SIZES = [(48, 32, {}), (160, 96, dict(jsample=2)), (24, 40, {}), (200, 120, {}), (64, 16, dict(jsample=2))]


def calls(w, h, kw):
    """(name, call) for every scratch user at w x h: call(renderer) returns its outputs"""
    def opt(**more):
        return skr.Options(w, h, **KW, **kw, **more)

    def shade(r):
        rays = r.camera_rays(opt()).view(-1, 8)
        return [r.shade(rays, opt(), 0, keys=torch.arange(w * h, dtype=torch.int32, device=rays.device))]

    return [
        ("render", lambda r: r.render(opt(), want_float=True)),
        ("render_progressive3", lambda r: r.render(opt(progressive=3), want_float=True)),
        ("shade_camera_rays", shade),
        ("render_denoised", lambda r: r.render_denoised(opt(), want_float=True)[:2]),
        ("render_adaptive_host", lambda r: r.render_adaptive_host(opt(), 0.05, 2, 8, want_float=True)[:3]),
        ("render_progressive_host", lambda r: r.render_progressive_host(opt(progressive=3), want_float=True)[:2]),
        ("render_progressive_host_every", lambda r: r.render_progressive_host(opt(progressive=3), every=1, want_float=True, progress=lambda *a: False)[:2]),
        ("render_rows", lambda r: r.render_rows(opt(), h // 3, h, want_float=True)),
    ]


def check(scene, r, name, call, what):
    """call(r) == call(a fresh renderer), byte for byte"""
    def words(outs):
        return [np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x).reshape(-1).view(np.uint8) for x in outs]
    got = words(call(r))
    fresh = skr.Renderer(scene, 0)
    try:
        want = words(call(fresh))
    finally:
        fresh.close()
    assert len(got) == len(want) and all(np.array_equal(g, f) for g, f in zip(got, want)), "%s, %s: differs from a fresh renderer" % (what, name)


@pytest.mark.parametrize("scn", ["spheres2.scn", "test.scn"])
def test_one_renderer_through_every_scratch_user_at_changing_sizes(scn):
    scene = skr.parse_scene(scene_path(scn))
    r = skr.Renderer(scene, 0)
    try:
        for w, h, kw in SIZES:
            for name, call in calls(w, h, kw):
                check(scene, r, name, call, "%s %dx%d %s" % (scn, w, h, kw))
    finally:
        r.close()


@pytest.mark.parametrize("scn", ["spheres2.scn", "test.scn"])
def test_a_clone_keeps_its_scratch_while_the_source_renders_other_sizes(scn):
    scene = skr.parse_scene(scene_path(scn))
    r = skr.Renderer(scene, 0)
    c = r.clone()
    try:
        for i, (w, h, kw) in enumerate(SIZES):
            for (name, call), (_, other) in zip(calls(w, h, kw)[1:], calls(*SIZES[(i + 2) % len(SIZES)])):
                check(scene, c, name, call, "clone, %s %dx%d %s" % (scn, w, h, kw))
                other(r)  # the source grows or shrinks its own buffers in between
        check(scene, r, "render_progressive_host_every", calls(*SIZES[1])[6][1], "the source after its clone")
    finally:
        c.close()
        r.close()
