"""Spot lights, lights with a radius, triangle shadows under them and the thin lens on the MI355X, over the cases of
tests/light_mode_cases.py (tests/test_light_modes_cpu.py shows on the host that the checkers are evidence on them and what each family
reaches): per case one renderer and one frame against the CPU checker — float words with no tolerance, bytes, the four work counts —,
the kernel variant the case's features imply, then the case's 257 query rays through Renderer.shade against the checker's shade, values
word for word and the three counts.  Mesh cases render once more with culling off and must not move a bit."""
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
import light_mode_cases as lm
from lens_check import build as build_lens_checker
from soft_light_check import build as build_soft_checker
from test_camera_poses_gpu import same_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="session")
def soft(tmp_path_factory):
    return build_soft_checker(str(tmp_path_factory.mktemp("lightmodes_soft_gpu")))


@pytest.fixture(scope="session")
def lens(tmp_path_factory):
    return build_lens_checker(str(tmp_path_factory.mktemp("lightmodes_lens_gpu")))


@pytest.fixture(scope="session")
def folder(tmp_path_factory):
    return str(tmp_path_factory.mktemp("lightmodes_scenes_gpu"))


def load(case):
    sc = skr.parse_scene(case.scene, **case.flags)
    sc.set_light_radii(case.radii)
    if case.lens is not None:
        sc.set_lens(*case.lens)
    return sc


def render(torch, r, case):
    rgb, rgbf = r.render(skr.Options(case.w, case.h, **case.kw), want_float=True)
    torch.cuda.synchronize()
    c = r.work()
    return rgb.cpu().numpy(), rgbf.cpu().numpy(), [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"], c["sphere_tests"]], skr.Renderer.kernel_variant()


def check_case(torch, soft, lens, case):
    """The comparisons of one case: (what differs — empty: the case holds —, the frame's kernel variant); tests/fuzz_light_modes.py prints them."""
    bad = []
    nan_ok = case.name in lm.NAN
    sc = load(case)
    rows, cones = sc.spot_lights, sc.spot_cones
    r = skr.Renderer(sc)
    try:
        g_rgb, g_f, g_cnt, variant = render(torch, r, case)
        c_rgb, c_f, c_st = lm.checker_frame(soft, lens, case, rows, cones)
        eq = same_words(g_f, c_f, nan_ok)
        if not eq.all():
            bad.append("frame: %d float words differ, first at %s" % (int((~eq).sum()), np.argwhere(~eq)[:3].tolist()))
        if not np.array_equal(g_rgb, c_rgb):
            bad.append("frame: %d bytes differ" % int((g_rgb != c_rgb).sum()))
        if g_cnt != [int(x) for x in c_st[:4]]:
            bad.append("frame: work counts %s, the checker's %s" % (g_cnt, [int(x) for x in c_st[:4]]))
        want = lm.variant_name(case, sc.info.n_triangles)
        if variant != want:
            bad.append("kernel variant %s, expected %s" % (variant, want))
        if sc.info.n_triangles > 0:  # culling off: every triangle, the same bits
            os.environ["SKR_NO_CULL"] = "1"
            try:
                flat = skr.Renderer(load(case))
                try:
                    f_rgb, f_f, f_cnt, f_variant = render(torch, flat, case)
                finally:
                    flat.close()
            finally:
                del os.environ["SKR_NO_CULL"]
            if not (same_words(f_f, g_f, nan_ok).all() and np.array_equal(f_rgb, g_rgb) and f_cnt == g_cnt and f_variant == variant):
                bad.append("SKR_NO_CULL=1 moves the frame: %d words, counts %s against %s" % (int((~same_words(f_f, g_f, nan_ok)).sum()), f_cnt, g_cnt))
        # the shading query
        kw = lm.query_options(case)
        r.counters(reset=True)
        got = r.shade(torch.from_numpy(case.rays).to("cuda:0"), skr.Options(8, 8, **kw), sample=case.sample, keys=torch.from_numpy(case.keys.view(np.int32)).to("cuda:0"))
        torch.cuda.synchronize()
        c = r.counters()
        want_q, st = soft.shade(case.scene, case.rays, radii=case.radii, spots=rows, cones=cones, triangle_shadows=case.flags["triangle_shadows"], sample=case.sample, keys=case.keys,
                                strict=case.flags["strict"], **kw)
        eq = same_words(got.cpu().numpy(), want_q, nan_ok)
        if not eq.all():
            bad.append("query: %d float words differ, first at ray %s" % (int((~eq).sum()), np.argwhere(~eq)[:3].tolist()))
        if [c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]] != [int(x) for x in st]:
            bad.append("query: counts %s, the checker's %s" % ([c["radiance_rays"], c["sphere_hits"], c["shadow_rays"]], [int(x) for x in st]))
    finally:
        r.close()
    return bad, variant


ERRORS = []  # a case that ended in an error (not a mismatch, not a refused launch): nothing further is started on the GPU after it


@pytest.mark.parametrize("fi", lm.EDGE + lm.RANDOM, ids=lm.case_id)
def test_frame_and_query_match_the_checker_bit_for_bit(gpu, soft, lens, folder, fi):
    assert not ERRORS, "not run: %s ended in an error before it" % ERRORS[0]
    case = lm.build(*fi, folder)
    try:
        bad, _ = check_case(gpu, soft, lens, case)
    except Exception as e:
        if "(status 4)" not in str(e):  # (a refused launch leaves the device as it was)
            ERRORS.append(case.name)
        raise
    assert not bad, "%s (%s): %s" % (case.name, case.meta.get("what", case.meta.get("mode")), "; ".join(bad))
