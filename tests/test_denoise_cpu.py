"""CPU checks of the denoiser (include/skr.h skr_denoise): the public surface is declared and exported, and the C checker
(tests/denoise_checker.c) equals an independent numpy restatement bit for bit and keeps the rule's invariants."""
import os
import re
import subprocess

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import ROOT
from denoise_check import MISS, build as build_checker, classes, denoise_numpy, quantise, random_frame, random_guides


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("denoise_checker")))


def test_denoise_surface_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "skr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("skr_denoise", "skr_render_denoised_host"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in skr.EXPORTED_SYMBOLS
    assert re.search(r"#define SKR_HAS_DENOISE 1\b", header)
    assert re.search(r"#define SKR_ABI_VERSION 7\b", header)
    for const in ("SKR_DENOISE_SIGMA_L", "SKR_DENOISE_SIGMA_Z", "SKR_DENOISE_EPS", "SKR_DENOISE_ITERATIONS", "SKR_DENOISE_MAX_ITERATIONS"):
        assert re.search(r"#define %s\b" % const, header), const
    out = subprocess.check_output(["nm", "-D", "--defined-only", skr.lib_path()], text=True)
    exported = set(re.findall(r" T (skr_[a-z0-9_]+)", out))
    assert {"skr_denoise", "skr_render_denoised_host"} <= exported
    assert callable(skr.Renderer.denoise) and callable(skr.Renderer.render_denoised)


def test_cli_usage_errors_need_no_gpu():
    # the combinations the filter cannot serve are refused before a device is opened
    cli = os.path.join(ROOT, "bin", "raytracer")
    scn = os.path.join(ROOT, "tests", "golden", "scenes", "spheres2.scn")
    for extra in (["--gpus", "2"], ["--progressive", "4", "--progressive-every", "2"], ["--denoise", "17"]):
        args = ["--denoise", "5"] + extra if extra[0] != "--denoise" else extra
        p = subprocess.run([cli, "--path", scn, "--output", os.devnull, "--width", "8", "--height", "8", "--quiet"] + args, capture_output=True, text=True)
        assert p.returncode == 2 and "--denoise" in p.stderr, (args, p.returncode, p.stderr)


SIZES = [(1, 1), (1, 9), (17, 13), (40, 23)]


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("L", [0, 1, 5, 16])
def test_checker_equals_numpy_restatement(chk, h, w, L):
    seed = 1000 * h + w + L
    g = random_guides(h, w, seed)
    c = random_frame(h, w, seed)
    rgb, out = chk.denoise(c, g, L)
    nrgb, nout = denoise_numpy(c, g, L)
    assert np.array_equal(out.view(np.uint32), nout.view(np.uint32)), np.argwhere(out.view(np.uint32) != nout.view(np.uint32))[:5]
    assert np.array_equal(rgb, nrgb)
    assert np.array_equal(rgb, quantise(out))


def test_checker_zero_iterations_is_identity(chk):
    g = random_guides(17, 13, 5)
    c = random_frame(17, 13, 5)
    c[0, 0] = [np.inf, np.nan, -1.0]
    rgb, out = chk.denoise(c, g, 0)
    assert np.array_equal(out.view(np.uint32), c.view(np.uint32))
    assert np.array_equal(rgb, quantise(c))


def test_checker_filters(chk):
    # it does something: a noisy frame of one class loses most of its variance
    h, w = 40, 23
    g = random_guides(h, w, 9)
    c = random_frame(h, w, 9)
    _, out = chk.denoise(c, g, 5)
    assert not np.array_equal(out, c)
    cls = classes(g, h, w)
    for k in np.unique(cls):
        m = cls == k
        if m.sum() > 20:
            assert out[m].var(axis=0).sum() <= c[m].var(axis=0).sum() + 1e-7


@pytest.mark.parametrize("L", [1, 5, 16])
def test_zero_class_stays_zero(chk, L):
    h, w = 40, 23
    g = random_guides(h, w, 11)
    c = random_frame(h, w, 11) * np.float32(3)
    cls = classes(g, h, w)
    for k in np.unique(cls):
        cz = c.copy()
        cz[cls == k] = 0
        _, out = chk.denoise(cz, g, L)
        assert np.all(out[cls == k].view(np.uint32) == 0), k


@pytest.mark.parametrize("L", [1, 5, 16])
def test_constant_colour_per_class_keeps_its_bytes(chk, L):
    h, w = 40, 23
    g = random_guides(h, w, 13)
    cls = classes(g, h, w)
    rng = np.random.default_rng(13)
    c = np.zeros((h, w, 3), np.float32)
    for k in np.unique(cls):
        c[cls == k] = ((rng.integers(0, 255, 3) + 0.5) / 255).astype(np.float32)
    rgb, _ = chk.denoise(c, g, L)
    assert np.array_equal(rgb, quantise(c))


def test_miss_pixels_ignore_guides(chk):
    # a miss has no normal and no depth: its weights are luminance and kernel only
    h, w = 17, 13
    g = random_guides(h, w, 17).reshape(h, w, 8)
    g.view(np.int32)[..., 1] = 0
    g.view(np.int32)[..., 2] = -1
    g[..., 0] = np.inf
    g[..., 3:6] = 0
    c = random_frame(h, w, 17)
    _, out = chk.denoise(c, g.reshape(-1, 8), 3)
    assert np.all(np.isfinite(out))
    assert np.all(classes(g.reshape(-1, 8), h, w) == np.uint32(MISS))
