"""CPU checks of adaptive frames denoised under their measured variance (include/skr.h skr_render_adaptive_var, skr_denoise_var,
skr_render_adaptive_denoised_host): the public surface is declared and compiles as C, the C checker
(tests/denoise_var_checker.c) equals an independent numpy restatement bit for bit, the identities of the rule hold, and the variance of
the mean is the e2 the stopping rule tests."""
import os
import re
import subprocess

import numpy as np
import pytest

import skele_raytracer_amd as skr
from adaptive_check import LUM_FLOOR, converged
from conftest import ROOT
from denoise_check import build as build_old_checker, classes, quantise, random_frame, random_guides
from denoise_var_check import VAR_SIGMA_L, adaptive_with_variance, build as build_checker, denoise_var_numpy, random_variance, variance_of_mean
from skele_raytracer_amd import DENOISE_VAR_SIGMA_L  # (the feature: without it nothing below means anything)

ENTRY_POINTS = ("skr_render_adaptive_var", "skr_denoise_var", "skr_render_adaptive_denoised_host")
f32 = np.float32


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("denoise_var_checker")))


@pytest.fixture(scope="module")
def old_chk(tmp_path_factory):
    return build_old_checker(str(tmp_path_factory.mktemp("denoise_checker_for_var")))


def test_surface_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "skr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in skr.EXPORTED_SYMBOLS
    assert re.search(r"#define SKR_ABI_VERSION 7\b", header)
    m = re.search(r"#define SKR_DENOISE_VAR_SIGMA_L\s+([0-9.]+)f\b", header)
    assert m and float(m.group(1)) in (2.0, 4.0, 8.0) and float(m.group(1)) == DENOISE_VAR_SIGMA_L == float(VAR_SIGMA_L)
    checker = open(os.path.join(ROOT, "tests", "denoise_var_checker.c")).read()
    assert re.search(r"#define VAR_SIGMA_L %sf\b" % m.group(1), checker), "the C checker restates the header's sigma"
    out = subprocess.check_output(["nm", "-D", "--defined-only", skr.lib_path()], text=True)
    assert set(ENTRY_POINTS) <= set(re.findall(r" T (skr_[a-z0-9_]+)", out))
    assert callable(skr.Renderer.render_adaptive_denoised)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "skr.h"\n'
                   "#if SKR_ABI_VERSION != 7\n#error abi\n#endif\n"
                   "int (*a)(skr_renderer *, const skr_options *, const skr_adaptive *, uint8_t *, float *, uint32_t *, float *, void *) = skr_render_adaptive_var;\n"
                   "int (*b)(skr_renderer *, uint32_t, uint32_t, const float *, const skr_hit *, const float *, uint32_t, float *, uint8_t *, void *) = skr_denoise_var;\n"
                   "int (*c)(skr_renderer *, const skr_options *, const skr_adaptive *, uint32_t, uint8_t *, float *, uint32_t *, float *) = skr_render_adaptive_denoised_host;\n"
                   "float sigma = SKR_DENOISE_VAR_SIGMA_L;\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "use.o"), str(src)])


def test_cli_usage_errors_need_no_gpu():
    cli = os.path.join(ROOT, "bin", "raytracer")
    scn = os.path.join(ROOT, "tests", "golden", "scenes", "spheres2.scn")
    base = [cli, "--path", scn, "--output", os.devnull, "--width", "8", "--height", "8", "--quiet"]
    for args, word in ((["--adaptive-denoise", "5"], "--adaptive"), (["--adaptive", "0.1", "--adaptive-denoise", "17"], "--adaptive-denoise"),
                       (["--adaptive", "0.1", "--adaptive-denoise", "5", "--denoise", "5"], "--denoise"), (["--adaptive", "0.1", "--denoise", "5"], "--adaptive")):
        p = subprocess.run(base + args, capture_output=True, text=True)
        assert p.returncode == 2 and word in p.stderr, (args, p.returncode, p.stderr)


SIZES = [(1, 1), (1, 9), (17, 13), (40, 23)]


def inputs(h, w, seed):
    g = random_guides(h, w, seed)
    return random_frame(h, w, seed), g, random_variance(g, h, w, seed)


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("L", [0, 1, 5, 16])
def test_checker_equals_numpy_restatement(chk, h, w, L):
    c, g, v = inputs(h, w, 1000 * h + w + L)
    rgb, out = chk.denoise(c, g, v, L)
    nrgb, nout = denoise_var_numpy(c, g, v, L)
    assert np.array_equal(out.view(np.uint32), nout.view(np.uint32)), np.argwhere(out.view(np.uint32) != nout.view(np.uint32))[:5]
    assert np.array_equal(rgb, nrgb)
    assert np.array_equal(rgb, quantise(out))


def test_variance_images_cover_every_kind_of_entry():
    h, w = 40, 23
    c, g, v = inputs(h, w, 1000 * h + w)
    cls = classes(g, h, w)
    pos = v[np.isfinite(v) & (v > 0)]
    assert pos.max() / pos.min() > 1e5 and (v == 0).any() and (v == -1).any() and np.isnan(v).any() and np.isposinf(v).any()
    assert any((v[cls == k] == -1).all() and (cls == k).sum() > 1 for k in np.unique(cls)), "a whole class is unmeasured"


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("L", [0, 1, 5, 16])
def test_all_unmeasured_is_the_existing_denoiser(chk, old_chk, h, w, L):
    c, g, v = inputs(h, w, 77 * h + w)
    want_rgb, want = old_chk.denoise(c, g, L)
    unmeasured = np.where(np.isnan(v), v, f32(-1)).astype(np.float32)  # -1 and NaN, no entry >= 0
    unmeasured[0, 0] = f32(-0.5)
    for var in (None, np.full((h, w), -1, np.float32), unmeasured):
        rgb, out = chk.denoise(c, g, var, L)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and np.array_equal(rgb, want_rgb)
        nrgb, nout = denoise_var_numpy(c, g, var, L)
        assert np.array_equal(nout.view(np.uint32), want.view(np.uint32)) and np.array_equal(nrgb, want_rgb)


def test_zero_iterations_is_identity(chk):
    c, g, v = inputs(17, 13, 5)
    c[0, 0] = [np.inf, np.nan, -1.0]
    rgb, out = chk.denoise(c, g, v, 0)
    assert np.array_equal(out.view(np.uint32), c.view(np.uint32))
    assert np.array_equal(rgb, quantise(c))


@pytest.mark.parametrize("L", [1, 5, 16])
def test_constant_colour_per_class_keeps_its_bytes(chk, L):
    h, w = 40, 23
    g = random_guides(h, w, 13)
    cls = classes(g, h, w)
    rng = np.random.default_rng(13)
    c = np.zeros((h, w, 3), np.float32)
    for k in np.unique(cls):
        c[cls == k] = ((rng.integers(0, 255, 3) + 0.5) / 255).astype(np.float32)
    for v in (random_variance(g, h, w, 13), np.full((h, w), 0.01, np.float32), np.zeros((h, w), np.float32)):
        rgb, _ = chk.denoise(c, g, v, L)
        assert np.array_equal(rgb, quantise(c))


def test_an_infinite_variance_keeps_the_pixel(chk):
    h, w = 17, 13
    c, g, _ = inputs(h, w, 21)
    v = np.full((h, w), 1e-3, np.float32)
    v[8, 6] = np.inf
    _, out = chk.denoise(c, g, v, 5)
    assert np.array_equal(out[8, 6].view(np.uint32), c[8, 6].view(np.uint32))
    assert not np.array_equal(out, c)


def test_a_measured_variance_changes_the_filter(chk, old_chk):
    c, g, _ = inputs(40, 23, 9)
    _, spatial = old_chk.denoise(c, g, 5)
    _, small = chk.denoise(c, g, np.zeros((40, 23), np.float32), 5)
    _, large = chk.denoise(c, g, np.full((40, 23), 10.0, np.float32), 5)
    assert not np.array_equal(small, spatial) and not np.array_equal(large, spatial)
    assert np.abs(small - c).mean() < np.abs(large - c).mean()  # no variance: the luminance weight stops nearly every tap


# ---- the variance of the mean ----
def random_states(n, seed):
    rng = np.random.default_rng(seed)
    passes = rng.integers(2, 65, n)
    l = rng.exponential(0.3, (64, n)).astype(np.float32)
    l[:, rng.random(n) < 0.2] = f32(0.25)  # constant pixels
    S1 = np.zeros(n, np.float32)
    S2 = np.zeros(n, np.float32)
    for k in range(64):
        on = k < passes
        S1 = np.where(on, S1 + l[k], S1).astype(np.float32)
        S2 = np.where(on, S2 + l[k] * l[k], S2).astype(np.float32)
    return S1, S2, passes


def test_variance_of_mean_is_the_e2_of_the_stopping_rule():
    S1, S2, n = random_states(4000, 3)
    var = variance_of_mean(S1, S2, n)
    assert (var >= 0).all() and (var > 0).any() and (var == 0).any()
    m = (S1 / n.astype(np.float32)).astype(np.float32)
    floor = np.where(m > LUM_FLOOR, m, LUM_FLOOR).astype(np.float64)
    # converged(t) is e2 <= (t * floor)^2 with the rule's own e2: a threshold a little under sqrt(var) / floor must not converge, one a
    # little over it must, so var is that e2 to within the nudge (and 0 where it is 0: converged at every threshold >= 0)
    for i in range(len(n)):
        t = np.sqrt(float(var[i])) / floor[i]
        one = lambda thr: bool(converged(S1[i:i + 1], S2[i:i + 1], int(n[i]), thr)[0])
        assert one(t * (1 + 1e-4) + 1e-30)
        assert var[i] == 0 or not one(t * (1 - 1e-4))


def test_variance_of_mean_edge_cases():
    one = variance_of_mean(np.array([0.5], np.float32), np.array([0.25], np.float32), np.array([1]))
    assert one[0] == f32(-1)
    const = variance_of_mean(np.array([0.25 * 8], np.float32), np.array([0.0625 * 8], np.float32), np.array([8]))
    assert const[0] == 0
    nan = variance_of_mean(np.array([np.nan], np.float32), np.array([np.nan], np.float32), np.array([5]))
    assert nan[0] == 0  # d > 0 is false for NaN, as in the stopping rule


def test_adaptive_with_variance_over_synthetic_frames():
    rng = np.random.default_rng(8)
    base = rng.uniform(0, 0.8, (500, 3)).astype(np.float32)
    noise = rng.uniform(0, 0.5, 500).astype(np.float32)
    frames = [(base + noise[:, None] * rng.normal(size=(500, 3))).astype(np.float32) for _ in range(12)]
    frames[0][7] = np.nan
    mean, b, n, var = adaptive_with_variance(lambda k: frames[k], 2, 12, 0.1)
    assert n.min() >= 2 and n.max() == 12 and n.min() < 12
    assert var[7] == 0 and (var >= 0).all()
    _, _, n1, var1 = adaptive_with_variance(lambda k: frames[k], 1, 1, 0.1)
    assert (n1 == 1).all() and (var1 == -1).all()
