"""Adaptive frames denoised under their measured variance on the MI355X (include/skr.h skr_render_adaptive_var, skr_denoise_var,
skr_render_adaptive_denoised_host), bit for bit: the variance image against the numpy rule over the renderer's own
frames, the filter against the C checker (tests/denoise_var_checker.c) on real and synthetic inputs, the one-call sequence against its
three steps, both command lines, the argument errors, no side effects, and the quality against a 256-pass mean."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import skele_raytracer_amd as skr
from conftest import ROOT, read_ppm_bytes, scene_path
from denoise_check import random_frame, random_guides
from denoise_var_check import adaptive_with_variance, build as build_checker, random_variance
from skele_raytracer_amd import DENOISE_VAR_SIGMA_L  # noqa: F401  (the feature: without it nothing below means anything)

pytestmark = pytest.mark.gpu

_renderers = {}


def renderer(scn):
    if scn not in _renderers:
        _renderers[scn] = skr.Renderer(skr.parse_scene(scene_path(scn)), 0)
    return _renderers[scn]


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    return build_checker(str(tmp_path_factory.mktemp("denoise_var_gpu")))


def host(t):
    torch.cuda.synchronize()
    return None if t is None else t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def guide_options(opt):
    """opt with jsample 0: the pixel centres."""
    g = skr.Options(opt.width, opt.height)
    C.memmove(C.byref(g.c), C.byref(opt.c), C.sizeof(opt.c))
    g.c.grid_size = 0
    return g


def guides(r, opt):
    return r.trace(r.camera_rays(guide_options(opt)).view(-1, 8))


def gpu_frames(r, kw, w, h, seed):
    cache = {}

    def frame(k):
        if k not in cache:
            _, f = r.render(skr.Options(w, h, seed=seed + k, **kw), want_float=True)
            cache[k] = host(f).reshape(-1, 3)
        return cache[k]
    return frame


# ---- render_adaptive(want_variance=True) ----
@pytest.mark.parametrize("wh", [(48, 27), (97, 61)])
@pytest.mark.parametrize("scn,kw", [("spheres2.scn", dict(gillum=4, shadow=True)), ("test.scn", dict(gillum=4, depth=3, shadow=True))])
def test_variance_is_the_rule_and_moves_nothing_else(scn, kw, wh, monkeypatch):
    r = renderer(scn)
    w, h = wh
    lo, hi, t, seed = 2, 7, 0.08, 3
    opt = skr.Options(w, h, seed=seed, **kw)
    mean, b, n, var = adaptive_with_variance(gpu_frames(r, kw, w, h, seed), lo, hi, t)
    assert n.min() < hi and n.max() > lo and (var > 0).any()
    for path in ("frame", "query", None):
        if path:
            monkeypatch.setenv("SKR_ADAPTIVE_PATH", path)
        else:
            monkeypatch.delenv("SKR_ADAPTIVE_PATH", raising=False)
        rgb0, f0, n0 = r.render_adaptive(opt, t, lo, hi, want_float=True)
        rgb1, f1, n1, v1 = r.render_adaptive(opt, t, lo, hi, want_float=True, want_variance=True)
        what = "%s %dx%d path=%s" % (scn, w, h, path)
        assert v1.shape == (h, w) and v1.dtype == torch.float32
        assert torch.equal(rgb0, rgb1) and torch.equal(f0.view(torch.int32), f1.view(torch.int32)) and torch.equal(n0, n1), what
        assert np.array_equal(host(n1).reshape(-1), n) and np.array_equal(bits(host(f1)), bits(mean)) and np.array_equal(host(rgb1).reshape(-1, 3), b), what
        assert np.array_equal(bits(host(v1)), bits(var)), what
        only_var = r.render_adaptive(opt, t, lo, hi, want_variance=True)
        assert only_var[1] is None and np.array_equal(bits(host(only_var[3])), bits(var)), what


def test_one_pass_is_not_measured():
    r = renderer("spheres2.scn")
    _, _, n, var = r.render_adaptive(skr.Options(97, 61, gillum=2, seed=4), 0.05, 1, 1, want_variance=True)
    assert (host(n) == 1).all() and (host(var) == np.float32(-1)).all()
    _, _, n, var = r.render_adaptive(skr.Options(97, 61, gillum=2, seed=4), 0.05, 2, 2, want_variance=True)
    assert (host(n) == 2).all() and (host(var) >= 0).all()


# ---- denoise(variance=...) ----
def assert_same(gpu_rgb, gpu_f, ref_rgb, ref_f, what):
    gf = host(gpu_f)
    bad = gf.view(np.uint32) != ref_f.view(np.uint32)
    assert not bad.any(), "%s: %d float words differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[:3].tolist())
    assert np.array_equal(host(gpu_rgb), ref_rgb), what


FRAMES = {
    "spheres2": ("spheres2.scn", dict(gillum=4, shadow=True)),
    "bear": ("bear.scn", dict(gillum=4, shadow=True)),
    "dragon": ("dragon.scn", dict(gillum=2, depth=2, shade_triangles=True)),  # (without shaded triangles the dragon has no Monte-Carlo term)
}


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_gpu_equals_checker_on_adaptive_frames(chk, name):
    scn, kw = FRAMES[name]
    r = renderer(scn)
    opt = skr.Options(160, 90, seed=3, **kw)
    _, rgbf, n, var = r.render_adaptive(opt, 0.1, 2, 6, want_float=True, want_variance=True)
    hits = guides(r, opt)
    c, g, v = host(rgbf), host(hits.raw), host(var)
    assert (v >= 0).all() and (v > 0).any() and len(np.unique(host(hits.kind))) >= 2
    mixed = v.copy()  # and with unmeasured pixels among the measured ones
    mixed[::3, 1::2] = -1
    mixed[5, :] = np.nan
    for L in (0, 1, 5, 16):
        for tag, vv in (("measured", v), ("mixed", mixed)):
            rgb, out = r.denoise(rgbf, hits, L, variance=torch.from_numpy(vv).cuda())
            ref_rgb, ref_f = chk.denoise(c, g, vv, L)
            assert_same(rgb, out, ref_rgb, ref_f, "%s %s L=%d" % (name, tag, L))
        want_rgb, want = r.denoise(rgbf, hits, L)
        for tag, vv in (("none", None), ("all -1", torch.full((90, 160), -1.0, device="cuda"))):
            rgb, out = r.denoise(rgbf, hits, L, variance=vv)
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(rgb, want_rgb), (name, tag, L)
    _, out5 = r.denoise(rgbf, hits, 5, variance=var)
    assert not torch.equal(out5, r.denoise(rgbf, hits, 5)[1]), "the measured variance must change the filter"


@pytest.mark.parametrize("h,w", [(1, 1), (3, 257), (17, 13)])
@pytest.mark.parametrize("L", [0, 1, 5, 16])
def test_gpu_equals_checker_on_synthetic_inputs(chk, h, w, L):
    r = renderer("spheres2.scn")
    seed = 7 * h + w
    g, c = random_guides(h, w, seed), random_frame(h, w, seed)
    v = random_variance(g, h, w, seed)
    rgb, out = r.denoise(torch.from_numpy(c).cuda(), torch.from_numpy(g).cuda(), L, variance=torch.from_numpy(v).cuda())
    ref_rgb, ref_f = chk.denoise(c, g, v, L)
    assert_same(rgb, out, ref_rgb, ref_f, "%dx%d L=%d" % (h, w, L))


# ---- the one-call sequence ----
def three_steps(r, opt, t, lo, hi, L):
    _, rgbf, n, var = r.render_adaptive(opt, t, lo, hi, want_float=True, want_variance=True)
    rgb, out = r.denoise(rgbf, guides(r, opt), L, variance=var)
    return host(rgb), host(out), host(n)


@pytest.mark.parametrize("jsample", [0, 2])
def test_render_adaptive_denoised_equals_the_three_steps(jsample):
    r = renderer("spheres2.scn")
    opt = skr.Options(200, 112, gillum=4, shadow=True, jsample=jsample, seed=6)
    want_rgb, want_f, want_n = three_steps(r, opt, 0.1, 2, 8, 5)
    assert want_n.min() < want_n.max()
    rgb, f, n, ms = r.render_adaptive_denoised(opt, 0.1, 2, 8, 5, want_float=True)
    assert ms > 0
    assert np.array_equal(n, want_n) and np.array_equal(bits(f), bits(want_f)) and np.array_equal(rgb, want_rgb)
    only_rgb, none, n2, _ = r.render_adaptive_denoised(opt, 0.1, 2, 8, 5)
    assert none is None and np.array_equal(only_rgb, want_rgb) and np.array_equal(n2, want_n)
    # the C entry with single outputs: the pass counts alone, the float frame alone
    a = skr.adaptive_params(0.1, 2, 8)
    alone_n = np.zeros((112, 200), np.uint32)
    alone_f = np.zeros((112, 200, 3), np.float32)
    L = skr.lib()
    assert L.skr_render_adaptive_denoised_host(r.h, C.byref(opt.c), C.byref(a), 5, None, None, alone_n.ctypes.data, None) == 0
    assert L.skr_render_adaptive_denoised_host(r.h, C.byref(opt.c), C.byref(a), 5, None, alone_f.ctypes.data, None, None) == 0
    assert np.array_equal(alone_n, want_n) and np.array_equal(bits(alone_f), bits(want_f))
    # iterations 0: the adaptive frame itself
    rgb0, f0, n0, _ = r.render_adaptive_denoised(opt, 0.1, 2, 8, 0, want_float=True)
    a_rgb, a_f, a_n = r.render_adaptive(opt, 0.1, 2, 8, want_float=True)
    assert np.array_equal(bits(f0), bits(host(a_f))) and np.array_equal(rgb0, host(a_rgb)) and np.array_equal(n0, host(a_n))


def _read_pfm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], "<f4", w * h * 3).reshape(h, w, 3)[::-1]


def test_both_command_lines(tmp_path, capsys):
    from skele_raytracer_amd import render_cli
    scn = scene_path("spheres2.scn")
    W, H = 200, 120
    r = renderer("spheres2.scn")
    want_rgb, want_f, want_n, _ = r.render_adaptive_denoised(skr.Options(W, H, gillum=4, shadow=True, seed=5), 0.1, 3, 12, 5, want_float=True)
    base = ["--path", scn, "--width", str(W), "--height", str(H), "--gillum", "4", "--shadow", "--seed", "5"]
    args = base + ["--adaptive", "0.1", "--adaptive-min", "3", "--adaptive-max", "12", "--adaptive-denoise", "5"]
    exe = os.path.join(ROOT, "bin", "raytracer")

    def native(a, out):
        p = subprocess.run([exe, *a, "--output", out, "--quiet"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        return p.returncode, p.stderr

    def py_process(a, out):
        p = subprocess.run([sys.executable, "-m", "skele_raytracer_amd.render_cli", *a, "--output", out], cwd=ROOT, capture_output=True, text=True, timeout=300)
        return p.returncode, p.stderr

    def py_main(a, out):  # the same entry in this process (the module's __main__ is sys.exit(main())): no interpreter start per case
        rc = render_cli.main([*a, "--output", out])
        return rc, capsys.readouterr().err

    for tag, run, run_more in (("native", native, native), ("py", py_process, py_main)):
        ppm, pfm, x = str(tmp_path / (tag + ".ppm")), str(tmp_path / (tag + ".pfm")), str(tmp_path / "x.ppm")
        rc, err = run(args, ppm)
        assert rc == 0, (tag, err)
        assert "passes per pixel" in err and "%.3f" % want_n.mean() in err, (tag, err)
        assert np.array_equal(read_ppm_bytes(open(ppm, "rb").read()).reshape(-1), want_rgb.reshape(-1)), tag
        rc, err = run_more(args + ["--format", "pfm"], pfm)
        assert rc == 0, (tag, err)
        assert np.array_equal(bits(_read_pfm(pfm)), bits(want_f)), tag
        for bad, word in ((base + ["--adaptive-denoise", "5"], "--adaptive"),                                   # needs --adaptive
                          (args + ["--denoise", "5"], "--denoise"),
                          (base + ["--adaptive", "0.1", "--denoise", "5"], "--adaptive"),                       # still refused
                          (base + ["--adaptive", "0.1", "--adaptive-denoise", "17"], "--adaptive-denoise"),
                          (args + ["--progressive", "3"], "--adaptive"), (args + ["--progressive-every", "2"], "--adaptive")):
            rc, err = run_more(bad, x)
            assert rc != 0 and word in err, (tag, bad, err)
    rc, err = native(args + ["--gpus", "2"], str(tmp_path / "x.ppm"))
    assert rc != 0 and "--adaptive" in err


def test_uniform_sampling_with_measured_variance():
    """--adaptive -1 --adaptive-min K --adaptive-max K is --progressive K; with the filter it carries the variance of those K passes."""
    r = renderer("spheres2.scn")
    opt = skr.Options(160, 90, gillum=4, shadow=True, seed=2)
    _, rgbf, n, var = r.render_adaptive(opt, -1.0, 4, 4, want_float=True, want_variance=True)
    _, prog = r.render(skr.Options(160, 90, gillum=4, shadow=True, seed=2, progressive=4), want_float=True)
    assert (host(n) == 4).all() and torch.equal(rgbf.view(torch.int32), prog.view(torch.int32)) and (host(var) >= 0).all()
    rgb, f, _, _ = r.render_adaptive_denoised(opt, -1.0, 4, 4, 5, want_float=True)
    want_rgb, want = r.denoise(prog, guides(r, opt), 5, variance=var)
    assert np.array_equal(bits(f), bits(host(want))) and np.array_equal(rgb, host(want_rgb))


def test_argument_errors():
    L = skr.lib()
    r = renderer("spheres2.scn")
    h, w = 8, 16
    c = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    g = torch.zeros((h * w, 8), dtype=torch.float32, device="cuda")
    v = torch.zeros((h * w + 64,), dtype=torch.float32, device="cuda")
    o = torch.zeros((h * w * 3 + 64,), dtype=torch.float32, device="cuda")
    b = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    dn = lambda *a: L.skr_denoise_var(r.h, *a, None)
    assert dn(w, h, c.data_ptr(), g.data_ptr(), v.data_ptr(), 5, o.data_ptr(), b.data_ptr()) == 0
    assert dn(w, h, c.data_ptr(), g.data_ptr(), None, 5, o.data_ptr(), None) == 0
    bad = [
        (w, h, c.data_ptr(), g.data_ptr(), v.data_ptr() + 2, 5, o.data_ptr(), None),       # misaligned variance
        (w, h, c.data_ptr(), g.data_ptr(), o.data_ptr(), 5, o.data_ptr(), None),           # the float output over the variance
        (w, h, c.data_ptr(), g.data_ptr(), o.data_ptr() + 64, 5, o.data_ptr(), None),      # overlapping it
        (w, h, c.data_ptr(), g.data_ptr(), v.data_ptr(), 5, None, v.data_ptr() + 16),      # the bytes over the variance
        (w, h, c.data_ptr(), g.data_ptr(), v.data_ptr(), 17, o.data_ptr(), None),          # iterations
        (w, h, c.data_ptr(), g.data_ptr(), v.data_ptr(), 5, None, None),                   # no output
        (w, h, None, g.data_ptr(), v.data_ptr(), 5, o.data_ptr(), None),                   # no frame
        (w, h, c.data_ptr(), g.data_ptr() + 4, v.data_ptr(), 5, o.data_ptr(), None),       # misaligned guides
        (0, h, c.data_ptr(), g.data_ptr(), v.data_ptr(), 5, o.data_ptr(), None),           # size
        (w, h, c.data_ptr(), g.data_ptr(), v.data_ptr(), 5, c.data_ptr(), None),           # in place
    ]
    for a in bad:
        assert dn(*a) == 2, a
    with pytest.raises(skr.SkrError, match="variance"):
        r.denoise(c, g, 5, variance=v[:h * w].view(w, h))
    opt = skr.Options(w, h, gillum=2, seed=1)
    a = skr.adaptive_params(0.1, 1, 4)
    n = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    ad = lambda *x: L.skr_render_adaptive_var(r.h, C.byref(opt.c), C.byref(a), *x, None)
    assert ad(None, None, None, v.data_ptr()) == 0  # the variance alone is an output
    assert ad(None, None, None, None) == 2          # all four NULL
    assert ad(None, None, n.data_ptr(), v.data_ptr() + 2) == 2
    assert L.skr_render_adaptive(r.h, C.byref(opt.c), C.byref(a), None, None, None, None) == 2
    hn = np.zeros((h, w), np.uint32)
    hostcall = lambda it, *x: L.skr_render_adaptive_denoised_host(r.h, C.byref(opt.c), C.byref(a), it, *x, None)
    assert hostcall(5, None, None, hn.ctypes.data) == 0
    assert hostcall(17, None, None, hn.ctypes.data) == 2
    assert hostcall(5, None, None, None) == 2
    with pytest.raises(skr.SkrError, match="min_passes"):
        r.render_adaptive_denoised(opt, 0.1, 5, 4, 5)
    with pytest.raises(skr.SkrError, match="progressive"):
        r.render_adaptive_denoised(skr.Options(w, h, gillum=2, progressive=2), 0.1, 1, 4, 5)
    with pytest.raises(skr.SkrError, match="depth"):
        r.render_adaptive_denoised(skr.Options(w, h, gillum=2, depth=0), 0.1, 1, 4, 5)
    torch.cuda.synchronize()


def test_the_sequence_changes_nothing_a_render_reads():
    r = skr.Renderer(skr.parse_scene(scene_path("spheres2.scn")), 0)
    opt = skr.Options(320, 180, gillum=4, shadow=True)
    r.counters(reset=True)
    a, af = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    ca, va = r.counters(reset=True), r.kernel_variant()
    small = skr.Options(160, 90, gillum=2, seed=1)
    first = r.render_adaptive_denoised(small, 0.1, 2, 5, 5, want_float=True)
    _, rgbf, n, var = r.render_adaptive(small, 0.1, 2, 5, want_float=True, want_variance=True)
    hits = guides(r, small)
    torch.cuda.synchronize()
    r.counters(reset=True)
    v0 = r.kernel_variant()
    r.denoise(rgbf, hits, 5, variance=var)  # the filter alone: no counter, no variant
    torch.cuda.synchronize()
    assert r.counters(reset=True) == {k: 0 for k in ca} and r.kernel_variant() == v0
    r.render_adaptive_denoised(skr.Options(200, 120, gillum=2, seed=1), 0.1, 2, 5, 3)  # (the scratch grows, then is reused smaller)
    again = r.render_adaptive_denoised(small, 0.1, 2, 5, 5, want_float=True)
    assert np.array_equal(first[0], again[0]) and np.array_equal(bits(first[1]), bits(again[1])) and np.array_equal(first[2], again[2])
    r.counters(reset=True)
    b, bf = r.render(opt, want_float=True)
    torch.cuda.synchronize()
    assert r.counters(reset=True) == ca and r.kernel_variant() == va
    assert torch.equal(a, b) and torch.equal(af.view(torch.int32), bf.view(torch.int32))


# ---- quality ----
def _mse(x, ref):
    return float(np.mean((np.minimum(x, 1) - np.minimum(ref, 1)) ** 2))


# bound: the N / A ratio measured on the MI355X x 1.5, rounded up to two digits (the ratio moves with the seed; the project's other
# quality bounds leave the same kind of margin: 0.62 -> 0.8, 0.150 -> 0.40).  Measured at seed 1 (seeds 2 and 3 in brackets):
#   spheres2  N/A 0.4453 (0.4454, 0.4490)  B/A 0.6530  N/B 0.682   -> bound 0.67
#   bear      N/A 0.1349 (0.1362, 0.1353)  B/A 0.1360  N/B 0.992   -> bound 0.21
# SKR_DENOISE_VAR_SIGMA_L = 4 has the lowest sum of the two N/A ratios: 2 -> 0.4318 + 0.1786, 4 -> 0.4453 + 0.1349, 8 -> 0.5765 + 0.1413.
QUALITY = [("spheres2.scn", dict(gillum=4, shadow=True, depth=3), 0.67), ("bear.scn", dict(gillum=8, shadow=True), 0.21)]


@pytest.mark.parametrize("scn,kw,bound", QUALITY)
def test_quality_against_a_256_pass_mean(scn, kw, bound):
    """A = the raw adaptive mean, B = A through denoise (the spatial variance), N = the new sequence (the measured variance)."""
    w, h = 480, 270
    r = skr.Renderer(skr.parse_scene(scene_path(scn)), 0)
    ref = host(r.render(skr.Options(w, h, seed=1000, progressive=256, **kw), want_float=True)[1]).astype(np.float64)
    opt = skr.Options(w, h, seed=1, **kw)
    lo, hi, t = skr.ADAPTIVE_MIN_PASSES, skr.ADAPTIVE_MAX_PASSES, skr.ADAPTIVE_THRESHOLD
    _, fa, n, var = r.render_adaptive(opt, t, lo, hi, want_float=True, want_variance=True)
    hits = guides(r, opt)
    _, fb = r.denoise(fa, hits, 5)
    _, fn = r.denoise(fa, hits, 5, variance=var)
    _, seq, _, _ = r.render_adaptive_denoised(opt, t, lo, hi, 5, want_float=True)
    assert np.array_equal(bits(seq), bits(host(fn)))
    ma, mb, mn = (_mse(host(x).astype(np.float64), ref) for x in (fa, fb, fn))
    print("\nquality %s: mean passes %.3f, mse A (adaptive) %.6g, B (spatial variance) %.6g, N (measured variance) %.6g; N/A %.4f, B/A %.4f, N/B %.4f"
          % (scn, host(n).mean(), ma, mb, mn, mn / ma, mb / ma, mn / mb))
    assert mn < ma, "the filter must not cost accuracy"
    assert bound < 1 and mn <= bound * ma, (mn / ma, bound)
