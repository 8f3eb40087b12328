"""CPU checks of adaptive sampling (include/skr.h skr_render_adaptive): the public surface is declared and exported, the
binding's defaults are the header's, and the numpy restatement of the rule (tests/adaptive_check.py) keeps the rule's consequences on
hand-made pass sequences."""
import os
import re
import subprocess

import numpy as np
import pytest

import skele_raytracer_amd as skr
from adaptive_check import LUM_FLOOR, adaptive, lum
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "skr.h")).read()


def define(name):
    m = re.search(r"#define %s\s+([^\s/]+)" % name, HEADER)
    assert m, name
    return float(m.group(1).rstrip("f"))


def test_adaptive_surface_declared_and_exported():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("skr_render_adaptive", "skr_render_adaptive_host"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in skr.EXPORTED_SYMBOLS
    assert re.search(r"\bvoid\s+skr_adaptive_default\s*\(\s*skr_adaptive\s*\*", code)
    assert re.search(r"typedef struct\s*\{\s*int32_t min_passes, max_passes;\s*float threshold;[^}]*int32_t reserved;[^}]*\}\s*skr_adaptive;", code)
    assert re.search(r"#define SKR_HAS_ADAPTIVE 1\b", HEADER)
    assert re.search(r"#define SKR_ABI_VERSION 7\b", HEADER)
    out = subprocess.check_output(["nm", "-D", "--defined-only", skr.lib_path()], text=True)
    exported = set(re.findall(r" T (skr_[a-z0-9_]+)", out))
    assert {"skr_adaptive_default", "skr_render_adaptive", "skr_render_adaptive_host"} <= exported
    assert callable(skr.Renderer.render_adaptive) and callable(skr.Renderer.render_adaptive_host)


def test_binding_defaults_are_the_headers():
    assert np.float32(define("SKR_ADAPTIVE_LUM_FLOOR")) == np.float32(skr.ADAPTIVE_LUM_FLOOR) == LUM_FLOOR == np.float32(2.0 ** -8)
    assert define("SKR_ADAPTIVE_MIN_PASSES") == skr.ADAPTIVE_MIN_PASSES
    assert define("SKR_ADAPTIVE_MAX_PASSES") == skr.ADAPTIVE_MAX_PASSES
    assert np.float32(define("SKR_ADAPTIVE_THRESHOLD")) == np.float32(skr.ADAPTIVE_THRESHOLD)
    assert define("SKR_ADAPTIVE_PASS_LIMIT") == skr.ADAPTIVE_PASS_LIMIT == 65535
    import ctypes as C
    a = skr.binding.CAdaptive()
    skr.lib().skr_adaptive_default(C.byref(a))  # (libskr's own defaults: no device needed)
    assert (a.min_passes, a.max_passes, np.float32(a.threshold), a.reserved) == (skr.ADAPTIVE_MIN_PASSES, skr.ADAPTIVE_MAX_PASSES,
                                                                                np.float32(skr.ADAPTIVE_THRESHOLD), 0)


def noisy(seed, n=64, mean=0.5, rel=0.3):
    rng = np.random.default_rng(seed)
    return lambda k: (mean * (1 + rel * np.random.default_rng([seed, k]).standard_normal((n, 3)))).astype(np.float32)


def test_lum_is_left_to_right_binary32():
    v = np.array([[0.1, 0.7, 0.3]], np.float32)
    want = np.float32(np.float32(np.float32(0.2126) * v[0, 0]) + np.float32(np.float32(0.7152) * v[0, 1]))
    want = np.float32(want + np.float32(np.float32(0.0722) * v[0, 2]))
    assert lum(v)[0] == want


@pytest.mark.parametrize("lo,hi", [(1, 10), (2, 10), (5, 10), (7, 7)])
def test_constant_passes_stop_at_max_2_min(lo, hi):
    v = np.random.default_rng(3).uniform(0, 1, (40, 3)).astype(np.float32)
    mean, b, n = adaptive(lambda k: v, lo, hi, 0.01)
    assert (n == min(max(2, lo), hi)).all()
    acc = v.copy()
    for k in range(1, int(n[0])):
        acc = acc + v
    assert np.array_equal(mean.view(np.uint32), (acc / np.float32(n[0])).view(np.uint32))


def test_negative_threshold_never_stops_and_is_progressive():
    f = noisy(1)
    mean, _, n = adaptive(f, 2, 9, -1.0)
    assert (n == 9).all()
    acc = f(0).copy()
    for k in range(1, 9):
        acc = acc + f(k)
    assert np.array_equal(mean.view(np.uint32), (acc / np.float32(9)).view(np.uint32))


def test_min_equals_max_is_progressive():
    f = noisy(2)
    mean, b, n = adaptive(f, 6, 6, 0.0)
    assert (n == 6).all()
    acc = f(0).copy()
    for k in range(1, 6):
        acc = acc + f(k)
    assert np.array_equal(mean.view(np.uint32), (acc / np.float32(6)).view(np.uint32))


def test_infinite_threshold_stops_everything_at_max_2_min():
    for lo in (1, 2, 4):
        _, _, n = adaptive(noisy(3), lo, 20, np.inf)
        assert (n == max(2, lo)).all()


def test_min_one_still_takes_two_passes_unless_max_is_one():
    _, _, n = adaptive(noisy(4), 1, 1, 0.5)
    assert (n == 1).all()
    _, _, n = adaptive(noisy(4), 1, 5, 1e9)
    assert (n == 2).all()


def test_nan_passes_stop_like_constant_ones():
    # d = NaN fails d > 0, so var = 0 and e2 = 0 <= b * b (b from the floor, as m = NaN fails m > floor): the rule as written stops a
    # NaN pixel at max(2, min), and its mean stays NaN
    def f(k):
        v = np.full((8, 3), 0.25 + 0.01 * (k % 2), np.float32)
        v[3] = np.nan
        return v
    mean, b, n = adaptive(f, 3, 12, 1e-6)
    assert n[3] == 3 and (np.delete(n, 3) == 12).all()
    assert np.isnan(mean[3]).all() and (b[3] == 255).all()  # quantise: NaN -> 255


def test_the_floor_stops_dark_pixels_on_absolute_noise():
    # a dark pixel and a bright one with the same relative noise: only the dark one is under the floor's absolute bound
    rel = lambda mean: (lambda k: np.full((1, 3), mean * (1.5 if k % 2 else 0.5), np.float32))
    _, _, n_dark = adaptive(rel(1e-4), 2, 30, 0.05)
    _, _, n_bright = adaptive(rel(0.5), 2, 30, 0.05)
    assert n_dark[0] == 2 and n_bright[0] == 30


def test_the_active_set_only_shrinks_and_passes_lie_in_range():
    f = noisy(6, 500, rel=0.5)
    for lo, hi, t in ((1, 16, 0.05), (3, 24, 0.02), (8, 8, 0.1), (2, 40, 0.1)):
        _, _, n = adaptive(f, lo, hi, t)
        assert n.min() >= min(max(2, lo), hi) and n.max() <= hi
