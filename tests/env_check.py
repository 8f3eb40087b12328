"""The CPU checker of the environment map (tests/env_checker.c; include/skr.h skr_scene_set_environment): compiled once
per session with the oracle's flags.  The C file looks the environment up and shades rays, on a scene in motion where asked; a frame is
composed here, per aa in aa order from the lens checker's rays, exactly as lens_check.Checker.render and motion_check.Checker.render
compose one.  `exact_taps` restates the lookup's index rule in exact rational arithmetic, rounded to nearest-even per step.  Test
infrastructure; the product never loads it."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np

from motion_check import in_force
from oracle import pyoracle
from shade_query_check import _flags, oracle_options
from soft_light_check import _radii
from spot_check import ORACLE_DIR, TESTS, _scene, _spots

ENV_MAX_EDGE = 4096  # include/skr.h SKR_ENV_MAX_EDGE


def build(out_dir):
    """The checker into out_dir (it includes tests/motion_checker.c and with it the lens, soft-light and spot checkers and
    oracle/skr_oracle.c whole: no liboracle)."""
    pyoracle.lib()
    so = os.path.join(out_dir, "libenvcheck.so")
    subprocess.check_call(["gcc", *_flags(), "-I" + ORACLE_DIR, "-I" + TESTS, "-shared", "-o", so, os.path.join(TESTS, "env_checker.c"), "-lm"])
    L = C.CDLL(so)
    L.env_records.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.env_records.restype = None
    L.env_lookup.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.env_lookup.restype = C.c_int
    L.lens_rays.argtypes = [C.POINTER(pyoracle.Scene), C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint32, C.c_float, C.c_float, C.c_void_p]
    L.lens_rays.restype = None
    L.env_shade_rays.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                                 C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.env_shade_rays.restype = C.c_int
    return Checker(L)


def records(d, E):
    """uint32 [n, 4] = (d(3), E): the input of skr_debug_eval's op 25."""
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    rec = np.zeros((len(d), 4), np.uint32)
    rec[:, :3] = d.view(np.uint32)
    rec[:, 3] = E
    return rec


# ---- the rule restated exactly: every step computed in rationals from the binary32 operands, then rounded to nearest-even ----
def _rn(q):
    """The binary32 nearest to the rational q, ties to even, as a Fraction (inf: None).  q's sign is kept for a zero result by the callers
    that need it (none does: the rule's comparisons read < 0 only, and -0 is not < 0)."""
    if q == 0:
        return Fraction(0)
    sign = -1 if q < 0 else 1
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, -126)  # subnormals: the spacing of the smallest binade
    ulp = Fraction(2) ** (e - 23)
    n = a / ulp
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    r = fl * ulp
    if r >= Fraction(2) ** 128:
        return None
    return sign * r


def exact_taps(d, E):
    """(flag, i0, i1, j0, j1, fx, fy) of include/skr.h's steps 1-5 for one direction d (three binary32 values): flag 1 = the background
    arm (then the rest is 0); fx, fy as np.float32."""
    d = [np.float32(x) for x in d]
    if not all(math.isfinite(float(x)) for x in d):
        return (1, 0, 0, 0, 0, np.float32(0), np.float32(0))
    dx, dy, dz = (Fraction(float(x)) for x in d)
    s = _rn(abs(dx) + abs(dy))
    s = None if s is None else _rn(s + abs(dz))
    if s is None or not s > 0:
        return (1, 0, 0, 0, 0, np.float32(0), np.float32(0))
    px, pz = _rn(dx / s), _rn(dz / s)
    if dy < 0:
        qx = _rn(_rn(1 - abs(pz)) * (-1 if px < 0 else 1))
        qz = _rn(_rn(1 - abs(px)) * (-1 if pz < 0 else 1))
    else:
        qx, qz = px, pz
    out = []
    for q in (qx, qz):
        u = _rn(_rn(q * Fraction(1, 2)) + Fraction(1, 2))
        x = _rn(_rn(u * E) - Fraction(1, 2))
        x0 = Fraction(math.floor(x))
        f = _rn(x - x0)
        clamp = lambda i: min(max(i, 0), E - 1)
        out.append((clamp(int(x0)), clamp(int(x0) + 1), np.float32(float(f))))
    return (0, out[0][0], out[0][1], out[1][0], out[1][1], out[0][2], out[1][2])


def octa_decode(u, v):
    """float64: the direction whose octahedral coordinates are (u, v) in [0, 1]^2 — the inverse of steps 2-4 (world +y at the centre)."""
    qx, qz = 2.0 * u - 1.0, 2.0 * v - 1.0
    y = 1.0 - abs(qx) - abs(qz)
    if y >= 0:
        return np.array([qx, y, qz])
    sx, sz = (-1.0 if qx < 0 else 1.0), (-1.0 if qz < 0 else 1.0)
    return np.array([(1.0 - abs(qz)) * sx, y, (1.0 - abs(qx)) * sz])


class Checker:
    def __init__(self, lib):
        self.lib = lib

    def taps(self, d, E):
        """uint32 [n, 7] = (flag, i0, i1, j0, j1, fx bits, fy bits) of directions d [n, 3]: env_records."""
        rec = records(d, E)
        out = np.zeros((len(rec), 7), np.uint32)
        self.lib.env_records(rec.ctypes.data, len(rec), out.ctypes.data)
        return out

    def lookup(self, texels, d, background=(0, 0, 0)):
        """float32 [n, 3] = env(d) for directions d [n, 3] on the map texels [E, E, 3]."""
        t = np.ascontiguousarray(texels, np.float32)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        bg = np.ascontiguousarray(background, np.float32)
        out = np.zeros_like(d)
        for i in range(len(d)):
            self.lib.env_lookup(t.ctypes.data, t.shape[0], d[i:i + 1].ctypes.data, bg.ctypes.data, out[i:i + 1].ctypes.data)
        return out

    def rays(self, scene, width, height, *, aperture=0.0, focus=1.0, fov=60.0, jsample=0, seed=1, sample=0, strict=False):
        """float32 [h * w, 8]: the primary rays of AA sample `sample` of the frame under the lens (A = 0: the pinhole); keys y * w + x."""
        sc = _scene(scene, strict)
        rays = np.zeros((height * width, 8), np.float32)
        self.lib.lens_rays(C.byref(sc.s), width, height, fov, int(jsample > 0), seed, sample, C.c_float(float(np.float32(aperture))),
                           C.c_float(float(np.float32(focus))), rays.ctypes.data)
        return rays

    def shade(self, scene, rays, *, environment=None, velocities=None, shutter=1.0, radii=None, spots=None, cones=None, triangle_shadows=False, sample=0, keys=None,
              strict=False, **opt):
        """(float32 [n, 3], stats uint64[7]: pyoracle.render's five, then the lookups at level 0 and at levels >= 1) for rays float32
        [n, 8] on the scene with the environment [E, E, 3] (None: none), in motion where the rule says so."""
        sc = _scene(scene, strict)
        s, c = _spots(spots, cones)
        rd = _radii(sc, len(s), radii, opt.get("legacy_reflect"))
        o = oracle_options(**opt)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(-1)
        force = in_force(velocities, shutter)
        v = np.ascontiguousarray(velocities if force else np.zeros((sc.s.n_spheres, 3)), np.float32).reshape(-1, 3)
        if len(v) != sc.s.n_spheres:
            raise ValueError("%d velocities, %d spheres" % (len(v), sc.s.n_spheres))
        t = None if environment is None else np.ascontiguousarray(environment, np.float32)
        if t is not None and (t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3):
            raise ValueError("environment: [E, E, 3]")
        out = np.zeros((len(r), 3), np.float32)
        stats = np.zeros(7, np.uint64)
        rc = self.lib.env_shade_rays(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), len(s), s.ctypes.data, c.ctypes.data, rd.ctypes.data, v.ctypes.data,
                                     C.c_float(float(np.float32(shutter))), int(force), None if t is None else t.ctypes.data, 0 if t is None else t.shape[0], r.ctypes.data,
                                     len(r), sample, None if k is None else k.ctypes.data, out.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("env_shade_rays failed: %d" % rc)
        return out, stats

    def render_samples(self, scene, width, height, *, aperture=0.0, focus=1.0, fov=60.0, jsample=0, seed=1, strict=False, **kw):
        """[(float32 [h * w, 3], stats)] per aa: the samples a frame sums."""
        sc = _scene(scene, strict)
        keys = np.arange(width * height, dtype=np.uint32)
        g2 = jsample * jsample if jsample > 0 else 1
        return [self.shade(sc, self.rays(sc, width, height, aperture=aperture, focus=focus, fov=fov, jsample=jsample, seed=seed, sample=aa), sample=aa, keys=keys,
                           seed=seed, **kw) for aa in range(g2)]

    def render(self, scene, width, height, *, jsample=0, **kw):
        """(rgb uint8 [h, w, 3], float32 [h, w, 3], stats uint64[7]) of the frame: per aa the (lens) rays shaded with keys y * w + x and
        sample aa, summed in aa order and divided by (float) (g * g), exactly as sko_render does.  kw: environment, aperture, focus,
        velocities, shutter, radii, spots, cones, triangle_shadows, strict and the options of shade_query_check.oracle_options."""
        stats = np.zeros(7, np.uint64)
        px = None
        for c, st in self.render_samples(scene, width, height, jsample=jsample, **kw):
            stats += st
            if jsample > 0:
                px = (np.zeros_like(c) + c) if px is None else px + c  # (0, 0, 0) + the first sample, as the render loop starts
            else:
                px = c
        if jsample > 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                px = px / np.float32(jsample * jsample)
        f = px.reshape(height, width, 3).astype(np.float32)
        return pyoracle.quantise(f), f, stats

    def render_progressive(self, scene, width, height, passes, *, seed=1, **kw):
        """--progressive K: K frames under the seeds seed .. seed + K - 1 summed in that order, / (float) K once
        (pyoracle.render_progressive's steps).  Returns (rgb, mean, summed stats)."""
        sc = _scene(scene, kw.get("strict", False))
        acc, stats = None, np.zeros(7, np.uint64)
        for k in range(passes):
            _, f, st = self.render(sc, width, height, seed=(seed + k) & 0xFFFFFFFFFFFFFFFF, **kw)
            acc = f.copy() if acc is None else acc + f
            stats += st
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = acc / np.float32(passes)
        return pyoracle.quantise(mean), mean, stats


def edge_directions():
    """float32 [n, 3]: the catalogue of the rule's edges (tests/test_env_cpu.py, the GPU's op 25): the axes, dy = +-0, the folds
    |px| + |pz| = 1, the corners (the -y pole) and borders, zero, NaN, +-inf, s overflowing, subnormal components, d and 2 d."""
    big, tiny, sub = np.float32(3e38), np.float32(1.2e-38), np.float32(1e-42)
    rows = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
            (0.3, 0.0, 0.7), (0.3, -0.0, 0.7), (-0.3, 0.0, -0.7), (-0.3, -0.0, 0.7), (1, -0.0, 0), (0, -0.0, -1),
            (0.5, 0.0, 0.5), (0.5, 0.0, -0.5), (-0.25, 0.0, 0.75), (-0.5, -0.0, -0.5), (0.5, 1e-30, 0.5), (0.5, -1e-30, 0.5), (0.25, -1e-8, -0.75),
            (0, -1, 0), (1e-30, -1, 1e-30), (-1e-30, -1, 1e-30), (1e-30, -1, -1e-30), (-1e-30, -1, -1e-30), (-0.0, -1, -0.0), (0.0, -1, -0.0),
            (1, -1e-3, 0), (-1, -1e-3, 0), (0, -1e-3, 1), (0, -1e-3, -1), (1, -1, 0), (-1, -1, 0), (0, -1, 1), (0, -1, -1), (1, -1, 1e-4), (1e-4, -1, -1),
            (0, 0, 0), (-0.0, 0.0, -0.0), (np.nan, 0, 1), (0, np.nan, 1), (0, 1, np.nan), (np.inf, 0, 0), (0, -np.inf, 0), (1, 1, -np.inf), (np.inf, -np.inf, np.inf),
            (big, big, 0), (big, -big, big), (-big, 0.5, -big), (2e38, 1e38, 1e37), (1.5e38, -1.5e38, 0),
            (sub, 0, 0), (0, sub, 0), (0, -sub, 0), (sub, -sub, sub), (-sub, sub, 3 * sub), (tiny, -tiny, sub), (sub, 1, 0), (sub, -1, -sub), (1, -sub, sub), (1.4e-45, -1.4e-45, 1.4e-45),
            (0.1, 0.2, 0.3), (0.2, 0.4, 0.6), (0.1, -0.2, 0.3), (0.2, -0.4, 0.6), (-0.7, -0.05, 0.11), (-1.4, -0.1, 0.22), (123.5, 77.25, -3e3), (247.0, 154.5, -6e3)]
    return np.array(rows, np.float32)
