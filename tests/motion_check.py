"""The CPU checker of motion blur (tests/motion_checker.c; include/skr.h skr_scene_set_sphere_velocities): compiled once
per session with the oracle's flags.  The C file draws the shutter time, displaces the centres and shades rays on the displaced scene;
a frame is composed here, per aa in aa order, exactly as lens_check.Checker.render composes one.  Test infrastructure; the product
never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle
from shade_query_check import _flags, oracle_options
from soft_light_check import _radii
from spot_check import ORACLE_DIR, TESTS, _scene, _spots

SHUTTER_CTR3 = 0x800000E0  # include/skr.h SKR_SHUTTER_CTR3


def build(out_dir):
    """The checker into out_dir (it includes tests/lens_checker.c and with it oracle/skr_oracle.c whole: no liboracle)."""
    pyoracle.lib()
    so = os.path.join(out_dir, "libmotioncheck.so")
    subprocess.check_call(["gcc", *_flags(), "-I" + ORACLE_DIR, "-I" + TESTS, "-shared", "-o", so, os.path.join(TESTS, "motion_checker.c"), "-lm"])
    L = C.CDLL(so)
    L.motion_word.argtypes = [C.c_uint32] * 4
    L.motion_word.restype = C.c_uint32
    L.motion_tau.argtypes = [C.c_uint32] * 4 + [C.c_float]
    L.motion_tau.restype = C.c_float
    L.motion_centres.argtypes = [C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.motion_centres.restype = None
    L.motion_records.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.motion_records.restype = None
    L.lens_rays.argtypes = [C.POINTER(pyoracle.Scene), C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint32, C.c_float, C.c_float, C.c_void_p]
    L.lens_rays.restype = None
    L.motion_shade_rays.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                    C.c_int, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.motion_shade_rays.restype = C.c_int
    return Checker(L)


def records(pixel, aa, seed, S, c, v):
    """uint32 [n, 11] = (pixel, aa, seed_lo, seed_hi, S, c(3), v(3)): the input of skr_debug_eval's motion op.  Scalars and vectors are
    broadcast against the longest argument."""
    cols = [np.atleast_2d(np.asarray(x, np.float32).reshape(-1, w)) for x, w in ((S, 1), (c, 3), (v, 3))]
    ints = [np.atleast_1d(np.asarray(x, np.uint64)) for x in (pixel, aa, seed)]
    n = max(len(x) for x in cols + ints)
    f = np.concatenate([np.broadcast_to(x, (n, x.shape[1])) for x in cols], axis=1).astype(np.float32)
    px, a, s = (np.broadcast_to(x, (n,)) for x in ints)
    rec = np.zeros((n, 11), np.uint32)
    rec[:, 0], rec[:, 1] = px.astype(np.uint32), a.astype(np.uint32)
    rec[:, 2], rec[:, 3] = (s & np.uint64(0xFFFFFFFF)).astype(np.uint32), (s >> np.uint64(32)).astype(np.uint32)
    rec[:, 4:] = np.ascontiguousarray(f).view(np.uint32)
    return rec


def in_force(velocities, shutter):
    """include/skr.h: motion is in force iff S > 0 and some velocity component is != 0"""
    return bool(shutter > 0) and velocities is not None and bool(np.any(np.asarray(velocities, np.float32) != 0))


class Checker:
    def __init__(self, lib):
        self.lib = lib

    def word(self, pixel, aa, seed):
        return self.lib.motion_word(pixel & 0xFFFFFFFF, aa, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)

    def tau(self, pixel, aa, seed, S):
        return np.float32(self.lib.motion_tau(pixel & 0xFFFFFFFF, aa, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, C.c_float(float(np.float32(S)))))

    def centres(self, tau, c, v):
        c = np.ascontiguousarray(c, np.float32).reshape(-1, 3)
        v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
        out = np.zeros_like(c)
        self.lib.motion_centres(C.c_float(float(np.float32(tau))), c.ctypes.data, v.ctypes.data, len(c), out.ctypes.data)
        return out

    def samples(self, rec):
        """float32 [n, 4] = (tau, c'(3)) of records uint32 [n, 11] (`records`)."""
        rec = np.ascontiguousarray(rec, np.uint32).reshape(-1, 11)
        out = np.zeros((len(rec), 4), np.float32)
        self.lib.motion_records(rec.ctypes.data, len(rec), out.ctypes.data)
        return out

    def rays(self, scene, width, height, *, fov=60.0, jsample=0, seed=1, sample=0, strict=False):
        """float32 [h * w, 8]: the pinhole primary rays of AA sample `sample` of the frame (include/skr.h skr_ray); keys y * w + x."""
        sc = _scene(scene, strict)
        rays = np.zeros((height * width, 8), np.float32)
        self.lib.lens_rays(C.byref(sc.s), width, height, fov, int(jsample > 0), seed, sample, C.c_float(0.0), C.c_float(1.0), rays.ctypes.data)
        return rays

    def shade(self, scene, rays, *, velocities=None, shutter=1.0, radii=None, spots=None, cones=None, triangle_shadows=False, sample=0, keys=None, strict=False, force=None, **opt):
        """(float32 [n, 3], stats uint64[5] as pyoracle.render's) for rays float32 [n, 8] on the scene in motion.  force: take the
        displaced path (True) or the scene as it lies (False) whatever the rule says; None: the rule (in_force)."""
        sc = _scene(scene, strict)
        s, c = _spots(spots, cones)
        rd = _radii(sc, len(s), radii, opt.get("legacy_reflect"))
        o = oracle_options(**opt)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(-1)
        force = in_force(velocities, shutter) if force is None else bool(force)
        v = np.ascontiguousarray(velocities if force and velocities is not None else np.zeros((sc.s.n_spheres, 3)), np.float32).reshape(-1, 3)
        if len(v) != sc.s.n_spheres:
            raise ValueError("%d velocities, %d spheres" % (len(v), sc.s.n_spheres))
        out = np.zeros((len(r), 3), np.float32)
        stats = np.zeros(5, np.uint64)
        rc = self.lib.motion_shade_rays(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), len(s), s.ctypes.data, c.ctypes.data, rd.ctypes.data, v.ctypes.data,
                                        C.c_float(float(np.float32(shutter))), int(force), r.ctypes.data, len(r), sample, None if k is None else k.ctypes.data,
                                        out.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("motion_shade_rays failed: %d" % rc)
        return out, stats

    def render_samples(self, scene, width, height, *, fov=60.0, jsample=0, seed=1, strict=False, **kw):
        """[(float32 [h * w, 3], stats)] per aa: the samples a frame sums."""
        sc = _scene(scene, strict)
        keys = np.arange(width * height, dtype=np.uint32)
        g2 = jsample * jsample if jsample > 0 else 1
        return [self.shade(sc, self.rays(sc, width, height, fov=fov, jsample=jsample, seed=seed, sample=aa), sample=aa, keys=keys, seed=seed, **kw) for aa in range(g2)]

    def render(self, scene, width, height, *, fov=60.0, jsample=0, seed=1, strict=False, **kw):
        """(rgb uint8 [h, w, 3], float32 [h, w, 3], stats uint64[5]) of the frame of the scene in motion: per aa the pinhole rays shaded
        with keys y * w + x and sample aa, summed in aa order and divided by (float) (g * g), exactly as sko_render does.  kw:
        velocities, shutter, radii, spots, cones, triangle_shadows and the options of shade_query_check.oracle_options."""
        stats = np.zeros(5, np.uint64)
        px = None
        for c, st in self.render_samples(scene, width, height, fov=fov, jsample=jsample, seed=seed, strict=strict, **kw):
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
        acc, stats = None, np.zeros(5, np.uint64)
        for k in range(passes):
            _, f, st = self.render(sc, width, height, seed=(seed + k) & 0xFFFFFFFFFFFFFFFF, **kw)
            acc = f.copy() if acc is None else acc + f
            stats += st
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = acc / np.float32(passes)
        return pyoracle.quantise(mean), mean, stats
