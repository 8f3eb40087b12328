"""The CPU checker of the thin-lens camera (tests/lens_checker.c; include/skr.h skr_scene_set_lens): compiled once per
session with the oracle's flags.  The C file fills the rays of a (frame, aa) and shades rays; a frame is composed here, per aa in aa
order, as sko_render sums its samples.  Test infrastructure; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle
from shade_query_check import _flags, oracle_options
from soft_light_check import _radii
from spot_check import ORACLE_DIR, TESTS, _scene, _spots

LENS_CTR3 = 0x800000C0  # include/skr.h SKR_LENS_CTR3
TWO_PI_F = np.float32(float.fromhex("0x1.921fb6p+2"))


def build(out_dir):
    """The checker into out_dir (it includes tests/soft_light_checker.c and with it oracle/skr_oracle.c whole: no liboracle)."""
    pyoracle.lib()
    so = os.path.join(out_dir, "liblenscheck.so")
    subprocess.check_call(["gcc", *_flags(), "-I" + ORACLE_DIR, "-I" + TESTS, "-shared", "-o", so, os.path.join(TESTS, "lens_checker.c"), "-lm"])
    L = C.CDLL(so)
    L.lens_sample.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.lens_sample.restype = None
    L.lens_records.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.lens_records.restype = None
    L.lens_rays.argtypes = [C.POINTER(pyoracle.Scene), C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint32, C.c_float, C.c_float, C.c_void_p]
    L.lens_rays.restype = None
    L.lens_shade_rays.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lens_shade_rays.restype = C.c_int
    return Checker(L)


def records(pixel, aa, seed, A, k, cam_pos, right, up, d):
    """uint32 [n, 18] = (pixel, aa, seed_lo, seed_hi, A, k, cam_pos(3), right(3), up(3), d(3)): the input of skr_debug_eval's lens op.
    Scalars and vectors are broadcast against the longest argument."""
    cols = [np.atleast_2d(np.asarray(v, np.float32).reshape(-1, w)) for v, w in ((A, 1), (k, 1), (cam_pos, 3), (right, 3), (up, 3), (d, 3))]
    ints = [np.atleast_1d(np.asarray(v, np.uint64)) for v in (pixel, aa, seed)]
    n = max(len(c) for c in cols + ints)
    f = np.concatenate([np.broadcast_to(c, (n, c.shape[1])) for c in cols], axis=1).astype(np.float32)
    px, a, s = (np.broadcast_to(v, (n,)) for v in ints)
    rec = np.zeros((n, 18), np.uint32)
    rec[:, 0], rec[:, 1] = px.astype(np.uint32), a.astype(np.uint32)
    rec[:, 2], rec[:, 3] = (s & np.uint64(0xFFFFFFFF)).astype(np.uint32), (s >> np.uint64(32)).astype(np.uint32)
    rec[:, 4:] = np.ascontiguousarray(f).view(np.uint32)
    return rec


class Checker:
    def __init__(self, lib):
        self.lib = lib

    def samples(self, rec):
        """float32 [n, 8] = (lx, ly, o'(3), d'(3)) of records uint32 [n, 18] (`records`): lens_record."""
        rec = np.ascontiguousarray(rec, np.uint32).reshape(-1, 18)
        out = np.zeros((len(rec), 8), np.float32)
        self.lib.lens_records(rec.ctypes.data, len(rec), out.ctypes.data)
        return out

    def rays(self, scene, width, height, *, aperture=0.0, focus=1.0, fov=60.0, jsample=0, seed=1, sample=0, strict=False):
        """float32 [h * w, 8]: the primary rays of AA sample `sample` of the frame under the lens (include/skr.h skr_ray); keys y * w + x."""
        sc = _scene(scene, strict)
        rays = np.zeros((height * width, 8), np.float32)
        self.lib.lens_rays(C.byref(sc.s), width, height, fov, int(jsample > 0), seed, sample, C.c_float(float(np.float32(aperture))),
                           C.c_float(float(np.float32(focus))), rays.ctypes.data)
        return rays

    def shade(self, scene, rays, *, radii=None, spots=None, cones=None, triangle_shadows=False, sample=0, keys=None, strict=False, **opt):
        """(float32 [n, 3], stats uint64[5] as pyoracle.render's) for rays float32 [n, 8]: the soft-light checker's shade tree."""
        sc = _scene(scene, strict)
        s, c = _spots(spots, cones)
        rd = _radii(sc, len(s), radii, opt.get("legacy_reflect"))
        o = oracle_options(**opt)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(-1)
        out = np.zeros((len(r), 3), np.float32)
        stats = np.zeros(5, np.uint64)
        rc = self.lib.lens_shade_rays(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), len(s), s.ctypes.data, c.ctypes.data, rd.ctypes.data, r.ctypes.data, len(r),
                                      sample, None if k is None else k.ctypes.data, out.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("lens_shade_rays failed: %d" % rc)
        return out, stats

    def render(self, scene, width, height, *, aperture=0.0, focus=1.0, fov=60.0, jsample=0, seed=1, strict=False, **kw):
        """(rgb uint8 [h, w, 3], float32 [h, w, 3], stats uint64[5]) of the frame under the lens (aperture, focus): per aa the rays
        shaded with keys y * w + x and sample aa, summed in aa order and divided by (float) (g * g), exactly as sko_render does.  kw:
        radii, spots, cones, triangle_shadows and the options of shade_query_check.oracle_options."""
        sc = _scene(scene, strict)
        keys = np.arange(width * height, dtype=np.uint32)
        stats = np.zeros(5, np.uint64)
        g2 = jsample * jsample if jsample > 0 else 1
        px = None
        for aa in range(g2):
            rays = self.rays(sc, width, height, aperture=aperture, focus=focus, fov=fov, jsample=jsample, seed=seed, sample=aa)
            c, st = self.shade(sc, rays, sample=aa, keys=keys, seed=seed, **kw)
            stats += st
            if jsample > 0:
                px = (np.zeros_like(c) + c) if px is None else px + c  # (0, 0, 0) + the first sample, as the render loop starts
            else:
                px = c
        if jsample > 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                px = px / np.float32(g2)
        f = px.reshape(height, width, 3).astype(np.float32)
        return pyoracle.quantise(f), f, stats

    def render_progressive(self, scene, width, height, passes, *, seed=1, **kw):
        """--progressive K under the lens: K frames under the seeds seed .. seed + K - 1 summed in that order, / (float) K once
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
