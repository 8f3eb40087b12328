"""The CPU checker of lights with a radius (tests/soft_light_checker.c; include/skr.h skr_scene_set_light_radii): compiled
once per session with the oracle's flags.  Test infrastructure; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle
from shade_query_check import _flags, oracle_options
from spot_check import ORACLE_DIR, TESTS, _scene, _spots


def build(out_dir):
    """The checker into out_dir (it includes oracle/skr_oracle.c whole: no liboracle)."""
    pyoracle.lib()
    so = os.path.join(out_dir, "libsoftlightcheck.so")
    subprocess.check_call(["gcc", *_flags(), "-I" + ORACLE_DIR, "-shared", "-o", so, os.path.join(TESTS, "soft_light_checker.c"), "-lm"])
    L = C.CDLL(so)
    L.sl_render.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p]
    L.sl_render.restype = C.c_int
    L.sl_shade_rays.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sl_shade_rays.restype = C.c_int
    L.sl_sample.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float)]
    L.sl_sample.restype = None
    return Checker(L)


def _radii(sc, n_spot, radii, legacy):
    """One radius per point and spot light of the oracle scene, in shading order; a scalar: every light; None: 0."""
    n = int(sc.s.n_point_lights) + n_spot
    r = np.zeros(n, np.float32) if radii is None else np.asarray(radii, np.float32)
    if r.ndim == 0:
        r = np.full(n, r, np.float32)
    r = np.ascontiguousarray(r, np.float32).reshape(-1)
    if len(r) != n:
        raise ValueError("%d radii for %d point and spot lights" % (len(r), n))
    if legacy and (r > 0).any():
        raise ValueError("light radii refuse legacy_reflect: the checker has no rule for the pair")
    return np.concatenate([r, np.zeros(1, np.float32)])  # (never an empty array: its pointer is passed)


class Checker:
    def __init__(self, lib):
        self.lib = lib

    def render(self, scene, width, height, *, radii=None, spots=None, cones=None, triangle_shadows=False, strict=False, **opt):
        """(rgb uint8 [h, w, 3], float32 [h, w, 3], stats uint64[5] as pyoracle.render's) of the scene file `scene` (or a
        pyoracle.OracleScene) with the spot lights `spots` behind its point lights and the radii `radii` (a scalar, or one per point and
        spot light in shading order); opt as shade_query_check.oracle_options."""
        sc = _scene(scene, strict)
        s, c = _spots(spots, cones)
        r = _radii(sc, len(s), radii, opt.get("legacy_reflect"))
        o = oracle_options(width=width, height=height, **opt)
        rgb = np.zeros((height, width, 3), np.uint8)
        rgbf = np.zeros((height, width, 3), np.float32)
        stats = np.zeros(5, np.uint64)
        rc = self.lib.sl_render(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), len(s), s.ctypes.data, c.ctypes.data, r.ctypes.data, rgb.ctypes.data,
                                rgbf.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("sl_render failed: %d" % rc)
        return rgb, rgbf, stats

    def shade(self, scene, rays, *, radii=None, spots=None, cones=None, triangle_shadows=False, sample=0, keys=None, strict=False, **opt):
        """(float32 [n, 3], stats uint64 {rays, hits, shadow rays}) for rays float32 [n, 8] (include/skr.h skr_ray)."""
        sc = _scene(scene, strict)
        s, c = _spots(spots, cones)
        rd = _radii(sc, len(s), radii, opt.get("legacy_reflect"))
        o = oracle_options(**opt)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(-1)
        if k is not None and len(k) != len(r):
            raise ValueError("%d keys for %d rays" % (len(k), len(r)))
        out = np.zeros((len(r), 3), np.float32)
        stats = np.zeros(3, np.uint64)
        rc = self.lib.sl_shade_rays(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), len(s), s.ctypes.data, c.ctypes.data, rd.ctypes.data, r.ctypes.data, len(r),
                                    sample, None if k is None else k.ctypes.data, out.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("sl_shade_rays failed: %d" % rc)
        return out, stats

    def sample(self, pixel, aa, node, l, seed, Lp, R):
        """Lp' float32 [3] of one record: sl_sample."""
        lp = (C.c_float * 3)(*[float(x) for x in np.asarray(Lp, np.float32)])
        out = (C.c_float * 3)()
        seed = int(seed)
        self.lib.sl_sample(int(pixel) & 0xFFFFFFFF, int(aa), int(node) & 0xFFFFFFFF, int(l), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, lp, C.c_float(float(np.float32(R))), out)
        return np.array(list(out), np.float32)

    def samples(self, records):
        """Lp' float32 [n, 3] for records uint32 [n, 10] = (pixel, aa, node, l, seed_lo, seed_hi, Lp(3) bits, R bits): skr_debug_eval op 18's input."""
        rec = np.ascontiguousarray(records, np.uint32).reshape(-1, 10)
        out = np.zeros((len(rec), 3), np.float32)
        f = rec[:, 6:].copy().view(np.float32)
        for i, q in enumerate(rec):
            lp = (C.c_float * 3)(*[float(x) for x in f[i, :3]])
            o = (C.c_float * 3)()
            self.lib.sl_sample(int(q[0]), int(q[1]), int(q[2]), int(q[3]), int(q[4]), int(q[5]), lp, C.c_float(float(f[i, 3])), o)
            out[i] = list(o)
        return out
