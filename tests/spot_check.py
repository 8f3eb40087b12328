"""The CPU checker of spot lights (tests/spot_checker.c; include/skr.h SKR_SCN_SPOT): compiled once per session with the
oracle's flags, and the small scenes of the rule's clauses.  Test infrastructure; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle
from shade_query_check import _flags, oracle_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
ORACLE_DIR = os.path.join(ROOT, "oracle")


def build(out_dir):
    """The checker into out_dir (it includes oracle/skr_oracle.c whole: no liboracle)."""
    pyoracle.lib()
    so = os.path.join(out_dir, "libspotcheck.so")
    subprocess.check_call(["gcc", *_flags(), "-I" + ORACLE_DIR, "-shared", "-o", so, os.path.join(TESTS, "spot_checker.c"), "-lm"])
    L = C.CDLL(so)
    L.sp_render.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sp_render.restype = C.c_int
    L.sp_shade_rays.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32,
                                C.c_void_p, C.c_void_p, C.c_void_p]
    L.sp_shade_rays.restype = C.c_int
    L.sp_cone.argtypes = [C.POINTER(C.c_float), C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.sp_cone.restype = C.c_int
    return Checker(L)


def _scene(scene, strict):
    return pyoracle.OracleScene(scene, strict=strict) if isinstance(scene, (str, os.PathLike)) else scene


def _spots(spots, cones):
    """The rows [n, 11] and THE LIBRARY's cones [n, 5] (Scene.spot_lights, Scene.spot_cones); None: no spot light."""
    s = np.zeros((0, 11), np.float32) if spots is None else np.ascontiguousarray(spots, np.float32).reshape(-1, 11)
    c = np.zeros((0, 5), np.float32) if cones is None else np.ascontiguousarray(cones, np.float32).reshape(-1, 5)
    if len(s) != len(c):
        raise ValueError("%d spot rows, %d cones" % (len(s), len(c)))
    return s, c


class Checker:
    def __init__(self, lib):
        self.lib = lib

    def render(self, scene, width, height, *, spots=None, cones=None, triangle_shadows=False, strict=False, **opt):
        """(rgb uint8 [h, w, 3], float32 [h, w, 3], stats uint64[5] as pyoracle.render's) of the scene file `scene` (or a
        pyoracle.OracleScene: its spot_light lines are unknown commands to it) with the spot lights `spots` behind its point lights;
        opt as shade_query_check.oracle_options."""
        sc = _scene(scene, strict)
        s, c = _spots(spots, cones)
        o = oracle_options(width=width, height=height, **opt)
        rgb = np.zeros((height, width, 3), np.uint8)
        rgbf = np.zeros((height, width, 3), np.float32)
        stats = np.zeros(5, np.uint64)
        rc = self.lib.sp_render(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), len(s), s.ctypes.data, c.ctypes.data, rgb.ctypes.data, rgbf.ctypes.data,
                                stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("sp_render failed: %d" % rc)
        return rgb, rgbf, stats

    def shade(self, scene, rays, *, spots=None, cones=None, triangle_shadows=False, sample=0, keys=None, strict=False, **opt):
        """(float32 [n, 3], stats uint64 {rays, hits, shadow rays}) for rays float32 [n, 8] (include/skr.h skr_ray)."""
        sc = _scene(scene, strict)
        s, c = _spots(spots, cones)
        o = oracle_options(**opt)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(-1)
        if k is not None and len(k) != len(r):
            raise ValueError("%d keys for %d rays" % (len(k), len(r)))
        out = np.zeros((len(r), 3), np.float32)
        stats = np.zeros(3, np.uint64)
        rc = self.lib.sp_shade_rays(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), len(s), s.ctypes.data, c.ctypes.data, r.ctypes.data, len(r), sample,
                                    None if k is None else k.ctypes.data, out.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("sp_shade_rays failed: %d" % rc)
        return out, stats

    def cone(self, a, c1, c2, L):
        """(f, outside) of one record: sp_cone."""
        av = (C.c_float * 3)(*[float(x) for x in np.asarray(a, np.float32)])
        lv = (C.c_float * 3)(*[float(x) for x in np.asarray(L, np.float32)])
        f = C.c_float()
        outside = self.lib.sp_cone(av, C.c_float(float(np.float32(c1))), C.c_float(float(np.float32(c2))), lv, C.byref(f))
        return np.float32(f.value), int(outside)


# ---- the small scenes: one floor sphere (its top is the plane y = 0 around the origin), lights above it, the camera looks at the floor ----
FLOOR = (0.0, -1000.0, 0.0, 1000.0)
CAMERA = "camera 0 7 -9 0 -0.62 0.78 0 1 0 30"
# the accept region of a triangle (v0, v1, v2) is the mirrored triangle (v0, 2 v0 - v1, v2): over the floor the camera sees
OCCLUDER = ((2.5, 3.0, -2.0), (7.0, 3.0, -2.0), (2.5, 3.0, 5.0))


def write_floor_scene(path, *, points=(), spots=(), tris=(), directional=False):
    """points: (r g b px py pz) lines, spots: (r g b px py pz dx dy dz angle1 angle2) lines, in this order in the file."""
    lines = [CAMERA, "background .1 .2 .3", "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1", "sphere %g %g %g %g" % FLOOR]
    for i, t in enumerate(tris):
        for v in t:
            lines.append("vertex %.9g %.9g %.9g" % tuple(v))
        lines.append("material .5 .4 .3 .6 .5 .4 .3 .3 .3 4 0 0 0 1")
        lines.append("triangle %d %d %d" % (3 * i, 3 * i + 1, 3 * i + 2))
    for p in points:
        lines.append("point_light " + " ".join("%.9g" % x for x in p))
    for s in spots:
        lines.append("spot_light " + " ".join("%.9g" % x for x in s))
    if directional:
        lines.append("directional_light .4 .4 .4 0.04 1 0.08")
    open(path, "w").write("\n".join(lines) + "\n")
    return path


# one point light and three spot lights: one 180/180 (a point light), one 5/20, one with angle1 == angle2 == 30 (a hard edge): mixed pairs,
# an odd light count, pairs with one and with both lights outside
MIXED_POINTS = [(60, 60, 60, -3.0, 9.0, 2.0)]
MIXED_SPOTS = [(40, 30, 20, 4.0, 10.0, 3.0, 0.3, -1.0, 0.1, 180, 180),
               (0, 0, 300, 1.0, 8.0, 0.0, 0.1, -1.0, 0.05, 5, 20),
               (200, 40, 0, -2.0, 7.0, 3.0, -0.2, -1.0, 0.3, 30, 30)]
