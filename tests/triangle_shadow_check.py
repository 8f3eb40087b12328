"""The CPU checker of triangle shadows (tests/triangle_shadow_checker.c; include/skr.h skr_scene_set_triangle_shadows): compiled once
per session with the oracle's flags, and small scenes for the rule's clauses.  Test infrastructure; the product never loads it."""
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
    so = os.path.join(out_dir, "libtrishadowcheck.so")
    subprocess.check_call(["gcc", *_flags(), "-I" + ORACLE_DIR, "-shared", "-o", so, os.path.join(TESTS, "triangle_shadow_checker.c"), "-lm"])
    L = C.CDLL(so)
    L.ts_render.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ts_render.restype = C.c_int
    L.ts_shade_rays.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p,
                                C.c_void_p]
    L.ts_shade_rays.restype = C.c_int
    return Checker(L)


def _scene(scene, strict):
    return pyoracle.OracleScene(scene, strict=strict) if isinstance(scene, (str, os.PathLike)) else scene


class Checker:
    def __init__(self, lib):
        self.lib = lib

    def render(self, scene, width, height, *, triangle_shadows, strict=False, **opt):
        """(rgb uint8 [h, w, 3], float32 [h, w, 3], stats uint64[5] as pyoracle.render's) of the scene file `scene` (or a
        pyoracle.OracleScene) under the counter RNG and the shared math; opt as shade_query_check.oracle_options."""
        sc = _scene(scene, strict)
        o = oracle_options(width=width, height=height, **opt)
        rgb = np.zeros((height, width, 3), np.uint8)
        rgbf = np.zeros((height, width, 3), np.float32)
        stats = np.zeros(5, np.uint64)
        rc = self.lib.ts_render(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), rgb.ctypes.data, rgbf.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("ts_render failed: %d" % rc)
        return rgb, rgbf, stats

    def shade(self, scene, rays, *, triangle_shadows, sample=0, keys=None, strict=False, **opt):
        """(float32 [n, 3], stats uint64 {rays, hits, shadow rays}) for rays float32 [n, 8] (include/skr.h skr_ray)."""
        sc = _scene(scene, strict)
        o = oracle_options(**opt)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(-1)
        if k is not None and len(k) != len(r):
            raise ValueError("%d keys for %d rays" % (len(k), len(r)))
        out = np.zeros((len(r), 3), np.float32)
        stats = np.zeros(3, np.uint64)
        rc = self.lib.ts_shade_rays(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), r.ctypes.data, len(r), sample, None if k is None else k.ctypes.data,
                                    out.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("ts_shade_rays failed: %d" % rc)
        return out, stats


# ---- the small scenes of the rule's clauses: one floor sphere, one light, occluder triangles; the camera looks at the floor ----
FLOOR = (0.0, -1000.0, 0.0, 1000.0)  # its top is the plane y = 0 around the origin
CAMERA = "camera 0 7 -9 0 -0.62 0.78 0 1 0 30"
LIGHT_POS = (0.5, 12.0, 1.0)
# the accept region of a triangle (v0, v1, v2) is the mirrored triangle (v0, 2 v0 - v1, v2): these are chosen so that
# the region lies over the part of the floor the camera sees
OCCLUDER = ((3.5, 3.0, -2.0), (8.0, 3.0, -2.0), (3.5, 3.0, 5.0))


def moved(tri, dy):
    return tuple((x, y + dy, z) for x, y, z in tri)


def write_floor_scene(path, tris, *, light="point", materials=None):
    """tris: triangles as three (x, y, z); light: "point", "directional" (needs the strict loader) or None; materials[i]: the `material`
    line in front of triangle i (default: one grey material for all)."""
    lines = [CAMERA, "background .1 .2 .3", "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1", "sphere %g %g %g %g" % FLOOR]
    tl = []
    for i, t in enumerate(tris):
        for v in t:
            lines.append("vertex %.9g %.9g %.9g" % tuple(v))
        tl.append(materials[i] if materials else "material .5 .4 .3 .6 .5 .4 .3 .3 .3 4 0 0 0 1")
        tl.append("triangle %d %d %d" % (3 * i, 3 * i + 1, 3 * i + 2))
    lines += tl
    if light == "point":
        lines.append("point_light 90 90 90 %g %g %g" % LIGHT_POS)
    elif light == "directional":
        lines.append("directional_light .8 .8 .8 0.04 1 0.08")  # towards the light: nearly straight up
    open(path, "w").write("\n".join(lines) + "\n")
    return path
