"""The CPU checkers of the shading queries (tests/shade_query_checker.c, tests/shade_query_fog_checker.c): compiled once per session
with the oracle's flags.  Test infrastructure; the product never loads them."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
ORACLE_DIR = os.path.join(ROOT, "oracle")


def _flags():
    flags = ["-O2", "-std=c11", "-fPIC", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function"]
    with open("/proc/cpuinfo") as f:
        if " fma " in f.read():
            flags.append("-mfma")
    return flags


def build(out_dir):
    """Both checkers into out_dir.  The plain one includes oracle/skr_oracle.c whole (no liboracle); the fog one includes
    tests/fog_checker.c and links liboracle, as fog_check.py does."""
    pyoracle.lib()  # liboracle.so built if missing
    plain = os.path.join(out_dir, "libshadecheck.so")
    fog = os.path.join(out_dir, "libshadefogcheck.so")
    subprocess.check_call(["gcc", *_flags(), "-I" + ORACLE_DIR, "-shared", "-o", plain, os.path.join(TESTS, "shade_query_checker.c"), "-lm"])
    subprocess.check_call(["gcc", *_flags(), "-I" + TESTS, "-shared", "-o", fog, os.path.join(TESTS, "shade_query_fog_checker.c"), "-L" + ORACLE_DIR,
                           "-l:liboracle.so", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    P, F = C.CDLL(plain), C.CDLL(fog)
    P.shade_rays.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    P.shade_rays.restype = None
    F.shade_rays_fog.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_uint32,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    F.shade_rays_fog.restype = C.c_int
    return Checker(P, F)


def oracle_options(*, gillum=None, depth=3, shadow=False, seed=1, shade_triangles=False, legacy_reflect=False, width=1, height=1, fov=60.0, jsample=0):
    """pyoracle.Options under the counter RNG and the shared math (what the GPU computes)."""
    return pyoracle.Options(width, height, fov, 0 if gillum is None else 1, 1 if gillum is None else gillum, jsample, depth, int(bool(shadow)),
                            pyoracle.RNG_COUNTER, pyoracle.MATH_SHARED, seed, 0, height, pyoracle.host_cores(), int(bool(shade_triangles)),
                            int(bool(legacy_reflect)))


class Checker:
    def __init__(self, plain, fog):
        self.plain, self.fogl = plain, fog

    def shade(self, scene, rays, *, sample=0, keys=None, fog=None, strict=False, **opt):
        """(float32 [n, 3], stats uint64 {rays, hits, shadow rays}) for rays float32 [n, 8] (include/skr.h skr_ray) on the scene file
        `scene` (or a pyoracle.OracleScene); opt as oracle_options; fog [k, 9] rows (skr_scene_get_fog) select the fog checker."""
        if isinstance(scene, (str, os.PathLike)):
            scene = pyoracle.OracleScene(scene, strict=strict)
        o = oracle_options(**opt)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(-1)
        if k is not None and len(k) != len(r):
            raise ValueError("%d keys for %d rays" % (len(k), len(r)))
        out = np.zeros((len(r), 3), np.float32)
        stats = np.zeros(3, np.uint64)
        kp = None if k is None else k.ctypes.data
        if fog is None:
            self.plain.shade_rays(C.byref(scene.s), C.byref(o), r.ctypes.data, len(r), sample, kp, out.ctypes.data, stats.ctypes.data)
        else:
            f = np.ascontiguousarray(fog, np.float32).reshape(-1, 9)
            rc = self.fogl.shade_rays_fog(C.byref(scene.s), C.byref(o), f.ctypes.data, len(f), r.ctypes.data, len(r), sample, kp, out.ctypes.data,
                                          stats.ctypes.data)
            if rc != 0:
                raise RuntimeError("shade_rays_fog failed: %d" % rc)
        return out, stats


def camera_rays(scene, width, height, *, fov=60.0, jsample=0, seed=1, sample=0):
    """float32 [h * w, 8]: the frame's primary rays of AA sample `sample` (sko_primary_direction, the oracle render loop's own), keys y*w+x."""
    sc = scene if isinstance(scene, pyoracle.OracleScene) else pyoracle.OracleScene(scene)
    L = pyoracle.lib()
    rays = np.zeros((height, width, 8), np.float32)
    cam = sc.s.cam_pos
    rays[:, :, 0:3] = (cam.x, cam.y, cam.z)
    rays[:, :, 3] = np.inf
    rays[:, :, 7] = np.array([-1], np.int32).view(np.float32)[0]
    d = (C.c_float * 3)()
    for y in range(height):
        for x in range(width):
            r = L.sko_counter_jitter(seed, y * width + x, sample) if jsample > 0 else 0.0
            L.sko_primary_direction(C.byref(sc.s), width, height, fov, x, y, int(jsample > 0), r, d)
            rays[y, x, 4:7] = d[0], d[1], d[2]
    return rays.reshape(-1, 8)
