"""The CPU checker of the ray queries (tests/ray_query_checker.c): compiled once per session with the oracle's flags, linked against
oracle/liboracle.so.  Test infrastructure; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ray_query_checker.c")
ORACLE_DIR = os.path.join(ROOT, "oracle")


def build(out_dir):
    """Compile the checker into out_dir (oracle/Makefile's CFLAGS: -O2 -ffp-contract=off, -mfma where the CPU has it)."""
    pyoracle.lib()  # liboracle.so built if missing
    so = os.path.join(out_dir, "libraycheck.so")
    flags = ["-O2", "-std=c11", "-fPIC", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter"]
    with open("/proc/cpuinfo") as f:
        if " fma " in f.read():
            flags.append("-mfma")
    subprocess.check_call(["gcc", *flags, "-I" + ORACLE_DIR, "-shared", "-o", so, SRC, "-L" + ORACLE_DIR, "-l:liboracle.so",
                           "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.skq_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.skq_trace.restype = None
    L.skq_camera_rays.argtypes = [C.POINTER(pyoracle.Scene), C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p]
    L.skq_camera_rays.restype = None
    return Checker(L)


def pack_rays(origins, directions, tmax=None, ignore_triangle=None):
    """float32 [n, 8] in the include/skr.h skr_ray layout (numpy)."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    n = len(o)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = o
    r[:, 3] = np.inf if tmax is None else np.broadcast_to(np.asarray(tmax, np.float32), (n,))
    r[:, 4:7] = d
    ign = np.full(n, -1, np.int32) if ignore_triangle is None else np.broadcast_to(np.asarray(ignore_triangle, np.int32), (n,))
    r[:, 7] = np.ascontiguousarray(ign, np.int32).view(np.float32)
    return r


class Checker:
    def __init__(self, L):
        self.L = L

    def trace(self, spheres, triangles, rays):
        """(hits float32 [n, 8] in the skr_hit layout, occluded int32 [n]) for spheres [ns, 14], triangles [nt, 9] (Scene.arrays())."""
        s = np.ascontiguousarray(spheres, np.float32).reshape(-1, 14)
        t = np.ascontiguousarray(triangles, np.float32).reshape(-1, 9)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        hits = np.zeros((len(r), 8), np.float32)
        occ = np.zeros(len(r), np.int32)
        self.L.skq_trace(s.ctypes.data, len(s), t.ctypes.data, len(t), r.ctypes.data, len(r), hits.ctypes.data, occ.ctypes.data)
        return hits, occ

    def camera_rays(self, scn, width, height, *, fov=60.0, jsample=0, seed=1, sample=0):
        """float32 [h, w, 8]: what skr_camera_rays writes for the scene file scn."""
        sc = pyoracle.OracleScene(scn)
        out = np.zeros((height, width, 8), np.float32)
        self.L.skq_camera_rays(C.byref(sc.s), width, height, fov, jsample, seed, sample, out.ctypes.data)
        return out
