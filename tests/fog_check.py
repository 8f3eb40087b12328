"""The CPU checker of the spherical fog (tests/fog_checker.c): compiled once per session with the oracle's flags, linked against
oracle/liboracle.so.  Test infrastructure; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "fog_checker.c")
ORACLE_DIR = os.path.join(ROOT, "oracle")


def build(out_dir):
    """Compile the checker into out_dir (oracle/Makefile's CFLAGS: -O2 -ffp-contract=off, -mfma where the CPU has it)."""
    pyoracle.lib()  # liboracle.so built if missing
    so = os.path.join(out_dir, "libfogcheck.so")
    flags = ["-O2", "-std=c11", "-fPIC", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter"]
    with open("/proc/cpuinfo") as f:
        if " fma " in f.read():
            flags.append("-mfma")
    subprocess.check_call(["gcc", *flags, "-shared", "-o", so, SRC, "-L" + ORACLE_DIR, "-l:liboracle.so", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    L = C.CDLL(so)
    L.skf_exp_spec.argtypes = [C.c_double]
    L.skf_exp_spec.restype = C.c_double
    L.skf_fog_term_record.argtypes = [C.c_void_p, C.c_void_p]
    L.skf_fog_term_record.restype = None
    L.skf_render.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.skf_render.restype = C.c_int
    return Checker(L)


class Checker:
    def __init__(self, L):
        self.L = L

    def exp(self, x):
        return self.L.skf_exp_spec(float(x))

    def fog_term_records(self, rec):
        """skr_debug_eval op 11 on the CPU: rec uint32 [n, 40] -> uint32 [n, 4]."""
        rec = np.ascontiguousarray(rec, np.uint32)
        out = np.zeros((len(rec), 4), np.uint32)
        for i in range(len(rec)):
            self.L.skf_fog_term_record(rec[i].ctypes.data, out[i].ctypes.data)
        return out

    def render(self, scene, width, height, fog=None, *, fov=60.0, gillum=None, jsample=0, depth=3, shadow=False, seed=1, y0=0, y1=None,
               strict=False, threads=None):
        """As pyoracle.render (counter RNG, shared math) with the fog volumes fog [n, 9] (skr_scene_get_fog rows).
        Returns (rgb uint8 [rows, W, 3], float32 [rows, W, 3], stats {rays, hits, shadow rays})."""
        if isinstance(scene, (str, os.PathLike)):
            scene = pyoracle.OracleScene(scene, strict=strict)
        y1 = height if y1 is None else y1
        fog = np.ascontiguousarray(np.zeros((0, 9)) if fog is None else fog, np.float32).reshape(-1, 9)
        o = pyoracle.Options(width, height, fov, 0 if gillum is None else 1, 1 if gillum is None else gillum, jsample, depth, int(bool(shadow)),
                             pyoracle.RNG_COUNTER, pyoracle.MATH_SHARED, seed, y0, y1, threads or pyoracle.host_cores(), 0, 0)
        rgb = np.zeros((y1 - y0, width, 3), np.uint8)
        rgbf = np.zeros((y1 - y0, width, 3), np.float32)
        stats = np.zeros(3, np.uint64)
        rc = self.L.skf_render(C.byref(scene.s), C.byref(o), fog.ctypes.data, len(fog), rgb.ctypes.data, rgbf.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("skf_render failed: %d" % rc)
        return rgb, rgbf, stats
