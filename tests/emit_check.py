"""The CPU checker of emissive spheres (tests/emit_checker.c; include/skr.h skr_scene_set_sphere_emission): compiled once
per session with the oracle's flags, the way tex_check.build builds its own.  The C file is the texture checker's shade tree with the
one add at a sphere hit; a frame is composed here exactly as tex_check.Checker.render composes one.  Besides the frame the checker
reports, per ray, the surface its first segment ends on: the tests' reach conditions are asserted on that.  Test infrastructure; the
product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

import tex_check
from motion_check import in_force
from oracle import pyoracle
from shade_query_check import _flags, oracle_options
from soft_light_check import _radii
from spot_check import ORACLE_DIR, TESTS, _scene, _spots
from tex_check import TEX_MAX_EDGE, g9, scene_text  # noqa: F401  (scene_text: the geometry of the frame tests)


def build(out_dir):
    """The checker into out_dir (it includes tests/tex_checker.c and with it the whole chain and oracle/skr_oracle.c: no liboracle)."""
    pyoracle.lib()
    so = os.path.join(out_dir, "libemitcheck.so")
    subprocess.check_call(["gcc", *_flags(), "-I" + ORACLE_DIR, "-I" + TESTS, "-shared", "-o", so, os.path.join(TESTS, "emit_checker.c"), "-lm"])
    L = C.CDLL(so)
    L.env_records.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.env_records.restype = None
    L.env_lookup.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.env_lookup.restype = C.c_int
    L.tex_colour.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.tex_colour.restype = C.c_int
    L.lens_rays.argtypes = [C.POINTER(pyoracle.Scene), C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint32, C.c_float, C.c_float, C.c_void_p]
    L.lens_rays.restype = None
    shade = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_int32,
             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tex_shade_rays.argtypes = shade + [C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tex_shade_rays.restype = C.c_int
    L.emit_shade_rays.argtypes = shade + [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.emit_shade_rays.restype = C.c_int
    return Checker(L)


def emission_scene_text(emission, **kw):
    """tex_check.scene_text with an `emission r g b` line ahead of each of its four spheres (emission: [4, 3]; the ground is the last)"""
    lines = scene_text(**kw).split("\n")
    out, i = [], 0
    for ln in lines:
        if ln.startswith("sphere "):
            out.append("emission " + g9(emission[i]))
            i += 1
        out.append(ln)
    return "\n".join(out)


class Checker(tex_check.Checker):
    def without_the_add(self):
        """the texture checker on this library: tex_shade_rays, the shade tree emit_shade restates, as the same compiler run built it"""
        return tex_check.Checker(self.lib)

    def shade(self, scene, rays, *, emission=None, winners=None, textures=None, sphere_textures=None, environment=None, velocities=None, shutter=1.0, radii=None, spots=None,
              cones=None, triangle_shadows=False, sample=0, keys=None, strict=False, **opt):
        """(float32 [n, 3], stats uint64[9]: tex_check's eight, then the adds at emitters) for rays float32 [n, 8] on the scene whose
        sphere i has the emission emission[i] ([n_spheres, 3]; None: none).  winners: a list that receives an int32 [n] array, per ray
        the surface its first segment ends on (a sphere index, -1 a miss, -2 - i triangle i)."""
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
        tex = [np.ascontiguousarray(x, np.float32) for x in (textures or [])]
        for x in tex:
            if x.ndim != 3 or x.shape[0] != x.shape[1] or x.shape[2] != 3 or not 1 <= x.shape[0] <= TEX_MAX_EDGE:
                raise ValueError("texture: [E, E, 3]")
        idx = None
        if sphere_textures is not None and len(tex) > 0:
            idx = np.ascontiguousarray(sphere_textures, np.int32).reshape(-1)
            if len(idx) != sc.s.n_spheres or idx.min(initial=0) < -1 or idx.max(initial=-1) >= len(tex):
                raise ValueError("sphere_textures: one index in [-1, %d) per sphere" % len(tex))
        flat = np.concatenate([x.reshape(-1) for x in tex]) if tex else np.zeros(3, np.float32)
        first = np.array([0] + list(np.cumsum([x.size for x in tex]))[:-1], np.int64) if tex else np.zeros(1, np.int64)
        edges = np.array([x.shape[0] for x in tex] or [0], np.int32)
        e = None
        if emission is not None:
            e = np.ascontiguousarray(emission, np.float32).reshape(-1, 3)
            if len(e) != sc.s.n_spheres or not np.isfinite(e).all() or (e < 0).any():
                raise ValueError("emission: [%d, 3] finite floats >= 0" % sc.s.n_spheres)
        out = np.zeros((len(r), 3), np.float32)
        win = np.full(len(r), -1, np.int32)
        stats = np.zeros(9, np.uint64)
        rc = self.lib.emit_shade_rays(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), len(s), s.ctypes.data, c.ctypes.data, rd.ctypes.data, v.ctypes.data,
                                      C.c_float(float(np.float32(shutter))), int(force), None if t is None else t.ctypes.data, 0 if t is None else t.shape[0],
                                      flat.ctypes.data, first.ctypes.data, edges.ctypes.data, None if idx is None else idx.ctypes.data, None if e is None else e.ctypes.data,
                                      r.ctypes.data, len(r), sample, None if k is None else k.ctypes.data, out.ctypes.data, win.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("emit_shade_rays failed: %d" % rc)
        if winners is not None:
            winners.append(win)
        return out, stats

    def render(self, scene, width, height, *, jsample=0, **kw):
        """(rgb uint8 [h, w, 3], float32 [h, w, 3], stats uint64[9]) of the frame, composed as tex_check.Checker.render composes one.
        kw: emission, winners (one array per aa is appended), and everything tex_check.Checker.render takes."""
        stats = np.zeros(9, np.uint64)
        px = None
        for c, st in self.render_samples(scene, width, height, jsample=jsample, **kw):
            stats += st
            if jsample > 0:
                px = (np.zeros_like(c) + c) if px is None else px + c
            else:
                px = c
        if jsample > 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                px = px / np.float32(jsample * jsample)
        f = px.reshape(height, width, 3).astype(np.float32)
        return pyoracle.quantise(f), f, stats

    def render_progressive(self, scene, width, height, passes, *, seed=1, **kw):
        sc = _scene(scene, kw.get("strict", False))
        acc, stats = None, np.zeros(9, np.uint64)
        for k in range(passes):
            _, f, st = self.render(sc, width, height, seed=(seed + k) & 0xFFFFFFFFFFFFFFFF, **kw)
            acc = f.copy() if acc is None else acc + f
            stats += st
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = acc / np.float32(passes)
        return pyoracle.quantise(mean), mean, stats
