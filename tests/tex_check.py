"""The CPU checker of sphere textures (tests/tex_checker.c; include/skr.h skr_scene_add_texture): compiled once per session
with the oracle's flags.  The C file is the environment checker's shade tree with the two primed material rows at a textured sphere; a
frame is composed here, per aa in aa order from the lens checker's rays, exactly as env_check.Checker.render composes one.  Test
infrastructure; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

import env_check
from motion_check import in_force
from oracle import pyoracle
from shade_query_check import _flags, oracle_options
from soft_light_check import _radii
from spot_check import ORACLE_DIR, TESTS, _scene, _spots

TEX_MAX, TEX_MAX_EDGE = 16, 1024  # include/skr.h SKR_TEX_MAX, SKR_TEX_MAX_EDGE
DEBUG_EDGES = (1, 2, 3, 64)       # include/skr.h skr_debug_eval op 26: the op's own textures


def build(out_dir):
    """The checker into out_dir (it includes tests/env_checker.c and with it the whole chain and oracle/skr_oracle.c: no liboracle)."""
    pyoracle.lib()
    so = os.path.join(out_dir, "libtexcheck.so")
    subprocess.check_call(["gcc", *_flags(), "-I" + ORACLE_DIR, "-I" + TESTS, "-shared", "-o", so, os.path.join(TESTS, "tex_checker.c"), "-lm"])
    L = C.CDLL(so)
    L.env_records.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.env_records.restype = None
    L.env_lookup.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.env_lookup.restype = C.c_int
    L.tex_colour.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.tex_colour.restype = C.c_int
    L.lens_rays.argtypes = [C.POINTER(pyoracle.Scene), C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_uint32, C.c_float, C.c_float, C.c_void_p]
    L.lens_rays.restype = None
    L.tex_shade_rays.argtypes = [C.POINTER(pyoracle.Scene), C.POINTER(pyoracle.Options), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                                 C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tex_shade_rays.restype = C.c_int
    return Checker(L)


def records(N, k):
    """uint32 [n, 4] = (N(3), texture index): the input of skr_debug_eval's op 26."""
    N = np.ascontiguousarray(N, np.float32).reshape(-1, 3)
    rec = np.zeros((len(N), 4), np.uint32)
    rec[:, :3] = N.view(np.uint32)
    rec[:, 3] = np.asarray(k, np.int64).astype(np.uint32)
    return rec


def debug_texture(k):
    """float32 [E, E, 3]: texture k of skr_debug_eval's op 26, texel (row j, column i) = (i + 1, j + 1, 0.5 (i + j) + 0.25)."""
    E = DEBUG_EDGES[k]
    j, i = np.meshgrid(np.arange(E, dtype=np.float32), np.arange(E, dtype=np.float32), indexing="ij")
    return np.stack([i + 1, j + 1, np.float32(0.5) * (i + j) + np.float32(0.25)], axis=2).astype(np.float32)


# the scene of the frame tests: (ka, kd) of its three small spheres
MATS = [((0.5, 0.25, 1.0), (0.6, 0.5, 0.4)), ((1.0, 0.75, 0.5), (0.3, 0.9, 0.7)), ((0.25, 0.5, 0.125), (0.8, 0.2, 0.55))]  # (ka, kd) of the three spheres


def g9(v):
    return " ".join("%.9g" % np.float32(x) for x in v)  # (nine digits give a binary32 back exactly)


def scene_text(scale=(1.0, 1.0, 1.0), texture_lines=None):
    """three spheres over a large one, two lights; sphere i's ka and kd are MATS[i] times scale[i] (a power of two: exact)"""
    t = "camera 0 1.5 -9 0 -0.1 1 0 1 0 30\nbackground .1 .2 .3\nambient_light .2 .3 .4\npoint_light 40 40 40 4 8 -3\npoint_light 20 25 30 -5 6 -4\n"
    for i, ((ka, kd), s, c) in enumerate(zip(MATS, scale, ((-2.2, 1, 1), (0, 1.2, 0), (2.2, 1, 1.5)))):
        if texture_lines:
            t += texture_lines[i]
        t += "material %s %s .5 .5 .5 16 0 0 0 1.3\nsphere %s 1\n" % (g9(np.array(ka, np.float32) * np.float32(s)), g9(np.array(kd, np.float32) * np.float32(s)), g9(c))
    if texture_lines:
        t += "texture none\n"
    return t + "material .5 .5 .5 .5 .5 .5 0 0 0 1 0 0 0 1\nsphere 0 -1000 0 1000\n"


class Checker(env_check.Checker):
    def colour(self, texels, N):
        """float32 [n, 3] = tex(N) for normals N [n, 3] on the texture texels [E, E, 3]: (1, 1, 1) where the rule's first step fails."""
        t = np.ascontiguousarray(texels, np.float32)
        N = np.ascontiguousarray(N, np.float32).reshape(-1, 3)
        out = np.zeros_like(N)
        for i in range(len(N)):
            self.lib.tex_colour(t.ctypes.data, t.shape[0], N[i:i + 1].ctypes.data, out[i:i + 1].ctypes.data)
        return out

    def shade(self, scene, rays, *, textures=None, sphere_textures=None, environment=None, velocities=None, shutter=1.0, radii=None, spots=None, cones=None,
              triangle_shadows=False, sample=0, keys=None, strict=False, **opt):
        """(float32 [n, 3], stats uint64[8]: env_check's seven, then the texture lookups) for rays float32 [n, 8] on the scene whose
        sphere i carries textures[sphere_textures[i]] (-1, or None: no texture)."""
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
        out = np.zeros((len(r), 3), np.float32)
        stats = np.zeros(8, np.uint64)
        rc = self.lib.tex_shade_rays(C.byref(sc.s), C.byref(o), int(bool(triangle_shadows)), len(s), s.ctypes.data, c.ctypes.data, rd.ctypes.data, v.ctypes.data,
                                     C.c_float(float(np.float32(shutter))), int(force), None if t is None else t.ctypes.data, 0 if t is None else t.shape[0],
                                     flat.ctypes.data, first.ctypes.data, edges.ctypes.data, None if idx is None else idx.ctypes.data, r.ctypes.data, len(r), sample,
                                     None if k is None else k.ctypes.data, out.ctypes.data, stats.ctypes.data)
        if rc != 0:
            raise RuntimeError("tex_shade_rays failed: %d" % rc)
        return out, stats

    def render(self, scene, width, height, *, jsample=0, **kw):
        """(rgb uint8 [h, w, 3], float32 [h, w, 3], stats uint64[8]) of the frame, composed as env_check.Checker.render composes one.
        kw: textures, sphere_textures, and everything env_check.Checker.render takes."""
        stats = np.zeros(8, np.uint64)
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
        acc, stats = None, np.zeros(8, np.uint64)
        for k in range(passes):
            _, f, st = self.render(sc, width, height, seed=(seed + k) & 0xFFFFFFFFFFFFFFFF, **kw)
            acc = f.copy() if acc is None else acc + f
            stats += st
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = acc / np.float32(passes)
        return pyoracle.quantise(mean), mean, stats


def decision_normals(E):
    """float32 [n, 3]: normals at the rule's decision points for a texture of edge E (tests/test_tex_gpu.py's op 26): the six axes,
    N.y = +-0 (the fold), directions whose u or v lands exactly on a texel centre and on a texel edge, the square's border where the
    clamps act, a zero vector and a NaN (the fallback)."""
    rows = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
            (0.5, 0.0, 0.5), (0.5, -0.0, 0.5), (-0.25, 0.0, 0.75), (-0.25, -0.0, 0.75), (0.5, 1e-30, -0.5), (0.5, -1e-30, -0.5), (1, -0.0, 0), (0, -0.0, -1)]
    for i in range(min(E, 8) + 1):  # u on a texel edge (i / E) and on a texel centre ((i + 0.5) / E), v likewise, on both sheets
        for u in (i / E, (i + 0.5) / E):
            if u <= 1.0:
                rows.append(env_check.octa_decode(u, 0.5))
                rows.append(env_check.octa_decode(0.5, u))
                rows.append(env_check.octa_decode(u, u))
                rows.append(env_check.octa_decode(u, 1.0 - u))
    e = 1e-6
    rows += [(sx * a, -1.0, sz * b) for sx in (-1, 1) for sz in (-1, 1) for a, b in ((e, e), (0.0, 0.0), (e, 0.0), (0.3, e))]  # the corners: the -y pole from every side
    rows += [(sx, -e, sz * 0.5) for sx in (-1, 1) for sz in (-1, 1)] + [(sx * 0.5, -e, sz) for sx in (-1, 1) for sz in (-1, 1)]  # the four borders
    rows += [(0, 0, 0), (-0.0, 0.0, -0.0), (np.nan, 0, 1), (0, np.nan, 0), (np.inf, 0, 0), (3e38, 3e38, 0)]  # the fallback
    return np.array(rows, np.float32)
