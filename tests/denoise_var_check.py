"""The CPU checkers of the denoiser under a per-pixel variance image (include/skr.h skr_denoise_var, skr_render_adaptive_var; DESIGN.md
8.11): tests/denoise_var_checker.c, compiled with the flags of denoise_check.build, and a numpy restatement of the same rule in explicit
np.float32 operations, in the same order.  Test infrastructure; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

from adaptive_check import converged, lum
from denoise_check import MISS, _lum, _shift, classes, quantise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "denoise_var_checker.c")
f32 = np.float32
VAR_SIGMA_L = f32(4.0)  # include/skr.h SKR_DENOISE_VAR_SIGMA_L


def build(out_dir):
    """Compile the checker into out_dir; returns a Checker."""
    so = os.path.join(out_dir, "libdenoisevarcheck.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-shared", "-o", so, SRC, "-lm"])
    L = C.CDLL(so)
    L.skdv_denoise.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.skdv_denoise.restype = None
    return Checker(L)


class Checker:
    def __init__(self, L):
        self.L = L

    def denoise(self, rgbf, hits, var, iterations):
        """(rgb uint8 [h, w, 3], rgbf float32 [h, w, 3]) for rgbf float32 [h, w, 3], hits float32 [h * w, 8] (skr_hit layout) and var
        float32 [h, w] or None."""
        c = np.ascontiguousarray(rgbf, np.float32)
        h, w = c.shape[:2]
        g = np.ascontiguousarray(hits, np.float32).reshape(h * w, 8)
        v = None if var is None else np.ascontiguousarray(var, np.float32).reshape(h, w)
        out = np.zeros((h, w, 3), np.float32)
        rgb = np.zeros((h, w, 3), np.uint8)
        self.L.skdv_denoise(w, h, c.ctypes.data, g.ctypes.data, None if v is None else v.ctypes.data, int(iterations), out.ctypes.data, rgb.ctypes.data)
        return rgb, out


def variance_of_mean(S1, S2, n):
    """var_p of include/skr.h skr_render_adaptive_var for the final state S1, S2 (float32 arrays) and n (integer array): -1 under two
    passes, else the e2 of the convergence test."""
    S1, S2 = np.asarray(S1, np.float32), np.asarray(S2, np.float32)
    n = np.asarray(n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nf = n.astype(np.float32)
        m = (S1 / nf).astype(np.float32)
        d = (S2 / nf - m * m).astype(np.float32)
        v = np.where(d > 0, d, f32(0)).astype(np.float32)
        e2 = (v / (nf - f32(1))).astype(np.float32)
    return np.where(n < 2, f32(-1), e2).astype(np.float32)


def adaptive_with_variance(frame, min_passes, max_passes, threshold):
    """adaptive_check.adaptive with the final statistics kept: (mean float32 [N, 3], bytes uint8 [N, 3], passes uint32 [N], var float32 [N])."""
    assert 1 <= min_passes <= max_passes and not np.isnan(threshold)
    v = np.asarray(frame(0), np.float32).reshape(-1, 3)
    C_ = v.copy()
    l = lum(v)
    S1, S2 = l.copy(), (l * l).astype(np.float32)
    n = np.ones(len(v), np.uint32)
    active = np.ones(len(v), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, max_passes):
            if k >= min_passes and k >= 2 and threshold >= 0:
                active &= ~converged(S1, S2, k, threshold)
            if not active.any():
                break
            v = np.asarray(frame(k), np.float32).reshape(-1, 3)
            l = lum(v)
            C_[active] = C_[active] + v[active]
            S1[active] = S1[active] + l[active]
            S2[active] = S2[active] + (l * l).astype(np.float32)[active]
            n[active] += 1
        mean = (C_ / n.astype(np.float32)[:, None]).astype(np.float32)
    return mean, quantise(mean), n, variance_of_mean(S1, S2, n)


def init_variance_numpy(c, cls, var):
    """The init value of every pixel: the 3x3 pre-filter of the measured variances where var >= 0, else the spatial estimate."""
    h, w = cls.shape
    with np.errstate(all="ignore"):
        l = _lum(c)
        s1 = np.zeros((h, w), np.float32)
        s2 = np.zeros((h, w), np.float32)
        cnt = np.zeros((h, w), np.int32)
        sv = np.zeros((h, w), np.float32)
        sg = np.zeros((h, w), np.float32)
        measured = np.zeros((h, w), bool) if var is None else (var >= f32(0))
        vimg = np.zeros((h, w), np.float32) if var is None else np.ascontiguousarray(var, np.float32)
        g3 = np.array([0.25, 0.5, 0.25], np.float32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                lq, ok = _shift(l, dy, dx)
                cq, _ = _shift(cls, dy, dx)
                vq, _ = _shift(vimg, dy, dx)
                mq, _ = _shift(measured, dy, dx)
                m = ok & (cq == cls)
                s1 = np.where(m, s1 + lq, s1)
                s2 = np.where(m, s2 + lq * lq, s2)
                cnt = cnt + m
                g = f32(g3[dy + 1] * g3[dx + 1])
                mm = m & mq
                sv = np.where(mm, sv + g * vq, sv)
                sg = np.where(mm, sg + g, sg)
        m1 = s1 / cnt.astype(np.float32)
        m2 = s2 / cnt.astype(np.float32)
        d = m2 - m1 * m1
        spatial = np.where(d > f32(0), d, f32(0)).astype(np.float32)
        return np.where(measured, sv / sg, spatial).astype(np.float32)


def denoise_var_numpy(rgbf, hits, var, iterations):
    """The rule of include/skr.h skr_denoise_var over whole images, every operation one np.float32 operation in the rule's order."""
    c = np.ascontiguousarray(rgbf, np.float32)
    h, w = c.shape[:2]
    g = np.ascontiguousarray(hits, np.float32).reshape(h, w, 8)
    cls = classes(hits, h, w)
    if iterations == 0:
        return quantise(c), c.copy()
    t, nrm = g[..., 0], g[..., 3:6]
    miss = cls == np.uint32(MISS)
    v0 = init_variance_numpy(c, cls, None if var is None else np.asarray(var, np.float32).reshape(h, w))
    with np.errstate(all="ignore"):
        a = np.concatenate([c, v0[..., None]], axis=2).astype(np.float32)
        k = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)
        for it in range(iterations):
            s = 1 << it
            lp = _lum(a)
            V = VAR_SIGMA_L * VAR_SIGMA_L * a[..., 3] + f32(1e-6)
            sw = np.zeros((h, w), np.float32)
            acc = np.zeros((h, w, 3), np.float32)
            sv = np.zeros((h, w), np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    aq, ok = _shift(a, s * dy, s * dx)
                    cq, _ = _shift(cls, s * dy, s * dx)
                    gq, _ = _shift(g, s * dy, s * dx)
                    m = ok & (cq == cls)
                    nq = gq[..., 3:6]
                    dot = nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1] + nrm[..., 2] * nq[..., 2]
                    wn = np.where(dot > f32(0), dot, f32(0)).astype(np.float32)
                    for _ in range(7):
                        wn = wn * wn
                    if dx or dy:
                        D = f32(0.05) * t * f32(s * max(abs(dx), abs(dy)))
                        wz = D / (D + np.abs(t - gq[..., 0]))
                    else:
                        wz = np.ones((h, w), np.float32)
                    wn = np.where(miss, f32(1), wn)
                    wz = np.where(miss, f32(1), wz)
                    dl = lp - _lum(aq)
                    wl = V / (V + dl * dl)
                    wt = k[dx + 2] * k[dy + 2] * wn * wz * wl
                    sw = np.where(m, sw + wt, sw)
                    acc = np.where(m[..., None], acc + wt[..., None] * aq[..., :3], acc)
                    sv = np.where(m, sv + wt * wt * aq[..., 3], sv)
            pos = sw > f32(0)
            nxt = np.empty_like(a)
            nxt[..., :3] = np.where(pos[..., None], acc / sw[..., None], a[..., :3])
            nxt[..., 3] = np.where(pos, sv / (sw * sw), a[..., 3])
            a = nxt
    out = np.ascontiguousarray(a[..., :3])
    return quantise(out), out


def random_variance(hits, h, w, seed):
    """A variance image for guides `hits`: measured values over six decades, zeros, -1, NaN, +inf, and whole classes unmeasured."""
    rng = np.random.default_rng(seed + 2)
    cls = classes(hits, h, w)
    v = (10.0 ** rng.uniform(-7, -1, (h, w))).astype(np.float32)
    u = rng.random((h, w))
    v[u < 0.10] = 0
    v[(u >= 0.10) & (u < 0.25)] = -1
    v[(u >= 0.25) & (u < 0.30)] = np.nan
    v[(u >= 0.30) & (u < 0.33)] = np.inf
    ids = np.unique(cls)
    for c in ids[rng.random(len(ids)) < 0.34]:
        v[cls == c] = -1
    return v
