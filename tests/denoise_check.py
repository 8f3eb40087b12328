"""The CPU checkers of the denoiser (include/skr.h skr_denoise): tests/denoise_checker.c, compiled with -ffp-contract=off, and a numpy
restatement of the same rule in explicit np.float32 operations, in the same order.  Test infrastructure; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "denoise_checker.c")
MISS, MESH = 0xFFFFFFFF, 0xFFFFFFFE
f32 = np.float32


def build(out_dir):
    """Compile the checker into out_dir; returns a Checker."""
    so = os.path.join(out_dir, "libdenoisecheck.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-shared", "-o", so, SRC, "-lm"])
    L = C.CDLL(so)
    L.skd_denoise.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.skd_denoise.restype = None
    return Checker(L)


class Checker:
    def __init__(self, L):
        self.L = L

    def denoise(self, rgbf, hits, iterations):
        """(rgb uint8 [h, w, 3], rgbf float32 [h, w, 3]) for rgbf float32 [h, w, 3] and hits float32 [h * w, 8] (skr_hit layout)."""
        c = np.ascontiguousarray(rgbf, np.float32)
        h, w = c.shape[:2]
        g = np.ascontiguousarray(hits, np.float32).reshape(h * w, 8)
        out = np.zeros((h, w, 3), np.float32)
        rgb = np.zeros((h, w, 3), np.uint8)
        self.L.skd_denoise(w, h, c.ctypes.data, g.ctypes.data, int(iterations), out.ctypes.data, rgb.ctypes.data)
        return rgb, out


def quantise(c):
    """device_math.h quantise, elementwise."""
    m = np.where(c < f32(1), c, f32(1)).astype(np.float32)
    s = (m * f32(255)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        q = np.where(s > f32(-2147483648.0), s, f32(0)).astype(np.int64)
    return (q & 0xFF).astype(np.uint8)


def classes(hits, h, w):
    ints = np.ascontiguousarray(hits, np.float32).reshape(h, w, 8).view(np.int32)
    kind, idx = ints[..., 1], ints[..., 2].view(np.uint32)
    return np.where(kind == 1, idx, np.where(kind == 2, np.uint32(MESH), np.uint32(MISS))).astype(np.uint32)


def _lum(c):
    return f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1] + f32(0.0722) * c[..., 2]


def _shift(a, oy, ox):
    """a[y + oy, x + ox] where in the image (zeros elsewhere) and the mask of where."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        ok[y0:y1, x0:x1] = True
    return out, ok


def denoise_numpy(rgbf, hits, iterations):
    """The rule of include/skr.h skr_denoise over whole images, every operation one np.float32 operation in the rule's order."""
    c = np.ascontiguousarray(rgbf, np.float32)
    h, w = c.shape[:2]
    g = np.ascontiguousarray(hits, np.float32).reshape(h, w, 8)
    cls = classes(hits, h, w)
    if iterations == 0:
        return quantise(c), c.copy()
    t, nrm = g[..., 0], g[..., 3:6]
    miss = cls == np.uint32(MISS)
    with np.errstate(all="ignore"):
        l = _lum(c)
        s1 = np.zeros((h, w), np.float32)
        s2 = np.zeros((h, w), np.float32)
        cnt = np.zeros((h, w), np.int32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                lq, ok = _shift(l, dy, dx)
                cq, _ = _shift(cls, dy, dx)
                m = ok & (cq == cls)
                s1 = np.where(m, s1 + lq, s1)
                s2 = np.where(m, s2 + lq * lq, s2)
                cnt = cnt + m
        m1 = s1 / cnt.astype(np.float32)
        m2 = s2 / cnt.astype(np.float32)
        d = m2 - m1 * m1
        a = np.concatenate([c, np.where(d > f32(0), d, f32(0))[..., None]], axis=2).astype(np.float32)
        k = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)
        for it in range(iterations):
            s = 1 << it
            lp = _lum(a)
            V = f32(4.0) * f32(4.0) * a[..., 3] + f32(1e-6)
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


def random_guides(h, w, seed):
    """Guides with all three classes in blocks, normals shared within a block (and random ones), and steps in t."""
    rng = np.random.default_rng(seed)
    g = np.zeros((h, w, 8), np.float32)
    ints = g.view(np.int32)
    by, bx = max(1, h // 3), max(1, w // 4)
    blk = (np.arange(h)[:, None] // by) * 7 + (np.arange(w)[None, :] // bx)
    kind = rng.integers(0, 3, blk.max() + 1)[blk]
    kind[rng.random((h, w)) < 0.08] = 0
    index = rng.integers(0, 3, blk.max() + 1)[blk]
    normals = rng.normal(size=(6, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    n = normals[rng.integers(0, 6, blk.max() + 1)[blk]]
    own = rng.random((h, w)) < 0.3
    rn = rng.normal(size=(h, w, 3))
    rn /= np.linalg.norm(rn, axis=2, keepdims=True)
    n = np.where(own[..., None], rn, n).astype(np.float32)
    t = (rng.uniform(1.5, 30, blk.max() + 1)[blk] * (1 + 0.02 * rng.random((h, w)))).astype(np.float32)
    t[rng.random((h, w)) < 0.1] *= np.float32(3)
    hit = kind != 0
    g[..., 0] = np.where(hit, t, np.float32(np.inf))
    ints[..., 1] = kind
    ints[..., 2] = np.where(kind == 1, index, np.where(kind == 2, rng.integers(0, 1000, (h, w)), -1))
    g[..., 3:6] = np.where(hit[..., None], n, np.float32(0))
    return g.reshape(h * w, 8)


def random_frame(h, w, seed):
    rng = np.random.default_rng(seed + 1)
    base = rng.uniform(0, 0.8, (h, w, 3)) * (rng.random((h, w, 1)) < 0.7)
    noise = rng.exponential(0.2, (h, w, 3)) * (rng.random((h, w, 1)) < 0.4)
    return (base + noise).astype(np.float32)
