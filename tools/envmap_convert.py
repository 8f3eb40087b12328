"""A latitude-longitude PFM (width = 2 x height, the usual panorama: row 0 the zenith, column 0 the direction -x turning through +z)
into the octahedral PFM `raytracer --envmap` reads (include/skr.h skr_scene_set_environment: world +y at the centre of the square).
Every texel of the output is the bilinear sample of the panorama in the direction of the texel's centre, in numpy float64.  A
convenience: nothing here is bit-pinned.
    python tools/envmap_convert.py PANORAMA.pfm OUT.pfm --edge 512"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import skele_raytracer_amd as skr  # noqa: E402


def octa_directions(E):
    """float64 [E, E, 3]: the unit direction of the centre of texel (j, i)"""
    c = (np.arange(E) + 0.5) / E * 2.0 - 1.0
    qx, qz = np.meshgrid(c, c)  # qx along a row (i), qz down the rows (j)
    y = 1.0 - np.abs(qx) - np.abs(qz)
    sx, sz = np.where(qx < 0, -1.0, 1.0), np.where(qz < 0, -1.0, 1.0)
    x = np.where(y >= 0, qx, (1.0 - np.abs(qz)) * sx)
    z = np.where(y >= 0, qz, (1.0 - np.abs(qx)) * sz)
    d = np.stack([x, y, z], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def sample_latlong(pano, d):
    """bilinear, wrapping in longitude and clamped at the poles"""
    h, w, _ = pano.shape
    u = (np.arctan2(d[..., 2], d[..., 0]) / (2.0 * np.pi) + 0.5) * w - 0.5
    v = np.arccos(np.clip(d[..., 1], -1.0, 1.0)) / np.pi * h - 0.5
    u0, v0 = np.floor(u), np.floor(v)
    fu, fv = (u - u0)[..., None], (v - v0)[..., None]
    i0, i1 = u0.astype(int) % w, (u0.astype(int) + 1) % w
    j0, j1 = np.clip(v0.astype(int), 0, h - 1), np.clip(v0.astype(int) + 1, 0, h - 1)
    p = pano.astype(np.float64)
    top = p[j0, i0] * (1 - fu) + p[j0, i1] * fu
    bot = p[j1, i0] * (1 - fu) + p[j1, i1] * fu
    return top * (1 - fv) + bot * fv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("panorama")
    ap.add_argument("out")
    ap.add_argument("--edge", type=int, default=512)
    a = ap.parse_args()
    if not 1 <= a.edge <= skr.binding.ENV_MAX_EDGE:
        sys.exit("--edge takes 1 .. %d" % skr.binding.ENV_MAX_EDGE)
    pano = skr.read_pfm(a.panorama)
    if not np.isfinite(pano).all():
        sys.exit("%s holds values that are not finite: an environment takes none" % a.panorama)
    skr.write_pfm(a.out, sample_latlong(pano, octa_directions(a.edge)).astype(np.float32))


if __name__ == "__main__":
    main()
