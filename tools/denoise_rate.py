"""Denoiser cost on one MI355X (include/skr.h skr_denoise): the filter on the 1080p headline frame (spheres2.scn
`--gillum 16 --shadow`) at several iteration counts, the same under a per-pixel variance image (skr_denoise_var, DESIGN.md 8.11: the
variance of a 4-pass adaptive frame), and the guides (camera_rays + trace of the pixel centres) on spheres2.scn and
dragon.scn at 1080p.  HIP events around `--iters` back-to-back calls after `--warmup` calls; one JSON line per case.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/denoise_rate.py` (its own process) for the per-kernel split."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import skele_raytracer_amd as skr  # noqa: E402


def time_calls(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    scenes = os.path.join(ROOT, "tests", "golden", "scenes")
    W, H = 1920, 1080
    for name, kw in (("spheres2.scn", dict(gillum=16, shadow=True)), ("dragon.scn", dict(gillum=16))):
        r = skr.Renderer(skr.parse_scene(os.path.join(scenes, name)), 0)
        g = skr.Options(W, H)
        guides = lambda: r.trace(r.camera_rays(g).view(-1, 8))
        ms = time_calls(guides, a.warmup, a.iters)
        print(json.dumps({"scene": name, "case": "guides_1080p", "ms": round(ms, 4)}), flush=True)
        rays = r.camera_rays(g).view(-1, 8)
        ms = time_calls(lambda: r.trace(rays), a.warmup, a.iters)
        print(json.dumps({"scene": name, "case": "trace_camera_1080p_closest", "ms": round(ms, 4)}), flush=True)
        _, rgbf = r.render(skr.Options(W, H, **kw), want_float=True)
        hits = r.trace(rays)
        torch.cuda.synchronize()
        for L in (1, 5) if name == "dragon.scn" else (0, 1, 2, 3, 5):
            ms = time_calls(lambda: r.denoise(rgbf, hits, L), a.warmup, a.iters)
            print(json.dumps({"scene": name, "case": "denoise_1080p", "iterations": L, "ms": round(ms, 4)}), flush=True)
        if name == "spheres2.scn":
            _, mean, _, var = r.render_adaptive(skr.Options(W, H, **kw), -1.0, 4, 4, want_float=True, want_variance=True)
            torch.cuda.synchronize()
            for L in (1, 5):
                ms = time_calls(lambda: r.denoise(mean, hits, L, variance=var), a.warmup, a.iters)
                print(json.dumps({"scene": name, "case": "denoise_var_1080p", "iterations": L, "ms": round(ms, 4)}), flush=True)


if __name__ == "__main__":
    main()
