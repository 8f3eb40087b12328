"""Shading-query cost on one MI355X (include/skr.h skr_shade_rays).  For BASELINE configs 3 (spheres2 1080p --gillum 16
--shadow) and 4 (dragon 1080p --gillum 16): the frame through its default path, the frame through SKR_PIPELINE=generic, and
shade(camera_rays) of the same frame (keys y*W+x).  Then 2^22 random-origin rays on spheres2 --gillum 4 --depth 3 --shadow and on dragon
(config 4's options).  Timed with HIP events around `--iters` back-to-back calls after `--warmup` calls; one JSON line per case.  Run it
under `rocprofv3 --kernel-trace --stats -- python tools/shade_rate.py` for the per-kernel view."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import skele_raytracer_amd as skr  # noqa: E402
from tools.trace_rate import random_rays  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def frame_fn(r, opt):
    dev = torch.device("cuda", r.device)
    rgb = torch.empty((opt.height, opt.width, 3), dtype=torch.uint8, device=dev)
    rgbf = torch.empty((opt.height, opt.width, 3), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    return lambda: r.render_tiles_into(opt, opt.height, 0, 1, rgb.data_ptr(), rgbf.data_ptr(), stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--random", type=int, default=1 << 22)
    a = ap.parse_args()
    scenes = os.path.join(ROOT, "tests", "golden", "scenes")
    configs = [(3, "spheres2.scn", dict(gillum=16, shadow=True, depth=3)), (4, "dragon.scn", dict(gillum=16, depth=3))]
    for cfg, name, kw in configs:
        sc = skr.parse_scene(os.path.join(scenes, name))
        r = skr.Renderer(sc, 0)
        opt = skr.Options(1920, 1080, **kw)
        n = opt.width * opt.height

        def emit(case, ms, variant):
            print(json.dumps({"config": cfg, "scene": name, "case": case, "n": n, "ms": round(ms, 4), "grays_per_s": round(n / ms / 1e6, 3),
                              "variant": variant}), flush=True)
        emit("frame_default", timed(frame_fn(r, opt), a.warmup, a.iters), skr.Renderer.kernel_variant())
        os.environ["SKR_PIPELINE"] = "generic"
        try:
            emit("frame_generic", timed(frame_fn(r, opt), a.warmup, a.iters), skr.Renderer.kernel_variant())
        finally:
            del os.environ["SKR_PIPELINE"]
        r._sync_switches()
        rays = r.camera_rays(opt).view(-1, 8)
        keys = torch.arange(n, dtype=torch.int32, device="cuda")
        emit("shade_camera_rays", timed(lambda: r.shade(rays, opt, 0, keys), a.warmup, a.iters), skr.Renderer.kernel_variant())
    randoms = [("spheres2.scn", dict(gillum=4, depth=3, shadow=True)), ("dragon.scn", dict(gillum=16, depth=3))]
    for name, kw in randoms:
        sc = skr.parse_scene(os.path.join(scenes, name))
        r = skr.Renderer(sc, 0)
        opt = skr.Options(1920, 1080, **kw)
        rays = random_rays(sc, a.random, 1)
        ms = timed(lambda: r.shade(rays, opt), a.warmup, a.iters)
        print(json.dumps({"scene": name, "case": "shade_random_2^22", "options": kw, "n": a.random, "ms": round(ms, 4),
                          "grays_per_s": round(a.random / ms / 1e6, 3)}), flush=True)


if __name__ == "__main__":
    main()
