"""Ray-query throughput on one MI355X (include/skr.h skr_trace_rays; DESIGN.md "Ray queries"): G rays/s of the closest-hit and the
any-hit kernel for camera rays (1080p, coherent) and 2^22 seeded random rays (origins across the scene, random directions:
incoherent), on spheres2.scn and dragon.scn.  Timed with HIP events around `--iters` back-to-back calls after `--warmup` calls; one
JSON line per case.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/trace_rate.py` for the per-kernel view."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import skele_raytracer_amd as skr  # noqa: E402


def random_rays(scene, n, seed):
    rng = np.random.default_rng(seed)
    s, t, _ = scene.arrays()
    pts = [np.array(list(scene.info.camera)[:3], np.float32)[None, :]]
    if len(s):
        pts.append(s[:, :3])
    if len(t):
        pts.append(t.reshape(-1, 3))
    pts = np.concatenate(pts)
    lo, hi = pts.min(0), pts.max(0)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    return skr.make_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())


def time_case(r, rays, any_hit, warmup, iters):
    for _ in range(warmup):
        r.trace(rays, any_hit=any_hit)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        r.trace(rays, any_hit=any_hit)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--random", type=int, default=1 << 22)
    a = ap.parse_args()
    scenes = os.path.join(ROOT, "tests", "golden", "scenes")
    for name in ("spheres2.scn", "dragon.scn"):
        sc = skr.parse_scene(os.path.join(scenes, name))
        r = skr.Renderer(sc, 0)
        cases = [("camera_1080p", r.camera_rays(skr.Options(1920, 1080)).view(-1, 8)), ("random_2^22", random_rays(sc, a.random, 1))]
        for label, rays in cases:
            n = rays.shape[0]
            hits = r.trace(rays)
            torch.cuda.synchronize()
            hit_rate = float((hits.kind != 0).float().mean())
            for any_hit in (False, True):
                ms = time_case(r, rays, any_hit, a.warmup, a.iters)
                print(json.dumps({"scene": name, "rays": label, "n": n, "mode": "any_hit" if any_hit else "closest", "ms": round(ms, 4),
                                  "grays_per_s": round(n / ms / 1e6, 3), "hit_rate": round(hit_rate, 3)}), flush=True)


if __name__ == "__main__":
    main()
