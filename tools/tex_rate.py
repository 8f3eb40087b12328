"""What sphere textures cost on one MI355X (include/skr.h skr_scene_add_texture).  tools/env_rate.py's method: frames at
1920x1080, every frame timed on its own with HIP events, the arms alternating frame by frame in one process; mean, median and spread
of `--frames` frames after `--warmup`.  spheres2.scn, --shadow and --shadow --gillum 4:
  * tex_64, tex_1024   textures in force, every sphere carrying one random texture of edge 64 (64 KB of texels: cache resident) and
                       1024 (16 MB: a tap is a line from HBM or the last-level cache);
  * plain_generic      no textures under SKR_PIPELINE=generic: the same pipeline, so the difference to the tex arms is the four
                       gathers and the blend per shaded hit (and per node of the finalize kernel), and the activate instance that
                       carries the spot and radius tables in place of the plain one;
  * plain_default      no textures on the scene's default path (the direct kernel, the node pipeline): what leaving that path costs.
--baseline: only the two plain arms, without calling the texture setters — for a run from a checkout of the parent commit (a copy of
this script in its tools/: the parent's binding does not know the setters), the baseline of the unchanged arms.
One JSON line per arm, with the variant and the work counters of one frame, and one line per mode with the ratios of the means."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import skele_raytracer_amd as skr  # noqa: E402
from spot_rate import frame_fn  # noqa: E402


def renderer(path, edge, generic):
    """a renderer of the scene whose spheres all carry one random texture of that edge (0: none, and no setter called); generic: its
    switches were read with SKR_PIPELINE=generic set"""
    if generic:
        os.environ["SKR_PIPELINE"] = "generic"
    try:
        scene = skr.parse_scene(path)
        if edge:
            k = scene.add_texture(np.random.default_rng(17).uniform(0.0, 1.0, (edge, edge, 3)).astype(np.float32))
            scene.set_sphere_textures(np.full(scene.info.n_spheres, k, np.int32))
        return skr.Renderer(scene, 0)
    finally:
        os.environ.pop("SKR_PIPELINE", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=21)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    path = os.path.join(ROOT, "tests", "golden", "scenes", "spheres2.scn")
    for kw in (dict(shadow=True), dict(shadow=True, gillum=4)):
        opt = skr.Options(1920, 1080, **kw)
        arms = [("tex_64", 64, False), ("tex_1024", 1024, False), ("plain_generic", 0, True), ("plain_default", 0, False)][2 if a.baseline else 0:]
        rs = [renderer(path, e, g) for _, e, g in arms]
        fns = [frame_fn(r, opt) for r in rs]
        work, variants = [], []
        for r, fn in zip(rs, fns):
            r.work(reset=True)
            fn()
            torch.cuda.synchronize()
            work.append(r.work(reset=True))
            variants.append(skr.Renderer.kernel_variant())
        times = [[] for _ in arms]
        for k in range(a.warmup + a.frames):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if k >= a.warmup:
                    times[i].append(e0.elapsed_time(e1))
        for (name, e, g), t, w, v in zip(arms, times, work, variants):
            print(json.dumps({"scene": "spheres2.scn", "arm": name, "options": kw, "edge": e, "baseline": a.baseline, "frames": len(t), "mean_ms": round(statistics.fmean(t), 4),
                              "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "variant": v, **w}), flush=True)
        mean = {name: statistics.fmean(t) for (name, _, _), t in zip(arms, times)}
        if not a.baseline:
            print(json.dumps({"scene": "spheres2.scn", "options": kw, "tex_64_over_plain_generic": round(mean["tex_64"] / mean["plain_generic"], 4),
                              "tex_1024_over_plain_generic": round(mean["tex_1024"] / mean["plain_generic"], 4),
                              "plain_generic_over_plain_default": round(mean["plain_generic"] / mean["plain_default"], 4)}), flush=True)
        for r in rs:
            r.close()


if __name__ == "__main__":
    main()
