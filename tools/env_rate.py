"""What an environment map costs on one MI355X (include/skr.h skr_scene_set_environment).  tools/motion_rate.py's method:
frames at 1920x1080, every frame timed on its own with HIP events, the arms alternating frame by frame in one process; mean, median and
spread of `--frames` frames after `--warmup`.  spheres2.scn, --shadow and --shadow --gillum 4:
  * env_64, env_2048   the environment in force, a random map of edge 64 (64 KB of texels: cache resident) and 2048 (64 MB: every tap a
                       line from HBM);
  * const_generic      the constant background under SKR_PIPELINE=generic: the same pipeline, so the difference to the env arms is the
                       finalize kernel's recomputed directions and its four gathers per miss;
  * const_default      the constant background on its default path (the direct kernel, the node pipeline): what leaving that path costs.
--baseline: only the two constant arms, without calling the environment setter — for a run from a checkout of the parent commit (a copy
of this script in its tools/: the parent's binding does not know the setter), the baseline of the unchanged arms.
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
    """a renderer of the scene with a random environment of that edge (0: none, and no setter called); generic: its switches were read
    with SKR_PIPELINE=generic set"""
    if generic:
        os.environ["SKR_PIPELINE"] = "generic"
    try:
        scene = skr.parse_scene(path)
        if edge:
            scene.set_environment(np.random.default_rng(17).uniform(0.0, 2.0, (edge, edge, 3)).astype(np.float32))
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
        arms = [("env_64", 64, False), ("env_2048", 2048, False), ("const_generic", 0, True), ("const_default", 0, False)][2 if a.baseline else 0:]
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
            print(json.dumps({"scene": "spheres2.scn", "options": kw, "env_64_over_const_generic": round(mean["env_64"] / mean["const_generic"], 4),
                              "env_2048_over_const_generic": round(mean["env_2048"] / mean["const_generic"], 4),
                              "const_generic_over_const_default": round(mean["const_generic"] / mean["const_default"], 4)}), flush=True)
        for r in rs:
            r.close()


if __name__ == "__main__":
    main()
