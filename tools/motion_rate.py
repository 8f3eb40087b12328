"""What motion blur costs on one MI355X (include/skr.h skr_scene_set_sphere_velocities).  tools/lens_rate.py's method:
frames at 1920x1080, every frame timed on its own with HIP events, the arms alternating frame by frame in one process; mean, median and
spread of `--frames` frames after `--warmup`.  spheres2.scn with a velocity on its small spheres, --shadow and --shadow --gillum 4:
  * motion        motion in force (S = 1);
  * rest_generic  the same scene with S = 0 under SKR_PIPELINE=generic: the same pipeline, so the difference to `motion` is the shutter
                  draw, the displaced centres and the shadow masks the motion instances do not consult;
  * rest_default  S = 0 on its default path (the direct kernel, the node pipeline): what leaving that path costs.
--baseline: only the two arms at rest, and without calling a motion setter (a scene that never heard of motion is the same launch) —
for a run under SKR_LIBRARY=<the parent commit's libskr.so>, the baseline of the unchanged arms.
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


def small_sphere_velocities(scene):
    """a velocity on every sphere of radius <= 1.25 (the ground and nothing else stays)"""
    spheres = scene.arrays()[0].reshape(-1, 14)
    rng = np.random.default_rng(16)
    v = rng.uniform(-1.5, 1.5, (len(spheres), 3)).astype(np.float32)
    v[spheres[:, 3] > 1.25] = 0
    return v


def renderer(path, shutter, generic, baseline):
    """a renderer of the scene in motion under the shutter (0: at rest); generic: its switches were read with SKR_PIPELINE=generic set"""
    if generic:
        os.environ["SKR_PIPELINE"] = "generic"
    try:
        scene = skr.parse_scene(path)
        if not baseline:
            scene.set_velocities(small_sphere_velocities(scene))
            scene.set_shutter(shutter)
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
        arms = [("motion", 1.0, False), ("rest_generic", 0.0, True), ("rest_default", 0.0, False)][1 if a.baseline else 0:]
        rs = [renderer(path, s, g, a.baseline) for _, s, g in arms]
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
        for (name, s, g), t, w, v in zip(arms, times, work, variants):
            print(json.dumps({"scene": "spheres2.scn", "arm": name, "options": kw, "shutter": s, "baseline": a.baseline, "frames": len(t), "mean_ms": round(statistics.fmean(t), 4),
                              "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "variant": v, **w}), flush=True)
        mean = {name: statistics.fmean(t) for (name, _, _), t in zip(arms, times)}
        if not a.baseline:
            print(json.dumps({"scene": "spheres2.scn", "options": kw, "motion_over_rest_generic": round(mean["motion"] / mean["rest_generic"], 4),
                              "rest_generic_over_rest_default": round(mean["rest_generic"] / mean["rest_default"], 4)}), flush=True)
        for r in rs:
            r.close()


if __name__ == "__main__":
    main()
