"""What a lens costs on one MI355X (include/skr.h skr_scene_set_lens).  tools/soft_rate.py's method: pairs of frames at
1920x1080, every frame timed on its own with HIP events, the two arms of a pair alternating frame by frame in one process; mean, median
and spread of `--frames` frames after `--warmup`:
  * spheres2.scn --shadow, and --shadow --gillum 4, with --aperture against the same frame with A = 0 under SKR_PIPELINE=generic: the
    same pipeline, so the difference is the lens draw in the trace and activate kernels of level 1 (a sphere scene walks no tree);
  * dragon.scn with --aperture against A = 0 under SKR_PIPELINE=generic: level-1 waves walk the trace tree (origins in its ball) where
    the pinhole's walk the renderer's tree built for the scene camera.
One JSON line per arm, with the work counters of one frame, and one line per pair with the ratio of the means."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import skele_raytracer_amd as skr  # noqa: E402
from spot_rate import frame_fn  # noqa: E402


def renderer(path, lens):
    """a renderer of the scene under the lens (None: A = 0) whose switches were read with SKR_PIPELINE=generic set"""
    os.environ["SKR_PIPELINE"] = "generic"
    try:
        scene = skr.parse_scene(path)
        if lens is not None:
            scene.set_lens(*lens)
        return skr.Renderer(scene, 0)
    finally:
        os.environ.pop("SKR_PIPELINE", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=21)
    a = ap.parse_args()
    scenes = os.path.join(ROOT, "tests", "golden", "scenes")
    spheres2, dragon = os.path.join(scenes, "spheres2.scn"), os.path.join(scenes, "dragon.scn")
    pairs = [("spheres2.scn", spheres2, dict(shadow=True), (0.3, 11.0)), ("spheres2.scn", spheres2, dict(shadow=True, gillum=4), (0.3, 11.0)),
             ("dragon.scn", dragon, dict(), (0.01, 0.3))]
    for scene, path, kw, lens in pairs:
        opt = skr.Options(1920, 1080, **kw)
        arms = [("lens", lens), ("pinhole_generic", None)]
        rs = [renderer(path, l) for _, l in arms]
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
        for (name, l), t, w, v in zip(arms, times, work, variants):
            print(json.dumps({"scene": scene, "arm": name, "options": kw, "lens": list(l) if l else [0.0, 1.0], "frames": len(t), "mean_ms": round(statistics.fmean(t), 4),
                              "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "variant": v, **w}), flush=True)
        print(json.dumps({"scene": scene, "options": kw, "lens_over_pinhole": round(statistics.fmean(times[0]) / statistics.fmean(times[1]), 4)}), flush=True)
        for r in rs:
            r.close()


if __name__ == "__main__":
    main()
