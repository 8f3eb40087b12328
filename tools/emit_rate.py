"""What sphere emission costs on one MI355X (include/skr.h skr_scene_set_sphere_emission).  tools/tex_rate.py's method:
frames at 1920x1080, every frame timed on its own with HIP events, the arms alternating frame by frame in one process; mean, median and
spread of `--frames` frames after `--warmup`.  spheres2.scn, --shadow and --shadow --gillum 4:
  * emit               emission in force, every sphere glowing: the general level pipeline's instances with Textures (every edge 0) and
                       Emission in the pack;
  * tex_64             no emission, every sphere carrying one random texture of edge 64: the instances an emission launch mirrors, with
                       the lookup it does not make;
  * plain_generic      neither, under SKR_PIPELINE=generic: the same pipeline, so the difference to the emit arm is the row gather and
                       the add per finished hit, the texture row read per shaded hit, and the activate instance that carries the spot
                       and radius tables in place of the plain one;
  * plain_default      neither on the scene's default path (the direct kernel, the node pipeline): what leaving that path costs.
--baseline: the arms without emission only, without calling the emission setter — for a run from a checkout of the parent commit (a
copy of this script in its tools/: the parent's binding does not know the setter), the baseline of the unchanged arms.
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


def renderer(path, emit, edge, generic):
    """a renderer of the scene whose spheres all glow (emit) or all carry one random texture of that edge (0: none); generic: its
    switches were read with SKR_PIPELINE=generic set"""
    if generic:
        os.environ["SKR_PIPELINE"] = "generic"
    try:
        scene = skr.parse_scene(path)
        if emit:
            scene.set_emission(np.random.default_rng(19).uniform(0.05, 0.5, (scene.info.n_spheres, 3)).astype(np.float32))
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
        arms = [("emit", True, 0, False), ("tex_64", False, 64, False), ("plain_generic", False, 0, True), ("plain_default", False, 0, False)][1 if a.baseline else 0:]
        rs = [renderer(path, e, t, g) for _, e, t, g in arms]
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
        for (name, e, t, g), ts, w, v in zip(arms, times, work, variants):
            print(json.dumps({"scene": "spheres2.scn", "arm": name, "options": kw, "baseline": a.baseline, "frames": len(ts), "mean_ms": round(statistics.fmean(ts), 4),
                              "median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "variant": v, **w}), flush=True)
        mean = {name: statistics.fmean(ts) for (name, _, _, _), ts in zip(arms, times)}
        if not a.baseline:
            print(json.dumps({"scene": "spheres2.scn", "options": kw, "emit_over_plain_generic": round(mean["emit"] / mean["plain_generic"], 4),
                              "emit_over_tex_64": round(mean["emit"] / mean["tex_64"], 4), "tex_64_over_plain_generic": round(mean["tex_64"] / mean["plain_generic"], 4),
                              "plain_generic_over_plain_default": round(mean["plain_generic"] / mean["plain_default"], 4)}), flush=True)
        for r in rs:
            r.close()


if __name__ == "__main__":
    main()
