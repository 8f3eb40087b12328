"""What lights with a radius cost on one MI355X (include/skr.h skr_scene_set_light_radii).  tools/spot_rate.py's method: two
pairs of frames at 1920x1080, every frame timed on its own with HIP events, the two arms of a pair alternating frame by frame in one
process; median and spread of `--frames` frames after `--warmup`:
  * test.scn --scn-spot --shade-triangles --shadow --gillum 4 with --light-radius against the same without it under
    SKR_PIPELINE=generic: the same pipeline, so the difference is the light sample and the unmasked sphere walk;
  * the generated scene of tools/spot_rate.py — a floor, a dozen spheres, eight lights — as eight point lights with a radius against the
    same eight as points (SKR_PIPELINE=generic): soft pairs walk every sphere where point pairs walk their masked candidates.
One JSON line per arm, with the work counters of one frame."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import skele_raytracer_amd as skr  # noqa: E402
from spot_rate import frame_fn, write_eight  # noqa: E402


def renderer(path, spot, radius, generic):
    """a renderer whose switches were read with SKR_PIPELINE=generic set (or not)"""
    if generic:
        os.environ["SKR_PIPELINE"] = "generic"
    try:
        scene = skr.parse_scene(path, spot=spot)
        if radius is not None:
            scene.set_light_radii(radius)
        return skr.Renderer(scene, 0)
    finally:
        os.environ.pop("SKR_PIPELINE", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=21)
    ap.add_argument("--radius", type=float, default=0.5)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    test = os.path.join(ROOT, "tests", "golden", "scenes", "test.scn")
    eight = write_eight(os.path.join(tmp, "point.scn"), False)
    pairs = [("test.scn", dict(shade_triangles=True, shadow=True, gillum=4), [("light_radius", test, True, a.radius, False), ("no_radius_generic", test, True, None, True)]),
             ("eight_lights", dict(shadow=True, gillum=4), [("eight_soft_lights", eight, False, a.radius, False), ("eight_point_lights_generic", eight, False, None, True)])]
    for scene, kw, arms in pairs:
        opt = skr.Options(1920, 1080, **kw)
        rs = [renderer(path, spot, radius, generic) for _, path, spot, radius, generic in arms]
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
        for (name, *_), t, w, v in zip(arms, times, work, variants):
            print(json.dumps({"scene": scene, "arm": name, "options": kw, "radius": a.radius if "generic" not in name else 0.0, "frames": len(t),
                              "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "variant": v, **w}), flush=True)
        for r in rs:
            r.close()


if __name__ == "__main__":
    main()
