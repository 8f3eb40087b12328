"""What a spot light costs on one MI355X (include/skr.h SKR_SCN_SPOT).  Two pairs of frames at 1920x1080, every frame timed
on its own with HIP events, the two arms of a pair alternating frame by frame in one process; median and spread of `--frames` frames
after `--warmup`:
  * test.scn --shade-triangles --shadow --gillum 4 with --scn-spot (its one spot light kept) against the same without it under
    SKR_PIPELINE=generic: the same pipeline, so the difference is the light and not the pipeline;
  * a generated scene — a floor, a dozen spheres, eight narrow spot lights — against the same scene with the eight as point lights
    (SKR_PIPELINE=generic): what the shadow rays the cones cull are worth.
One JSON line per arm, with the work counters of one frame."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import skele_raytracer_amd as skr  # noqa: E402


def renderer(path, spot, generic):
    """a renderer whose switches were read with SKR_PIPELINE=generic set (or not)"""
    if generic:
        os.environ["SKR_PIPELINE"] = "generic"
    try:
        return skr.Renderer(skr.parse_scene(path, spot=spot), 0)
    finally:
        os.environ.pop("SKR_PIPELINE", None)


def frame_fn(r, opt):
    dev = torch.device("cuda", r.device)
    rgb = torch.empty((opt.height, opt.width, 3), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    return lambda: skr.binding._check(skr.lib().skr_render_tiles(r.h, C.byref(opt.c), opt.height, 0, 1, rgb.data_ptr(), None, stream), "skr_render_tiles")


def write_eight(path, spot):
    rng = np.random.default_rng(8)
    lines = ["camera 0 6 -14 0 -0.35 0.94 0 1 0 30", "background .1 .2 .3", "ambient_light .3 .3 .3", "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1",
             "sphere 0 -1000 0 1000"]
    for _ in range(12):
        lines.append("material .2 .2 .2 %.3f %.3f %.3f .3 .3 .3 16 0 0 0 1" % tuple(rng.uniform(0.2, 0.9, 3)))
        lines.append("sphere %.3f %.3f %.3f %.3f" % (rng.uniform(-8, 8), rng.uniform(0.5, 2.0), rng.uniform(-4, 10), rng.uniform(0.5, 1.2)))
    for _ in range(8):
        col, pos = rng.uniform(20, 60, 3), (rng.uniform(-8, 8), rng.uniform(7, 11), rng.uniform(-4, 10))
        axis = (rng.normal(0, 0.2), -1.0, rng.normal(0, 0.2))
        if spot:
            lines.append("spot_light %.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f 8 16" % (*col, *pos, *axis))
        else:
            lines.append("point_light %.3f %.3f %.3f %.3f %.3f %.3f" % (*col, *pos))
    open(path, "w").write("\n".join(lines) + "\n")
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=21)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    test = os.path.join(ROOT, "tests", "golden", "scenes", "test.scn")
    pairs = [("test.scn", dict(shade_triangles=True, shadow=True, gillum=4), [("scn_spot", test, True, False), ("no_spot_generic", test, False, True)]),
             ("eight_lights", dict(shadow=True, gillum=4), [("eight_spot_lights", write_eight(os.path.join(tmp, "spot.scn"), True), True, False),
                                                            ("eight_point_lights_generic", write_eight(os.path.join(tmp, "point.scn"), False), False, True)])]
    for scene, kw, arms in pairs:
        opt = skr.Options(1920, 1080, **kw)
        rs = [renderer(path, spot, generic) for _, path, spot, generic in arms]
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
        for (name, _, _, _), t, w, v in zip(arms, times, work, variants):
            print(json.dumps({"scene": scene, "arm": name, "options": kw, "frames": len(t), "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4),
                              "max_ms": round(max(t), 4), "variant": v, **w}), flush=True)
        for r in rs:
            r.close()


if __name__ == "__main__":
    main()
