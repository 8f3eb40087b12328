"""Adaptive sampling (include/skr.h skr_render_adaptive) against uniform sampling at 1080p: device time of an adaptive
frame at the defaults (HIP events around the whole sequence, skr_render_adaptive_host) against --progressive K at K = ceil(mean passes),
the rounds it took and the active share of each, and the time of each round path forced (SKR_ADAPTIVE_PATH = frame | query).
With --denoise L also the adaptive frame denoised, HIP events around each whole sequence, median [min, max]: the old
route (render_adaptive, the guides, denoise under the spatial variance), the same three steps with the measured variance, and the one
call skr_render_adaptive_denoised_host.
usage: python tools/adaptive_rate.py [--repeats N] [--denoise L]   (one JSON line per configuration)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import skele_raytracer_amd as skr  # noqa: E402

CROSSOVER = 0.5  # skele_raytracer_amd/csrc/launch.h SKR_ADAPTIVE_CROSSOVER: the share at and above which a round takes the frame path
CONFIGS = {"config3": ("spheres2.scn", dict(gillum=16, shadow=True, depth=3)), "config4": ("dragon.scn", dict(gillum=16, depth=3))}


def denoised_arms(r, a, kw, t, lo, hi):
    """median [min, max] ms of the three routes to a denoised adaptive frame, interleaved so that drift hits them alike"""
    import torch
    opt = skr.Options(a.width, a.height, seed=1, **kw)
    g = skr.Options(a.width, a.height, **kw)
    g.c.grid_size = 0

    def spatial():
        _, f, _ = r.render_adaptive(opt, t, lo, hi, want_float=True)
        r.denoise(f, r.trace(r.camera_rays(g).view(-1, 8)), a.denoise)

    def measured():
        _, f, _, v = r.render_adaptive(opt, t, lo, hi, want_float=True, want_variance=True)
        r.denoise(f, r.trace(r.camera_rays(g).view(-1, 8)), a.denoise, variance=v)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    arms = {"adaptive_then_denoise": lambda: events(spatial), "adaptive_var_then_denoise_var": lambda: events(measured),
            "render_adaptive_denoised_host": lambda: r.render_adaptive_denoised(opt, t, lo, hi, a.denoise)[3]}
    ms = {k: [] for k in arms}
    for rep in range(a.repeats + 1):
        for k, fn in arms.items():
            m = fn()
            if rep:  # (the first round warms up)
                ms[k].append(m)
    return {k: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--denoise", type=int, default=None, help="also time the adaptive frame denoised by L iterations")
    a = ap.parse_args()
    lo, hi, t = skr.ADAPTIVE_MIN_PASSES, skr.ADAPTIVE_MAX_PASSES, skr.ADAPTIVE_THRESHOLD
    for name, (scn, kw) in CONFIGS.items():
        r = skr.Renderer(skr.parse_scene(os.path.join(ROOT, "tests", "golden", "scenes", scn)), 0)
        opt = skr.Options(a.width, a.height, seed=1, **kw)
        row = {"config": name, "size": [a.width, a.height], "min": lo, "max": hi, "threshold": t}
        times = {}
        for path in (None, "frame", "query"):
            if path:
                os.environ["SKR_ADAPTIVE_PATH"] = path
            else:
                os.environ.pop("SKR_ADAPTIVE_PATH", None)
            r.render_adaptive_host(opt, t, lo, hi)  # warm-up
            ms = []
            for _ in range(a.repeats):
                _, _, n, m = r.render_adaptive_host(opt, t, lo, hi)
                ms.append(m)
            times[path or "auto"] = float(np.median(ms))
        os.environ.pop("SKR_ADAPTIVE_PATH", None)
        npix = n.size
        k = int(np.ceil(n.mean()))
        active = [int((n > j).sum()) for j in range(lo, hi)]
        rounds = [c for c in active if c > 0]
        share = [c / npix for c in rounds]
        one = []
        for _ in range(a.repeats):
            one.append(r.render_progressive_host(skr.Options(a.width, a.height, seed=1, progressive=1, **kw))[2])
        uni = []
        for _ in range(a.repeats):
            uni.append(r.render_progressive_host(skr.Options(a.width, a.height, seed=1, progressive=k, **kw))[2])
        row.update(mean_passes=float(n.mean()), at_max=float((n == hi).mean()), rounds=len(rounds),
                   rounds_frame_path=sum(s >= CROSSOVER for s in share), rounds_query_path=sum(s < CROSSOVER for s in share),
                   active_share_per_round=[round(s, 5) for s in share], adaptive_ms=times, frame_ms=float(np.median(one)),
                   uniform_k=k, uniform_ms=float(np.median(uni)))
        if a.denoise is not None:
            row["denoised_ms"] = denoised_arms(r, a, kw, t, lo, hi)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
