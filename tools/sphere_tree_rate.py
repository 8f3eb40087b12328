#!/usr/bin/env python3
"""Dev aid: frame time and executed tests per ray over a ladder of sphere counts, for three arms — the sphere tree off
(where the LDS path accepts the scene), on, and on with SKR_NO_SPHERE_CULL=1 (spheres in HBM, the loop over every sphere).  One JSON
line per row.  Times are medians over --frames event-timed frames (after --warmup), with the spread (min, max) of the series; the test
counts come from one extra frame rendered with counting on, never from a timed frame.
usage: sphere_tree_rate.py [--counts 16,64,...] [--width 1920 --height 1080] [--gillum 16] [--depth 3] [--frames 15] [--warmup 3]
                           [--arms off,on,nocull] [--build-time]
--build-time adds the host build time of the tree, single thread, best of three."""
import argparse
import json
import math
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_grid_scene(path, n):
    """sphere 0 a 1000-radius ground sphere, spheres 1 .. n-1 on a grid that fills the view in front of it, one point light"""
    lines = ["camera 0 0 -10 0 0 1 0 1 0 30", "background .05 .1 .15", "ambient_light .25 .25 .25",
             "material .3 .3 .3 .5 .5 .5 .1 .1 .1 4 0 0 0 1", "sphere 0 -1005.6 0 1000"]
    m = n - 1
    if m > 0:
        cols = max(1, math.ceil(math.sqrt(m * 19.0 / 10.6)))
        rows = math.ceil(m / cols)
        cell = min(19.0 / cols, 10.6 / rows)
        for i in range(1, n):
            k = i - 1
            x, y, z = (k % cols - (cols - 1) / 2) * cell, ((rows - 1) / 2 - k // cols) * cell, (i * 37 % 11) * cell * 0.1
            c = ((i * 97) % 251 / 250.0, (i * 57 + 90) % 241 / 240.0, (i * 151 + 30) % 239 / 238.0)
            lines.append("material %.4f %.4f %.4f %.4f %.4f %.4f .2 .2 .2 %d 0 0 0 1" % (*(0.3 * v for v in c), *c, (1, 2, 7, 16, 33)[i % 5]))
            lines.append("sphere %.6g %.6g %.6g %.6g" % (x, y, z, 0.45 * cell))
    lines.append("point_light 1.5 1.35 1.2 8 9 -12")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="16,64,256,1024,2554,4000,20000,100000")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--gillum", type=int, default=16)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arms", default="off,on,nocull")
    ap.add_argument("--build-time", action="store_true")
    a = ap.parse_args()
    import torch
    import skele_raytracer_amd as skr
    tmp = tempfile.mkdtemp(prefix="sphere_tree_rate_")
    st = torch.cuda.current_stream()
    for n in [int(v) for v in a.counts.split(",")]:
        path = write_grid_scene(os.path.join(tmp, "n%d.scn" % n), n)
        for arm in a.arms.split(","):
            row = dict(spheres=n, arm=arm, width=a.width, height=a.height, gillum=a.gillum, depth=a.depth, shadow=True)
            if arm == "nocull":
                os.environ["SKR_NO_SPHERE_CULL"] = "1"
            else:
                os.environ.pop("SKR_NO_SPHERE_CULL", None)
            try:
                sc = skr.parse_scene(path, sphere_tree=True) if arm != "off" else skr.parse_scene(path)
                if a.build_time and arm == "on":
                    best = None
                    for _ in range(3):
                        t0 = time.perf_counter()
                        sc.sphere_tree_data()
                        dt = time.perf_counter() - t0
                        best = dt if best is None else min(best, dt)
                    row["tree_build_ms"] = round(best * 1e3, 2)  # (includes copying the arrays out)
                r = skr.Renderer(sc)
                opt = skr.Options(a.width, a.height, gillum=a.gillum, depth=a.depth, shadow=True, seed=3)
                buf = torch.zeros((a.height, a.width, 3), dtype=torch.uint8, device="cuda")
                for _ in range(a.warmup):
                    r.render_tiles_into(opt, a.height, 0, 1, buf.data_ptr(), None, st.cuda_stream)
                torch.cuda.synchronize()
                ms = []
                for _ in range(a.frames):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    r.render_tiles_into(opt, a.height, 0, 1, buf.data_ptr(), None, st.cuda_stream)
                    e1.record(st)
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                row.update(variant=r.kernel_variant(), frames=a.frames, ms_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3))
                # the counts: one frame with counting on
                r.work(reset=True)
                r.count_triangle_work(True)
                r.sphere_tree_work(reset=True)
                r.render_tiles_into(opt, a.height, 0, 1, buf.data_ptr(), None, st.cuda_stream)
                torch.cuda.synchronize()
                w = r.sphere_tree_work(reset=True)
                r.count_triangle_work(False)
                c = r.work(reset=True)
                rays = c["radiance_rays"] + c["shadow_rays"]
                row.update(rays=rays, reference_tests_per_ray=round(c["sphere_tests"] / max(1, rays), 1))
                if arm == "on":
                    row.update(cull_tests_per_ray=round(w["cull_tests"] / max(1, rays), 2), sphere_tests_per_ray=round(w["sphere_tests"] / max(1, rays), 2))
                r.close()
            except skr.SkrError as e:
                row["refused"] = str(e)[:160]
            print(json.dumps(row), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
