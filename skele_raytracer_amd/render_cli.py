"""`raytracer` for one node of MI355Xs: the reference's command line (README.md:24-34, main.cpp:246-391), one process
per GPU.

    python -m skele_raytracer_amd.render_cli --path S.scn --output O.ppm [--width i] [--height i] [--fov f]
           [--gillum n] [--jsample g] [--depth d] [--parallel true|false] [--shadow] [--seed N] [--tile-rows r]
           [--strict-scn] [--scn-fog] [--scn-spot] [--light-radius R] [--aperture A [--focus F]] [--scn-motion] [--shutter S] [--envmap FILE.pfm] [--scn-texture] [--scn-emission] [--scn-fov] [--shade-triangles] [--triangle-shadows] [--sphere-tree] [--legacy-reflect] [--progressive K [--progressive-every M]] [--format ppm|png|pfm] [--denoise L]
           [--adaptive T [--adaptive-min K] [--adaptive-max N] [--adaptive-denoise L]]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
           -m skele_raytracer_amd.render_cli --path spheres2.scn --output out.ppm --width 3840 --height 2160 \\
           --gillum 64 --jsample 5 --shadow            # BASELINE config 5

The framebuffer is cut into interleaved row tiles (tile t -> rank t mod G), every rank renders its tiles with one
`skr_render_tiles` launch sequence, ONE RCCL all-gather brings the u8 tiles to every rank and rank 0 de-interleaves
and writes the PPM (distributed.py).  The image does not depend on G: random numbers are keyed by the global pixel.
--triangle-shadows (triangles cast shadows) needs --shade-triangles and --shadow to have an effect; it is accepted without them.
--sphere-tree renders on the culled sphere walk (spheres in HBM, any sphere count; include/skr.h skr_scene_set_sphere_tree): the same image.
Flags are matched like the reference does — by `strcmp` anywhere in argv, unknown tokens ignored — and usage errors
print the reference's messages and exit with status 0 (main.cpp:381-391).  There is no CPU path.
"""
import math
import os
import sys
import time

import numpy as np


def _atoi(s):
    """C atoi: leading white space, an optional sign, digits; 0 when there are none (what main.cpp:246-379 calls)."""
    import re
    m = re.match(r"[ \t\n\v\f\r]*([+-]?\d+)", s)
    return max(-2 ** 31, min(2 ** 31 - 1, int(m.group(1)))) if m else 0


def _atof(s):
    """C atof: the longest leading decimal / hex-float / inf / nan prefix; 0.0 when there is none."""
    import re
    m = re.match(r"[ \t\n\v\f\r]*([+-]?(?:0[xX](?:[0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)(?:[pP][+-]?\d+)?|(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?|inf(?:inity)?|nan))", s, re.I)
    if not m:
        return 0.0
    t = m.group(1)
    return float.fromhex(t) if "x" in t.lower() else float(t)


def _parse(argv):
    """main.cpp:246-379 as bin/raytracer restates it: flags anywhere, the value is the next token read with atoi / atof
    (`--width abc` is width 0, not a usage error); only a MISSING value is a usage error — and for --gillum a warning."""
    opt = dict(path=None, output=None, width=1920, height=1080, fov=60.0, gillum=None, jsample=None, depth=3, shadow=False, seed=1, tile_rows=8)
    given = set()  # --strict-scn: the .scn's film_resolution / max_depth hold for what the command line leaves open

    def value(i, kind, what):
        if i + 1 >= len(argv):
            raise ValueError(what)
        return kind(argv[i + 1])

    for i, a in enumerate(argv):
        if a == "--path":
            opt["path"] = value(i, str, "path must be passed after --path")
        elif a == "--output":
            opt["output"] = value(i, str, "output path must be passed after --output")
        elif a == "--width":
            opt["width"] = value(i, _atoi, "width takes an int after flag for the width")
            given.add("width")
        elif a == "--height":
            opt["height"] = value(i, _atoi, "height takes an int after flag for the width")
            given.add("height")
        elif a == "--fov":
            opt["fov"] = value(i, _atof, "fov takes a float (degrees) after flag for the field of view")
            given.add("fov")
        elif a == "--gillum":
            if i + 1 < len(argv):  # main.cpp:250-253: monte_carlo = true, num_path_traces = atoi(next) — 0 for a non-number
                opt["gillum"] = _atoi(argv[i + 1])
            else:  # main.cpp:258 warns and goes on
                print("gillum takes an int after flag for the number of paths traced", file=sys.stderr)
        elif a == "--jsample":
            opt["jsample"] = value(i, _atoi, "jsample takes an int after flag for the supersampling grid size")
        elif a == "--depth":
            opt["depth"] = value(i, _atoi, "depth takes a positive int after flag for the max depth")
            if opt["depth"] <= 0:
                raise ValueError("depth takes a positive int after flag for the max depth")
            given.add("depth")
        elif a == "--shadow":
            opt["shadow"] = True
        elif a == "--strict-scn":
            opt["strict_scn"] = True
        elif a == "--scn-fog":
            opt["scn_fog"] = True
        elif a == "--scn-spot":
            opt["scn_spot"] = True
        elif a == "--light-radius":
            opt["light_radius"] = value(i, _atof, "light-radius takes a float (the radius of every point and spot light)")
        elif a == "--scn-motion":
            opt["scn_motion"] = True
        elif a == "--scn-texture":
            opt["scn_texture"] = True
        elif a == "--scn-emission":
            opt["scn_emission"] = True
        elif a == "--shutter":
            opt["shutter"] = value(i, _atof, "shutter takes a float (how long the shutter is open)")
        elif a == "--envmap":
            opt["envmap"] = value(i, str, "envmap takes the path of a square colour PFM file (the scene's environment)")
        elif a == "--aperture":
            opt["aperture"] = value(i, _atof, "aperture takes a float (the radius of the lens)")
        elif a == "--focus":
            opt["focus"] = value(i, _atof, "focus takes a float (the t of the primary rays that is in focus)")
        elif a == "--scn-fov":
            opt["scn_fov"] = True
        elif a == "--shade-triangles":
            opt["shade_triangles"] = True
        elif a == "--triangle-shadows":
            opt["triangle_shadows"] = True
        elif a == "--sphere-tree":
            opt["sphere_tree"] = True
        elif a == "--legacy-reflect":
            opt["legacy_reflect"] = True
        elif a == "--progressive":
            opt["progressive"] = max(1, value(i, _atoi, "progressive takes the number of passes"))
        elif a == "--progressive-every":
            opt["progressive_every"] = max(0, value(i, _atoi, "progressive-every takes a number of passes"))
        elif a == "--format":
            opt["format"] = value(i, str, "format takes ppm, png or pfm")
        elif a == "--denoise":
            opt["denoise"] = value(i, _atoi, "denoise takes a number of iterations")
        elif a == "--adaptive":
            opt["adaptive"] = value(i, _atof, "adaptive takes a float (the relative standard error at which a pixel stops)")
        elif a == "--adaptive-min":
            opt["adaptive_min"] = value(i, _atoi, "adaptive-min takes the number of passes every pixel gets")
        elif a == "--adaptive-max":
            opt["adaptive_max"] = value(i, _atoi, "adaptive-max takes the largest number of passes of a pixel")
        elif a == "--adaptive-denoise":
            opt["adaptive_denoise"] = value(i, _atoi, "adaptive-denoise takes a number of iterations")
        elif a == "--seed":
            opt["seed"] = value(i, _atoi, "seed takes an int")
        elif a == "--tile-rows":
            opt["tile_rows"] = value(i, _atoi, "tile-rows takes a positive int")
    if opt["tile_rows"] <= 0:
        raise ValueError("tile-rows takes a positive int")
    if opt.get("format", "ppm") not in ("ppm", "png", "pfm"):
        raise ValueError("format takes ppm, png or pfm")
    if opt.get("strict_scn") or opt.get("scn_fov"):
        opt["_given"] = given
    if opt["path"] is None:
        raise ValueError("no scene file was passed. Pass with --path path_to_scn")
    if opt["output"] is None:
        raise ValueError("no output destination was passed. Pass with --output destination_path.ppm")
    return opt


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    try:
        o = _parse(argv)
    except ValueError as e:
        print(str(e), file=sys.stderr)
        return 0  # the reference's usage errors leave with status 0
    if o["width"] <= 0 or o["height"] <= 0 or o["width"] > 65536 or o["height"] > 65536:
        print("raytracer: bad image size %dx%d" % (o["width"], o["height"]), file=sys.stderr)  # as bin/raytracer: before anything is sized from it
        return 2
    radius = o.get("light_radius")
    if radius is not None and not (math.isfinite(radius) and radius >= 0.0):
        print("raytracer: --light-radius takes a finite radius >= 0", file=sys.stderr)  # as bin/raytracer
        return 2
    aperture, focus = o.get("aperture"), o.get("focus", 1.0)
    if aperture is not None and not (math.isfinite(aperture) and aperture >= 0.0 and math.isfinite(focus) and focus > 0.0):
        print("raytracer: --aperture takes a finite radius >= 0 and --focus a finite distance > 0", file=sys.stderr)  # as bin/raytracer
        return 2
    import skele_raytracer_amd as skr
    env = None
    if o.get("envmap") is not None:  # --envmap FILE.pfm: read and checked on the host before anything touches the GPU, as bin/raytracer does
        try:
            env = skr.read_pfm(o["envmap"])
            if env.shape[0] != env.shape[1] or env.shape[0] > skr.binding.ENV_MAX_EDGE:
                raise skr.SkrError("the environment must be square with an edge of at most %d, the file is %d x %d" % (skr.binding.ENV_MAX_EDGE, env.shape[1], env.shape[0]))
        except skr.SkrError as e:
            print("raytracer: --envmap %s: %s" % (o["envmap"], e), file=sys.stderr)
            return 2
    import torch
    import torch.distributed as dist
    from .distributed import FrameSharder

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise skr.SkrError("no MI355X visible: the renderer has no CPU path")
    # SKR_REHEARSE_GLOO=1: every rank on GPU 0, collectives over gloo (rehearsal of the N > 1 path on a one-GPU box)
    rehearsal = world > 1 and os.environ.get("SKR_REHEARSE_GLOO") == "1"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)  # RCCL over xGMI
    shutter = o.get("shutter")
    if shutter is not None and not (math.isfinite(shutter) and shutter >= 0.0):
        print("raytracer: --shutter takes a finite number >= 0", file=sys.stderr)  # as bin/raytracer
        return 2
    try:
        scene = skr.parse_scene(o["path"], strict=bool(o.get("strict_scn")), fog=bool(o.get("scn_fog")), triangle_shadows=bool(o.get("triangle_shadows")),
                                sphere_tree=bool(o.get("sphere_tree")), spot=bool(o.get("scn_spot")), motion=bool(o.get("scn_motion")), texture=bool(o.get("scn_texture")),
                                emission=bool(o.get("scn_emission")))
    except skr.SkrError as e:
        if rank == 0:
            print(str(e))  # scene.cpp:24: "Can't open file" on stdout, exit(0)
        if world > 1:
            dist.destroy_process_group()
        return 0
    if o.get("strict_scn"):  # as bin/raytracer --strict-scn: the .scn's film_resolution and max_depth for what argv leaves open
        info = scene.info
        if "width" not in o["_given"] and info.film_width > 0:
            o["width"] = info.film_width
        if "height" not in o["_given"] and info.film_height > 0:
            o["height"] = info.film_height
        if "depth" not in o["_given"] and info.max_depth_parsed > 0:
            o["depth"] = info.max_depth_parsed
    if o.get("scn_fov") and "fov" not in o["_given"]:  # as bin/raytracer --scn-fov: 2 x the camera line's half_height_angle unless --fov is given
        o["fov"] = skr.scene_fov(scene)
    if radius is not None:  # as bin/raytracer --light-radius: every point and spot light of the loaded scene (include/skr.h skr_scene_set_light_radii)
        scene.set_light_radii(radius)
    if aperture is not None:  # as bin/raytracer --aperture A [--focus F]: a thin lens (include/skr.h skr_scene_set_lens); --focus alone has no effect
        scene.set_lens(aperture, focus)
    if shutter is not None:  # as bin/raytracer --shutter S (include/skr.h skr_scene_set_shutter); without velocities it has no effect
        scene.set_shutter(shutter)
    if env is not None:  # as bin/raytracer --envmap FILE.pfm: the scene's environment (include/skr.h skr_scene_set_environment)
        try:
            scene.set_environment(env)
        except skr.SkrError as e:  # (a texel that is not finite)
            if rank == 0:
                print("raytracer: --envmap %s: %s" % (o["envmap"], e), file=sys.stderr)
            if world > 1:
                dist.destroy_process_group()
            return 2
    r = skr.Renderer(scene, local_rank)
    kw = dict(fov=o["fov"], depth=o["depth"], shadow=o["shadow"], seed=o["seed"], shade_triangles=bool(o.get("shade_triangles")), progressive=o.get("progressive", 1), legacy_reflect=bool(o.get("legacy_reflect")))
    if o["gillum"] is not None:
        kw["gillum"] = o["gillum"]
    if o["jsample"] is not None:
        kw["jsample"] = o["jsample"]
    opt = skr.Options(o["width"], o["height"], **kw)
    fmt, every = o.get("format", "ppm"), o.get("progressive_every", 0)
    if world > 1 and (fmt == "pfm" or every):
        # the ranks exchange quantised tiles (one all-gather of bytes): the float frame and the running mean stay on their devices
        if rank == 0:
            print("raytracer: --format pfm and --progressive-every need the single-device path", file=sys.stderr)
        dist.destroy_process_group()
        return 2
    denoise = o.get("denoise")
    if denoise is not None and (world > 1 or every or not 0 <= denoise <= 16):
        # the filter needs whole-frame neighbours (the ranks exchange quantised tiles) and filters the finished mean only
        if rank == 0:
            print("raytracer: --denoise takes 0 .. 16 iterations on the single-device path (no world > 1, no --progressive-every)", file=sys.stderr)
        if world > 1:
            dist.destroy_process_group()
        return 2
    adaptive = o.get("adaptive")
    if adaptive is not None and (o.get("progressive", 1) > 1 or every or world > 1 or denoise is not None):
        # the passes are chosen per pixel on one device; --denoise estimates its variance spatially, --adaptive-denoise takes the measured one
        if rank == 0:
            print("raytracer: --adaptive cannot be combined with --progressive K > 1, --progressive-every, --gpus N > 1 or --denoise "
                  "(--adaptive-denoise L filters an adaptive frame)", file=sys.stderr)
        if world > 1:
            dist.destroy_process_group()
        return 2
    adaptive_denoise = o.get("adaptive_denoise")
    if adaptive_denoise is not None and (adaptive is None or denoise is not None or not 0 <= adaptive_denoise <= 16):
        if rank == 0:
            print("raytracer: --adaptive-denoise takes 0 .. 16 iterations, needs --adaptive T and excludes --denoise", file=sys.stderr)
        if world > 1:
            dist.destroy_process_group()
        return 2
    if adaptive is not None:
        try:
            lo, hi = o.get("adaptive_min", skr.ADAPTIVE_MIN_PASSES), o.get("adaptive_max", skr.ADAPTIVE_MAX_PASSES)
            if adaptive_denoise is not None:
                rgb, rgbf, passes, ms = r.render_adaptive_denoised(opt, adaptive, lo, hi, adaptive_denoise, want_float=(fmt == "pfm"))
            else:
                rgb, rgbf, passes, ms = r.render_adaptive_host(opt, adaptive, lo, hi, want_float=(fmt == "pfm"))
        except skr.SkrError as e:
            print("raytracer: %s" % e, file=sys.stderr)
            return 2
        if fmt == "pfm":
            skr.write_pfm(o["output"], rgbf)
        else:
            (skr.write_png if fmt == "png" else skr.write_ppm)(o["output"], rgb)
        print("***\nWROTE TO PPM\n***")  # main.cpp:213
        nmax = o.get("adaptive_max", skr.ADAPTIVE_MAX_PASSES)
        print("adaptive: %.3f passes per pixel, %.2f %% of the pixels at max (%d)" % (float(passes.mean(dtype=np.float64)), 100.0 * float((passes == nmax).mean()), nmax),
              file=sys.stderr)
        print("1 GPU(s), %dx%d, %.3f ms (device, adaptive), kernel %s" % (o["width"], o["height"], ms, r.kernel_variant()), file=sys.stderr)
        return 0
    if denoise is not None:
        rgb, rgbf, ms = r.render_denoised(opt, denoise, want_float=(fmt == "pfm"))
        if fmt == "pfm":
            skr.write_pfm(o["output"], rgbf)
        else:
            (skr.write_png if fmt == "png" else skr.write_ppm)(o["output"], rgb)
        print("***\nWROTE TO PPM\n***")  # main.cpp:213
        print("1 GPU(s), %dx%d, %.3f ms (device, denoised), kernel %s" % (o["width"], o["height"], ms, r.kernel_variant()), file=sys.stderr)
        return 0
    if fmt == "pfm" or every:
        # the file is the window (main.cpp:183-197 redraws its SDL window as rows finish): rewritten with the mean so far
        def write(rgb, rgbf):
            if fmt == "pfm":
                skr.write_pfm(o["output"], rgbf)
            else:
                (skr.write_png if fmt == "png" else skr.write_ppm)(o["output"], rgb)

        def progress(done, total, rgb, rgbf):
            if done < total:
                write(rgb, rgbf)
            print("pass %d of %d" % (done, total))
            return False

        opt = skr.Options(o["width"], o["height"], **kw)
        rgb, rgbf, ms = r.render_progressive_host(opt, every, want_float=(fmt == "pfm"), progress=progress if every else None)
        write(rgb, rgbf)
        print("***\nWROTE TO PPM\n***")  # main.cpp:213
        print("1 GPU(s), %dx%d, %.3f ms (device), kernel %s" % (o["width"], o["height"], ms, r.kernel_variant()), file=sys.stderr)
        return 0
    sharder = FrameSharder(o["width"], o["height"], o["tile_rows"], rank, world, dev)
    stream = torch.cuda.current_stream(dev)
    t0 = time.perf_counter()
    frame = sharder.step(lambda buf: r.render_tiles_into(opt, o["tile_rows"], rank, world, buf.data_ptr(), None, stream.cuda_stream))
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    if rank == 0:
        (skr.write_png if fmt == "png" else skr.write_ppm)(o["output"], frame.cpu().numpy())
        print("***\nWROTE TO PPM\n***")  # main.cpp:213
        print("%d GPU(s), %dx%d, %.3f ms (render + gather), kernel %s" % (world, o["width"], o["height"], dt * 1e3, r.kernel_variant()), file=sys.stderr)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
