#!/usr/bin/env python3
"""Event counts of one headline frame from a diagnostic build (-DSKR_DIAG=1, loaded through SKR_LIBRARY):
how often the sphere loops take their candidate paths, how full the shading batches are."""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import skele_raytracer_amd as skr
from skele_raytracer_amd import binding
r = skr.Renderer(skr.parse_scene(os.path.join(ROOT, "tests/golden/scenes/spheres2.scn")))
opt = skr.Options(1920, 1080, gillum=16, shadow=True, seed=20261004)
L = binding.lib()
out = np.zeros(36, np.uint64)  # SKR_DIAG_SLOTS (device_math.h)
r.render(opt); torch.cuda.synchronize()
L.skr_diag_read_nodes(C.c_void_p(out.ctypes.data), 1)
r.render(opt); torch.cuda.synchronize()
L.skr_diag_read_nodes(C.c_void_p(out.ctypes.data), 1)
# (the counters of render_nodes.hip's translation unit: the trace, leaf and finalize kernels of the node pipeline)
names = ["closest-pair iterations", "closest-pair candidate paths", "  lanes in them", "exact-root fallbacks of bracket tests, pair and scalar (lanes)", "shadow-pair iterations", "shadow candidate paths",
         "  lanes in them", "exact-root fallbacks, bracket (pair and scalar) and any-hit tests (wave events)", "bracket overlaps -> exact loop (wave events)", "leaf shading batches", "  hits in them",
         "activation batches", "  records in them", "closest-pair candidate RAYS", "  accepted", "shadow candidate RAYS", "  occluders found", "  closest-pair candidates a t2 <= 1 pre-test rejects", "  closest-pair candidate paths left with it",
         "masked shadow-pair calls (wave events)", "  (a) spheres named by some lane, summed", "  (b) most spheres one lane names, summed", "  ns, summed",
         "  spheres named, summed over lanes", "  lanes in them",
         "masked closest-pair calls (wave events)", "  (a) spheres named by some lane, summed", "  (b) most spheres one lane names, summed", "  ns, summed",
         "  spheres named, summed over lanes", "  lanes in them", "  calls with a lane that names every sphere",
         "roots near_root was asked for (lanes)", "  of them from the binary64 form (lanes)", "near_root calls (wave events)", "  of them with a lane in the binary64 form (wave events)"]
print(r.kernel_variant())
for n, v in zip(names, out):
    if v: print("%-48s %d" % (n, v))
if out[32]:  # the share of roots the binary32 pair form could not decide (DESIGN.md "The root from binary32 pairs")
    print("near_root: binary64 form for %.4f %% of the lanes, in %.3f %% of the wave events" % (100.0 * out[33] / out[32], 100.0 * out[35] / max(out[34], 1)))
if out[19]:  # the gate of DESIGN.md "Shadow masks": per masked shadow-pair call of a wave, against ns
    print("per masked shadow-pair call: (a) %.2f  (b) %.2f  lane mean %.2f  of ns = %.2f"
          % (out[20] / out[19], out[21] / out[19], out[23] / max(out[24], 1), out[22] / out[19]))
if out[25]:  # the gate of DESIGN.md "GI masks": per masked closest-pair call of a wave, against ns
    print("per masked closest-pair call: (a) %.2f  (b) %.2f  lane mean %.2f  of ns = %.2f; waves walking every sphere %.1f %%"
          % (out[26] / out[25], out[27] / out[25], out[29] / max(out[30], 1), out[28] / out[25], 100.0 * out[31] / out[25]))
