#!/usr/bin/env python3
"""Randomised GPU-vs-checker campaign over spot lights, lights with a radius, triangle shadows under them and the thin lens (development
aid; the committed tests hold 64 cases of one seed and the edge families): the random family of tests/light_mode_cases.py at any case
count and seed, each case compared as tests/test_light_modes_gpu.py compares it — the frame's float words, bytes and four work counts,
the kernel variant, SKR_NO_CULL=1 on meshes, then 257 query rays — against tests/soft_light_checker.c and tests/lens_checker.c.
tests/fuzz_parity.py is the counterpart for the modes the frozen oracle knows.

    python tests/fuzz_light_modes.py [cases=200] [seed=1]
    FUZZ_ONLY=<index> python tests/fuzz_light_modes.py [cases] [seed]      replay one case, with its scene text

A mismatch is a finding: one line, and the campaign runs on.  A launch the library refuses (SkrError) is reported and skipped.  Any other
exception ends the campaign at once: after a HIP error nothing further is started on the GPU."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import skele_raytracer_amd as skr  # noqa: E402
import light_mode_cases as lm  # noqa: E402
from lens_check import build as build_lens_checker  # noqa: E402
from soft_light_check import build as build_soft_checker  # noqa: E402
from test_light_modes_gpu import check_case  # noqa: E402


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    only = int(os.environ["FUZZ_ONLY"]) if os.environ.get("FUZZ_ONLY") else None
    tmp = tempfile.mkdtemp()
    soft, lens = build_soft_checker(tmp), build_lens_checker(tmp)
    print("command line: %s (FUZZ_ONLY=%s)" % (" ".join(sys.argv), os.environ.get("FUZZ_ONLY", "")), flush=True)
    bad = refused = 0
    seen = {}
    for index in range(cases):
        if only is not None and index != only:
            continue
        case = lm.random_case(index, tmp, seed)
        try:
            differs, variant = check_case(torch, soft, lens, case)
        except skr.SkrError as e:
            if "(status 4)" not in str(e):  # include/skr.h SKR_ERR_UNSUPPORTED: launch_params refuses the configuration
                raise  # anything else, a HIP error among them: the campaign ends here
            refused += 1
            print("case %d refused (%s): %s" % (index, case.kw, str(e)[:120]), flush=True)
            continue
        seen[variant] = seen.get(variant, 0) + 1
        if differs:
            bad += 1
            print("MISMATCH case %d seed %d: %s %dx%d %s flags=%s radii=%s lens=%s variant=%s: %s" % (index, seed, case.scene, case.w, case.h, case.kw, case.flags,
                  case.radii.tolist(), case.lens, variant, "; ".join(differs)), flush=True)
            if only is not None:
                print(open(case.scene).read(), flush=True)
        if index % 50 == 49:
            print("%d cases, %d mismatches, %d refused" % (index + 1, bad, refused), flush=True)
    print("done: %d cases under seed %d, %d mismatches, %d refused; kernel variants: %s" % (cases, seed, bad, refused, ", ".join("%s x %d" % kv for kv in sorted(seen.items()))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
