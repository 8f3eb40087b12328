"""Cases and assertions for the hit root from binary32 pairs (device_math.h near_root), shared by tests/test_exact_forms_cpu.py (the C
restatement, tests/exact_forms_checker.c) and tests/test_exact_forms_gpu.py (the device's own function, skr_debug_eval op 19).
numpy only, seeded, no GPU.

A record is (2a, b, D), the coefficients of utils.h:115-118 / :89 in binary32 as tests/predicate_cases.py forms them; a result is the
seven words of op 19: near_root, near_root_exact, 1 where the binary64 form was taken, lo, hi, q_h, q_l."""
import ctypes as C
import os
import subprocess

import numpy as np

import predicate_cases as pc

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "exact_forms_checker.c")
E_SCALE = 2.0 ** -41   # E = (s + |n_h|) / 2a * 2^-41 (DESIGN.md "The root from binary32 pairs")
RATIO_MAX = 0.25       # the derivation leaves a factor >= 4: |q_h + q_l - binary64 quotient| <= E / 4
SHARE_MIN = {"baseline": 0.99, "ground": 0.95}  # of the records with a root: decided by the short path, at least


def ground(n, seed=23):
    """Origins 0.01 .. 3 above a sphere of radius 1000, rays back onto it: the headline scene's floor, where -b and sqrt(D) nearly
    cancel (t2 is 1e-3 of either)."""
    rng = np.random.default_rng(seed)
    Cc = np.tile(np.array([0.0, -1000.0, 0.0]), (n, 1))
    r = np.full(n, 1000.0)
    up = pc._unit(rng, n) * 0.05 + np.array([0.0, 1.0, 0.0])
    up /= np.linalg.norm(up, axis=1, keepdims=True)
    o = Cc + up * (r + 10.0 ** rng.uniform(-2, np.log10(3.0), n))[:, None]
    to = up + pc._perp(pc._unit(rng, n), up) * (10.0 ** rng.uniform(-5, -1.5, n))[:, None]
    to /= np.linalg.norm(to, axis=1, keepdims=True)
    aim = Cc + to * r[:, None]
    d = (aim - o.astype(f32)) * (10.0 ** rng.uniform(-0.5, 0.5, n))[:, None]
    return pc._family(o, d, Cc, r)


def families(n):
    """name -> family: unit_families(n) (threshold, tangent, surface, baseline, nonfinite, the scale sweep), a baseline of n, the ground."""
    fams = dict(pc.unit_families(n))
    fams["baseline"] = pc.baseline(n, 11)
    fams["ground"] = ground(n)
    return fams


def records(fam):
    """float32 [n, 3] = (2a, b, D)"""
    a, b, _, D = pc.coeffs(fam["o"], fam["d"], fam["C"], pc.r2_of(fam))
    with np.errstate(all="ignore"):
        return np.stack([(f32(2) * a).astype(f32), b, D], 1).astype(f32)


def in_ranges(rec):
    """The ranges near_root_pair states: 2^-40 <= 2a < 2^40, 2^-60 <= D < 2^60, sqrt(D) <= -b < 2^40 (binary32 sqrt, correctly rounded)."""
    two_a, b, D = (rec[:, k] for k in range(3))
    with np.errstate(all="ignore"):
        s = np.sqrt(D)
        return (two_a >= f32(2.0 ** -40)) & (two_a < f32(2.0 ** 40)) & (D >= f32(2.0 ** -60)) & (D < f32(2.0 ** 60)) & (-b >= s) & (-b < f32(2.0 ** 40))


def check(name, rec, out, say=print):
    """The assertions of both tests on one family's results (uint32 [n, 7]).  Returns the share the short path decided."""
    two_a, b, D = (rec[:, k] for k in range(3))
    root, exact, took_exact = out[:, 0], out[:, 1], out[:, 2]
    lo, hi, q_h, q_l = (out[:, k].view(f32) for k in (3, 4, 5, 6))
    with np.errstate(all="ignore"):  # utils.h:87-110 as predicate_cases.root_t2 states it, on 2a as given
        t = (((-b).astype(np.float64) - np.sqrt(D.astype(np.float64))) / two_a.astype(np.float64)).astype(f32)
        want = np.where(t >= 0, t, pc.INF).astype(f32)
    same = lambda x, y: (x == y) | (np.isnan(x.view(f32)) & np.isnan(y.view(f32)))
    assert same(exact, want.view(np.uint32)).all(), "%s: the binary64 form differs from the numpy restatement" % name
    assert same(root, exact).all(), "%s: %d roots differ from the binary64 form" % (name, int((~same(root, exact)).sum()))
    short = took_exact == 0
    outside = ~in_ranges(rec)
    assert not (short & outside).any(), "%s: %d records outside the stated ranges took the short path" % (name, int((short & outside).sum()))
    assert (lo[short] == hi[short]).all() and (lo[short].view(np.uint32) == root[short]).all()
    ratio = 0.0
    if short.any():
        k = short
        with np.errstate(all="ignore"):
            q64 = ((-b[k]).astype(np.float64) - np.sqrt(D[k].astype(np.float64))) / two_a[k].astype(np.float64)
            s = np.sqrt(D[k])
            E = (s.astype(np.float64) + np.abs((-b[k]) - s).astype(np.float64)) / two_a[k].astype(np.float64) * E_SCALE
            ratio = float(np.max(np.abs(q_h[k].astype(np.float64) + q_l[k].astype(np.float64) - q64) / E))
    # The share is taken over the records that HAVE a root, a finite t2 >= 0: half the baseline's rays miss their sphere (D < 0) or
    # leave it behind (b >= 0, t2 < 0 -> +inf), and no form has a root to decide there (the kernels ask for the root of a candidate only).
    has_root = np.isfinite(exact.view(f32))
    share = float(short[has_root].mean()) if has_root.any() else 1.0
    say("%-12s n = %7d  with a root %7d  short path %9.5f %% of them  max |q_h + q_l - q64| / E = %.4f" % (name, len(rec), int(has_root.sum()), 100 * share, ratio))
    assert ratio <= RATIO_MAX, "%s: |q_h + q_l - q64| / E = %.4f" % (name, ratio)
    if name in SHARE_MIN:
        assert share >= SHARE_MIN[name], "%s: the short path decided %.3f %% of the records" % (name, 100 * share)
    return share


def build_checker(out_dir):
    """tests/exact_forms_checker.c compiled into out_dir (-ffp-contract=off; -mfma where the CPU has it, else libm's fmaf)."""
    so = os.path.join(out_dir, "libexactforms.so")
    flags = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra"]
    with open("/proc/cpuinfo") as f:
        if " fma " in f.read():
            flags.append("-mfma")
    subprocess.check_call(["gcc", *flags, "-shared", "-o", so, SRC, "-lm"])
    L = C.CDLL(so)
    L.skx_near_root.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    L.skx_near_root.restype = None

    def near_root(rec):
        rec = np.ascontiguousarray(rec, f32)
        out = np.zeros((len(rec), 7), np.uint32)
        L.skx_near_root(len(rec), rec.ctypes.data, out.ctypes.data)
        return out
    return near_root
