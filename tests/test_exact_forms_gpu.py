"""The hit root from binary32 pairs on the device: skr_debug_eval op 19 (near_root, near_root_exact and the interval between them, the
functions the kernels call) over the families of tests/test_exact_forms_cpu.py, about 5e5 records."""
import numpy as np
import pytest

import exact_forms_cases as xc
from skele_raytracer_amd import binding

pytestmark = pytest.mark.gpu
N = 1 << 17
ROOT_OP = 19  # include/skr.h skr_debug_eval


def test_root_pairs_return_the_binary64_forms_float_on_the_device():
    fams = xc.families(N)
    recs = {name: xc.records(fam) for name, fam in fams.items()}
    out = binding.debug_eval(ROOT_OP, np.concatenate(list(recs.values())).view(np.uint32), 7)
    at = 0
    for name, rec in recs.items():
        xc.check(name, rec, out[at:at + len(rec)])
        at += len(rec)
    assert at >= 450000


def test_records_outside_the_ranges_take_the_binary64_form_on_the_device():
    rng = np.random.default_rng(31)
    n = 1 << 14
    rec = np.stack([2.0 ** rng.uniform(-60, 60, n), -(2.0 ** rng.uniform(-60, 60, n)), 2.0 ** rng.uniform(-90, 90, n)], 1).astype(np.float32)
    rec[::7, rng.integers(0, 3)] = np.float32(np.nan)
    rec[3::11, 2] *= np.float32(-1)
    out = binding.debug_eval(ROOT_OP, rec.view(np.uint32), 7)
    outside = ~xc.in_ranges(rec)
    assert outside.sum() > n // 4 and (~outside).sum() > n // 64
    assert (out[outside, 2] == 1).all()
    assert (out[:, 0] == out[:, 1]).all()
