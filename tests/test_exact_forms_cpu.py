"""The hit root from binary32 pairs on the host (no GPU): tests/exact_forms_checker.c, a C restatement of device_math.h near_root_pair,
against the binary64 form of utils.h:87-110 over the boundary families of the filtered predicates and the headline scene's floor
(DESIGN.md "The root from binary32 pairs")."""
import re

import numpy as np
import pytest

import exact_forms_cases as xc

N = 1 << 15


@pytest.fixture(scope="module")
def near_root(tmp_path_factory):
    return xc.build_checker(str(tmp_path_factory.mktemp("exactforms")))


def test_root_pairs_return_the_binary64_forms_float(near_root):
    shares = {}
    for name, fam in xc.families(N).items():
        rec = xc.records(fam)
        shares[name] = xc.check(name, rec, near_root(rec))
    assert set(xc.SHARE_MIN) <= set(shares)


def test_records_outside_the_ranges_take_the_binary64_form(near_root):
    rec = np.array([[2.0, -4.0, 2.0 ** 60], [2.0, -4.0, 2.0 ** -61], [2.0 ** 40, -4.0, 4.0], [2.0 ** -41, -4.0, 4.0], [2.0, -1.0, 4.0],
                    [2.0, 1.0, 0.5], [2.0, -(2.0 ** 40), 4.0], [2.0, -4.0, -1.0], [np.nan, -4.0, 4.0], [2.0, np.nan, 4.0], [2.0, -4.0, np.nan],
                    [np.inf, -4.0, 4.0], [2.0, -np.inf, 4.0], [2.0, -4.0, np.inf], [0.0, -4.0, 4.0], [2.0, -4.0, 0.0], [2.0, -2.0, 4.0]], np.float32)
    out = near_root(rec)
    assert (out[:, 2] == 1).all()
    assert (out[:, 0] == out[:, 1]).all()
    inside = np.array([[2.0, -4.0, 4.0], [2.0 ** -40, -4.0, 4.0], [2.0, -4.0, 2.0 ** -60], [2.0, -2.0, 3.0]], np.float32)
    out = near_root(inside)
    assert (out[:, 2] == 0).all() and (out[:, 0] == out[:, 1]).all()


def test_header_names_the_op():
    import os
    with open(os.path.join(xc.ROOT, "include", "skr.h")) as f:
        assert re.search(r"#define SKR_HAS_ROOT_PAIRS 1\b", f.read())
