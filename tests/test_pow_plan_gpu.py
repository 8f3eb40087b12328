"""The shaped leaf instances compiled for an exponent mask (csrc/launch.h skr_leaf_pow_plan, csrc/device_math.h pow_int_sparse), on the
MI355X (pytest -m gpu): the sparse pow against the full one and the oracle's, bit for bit, for every exponent inside each listed mask;
and frames whose launch gets a mask against the same frames under SKR_LEAF_POW=0 (all seven steps), under SKR_LEAF_SHAPE=0 (the
run-time instance) and against the CPU oracle — float words, bytes and the four work counts.  SKR_FLAT=0 and the variant, the shape and
the mask are asserted, so that the leaf kernel's instance under test is what ran.

16-byte records: --gillum 4 tables never exceed the smallest budget (1 MiB), so those cases take the launch tests/test_wide_records_gpu.py
takes for them, 16x36 at --gillum 97 under 1 MiB."""
import os

import numpy as np
import pytest

import skele_raytracer_amd as skr
from skele_raytracer_amd import binding
from pow_plan_cases import FULL, MASKS, NO_PLAN, P30, PLANS, SWITCHES, last_leaf, leaf_pow, write_scene
from test_record_tables_host import narrow_budget, plan

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


# --------------------------------------------------------------------------------------------------------------- the unit level ----
def pow_x():
    rng = np.random.default_rng(20261021)
    edge = np.array([0.0, 1e-45, 2.0 ** -100, np.nextafter(f32(1), f32(0)), 1.0, np.nextafter(f32(1), f32(2)), np.finfo(f32).max, np.inf], f32)
    assert edge[1] > 0 and edge[1].view(np.uint32) == 1  # the smallest denormal
    return np.concatenate([edge, rng.random(1500).astype(f32), (1.0 + rng.random(1500)).astype(f32)])


def inside(mask):
    return [n for n in range(1, 128) if n & ~mask == 0]


def test_sparse_pow_equals_the_full_one_inside_its_mask(gpu, oracle):
    """Op 23 (x, p, mask) for every integer p inside each listed mask: the bits of op 20's two instances (steps = 7) and of
    sko_powf_shared, which is what tests/test_shading_values_gpu.py holds op 20 to.  Exponents that are not plain take the cold path
    in every instance."""
    x = pow_x()
    L = oracle.lib()
    assert sorted(inside(P30)) == [16, 32, 48] and len(inside(FULL)) == 127
    for mask in MASKS:
        ps = [float(n) for n in inside(mask)] + [0.0, 0.2, 0.5, 2000.0, 1025.0]
        xx = np.tile(x, len(ps))
        pp = np.repeat(f32(ps), len(x))
        rec = np.stack([xx.view(np.uint32), pp.view(np.uint32), np.full(len(xx), mask, np.uint32)], 1)
        got = binding.debug_eval(23, rec, 1)[:, 0]
        rec[:, 2] = 7
        full = binding.debug_eval(20, rec, 2)
        want = f32([L.sko_powf_shared(float(a), float(b)) for a, b in zip(xx, pp)]).view(np.uint32)
        for name, ref in (("powf_spec<true>", full[:, 1]), ("powf_spec<false>", full[:, 0]), ("sko_powf_shared", want)):
            bad = got != ref
            assert not bad.any(), "mask %#x against %s: %d of %d differ, first (x, p) = %s" % (
                mask, name, int(bad.sum()), len(bad), [(float(a), float(b)) for a, b in zip(xx[bad][:3], pp[bad][:3])])


def test_an_unlisted_mask_has_no_instance(gpu):
    rec = np.array([[f32(0.5).view(np.uint32), f32(16).view(np.uint32), 0x10]], np.uint32)
    assert binding.debug_eval(23, rec, 1)[0, 0] == 0xFFFFFFFF


# -------------------------------------------------------------------------------------------------------------- the frame level ----
_ORACLE = {}


def want(oracle, path, w, h, kw):
    key = (path, w, h, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        rgb, f, st = oracle.render(path, w, h, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw)
        _ORACLE[key] = (rgb, f.view(np.uint32), tuple(int(v) for v in st[:4]))
    return _ORACLE[key]


def frame(gpu, monkeypatch, path, opt, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = skr.parse_scene(path)
    r = skr.Renderer(scene)
    try:
        r.work(reset=True)
        rgb, rgbf = r.render(opt, want_float=True)
        gpu.cuda.synchronize()
        wk = r.work(reset=True)
        return (rgb.cpu().numpy(), rgbf.cpu().numpy().view(np.uint32), (wk["radiance_rays"], wk["sphere_hits"], wk["shadow_rays"], wk["sphere_tests"]),
                r.kernel_variant(), last_leaf(r), leaf_pow(scene, opt))
    finally:
        r.close()


def assert_same(got, exp, what):
    assert got[0].shape == exp[0].shape, (what, got[0].shape, exp[0].shape)
    assert np.array_equal(got[1].reshape(-1), exp[1].reshape(-1)), "%s: %d float words differ" % (what, int((got[1].reshape(-1) != exp[1].reshape(-1)).sum()))
    assert np.array_equal(got[0], exp[0]), "%s: bytes differ at %d pixels" % (what, int((got[0] != exp[0]).any(-1).sum()))
    assert got[2] == exp[2], (what, got[2], exp[2])


def check(gpu, oracle, monkeypatch, path, w, h, kw, lights, mask, env=None):
    env = dict({"SKR_FLAT": "0"}, **(env or {}))
    opt = skr.Options(w, h, **kw)
    got = frame(gpu, monkeypatch, path, opt, env)
    full = frame(gpu, monkeypatch, path, opt, dict(env, SKR_LEAF_POW="0"))
    run = frame(gpu, monkeypatch, path, opt, dict(env, SKR_LEAF_SHAPE="0"))
    for f in (got, full, run):
        assert f[3] == "node_levels_v5", f[3]
    assert got[4] == (lights, mask) and got[5] == mask, (got[4], got[5], mask)
    assert full[4] == (lights, FULL) and run[4] == (0, NO_PLAN), (full[4], run[4])
    exp = want(oracle, path, w, h, kw)
    assert exp[2][0] > 0 and exp[2][1] > 0 and exp[2][2] > 0, exp[2]
    what = "%s %s" % (os.path.basename(path), kw)
    assert_same(got, full, what + " against SKR_LEAF_POW=0")
    assert_same(got, run, what + " against SKR_LEAF_SHAPE=0")
    assert_same(got, exp, what + " against the oracle")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pow_plan_gpu"))


def scene_file(folder, powers, lights):
    path = os.path.join(folder, "p%s_l%d.scn" % ("_".join("%g" % p for p in powers), lights))
    return path if os.path.exists(path) else write_scene(path, powers, lights=lights)


SIZES = [(48, 27), (64, 36)]
# the two sets the kernels of real scenes run (and the one with a cold-path material): depth x lights, the size alternating
CROSS = [(pw, depth, lights, SIZES[(depth + lights) & 1]) for pw in ((16, 32), (16, 32, 0.2)) for depth in (2, 3) for lights in (1, 2)]
# every other set of the plan table once per depth, lights and size alternating
REST = [(pw, 2 + (i & 1), 1 + ((i >> 1) & 1), SIZES[((i >> 1) ^ i) & 1]) for i, (pw, _) in enumerate(p for p in PLANS if p[0] not in ((16, 32), (16, 32, 0.2)))]
REST += [(pw, 3 - (i & 1), 2 - ((i >> 1) & 1), SIZES[i & 1]) for i, (pw, _) in enumerate(p for p in PLANS if p[0] not in ((16, 32), (16, 32, 0.2)))]


@pytest.mark.parametrize("powers, depth, lights, size", CROSS + REST,
                         ids=["%s-d%d-l%d-%dx%d" % ("_".join("%g" % p for p in pw), d, l, s[0], s[1]) for pw, d, l, s in CROSS + REST])
def test_frames_with_32_byte_records(gpu, oracle, monkeypatch, folder, powers, depth, lights, size):
    mask = dict(PLANS)[powers]
    check(gpu, oracle, monkeypatch, scene_file(folder, powers, lights), size[0], size[1], dict(gillum=4, depth=depth, shadow=True, seed=61), lights, mask)


@pytest.mark.parametrize("powers, lights", [((16, 32), 2), ((16, 32, 0.2), 1), ((48, 16), 1), ((8, 16), 2)],
                         ids=["16_32-l2", "16_32_0.2-l1", "48_16-l1", "8_16-l2"])
def test_frames_with_16_byte_records(gpu, oracle, monkeypatch, folder, powers, lights):
    w, h, kw = 16, 36, dict(gillum=97, depth=3, shadow=True, seed=62)
    mb = narrow_budget(w, h, kw["gillum"], kw["depth"], False)
    assert mb is not None and plan(w, h, kw["gillum"], kw["depth"], False, budget_mb=mb)["rec_bytes"] == 16
    check(gpu, oracle, monkeypatch, scene_file(folder, powers, lights), w, h, kw, lights, dict(PLANS)[powers], env={"SKR_LEVELS_BUDGET_MB": str(mb)})
