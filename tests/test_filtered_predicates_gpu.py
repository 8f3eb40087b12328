"""The filtered sphere predicates (device_math.h) and the selection code on top of them (shade_common.h, wave_common.h, trace_rays.hip)
at their decision boundaries, on the MI355X (pytest -m gpu).  Inputs: tests/predicate_cases.py, whose reach
tests/test_predicate_cases_cpu.py holds.  Unit level through the debug ops 12..16 of include/skr.h, which call the kernels' own
functions; end to end through Renderer.trace against tests/ray_query_checker.c and Renderer.shade / render against the oracle.
Every comparison is on bits and no record is left out: the exact form (utils.h:87-121) answers every input, NaN and inf included."""
import os

import numpy as np
import pytest

import predicate_cases as pc
from skele_raytracer_amd import binding

pytestmark = pytest.mark.gpu

N_UNIT = 160000  # records of the threshold family; the other families in proportion (predicate_cases.unit_families)
N_PAIR = 40000  # the same for the packed forms, where every record runs with four partners in either slot


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def store_slack(request, key, worst, records):
    """The measured figure goes into the run's records: a property of the test's report (--junitxml) and pytest's cache
    (filtered_predicates/<key>), beside the printed line."""
    request.node.user_properties.append((key, worst))
    cache = getattr(request.config, "cache", None)
    if cache is not None:
        cache.set("filtered_predicates/" + key, {"max_abs_ta_minus_t2_over_E": worst, "records": records})


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_float(got_bits, want):
    """bit for bit, any NaN standing for any NaN"""
    got = got_bits.view(np.float32)
    return (got_bits == bits(want)) | (np.isnan(got) & np.isnan(want))


def exact(o, d, C, r2):
    a, b, c, D = pc.coeffs(o, d, C, r2)
    t = pc.root_t2(a, b, D)
    with np.errstate(all="ignore"):
        q = ((-b).astype(np.float64) - np.sqrt(D.astype(np.float64))) / (np.float32(2) * a).astype(np.float64)
        # where device_math.h lets binary32 decide at all (its `sane` and `normal`): only the slack figure below looks at this
        normal = (a > np.float32(1e-18)) & (a < np.float32(1e18)) & (D > np.float32(1e-30)) & (b < np.float32(-1e-15))
    return dict(a=a, b=b, D=D, t=t, q=q, acc=pc.accept(t), cand=(D >= 0) & (b < 0), normal=normal)


def check_bracket(name, ex, acc, lo, hi, b, D):
    """One bracket form against the exact one; returns max |ta - t2| / E over the brackets it left unresolved."""
    n = len(ex["t"])
    assert set(np.unique(acc).tolist()) <= {0, 1}, name + ": the accept word is neither 0 nor 1"
    acc = acc.astype(bool)
    bad = np.nonzero(acc != ex["acc"])[0]
    assert len(bad) == 0, "%s: accept differs from the exact form on %d of %d records, first %d (t2 = %r)" % (name, len(bad), n, bad[0], ex["t"][bad[0]])
    assert not acc[~ex["cand"]].any(), name + ": a non-candidate accepted"
    assert same_float(b, ex["b"]).all() and same_float(D, ex["D"]).all(), name + ": b or D are not the spec's"
    lo, hi, t = lo.view(np.float32), hi.view(np.float32), ex["t"]
    inside = (lo <= t) & (t <= hi)
    assert inside[acc].all(), "%s: the bracket of an accepted sphere does not hold t2 on %d records" % (name, (~inside[acc]).sum())
    resolved = acc & (lo == hi)
    assert (bits(lo)[resolved] == bits(t)[resolved]).all(), name + ": lo == hi but not t2"
    # a bracket that decided in binary32, accepted (lo < hi) or certainly rejected (normal, hi < 1): ta and E back from its ends
    with np.errstate(all="ignore"):
        open_ = ex["cand"] & np.isfinite(lo) & np.isfinite(hi) & (lo < hi) & (acc | (ex["normal"] & (hi < 1)))
        ta, E = (lo.astype(np.float64) + hi) / 2, (hi.astype(np.float64) - lo) / 2
        ratio = np.abs(ta - ex["q"]) / E
    return float(ratio[open_].max()) if open_.any() else 0.0, int(open_.sum())


def test_scalar_and_from_ec_brackets(gpu, request):
    """Op 12: sphere_bracket and bracket_from_ec (on the row skr_camec_kernel forms) against the exact form, every family and scale."""
    worst, records = 0.0, 0
    for name, fam in pc.unit_families(N_UNIT).items():
        r2 = pc.r2_of(fam)
        out = binding.debug_eval(12, np.concatenate([bits(fam["o"]), bits(fam["d"]), bits(fam["C"]), bits(r2)[:, None]], axis=1), 10)
        ex = exact(fam["o"], fam["d"], fam["C"], r2)
        for form, k in (("sphere_bracket", 0), ("bracket_from_ec", 5)):
            w, n_open = check_bracket("%s %s" % (name, form), ex, out[:, k], out[:, k + 1], out[:, k + 2], out[:, k + 3], out[:, k + 4])
            worst = max(worst, w)
        assert (out[:, 0] == out[:, 5]).all() and same_float(out[:, 1:5], out[:, 6:10].view(np.float32)).all(), name + ": the two forms differ"
        records += len(ex["t"])
        print("%-10s records %6d, accepted %5.1f %%, decided in binary32 %5.1f %%, max |ta - t2| / E %.4f"
              % (name, len(ex["t"]), 100 * ex["acc"].mean(), 100 * n_open / len(ex["t"]), w))
    print("device bracket: %d records, none skipped, max |ta - t2| / E = %.4f (slack %.1fx)" % (records, worst, 1 / worst))
    store_slack(request, "device_bracket_slack", worst, records)
    assert worst <= 1.0


def paired_inputs(fam, first):
    """[(partner name, slot of the record's own ray, input records)] for ops 13 and 14: the record's ray in either slot, each
    partner in the other."""
    r2 = pc.r2_of(fam)
    for pname, dp in pc.partners(fam).items():
        for slot in (0, 1):
            d0, d1 = (fam["d"], dp) if slot == 0 else (dp, fam["d"])
            yield pname, slot, d0, d1, np.concatenate([bits(first), bits(d0), bits(d1), bits(fam["C"]), bits(r2)[:, None]], axis=1)


def test_pair_brackets(gpu, request):
    """Op 13: the packed test of closest_pair_deferred.  The same b, D, candidate and accept flags as the scalar form in slot 0 and
    in slot 1, whatever ray sits in the other slot; each bracket holds t2."""
    worst, records = 0.0, 0
    for name, fam in pc.unit_families(N_PAIR).items():
        r2 = pc.r2_of(fam)
        for pname, slot, d0, d1, inp in paired_inputs(fam, fam["o"]):
            out = binding.debug_eval(13, inp, 12)
            for k, d in ((0, d0), (1, d1)):
                ex = exact(fam["o"], d, fam["C"], r2)
                w = out[:, 6 * k: 6 * k + 6]
                what = "%s, own ray in slot %d, partner %s, slot %d" % (name, slot, pname, k)
                assert np.array_equal(w[:, 0].astype(bool), ex["cand"]), what + ": candidate flag"
                ww, _ = check_bracket(what, ex, w[:, 1], w[:, 2], w[:, 3], w[:, 4], w[:, 5])
                worst = max(worst, ww)
                records += len(d)
    print("device pair bracket: %d records, none skipped, max |ta - t2| / E = %.4f" % (records, worst))
    store_slack(request, "device_pair_bracket_slack", worst, records)
    assert worst <= 1.0


def test_pair_any_hit(gpu):
    """Op 14: the any-hit test of occluded_pair (2^-18 margins, no sqrt) == accept(exact t2) per slot, from P + 1e-6."""
    records = 0
    for name, fam in pc.unit_families(N_PAIR, shadow=True).items():
        r2 = pc.r2_of(fam)
        o = pc.shadow_origin(fam["P"])
        for pname, slot, d0, d1, inp in paired_inputs(fam, fam["P"]):
            out = binding.debug_eval(14, inp, 4)
            for k, d in ((0, d0), (1, d1)):
                ex = exact(o, d, fam["C"], r2)
                what = "%s, own ray in slot %d, partner %s, slot %d" % (name, slot, pname, k)
                assert np.array_equal(out[:, 2 * k].astype(bool), ex["cand"]), what + ": candidate flag"
                bad = np.nonzero(out[:, 2 * k + 1].astype(bool) != ex["acc"])[0]
                assert len(bad) == 0, "%s: occluded differs from the exact form on %d of %d records, first %d (t2 = %r)" % (
                    what, len(bad), len(d), bad[0], ex["t"][bad[0]])
                records += len(d)
    print("device pair any-hit: %d records, none skipped" % records)


TABLE_ROWS, EC_PAD = 80, 8  # include/skr.h ops 15, 16


def selection_eval(rows, o, d0, d1):
    """Ops 15 and 16 on one scene: the ec tables, then the selection record [n, 22]."""
    ns, n = len(rows), len(o)
    table = np.zeros((TABLE_ROWS, 4), np.float32)
    table[:ns, :3] = rows[:, :3]
    with np.errstate(all="ignore"):
        table[:ns, 3] = rows[:, 3] * rows[:, 3]
    head = np.concatenate([np.array([ns, 0, 0, 0], np.uint32), bits(table).ravel()])
    recs = np.concatenate([bits(o), bits(d0), bits(d1)], axis=1).ravel()
    ec = binding.debug_eval(15, np.concatenate([head, recs]), (ns + EC_PAD) * 4, n=n)
    with np.errstate(all="ignore"):
        e = (o[:, None, :] - table[None, :ns, :3]).astype(np.float32)
        want = np.concatenate([e, (pc.dot(e, e) - table[None, :ns, 3])[..., None]], axis=2).astype(np.float32)
    got = ec.reshape(n, ns + EC_PAD, 4)
    assert same_float(got[:, :ns], want).all(), "ec rows are not utils.h:115-118"
    assert not got[:, ns:].any()
    pad = np.zeros((-9 * n) % 4, np.uint32)
    return binding.debug_eval(16, np.concatenate([head, recs, pad, ec.ravel()]), 22, n=n), table


def check_selection(what, rows, o, d0, d1):
    out, table = selection_eval(rows, o, d0, d1)
    ns = len(rows)
    want = [pc.brute_force(rows, o, d) for d in (d0, d1)]
    forms = ("closest_sphere", "closest_sphere", "closest_sphere_from", "closest_sphere_from", "closest_pair_deferred", "closest_pair_deferred",
             "closest_sphere_exact", "closest_sphere_exact")
    for k, form in enumerate(forms):
        idx, tmin, _ = want[k & 1]
        gi, gt = out[:, 2 * k].view(np.int32), out[:, 2 * k + 1]
        bad = np.nonzero((gi != idx) | (gt != bits(tmin)))[0]
        assert len(bad) == 0, "%s: %s slot %d differs on %d of %d rays; first %d: got (%d, %r) want (%d, %r)" % (
            what, form, k & 1, len(bad), len(o), bad[0], gi[bad[0]], gt.view(np.float32)[bad[0]], idx[bad[0]], tmin[bad[0]])
    # the shadow rays start at o + 1e-6 (utils.h:45)
    so = pc.shadow_origin(o)
    cnt = [pc.shadow_tests(pc.brute_force(rows, so, d)[2]) for d in (d0, d1)]
    tests = cnt[0][0] + cnt[1][0]
    for k, form in ((16, "occluded_pair<false>"), (19, "occluded_pair<true>")):
        for s in (0, 1):
            assert np.array_equal(out[:, k + s].astype(bool), cnt[s][1]), "%s: %s occ%d" % (what, form, s)
        assert np.array_equal(out[:, k + 2].astype(np.int64), tests), "%s: %s counts other sphere tests than the reference's loop runs" % (what, form)
    return len(o)


@pytest.mark.parametrize("ns", pc.TABLE_SIZES)
def test_selection(gpu, ns):
    """Ops 15, 16: index and t of closest_sphere, closest_sphere_from and both slots of closest_pair_deferred<false> ==
    closest_sphere_exact on the device == a brute-force loop on the CPU (first index wins ties); both occluded_pair forms == any
    sphere accepted, counting the tests the reference's loop runs.  Near ties, exact duplicates, ties at the threshold; scaled too."""
    rays = 0
    for i, (rows, o, d0, d1) in enumerate(pc.selection_scenes(ns, 24)):
        rays += check_selection("ns=%d scene %d" % (ns, i), rows, o, d0, d1)
        if i % 4 == 1:  # the two slots on either side of `sane`: the packed loop must give each slot its own flag
            far = np.float32(2.0 ** (40 if i % 8 == 1 else -40))
            with np.errstate(all="ignore"):
                rays += check_selection("ns=%d scene %d, slot 1 x 2^+-40" % (ns, i), rows, o, d0, d0 * far)
                rays += check_selection("ns=%d scene %d, slot 0 x 2^+-40" % (ns, i), rows, o, d1 * far, d1)
        if i % 4 == 0:
            m = (-31, -30, -20, 20, 30, 31)[(i // 4) % 6]
            s = np.float32(2.0 ** m)
            with np.errstate(all="ignore"):
                rays += check_selection("ns=%d scene %d x 2^%d" % (ns, i, m), rows * s, o * s, d0 * s, d1 * s)
    # plain rays and non-finite ones over one more table
    rng = np.random.default_rng(100 + ns)
    rows = np.concatenate([rng.uniform(-8, 8, (ns, 3)), 10.0 ** rng.uniform(-1, 0.5, (ns, 1))], axis=1).astype(np.float32)
    n = 4096 + 37
    o = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
    d0 = ((rows[rng.integers(0, ns, n), :3] + rng.normal(scale=0.5, size=(n, 3)) - o) * rng.uniform(0.05, 1.5, (n, 1))).astype(np.float32)
    d1 = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
    weird = rng.random(n) < 0.05
    d1[weird, rng.integers(0, 3, weird.sum())] = rng.choice(np.float32([np.nan, np.inf, 0.0, 1e-41, 3e19]), weird.sum())
    d0[rng.random(n) < 0.01] = 0
    o[rng.random(n) < 0.01, 0] = np.nan
    rays += check_selection("ns=%d plain" % ns, rows, o, d0, d1)
    print("selection ns=%d: %d ray pairs, none skipped" % (ns, rays))


# ------------------------------------------------------------------ end to end: the ray queries ----
@pytest.fixture(scope="module")
def ray_checker(tmp_path_factory):
    from ray_query_check import build
    return build(str(tmp_path_factory.mktemp("raycheck_predicates")))


def spheres14(rows):
    s = np.zeros((len(rows), 14), np.float32)
    s[:, :4] = rows
    s[:, 4:13] = 0.5
    s[:, 13] = 8
    return s


def check_trace(gpu, checker, what, rows, o, d):
    """Closest hit and any-hit of Renderer.trace on the rays (o, d) over the spheres `rows`, tmax = inf and tmax at each ray's exact t
    and one ulp either side of it, bit for bit against tests/ray_query_checker.c."""
    import skele_raytracer_amd as skr
    from ray_query_check import pack_rays
    from test_ray_query_gpu import arrays_scene, assert_bitwise, gpu_trace
    s = spheres14(rows)
    t = np.zeros((0, 9), np.float32)
    r = skr.Renderer(arrays_scene(s, t), 0)
    base = pack_rays(o, d)
    th = checker.trace(s, t, base)[0][:, 0]
    with np.errstate(all="ignore"):
        rays = np.concatenate([base] + [pack_rays(o, d, tm) for tm in (th, np.nextafter(th, np.float32(np.inf)), np.nextafter(th, np.float32(0)))])
    want, occ_want = checker.trace(s, t, rays)
    assert_bitwise(gpu_trace(r, rays), want, what + ": closest hit")
    assert np.array_equal(gpu_trace(r, rays, any_hit=True), occ_want), what + ": any-hit"
    n = len(base)
    hit = np.isfinite(th)
    kind = want[:, 1].view(np.int32)
    assert not kind[n: 2 * n][hit].any() and kind[2 * n: 3 * n][hit].all(), what + ": the checker itself, tmax at t"
    return len(rays)


@pytest.mark.parametrize("ns", pc.TABLE_SIZES)
def test_trace_on_tie_and_duplicate_scenes(gpu, ray_checker, ns):
    """Renderer.trace over the selection scenes (near ties, duplicates, ties at the threshold), some scaled across the ends of `sane`."""
    n = 0
    for i, (rows, o, d0, d1) in enumerate(pc.selection_scenes(ns, 6, seed=33)):
        m = (0, 0, -30, 30, -31, 20)[i]
        s = np.float32(2.0 ** m)
        n += check_trace(gpu, ray_checker, "ns=%d scene %d x 2^%d" % (ns, i, m), rows * s, np.concatenate([o, o]) * s, np.concatenate([d0, d1]) * s)
    print("trace ns=%d: %d rays" % (ns, n))


@pytest.mark.parametrize("m", (0, -31, -30, -20, 20, 29, 30, 31))
def test_trace_on_threshold_scenes(gpu, ray_checker, m):
    """Renderer.trace with a sphere of the table at t ~ 1 on every ray (threshold family over the table's 32 spheres), tangent and
    surface rays among them; the whole scene scaled by 2^m."""
    n = 0
    for k in range(4):
        rng = np.random.default_rng(50 + k)
        rows = np.concatenate([rng.uniform(-8, 8, (32, 3)), 10.0 ** rng.uniform(-1.5, 1.0, (32, 1))], axis=1).astype(np.float32)
        fam = pc.concat(pc.threshold(768, seed=41 + k, rows=rows), pc.tangent(128, seed=42 + k), pc.surface(128, seed=43 + k))
        f = pc.scaled(fam, m)
        n += check_trace(gpu, ray_checker, "threshold x 2^%d, table %d" % (m, k), rows * np.float32(2.0 ** m), f["o"], f["d"])
    print("trace threshold x 2^%d: %d rays" % (m, n))


# --------------------------------------------------- end to end: frames and shading queries ----
BASE_SCN, W, H = "spheres2.scn", 64, 36
SWITCHES = ("SKR_FLAT", "SKR_PIPELINE", "SKR_SHADOW_MASK", "SKR_GI_MASK")


class PatchedOracleScene:
    """The oracle's scene of a .scn file with further spheres appended: centre and radius given, the material that of sphere
    `like`.  Binary32 values go in as they are (no text round trip)."""

    def __init__(self, path, extra, like):
        import ctypes as C
        from oracle import pyoracle
        self.base = pyoracle.OracleScene(path)
        self.s = pyoracle.Scene.from_buffer_copy(self.base.s)
        n0 = self.base.s.n_spheres
        self.rows = (pyoracle.Sphere * (n0 + len(extra)))()
        for i in range(n0):
            C.memmove(C.byref(self.rows[i]), C.byref(self.base.s.spheres[i]), C.sizeof(pyoracle.Sphere))
        for k, (row, j) in enumerate(zip(extra, like)):
            C.memmove(C.byref(self.rows[n0 + k]), C.byref(self.base.s.spheres[int(j)]), C.sizeof(pyoracle.Sphere))
            sp = self.rows[n0 + k]
            sp.center.x, sp.center.y, sp.center.z, sp.radius = (float(v) for v in row)
        self.s.spheres = C.cast(self.rows, C.POINTER(pyoracle.Sphere))
        self.s.n_spheres = n0 + len(extra)


def product_scene(extra, like):
    import skele_raytracer_amd as skr
    from conftest import scene_path
    sc = skr.parse_scene(scene_path(BASE_SCN))
    s, t, l = sc.arrays()
    add = s[np.asarray(like, np.int64)].copy()
    add[:, :4] = extra
    info = sc.info
    return skr.Scene.from_arrays(np.concatenate([s, add]), t, l, list(info.camera[:9]), tuple(info.background), tuple(info.ambient)), np.concatenate([s, add]), l


def check_frames(gpu, monkeypatch, oracle, what, extra, like, modes, envs):
    """Renderer.render and Renderer.shade of the frame's camera rays == the oracle: float image and counters (sphere tests among them) bit for bit."""
    import skele_raytracer_amd as skr
    sc, _, _ = product_scene(extra, like)
    osc = PatchedOracleScene(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes", BASE_SCN), extra, like)
    seen = set()
    want = [oracle.render(osc, W, H, rng=oracle.RNG_COUNTER, math=oracle.MATH_SHARED, want_float=True, **kw) for kw in modes]
    keys = gpu.arange(W * H, dtype=gpu.int32, device="cuda")
    for env in envs:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = skr.Renderer(sc, 0)  # (the switches are read once per renderer)
        for kw, (o_rgb, o_f, st) in zip(modes, want):
            opt = skr.Options(W, H, **kw)
            r.work(reset=True)
            rgb, rgbf = r.render(opt, want_float=True)
            gpu.cuda.synchronize()
            got = r.work()
            tag = "%s %s %s (%s)" % (what, kw, env, r.kernel_variant())
            seen.add(r.kernel_variant())
            assert np.array_equal(rgbf.cpu().numpy().view(np.uint32), o_f.view(np.uint32)), tag + ": float image differs from the oracle"
            assert np.array_equal(rgb.cpu().numpy(), o_rgb), tag
            assert (got["radiance_rays"], got["sphere_hits"], got["shadow_rays"], got["sphere_tests"]) == tuple(int(v) for v in st[:4]), tag
            out = r.shade(r.camera_rays(opt).view(-1, 8), opt, 0, keys=keys)
            gpu.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(H, W, 3), o_f.view(np.uint32)), tag + ": shade() differs from the oracle"
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    print("%s: kernels %s" % (what, sorted(seen)))
    return seen


def cpu_camera_rays():
    from conftest import scene_path
    from shade_query_check import camera_rays
    return camera_rays(scene_path(BASE_SCN), W, H)


def test_frames_with_spheres_at_the_near_plane(gpu, monkeypatch, oracle):
    """(a) Spheres whose near surface lies at o + d (1 + k 2^-24) of a pixel's primary ray, some as near-tie pairs and duplicates: the
    primary kernels' closest_sphere_from meets the band; depth 1 and gillum 2."""
    rng = np.random.default_rng(71)
    rays = cpu_camera_rays()
    pix = np.array([y * W + x for y in range(1, H, 3) for x in range(1, W, 3)])
    o, d = rays[pix, 0:3].astype(np.float64), rays[pix, 4:7].astype(np.float64)
    n = len(pix)
    k = pc._ulps(rng, n, 14, 0.1)
    S = o + d * (1 + k * 2.0 ** -24)[:, None]
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    rad = rng.uniform(0.001, 0.004, n)
    extra = [np.concatenate([S + dn * rad[:, None], rad[:, None]], axis=1).astype(np.float32)]
    tie = np.arange(n) % 3 == 0   # a second sphere through the same point, its radius then moved by ulps
    r2 = rng.uniform(0.001, 0.004, n).astype(np.float32)
    C2 = (S + dn * r2[:, None]).astype(np.float32)
    r2 = (r2.view(np.int32) + np.rint(pc._ulps(rng, n, 8, 0.15)).astype(np.int32)).view(np.float32)
    extra.append(np.concatenate([C2, r2[:, None]], axis=1)[tie])
    extra.append(extra[0][np.arange(n) % 3 == 1])  # exact duplicates at later indices
    extra = np.concatenate(extra).astype(np.float32)
    like = rng.integers(1, 11, len(extra))
    # the inputs reach the band: the exact t2 of the pixel's ray on its own sphere, from the oracle's own primary directions
    t = pc.exact_t2(rays[pix, 0:3], rays[pix, 4:7], extra[:n, :3], extra[:n, 3] * extra[:n, 3])
    acc = pc.accept(t)
    print("near plane: %d pixels, %d spheres added, own sphere accepted %.0f %%, |t2 - 1| < 2^-10 %.0f %%, < 2^-20 %.0f %%"
          % (n, len(extra), 100 * acc.mean(), 100 * (np.abs(t.astype(np.float64) - 1) < 2.0 ** -10).mean(), 100 * (np.abs(t.astype(np.float64) - 1) < 2.0 ** -20).mean()))
    assert 0.2 <= acc.mean() <= 0.8 and (np.abs(t.astype(np.float64) - 1) < 2.0 ** -10).mean() >= 0.9
    check_frames(gpu, monkeypatch, oracle, "near plane", extra, like, [dict(depth=1), dict(gillum=2, seed=5)], [{}, {"SKR_PIPELINE": "generic"}])


def occluder_pixels(ray_checker):
    """The frame's pixels with a sphere under them (the checker's trace of the base scene), every third of every second row."""
    from conftest import scene_path
    import skele_raytracer_amd as skr
    rays = cpu_camera_rays()
    s, tr, lights = skr.parse_scene(scene_path(BASE_SCN)).arrays()
    hits, _ = ray_checker.trace(s, tr, rays)
    pix = np.array([y * W + x for y in range(1, H, 2) for x in range(2, W, 3)])
    return pix[hits[pix, 1].view(np.int32) == 1], (rays, s, tr, lights, hits)


def occluder_scene(base, pix, seed):
    """(b) For each pixel of `pix` a small sphere whose near surface along L = normalize(Lp - P) lies at P + 1e-6 + L (1 + k 2^-24):
    t2 ~ 1 on the pixel's shadow ray towards that light.  Returns (extra rows, like, per pixel: primary hit unchanged, t2 within 2^-10
    of 1, occluded), all from the checker's primitives."""
    ray_checker, (rays, s, tr, lights, hits) = base
    rng = np.random.default_rng(seed)
    n = len(pix)
    f32 = np.float32
    o, d, t = rays[pix, 0:3], rays[pix, 4:7], hits[pix, 0]
    P = (o + d * t[:, None]).astype(f32)              # raytrace.h: the hit point, binary32
    which = np.arange(n) % len(lights)
    Lp = lights[which, 0:3]
    v = (Lp - P).astype(f32)
    inv = f32(1) / np.sqrt(pc.dot(v, v))              # the checker's normalize3
    so, L = pc.shadow_origin(P), (v * inv[:, None]).astype(f32)
    k = pc._ulps(rng, n, 14, 0.1)
    S = so.astype(np.float64) + L.astype(np.float64) * (1 + k * 2.0 ** -24)[:, None]
    rad = rng.uniform(0.002, 0.01, n)
    extra = np.concatenate([S + L * rad[:, None], rad[:, None]], axis=1).astype(f32)
    like = rng.integers(1, 11, n)
    s2 = np.concatenate([s, np.concatenate([extra, s[like, 4:]], axis=1)])
    hits2, _ = ray_checker.trace(s2, tr, rays)
    same = (hits2[pix, :3].view(np.uint32) == hits[pix, :3].view(np.uint32)).all(1)
    t2 = pc.exact_t2(so, L, extra[:, :3], extra[:, 3] * extra[:, 3])
    return extra, like, same, np.abs(t2.astype(np.float64) - 1) < 2.0 ** -10, pc.accept(t2)


def occluder_shares(same, band, acc):
    return dict(pixels=len(same), unchanged=same.mean(), in_band=band[same].mean(), occluded=acc[same & band].mean(), clear=(~acc)[same & band].mean())


def assert_occluder_conditions(what, sh, least):
    """The two conditions on scene (b), before the GPU is asked anything."""
    print(what + ": " + ", ".join("%s %.3g" % kv for kv in sh.items()))
    assert sh["pixels"] >= least and sh["unchanged"] >= 0.5 and sh["in_band"] >= 0.5 and sh["occluded"] >= 0.2 and sh["clear"] >= 0.2, sh


OCCLUDER_MODES = [dict(depth=1, shadow=True), dict(gillum=2, shadow=True, seed=3), dict(gillum=4, shadow=True, seed=9)]


def test_frames_with_occluders_at_unit_distance(gpu, monkeypatch, oracle, ray_checker):
    """(b) One occluder for each of a few hundred pixels.  A scene of this size carries no shadow or GI masks (more than 32 spheres), so
    the walks over every sphere meet the occluders here; the masked walks meet them in the next test."""
    pix, base = occluder_pixels(ray_checker)
    extra, like, same, band, acc = occluder_scene((ray_checker, base), pix, 72)
    assert_occluder_conditions("unit-distance occluders", occluder_shares(same, band, acc), 36)
    envs = [{}, {"SKR_FLAT": "0"}, {"SKR_PIPELINE": "generic"}]
    seen = check_frames(gpu, monkeypatch, oracle, "unit-distance occluders", extra, like, OCCLUDER_MODES, envs)
    # the direct kernel, both schedules of the node pipeline and the general level pipeline all met them
    assert {"node_levels_v5_flat", "node_levels_v5", "level_pipeline_g1"} <= seen and len(seen) >= 4, seen


def test_frames_with_occluders_under_shadow_and_gi_masks(gpu, monkeypatch, oracle, ray_checker):
    """(b) in scenes small enough to carry shadow and GI masks (at most 32 spheres: shadow_cells.h), a dozen and a half occluders each,
    rendered with the masks and with SKR_SHADOW_MASK=0 SKR_GI_MASK=0, on both schedules of the node pipeline and the general level
    pipeline: the masked walk of occluded_pair and the walk over every sphere must both give the oracle's frame and counts."""
    pix, base = occluder_pixels(ray_checker)
    n0 = len(base[1])
    per = 32 - n0
    assert per >= 12, "the base scene leaves no room for occluders under the masks' sphere limit"
    parts, scenes = [], []
    for k in range(3):
        sub = pix[k::len(pix) // per + 1][:per]   # spread over the frame, other pixels in every scene
        extra, like, same, band, acc = occluder_scene((ray_checker, base), sub, 80 + k)
        parts.append((same, band, acc))
        scenes.append((extra, like))
    sh = occluder_shares(*(np.concatenate([p[j] for p in parts]) for j in range(3)))
    assert_occluder_conditions("unit-distance occluders under masks", sh, 36)
    envs = [{}, {"SKR_SHADOW_MASK": "0", "SKR_GI_MASK": "0"}, {"SKR_FLAT": "0"}, {"SKR_PIPELINE": "generic"}]
    seen = set()
    for k, (extra, like) in enumerate(scenes):
        sc = product_scene(extra, like)[0]
        assert sc.info.n_spheres <= 32
        assert sc.shadow_masks()[0].shape[0] > 0 and len(sc.gi_masks()[0]) > 0, "scene %d carries no masks: masks on and off would be the same run" % k
        seen |= check_frames(gpu, monkeypatch, oracle, "masked occluders, scene %d" % k, extra, like, OCCLUDER_MODES, envs)
    assert {"node_levels_v5_flat", "node_levels_v5", "level_pipeline_g1"} <= seen and len(seen) >= 4, seen
