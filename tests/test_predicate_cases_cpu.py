"""The inputs of the filtered-predicate tests (tests/predicate_cases.py) reach the boundaries they are built for: conditions on the
generator, held against the exact form alone (sko_smallest_root and the accept rule), so that a later edit of the generator cannot
hollow out tests/test_filtered_predicates_gpu.py.  No GPU.

It also carries a numpy binary32 emulation of the bracket of device_math.h (correctly rounded sqrt and 1/x in place of v_sqrt_f32 /
v_rcp_f32) and holds it to the exact form on every family: a certain verdict is the exact one, lo <= t2 <= hi, and |ta - t2| / E is
printed (DESIGN.md "Filtered predicates" records it)."""
import numpy as np

import predicate_cases as pc

N = 200000


def _exact(fam):
    a, b, c, D = pc.coeffs(fam["o"], fam["d"], fam["C"], pc.r2_of(fam))
    return a, b, c, D, pc.root_t2(a, b, D)


def test_the_numpy_exact_form_is_the_oracles(oracle):
    """exact_t2 (vectorised, what the GPU tests compare with) == sko_smallest_root, bit for bit, on every family and scale."""
    n = 0
    for name, fam in pc.unit_families(16000).items():
        a, b, c, D, t = _exact(fam)
        want = pc.oracle_t2(a, b, c)
        assert np.array_equal(t.view(np.uint32), want.view(np.uint32)), name
        n += len(t)
    print("records held to sko_smallest_root: %d" % n)


def test_threshold_family_straddles_the_band(oracle):
    fam = pc.threshold(N)
    a, b, c, D, t = _exact(fam)
    assert np.array_equal(t[:20000].view(np.uint32), pc.oracle_t2(a[:20000], b[:20000], c[:20000]).view(np.uint32))
    cand, ca, cr, lo, hi, ta, E = pc.emulated_bracket(a, b, D)
    acc = pc.accept(t)
    nc = cand.sum()
    shares = dict(candidates=cand.mean(), accepted=acc[cand].mean(), rejected=(~acc)[cand].mean(),
                  undecided=(cand & ~ca & ~cr).sum() / nc, certain_accept=ca.sum() / nc, certain_reject=cr.sum() / nc)
    print("threshold family: " + ", ".join("%s %.1f %%" % (k, 100 * v) for k, v in shares.items()))
    assert shares["candidates"] >= 0.9
    assert shares["accepted"] >= 0.30 and shares["rejected"] >= 0.30
    assert shares["undecided"] >= 0.15
    assert shares["certain_accept"] >= 0.20 and shares["certain_reject"] >= 0.20
    # the any-hit form's 2^-18 margins: records on both sides of each
    with np.errstate(all="ignore"):
        rel = np.abs(t.astype(np.float64) - 1)
    for lo_, hi_ in ((0, 2.0 ** -20), (2.0 ** -20, 2.0 ** -18), (2.0 ** -18, 2.0 ** -16), (2.0 ** -16, 2.0 ** -10)):
        for side in (acc, ~acc):
            share = (cand & side & (rel >= lo_) & (rel < hi_)).sum() / nc
            assert share >= 0.02, (lo_, hi_, share)


def test_near_tie_family_ties(oracle):
    tp = pc.near_tie_pairs(N)
    t1 = pc.exact_t2(tp["o"], tp["d"], tp["C1"], tp["r1"] * tp["r1"])
    t2 = pc.exact_t2(tp["o"], tp["d"], tp["C2"], tp["r2"] * tp["r2"])
    a, b, c, D = pc.coeffs(tp["o"][:20000], tp["d"][:20000], tp["C2"][:20000], (tp["r2"] * tp["r2"])[:20000])
    assert np.array_equal(t2[:20000].view(np.uint32), pc.oracle_t2(a, b, c).view(np.uint32))
    both = pc.accept(t1) & pc.accept(t2)
    ul = np.abs(t1.view(np.int32).astype(np.int64) - t2.view(np.int32).astype(np.int64))[both]
    second = (t2[both] < t1[both]).mean()
    print("near ties: both accepted %.1f %%, exact ties %.1f %%, within 8 ulps %.1f %%, second nearer %.1f %%"
          % (100 * both.mean(), 100 * (ul == 0).mean(), 100 * (ul <= 8).mean(), 100 * second))
    assert both.mean() >= 0.80
    assert (ul == 0).mean() >= 0.01
    assert (ul <= 8).mean() >= 0.25
    assert 0.35 <= second <= 0.65


def test_selection_scenes_hold_ties_duplicates_and_misses():
    """The scenes of the selection op: near ties and exact ties between different indices, in the threshold band too, and rays that
    hit nothing, at every table size."""
    for ns in pc.TABLE_SIZES:
        ties = close = none = thr = n = 0
        for rows, o, d0, d1 in pc.selection_scenes(ns, 12):
            assert rows.shape == (ns, 4)
            for d in (d0, d1):
                idx, tmin, t = pc.brute_force(rows, o, d)
                ts = np.sort(t, axis=1)
                n += len(o)
                none += (idx < 0).sum()
                if ns > 1:
                    hit2 = ts[:, 1] != pc.INF
                    ul = np.abs(ts[:, 0].view(np.int32).astype(np.int64) - ts[:, 1].view(np.int32).astype(np.int64))
                    ties += (hit2 & (ul == 0)).sum()
                    close += (hit2 & (ul <= 8)).sum()
                    thr += (hit2 & (ul <= 8) & (np.abs(ts[:, 0].astype(np.float64) - 1) < 2.0 ** -16)).sum()
        print("selection scenes ns=%d: rays %d, nearest two equal %d, within 8 ulps %d (of them t within 2^-16 of 1: %d), no hit %d"
              % (ns, n, ties, close, thr, none))
        if ns > 1:
            assert ties >= 0.02 * n and close >= 0.10 * n and thr >= 0.01 * n
        assert none >= 1 or ns >= 33


def test_scale_sweep_is_invariant_where_nothing_over_or_underflows(oracle):
    fam = pc.threshold(N)
    _, _, _, _, t0 = _exact(fam)
    q0 = pc.qualifies(fam["o"], fam["d"], fam["C"], fam["r"])
    for m, f in pc.scale_sweep(fam):
        a, b, c, D, t = _exact(f)
        q = q0 & pc.qualifies(f["o"], f["d"], f["C"], f["r"])
        same = t.view(np.uint32) == t0.view(np.uint32)
        print("scale 2^%+d: qualifying %.1f %%, t2 bit-identical among them %.2f %%, overall %.1f %%"
              % (m, 100 * q.mean(), 100 * same[q].mean() if q.any() else float("nan"), 100 * same.mean()))
        assert same[q].all(), m
        if abs(m) <= 20:
            assert q.all(), m
        if m == -31:
            assert q.mean() >= 0.5
        if m == 30:
            assert q.mean() >= 0.2
        sub = slice(0, 4000)
        assert np.array_equal(t[sub].view(np.uint32), pc.oracle_t2(a[sub], b[sub], c[sub]).view(np.uint32)), m


def test_emulated_bracket_holds_the_exact_root(oracle):
    """The bracket formula with correctly rounded binary32 sqrt and 1/x: a certain verdict is the exact one, lo <= t2 <= hi, on
    every family and scale; max |ta - t2| / E printed."""
    worst = 0.0
    for name, fam in pc.unit_families(N // 2).items():
        a, b, c, D, t = _exact(fam)
        cand, ca, cr, lo, hi, ta, E = pc.emulated_bracket(a, b, D)
        acc = pc.accept(t)
        assert acc[ca].all() and not acc[cr].any(), name
        assert not acc[~cand].any(), name  # D < 0, b >= 0, NaN: never accepted
        assert ((lo <= t) & (t <= hi))[ca].all(), name
        with np.errstate(all="ignore"):
            q = ((-b).astype(np.float64) - np.sqrt(D.astype(np.float64))) / (np.float32(2) * a).astype(np.float64)
            ratio = np.abs(ta.astype(np.float64) - q) / E.astype(np.float64)
        dec = ca | cr
        w = float(ratio[dec].max()) if dec.any() else 0.0
        worst = max(worst, w)
        print("%-10s records %6d, decided in binary32 %5.1f %%, max |ta - t2| / E %.4f" % (name, len(t), 100 * dec.mean(), w))
    print("emulated bracket: max |ta - t2| / E = %.4f (slack %.1fx)" % (worst, 1 / worst))
    assert worst <= 1.0
