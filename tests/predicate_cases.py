"""Boundary cases for the filtered sphere predicates (device_math.h) and the selection code on top of them, shared by
tests/test_predicate_cases_cpu.py and tests/test_filtered_predicates_gpu.py.  numpy only, seeded, no GPU.

Every value is formed in binary64 and rounded once to binary32.  A family is a dict of float32 arrays
    o [n, 3] ray origin, d [n, 3] ray direction, C [n, 3] sphere centre, r [n] sphere radius, P [n, 3]
P is the point a shadow ray starts from: the any-hit forms (utils.h:45) add 1e-6 to it, and the family is built around
o = fl32(P + 1e-6), so that the boundary sits where the device evaluates it.  Without `shadow`, P == o.

The arithmetic of utils.h:87-121 is restated here in numpy binary32 (coeffs, exact_t2): IEEE operations in the reference's order, the
binary64 sqrt and divide of the root correctly rounded as the C library's are.  The CPU test holds exact_t2 to sko_smallest_root on
every record, so that the GPU tests may use the vectorised form."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)
SCALES = (-70, -40, -31, -30, -29, -20, -10, 0, 10, 20, 25, 29, 30, 31, 40, 62)
TABLE_SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64)  # the trip sizes of table_rows and their neighbours
SHADOW_EPS = f32(0.000001)


# ---------------------------------------------------------------- the spec in numpy binary32 ----
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def coeffs(o, d, C, r2):
    """a, b, c, D of utils.h:115-118 / :89 (binary32, one operation at a time); r2 = fl32(r * r)."""
    with np.errstate(all="ignore"):
        o, d, C, r2 = (np.asarray(x, f32) for x in (o, d, C, r2))
        e = o - C
        a = dot(d, d)
        b = f32(2) * dot(d, e)
        c = dot(e, e) - r2
        D = b * b - (f32(4) * a) * c
    return a, b, c, D


def root_t2(a, b, D):
    """utils.h:87-110 given D: fl32 of the binary64 near root, +inf where D < 0 or the root is negative or NaN."""
    with np.errstate(all="ignore"):
        q = ((-b).astype(np.float64) - np.sqrt(D.astype(np.float64))) / (f32(2) * a).astype(np.float64)
        t = q.astype(f32)
        t = np.where(t >= 0, t, INF)
        return np.where(D < 0, INF, t).astype(f32)


def exact_t2(o, d, C, r2):
    a, b, _, D = coeffs(o, d, C, r2)
    return root_t2(a, b, D)


def accept(t):
    """utils.h:169-179: 1 < t < inf"""
    return ~((t <= 1) | (t == INF))


def oracle_t2(a, b, c):
    """sko_smallest_root per record (the exact form as the oracle states it)."""
    from oracle import pyoracle
    fn = pyoracle.lib().sko_smallest_root
    a, b, c = (np.asarray(x, f32).ravel().tolist() for x in (a, b, c))
    return np.array([fn(x, y, z) for x, y, z in zip(a, b, c)], np.float64).astype(f32)


def shadow_origin(P):
    return (np.asarray(P, f32) + SHADOW_EPS).astype(f32)


def emulated_bracket(a, b, D):
    """The bracket of device_math.h with correctly rounded binary32 sqrt and 1/x standing in for v_sqrt_f32 / v_rcp_f32:
    cand, certain_accept, certain_reject, lo, hi, ta, E."""
    with np.errstate(all="ignore"):
        two_a = f32(2) * a
        cand = (D >= 0) & (b < 0)
        s = np.sqrt(D)
        num = (-b) - s
        inv = f32(1) / two_a
        ta = num * inv
        E = np.abs(ta) * f32(2.0 ** -22) + (s + np.abs(num)) * (inv * f32(2.0 ** -20))
        lo, hi = ta - E, ta + E
        sane = (a > f32(1e-18)) & (a < f32(1e18))
        normal = sane & (D > f32(1e-30)) & (b < f32(-1e-15))
        ca = cand & normal & (lo > 1) & (hi < f32(3.0e38))
        cr = cand & normal & (hi < 1)
    return cand, ca, cr, lo, hi, ta, E


def qualifies(o, d, C, r):
    """Every intermediate of the spec normal (or exactly 0) in a binary32 evaluation: no under- or overflow anywhere.  A product
    counts as exactly 0 only where a factor is 0 (a 0 that two non-zero factors give is an underflow)."""
    tiny = f32(np.finfo(f32).tiny)
    with np.errstate(all="ignore"):
        ok = np.ones(len(r), bool)

        def mul(x, y):
            nonlocal ok
            v = x * y
            k = np.isfinite(v) & ((np.abs(v) >= tiny) | (x == 0) | (y == 0))
            ok = ok & (k if k.ndim == 1 else k.all(1))
            return v

        def add(x, y, sign=1):
            nonlocal ok
            v = x + y if sign > 0 else x - y
            k = np.isfinite(v) & ((v == 0) | (np.abs(v) >= tiny))
            ok = ok & (k if k.ndim == 1 else k.all(1))
            return v

        def dot_(x, y):
            p = mul(x, y)
            return add(add(p[:, 0], p[:, 1]), p[:, 2])
        e = add(o, C, -1)
        a = dot_(d, d)
        b = mul(np.full_like(a, 2), dot_(d, e))
        c = add(dot_(e, e), mul(r, r), -1)
        add(mul(b, b), mul(mul(np.full_like(a, 4), a), c), -1)
        mul(np.full_like(a, 2), a)
    return ok


def scaled(fam, m):
    """Every length of the family times 2^m (exact unless it under- or overflows)."""
    s = f32(2.0 ** m)
    with np.errstate(all="ignore"):
        return {k: (v * s).astype(f32) for k, v in fam.items()}


def _family(o, d, C, r, P=None):
    o, d, C, r = (np.ascontiguousarray(x, f32) for x in (o, d, C, r))
    return dict(o=o, d=d, C=C, r=r, P=o.copy() if P is None else np.ascontiguousarray(P, f32))


def concat(*fams):
    return {k: np.concatenate([f[k] for f in fams]) for k in ("o", "d", "C", "r", "P")}


def take(fam, idx):
    return {k: v[idx] for k, v in fam.items()}


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _perp(u, w):
    """u made perpendicular to the unit vectors w, normalised (binary64)."""
    p = u - w * (u * w).sum(1, keepdims=True)
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def _spheres_and_origins(rng, n, shadow, lo=1.05, hi=20.0, rows=None):
    C = rng.uniform(-8, 8, (n, 3)).astype(f32)
    r = (10.0 ** rng.uniform(-1.5, 1.5, n)).astype(f32)
    if rows is not None:  # the records share the spheres of one table [m, 4] = C, r
        C, r = rows[np.arange(n) % len(rows), :3].astype(f32), rows[np.arange(n) % len(rows), 3].astype(f32)
    P = (C + _unit(rng, n) * (r * rng.uniform(lo, hi, n))[:, None]).astype(f32)
    o = shadow_origin(P) if shadow else P
    return C, r, P, o


def _ulps(rng, n, max_log2, zero_share):
    k = np.rint(np.sign(rng.normal(size=n)) * 2.0 ** rng.uniform(0, max_log2, n))
    k[rng.random(n) < zero_share] = 0
    return k


# ------------------------------------------------------------------------------- the families ----
def threshold(n, seed=5, shadow=False, rows=None):
    """t2 from exactly-1-ish to 1 +- 2^-10: d = (P - o)(1 + k 2^-24) for a point P of the cap that faces o."""
    rng = np.random.default_rng(seed)
    C, r, P, o = _spheres_and_origins(rng, n, shadow, rows=rows)
    oc = o.astype(np.float64) - C
    ocn = oc / np.linalg.norm(oc, axis=1, keepdims=True)
    w = ocn * rng.uniform(0.05, 1, n)[:, None] + _perp(_unit(rng, n), ocn) * rng.uniform(0, 1, n)[:, None]
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    S = C.astype(np.float64) + w * r[:, None].astype(np.float64)
    k = _ulps(rng, n, 14, 0.1)
    d = ((S - o.astype(np.float64)) * (1 + k * 2.0 ** -24)[:, None]).astype(f32)
    return _family(o, d, C, r, P)


def tangent(n, seed=7, shadow=False):
    """d aimed at the silhouette, off it by 0, +-ulps .. 1e-4 r: D negative, zero, tiny, and s ~ 0."""
    rng = np.random.default_rng(seed)
    C, r, P, o = _spheres_and_origins(rng, n, shadow)
    oc = C.astype(np.float64) - o
    L = np.linalg.norm(oc, axis=1)
    w = oc / L[:, None]
    u = _perp(_unit(rng, n), w)
    sin = np.minimum(r / L, 1.0)
    cos = np.sqrt(1 - sin * sin)
    T = o + (L * cos)[:, None] * (cos[:, None] * w + sin[:, None] * u)
    out = (T - C) / np.linalg.norm(T - C, axis=1, keepdims=True)
    delta = np.sign(rng.normal(size=n)) * r * 10.0 ** rng.uniform(-8, -4, n)
    delta[rng.random(n) < 0.2] = 0
    d = ((T + out * delta[:, None] - o) * rng.uniform(0.3, 3, n)[:, None]).astype(f32)
    return _family(o, d, C, r, P)


def surface(n, seed=9, shadow=False):
    """Origin on, in and just off the surface; b within ulps of 0; origin at the centre; r = 0."""
    rng = np.random.default_rng(seed)
    C = rng.uniform(-8, 8, (n, 3)).astype(f32)
    r = (10.0 ** rng.uniform(-1.5, 1.5, n)).astype(f32)
    nrm = _unit(rng, n)
    kind = rng.integers(0, 6, n)
    off = np.where(kind == 0, 0.0, np.sign(rng.normal(size=n)) * 10.0 ** rng.uniform(-8, -2, n))  # kind 0: on the surface
    off[kind == 1] = -np.abs(off[kind == 1])   # inside
    off[kind == 2] = np.abs(off[kind == 2])    # just off
    P = (C + nrm * (r * (1 + off))[:, None]).astype(f32)
    P[kind == 4] = C[kind == 4]                # at the centre
    r = np.where(kind == 5, f32(0), r).astype(f32)
    o = shadow_origin(P) if shadow else P
    # directions: inward, outward, and tangential nudged by ulps (b ~ 0, b >= -1e-15)
    e = o.astype(np.float64) - C
    en = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-300)
    tang = _perp(_unit(rng, n), np.where(np.isfinite(en) & (np.abs(en).sum(1, keepdims=True) > 0), en, [[1.0, 0, 0]]))
    mix = rng.choice([-1.0, 1.0, 0.0, 0.0], n) * rng.uniform(0, 1, n) ** 4
    mix[rng.random(n) < 0.25] *= 1e-7
    dd = tang + en * mix[:, None]
    d = (dd * (10.0 ** rng.uniform(-1, 1.5, n))[:, None]).astype(f32)
    tiny = rng.random(n) < 0.1  # |d| so small that b >= -1e-15
    d[tiny] = (d[tiny] * f32(1e-9)).astype(f32)
    return _family(o, d, C, r, P)


def baseline(n, seed=11, shadow=False):
    """Plain random rays: about half aimed into the sphere, half past it."""
    rng = np.random.default_rng(seed)
    C, r, P, o = _spheres_and_origins(rng, n, shadow, 0.2, 20.0)
    aim = C + _unit(rng, n) * (r * rng.uniform(0, 2.0, n))[:, None]
    d = ((aim - o) * (10.0 ** rng.uniform(-1.5, 1.0, n))[:, None]).astype(f32)
    return _family(o, d, C, r, P)


def nonfinite(n, seed=13, shadow=False):
    """d = 0, denormal d, inf / NaN in any one of o, d, C, r, |d| near 1e19, 1e-19 and near the ends of `sane` (1e9, 1e-9)."""
    rng = np.random.default_rng(seed)
    base = threshold(n, seed + 1, shadow) if n else None
    o, d, C, r, P = (base[k].copy() for k in ("o", "d", "C", "r", "P"))
    kind = np.arange(n) % 12
    comp = rng.integers(0, 3, n)
    bad = np.where(rng.random(n) < 0.5, np.nan, np.where(rng.random(n) < 0.5, np.inf, -np.inf)).astype(f32)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        d[kind == 0] = 0
        d[kind == 1] = (d[kind == 1] / np.linalg.norm(d[kind == 1], axis=1, keepdims=True) * 1e-41).astype(f32)
        for k, arr in ((2, o), (3, d), (4, C)):
            m = kind == k
            arr[rows[m], comp[m]] = bad[m]
        P[kind == 2] = o[kind == 2]
        r[kind == 5] = bad[kind == 5]
        unit = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
        for k, mag in ((6, 1e19), (7, 1e-19), (8, 1e9), (9, 1e-9), (10, 1.8e19), (11, 3.0e-23)):
            m = kind == k
            d[m] = (unit[m] * (mag * rng.uniform(0.5, 2.0, m.sum()))[:, None]).astype(f32)
    return _family(o, d, C, r, P)


def r2_of(fam):
    with np.errstate(all="ignore"):
        return (fam["r"] * fam["r"]).astype(f32)


def partners(fam, seed=17):
    """What sits in the other slot of a packed pair: the ray itself, a baseline ray, a non-finite ray, a ray whose `sane` differs."""
    rng = np.random.default_rng(seed)
    d = fam["d"]
    n = len(d)
    with np.errstate(all="ignore"):
        base = ((fam["C"] + _unit(rng, n) * (fam["r"] * rng.uniform(0, 2, n))[:, None] - fam["o"]) * rng.uniform(0.2, 2, (n, 1))).astype(f32)
        bad = d.copy()
        bad[np.arange(n), rng.integers(0, 3, n)] = rng.choice(f32([np.nan, np.inf, -np.inf, 0.0]), n)
        bad[rng.random(n) < 0.2] = 0
        a = dot(d, d)
        sane = (a > f32(1e-18)) & (a < f32(1e18))
        far = (d * np.where(rng.random(n) < 0.5, f32(2.0 ** 40), f32(2.0 ** -40))[:, None]).astype(f32)
        other = np.where(sane[:, None], far, _unit(rng, n).astype(f32)).astype(f32)
    return {"itself": d, "baseline": base, "nonfinite": bad, "other sane": other}


def scale_sweep(fam, ms=SCALES):
    """[(m, family scaled by 2^m)]"""
    return [(m, scaled(fam, m)) for m in ms]


def unit_families(n, shadow=False):
    """name -> family, the sizes in proportion to n (the threshold family's size)."""
    thr = threshold(n, 5, shadow)
    fams = {
        "threshold": thr,
        "tangent": tangent(n // 4, 7, shadow),
        "surface": surface(n // 4, 9, shadow),
        "baseline": baseline(n // 4, 11, shadow),
        "nonfinite": nonfinite(n // 8, 13, shadow),
    }
    sub = concat(take(thr, slice(0, n // 16)), take(fams["tangent"], slice(0, n // 64)), take(fams["surface"], slice(0, n // 64)))
    for m, f in scale_sweep(sub):
        if m != 0:
            fams["scale%+d" % m] = f
    return fams


# ------------------------------------------------------------- near ties, for the selection ----
def near_tie_pairs(n, seed=6):
    """Per record a ray (o, d) with an accepted hit t1 on sphere 1 (C1, r1), and sphere 2 (C2, r2) through the hit point
    P' = o + t1 d: C2 = P' + r2 n2 with n2 . d > 0, r2 then moved by k ulps, k = 0 (15 %) or +-2^u, u in [0, 8]."""
    rng = np.random.default_rng(seed)
    C = rng.uniform(-8, 8, (n, 3)).astype(f32)
    r = (10.0 ** rng.uniform(-1, 1, n)).astype(f32)
    o = (C + rng.normal(size=(n, 3)) * (r * rng.uniform(1.5, 10, n))[:, None]).astype(f32)
    aim = C + rng.normal(size=(n, 3)) * (r * 0.4)[:, None]
    d = ((aim - o) * rng.uniform(0.05, 0.6, n)[:, None]).astype(f32)
    t1 = exact_t2(o, d, C, r * r)
    t1 = np.where(accept(t1), t1, INF)
    with np.errstate(all="ignore"):
        Pp = o.astype(np.float64) + d.astype(np.float64) * np.where(np.isfinite(t1), t1, 1.0)[:, None]
    dn = d.astype(np.float64) / np.linalg.norm(d, axis=1, keepdims=True)
    n2 = dn * rng.uniform(0.3, 1, n)[:, None] + _perp(_unit(rng, n), dn) * rng.uniform(0, 0.8, n)[:, None]
    n2 /= np.linalg.norm(n2, axis=1, keepdims=True)
    r2 = (10.0 ** rng.uniform(-1, 1, n)).astype(f32)
    C2 = (Pp + n2 * r2[:, None]).astype(f32)
    k = np.rint(np.sign(rng.normal(size=n)) * 2.0 ** rng.uniform(0, 8, n)).astype(np.int64)
    k[rng.random(n) < 0.15] = 0
    r2 = (r2.view(np.int32) + k.astype(np.int32)).view(f32)
    return dict(o=o, d=d, C1=C, r1=r, C2=C2, r2=r2)


def selection_scenes(ns, n_scenes, seed=21):
    """Scenes of ns spheres for the selection op and the ray queries: [(rows [ns, 4] = C, r; o [n, 3]; d0 [n, 3]; d1 [n, 3])].
    Near-tie pairs in both orders, exact duplicates (twice, three times) at different indices, ties in the threshold band, further
    spheres in front, behind and missing; slot 1 holds another ray from the same origin."""
    rng = np.random.default_rng(seed + 1000 * ns)
    out = []
    for s in range(n_scenes):
        npairs = max(1, ns // 2)
        tp = near_tie_pairs(npairs, int(rng.integers(1 << 30)))
        rows = []
        for i in range(npairs):
            a = np.concatenate([tp["C1"][i], tp["r1"][i:i + 1]])
            b = np.concatenate([tp["C2"][i], tp["r2"][i:i + 1]])
            mode = (s + i) % 5
            if mode == 3:
                b = a.copy()                      # exact duplicate
            rows += [b, a] if (s + i) % 2 else [a, b]
            if mode == 4 and len(rows) < ns:
                rows.append(rows[-2].copy())      # the same row once more
        rows = rows[:ns]
        while len(rows) < ns:                     # further random spheres: anywhere, so in front, behind and missing
            if rng.random() < 0.3 and rows:
                rows.append(rows[int(rng.integers(len(rows)))].copy())  # a duplicate at a distant index
            else:
                rows.append(np.concatenate([rng.uniform(-8, 8, 3), [10.0 ** rng.uniform(-1, 0.5)]]).astype(f32))
        rows = np.array(rows, f32)
        perm_keep = (s % 3) != 2
        if not perm_keep:                         # a third of the scenes: table order shuffled
            rows = rows[rng.permutation(ns)]
        o = tp["o"].copy()
        d0 = tp["d"].copy()
        # a second set of the same rays stretched so that the tie sits at t ~ 1 (threshold band)
        t1 = exact_t2(o, d0, tp["C1"], tp["r1"] * tp["r1"])
        k = _ulps(rng, npairs, 6, 0.2)
        with np.errstate(all="ignore"):
            dthr = (d0.astype(np.float64) * (np.where(np.isfinite(t1), t1, 1.0) * (1 + k * 2.0 ** -24))[:, None]).astype(f32)
        o = np.concatenate([o, o])
        d0 = np.concatenate([d0, dthr])
        n = len(o)
        # slot 1: the same ray, an ulp-nudged copy, a ray at another sphere of the table, a stretched copy
        pick = rng.integers(0, 4, n)
        tgt = rows[rng.integers(0, ns, n)]
        d1 = np.where((pick == 0)[:, None], d0,
                      np.where((pick == 1)[:, None], (d0.astype(np.float64) * (1 + 2.0 ** -22)).astype(f32),
                               np.where((pick == 2)[:, None], ((tgt[:, :3] - o) * rng.uniform(0.1, 1.2, n)[:, None]).astype(f32),
                                        (d0 * f32(0.37)).astype(f32)))).astype(f32)
        out.append((rows, o.astype(f32), d0.astype(f32), d1))
    return out


def brute_force(rows, o, d):
    """raytrace.h:152-165 over the table: (index, t) of the closest accepted sphere, the first index winning ties (-1, inf: none);
    per-sphere accepted t [n, ns]."""
    rows = np.asarray(rows, f32)
    r2 = (rows[:, 3] * rows[:, 3]).astype(f32)
    t = exact_t2(o[:, None, :], d[:, None, :], rows[None, :, :3], r2[None, :])
    t = np.where(accept(t), t, INF).astype(f32)
    idx = np.argmin(t, axis=1)            # the first of equal minima
    tmin = t[np.arange(len(t)), idx]
    idx = np.where(tmin == INF, -1, idx).astype(np.int32)
    return idx, tmin.astype(f32), t


def shadow_tests(t):
    """The sphere tests utils.h:42-58 runs for one ray given its accepted t per sphere [n, ns]: i + 1 at the first accepted one, else ns."""
    acc = t != INF
    first = np.argmax(acc, axis=1)
    return np.where(acc.any(1), first + 1, t.shape[1]).astype(np.int64), acc.any(1)
