"""The triangle walks at their decision boundaries: restatements and a catalogue of cases (numpy, seeded, no GPU).

The restatements are numpy binary32 with the device's operation order: the acceptance test and its t (device_math.h triangle_hit),
the conservative line-sphere test (shade_common.h line_touches), the distance pruning of the closest-hit walk (entry_may_hold_nearer),
the walk itself (tree_walk_closest with tri_consider's update rule) for a lane that is alone in its wave, and brute force in file
order.  A lane alone in its wave prunes the most: in a wave an entry is entered when ANY lane's test says so, and a lane's own `mine`
flag is the same test with the same running best, so a lane in company sees every triangle it sees alone.

The families build rays (float32 [n, 8], the include/skr.h skr_ray layout) that sit on those decisions: formed in binary64 and rounded
once.  tests/test_triangle_cases_cpu.py holds their reach and the proof that the walk equals brute force on them;
tests/test_triangle_walks_gpu.py runs them on the device.  The restatements tests/test_culling_host.py has (triangle_accepts,
sphere_culls, tree_parents, _border_rays) are imported from there, as tests/test_camera_poses_cpu.py and
tests/test_triangle_shadows_cpu.py import them: there is one copy of each."""
import os

import numpy as np

import skele_raytracer_amd as skr
from conftest import scene_path
# the restatements tests/test_culling_host.py already has: one copy, there
from test_culling_host import BOUNDS, _border_rays, _cross, _dot, _soup_scene, sphere_culls, tree_parents, triangle_accepts  # noqa: F401

f32 = np.float32
LEVEL_LIMS = tuple(f32(b * b * 0.998) for b in BOUNDS)  # wave_common.h pick_query_tree
ARRAY_CAMERA = (0, 0, -10, 0, 0, 1, 0, 1, 0)


# ---- restatements -------------------------------------------------------------------------------------------------------------------
def triangle_terms(o, d, v0, e1, e2):
    """Every intermediate of utils.h:181-213 in binary32, in device_math.h triangle_hit's order: det, u, v, u + v, t (float32, broadcast
    shapes [..., 3] in).  Nothing is cut: a caller applies the decisions."""
    with np.errstate(all="ignore"):
        p = _cross(d, e2)
        det = _dot(e1, p)
        inv = f32(1.0) / det
        tv = o - v0
        u = inv * _dot(-tv, p)
        q = _cross(tv, e1)
        v = _dot(d, q) * inv
        t = _dot(e2, q) * inv
    return det, u, v, u + v, t


def triangle_t(o, d, v0, e1, e2):
    """(accepted, t): device_math.h triangle_hit.  t is meaningful where accepted (no t > 0 test, as there)."""
    with np.errstate(all="ignore"):
        det, u, v, uv, t = triangle_terms(o, d, v0, e1, e2)
        ok = ~(np.abs(det) < f32(0.00001))
        ok &= ~((u < 0) | (u > 1))
        ok &= ~((v < 0) | (uv > 1))
    return ok, t


def _radius2(d, dd, ent, cones):
    R2 = ent[..., 3]
    if cones:
        gb = _dot(d, ent[..., 4:7])
        R2 = np.where(gb * gb >= dd, ent[..., 7], ent[..., 3])
    return R2


def may_hold_nearer(o, d, entry, t_best, factor=1.27, cones=True):
    """shade_common.h entry_may_hold_nearer in binary32: (enter, lhs^2 / lim).  The ratio is 0 where lhs <= 0 (the entry's centre is
    not behind the running best) and where the line misses the sphere."""
    with np.errstate(all="ignore"):
        e = entry[..., :3] - o
        cr = _cross(e, d)
        dd = _dot(d, d)
        lim = _radius2(d, dd, entry, cones) * dd
        miss = _dot(cr, cr) > lim
        lhs = _dot(d, e) - t_best * dd
        l2 = lhs * lhs
        enter = ~miss & ~((lhs > 0) & (l2 > lim * f32(factor)))
        ratio = np.where(~miss & (lhs > 0), l2.astype(np.float64) / lim.astype(np.float64), 0.0)
    return enter, np.nan_to_num(ratio, nan=0.0, posinf=0.0)


def ray_parts(rays):
    r = np.ascontiguousarray(rays, f32).reshape(-1, 8)
    return r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7].copy().view(np.int32)


def start_best(rays, t_sphere=None):
    """The running best a query's walk starts at: trace_rays.hip `fminf(ts, tmax)`."""
    tmax = ray_parts(rays)[2]
    return tmax.copy() if t_sphere is None else np.fmin(np.asarray(t_sphere, f32), tmax)


def walk_closest(tree, rays, factor=1.27, cones=True, t_start=None):
    """shade_common.h tree_walk_closest for every ray as a lane alone in its wave, over `tree` = Scene.culling(level) or
    Scene.trace_culling(level): nodes depth-first by skip link, the chunk entries of a height-1 node, tri_consider's update rule with
    the ray's ignore_triangle.  t_start [n]: the running best at the start (start_best: tmax, or the closest sphere's t where nearer).
    Returns (file index of the winner or -1, its t or t_start, lhs^2 / lim of the chunk entry that delivered the winner, whether the
    tie arm `t == b.t && file < b.file` installed it)."""
    cs, tris, sph, links, ch = tree[:5]
    o, d, tmax, ign = ray_parts(rays)
    n, nn, nt = len(o), links.shape[0], tris.shape[0]
    best_t = (start_best(rays) if t_start is None else np.asarray(t_start, f32)).copy()
    best_file = np.full(n, -1, np.int64)
    best_ratio = np.zeros(n)
    best_tie = np.zeros(n, bool)
    files = tris[:, 1, 3].copy().view(np.int32).astype(np.int64)
    node = np.zeros(n, np.int64)
    while True:
        idx = np.nonzero(node < nn)[0]
        if idx.size == 0:
            break
        i = node[idx]
        enter, _ = may_hold_nearer(o[idx], d[idx], sph[i], best_t[idx], factor, cones)
        count = links[i, 2]
        for c in range(int(count[enter].max()) if enter.any() else 0):
            sel = enter & (count > c)
            r = idx[sel]
            chunk = links[i[sel], 1] + c
            mine, ratio = may_hold_nearer(o[r], d[r], ch[chunk], best_t[r], factor, cones)
            r, chunk, ratio = r[mine], chunk[mine], ratio[mine]
            for k in range(cs):
                slot = chunk * cs + k
                inside = slot < nt
                rr, sl, rat = r[inside], slot[inside], ratio[inside]
                ok, t = triangle_t(o[rr], d[rr], tris[sl, 0, :3], tris[sl, 1, :3], tris[sl, 2, :3])
                with np.errstate(invalid="ignore"):
                    ok &= t > 0
                    file = files[sl]
                    nearer = t < best_t[rr]
                    tie = (t == best_t[rr]) & (best_file[rr] >= 0) & (file < best_file[rr])
                take = ok & (file != ign[rr]) & (nearer | tie)
                w = rr[take]
                best_t[w], best_file[w], best_ratio[w], best_tie[w] = t[take], file[take], rat[take], tie[take]
        node[idx] = np.where(enter, i + 1, links[i, 0])
    return best_file, best_t, best_ratio, best_tie


def brute_closest(triangles, rays, t_start=None, block=128):
    """Every triangle of `triangles` (float32 [nt, 9], Scene.arrays(): file order) with a strict `<`: (winner or -1, its t or t_start)."""
    tr = np.ascontiguousarray(triangles, f32).reshape(-1, 3, 3)
    o, d, tmax, ign = ray_parts(rays)
    n = len(o)
    best_t = (start_best(rays) if t_start is None else np.asarray(t_start, f32)).copy()
    best_file = np.full(n, -1, np.int64)
    v0, e1, e2 = tr[:, 0], tr[:, 1] - tr[:, 0], tr[:, 2] - tr[:, 0]  # utils.h:183-184
    rows = max(1, (1 << 22) // max(block, 1))
    for r0 in range(0, n, rows):
        rs = slice(r0, min(n, r0 + rows))
        oo, ddd = o[rs, None, :], d[rs, None, :]
        for k0 in range(0, len(tr), block):
            ks = slice(k0, min(len(tr), k0 + block))
            ok, t = triangle_t(oo, ddd, v0[None, ks], e1[None, ks], e2[None, ks])
            with np.errstate(invalid="ignore"):
                ok &= t > 0
            ok &= np.arange(ks.start, ks.stop)[None, :] != ign[rs, None]
            t = np.where(ok, t, f32(np.inf))
            j = np.argmin(t, axis=1)  # the first of equal values: the lower file index
            tj = t[np.arange(t.shape[0]), j]
            better = tj < best_t[rs]
            best_t[rs] = np.where(better, tj, best_t[rs])
            best_file[rs] = np.where(better, j + k0, best_file[rs])
    return best_file, best_t


def query_level(dd):
    """wave_common.h pick_query_tree for a wave of one lane: 0, 1, 2, or 3 = no tree (NaN and inf: 3)."""
    dd = np.asarray(dd, f32)
    level = np.zeros(dd.shape, np.int64)
    with np.errstate(invalid="ignore"):
        for k, lim in enumerate(LEVEL_LIMS):
            level += (level == k) & ~(dd < lim)
    return level


def in_ball(o, ball):
    """pick_query_tree's rule (b) in binary32."""
    e = np.asarray(o, f32) - ball[:3]
    with np.errstate(invalid="ignore"):
        return _dot(e, e) <= ball[3] * ball[3]


def pack_rays(o, d, tmax=None, ignore=None):
    o = np.asarray(o, np.float64).reshape(-1, 3)
    r = np.zeros((len(o), 8), f32)
    r[:, 0:3] = o
    r[:, 4:7] = np.asarray(d, np.float64).reshape(-1, 3)
    r[:, 3] = np.inf if tmax is None else tmax
    ign = np.full(len(o), -1, np.int32) if ignore is None else np.broadcast_to(np.asarray(ignore, np.int32), (len(o),))
    r[:, 7] = np.ascontiguousarray(ign).view(f32)
    return r


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
_scene_cache = {}


def load(scene):
    """A family's scene -> (skr.Scene, spheres [ns, 14], triangles [nt, 9] in file order).  `scene` is a .scn path or a float32
    [nt, 9] array of triangles (a sphere-free scene under ARRAY_CAMERA)."""
    key = scene if isinstance(scene, str) else id(scene)
    if key not in _scene_cache:
        if isinstance(scene, str):
            sc = skr.parse_scene(scene)
        else:
            sc = skr.Scene.from_arrays(np.zeros((0, 14), f32), scene, np.zeros((0, 6), f32), ARRAY_CAMERA)
        s, t, _ = sc.arrays()
        _scene_cache[key] = (sc, s, t, scene)  # (the array is kept alive: its id is the key)
    return _scene_cache[key][:3]


def camera_of(sc):
    return np.array(list(sc.info.camera)[:3], f32)


def accept_corners(tri9):
    """The corners (v0, v0 - e1, v0 + e2) of the region utils.h:181-213 accepts, binary64 [n, 3, 3], from file triangles [n, 9]."""
    t = np.asarray(tri9, f32).reshape(-1, 3, 3)
    v0 = t[:, 0].astype(np.float64)
    e1, e2 = (t[:, 1] - t[:, 0]).astype(np.float64), (t[:, 2] - t[:, 0]).astype(np.float64)
    return np.stack([v0, v0 - e1, v0 + e2], axis=1)


def soup_path(folder):
    """test_culling_host's soup (small triangles between a camera and a few spheres: chunk spheres bounded at every level) as a file."""
    import pathlib
    _soup_scene(pathlib.Path(str(folder)))
    return os.path.join(str(folder), "soup.scn")


def border_targets(tris, k, o, d):
    """Where each ray of _border_rays meets the plane of the triangle it was aimed at (binary64 [n, 3]: the border point, up to the
    rounding of o and d), and whether that is well conditioned (the ray does not graze the triangle, which has an area)."""
    t = tris[k].astype(np.float64)
    v0, nrm = t[:, 0, :3], np.cross(t[:, 1, :3], t[:, 2, :3])
    o, d = o.astype(np.float64), d.astype(np.float64)
    dn = np.sum(d * nrm, axis=1)
    ok = np.abs(dn) > 1e-3 * np.linalg.norm(d, axis=1) * np.linalg.norm(nrm, axis=1)
    s = np.sum((v0 - o) * nrm, axis=1) / np.where(ok, dn, 1.0)
    return o + s[:, None] * d, ok


def ulp_step(x, steps):
    """x (float32 array) moved by `steps` (int array) units in the last place."""
    x = np.ascontiguousarray(x, f32)
    bits = x.view(np.int32).astype(np.int64)
    key = np.where(bits < 0, -(bits & 0x7fffffff), bits) + steps  # monotone integer image of the floats
    out = np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)
    return out.view(f32).reshape(x.shape)


def ulps_apart(a, b):
    """Signed distance a - b in units in the last place (int64), for finite float32 arrays."""
    def key(x):
        bits = np.ascontiguousarray(x, f32).view(np.int32).astype(np.int64)
        return np.where(bits < 0, -(bits & 0x7fffffff), bits)
    return key(a) - key(b)


def _ball_origins(rng, sc, n):
    """Origins anywhere in the middle half of the trace ball (well inside: rule (b) of pick_query_tree holds for each)."""
    ball = sc.trace_culling(0)[5].astype(np.float64)
    v = rng.normal(size=(n, 3))
    v *= (rng.random((n, 1)) ** (1 / 3)) * 0.5 * ball[3] / np.linalg.norm(v, axis=1, keepdims=True)
    return ball[:3] + v


# ---- families: each returns (scene, rays float32 [n, 8], meta) ------------------------------------------------------------------------
def plate_triangles(cells=12, seed=3):
    """A cells x cells tessellated plate facing the array camera, slightly tilted; its vertices are shared exactly."""
    rng = np.random.default_rng(seed)
    g = np.linspace(-3.0, 3.0, cells + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    z = 2.0 + 0.31 * x - 0.17 * y
    p = np.stack([x, y, z], axis=-1).astype(f32)
    tris = []
    for j in range(cells):
        for i in range(cells):
            a, b, c, e = p[j, i], p[j, i + 1], p[j + 1, i + 1], p[j + 1, i]
            tris += [np.concatenate(q) for q in ((a, b, c), (a, c, e))]
    tris = np.array(tris, f32)
    return tris[rng.permutation(len(tris))]  # file order is not the grid's


_arrays = {}


def _memo(name, make):
    if name not in _arrays:
        _arrays[name] = make()
    return _arrays[name]


def deck_triangles(decks=40, cards=8, seed=11):
    """`decks` stacks of `cards` small parallel triangles receding from the array camera along the line of sight of the stack, and one
    wide triangle just behind each stack's first card.  A ray through a stack finds the wide triangle or a far card first (the
    device order is a Morton curve, not depth) and must then still visit the chunk whose centre lies behind that best."""
    rng = np.random.default_rng(seed)
    cam = np.array(ARRAY_CAMERA[:3], np.float64)
    out, meta = [], []
    for k in range(decks):
        c = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(0, 8)])
        w = (c - cam) / np.linalg.norm(c - cam)
        a = np.cross(w, rng.normal(size=3))
        a /= np.linalg.norm(a)
        b = np.cross(w, a)
        size, gap = rng.uniform(0.008, 0.02), rng.uniform(0.25, 0.6)  # small cards: little rounding slack in the radii
        first = len(out)
        for j in range(cards):
            centre = c + w * gap * j
            # the accept region (v0, v0 - e1, v0 + e2) is centred on the line of sight
            e1, e2 = size * (a + 0.3 * b), size * (0.2 * a + b)
            v0 = centre - (e2 - e1) / 3
            out.append(np.concatenate([v0, v0 + e1, v0 + e2]))
        # the wide triangle: behind the first card by a small part of the gap.  Its accept region reaches 90 units towards -x and -y,
        # so its centre lies in the low half of the scene's box on both axes (of the centres' and of the corners'): the Morton order puts every wide triangle before every
        # card, and a ray has the wide triangle's t as its running best when it comes to the cards
        behind = c + w * gap * rng.uniform(0.02, 0.15)
        ax, ay = np.array([-1.0, -0.9, 0]), np.array([-0.9, -1.0, 0])
        ax, ay = ax - w * np.dot(ax, w), ay - w * np.dot(ay, w)
        ax, ay = 90 * ax / np.linalg.norm(ax), 90 * ay / np.linalg.norm(ay)
        c0, c1, c2 = behind + ax, behind + ay, behind - 0.01 * (ax + ay)
        v0, e1, e2 = c0, c0 - c1, c2 - c0  # region: (v0, v0 - e1, v0 + e2) = (c0, c1, c2)
        out.append(np.concatenate([v0, v0 + e1, v0 + e2]))
        meta.append((first, cards, c, w, a, b, size, gap))
    tris = np.array(out, f32)
    return tris, meta


def decks(n=20000, seed=12):
    tris, meta = _memo("decks", deck_triangles)
    rng = np.random.default_rng(seed)
    cam = np.array(ARRAY_CAMERA[:3], np.float64)
    k = rng.integers(0, len(meta), n)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        first, cards, c, w, a, b, size, gap = meta[k[i]]
        P = c + size * 0.15 * (rng.uniform(-1, 1) * a + rng.uniform(-1, 1) * b)
        o[i] = cam
        d[i] = (P - cam) / np.linalg.norm(P - cam) * rng.choice([0.5, 1.0, 2.0, 3.5])
    # the second half starts off the camera, in the ball, on the stack's line of sight: the trace tree
    half = np.arange(n) >= n // 2
    back = rng.uniform(0.5, 6.0, (n, 1))
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    tgt = o + dn * np.linalg.norm(np.array([meta[j][2] for j in k]) - cam, axis=1, keepdims=True)
    o = np.where(half[:, None], tgt - dn * back, o)
    return tris, pack_rays(o, d), {"deck": k}


def nest_triangles(pairs=134, seed=21, third=True):
    """Pairs (T, 2^k T about v0), k in {1, 2, 3}: e1' = 2^k e1, e2' = 2^k e2, so det, q and inv scale exactly and both give the same
    bits of t wherever both accept.  Coordinates are multiples of 2^-10 below 16, so every sum here is exact in binary32.  Half the
    pairs have the scaled copy first in the file; the two file indices are `pairs` apart.  third: half of them also get a third
    triangle behind the pair that ties with neither."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -10
    v0 = np.round(rng.uniform(-4, 4, (pairs, 3)) / q) * q
    v0[:, 2] = np.round(rng.uniform(0, 6, pairs) / q) * q
    e1 = np.round(rng.uniform(-0.12, 0.12, (pairs, 3)) / q) * q
    e2 = np.round(rng.uniform(-0.12, 0.12, (pairs, 3)) / q) * q
    k = rng.integers(1, 4, pairs)
    s = (2.0 ** k)[:, None]
    small = np.concatenate([v0, v0 + e1, v0 + e2], axis=1)
    large = np.concatenate([v0, v0 + s * e1, v0 + s * e2], axis=1)
    large_first = rng.random(pairs) < 0.5
    first = np.where(large_first[:, None], large, small)
    second = np.where(large_first[:, None], small, large)
    tris = [first, second]
    if third:
        cam = np.array(ARRAY_CAMERA[:3], np.float64)
        centre = v0 + (e2 - e1) / 3
        w = centre - cam
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        a = np.cross(w, rng.normal(size=(pairs, 3)))
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        b = np.cross(w, a)
        c3 = centre + w * rng.uniform(0.05, 0.4, (pairs, 1))
        v3 = c3 - 0.5 * (b - a) / 3
        t3 = np.concatenate([v3, v3 + 0.5 * a, v3 + 0.5 * b], axis=1)
        tris.append(t3[rng.random(pairs) < 0.5])
    tris = np.concatenate(tris).astype(f32)
    assert np.array_equal(tris[:2 * pairs].astype(np.float64), np.concatenate([first, second]))  # nothing was rounded
    return tris, {"v0": v0, "e1": e1, "e2": e2, "large_first": large_first, "pairs": pairs}


def nests(per_pair=80, seed=22, third=True):
    tris, m = _memo("nests%d" % third, lambda: nest_triangles(third=third))
    rng = np.random.default_rng(seed)
    pairs = m["pairs"]
    n = pairs * per_pair
    k = np.repeat(np.arange(pairs), per_pair)
    # a point of the common accept region: the small triangle's (v0, v0 - e1, v0 + e2), strictly inside
    u, v = rng.uniform(0.02, 0.96, n), rng.uniform(0.02, 0.96, n)
    flip = u + v > 0.98
    u, v = np.where(flip, 0.98 - u, u), np.where(flip, 0.98 - v, v)
    P = m["v0"][k] - u[:, None] * m["e1"][k] + v[:, None] * m["e2"][k]
    cam = np.array(ARRAY_CAMERA[:3], np.float64)
    o = np.repeat(cam[None], n, axis=0)
    sc = load(tris)[0]
    away = _ball_origins(rng, sc, n)
    from_ball = (np.arange(n) % per_pair) >= per_pair // 2
    o = np.where(from_ball[:, None], away, o)
    d = P - o
    d *= rng.choice([0.3, 1.0, 3.0], n)[:, None] / np.linalg.norm(d, axis=1, keepdims=True)
    order = np.argsort(from_ball, kind="stable")  # whole waves at the camera first
    rays, k = pack_rays(o, d)[order], k[order]
    again = rays.copy()  # the same rays with the tie's lower file index ignored: the higher one must win
    again[:, 7] = k.astype(np.int32).view(f32)
    return tris, np.concatenate([rays, again]), {"pair": np.concatenate([k, k]), "pairs": pairs}


def border(scene, level, n, seed=7, tree="renderer"):
    """_border_rays on `scene`.  tree = "renderer": every ray starts at the camera (the waves of such rays walk the renderer's tree);
    "trace": the origins _border_rays chose beside the camera (sphere surfaces, points near the grazed triangle) and origins in the ball."""
    sc = load(scene)[0]
    tris = sc.culling(level)[1]
    rng = np.random.default_rng(seed + level)
    k, o, d = _border_rays(rng, sc, tris, 4 * n, level)
    P, aimed = border_targets(tris, k, o, d)
    cam = camera_of(sc)
    at_cam = np.all(o == cam[None], axis=1)
    file = tris[:, 1, 3].copy().view(np.int32)  # k indexes the device order
    if tree == "renderer":
        keep = np.nonzero(at_cam)[0][:n]
        return scene, pack_rays(o[keep], d[keep]), {"tri_file": file[k[keep]]}
    keep = np.nonzero(~at_cam & in_ball(o, sc.trace_culling(level)[5]))[0][:n // 2]
    more = np.nonzero(at_cam & aimed)[0][:n - len(keep)]  # their targets, from origins in the ball
    o2 = _ball_origins(rng, sc, len(more))
    o2 = o2.astype(f32).astype(np.float64)
    d2 = P[more] - o2
    d2 *= np.linalg.norm(d[more].astype(np.float64), axis=1, keepdims=True) / np.linalg.norm(d2, axis=1, keepdims=True)
    return scene, np.concatenate([pack_rays(o[keep], d[keep]), pack_rays(o2, d2)]), {"tri_file": file[np.concatenate([k[keep], k[more]])]}


EDGE_A = (0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24, 1.0)


def _edge_targets(rng, A, B, n_each):
    """Targets a A + (1 - a) B for a in EDGE_A and random a (binary64, not yet rounded), and every target rounded to binary32 and moved
    by +-1, +-4 ulps (each coordinate, one random sign pattern): [m, 3] with the index of the (A, B) pair of each."""
    m = len(A)
    a = np.concatenate([np.repeat(np.array(EDGE_A)[None], m, axis=0), rng.random((m, n_each))], axis=1)
    P = a[..., None] * A[:, None, :] + (1 - a[..., None]) * B[:, None, :]
    which = np.repeat(np.arange(m)[:, None], a.shape[1], axis=1)
    P, which = P.reshape(-1, 3), which.reshape(-1)
    out, idx = [P], [which]
    for steps in (1, -1, 4, -4):
        sign = rng.choice([-1, 1], P.shape)
        out.append(ulp_step(P.astype(f32), steps * sign).astype(np.float64))
        idx.append(which)
    return np.concatenate(out), np.concatenate(idx)


def edges(which="plate", pairs=2000, seed=31):
    """Targets on the edges two triangles share and at shared vertices.  plate: every edge of every accept region of the tessellated
    plate (a regular grid: each is an edge or a diagonal of the grid, shared with the neighbours' regions and triangles).  dragon:
    `pairs` dragon.scn triangles with a neighbour across an edge: targets on that shared edge and on the three edges of the first
    triangle's accept region.  Half the rays start at the camera.  The others start close to their target, so that the rounding of d
    moves the ray by less than a unit of the triangle's u, v (an ulp of a dragon vertex is 40 such units), with |d| brought into
    [2, 4) by a power of two: long enough for the |det| >= 1e-5 cut on dragon's small triangles."""
    rng = np.random.default_rng(seed)
    if which == "plate":
        scene = _memo("plate", plate_triangles)
        sc, _, t = load(scene)
        c = accept_corners(t)
        A = np.concatenate([c[:, 0], c[:, 1], c[:, 2]])
        B = np.concatenate([c[:, 1], c[:, 2], c[:, 0]])
        tri = np.tile(np.arange(len(t)), 3)
        P, w = _edge_targets(rng, A, B, 3)
        near = (0.5, 2.0)
    else:
        scene = scene_path("dragon.scn")
        sc, _, t = load(scene)
        v = t.reshape(-1, 3, 3)
        owner = {}
        for i in range(len(v)):
            for a, b in ((0, 1), (1, 2), (2, 0)):
                owner.setdefault(tuple(sorted((v[i, a].tobytes(), v[i, b].tobytes()))), []).append(i)
        found = []
        for i in dragon_sample(rng, t, len(t)):
            for a, b in ((0, 1), (1, 2), (2, 0)):
                if len(owner[tuple(sorted((v[i, a].tobytes(), v[i, b].tobytes())))]) > 1:
                    found.append((i, v[i, a], v[i, b]))
                    break
            if len(found) >= pairs:
                break
        tri = np.array([f[0] for f in found])
        c = accept_corners(t[tri])
        A = np.concatenate([np.array([f[1] for f in found], np.float64), c[:, 0], c[:, 1], c[:, 2]])
        B = np.concatenate([np.array([f[2] for f in found], np.float64), c[:, 1], c[:, 2], c[:, 0]])
        tri = np.tile(tri, 4)
        P, w = _edge_targets(rng, A, B, 2)
        near = (0.1, 0.4)
    cam = camera_of(sc).astype(np.float64)
    n = len(P)
    from_near = rng.random(n) < 0.5
    dirn = rng.normal(size=(n, 3))
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    o = np.where(from_near[:, None], P - dirn * rng.uniform(*near, (n, 1)), cam[None]).astype(f32).astype(np.float64)
    d = P - o
    ln = np.linalg.norm(d, axis=1, keepdims=True)
    exact = 2.0 ** np.ceil(np.log2(2.0 / ln))  # into [2, 4), exactly
    d = np.where(from_near[:, None], d * exact, d / ln * rng.uniform(2.0, 3.9, (n, 1)))
    order = np.argsort(from_near, kind="stable")  # camera waves first
    return scene, pack_rays(o, d)[order], {"tri": tri[w][order]}


def dragon_sample(rng, t, count, area2=1.5e-5):
    """`count` dragon.scn triangles (file indices) that a ray of |d| = 2 .. 4 can pass the |det| >= 1e-5 cut on: |e1 x e2| >= area2
    (the median dragon triangle has 8e-6, and det = |d| |e1 x e2| cos)."""
    v = t.reshape(-1, 3, 3).astype(np.float64)
    big = np.nonzero(np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) >= area2)[0]
    return big[rng.permutation(len(big))[:count]]


def _inner_points(rng, c, n):
    """Points well inside accept regions c [m, 3, 3] (binary64), n per region: ([m * n, 3], region index)."""
    m = len(c)
    u, v = rng.uniform(0.1, 0.8, (m, n)), rng.uniform(0.1, 0.8, (m, n))
    flip = u + v > 0.9
    u, v = np.where(flip, 0.9 - u, u), np.where(flip, 0.9 - v, v)
    P = c[:, None, 0] + u[..., None] * (c[:, None, 1] - c[:, None, 0]) + v[..., None] * (c[:, None, 2] - c[:, None, 0])
    return P.reshape(-1, 3), np.repeat(np.arange(m), n)


def det_cut(triangles=1500, seed=41):
    """Rays into the inside of dragon.scn accept regions with d scaled (det is linear in d) so that the restated binary32 det sits on
    the 1e-5 cut: scales s (1 + j 2^-23), j in -6 .. 6, around the one that lands on it.  From both sides of each triangle: both
    signs of det."""
    rng = np.random.default_rng(seed)
    scene = scene_path("dragon.scn")
    sc, _, t = load(scene)
    tri = dragon_sample(rng, t, triangles)
    c = accept_corners(t[tri])
    P, w = _inner_points(rng, c, 2)
    tri = tri[w]
    n = len(P)
    side = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    nrm = np.cross(c[w, 1] - c[w, 0], c[w, 2] - c[w, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    dirn = nrm * side[:, None] * rng.uniform(0.3, 1.0, (n, 1)) + rng.normal(size=(n, 3)) * 0.4
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    cam = camera_of(sc).astype(np.float64)
    from_cam = rng.random(n) < 0.5
    o = np.where(from_cam[:, None], cam[None], P - dirn * rng.uniform(0.5, 4.0, (n, 1)))
    o = o.astype(f32)
    d = P - o.astype(np.float64)
    v = t[tri].reshape(-1, 3, 3)
    v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    det0 = triangle_terms(o, d.astype(f32), v0, e1, e2)[0].astype(np.float64)
    ok = np.abs(det0) > 1e-12
    s = np.where(ok, 1e-5 / np.abs(np.where(ok, det0, 1.0)), 1.0)
    for _ in range(3):  # land on the cut under the rounding of d and of det
        det = triangle_terms(o, (d * s[:, None]).astype(f32), v0, e1, e2)[0].astype(np.float64)
        s = np.where(ok & (det != 0), s * 1e-5 / np.abs(np.where(det != 0, det, 1.0)), s)
    j = np.arange(-6, 7)
    S = s[:, None] * (1 + j[None, :] * 2.0 ** -23)
    keep = ok & (np.linalg.norm(d, axis=1) * s < 3.9)
    o = np.repeat(o[keep][:, None, :], len(j), axis=1).reshape(-1, 3)
    dd = (d[keep][:, None, :] * S[keep][:, :, None]).reshape(-1, 3)
    tri = np.repeat(tri[keep], len(j))
    at_cam = np.repeat(from_cam[keep], len(j))
    order = np.argsort(~at_cam, kind="stable")
    return scene, pack_rays(o, dd)[order], {"tri": tri[order]}


def t_zero(triangles=1500, seed=51):
    """Origins on the plane of a dragon.scn triangle, inside its accept region, and moved off it by +-1, +-4 ulps of each coordinate
    along d; each ray with and without ignore_triangle set to that triangle."""
    rng = np.random.default_rng(seed)
    scene = scene_path("dragon.scn")
    sc, _, t = load(scene)
    tri = dragon_sample(rng, t, triangles)
    c = accept_corners(t[tri])
    P, w = _inner_points(rng, c, 2)
    tri = tri[w]
    n = len(P)
    nrm = np.cross(c[w, 1] - c[w, 0], c[w, 2] - c[w, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    d = nrm * rng.choice([-1.0, 1.0], (n, 1)) + rng.normal(size=(n, 3)) * 0.5
    d *= rng.choice([2.0, 3.0, 3.9], (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    o0 = P.astype(f32)
    steps = np.array([0, 1, -1, 4, -4])
    sgn = np.sign(d).astype(np.int64)
    o = np.stack([ulp_step(o0, sgn * s) for s in steps], axis=1).reshape(-1, 3)
    d = np.repeat(d[:, None, :], len(steps), axis=1).reshape(-1, 3)
    tri = np.repeat(tri, len(steps))
    rays = pack_rays(o, d)
    own = rays.copy()
    own[:, 7] = tri.astype(np.int32).view(f32)
    return scene, np.concatenate([rays, own]), {"tri": np.concatenate([tri, tri])}


def cone_edge(scene=None, level=0, per_entry=6, entries=400, seed=61):
    """Per chunk entry of the trace tree with a cone (entry[4:7] != 0): directions on the border of the cone, (d . B)^2 within a few
    ulps of d . d on both sides, through a point of one of the entry's accept regions, from an origin in the ball.  The border is
    found by bisection on the angle to the axis under the restated binary32 test."""
    rng = np.random.default_rng(seed)
    scene = scene_path("test.scn") if scene is None else scene
    sc, _, t = load(scene)
    cs, tris, sph, links, ch, ball = sc.trace_culling(level)
    has = np.nonzero(np.any(ch[:, 4:7] != 0, axis=1))[0]
    has = has[rng.permutation(len(has))[:entries]]
    e = np.repeat(has, per_entry)
    n = len(e)
    slot = np.minimum(e * cs + rng.integers(0, cs, n), len(tris) - 1)
    file = tris[slot, 1, 3].copy().view(np.int32)
    P, _ = _inner_points(rng, accept_corners(t[file]), 1)
    B = ch[e, 4:7]
    axis = B.astype(np.float64) / np.linalg.norm(B.astype(np.float64), axis=1, keepdims=True)
    w = np.cross(axis, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    length = rng.choice([0.5, 1.0, 3.0], (n, 1))

    def direction(alpha):
        return ((np.cos(alpha)[:, None] * axis + np.sin(alpha)[:, None] * w) * length).astype(f32)

    def inside(alpha):
        d = direction(alpha)
        gb = _dot(d, B)
        return gb * gb >= _dot(d, d)

    lo, hi = np.zeros(n), np.full(n, np.pi / 2)
    usable = inside(lo) & ~inside(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        m = inside(mid)
        lo, hi = np.where(m, mid, lo), np.where(m, hi, mid)
    alphas = np.stack([lo, hi, lo - 2e-7, hi + 2e-7, lo - 1e-6, hi + 1e-6], axis=1)[usable]
    P, B, e = P[usable], B[usable], e[usable]
    axis, w, length = axis[usable], w[usable], length[usable]
    rays, ent = [], []
    for j in range(alphas.shape[1]):
        d = direction(alphas[:, j]).astype(np.float64)
        back = rng.uniform(0.2, 0.45, (len(d), 1)) * float(ball[3]) / np.linalg.norm(d, axis=1, keepdims=True)
        rays.append(pack_rays(P - d * back, d))
        ent.append(e)
    rays, ent = np.concatenate(rays), np.concatenate(ent)
    keep = in_ball(rays[:, 0:3], ball)
    return scene, rays[keep], {"entry": ent[keep], "level": level}


def graze_triangles(grid=10, per=12, seed=71):
    """grid x grid large triangles 10 units apart, each grazed by `per` rays (sin phi 1e-6 .. 1e-2) through points of its accept
    region, and per ray a small face-on triangle across it whose t lies within 1e-3 relative of the grazed one's, before or behind it."""
    rng = np.random.default_rng(seed)
    tris, rays, grazed, face = [], [], [], []
    for k in range(grid * grid):
        c = np.array([10.0 * (k % grid) - 5.0 * grid, 10.0 * (k // grid) - 5.0 * grid, rng.uniform(0, 2)])
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        a = np.cross(nrm, rng.normal(size=3))
        a /= np.linalg.norm(a)
        b = np.cross(nrm, a)
        size = rng.uniform(2.0, 4.0)
        e1, e2 = size * a, size * b
        v0 = c - (e2 - e1) / 3  # accept region (v0, v0 - e1, v0 + e2) centred on c
        big = len(tris)
        tris.append(np.concatenate([v0, v0 + e1, v0 + e2]))
        for _ in range(per):
            u, v = rng.uniform(0.15, 0.4, 2)
            P = v0 - u * e1 + v * e2
            sinphi = 10.0 ** rng.uniform(-6, -2) * rng.choice([-1.0, 1.0])
            ang = rng.uniform(0, 2 * np.pi)
            dirn = (np.cos(ang) * a + np.sin(ang) * b) * np.sqrt(1 - sinphi ** 2) + nrm * sinphi
            length = rng.uniform(2.0, 3.9)
            o = (P - dirn * length * rng.uniform(0.3, 1.2)).astype(f32).astype(np.float64)
            d = (dirn * length).astype(f32).astype(np.float64)
            tg = np.dot(P - o, nrm) / np.dot(d, nrm)  # the exact t of the rounded ray on the grazed plane
            rel = 10.0 ** rng.uniform(-7, -3) * rng.choice([-1.0, 1.0])
            Pf = o + d * tg * (1 + rel)
            w = d / np.linalg.norm(d)
            fa = np.cross(w, rng.normal(size=3))
            fa /= np.linalg.norm(fa)
            fb = np.cross(w, fa)
            fs = 0.1
            f0 = Pf - fs * (fb - fa) / 3
            grazed.append(big)
            face.append(len(tris))
            tris.append(np.concatenate([f0, f0 + fs * fa, f0 + fs * fb]))
            rays.append(np.concatenate([o, d]))
    return np.array(tris, f32), np.array(rays), np.array(grazed), np.array(face)


def graze_behind():
    tris, r, grazed, face = _memo("graze", graze_triangles)
    return tris, pack_rays(r[:, 0:3], r[:, 3:6]), {"grazed": grazed, "face_on": face}


def levels(scene, n=1536, seed=81):
    """The rays of border(scene, trace and renderer) with d . d set on lim[k] of pick_query_tree, k = 0, 1, 2: d rescaled so that the
    restated binary32 d . d lands within 2 ulps of lim[k], on both sides of it; and rays with |d| = 300 (no tree)."""
    rng = np.random.default_rng(seed)
    parts = []
    for tree in ("renderer", "trace"):
        base = border(scene, 0, n, seed=seed, tree=tree)[1]
        for k, lim in enumerate(LEVEL_LIMS):
            r = base[rng.permutation(len(base))[:n // 2]].copy()
            d = r[:, 4:7].astype(np.float64)
            s = np.sqrt(float(lim) / np.sum(d * d, axis=1))
            best = None
            for j in np.arange(-8, 9):
                dj = (d * (s * (1 + j * 2.0 ** -24))[:, None]).astype(f32)
                off = ulps_apart(_dot(dj, dj), np.full(len(dj), lim, f32))
                cand = r.copy()
                cand[:, 4:7] = dj
                near = np.abs(off) <= 2
                best = cand[near] if best is None else np.concatenate([best, cand[near]])
            best = best[rng.permutation(len(best))[:n // 2]]
            dd = _dot(best[:, 4:7], best[:, 4:7])
            parts.append(best[np.argsort(~(dd < lim), kind="stable")])  # whole waves below lim[k] first, then the waves at and above it
        far = base[: n // 8].copy()
        d = far[:, 4:7].astype(np.float64)
        far[:, 4:7] = d * 300.0 / np.linalg.norm(d, axis=1, keepdims=True)
        parts.append(far)
    return scene, np.concatenate(parts), {}


def write_scn(path, triangles, lights=1):
    """`triangles` (float32 [nt, 9]) as a .scn file under ARRAY_CAMERA, with three spheres beside and behind the mesh and `lights` point
    lights in front of it: every value with 9 digits, so the parser reads back the same binary32 numbers."""
    t = np.asarray(triangles, f32).reshape(-1, 3, 3)
    lines = ["camera 0 0 -10 0 0 1 0 1 0 30", "background .1 .2 .3", "ambient_light .3 .3 .3",
             "material .6 .6 .6 .7 .7 .7 .2 .2 .2 8 0 0 0 1", "sphere 0 -46 4 40",
             "material .8 .3 .2 .6 .6 .6 .3 .3 .3 20 0 0 0 1", "sphere -4.5 3.5 9 1.5",
             "material .2 .4 .8 .5 .5 .5 .4 .4 .4 5 0 0 0 1", "sphere 4 -3 10 2"]
    for v in t.reshape(-1, 3):
        lines.append("vertex %.9g %.9g %.9g" % tuple(float(x) for x in v))
    for i in range(len(t)):
        if i % 7 == 0:
            lines.append("material %.3g %.3g %.3g .6 .6 .6 .2 .2 .2 6 0 0 0 1" % (0.2 + 0.1 * (i % 5), 0.3 + 0.1 * (i % 3), 0.9 - 0.1 * (i % 4)))
        lines.append("triangle %d %d %d" % (3 * i, 3 * i + 1, 3 * i + 2))
    lines += ["point_light 30 30 30 2 6 -7", "point_light 20 25 30 -5 3 -4"][:lights]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


# the shadow walk's far end: the occluder of tests/triangle_shadow_check.py lifted into the plane of two point lights that lie inside its
# accept region, so t = tmax up to rounding for every shadow ray from the floor; two lights: the walk's pair instance (NR = 2)
LIGHTS_IN_PLANE = ((2.0, 12.0, 0.0), (1.0, 12.0, -1.0))


def write_lights_in_plane_scene(path):
    from triangle_shadow_check import OCCLUDER, moved, write_floor_scene
    write_floor_scene(path, [moved(OCCLUDER, LIGHTS_IN_PLANE[0][1] - OCCLUDER[0][1])], light=None)
    with open(path, "a") as f:
        for x, y, z in LIGHTS_IN_PLANE:
            f.write("point_light 90 90 90 %g %g %g\n" % (x, y, z))
    return path
