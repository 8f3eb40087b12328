"""Cases for the sphere tree (include/skr.h skr_scene_set_sphere_tree), shared by test_sphere_tree_cpu.py and
test_sphere_tree_gpu.py: random sphere scenes with the features a tree can get wrong, border rays for a built tree, and the device's
two tests — the candidate test of device_math.h sphere_bracket and the entry test of shade_common.h sphere_entry_touched — restated in
numpy binary32 with the device's operation order (no contraction: every product and sum is rounded, as -ffp-contract=off compiles them)."""
import numpy as np

f32 = np.float32
RANDOM_KINDS = ("overlapping", "nested", "coincident", "radii_6_decades", "camera_inside", "zero", "one")


def _materials(n, rng):
    """per-sphere materials that tell the spheres apart: a wrong sphere id is a wrong colour"""
    m = np.zeros((n, 10), f32)
    i = np.arange(n)
    col = np.stack([(i * 97 % 251) / 250.0, ((i * 57 + 90) % 241) / 240.0, ((i * 151 + 30) % 239) / 238.0], axis=1)
    m[:, 0:3] = 0.3 * col
    m[:, 3:6] = col
    m[:, 6:9] = 0.2
    m[:, 9] = np.array([1, 2, 7, 16, 33])[i % 5]
    return m


def random_scene(kind, seed=0):
    """dict(spheres [n, 14], lights [l, 6], camera [9], background, ambient) for Scene.from_arrays / the .scn writer below"""
    rng = np.random.default_rng(1000 + seed)
    cam = np.array([0, 0, -10, 0, 0, 1, 0, 1, 0], f32)
    if kind == "zero":
        geo = np.zeros((0, 4))
    elif kind == "one":
        geo = np.array([[0.3, -0.2, 1.0, 1.5]])
    elif kind == "overlapping":
        n = 300
        geo = np.concatenate([rng.uniform(-6, 6, (n, 2)), rng.uniform(-1, 3, (n, 1)), rng.uniform(0.4, 1.4, (n, 1))], axis=1)
    elif kind == "nested":
        c = np.concatenate([rng.uniform(-5, 5, (40, 2)), rng.uniform(0, 2, (40, 1))], axis=1)
        geo = np.concatenate([np.concatenate([c, np.full((40, 1), r)], axis=1) for r in (1.2, 0.8, 0.5, 0.1)])  # the outer shells first
        geo = geo[rng.permutation(len(geo))]
    elif kind == "coincident":
        c = np.concatenate([rng.uniform(-5, 5, (60, 2)), rng.uniform(0, 2, (60, 1)), rng.uniform(0.3, 0.9, (60, 1))], axis=1)
        geo = np.concatenate([c, c, c[:20]])  # every sphere twice, some three times, far apart in the file
    elif kind == "radii_6_decades":
        n = 400
        geo = np.concatenate([rng.uniform(-6, 6, (n, 2)), rng.uniform(-1, 3, (n, 1)), 10.0 ** rng.uniform(-4, 2, (n, 1))], axis=1)
        geo[:, 2] += geo[:, 3]  # (keep the big ones behind the small ones)
    elif kind == "camera_inside":
        n = 120
        geo = np.concatenate([rng.uniform(-4, 4, (n, 2)), rng.uniform(-2, 4, (n, 1)), rng.uniform(0.2, 0.8, (n, 1))], axis=1)
        geo = np.concatenate([[[0.5, 0.2, -9.0, 3.0], [0.0, 0.0, 0.0, 40.0]], geo])  # the camera inside a small and inside a huge sphere
    else:
        raise ValueError(kind)
    n = len(geo)
    spheres = np.zeros((n, 14), f32)
    spheres[:, 0:4] = geo
    spheres[:, 4:14] = _materials(n, rng)
    lights = np.array([[0.9, 0.8, 0.7, 6, 9, -12], [0.5, 0.6, 0.7, -7, 8, -9]], f32)  # colour, position (the .scn order); from_arrays takes position colour
    return dict(spheres=spheres, lights=lights, camera=cam, background=(0.05, 0.1, 0.15), ambient=(0.25, 0.25, 0.25))


def write_case_scene(path, case):
    """the case as a .scn file (what the oracle reads); returns the path"""
    cam = case["camera"]
    lines = ["camera %s 30" % " ".join("%.9g" % v for v in cam), "background %g %g %g" % tuple(case["background"]), "ambient_light %g %g %g" % tuple(case["ambient"])]
    for s in case["spheres"]:
        lines.append("material %s 0 0 0 1" % " ".join("%.9g" % v for v in s[4:14]))
        lines.append("sphere %s" % " ".join("%.9g" % v for v in s[0:4]))
    for l in case["lights"]:
        lines.append("point_light %s" % " ".join("%.9g" % v for v in l))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)


# ---- the device's arithmetic in numpy binary32 ----
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(x, y):
    return np.stack([x[..., 1] * y[..., 2] - y[..., 1] * x[..., 2], x[..., 2] * y[..., 0] - y[..., 2] * x[..., 0], x[..., 0] * y[..., 1] - y[..., 0] * x[..., 1]], axis=-1)


def is_candidate(o, d, sph):
    """device_math.h sphere_bracket's candidate test: binary32 D = b b - 4a c >= 0 and b < 0 (utils.h:113-121's operation order)"""
    assert o.dtype == f32 and d.dtype == f32 and sph.dtype == f32
    with np.errstate(all="ignore"):
        e = o - sph[..., 0:3]
        b = f32(2) * dot3(d, e)
        c = dot3(e, e) - sph[..., 3]
        a = dot3(d, d)
        D = b * b - (f32(4) * a) * c
        return (D >= 0) & (b < 0)


def entry_touched(o, d, ent, shrink=1.0):
    """shade_common.h sphere_entry_touched for entries [.., 5] = {C, R^2, kappa}; shrink: R^2 scaled (the test of the test)"""
    assert o.dtype == f32 and d.dtype == f32 and ent.dtype == f32
    with np.errstate(all="ignore"):
        e = ent[..., 0:3] - o
        cr = cross3(e, d)
        dd = dot3(d, d)
        R2 = ent[..., 3] * f32(shrink) if shrink != 1.0 else ent[..., 3]
        return ~(dot3(cr, cr) > (R2 + ent[..., 4] * dot3(e, e)) * dd)


def ancestors(tree):
    """per chunk the node indices above it, root first, -1 padded [n_chunks, depth]; the always-tested chunks have none"""
    links = tree["node_links"]
    nn, nc = len(links), len(tree["chunk_links"])
    parent = np.full(nn, -1, np.int64)
    stack = []
    for i in range(nn):
        while stack and links[stack[-1], 0] <= i:
            stack.pop()
        if stack:
            parent[i] = stack[-1]
        stack.append(i)
    chains = [[] for _ in range(nc)]
    for i in range(nn):
        if links[i, 2] > 0:
            chain = []
            k = i
            while k >= 0:
                chain.append(k)
                k = parent[k]
            for c in range(links[i, 1], links[i, 1] + links[i, 2]):
                chains[c] = chain[::-1]
    depth = max([len(c) for c in chains] + [1])
    out = np.full((nc, depth), -1, np.int64)
    for c, chain in enumerate(chains):
        out[c, :len(chain)] = chain
    return out, parent


def border_rays(tree, n_rays, seed):
    """(o, d, target device sphere) float32: rays tangent and nearly tangent to member spheres — the target's radius scaled by 1 + eps,
    eps from 0 to +-1e-2 —, origins spread through the ball and on sphere surfaces, |d| from 2^-20 to 2^20"""
    rng = np.random.default_rng(seed)
    sph = tree["spheres"].astype(np.float64)
    n = len(sph)
    ball = tree["ball"].astype(np.float64)
    tgt = rng.integers(0, n, n_rays)
    # origins: a third anywhere in the ball, a third near the scene (the ball's inner quarter), a third on sphere surfaces
    u = rng.normal(size=(n_rays, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = ball[3] * 0.999 * rng.uniform(0, 1, n_rays) ** (1 / 3)
    rad[n_rays // 3: 2 * n_rays // 3] *= 0.25
    o = ball[0:3] + u * rad[:, None]
    k = np.arange(n_rays) >= 2 * n_rays // 3
    src = rng.integers(0, n, n_rays)
    on = sph[src, 0:3] + u * (np.sqrt(sph[src, 3]) * (1 + rng.choice([0, 1e-6, -1e-6, 1e-5], n_rays)))[:, None]
    inside = np.linalg.norm(on - ball[0:3], axis=1) < ball[3] * 0.999
    o[k & inside] = on[k & inside]
    # directions: tangent to the target scaled by 1 + eps, turned about a random axis
    c, r = sph[tgt, 0:3], np.sqrt(sph[tgt, 3])
    eps = rng.choice([0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3, 1e-2, -1e-2], n_rays)
    v = c - o
    L = np.linalg.norm(v, axis=1)
    s = np.clip(r * (1 + eps) / np.maximum(L, 1e-300), 0, 1)
    th = np.arcsin(s)
    w = np.cross(v, rng.normal(size=(n_rays, 3)))
    w /= np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-300)
    vh = v / np.maximum(L, 1e-300)[:, None]
    d = np.cos(th)[:, None] * vh + np.sin(th)[:, None] * w
    free = L <= r * (1 + eps)  # the origin lies inside the target: any direction
    d[free] = u[::-1][free]
    d *= (2.0 ** rng.uniform(-20, 20, n_rays))[:, None]
    return o.astype(f32), d.astype(f32), tgt


def culled_candidates(tree, o, d, tgt, shrink=1.0):
    """the (ray, target sphere) pairs that are candidates and that the target's chunk sphere or a node above it culls"""
    first, count = tree["chunk_links"][:, 1], tree["chunk_links"][:, 2]
    chunk_of = np.repeat(np.arange(len(first)), count)
    assert np.array_equal(np.repeat(first, count) + np.concatenate([np.arange(c) for c in count] or [np.zeros(0, int)]), np.arange(len(tree["spheres"])))
    ch = chunk_of[tgt]
    cand = is_candidate(o, d, tree["spheres"][tgt])
    culled = ~entry_touched(o, d, tree["chunk_spheres"][ch], shrink)
    anc, _ = ancestors(tree)
    for k in range(anc.shape[1]):
        node = anc[ch, k]
        has = node >= 0
        if has.any():
            t = entry_touched(o[has], d[has], tree["node_spheres"][node[has]], shrink)
            culled[np.nonzero(has)[0][~t]] = True
    return cand, cand & culled
