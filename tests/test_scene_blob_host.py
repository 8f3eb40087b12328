"""The scene blob a renderer uploads (csrc/scene_pack.h): where its sections lie and what they hold — no GPU.

skr_scene_pack (internal) packs a scene on the host exactly as skr_renderer_create does and reports the blob's rows and, per section
of scene_pack.h's table, its first row and its rows.  Every rule of the layout is stated here once: the order and the tiling of the
sections, the 16 rows of padding, each section's words against the scene's own getters, the shadow surface headers in the kd rows,
the GI surface patches behind the grids' rows, and pow_steps.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skele_raytracer_amd as skr
from conftest import ROOT, scene_path

SECTIONS = "geom amb kd ks lights tris chunks tri_mats fog spot radii smask ssurf gi trace st_rows st_chunks st_nodes pad".split()
PAD_ROWS = 16
ALWAYS = SECTIONS[:11] + ["pad"]  # packed for every scene, with 0 rows where the scene has nothing of the kind
CELLS = open(os.path.join(ROOT, "skele_raytracer_amd", "csrc", "shadow_cells.h")).read()
LIMIT = {k: int(re.search(r"#define\s+%s\s+(\d+)" % k, CELLS).group(1)) for k in ("SKR_SHADOW_MAX_SPHERES", "SKR_GI_MAX_SPHERES")}
CAMERA = [0, 2, -10, 0, -.1, .9, 0, 1, 0]


class Blob:
    def __init__(self, scene):
        fn = skr.lib().skr_scene_pack
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        n = fn(scene.h, None, None, None, 0, None, None)
        assert n >= PAD_ROWS, n
        first, count = np.zeros(len(SECTIONS), np.int64), np.zeros(len(SECTIONS), np.int64)
        names, scalars = (C.c_char_p * len(SECTIONS))(), np.zeros(2, np.int64)
        self.words = np.full((n, 4), 0xDEADBEEF, np.uint32)
        assert fn(scene.h, first.ctypes.data, count.ctypes.data, self.words.ctypes.data, n, names, scalars.ctypes.data) == n
        assert [s.decode() for s in names] == SECTIONS  # the table of scene_pack.h
        self.first, self.count = dict(zip(SECTIONS, first.tolist())), dict(zip(SECTIONS, count.tolist()))
        self.pow_steps, self.gi_surface_word = int(scalars[0]), int(scalars[1])

    def sec(self, name, dtype=np.uint32):
        """the words of a section, flat"""
        return self.words[self.first[name]:self.first[name] + self.count[name]].reshape(-1).view(dtype)


def arrays_scene(n_spheres, n_triangles=0, n_lights=2, powers=(32, 8), **kw):
    """A ground sphere and n_spheres - 1 small ones over it, n_triangles small triangles, n_lights point lights: fixed places."""
    s = np.zeros((n_spheres, 14), np.float32)
    for i in range(n_spheres):
        x, z, r = -4.5 + 1.1 * (i % 8), 1.0 + 1.3 * (i // 8), 0.3 + 0.05 * (i % 3)
        s[i, :4] = (0, -40, 0, 40) if i == 0 else (x, r, z, r)
        s[i, 4:13] = [.5, .4, .1 * (1 + i % 9), .1 * (9 - i % 9), .6, .5, .3, .3, .2]
        s[i, 13] = powers[i % len(powers)]
    t = np.zeros((n_triangles, 9), np.float32)
    for i in range(n_triangles):
        p = np.array([-3 + 0.7 * (i % 9), 0.2 + 0.1 * (i % 4), 2 + 0.6 * (i // 9)], np.float32)
        t[i] = np.concatenate([p, p + np.float32([.5, 0, .1]), p + np.float32([.2, .6, 0])])
    l = np.float32([[2.0 - 3.0 * k, 9, -1.0 - k, .8, .1 * (8 - k), .7] for k in range(n_lights)]).reshape(-1, 6)
    return skr.Scene.from_arrays(s, t, l, CAMERA, background=(.2, .3, .5), ambient=(.3, .3, .3), **kw)


def spheres2_lit():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    sc.set_spot_lights([[1.0, 0.9, 0.8, 0.5, 3.0, 1.5, 0.1, -1.0, -0.2, 20.0, 35.0], [0.3, 0.4, 2.0, -2.0, 1.0, -3.0, 1.0, 0.5, 1.0, 0.0, 90.0]])
    sc.set_light_radii(0.2)
    sc.set_fog([[0.5, 1.0, 2.0, 3.0, 0.9, 0.8, 0.7, 0.05, 0.02]])
    return sc


def spheres2_tree():
    sc = skr.parse_scene(scene_path("spheres2.scn"))
    sc.set_sphere_tree(True)
    return sc


SCENES = {
    "test.scn": lambda: skr.parse_scene(scene_path("test.scn")),
    "spheres2.scn": lambda: skr.parse_scene(scene_path("spheres2.scn")),
    "dragon.scn": lambda: skr.parse_scene(scene_path("dragon.scn")),
    "spheres2 + sphere tree": spheres2_tree,
    "spheres2 + spots, radii, fog": spheres2_lit,
    "nothing at all": lambda: arrays_scene(0, 0, 0),
    "no spheres": lambda: arrays_scene(0, 5, 2),
    "no triangles, no lights": lambda: arrays_scene(3, 0, 0),
    "1 sphere": lambda: arrays_scene(1),
    "16 spheres": lambda: arrays_scene(16, sphere_tree=True),
    "17 spheres": lambda: arrays_scene(17, 3, triangle_materials=np.float32([[.1] * 9 + [p] for p in (1024, 1025, 2.5)])),
    "no integer exponent": lambda: arrays_scene(4, powers=(2.5, 0.5, 1025)),
}
for _n in sorted({LIMIT["SKR_SHADOW_MAX_SPHERES"] + 1, LIMIT["SKR_GI_MAX_SPHERES"] + 1}):
    SCENES["%d spheres: past a mask limit" % _n] = lambda n=_n: arrays_scene(n, n_lights=1, sphere_tree=True)


@pytest.fixture(scope="module", params=list(SCENES), ids=lambda k: k.replace(" ", "_"))
def packed(request):
    scene = SCENES[request.param]()
    return scene, Blob(scene)


def shadow_surface(scene):
    fn = skr.lib().skr_scene_get_shadow_surface
    fn.argtypes = [C.c_void_p] * 5
    npairs, stride = C.c_int32(), C.c_int32()
    fn(scene.h, C.byref(npairs), C.byref(stride), None, None)
    head, table = np.zeros(scene.info.n_spheres if stride.value else 0, np.uint32), np.zeros(npairs.value * stride.value, np.uint32)
    fn(scene.h, None, None, head.ctypes.data, table.ctypes.data)
    return head, table


def gi_surface(scene):
    fn = skr.lib().skr_scene_get_gi_surface
    fn.argtypes = [C.c_void_p] * 5
    nw, hw, fr = C.c_int32(), C.c_int32(), C.c_int32()
    fn(scene.h, C.byref(nw), C.byref(hw), C.byref(fr), None)
    table = np.zeros(nw.value, np.uint32)
    fn(scene.h, None, None, None, table.ctypes.data)
    return table, hw.value, fr.value


def padded(words, dtype=np.uint32):
    """flat 32-bit words as the packer lays them: whole rows, zeros behind the last word"""
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint32)
    return np.concatenate([w, np.zeros(-len(w) % 4, np.uint32)])


def test_sections_tile_the_blob_in_table_order(packed):
    """(a), (b): the present sections follow each other in the table's order without a gap or an overlap, from row 0 to the last;
    the last is the padding: exactly 16 rows of zeros."""
    _, b = packed
    at = 0
    for name in SECTIONS:
        assert b.count[name] >= 0
        if b.count[name] or name in ALWAYS:
            assert b.first[name] == at, name
        at += b.count[name]
    assert at == len(b.words)
    assert b.count["pad"] == PAD_ROWS and not b.sec("pad").any()
    assert not (b.words == 0xDEADBEEF).all(axis=1).any()  # (every row was written)


def test_sphere_and_light_rows(packed):
    """(c), (d): geom = centre and the binary32 product r * r; kd, ks, lights, spot cones, radii and fog rows as the getters give them;
    the .w of a kd row is the sphere's shadow-surface header where the scene has such patches, and what sph_kd held (0) where not."""
    scene, b = packed
    info = scene.info
    s, _, l = scene.arrays()
    n = info.n_spheres
    for name in ("geom", "amb", "kd", "ks"):
        assert b.count[name] == n
    geom = b.sec("geom", np.float32).reshape(n, 4)
    assert np.array_equal(geom[:, :3].view(np.uint32), s[:, :3].view(np.uint32))
    assert np.array_equal(geom[:, 3].view(np.uint32), (s[:, 3] * s[:, 3]).astype(np.float32).view(np.uint32))
    amb = b.sec("amb", np.float32).reshape(n, 4)
    assert np.array_equal(amb[:, :3], np.float32(list(info.ambient)) * s[:, 4:7]) and np.array_equal(amb[:, 3].view(np.uint32), s[:, 13].view(np.uint32))
    kd, ks = b.sec("kd", np.float32).reshape(n, 4), b.sec("ks", np.float32).reshape(n, 4)
    assert np.array_equal(kd[:, :3].view(np.uint32), s[:, 7:10].view(np.uint32))
    assert np.array_equal(ks[:, :3].view(np.uint32), s[:, 10:13].view(np.uint32))  # (.w: the index of refraction, which has no getter)
    head, table = shadow_surface(scene)
    assert b.count["ssurf"] == (len(table) + 3) // 4
    if len(table):
        assert len(head) == n and np.array_equal(kd[:, 3].view(np.uint32), head)
    else:
        assert not kd[:, 3].view(np.uint32).any()
    assert np.array_equal(b.sec("ssurf"), padded(table))
    # lights: point lights, then the spot lights as point-light rows {position} {colour}
    spots, cones, radii, fog = scene.spot_lights, scene.spot_cones, scene.light_radii, scene.fog
    want = np.zeros((info.n_point_lights + len(spots), 2, 4), np.float32)
    want[:info.n_point_lights, :, :3] = l.reshape(-1, 2, 3)
    want[info.n_point_lights:, 0, :3], want[info.n_point_lights:, 1, :3] = spots[:, 3:6], spots[:, 0:3]
    assert info.n_directional_lights == 0 and np.array_equal(b.sec("lights"), padded(want))
    want = np.zeros((len(spots), 2, 4), np.float32)
    want[:, 0, :], want[:, 1, 0] = cones[:, :4], cones[:, 4]
    assert np.array_equal(b.sec("spot"), padded(want))
    assert len(radii) == info.n_point_lights + len(spots) and np.array_equal(b.sec("radii"), padded(radii))
    want = np.zeros((len(fog), 2, 4), np.float32)  # [radius absorption scattering 0] [albedo 0]
    want[:, 0, :3], want[:, 1, :3] = fog[:, [3, 8, 7]], fog[:, 4:7]
    assert np.array_equal(b.sec("fog"), padded(want))


def test_mask_sections(packed):
    """(c): the shadow masks and the GI table as their getters give them; the GI surface patches' words start right behind the grids'
    rows of masks, and gi_surface_word names their headers."""
    scene, b = packed
    n = scene.info.n_spheres
    masks, _ = scene.shadow_masks()
    assert (len(masks) > 0) == (0 < n <= LIMIT["SKR_SHADOW_MAX_SPHERES"] and scene.info.n_point_lights + len(scene.spot_lights) > 0)
    assert np.array_equal(b.sec("smask"), padded(masks))
    table, mask_word, wide, dir_cells, _ = scene.gi_masks()
    assert (len(table) > 0) == (0 < n <= LIMIT["SKR_GI_MAX_SPHERES"] and scene.info.n_triangles == 0)
    surf, head_word, first_row = gi_surface(scene)
    gi = b.sec("gi")
    if not len(table):
        assert b.count["gi"] == 0 and b.gi_surface_word == 0 and not len(surf)
        return
    assert wide == (1 if n > 16 else 0)
    assert len(table) % 4 == 0 and np.array_equal(gi[:len(table)], table)
    if not len(surf):
        assert b.gi_surface_word == 0 and len(gi) == len(table)
        return
    patch_word = mask_word + first_row * (6 * dir_cells * dir_cells * (4 if wide else 2) // 4)  # a row of masks: one per direction cell, 16 or 32 bits each
    assert patch_word >= len(table) - 3 and b.gi_surface_word == patch_word + head_word
    assert np.array_equal(gi[patch_word:], padded(np.concatenate([np.zeros(patch_word % 4, np.uint32), surf]))[patch_word % 4:])
    assert not gi[len(table):patch_word].any()


def test_sphere_tree_sections(packed):
    """(c): the sphere tree's rows, chunks {bound} {kappa, smallest file index, first, count} {file indices} and nodes {bound}
    {kappa, skip, first chunk, smallest file index}, each with its pad entry, against skr_scene_get_sphere_tree_data; absent where the
    scene's switch is off or it has no sphere."""
    scene, b = packed
    if not (scene.sphere_tree() and scene.info.n_spheres):
        assert b.count["st_rows"] == b.count["st_chunks"] == b.count["st_nodes"] == 0
        return
    d = scene.sphere_tree_data()
    n, nc, nn = scene.info.n_spheres, len(d["chunk_spheres"]), len(d["node_spheres"])
    assert (b.count["st_rows"], b.count["st_chunks"], b.count["st_nodes"]) == (n, 3 * (nc + 1), 2 * (nn + 1))
    assert np.array_equal(b.sec("st_rows"), d["spheres"].reshape(-1).view(np.uint32))
    ch = b.sec("st_chunks").reshape(nc + 1, 3, 4)[:nc]
    assert np.array_equal(ch[:, 0], d["chunk_spheres"][:, :4].view(np.uint32)) and np.array_equal(ch[:, 1, 0], d["chunk_spheres"][:, 4].view(np.uint32))
    assert np.array_equal(ch[:, 1, 1:].view(np.int32), d["chunk_links"])
    for c in range(nc):
        first, count = d["chunk_links"][c, 1:]
        assert np.array_equal(ch[c, 2].view(np.int32), np.concatenate([d["file_index"][first:first + count], np.zeros(4 - count, np.int32)]))
    nd = b.sec("st_nodes").reshape(nn + 1, 2, 4)[:nn]
    assert np.array_equal(nd[:, 0], d["node_spheres"][:, :4].view(np.uint32)) and np.array_equal(nd[:, 1, 0], d["node_spheres"][:, 4].view(np.uint32))
    links = nd[:, 1, 1:].view(np.int32)
    assert np.array_equal(links[:, 0], d["node_links"][:, 0]) and np.array_equal(links[:, 2], d["node_links"][:, 3])
    leaf = d["node_links"][:, 2] > 0  # (a node without chunks of its own holds a negative first chunk)
    assert np.array_equal(links[leaf, 1], d["node_links"][leaf, 1]) and (links[~leaf, 1] < 0).all()


def test_triangle_sections_and_pow_steps(packed):
    """(e): pow_steps is the bit length of the largest integer exponent in [1, 1024] among the sphere and triangle materials, 1 without
    one.  The triangle sections hold 3 rows per triangle (and a pad triangle), SKR_CULL_LEVELS sets of the chunk tree and the trace tree."""
    scene, b = packed
    info = scene.info
    s, t, _ = scene.arrays()
    levels = int(re.search(r"#define\s+SKR_CULL_LEVELS\s+(\d+)", open(os.path.join(ROOT, "skele_raytracer_amd", "csrc", "tri_chunks.h")).read()).group(1))
    assert b.count["tris"] == 3 * info.n_triangles + 3 and b.count["tri_mats"] == 3 * info.n_triangles  # (tris: + one pad triangle of zeros)
    assert not b.sec("tris")[12 * info.n_triangles:].any()
    assert b.count["chunks"] % levels == 0 and (b.count["trace"] == b.count["chunks"] if info.n_triangles else b.count["trace"] == 0)
    if info.n_triangles:
        _, tris, _, _, _ = scene.culling(0)
        assert np.array_equal(b.sec("tris")[:12 * info.n_triangles], tris.reshape(-1).view(np.uint32))
    powers = np.concatenate([s[:, 13], b.sec("tri_mats", np.float32).reshape(-1, 3, 4)[:, 0, 3]]).astype(np.float64)
    whole = [int(p) for p in powers if 1 <= p <= 1024 and p == int(p)]
    assert b.pow_steps == max([1] + whole).bit_length()
    assert 1 <= b.pow_steps <= 11


def test_known_exponents():
    """(e) on exponents the test chose: 1024 counts (11 bits), 1025 and 2.5 do not."""
    assert Blob(SCENES["17 spheres"]()).pow_steps == 11
    assert Blob(SCENES["no integer exponent"]()).pow_steps == 1
    assert Blob(arrays_scene(2, powers=(127,))).pow_steps == 7 and Blob(arrays_scene(2, powers=(128,))).pow_steps == 8


def test_packing_twice_gives_the_same_bytes(packed):
    """(f)"""
    scene, b = packed
    again = Blob(scene)
    assert np.array_equal(again.words, b.words) and again.first == b.first and again.count == b.count
    assert (again.pow_steps, again.gi_surface_word) == (b.pow_steps, b.gi_surface_word)
