"""The cases of tests/light_mode_cases.py on the host (no GPU): before a GPU sees one, the CPU checkers (tests/soft_light_checker.c,
tests/lens_checker.c) are shown to be evidence on these scenes, and every family is shown to reach what it names.  Everything here is
measured on the checkers alone.

1. the anchor: with every radius 0, every cone 180 / 180, no lens and no triangle shadows a random case is a scene of point lights, and
   both checkers must give the frozen oracle's frame of it (spot_light lines written as point_light lines), words, bytes and all five
   counts;
2. conditions on the 64 random cases: what the campaign's scenes have to contain;
3. the reach of each edge family, from checker frames."""
import numpy as np
import pytest

import skele_raytracer_amd as skr
from oracle import pyoracle
import light_mode_cases as lm
from lens_check import build as build_lens_checker
from soft_light_check import build as build_soft_checker

f32 = np.float32


@pytest.fixture(scope="session")
def soft(tmp_path_factory):
    return build_soft_checker(str(tmp_path_factory.mktemp("lightmodes_soft")))


@pytest.fixture(scope="session")
def lens(tmp_path_factory):
    return build_lens_checker(str(tmp_path_factory.mktemp("lightmodes_lens")))


@pytest.fixture(scope="session")
def folder(tmp_path_factory):
    return str(tmp_path_factory.mktemp("lightmodes_scenes"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing_pixels(a, b):
    return int((bits(a) != bits(b)).any(-1).sum())


def library_rows(case, wide=False):
    """(rows, cones) of the case's spot lights as the library holds and derives them; wide: every cone 180 / 180"""
    sc = skr.parse_scene(case.scene, **case.flags)
    rows = sc.spot_lights.copy()
    if wide and len(rows):
        rows[:, 9:11] = 180.0
        sc.set_spot_lights(rows)
    return rows, sc.spot_cones


def frame(soft, lens, case, *, wide=False, **over):
    rows, cones = library_rows(case, wide)
    return lm.checker_frame(soft, lens, case, rows, cones, **over)


def write_variant(case, text, tag):
    path = "%s.%s.scn" % (case.scene[:-4], tag)
    with open(path, "w") as f:
        f.write(text)
    return path


# ---- 1. the anchor ----
@pytest.mark.parametrize("fi", lm.RANDOM, ids=lm.case_id)
def test_checkers_are_the_oracle_on_every_random_scene(soft, lens, folder, fi):
    case = lm.build(*fi, folder)
    text = open(case.scene).read()
    as_points = []
    for ln in text.split("\n"):
        t = ln.split()
        as_points.append("point_light " + " ".join(t[1:7]) if t[:1] == ["spot_light"] else ln)
    points_scn = write_variant(case, "\n".join(as_points), "points")
    kw = dict(case.kw)
    passes = kw.pop("progressive", 1)
    strict = case.flags["strict"]
    if passes > 1:
        o_rgb, o_f, o_st, _ = pyoracle.render_progressive(points_scn, case.w, case.h, passes, strict=strict, **kw)
    else:
        o_rgb, o_f, o_st = pyoracle.render(points_scn, case.w, case.h, want_float=True, strict=strict, **kw)
    plain = case._replace(flags=dict(case.flags, triangle_shadows=False), lens=None)
    zero = np.zeros_like(case.radii)
    for name, got in (("soft checker", frame(soft, lens, plain, wide=True, radii=zero)), ("lens checker, A = 0", frame(soft, lens, plain, wide=True, radii=zero, aperture=0.0))):
        assert np.array_equal(bits(got[1]), bits(o_f)), name
        assert np.array_equal(got[0], o_rgb), name
        assert got[2].tolist() == o_st.tolist(), name  # all five


# ---- 2. conditions on the random cases ----
@pytest.fixture(scope="module")
def random_cases(folder):
    return [lm.build(*fi, folder) for fi in lm.RANDOM]


def test_a_case_is_its_family_and_index_alone(random_cases, tmp_path):
    for case in random_cases[:8]:
        again = lm.build(case.family, case.index, str(tmp_path))
        assert open(again.scene).read() == open(case.scene).read()
        assert again.flags == case.flags and np.array_equal(again.radii, case.radii)
        assert again.lens == case.lens and (again.w, again.h, again.kw, again.sample) == (case.w, case.h, case.kw, case.sample)
        assert np.array_equal(bits(again.rays), bits(case.rays)) and np.array_equal(again.keys, case.keys)
    for case in random_cases:
        assert case.rays.shape == (lm.N_RAYS, 8) and case.sample > 0
        assert not np.array_equal(case.keys, np.arange(lm.N_RAYS))
        assert np.isfinite(case.rays[:, 3]).any() and np.isinf(case.rays[:, 3]).any()
        assert 8 <= case.w <= 96 and 8 <= case.h <= 64
        assert len(case.radii) == case.meta["n_point"] + case.meta["n_spot"] >= 1 and (case.meta["n_spot"] > 0 or (case.radii > 0).any())
        if "gillum" in case.kw:
            assert case.kw["gillum"] ** (case.kw["depth"] - 1) * case.w * case.h <= 2e5 and 2 <= case.kw["depth"] <= 3


def test_the_random_cases_hold_what_the_campaign_is_for(random_cases):
    m = [c.meta for c in random_cases]
    assert len(random_cases) == 64
    assert sum(x["tshadow_in_force"] for x in m) >= 8
    assert sum(x["n_spheres"] > lm.MAX_MASK_SPHERES for x in m) >= 8 and sum(x["n_spheres"] <= lm.MAX_MASK_SPHERES for x in m) >= 8
    assert sum(x["n_directional"] > 0 for x in m) >= 4
    assert sum(c.lens is not None for c in random_cases) >= 12
    for mode in lm.MODES:
        assert sum(x["mode"] == mode for x in m) >= 8, mode
    assert 16 <= sum(x["posed"] for x in m) <= 48  # about half


def test_random_frames_are_finite_some_light_is_outside_and_the_radii_show(soft, lens, random_cases):
    """The shadow-ray comparison is made with --shadow on in both frames, whatever the case's own switch: without it neither frame
    casts one, and the count could not show that a light is outside its cone."""
    with_spot = fewer = with_radius = moved = 0
    for case in random_cases:
        _, f, st = frame(soft, lens, case)
        assert np.isfinite(f).all(), case.name
        if case.meta["n_spot"] > 0:
            with_spot += 1
            narrow = st if case.kw["shadow"] else frame(soft, lens, case, shadow=True)[2]
            wide = frame(soft, lens, case, wide=True, shadow=True)[2]
            assert int(narrow[2]) <= int(wide[2]), case.name
            fewer += int(narrow[2]) < int(wide[2])
        if (case.radii > 0).any():
            with_radius += 1
            moved += differing_pixels(f, frame(soft, lens, case, radii=np.zeros_like(case.radii))[1]) > 0
    print("spot cases %d, with a light outside %d; radius cases %d, differing %d" % (with_spot, fewer, with_radius, moved))
    assert 2 * fewer >= with_spot > 0
    assert 4 * moved >= 3 * with_radius > 0


# ---- 3. the reach of each edge family ----
def edge_cases(folder, family):
    return [lm.build(*fi, folder) for fi in lm.EDGE if fi[0] == family]


def test_no_edge_case_holds_a_nan_outside_the_nan_list(soft, lens, folder):
    assert set(lm.NAN) <= {lm.case_id(fi) for fi in lm.EDGE}
    for fi in lm.EDGE:
        case = lm.build(*fi, folder)
        assert case.w <= 64 and case.h <= 48
        if case.name not in lm.NAN:
            assert np.isfinite(frame(soft, lens, case)[1]).all(), case.name


def test_every_family_has_one_lens_case_at_jsample_2(folder):
    for family in lm.COUNTS:
        lensed = [c for c in edge_cases(folder, family) if c.lens is not None]
        assert len(lensed) == 1 and lensed[0].kw.get("jsample") == 2, family


DIRECT = dict(shadow=False, jsample=0)  # depth-1 frames without shadows: a pixel's value says which lights reach it


def test_pair_shapes_has_all_four_shapes_of_the_pair(soft, lens, folder):
    case = lm.build("pair_shapes", 0, folder)
    assert case.meta["what"].startswith("spots_only") and (case.radii == 0).all()
    frames = {}
    for a, b in ((False, False), (True, False), (False, True), (True, True)):
        scn = write_variant(case, lm.pair_text(a, b), "a%db%d" % (a, b))
        frames[a, b] = frame(soft, lens, case._replace(scene=scn, radii=np.zeros(a + b, f32)), **DIRECT)[1]
    none = frames[False, False]
    colours, counts = np.unique(none.reshape(-1, 3), axis=0, return_counts=True)
    floor = (none == colours[counts.argmax()]).all(-1)  # the ambient floor: the two small spheres and the sky apart
    assert floor.sum() > 0.5 * floor.size  # (the ground of radius 40 ends at a horizon inside the frame)
    in_a, in_b = (bits(frames[True, False]) != bits(none)).any(-1), (bits(frames[False, True]) != bits(none)).any(-1)
    assert np.array_equal((bits(frames[True, True]) != bits(none)).any(-1) & floor, (in_a | in_b) & floor)
    for name, cls in (("both", in_a & in_b), ("a alone", in_a & ~in_b), ("b alone", ~in_a & in_b), ("neither", ~in_a & ~in_b)):
        share = (cls & floor).sum() / floor.sum()
        print("pair_shapes %s: %.1f %% of the floor" % (name, 100 * share))
        assert share >= 0.02, name
    # the cases: both table starts, the four radius patterns, with and without shadows
    cases = edge_cases(folder, "pair_shapes")[:16]
    assert {(c.meta["point"], c.kw["shadow"], tuple(c.radii[-2:] > 0)) for c in cases} == {(p, s, r) for p in (False, True) for s in (False, True)
                                                                                         for r in ((False, False), (True, False), (False, True), (True, True))}
    assert all(len(c.radii) == 2 + c.meta["point"] for c in cases)


def test_cone_edges_cross_the_frame(soft, lens, folder):
    """Per pair: pixels inside (the 180 / 180 light's value), outside (the value without the light) and with 0 < f < 1.  A cone with
    angle1 == 0 has c1 == 1: its inside is the axis alone, no area; one with angle2 == 180 has c2 == -1: no outside.  Those two classes
    are asked of the pairs that can have them, the third of the pairs with angle1 < angle2 by at least half a degree: the last pair's
    ring (1e-4 degree) is narrower than any pixel, it is there for its c1 and c2 a few binary32 steps apart."""
    seen = set()
    for case in edge_cases(folder, "cone_edges"):
        pair = case.meta.get("pair")
        if pair is None:
            continue
        seen.add((pair, case.meta["tilted"]))
        spot = frame(soft, lens, case, **DIRECT)[1]
        point = frame(soft, lens, case, wide=True, **DIRECT)[1]
        dark = lm.checker_frame(soft, lens, case, None, None, scene=write_variant(case, case.meta["off_text"], "off"), radii=case.radii[:-1], **DIRECT)[1]
        lit = (bits(point) != bits(dark)).any(-1)
        inside = lit & (bits(spot) == bits(point)).all(-1)
        outside = lit & (bits(spot) == bits(dark)).all(-1)
        between = lit & ~inside & ~outside
        assert ((spot[between] >= dark[between]) & (spot[between] <= point[between])).all(), case.name
        print("%s %s: inside %d, outside %d, between %d" % (case.name, case.meta["what"], inside.sum(), outside.sum(), between.sum()))
        a1, a2 = pair
        if pair == (0, 0):
            assert outside.sum() >= lit.sum() - 1  # all but, at most, the pixel under the light
        elif pair == (180, 180):
            assert inside.sum() == lit.sum() >= 16
        else:
            assert a1 == 0 or inside.sum() >= 16, case.name
            assert a2 == 180 or outside.sum() >= 16, case.name
            assert not a2 - a1 >= 0.5 or between.sum() >= 16, case.name
    assert seen == {(p, t) for p in lm.CONE_PAIRS for t in (False, True)}
    lengths = {round(float(np.log10(np.linalg.norm(library_rows(c)[0][0, 6:9])))) for c in edge_cases(folder, "cone_edges") if "pair" in c.meta}
    assert lengths == {-3, 3}


def test_the_edge_c_equals_c1_is_reached(soft, folder):
    """the on-axis query rays of the straight-down (0, 0) cone: c == 1 == c1 exactly, inside by the rule's c >= c1; the cone has no other
    inside, so a c > c1 there would leave these rays dark and without a shadow ray"""
    case = lm.build("cone_edges", lm.CONE_PAIRS.index((0, 0)), folder)
    assert not case.meta["tilted"]
    rows, cones = library_rows(case)
    assert cones[0, 3] == f32(1) and cones[0, 4] == f32(1) and cones[0, 0:3].tolist() == [0.0, -1.0, 0.0]
    n = len(lm.AXIS_RAYS)
    kw = lm.query_options(case)
    got, st = soft.shade(case.scene, case.rays[:n], spots=rows, cones=cones, radii=case.radii, keys=case.keys[:n], sample=case.sample, **kw)
    dark, dst = soft.shade(write_variant(case, case.meta["off_text"], "off"), case.rays[:n], keys=case.keys[:n], sample=case.sample, **kw)
    assert (got > dark).all() and int(st[2]) == n and int(dst[2]) == 0


@pytest.mark.parametrize("family", ["ball_meets_geometry", "sampled_far_end"])
def test_the_radii_and_the_triangle_shadows_show(soft, lens, folder, family):
    for case in edge_cases(folder, family):
        f = frame(soft, lens, case)[1]
        hard = frame(soft, lens, case, radii=np.zeros_like(case.radii))[1]
        n = differing_pixels(f, hard)
        print("%s %s: %d pixels differ from the radius-0 frame" % (case.name, case.meta["what"], n))
        assert n >= 16, case.name
        if family == "sampled_far_end":
            assert case.flags["triangle_shadows"] and case.kw["shade_triangles"] and case.kw["shadow"]
            n = differing_pixels(f, frame(soft, lens, case._replace(flags=dict(case.flags, triangle_shadows=False)))[1])
            print("%s: %d pixels differ from the frame without triangle shadows" % (case.name, n))
            assert n >= 16, case.name


def test_sampled_far_end_shadows_some_samples_and_not_others(soft, lens, folder):
    """the triangle behind the light's centre: with radius 0 it shadows nothing (the frame with triangle shadows is the frame without),
    with the radius it does"""
    case = next(c for c in edge_cases(folder, "sampled_far_end") if c.meta["what"] == "triangle_behind_the_centre_inside_the_ball")
    zero = np.zeros_like(case.radii)
    off = case._replace(flags=dict(case.flags, triangle_shadows=False))
    assert differing_pixels(frame(soft, lens, case, radii=zero)[1], frame(soft, lens, off, radii=zero)[1]) == 0
    assert differing_pixels(frame(soft, lens, case)[1], frame(soft, lens, off)[1]) >= 16
    mesh = next(c for c in edge_cases(folder, "sampled_far_end") if c.meta["what"] == "random_mesh")
    sc = skr.parse_scene(mesh.scene, **mesh.flags)
    assert sc.info.n_triangles > 64 and len(sc.trace_culling(0)[4]) > 1  # a tree over more than one chunk


def mask_cell(v, n=32):
    """csrc/shadow_cells.h: the cell (face, i, j) of direction v in a light's table"""
    v = np.asarray(v, np.float64)
    axis = int(np.argmax(np.abs(v)))
    i, j = (min(n - 1, max(0, int((v[k] / abs(v[axis]) + 1) * 0.5 * n))) for k in range(3) if k != axis)
    return 2 * axis + int(v[axis] < 0), i, j


def test_masks_exist_and_say_something_where_a_case_needs_them(folder):
    for case in edge_cases(folder, "ball_meets_geometry") + edge_cases(folder, "pair_shapes"):
        sc = skr.parse_scene(case.scene, **case.flags)
        masks = sc.shadow_masks()[0]
        assert masks.shape[0] == len(case.radii), case.name  # a table per light
        if case.family == "pair_shapes" or "masks" in case.meta["what"]:
            every = (1 << sc.info.n_spheres) - 1
            assert ((masks & every) != every).mean() > 0.5, case.name  # most cells leave some sphere out: using, uniting or dropping them differs
    mixed = next(c for c in edge_cases(folder, "ball_meets_geometry") if c.meta["what"] == "soft_and_hard_pairs_with_masks")
    assert (mixed.radii > 0).tolist() == [True, False, False, False]  # the pairs (soft, hard) and (hard, hard)
    # pair_shapes: where the high sphere's shadow from A falls, A's cell names the sphere and B's does not, and the other way round:
    # a walk with one light's mask for both rays misses the occluder there
    case = lm.build("pair_shapes", 2, folder)
    masks = skr.parse_scene(case.scene, **case.flags).shadow_masks()[0]
    a, b, s = np.array(lm.PAIR_A[3:6]), np.array(lm.PAIR_B[3:6]), np.array(lm.PAIR_SPHERES[2][:3])
    bit = 1 << 3  # the ground, the two small spheres, then the high one
    for own, other, lp, lq in ((0, 1, a, b), (1, 0, b, a)):
        p = lp + (s - lp) * (lp[1] / (lp[1] - s[1]))  # the centre of the shadow on y = 0
        assert int(masks[own][mask_cell(lp - p)]) & bit and not int(masks[other][mask_cell(lq - p)]) & bit


def test_the_far_light_shades_through_the_fallback_range(soft, lens, folder):
    for case in edge_cases(folder, "far_light"):
        f = frame(soft, lens, case)[1]
        assert np.isfinite(f).all(), case.name
        off = frame(soft, lens, case._replace(scene=write_variant(case, case.meta["off_text"], "off"), radii=np.array(case.meta["off_radii"], f32)))[1]  # the scene without the far light
        n = differing_pixels(f, off)
        print("%s %s: the far light changes %d pixels" % (case.name, case.meta["what"], n))
        assert n >= 16, case.name
        far = np.linalg.norm(np.array(lm.FAR_POS, np.float64))
        assert far * far > 2.0 ** 98 and (far - 2.1e14) ** 2 > 2.0 ** 98  # every sample of the ball too
