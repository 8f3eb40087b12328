"""Camera poses the five scene files never use, shared by tests/test_camera_poses_cpu.py, tests/test_camera_poses_gpu.py and
tests/golden/make_golden.py.  Plain data and numpy, no GPU.

A pose is a `camera` line (scene.cpp:84-97: position, direction, up, half-angle; the reference keeps the file's magnitudes and forms
right = cross(-direction, up)) put into one of the base scenes, plus the option keywords that belong to it.  The posed scenes are
tests/golden/scenes/pose_<name>.scn.  They repeat their base scene but for one line, so they are not kept in git: write_all() writes
them, called by __graft_entry__.build() and by tests/golden/make_golden.py, which renders them through the reference.

What a pose is meant to reach is stated in `reach` and held by tests/test_camera_poses_cpu.py:
    family "rolled"      up oblique to the direction and not unit, roll, views along the axes
    family "long"        |direction|, |up|, |right| put dmax (api.cpp launch_params) into the culling set `level` names
    family "inside"      the camera inside sphere `sphere`: c < 0 in its camera row, and utils.h:87-110 takes the near root only, so that
                         sphere is never hit from within and the frame shows the others through it
    family "surface"     the camera on a sphere's surface, at a point light, within 1e-3 of a surface, 1e4 units away
    family "interior"    the camera amid a mesh: accepting triangles lie behind it (utils.h:181-213 has no t > 0 test)
    family "degenerate"  right = 0 or direction = 0: NaN may reach the quantiser; these keep their own list
"""
import collections
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")

BOUNDS = (4.0, 32.0, 256.0)  # csrc/tri_chunks.h SKR_CULL_DMAX_LIST

Pose = collections.namedtuple("Pose", "name base camera kw family reach level sphere")


def _p(name, base, camera, family, reach, kw=None, level=None, sphere=None):
    return Pose(name, base, "camera " + camera, dict(kw or {}), family, reach, level, sphere)


def _f32(x):
    return "%.9g" % np.float32(x)


# the point of spheres2.scn's sphere 2 (centre 3 1.5 0, radius 1.25) along (1, 2, -2) / 3, rounded once to binary32 a component
_ON_SURFACE = " ".join(_f32(c + 1.25 * n / 3.0) for c, n in zip((3.0, 1.5, 0.0), (1.0, 2.0, -2.0)))

POSES = [
    # ---- rolled and oblique
    _p("s2_rolled", "spheres2.scn", "0 2 -10 0 -.1 .9 .4 .8 .2 26", "rolled", "up far from perpendicular to the direction, not unit: right has three non-zero components"),
    _p("s2_up3", "spheres2.scn", "0 2 -10 0 -.1 .9 0 3 0 26", "rolled", "|up| = 3"),
    _p("s2_down", "spheres2.scn", "0 12 0 0 -1 .001 0 0 1 26", "rolled", "looking straight down, up along +z"),
    _p("s2_plus_x", "spheres2.scn", "-14 3 0 1 -.1 0 .1 1 .3 26", "rolled", "looking along +x, rolled"),
    _p("test_rolled", "test.scn", "3 -2 -20 .1 .05 1 .4 .8 .2 30", "rolled", "rolled over the wall and the four spheres"),
    _p("test_minus_z", "test.scn", "2 1 40 -.05 0 -1 0 1 .1 30", "rolled", "looking along -z: the wall in front of the spheres"),
    _p("dragon_rolled", "dragon.scn", "0 .6 .02 0 -1 .001 .3 0 .9 23", "rolled", "looking along -y onto the dragon, rolled"),
    # ---- long vectors: one frame per culling set
    _p("dragon_long4", "dragon.scn", "0 .1 .3 0 0 -3 0 3 0 23", "long", "dmax in [4, 32)", level=1),
    _p("dragon_long32", "dragon.scn", "0 .1 .25 0 0 -6 0 6 0 23", "long", "dmax in [32, 256)", level=2),
    _p("dragon_long256", "dragon.scn", "0 .1 .2 0 0 -20 0 20 0 23", "long", "dmax >= 256: every triangle", level=3),
    _p("s2_long", "spheres2.scn", "0 6 -12 0 -3 6.5 0 5 0 26", "long", "|dir| = 7.2, |up| = 5, |right| = 33", level=2),
    _p("s2_dir300", "spheres2.scn", "0 40 -350 0 -33 300 0 1 0 26", "long", "|dir| = 300 from 350 units away (hits need t > 1)", kw=dict(fov=3.0), level=3),
    # ---- inside geometry
    _p("s2_in_ground", "spheres2.scn", "0 -.5 -6 0 .35 1 0 1 0 26", "inside", "just below the ground sphere's surface, looking up through it: c < 0", sphere=0),
    _p("s2_in_small", "spheres2.scn", "0 1.25 .2 0 0 .4 0 .5 0 26", "inside", "inside sphere 1 (radius 1): hits with t around the t > 1 rule", sphere=1),
    _p("s2_at_centre", "spheres2.scn", "0 3.2 -3 0 0 .5 0 1 0 26", "inside", "at the centre of sphere 8: e = 0", sphere=8),
    _p("s2_on_surface", "spheres2.scn", _ON_SURFACE + " -1 -.3 .2 0 1 0 26", "surface", "on the surface of sphere 2: c ~ 0"),
    _p("s2_at_light", "spheres2.scn", "0 5 0 0 -1 .2 0 0 1 26", "surface", "at the first point light's position"),
    _p("s2_near", "spheres2.scn", "0 1.25 -1.0005 .3 -.1 1 0 1 0 26", "surface", "5e-4 outside sphere 1, looking past it"),
    _p("s2_far", "spheres2.scn", "0 2 -10000 0 0 1 0 1 0 26", "surface", "1e4 units away: cancellation in e.e - r^2", kw=dict(fov=0.2)),
    _p("dragon_inside", "dragon.scn", "0 .1 0 0 0 -1 0 1 0 23", "interior", "in the middle of the dragon: accepting triangles behind the camera"),
    _p("test_behind", "test.scn", "0 0 12 0 0 1 0 1 0 30", "interior", "the whole wall behind the camera"),
    _p("test_on_plane", "test.scn", ".7 .3 10 .3 .2 1 0 1 0 30", "surface", "on the plane of the wall's triangles, inside one's accept region: t = 0"),
    _p("test_near", "test.scn", "0 0 9.9995 0 .3 1 0 1 0 30", "surface", "5e-4 in front of the wall"),
    _p("test_far", "test.scn", "0 0 -10000 0 0 1 0 1 0 30", "surface", "1e4 units away", kw=dict(fov=0.25)),
    # ---- degenerate: kept apart, float images compared bit for bit with any NaN standing for any NaN
    _p("s2_up_parallel", "spheres2.scn", "0 2 -10 0 -.125 1 0 -.25 2 26", "degenerate", "up = 2 direction: right = 0"),
    _p("s2_zero_dir", "spheres2.scn", "0 2 -10 0 0 0 0 1 0 26", "degenerate", "direction = 0: right = 0, d = 0 on the centre row of an odd height"),
    _p("s2_zero_up", "spheres2.scn", "0 2 -10 0 -.1 .9 0 0 0 26", "degenerate", "up = 0: right = 0, every pixel the same ray"),
    _p("test_up_parallel", "test.scn", "0 0 -20 0 0 1 0 0 3 30", "degenerate", "up = 3 direction over the mesh"),
    _p("test_zero_dir", "test.scn", "0 0 -20 0 0 0 0 1 0 30", "degenerate", "direction = 0 over the mesh"),
]

BY_NAME = {p.name: p for p in POSES}
REGULAR = [p for p in POSES if p.family != "degenerate"]
DEGENERATE = [p for p in POSES if p.family == "degenerate"]
MESH = [p for p in POSES if p.base in ("test.scn", "dragon.scn")]
INSIDE = [p for p in POSES if p.family == "inside"]
INTERIOR = [p for p in POSES if p.family == "interior"]
LONG = [p for p in POSES if p.family == "long"]

# The three bounds on one scene file: dragon_inside at 4:3 with the fov alone varied, dmax within 1 % below and above each bound,
# and the two widest lenses (fov 181: a negative tangent, launch_params takes fabs).  (name, fov, level the frame must take)
BOUND_POSE = "dragon_inside"
BOUND_ASPECT = (96, 72)
BOUND_CASES = [
    ("below4", 104.17, 0), ("above4", 104.21, 1),
    ("below32", 171.37, 1), ("above32", 171.39, 2),
    ("below256", 178.946, 2), ("above256", 178.954, 3),
]
WIDE_CASES = [("fov179", 179.0, 3), ("fov181", 181.0, 3)]


GOLDEN_SIZE = (160, 120)
DEGENERATE_SIZE = (160, 119)  # an odd height: the centre row has v = 0 exactly


def _size_args(w, h, kw):
    return ["--width", str(w), "--height", str(h)] + (["--fov", repr(float(kw["fov"]))] if "fov" in kw else [])


def golden_cases():
    """(name, scene file, ref_render arguments) of the reference goldens of the poses: deterministic modes only.  The degenerate poses
    come last, under DEGENERATE_NAMES: tests/golden/make_golden.py keeps one only if two runs of the reference agree on it."""
    out = []
    for p in REGULAR:
        a = _size_args(*GOLDEN_SIZE, p.kw)
        out.append(("pose_%s" % p.name, scene_file(p), a))
        out.append(("pose_%s_shadow" % p.name, scene_file(p), a + ["--shadow"]))
    out.append(("pose_s2_rolled_strict", scene_file(BY_NAME["s2_rolled"]), _size_args(*GOLDEN_SIZE, {}) + ["--shadow", "--strict"]))
    out.append(("pose_s2_in_small_legacy", scene_file(BY_NAME["s2_in_small"]), _size_args(*GOLDEN_SIZE, {}) + ["--depth", "3", "--shadow", "--legacy"]))
    for name, fov, _ in BOUND_CASES + WIDE_CASES:
        out.append(("pose_bound_%s" % name, scene_file(BY_NAME[BOUND_POSE]), _size_args(*BOUND_ASPECT, dict(fov=fov)) + ["--depth", "1"]))
    for p in DEGENERATE:
        out.append(("pose_%s_shadow" % p.name, scene_file(p), _size_args(*DEGENERATE_SIZE, p.kw) + ["--shadow"]))
    return out


DEGENERATE_GOLDENS = {"pose_%s_shadow" % p.name for p in DEGENERATE}


def scene_file(pose):
    return "pose_%s.scn" % pose.name


def posed_text(base_text, camera_line):
    """base_text with every `camera` line replaced by camera_line (commented ones stay as they are)."""
    out, seen = [], 0
    for ln in base_text.split("\n"):
        if ln.split()[:1] == ["camera"]:
            ln = camera_line
            seen += 1
        out.append(ln)
    assert seen == 1, "the base scene must have exactly one camera line (%d)" % seen
    return "\n".join(out)


def write_pose(pose, path, base_path=None):
    """Write pose's scene to path; base_path: the scene whose camera is replaced (default: the base scene in tests/golden/scenes)."""
    with open(base_path or os.path.join(SCENES, pose.base)) as f:
        text = posed_text(f.read(), pose.camera)
    with open(path, "w") as f:
        f.write(text)
    return path


def write_all(folder=SCENES):
    return [write_pose(p, os.path.join(folder, scene_file(p))) for p in POSES]


def dump_lines(manifest, scn):
    """The lines of the reference's parseScene() dump of scene scn (manifest.json scene_dumps).  A base scene's dump is a file.  A posed
    scene differs from its base in the camera line alone, so its entry holds that line, the base's name and the sha256 of the whole
    dump the reference wrote: the base's lines with the camera line replaced, which must have that sha256."""
    import gzip
    import hashlib
    e = manifest["scene_dumps"][scn]
    with gzip.open(os.path.join(HERE, "golden", manifest["scene_dumps"][e.get("base", scn)]["file"]), "rt") as f:
        lines = f.read().splitlines()
    if "base" in e:
        lines[0] = e["camera"]
        assert hashlib.sha256(("\n".join(lines) + "\n").encode()).hexdigest() == e["sha256_uncompressed"], scn
    return lines


def dmax(camera, fov, width, height):
    """api.cpp launch_params: the bound on |d| over a frame's primary rays, from the 13 camera words (position, direction, up, right,
    half-angle).  camera_params: angle = (float) tan(pi * 0.5 * fov / 180.) with fov a binary32, aspect = width / float(height)."""
    c = np.asarray(camera, np.float32).astype(np.float64)
    angle = np.float32(math.tan(math.pi * 0.5 * float(np.float32(fov)) / 180.0))
    aspect = np.float32(width) / np.float32(height)
    umax = abs(float(angle) * float(aspect)) * 1.001
    vmax = abs(float(angle)) * 1.001
    ln = lambda v: math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return ln(c[3:6]) + umax * ln(c[9:12]) + vmax * ln(c[6:9])


def cull_level(d):
    """The culling set launch_params picks: 0, 1, 2, or 3 = none (every triangle)."""
    level = 0
    while level < len(BOUNDS) and not d < BOUNDS[level]:
        level += 1
    return level


def query_levels(dd):
    """wave_common.h pick_query_tree per 64-ray wave: dd float32 [n] in ray order -> the level each wave walks."""
    lim = [np.float32(b * b * 0.998) for b in BOUNDS]
    dd = np.asarray(dd, np.float32)
    pad = (-len(dd)) % 64
    w = np.concatenate([dd, np.zeros(pad, np.float32)]).reshape(-1, 64)
    level = np.zeros(len(w), np.int64)
    for k in range(len(BOUNDS)):
        with np.errstate(invalid="ignore"):
            level += (level == k) & ~np.all(w < lim[k], axis=1)
    return level


def random_camera(rng, centre, spheres=()):
    """A camera line of one of the non-degenerate pose families for a generated scene (tests/fuzz_parity.py): `centre` is a point
    to look at, spheres [(x, y, z, r), ...] the ones the camera may stand inside.  Seeded by rng alone."""
    centre = np.asarray(centre, np.float64)
    family = rng.choice(["rolled", "long", "inside", "axis", "near"])
    pos = centre + rng.normal(size=3) * rng.uniform(4, 12)
    if family == "inside" and len(spheres):
        x, y, z, r = spheres[int(rng.integers(0, len(spheres)))]
        off = rng.normal(size=3)
        pos = np.array([x, y, z]) + off / np.linalg.norm(off) * r * rng.choice([0.0, 0.3, 0.9, 1.0])  # centre .. surface
    elif family == "near" and len(spheres):
        x, y, z, r = spheres[int(rng.integers(0, len(spheres)))]
        off = rng.normal(size=3)
        pos = np.array([x, y, z]) + off / np.linalg.norm(off) * r * (1 + 10.0 ** rng.uniform(-4, -2))
    look = centre - pos + rng.normal(size=3)
    if family == "axis":
        look = np.eye(3)[int(rng.integers(0, 3))] * rng.choice([-1.0, 1.0]) + rng.normal(size=3) * 1e-3
        pos = centre - look * rng.uniform(5, 12)
    look /= max(np.linalg.norm(look), 1e-9)
    up = rng.normal(size=3)  # any roll, oblique to the direction
    while np.linalg.norm(np.cross(look, up)) < 0.2 * np.linalg.norm(up):
        up = rng.normal(size=3)
    up /= np.linalg.norm(up)
    scale_d, scale_u = 1.0, 1.0
    if family == "long":
        scale_d, scale_u = 10.0 ** rng.uniform(0, 2.5), 10.0 ** rng.uniform(-0.5, 1.5)
        pos = centre - look * scale_d * rng.uniform(1.1, 2.0)  # hits need t > 1 in units of |direction|
    elif family == "rolled":
        scale_u = rng.uniform(0.3, 3.0)
    return "camera %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g 30" % (*pos, *(look * scale_d), *(up * scale_u))
