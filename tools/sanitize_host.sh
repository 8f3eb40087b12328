#!/bin/sh
# Host code under AddressSanitizer + UBSan (CPU build only; the GPU pool runs no sanitizers): the .scn loader on
# the reference scenes and on malformed / random input, every table builder and the getters.  The digests of every
# derived table of every scene go to build/scene_tables.txt.  SANITIZE_HOST_FLAGS / SANITIZE_HOST_SRCS replace the
# compiler flags / the sources under test: two builds (-O2, no sanitizer) on one machine must print the same digests.
set -e
cd "$(dirname "$0")/.."
mkdir -p build
CSRC=skele_raytracer_amd/csrc
FLAGS=${SANITIZE_HOST_FLAGS:--g -O1 -fsanitize=address,undefined,float-cast-overflow -fno-omit-frame-pointer}
SRCS=${SANITIZE_HOST_SRCS:-$CSRC/scene_host.cpp $CSRC/scene_masks.cpp $CSRC/scene_trees.cpp $CSRC/scene_pack.cpp}
rm -rf build/sanitize_obj && mkdir -p build/sanitize_obj
pids=""
for f in tools/sanitize_host.cpp $SRCS; do # (side by side)
	g++ -std=c++17 $FLAGS -Iinclude -c -o build/sanitize_obj/"$(basename "$f" .cpp)".o "$f" &
	pids="$pids $!"
done
for p in $pids; do wait "$p"; done # (set -e: the script stops at the first file that did not compile)
g++ $FLAGS -o build/sanitize_host build/sanitize_obj/*.o
printf 'sphere 1 2\nvertex 1 2\ntriangle 0 1 999999\ntriangle -5 0 1\nmaterial 1\ncamera\npoint_light 1 2 3\nvertex nan inf -inf\nvertex 1e39 0 0\ntriangle 0 0 0\ntriangle 1.7 0.2 2.9\nvelocity 1 nan 3\nvelocity 1 2\nvelocity 1 2 3\nsphere 0 0 0 1\n' > build/bad1.scn
: > build/empty.scn
rm -f build/gen_*.scn
python3 - <<'PY'
import random, re
random.seed(1)
words = ["sphere", "vertex", "triangle", "material", "camera", "point_light", "directional_light", "ambient_light", "background",
         "max_depth", "film_resolution", "spherical_fog", "normal", "max_vertices", "max_normals", "#", "output_image"]
with open("build/fuzz.scn", "w") as f:
    for _ in range(3000):
        f.write(random.choice(words) + " " + " ".join(random.choice(["1", "-2.5", "1e30", "nan", "x", "0", "3", "100000", "-1", ""]) for _ in range(random.randint(0, 16))) + "\n")

# seeded scenes for the mask and tree builders: sphere counts around every limit, 1-3 lights, a light inside a sphere, a sphere
# too small for surface patches, spheres beside a mesh
cells = open("skele_raytracer_amd/csrc/shadow_cells.h").read()
limit = {k: int(re.search(r"#define\s+%s\s+(\d+)" % k, cells).group(1)) for k in ("SKR_SHADOW_MAX_SPHERES", "SKR_GI_MAX_SPHERES")}

def scene(name, n_spheres, n_lights, seed, light_in_sphere=False, tiny=False, mesh=0, tri_size=2.0, ground=True):
    rnd = random.Random(seed)
    u = lambda a, b: "%.6g" % rnd.uniform(a, b)
    with open("build/gen_%s.scn" % name, "w") as f:
        f.write("camera 0 2 9 0 -0.15 -1 0 1 0 30\nambient_light 0.2 0.2 0.2\nbackground 0.1 0.1 0.2\n")
        spheres = []
        for k in range(n_spheres):
            f.write("material %s %s %s %s %s %s %s %s %s %s 0 0 0 1\n" % tuple([u(0, 1) for _ in range(9)] + [u(1, 64)]))
            if ground and k == 0 and n_spheres > 2:
                spheres.append((0.0, -1000.0, 0.0, 1000.0))  # the ground
            else:
                spheres.append((rnd.uniform(-4, 4), rnd.uniform(0.2, 3), rnd.uniform(-4, 4), 5e-4 if tiny and k == 1 else rnd.uniform(0.15, 0.9)))
            f.write("sphere %.6g %.6g %.6g %.6g\n" % spheres[-1])
        for l in range(n_lights):
            if light_in_sphere and l == 0:
                x, y, z, r = spheres[-1]
                f.write("point_light 1 1 1 %.6g %.6g %.6g\n" % (x + 0.3 * r, y - 0.2 * r, z + 0.1 * r))
            else:
                f.write("point_light %s %s %s %s %s %s\n" % (u(0.2, 1), u(0.2, 1), u(0.2, 1), u(-6, 6), u(4, 9), u(-6, 6)))
        for t in range(mesh):
            p = [rnd.uniform(-3, 3), rnd.uniform(0, 3), rnd.uniform(-3, 3)]
            for v in range(3):
                f.write("vertex %.6g %.6g %.6g\n" % tuple(c + rnd.uniform(-tri_size, tri_size) for c in p))
        for t in range(mesh):
            f.write("triangle %d %d %d\n" % (3 * t, 3 * t + 1, 3 * t + 2))

counts = [1, 2, 9, 16, 17, 32] + sorted({limit["SKR_SHADOW_MAX_SPHERES"] + 1, limit["SKR_GI_MAX_SPHERES"] + 1})
for i, n in enumerate(counts):
    scene("spheres%03d" % n, n, 1 + i % 3, 100 + n)
scene("light_inside", 6, 2, 201, light_in_sphere=True)
scene("tiny_sphere", 5, 1, 202, tiny=True)
scene("mixed_a", 4, 2, 203, mesh=7)
scene("mixed_b", 20, 3, 204, mesh=40, tri_size=0.02, ground=False)  # (small and near enough for finite culling radii)
PY
./build/sanitize_host tests/golden/scenes/*.scn build/gen_*.scn build/bad1.scn build/empty.scn build/fuzz.scn /nonexistent.scn > build/scene_tables.txt 2> build/sanitize_host.log
if grep -q "runtime error\|Sanitizer" build/sanitize_host.log; then grep "runtime error\|Sanitizer" build/sanitize_host.log; exit 1; fi
echo "sanitize_host: clean"
