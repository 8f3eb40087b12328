/* include/skr.h — C ABI of libskr.so, the MI355X-native replacement for the
 * reference's per-pixel hot path (lilinitsy/skele-raytracer).
 *
 * The reference has no plugin/FFI interface: its seam is the in-process call
 *     glm::vec3 shade(Ray, Scene, int depth, bool monte_carlo, short num_path_traces)
 *         src/raytrace.h:139, called once per pixel-sample from src/main.cpp:64,83,162,181
 * fed by   Scene parseScene(std::string)          src/scene.h:31, src/scene.cpp:12
 * and      struct Options                         src/utils.h:26-34
 * and drained by the inline P6 writer             src/main.cpp:199-211 (== :88-100).
 * This header lifts that seam to frame / row-tile granularity: plain pointers
 * and sizes, no C++ or torch types.  Every entry point names the reference
 * interface it replaces.  Return value 0 = ok; otherwise an skr_status (the
 * reference itself has no error returns: it prints and exits with status 0).
 *
 * Threading: a renderer is bound to one HIP device; calls on one renderer must
 * not overlap; different renderers are independent.  All device work is
 * enqueued on the caller's stream and is asynchronous unless stated.
 */
#ifndef SKR_H
#define SKR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKR_ABI_VERSION 7 /* 7: skr_ray, skr_hit, skr_trace_rays, skr_camera_rays (ray queries), then skr_shade_rays (shading queries: an addition that leaves every
                            * existing entry point and struct as it was; SKR_HAS_SHADE_RAYS tells a caller it is there); 6: skr_scene_get_gi_masks; 5: skr_scene_get_shadow_masks; 4: SKR_SCN_FOG, skr_scene_get_fog, skr_scene_set_fog (spherical fog; skr_options unchanged); 3: skr_options grew by shade_triangles, progressive_passes and legacy_reflect (56 bytes); 2: multi-GPU entry points, skr_scene_info.n_directional_lights */
#define SKR_HAS_SHADE_RAYS 1
#define SKR_HAS_DENOISE 1    /* skr_denoise, skr_render_denoised_host: an addition that leaves every existing entry point and struct as it was */
#define SKR_HAS_ADAPTIVE 1   /* skr_adaptive, skr_render_adaptive(_host): an addition that leaves every existing entry point and struct as it was */
#define SKR_HAS_ADAPTIVE_DENOISE 1 /* skr_render_adaptive_var, skr_denoise_var, skr_render_adaptive_denoised_host: additions, likewise */
#define SKR_HAS_SPOT_LIGHTS 1 /* SKR_SCN_SPOT, skr_scene_get/set_spot_lights, skr_scene_get_spot_cones, skr_debug_eval op 17: an addition that leaves every existing entry point and struct as it was */
#define SKR_HAS_SOFT_LIGHTS 1 /* skr_scene_set/get_light_radii, skr_debug_eval op 18: an addition that leaves every existing entry point and struct as it was */
#define SKR_HAS_ROOT_PAIRS 1 /* skr_debug_eval op 19: an addition that leaves every existing entry point and struct as it was */
#define SKR_HAS_LENS 1 /* skr_scene_set/get_lens, skr_debug_eval op 22: an addition that leaves every existing entry point and struct as it was */
#define SKR_HAS_MOTION 1 /* SKR_SCN_MOTION, skr_scene_set/get_sphere_velocities, skr_scene_set/get_shutter, skr_debug_eval op 24: an addition that leaves every existing entry point and struct as it was */
#define SKR_HAS_ENVIRONMENT 1 /* skr_scene_set/get_environment, skr_read_pfm, skr_debug_eval op 25: an addition that leaves every existing entry point and struct as it was */
#define SKR_HAS_TEXTURES 1 /* SKR_SCN_TEXTURE, skr_scene_add/get_texture, skr_scene_texture_count, skr_scene_set/get_sphere_textures, skr_scene_clear_textures, skr_debug_eval op 26: an addition that leaves every existing entry point and struct as it was */
#define SKR_HAS_EMISSION 1 /* SKR_SCN_EMISSION, skr_scene_set/get_sphere_emission: an addition that leaves every existing entry point and struct as it was */
#define SKR_HAS_TRIANGLE_SHADOWS 1 /* SKR_SCN_TRIANGLE_SHADOWS, skr_scene_set/get_triangle_shadows, skr_scene_get_trace_culling: an addition that leaves every existing entry point and struct as it was */

typedef enum {
	SKR_OK = 0,
	SKR_ERR_IO = 1,            /* cannot open / write a file */
	SKR_ERR_ARG = 2,           /* bad argument (null, zero size, bad row range ...) */
	SKR_ERR_HIP = 3,           /* a HIP runtime call failed; see skr_last_error() */
	SKR_ERR_UNSUPPORTED = 4,   /* configuration outside what the kernels cover (see skr_last_error()) */
	SKR_ERR_NO_DEVICE = 5      /* no gfx950 device / HIP runtime unusable: there is NO CPU fallback */
} skr_status;

/* Host-side scene in the SoA layout that is uploaded to HBM.  Opaque. */
typedef struct skr_scene skr_scene;
/* Device context: one HIP device, the scene resident in HBM.  Opaque. */
typedef struct skr_renderer skr_renderer;

/* Mirrors struct Options (utils.h:26-34) plus the locals main() folds into the
 * scene before rendering (width/height/use_shadows, main.cpp:236-244,393-396).
 * skr_options_default() fills the reference's defaults. */
typedef struct {
	int32_t width;            /* --width,  default 1920 (scene.h:15) */
	int32_t height;           /* --height, default 1080 */
	float fov;                /* --fov degrees, default 60 (utils.h:30) */
	int32_t monte_carlo;      /* --gillum given (utils.h:28) */
	int32_t num_path_traces;  /* --gillum N, default 1 (utils.h:31, a short) */
	int32_t grid_size;        /* --jsample g, default 0 = pixel centres (utils.h:32) */
	int32_t max_depth;        /* --depth d > 0, default 3 (utils.h:33) */
	int32_t use_shadows;      /* --shadow (main.cpp:375-378); absent == 0 */
	uint64_t seed;            /* new: key of the counter RNG that replaces srand(time(0)) (main.cpp:400) */
	int32_t shade_triangles;  /* new, default 0 (`raytracer --shade-triangles`).  0 = HEAD: a ray whose closest hit is a
	                           * triangle returns black (raytrace.h:221-224).  1 = triangles are surfaces: among the triangles
	                           * utils.h:181-213 accepts with t > 0 (the one the ray starts on excepted) the smallest t wins if it is
	                           * strictly below the closest sphere's (equal t: lower index in the file); the hit is shaded as a
	                           * sphere is (blinn_phong.h, raytrace.h:107-136,208-218) with the material in force on its
	                           * `triangle` line and the geometric normal normalize(cross(v1-v0, v2-v0)) turned against the ray;
	                           * shadow rays test spheres only (utils.h:42-76) unless the scene has triangle shadows switched on
	                           * (skr_scene_set_triangle_shadows, below); the child rays of a triangle hit start at
	                           * P + 1e-5 like a sphere's (raytrace.h:128).  No counterpart in the reference, so no reference output
	                           * pins it (tests/test_shade_triangles.py).  Any --depth, with or without --gillum (the general level pipeline). */
	int32_t progressive_passes; /* new, default 1 (`raytracer --progressive K`, SURVEY.md 8f-4: what the SDL viewer of main.cpp:183-197 is
	                           * for, headless).  K > 1: every render entry point traces K whole frames under the seeds seed, seed+1, ...,
	                           * seed+K-1, sums them in binary32 in that order, divides by (float) K once and quantises the mean like
	                           * a single frame (main.cpp:205).  K <= 1 is the single frame, bit for bit. */
	int32_t legacy_reflect;   /* new, default 0 (`raytracer --legacy-reflect`).  1 = the code behind the early
	                           * `return total_colour;` of raytrace.h:44 runs: the Fresnel term fr (blinn_phong.h:156-184) and, where the
	                           * material's specular colour is not (0,0,0), for every light (point lights first) a refraction ray
	                           * (:143-153; `refraction_colour = fr * shade(...)`: the last light's stays) and a reflection ray (:137-140:
	                           * the LIGHT direction mirrored at the normal; `+= (1 - fr) * specular * shade(...)`), both from the hit point
	                           * itself with depth - 1, added to the direct term as raytrace.h:102 does.  The index of refraction is the
	                           * 14th number of the `material` line (skr_scene_set_sphere_ior for scenes from arrays; default 1).
	                           * Children of the counter RNG's tree: arity N + 2 L (L lights); child N + 2 l = refraction of light l,
	                           * N + 2 l + 1 = its reflection.  Unreachable at HEAD, so no output of the reference's program pins it: the
	                           * reference's own fresnel / refraction / reflect_direction functions pin the three formulas, a restated
	                           * composition the rest, and the README pictures (made when it ran) are the visual check
	                           * (tests/test_legacy_reflect.py).  Any --depth, with --gillum and with shade_triangles (the general level pipeline). */
} skr_options;

typedef struct {
	int32_t n_spheres, n_triangles, n_point_lights, n_vertices;
	int32_t n_directional_dropped; /* parsed and never pushed, scene.cpp:139-163 (0 under SKR_SCN_STRICT) */
	int32_t n_fog_skipped;         /* spherical_fog lines (UB in the reference, scene.cpp:207-212): warned + skipped */
	int32_t n_unknown;             /* "WARNING. Do not know command" lines, scene.cpp:214-217 */
	int32_t n_bad_triangles;       /* triangle lines whose indices fall outside the vertex pool (skipped) */
	int32_t film_width, film_height; /* film_resolution: parsed, overridden by the CLI (main.cpp:393-395) */
	int32_t max_depth_parsed;      /* max_depth: parsed, never read (scene.cpp:192-198) */
	float camera[13];              /* position, direction, up, right (camera.h:30), half_height_angle */
	float background[3];
	float ambient[3];
	int32_t n_directional_lights;  /* SKR_SCN_STRICT: directional lights kept (after the point lights in shading order) */
} skr_scene_info;

/* ---- scene: replaces Scene parseScene(std::string) (scene.cpp:12-227) ---- */
/* echo != 0 prints the reference's per-line echo to stdout (scene.cpp:50,...). */
int skr_scene_create_from_scn(const char *path, int echo, skr_scene **out);
/* flags: SKR_SCN_STRICT = the loader as its author evidently meant it (`raytracer --strict-scn`):
 * directional lights are pushed (scene.cpp:139-163 builds each one, clamps its colour to <= 1 and forgets the push_back)
 * and shaded by the reference's own loops (blinn_phong.h:77-85,122-131; shadow test utils.h:60-76).  film_resolution and
 * max_depth are reported in skr_scene_info either way; --strict-scn makes the CLI honour them. */
#define SKR_SCN_STRICT 1u
/* SKR_SCN_FOG (`raytracer --scn-fog`; combines with SKR_SCN_STRICT): `spherical_fog x y z radius r g b scattering [absorption]` lines
 * are parsed in the field order of the reference's sscanf (scene.cpp:210; a missing absorption is 0) and kept, in file order; a line with
 * fewer than 8 numbers is still warned about, skipped and counted in n_fog_skipped.  Without the flag every fog line is skipped (the
 * reference's parse is undefined behaviour).  A scene with fog volumes is shaded with the fog term of blinn_phong.h:19-43 (DESIGN.md
 * "Spherical fog": for every lit point light at a sphere hit, the term of every fog volume instead of the diffuse and again instead of
 * the specular term, the reference's rand() replaced by the counter RNG) on the general level pipeline; it cannot be combined with
 * skr_options.legacy_reflect or shade_triangles (SKR_ERR_UNSUPPORTED). */
#define SKR_SCN_FOG 2u
#define SKR_FOG_MAX_VOLUMES 64
/* SKR_SCN_TRIANGLE_SHADOWS (`raytracer --triangle-shadows`; combines with the other two): the scene is created with triangle shadows
 * switched on (skr_scene_set_triangle_shadows below states the rule). */
#define SKR_SCN_TRIANGLE_SHADOWS 4u
int skr_scene_create_from_scn_ex(const char *path, int echo, uint32_t flags, skr_scene **out);
/* Build a scene from arrays (synthetic tests): spheres[n][14] = centre(3) radius
 * ambient(3) diffuse(3) specular(3) power; triangles[n][9] = v0 v1 v2;
 * point_lights[n][6] = position colour; camera[9] = position direction up. */
int skr_scene_create_from_arrays(const float *spheres, int32_t n_spheres, const float *triangles, int32_t n_triangles,
								 const float *point_lights, int32_t n_point_lights, const float camera[9],
								 const float background[3], const float ambient[3], skr_scene **out);
/* The fog volumes of a scene, rows[n][9] = centre(3) radius albedo(3) scattering absorption, in file order (at most
 * SKR_FOG_MAX_VOLUMES).  get: *n = their number, rows (if not NULL) receives them.  set: replaces them (n = 0: no fog) — scenes made
 * from arrays, and tests that choose scattering and absorption; a renderer takes the volumes the scene has when it is created. */
int skr_scene_get_fog(const skr_scene *scene, float *rows, int32_t *n);
int skr_scene_set_fog(skr_scene *scene, const float *rows, int32_t n);
/* Triangle shadows (new, off by default; no counterpart in the reference, whose shadow rays test spheres only and whose triangles are
 * no surfaces).  A switch of the scene; a renderer takes the scene's setting when it is created, as it takes the fog volumes (its
 * clones and the multi-GPU frame steps with it).  The rule (normative):
 *   - In force for a launch iff the renderer's scene has the switch on AND the launch's effective shade_triangles is 1 (the option is
 *     set and the scene has triangles) AND use_shadows is set.  Otherwise the launch is what it is without the switch, bit for bit, with
 *     the same kernels, skr_kernel_variant() and counters: without shade_triangles a triangle is a black hole, not a surface, and the
 *     switch is a no-op.
 *   - When in force, at every shaded hit (sphere or triangle surface; the hits of --gillum and legacy_reflect child rays are shaded
 *     hits like any other) and for every light, in the reference's light order:
 *     1. the sphere test runs first, exactly as without the switch (utils.h:42-76: origin o = P + 1e-6 added to every component,
 *        direction L; the same shadow-ray and sphere-test counts).  If a sphere occludes, the light is dark and no triangle is looked at;
 *     2. otherwise the triangles are tested with the same o and the same L (the bits the sphere test used).  Triangle i (file index)
 *        occludes iff utils.h:181-213 accepts (o, L, triangle i) with distance t AND t > 0 AND i is not the file index of the triangle
 *        being shaded (none at a sphere hit) AND, for a point light, t < dist with dist = sqrtf(to_l . to_l), to_l = Lp - P, the
 *        correctly rounded binary32 value blinn_phong.h calls `distance`.  A directional light has no upper bound.  The outcome is
 *        binary and does not depend on the order in which triangles are tried; the occluder is the accept region of the reference's
 *        test (its mirrored triangle), the same surface that is rendered;
 *     3. an occluded light adds neither its diffuse nor its specular term (as for a sphere occluder).  Nothing else changes: ambient,
 *        the child rays, node ids and RNG draws are as they are.  Fog cannot be combined with shade_triangles and stays excluded.
 *   - Counters: skr_renderer_read_counters / read_work advance exactly as without the switch (one shadow ray per light per hit; sphere
 *     tests as the reference's loop runs them).  While skr_renderer_count_triangle_work is on, the culling-sphere and triangle tests the
 *     shadow walk executes are added to out[0] / out[1] of skr_renderer_read_triangle_work; its out[2] (the reference's own loop) is
 *     not advanced by shadow rays: the reference has no such loop. */
int skr_scene_set_triangle_shadows(skr_scene *scene, int enable);
int skr_scene_get_triangle_shadows(const skr_scene *scene, int *enabled);
/* The sphere tree (new, off by default: DESIGN.md 8.10).  A switch of the scene, as triangle shadows are: a renderer takes the scene's
 * setting when it is created, its clones and the multi-GPU frame steps with it.  SKR_SCN_SPHERE_TREE (`raytracer --sphere-tree`;
 * combines with the other scene flags) creates the scene with it switched on.  The rule (normative):
 *   - Off: every launch is what it is without the switch, bit for bit: the same kernels, skr_kernel_variant(), counters, and the same
 *     refusal of a scene whose sphere table does not fit a workgroup's LDS.
 *   - On, for a scene with at least one sphere: every frame and every shading query renders on the general level pipeline, in every
 *     mode it has; skr_kernel_variant() is "level_pipeline_g1_stree" ("level_pipeline_g1_stree_tshadow" where triangle shadows are in
 *     force; shading queries: "shade_rays_g1_stree", "shade_rays_g1_stree_tshadow").  Sphere geometry and materials are read from HBM:
 *     no kernel's LDS need depends on the sphere count, which is limited by memory and n < 2^31 only.  Lights stay in LDS.  The shadow
 *     masks and GI masks are not consulted.
 *   - Images (bytes and floats) and skr_renderer_read_work out[0..3] are what they are without the switch where both render the scene:
 *     the closest hit is the sphere with the smallest t2, equal t2 going to the lower file index; out[3] counts n_spheres per radiance
 *     ray and, per shadow ray, the spheres up to and including the first occluder in file order, as the reference's loops run.
 *   - Culling is exactly conservative: no sphere whose binary32 discriminant makes it a candidate for a ray (D >= 0 and b < 0,
 *     utils.h:113-121 in the reference's operation order) is skipped for that ray.  A wave with a ray that starts outside the tree's
 *     ball, or whose direction is not finite or of extreme length, runs the loop over every sphere instead; so does every wave under
 *     SKR_NO_SPHERE_CULL=1 (read like the other SKR_* switches).  The answers are the same.
 *   - Ray queries (skr_trace_rays, closest and any-hit) walk the same tree under the same rule — a wave with a ray outside the ball or with
 *     a direction that is not finite runs the loop over every sphere — and give the answers they give without the switch. */
#define SKR_HAS_SPHERE_TREE 1
#define SKR_SCN_SPHERE_TREE 8u
int skr_scene_set_sphere_tree(skr_scene *scene, int enable);
int skr_scene_get_sphere_tree(const skr_scene *scene, int *enabled);
/* Spot lights (new, opt-in; no counterpart in the reference, whose parseScene answers a `spot_light` line with "WARNING. Do not know
 * command", scene.cpp:214-217).  SKR_SCN_SPOT (`raytracer --scn-spot`; combines with the other scene flags): a line
 *     spot_light r g b px py pz dx dy dz angle1 angle2
 * (the field order of the format's other light lines; the angles in degrees from the axis d) is kept, in file order, and no longer
 * counted in n_unknown.  A line with fewer than 11 numbers, a field that is not finite, a zero direction, or angles outside
 * 0 <= angle1 <= angle2 <= 180 (or one past SKR_SPOT_MAX_LIGHTS) is warned about, skipped and still counted in n_unknown.  Without
 * the flag everything is as it was, byte for byte; skr_scene_info does not grow.  The rule (normative):
 *   - A spot light is a point light with a cone: a point-light row of the light table at its position, colour not clamped.  Shading
 *     order: the point lights in file order, the spot lights in file order, then (SKR_SCN_STRICT) the directional lights.  L, the
 *     colour lc and the intensity 1 / d^2 are the point light's (blinn_phong.h:67-72); the shadow masks treat it as the point light
 *     it geometrically is (skr_scene_get_shadow_masks reports n_point + n_spot lights).  Spot lights count as lights wherever a
 *     light limit exists (a workgroup's LDS holds the light table).
 *   - The host derives once per light, in binary32 with one IEEE operation per step, the unit axis a = d * (1 / sqrt(d . d)) (the
 *     device's normalize3), c1 = (float) cos((double) angle1 * (M_PI / 180.0)) and c2 = min(c1, (float) cos((double) angle2 *
 *     (M_PI / 180.0))): skr_scene_get_spot_cones.  Kernels and checkers read these values; neither calls cos again.
 *   - Cone factor at a shading point P, with L the unit vector from P to the light: c = -dot(a, L) ((x + y) + z of the products).
 *     c >= c1: f = 1.  Else !(c > c2) (NaN included): the light is OUTSIDE.  Else u = (c - c2) / (c1 - c2) and
 *     f = (u * u) * (3.0f - 2.0f * u), binary32, one correctly rounded operation per step, not contracted.
 *   - A light that is not outside enters the point-light expression with the colour lc * f (per component, before anything else) and
 *     casts its shadow ray exactly as a point light does (triangle shadows included: t < the distance to the light).  x * 1 == x:
 *     a spot light with angle1 = 180 shades exactly as a point light.
 *   - A light that is outside at P adds nothing, casts no shadow ray, adds nothing to the shadow-ray count or the sphere-test count
 *     and is never tested against triangles.
 *   - A scene with at least one spot light renders every frame and every shading query on the general level pipeline
 *     (skr_kernel_variant() "level_pipeline_g1_spot", "level_pipeline_g1_spot_tshadow", "shade_rays_g1_spot",
 *     "shade_rays_g1_spot_tshadow"), in every mode it has but three: skr_options.legacy_reflect, fog volumes and the sphere-tree
 *     switch are refused with SKR_ERR_UNSUPPORTED.  A scene loaded with the flag that holds no spot light is planned and rendered
 *     exactly as without it. */
#define SKR_SCN_SPOT 16u
#define SKR_SPOT_MAX_LIGHTS 8192 /* (more light rows than a workgroup's LDS holds: the LDS check refuses a scene first) */
/* The spot lights of a scene, rows[n][11] = the file's fields in file order.  get: *n = their number, rows (if not NULL) receives
 * them.  set: replaces them (n = 0: none) under the loader's validation — SKR_ERR_ARG on a bad row, the scene unchanged — for scenes
 * made from arrays and for tests; a renderer takes the spot lights the scene has when it is created, as it takes the fog volumes.
 * skr_scene_get_spot_cones: cones[n][5] = {a.xyz, c1, c2} as derived above.
 * skr_scene_set_spot_lights changes the light count, so it resets every light radius (skr_scene_set_light_radii below) to 0. */
int skr_scene_get_spot_lights(const skr_scene *scene, float *rows, int32_t *n);
int skr_scene_set_spot_lights(skr_scene *scene, const float *rows, int32_t n);
int skr_scene_get_spot_cones(const skr_scene *scene, float *cones);
/* Sphere lights: point and spot lights with a radius, for soft shadows (new, opt-in; no counterpart in the reference, whose lights
 * are points).  The rule (normative):
 *   - Every point light and every spot light has a radius R >= 0, default 0.  Directional lights have none.  l is a light's index in
 *     shading order: the point lights, then the spot lights, then the directional lights.
 *   - For a light l with R > 0 a shading node — the (pixel, aa, node) of the counter RNG — takes ONE sample position Lp' on the sphere
 *     of radius R about the light's position Lp; from then on the light is, for that node, the point light at Lp'.
 *   - The draw: one call philox4x32(pixel, aa, node, soft_ctr3(l), seed_lo, seed_hi) with soft_ctr3(l) = 0x80000080u | (l << 8).  The
 *     word is disjoint from every other draw: the hemisphere draws have bit 31 clear, the fog draws' word has bit 7 clear, the jitter
 *     word is 0xFFFFFFFF and here bits 0-6 are 0.  u1 = u31_to_unit(out[0]), u2 = u31_to_unit(out[1]); out[2] and out[3] are unused.
 *   - The position, in binary32, one correctly rounded operation per step, no libm, no binary64:
 *         z = 1 - 2 * u1;  s = sqrt(max0(1 - z * z));  phi = 0x1.921fb6p+2f * u2  ((float) 2 pi times u2, not the hemisphere sampler's
 *         binary64 product; phi <= (float) 2 pi, inside the range sincos_spec is exhaustively checked on);  (sn, cs) = sincos_spec(phi);
 *         Lp' = (Lp.x + R * (s * cs), Lp.y + R * z, Lp.z + R * (s * sn)).
 *   - Everything the point-light expression derives from the position uses Lp': to_l = Lp' - P, L and 1 / d^2; the shadow ray from
 *     P + 1e-6 along that L (the any-hit rule is unchanged: any sphere with 1 < t < inf occludes, no closer-than-the-light test); the
 *     far end length(Lp' - P) of the triangle-shadow walk; for a spot light the cone decision spot_cone(a, c1, c2, L) with that L (axis
 *     and cosines unchanged; a sample outside the cone adds nothing and casts nothing).  One sample per (node, light) serves the
 *     diffuse and the specular term, as one cast does.
 *   - A light with R == 0 makes no draw and is the point light it was, bit for bit.  A point inside a light's ball, or at Lp', gets no
 *     special case.  The work counters keep their meaning: shadow_rays the casts, sphere_tests the reference's loop count up to the
 *     first occluder in file order.
 *   - A scene with at least one R > 0 renders every frame and every shading query on the general level pipeline (skr_kernel_variant()
 *     "level_pipeline_g1_soft", "level_pipeline_g1_soft_tshadow", "shade_rays_g1_soft", "shade_rays_g1_soft_tshadow"), in every mode
 *     it has but three: skr_options.legacy_reflect, fog volumes and the sphere-tree switch are refused with SKR_ERR_UNSUPPORTED.  A
 *     pair of lights in which either has R > 0 tests every sphere (the shadow masks are built for rays toward Lp).  A scene whose
 *     radii are all 0 is planned and rendered exactly as before.
 * set: radii[n], n == n_point + n_spot, every value finite and >= 0; otherwise SKR_ERR_ARG and the scene is unchanged.  A renderer
 * takes the radii the scene has when it is created, as it takes the spot lights.  skr_scene_set_spot_lights resets every radius to 0
 * (it changes the light count).  get: *n = n_point + n_spot, radii (if not NULL) receives them. */
int skr_scene_set_light_radii(skr_scene *scene, const float *radii, int32_t n);
int skr_scene_get_light_radii(const skr_scene *scene, float *radii, int32_t *n);
/* Thin-lens camera: depth of field from an aperture and a focus (new, opt-in; no counterpart in the reference, whose camera is a
 * pinhole).  A scene has a lens (A, F): aperture radius A >= 0, default 0, and focus parameter F > 0, default 1; both finite.  The rule
 * (normative):
 *   - A == 0 is the pinhole camera: no draw is made; planning, skr_kernel_variant(), frames and counters are what they are without a
 *     lens, bit for bit.
 *   - With A > 0 the primary sample of (pixel, aa) under seed s takes ONE lens sample.  The draw: one call philox4x32(pixel, aa, 0,
 *     SKR_LENS_CTR3, seed_lo, seed_hi) with SKR_LENS_CTR3 = 0x800000C0u.  The word is disjoint from every other draw: the hemisphere draws
 *     have bit 31 clear, the fog draws' word has bit 7 clear, the light samples' word (0x80000080u | (l << 8)) has bit 6 clear, the jitter
 *     word is 0xFFFFFFFF.  u1 = u31_to_unit(out[0]), u2 = u31_to_unit(out[1]); out[2] and out[3] are unused.
 *   - The disk point, in binary32, one correctly rounded operation per step, no libm, no binary64, not contracted:
 *         r = sqrt(u1);  phi = 0x1.921fb6p+2f * u2  (the light sample's product, inside the range sincos_spec is exhaustively checked
 *         on);  (sn, cs) = sincos_spec(phi);  lx = r * cs;  ly = r * sn.
 *   - The ray: d is the pinhole direction of that pixel and sample (main.cpp:140-182: both branches and the jitter draw untouched);
 *     k = A / F is one binary32 division, done once on the host;
 *         o' = (cam_pos + cam_right * (A * lx)) + cam_up * (A * ly)
 *         d' = (d - cam_right * (k * lx)) - cam_up * (k * ly)
 *     with cam_right and cam_up as the camera holds them (not unit length, as d is not).
 *   - Focus and the t window: the ray reaches the pinhole ray's point cam_pos + F d at t = F, so F is in units of d, as every t of the
 *     renderer is.  d' keeps d's scale, so the sphere acceptance window 1 < t (raytrace.h:152-165) means what it means for the pinhole.
 *   - Shading: the primary segment of (pixel, aa) is the ray (o', d'), node 0, ignore_triangle = -1, tmax = +inf.  Everything below it
 *     is unchanged: child rays, GI draws, light samples, counters, the AA sum and its / (float) (g * g), and progressive_passes (the
 *     seeds s .. s + K - 1 give K lens samples).  The specular view vector still points to the scene camera cam_pos, as everywhere
 *     (blinn_phong.h:93; skr_shade_rays says the same).
 *   - A scene with A > 0 renders every frame on the general level pipeline (skr_kernel_variant() carries one "_lens" part behind the
 *     light part: "level_pipeline_g1_lens", "level_pipeline_g1_spot_lens_tshadow", ...), in every mode it has but three:
 *     skr_options.legacy_reflect, fog volumes and the sphere-tree switch are refused with SKR_ERR_UNSUPPORTED, as spot lights and light
 *     radii refuse them.  skr_render_denoised_host and skr_render_adaptive_denoised_host are refused too (their guides are pinhole
 *     first hits, and their edge-stopping would undo the blur); skr_denoise / skr_denoise_var on caller-supplied guides are unaffected.
 *   - skr_camera_rays under a lens returns (o', d') for (opt, sample), keyed to opt->seed: skr_shade_rays of a frame's camera rays with
 *     keys y * width + x stays that sample of the frame, bit for bit.  skr_shade_rays and skr_trace_rays themselves are unaffected: the
 *     rays are the caller's.
 * set: a value that is not finite, aperture < 0 or focus <= 0: SKR_ERR_ARG and the scene is unchanged.  A renderer takes the lens the
 * scene has when it is created, as it takes the light radii; skr_renderer_clone carries it. */
#define SKR_LENS_CTR3 0x800000C0u
int skr_scene_set_lens(skr_scene *scene, float aperture, float focus);
int skr_scene_get_lens(const skr_scene *scene, float *aperture, float *focus);
/* Motion blur: moving spheres, one shutter time per sample (new, opt-in; no counterpart in the reference, whose spheres are frozen).  A
 * scene carries one velocity v_i (3 floats) per sphere, default (0, 0, 0), and a shutter S, default 1; every value finite, S >= 0.
 * SKR_SCN_MOTION (`raytracer --scn-motion`; combines with the other scene flags): a line
 *     velocity vx vy vz
 * sets the velocity in force for the `sphere` lines that follow, stateful exactly as `material` is; the initial value is 0 0 0.  A line
 * without 3 finite numbers is warned about, skipped and counted in n_unknown.  Without the flag the line stays "WARNING. Do not know
 * command" and everything is as it was, byte for byte; skr_scene_info does not grow.  The rule (normative):
 *   - In force.  Motion is in force for a launch iff S > 0 and some component of some v_i is != 0.  Otherwise no draw is made:
 *     planning, skr_kernel_variant(), frames, floats and all work counters are exactly what they are without velocities.
 *   - The draw: one call per (pixel, aa), philox4x32(pixel, aa, 0, SKR_SHUTTER_CTR3, seed_lo, seed_hi) with SKR_SHUTTER_CTR3 =
 *     0x800000E0u.  The word is disjoint from every other draw: bit 31 is set (the hemisphere draws have it clear), bit 7 is set (the
 *     fog word has it clear), bit 6 is set (the light samples' word 0x80000080u | (l << 8) has it clear), bit 5 is set (SKR_LENS_CTR3 =
 *     0x800000C0u has it clear), bits 0-4 are clear (never the jitter word 0xFFFFFFFF).  u = u31_to_unit(out[0]); tau = S * u is one
 *     binary32 multiply; out[1..3] are unused.
 *   - The displaced centres: for this sample sphere i has the centre
 *         c'_i = (fmaf(tau, v_i.x, c_i.x), fmaf(tau, v_i.y, c_i.y), fmaf(tau, v_i.z, c_i.z)),
 *     one correctly rounded fused multiply-add per component — a stated exception to "not contracted", as fma2 is where the spec names
 *     it.  r^2 is unchanged.  A sphere with v_i = 0 keeps c_i up to the sign of a zero.
 *   - The sample: the radiance of sample (pixel, aa) is what the renderer returns for that pixel, aa and seed on the static scene whose
 *     sphere i has the centre c'_i.  Untouched: the primary ray and its jitter draw; child rays, GI draws, light samples, cone
 *     decisions and triangle shadows; the specular view vector toward cam_pos; the acceptance window 1 < t; "origin inside a sphere =>
 *     miss"; the shadow rule "any sphere with 1 < t < inf"; the AA sum and its divide, and progressive_passes.  The whole tree under
 *     one primary sample sees one tau.  Triangles, lights and the camera do not move.
 *   - Keys: tau depends only on (pixel word, aa, seed), and the pixel word of a query ray is its key.  So skr_shade_rays with keys
 *     y * width + x and sample = aa on a scene with motion in force gives that sample of the frame, bit for bit.  skr_camera_rays is
 *     unchanged.  skr_trace_rays answers for the scene at rest (tau = 0).
 *   - Where it runs: a launch with motion in force always takes the general level pipeline; skr_kernel_variant() carries one "_motion"
 *     part behind the light part ("level_pipeline_g1_motion", "level_pipeline_g1_soft_motion_tshadow", "shade_rays_g1_motion", ...).
 *     It combines with use_shadows, grid_size, num_path_traces at any depth, SKR_SCN_STRICT, shade_triangles with or without triangle
 *     shadows, spot lights, light radii, tiles and strides, clones, skr_multi / skr_comm, progressive and adaptive frames.
 *   - Refused with SKR_ERR_UNSUPPORTED where motion is in force (and only there): skr_options.legacy_reflect, fog volumes, the
 *     sphere-tree switch, a lens with A > 0, and skr_render_denoised_host / skr_render_adaptive_denoised_host (guides at rest would
 *     sharpen what the shutter blurs, as under a lens).
 * set: a value that is not finite, S < 0, or n != the sphere count: SKR_ERR_ARG and the scene is unchanged.  get: *n = the sphere
 * count, v (if not NULL) receives v[n][3].  A renderer takes velocities and shutter when it is created; skr_renderer_clone and the
 * multi-GPU frame steps carry them. */
#define SKR_SCN_MOTION 32u
#define SKR_SHUTTER_CTR3 0x800000E0u
int skr_scene_set_sphere_velocities(skr_scene *scene, const float *v, int32_t n);
int skr_scene_get_sphere_velocities(const skr_scene *scene, float *v, int32_t *n);
int skr_scene_set_shutter(skr_scene *scene, float shutter);
int skr_scene_get_shutter(const skr_scene *scene, float *shutter);
/* Environment map: an image-based background and GI light (new, opt-in; no counterpart in the reference, whose misses return one
 * constant colour).  A scene may carry an environment: a square image of E x E RGB binary32 texels T[j][i], 1 <= E <= SKR_ENV_MAX_EDGE,
 * every texel finite.  The environment is in force iff the scene has one.  The rule (normative):
 *   - Where it is read.  With the environment in force every ray for which shade() would return scene.background (raytrace.h:189-192)
 *     returns env(d) instead, d that ray's direction as traced: a frame's primary ray (under a lens: d'), a --gillum child ray at any
 *     level, a shading query's ray, including one whose winner lies at or beyond tmax.  A ray that a triangle blackens
 *     (raytrace.h:221-224) stays black.  Shadow rays and the direct light loop do not read the environment: it lights surfaces only
 *     through --gillum children.  All work counters are those of the same frame with a constant background.
 *   - env(d): an octahedral map with world +y at the centre of the square, filtered bilinearly, clamped at the square's border.
 *     Everything is binary32, each step one correctly rounded operation, nothing contracted, no transcendental function:
 *       1. s = (|dx| + |dy|) + |dz|.  If !(s > 0) or s is not finite, env(d) is the scene's background (a zero direction, a NaN, an
 *          overflow, infinities).
 *       2. px = dx / s, pz = dz / s.
 *       3. If dy < 0 (a -0 is not < 0): qx = (1 - |pz|) * sgn(px), qz = (1 - |px|) * sgn(pz), sgn(x) = x < 0 ? -1 : +1.  Otherwise
 *          qx = px, qz = pz.
 *       4. u = qx * 0.5f + 0.5f, v = qz * 0.5f + 0.5f.
 *       5. x = u * (float) E - 0.5f, x0 = floorf(x), fx = x - x0, i0 = clamp((int) x0, 0, E - 1), i1 = clamp((int) x0 + 1, 0, E - 1);
 *          likewise y, y0, fy, j0, j1 from v.
 *       6. Per channel: top = T[j0][i0] + fx * (T[j0][i1] - T[j0][i0]); bot the same on row j1; env = top + fy * (bot - top).
 *     So env depends on d only up to a power-of-two scale; a map whose texels all equal a finite colour c returns c exactly (c = -0
 *     gives +0), and a map holding the scene's background is the frame it was; with E = 1 every lookup is texel (0, 0).
 *   - Where it runs: a launch with the environment in force always takes the general level pipeline, frames the direct kernel or the
 *     node pipeline would otherwise render included; skr_kernel_variant() carries one "_env" part at its end
 *     ("level_pipeline_g1_env", "level_pipeline_g1_soft_lens_tshadow_env", "shade_rays_g1_env", ...).  It combines with use_shadows,
 *     grid_size, num_path_traces at any depth, SKR_SCN_STRICT, shade_triangles with or without triangle shadows, spot lights, light
 *     radii, motion, a lens, tiles and strides, bands, clones, skr_multi / skr_comm, progressive and adaptive frames, shading queries.
 *   - Refused with SKR_ERR_UNSUPPORTED where the environment is in force (and only there): skr_options.legacy_reflect, fog volumes,
 *     the sphere-tree switch, and skr_render_denoised_host / skr_render_adaptive_denoised_host (their guides hold one class for every
 *     miss: the filter would smear the backdrop).  skr_denoise on caller-supplied guides stays as it is.
 * set: texels float[edge][edge][3], row j first; edge == 0 or NULL texels clears the environment; an edge outside
 * [1, SKR_ENV_MAX_EDGE] or a texel that is not finite: SKR_ERR_ARG and the scene is unchanged.  get: *edge = E (0: none), texels (if
 * not NULL) receives float[E][E][3].  A renderer takes the environment when it is created (an allocation of its own beside the scene
 * blob); skr_renderer_clone and the multi-GPU frame steps share it. */
#define SKR_ENV_MAX_EDGE 4096
int skr_scene_set_environment(skr_scene *scene, const float *texels, int32_t edge);
int skr_scene_get_environment(const skr_scene *scene, float *texels, int32_t *edge);
/* Sphere textures: an image albedo on an octahedral map of the shading normal (new, opt-in; no counterpart in the reference, whose
 * `material` line gives every sphere one flat colour).  A scene holds 0 <= n_tex <= SKR_TEX_MAX textures; texture k is a square image of
 * E_k x E_k RGB binary32 texels, 1 <= E_k <= SKR_TEX_MAX_EDGE, every texel finite, row j first as for the environment.  Every sphere
 * has a texture index x_i in [-1, n_tex), -1 (the default) = none.  Textures are in force for a launch iff some x_i >= 0; otherwise
 * planning, skr_kernel_variant(), frames, floats and all work counters are exactly what they are without this section.  The rule
 * (normative):
 *   - tex_k(N) is steps 1-6 of the environment rule above applied to d = N with E = E_k and T = texture k: the axes are the world's,
 *     +y at the centre of the square, the map turns with nothing.  Where step 1 fails (!(s > 0) or s not finite: a zero or NaN
 *     normal) tex_k(N) = (1, 1, 1).  The kernels compute it by the environment's own index code (wave_common.h env_taps).
 *   - Where it is read.  At a node whose surface is sphere i with x_i = k >= 0, c = tex_k(N), N the node's shading normal as the
 *     kernel holds it: normalize3(P - centre), under motion the displaced centre.  The material rows of that node become
 *     kd' = (kd.x c.x, kd.y c.y, kd.z c.z) and ambp' = (ambp.x c.x, ambp.y c.y, ambp.z c.z, ambp.w), ambp = {La * ka, power}: one
 *     binary32 multiply each.  ks, the exponent and the ior are unchanged.  Every use of that node's kd and ambp takes the primed
 *     values: the diffuse and ambient terms of the light loop, and the final `* kd` of raytrace.h:213.  Triangles have no texture.
 *     Rays, hits, child rays, draws, shadow rays and all work counters are those of the same scene without textures.
 *   - Where it runs: a launch with textures in force always takes the general level pipeline; skr_kernel_variant() carries one "_tex"
 *     part at its very end, behind "_env" where that is present ("level_pipeline_g1_tex", "level_pipeline_g1_soft_lens_tshadow_env_tex",
 *     "shade_rays_g1_env_tex", ...).  It combines with use_shadows, grid_size,
 *     num_path_traces at any depth, SKR_SCN_STRICT, shade_triangles with or without triangle shadows, spot lights, light radii,
 *     motion, a lens, the environment, tiles and strides, bands, clones, skr_multi / skr_comm, progressive and adaptive frames,
 *     shading queries.  skr_trace_rays is unaffected.
 *   - Refused with SKR_ERR_UNSUPPORTED where textures are in force (and only there): skr_options.legacy_reflect, fog volumes, the
 *     sphere-tree switch, and skr_render_denoised_host / skr_render_adaptive_denoised_host (their guides hold one class per sphere:
 *     the filter would smear the pattern).
 * SKR_SCN_TEXTURE (`raytracer --scn-texture`; combines with the other scene flags): a line `texture NAME` sets the texture in force
 * for the `sphere` lines that follow, stateful exactly as `velocity` and `material` are; `texture none` clears it; the initial state
 * is none.  NAME is a colour PFM read by skr_read_pfm, a relative name resolved against the scene file's directory; the same NAME
 * twice is one texture.  A line without a name, whose file cannot be read, is not square, has an edge above the limit or a texel that
 * is not finite, or that would be a 17th distinct texture, is warned about, skipped and counted in n_unknown, the texture in force
 * unchanged.  Without the flag the line stays "WARNING. Do not know command" and everything is byte for byte as it was.
 * add: texels float[edge][edge][3]; returns the new texture's index, or -SKR_ERR_ARG (a bad edge, a texel that is not finite, a 17th
 * texture), the scene unchanged.  get: *edge = E_k, texels (if not NULL) receives float[E_k][E_k][3].  set_sphere_textures: n must be
 * the sphere count and every index in [-1, n_tex), else SKR_ERR_ARG and the scene is unchanged.  get_sphere_textures: *n = the sphere
 * count, idx (if not NULL) receives it.  clear: every index back to -1 (the textures stay).  A renderer takes textures and indices
 * when it is created (an allocation of its own beside the scene blob); skr_renderer_clone and the multi-GPU frame steps share it. */
#define SKR_SCN_TEXTURE 64u
#define SKR_TEX_MAX 16
#define SKR_TEX_MAX_EDGE 1024
int skr_scene_add_texture(skr_scene *scene, const float *texels, int32_t edge);
int skr_scene_get_texture(const skr_scene *scene, int32_t k, float *texels, int32_t *edge);
int skr_scene_texture_count(const skr_scene *scene);
int skr_scene_set_sphere_textures(skr_scene *scene, const int32_t *idx, int32_t n);
int skr_scene_get_sphere_textures(const skr_scene *scene, int32_t *idx, int32_t *n);
int skr_scene_clear_textures(skr_scene *scene);
/* Emissive spheres: surfaces that glow (new, opt-in; no counterpart in the reference, whose `material` line holds no such term).
 * Every sphere has an emission e_i = (r, g, b), default (0, 0, 0); every component is finite and >= 0.0f (-0.0f passes that test and is
 * stored as given: x + (-0) = x).  Emission is in force for a launch iff some component of some sphere is > 0; otherwise planning,
 * skr_kernel_variant(), frames, floats and all work counters are exactly what they are without this section.  The rule (normative):
 *   - Where it is added.  With emission in force every shade() whose winner is sphere i, at depth > 0, returns v + e_i, v what it
 *     returned before: raytrace.h:213 under num_path_traces > 0 (--gillum), :218 without.  The add is one correctly rounded binary32 add
 *     per component, after the multiply by kd and not contracted with it.  It applies to primary rays, under a lens and under motion
 *     (emission belongs to the sphere index, not to a place), to --gillum children at any level, and to shading queries.
 *     shade(depth 0) stays (0, 0, 0) (:142-145).  A triangle has no emission.  A texture on the sphere primes kd and the ambient row as
 *     before and leaves e_i alone.
 *   - What emission is not.  The light loop and shadow rays do not know emitters: an emitter lights other surfaces only through
 *     --gillum children that hit it, and is itself shaded and casts shadows like any sphere.  Rays, hits, child rays, draws, shadow
 *     rays and all four work counters are those of the same scene without emission.
 *   - Where it runs: a launch with emission in force always takes the general level pipeline; skr_kernel_variant() carries one "_emit"
 *     part at its very end, behind "_env" and "_tex" where those are present ("level_pipeline_g1_emit",
 *     "level_pipeline_g1_soft_lens_tshadow_env_tex_emit", "shade_rays_g1_emit", ...).  It combines with everything textures combine
 *     with: use_shadows, grid_size, num_path_traces at any depth, SKR_SCN_STRICT, shade_triangles with or without triangle shadows, spot
 *     lights, light radii, motion, a lens, the environment, textures, tiles and strides, bands, clones, skr_multi / skr_comm,
 *     progressive and adaptive frames, shading queries — and with skr_render_denoised_host / skr_render_adaptive_denoised_host
 *     (emission is constant per sphere: the guides' one class per sphere still describes the surface).  skr_trace_rays is unaffected.
 *   - Refused with SKR_ERR_UNSUPPORTED where emission is in force (and only there): skr_options.legacy_reflect, fog volumes and the
 *     sphere-tree switch.
 * SKR_SCN_EMISSION (`raytracer --scn-emission`; combines with the other scene flags): a line `emission r g b` sets the emission in
 * force for the `sphere` lines that follow, stateful exactly as `velocity` and `material` are; `emission 0 0 0` ends it; the initial
 * state is (0, 0, 0).  A line without three finite numbers >= 0 is warned about, skipped and counted in n_unknown, the emission in force
 * unchanged.  Without the flag the line stays "WARNING. Do not know command" and everything is byte for byte as it was.
 * set: rgb float[n][3], n the sphere count; a wrong n, a value that is not finite or a negative value returns SKR_ERR_ARG and leaves
 * the scene unchanged; rgb == NULL or n == 0 clears the emission.  get: *n = the sphere count, rgb (if not NULL) receives
 * float[n][3], zeros where none was set.  skr_scene_create_from_arrays scenes start with no emission.  A renderer takes the emission
 * when it is created (an allocation of its own beside the scene blob); skr_renderer_clone and the multi-GPU frame steps share it. */
#define SKR_SCN_EMISSION 128u
int skr_scene_set_sphere_emission(skr_scene *scene, const float *rgb, int32_t n);
int skr_scene_get_sphere_emission(const skr_scene *scene, float *rgb, int32_t *n);
/* The sphere tree as a renderer uploads it (built on demand, whatever the switch says).  chunk_size spheres at most per chunk; the
 * first *n_always chunks hold the always-tested spheres (no culling sphere); the other chunks hold consecutive spheres of the Morton
 * order and lie under a depth-first, skip-linked 8-ary tree of *n_nodes nodes.  device_spheres[n_spheres][4] = {centre, r^2} in device
 * order, file_index[n_spheres] = their indices in the file; node_spheres[n_nodes][5] = {centre, R^2, kappa}: a line o + t d may hold a
 * candidate below the node only if |(C - o) x d|^2 <= (R^2 + kappa |C - o|^2) |d|^2 in the device's binary32 (NaN: it may);
 * node_links[n_nodes][4] = {skip, first chunk, chunk count (height-1 nodes only, else 0), smallest file index below};
 * chunk_spheres[n_chunks][5] likewise (the always-tested chunks: R^2 = inf), chunk_links[n_chunks][3] = {smallest file index, first
 * device sphere, sphere count}; ball = {centre, radius}.  Any pointer may be NULL; the counts are returned first so the caller can size
 * the arrays.  Used by the host-logic tests. */
int skr_scene_get_sphere_tree_data(const skr_scene *scene, int32_t *chunk_size, int32_t *n_nodes, int32_t *n_chunks, int32_t *n_always,
								   float *device_spheres, int32_t *file_index, float *node_spheres, int32_t *node_links, float *chunk_spheres,
								   int32_t *chunk_links, float ball[4]);
void skr_scene_destroy(skr_scene *scene);
int skr_scene_get_info(const skr_scene *scene, skr_scene_info *info);
/* Copy the parsed arrays back out in the skr_scene_create_from_arrays layouts
 * (any pointer may be NULL).  Used by the loader parity tests. */
int skr_scene_get_arrays(const skr_scene *scene, float *spheres, float *triangles, float *point_lights);
/* The culling data the triangle walk of raytrace.h:171-186 runs on, as uploaded:
 * device_tris[n_triangles][12] = {v0, 0, v1-v0, file index (int32 bits), v2-v0, 0} in device (Morton) order; chunk_spheres[n_chunks][8]
 * = {centre, R^2, axis / kappa, R_tight^2} of every *chunk_size consecutive device triangles (R_tight applies to
 * rays with (d . axis / kappa)^2 >= d . d; axis = 0 and R_tight = R where there is none); above them a tree in
 * depth-first order, node_spheres[n_nodes][8] likewise and node_links[n_nodes][4] = {skip (index of the next node
 * that is not below this one), first chunk, chunk count (height-1 nodes only, else 0), height}.  level 0..2
 * selects the R built for ray directions up to 4 / 32 / 256 long (the launcher picks by camera and --fov).  Any
 * pointer may be NULL; the counts are returned first so the caller can size the arrays.  Used by the host-logic
 * tests. */
int skr_scene_get_culling(const skr_scene *scene, int32_t level, int32_t *chunk_size, int32_t *n_nodes, int32_t *n_chunks,
						  float *device_tris, float *node_spheres, int32_t *node_links, float *chunk_spheres);
/* The same arrays for the trace tree: the tree the ray queries and the triangle-shadow walk run on, built for rays that start anywhere
 * in ball = {centre, radius} (device_tris and the counts are those of skr_scene_get_culling).  Used by the host-logic tests. */
int skr_scene_get_trace_culling(const skr_scene *scene, int32_t level, int32_t *chunk_size, int32_t *n_nodes, int32_t *n_chunks,
								float *device_tris, float *node_spheres, int32_t *node_links, float *chunk_spheres, float ball[4]);
/* The shadow masks the level pipelines' shadow walk runs on (DESIGN.md "Shadow masks"), as uploaded: per point light a cube map of
 * 6 x cells x cells uint32_t, masks[light][face][i][j], face = 2 axis + (negative), bit k = sphere k may stop a shadow ray of that light
 * whose direction from the shading point towards the light falls in the cell; they hold for shading points P with
 * fl(|Lp - P|^2) <= *reach2.  *n_lights = 0 where the scene has none (no sphere, more than 32, a directional light).  Any pointer may be
 * NULL; the counts are returned first so the caller can size the array.  Used by the host-logic tests. */
int skr_scene_get_shadow_masks(const skr_scene *scene, int32_t *n_lights, int32_t *cells, float *reach2, uint32_t *masks);
/* The GI masks the node pipeline's closest-hit walk of GI children runs on (DESIGN.md "GI masks"), as uploaded: *n_words uint32_t words
 * (0 = the scene has none: no sphere, more than 32, triangles); the masks start at word *mask_word, uint16_t entries (uint32_t where
 * *wide), 6 x dir_cells x dir_cells of them per origin cell, addressed like the shadow masks.  grids[2][8] = the fine and the coarse
 * origin grid: lo.xyz, 1 / cell edge, the cell counts n.xyz and the grid's first index word (as floats); index word
 * base + (k n1 + j) n0 + i = the origin cell's row of masks, -1 = none.  Any pointer may be NULL.  Used by the host-logic tests. */
int skr_scene_get_gi_masks(const skr_scene *scene, int32_t *n_words, int32_t *mask_word, int32_t *wide, int32_t *dir_cells, float *grids, uint32_t *table);

/* Materials of the triangles of a scene built from arrays, materials[n_triangles][10] = ambient(3) diffuse(3) specular(3)
 * phong power — what the `material` line in force gives a `triangle` line in a .scn file (scene.cpp:110-137; the reference
 * keeps no material for a triangle, shapes.h:26).  Read by skr_options.shade_triangles only; default: material.h:9-17's. */
int skr_scene_set_triangle_materials(skr_scene *scene, const float *materials);

/* Index of refraction of every sphere of a scene built from arrays, ior[n_spheres] (material.h:16; the 14th number of a
 * `material` line, scene.cpp:110-137).  Read by skr_options.legacy_reflect only; default 1. */
int skr_scene_set_sphere_ior(skr_scene *scene, const float *ior);

/* ---- options: replaces Options' in-class defaults (utils.h:28-33) ---- */
void skr_options_default(skr_options *opt);
/* R = W*H*max(1,g*g)*sum_{k<depth} N^k: number of shade() calls with depth > 0
 * (SURVEY.md §8d); the metric's numerator. */
uint64_t skr_radiance_ray_count(const skr_options *opt);

/* ---- device ---- */
int skr_device_count(void);
/* Uploads the SoA scene to HBM of `device`. */
int skr_renderer_create(const skr_scene *scene, int device, skr_renderer **out);
/* A second renderer for the same scene on the same device with its own scratch tables: what a second frame in flight needs (the
 * pipelined frame steps make one themselves).  It shares the uploaded scene and the work counters with `src`, which must outlive it. */
int skr_renderer_clone(const skr_renderer *src, skr_renderer **out);
void skr_renderer_destroy(skr_renderer *r);

/* The hot path: replaces the loop nest main.cpp:125-197 (== :36-85) and every
 * shade() call under it, for image rows owned by this caller.
 *
 * Rows are grouped in row tiles of `tile_rows` rows; this call renders tiles
 * first_tile, first_tile + tile_stride, ... (the interleaved partition used to
 * shard a frame over GPUs: rank r of G passes first_tile = r, tile_stride = G).
 * Output is compact and tile-major: the k-th rendered tile occupies rows
 * [k*tile_rows, (k+1)*tile_rows) of d_rgb (W*3 bytes per row, quantised exactly
 * like main.cpp:205: (unsigned char)(std::min(1.0f, c) * 255)); rows of a final
 * partial tile beyond the image are left untouched.  d_rgbf, if not NULL,
 * receives the unquantised float3 image in the same layout (tests).
 * Both are DEVICE pointers.  stream is a hipStream_t (NULL = default stream).
 * Random numbers are keyed by the global pixel index, so the image does not
 * depend on the partition. */
int skr_render_tiles(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, uint32_t first_tile,
					 uint32_t tile_stride, uint8_t *d_rgb, float *d_rgbf, void *stream);
/* The same for an explicit list of tiles: slot k of the compact output (rows k*tile_rows ..) holds tile d_tiles[k] — a DEVICE array
 * of n_slots tile indices, 0xFFFFFFFF = an empty slot (its rows are left untouched).  What the multi-GPU frame steps render with
 * once the tiles are dealt by cost instead of by `t mod G`. */
int skr_render_tile_list(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, const uint32_t *d_tiles, uint32_t n_slots,
						 uint8_t *d_rgb, float *d_rgbf, void *stream);
/* Per tile of tile_rows image rows, the work it costs, counted: the tile is rendered on its own and its rays, shaded hits and
 * ray-sphere tests (skr_renderer_read_work) are priced in flops as bench.py prices a frame.  The numbers behind the multi-GPU tile
 * map; integer counts of a bit-reproducible render, so every rank of a job gets the same ones.  Synchronous (one small render per
 * tile); the renderer's work counters are preserved.  h_cost has ceil(height / tile_rows) entries. */
int skr_tile_costs(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, uint64_t *h_cost);
/* Number of tiles / output rows skr_render_tiles will produce for this partition. */
uint32_t skr_tile_count(const skr_options *opt, uint32_t tile_rows, uint32_t first_tile, uint32_t tile_stride);
/* Contiguous rows [y0, y1) (one tile of y1-y0 rows starting at y0). */
int skr_render_rows(skr_renderer *r, const skr_options *opt, uint32_t y0, uint32_t y1, uint8_t *d_rgb, float *d_rgbf,
					void *stream);
/* The two steps of the progressive mean, for callers that want to look at it while it forms (`raytracer --progressive K
 * --progressive-every M`): d_acc = d_frame (first != 0) or d_acc + d_frame over n_floats binary32 values; then
 * d_rgbf = d_acc / (float) passes and d_rgb = its quantised bytes for a whole width x height frame.  DEVICE pointers. */
int skr_accumulate(float *d_acc, const float *d_frame, uint64_t n_floats, int first, void *stream);
int skr_resolve_accumulated(const float *d_acc, uint32_t passes, uint32_t width, uint32_t height, uint8_t *d_rgb, float *d_rgbf, void *stream);
/* Work counters accumulated by the kernels since the last reset (synchronous):
 * out[0] radiance rays = shade() calls with depth > 0, out[1] sphere hits shaded,
 * out[2] shadow rays (one per light per hit; the reference casts each twice). */
int skr_renderer_read_counters(skr_renderer *r, uint64_t out[3], int reset);
/* The same plus out[3] = ray-sphere tests as the reference runs them: every sphere for a radiance ray
 * (raytrace.h:152-165), up to and including the first occluder for a shadow ray (utils.h:52-55).  The
 * numerator of bench.py's FP32-VALU roofline; asserted equal to the oracle's count. */
int skr_renderer_read_work(skr_renderer *r, uint64_t out[4], int reset);
/* The work (as skr_renderer_read_work counts it) of the ONE kernel skr_renderer_kernel_ms times, in the last launch made with kernel
 * timing on: the counters are copied on the launch stream in front of and behind that kernel, outside the timed window.  Do not
 * reset the counters between that launch and this call.  Synchronous. */
int skr_renderer_kernel_work(skr_renderer *r, uint64_t out[4]);
/* The triangle walks count what they execute only while this is on (off at creation): counting costs the dragon walk ~19 %, so a
 * measurement takes its counts from frames rendered for that purpose and its times from frames rendered without. */
int skr_renderer_count_triangle_work(skr_renderer *r, int enable);
/* What the triangle walks did while counting since the last reset (synchronous; read it BEFORE resetting the counters above): out[0] culling-sphere
 * tests and out[1] ray-triangle tests (utils.h:181-213) the kernels executed — lanes that needed the test, counted by the walks
 * themselves —, out[2] the ray-triangle tests the reference's loop runs for the same rays (raytrace.h:171-186: every triangle for
 * every radiance ray).  bench.py prices mesh scenes with out[0] and out[1]; out[2] / out[1] is what the exact culling saves. */
int skr_renderer_read_triangle_work(skr_renderer *r, uint64_t out[3], int reset);
/* The same for the sphere tree's walks (skr_scene_set_sphere_tree), counted only while skr_renderer_count_triangle_work is on: out[0]
 * culling-sphere tests and out[1] ray-sphere tests the walks executed, lanes that needed the test (a pair of shadow rays counts each
 * ray).  What the reference's loops run for the same rays is skr_renderer_read_work out[3]. */
int skr_renderer_read_sphere_tree_work(skr_renderer *r, uint64_t out[2], int reset);
/* The SKR_* development switches (kernel variant, budgets: DESIGN.md) are read from the environment
 * once, at skr_renderer_create; this reads them again (tests and A/B tools change them between frames). */
int skr_renderer_reload_switches(skr_renderer *r);
/* Time the dominant kernel of each launch with HIP events recorded on the launch stream (off by
 * default).  skr_renderer_kernel_ms() waits for the launches made since the last call and returns
 * their mean duration in ms and their number: what bench.py's roofline is computed from. */
int skr_renderer_kernel_timing(skr_renderer *r, int enable);
int skr_renderer_kernel_ms(skr_renderer *r, float *mean_ms, int32_t *launches);
/* Number of primary sphere hits the last launch (its last band) queued as level-0 nodes / parents for the
 * --gillum kernels (0 if that launch had no --gillum tree); synchronous. */
int skr_renderer_last_parent_count(skr_renderer *r, uint32_t *n);
/* Number of level-1 sphere hit records the last launch (its last band) queued (node pipeline;
 * 0 for the other kernel variants and at depth 2); synchronous. */
int skr_renderer_last_level1_count(skr_renderer *r, uint32_t *n);
/* Frames of one camera share their primary stage: where a --gillum frame takes the node pipeline without --jsample, the primary hits,
 * the pixels of the rays that hit no sphere and their counted work depend on the scene, the camera, the image and the tile selection
 * but not on the seed, so a renderer keeps them from one frame and the next frame under the same options (another seed, another
 * pass of a progressive or adaptive render) starts behind them.  Images and work counters are what they are without it.  This
 * returns how many frames of `r` built that stage and how many reused it (either pointer may be null); SKR_PRIMARY_CACHE=0 turns
 * the reuse off.  A tile table in caller memory (skr_render_tile_list) is never assumed unchanged: such frames always build. */
int skr_renderer_primary_cache_stats(skr_renderer *r, uint64_t *builds, uint64_t *replays);
/* Whole frame into HOST memory (W*H*3 bytes), synchronous; what the CLI uses. */
int skr_render_frame_host(skr_renderer *r, const skr_options *opt, uint8_t *h_rgb, float *kernel_ms);
/* The same with the float frame as a second output (h_rgb or h_rgbf may be NULL, not both) and — under
 * opt->progressive_passes = K > 1 — a look at the mean while it forms: after every `every` passes and after the last one the
 * mean so far is resolved into the host buffers and `progress(user, passes_done, K, h_rgb, h_rgbf)` is called (the place where
 * the SDL viewer of main.cpp:183-197 blits; a non-zero return stops the render with that mean in the buffers).  every == 0 or
 * progress == NULL: one call at the end / none.  The final buffers never depend on `every`.  kernel_ms: device time, summed. */
typedef int (*skr_progress_fn)(void *user, uint32_t passes_done, uint32_t passes, const uint8_t *h_rgb, const float *h_rgbf);
int skr_render_progressive_host(skr_renderer *r, const skr_options *opt, uint32_t every, uint8_t *h_rgb, float *h_rgbf,
								skr_progress_fn progress, void *user, float *kernel_ms);

/* ---- multi-GPU: the frame sharded over the GPUs of one node ----
 * Replaces the reference's only parallel entry, `generate_rays_parallel` (main.cpp:19-104: `#pragma omp parallel for`
 * over the rows at :33, dispatched at main.cpp:402-410) — the reference has no distributed path.
 * The framebuffer is cut into tiles of tile_rows rows and the tiles are dealt to the ranks: tile t to rank t mod G, unless the counted
 * work of the tiles (skr_tile_costs) says that leaves the heaviest rank above 1.10 of the mean — then longest-processing-time-first
 * over those costs (skr_shard_plan; SKR_SHARD=interleave / lpt in the environment forces one or the other).  Every rank renders its
 * tiles (skr_render_tile_list) straight
 * into its slot of a gather buffer, ONE RCCL all-gather over xGMI brings the slots together and rank 0 de-interleaves on the device.
 * The image does not depend on G or on the map (the RNG is keyed by the global pixel).  RCCL is bound at run time;
 * skr_rccl_available() says whether it could be. */
int skr_rccl_available(void);
/* (a) ONE process, N devices (ncclCommInitAll; a renderer, a stream and a worker thread per device).
 * devices == NULL: devices 0 .. n_devices-1.  What `raytracer --gpus N` uses. */
typedef struct skr_multi skr_multi;
int skr_multi_create(const skr_scene *scene, int n_devices, const int *devices, skr_multi **out);
void skr_multi_destroy(skr_multi *m);
int skr_multi_device_count(const skr_multi *m);
skr_renderer *skr_multi_renderer(skr_multi *m, int i); /* device i's renderer (counters, timing); owned by m */
/* Synchronous.  *d_frame: the W*H*3 frame in device 0's memory (owned by m, valid until the next call);
 * frame_ms: first launch to de-interleaved frame, on the root's stream. */
int skr_multi_render_frame(skr_multi *m, const skr_options *opt, uint32_t tile_rows, uint8_t **d_frame, float *frame_ms);
int skr_multi_render_frame_host(skr_multi *m, const skr_options *opt, uint32_t tile_rows, uint8_t *h_rgb, float *frame_ms);
/* The pipelined form (throughput of a run of frames; what skr_comm_render_frame_async is to shape (b)): frame f's all-gather and
 * de-interleave go to a second stream per device while the render streams take frame f + 1 into the other of two buffer sets.
 * Returns once frame f is enqueued; *d_prev_frame = the PREVIOUS call's frame, complete (NULL on the first call; pass NULL not to
 * wait for it).  skr_multi_flush waits for everything in flight; *d_frame = the last frame. */
int skr_multi_render_frame_async(skr_multi *m, const skr_options *opt, uint32_t tile_rows, uint8_t **d_prev_frame);
int skr_multi_flush(skr_multi *m, uint8_t **d_frame);
/* (b) one process PER device (torchrun, mpirun): rank 0 makes an id, the caller broadcasts it by whatever transport
 * it has, every rank creates its communicator on its renderer's device.  id == NULL with world == 1: no RCCL at all. */
#define SKR_COMM_ID_BYTES 128
typedef struct skr_comm skr_comm;
int skr_comm_unique_id(uint8_t id[SKR_COMM_ID_BYTES]);
int skr_comm_create(skr_renderer *r, int device, const uint8_t id[SKR_COMM_ID_BYTES], int rank, int world, skr_comm **out);
void skr_comm_destroy(skr_comm *c);
/* Asynchronous on `stream`: this rank's tiles, the all-gather, rank 0's de-interleave.  *d_frame: rank 0's finished
 * frame (device memory owned by c; NULL on the other ranks) once the stream has drained. */
int skr_comm_render_frame(skr_comm *c, const skr_options *opt, uint32_t tile_rows, uint8_t **d_frame, void *stream);
/* The frame step with its collective off the render stream (throughput of a run of frames): frame f's all-gather and
 * de-interleave run on a stream the communicator owns while `stream` renders frame f + 1 into the other of two buffer sets.
 * *d_prev_frame (rank 0; NULL elsewhere and on the first call): the PREVIOUS call's frame, complete in `stream` order after
 * this call (pass d_prev_frame = NULL not to look at it: one stream wait less per frame).  skr_comm_flush ends the run: `stream` waits for the last collective, *d_frame = the last frame.  Every frame is
 * the one skr_comm_render_frame would have produced. */
int skr_comm_render_frame_async(skr_comm *c, const skr_options *opt, uint32_t tile_rows, uint8_t **d_prev_frame, void *stream);
int skr_comm_flush(skr_comm *c, uint8_t **d_frame, void *stream);
/* Rank 0: waits for `stream` and copies that frame to host memory (W*H*3 bytes). */
int skr_comm_frame_to_host(skr_comm *c, uint8_t *h_rgb, void *stream);
/* The partition itself (host logic, no GPU): padded tiles per rank, and the de-interleave of a rank-major gathered
 * buffer [world][tiles_per_rank * tile_rows][W*3] into frame[H][W*3]. */
uint32_t skr_shard_tiles_per_rank(int32_t height, uint32_t tile_rows, uint32_t world);
int skr_shard_deinterleave_host(const uint8_t *gathered, uint8_t *frame, int32_t width, int32_t height, uint32_t tile_rows, uint32_t world);
/* Maps: slot_of_tile[t] = rank * k_max + slot (k_max = skr_shard_tiles_per_rank) for n_tiles tiles of cost[t] each.
 * skr_shard_lpt: most expensive tile first, each to the least loaded rank with a free slot; a rank's tiles sit in its slots in image
 * order; deterministic.  skr_shard_by_cost: the rule of the frame steps — tile t to rank t mod world unless that leaves the heaviest
 * rank above 1.10 of the mean cost, then skr_shard_lpt.  skr_shard_plan: the map a frame step of `world` ranks uses for this renderer
 * and these options (skr_tile_costs + the rule).  skr_shard_deinterleave_map_host: the de-interleave under such a map. */
int skr_shard_lpt(const uint64_t *cost, uint32_t n_tiles, uint32_t world, uint32_t *slot_of_tile);
int skr_shard_by_cost(const uint64_t *cost, uint32_t n_tiles, uint32_t world, uint32_t *slot_of_tile);
int skr_shard_plan(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, uint32_t world, uint32_t *slot_of_tile);
int skr_shard_deinterleave_map_host(const uint8_t *gathered, uint8_t *frame, int32_t width, int32_t height, uint32_t tile_rows, const uint32_t *slot_of_tile);

/* ---- ray queries (new; DESIGN.md "Ray queries"): caller-supplied rays traced against a renderer's scene ----
 * The hit rule is the renderer's own closest hit under skr_options.shade_triangles:
 *   - a sphere is accepted when 1 < t < inf (raytrace.h:152-165); t is the binary64 near root the renderer computes (utils.h:87-110);
 *   - a triangle is accepted when utils.h:181-213 passes with t > 0 and its file index is not the ray's ignore_triangle;
 *   - the smallest t wins; a triangle wins against a sphere only with a strictly smaller t; among triangles with equal t the lower
 *     file index wins;
 *   - a winner with t >= tmax makes the result a miss; fog volumes are not surfaces.
 * n is the shading normal of the general level pipeline: normalize(P - C) with P = o + d t (sphere), normalize(cross(v1 - v0, v2 - v0))
 * turned against d (triangle).  Rays with a non-finite or zero-length direction get an unspecified result; they never change
 * the results of other rays.  Neither call changes anything a render or a counter reads (work counters, kernel timing,
 * skr_kernel_variant). */
typedef struct {              /* 32 bytes, two float4; DEVICE arrays of it are 16-byte aligned */
	float o[3];
	float tmax;               /* hits with t >= tmax are ignored; +inf = no limit */
	float d[3];               /* need not be unit length; t is in units of d, as in the renderer */
	int32_t ignore_triangle;  /* file index of a triangle this ray may not hit (the surface it leaves), -1 = none */
} skr_ray;

typedef struct {              /* 32 bytes */
	float t;                  /* +inf on a miss */
	int32_t kind;             /* 0 miss, 1 sphere, 2 triangle */
	int32_t index;            /* sphere index / triangle file index, -1 on a miss */
	float n[3];               /* shading normal of the hit (see above); 0 on a miss */
	int32_t reserved[2];      /* 0 */
} skr_hit;

#define SKR_TRACE_ANY_HIT 1u
/* Trace n rays (DEVICE array) against the renderer's scene, asynchronously on `stream` (a hipStream_t, NULL = default stream).
 * flags = 0: d_out is a DEVICE skr_hit[n] (16-byte aligned).  SKR_TRACE_ANY_HIT: d_out is a DEVICE int32_t[n]: 1 exactly where the
 * closest-hit result would not be a miss, else 0.  n == 0: SKR_OK, nothing is launched.  Null pointers, misaligned arrays and
 * unknown flags: SKR_ERR_ARG. */
int skr_trace_rays(skr_renderer *r, const skr_ray *d_rays, uint32_t n, uint32_t flags, void *d_out, void *stream);
/* The primary rays of sample `sample` of a frame with options `opt` (the AA index, < grid_size^2; 0 with grid_size == 0, the pixel
 * centres) into a DEVICE skr_ray[height][width]: o = the camera position, d = bit for bit the direction the renderer traces for that
 * pixel and sample (main.cpp:140-182), tmax = +inf, ignore_triangle = -1.  Asynchronous on `stream`.  Where the renderer's scene has a
 * lens with an aperture > 0 (skr_scene_set_lens): (o', d') of that rule for (opt, sample), keyed to opt->seed. */
int skr_camera_rays(skr_renderer *r, const skr_options *opt, uint32_t sample, skr_ray *d_rays, void *stream);

/* ---- shading queries (new): the radiance of caller-supplied rays, what shade() returns for them ----
 * Radiance of n caller-supplied rays (DEVICE skr_ray[n], 16-byte aligned) under options opt, asynchronously on `stream`.
 * d_rgbf: DEVICE float[n][3], the unquantised value shade() returns for each ray (what a 1-spp frame's float output holds).
 * d_keys: DEVICE uint32_t[n] or NULL (= ray index): the counter RNG's pixel word for each ray; `sample` is its AA word.
 *   - Shading rule: the renderer's own, for opt's monte_carlo, num_path_traces, max_depth, use_shadows, seed, shade_triangles and
 *     legacy_reflect, and for the scene's fog volumes and triangle-shadow switch as the renderer took them.  The result does not depend on width, height, fov, grid_size or
 *     progressive_passes.
 *   - Specular view: as everywhere in the renderer (blinn_phong.h), the view vector of the specular term points to the SCENE CAMERA,
 *     not to the ray's origin.
 *   - Counter RNG: ray i is keyed (pixel = d_keys ? d_keys[i] : i, aa = sample, node 0); its GI and fog draws are then exactly those of
 *     frame pixel `key` at AA sample `sample`.  So skr_camera_rays(opt, s) with keys y * width + x reproduces the frame's sample s,
 *     bit for bit.
 *   - tmax: the winner the frame's rule picks for the first segment is found first — the closest sphere at 1 < t, or a triangle that
 *     blackens (shade_triangles = 0) or is shaded (shade_triangles = 1) under the mode's own triangle rule.  If its t is >= tmax the
 *     ray is a miss and returns the background.  With tmax = +inf this is exactly the frame's rule.  tmax does not apply to child rays.
 *   - ignore_triangle: honoured under shade_triangles, as the from_triangle of the first segment (what a --gillum child has).
 *     Without shade_triangles it is not read: no ray the renderer traces in that mode carries one.
 *   - Counters: the work counters (skr_renderer_read_counters: rays, hits, shadow rays) advance exactly as a render of those rays
 *     would.  Nothing a later render reads is changed.  skr_kernel_variant() names the shading path.
 *   - Errors: n == 0: SKR_OK, nothing is launched.  SKR_ERR_ARG: null or misaligned arrays, bad options.  As skr_render_tiles
 *     returns them: a tree over 2^32 node ids, fog with legacy_reflect or shade_triangles, tables over the scratch budget
 *     (SKR_ERR_UNSUPPORTED).  Rays with a non-finite or zero direction get an unspecified result for that ray only; they never
 *     fault and never change another ray's result. */
int skr_shade_rays(skr_renderer *r, const skr_options *opt, const skr_ray *d_rays, uint32_t n, uint32_t sample, const uint32_t *d_keys, float *d_rgbf,
                   void *stream);

/* ---- denoiser (new): an edge-aware filter for Monte-Carlo frames ----
 * A spatial a-trous wavelet filter with edge-stopping weights (Dammertz 2010) and SVGF's luminance-variance guidance (Schied 2017)
 * without its temporal part.  All arithmetic is binary32 + - * / max, not contracted, divide correctly rounded, taps summed in order:
 *   - Guides: skr_hit[height][width], the first hits of the pixel-centre camera rays of the frame's options (grid_size = 0, sample 0)
 *     traced by skr_trace_rays.  Class of a pixel: a miss is one class, each sphere index one, all triangles together one.
 *   - Luminance l = 0.2126 r + 0.7152 g + 0.0722 b, left to right.
 *   - Init: var_p = max(0, m2 - m1 * m1), m1 and m2 the means of l and l * l over the same-class in-image pixels of the 3x3 window
 *     (row-major).
 *   - Iteration i = 0 .. iterations - 1, s = 2^i: over the taps (dy, dx) in {-2..2}^2, row-major, q = p + s (dx, dy) in the image:
 *     w = 0 where q's class differs from p's, else w = h * wn * wz * wl in that order, with h = k[dx+2] * k[dy+2],
 *     k = {1/16, 1/4, 3/8, 1/4, 1/16}; wn = max(0, n_p . n_q)^128 (seven squarings); wz = D / (D + |t_p - t_q|) with
 *     D = SIGMA_Z * t_p * (s * max(|dx|, |dy|)), 1 at the centre tap; wn = wz = 1 for a miss; wl = V / (V + (l_p - l_q)^2) with
 *     V = SIGMA_L^2 * var_p + EPS.  c'_p = sum w c_q / sum w per channel, var'_p = sum w^2 var_q / (sum w)^2; a pixel whose weights
 *     sum to no positive number (non-finite input) keeps its colour and variance.
 *   - Output: the float frame after the last iteration and its bytes, quantised exactly as a frame is.
 */
#define SKR_DENOISE_SIGMA_L 4.0f
#define SKR_DENOISE_SIGMA_Z 0.05f
#define SKR_DENOISE_EPS 1e-6f
#define SKR_DENOISE_ITERATIONS 5       /* the default of the CLIs and of Renderer.denoise */
#define SKR_DENOISE_MAX_ITERATIONS 16
/* Filter the DEVICE float frame d_rgbf[height][width][3] guided by the DEVICE d_hits[height][width] (16-byte aligned) into
 * d_out_rgbf (float[height][width][3]) and / or d_out_rgb (uint8_t[height][width][3]): either may be NULL, not both.  Asynchronous
 * on `stream`.  iterations 0 .. SKR_DENOISE_MAX_ITERATIONS; 0: the output is the input, bit for bit.  No whole-frame neighbours, no
 * filter: there is no tiled or multi-GPU form.  Scratch (4 x 16 + 4 bytes a pixel) is the renderer's, grown on demand and kept.
 * SKR_ERR_ARG: null or misaligned arrays, an output that overlaps an input or the other output, a size outside 1 .. 65536, iterations
 * out of range.  Touches no work counter, no kernel timing and not skr_kernel_variant(). */
int skr_denoise(skr_renderer *r, uint32_t width, uint32_t height, const float *d_rgbf, const skr_hit *d_hits, uint32_t iterations, float *d_out_rgbf,
                uint8_t *d_out_rgb, void *stream);
/* The whole frame, denoised, into HOST memory (h_rgb W*H*3 bytes and / or h_rgbf W*H*3 floats; either may be NULL, not both):
 * the frame's float output (the mean of opt->progressive_passes passes), the guides skr_trace_rays(skr_camera_rays(opt with
 * grid_size = 0, sample 0)), then skr_denoise.  Synchronous.  kernel_ms: device time of the whole sequence. */
int skr_render_denoised_host(skr_renderer *r, const skr_options *opt, uint32_t iterations, uint8_t *h_rgb, float *h_rgbf, float *kernel_ms);

/* ---- adaptive sampling (adaptive.hip): extra passes only for the pixels whose estimate is still noisy ----
 * The rule (normative):
 *   - Pass k of pixel p (k = 0, 1, ...): v_k, the float frame pixel of opt with seed = opt->seed + k (uint64 wrap-around); with
 *     grid_size g > 0 the frame's own value, its g^2 AA samples summed in sample order and divided by (float) g^2.
 *   - Luminance l_k = 0.2126f * r + 0.7152f * g + 0.0722f * b, left to right (the denoiser's).
 *   - Running sums in binary32, in pass order, not contracted: C = v_0, then C + v_k per channel (skr_accumulate's order);
 *     S1 = sum l_k and S2 = sum (l_k * l_k) in the same order.
 *   - Convergence after n passes, tested only when n >= max(2, min_passes) and threshold >= 0: nf = (float) n, m = S1 / nf,
 *     d = S2 / nf - m * m, var = d > 0 ? d : 0, e2 = var / (nf - 1), b = threshold * (m > SKR_ADAPTIVE_LUM_FLOOR ? m :
 *     SKR_ADAPTIVE_LUM_FLOOR); converged iff e2 <= b * b.  Divides are correctly rounded.  A negative threshold: nothing converges.
 *   - Pixel p gets pass n iff n < min_passes, or n < max_passes and it has not converged after n passes (a pixel the test has not
 *     run on counts as not converged; a converged pixel never resumes).  So its pass count n_p lies in [min_passes, max_passes].
 *   - Outputs: mean_p = C / (float) n_p per channel (as skr_resolve_accumulated divides), its bytes quantised as a frame's are,
 *     passes[p] = n_p.
 *   - min_passes == max_passes == K is opt->progressive_passes = K bit for bit; a negative threshold is K = max_passes.
 * Limits: 1 <= min_passes <= max_passes <= SKR_ADAPTIVE_PASS_LIMIT, threshold not NaN (+inf: every pixel stops at
 * max(2, min_passes)), reserved 0; anything else SKR_ERR_ARG. */
#define SKR_ADAPTIVE_LUM_FLOOR 0.00390625f /* 2^-8: dark pixels stop on absolute noise */
#define SKR_ADAPTIVE_MIN_PASSES 8          /* the defaults of skr_adaptive_default, the CLIs and Renderer.render_adaptive */
#define SKR_ADAPTIVE_MAX_PASSES 64
#define SKR_ADAPTIVE_THRESHOLD 0.05f
#define SKR_ADAPTIVE_PASS_LIMIT 65535      /* the largest max_passes */
typedef struct {
	int32_t min_passes, max_passes;
	float threshold;  /* relative standard error of a pixel's mean luminance at which it stops */
	int32_t reserved; /* 0 */
} skr_adaptive;
void skr_adaptive_default(skr_adaptive *a);
/* The whole frame under the rule above into DEVICE outputs: d_rgb uint8_t[H][W][3], d_rgbf float[H][W][3] (the means),
 * d_passes uint32_t[H][W] (n_p); any may be NULL, not all three.  opt->progressive_passes must be <= 1 (SKR_ERR_ARG).  The option
 * errors of skr_render_tiles apply.  SYNCHRONOUS: after the first min_passes whole frames it reads back one 4-byte count of the
 * still-active pixels per round (at most max_passes - min_passes rounds), so it cannot be captured in a graph.  Each round gives
 * the active pixels one more pass, as a whole frame or as shading queries of just those pixels, whichever costs less; both give the
 * same bits.  The work counters advance by the work done.  Scratch is the renderer's, grown on demand and kept. */
int skr_render_adaptive(skr_renderer *r, const skr_options *opt, const skr_adaptive *a, uint8_t *d_rgb, float *d_rgbf, uint32_t *d_passes, void *stream);
/* The same into HOST memory (h_rgb W*H*3 bytes, h_rgbf W*H*3 floats, h_passes W*H uint32; any may be NULL, not all three).
 * kernel_ms: device time of the whole sequence, as skr_render_progressive_host reports it. */
int skr_render_adaptive_host(skr_renderer *r, const skr_options *opt, const skr_adaptive *a, uint8_t *h_rgb, float *h_rgbf, uint32_t *h_passes, float *kernel_ms);

/* ---- adaptive frames, denoised under each pixel's measured variance (new) ----
 * The adaptive sampler knows the variance of every pixel's mean luminance; the denoiser takes it in place of its spatial estimate,
 * which cannot tell noise from signal.  The rule (normative), all binary32 + - * / max, not contracted, divides correctly rounded,
 * in the order written:
 *   - Variance of the mean, of a pixel with final state S1, S2, n: n < 2: var_p = -1.0f ("not measured").  Otherwise the
 *     expressions of the convergence test: nf = (float) n, m = S1 / nf, d = S2 / nf - m * m, v = d > 0 ? d : 0,
 *     var_p = v / (nf - 1): the e2 the pixel was stopped on.  A NaN pass gives 0, as the stopping rule does.
 *   - Denoiser init with a variance image d_var[H][W]: pixel q is measured iff d_var[q] >= 0 (false for NaN and negatives).  An
 *     unmeasured pixel p takes skr_denoise's init value, the same-class 3x3 max(0, m2 - m1 * m1), unchanged.  A measured p takes
 *     var0_p = (sum g * d_var[q]) / (sum g) over the in-image, same-class, measured q of the 3x3 window in row-major order,
 *     g = {1/16, 1/8, 1/16; 1/8, 1/4, 1/8; 1/16, 1/8, 1/16}: each term sum += g * d_var[q], then one divide (the centre is always
 *     in: sum g > 0).  SVGF's 3x3 variance pre-filter, applied once.
 *   - Iterations, output and iterations == 0: skr_denoise's, with SIGMA_L = SKR_DENOISE_VAR_SIGMA_L (SIGMA_Z, EPS and the taps
 *     are skr_denoise's).  The two sigmas are equal, so d_var == NULL or an image with no measured pixel gives skr_denoise's
 *     output bit for bit.  A +inf entry is measured: that pixel keeps its value (no positive weight). */
#define SKR_DENOISE_VAR_SIGMA_L 4.0f
/* skr_render_adaptive plus d_var float[H][W], the variance of each pixel's mean luminance under the rule above; any output may be
 * NULL, not all four.  skr_render_adaptive is this with d_var = NULL. */
int skr_render_adaptive_var(skr_renderer *r, const skr_options *opt, const skr_adaptive *a, uint8_t *d_rgb, float *d_rgbf, uint32_t *d_passes, float *d_var,
                            void *stream);
/* skr_denoise with the DEVICE variance image d_var float[height][width] (4-byte aligned; NULL: skr_denoise itself).  skr_denoise's
 * contract and errors; d_var must not overlap an output either.  Touches no work counter, no kernel timing and not
 * skr_kernel_variant(). */
int skr_denoise_var(skr_renderer *r, uint32_t width, uint32_t height, const float *d_rgbf, const skr_hit *d_hits, const float *d_var, uint32_t iterations,
                    float *d_out_rgbf, uint8_t *d_out_rgb, void *stream);
/* The whole sequence into HOST memory: skr_render_adaptive_var (the float means, the variance, the pass counts), the guides exactly
 * as skr_render_denoised_host takes them (skr_trace_rays(skr_camera_rays(opt with grid_size = 0, sample 0))), then skr_denoise_var.
 * h_rgb W*H*3 bytes and h_rgbf W*H*3 floats: the filtered frame; h_passes W*H uint32: the adaptive pass counts; any may be NULL,
 * not all three.  The option and argument errors of both halves apply.  Synchronous.  kernel_ms: device time of the whole sequence. */
int skr_render_adaptive_denoised_host(skr_renderer *r, const skr_options *opt, const skr_adaptive *a, uint32_t iterations, uint8_t *h_rgb, float *h_rgbf,
                                      uint32_t *h_passes, float *kernel_ms);

/* ---- image file: replaces the inline writer main.cpp:199-211 ---- */
int skr_write_ppm(const char *path, uint32_t width, uint32_t height, const uint8_t *rgb);
/* Other outputs (new; `raytracer --format ppm|png|pfm`).  PNG: the same bytes as the PPM, 8-bit RGB (stored
 * deflate blocks: no compressor is linked).  PFM: the unquantised float frame, "PF\nW H\n-1.0\n" + binary32 RGB, bottom row
 * first; rgbf is top row first like every buffer of this interface. */
int skr_write_png(const char *path, uint32_t width, uint32_t height, const uint8_t *rgb);
int skr_write_pfm(const char *path, uint32_t width, uint32_t height, const float *rgbf);
/* The inverse of skr_write_pfm (new; `raytracer --envmap FILE.pfm`): a colour "PF" file, either sign of the scale line (negative:
 * little-endian, positive: big-endian; its magnitude is not applied).  *width, *height: the sizes; rgbf (if not NULL) receives
 * height * width * 3 floats, TOP row first, so that reading what skr_write_pfm wrote gives the buffer back bit for bit; NULL: the
 * sizes only.  A file that is no colour PFM, has a size < 1, a scale of 0 or not finite, or ends early: SKR_ERR_IO with a text.
 * Row j of an environment (skr_scene_set_environment) is row j of this array. */
int skr_read_pfm(const char *path, uint32_t *width, uint32_t *height, float *rgbf);

/* ---- diagnostics ---- */
const char *skr_last_error(void);      /* thread-local text of the last failure */
const char *skr_kernel_variant(void);  /* name of the kernel the last render launched */
/* Device-side evaluation of the arithmetic spec for unit tests: op selects
 * 0 philox(ctr4,key2 -> out4 u32), 1 sincos(phi -> s,c), 2 powf(x,p),
 * 3 smallest_root(a,b,c), 4 triangle test (o,d,v0,v1,v2 -> hit,t),
 * 5 quantise(c -> u8 as u32), 6 basis(n -> nt,nb), 7 (a,b -> sqrtf(a), a/b), 8 philox at 10 rounds (op 0: the 7 the draws use),
 * 9 (hi16 -> mismatch counts of the short exact sqrt, 1/x, x/pi, x/pdf forms against the correctly rounded expansions over the
 * 65536 binary32 values with those high 16 bits), 10 exp_spec (binary64 x as lo, hi words -> exp(x) likewise), 11 the fog term
 * (40 words: [0..2] radius absorption scattering, [4..6] albedo, [8..10] L, [11] intensity, [12..14] light colour, [15] pass
 * (0 diffuse, 1 specular), [16..18] sphere centre, [19] fog index, [20..22] light position, [23] light index, [24..26] kd, [27] pixel,
 * [28..30] N, [31] node, [32] aa, [33..34] seed lo, hi; the rest 0 -> colour(3), no-interaction probability).  in/out are DEVICE pointers
 * to n records of the op's input/output width in 32-bit words.
 *
 * Ops 12..16 evaluate the filtered sphere predicates (device_math.h) and the selection code on top of them (shade_common.h,
 * wave_common.h) through the functions the render kernels call (tests/test_filtered_predicates_gpu.py).  A sphere row is
 * {centre.xyz, r*r}.  They run whole waves: a lane past the last record evaluates a copy of it and writes nothing.
 * 12 bracket: (o(3), d(3), row(4)) -> sphere_bracket {accept, lo, hi, b, D}, then the same five words of bracket_from_ec on the row
 *    {e, c} skr_camec_kernel forms for origin o.  lo, hi are NaN for a non-candidate (D < 0, b >= 0, NaN), the binary32 bracket
 *    where binary32 decided (also for a certain reject), lo == hi == t2 where the exact form decided and accepted.
 * 13 pair bracket: (o(3), d0(3), d1(3), row(4)) -> per slot {candidate, accept, lo, hi, b, D}: pair_closest_step, the per-sphere
 *    body of closest_pair_deferred (make_pair, pair_bD, pair_bracket, bracket_decide, best_update), on one sphere.
 * 14 pair any-hit: (P(3), L0(3), L1(3), row(4)) -> per slot {candidate, occluded}: pair_any_step, the per-sphere body of
 *    occluded_pair (pair_bD, pair_any_m, any_decide), on one sphere; the rays start at P + 1e-6 (utils.h:45), which the op adds.
 * 15, 16 take a scene at the head of the input: [0] ns (<= 64), [1..3] 0, then 80 rows of 4 words (the ns spheres, the rest 0:
 *    the pad rows the sphere loops ask for), then n records (o(3), d0(3), d1(3)).
 * 15 ec tables: -> per record ns + 8 rows {o - centre, |o - centre|^2 - r*r} (skr_camec_kernel's rows for a camera at o; the
 *    last 8 rows are left as they are: pass them zeroed).
 * 16 selection: the input of op 15, the records padded to a multiple of 4 words, then the output of op 15 -> 22 words:
 *    {index, t} of closest_sphere(d0), (d1), closest_sphere_from(d0), (d1) on the record's ec table, closest_pair_deferred<false> slot 0,
 *    slot 1 (t = near_root_exact of the slot's b, D), closest_sphere_exact(d0), (d1); then {occ0, occ1, tests} of occluded_pair<false>
 *    and of occluded_pair<true> from P = o.  index -1, t +inf: no sphere accepted.  The scene view is the one trace_rays.hip builds:
 *    every table in global memory, no masks.
 * Ops 13 and 14 call the very functions the two loops call per sphere, with `second` set and neither ray occluded yet.  The loops
 * themselves run in op 16 (closest_pair_deferred<false>, both occluded_pair forms, with rays on either side of `sane` in the two
 * slots) and in the frames of the same test file; the masked walks (closest_pair_deferred<true>, occluded_pair with shadow masks:
 * masked_rows) run only in those frames.
 * 17 the spot-light cone (SKR_SCN_SPOT above; shade_common.h spot_cone, the function the light loop calls): (a(3), c1, c2, L(3))
 *    -> {f, outside}: f as a float (0 where outside), outside 0 / 1.  (Ops 12..16 were taken when spot lights came.)
 * 18 the sample of a light with a radius (skr_scene_set_light_radii above; shade_common.h soft_sample, the function the light loop calls):
 *    (pixel, aa, node, l, seed_lo, seed_hi, Lp(3), R), 10 words -> Lp'(3).  R == 0: Lp itself.
 * 19 the hit root (device_math.h near_root, the function the kernels take a hit's t from): (2a, b, D) -> 7 words: near_root, near_root_exact (the
 *    binary64 form of utils.h:87-110), 1 where near_root took the binary64 form (else 0), then the interval lo, hi and the pair q_h, q_l
 *    of the binary32 form (meaningful only where the operands are in its ranges; word 2 is 1 for every record outside them).
 * 20 the Phong power as the kernels call it (device_math.h powf_spec, tests/test_shading_values_gpu.py): (x, p, steps as an integer)
 *    -> {powf_spec<false>(x, p, steps), powf_spec<true>(x, p, steps)}: the instance that reads RenderParams::pow_steps and the one
 *    the shaped leaf instances compile in, which is right only for integer p <= 127 (op 2 is the first at steps = 11).
 * 21 (hi16 -> mismatch counts of len_terms<true>'s len, inv, inv2 and len_terms<false>'s inv against sqrtf(ss), 1.0f / len and
 *    1.0f / (len * len) in the correctly rounded expansions, over the 65536 binary32 values with those high 16 bits; as op 9).
 * 22 the lens sample and ray (skr_scene_set_lens above; wave_common.h lens_ray, the function the camera kernels call), laid out as op 18
 *    is: (pixel, aa, seed_lo, seed_hi, A, k, cam_pos(3), cam_right(3), cam_up(3), d(3)), 18 words -> (lx, ly, o'(3), d'(3)), 8 words.
 *    (Ops 20 and 21 were taken when the lens came.)
 * 23 the Phong power of the shaped leaf instance compiled for an exponent mask (device_math.h pow_int_sparse; csrc/launch.h
 *    SKR_LEAF_POW_MASKS): (x, p, mask as an integer) -> one word, right for every integer p inside the mask and for every p that is
 *    not plain; 0xFFFFFFFF for a mask that has no instance.
 * 24 the shutter time and a displaced centre (skr_scene_set_sphere_velocities above; wave_common.h shutter_time and shade_common.h
 *    MovingCentres::centre, the functions the kernels of a launch with motion call): (pixel, aa, seed_lo, seed_hi, S, c(3), v(3)),
 *    11 words -> (tau, c'(3)), 4 words.
 * 25 the environment lookup's taps (skr_scene_set_environment above; wave_common.h env_taps, the index code env_lookup itself runs):
 *    (d(3), E as an integer), 4 words -> (flag: 1 = the background arm, i0, i1, j0, j1 as integers, fx, fy), 7 words; the six
 *    behind a flag of 1 are 0.
 * 26 the texture colour of a normal (skr_scene_add_texture above; render_generic.hip texture_colour, the function textured_material
 *    multiplies the material rows by): (N(3), texture index k), 4 words -> c(3), 3 words, on the op's own fixed textures: texture k
 *    (0 <= k < 4) has the edge (1, 2, 3, 64)[k] and the texel (row j, column i) = (i + 1, j + 1, 0.5 (i + j) + 0.25); any other k is
 *    no texture, c = (1, 1, 1). */
int skr_debug_eval(int op, const void *d_in, void *d_out, uint32_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SKR_H */
