// Host side of a render launch, shared by the translation units of libskr: the launch entry points, and the plan that decides once
// per launch which kernels render it and how the scratch of a level pipeline is cut (skr_plan_launch, render_kernel.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "render_params.h"

// The level-0 stage of the node pipeline (skr_primary_kernel: the primary hits as nodes, the final pixels of the rays that hit no sphere,
// its share of the work counters) reads neither the seed nor the AA index where grid_size == 0, so frames of one camera share it:
//   RUN     the primary kernel, nothing kept (several bands, --jsample, triangle work counted, SKR_PRIMARY_CACHE=0);
//   BUILD   the primary kernel, which also records each output pixel's class and its counter sums in the scratch;
//   REPLAY  no primary kernel: the level-0 tables and their count are still in the scratch, skr_primary_replay_kernel emits the pixels
//           that are no node and adds the recorded sums.
enum { SKR_LEVEL0_RUN = 0, SKR_LEVEL0_BUILD, SKR_LEVEL0_REPLAY };
// the class of an output pixel (one byte each at NodePlan::off_cls)
enum { SKR_PIX_NONE = 0, SKR_PIX_NODE, SKR_PIX_BACKGROUND, SKR_PIX_TRIANGLE }; // NONE: no pixel of the image (an empty tile slot, a row past the height)

// The plan of one band of the node pipeline (render_nodes.hip): table sizes for the worst case, every pixel a node, every child a hit.
constexpr int SKR_NODE_LEVELS_MAX = 33;
struct NodePlan {
	bool wide = false;       // the launch's hit records are 32 bytes and carry their ray (SKR_WIDE_RECORDS below)
	bool flat = false;       // the flat schedule (render_nodes.hip nodes_flat_wanted): the leaves' hits are a record level of their own
	int levels = 0;          // node / record levels 0 .. max_depth - 2 (flat: .. max_depth - 1)
	uint32_t band_nblk = 0;  // 16x16 pixel blocks per band
	uint64_t nodes_max[SKR_NODE_LEVELS_MAX] = {};
	uint32_t cap[SKR_NODE_LEVELS_MAX] = {};
	size_t off_nodes[SKR_NODE_LEVELS_MAX] = {}, off_shade[SKR_NODE_LEVELS_MAX] = {}, off_recs[SKR_NODE_LEVELS_MAX] = {}, off_res[SKR_NODE_LEVELS_MAX] = {}, off_ixh[SKR_NODE_LEVELS_MAX] = {};
	size_t off_ctr = 0, ctr_bytes = 0, total = 0, banded = 0;
	size_t off_cls = 0, off_sums = 0; // the kept level-0 stage (PrimaryKey): a class byte per output pixel of the band; the primary kernel's work counters, shard by shard
	size_t off_girow = 0;             // ... and a word per level-0 node: its row of GI masks (RenderParams::gi_row0)
	int level0 = SKR_LEVEL0_RUN; // how this launch gets its level-0 nodes (api.cpp render_pass decides; the plan itself says SKR_LEVEL0_RUN)
	size_t lds_leaf = 0;     // the leaf kernel's workgroup LDS: the scene + the per-wave rings and windows
	size_t lds = 0;          // the largest workgroup LDS among the schedule's kernels (flat: skr_scene_kernels_lds; persistent: lds_leaf)
};

// The plan of one band of the general level pipeline (render_generic.hip).
constexpr int SKR_GLEVELS_MAX = 64;
struct GPlan {
	int levels = 0;            // traced levels 1 .. levels (= --depth)
	uint32_t band_rows = 0;    // output rows per band
	uint64_t nodes_max[SKR_GLEVELS_MAX + 1] = {}; // worst case: roots of the band; then every ray of the level above a hit
	uint32_t cap[SKR_GLEVELS_MAX + 1] = {};       // records per region
	size_t off_nodes[SKR_GLEVELS_MAX + 1] = {}, off_recs[SKR_GLEVELS_MAX + 1] = {}, off_res[SKR_GLEVELS_MAX + 1] = {}, off_hdr[SKR_GLEVELS_MAX + 1] = {};
	size_t off_ctr = 0, ctr_bytes = 0, total = 0;
};

// The trees a wave of query rays may walk (wave_common.h pick_query_tree), under the renderer's switches (api.cpp
// query_trees).  Both trees are SKR_CULL_LEVELS sets of `stride` rows.
struct QueryTrees {
	const float4 *tree;  // the renderer's chunk tree, its first set: it holds for rays that start at the scene camera or on a surface
	const float4 *trace; // the trace tree (skr_scene::trace_chunks), its first set; null: none
	uint32_t stride;
	int32_t nchunks;     // nodes of either tree; 0 = every triangle (no mesh, SKR_NO_CULL)
	int32_t cones, trace_cones; // the renderer tree's and the trace tree's
	float4 ball;         // {centre, radius}: the trace tree holds for rays that start in it
};

// The lens of a scene with an aperture (include/skr.h skr_scene_set_lens; wave_common.h lens_ray): what the kernels that
// form camera rays read — the general level pipeline's trace and activate instances for such a scene, in a kernel argument of their own
// as every feature is, and the camera-ray kernels of the ray queries and the adaptive sampler.  k = A / F, one binary32 division on the
// host.  Level-1 rays under a lens do not start at the scene camera: their waves pick a tree as query rays do (pick_query_tree).
struct Lens {
	float A, k;
	QueryTrees trees; // (the level pipeline's instances only)
};

// The motion of a scene whose spheres move while the shutter is open (include/skr.h skr_scene_set_sphere_velocities, DESIGN.md 8.16;
// wave_common.h shutter_time, shade_common.h MovingCentres): what the general level pipeline's trace and activate instances for a launch
// with motion in force read, in a kernel argument of their own as every feature is.  vel: one row {v.xyz, 0} per sphere in file order,
// an allocation of the renderer's beside the scene blob (the blob's section table stays as it is), with the blob's rows of padding behind.
// Below level 1 and in the shadow walk the rays of such a launch start on displaced surfaces: their waves pick a tree as query rays do
// (pick_query_tree with surface = false).
struct Motion {
	const float4 *vel;
	float S;
	QueryTrees trees;
};

// The environment of a scene that has one (include/skr.h skr_scene_set_environment; wave_common.h env_lookup): what the
// general level pipeline's finalize instances for a launch with the environment in force read — the only kernel that decides a miss — in
// a kernel argument of its own as every feature is.  texels: edge * edge rows {r, g, b, 0}, row j first, an allocation of the
// renderer's beside the scene blob (the blob's section table stays as it is).
struct EnvMap {
	const float4 *texels;
	int32_t edge;
};

// The textures of a scene some sphere of which has one (include/skr.h skr_scene_add_texture; render_generic.hip
// textured_material): what the general level pipeline's activate and finalize instances for a launch with textures in force read, in a
// kernel argument of their own as every feature is.  texels: one allocation for all textures, rows {r, g, b, 0} so that a tap is one
// 16-byte gather, each texture row j first; rows: per sphere in file order {where its texture's texels start, its edge}, edge 0 = none,
// read by per-lane index as the material rows are.  An allocation of the renderer's beside the scene blob.
struct Textures {
	const float4 *texels;
	const uint2 *rows;
};

// The emission of a scene some sphere of which glows (include/skr.h skr_scene_set_sphere_emission; render_generic.hip
// node_value): what the activate and finalize instances for a launch with emission in force read, in a kernel argument of their own as
// every feature is, the last of the pack.  rows: one row {r, g, b, 0} per sphere in file order, read by per-lane index as the texture
// rows are.  An allocation of the renderer's beside the scene blob.
struct Emission {
	const float4 *rows;
};

// A shading query (include/skr.h skr_shade_rays) on the general level pipeline: the rays are its roots, as rows of RenderParams::width
// rays (the last row partial), banded like a frame's rows.  The kernels' second argument (render_generic.hip).
struct ShadeRays {
	const float4 *rays;   // the caller's skr_ray[n]: {o, tmax} {d, ignore_triangle}
	const uint32_t *keys; // the counter RNG's pixel word of each ray, or null (= the ray's index)
	float *out;           // float[n][3]
	uint32_t n, ray0;     // rays in all; the first ray of the band being launched
	QueryTrees trees;
};
// the rays of one row of a shading query's plan
constexpr uint32_t SKR_SHADE_ROW = 1024;

// Triangle shadows (include/skr.h skr_scene_set_triangle_shadows): what the shadow walk of the activate kernel reads.
struct TriShadows {
	QueryTrees trees; // the walk runs on the trace tree's first set (|L| = 1) for a wave whose shadow rays all start in the ball
};

// The optional features of a launch on the general level pipeline (render_generic.hip), decided once per launch (api.cpp
// generic_features) and followed by the plan, the variant's name and the launcher.  Each feature that is on is a kernel argument of its
// own behind RenderParams, in the one order render_generic.hip with_pack writes down, so that RenderParams — and with it the code of every
// instance without the feature — stays as it was.  Which features exclude which: skr_features_conflict.
struct GenericFeatures {
	bool tri_shadows = false; // triangle shadows are in force: the scene has them switched on, the launch shades triangles and casts shadow rays
	bool sphere_tree = false; // the scene has the sphere tree switched on and at least one sphere (include/skr.h skr_scene_set_sphere_tree)
	bool spot = false;        // the scene has at least one spot light (include/skr.h SKR_SCN_SPOT)
	bool soft = false;        // at least one light of the scene has a radius > 0 (include/skr.h skr_scene_set_light_radii)
	bool lens = false;        // the scene has a lens with an aperture > 0 and the launch is a frame (include/skr.h skr_scene_set_lens); never with a shading query: its rays are the caller's
	TriShadows shadows{};     // (tri_shadows)
	SphereTree stree{};       // (sphere_tree)
	SpotLights spots{};       // (spot or soft; n = 0 where the scene has no spot light)
	SoftLights softs{};       // (soft)
	Lens thin_lens{};         // (lens)
	bool motion = false;      // motion is in force: the shutter is > 0 and some sphere has a velocity other than 0 (include/skr.h skr_scene_set_sphere_velocities); frames and shading queries
	Motion mot{};             // (motion; such a launch always carries spots and softs, n = 0 where the scene has none)
	bool env = false;         // the environment is in force: the scene has one (include/skr.h skr_scene_set_environment); frames and shading queries
	EnvMap envmap{};          // (env; with it the finalize kernel also takes thin_lens where lens is set: a primary miss looks up d')
	bool tex = false;         // textures are in force: some sphere has a texture (include/skr.h skr_scene_add_texture); frames and shading queries
	Textures textures{};      // (tex or emit; such a launch always carries spots and softs, n = 0 where the scene has none)
	bool emit = false;        // emission is in force: some sphere has an emission component > 0 (include/skr.h skr_scene_set_sphere_emission); frames and shading queries
	Emission emission{};      // (emit; such a launch always carries textures, every row's edge 0 where the scene has none, and with them spots and softs)
};

enum SkrPath { SKR_PATH_DIRECT = 0, SKR_PATH_NODES, SKR_PATH_GENERIC };

// Everything render_pass (api.cpp) sizes and checks and the launchers follow, computed once per launch.
struct LaunchPlan {
	SkrPath path = SKR_PATH_DIRECT;
	const char *variant = "direct_v3"; // what skr_kernel_variant() reports
	size_t scratch_bytes = 0;          // the level pipeline's one allocation (RenderParams::node_scratch)
	size_t acc_bytes = 0;              // its AA accumulation image (RenderParams::acc)
	size_t lds_bytes = 0;              // the largest workgroup LDS among the launch's kernels
	size_t off_ctr = 0;                // node pipeline: where the counter block sits in the scratch ...
	int levels = 0;                    // ... and how many node / record levels it counts (0 on the other paths)
	NodePlan nodes;                    // (path == SKR_PATH_NODES)
	GPlan generic;                     // (path == SKR_PATH_GENERIC)
	GenericFeatures features;          // (path == SKR_PATH_GENERIC) what skr_plan_launch was given
};

// the scene SoA every kernel stages into LDS (wave_common.h stage_scene): 4 rows per sphere, a zero row, 2 rows per light
static inline size_t skr_scene_lds_bytes(const RenderParams &p) { return ((size_t) 4 * p.n_spheres + 1 + 2 * p.n_lights) * 16; }

// The workgroup LDS of the kernels that keep only the scene there: the node pipeline's primary, trace, activate and flat shade-leaf
// kernels and the general level pipeline's.  Their dynamic LDS is the scene + 32 bytes; the activate and shade-leaf kernels add the
// prefix sums (SKR_PREFIX_WORDS words of static LDS, ahead of the dynamic LDS on a 16-byte boundary).  The runtime does not refuse a
// launch whose static + dynamic LDS exceeds the device's: on gfx950 such a launch (2 558 spheres under fog: 163 792 + 272 bytes) ran
// and faulted.  So the plans count both.
constexpr size_t SKR_PREFIX_LDS = ((size_t) SKR_PREFIX_WORDS * sizeof(uint32_t) + 15) & ~(size_t) 15;
static inline size_t skr_scene_kernels_lds(const RenderParams &p) { return skr_scene_lds_bytes(p) + 32 + SKR_PREFIX_LDS; }
// the same for the general level pipeline's instances with the sphere tree: only the lights are staged
static inline size_t skr_lights_lds_bytes(const RenderParams &p) { return ((size_t) 1 + 2 * p.n_lights) * 16; }
static inline size_t skr_lights_kernels_lds(const RenderParams &p) { return skr_lights_lds_bytes(p) + 32 + SKR_PREFIX_LDS; }

// children per node of the --gillum tree: N --gillum rays, and under --legacy-reflect 2 per light (the arity of the counter RNG's
// node ids, include/skr.h)
static inline uint32_t skr_tree_arity(const RenderParams &p) { return (uint32_t) (p.monte_carlo ? p.num_path_traces : 0) + (p.legacy_reflect ? 2u * (uint32_t) p.n_lights : 0u); }

// the scratch tables of a level pipeline, one after the other on 256-byte boundaries
struct ScratchLayout {
	size_t off = 0;
	size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t) 255; return o; }
};

// the largest band in [1, all] whose worst-case tables fit the budget (`fits`: they grow with the band); 0: not even a band of 1
template <class Fits>
static uint32_t skr_largest_band(uint32_t all, Fits fits)
{
	if(fits(all)) return all;
	uint32_t lo = 1, hi = all;
	if(!fits(lo)) return 0;
	while(hi - lo > 1)
	{
		const uint32_t mid = lo + (hi - lo) / 2;
		if(fits(mid)) lo = mid;
		else hi = mid;
	}
	return lo;
}

// ---- the node pipeline's trace waves, their headers and their hit regions (render_nodes.hip) ----
// SKR_TRACE_BY_NODE 1: a trace wave holds a block of 64 consecutive nodes, one per lane, and runs over sibling pairs j; its header for
// pair j is row (node >> 6) * PP + j and a node's bit in the ballots is node & 63.  0 (A/B builds): a lane is one sibling pair
// tp = node * PP + j, a wave 64 consecutive pairs: row tp >> 6, bit tp & 63.  Either way a row's wave appends at most 128 hits, to
// region row & 63.  The kernels, the plan and the tests (render_nodes.hip skr_trace_header_map) all ask these functions.
#ifndef SKR_TRACE_BY_NODE
#define SKR_TRACE_BY_NODE 1
#endif
#ifndef SKR_TRACE_RUN
#define SKR_TRACE_RUN 2 // sibling pairs a trace wave runs over before it takes its next block of nodes (0 = all PP of them); measured at PP, 4 and 2: DESIGN.md 5.2
#endif
// A hit record of the node pipeline.  SKR_WIDE_RECORDS 1: 32 bytes, {parent, sphere | child << 16, r1, D} {d.xyz, b} — the record carries
// the ray that found the hit and its b, D of utils.h:116-118 for the sphere it hit, as the trace kernel's walk held them, and whoever
// shades the hit (render_nodes.hip activate_record) forms neither again.  0 (A/B builds): 16 bytes, {parent, sphere | child << 16, r1, r2},
// the ray formed again from its two draws.  Which form a launch's records have is the plan's decision (NodePlan::wide; render_nodes.hip
// plan_bands): the wide one, except where not even one 16x16 block's tables fit the scratch budget with it — such a launch runs the
// instances with 16-byte records, as it did before there were wide ones, and is not refused.  The kernels are compiled for either form
// (template <bool WIDE>) and index the table in rows of skr_rec_rows(WIDE) float4; the plan sizes it with skr_records_bytes: the record
// size is stated here alone.
#ifndef SKR_WIDE_RECORDS
#define SKR_WIDE_RECORDS 1
#endif
__host__ __device__ constexpr int skr_rec_rows(bool wide) { return wide ? 2 : 1; } // float4 per hit record
static inline size_t skr_records_bytes(uint64_t records, bool wide) { return (size_t) records * (size_t) skr_rec_rows(wide) * 16; }
__host__ __device__ static inline uint64_t skr_trace_header_row(uint64_t node, uint32_t j, uint32_t PP)
{
	return SKR_TRACE_BY_NODE ? (node >> 6) * PP + j : (node * PP + j) >> 6;
}
__host__ __device__ static inline uint32_t skr_trace_header_bit(uint64_t node, uint32_t j, uint32_t PP)
{
	return (uint32_t) (SKR_TRACE_BY_NODE ? node : node * PP + j) & 63u;
}
// the header rows that `nodes` nodes of PP sibling pairs use: rows 0 .. this - 1
static inline uint64_t skr_trace_rows_used(uint64_t nodes, uint64_t PP) { return SKR_TRACE_BY_NODE ? (nodes + 63) / 64 * PP : (nodes * PP + 63) / 64; }
// the rows their table holds (4 more: the old mapping's last workgroup writes the headers of all its four waves)
static inline uint64_t skr_trace_rows_alloc(uint64_t nodes, uint64_t PP) { return skr_trace_rows_used(nodes, PP) + 4; }
// records per region: region r receives the hits of the rows = r (mod 64), 128 at most from each
static inline uint64_t skr_trace_region_cap(uint64_t nodes, uint64_t PP) { return (skr_trace_rows_used(nodes, PP) + SKR_P1_REGIONS - 1) / SKR_P1_REGIONS * 128; }

// The launch shape the leaf kernel (render_nodes.hip skr_leaf_kernel2) has an instance for (shade_common.h PointLightShape<1 | 2>), or
// none: the instance that reads every fact at run time.  A shape is picked only where EVERY fact it compiles in equals the launch's value:
// a sphere-only scene with GI masks (the instances are <false, FIRST, true, shape>) of 16-bit entries (at most 16 spheres), shadow rays
// cast through the shadow masks — which exist only for scenes whose lights are all point lights (scene_masks.cpp build_shadow_masks), so no
// light is directional —, every integer Phong exponent below 128, and exactly one or two lights.  SKR_LEAF_SHAPE=0: never.
enum SkrLeafShape { SKR_LEAF_RUNTIME = 0, SKR_LEAF_POINT1 = 1, SKR_LEAF_POINT2 = 2 };
static inline SkrLeafShape skr_leaf_shape(const RenderParams &p)
{
	if(!(p.sw.shadow_mask & SKR_SW_LEAF_SHAPE)) return SKR_LEAF_RUNTIME;
	if(p.n_tris != 0 || p.gi_index == nullptr || p.gi_wide != 0) return SKR_LEAF_RUNTIME;
	if(!p.use_shadows || p.shadow_masks == nullptr) return SKR_LEAF_RUNTIME;
	if(p.pow_steps > 7) return SKR_LEAF_RUNTIME;
	return p.n_lights == 2 ? SKR_LEAF_POINT2 : p.n_lights == 1 ? SKR_LEAF_POINT1 : SKR_LEAF_RUNTIME;
}

// The exponent masks the shaped instances are compiled for (shade_common.h PointLightShape<L, ANY>; device_math.h pow_int_sparse): the
// straight-line pow of an instance forms a product only at the bits of its mask.  SKR_LEAF_POW_FULL, all seven steps, comes first and
// serves every launch with a shape; 0x30 is the exponents 16, 32 and 48 (spheres1.scn, spheres2.scn).  One instance per mask, shape,
// FIRST and record form: a mask is worth its code only for exponents that scenes in use have.
#define SKR_LEAF_POW_MASKS(X) X(0x7Fu) X(0x30u)
constexpr unsigned SKR_LEAF_POW_FULL = 0x7Fu;
// The mask of the instance a launch gets: of the listed masks that cover the OR of its scene's integer exponents (SkrSwitches::pow_any)
// the one with the fewest bits, else the full one; 0: the launch has no shape, and the run-time instance no mask.  SKR_LEAF_POW=0: the
// full mask always.
static inline unsigned skr_leaf_pow_plan(const RenderParams &p)
{
	if(skr_leaf_shape(p) == SKR_LEAF_RUNTIME) return 0u;
	unsigned best = SKR_LEAF_POW_FULL;
	if(!(p.sw.shadow_mask & SKR_SW_LEAF_POW)) return best;
	const unsigned list[] = {
#define X(m) m,
		SKR_LEAF_POW_MASKS(X)
#undef X
	};
	for(unsigned m : list)
		if(((unsigned) p.sw.pow_any & ~m) == 0u && __builtin_popcount(m) < __builtin_popcount(best)) best = m;
	return best;
}

// render_kernel.hip
// lds_limit: the device's workgroup LDS.  A path whose kernels need more is not taken; lp.lds_bytes > lds_limit: no path fits.
// f: the features of the renderer's scene under this launch's options; the sphere tree, spot lights, lights with a radius, a lens, motion, the environment, textures and emission take the general level pipeline
bool skr_plan_launch(const RenderParams &p, size_t lds_limit, LaunchPlan &lp, const GenericFeatures &f); // false: the launch takes a level pipeline and not one band of it fits the budget
// The features a launch cannot combine, given the options as the caller set them: spot lights, lights with a radius and a lens exclude
// --legacy-reflect, fog volumes and the sphere tree; fog excludes --legacy-reflect and --shade-triangles, and with the latter triangle
// shadows; motion excludes what they exclude, and a lens; the environment excludes --legacy-reflect, fog volumes and the sphere tree, and so do
// textures and emission.
// (Lights with a radius need the SpotLights argument: the record always carries it.)  The text for the user, or null.
const char *skr_features_conflict(const GenericFeatures &f, bool legacy_reflect, bool shade_triangles, bool fog);
// what skr_kernel_variant() reports for a frame (query: a shading query) on the general level pipeline; static storage
const char *skr_generic_variant(bool query, const GenericFeatures &f);
hipError_t skr_launch_render(const RenderParams &p, const LaunchPlan &lp, hipStream_t stream, const SkrTimingHook *hook);
hipError_t skr_launch_debug(int op, const void *d_in, void *d_out, uint32_t n, hipStream_t stream);
// render_nodes.hip
bool skr_nodes_plan(const RenderParams &p, size_t lds_limit, NodePlan &pl); // false: the node pipeline does not take this launch
hipError_t skr_launch_nodes(const RenderParams &p, const NodePlan &pl, hipStream_t stream, const SkrTimingHook *hook);
hipError_t skr_nodes_level_count(const void *scratch, size_t off_ctr, int level, uint32_t *n);
// render_generic.hip
bool skr_generic_plan(const RenderParams &p, GPlan &pl, bool sphere_tree = false); // false: not one band fits the budget
// f: the launch's features (the instances with the arguments they name); a combination skr_features_conflict refuses is an invalid value
// q: a shading query (p.width = SKR_SHADE_ROW, p.out_rows its rows, p.aa_index its sample); null: a frame
hipError_t skr_launch_generic(const RenderParams &p, const GPlan &pl, hipStream_t stream, const SkrTimingHook *hook, const GenericFeatures &f, const ShadeRays *q = nullptr);
// render_wave.hip
// Every value the level-0 stage of a node-pipeline launch depends on, and where it is kept: what skr_primary_kernel and plan_for
// (render_nodes.hip) read.  A frame replays the stage only if its key equals, byte for byte, the key the scratch was last built under
// (api.cpp render_pass).  The outputs (rgb, rgbf) are not in it: the nodes carry output-pixel indices, and the replay kernel emits into
// whatever the frame names.
struct PrimaryKey {
	int32_t width, height;
	uint32_t tile_rows, first_tile, tile_stride, out_rows;
	const uint32_t *tile_table; // the table's address says nothing about its contents: ...
	uint64_t tile_table_id;     // ... the identity of its contents, from whoever owns it (multi_gpu.cpp ShardMap::generation)
	float inv_width, inv_height, aspect, angle;
	f3 cam_pos, cam_dir, cam_up, cam_right, background;
	int32_t n_spheres, n_tris, n_lights;
	const float4 *scene, *cam_ec, *tri_chunks; // the scene blob, the camera rows, the chunk tree's level
	int32_t tri_chunk_size, tri_cones, n_tri_chunks;
	int32_t use_shadows, pow_steps, num_path_traces, max_depth, flat, levels;
	const void *gi_index, *gi_surface; // what the stored rows of GI masks were looked up in (null: SKR_GI_MASK=0 / SKR_GI_SURFACE=0)
	uint32_t band_nblk;
	const void *scratch;        // the renderer's allocation, and where the plan puts the stage in it
	const void *counters;
	size_t off_ctr, off_nodes0, off_shade0, off_cls, off_sums, off_girow, total;
};
// false: the launch does not keep its level-0 stage (see SKR_LEVEL0_RUN); tile_table_id: 0 = a table of unknown contents
bool skr_primary_key(const RenderParams &p, const NodePlan &pl, uint64_t tile_table_id, PrimaryKey &key);
hipError_t skr_launch_wave(const RenderParams &p, size_t lds, hipStream_t stream);
hipError_t skr_launch_primary(const RenderParams &p, dim3 grid, size_t lds, hipStream_t stream);
// the same, recording the stage: cls = a byte per output pixel, sums = SKR_COUNTER_SHARDS x 4 words, zeroed here; p.gi_row0 = a word per node
hipError_t skr_launch_primary_build(const RenderParams &p, dim3 grid, size_t lds, uint8_t *cls, unsigned long long *sums, hipStream_t stream);
hipError_t skr_launch_primary_replay(const RenderParams &p, const uint8_t *cls, const unsigned long long *sums, hipStream_t stream);
hipError_t skr_launch_resolve(const RenderParams &p, hipStream_t stream);
hipError_t skr_launch_camec(const float4 *geom, int ns, f3 cam_pos, float4 *out, hipStream_t stream);
// trace_rays.hip: the ray queries (include/skr.h skr_trace_rays, skr_camera_rays).  Not a render: no plan, no counters, no timing.
struct TraceScene {
	const float4 *geom;   // sphere rows {centre, r^2} (HBM; the rows behind them are readable: the blob's padding)
	const float4 *tris;   // device triangles, 3 float4 each (scene_host.h)
	QueryTrees trees;
	int32_t ns, nt, chunk;
	f3 cam;               // the scene camera: the renderer's tree holds for rays that start there
};
// st: the renderer's scene has the sphere tree switched on (the instances whose sphere searches are the tree's walks); null: it has not
hipError_t skr_launch_trace(const TraceScene &s, const float4 *rays, uint32_t n, bool any_hit, void *out, hipStream_t stream, const SphereTree *st = nullptr);
// lens: the scene's lens where its aperture is > 0 (the rays (o', d') of include/skr.h skr_scene_set_lens); null: the pinhole
hipError_t skr_launch_camera_rays(const RenderParams &p, float4 *rays, hipStream_t stream, const Lens *lens = nullptr);
// denoise.hip: the denoiser (include/skr.h skr_denoise).  Not a render: no plan, no counters, no timing.
struct DenoiseScratch {
	float4 *img[2]; // the {r, g, b, var} ping-pong images (img[1] first holds {r, g, b, l})
	float4 *guide;  // {n, t} of every pixel's guide hit
	uint32_t *cls;  // its class: the sphere index, 0xFFFFFFFE for every triangle, 0xFFFFFFFF for a miss
};
// var: null, or the per-pixel variance image of skr_denoise_var (init by skr_dn_init_var_kernel)
hipError_t skr_launch_denoise(const DenoiseScratch &b, uint32_t w, uint32_t h, const float *rgbf, const float4 *hits, const float *var, int iterations,
							  float *out_rgbf, uint8_t *out_rgb, hipStream_t stream);
// accumulate.hip
hipError_t skr_launch_accumulate(float *acc, const float *frame, size_t n, int first, hipStream_t stream);
hipError_t skr_launch_resolve_accumulated(const float *acc, uint32_t passes, uint32_t width, uint32_t out_rows, uint32_t height, uint32_t tile_rows,
										  uint32_t first_tile, uint32_t tile_stride, const uint32_t *tile_table, uint8_t *rgb, float *rgbf, hipStream_t stream);
// adaptive.hip: the adaptive sampler's kernels (include/skr.h skr_render_adaptive)
struct AdaptiveScratch {
	float4 *st;        // per pixel {C.r, C.g, C.b, S1}
	uint2 *st2;        // per pixel {S2 (bits), n}
	uint32_t *list[2]; // the active lists, ping-pong: pixel indices in ascending order
	uint32_t *blocks;  // per workgroup of a selection: its survivors, then their offset
	uint32_t *count;   // the survivors of the last selection (one word)
	float4 *rays;      // the query path: the camera rays of the listed pixels (skr_ray)
	float *shade;      // their radiance at one AA sample [m][3]
	float *sacc;       // the running sum of their AA samples [m][3]
};
struct AdaptiveRule {
	uint32_t min_passes, max_passes;
	float threshold;
};
// an active share at or above this gives the round a whole frame; below it, shading queries of the active pixels
constexpr float SKR_ADAPTIVE_CROSSOVER = 0.5f;
size_t skr_adaptive_scratch_bytes(uint64_t pixels);
AdaptiveScratch skr_adaptive_carve(void *base, uint64_t pixels);
hipError_t skr_launch_adaptive_fold(const AdaptiveScratch &s, const float *frame, const uint32_t *list, uint32_t m, int first, hipStream_t stream);
hipError_t skr_launch_adaptive_select(const AdaptiveScratch &s, const AdaptiveRule &rule, const uint32_t *in, uint32_t m, uint32_t *out, hipStream_t stream);
hipError_t skr_launch_adaptive_rays(const RenderParams &p, const uint32_t *list, uint32_t m, float4 *rays, hipStream_t stream, const Lens *lens = nullptr);
hipError_t skr_launch_adaptive_sample(const AdaptiveScratch &s, const uint32_t *list, uint32_t m, uint32_t sample, uint32_t samples, hipStream_t stream);
// var: null, or the variance image of skr_render_adaptive_var (the second instance of the resolve kernel)
hipError_t skr_launch_adaptive_resolve(const AdaptiveScratch &s, uint64_t pixels, uint8_t *rgb, float *rgbf, uint32_t *passes, float *var, hipStream_t stream);
