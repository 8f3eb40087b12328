// Kernel argument block shared by the launcher (api.cpp) and the kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shadow_cells.h"

struct f3 {
	float x, y, z;
};

#define SKR_COUNTER_SHARDS 4096u
// Counters that thousands of waves hit with atomics sit SKR_PULL_STRIDE uint32 apart (one word sustains only ~88 atomics/us);
// SKR_PULL_QUEUES words of that kind are reserved behind the work counters (api.cpp).
#ifndef SKR_PULL_QUEUES
#define SKR_PULL_QUEUES 16u
#endif
#define SKR_PULL_STRIDE 256u
// the level pipelines append the hit records of a level to SKR_P1_REGIONS regions, one counter each
#define SKR_P1_REGIONS 64u
// the regions' prefix sums (wave_common.h region_prefix), kept in static LDS by the kernels that number a level's records densely
#define SKR_PREFIX_WORDS (SKR_P1_REGIONS + 1u)

// The SKR_* development switches (A/B runs, tests), read from the environment ONCE per renderer (skr_renderer_create,
// skr_renderer_reload_switches) — the launch path never calls getenv.
enum SkrPipeline { SKR_PIPE_AUTO = 0, SKR_PIPE_NODES, SKR_PIPE_GENERIC, SKR_PIPE_OTHER };
struct SkrSwitches {
	int16_t pipeline = SKR_PIPE_AUTO; // SKR_PIPELINE = nodes | generic: which level pipeline takes a --gillum tree (tests, A/B runs)
	uint16_t pow_any = 0x7FF;         // no switch but a host fact of the launch's scene, in the spare half of this word (api.cpp launch_params): the OR of its
	                                  // integer Phong exponents in [1, 1024] (scene_pack.h SceneLayout::pow_any; launch.h skr_leaf_pow_plan)
	int8_t no_cones = 0, no_cull = 0;  // SKR_NO_CONES, SKR_NO_CULL: triangle-walk culling off  (four quarters of one word: the struct stays 20 bytes, so that
	                                   // every field of RenderParams behind it keeps its offset and the kernels that never read the switches their code)
	int8_t primary_cache = 1;          // SKR_PRIMARY_CACHE = 1 | 0: frames of one camera replay the node pipeline's level-0 stage / every frame runs skr_primary_kernel
	int8_t no_sphere_cull = 0;         // SKR_NO_SPHERE_CULL: a renderer on the sphere tree runs the loop over every sphere in every wave (the A/B arm of DESIGN.md 8.10)
	int32_t budget_mb = 0;            // SKR_LEVELS_BUDGET_MB: scratch budget of the level pipelines (0 = default)
	int32_t flat = 0;                 // SKR_FLAT = 1 | 0: the node pipeline's flat schedule forced on (+1) / off (-1); unset: by launch size
	int8_t shadow_mask = 15;          // bit 0: SKR_SHADOW_MASK = 1 | 0: the shadow walk of the level pipelines visits only the spheres the masks name / every sphere;
	                                  // bit 1: SKR_SHADOW_SURFACE = 1 | 0: a shading point on a sphere takes its mask from the surface patches / the direction masks only;
	                                  // bit 2 (SKR_SW_LEAF_SHAPE, a spare bit of this byte): SKR_LEAF_SHAPE = 1 | 0: the leaf kernel's instance with the launch's shape
	                                  // compiled in where there is one (launch.h skr_leaf_shape) / always the instance that reads it at run time (A/B runs, tests)
	                                  // bit 3 (SKR_SW_LEAF_POW): SKR_LEAF_POW = 1 | 0: the shaped instance for the scene's exponent bits (launch.h skr_leaf_pow_plan) /
	                                  // always the one with all seven pow steps (A/B runs, tests)
	int8_t gi_mask = 1;               // SKR_GI_MASK = 1 | 0: the same for the closest-hit walk of the node pipeline's GI children
	int8_t gi_surface = 1;            // SKR_GI_SURFACE = 1 | 0: GI origins on a sphere take their row of masks from the surface patches / the 3D grids only
	int8_t adaptive_path = 0;         // SKR_ADAPTIVE_PATH = frame | query: the path of every adaptive round (+1 / +2); unset: by active share (four quarters of one word, as above)
};

constexpr int SKR_SW_LEAF_SHAPE = 4;
constexpr int SKR_SW_LEAF_POW = 8;
static_assert(sizeof(SkrSwitches) == 20, "SkrSwitches keeps its 20 bytes");

struct RenderParams {
	SkrSwitches sw; // (host side only)
	// image and partition (include/skr.h skr_render_tiles)
	int32_t width, height;
	uint32_t tile_rows, first_tile, tile_stride, out_rows;
	const uint32_t *tile_table; // device, or null: slot k of the compact output holds tile tile_table[k] (0xFFFFFFFF: an empty padding slot) instead of first_tile + k * tile_stride
	uint32_t band_row0, band_rows; // the band of output rows [band_row0, band_row0 + band_rows) a launch of the general level pipeline works on (the whole launch elsewhere)
	// per-frame invariants of main.cpp:134-137, computed once on the host
	float inv_width, inv_height, aspect, angle;
	// camera.h:8-32 (direction/up/right keep the file's magnitudes) and scene.h:24
	f3 cam_pos, cam_dir, cam_up, cam_right, background;
	// SoA scene in HBM (scene_host.h)
	int32_t n_spheres, n_tris, n_lights;
	const float4 *sph_geom, *sph_amb, *sph_kd, *sph_ks, *lights, *tris;
	const float4 *cam_ec;     // per sphere {cam_pos - centre, |cam_pos - centre|^2 - r^2}: e and c of utils.h:115-118 for every ray that starts at the camera (skr_camec_kernel)
	const float4 *tri_chunks; // the chunk tree of the triangle walk (scene_host.h): 3 float4 per node, depth-first, skip links, then 2 float4 per chunk
	int32_t tri_chunk_size;
	int32_t tri_cones;        // some entry has a tight radius for non-grazing rays (else the cone test is compiled out of the walk)
	int32_t n_tri_chunks;     // its node count; 0 = culling off (ray directions longer than the bounds were built for)
	// utils.h:26-34 Options + scene.use_shadows
	int32_t monte_carlo, num_path_traces, grid_size, max_depth, use_shadows;
	uint32_t seed_lo, seed_hi;
	int32_t pow_steps;        // bit length of the scene's largest integer phong exponent in [1, 1024] (device_math.h powf_spec): 1 .. 11
	// the surface patches of the shadow masks (shadow_cells.h; shade_common.h shadow_cands), in the scene blob behind the shadow masks: one
	// table of shadow_surface_stride words (below) per pair of lights, the first at word shadow_surface_word from shadow_masks; a sphere's
	// header word is the .w of its kd row.  0 = the direction masks only.  Both words sit in alignment holes, as fog_row does.
	uint32_t shadow_surface_word;
	// outputs (device)
	uint8_t *rgb;
	float *rgbf;
	unsigned long long *counters; // SKR_COUNTER_SHARDS x {radiance rays, sphere hits shaded, shadow rays, pad}
	unsigned long long *tri_work; // 256 x {culling-sphere tests, triangle tests} the triangle walks executed (shade_common.h tri_work_add); null: not counted
	uint32_t *qctr;     // [0] the number of level-0 nodes skr_primary_kernel appended
	float *acc;         // float3 per output pixel: the running `image[y][x] += shade(...)` of main.cpp:162 (AA under --gillum: one pass per sample)
	uint32_t aa_index;  // which AA sample this launch traces
	// --scn-fog (DESIGN.md "Spherical fog"; general level pipeline): the fog volumes in file order, 2 float4 each — [radius absorption
	// scattering 0] [albedo 0] —, at row fog_row of the scene blob (sph_geom + fog_row; HBM, never written by a kernel); n_fog of them
	// (<= SKR_FOG_MAX, device_math.h; 0 = no fog).  Both sit in alignment holes: the struct keeps its size and every other field its
	// offset, so the kernels that never read them compile to the same code.
	uint32_t fog_row;
	// node pipeline (render_nodes.hip): the --gillum tree cut at every level.  A node is a shaded sphere hit; level 0 = the
	// primary hits.  A node is two rows of two float4 in two arrays, so that every kernel reads only the half it needs:
	//   geometry (tracing its children): [co.xyz N.x] [N.yz pixel node-id]                       (node id 0 at level 0)
	//   shading  (summing them):         [direct.xyz sphere] [r1 record|output-pixel pixel node-id]   (level 0: output pixel; deeper: its own record)
	const float4 *nd_src;     // geometry rows of the nodes whose children are traced (trace, activate, leaf)
	const float4 *ns_src;     // shading rows of the nodes whose children are summed (finalize, the depth-2 leaf kernel)
	float4 *nd_dst, *ns_dst;  // nodes being written (primary hits; activated records)
	uint32_t nd_src_level0;   // nd_src / ns_src hold the primary hits
	uint32_t shadow_surface_stride; // (see shadow_surface_word)
	const uint32_t *nd_count; // number of nodes in nd_src
	float4 *rc;               // hit records of the level being produced (trace) or consumed (activate, leaf): SKR_REC_ROWS float4 each (launch.h): [parent, sphere | child << 16, r1, D] [d.xyz, b]
	uint32_t rc_cap;          // records per region (SKR_P1_REGIONS regions)
	uint32_t *rc_ctr;         // that level's counters: [STRIDE r] records in region r, [STRIDE (64 + r)] units handed out, [STRIDE 128] exhausted mask, [STRIDE 129 ..] prefix sums
	uint4 *ixh;               // per trace wave and round (64 consecutive nd_src nodes, sibling pair j of each: row (node >> 6) * PP + j, launch.h skr_trace_header_row) three uint4: {first record of its hits, how many of them are even children's, -, -}, the ballots of the even / odd children that hit (64 bits each), the ballots of the children a triangle took (triangle scenes)
	uint32_t band_blk0, band_nblk, blocks_x; // node_layout: skr_primary_kernel covers the 16x16 pixel blocks [band_blk0, band_blk0 + band_nblk) of the launch (row-major, blocks_x per row)
	void *node_scratch;       // (host) the pipeline's one allocation
	const float *res_in;      // (colour r1)/pdf of every child record (finalize)
	float *res_out;           // the same for this level's records (leaf kernel; finalize of a level >= 1)
	// --shade-triangles (general level pipeline): triangles are surfaces, not black holes
	int32_t shade_triangles;
	int32_t legacy_reflect;   // --legacy-reflect (general level pipeline): raytrace.h:45-103 runs; sph_ks[i].w = the sphere's index of refraction
	const float4 *tri_mats;   // 3 float4 per triangle, in tris[] order: [La*ka, power] [kd] [ks] (the rows sph_amb / sph_kd / sph_ks hold for a sphere)
	// general level pipeline (render_generic.hip): one lane per ray, every mode, any depth
	uint32_t g_level;         // the level a launch works on (trace / activate: the rays' level, 1 = primary; finalize: the nodes' level, 0 = the camera)
	uint32_t g_arity;         // children per node of the level whose children are traced / summed (1 at the camera level); activate: the tree's arity (node ids)
	uint32_t g_last;          // activate: the hits of the last level (their children are shade(depth 0) == 0) are finished at once
	int32_t n_fog;            // (see fog_row)
	const float4 *g_nodes_src; // nodes of the level above (trace, activate) / of the level being summed (finalize): 5 float4 each
	union {
		float4 *g_nodes_dst;  // nodes being written (activate)
		// node pipeline (it has no g_nodes_dst; one word for both, so that every field keeps its offset and every kernel that reads neither
		// its code): the row of GI masks of every level-0 node (shade_common.h gi_surface_row), stored by skr_primary_build_kernel with the
		// node and kept with it across frames (launch.h SKR_LEVEL0_BUILD); null = not stored, skr_trace_kernel looks its lanes' rows up itself
		int32_t *gi_row0;
	};
	// the shadow masks (shadow_cells.h; the level pipelines' shadow walk, shade_common.h occluded_pair): SKR_SHADOW_TABLE_WORDS per point light,
	// in the scene blob (HBM, never written by a kernel); null = every shadow ray tests every sphere.  They hold for shading points P with
	// fl(|Lp - P|^2) <= shadow_reach2; shadow_all = the mask of every sphere.
	const uint32_t *shadow_masks;
	float shadow_reach2;
	uint32_t shadow_all;
	// the GI masks (shadow_cells.h; the node pipeline's closest-hit walk of GI children, wave_common.h closest_pair), in the scene blob:
	// gi_index = the index words of both grids, gi_masks = the rows of masks (uint16_t entries, uint32_t where gi_wide); null = every
	// GI child tests every sphere.  gi_all = the mask of every sphere.
	const int32_t *gi_index;
	const uint32_t *gi_masks;
	SkrGiGrid gi_grid[2];
	int32_t gi_wide;
	uint32_t gi_all;
	// the surface patches of the GI masks (shadow_cells.h; shade_common.h gi_surface_row), in the scene blob behind the grids' rows:
	// SKR_GI_SURFACE_HEAD words per sphere, then the patch index words; their rows continue the grids' rows of gi_masks.  null = the
	// grids only.
	const uint32_t *gi_surface;
};
// (a by-value kernel argument: the hidden arguments and every kernel's further arguments follow it, so a change of its size moves their
// offsets in every kernel, and with them the code of kernels that no change meant to touch)
static_assert(sizeof(RenderParams) == 624, "RenderParams keeps its size: new fields go into its alignment holes");

// The sphere tree (include/skr.h skr_scene_set_sphere_tree): what the sphere walks of the general level pipeline read
// (shade_common.h stree_walk), handed to the instances that have the walks in a kernel argument of their own — RenderParams, and with it
// the code of every kernel that takes only it, stays as it was.  All tables sit in the scene blob (HBM, never written by a kernel).
struct SphereTree {
	const float4 *nodes;  // 2 rows per node, depth-first: {centre, R^2} {kappa, skip, first chunk (height 1: it has the next 8, or those left; else -1), smallest file index below}; + a pad node
	const float4 *chunks; // 3 rows per chunk: {centre, R^2} {kappa, smallest file index, first sphere row, spheres} {their file indices}; + a pad chunk
	const float4 *rows;   // the spheres {centre, r^2} in device order: the always-tested ones, then Morton order
	int32_t n_nodes;      // nodes of the tree over the chunks behind the always-tested ones (0: there are none)
	int32_t n_chunks;     // chunks in all
	int32_t n_always;     // chunks at the front that every ray tests (no culling sphere holds them)
	int32_t cull;         // 0: every wave runs the loop over all spheres in file order (SKR_NO_SPHERE_CULL)
	float4 ball;          // {centre, radius}: the walk is taken by a wave whose rays all start in it
	unsigned long long *work; // HBM, or null (not counting): SKR_TRI_WORK_SHARDS x {culling-sphere tests, sphere tests} the walks executed
};

// The spot lights (include/skr.h SKR_SCN_SPOT): lights [first, first + n) of the light table are spot lights, and
// `cones` holds what the host derived for each, 2 rows per light in file order — {unit axis, c1} {c2, 0, 0, 0} — in the scene blob behind
// the fog rows (HBM, never written by a kernel).  Handed to the activate kernel's instances with the cone decision in a kernel argument
// of their own, as SphereTree is: RenderParams keeps its size and every offset, and every other kernel its code.
struct SpotLights {
	const float4 *cones;
	int32_t first, n;
};

// The radii of the point and spot lights (include/skr.h skr_scene_set_light_radii): radii[l] for the lights [0, n) of
// the light table, n = point lights + spot lights (a directional light has none), one float per light in the scene blob behind the cone
// rows (HBM, never written by a kernel).  Handed to the activate kernel's instances with the light sample in a kernel argument of their
// own, behind SpotLights (n = 0 where the scene has no spot light): RenderParams keeps its size and every offset.
struct SoftLights {
	const float *radii;
	int32_t n;
};

// Optional timing of the dominant kernel of a launch (skr_renderer_kernel_ms): the launcher records the
// two events right around that kernel on the launch stream — and, where `snap` is set, copies the work counters in front of the
// first event and behind the second (stream-ordered device-to-device copies outside the timed window), so that the work of that
// one kernel can be told from the frame's (skr_renderer_kernel_work: the numerator of bench.py's kernel-level roofline).
struct SkrTimingHook {
	hipEvent_t start = nullptr, stop = nullptr;
	unsigned long long *snap = nullptr;             // device: 2 x SKR_COUNTER_SHARDS x 4 words, or null
	const unsigned long long *counters = nullptr;   // device: RenderParams::counters
};
static inline void skr_hook_start(const SkrTimingHook *h, hipStream_t stream)
{
	if(!h) return;
	if(h->snap) (void) hipMemcpyAsync(h->snap, h->counters, (size_t) SKR_COUNTER_SHARDS * 4 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream);
	if(h->start) (void) hipEventRecord(h->start, stream);
}
static inline void skr_hook_stop(const SkrTimingHook *h, hipStream_t stream)
{
	if(!h) return;
	if(h->stop) (void) hipEventRecord(h->stop, stream);
	if(h->snap) (void) hipMemcpyAsync(h->snap + (size_t) SKR_COUNTER_SHARDS * 4, h->counters, (size_t) SKR_COUNTER_SHARDS * 4 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream);
}
