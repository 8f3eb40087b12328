// Host-side scene: what the .scn loader produces and what is uploaded to HBM.
// Replaces struct Scene (reference src/scene.h:13-28) and its AoS members
// (shapes.h:12,26  material.h:9  lights.h:19  camera.h:8) with the SoA layout the
// kernels read.  See DESIGN.md "Data layout in HBM".
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/skr.h"
#include "shadow_cells.h"
#include "tri_chunks.h"


struct skr_f4 {
	float x, y, z, w;
};

// An axis-aligned box in binary64 that grows around balls, from nothing or from a first point (which may be NaN, and then stays).
struct SkrBox {
	double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
	SkrBox() {}
	SkrBox(double x, double y, double z) : lo{x, y, z}, hi{x, y, z} {}
	void grow(double x, double y, double z, double r)
	{
		const double p[3] = {x, y, z};
		for(int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], p[k] - r); hi[k] = std::max(hi[k], p[k] + r); }
	}
	double centre(int k) const { return 0.5 * (lo[k] + hi[k]); }
};

// One set of the triangle chunk tree (skr_scene::tri_chunks) as skr_scene::build_triangle_chunk_level returns it.
struct SkrChunkLevel {
	std::vector<skr_f4> rows; // the nodes, a pad node, the chunk entries, a pad entry
	int node_count = 0;
	bool any_cone = false; // at least a quarter of the chunks have a tight radius for non-grazing rays
};

struct skr_scene {
	// raw values as parsed (skr_scene_get_arrays, loader parity tests)
	std::vector<float> raw_spheres;      // [n][14] centre radius ambient diffuse specular power
	std::vector<float> raw_sphere_ior;   // [n] index of refraction (material.h:16); shorter than n = 1.0.  Read by --legacy-reflect only
	std::vector<float> raw_triangles;    // [n][9]  v0 v1 v2
	std::vector<float> raw_triangle_materials; // [n][10] ambient diffuse specular power: the material in force on each `triangle` line
	                                     //         (read by --shade-triangles only; shorter than n = the default material, material.h:9-17)
	std::vector<float> raw_point_lights; // [n][6]  position colour
	std::vector<float> raw_directional_lights; // [n][6] direction colour — --strict-scn only (scene.cpp:139-163 drops them)
	std::vector<float> raw_fog;          // [n][9] centre radius albedo scattering absorption — SKR_SCN_FOG / skr_scene_set_fog only (file order)
	std::vector<float> raw_spot_lights;  // [n][11] colour position direction angle1 angle2, the file's fields in file order — SKR_SCN_SPOT / skr_scene_set_spot_lights only
	std::vector<float> light_radii;      // [n_point + n_spot] the radius of every point and spot light in light order, 0 = a point — skr_scene_set_light_radii only (build_lights() sizes it)
	float lens_aperture = 0.0f, lens_focus = 1.0f; // the lens (A, F), A = 0: the pinhole — skr_scene_set_lens only (include/skr.h)
	std::vector<float> velocities;       // [n][3] the velocity of every sphere in file order; empty = every sphere at rest — SKR_SCN_MOTION / skr_scene_set_sphere_velocities only (include/skr.h)
	float shutter = 1.0f;                // the shutter S >= 0 — skr_scene_set_shutter only
	bool motion() const                  // motion is in force: S > 0 and some velocity component is not 0
	{
		if(!(shutter > 0.0f)) return false;
		for(float v : velocities)
			if(v != 0.0f) return true;
		return false;
	}
	std::vector<float> env_texels;       // [E][E][3] the environment's texels, row j first; empty = none — skr_scene_set_environment only (include/skr.h)
	int32_t env_edge = 0;                // E; 0 = no environment (then misses return info.background, as ever)
	std::vector<std::vector<float>> textures; // texture k: [E_k][E_k][3] texels, row j first — SKR_SCN_TEXTURE / skr_scene_add_texture only (include/skr.h)
	std::vector<int32_t> texture_edges;  // E_k
	std::vector<int32_t> sphere_textures; // [n] the texture index of every sphere in file order, -1 = none; shorter than n = -1 — skr_scene_set_sphere_textures
	bool textured() const                // textures are in force: some sphere has a texture
	{
		for(int32_t x : sphere_textures)
			if(x >= 0) return true;
		return false;
	}
	std::vector<float> emission;         // [n][3] the emission of every sphere in file order, each finite and >= 0; empty = none — SKR_SCN_EMISSION / skr_scene_set_sphere_emission only (include/skr.h)
	bool emissive() const                // emission is in force: some component of some sphere is > 0
	{
		for(float v : emission)
			if(v > 0.0f) return true;
		return false;
	}
	bool strict = false;                 // parsed with SKR_SCN_STRICT
	bool triangle_shadows = false;       // SKR_SCN_TRIANGLE_SHADOWS / skr_scene_set_triangle_shadows: a renderer made from the scene takes it (include/skr.h)
	bool sphere_tree = false;            // SKR_SCN_SPHERE_TREE / skr_scene_set_sphere_tree: likewise
	skr_scene_info info{};

	// SoA arrays as uploaded (built by finalize())
	std::vector<skr_f4> sph_geom; // centre.xyz, radius*radius (utils.h:118 forms r*r per test; same product)
	std::vector<skr_f4> sph_amb;  // ambient_light.colour * material.ambient (blinn_phong.h:15), .w = phong power
	std::vector<skr_f4> sph_kd;   // material.diffuse
	std::vector<skr_f4> sph_ks;   // material.specular, .w = index of refraction
	std::vector<skr_f4> lights;   // [2*i] position (.w = 0) or, behind the point lights, direction (.w = 1: --strict-scn), [2*i+1] colour
	                              // (the spot lights are point-light rows between the point lights and the directional ones: build_lights())
	std::vector<skr_f4> spot_cones; // 2 per spot light, in file order: {unit axis, c1} {c2, 0, 0, 0} (include/skr.h skr_scene_get_spot_cones)
	std::vector<skr_f4> tris;     // [3*i] v0, [3*i+1] v1-v0, [3*i+2] v2-v0 (utils.h:183-184 subtractions); [3*i+1].w = the triangle's index in the file (int bits)
	std::vector<skr_f4> tri_mats; // [3*i] La*ka, power  [3*i+1] kd  [3*i+2] ks of the triangle stored at tris[3*i] (--shade-triangles)
	// the culling data of the triangle walk: a tree, depth-first with skip links, three float4 per node — {centre, R^2}
	// {axis / kappa, R_tight^2} {skip, first chunk, chunk count, height} (ints) — + one pad node, then two float4 per
	// chunk of tri_chunk_size consecutive triangles — {centre, R^2} {axis / kappa, R_tight^2} — + one pad entry.
	// Every inner node has SKR_TRI_SUPER children; a sphere is conservative: a line that
	// misses it cannot pass utils.h:181-213 for any triangle of the chunk (scene_trees.cpp build_triangle_chunks)
	std::vector<skr_f4> tri_chunks; // SKR_CULL_LEVELS sets of them, one per bound on |d| (tri_chunks.h)
	int tri_chunk_size = SKR_TRI_CHUNK_MIXED;

	void finalize();
	void build_lights(); // lights and spot_cones from the raw light arrays
	int n_spot() const { return (int) (raw_spot_lights.size() / 11); }
	bool soft() const // some light has a radius > 0
	{
		for(float r : light_radii)
			if(r > 0.0f) return true;
		return false;
	}
	size_t tri_chunk_stride = 0; // float4 entries per |d| level
	int tri_node_count = 0;
	bool tri_any_cone = false; // some chunk has a tight radius for non-grazing rays (scene_trees.cpp)
	void build_triangle_chunks(); // every tri_* and trace_* member below tris: both trees, tri_chunk_size chosen here
	std::vector<int> tri_order; // tris[3*i] holds triangle tri_order[i] of the file
	void build_triangle_materials();
	// one set of a tree for |d| <= d_max.  origin_ball (x, y, z, radius) or null: the rays start anywhere in that ball instead of at
	// the camera or on a sphere
	SkrChunkLevel build_triangle_chunk_level(double d_max, const double *origin_ball = nullptr) const;
	// the same tree for the ray queries (skr_trace_rays): SKR_CULL_LEVELS sets of tri_chunk_stride entries that hold for rays starting
	// anywhere in the ball trace_ball = {centre, radius} (twice the radius of a ball around the camera, the spheres and the triangles'
	// accept regions); the kernel walks them for a wave whose rays all start inside it, and every triangle otherwise
	std::vector<skr_f4> trace_chunks;
	float trace_ball[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	bool trace_any_cone = false;
	// the shadow masks of the level pipelines' shadow walk (shadow_cells.h, DESIGN.md "Shadow masks"): SKR_SHADOW_TABLE_WORDS per point
	// light, in light order; empty where the walk keeps its plain loop (no sphere, more than SKR_SHADOW_MAX_SPHERES, a directional light)
	std::vector<uint32_t> shadow_masks;
	float shadow_reach2 = 0.0f; // the masks hold for shading points P with fl(|Lp - P|^2) <= shadow_reach2 (every light); other lanes test every sphere
	void build_shadow_masks();
	// the GI masks of the node pipeline's closest-hit walk (shadow_cells.h, DESIGN.md "GI masks"): the index words of both grids, then
	// the masks (uint16_t, or uint32_t where gi_wide), padded to whole 16-byte rows; empty where the walk keeps its plain loop
	// (no sphere, more than SKR_GI_MAX_SPHERES, triangles)
	std::vector<uint32_t> gi_table;
	SkrGiGrid gi_grid[2] = {}; // fine, coarse
	uint32_t gi_mask_word = 0; // the first word of the masks in gi_table
	int gi_wide = 0;
	void build_gi_masks();
	// the surface patches of the GI masks (shadow_cells.h, DESIGN.md "GI surface patches"): the patches' masks (rows gi_rows,
	// gi_rows + 1, ... of the device's table, which are laid behind the grids' rows), then SKR_GI_SURFACE_HEAD words per sphere from
	// word gi_surface_head, then the index words; empty where there are no GI masks
	std::vector<uint32_t> gi_surface;
	uint32_t gi_surface_head = 0;
	uint32_t gi_rows = 0; // rows of masks of the grids in gi_table
	double gi_surface_edge = 0.0; // the patches' cell edge (G_s = ceil(2 r_s / edge)); 0 = no patches
	void build_gi_surface();
	// the surface patches of the shadow masks (shadow_cells.h, DESIGN.md "Shadow surface patches"): one table of shadow_surface_stride
	// words per pair of lights, in pair order, and one header word per sphere (base | G << 24); empty where there are no shadow masks.
	// rho_scale, cone_scale: the tests' shrunk margins (1 = the product's)
	std::vector<uint32_t> shadow_surface, shadow_surface_head;
	uint32_t shadow_surface_stride = 0;
	void build_shadow_surface(double rho_scale = 1.0, double cone_scale = 1.0);
};

// The sphere tree (include/skr.h skr_scene_set_sphere_tree) in the layout of render_params.h SphereTree.  Built on
// demand (a renderer of a scene with the switch on; skr_scene_get_sphere_tree_data), not by finalize(): a scene without the switch
// does not pay for it.
#define SKR_SPHERE_CHUNK 4 // spheres per chunk: the file indices of a chunk fill one row
#define SKR_SPHERE_SUPER 8 // children per node
struct SkrSphereTree {
	int n_nodes = 0, n_chunks = 0, n_always = 0; // n_always: chunks of always-tested spheres, at the front
	std::vector<skr_f4> rows;    // n_spheres rows {centre, r^2} in device order
	std::vector<int32_t> file;   // their file indices
	std::vector<skr_f4> nodes;   // 2 per node + a pad node
	std::vector<skr_f4> chunks;  // 3 per chunk + a pad chunk
	float ball[4] = {0.0f, 0.0f, 0.0f, -1.0f};
};
void skr_build_sphere_tree(const skr_scene &scene, SkrSphereTree &out);

// The order finalize() stores the first nt triangles of raw_triangles in: along a Morton curve (scene_trees.cpp).
std::vector<int> skr_triangle_order(const std::vector<float> &raw_triangles, int nt);

// A spot-light row as the loader and skr_scene_set_spot_lights accept it (include/skr.h SKR_SCN_SPOT): every field finite, a direction
// other than zero, 0 <= angle1 <= angle2 <= 180.
bool skr_spot_row_ok(const float row[11]);

// scene.cpp:12-227 replacement.  Returns SKR_OK or SKR_ERR_IO.
int skr_parse_scn(const std::string &path, bool echo, uint32_t flags, skr_scene &out);

void skr_set_error(const char *fmt, ...);
