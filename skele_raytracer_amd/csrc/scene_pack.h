// The scene blob: the one allocation a renderer uploads its scene as, in rows of 16 bytes.  Host only: the format, the packer
// (scene_pack.cpp) and nothing of the device, so the unit compiles without the HIP runtime and the sanitizer run reaches it
// (tools/sanitize_host.sh).
#pragma once

#include "scene_host.h"
#include "shadow_cells.h"

// The sections of the blob, in blob order.  The packer, SceneLayout and skr_scene_pack all follow this table.
//   geom amb kd ks      the spheres (skr_scene sph_*); with shadow surface patches the .w of a kd row is its sphere's header word
//   lights              2 rows per light (skr_scene::lights)
//   tris chunks tri_mats  the triangles, SKR_CULL_LEVELS sets of their chunk tree, their materials
//   fog                 2 rows per volume: [radius absorption scattering 0] [albedo 0] (render_params.h RenderParams::fog_row)
//   spot                2 rows per spot light: {unit axis, c1} {c2, 0, 0, 0} (render_params.h SpotLights)
//   radii               one float per point and spot light, in light order (render_params.h SoftLights)
//   smask ssurf         the shadow masks, 4 words per row, and their surface patches (shadow_cells.h)
//   gi                  the GI masks (skr_scene::gi_table), the surface patches' masks right behind the grids' rows, then the patches' headers and index
//   trace               the ray queries' tree (skr_scene::trace_chunks)
//   st_rows st_chunks st_nodes  the sphere tree (render_params.h SphereTree); the walk asks for the rows of a whole chunk, up to 3 behind the last sphere: the chunks follow
//   pad                 SKR_BLOB_PAD_ROWS rows of zeros: the sphere loops ask for the rows of a trip ahead without a bounds test (shade_common.h sphere_rows)
#define SKR_BLOB_SECTIONS(X) X(geom) X(amb) X(kd) X(ks) X(lights) X(tris) X(chunks) X(tri_mats) X(fog) X(spot) X(radii) X(smask) X(ssurf) X(gi) X(trace) X(st_rows) X(st_chunks) X(st_nodes) X(pad)
enum SkrBlobSection {
#define X(name) SKR_SEC_##name,
	SKR_BLOB_SECTIONS(X)
#undef X
	SKR_BLOB_SECTION_COUNT
};
#define SKR_BLOB_PAD_ROWS 16

// Where a packed scene's sections lie and the scalars that travel with them: host facts of an skr_scene, no device pointer.
struct SceneLayout {
	size_t first[SKR_BLOB_SECTION_COUNT] = {}, rows[SKR_BLOB_SECTION_COUNT] = {}; // per section its first row and its rows; 0 rows: absent
	bool has(SkrBlobSection s) const { return rows[s] != 0; }
	int pow_steps = 11; // bit length of the largest integer phong exponent in [1, 1024] among the scene's materials (device_math.h powf_spec)
	unsigned pow_any = 0x7FF; // the OR of those exponents (0: the scene has none): the bits at which the straight-line pow needs a product (launch.h skr_leaf_pow_plan)
	int n_chunks = 0, chunk_size = 0, cones = 0; // nodes of the chunk tree (scene_host.h)
	size_t chunk_stride = 0;
	int n_fog = 0;
	int n_spot = 0, spot_first = 0; // lights [spot_first, spot_first + n_spot) of the light table are spot lights
	int n_radii = 0;
	bool soft = false;        // some radius is > 0: frames and shading queries take the instances with the light sample
	float lens_A = 0.0f, lens_F = 1.0f, lens_k = 0.0f; // skr_scene_set_lens: the aperture, the focus and k = A / F (one binary32 division); A > 0: frames take the instances with the lens sample
	uint32_t ssurf_stride = 0; // words per pair of lights in ssurf
	float shadow_reach2 = 0.0f;
	SkrGiGrid gi_grid[2] = {};
	uint32_t gi_mask_word = 0;
	int gi_wide = 0;
	size_t gi_surface_word = 0; // the surface patches' headers (skr_scene::gi_surface), in words from the gi section; 0 = none
	skr_f4 trace_ball{};
	int trace_cones = 0;
	bool tri_shadows = false; // the scene's triangle-shadow switch when it was packed (include/skr.h skr_scene_set_triangle_shadows)
	bool sphere_tree = false; // the sphere tree (include/skr.h skr_scene_set_sphere_tree), packed where the scene had the switch on
	int st_nodes = 0, st_chunks = 0, st_always = 0;
	skr_f4 st_ball{};
	bool motion = false;  // motion is in force (skr_scene::motion(), include/skr.h skr_scene_set_sphere_velocities): frames and shading queries take the instances with the shutter draw.
	float shutter = 1.0f; // The velocities are no section of the blob: the renderer uploads them beside it (api.cpp DeviceScene::d_vel)
	int env_edge = 0;     // the environment's edge E, 0 = none (include/skr.h skr_scene_set_environment): in force, frames and shading queries take the finalize instances
	                      // with the lookup.  The texels are no section of the blob either (api.cpp DeviceScene::d_env)
	bool textured = false; // textures are in force (skr_scene::textured(), include/skr.h skr_scene_add_texture): frames and shading queries take the activate and finalize
	                       // instances with the lookup.  Rows and texels are no section of the blob either (api.cpp DeviceScene::d_tex)
	bool emissive = false; // emission is in force (skr_scene::emissive(), include/skr.h skr_scene_set_sphere_emission): frames and shading queries take the activate and finalize
	                       // instances with the add.  The rows are no section of the blob either (api.cpp DeviceScene::d_emit)
};

// The blob of `s` and its layout; nothing is uploaded.
std::vector<skr_f4> skr_pack_scene(const skr_scene &s, SceneLayout &layout);

// Internal export (not in include/skr.h: tests/test_scene_blob_host.py and tools/sanitize_host.cpp only).  Packs `scene` on the host and
// returns the blob's rows (< 0: minus an error code).  first, count (null, or SKR_BLOB_SECTION_COUNT entries): per section of the table
// its first row and its rows.  rows (null, or room for row_cap rows of 4 words): the blob, if it fits.  names (null, or
// SKR_BLOB_SECTION_COUNT entries): the table.  scalars (null, or 2 entries): pow_steps, gi_surface_word.
extern "C" int64_t skr_scene_pack(const skr_scene *scene, int64_t *first, int64_t *count, uint32_t *rows, int64_t row_cap, const char **names, int64_t *scalars);
