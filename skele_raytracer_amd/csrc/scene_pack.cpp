// The scene blob's packer (scene_pack.h): host only.
#include "scene_pack.h"

#include <cmath>
#include <cstring>

std::vector<skr_f4> skr_pack_scene(const skr_scene &s, SceneLayout &d)
{
	std::vector<skr_f4> rows;
	auto put = [&](SkrBlobSection sec, const void *src, size_t bytes) { // section `sec`: `bytes` of `src` (null: zeros) as whole rows
		const size_t at = rows.size();
		rows.resize(at + (bytes + 15) / 16, skr_f4{0.0f, 0.0f, 0.0f, 0.0f});
		if(src && bytes) memcpy(&rows[at], src, bytes);
		d.first[sec] = at;
		d.rows[sec] = rows.size() - at;
	};
	auto put4 = [&](SkrBlobSection sec, const std::vector<skr_f4> &v) { put(sec, v.data(), v.size() * 16); };
	put4(SKR_SEC_geom, s.sph_geom);
	put4(SKR_SEC_amb, s.sph_amb);
	put4(SKR_SEC_kd, s.sph_kd);
	put4(SKR_SEC_ks, s.sph_ks);
	put4(SKR_SEC_lights, s.lights);
	put4(SKR_SEC_tris, s.tris);
	put4(SKR_SEC_chunks, s.tri_chunks);
	d.chunk_size = s.tri_chunk_size;
	d.chunk_stride = s.tri_chunk_stride;
	d.cones = s.tri_any_cone ? 1 : 0;
	d.n_chunks = s.info.n_triangles ? s.tri_node_count : 0;
	put4(SKR_SEC_tri_mats, s.tri_mats);
	d.n_fog = (int) (s.raw_fog.size() / 9);
	std::vector<skr_f4> fog;
	for(int j = 0; j < d.n_fog; j++)
	{
		const float *f = &s.raw_fog[9 * j]; // x y z radius r g b scattering absorption
		fog.push_back({f[3], f[8], f[7], 0.0f});
		fog.push_back({f[4], f[5], f[6], 0.0f});
	}
	put4(SKR_SEC_fog, fog);
	d.n_spot = s.n_spot();
	d.spot_first = s.info.n_point_lights;
	put4(SKR_SEC_spot, s.spot_cones);
	d.n_radii = (int) s.light_radii.size();
	d.soft = s.soft();
	put(SKR_SEC_radii, s.light_radii.data(), s.light_radii.size() * 4);
	d.lens_A = s.lens_aperture;
	d.lens_F = s.lens_focus;
	d.lens_k = s.lens_aperture / s.lens_focus;
	if(!s.shadow_masks.empty()) put(SKR_SEC_smask, s.shadow_masks.data(), s.shadow_masks.size() * 4);
	d.shadow_reach2 = s.shadow_reach2;
	if(!s.shadow_surface.empty())
	{
		put(SKR_SEC_ssurf, s.shadow_surface.data(), s.shadow_surface.size() * 4);
		d.ssurf_stride = s.shadow_surface_stride;
		for(size_t k = 0; k < s.shadow_surface_head.size(); k++) memcpy(&rows[d.first[SKR_SEC_kd] + k].w, &s.shadow_surface_head[k], 4);
	}
	if(!s.gi_table.empty())
	{ // (whole rows: scene_masks.cpp build_gi_masks; the patches' rows continue the grids' rows)
		const size_t patch_word = s.gi_mask_word + (size_t) s.gi_rows * (SKR_GI_ROW_ENTRIES * (s.gi_wide ? 4 : 2) / 4);
		d.gi_surface_word = s.gi_surface.empty() ? 0 : patch_word + s.gi_surface_head;
		put(SKR_SEC_gi, nullptr, std::max(s.gi_table.size(), s.gi_surface.empty() ? 0 : patch_word + s.gi_surface.size()) * 4);
		uint32_t *words = reinterpret_cast<uint32_t *>(&rows[d.first[SKR_SEC_gi]]);
		memcpy(words, s.gi_table.data(), s.gi_table.size() * 4);
		if(d.gi_surface_word) memcpy(words + patch_word, s.gi_surface.data(), s.gi_surface.size() * 4);
	}
	d.gi_grid[0] = s.gi_grid[0];
	d.gi_grid[1] = s.gi_grid[1];
	d.gi_mask_word = s.gi_mask_word;
	d.gi_wide = s.gi_wide;
	if(s.info.n_triangles && !s.trace_chunks.empty()) put4(SKR_SEC_trace, s.trace_chunks);
	d.trace_ball = skr_f4{s.trace_ball[0], s.trace_ball[1], s.trace_ball[2], s.trace_ball[3]};
	d.trace_cones = s.trace_any_cone ? 1 : 0;
	d.tri_shadows = s.triangle_shadows;
	d.sphere_tree = s.sphere_tree && !s.sph_geom.empty();
	if(d.sphere_tree)
	{
		SkrSphereTree t;
		skr_build_sphere_tree(s, t);
		put4(SKR_SEC_st_rows, t.rows);
		put4(SKR_SEC_st_chunks, t.chunks);
		put4(SKR_SEC_st_nodes, t.nodes);
		d.st_nodes = t.n_nodes;
		d.st_chunks = t.n_chunks;
		d.st_always = t.n_always;
		d.st_ball = skr_f4{t.ball[0], t.ball[1], t.ball[2], t.ball[3]};
	}
	d.motion = s.motion();
	d.shutter = s.shutter;
	d.env_edge = s.env_edge;
	d.textured = s.textured();
	d.emissive = s.emissive();
	put(SKR_SEC_pad, nullptr, SKR_BLOB_PAD_ROWS * 16);
	{ // the straight-line pow runs as many squarings as the scene's largest integer exponent has bits
		// ... and needs a product only at a bit that some integer exponent has set (pow_any; the others take powf_spec_cold lane by lane)
		float top = 1.0f;
		unsigned any = 0;
		auto look = [&](float pw) {
			if(!(pw >= 1.0f && pw <= 1024.0f && pw == rintf(pw))) return;
			any |= (unsigned) pw;
			if(pw > top) top = pw;
		};
		for(const skr_f4 &a : s.sph_amb) look(a.w);
		for(size_t i = 0; i + 2 < s.tri_mats.size(); i += 3) look(s.tri_mats[i].w);
		int bits = 0;
		for(unsigned v = (unsigned) top; v; v >>= 1) bits++;
		d.pow_steps = bits < 1 ? 1 : bits;
		d.pow_any = any;
	}
	return rows;
}

extern "C" int64_t skr_scene_pack(const skr_scene *scene, int64_t *first, int64_t *count, uint32_t *rows, int64_t row_cap, const char **names, int64_t *scalars)
{
	static const char *const table[SKR_BLOB_SECTION_COUNT] = {
#define X(name) #name,
		SKR_BLOB_SECTIONS(X)
#undef X
	};
	if(!scene) return -SKR_ERR_ARG;
	SceneLayout l;
	const std::vector<skr_f4> blob = skr_pack_scene(*scene, l);
	for(int k = 0; k < SKR_BLOB_SECTION_COUNT; k++)
	{
		if(first) first[k] = (int64_t) l.first[k];
		if(count) count[k] = (int64_t) l.rows[k];
		if(names) names[k] = table[k];
	}
	if(rows && (int64_t) blob.size() <= row_cap && !blob.empty()) memcpy(rows, blob.data(), blob.size() * 16);
	if(scalars)
	{
		scalars[0] = l.pow_steps;
		scalars[1] = (int64_t) l.gi_surface_word;
	}
	return (int64_t) blob.size();
}
