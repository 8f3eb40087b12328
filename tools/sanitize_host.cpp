// Host-code sanitizer run (CPU only): loader, finalize, every table builder, the getters, the scene blob's packer, PPM writer.  Prints one 64-bit digest
// (FNV-1a over the 32-bit words) per derived table and scene, so that two builds of the host code can be compared table by table
// (the digests depend on the host's libm: compare builds on one machine).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <string>
#include "skr.h"
#include "../skele_raytracer_amd/csrc/tri_chunks.h" // SKR_CULL_LEVELS (plain #defines)
#include "../skele_raytracer_amd/csrc/scene_pack.h" // skr_scene_pack, the blob's section table

// internal exports of the library (tests only: not in include/skr.h)
extern "C" {
int skr_scene_get_gi_surface(const skr_scene *scene, int32_t *n_words, int32_t *head_word, int32_t *first_row, uint32_t *table);
int skr_scene_get_shadow_surface(const skr_scene *scene, int32_t *n_pairs, int32_t *stride, uint32_t *head, uint32_t *table);
int skr_scene_rebuild_shadow_surface(skr_scene *scene, double rho_scale, double cone_scale);
}

namespace {

struct Digest {
	uint64_t h = 0xcbf29ce484222325ull;
	template <class T> Digest &words(const T *p, size_t n)
	{
		static_assert(sizeof(T) == 4, "32-bit words");
		for(size_t i = 0; i < n; i++)
		{
			uint32_t w;
			memcpy(&w, p + i, 4);
			for(int b = 0; b < 4; b++) h = (h ^ ((w >> (8 * b)) & 0xffu)) * 0x100000001b3ull;
		}
		return *this;
	}
	template <class T> Digest &word(T v) { return words(&v, 1); }
};

void print(const char *scene, const char *stage, const char *table, const Digest &d)
{
	printf("%s %s %s %016llx\n", scene, stage, table, (unsigned long long) d.h);
}

// the two direction-mask tables every light change rebuilds
void shadow_tables(const skr_scene *sc, int n_spheres, const char *name, const char *stage)
{
	int32_t nl = 0, cells = 0;
	float reach2 = 0;
	skr_scene_get_shadow_masks(sc, &nl, &cells, &reach2, nullptr);
	std::vector<uint32_t> masks((size_t) nl * 6 * cells * cells + 1);
	skr_scene_get_shadow_masks(sc, nullptr, nullptr, nullptr, masks.data());
	print(name, stage, "shadow_masks", Digest().word(nl).word(cells).word(reach2).words(masks.data(), masks.size() - 1));
	int32_t np = 0, stride = 0;
	skr_scene_get_shadow_surface(sc, &np, &stride, nullptr, nullptr);
	std::vector<uint32_t> head((size_t) (stride ? n_spheres : 0) + 1), table((size_t) np * stride + 1);
	skr_scene_get_shadow_surface(sc, nullptr, nullptr, head.data(), table.data());
	print(name, stage, "shadow_surface", Digest().word(np).word(stride).words(head.data(), head.size() - 1).words(table.data(), table.size() - 1));
}

void gi_tables(const skr_scene *sc, const char *name)
{
	int32_t nw = 0, mw = 0, wide = 0, dc = 0, hw = 0, fr = 0;
	float grids[16] = {0};
	skr_scene_get_gi_masks(sc, &nw, &mw, &wide, &dc, grids, nullptr);
	std::vector<uint32_t> table((size_t) nw + 1);
	skr_scene_get_gi_masks(sc, nullptr, nullptr, nullptr, nullptr, nullptr, table.data());
	print(name, "built", "gi_masks", Digest().word(nw).word(mw).word(wide).word(dc).words(grids, 16).words(table.data(), nw));
	skr_scene_get_gi_surface(sc, &nw, &hw, &fr, nullptr);
	table.assign((size_t) nw + 1, 0u);
	skr_scene_get_gi_surface(sc, nullptr, nullptr, nullptr, table.data());
	print(name, "built", "gi_surface", Digest().word(nw).word(hw).word(fr).words(table.data(), nw));
}

void culling_tables(const skr_scene *sc, int n_triangles, const char *name)
{
	for(int trace = 0; trace < 2; trace++)
		for(int level = 0; level < SKR_CULL_LEVELS; level++)
		{
			int32_t cs = 0, nn = 0, nc = 0;
			float ball[4] = {0, 0, 0, 0};
			if(trace) skr_scene_get_trace_culling(sc, level, &cs, &nn, &nc, nullptr, nullptr, nullptr, nullptr, ball);
			else skr_scene_get_culling(sc, level, &cs, &nn, &nc, nullptr, nullptr, nullptr, nullptr);
			std::vector<float> dt((size_t) n_triangles * 12 + 1), ns((size_t) nn * 8 + 1), ch((size_t) nc * 8 + 1);
			std::vector<int32_t> nl((size_t) nn * 4 + 1);
			if(trace) skr_scene_get_trace_culling(sc, level, nullptr, nullptr, nullptr, dt.data(), ns.data(), nl.data(), ch.data(), nullptr);
			else skr_scene_get_culling(sc, level, nullptr, nullptr, nullptr, dt.data(), ns.data(), nl.data(), ch.data());
			Digest d;
			d.word(cs).word(nn).word(nc).words(ball, 4).words(dt.data(), dt.size() - 1).words(ns.data(), ns.size() - 1);
			d.words(nl.data(), nl.size() - 1).words(ch.data(), ch.size() - 1);
			const std::string table = std::string(trace ? "trace_culling" : "culling") + "[" + std::to_string(level) + "]";
			print(name, "built", table.c_str(), d);
		}
}

void sphere_tree_table(const skr_scene *sc, int n_spheres, const char *name)
{
	int32_t cs = 0, nn = 0, nc = 0, na = 0;
	float ball[4] = {0, 0, 0, 0};
	skr_scene_get_sphere_tree_data(sc, &cs, &nn, &nc, &na, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ball);
	std::vector<float> rows((size_t) n_spheres * 4 + 1), nsph((size_t) nn * 5 + 1), csph((size_t) nc * 5 + 1);
	std::vector<int32_t> file((size_t) n_spheres + 1), nlink((size_t) nn * 4 + 1), clink((size_t) nc * 3 + 1);
	skr_scene_get_sphere_tree_data(sc, nullptr, nullptr, nullptr, nullptr, rows.data(), file.data(), nsph.data(), nlink.data(), csph.data(), clink.data(), nullptr);
	Digest d;
	d.word(cs).word(nn).word(nc).word(na).words(ball, 4).words(rows.data(), rows.size() - 1).words(file.data(), file.size() - 1);
	d.words(nsph.data(), nsph.size() - 1).words(nlink.data(), nlink.size() - 1).words(csph.data(), csph.size() - 1).words(clink.data(), clink.size() - 1);
	print(name, "built", "sphere_tree_data", d);
}

void spot_cones_table(const skr_scene *sc, const char *name, const char *stage)
{
	int32_t n = 0;
	skr_scene_get_spot_lights(sc, nullptr, &n);
	std::vector<float> cones((size_t) n * 5 + 1);
	skr_scene_get_spot_cones(sc, cones.data());
	print(name, stage, "spot_cones", Digest().word(n).words(cones.data(), cones.size() - 1));
}

// the scene as a renderer would upload it (scene_pack.h): the rows and the section table
void blob_table(const skr_scene *sc, const char *name, const char *stage)
{
	int64_t first[SKR_BLOB_SECTION_COUNT], count[SKR_BLOB_SECTION_COUNT], scalars[2];
	const int64_t n = skr_scene_pack(sc, nullptr, nullptr, nullptr, 0, nullptr, nullptr);
	std::vector<uint32_t> rows((size_t) n * 4 + 1);
	skr_scene_pack(sc, first, count, rows.data(), n, nullptr, scalars);
	Digest d;
	d.words(rows.data(), rows.size() - 1);
	for(int k = 0; k < SKR_BLOB_SECTION_COUNT; k++) d.word((uint32_t) first[k]).word((uint32_t) count[k]);
	print(name, stage, "blob", d.word((uint32_t) scalars[0]).word((uint32_t) scalars[1]));
}

} // namespace

int main(int argc, char **argv)
{
	for(int a = 1; a < argc; a++)
	{
		skr_scene *sc = nullptr;
		int rc = skr_scene_create_from_scn(argv[a], 0, &sc);
		if(rc != 0) { printf("%s: rc %d (%s)\n", argv[a], rc, skr_last_error()); continue; }
		skr_scene_info info;
		skr_scene_get_info(sc, &info);
		std::vector<float> s((size_t) info.n_spheres * 14 + 1), t((size_t) info.n_triangles * 9 + 1), l((size_t) info.n_point_lights * 6 + 1);
		skr_scene_get_arrays(sc, s.data(), t.data(), l.data());
		printf("%s: %d spheres %d triangles %d lights ok\n", argv[a], info.n_spheres, info.n_triangles, info.n_point_lights);
		shadow_tables(sc, info.n_spheres, argv[a], "built");
		gi_tables(sc, argv[a]);
		culling_tables(sc, info.n_triangles, argv[a]);
		sphere_tree_table(sc, info.n_spheres, argv[a]);
		spot_cones_table(sc, argv[a], "built");
		blob_table(sc, argv[a], "built");
		// the rebuild paths: new lights, then the tests' shrunk margins
		const float spots[2][11] = {{1.0f, 0.9f, 0.8f, 0.5f, 3.0f, 1.5f, 0.1f, -1.0f, -0.2f, 20.0f, 35.0f},
									{0.3f, 0.4f, 2.0f, -2.0f, 1.0f, -3.0f, 1.0f, 0.5f, 1.0f, 0.0f, 90.0f}};
		rc = skr_scene_set_spot_lights(sc, &spots[0][0], 2);
		if(rc != 0) printf("%s: skr_scene_set_spot_lights rc %d (%s)\n", argv[a], rc, skr_last_error());
		shadow_tables(sc, info.n_spheres, argv[a], "spots");
		spot_cones_table(sc, argv[a], "spots");
		blob_table(sc, argv[a], "spots");
		skr_scene_rebuild_shadow_surface(sc, 0.5, 1.0);
		shadow_tables(sc, info.n_spheres, argv[a], "rho/2");
		blob_table(sc, argv[a], "rho/2");
		skr_scene_rebuild_shadow_surface(sc, 1.0, 0.5);
		shadow_tables(sc, info.n_spheres, argv[a], "cone/2");
		blob_table(sc, argv[a], "cone/2");
		skr_scene_set_sphere_tree(sc, 1);
		blob_table(sc, argv[a], "sphere_tree");
		skr_scene_destroy(sc);
		// motion: the loader under its flag, the setters with good and bad arguments, the getters; the velocities are no section of the blob
		skr_scene *mv = nullptr;
		if(skr_scene_create_from_scn_ex(argv[a], 0, SKR_SCN_MOTION, &mv) == 0)
		{
			const int32_t ns = info.n_spheres;
			std::vector<float> v((size_t) ns * 3 + 3, 0.5f), back((size_t) ns * 3 + 3, -1.0f);
			int32_t n = -1;
			skr_scene_get_sphere_velocities(mv, back.data(), &n);
			const int ok = skr_scene_set_sphere_velocities(mv, v.data(), ns);
			const int wrong_n = skr_scene_set_sphere_velocities(mv, v.data(), ns + 1);
			v[0] = NAN;
			const int not_finite = skr_scene_set_sphere_velocities(mv, v.data(), ns);
			skr_scene_get_sphere_velocities(mv, back.data(), &n);
			float S = -1.0f;
			const int s_ok = skr_scene_set_shutter(mv, 0.25f), s_bad = skr_scene_set_shutter(mv, -1.0f);
			skr_scene_get_shutter(mv, &S);
			printf("%s: motion %d spheres, set %d %d %d, v0 %g, shutter %d %d %g\n", argv[a], n, ok, wrong_n, not_finite, ns > 0 ? back[0] : 0.0f, s_ok, s_bad, S);
			blob_table(mv, argv[a], "motion");
			skr_scene_destroy(mv);
		}
	}
	std::vector<uint8_t> px(7 * 5 * 3, 200);
	skr_write_ppm("build/asan_out.ppm", 7, 5, px.data());
	{ // the PFM reader on what the writer wrote, on short, malformed and absurd files; the environment's setter and getter with good and bad arguments
		std::vector<float> f(7 * 5 * 3), back(7 * 5 * 3, -1.0f);
		for(size_t i = 0; i < f.size(); i++) f[i] = 0.25f * (float) i;
		skr_write_pfm("build/asan_out.pfm", 7, 5, f.data());
		uint32_t w = 0, h = 0;
		const int sizes = skr_read_pfm("build/asan_out.pfm", &w, &h, nullptr), whole = skr_read_pfm("build/asan_out.pfm", &w, &h, back.data());
		printf("pfm: sizes %d whole %d %u x %u same %d\n", sizes, whole, w, h, (int) (back == f));
		const char *const bad[] = {"PF\n7 5\n-1.0\n", "PF\n7 5\n", "PF\n7", "PF\n4294967295 4294967295\n-1.0\nxxxx", "PF\n-3 5\n-1.0\n", "Pf\n7 5\n-1.0\n", "PF\n7 5\n0.0\n", "PF\n7 5\nnan\n", "", "PF",
								   "PF\n99999999999999999999999 1\n1\n", "PF\n1 1\n1\n\1\2\3\4\5\6\7\1\2\3\4"};
		for(const char *text : bad)
		{
			FILE *fp = fopen("build/asan_bad.pfm", "wb");
			if(!fp) break;
			fputs(text, fp);
			fclose(fp);
			const int a = skr_read_pfm("build/asan_bad.pfm", &w, &h, nullptr);
			const int b = (a == 0 && (size_t) w * h * 3 <= back.size()) ? skr_read_pfm("build/asan_bad.pfm", &w, &h, back.data()) : -1;
			printf("pfm: bad file rc %d %d\n", a, b);
		}
		skr_scene *sc = nullptr;
		if(skr_scene_create_from_scn("build/empty.scn", 0, &sc) == 0)
		{
			std::vector<float> tex(5 * 5 * 3, 0.5f), got(5 * 5 * 3 + 3, -1.0f);
			int32_t e = -1;
			const int ok = skr_scene_set_environment(sc, tex.data(), 5), neg = skr_scene_set_environment(sc, tex.data(), -1), big = skr_scene_set_environment(sc, tex.data(), SKR_ENV_MAX_EDGE + 1);
			tex[74] = INFINITY;
			const int not_finite = skr_scene_set_environment(sc, tex.data(), 5);
			skr_scene_get_environment(sc, got.data(), &e);
			printf("env: set %d %d %d %d, edge %d, last %g guard %g\n", ok, neg, big, not_finite, e, got[74], got[75]);
			blob_table(sc, "env", "set");
			const int cleared = skr_scene_set_environment(sc, nullptr, 5);
			skr_scene_get_environment(sc, got.data(), &e);
			printf("env: cleared %d edge %d\n", cleared, e);
			skr_scene_destroy(sc);
		}
	}
	{ // sphere textures: add, get, the per-sphere indices with good and bad arguments, and the parser's `texture` lines on good, missing, malformed and too many files
		std::vector<float> t2(2 * 2 * 3), t3(3 * 3 * 3, 0.25f);
		for(size_t i = 0; i < t2.size(); i++) t2[i] = 0.5f * (float) i;
		skr_write_pfm("build/asan_t2.pfm", 2, 2, t2.data());
		skr_write_pfm("build/asan_t3.pfm", 3, 3, t3.data());
		skr_write_pfm("build/asan_wide.pfm", 3, 2, t3.data());
		t3[7] = INFINITY;
		skr_write_pfm("build/asan_inf.pfm", 3, 3, t3.data());
		t3[7] = 0.25f;
		FILE *fp = fopen("build/asan_tex.scn", "w");
		if(fp)
		{
			fputs("sphere 0 0 0 1\ntexture asan_t2.pfm\nsphere 1 0 0 1\ntexture\ntexture  \t \ntexture asan_missing.pfm\ntexture asan_wide.pfm\ntexture asan_inf.pfm\ntexture asan_bad.pfm\n"
				  "sphere 2 0 0 1\ntexture asan_t3.pfm trailing words\nsphere 3 0 0 1\ntexture none\nsphere 4 0 0 1\ntexture asan_t2.pfm\nsphere 5 0 0 1\n", fp);
			for(int k = 0; k < SKR_TEX_MAX + 2; k++)
			{ // more distinct names than a scene holds: copies of one file
				char name[64];
				snprintf(name, sizeof name, "build/asan_many%02d.pfm", k);
				skr_write_pfm(name, 1, 1, t2.data());
				fprintf(fp, "texture asan_many%02d.pfm\nsphere %d 0 0 1\n", k, 6 + k);
			}
			fclose(fp);
		}
		for(uint32_t flags : {0u, (uint32_t) SKR_SCN_TEXTURE, (uint32_t) (SKR_SCN_TEXTURE | SKR_SCN_MOTION | SKR_SCN_STRICT)})
		{
			skr_scene *sc = nullptr;
			if(skr_scene_create_from_scn_ex("build/asan_tex.scn", 0, flags, &sc) != 0) continue;
			skr_scene_info info;
			skr_scene_get_info(sc, &info);
			int32_t n = -1;
			skr_scene_get_sphere_textures(sc, nullptr, &n);
			std::vector<int32_t> idx((size_t) (n > 0 ? n : 0) + 1, 77);
			skr_scene_get_sphere_textures(sc, idx.data(), &n);
			printf("tex: flags %u spheres %d unknown %d textures %d, indices", flags, n, info.n_unknown, skr_scene_texture_count(sc));
			for(int32_t i = 0; i < n; i++) printf(" %d", idx[(size_t) i]);
			printf(", guard %d\n", idx[(size_t) n]);
			for(int k = 0; k < skr_scene_texture_count(sc); k++)
			{
				int32_t e = -1;
				skr_scene_get_texture(sc, k, nullptr, &e);
				std::vector<float> got((size_t) e * e * 3 + 1, -1.0f);
				skr_scene_get_texture(sc, k, got.data(), &e);
				if(k < 2) printf("tex: texture %d edge %d first %g last %g guard %g\n", k, e, got[0], got[got.size() - 2], got.back());
			}
			blob_table(sc, "tex", "parsed");
			skr_scene_destroy(sc);
		}
		skr_scene *sc = nullptr;
		if(skr_scene_create_from_scn("build/bad1.scn", 0, &sc) == 0)
		{
			skr_scene_info info;
			skr_scene_get_info(sc, &info);
			const int a = skr_scene_add_texture(sc, t2.data(), 2), b = skr_scene_add_texture(sc, t3.data(), 3);
			const int zero = skr_scene_add_texture(sc, t2.data(), 0), neg = skr_scene_add_texture(sc, t2.data(), -3), big = skr_scene_add_texture(sc, t2.data(), SKR_TEX_MAX_EDGE + 1),
					  null = skr_scene_add_texture(sc, nullptr, 2);
			t3[26] = NAN;
			const int not_finite = skr_scene_add_texture(sc, t3.data(), 3);
			printf("tex: add %d %d, refused %d %d %d %d %d, count %d\n", a, b, zero, neg, big, null, not_finite, skr_scene_texture_count(sc));
			std::vector<int32_t> idx((size_t) info.n_spheres, 1), back((size_t) info.n_spheres + 1, 77);
			if(!idx.empty()) idx[0] = -1;
			const int set = skr_scene_set_sphere_textures(sc, idx.data(), info.n_spheres), shorter = skr_scene_set_sphere_textures(sc, idx.data(), info.n_spheres - 1),
					  longer = skr_scene_set_sphere_textures(sc, idx.data(), info.n_spheres + 1), null_idx = skr_scene_set_sphere_textures(sc, nullptr, info.n_spheres);
			if(!idx.empty()) idx.back() = 2;
			const int outside = skr_scene_set_sphere_textures(sc, idx.data(), info.n_spheres);
			if(!idx.empty()) idx.back() = -2;
			const int below = skr_scene_set_sphere_textures(sc, idx.data(), info.n_spheres);
			int32_t n = -1;
			skr_scene_get_sphere_textures(sc, back.data(), &n);
			printf("tex: set %d, refused %d %d %d %d %d, n %d first %d last %d guard %d\n", set, shorter, longer, null_idx, outside, below, n, back[0], n > 0 ? back[(size_t) n - 1] : 0, back[(size_t) n]);
			int32_t e = -1;
			printf("tex: get outside %d %d\n", skr_scene_get_texture(sc, -1, nullptr, &e), skr_scene_get_texture(sc, 2, nullptr, &e));
			blob_table(sc, "tex", "set");
			const int cleared = skr_scene_clear_textures(sc);
			skr_scene_get_sphere_textures(sc, back.data(), &n);
			printf("tex: cleared %d first %d count %d\n", cleared, back[0], skr_scene_texture_count(sc));
			for(int k = 2; k < SKR_TEX_MAX + 1; k++)
			{
				const int rc = skr_scene_add_texture(sc, t2.data(), 1);
				if(k >= SKR_TEX_MAX - 1) printf("tex: add %d -> %d\n", k, rc);
			}
			skr_scene_destroy(sc);
		}
		printf("tex: null scene %d %d %d %d %d %d\n", skr_scene_add_texture(nullptr, t2.data(), 2), skr_scene_texture_count(nullptr), skr_scene_get_texture(nullptr, 0, nullptr, nullptr),
			   skr_scene_set_sphere_textures(nullptr, nullptr, 0), skr_scene_get_sphere_textures(nullptr, nullptr, nullptr), skr_scene_clear_textures(nullptr));
	}
	{ // sphere emission: the setter and the getter with good and bad arguments, and the parser's `emission` lines, valid, malformed, negative and not finite
		FILE *fp = fopen("build/asan_emit.scn", "w");
		if(fp)
		{
			fputs("sphere 0 0 0 1\nemission 1 0.5 0.25\nsphere 1 0 0 1\nemission\nemission  \t \nemission 1 2\nemission 1 -2 3\nemission nan 0 0\nemission 0 inf 0\nemission 0 0 -inf\nemission a b c\n"
				  "emission 1e39 0 0\nsphere 2 0 0 1\nemission 0 0 7 trailing words\nsphere 3 0 0 1\nemission 0 0 0\nsphere 4 0 0 1\nemission -0 -0 -0\nsphere 5 0 0 1\nemission 1e-46 3 3\nsphere 6 0 0 1\n", fp);
			fclose(fp);
		}
		for(uint32_t flags : {0u, (uint32_t) SKR_SCN_EMISSION, (uint32_t) (SKR_SCN_EMISSION | SKR_SCN_TEXTURE | SKR_SCN_MOTION | SKR_SCN_STRICT)})
		{
			skr_scene *sc = nullptr;
			if(skr_scene_create_from_scn_ex("build/asan_emit.scn", 0, flags, &sc) != 0) continue;
			skr_scene_info info;
			skr_scene_get_info(sc, &info);
			int32_t n = -1;
			skr_scene_get_sphere_emission(sc, nullptr, &n);
			std::vector<float> e((size_t) (n > 0 ? n : 0) * 3 + 1, 77.0f);
			skr_scene_get_sphere_emission(sc, e.data(), &n);
			printf("emit: flags %u spheres %d unknown %d, emission", flags, n, info.n_unknown);
			for(int32_t i = 0; i < 3 * n; i++) printf(" %g", e[(size_t) i]);
			printf(", guard %g\n", e[(size_t) n * 3]);
			blob_table(sc, "emit", "parsed");
			skr_scene_destroy(sc);
		}
		skr_scene *sc = nullptr;
		if(skr_scene_create_from_scn("build/bad1.scn", 0, &sc) == 0)
		{
			skr_scene_info info;
			skr_scene_get_info(sc, &info);
			const int32_t ns = info.n_spheres;
			std::vector<float> e((size_t) ns * 3 + 3, 0.5f), back((size_t) ns * 3 + 1, 77.0f);
			if(ns > 0) e[1] = -0.0f;
			const int set = skr_scene_set_sphere_emission(sc, e.data(), ns), shorter = skr_scene_set_sphere_emission(sc, e.data(), ns - 1), longer = skr_scene_set_sphere_emission(sc, e.data(), ns + 1),
					  negative_n = skr_scene_set_sphere_emission(sc, e.data(), -ns);
			int refused[4] = {0, 0, 0, 0};
			const float bad[4] = {NAN, INFINITY, -INFINITY, -1.0f};
			for(int k = 0; k < 4 && ns > 0; k++)
			{ // the last component of the last sphere: the whole array is read before anything is stored
				e[(size_t) ns * 3 - 1] = bad[k];
				refused[k] = skr_scene_set_sphere_emission(sc, e.data(), ns);
			}
			int32_t n = -1;
			skr_scene_get_sphere_emission(sc, back.data(), &n);
			printf("emit: set %d, refused %d %d %d, %d %d %d %d, n %d first %g %g last %g guard %g\n", set, shorter, longer, negative_n, refused[0], refused[1], refused[2], refused[3], n,
				   n > 0 ? back[0] : 0.0f, n > 0 ? back[1] : 0.0f, n > 0 ? back[(size_t) n * 3 - 1] : 0.0f, back[(size_t) n * 3]);
			blob_table(sc, "emit", "set");
			const int cleared = skr_scene_set_sphere_emission(sc, nullptr, ns);
			skr_scene_get_sphere_emission(sc, back.data(), &n);
			e[(size_t) ns * 3 - (ns > 0 ? 1 : 0)] = 0.5f;
			const int again = skr_scene_set_sphere_emission(sc, e.data(), ns), zero_n = skr_scene_set_sphere_emission(sc, e.data(), 0);
			printf("emit: cleared %d first %g, set %d, n = 0 clears %d\n", cleared, n > 0 ? back[0] : 0.0f, again, zero_n);
			skr_scene_destroy(sc);
		}
		printf("emit: null scene %d %d\n", skr_scene_set_sphere_emission(nullptr, nullptr, 0), skr_scene_get_sphere_emission(nullptr, nullptr, nullptr));
	}
	return 0;
}
