// The scene on the host: the error string, the .scn loader, finalize() with the light and material rows, the C API of a scene
// (setters, getters), options defaults and the image writers (PPM, PFM, PNG): the host side of the drop-in boundary.  Behavioural
// restatement of reference src/scene.cpp:12-227, src/utils.h:26-34 and src/main.cpp:199-211.  The tables finalize() derives for
// the kernels are built in scene_masks.cpp (cube_cells, build_shadow_masks, build_gi_masks, build_gi_surface, build_shadow_surface)
// and scene_trees.cpp (build_triangle_chunks, skr_build_sphere_tree).  No GPU code in this file.
#include "scene_host.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <fstream>

static thread_local char g_err[512] = "";

void skr_set_error(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
}

extern "C" const char *skr_last_error(void) { return g_err; }

namespace {

// Reads up to n floats the way sscanf("%f ...") does (strtof underneath);
// fields that are missing stay 0 (the reference leaves them uninitialised).
int read_floats(const char *p, float *dst, int n)
{
	int got = 0;
	for(; got < n; got++)
	{
		char *end = nullptr;
		float v = strtof(p, &end);
		if(end == p) break;
		dst[got] = v;
		p = end;
	}
	return got;
}

struct Material { // material.h:9-17
	float ambient[3] = {0, 0, 0}, diffuse[3] = {0, 0, 0}, specular[3] = {0, 0, 0};
	float power = 1.0f;
	float ior = 1.0f; // (only the dead code of raytrace.h:45-103 reads it: --legacy-reflect)
};

} // namespace

void skr_scene::finalize()
{
	const int ns = info.n_spheres, nt = info.n_triangles;
	sph_geom.resize(ns);
	sph_amb.resize(ns);
	sph_kd.resize(ns);
	sph_ks.resize(ns);
	for(int i = 0; i < ns; i++)
	{
		const float *s = &raw_spheres[(size_t) i * 14];
		sph_geom[i] = {s[0], s[1], s[2], s[3] * s[3]};
		sph_amb[i] = {info.ambient[0] * s[4], info.ambient[1] * s[5], info.ambient[2] * s[6], s[13]};
		sph_kd[i] = {s[7], s[8], s[9], 0.0f};
		sph_ks[i] = {s[10], s[11], s[12], (size_t) i < raw_sphere_ior.size() ? raw_sphere_ior[i] : 1.0f};
	}
	build_lights();
	tri_order = skr_triangle_order(raw_triangles, nt); // (scene_trees.cpp: the order of tris[] is free)
	tris.assign((size_t) nt * 3 + 3, skr_f4{0.0f, 0.0f, 0.0f, 0.0f}); // + one pad triangle (kernel prefetch)
	for(int i = 0; i < nt; i++)
	{
		const float *t = &raw_triangles[(size_t) tri_order[i] * 9];
		tris[3 * i] = {t[0], t[1], t[2], 0.0f};
		float file_index;
		const int32_t fi = tri_order[i];
		memcpy(&file_index, &fi, 4);
		tris[3 * i + 1] = {t[3] - t[0], t[4] - t[1], t[5] - t[2], file_index};
		tris[3 * i + 2] = {t[6] - t[0], t[7] - t[1], t[8] - t[2], 0.0f};
	}
	build_triangle_materials();
	build_triangle_chunks();
	build_shadow_masks();
	build_gi_masks();
	build_gi_surface();
	build_shadow_surface(); // (behind the GI patches: it takes its cell edge from theirs)
}

// The light table: point lights first, then the spot lights (SKR_SCN_SPOT: point-light rows at their positions, the cone is the
// kernels' business), then (--strict-scn) the directional ones: the order blinn_phong.h:50-85 / :95-131 adds them in.  And what the
// host derives once per spot light (include/skr.h skr_scene_get_spot_cones), in binary32, one IEEE operation per step.
void skr_scene::build_lights()
{
	const int nl = info.n_point_lights, nsp = n_spot();
	const int nd = (int) (raw_directional_lights.size() / 6);
	lights.resize((size_t) (nl + nsp + nd) * 2);
	for(int i = 0; i < nl; i++)
	{
		const float *l = &raw_point_lights[(size_t) i * 6];
		lights[2 * i] = {l[0], l[1], l[2], 0.0f};
		lights[2 * i + 1] = {l[3], l[4], l[5], 0.0f};
	}
	light_radii.resize((size_t) (nl + nsp), 0.0f); // (a new light is a point; skr_scene_set_spot_lights resets them all)
	spot_cones.resize((size_t) nsp * 2);
	for(int i = 0; i < nsp; i++)
	{
		const float *l = &raw_spot_lights[(size_t) i * 11]; // r g b px py pz dx dy dz angle1 angle2
		lights[2 * (nl + i)] = {l[3], l[4], l[5], 0.0f};
		lights[2 * (nl + i) + 1] = {l[0], l[1], l[2], 0.0f}; // (not clamped: a point light with a cone)
		const float ss = (l[6] * l[6] + l[7] * l[7]) + l[8] * l[8];
		const float inv = 1.0f / sqrtf(ss); // the device's normalize3: v * (1 / sqrt(v . v))
		const float c1 = (float) cos((double) l[9] * (M_PI / 180.0)), c2 = (float) cos((double) l[10] * (M_PI / 180.0));
		spot_cones[2 * i] = {l[6] * inv, l[7] * inv, l[8] * inv, c1};
		spot_cones[2 * i + 1] = {c2 < c1 ? c2 : c1, 0.0f, 0.0f, 0.0f};
	}
	for(int i = 0; i < nd; i++)
	{
		const float *l = &raw_directional_lights[(size_t) i * 6];
		lights[2 * (nl + nsp + i)] = {l[0], l[1], l[2], 1.0f}; // .w = 1: a direction, not a position (shade_common.h light_term)
		lights[2 * (nl + nsp + i) + 1] = {l[3], l[4], l[5], 0.0f};
	}
}

bool skr_spot_row_ok(const float row[11])
{
	for(int k = 0; k < 11; k++)
		if(!std::isfinite(row[k])) return false;
	if(row[6] == 0.0f && row[7] == 0.0f && row[8] == 0.0f) return false;
	return 0.0f <= row[9] && row[9] <= row[10] && row[10] <= 180.0f;
}

void skr_scene::build_triangle_materials()
{
	const int nt = info.n_triangles;
	tri_mats.assign((size_t) nt * 3, skr_f4{0.0f, 0.0f, 0.0f, 0.0f});
	for(int i = 0; i < nt; i++)
	{
		const Material dflt;
		const size_t at = (size_t) tri_order[i] * 10;
		const bool have = at + 10 <= raw_triangle_materials.size();
		const float *m = have ? &raw_triangle_materials[at] : dflt.ambient;
		const float power = have ? m[9] : dflt.power;
		const float *kd = have ? m + 3 : dflt.diffuse, *ks = have ? m + 6 : dflt.specular;
		tri_mats[3 * i] = {info.ambient[0] * m[0], info.ambient[1] * m[1], info.ambient[2] * m[2], power};
		tri_mats[3 * i + 1] = {kd[0], kd[1], kd[2], 0.0f};
		tri_mats[3 * i + 2] = {ks[0], ks[1], ks[2], 0.0f};
	}
}

static void set_camera(skr_scene_info &info, const float p[3], const float d[3], const float u[3], float ha)
{
	for(int k = 0; k < 3; k++)
	{
		info.camera[k] = p[k];
		info.camera[3 + k] = d[k]; // scene.cpp:92-93 discard normalize(): file magnitudes are kept
		info.camera[6 + k] = u[k];
	}
	// camera.h:30: right = cross(direction * -1.0f, up), glm::cross operand order
	const float nx = d[0] * -1.0f, ny = d[1] * -1.0f, nz = d[2] * -1.0f;
	info.camera[9] = ny * u[2] - u[1] * nz;
	info.camera[10] = nz * u[0] - u[2] * nx;
	info.camera[11] = nx * u[1] - u[0] * ny;
	info.camera[12] = ha;
}

int skr_parse_scn(const std::string &path, bool echo, uint32_t flags, skr_scene &sc)
{
	const bool strict = (flags & SKR_SCN_STRICT) != 0, fog = (flags & SKR_SCN_FOG) != 0, spot = (flags & SKR_SCN_SPOT) != 0;
	const bool motion = (flags & SKR_SCN_MOTION) != 0;
	float vel[3] = {0.0f, 0.0f, 0.0f}; // SKR_SCN_MOTION: the velocity in force for the sphere lines that follow, stateful as `material` is
	std::vector<float> vels;
	const bool texture = (flags & SKR_SCN_TEXTURE) != 0;
	int32_t tex = -1; // SKR_SCN_TEXTURE: the texture in force for the sphere lines that follow (-1: none), stateful as `material` is
	std::vector<int32_t> texs;
	std::vector<std::string> tex_names; // the resolved name of texture k: the same name twice is one texture
	const bool emission = (flags & SKR_SCN_EMISSION) != 0;
	float emi[3] = {0.0f, 0.0f, 0.0f}; // SKR_SCN_EMISSION: the emission in force for the sphere lines that follow, stateful as `material` is
	std::vector<float> emis;
	FILE *fp = fopen(path.c_str(), "r");
	if(!fp)
	{
		skr_set_error("Can't open file '%s'", path.c_str()); // scene.cpp:24
		return SKR_ERR_IO;
	}
	sc = skr_scene();
	sc.strict = strict;
	skr_scene_info &info = sc.info;
	info.film_width = 1920; // scene.h:15
	info.film_height = 1080;
	info.max_depth_parsed = 1; // scene.h:26
	Material mat;
	std::vector<float> verts;

	char line[1024]; // scene.cpp:19: lines are read in 1024-byte pieces
	while(fgets(line, sizeof line, fp))
	{
		if(line[0] == '#')
		{
			if(echo) printf("Skipping comment: %s\n", line);
			continue;
		}
		// first whitespace-delimited token = command
		const char *p = line;
		while(*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n' || *p == '\v' || *p == '\f') p++;
		if(!*p) continue;
		const char *q = p;
		while(*q && !(*q == ' ' || *q == '\t' || *q == '\r' || *q == '\n' || *q == '\v' || *q == '\f')) q++;
		const std::string cmd(p, q);
		const char *args = q;

		if(cmd == "sphere")
		{
			float v[4] = {0, 0, 0, 0};
			read_floats(args, v, 4);
			if(echo) printf("Sphere as position (%f, %f, %f) with radius %f\n", v[0], v[1], v[2], v[3]);
			const float rec[14] = {v[0], v[1], v[2], v[3], mat.ambient[0], mat.ambient[1], mat.ambient[2],
								   mat.diffuse[0], mat.diffuse[1], mat.diffuse[2], mat.specular[0], mat.specular[1], mat.specular[2], mat.power};
			sc.raw_spheres.insert(sc.raw_spheres.end(), rec, rec + 14);
			sc.raw_sphere_ior.push_back(mat.ior);
			vels.insert(vels.end(), vel, vel + 3);
			texs.push_back(tex);
			emis.insert(emis.end(), emi, emi + 3);
			info.n_spheres++;
		}
		else if(cmd == "vertex")
		{
			float v[3] = {0, 0, 0};
			read_floats(args, v, 3);
			verts.insert(verts.end(), v, v + 3);
			info.n_vertices++;
		}
		else if(cmd == "triangle")
		{
			float v[3] = {0, 0, 0}; // scene.cpp:69-70: indices are read as floats
			read_floats(args, v, 3);
			// the float is range-checked BEFORE the conversion: (long) of nan, inf or 1e39 is undefined behaviour
			long idx[3] = {0, 0, 0};
			bool ok = true;
			for(int k = 0; k < 3; k++)
			{
				ok = ok && std::isfinite(v[k]) && v[k] > -1.0f && v[k] < (float) info.n_vertices; // (long) truncates: -0.5 -> 0
				if(ok) idx[k] = (long) v[k];
			}
			for(long i : idx) ok = ok && i >= 0 && i < info.n_vertices;
			if(!ok)
			{ // the reference reads out of bounds here; no shipped scene does
				fprintf(stderr, "WARNING. triangle references a vertex outside the pool (%d vertices so far): skipped\n", info.n_vertices);
				info.n_bad_triangles++;
				continue;
			}
			for(long i : idx) sc.raw_triangles.insert(sc.raw_triangles.end(), &verts[(size_t) i * 3], &verts[(size_t) i * 3] + 3);
			{
				const float rec[10] = {mat.ambient[0], mat.ambient[1], mat.ambient[2], mat.diffuse[0], mat.diffuse[1], mat.diffuse[2],
									   mat.specular[0], mat.specular[1], mat.specular[2], mat.power};
				sc.raw_triangle_materials.insert(sc.raw_triangle_materials.end(), rec, rec + 10);
			}
			info.n_triangles++;
		}
		else if(cmd == "camera")
		{
			float v[10] = {0};
			read_floats(args, v, 10);
			if(echo)
				printf("Camera with position (%f, %f, %f) with viewing direction (%f, %f, %f), up glm::vec3 (%f, %f, %f), and halfHeightAngle %f\n",
					   v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]);
			set_camera(info, v, v + 3, v + 6, v[9]);
			// (the reference also drops a "simplesphere.txt" camera dump into the CWD here,
			//  scene.cpp:96-102 — a debugging leftover that is deliberately not reproduced)
		}
		else if(cmd == "film_resolution")
		{
			int w = info.film_width, h = info.film_height;
			sscanf(args, "%d %d", &w, &h);
			info.film_width = w;
			info.film_height = h;
			if(echo) printf("Film resolution: %d x %d\n", w, h);
		}
		else if(cmd == "background")
		{
			float v[3] = {0, 0, 0};
			read_floats(args, v, 3);
			if(echo) printf("Background color of (%f,%f,%f)\n", v[0], v[1], v[2]);
			memcpy(info.background, v, sizeof v);
		}
		else if(cmd == "material")
		{
			float v[14] = {0};
			read_floats(args, v, 14);
			if(echo)
				printf("material properties with ambient colour (%f, %f, %f), diffuse colour (%f, %f, %f), specular colour (%f, %f, %f), phong Cosine power %f, transmissive colour (%f, %f, %f), index of refraction %f\n",
					   v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13]);
			memcpy(mat.ambient, v, 12);
			memcpy(mat.diffuse, v + 3, 12);
			memcpy(mat.specular, v + 6, 12);
			mat.power = v[9]; // the transmissive colour feeds only dead code (raytrace.h:45-103)
			mat.ior = v[13];  // so does this one: kept for --legacy-reflect
		}
		else if(cmd == "directional_light")
		{
			float v[6] = {0};
			read_floats(args, v, 6);
			if(echo) printf("directional light colour (%f, %f, %f), direction (%f, %f, %f)\n", v[0], v[1], v[2], v[3], v[4], v[5]);
			if(!strict) info.n_directional_dropped++; // scene.cpp:157-163: built, never pushed
			else
			{ // --strict-scn: pushed, with the clamp of scene.cpp:143-154
				for(int k = 0; k < 3; k++)
					if(v[k] > 1) v[k] = 1;
				const float rec[6] = {v[3], v[4], v[5], v[0], v[1], v[2]}; // file order is colour then direction
				sc.raw_directional_lights.insert(sc.raw_directional_lights.end(), rec, rec + 6);
				info.n_directional_lights++;
			}
		}
		else if(cmd == "point_light")
		{
			float v[6] = {0};
			read_floats(args, v, 6);
			if(echo) printf("point light colour (%f, %f, %f), located at (%f, %f, %f)\n", v[0], v[1], v[2], v[3], v[4], v[5]);
			const float rec[6] = {v[3], v[4], v[5], v[0], v[1], v[2]}; // file order is colour then position
			sc.raw_point_lights.insert(sc.raw_point_lights.end(), rec, rec + 6);
			info.n_point_lights++;
		}
		else if(cmd == "ambient_light")
		{
			float v[3] = {0, 0, 0};
			read_floats(args, v, 3);
			if(echo) printf("Ambient light colour (%f, %f, %f)\n", v[0], v[1], v[2]);
			for(int k = 0; k < 3; k++) info.ambient[k] += v[k]; // scene.cpp:187-189 accumulates
		}
		else if(cmd == "max_depth")
		{
			float n = 0;
			read_floats(args, &n, 1);
			if(echo) printf("max_depth %f\n", n);
			info.max_depth_parsed = (std::isfinite(n) && n > -2147483648.0f && n < 2147483648.0f) ? (int) n : 0; // (int) of nan / 1e30 is undefined
		}
		else if(cmd == "output_image")
		{
			if(echo) printf("Render to file named: %s", args + (*args ? 1 : 0));
		}
		else if(cmd == "spherical_fog")
		{
			// scene.cpp:207-212 pushes a fog volume built from uninitialised floats
			// (sscanf "fog ..." never matches): undefined behaviour, pinned as "ignored".
			// SKR_SCN_FOG: the fields in the order of that sscanf, x y z radius r g b scattering [absorption = 0]
			float v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
			const int got = fog ? read_floats(args, v, 9) : 0;
			if(got >= 8)
			{
				if(echo) printf("spherical fog at (%f, %f, %f), radius %f, albedo (%f, %f, %f), scattering %f, absorption %f\n", v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]);
				sc.raw_fog.insert(sc.raw_fog.end(), v, v + 9);
			}
			else
			{
				fprintf(stderr, fog ? "WARNING. spherical_fog needs at least 8 numbers (x y z radius r g b scattering [absorption]): line skipped\n"
				                    : "WARNING. spherical_fog is not reproducible in the reference (uninitialised data): line skipped\n");
				info.n_fog_skipped++;
			}
		}
		else if(spot && cmd == "spot_light")
		{ // SKR_SCN_SPOT (the reference does not know the command, scene.cpp:214-217): r g b px py pz dx dy dz angle1 angle2
			float v[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
			const int got = read_floats(args, v, 11);
			if(got == 11 && skr_spot_row_ok(v) && sc.n_spot() < SKR_SPOT_MAX_LIGHTS)
			{
				if(echo) printf("spot light colour (%f, %f, %f), located at (%f, %f, %f), direction (%f, %f, %f), angles %f %f\n", v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]);
				sc.raw_spot_lights.insert(sc.raw_spot_lights.end(), v, v + 11);
			}
			else
			{
				fprintf(stderr, "WARNING. spot_light needs 11 finite numbers (r g b px py pz dx dy dz angle1 angle2), a direction other than zero and 0 <= angle1 <= angle2 <= 180 (at most %d spot lights): line skipped\n", SKR_SPOT_MAX_LIGHTS);
				info.n_unknown++;
			}
		}
		else if(motion && cmd == "velocity")
		{ // SKR_SCN_MOTION (the reference does not know the command): vx vy vz
			float v[3] = {0, 0, 0};
			const int got = read_floats(args, v, 3);
			if(got == 3 && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]))
			{
				if(echo) printf("velocity (%f, %f, %f)\n", v[0], v[1], v[2]);
				memcpy(vel, v, sizeof vel);
			}
			else
			{
				fprintf(stderr, "WARNING. velocity needs 3 finite numbers (vx vy vz): line skipped\n");
				info.n_unknown++;
			}
		}
		else if(emission && cmd == "emission")
		{ // SKR_SCN_EMISSION (the reference does not know the command): r g b
			float v[3] = {0, 0, 0};
			const int got = read_floats(args, v, 3);
			if(got == 3 && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && v[0] >= 0.0f && v[1] >= 0.0f && v[2] >= 0.0f)
			{
				if(echo) printf("emission (%f, %f, %f)\n", v[0], v[1], v[2]);
				memcpy(emi, v, sizeof emi);
			}
			else
			{
				fprintf(stderr, "WARNING. emission needs 3 finite numbers that are not negative (r g b): line skipped\n");
				info.n_unknown++;
			}
		}
		else if(texture && cmd == "texture")
		{ // SKR_SCN_TEXTURE (the reference does not know the command): NAME, a square colour PFM, or `none`
			const char *a = args;
			while(*a == ' ' || *a == '\t' || *a == '\r' || *a == '\n' || *a == '\v' || *a == '\f') a++;
			const char *b = a;
			while(*b && !(*b == ' ' || *b == '\t' || *b == '\r' || *b == '\n' || *b == '\v' || *b == '\f')) b++;
			std::string name(a, b);
			const char *why = nullptr;
			if(name.empty()) why = "needs the name of a square colour PFM file, or none";
			else if(name == "none")
			{
				if(echo) printf("texture none\n");
				tex = -1;
			}
			else
			{
				if(name[0] != '/')
				{ // a relative name is the scene file's neighbour
					const size_t slash = path.find_last_of('/');
					if(slash != std::string::npos) name = path.substr(0, slash + 1) + name;
				}
				int32_t k = 0;
				while(k < (int32_t) tex_names.size() && tex_names[(size_t) k] != name) k++;
				if(k == (int32_t) tex_names.size())
				{
					uint32_t tw = 0, th = 0;
					std::vector<float> texels;
					if(k >= SKR_TEX_MAX) why = "would be one texture too many";
					else if(skr_read_pfm(name.c_str(), &tw, &th, nullptr) != SKR_OK) why = "names a file that cannot be read as a colour PFM";
					else if(tw != th || tw > (uint32_t) SKR_TEX_MAX_EDGE) why = "names a file that is not square or has too long an edge";
					else
					{
						texels.resize((size_t) tw * th * 3);
						if(skr_read_pfm(name.c_str(), &tw, &th, texels.data()) != SKR_OK) why = "names a file that cannot be read as a colour PFM";
						for(size_t i = 0; !why && i < texels.size(); i++)
							if(!std::isfinite(texels[i])) why = "names a file with a texel that is not finite";
					}
					if(!why)
					{
						sc.textures.push_back(std::move(texels));
						sc.texture_edges.push_back((int32_t) tw);
						tex_names.push_back(name);
					}
				}
				if(!why)
				{
					if(echo) printf("texture %d: %s (%d x %d)\n", k, name.c_str(), sc.texture_edges[(size_t) k], sc.texture_edges[(size_t) k]);
					tex = k;
				}
			}
			if(why)
			{
				fprintf(stderr, "WARNING. texture %s (at most %d textures, edges up to %d): line skipped\n", why, SKR_TEX_MAX, SKR_TEX_MAX_EDGE);
				info.n_unknown++;
			}
		}
		else
		{
			if(echo) printf("WARNING. Do not know command: %s\n", cmd.c_str());
			info.n_unknown++;
		}
	}
	fclose(fp);
	sc.finalize();
	if(motion) sc.velocities = vels;
	if(texture) sc.sphere_textures = texs;
	if(emission) sc.emission = emis;
	return SKR_OK;
}

extern "C" {

int skr_scene_create_from_scn(const char *path, int echo, skr_scene **out) { return skr_scene_create_from_scn_ex(path, echo, 0, out); }

int skr_scene_create_from_scn_ex(const char *path, int echo, uint32_t flags, skr_scene **out)
{
	if(!path || !out)
	{
		skr_set_error("skr_scene_create_from_scn: null argument");
		return SKR_ERR_ARG;
	}
	skr_scene *sc = new skr_scene();
	int rc = skr_parse_scn(path, echo != 0, flags, *sc);
	if(rc != SKR_OK)
	{
		delete sc;
		*out = nullptr;
		return rc;
	}
	sc->triangle_shadows = (flags & SKR_SCN_TRIANGLE_SHADOWS) != 0;
	sc->sphere_tree = (flags & SKR_SCN_SPHERE_TREE) != 0;
	*out = sc;
	return SKR_OK;
}

int skr_scene_create_from_arrays(const float *spheres, int32_t n_spheres, const float *triangles, int32_t n_triangles,
								 const float *point_lights, int32_t n_point_lights, const float camera[9],
								 const float background[3], const float ambient[3], skr_scene **out)
{
	if(!out || !camera || n_spheres < 0 || n_triangles < 0 || n_point_lights < 0 || (n_spheres && !spheres) ||
	   (n_triangles && !triangles) || (n_point_lights && !point_lights))
	{
		skr_set_error("skr_scene_create_from_arrays: bad argument");
		return SKR_ERR_ARG;
	}
	skr_scene *sc = new skr_scene();
	sc->info.film_width = 1920;
	sc->info.film_height = 1080;
	sc->info.max_depth_parsed = 1;
	sc->info.n_spheres = n_spheres;
	sc->info.n_triangles = n_triangles;
	sc->info.n_point_lights = n_point_lights;
	sc->raw_spheres.assign(spheres, spheres + (size_t) n_spheres * 14);
	sc->raw_triangles.assign(triangles, triangles + (size_t) n_triangles * 9);
	sc->raw_point_lights.assign(point_lights, point_lights + (size_t) n_point_lights * 6);
	set_camera(sc->info, camera, camera + 3, camera + 6, 0.0f);
	if(background) memcpy(sc->info.background, background, 12);
	if(ambient) memcpy(sc->info.ambient, ambient, 12);
	sc->finalize();
	*out = sc;
	return SKR_OK;
}

int skr_scene_set_triangle_materials(skr_scene *scene, const float *materials)
{
	if(!scene || (scene->info.n_triangles && !materials))
	{
		skr_set_error("skr_scene_set_triangle_materials: bad argument");
		return SKR_ERR_ARG;
	}
	scene->raw_triangle_materials.assign(materials, materials + (size_t) scene->info.n_triangles * 10);
	scene->build_triangle_materials();
	return SKR_OK;
}

int skr_scene_set_sphere_ior(skr_scene *scene, const float *ior)
{
	if(!scene || (scene->info.n_spheres && !ior))
	{
		skr_set_error("skr_scene_set_sphere_ior: bad argument");
		return SKR_ERR_ARG;
	}
	scene->raw_sphere_ior.assign(ior, ior + scene->info.n_spheres);
	for(int i = 0; i < scene->info.n_spheres; i++) scene->sph_ks[i].w = ior[i];
	return SKR_OK;
}

int skr_scene_set_fog(skr_scene *scene, const float *rows, int32_t n)
{
	if(!scene || n < 0 || n > SKR_FOG_MAX_VOLUMES || (n && !rows))
	{
		skr_set_error("skr_scene_set_fog: bad argument (at most %d fog volumes)", SKR_FOG_MAX_VOLUMES);
		return SKR_ERR_ARG;
	}
	scene->raw_fog.assign(rows, rows + (size_t) n * 9);
	return SKR_OK;
}

int skr_scene_get_fog(const skr_scene *scene, float *rows, int32_t *n)
{
	if(!scene) return SKR_ERR_ARG;
	if(n) *n = (int32_t) (scene->raw_fog.size() / 9);
	if(rows && !scene->raw_fog.empty()) memcpy(rows, scene->raw_fog.data(), scene->raw_fog.size() * 4);
	return SKR_OK;
}

int skr_scene_set_spot_lights(skr_scene *scene, const float *rows, int32_t n)
{
	if(!scene || n < 0 || n > SKR_SPOT_MAX_LIGHTS || (n && !rows))
	{
		skr_set_error("skr_scene_set_spot_lights: bad argument (at most %d spot lights)", SKR_SPOT_MAX_LIGHTS);
		return SKR_ERR_ARG;
	}
	for(int32_t i = 0; i < n; i++)
		if(!skr_spot_row_ok(rows + (size_t) i * 11))
		{
			skr_set_error("skr_scene_set_spot_lights: row %d is not a spot light (11 finite numbers, a direction other than zero, 0 <= angle1 <= angle2 <= 180)", i);
			return SKR_ERR_ARG;
		}
	scene->raw_spot_lights.assign(rows, rows + (size_t) n * 11);
	scene->light_radii.clear(); // (the light count changes: every radius is 0 again, include/skr.h)
	scene->build_lights();
	scene->build_shadow_masks(); // (a spot light has a table like the point light it geometrically is)
	scene->build_shadow_surface();
	return SKR_OK;
}

int skr_scene_get_spot_lights(const skr_scene *scene, float *rows, int32_t *n)
{
	if(!scene) return SKR_ERR_ARG;
	if(n) *n = (int32_t) scene->n_spot();
	if(rows && !scene->raw_spot_lights.empty()) memcpy(rows, scene->raw_spot_lights.data(), scene->raw_spot_lights.size() * 4);
	return SKR_OK;
}

int skr_scene_set_light_radii(skr_scene *scene, const float *radii, int32_t n)
{
	if(!scene || n < 0 || (n && !radii) || (size_t) n != scene->light_radii.size())
	{
		skr_set_error("skr_scene_set_light_radii: bad argument (one radius per point and spot light: %d)", scene ? (int) scene->light_radii.size() : 0);
		return SKR_ERR_ARG;
	}
	for(int32_t i = 0; i < n; i++)
		if(!std::isfinite(radii[i]) || !(radii[i] >= 0.0f))
		{
			skr_set_error("skr_scene_set_light_radii: radius %d is not a finite number >= 0", i);
			return SKR_ERR_ARG;
		}
	for(int32_t i = 0; i < n; i++) scene->light_radii[i] = radii[i] + 0.0f; // (-0 -> +0)
	return SKR_OK;
}

int skr_scene_get_light_radii(const skr_scene *scene, float *radii, int32_t *n)
{
	if(!scene) return SKR_ERR_ARG;
	if(n) *n = (int32_t) scene->light_radii.size();
	if(radii && !scene->light_radii.empty()) memcpy(radii, scene->light_radii.data(), scene->light_radii.size() * 4);
	return SKR_OK;
}

int skr_scene_set_lens(skr_scene *scene, float aperture, float focus)
{
	if(!scene || !std::isfinite(aperture) || !std::isfinite(focus) || !(aperture >= 0.0f) || !(focus > 0.0f))
	{
		skr_set_error("skr_scene_set_lens: the aperture must be a finite number >= 0 and the focus a finite number > 0");
		return SKR_ERR_ARG;
	}
	scene->lens_aperture = aperture + 0.0f; // (-0 -> +0)
	scene->lens_focus = focus;
	return SKR_OK;
}

int skr_scene_get_lens(const skr_scene *scene, float *aperture, float *focus)
{
	if(!scene) return SKR_ERR_ARG;
	if(aperture) *aperture = scene->lens_aperture;
	if(focus) *focus = scene->lens_focus;
	return SKR_OK;
}

int skr_scene_set_sphere_velocities(skr_scene *scene, const float *v, int32_t n)
{
	if(!scene || n < 0 || n != scene->info.n_spheres || (n && !v))
	{
		skr_set_error("skr_scene_set_sphere_velocities: bad argument (one velocity of 3 floats per sphere: %d)", scene ? scene->info.n_spheres : 0);
		return SKR_ERR_ARG;
	}
	for(size_t i = 0; i < (size_t) n * 3; i++)
		if(!std::isfinite(v[i]))
		{
			skr_set_error("skr_scene_set_sphere_velocities: velocity %zu has a component that is not finite", i / 3);
			return SKR_ERR_ARG;
		}
	scene->velocities.assign(v, v + (size_t) n * 3);
	return SKR_OK;
}

int skr_scene_get_sphere_velocities(const skr_scene *scene, float *v, int32_t *n)
{
	if(!scene) return SKR_ERR_ARG;
	const size_t ns = (size_t) scene->info.n_spheres;
	if(n) *n = (int32_t) ns;
	for(size_t i = 0; v && i < ns * 3; i++) v[i] = i < scene->velocities.size() ? scene->velocities[i] : 0.0f;
	return SKR_OK;
}

int skr_scene_set_shutter(skr_scene *scene, float shutter)
{
	if(!scene || !std::isfinite(shutter) || !(shutter >= 0.0f))
	{
		skr_set_error("skr_scene_set_shutter: the shutter must be a finite number >= 0");
		return SKR_ERR_ARG;
	}
	scene->shutter = shutter + 0.0f; // (-0 -> +0)
	return SKR_OK;
}

int skr_scene_get_shutter(const skr_scene *scene, float *shutter)
{
	if(!scene) return SKR_ERR_ARG;
	if(shutter) *shutter = scene->shutter;
	return SKR_OK;
}

int skr_scene_set_environment(skr_scene *scene, const float *texels, int32_t edge)
{
	if(!scene)
	{
		skr_set_error("skr_scene_set_environment: null scene");
		return SKR_ERR_ARG;
	}
	if(edge == 0 || !texels)
	{ // cleared: misses return the background again
		scene->env_texels.clear();
		scene->env_edge = 0;
		return SKR_OK;
	}
	if(edge < 1 || edge > SKR_ENV_MAX_EDGE)
	{
		skr_set_error("skr_scene_set_environment: the edge must be in [1, %d] (0 clears the environment): %d", SKR_ENV_MAX_EDGE, edge);
		return SKR_ERR_ARG;
	}
	const size_t n = (size_t) edge * (size_t) edge * 3;
	for(size_t i = 0; i < n; i++)
		if(!std::isfinite(texels[i]))
		{
			skr_set_error("skr_scene_set_environment: texel (row %zu, column %zu) has a channel that is not finite", i / 3 / (size_t) edge, i / 3 % (size_t) edge);
			return SKR_ERR_ARG;
		}
	scene->env_texels.assign(texels, texels + n);
	scene->env_edge = edge;
	return SKR_OK;
}

int skr_scene_get_environment(const skr_scene *scene, float *texels, int32_t *edge)
{
	if(!scene) return SKR_ERR_ARG;
	if(edge) *edge = scene->env_edge;
	if(texels && scene->env_edge > 0) memcpy(texels, scene->env_texels.data(), scene->env_texels.size() * sizeof(float));
	return SKR_OK;
}

int skr_scene_add_texture(skr_scene *scene, const float *texels, int32_t edge)
{
	if(!scene || !texels)
	{
		skr_set_error("skr_scene_add_texture: null argument");
		return -SKR_ERR_ARG;
	}
	if(edge < 1 || edge > SKR_TEX_MAX_EDGE)
	{
		skr_set_error("skr_scene_add_texture: the edge must be in [1, %d]: %d", SKR_TEX_MAX_EDGE, edge);
		return -SKR_ERR_ARG;
	}
	if((int) scene->textures.size() >= SKR_TEX_MAX)
	{
		skr_set_error("skr_scene_add_texture: the scene holds %d textures already", SKR_TEX_MAX);
		return -SKR_ERR_ARG;
	}
	const size_t n = (size_t) edge * (size_t) edge * 3;
	for(size_t i = 0; i < n; i++)
		if(!std::isfinite(texels[i]))
		{
			skr_set_error("skr_scene_add_texture: texel (row %zu, column %zu) has a channel that is not finite", i / 3 / (size_t) edge, i / 3 % (size_t) edge);
			return -SKR_ERR_ARG;
		}
	scene->textures.emplace_back(texels, texels + n);
	scene->texture_edges.push_back(edge);
	return (int) scene->textures.size() - 1;
}

int skr_scene_texture_count(const skr_scene *scene) { return scene ? (int) scene->textures.size() : -SKR_ERR_ARG; }

int skr_scene_get_texture(const skr_scene *scene, int32_t k, float *texels, int32_t *edge)
{
	if(!scene || k < 0 || k >= (int32_t) scene->textures.size())
	{
		skr_set_error("skr_scene_get_texture: bad argument (the scene holds %d textures: %d)", scene ? (int) scene->textures.size() : 0, k);
		return SKR_ERR_ARG;
	}
	if(edge) *edge = scene->texture_edges[(size_t) k];
	if(texels) memcpy(texels, scene->textures[(size_t) k].data(), scene->textures[(size_t) k].size() * sizeof(float));
	return SKR_OK;
}

int skr_scene_set_sphere_textures(skr_scene *scene, const int32_t *idx, int32_t n)
{
	if(!scene || n != scene->info.n_spheres || (n > 0 && !idx))
	{
		skr_set_error("skr_scene_set_sphere_textures: bad argument (one texture index per sphere: %d)", scene ? scene->info.n_spheres : 0);
		return SKR_ERR_ARG;
	}
	for(int32_t i = 0; i < n; i++)
		if(idx[i] < -1 || idx[i] >= (int32_t) scene->textures.size())
		{
			skr_set_error("skr_scene_set_sphere_textures: sphere %d names texture %d, outside [-1, %d)", i, idx[i], (int) scene->textures.size());
			return SKR_ERR_ARG;
		}
	scene->sphere_textures.assign(idx, idx + n);
	return SKR_OK;
}

int skr_scene_get_sphere_textures(const skr_scene *scene, int32_t *idx, int32_t *n)
{
	if(!scene) return SKR_ERR_ARG;
	const size_t ns = (size_t) scene->info.n_spheres;
	if(n) *n = (int32_t) ns;
	for(size_t i = 0; idx && i < ns; i++) idx[i] = i < scene->sphere_textures.size() ? scene->sphere_textures[i] : -1;
	return SKR_OK;
}

int skr_scene_clear_textures(skr_scene *scene)
{
	if(!scene) return SKR_ERR_ARG;
	scene->sphere_textures.clear(); // (shorter than the sphere count: -1)
	return SKR_OK;
}

int skr_scene_set_sphere_emission(skr_scene *scene, const float *rgb, int32_t n)
{
	if(!scene)
	{
		skr_set_error("skr_scene_set_sphere_emission: null scene");
		return SKR_ERR_ARG;
	}
	if(!rgb || n == 0)
	{ // no emission
		scene->emission.clear();
		return SKR_OK;
	}
	if(n != scene->info.n_spheres)
	{
		skr_set_error("skr_scene_set_sphere_emission: bad argument (one emission of 3 floats per sphere: %d)", scene->info.n_spheres);
		return SKR_ERR_ARG;
	}
	for(size_t i = 0; i < (size_t) n * 3; i++)
		if(!std::isfinite(rgb[i]) || !(rgb[i] >= 0.0f))
		{
			skr_set_error("skr_scene_set_sphere_emission: emission %zu has a component that is not finite or is negative", i / 3);
			return SKR_ERR_ARG;
		}
	scene->emission.assign(rgb, rgb + (size_t) n * 3);
	return SKR_OK;
}

int skr_scene_get_sphere_emission(const skr_scene *scene, float *rgb, int32_t *n)
{
	if(!scene) return SKR_ERR_ARG;
	const size_t ns = (size_t) scene->info.n_spheres;
	if(n) *n = (int32_t) ns;
	for(size_t i = 0; rgb && i < ns * 3; i++) rgb[i] = i < scene->emission.size() ? scene->emission[i] : 0.0f;
	return SKR_OK;
}

int skr_scene_get_spot_cones(const skr_scene *scene, float *cones)
{
	if(!scene) return SKR_ERR_ARG;
	for(int i = 0; cones && i < scene->n_spot(); i++)
	{
		const skr_f4 a = scene->spot_cones[2 * (size_t) i], b = scene->spot_cones[2 * (size_t) i + 1];
		const float row[5] = {a.x, a.y, a.z, a.w, b.x};
		memcpy(cones + 5 * (size_t) i, row, sizeof row);
	}
	return SKR_OK;
}

int skr_scene_set_triangle_shadows(skr_scene *scene, int enable)
{
	if(!scene)
	{
		skr_set_error("skr_scene_set_triangle_shadows: null scene");
		return SKR_ERR_ARG;
	}
	scene->triangle_shadows = enable != 0;
	return SKR_OK;
}

int skr_scene_get_triangle_shadows(const skr_scene *scene, int *enabled)
{
	if(!scene || !enabled) return SKR_ERR_ARG;
	*enabled = scene->triangle_shadows ? 1 : 0;
	return SKR_OK;
}

int skr_scene_set_sphere_tree(skr_scene *scene, int enable)
{
	if(!scene)
	{
		skr_set_error("skr_scene_set_sphere_tree: null scene");
		return SKR_ERR_ARG;
	}
	scene->sphere_tree = enable != 0;
	return SKR_OK;
}

int skr_scene_get_sphere_tree(const skr_scene *scene, int *enabled)
{
	if(!scene || !enabled) return SKR_ERR_ARG;
	*enabled = scene->sphere_tree ? 1 : 0;
	return SKR_OK;
}

int skr_scene_get_sphere_tree_data(const skr_scene *scene, int32_t *chunk_size, int32_t *n_nodes, int32_t *n_chunks, int32_t *n_always,
								   float *device_spheres, int32_t *file_index, float *node_spheres, int32_t *node_links, float *chunk_spheres,
								   int32_t *chunk_links, float ball[4])
{
	if(!scene) return SKR_ERR_ARG;
	SkrSphereTree t;
	skr_build_sphere_tree(*scene, t);
	if(chunk_size) *chunk_size = SKR_SPHERE_CHUNK;
	if(n_nodes) *n_nodes = t.n_nodes;
	if(n_chunks) *n_chunks = t.n_chunks;
	if(n_always) *n_always = t.n_always;
	if(ball) memcpy(ball, t.ball, 16);
	if(device_spheres && !t.rows.empty()) memcpy(device_spheres, t.rows.data(), t.rows.size() * 16);
	if(file_index && !t.file.empty()) memcpy(file_index, t.file.data(), t.file.size() * 4);
	auto word = [](float f) { int32_t v; memcpy(&v, &f, 4); return v; };
	for(int i = 0; i < t.n_nodes; i++)
	{
		const skr_f4 A = t.nodes[2 * (size_t) i], L = t.nodes[2 * (size_t) i + 1];
		if(node_spheres)
		{
			const float row[5] = {A.x, A.y, A.z, A.w, L.x};
			memcpy(node_spheres + 5 * (size_t) i, row, sizeof row);
		}
		if(node_links)
		{
			const int32_t fc = word(L.z), left = t.n_chunks - fc;
			const int32_t row[4] = {word(L.y), fc < 0 ? 0 : fc, fc < 0 ? 0 : (left < SKR_SPHERE_SUPER ? left : SKR_SPHERE_SUPER), word(L.w)};
			memcpy(node_links + 4 * (size_t) i, row, sizeof row);
		}
	}
	for(int c = 0; c < t.n_chunks; c++)
	{
		const skr_f4 A = t.chunks[3 * (size_t) c], L = t.chunks[3 * (size_t) c + 1];
		if(chunk_spheres)
		{
			const float row[5] = {A.x, A.y, A.z, A.w, L.x};
			memcpy(chunk_spheres + 5 * (size_t) c, row, sizeof row);
		}
		if(chunk_links)
		{
			const int32_t row[3] = {word(L.y), word(L.z), word(L.w)};
			memcpy(chunk_links + 3 * (size_t) c, row, sizeof row);
		}
	}
	return SKR_OK;
}

void skr_scene_destroy(skr_scene *scene) { delete scene; }

int skr_scene_get_info(const skr_scene *scene, skr_scene_info *info)
{
	if(!scene || !info) return SKR_ERR_ARG;
	*info = scene->info;
	return SKR_OK;
}

int skr_scene_get_arrays(const skr_scene *scene, float *spheres, float *triangles, float *point_lights)
{
	if(!scene) return SKR_ERR_ARG;
	if(spheres && !scene->raw_spheres.empty()) memcpy(spheres, scene->raw_spheres.data(), scene->raw_spheres.size() * 4);
	if(triangles && !scene->raw_triangles.empty()) memcpy(triangles, scene->raw_triangles.data(), scene->raw_triangles.size() * 4);
	if(point_lights && !scene->raw_point_lights.empty()) memcpy(point_lights, scene->raw_point_lights.data(), scene->raw_point_lights.size() * 4);
	return SKR_OK;
}

// one set of a tree (`sets`: the renderer's tri_chunks or the ray queries' trace_chunks) in the layout of skr_scene_get_culling
static int get_culling_set(const skr_scene *scene, const std::vector<skr_f4> &sets, int32_t level, int32_t *chunk_size, int32_t *n_nodes, int32_t *n_chunks,
						   float *device_tris, float *node_spheres, int32_t *node_links, float *chunk_spheres)
{
	if(!scene || level < 0 || level >= SKR_CULL_LEVELS) return SKR_ERR_ARG;
	const int nt = scene->info.n_triangles, nn = nt ? scene->tri_node_count : 0, cs = scene->tri_chunk_size;
	const int nc = nt ? (nt + cs - 1) / cs : 0;
	if(chunk_size) *chunk_size = cs;
	if(n_nodes) *n_nodes = nn;
	if(n_chunks) *n_chunks = nc;
	if(device_tris && nt) memcpy(device_tris, scene->tris.data(), (size_t) nt * 48);
	const skr_f4 *base = sets.data() + (size_t) level * scene->tri_chunk_stride;
	for(int i = 0; i < nn; i++)
	{
		if(node_spheres) memcpy(node_spheres + 8 * (size_t) i, base + 3 * (size_t) i, 32);
		if(node_links) memcpy(node_links + 4 * (size_t) i, base + 3 * (size_t) i + 2, 16);
	}
	if(chunk_spheres && nc) memcpy(chunk_spheres, base + 3 * ((size_t) nn + 1), (size_t) nc * 32);
	return SKR_OK;
}

int skr_scene_get_culling(const skr_scene *scene, int32_t level, int32_t *chunk_size, int32_t *n_nodes, int32_t *n_chunks,
						  float *device_tris, float *node_spheres, int32_t *node_links, float *chunk_spheres)
{
	return get_culling_set(scene, scene ? scene->tri_chunks : std::vector<skr_f4>(), level, chunk_size, n_nodes, n_chunks, device_tris, node_spheres, node_links, chunk_spheres);
}

int skr_scene_get_trace_culling(const skr_scene *scene, int32_t level, int32_t *chunk_size, int32_t *n_nodes, int32_t *n_chunks,
								float *device_tris, float *node_spheres, int32_t *node_links, float *chunk_spheres, float ball[4])
{
	if(scene && ball) memcpy(ball, scene->trace_ball, 16);
	return get_culling_set(scene, scene ? scene->trace_chunks : std::vector<skr_f4>(), level, chunk_size, n_nodes, n_chunks, device_tris, node_spheres, node_links, chunk_spheres);
}

int skr_scene_get_shadow_masks(const skr_scene *scene, int32_t *n_lights, int32_t *cells, float *reach2, uint32_t *masks)
{
	if(!scene) return SKR_ERR_ARG;
	if(n_lights) *n_lights = (int32_t) (scene->shadow_masks.size() / SKR_SHADOW_TABLE_WORDS);
	if(cells) *cells = SKR_SHADOW_CELLS;
	if(reach2) *reach2 = scene->shadow_reach2;
	if(masks && !scene->shadow_masks.empty()) memcpy(masks, scene->shadow_masks.data(), scene->shadow_masks.size() * 4);
	return SKR_OK;
}

int skr_scene_get_gi_masks(const skr_scene *scene, int32_t *n_words, int32_t *mask_word, int32_t *wide, int32_t *dir_cells, float *grids, uint32_t *table)
{
	if(!scene) return SKR_ERR_ARG;
	if(n_words) *n_words = (int32_t) scene->gi_table.size();
	if(mask_word) *mask_word = (int32_t) scene->gi_mask_word;
	if(wide) *wide = scene->gi_wide;
	if(dir_cells) *dir_cells = SKR_GI_DIR_CELLS;
	if(grids)
		for(int g = 0; g < 2; g++)
		{
			const SkrGiGrid &G = scene->gi_grid[g];
			const float row[8] = {G.lo[0], G.lo[1], G.lo[2], G.inv, (float) G.n[0], (float) G.n[1], (float) G.n[2], (float) G.base};
			memcpy(grids + 8 * g, row, sizeof(row));
		}
	if(table && !scene->gi_table.empty()) memcpy(table, scene->gi_table.data(), scene->gi_table.size() * 4);
	return SKR_OK;
}

// Internal (not in include/skr.h: tests only): the surface patches of the GI masks (skr_scene::gi_surface).  first_row: the row
// number of the first patch (the grids' rows come first on the device).
int skr_scene_get_gi_surface(const skr_scene *scene, int32_t *n_words, int32_t *head_word, int32_t *first_row, uint32_t *table)
{
	if(!scene) return SKR_ERR_ARG;
	if(n_words) *n_words = (int32_t) scene->gi_surface.size();
	if(head_word) *head_word = (int32_t) scene->gi_surface_head;
	if(first_row) *first_row = (int32_t) scene->gi_rows;
	if(table && !scene->gi_surface.empty()) memcpy(table, scene->gi_surface.data(), scene->gi_surface.size() * 4);
	return SKR_OK;
}

// Internal (not in include/skr.h: tests only): the surface patches of the shadow masks (skr_scene::shadow_surface): the pairs' tables
// and the one header word per sphere.  skr_scene_rebuild_shadow_surface builds them again with the patch ball and the light cone
// scaled (1, 1: the product's), for the tests that shrink the margins.
int skr_scene_get_shadow_surface(const skr_scene *scene, int32_t *n_pairs, int32_t *stride, uint32_t *head, uint32_t *table)
{
	if(!scene) return SKR_ERR_ARG;
	if(stride) *stride = (int32_t) scene->shadow_surface_stride;
	if(n_pairs) *n_pairs = scene->shadow_surface_stride ? (int32_t) (scene->shadow_surface.size() / scene->shadow_surface_stride) : 0;
	if(head && !scene->shadow_surface_head.empty()) memcpy(head, scene->shadow_surface_head.data(), scene->shadow_surface_head.size() * 4);
	if(table && !scene->shadow_surface.empty()) memcpy(table, scene->shadow_surface.data(), scene->shadow_surface.size() * 4);
	return SKR_OK;
}

int skr_scene_rebuild_shadow_surface(skr_scene *scene, double rho_scale, double cone_scale)
{
	if(!scene) return SKR_ERR_ARG;
	scene->build_shadow_surface(rho_scale, cone_scale);
	return SKR_OK;
}

void skr_options_default(skr_options *opt)
{
	if(!opt) return;
	opt->width = 1920; // scene.h:15
	opt->height = 1080;
	opt->fov = 60; // utils.h:28-33
	opt->monte_carlo = 0;
	opt->num_path_traces = 1;
	opt->grid_size = 0;
	opt->max_depth = 3;
	opt->use_shadows = 0;
	opt->seed = 1;
	opt->shade_triangles = 0;
	opt->progressive_passes = 1;
	opt->legacy_reflect = 0;
}

uint64_t skr_radiance_ray_count(const skr_options *opt)
{
	if(!opt || opt->width <= 0 || opt->height <= 0) return 0;
	const uint64_t S = opt->grid_size > 0 ? (uint64_t) opt->grid_size * opt->grid_size : 1;
	uint64_t per = 0, pw = 1;
	for(int k = 0; k < opt->max_depth; k++)
	{
		per += pw;
		if(!opt->monte_carlo) break;
		pw *= (uint64_t) (opt->num_path_traces > 0 ? opt->num_path_traces : 0);
	}
	const uint64_t K = opt->progressive_passes > 1 ? (uint64_t) opt->progressive_passes : 1; // every pass is a whole frame
	return (uint64_t) opt->width * opt->height * S * per * K;
}

// main.cpp:199-211: "P6\n" W " " H "\n255\n" then W*H*3 bytes, top row first.
int skr_write_ppm(const char *path, uint32_t width, uint32_t height, const uint8_t *rgb)
{
	if(!path || !rgb) return SKR_ERR_ARG;
	std::ofstream ofs(path, std::ios::out | std::ios::binary);
	if(!ofs)
	{
		skr_set_error("cannot open '%s' for writing", path);
		return SKR_ERR_IO;
	}
	ofs << "P6\n" << width << " " << height << "\n255\n";
	ofs.write(reinterpret_cast<const char *>(rgb), (std::streamsize) width * height * 3);
	ofs.close();
	return ofs ? SKR_OK : SKR_ERR_IO;
}

// ---- other outputs.  The reference writes P6 only (main.cpp:199-211). ----

// Portable float map: "PF\n<W> <H>\n-1.0\n" (negative scale = little-endian), then W*3 binary32 values per row, BOTTOM row
// first.  Carries the unquantised frame (what main.cpp:205 clamps away): rgbf is top row first, like every buffer here.
int skr_write_pfm(const char *path, uint32_t width, uint32_t height, const float *rgbf)
{
	if(!path || !rgbf) return SKR_ERR_ARG;
	std::ofstream ofs(path, std::ios::out | std::ios::binary);
	if(!ofs)
	{
		skr_set_error("cannot open '%s' for writing", path);
		return SKR_ERR_IO;
	}
	ofs << "PF\n" << width << " " << height << "\n-1.0\n";
	for(uint32_t y = height; y-- > 0;) ofs.write(reinterpret_cast<const char *>(rgbf + (size_t) y * width * 3), (std::streamsize) width * 12);
	ofs.close();
	return ofs ? SKR_OK : SKR_ERR_IO;
}

// The inverse of skr_write_pfm (include/skr.h): "PF", W H, the scale line (its sign is the byte order), one whitespace byte, then
// H rows of W*3 binary32 values, bottom row first; rgbf receives them top row first.
int skr_read_pfm(const char *path, uint32_t *width, uint32_t *height, float *rgbf)
{
	if(!path || !width || !height)
	{
		skr_set_error("skr_read_pfm: null argument");
		return SKR_ERR_ARG;
	}
	*width = *height = 0;
	FILE *fp = fopen(path, "rb");
	if(!fp)
	{
		skr_set_error("cannot open '%s' for reading", path);
		return SKR_ERR_IO;
	}
	auto fail = [&](const char *why) {
		fclose(fp);
		skr_set_error("'%s' is not a colour PFM file this reader takes: %s", path, why);
		return SKR_ERR_IO;
	};
	auto token = [&](char *buf, size_t cap) { // the next whitespace-delimited token of the header; the ONE whitespace byte behind it is consumed
		int c = fgetc(fp);
		while(c == ' ' || c == '\t' || c == '\n' || c == '\r') c = fgetc(fp);
		size_t n = 0;
		while(c != EOF && c != ' ' && c != '\t' && c != '\n' && c != '\r')
		{
			if(n + 1 < cap) buf[n++] = (char) c;
			c = fgetc(fp);
		}
		buf[n] = 0;
		return n > 0 && c != EOF;
	};
	char tok[64], *end = nullptr;
	if(!token(tok, sizeof tok) || strcmp(tok, "PF") != 0) return fail("the magic is not PF");
	if(!token(tok, sizeof tok)) return fail("no width");
	const long long w = strtoll(tok, &end, 10);
	if(*end || w < 1 || w > 0x7FFFFFFFll) return fail("bad width");
	if(!token(tok, sizeof tok)) return fail("no height");
	const long long h = strtoll(tok, &end, 10);
	if(*end || h < 1 || h > 0x7FFFFFFFll) return fail("bad height");
	if(!token(tok, sizeof tok)) return fail("no scale line");
	const double scale = strtod(tok, &end);
	if(*end || !std::isfinite(scale) || scale == 0.0) return fail("bad scale");
	const bool big = scale > 0.0;
	*width = (uint32_t) w;
	*height = (uint32_t) h;
	const size_t row = (size_t) w * 3;
	if(!rgbf)
	{ // the sizes only — of a file that holds its pixels
		const long at = ftell(fp);
		if(at < 0 || fseek(fp, 0, SEEK_END) != 0) return fail("cannot seek");
		const long len = ftell(fp);
		if(len < 0 || (unsigned long long) (len - at) < (unsigned long long) row * 4ull * (unsigned long long) h) return fail("the pixel data ends early");
		fclose(fp);
		return SKR_OK;
	}
	for(long long y = h; y-- > 0;)
	{
		float *dst = rgbf + (size_t) y * row;
		if(fread(dst, 4, row, fp) != row) return fail("the pixel data ends early");
		if(big)
			for(size_t i = 0; i < row; i++)
			{
				uint32_t u;
				memcpy(&u, dst + i, 4);
				u = (u >> 24) | ((u >> 8) & 0xFF00u) | ((u << 8) & 0xFF0000u) | (u << 24);
				memcpy(dst + i, &u, 4);
			}
	}
	fclose(fp);
	return SKR_OK;
}

// PNG, 8-bit RGB, the bytes of the PPM: filter 0 on every row, zlib stream of stored (uncompressed) deflate blocks — no
// compressor is linked; any PNG reader takes it.
int skr_write_png(const char *path, uint32_t width, uint32_t height, const uint8_t *rgb)
{
	if(!path || !rgb || width == 0 || height == 0) return SKR_ERR_ARG;
	static uint32_t crc_table[256];
	static bool have_table = false;
	if(!have_table)
	{
		for(uint32_t n = 0; n < 256; n++)
		{
			uint32_t c = n;
			for(int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
			crc_table[n] = c;
		}
		have_table = true;
	}
	auto be32 = [](std::vector<uint8_t> &v, uint32_t x) { for(int k = 3; k >= 0; k--) v.push_back((uint8_t) (x >> (8 * k))); };
	std::vector<uint8_t> out = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
	auto chunk = [&](const char type[4], const std::vector<uint8_t> &data) {
		be32(out, (uint32_t) data.size());
		const size_t at = out.size();
		out.insert(out.end(), type, type + 4);
		out.insert(out.end(), data.begin(), data.end());
		uint32_t c = 0xffffffffu;
		for(size_t i = at; i < out.size(); i++) c = crc_table[(c ^ out[i]) & 0xffu] ^ (c >> 8);
		be32(out, c ^ 0xffffffffu);
	};
	std::vector<uint8_t> ihdr;
	be32(ihdr, width);
	be32(ihdr, height);
	const uint8_t tail[5] = {8, 2, 0, 0, 0}; // bit depth 8, colour type 2 (RGB), deflate, adaptive filtering, no interlace
	ihdr.insert(ihdr.end(), tail, tail + 5);
	chunk("IHDR", ihdr);
	const size_t row = (size_t) width * 3 + 1, raw_n = row * height;
	if(raw_n > 0x7fffffffull)
	{
		skr_set_error("skr_write_png: image too large for one IDAT chunk");
		return SKR_ERR_ARG;
	}
	std::vector<uint8_t> raw(raw_n);
	for(uint32_t y = 0; y < height; y++)
	{
		raw[row * y] = 0;
		memcpy(&raw[row * y + 1], rgb + (size_t) y * width * 3, (size_t) width * 3);
	}
	std::vector<uint8_t> z = {0x78, 0x01};
	uint32_t a = 1, b = 0; // adler32
	for(size_t at = 0; at < raw_n; at += 65535)
	{
		const size_t len = raw_n - at < 65535 ? raw_n - at : 65535;
		z.push_back(at + len == raw_n ? 1 : 0);
		z.push_back((uint8_t) len);
		z.push_back((uint8_t) (len >> 8));
		z.push_back((uint8_t) ~len);
		z.push_back((uint8_t) (~len >> 8));
		z.insert(z.end(), raw.begin() + (ptrdiff_t) at, raw.begin() + (ptrdiff_t) (at + len));
		for(size_t i = at; i < at + len;)
		{ // 5552 bytes: the longest run before a + b can overflow 32 bits
			const size_t stop = i + 5552 < at + len ? i + 5552 : at + len;
			for(; i < stop; i++) { a += raw[i]; b += a; }
			a %= 65521u;
			b %= 65521u;
		}
	}
	be32(z, (b << 16) | a);
	chunk("IDAT", z);
	chunk("IEND", {});
	std::ofstream ofs(path, std::ios::out | std::ios::binary);
	if(!ofs)
	{
		skr_set_error("cannot open '%s' for writing", path);
		return SKR_ERR_IO;
	}
	ofs.write(reinterpret_cast<const char *>(out.data()), (std::streamsize) out.size());
	ofs.close();
	return ofs ? SKR_OK : SKR_ERR_IO;
}

} // extern "C"
