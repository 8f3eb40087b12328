// .scn loader, options defaults, PPM writer: the host side of the drop-in
// boundary.  Behavioural restatement of reference src/scene.cpp:12-227,
// src/utils.h:26-34 and src/main.cpp:199-211 (citations relative to
// /root/reference).  No GPU code in this file.
#include "scene_host.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
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
	// The triangle walk only answers "does any triangle accept this ray before tmin" (raytrace.h:168-176 turns
	// any such hit black), so the order of tris[] is free: store the triangles along a Morton curve through the
	// centres of their accept regions, which makes every run of tri_chunk_size triangles spatially tight.
	std::vector<int> order(nt);
	{
		std::vector<double> ctr((size_t) nt * 3);
		double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
		for(int i = 0; i < nt; i++)
		{
			const float *t = &raw_triangles[(size_t) i * 9];
			for(int k = 0; k < 3; k++)
			{
				// accept region (v0, v0 - e1, v0 + e2), see build_triangle_chunks()
				const double c = (double) t[k] + (((double) t[6 + k] - t[k]) - ((double) t[3 + k] - t[k])) / 3.0;
				ctr[(size_t) i * 3 + k] = c;
				if(std::isfinite(c)) { lo[k] = std::min(lo[k], c); hi[k] = std::max(hi[k], c); }
			}
		}
		auto spread = [](uint64_t v) { // 21 bits -> every third bit
			v &= 0x1fffff;
			v = (v | v << 32) & 0x1f00000000ffffull;
			v = (v | v << 16) & 0x1f0000ff0000ffull;
			v = (v | v << 8) & 0x100f00f00f00f00full;
			v = (v | v << 4) & 0x10c30c30c30c30c3ull;
			v = (v | v << 2) & 0x1249249249249249ull;
			return v;
		};
		std::vector<uint64_t> key(nt);
		for(int i = 0; i < nt; i++)
		{
			uint64_t code = 0;
			bool ok = true;
			for(int k = 0; k < 3; k++)
			{
				const double c = ctr[(size_t) i * 3 + k], ext = hi[k] - lo[k];
				if(!std::isfinite(c)) { ok = false; break; }
				const double u = ext > 0 ? (c - lo[k]) / ext : 0.0;
				code |= spread((uint64_t) std::min(2097151.0, std::max(0.0, u * 2097151.0))) << k;
			}
			key[i] = ok ? code : ~0ull;
			order[i] = i;
		}
		std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
	}
	tris.assign((size_t) nt * 3 + 3, skr_f4{0.0f, 0.0f, 0.0f, 0.0f}); // + one pad triangle (kernel prefetch)
	for(int i = 0; i < nt; i++)
	{
		const float *t = &raw_triangles[(size_t) order[i] * 9];
		tris[3 * i] = {t[0], t[1], t[2], 0.0f};
		float file_index;
		const int32_t fi = order[i];
		memcpy(&file_index, &fi, 4);
		tris[3 * i + 1] = {t[3] - t[0], t[4] - t[1], t[5] - t[2], file_index};
		tris[3 * i + 2] = {t[6] - t[0], t[7] - t[1], t[8] - t[2], 0.0f};
	}
	tri_order = order;
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

// The cells of a cube map of N x N cells per face (shadow_cells.h addressing): every cell's centre direction (unit, 3 doubles) and
// angular radius, taken at its farthest corner (a cube-map cell is a convex spherical quadrilateral) with the cell widened by 2^-12 in
// face coordinates: the device's v_rcp_f32 face coordinates are within 2^-20 of v's.
static void cube_cells(int N, std::vector<double> &cell_dir, std::vector<double> &cell_theta)
{
	cell_dir.assign((size_t) 6 * N * N * 3, 0.0);
	cell_theta.assign((size_t) 6 * N * N, 0.0);
	for(int f = 0; f < 6; f++)
		for(int i = 0; i < N; i++)
			for(int j = 0; j < N; j++)
			{
				const int ax = f >> 1, o1 = ax == 0 ? 1 : 0, o2 = ax == 2 ? 1 : 2;
				const double sg = (f & 1) ? -1.0 : 1.0, wid = 2.0 / N, pad = 0x1p-12;
				auto dir = [&](double a, double b, double *w) {
					w[ax] = sg;
					w[o1] = a;
					w[o2] = b;
					const double n = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
					for(int c = 0; c < 3; c++) w[c] /= n;
				};
				const double a0 = -1.0 + i * wid, b0 = -1.0 + j * wid;
				double *wc = &cell_dir[3 * ((size_t) (f * N + i) * N + j)];
				dir(a0 + 0.5 * wid, b0 + 0.5 * wid, wc);
				double theta = 0.0;
				for(int corner = 0; corner < 4; corner++)
				{
					double w[3];
					dir((corner & 1) ? a0 + wid + pad : a0 - pad, (corner & 2) ? b0 + wid + pad : b0 - pad, w);
					const double cx = wc[1] * w[2] - wc[2] * w[1], cy = wc[2] * w[0] - wc[0] * w[2], cz = wc[0] * w[1] - wc[1] * w[0];
					theta = std::max(theta, std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), wc[0] * w[0] + wc[1] * w[1] + wc[2] * w[2]));
				}
				cell_theta[(size_t) (f * N + i) * N + j] = theta;
			}
}

// The shadow masks (shadow_cells.h; DESIGN.md "Shadow masks" derives every margin below).  Every shadow ray of a point light runs along
// a line through (almost) the light's position Lp, so whether sphere k can stop it depends only on the ray's direction as seen from Lp:
// bit k of a cell is set when the line through Lp along the cell's centre direction, taken in both senses, passes within R of the
// centre of sphere k, where R grows the radius by
//   * the slack of the binary32 discriminant, which can come out >= 0 for a line that just misses the sphere (grazing),
//   * how far the ray's line lies from the ideal line through Lp: the 1e-6 offset of its origin and the error of L = normalize(Lp - P),
//     which grows with the distance from Lp (bounded through `reach`, the farthest shading point the device lets use a mask),
//   * the cell's angular radius (every corner; the cell widened to absorb the device's rounding of its face coordinates) times the
//     distance from Lp.
// A light inside the grown sphere sets the bit in every cell.  All in binary64.
void skr_scene::build_shadow_masks()
{
	shadow_masks.clear();
	shadow_reach2 = 0.0f;
	// (a spot light is the point light it geometrically is: its table follows the point lights', in light order)
	const int ns = info.n_spheres, nl = info.n_point_lights + n_spot(), nt = info.n_triangles;
	if(ns < 1 || ns > SKR_SHADOW_MAX_SPHERES || nl < 1 || !raw_directional_lights.empty()) return;
	auto light_pos = [&](int l, double lp[3]) {
		const skr_f4 &q = lights[2 * (size_t) l];
		lp[0] = q.x;
		lp[1] = q.y;
		lp[2] = q.z;
	};
	// reach: the farthest point of the scene (spheres, triangles with their accept regions v0 - e1, v0 + e2) from any light.  The device
	// checks fl(|Lp - P|^2) <= reach^2 per lane, so a shading point outside it only costs that lane the plain walk.
	double reach = 0.0;
	for(int l = 0; l < nl; l++)
	{
		double lp[3];
		light_pos(l, lp);
		auto dist = [&](double x, double y, double z) { return std::sqrt((x - lp[0]) * (x - lp[0]) + (y - lp[1]) * (y - lp[1]) + (z - lp[2]) * (z - lp[2])); };
		for(int k = 0; k < ns; k++)
			reach = std::max(reach, dist(sph_geom[k].x, sph_geom[k].y, sph_geom[k].z) + std::sqrt((double) sph_geom[k].w));
		for(int t = 0; t < nt; t++)
		{
			const float *v = &raw_triangles[(size_t) t * 9];
			for(int c = 0; c < 3; c++) reach = std::max(reach, dist(v[3 * c], v[3 * c + 1], v[3 * c + 2]));
			const double e1[3] = {(double) v[3] - v[0], (double) v[4] - v[1], (double) v[5] - v[2]}, e2[3] = {(double) v[6] - v[0], (double) v[7] - v[1], (double) v[8] - v[2]};
			reach = std::max(reach, dist(v[0] - e1[0], v[1] - e1[1], v[2] - e1[2]));
			reach = std::max(reach, dist(v[0] + e2[0], v[1] + e2[1], v[2] + e2[2]));
		}
	}
	reach *= 1.0 + 0x1p-10;
	if(!(reach > 0.0) || !(reach * reach < 1e36)) return; // (NaN, inf, or beyond binary32: no masks)
	const float reach2 = std::nextafter((float) (reach * reach), INFINITY);
	const double D = std::sqrt((double) reach2) * (1.0 + 0x1p-16); // bounds |Lp - P| of every lane that passes fl(|Lp - P|^2) <= reach2
	const double eta = 0x1p-16;                                  // bounds |L - (Lp - P) / |Lp - P||, L the device's binary32 normalize
	// every cell's centre direction and angular radius: the same for every light
	std::vector<double> cell_dir, cell_theta;
	cube_cells(SKR_SHADOW_CELLS, cell_dir, cell_theta);
	for(double &t : cell_theta) t = t * (1.0 + 0x1p-20) + 0x1p-16; // + the angle between fl(Lp - P) and Lp - P
	std::vector<uint32_t> masks((size_t) nl * SKR_SHADOW_TABLE_WORDS, 0u);
	for(int l = 0; l < nl; l++)
	{
		double lp[3];
		light_pos(l, lp);
		const double lmax = std::max(std::fabs(lp[0]), std::max(std::fabs(lp[1]), std::fabs(lp[2])));
		// |o - P| for o = fl(P + 1e-6f) per component, |P| <= |Lp| + D (twice over)
		const double eps_o = 2.0 * std::sqrt(3.0) * (1e-6 + 0x1p-23 * (lmax + D + 1e-6));
		for(int k = 0; k < ns; k++)
		{
			const double q[3] = {sph_geom[k].x - lp[0], sph_geom[k].y - lp[1], sph_geom[k].z - lp[2]};
			const double r2 = sph_geom[k].w, qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2], qn = std::sqrt(qq);
			const double E = (qn + D + eps_o) * (1.0 + 0x1p-20); // bounds |e| = |o - C| of the device's test
			const double rk = std::sqrt(r2 + 0x1p-16 * (E * E + r2)) + 0x1p-20 * E; // discriminant slack (16x), the rounding of e
			const double S = qn + rk;                                               // farthest point of the grown sphere from Lp
			const double base = rk + eps_o + eta * (S + D + eps_o) / (1.0 - eta) + 0x1p-30 * qn;
			for(int c = 0; c < SKR_SHADOW_TABLE_WORDS; c++)
			{
				const double *wc = &cell_dir[3 * (size_t) c];
				const double s = q[0] * wc[0] + q[1] * wc[1] + q[2] * wc[2];
				const double dist = std::sqrt(std::max(0.0, qq - s * s));
				if(dist <= base + cell_theta[c] * S) masks[(size_t) l * SKR_SHADOW_TABLE_WORDS + c] |= 1u << k;
			}
		}
	}
	shadow_masks.swap(masks);
	shadow_reach2 = reach2;
}

// Bit `bit` (sphere of centre C, squared radius r2) of every direction cell of a GI mask row, for origins in the ball (q, rho)
// (build_gi_masks' margins; cth, sth: the cosine and sine of each direction cell's padded angular radius).  All in binary64.
// (the ball of origins against one sphere: what every direction cone of ball_cone_touches shares)
struct BallSphere {
	double v[3], dist; // C - q and its length
	double rk;         // the grown radius r': the slack of the binary32 discriminant
	double behind, reach;
	bool meets; // the grown sphere meets the ball: every direction
};
static BallSphere ball_sphere(const double *q, double rho, const double *C, double r2)
{
	BallSphere b;
	for(int c = 0; c < 3; c++) b.v[c] = C[c] - q[c];
	b.dist = std::sqrt(b.v[0] * b.v[0] + b.v[1] * b.v[1] + b.v[2] * b.v[2]);
	const double E = (b.dist + rho) * (1.0 + 0x1p-20); // bounds |e| = |o - C| of the device's test
	b.rk = std::sqrt(r2 + 0x1p-16 * (E * E + r2)) + 0x1p-20 * E; // discriminant slack (16x), the rounding of e
	const double tol = 0x1p-30 * (b.dist + rho + b.rk);           // (this function's own rounding)
	b.behind = rho + 0x1p-16 * E + tol;                            // b < 0 needs (C - o).d > -2^-22 |e| |d|
	b.reach = b.rk + rho + tol;
	b.meets = b.dist <= b.reach;
	return b;
}
// The two rules of build_gi_masks for the lines along the directions of the cone of unit axis w and half-angle theta (ct, st: its
// cosine and sine) through the points of a ball, v = C - (the ball's centre), dist = |v|.  cone_ahead: the sphere may lie ahead of
// some origin (the half-line rule: b < 0); cone_line_touches: some line may pass within `reach` of C (the line rule: D >= 0).
struct ConeSphere {
	double cos_lo, min_sin; // the cosine of the smallest angle between v and a direction of the cone; the smallest sine, either sense
};
static ConeSphere cone_sphere(const double *v, double dist, const double *w, double ct, double st)
{
	const double cp = (v[0] * w[0] + v[1] * w[1] + v[2] * w[2]) / dist;
	const double x = v[1] * w[2] - v[2] * w[1], y = v[2] * w[0] - v[0] * w[2], z = v[0] * w[1] - v[1] * w[0];
	const double sp = std::sqrt(x * x + y * y + z * z) / dist;
	const bool lo0 = cp >= ct;   // phi <= theta
	const bool hipi = cp <= -ct; // phi + theta >= pi
	const double sin_lo = lo0 ? 0.0 : sp * ct - cp * st;
	const double sin_hi = hipi ? 0.0 : sp * ct + cp * st;
	return ConeSphere{lo0 ? 1.0 : cp * ct + sp * st, std::max(0.0, std::min(sin_lo, sin_hi))};
}
static bool cone_ahead(const ConeSphere &c, double dist, double behind) { return dist * c.cos_lo + behind >= 0.0; }
static bool cone_line_touches(const ConeSphere &c, double dist, double reach) { return dist * c.min_sin <= reach; }
// Whether a ray from the ball along some direction of the cone may have D >= 0 and b < 0 for the sphere.
static bool ball_cone_touches(const BallSphere &b, const double *w, double ct, double st)
{
	if(b.meets) return true;
	const ConeSphere c = cone_sphere(b.v, b.dist, w, ct, st);
	return cone_ahead(c, b.dist, b.behind) && cone_line_touches(c, b.dist, b.reach);
}
static void gi_ball_bits(const double *q, double rho, const double *C, double r2, uint32_t bit, const std::vector<double> &cell_dir,
						 const std::vector<double> &cth, const std::vector<double> &sth, uint32_t *row)
{
	const BallSphere b = ball_sphere(q, rho, C, r2);
	for(int e = 0; e < SKR_GI_ROW_ENTRIES; e++)
		if(ball_cone_touches(b, &cell_dir[3 * (size_t) e], cth[e], sth[e])) row[e] |= bit;
}

// The GI masks (shadow_cells.h; DESIGN.md "GI masks" derives every margin below).  A GI child ray starts at its node's hit point o
// and runs along d (not of unit length: the basis mix of shade_common.h gi_direction_pair); the device's closest-hit walk counts
// sphere k as a candidate when its binary32 D >= 0 and b < 0.  For a cell of origins — a ball of centre q and radius rho — and a cell
// of directions — a cone of axis w and half-angle theta — bit k is set unless, for every origin and every direction of the two cells,
//   * the line misses the sphere grown to r' (the slack of the binary32 discriminant, as for the shadow masks): the distance from C to
//     the line is at least |C - q| sin(psi) - rho, psi the angle between C - q and the direction, psi in [phi - theta, phi + theta],
//   * or the sphere lies behind the origin: (C - o).d/|d| <= |C - q| cos(max(0, phi - theta)) + rho < -(the rounding of b), so b > 0.
// All in binary64.  Origins are looked up in a fine grid over the small spheres (radius <= 4 x the median), grown by twice the largest
// of them, then in a coarse grid over every sphere's bounds, cut to the fine grid's box grown by its extent; only cells near some
// sphere's surface (where hit points lie) get masks.  The cells grow until the whole table fits SKR_GI_MAX_BYTES.  A device lane whose
// origin lies in no stored cell, or whose direction is degenerate, walks every sphere.
void skr_scene::build_gi_masks()
{
	gi_table.clear();
	gi_grid[0] = gi_grid[1] = SkrGiGrid{};
	gi_mask_word = 0;
	gi_wide = 0;
	const int ns = info.n_spheres;
	if(ns < 1 || ns > SKR_GI_MAX_SPHERES || info.n_triangles > 0) return;
	std::vector<double> C((size_t) 3 * ns), r2(ns), rad(ns);
	for(int k = 0; k < ns; k++)
	{
		C[3 * k] = sph_geom[k].x;
		C[3 * k + 1] = sph_geom[k].y;
		C[3 * k + 2] = sph_geom[k].z;
		r2[k] = sph_geom[k].w;
		rad[k] = std::sqrt(r2[k]);
		for(int c = 0; c < 3; c++)
			if(!(std::fabs(C[3 * k + c]) < 1e6)) return;
		if(!(rad[k] < 1e6)) return; // (NaN, inf, out of the range the margins are derived for: no masks)
	}
	std::vector<double> sorted(rad);
	std::sort(sorted.begin(), sorted.end());
	const double small = 4.0 * sorted[ns / 2];
	double flo[3] = {INFINITY, INFINITY, INFINITY}, fhi[3] = {-INFINITY, -INFINITY, -INFINITY}, alo[3] = {INFINITY, INFINITY, INFINITY},
		   ahi[3] = {-INFINITY, -INFINITY, -INFINITY}, rsmall = 0.0;
	for(int k = 0; k < ns; k++)
		for(int c = 0; c < 3; c++)
		{
			alo[c] = std::min(alo[c], C[3 * k + c] - rad[k]);
			ahi[c] = std::max(ahi[c], C[3 * k + c] + rad[k]);
			if(rad[k] <= small)
			{
				flo[c] = std::min(flo[c], C[3 * k + c] - rad[k]);
				fhi[c] = std::max(fhi[c], C[3 * k + c] + rad[k]);
				rsmall = std::max(rsmall, rad[k]);
			}
		}
	double ext_f = 0.0;
	for(int c = 0; c < 3; c++)
	{
		flo[c] -= 2.0 * rsmall;
		fhi[c] += 2.0 * rsmall;
		ext_f = std::max(ext_f, fhi[c] - flo[c]);
	}
	if(!(ext_f > 1e-6)) return;
	double clo[3], chi[3], ext_c = 0.0;
	for(int c = 0; c < 3; c++)
	{
		clo[c] = std::min(flo[c], std::max(alo[c], flo[c] - ext_f));
		chi[c] = std::max(fhi[c], std::min(ahi[c], fhi[c] + ext_f));
		ext_c = std::max(ext_c, chi[c] - clo[c]);
	}
	gi_wide = ns > 16 ? 1 : 0;
	const size_t row_bytes = (size_t) SKR_GI_ROW_ENTRIES * (gi_wide ? 4 : 2);
	struct Cell {
		double q[3], rho;
	};
	std::vector<Cell> cells;
	std::vector<int32_t> index;
	double hh[2] = {0.0, 0.0};
	bool fits = false;
	for(int attempt = 0; attempt < 64 && !fits; attempt++)
	{
		const double grow = std::pow(1.15, attempt);
		cells.clear();
		index.clear();
		for(int g = 0; g < 2; g++)
		{
			SkrGiGrid &G = gi_grid[g];
			const double *lo = g ? clo : flo, *hi = g ? chi : fhi;
			G.inv = (float) (1.0 / ((g ? ext_c / 16.0 : ext_f / 32.0) * grow));
			hh[g] = 1.0 / (double) G.inv; // the cell edge the device's (o - lo) * inv cuts at
			for(int c = 0; c < 3; c++)
			{
				float l = (float) lo[c];
				if((double) l > lo[c]) l = std::nextafter(l, -INFINITY);
				G.lo[c] = l;
				G.n[c] = std::max(1, std::min(256, (int) std::ceil((hi[c] - (double) l) / hh[g])));
				G.n_f[c] = (float) G.n[c];
			}
			G.base = (int32_t) index.size();
			const int n0 = G.n[0], n1 = G.n[1], n2 = G.n[2];
			// the device's cell of o is within 2^-22 (i + 1) hh of o's: pad every cell by 2^-18 n hh
			const double pad = 0x1p-18 * std::max(n0, std::max(n1, n2)) * hh[g];
			const double rho = std::sqrt(3.0) * (0.5 * hh[g] + pad) * (1.0 + 0x1p-20);
			for(int k = 0; k < n2; k++)
				for(int j = 0; j < n1; j++)
					for(int i = 0; i < n0; i++)
					{
						const int ijk[3] = {i, j, k};
						Cell cl;
						bool inside_fine = g == 1;
						for(int c = 0; c < 3; c++)
						{
							cl.q[c] = (double) G.lo[c] + (ijk[c] + 0.5) * hh[g];
							const double f0 = (double) gi_grid[0].lo[c], f1 = f0 + gi_grid[0].n[c] * hh[0];
							inside_fine = inside_fine && cl.q[c] - 0.5 * hh[g] >= f0 && cl.q[c] + 0.5 * hh[g] <= f1;
						}
						cl.rho = rho;
						bool near = false; // (which cells are stored decides only the speed: hit points lie near some sphere's surface)
						for(int s = 0; s < ns && !near && !inside_fine; s++)
						{
							const double dx = C[3 * s] - cl.q[0], dy = C[3 * s + 1] - cl.q[1], dz = C[3 * s + 2] - cl.q[2];
							const double dist = std::sqrt(dx * dx + dy * dy + dz * dz);
							near = std::fabs(dist - rad[s]) <= rho + 1e-4 + 0x1p-16 * (dist + rad[s]);
						}
						index.push_back(near ? (int32_t) cells.size() : -1);
						if(near) cells.push_back(cl);
					}
		}
		fits = ((index.size() + 1) & ~(size_t) 1) * 4 + cells.size() * row_bytes <= SKR_GI_MAX_BYTES;
	}
	if(!fits || cells.empty()) return;
	std::vector<double> cell_dir, cell_theta;
	cube_cells(SKR_GI_DIR_CELLS, cell_dir, cell_theta);
	std::vector<double> cth(SKR_GI_ROW_ENTRIES), sth(SKR_GI_ROW_ENTRIES);
	for(int e = 0; e < SKR_GI_ROW_ENTRIES; e++)
	{
		const double t = cell_theta[e] * (1.0 + 0x1p-20) + 0x1p-40;
		cth[e] = std::cos(t);
		sth[e] = std::sin(t);
	}
	std::vector<uint32_t> masks(cells.size() * SKR_GI_ROW_ENTRIES, 0u);
	for(size_t ci = 0; ci < cells.size(); ci++)
		for(int k = 0; k < ns; k++) gi_ball_bits(cells[ci].q, cells[ci].rho, &C[3 * k], r2[k], 1u << k, cell_dir, cth, sth, &masks[ci * SKR_GI_ROW_ENTRIES]);
	const size_t n_index = (index.size() + 1) & ~(size_t) 1;
	const size_t n_mask_words = gi_wide ? masks.size() : masks.size() / 2;
	std::vector<uint32_t> table((n_index + n_mask_words + 3) & ~(size_t) 3, 0u);
	memcpy(table.data(), index.data(), index.size() * 4);
	if(gi_wide) memcpy(&table[n_index], masks.data(), masks.size() * 4);
	else
		for(size_t e = 0; e < masks.size(); e += 2) table[n_index + e / 2] = masks[e] | masks[e + 1] << 16; // (uint16_t entries, little-endian)
	gi_mask_word = (uint32_t) n_index;
	gi_table.swap(table);
}

// The surface patches of the GI masks (shadow_cells.h; DESIGN.md "GI surface patches" derives every margin below).  A GI origin is a
// hit point of some sphere s, so the device keys it to the cell of e = o - C_s in a cube map on that sphere, once fl(|e|^2) - r_s^2
// is within the sphere's radial slack tau_s: every such origin lies in the shell R_lo <= |o - C_s| <= R_hi, in the directions of
// the cell padded like every cube-map cell.  A patch is that piece of the shell; its origins lie in a ball (q, rho) around the
// point at r_s cos(theta) along the cell's centre direction, and its row holds build_gi_masks' masks of that ball, except for
// sphere s itself: an origin on the patch sees it only behind its surface, so its bit is set only for the directions that some
// origin of the patch may see at an angle of 90 degrees or more from its own e (b >= 0 otherwise).  Patches are stored where their
// ball meets the fine grid's box (the small spheres and the ground under them); the cells grow by 1.15x until the whole table
// fits SKR_GI_MAX_BYTES.  A device lane off every stored patch takes the grids' row (shade_common.h gi_surface_row).  All in binary64.
// (the shell of a sphere's surface points and the ball of one patch of it: shared with build_shadow_surface)
struct SurfaceShell {
	float tau;         // the radial slack: |fl(|e|^2) - r^2| <= tau; negative: no patches
	double R_lo, R_hi; // every keyed point has R_lo <= |o - C| <= R_hi
};
static SurfaceShell surface_shell(double r2)
{
	SurfaceShell sh;
	// |fl(|e|^2) - r^2| <= tau gives (r^2 - tau)(1 - 2^-20) <= |fl(e)|^2 <= (r^2 + tau)(1 + 2^-20) (the dot product's and the
	// difference's rounding), and |e| is within 2^-23 |e| of |fl(e)|
	sh.tau = std::sqrt(r2) > 1e-3 ? (float) (r2 * 0x1p-7) : -1.0f; // (|o - C| within about r / 256 of r; tiny spheres: no patches)
	sh.R_lo = std::sqrt(std::max(0.0, (r2 - sh.tau) * (1.0 - 0x1p-20))) * (1.0 - 0x1p-22);
	sh.R_hi = std::sqrt((r2 + std::max(0.0f, sh.tau)) * (1.0 + 0x1p-20)) * (1.0 + 0x1p-22);
	return sh;
}
// The ball (q, rho) of the patch of sphere (C, rad) whose cell has the unit centre direction w and the padded angular radius th.
static void surface_patch_ball(const double *C, double rad, const SurfaceShell &sh, const double *w, double th, double *q, double &rho)
{
	const double h = rad * std::cos(th);
	for(int c = 0; c < 3; c++) q[c] = C[c] + h * w[c];
	// the farthest point of the patch from q: |o - q|^2 = R^2 + h^2 - 2 R h cos(phi) grows with phi and is convex in R
	double far = 0.0;
	for(double R : {sh.R_lo, sh.R_hi}) far = std::max(far, std::sqrt(std::max(0.0, R * R + h * h - 2.0 * R * h * std::cos(th))));
	double cmax = 0.0;
	for(int c = 0; c < 3; c++) cmax = std::max(cmax, std::fabs(C[c]));
	rho = far * (1.0 + 0x1p-20) + 0x1p-30 * (cmax + rad);
}
// The padded angular radii of a sphere's G x G x 6 cells (cube_cells) as the patches use them: + the angle between e and fl(e)
static void surface_cells(int g, std::vector<double> &dir, std::vector<double> &theta)
{
	dir.clear();
	theta.clear();
	if(g) cube_cells(g, dir, theta);
	for(double &t : theta) t = t * (1.0 + 0x1p-20) + 0x1p-20; // (2^-23 of each component)
}
// The first cell edge the GI patches try: half the one at which the small spheres' patches alone (about 24 r^2 / edge^2 each) fill a
// table of `rows` rows.
static double surface_first_edge(const std::vector<double> &rad, const std::vector<double> &r2, double rows)
{
	const int ns = (int) rad.size();
	std::vector<double> sorted(rad);
	std::sort(sorted.begin(), sorted.end());
	double small_area = 0.0;
	for(int k = 0; k < ns; k++)
		if(rad[k] <= 4.0 * sorted[ns / 2]) small_area += 24.0 * r2[k];
	return std::max(1e-6, 0.5 * std::sqrt(small_area / std::max(1.0, rows)));
}

void skr_scene::build_gi_surface()
{
	gi_surface.clear();
	gi_surface_head = 0;
	gi_rows = 0;
	gi_surface_edge = 0.0;
	if(gi_table.empty()) return;
	const int ns = info.n_spheres;
	const size_t row_words = (size_t) SKR_GI_ROW_ENTRIES * (gi_wide ? 4 : 2) / 4;
	gi_rows = (uint32_t) ((gi_table.size() - gi_mask_word) / row_words); // (the table's padding is below one row)
	std::vector<double> C((size_t) 3 * ns), r2(ns), rad(ns), R_lo(ns), R_hi(ns);
	std::vector<float> tau(ns);
	std::vector<SurfaceShell> shell(ns);
	for(int k = 0; k < ns; k++)
	{
		C[3 * k] = sph_geom[k].x;
		C[3 * k + 1] = sph_geom[k].y;
		C[3 * k + 2] = sph_geom[k].z;
		r2[k] = sph_geom[k].w;
		rad[k] = std::sqrt(r2[k]);
		shell[k] = surface_shell(r2[k]);
		tau[k] = shell[k].tau;
		R_lo[k] = shell[k].R_lo;
		R_hi[k] = shell[k].R_hi;
	}
	double blo[3], bhi[3]; // the fine grid's box
	for(int c = 0; c < 3; c++)
	{
		blo[c] = gi_grid[0].lo[c];
		bhi[c] = blo[c] + gi_grid[0].n[c] / (double) gi_grid[0].inv;
	}
	struct Patch {
		int s, cell;
		double q[3], rho;
	};
	std::vector<Patch> patches;
	std::vector<int> G(ns, 0);
	std::vector<std::vector<double>> cdir(ns), cth(ns); // per sphere: its cells' centre directions and padded angular radii
	size_t n_index = 0;
	bool fits = false;
	double edge = surface_first_edge(rad, r2, (double) SKR_GI_MAX_BYTES / (row_words * 4)), used_edge = 0.0;
	for(int attempt = 0; attempt < 200 && !fits; attempt++, edge *= 1.15)
	{
		patches.clear();
		n_index = 0;
		for(int k = 0; k < ns; k++)
		{
			const int g = tau[k] < 0.0f ? 0 : (int) std::min((double) SKR_GI_SURFACE_MAX_CELLS, std::max(1.0, std::ceil(2.0 * rad[k] / edge)));
			if(g != G[k])
			{
				G[k] = g;
				surface_cells(g, cdir[k], cth[k]);
			}
			n_index += (size_t) 6 * g * g;
			for(int cell = 0; cell < 6 * g * g; cell++)
			{
				Patch pt;
				pt.s = k;
				pt.cell = cell;
				surface_patch_ball(&C[3 * k], rad[k], shell[k], &cdir[k][3 * (size_t) cell], cth[k][cell], pt.q, pt.rho);
				double gap2 = 0.0; // from q to the box
				for(int c = 0; c < 3; c++)
				{
					const double o = std::max(0.0, std::max(blo[c] - pt.q[c], pt.q[c] - bhi[c]));
					gap2 += o * o;
				}
				if(gap2 <= pt.rho * pt.rho) patches.push_back(pt);
			}
		}
		fits = (SKR_GI_SURFACE_HEAD * (size_t) ns + n_index) * 4 + patches.size() * row_words * 4 <= SKR_GI_MAX_BYTES;
		if(fits) used_edge = edge;
	}
	if(!fits || patches.empty()) return;
	gi_surface_edge = used_edge;
	std::vector<double> cell_dir, cell_theta;
	cube_cells(SKR_GI_DIR_CELLS, cell_dir, cell_theta);
	std::vector<double> dth(SKR_GI_ROW_ENTRIES), dct(SKR_GI_ROW_ENTRIES), dst(SKR_GI_ROW_ENTRIES);
	for(int e = 0; e < SKR_GI_ROW_ENTRIES; e++)
	{
		dth[e] = cell_theta[e] * (1.0 + 0x1p-20) + 0x1p-40;
		dct[e] = std::cos(dth[e]);
		dst[e] = std::sin(dth[e]);
	}
	std::vector<uint32_t> masks(patches.size() * SKR_GI_ROW_ENTRIES, 0u);
	for(size_t pi = 0; pi < patches.size(); pi++)
	{
		const Patch &pt = patches[pi];
		uint32_t *row = &masks[pi * SKR_GI_ROW_ENTRIES];
		for(int k = 0; k < ns; k++)
			if(k != pt.s) gi_ball_bits(pt.q, pt.rho, &C[3 * k], r2[k], 1u << k, cell_dir, dct, dst, row);
		// sphere s: (C - o).d / |d| = -R cos(angle(e, d)) with R >= R_lo, and that angle is at most psi + theta_patch + theta_dir;
		// below 90 degrees b < 0 needs R_lo cos(.) < 2^-16 E (the rounding of b, as in build_gi_masks)
		const int s = pt.s;
		const double *wp = &cdir[s][3 * (size_t) pt.cell];
		const double E = R_hi[s] * (1.0 + 0x1p-20), behind = 0x1p-16 * E + 0x1p-30 * R_hi[s];
		for(int e = 0; e < SKR_GI_ROW_ENTRIES; e++)
		{
			const double *w = &cell_dir[3 * (size_t) e];
			const double x = wp[1] * w[2] - wp[2] * w[1], y = wp[2] * w[0] - wp[0] * w[2], z = wp[0] * w[1] - wp[1] * w[0];
			const double psi = std::atan2(std::sqrt(x * x + y * y + z * z), wp[0] * w[0] + wp[1] * w[1] + wp[2] * w[2]);
			const double ang = psi + cth[s][pt.cell] + dth[e] + 0x1p-30;
			if(!(ang < 0.5 * M_PI && R_lo[s] * std::cos(ang) > behind)) row[e] |= 1u << s;
		}
	}
	// masks (rows gi_rows + pi), headers, index
	const size_t n_mask_words = gi_wide ? masks.size() : masks.size() / 2;
	std::vector<uint32_t> table(n_mask_words + SKR_GI_SURFACE_HEAD * (size_t) ns + n_index, 0u);
	if(gi_wide) memcpy(table.data(), masks.data(), masks.size() * 4);
	else
		for(size_t e = 0; e < masks.size(); e += 2) table[e / 2] = masks[e] | masks[e + 1] << 16; // (uint16_t entries, little-endian)
	uint32_t *head = &table[n_mask_words];
	int32_t *index = reinterpret_cast<int32_t *>(head + SKR_GI_SURFACE_HEAD * ns);
	size_t at = SKR_GI_SURFACE_HEAD * (size_t) ns;
	for(int k = 0; k < ns; k++)
	{
		head[SKR_GI_SURFACE_HEAD * k] = (uint32_t) at;
		head[SKR_GI_SURFACE_HEAD * k + 1] = (uint32_t) G[k];
		const float t = G[k] ? tau[k] : -1.0f;
		memcpy(&head[SKR_GI_SURFACE_HEAD * k + 2], &t, 4);
		for(int c = 0; c < 6 * G[k] * G[k]; c++) head[at + c] = 0xffffffffu; // -1 = none
		at += (size_t) 6 * G[k] * G[k];
	}
	for(size_t pi = 0; pi < patches.size(); pi++)
		index[head[SKR_GI_SURFACE_HEAD * patches[pi].s] - SKR_GI_SURFACE_HEAD * ns + patches[pi].cell] = (int32_t) (gi_rows + pi);
	gi_surface_head = (uint32_t) n_mask_words;
	gi_surface.swap(table);
}

// The surface patches of the shadow masks (shadow_cells.h; DESIGN.md "Shadow surface patches" derives every margin below).  A shading
// point P of the level pipelines is a hit point of some sphere s, so the device keys it to the cell of e = P - C_s in a cube map on
// that sphere, once fl(|e|^2) - r_s^2 is within the sphere's radial slack: P lies in build_gi_surface's patch ball, the shadow
// ray's origin o = fl(P + 1e-6) within eps_o of it, and its direction in the cone about Lp - q of half-angle asin(rho / |Lp - q|),
// + eta for the device's normalize.  Bit k of a patch's word is set unless, for both lights of the pair, sphere k fails
// build_gi_masks' half-line rule for every such ray (from the patch's ball) or its line rule (taken from the light, which every
// ray's line passes almost through); the patch's own sphere follows build_gi_surface's own-sphere rule (clear where every ray leaves
// the sphere), and a light inside the ball sets every bit.  Every patch of every sphere is stored (one word each), at
// SKR_SHADOW_SURFACE_SCALE cells per edge of a GI patch's cell, the cells growing by 1.15x until every pair's table together fits
// SKR_SHADOW_SURFACE_MAX_BYTES.  All in binary64.
void skr_scene::build_shadow_surface(double rho_scale, double cone_scale)
{
	shadow_surface.clear();
	shadow_surface_head.clear();
	shadow_surface_stride = 0;
	if(shadow_masks.empty()) return;
	const int ns = info.n_spheres, nl = (int) (shadow_masks.size() / SKR_SHADOW_TABLE_WORDS), npairs = (nl + 1) / 2;
	std::vector<double> C((size_t) 3 * ns), r2(ns), rad(ns);
	std::vector<SurfaceShell> shell(ns);
	for(int k = 0; k < ns; k++)
	{
		C[3 * k] = sph_geom[k].x;
		C[3 * k + 1] = sph_geom[k].y;
		C[3 * k + 2] = sph_geom[k].z;
		r2[k] = sph_geom[k].w;
		rad[k] = std::sqrt(r2[k]);
		for(int c = 0; c < 3; c++)
			if(!(std::fabs(C[3 * k + c]) < 1e6)) return;
		if(!(rad[k] < 1e6)) return; // (NaN, inf, out of the range the margins are derived for: the direction masks only)
		shell[k] = surface_shell(r2[k]);
	}
	// the GI patches' edge, or what they would try first where the scene has none (triangles)
	double edge = gi_surface_edge > 0.0 ? gi_surface_edge : surface_first_edge(rad, r2, (double) SKR_GI_MAX_BYTES / (SKR_GI_ROW_ENTRIES * (ns > 16 ? 4 : 2)));
	edge /= SKR_SHADOW_SURFACE_SCALE;
	std::vector<int> G(ns, 0);
	size_t stride = 0;
	for(int attempt = 0; attempt < 200; attempt++, edge *= 1.15)
	{
		stride = 0;
		for(int k = 0; k < ns; k++)
		{
			G[k] = shell[k].tau < 0.0f ? 0 : (int) std::min((double) SKR_GI_SURFACE_MAX_CELLS, std::max(1.0, std::ceil(2.0 * rad[k] / edge)));
			stride += (size_t) 6 * G[k] * G[k];
		}
		if(stride * npairs * 4 <= SKR_SHADOW_SURFACE_MAX_BYTES) break;
	}
	if(stride == 0 || stride * npairs * 4 > SKR_SHADOW_SURFACE_MAX_BYTES) return;
	const uint32_t all = ns >= 32 ? 0xffffffffu : (1u << ns) - 1u;
	const double eta = 0x1p-15; // the angle between the device's L = normalize(fl(Lp - P)) and Lp - P (2^-23 or so: far over)
	std::vector<uint32_t> table(stride * npairs, 0u), head(ns, 0u);
	std::vector<double> cdir, cth;
	std::vector<BallSphere> bs(ns);
	size_t base = 0;
	for(int s = 0; s < ns; s++)
	{
		head[s] = (uint32_t) base | (uint32_t) G[s] << 24;
		surface_cells(G[s], cdir, cth);
		double cmax = 0.0;
		for(int c = 0; c < 3; c++) cmax = std::max(cmax, std::fabs(C[3 * s + c]));
		// |o - P| for o = fl(P + 1e-6f) per component (twice over, as build_shadow_masks)
		const double eps_o = 2.0 * std::sqrt(3.0) * (1e-6 + 0x1p-23 * (cmax + shell[s].R_hi + 1e-6));
		const double R_in = shell[s].R_lo - eps_o;                       // |o - C_s| at least
		const double E_own = (shell[s].R_hi + eps_o) * (1.0 + 0x1p-20); // ... and at most
		const double behind_own = 0x1p-16 * E_own + 0x1p-30 * shell[s].R_hi;
		const double tilt = R_in > 0.0 ? std::asin(std::min(1.0, eps_o / shell[s].R_lo)) : 0.0; // the angle between o - C_s and P - C_s
		for(int cell = 0; cell < 6 * G[s] * G[s]; cell++)
		{
			const double *wp = &cdir[3 * (size_t) cell];
			double q[3], rho;
			surface_patch_ball(&C[3 * s], rad[s], shell[s], wp, cth[cell], q, rho);
			rho = (rho + eps_o) * rho_scale;
			for(int k = 0; k < ns; k++)
				if(k != s) bs[k] = ball_sphere(q, rho, &C[3 * k], r2[k]);
			for(int l = 0; l < nl; l++)
			{
				uint32_t &word = table[(size_t) (l >> 1) * stride + base + cell];
				const skr_f4 &lp = lights[2 * (size_t) l];
				const double d[3] = {lp.x - q[0], lp.y - q[1], lp.z - q[2]};
				const double dl = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
				if(!(dl > rho * (1.0 + 0x1p-20) + 0x1p-30 * (cmax + rad[s])))
				{ // the light inside the ball: any direction
					word = all;
					continue;
				}
				const double w[3] = {d[0] / dl, d[1] / dl, d[2] / dl};
				const double theta = (std::asin(std::min(1.0, rho / dl)) * (1.0 + 0x1p-20) + eta) * cone_scale;
				const double ct = std::cos(theta), st = std::sin(theta);
				// every ray's line passes within near_l of Lp: |o - P|, and the error of L over the way to the light
				const double near_l = eps_o + eta * (dl + rho) * (1.0 + 0x1p-20);
				const double lpd[3] = {lp.x, lp.y, lp.z};
				for(int k = 0; k < ns; k++)
				{
					if(k == s) continue;
					// the half-line rule from the patch's ball; the line rule from the light, where the lines (nearly) meet: the
					// distance from C to a line grows with the distance from Lp, not with the width of the patch
					const BallSphere &b = bs[k];
					const bool ahead = b.meets || cone_ahead(cone_sphere(b.v, b.dist, w, ct, st), b.dist, b.behind);
					const double vl[3] = {C[3 * k] - lpd[0], C[3 * k + 1] - lpd[1], C[3 * k + 2] - lpd[2]};
					const double distl = std::sqrt(vl[0] * vl[0] + vl[1] * vl[1] + vl[2] * vl[2]);
					const double reach_l = b.rk + near_l + 0x1p-30 * (distl + dl + b.rk);
					const bool line = distl <= reach_l || cone_line_touches(cone_sphere(vl, distl, w, ct, st), distl, reach_l);
					if(ahead && line) word |= 1u << k;
				}
				// sphere s: (C - o).L = -|o - C| cos(angle(o - C, L)), and that angle is at most psi + theta_patch + tilt + theta; below 90
				// degrees b < 0 needs R_in cos(.) < 2^-16 E (the rounding of b, as in build_gi_masks)
				const double x = wp[1] * w[2] - wp[2] * w[1], y = wp[2] * w[0] - wp[0] * w[2], z = wp[0] * w[1] - wp[1] * w[0];
				const double psi = std::atan2(std::sqrt(x * x + y * y + z * z), wp[0] * w[0] + wp[1] * w[1] + wp[2] * w[2]);
				const double ang = psi + cth[cell] + tilt + theta + 0x1p-30;
				if(!(R_in > 0.0 && ang < 0.5 * M_PI && R_in * std::cos(ang) > behind_own)) word |= 1u << s;
			}
		}
		base += (size_t) 6 * G[s] * G[s];
	}
	shadow_surface_stride = (uint32_t) stride;
	shadow_surface.swap(table);
	shadow_surface_head.swap(head);
}

// Exact-preserving culling data for the triangle walk (DESIGN.md "Triangle chunks").
//
// In exact arithmetic utils.h:181-213 accepts the line o + t d iff it meets the plane of the triangle in
// X = v0 + a e1 + b e2 with a in [-1, 0] (the reference's u carries a flipped sign), b >= 0, b - a <= 1,
// i.e. inside the triangle (v0, v0 - e1, v0 + e2), and |det| >= 1e-5.  In binary32 the computed u, v differ
// from the exact ones by at most
//     eta_u <= 7 eps |d| |e2| (|T| + 1.01 |e1|) / 0.99e-5,   eta_v <= 7 eps |d| |e1| (|T| + 1.01 |e2|) / 0.99e-5
// (eps = 2^-24; three-term dot products and 2x2 cross terms of rounded inputs, divided by a determinant that
// the test itself bounds away from zero), so an accepted line passes within eta_u |e1| + eta_v |e2| of that
// triangle.  Every chunk gets a sphere around its triangles' accept regions, inflated by 16x that slack
// (evaluated for |d| <= d_max, one set of spheres per entry of SKR_CULL_DMAX_LIST, and the farthest possible ray origin: camera or any sphere surface) plus
// an absolute term for the rounding of the device's own line-sphere test.  Where the slack is not small the
// radius becomes infinite and the chunk is simply never culled.
void skr_scene::build_triangle_chunks()
{
	tri_chunks.clear();
	tri_any_cone = false;
	if(info.n_triangles == 0) return;
	const double dmax[SKR_CULL_LEVELS] = SKR_CULL_DMAX_LIST;
	for(int level = 0; level < SKR_CULL_LEVELS; level++)
	{
		std::vector<skr_f4> one;
		build_triangle_chunk_level(dmax[level], one);
		tri_chunk_stride = one.size();
		tri_chunks.insert(tri_chunks.end(), one.begin(), one.end());
	}
	// the ray queries' ball: around the bounding box of every point a renderer's ray can start at or hit, twice that box's half diagonal
	double lo[3] = {info.camera[0], info.camera[1], info.camera[2]}, hi[3] = {lo[0], lo[1], lo[2]};
	auto grow = [&](double x, double y, double z, double r) {
		const double p[3] = {x, y, z};
		for(int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], p[k] - r); hi[k] = std::max(hi[k], p[k] + r); }
	};
	for(int i = 0; i < info.n_spheres; i++)
	{
		const float *s = &raw_spheres[(size_t) i * 14];
		grow(s[0], s[1], s[2], std::fabs((double) s[3]));
	}
	for(int i = 0; i < info.n_triangles; i++)
	{ // the accept region (v0, v0 - e1, v0 + e2)
		const skr_f4 v0 = tris[3 * i], e1 = tris[3 * i + 1], e2 = tris[3 * i + 2];
		grow(v0.x, v0.y, v0.z, 0);
		grow((double) v0.x - e1.x, (double) v0.y - e1.y, (double) v0.z - e1.z, 0);
		grow((double) v0.x + e2.x, (double) v0.y + e2.y, (double) v0.z + e2.z, 0);
	}
	const double cx = 0.5 * (lo[0] + hi[0]), cy = 0.5 * (lo[1] + hi[1]), cz = 0.5 * (lo[2] + hi[2]);
	const double half = 0.5 * std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
	trace_ball[0] = (float) cx;
	trace_ball[1] = (float) cy;
	trace_ball[2] = (float) cz;
	trace_ball[3] = (float) (2 * half + 1e-3);
	// the device tests fl(|o - c|^2) <= fl(r)^2 against the float centre: the tree is built for a ball wider by far more than that rounding
	const double ball[4] = {trace_ball[0], trace_ball[1], trace_ball[2], (double) trace_ball[3] * 1.001 + 1e-3};
	trace_chunks.clear();
	const bool render_cone = tri_any_cone; // (the flag the builder raises belongs to the renderer's tree)
	tri_any_cone = false;
	for(int level = 0; level < SKR_CULL_LEVELS; level++)
	{
		std::vector<skr_f4> one;
		build_triangle_chunk_level(dmax[level], one, ball);
		trace_chunks.insert(trace_chunks.end(), one.begin(), one.end());
	}
	trace_any_cone = tri_any_cone;
	tri_any_cone = render_cone;
}

// Grazing rays are what makes the slack above large: |det| = |d . (e1 x e2)| may be as small as 1e-5.  Where a
// chunk's triangles are (nearly) coplanar — unit normals within an angle alpha of an axis a — every ray with
// |d . a| >= kappa |d| meets all of them at |d^ . n^_i| >= s = kappa cos(alpha) - sin(alpha) > 0, so that
// |det_i| >= |d| |e1_i x e2_i| s and
//     eta_u <= 7 eps |e2| (|T| + 1.01 |e1|) / (0.99 |e1 x e2| s)      (no |d|, no 1e-5),
// which gives such rays a second, "tight" radius that is finite for triangles of any size (test.scn's wall: eta
// ~ 2e-2 with kappa = 1e-3 against ~ 7 for the general bound).  The device picks per lane: tight where
// (d . a / kappa)^2 >= d . d, the general radius otherwise.  kappa = max(1e-3, 4 sin(alpha)); cones wider than
// kappa = 0.5 and chunks with sliver triangles get no tight radius.  Nodes merge their children's cones:
// kappa_p >= (kappa_c + sin(beta_c)) / cos(beta_c), beta_c the angle between the axes.
namespace {
struct Cone { // unit axis, kappa; valid = a tight radius exists
	double ax, ay, az, kappa;
	bool valid;
};
struct Ball {
	double x, y, z, r_loose, r_tight;
	bool unbounded; // loose radius infinite
	Cone cone;
};
const double KAPPA_MIN = 1e-3, KAPPA_MAX = 0.5;
const double KAPPA_DEVICE_ROOM = 1e-3; // the device's binary32 (d . a / kappa)^2 >= d . d may call a ray 1e-3 (relative) short of kappa non-grazing

float round_up_square(double r, bool infinite)
{
	const double r2 = r * r;
	float f = (float) r2;
	if((double) f < r2) f = std::nextafterf(f, INFINITY);
	if(infinite || !(r2 == r2)) f = INFINITY;
	return f;
}
void ball_entries(const Ball &b, skr_f4 &A, skr_f4 &B)
{
	A = {(float) b.x, (float) b.y, (float) b.z, round_up_square(b.r_loose, b.unbounded)};
	if(b.cone.valid)
	{
		const double inv = 1.0 / b.cone.kappa;
		B = {(float) (b.cone.ax * inv), (float) (b.cone.ay * inv), (float) (b.cone.az * inv), round_up_square(b.r_tight, false)};
		if(!(B.w < A.w)) B = {0.0f, 0.0f, 0.0f, A.w}; // the tight radius must be a gain
	}
	else B = {0.0f, 0.0f, 0.0f, A.w};
}
} // namespace

void skr_scene::build_triangle_chunk_level(double d_max, std::vector<skr_f4> &out, const double *origin_ball)
{
	const int nt = info.n_triangles;
	const double eps = 5.9604644775390625e-08; // 2^-24
	auto norm = [](double x, double y, double z) { return std::sqrt(x * x + y * y + z * z); };
	// where rays can start: the camera, or on a sphere (GI children, raytrace.h:128)
	struct Org { double x, y, z, r; };
	std::vector<Org> orgs;
	if(origin_ball) orgs.push_back({origin_ball[0], origin_ball[1], origin_ball[2], origin_ball[3]});
	else orgs.push_back({info.camera[0], info.camera[1], info.camera[2], 1e-3});
	for(int i = 0; i < info.n_spheres && !origin_ball; i++)
	{
		const float *s = &raw_spheres[(size_t) i * 14];
		orgs.push_back({s[0], s[1], s[2], std::fabs((double) s[3]) + 1e-3});
	}
	tri_chunk_size = info.n_spheres == 0 ? SKR_TRI_CHUNK_COHERENT : SKR_TRI_CHUNK_MIXED; // see tri_chunks.h
	if(const char *e = getenv("SKR_TRI_CHUNK")) // tuning runs only
		if(atoi(e) >= 1 && atoi(e) <= 64) tri_chunk_size = atoi(e);
	const int nc = (nt + tri_chunk_size - 1) / tri_chunk_size;
	std::vector<std::vector<Ball>> levels(1);
	for(int c = 0; c < nc; c++)
	{
		const int i0 = c * tri_chunk_size, i1 = std::min(nt, i0 + tri_chunk_size);
		Ball b{0, 0, 0, 0, 0, false, {0, 0, 0, 0, false}};
		int np = 0;
		std::vector<double> pts;
		double slack = 0, mag = 0;
		// pass 1: geometry, the general slack, the normal cone
		struct Tri { double l1, l2, area2, tmax, nx, ny, nz; };
		std::vector<Tri> tr;
		bool cone_ok = true;
		double sx = 0, sy = 0, sz = 0;
		for(int i = i0; i < i1; i++)
		{
			const skr_f4 v0 = tris[3 * i], e1 = tris[3 * i + 1], e2 = tris[3 * i + 2];
			const double P[3][3] = {{v0.x, v0.y, v0.z}, {(double) v0.x - e1.x, (double) v0.y - e1.y, (double) v0.z - e1.z},
									{(double) v0.x + e2.x, (double) v0.y + e2.y, (double) v0.z + e2.z}};
			for(auto &q : P)
			{
				pts.insert(pts.end(), q, q + 3);
				b.x += q[0]; b.y += q[1]; b.z += q[2];
				np++;
				mag = std::max(mag, std::max(std::fabs(q[0]), std::max(std::fabs(q[1]), std::fabs(q[2]))));
			}
			double tmax = 0;
			for(const Org &o : orgs) tmax = std::max(tmax, norm(o.x - v0.x, o.y - v0.y, o.z - v0.z) + o.r);
			const double l1 = norm(e1.x, e1.y, e1.z), l2 = norm(e2.x, e2.y, e2.z);
			const double eta_u = 7 * eps * d_max * l2 * (tmax + 1.01 * l1) / 0.99e-5;
			const double eta_v = 7 * eps * d_max * l1 * (tmax + 1.01 * l2) / 0.99e-5;
			const double rho_det = 7 * eps * d_max * l1 * l2 / 1e-5; // relative error of the computed determinant at the 1e-5 threshold
			if(!(eta_u < 0.25) || !(eta_v < 0.25) || !(rho_det < 0.01)) b.unbounded = true;
			slack = std::max(slack, 16 * (eta_u * l1 + eta_v * l2));
			mag = std::max(mag, tmax);
			// e1 x e2
			const double mx = (double) e1.y * e2.z - (double) e1.z * e2.y, my = (double) e1.z * e2.x - (double) e1.x * e2.z,
						 mz = (double) e1.x * e2.y - (double) e1.y * e2.x;
			const double area2 = norm(mx, my, mz);
			Tri t{l1, l2, area2, tmax, 0, 0, 0};
			if(!(area2 > 1e-3 * l1 * l2) || !(l1 * l2 > 0)) cone_ok = false; // sliver or degenerate: its determinant is noise
			else
			{
				t.nx = mx / area2; t.ny = my / area2; t.nz = mz / area2;
				if(!tr.empty() && t.nx * tr[0].nx + t.ny * tr[0].ny + t.nz * tr[0].nz < 0) { t.nx = -t.nx; t.ny = -t.ny; t.nz = -t.nz; } // |d . n| has no orientation
				sx += t.nx; sy += t.ny; sz += t.nz;
			}
			tr.push_back(t);
		}
		b.x /= np; b.y /= np; b.z /= np;
		double rad = 0;
		for(int k = 0; k < np; k++) rad = std::max(rad, norm(pts[3 * k] - b.x, pts[3 * k + 1] - b.y, pts[3 * k + 2] - b.z));
		b.r_loose = (rad + slack) * (1 + 1e-4) + 1e-5 * (1 + mag); // + relative and absolute room for the device-side test's own rounding
		// pass 2: the tight radius of non-grazing rays
		const double sl = norm(sx, sy, sz);
		if(cone_ok && sl > 0)
		{
			Cone cn{sx / sl, sy / sl, sz / sl, 0, false};
			double cosa = 1;
			for(const Tri &t : tr) cosa = std::min(cosa, std::fabs(t.nx * cn.ax + t.ny * cn.ay + t.nz * cn.az));
			cosa = std::max(0.0, cosa - 1e-12);
			const double sina = std::sqrt(std::max(0.0, 1 - cosa * cosa));
			cn.kappa = std::max(KAPPA_MIN, 4 * sina) * 1.001;
			const double s = (cn.kappa * (1 - KAPPA_DEVICE_ROOM) * cosa - sina) * 0.99;
			if(cn.kappa <= KAPPA_MAX && s > 0)
			{
				double tight = 0;
				bool ok = true;
				for(const Tri &t : tr)
				{
					const double det_min = 0.99 * t.area2 * s; // per unit |d|
					const double eta_u = 7 * eps * t.l2 * (t.tmax + 1.01 * t.l1) / det_min, eta_v = 7 * eps * t.l1 * (t.tmax + 1.01 * t.l2) / det_min;
					const double rho_det = 7 * eps * t.l1 * t.l2 / (t.area2 * s);
					if(!(eta_u < 0.25) || !(eta_v < 0.25) || !(rho_det < 0.01)) ok = false;
					tight = std::max(tight, 16 * (eta_u * t.l1 + eta_v * t.l2));
				}
				if(ok)
				{
					cn.valid = true;
					b.cone = cn;
					b.r_tight = (rad + tight) * (1 + 1e-4) + 1e-5 * (1 + mag);
				}
			}
		}
		levels[0].push_back(b);
	}
	// Upper levels: one ball around every SKR_TRI_SUPER consecutive balls of the level below (a line that touches a
	// child's sphere touches this one — for the general radii, and for the tight ones under the merged cone), until
	// a single root is left.  The levels above the chunks are laid out depth-first with skip links — node =
	// {centre, R^2} {axis / kappa, R_tight^2} {skip, first chunk, chunk count, height} — so that the device walks
	// them with one wave-uniform index and no stack: touched -> next entry, missed -> entry [skip]; a node of
	// height 1 runs over its (contiguous) chunk entries in a tight loop.  The chunk entries ({centre, R^2} {axis /
	// kappa, R_tight^2}) follow the nodes in the same array.
	do
	{
		const std::vector<Ball> &lo = levels.back();
		std::vector<Ball> up;
		for(size_t c0 = 0; c0 < lo.size(); c0 += SKR_TRI_SUPER)
		{
			const size_t c1 = std::min(lo.size(), c0 + SKR_TRI_SUPER);
			Ball b{0, 0, 0, 0, 0, false, {0, 0, 0, 0, false}};
			bool cones = true;
			double sx = 0, sy = 0, sz = 0;
			for(size_t c = c0; c < c1; c++)
			{
				b.x += lo[c].x; b.y += lo[c].y; b.z += lo[c].z;
				b.unbounded = b.unbounded || lo[c].unbounded;
				cones = cones && lo[c].cone.valid;
				if(cones)
				{
					const Cone &k = lo[c].cone, &k0 = lo[c0].cone;
					const double sgn = (k.ax * k0.ax + k.ay * k0.ay + k.az * k0.az) < 0 ? -1.0 : 1.0;
					sx += sgn * k.ax; sy += sgn * k.ay; sz += sgn * k.az;
				}
			}
			b.x /= (double) (c1 - c0); b.y /= (double) (c1 - c0); b.z /= (double) (c1 - c0);
			double mag = 0;
			for(size_t c = c0; c < c1; c++)
			{
				const double off = norm(lo[c].x - b.x, lo[c].y - b.y, lo[c].z - b.z);
				b.r_loose = std::max(b.r_loose, off + lo[c].r_loose * (1 + 1e-6));
				if(cones) b.r_tight = std::max(b.r_tight, off + lo[c].r_tight * (1 + 1e-6));
				mag = std::max(mag, std::max(std::fabs(lo[c].x), std::max(std::fabs(lo[c].y), std::fabs(lo[c].z))) + lo[c].r_loose);
			}
			if(!(mag < 1e300)) mag = 0; // unbounded children: the general radius is infinite anyway
			b.r_loose = b.r_loose * (1 + 1e-4) + 1e-5 * (1 + mag); // room for the float centre and the device-side test's own rounding
			const double sl = norm(sx, sy, sz);
			if(cones && sl > 0)
			{
				Cone cn{sx / sl, sy / sl, sz / sl, 0, true};
				for(size_t c = c0; c < c1 && cn.valid; c++)
				{
					const Cone &k = lo[c].cone;
					const double cosb = std::max(0.0, std::fabs(k.ax * cn.ax + k.ay * cn.ay + k.az * cn.az) - 1e-12);
					const double sinb = std::sqrt(std::max(0.0, 1 - cosb * cosb));
					// a ray the device calls non-grazing here has |d^ . a_p| >= kappa_p (1 - room); it must be non-grazing
					// for the child in the child's own sense, |d^ . a_c| >= kappa_c
					if(!(cosb > 0.5)) cn.valid = false;
					else cn.kappa = std::max(cn.kappa, (k.kappa + sinb) / cosb / (1 - KAPPA_DEVICE_ROOM) * 1.001);
				}
				if(cn.valid && cn.kappa <= KAPPA_MAX)
				{
					b.cone = cn;
					double mt = 0;
					for(size_t c = c0; c < c1; c++) mt = std::max(mt, std::max(std::fabs(lo[c].x), std::max(std::fabs(lo[c].y), std::fabs(lo[c].z))) + lo[c].r_tight);
					b.r_tight = b.r_tight * (1 + 1e-4) + 1e-5 * (1 + mt);
				}
			}
			up.push_back(b);
		}
		levels.push_back(up);
	} while(levels.back().size() > 1);
	std::vector<skr_f4> nodes;
	auto f4i = [](int32_t a, int32_t b, int32_t c, int32_t d) {
		skr_f4 v;
		memcpy(&v.x, &a, 4); memcpy(&v.y, &b, 4); memcpy(&v.z, &c, 4); memcpy(&v.w, &d, 4);
		return v;
	};
	struct Emit {
		const std::vector<std::vector<Ball>> &levels;
		std::vector<skr_f4> &nodes;
		decltype(f4i) &pack;
		void run(int level, size_t idx)
		{
			const size_t me = nodes.size();
			skr_f4 A, B;
			ball_entries(levels[level][idx], A, B);
			nodes.push_back(A);
			nodes.push_back(B);
			nodes.push_back({0, 0, 0, 0});
			int first = 0, count = 0;
			if(level == 1)
			{
				first = (int) idx * SKR_TRI_SUPER;
				count = (int) std::min(levels[0].size(), (size_t) first + SKR_TRI_SUPER) - first;
			}
			else
			{
				const size_t c0 = idx * SKR_TRI_SUPER, c1 = std::min(levels[level - 1].size(), c0 + SKR_TRI_SUPER);
				for(size_t c = c0; c < c1; c++) run(level - 1, c);
			}
			nodes[me + 2] = pack((int32_t) (nodes.size() / 3), first, count, level);
		}
	};
	Emit emit{levels, nodes, f4i};
	emit.run((int) levels.size() - 1, 0);
	// one pad node so that the walk may prefetch past the end, then the chunk entries (+ a pad entry)
	const int32_t n_nodes = (int32_t) (nodes.size() / 3);
	nodes.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	nodes.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	nodes.push_back(f4i(n_nodes + 1, 0, 0, 0));
	size_t with_cone = 0;
	for(const Ball &b : levels[0])
	{
		skr_f4 A, B;
		ball_entries(b, A, B);
		nodes.push_back(A);
		nodes.push_back(B);
		if(B.w < A.w) with_cone++;
	}
	// the cone test costs every sphere test ~8 instructions (dragon: +8 % with one planar chunk in 1251): the walk
	// only compiles it in where at least a quarter of the chunks gain a tighter radius from it
	const bool any_cone = 4 * with_cone >= levels[0].size();
	nodes.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	nodes.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	tri_node_count = n_nodes;
	tri_any_cone = tri_any_cone || any_cone;
	out.swap(nodes);
}

// Exact-preserving culling data for the sphere walks.
//
// A sphere {c, r^2} is a candidate for the ray (o, d) where the binary32 D = fl(b b - 4a c') of utils.h:113-121 is >= 0 (and b < 0), with
// e = fl(o - c), b = 2 fl(d . e), c' = fl(fl(e . e) - r^2), a = fl(d . d).  In reals D = 4 (r^2 |d|^2 - |e x d|^2).  With u = 2^-24, every
// three-term dot product within 3u of its sum of magnitudes and e within u of o - c, the two sides of the last (sign-exact) subtraction
// are off by at most 9u |d|^2 |e|^2 (the square of b / 2) and u (10 |e|^2 + 5 r^2) |d|^2 (4a c'), so a candidate's line passes the
// centre within rho, rho^2 <= r^2 (1 + 32u) + 32u |e|^2 (32 for 19 and 5: room for the second-order terms).  The slack grows with
// |e|, the distance from the ray's origin, so it is carried to the device as a factor: an entry {C, R^2, kappa} is touched where
//     |(C - o) x d|^2 <= (R^2 + kappa |C - o|^2) |d|^2.
// For a member sphere at g = |C - c| with h^2 = r^2 (1 + 32u), |e| <= |C - o| + g gives |e|^2 <= 2 |C - o|^2 + 2 g^2 and the line's
// distance from C is at most g + sqrt(h^2 + 32u |e|^2), whose square is at most
//     (g + h)^2 + 64u (1 + g / h) g^2  +  64u (1 + g / h) |C - o|^2              (sqrt(h^2 + x) <= h + x / 2h), or
//     (1 + s) (g + h)^2 + 2 (s + 32u) g^2  +  2 (s + 32u) |C - o|^2,  s = sqrt(32u)  (sqrt(h^2 + x) <= h + sqrt(x)),
// whichever has the smaller factor; R^2 and kappa of an entry are the largest of its members'.  The device's own test forms the cross
// product of rounded terms: its left side is within (1 + 3u) and 19u |C - o|^2 |d|^2 of the real one and its right side within 12u, so
// kappa carries 19u more and both carry a relative 1e-4.  Anything that is not finite makes the radius infinite (never culled).
namespace {
struct SphereBound {
	double x, y, z, R, kappa; // R: radius (before squaring); kappa: the factor of |C - o|^2
	bool unbounded;
};
const double ST_U = 5.9604644775390625e-08; // 2^-24

// the entry around device spheres [i0, i1) (rows: {centre, r^2})
SphereBound sphere_bound(const std::vector<skr_f4> &rows, size_t i0, size_t i1)
{
	double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
	for(size_t i = i0; i < i1; i++)
	{
		const double r = std::sqrt((double) rows[i].w), c[3] = {rows[i].x, rows[i].y, rows[i].z};
		for(int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], c[k] - r); hi[k] = std::max(hi[k], c[k] + r); }
	}
	SphereBound b{0, 0, 0, 0, 0, false};
	// the centre is the float the device reads: every distance below is taken from it
	b.x = (double) (float) (0.5 * (lo[0] + hi[0]));
	b.y = (double) (float) (0.5 * (lo[1] + hi[1]));
	b.z = (double) (float) (0.5 * (lo[2] + hi[2]));
	const double s = std::sqrt(32 * ST_U);
	double R2 = 0;
	for(size_t i = i0; i < i1; i++)
	{
		const double dx = rows[i].x - b.x, dy = rows[i].y - b.y, dz = rows[i].z - b.z;
		const double g = std::sqrt(dx * dx + dy * dy + dz * dz), h = std::sqrt((double) rows[i].w * (1 + 32 * ST_U));
		const double ka = 64 * ST_U * (1 + g / h), kb = 2 * (s + 32 * ST_U);
		double k, r2;
		if(ka <= kb) { k = ka; r2 = (g + h) * (g + h) + ka * g * g; }
		else { k = kb; r2 = (1 + s) * (g + h) * (g + h) + kb * g * g; }
		if(!(r2 == r2) || !(k == k) || !(r2 < 1e300)) b.unbounded = true;
		R2 = std::max(R2, r2);
		b.kappa = std::max(b.kappa, k);
	}
	b.R = std::sqrt(R2);
	if(!(b.x == b.x) || !(b.y == b.y) || !(b.z == b.z) || std::isinf(b.x) || std::isinf(b.y) || std::isinf(b.z)) b.unbounded = true;
	return b;
}
void sphere_bound_rows(const SphereBound &b, skr_f4 &A, float &kappa)
{
	A = {(float) b.x, (float) b.y, (float) b.z, round_up_square(b.R * std::sqrt(1 + 1e-4), b.unbounded)};
	const double k = (b.kappa + 19 * ST_U) * (1 + 1e-4);
	kappa = (float) k;
	if((double) kappa < k) kappa = std::nextafterf(kappa, INFINITY);
	if(b.unbounded) { A.x = A.y = A.z = 0.0f; kappa = 0.0f; }
}
skr_f4 pack_row(float a, int32_t b, int32_t c, int32_t d)
{
	skr_f4 v;
	v.x = a;
	memcpy(&v.y, &b, 4); memcpy(&v.z, &c, 4); memcpy(&v.w, &d, 4);
	return v;
}
uint64_t morton_spread(uint64_t v)
{ // 21 bits, two zero bits between neighbours
	v &= 0x1fffff;
	v = (v | v << 32) & 0x1f00000000ffffull;
	v = (v | v << 16) & 0x1f0000ff0000ffull;
	v = (v | v << 8) & 0x100f00f00f00f00full;
	v = (v | v << 4) & 0x10c30c30c30c30c3ull;
	v = (v | v << 2) & 0x1249249249249249ull;
	return v;
}
} // namespace

void skr_build_sphere_tree(const skr_scene &sc, SkrSphereTree &t)
{
	t = SkrSphereTree();
	const size_t n = sc.sph_geom.size();
	// the ball: around the bounding box of the camera, the spheres and the mesh, twice that box's half diagonal (as the trace tree's)
	double lo[3] = {sc.info.camera[0], sc.info.camera[1], sc.info.camera[2]}, hi[3] = {lo[0], lo[1], lo[2]};
	auto grow = [&](double x, double y, double z, double r) {
		const double p[3] = {x, y, z};
		for(int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], p[k] - r); hi[k] = std::max(hi[k], p[k] + r); }
	};
	for(size_t i = 0; i < n; i++) grow(sc.sph_geom[i].x, sc.sph_geom[i].y, sc.sph_geom[i].z, std::sqrt((double) sc.sph_geom[i].w));
	for(size_t i = 0; i + 2 < sc.raw_triangles.size(); i += 3) grow(sc.raw_triangles[i], sc.raw_triangles[i + 1], sc.raw_triangles[i + 2], 0);
	const double half = 0.5 * std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
	t.ball[0] = (float) (0.5 * (lo[0] + hi[0]));
	t.ball[1] = (float) (0.5 * (lo[1] + hi[1]));
	t.ball[2] = (float) (0.5 * (lo[2] + hi[2]));
	t.ball[3] = (float) (2 * half + 1e-3);
	// (the bounds above are relative: the ball only keeps |C - o|^2 |d|^2 far from the ends of binary32.  |d|^2 <= 2^44 on the device.)
	if(!(t.ball[3] < 1e8f) || !(t.ball[0] == t.ball[0]) || !(t.ball[1] == t.ball[1]) || !(t.ball[2] == t.ball[2])) t.ball[3] = -1.0f; // no wave walks the tree (api.cpp sphere_tree_of: the device squares the radius, so the sign is read there)
	// always tested: a sphere that is not finite or tiny (the relative bounds need normal numbers), and one that would blow up every
	// entry above it — a radius beyond 8x the median radius (the 1000-radius ground spheres of the shipped scenes)
	std::vector<double> radii(n);
	for(size_t i = 0; i < n; i++) radii[i] = std::sqrt((double) sc.sph_geom[i].w);
	double big = INFINITY;
	if(n > 0)
	{
		std::vector<double> sorted(radii);
		std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
		big = 8 * sorted[n / 2];
	}
	std::vector<int32_t> always, rest;
	for(size_t i = 0; i < n; i++)
	{
		const skr_f4 g = sc.sph_geom[i];
		const bool finite = std::isfinite(g.x) && std::isfinite(g.y) && std::isfinite(g.z) && std::isfinite(g.w);
		if(!finite || !(g.w >= 1e-30f) || !(radii[i] <= big)) always.push_back((int32_t) i);
		else rest.push_back((int32_t) i);
	}
	{ // Morton order of the centres
		double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
		for(int32_t i : rest)
		{
			const double c[3] = {sc.sph_geom[i].x, sc.sph_geom[i].y, sc.sph_geom[i].z};
			for(int k = 0; k < 3; k++) { clo[k] = std::min(clo[k], c[k]); chi[k] = std::max(chi[k], c[k]); }
		}
		const double ext = std::max(chi[0] - clo[0], std::max(chi[1] - clo[1], chi[2] - clo[2]));
		const double scale = ext > 0 ? 2097151.0 / ext : 0.0;
		std::vector<std::pair<uint64_t, int32_t>> keyed;
		keyed.reserve(rest.size());
		for(int32_t i : rest)
		{
			const uint64_t x = (uint64_t) ((sc.sph_geom[i].x - clo[0]) * scale), y = (uint64_t) ((sc.sph_geom[i].y - clo[1]) * scale),
						   z = (uint64_t) ((sc.sph_geom[i].z - clo[2]) * scale);
			keyed.push_back({morton_spread(x) | morton_spread(y) << 1 | morton_spread(z) << 2, i});
		}
		std::sort(keyed.begin(), keyed.end()); // (equal codes: file order)
		for(size_t k = 0; k < keyed.size(); k++) rest[k] = keyed[k].second;
	}
	for(int32_t i : always) { t.rows.push_back(sc.sph_geom[i]); t.file.push_back(i); }
	for(int32_t i : rest) { t.rows.push_back(sc.sph_geom[i]); t.file.push_back(i); }
	const size_t na = always.size(), CH = SKR_SPHERE_CHUNK;
	t.n_always = (int) ((na + CH - 1) / CH);
	const size_t n_reg = (rest.size() + CH - 1) / CH;
	t.n_chunks = t.n_always + (int) n_reg;
	// the chunks: rows [first, first + count), their smallest file index
	struct Ent { SphereBound b; size_t first, last; int32_t min_index; skr_f4 A; float kappa; };
	auto min_file = [&](size_t i0, size_t i1) { int32_t m = INT32_MAX; for(size_t i = i0; i < i1; i++) m = std::min(m, t.file[i]); return m; };
	std::vector<Ent> chunk_ents;
	for(int c = 0; c < t.n_chunks; c++)
	{
		const bool alw = c < t.n_always;
		const size_t i0 = alw ? (size_t) c * CH : na + (size_t) (c - t.n_always) * CH, i1 = std::min(alw ? na : n, i0 + CH);
		Ent e{};
		e.first = i0;
		e.last = i1;
		e.min_index = min_file(i0, i1);
		if(alw) e.b = SphereBound{0, 0, 0, 0, 0, true};
		else e.b = sphere_bound(t.rows, i0, i1);
		sphere_bound_rows(e.b, e.A, e.kappa);
		chunk_ents.push_back(e);
	}
	for(const Ent &e : chunk_ents)
	{
		t.chunks.push_back(e.A);
		t.chunks.push_back(pack_row(e.kappa, e.min_index, (int32_t) e.first, (int32_t) (e.last - e.first)));
		skr_f4 f{0, 0, 0, 0};
		int32_t fi[4] = {0, 0, 0, 0};
		for(size_t i = e.first; i < e.last; i++) fi[i - e.first] = t.file[i];
		memcpy(&f, fi, 16);
		t.chunks.push_back(f);
	}
	t.chunks.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	t.chunks.push_back(pack_row(0.0f, INT32_MAX, 0, 0));
	t.chunks.push_back({0.0f, 0.0f, 0.0f, 0.0f});
	// the levels above the regular chunks: every entry bounds its own members (the slack does not pile up level by level) and holds its
	// children's spheres
	std::vector<std::vector<Ent>> levels(1);
	levels[0].assign(chunk_ents.begin() + t.n_always, chunk_ents.end());
	while(!levels[0].empty() && (levels.size() == 1 || levels.back().size() > 1))
	{
		const std::vector<Ent> &lo_l = levels.back();
		std::vector<Ent> up;
		for(size_t c0 = 0; c0 < lo_l.size(); c0 += SKR_SPHERE_SUPER)
		{
			const size_t c1 = std::min(lo_l.size(), c0 + SKR_SPHERE_SUPER);
			Ent e{};
			e.first = lo_l[c0].first;
			e.last = lo_l[c1 - 1].last;
			e.min_index = INT32_MAX;
			e.b = sphere_bound(t.rows, e.first, e.last);
			for(size_t c = c0; c < c1; c++)
			{
				const Ent &k = lo_l[c];
				e.min_index = std::min(e.min_index, k.min_index);
				e.b.unbounded = e.b.unbounded || k.b.unbounded;
				if(!k.b.unbounded)
				{
					const double dx = (double) k.A.x - e.b.x, dy = (double) k.A.y - e.b.y, dz = (double) k.A.z - e.b.z;
					e.b.R = std::max(e.b.R, (std::sqrt(dx * dx + dy * dy + dz * dz) + std::sqrt((double) k.A.w)) * (1 + 1e-6));
				}
				e.b.kappa = std::max(e.b.kappa, (double) k.kappa); // (not needed for exactness: a parent never culls harder than its child)
			}
			sphere_bound_rows(e.b, e.A, e.kappa);
			up.push_back(e);
		}
		levels.push_back(up);
	}
	struct Emit {
		const std::vector<std::vector<Ent>> &levels;
		std::vector<skr_f4> &nodes;
		int first_regular;
		void run(int level, size_t idx)
		{
			const size_t me = nodes.size();
			const Ent &e = levels[level][idx];
			nodes.push_back(e.A);
			nodes.push_back({0, 0, 0, 0});
			int32_t fc = -1; // first chunk of a node of height 1 (it has the next SKR_SPHERE_SUPER chunks, or those that are left), else -1
			if(level == 1) fc = first_regular + (int32_t) idx * SKR_SPHERE_SUPER;
			else
			{
				const size_t c0 = idx * SKR_SPHERE_SUPER, c1 = std::min(levels[level - 1].size(), c0 + SKR_SPHERE_SUPER);
				for(size_t c = c0; c < c1; c++) run(level - 1, c);
			}
			nodes[me + 1] = pack_row(e.kappa, (int32_t) (nodes.size() / 2), fc, e.min_index);
		}
	};
	if(levels.size() > 1)
	{
		Emit emit{levels, t.nodes, t.n_always};
		emit.run((int) levels.size() - 1, 0);
	}
	t.n_nodes = (int) (t.nodes.size() / 2);
	t.nodes.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	t.nodes.push_back(pack_row(0.0f, t.n_nodes + 1, -1, INT32_MAX));
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
		else
		{
			if(echo) printf("WARNING. Do not know command: %s\n", cmd.c_str());
			info.n_unknown++;
		}
	}
	fclose(fp);
	sc.finalize();
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
