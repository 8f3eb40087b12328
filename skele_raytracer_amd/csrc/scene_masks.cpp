// The direction masks of the sphere walks, built once per scene on the host in binary64: the per-light shadow masks, the GI masks of
// the origin grids, and the surface patches of both (skr_scene::build_shadow_masks, build_gi_masks, build_gi_surface,
// build_shadow_surface; shapes in shadow_cells.h).  DESIGN.md 5.6 "Shadow masks" / "Shadow surface patches", 5.7 "GI masks" and 5.8
// "GI surface patches" derive every margin.  A cleared bit that should be set is a wrong pixel, so every rule that two builders share
// is stated once, in the helpers at the top.  No GPU code in this file.
#include "scene_host.h"

#include <cstring>
#include <algorithm>
#include <cmath>
#include <initializer_list>

namespace {

// ---- 3-vectors of doubles ----
double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
double len3(const double *a) { return std::sqrt(dot3(a, a)); }
void cross3(const double *a, const double *b, double *c)
{
	c[0] = a[1] * b[2] - a[2] * b[1];
	c[1] = a[2] * b[0] - a[0] * b[2];
	c[2] = a[0] * b[1] - a[1] * b[0];
}
double angle3(const double *a, const double *b) // between two unit vectors
{
	double c[3];
	cross3(a, b, c);
	return std::atan2(len3(c), dot3(a, b));
}
double max_abs3(const double *a) { return std::max(std::fabs(a[0]), std::max(std::fabs(a[1]), std::fabs(a[2]))); }

// The cells of a cube map of N x N cells per face (shadow_cells.h addressing): every cell's centre direction (unit, 3 doubles) and
// angular radius, taken at its farthest corner (a cube-map cell is a convex spherical quadrilateral) with the cell widened by 2^-12 in
// face coordinates: the device's v_rcp_f32 face coordinates are within 2^-20 of v's.
void cube_cells(int N, std::vector<double> &cell_dir, std::vector<double> &cell_theta)
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
					const double n = len3(w);
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
					theta = std::max(theta, angle3(wc, w));
				}
				cell_theta[(size_t) (f * N + i) * N + j] = theta;
			}
}

// The direction cells of a GI mask row (cube_cells(SKR_GI_DIR_CELLS)) as cones: unit axes, the angular radii padded for this file's own
// rounding, and their cosines and sines.
struct DirCones { std::vector<double> dir, theta, cth, sth; };
DirCones gi_dir_cones()
{
	DirCones d;
	cube_cells(SKR_GI_DIR_CELLS, d.dir, d.theta);
	for(double &t : d.theta)
	{
		t = t * (1.0 + 0x1p-20) + 0x1p-40;
		d.cth.push_back(std::cos(t));
		d.sth.push_back(std::sin(t));
	}
	return d;
}

// Mask entries (one sphere bit each, an even number of them) as the device reads them: uint32_t where `wide`, else uint16_t,
// little-endian.
std::vector<uint32_t> pack_masks(const std::vector<uint32_t> &masks, bool wide)
{
	if(wide) return masks;
	std::vector<uint32_t> words(masks.size() / 2);
	for(size_t e = 0; e < masks.size(); e += 2) words[e / 2] = masks[e] | masks[e + 1] << 16;
	return words;
}

// The grown radius r' of a sphere for the device's binary32 test, |e| = |o - C| <= E: the discriminant can come out >= 0 for a line
// that just misses the sphere (its slack, 16x), + the rounding of e.
double grown_radius(double r2, double E) { return std::sqrt(r2 + 0x1p-16 * (E * E + r2)) + 0x1p-20 * E; }

// Bounds |o - P| for a shadow ray's origin o = fl(P + 1e-6f) per component, |P| <= pmax (twice over).
double origin_offset_bound(double pmax) { return 2.0 * std::sqrt(3.0) * (1e-6 + 0x1p-23 * (pmax + 1e-6)); }

// (the shell of a sphere's surface points: what the surface patches of both tables are cut from)
struct SurfaceShell {
	float tau;         // the radial slack: |fl(|e|^2) - r^2| <= tau; negative: no patches
	double R_lo, R_hi; // every keyed point has R_lo <= |o - C| <= R_hi
};
SurfaceShell surface_shell(double r2)
{
	SurfaceShell sh;
	// |fl(|e|^2) - r^2| <= tau gives (r^2 - tau)(1 - 2^-20) <= |fl(e)|^2 <= (r^2 + tau)(1 + 2^-20) (the dot product's and the
	// difference's rounding), and |e| is within 2^-23 |e| of |fl(e)|
	sh.tau = std::sqrt(r2) > 1e-3 ? (float) (r2 * 0x1p-7) : -1.0f; // (|o - C| within about r / 256 of r; tiny spheres: no patches)
	sh.R_lo = std::sqrt(std::max(0.0, (r2 - sh.tau) * (1.0 - 0x1p-20))) * (1.0 - 0x1p-22);
	sh.R_hi = std::sqrt((r2 + std::max(0.0f, sh.tau)) * (1.0 + 0x1p-20)) * (1.0 + 0x1p-22);
	return sh;
}

// The scene's spheres in binary64, as every builder below reads them.
struct Spheres {
	int n;
	std::vector<double> C, r2, rad; // centres [n][3], squared radii, radii
	std::vector<SurfaceShell> shell;
	bool in_range = true; // every coordinate and radius below 1e6 (false: NaN, inf, out of the range the margins are derived for)
	explicit Spheres(const std::vector<skr_f4> &geom) : n((int) geom.size()), C((size_t) 3 * n), r2(n), rad(n), shell(n)
	{
		for(int k = 0; k < n; k++)
		{
			C[3 * k] = geom[k].x;
			C[3 * k + 1] = geom[k].y;
			C[3 * k + 2] = geom[k].z;
			r2[k] = geom[k].w;
			rad[k] = std::sqrt(r2[k]);
			shell[k] = surface_shell(r2[k]);
			for(int c = 0; c < 3; c++)
				if(!(std::fabs(C[3 * k + c]) < 1e6)) in_range = false;
			if(!(rad[k] < 1e6)) in_range = false;
		}
	}
};

// Cells per edge of a sphere's cube map of surface patches at the cell edge `edge` (0: no patches).
int cells_per_edge(const SurfaceShell &sh, double rad, double edge)
{
	return sh.tau < 0.0f ? 0 : (int) std::min((double) SKR_GI_SURFACE_MAX_CELLS, std::max(1.0, std::ceil(2.0 * rad / edge)));
}

// Bit `bit` (sphere of centre C, squared radius r2) of every direction cell of a GI mask row, for origins in the ball (q, rho)
// (build_gi_masks' margins).  All in binary64.
// (the ball of origins against one sphere: what every direction cone of ball_cone_touches shares)
struct BallSphere {
	double v[3], dist; // C - q and its length
	double rk;         // the grown radius r'
	double behind, reach;
	bool meets; // the grown sphere meets the ball: every direction
};
BallSphere ball_sphere(const double *q, double rho, const double *C, double r2)
{
	BallSphere b;
	for(int c = 0; c < 3; c++) b.v[c] = C[c] - q[c];
	b.dist = len3(b.v);
	const double E = (b.dist + rho) * (1.0 + 0x1p-20); // bounds |e| = |o - C| of the device's test
	b.rk = grown_radius(r2, E);
	const double tol = 0x1p-30 * (b.dist + rho + b.rk); // (this function's own rounding)
	b.behind = rho + 0x1p-16 * E + tol;                 // b < 0 needs (C - o).d > -2^-22 |e| |d|
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
ConeSphere cone_sphere(const double *v, double dist, const double *w, double ct, double st)
{
	double x[3];
	cross3(v, w, x);
	const double cp = dot3(v, w) / dist, sp = len3(x) / dist;
	const bool lo0 = cp >= ct;   // phi <= theta
	const bool hipi = cp <= -ct; // phi + theta >= pi
	const double sin_lo = lo0 ? 0.0 : sp * ct - cp * st;
	const double sin_hi = hipi ? 0.0 : sp * ct + cp * st;
	return ConeSphere{lo0 ? 1.0 : cp * ct + sp * st, std::max(0.0, std::min(sin_lo, sin_hi))};
}
bool cone_ahead(const ConeSphere &c, double dist, double behind) { return dist * c.cos_lo + behind >= 0.0; }
bool cone_line_touches(const ConeSphere &c, double dist, double reach) { return dist * c.min_sin <= reach; }
// Whether a ray from the ball along some direction of the cone may have D >= 0 and b < 0 for the sphere.
bool ball_cone_touches(const BallSphere &b, const double *w, double ct, double st)
{
	if(b.meets) return true;
	const ConeSphere c = cone_sphere(b.v, b.dist, w, ct, st);
	return cone_ahead(c, b.dist, b.behind) && cone_line_touches(c, b.dist, b.reach);
}
void gi_ball_bits(const double *q, double rho, const double *C, double r2, uint32_t bit, const DirCones &cones, uint32_t *row)
{
	const BallSphere b = ball_sphere(q, rho, C, r2);
	for(int e = 0; e < SKR_GI_ROW_ENTRIES; e++)
		if(ball_cone_touches(b, &cones.dir[3 * (size_t) e], cones.cth[e], cones.sth[e])) row[e] |= bit;
}

// The own-sphere rule of the surface patches: whether every ray from the patch of unit axis `axis` along the cone of unit axis `d`
// leaves the patch's own sphere, so that its bit stays clear.  (C - o).d / |d| = -|o - C| cos(angle(o - C, d)) with |o - C| >= R_in,
// and that angle is at most angle(axis, d) + `pads` (the angular radii of the patch and of the cone, and what else tilts either;
// added in the order given); below 90 degrees b < 0 needs R_in cos(.) < behind (the rounding of b, as in build_gi_masks).
bool leaves_own_sphere(const double *axis, const double *d, std::initializer_list<double> pads, double R_in, double behind)
{
	double ang = angle3(axis, d);
	for(double p : pads) ang += p;
	ang += 0x1p-30;
	return R_in > 0.0 && ang < 0.5 * M_PI && R_in * std::cos(ang) > behind;
}

// The ball (q, rho) of the patch of sphere (C, rad) whose cell has the unit centre direction w and the padded angular radius th.
void surface_patch_ball(const double *C, double rad, const SurfaceShell &sh, const double *w, double th, double *q, double &rho)
{
	const double h = rad * std::cos(th);
	for(int c = 0; c < 3; c++) q[c] = C[c] + h * w[c];
	// the farthest point of the patch from q: |o - q|^2 = R^2 + h^2 - 2 R h cos(phi) grows with phi and is convex in R
	double far = 0.0;
	for(double R : {sh.R_lo, sh.R_hi}) far = std::max(far, std::sqrt(std::max(0.0, R * R + h * h - 2.0 * R * h * std::cos(th))));
	rho = far * (1.0 + 0x1p-20) + 0x1p-30 * (max_abs3(C) + rad);
}
// The padded angular radii of a sphere's G x G x 6 cells (cube_cells) as the patches use them: + the angle between e and fl(e)
void surface_cells(int g, std::vector<double> &dir, std::vector<double> &theta)
{
	dir.clear();
	theta.clear();
	if(g) cube_cells(g, dir, theta);
	for(double &t : theta) t = t * (1.0 + 0x1p-20) + 0x1p-20; // (2^-23 of each component)
}
// The first cell edge the GI patches try: half the one at which the small spheres' patches alone (about 24 r^2 / edge^2 each) fill a
// table of `rows` rows.
double surface_first_edge(const Spheres &S, double rows)
{
	std::vector<double> sorted(S.rad);
	std::sort(sorted.begin(), sorted.end());
	double small_area = 0.0;
	for(int k = 0; k < S.n; k++)
		if(S.rad[k] <= 4.0 * sorted[S.n / 2]) small_area += 24.0 * S.r2[k];
	return std::max(1e-6, 0.5 * std::sqrt(small_area / std::max(1.0, rows)));
}

} // namespace

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
	// reach: the farthest point of the scene (spheres, triangles with their accept regions v0 - e1, v0 + e2) from any light.  The device
	// checks fl(|Lp - P|^2) <= reach^2 per lane, so a shading point outside it only costs that lane the plain walk.
	double reach = 0.0;
	for(int l = 0; l < nl; l++)
	{
		const double lp[3] = {lights[2 * (size_t) l].x, lights[2 * (size_t) l].y, lights[2 * (size_t) l].z};
		auto dist = [&](double x, double y, double z) { const double d[3] = {x - lp[0], y - lp[1], z - lp[2]}; return len3(d); };
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
		const double lp[3] = {lights[2 * (size_t) l].x, lights[2 * (size_t) l].y, lights[2 * (size_t) l].z};
		const double eps_o = origin_offset_bound(max_abs3(lp) + D); // |P| <= |Lp| + D
		for(int k = 0; k < ns; k++)
		{
			const double q[3] = {sph_geom[k].x - lp[0], sph_geom[k].y - lp[1], sph_geom[k].z - lp[2]};
			const double r2 = sph_geom[k].w, qq = dot3(q, q), qn = std::sqrt(qq);
			const double E = (qn + D + eps_o) * (1.0 + 0x1p-20); // bounds |e| = |o - C| of the device's test
			const double rk = grown_radius(r2, E);
			const double S = qn + rk; // farthest point of the grown sphere from Lp
			const double base = rk + eps_o + eta * (S + D + eps_o) / (1.0 - eta) + 0x1p-30 * qn;
			for(int c = 0; c < SKR_SHADOW_TABLE_WORDS; c++)
			{
				const double s = dot3(q, &cell_dir[3 * (size_t) c]);
				const double dist = std::sqrt(std::max(0.0, qq - s * s));
				if(dist <= base + cell_theta[c] * S) masks[(size_t) l * SKR_SHADOW_TABLE_WORDS + c] |= 1u << k;
			}
		}
	}
	shadow_masks.swap(masks);
	shadow_reach2 = reach2;
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
	const Spheres S(sph_geom);
	if(!S.in_range) return; // (no masks)
	const std::vector<double> &C = S.C, &rad = S.rad;
	std::vector<double> sorted(rad);
	std::sort(sorted.begin(), sorted.end());
	const double small = 4.0 * sorted[ns / 2];
	SkrBox all, fine; // around every sphere; around the small ones
	double rsmall = 0.0;
	for(int k = 0; k < ns; k++)
	{
		all.grow(C[3 * k], C[3 * k + 1], C[3 * k + 2], rad[k]);
		if(rad[k] <= small)
		{
			fine.grow(C[3 * k], C[3 * k + 1], C[3 * k + 2], rad[k]);
			rsmall = std::max(rsmall, rad[k]);
		}
	}
	double *flo = fine.lo, *fhi = fine.hi, ext_f = 0.0;
	const double *alo = all.lo, *ahi = all.hi;
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
							const double d[3] = {C[3 * s] - cl.q[0], C[3 * s + 1] - cl.q[1], C[3 * s + 2] - cl.q[2]};
							const double dist = len3(d);
							near = std::fabs(dist - rad[s]) <= rho + 1e-4 + 0x1p-16 * (dist + rad[s]);
						}
						index.push_back(near ? (int32_t) cells.size() : -1);
						if(near) cells.push_back(cl);
					}
		}
		fits = ((index.size() + 1) & ~(size_t) 1) * 4 + cells.size() * row_bytes <= SKR_GI_MAX_BYTES;
	}
	if(!fits || cells.empty()) return;
	const DirCones cones = gi_dir_cones();
	std::vector<uint32_t> masks(cells.size() * SKR_GI_ROW_ENTRIES, 0u);
	for(size_t ci = 0; ci < cells.size(); ci++)
		for(int k = 0; k < ns; k++) gi_ball_bits(cells[ci].q, cells[ci].rho, &C[3 * k], S.r2[k], 1u << k, cones, &masks[ci * SKR_GI_ROW_ENTRIES]);
	// index (an even number of words), masks, padded to whole 16-byte rows
	const size_t n_index = (index.size() + 1) & ~(size_t) 1;
	std::vector<uint32_t> table(n_index, 0u);
	memcpy(table.data(), index.data(), index.size() * 4);
	const std::vector<uint32_t> words = pack_masks(masks, gi_wide != 0);
	table.insert(table.end(), words.begin(), words.end());
	table.resize((table.size() + 3) & ~(size_t) 3, 0u);
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
	const Spheres S(sph_geom); // (in range: the scene has GI masks)
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
	double edge = surface_first_edge(S, (double) SKR_GI_MAX_BYTES / (row_words * 4)), used_edge = 0.0;
	for(int attempt = 0; attempt < 200 && !fits; attempt++, edge *= 1.15)
	{
		patches.clear();
		n_index = 0;
		for(int k = 0; k < ns; k++)
		{
			const int g = cells_per_edge(S.shell[k], S.rad[k], edge);
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
				surface_patch_ball(&S.C[3 * k], S.rad[k], S.shell[k], &cdir[k][3 * (size_t) cell], cth[k][cell], pt.q, pt.rho);
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
	const DirCones cones = gi_dir_cones();
	std::vector<uint32_t> masks(patches.size() * SKR_GI_ROW_ENTRIES, 0u);
	for(size_t pi = 0; pi < patches.size(); pi++)
	{
		const Patch &pt = patches[pi];
		uint32_t *row = &masks[pi * SKR_GI_ROW_ENTRIES];
		for(int k = 0; k < ns; k++)
			if(k != pt.s) gi_ball_bits(pt.q, pt.rho, &S.C[3 * k], S.r2[k], 1u << k, cones, row);
		// sphere s (leaves_own_sphere; the paddings are added in this order: another order can change a bit of a table): the origins
		// are the patch's own points, R_lo <= |o - C| <= R_hi
		const int s = pt.s;
		const SurfaceShell &sh = S.shell[s];
		const double E = sh.R_hi * (1.0 + 0x1p-20), behind = 0x1p-16 * E + 0x1p-30 * sh.R_hi;
		for(int e = 0; e < SKR_GI_ROW_ENTRIES; e++)
			if(!leaves_own_sphere(&cdir[s][3 * (size_t) pt.cell], &cones.dir[3 * (size_t) e], {cth[s][pt.cell], cones.theta[e]}, sh.R_lo, behind)) row[e] |= 1u << s;
	}
	// masks (rows gi_rows + pi), headers, index
	std::vector<uint32_t> table = pack_masks(masks, gi_wide != 0);
	const size_t n_mask_words = table.size();
	table.resize(n_mask_words + SKR_GI_SURFACE_HEAD * (size_t) ns + n_index, 0u);
	uint32_t *head = &table[n_mask_words];
	int32_t *index = reinterpret_cast<int32_t *>(head + SKR_GI_SURFACE_HEAD * ns);
	size_t at = SKR_GI_SURFACE_HEAD * (size_t) ns;
	for(int k = 0; k < ns; k++)
	{
		head[SKR_GI_SURFACE_HEAD * k] = (uint32_t) at;
		head[SKR_GI_SURFACE_HEAD * k + 1] = (uint32_t) G[k];
		const float t = G[k] ? S.shell[k].tau : -1.0f;
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
	const Spheres S(sph_geom);
	if(!S.in_range) return; // (the direction masks only)
	// the GI patches' edge, or what they would try first where the scene has none (triangles)
	double edge = gi_surface_edge > 0.0 ? gi_surface_edge : surface_first_edge(S, (double) SKR_GI_MAX_BYTES / (SKR_GI_ROW_ENTRIES * (ns > 16 ? 4 : 2)));
	edge /= SKR_SHADOW_SURFACE_SCALE;
	std::vector<int> G(ns, 0);
	size_t stride = 0;
	for(int attempt = 0; attempt < 200; attempt++, edge *= 1.15)
	{
		stride = 0;
		for(int k = 0; k < ns; k++)
		{
			G[k] = cells_per_edge(S.shell[k], S.rad[k], edge);
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
		const SurfaceShell &sh = S.shell[s];
		const double *Cs = &S.C[3 * s], cmax = max_abs3(Cs);
		const double eps_o = origin_offset_bound(cmax + sh.R_hi);
		const double R_in = sh.R_lo - eps_o;                       // |o - C_s| at least
		const double E_own = (sh.R_hi + eps_o) * (1.0 + 0x1p-20); // ... and at most
		const double behind_own = 0x1p-16 * E_own + 0x1p-30 * sh.R_hi;
		const double tilt = R_in > 0.0 ? std::asin(std::min(1.0, eps_o / sh.R_lo)) : 0.0; // the angle between o - C_s and P - C_s
		for(int cell = 0; cell < 6 * G[s] * G[s]; cell++)
		{
			const double *wp = &cdir[3 * (size_t) cell];
			double q[3], rho;
			surface_patch_ball(Cs, S.rad[s], sh, wp, cth[cell], q, rho);
			rho = (rho + eps_o) * rho_scale;
			for(int k = 0; k < ns; k++)
				if(k != s) bs[k] = ball_sphere(q, rho, &S.C[3 * k], S.r2[k]);
			for(int l = 0; l < nl; l++)
			{
				uint32_t &word = table[(size_t) (l >> 1) * stride + base + cell];
				const double lp[3] = {lights[2 * (size_t) l].x, lights[2 * (size_t) l].y, lights[2 * (size_t) l].z};
				const double d[3] = {lp[0] - q[0], lp[1] - q[1], lp[2] - q[2]};
				const double dl = len3(d);
				if(!(dl > rho * (1.0 + 0x1p-20) + 0x1p-30 * (cmax + S.rad[s])))
				{ // the light inside the ball: any direction
					word = all;
					continue;
				}
				const double w[3] = {d[0] / dl, d[1] / dl, d[2] / dl};
				const double theta = (std::asin(std::min(1.0, rho / dl)) * (1.0 + 0x1p-20) + eta) * cone_scale;
				const double ct = std::cos(theta), st = std::sin(theta);
				// every ray's line passes within near_l of Lp: |o - P|, and the error of L over the way to the light
				const double near_l = eps_o + eta * (dl + rho) * (1.0 + 0x1p-20);
				for(int k = 0; k < ns; k++)
				{
					if(k == s) continue;
					// the half-line rule from the patch's ball; the line rule from the light, where the lines (nearly) meet: the
					// distance from C to a line grows with the distance from Lp, not with the width of the patch
					const BallSphere &b = bs[k];
					const bool ahead = b.meets || cone_ahead(cone_sphere(b.v, b.dist, w, ct, st), b.dist, b.behind);
					const double vl[3] = {S.C[3 * k] - lp[0], S.C[3 * k + 1] - lp[1], S.C[3 * k + 2] - lp[2]};
					const double distl = len3(vl);
					const double reach_l = b.rk + near_l + 0x1p-30 * (distl + dl + b.rk);
					const bool line = distl <= reach_l || cone_line_touches(cone_sphere(vl, distl, w, ct, st), distl, reach_l);
					if(ahead && line) word |= 1u << k;
				}
				// sphere s (leaves_own_sphere; the paddings in this order, as above): the origins are o, within eps_o of the patch's
				// points, so o - C_s is tilted too
				if(!leaves_own_sphere(wp, w, {cth[cell], tilt, theta}, R_in, behind_own)) word |= 1u << s;
			}
		}
		base += (size_t) 6 * G[s] * G[s];
	}
	shadow_surface_stride = (uint32_t) stride;
	shadow_surface.swap(table);
	shadow_surface_head.swap(head);
}
