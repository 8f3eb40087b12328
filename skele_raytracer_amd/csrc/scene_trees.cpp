// The culling trees, built on the host in binary64: the Morton order finalize() stores the triangles in, the triangle chunk tree of
// the renderer and of the ray queries (skr_scene::build_triangle_chunks; shape in tri_chunks.h; DESIGN.md 5.5 "Triangles: exact
// conservative culling") and the sphere tree (skr_build_sphere_tree).  Every radius is conservative: a ray the
// device's binary32 test accepts is never culled.  No GPU code in this file.
#include "scene_host.h"

#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <cmath>
#include <functional>

namespace {

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

// a row of links: x a float or an int, y, z, w ints, all as their bits
template <class X> skr_f4 pack_row(X x, int32_t y, int32_t z, int32_t w)
{
	static_assert(sizeof(X) == 4, "one 32-bit word");
	skr_f4 v;
	memcpy(&v.x, &x, 4); memcpy(&v.y, &y, 4); memcpy(&v.z, &z, 4); memcpy(&v.w, &w, 4);
	return v;
}

// The ball every ray of a query may start in: around the box's centre, twice its half diagonal.
void scene_ball(const SkrBox &b, float ball[4])
{
	const double half = 0.5 * std::sqrt((b.hi[0] - b.lo[0]) * (b.hi[0] - b.lo[0]) + (b.hi[1] - b.lo[1]) * (b.hi[1] - b.lo[1]) + (b.hi[2] - b.lo[2]) * (b.hi[2] - b.lo[2]));
	for(int k = 0; k < 3; k++) ball[k] = (float) b.centre(k);
	ball[3] = (float) (2 * half + 1e-3);
}

float round_up_square(double r, bool infinite)
{
	const double r2 = r * r;
	float f = (float) r2;
	if((double) f < r2) f = std::nextafterf(f, INFINITY);
	if(infinite || !(r2 == r2)) f = INFINITY;
	return f;
}

} // namespace

// The triangle walk only answers "does any triangle accept this ray before tmin" (raytrace.h:168-176 turns
// any such hit black), so the order of tris[] is free: store the triangles along a Morton curve through the
// centres of their accept regions, which makes every run of tri_chunk_size triangles spatially tight.
std::vector<int> skr_triangle_order(const std::vector<float> &raw_triangles, int nt)
{
	std::vector<int> order(nt);
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
			code |= morton_spread((uint64_t) std::min(2097151.0, std::max(0.0, u * 2097151.0))) << k;
		}
		key[i] = ok ? code : ~0ull;
		order[i] = i;
	}
	std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
	return order;
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
	tri_chunk_size = info.n_spheres == 0 ? SKR_TRI_CHUNK_COHERENT : SKR_TRI_CHUNK_MIXED; // see tri_chunks.h
	if(const char *e = getenv("SKR_TRI_CHUNK")) // tuning runs only
		if(atoi(e) >= 1 && atoi(e) <= 64) tri_chunk_size = atoi(e);
	const double dmax[SKR_CULL_LEVELS] = SKR_CULL_DMAX_LIST;
	for(int level = 0; level < SKR_CULL_LEVELS; level++)
	{
		const SkrChunkLevel one = build_triangle_chunk_level(dmax[level]);
		if(level == 0) { tri_chunk_stride = one.rows.size(); tri_node_count = one.node_count; } // (the shape follows the triangle count alone: every set of both trees has it)
		tri_any_cone = tri_any_cone || one.any_cone;
		tri_chunks.insert(tri_chunks.end(), one.rows.begin(), one.rows.end());
	}
	// the ray queries' ball: around the bounding box of every point a renderer's ray can start at or hit, twice that box's half diagonal
	SkrBox box(info.camera[0], info.camera[1], info.camera[2]);
	for(int i = 0; i < info.n_spheres; i++)
	{
		const float *s = &raw_spheres[(size_t) i * 14];
		box.grow(s[0], s[1], s[2], std::fabs((double) s[3]));
	}
	for(int i = 0; i < info.n_triangles; i++)
	{ // the accept region (v0, v0 - e1, v0 + e2)
		const skr_f4 v0 = tris[3 * i], e1 = tris[3 * i + 1], e2 = tris[3 * i + 2];
		box.grow(v0.x, v0.y, v0.z, 0);
		box.grow((double) v0.x - e1.x, (double) v0.y - e1.y, (double) v0.z - e1.z, 0);
		box.grow((double) v0.x + e2.x, (double) v0.y + e2.y, (double) v0.z + e2.z, 0);
	}
	scene_ball(box, trace_ball);
	// the device tests fl(|o - c|^2) <= fl(r)^2 against the float centre: the tree is built for a ball wider by far more than that rounding
	const double ball[4] = {trace_ball[0], trace_ball[1], trace_ball[2], (double) trace_ball[3] * 1.001 + 1e-3};
	trace_chunks.clear();
	trace_any_cone = false;
	for(int level = 0; level < SKR_CULL_LEVELS; level++)
	{
		const SkrChunkLevel one = build_triangle_chunk_level(dmax[level], ball);
		trace_any_cone = trace_any_cone || one.any_cone;
		trace_chunks.insert(trace_chunks.end(), one.rows.begin(), one.rows.end());
	}
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

SkrChunkLevel skr_scene::build_triangle_chunk_level(double d_max, const double *origin_ball) const
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
	SkrChunkLevel out;
	std::vector<skr_f4> &nodes = out.rows;
	std::function<void(int, size_t)> emit = [&](int level, size_t idx) { // depth-first: a node, then its subtree
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
			for(size_t c = c0; c < c1; c++) emit(level - 1, c);
		}
		nodes[me + 2] = pack_row((int32_t) (nodes.size() / 3), first, count, level);
	};
	emit((int) levels.size() - 1, 0);
	// one pad node so that the walk may prefetch past the end, then the chunk entries (+ a pad entry)
	out.node_count = (int) (nodes.size() / 3);
	nodes.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	nodes.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	nodes.push_back(pack_row(out.node_count + 1, 0, 0, 0));
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
	out.any_cone = 4 * with_cone >= levels[0].size();
	nodes.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	nodes.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	return out;
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
	SkrBox box;
	for(size_t i = i0; i < i1; i++) box.grow(rows[i].x, rows[i].y, rows[i].z, std::sqrt((double) rows[i].w));
	SphereBound b{0, 0, 0, 0, 0, false};
	// the centre is the float the device reads: every distance below is taken from it
	b.x = (double) (float) box.centre(0);
	b.y = (double) (float) box.centre(1);
	b.z = (double) (float) box.centre(2);
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
} // namespace

void skr_build_sphere_tree(const skr_scene &sc, SkrSphereTree &t)
{
	t = SkrSphereTree();
	const size_t n = sc.sph_geom.size();
	// the ball: around the bounding box of the camera, the spheres and the mesh, twice that box's half diagonal (as the trace tree's)
	SkrBox box(sc.info.camera[0], sc.info.camera[1], sc.info.camera[2]);
	for(size_t i = 0; i < n; i++) box.grow(sc.sph_geom[i].x, sc.sph_geom[i].y, sc.sph_geom[i].z, std::sqrt((double) sc.sph_geom[i].w));
	for(size_t i = 0; i + 2 < sc.raw_triangles.size(); i += 3) box.grow(sc.raw_triangles[i], sc.raw_triangles[i + 1], sc.raw_triangles[i + 2], 0);
	scene_ball(box, t.ball);
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
		SkrBox cb;
		for(int32_t i : rest) cb.grow(sc.sph_geom[i].x, sc.sph_geom[i].y, sc.sph_geom[i].z, 0);
		const double *clo = cb.lo;
		const double ext = std::max(cb.hi[0] - clo[0], std::max(cb.hi[1] - clo[1], cb.hi[2] - clo[2]));
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
	std::function<void(int, size_t)> emit = [&](int level, size_t idx) { // depth-first: a node, then its subtree
		const size_t me = t.nodes.size();
		const Ent &e = levels[level][idx];
		t.nodes.push_back(e.A);
		t.nodes.push_back({0, 0, 0, 0});
		int32_t fc = -1; // first chunk of a node of height 1 (it has the next SKR_SPHERE_SUPER chunks, or those that are left), else -1
		if(level == 1) fc = t.n_always + (int32_t) idx * SKR_SPHERE_SUPER; // (the regular chunks follow the always-tested ones)
		else
		{
			const size_t c0 = idx * SKR_SPHERE_SUPER, c1 = std::min(levels[level - 1].size(), c0 + SKR_SPHERE_SUPER);
			for(size_t c = c0; c < c1; c++) emit(level - 1, c);
		}
		t.nodes[me + 1] = pack_row(e.kappa, (int32_t) (t.nodes.size() / 2), fc, e.min_index);
	};
	if(levels.size() > 1) emit((int) levels.size() - 1, 0);
	t.n_nodes = (int) (t.nodes.size() / 2);
	t.nodes.push_back({0.0f, 0.0f, 0.0f, INFINITY});
	t.nodes.push_back(pack_row(0.0f, t.n_nodes + 1, -1, INT32_MAX));
}
