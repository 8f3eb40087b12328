// Device functions shared by the render kernels: scene view, traversal,
// shading (reference src/raytrace.h, blinn_phong.h, utils.h restated for gfx950).
#pragma once

#include "device_math.h"
#include "render_params.h"
#include "shadow_cells.h"
#include "tri_chunks.h"

namespace {


// Scene as the kernel sees it: pointers into LDS (spheres, materials, lights)
// and HBM (triangles, read with wave-uniform addresses).
struct SceneView {
	const float4 *geom; // LDS  centre.xyz, r*r; ns + 1 entries (the last is a pad for the loops' prefetch)
	const float4 *amb;  // LDS  La*ka, .w = phong power
	const float4 *kd;   // LDS
	const float4 *ks;   // LDS
	const float4 *lights; // LDS [2i] position [2i+1] colour
	const float4 *tris; // HBM  [3i] v0 [3i+1] e1 [3i+2] e2
	int ns, nt, nl;
	const float4 *chunks; // HBM  culling data of the triangle walk (scene_host.h): the skip-linked tree, 2 float4 per node,
	                      //      + a pad node, then one conservative sphere (centre, radius^2) per chunk of triangles
	int nchunks;          // nodes in the tree; 0 = walk every triangle
	int chunk;            // triangles per chunk sphere (tri_chunks.h)
	int cones;            // some entry carries a tight radius for non-grazing rays
	unsigned long long *tri_work; // HBM, or null (not counting): SKR_TRI_WORK_SHARDS x {culling-sphere tests, triangle tests} the walks executed (lanes that needed them)
	const float4 *geom_u; // HBM: the same rows as `geom`, for the loops that walk the spheres in order with a wave-uniform index (sphere_rows)
	const uint32_t *smask; // HBM, or null: the shadow masks (RenderParams::shadow_masks; shadow_mask_of)
	float smask_reach2;
	uint32_t smask_all;
};
typedef float skr_v4f __attribute__((ext_vector_type(4)));

// ---- the shape of a launch, compiled in (DESIGN.md 5.2 "Launch shapes") ----
// Facts of a launch that are the same for every lane of every wave: how many lights, whether shadow rays are cast, how long the
// straight-line pow is, how wide a GI mask is.  Read from RenderParams / SceneView each of them holds a scalar register from the kernel's
// entry to its last use — the leaf kernel has more of those than registers, and a spilled one comes back through v_readlane_b32, a VALU
// slot — and costs the wave-uniform branch or loop counter that depends on it.  As constants of a type passed down the shading and
// tracing call tree as a template argument (as SS / TS of direct_light_of are) they cost neither.  RunTimeShape reads every fact where it
// was always read: the code of an instance on it is the code it had without the parameter.  The launcher picks a fixed shape only for a
// launch whose every fact equals the constant (launch.h skr_leaf_shape).
} // namespace
// (types with external linkage: a kernel instance names its shape)
struct RunTimeShape {
	static constexpr int lights = 0;             // 0: sv.nl lights of any kind
	static constexpr bool point_lights = false;  // true: no directional light (light_term)
	static constexpr bool shadows = false;       // true: p.use_shadows != 0
	static constexpr bool masks = false;         // true: the launch has shadow masks (sv.smask != null)
	static constexpr bool pow7 = false;          // true: p.pow_steps <= 7
	static constexpr unsigned pow_any = SKR_POW_FULL7; // (pow7) every integer Phong exponent of the scene lies inside this mask of bits
	static constexpr bool gi_narrow = false;     // true: p.gi_wide == 0 (16-bit GI masks: at most 16 spheres)
};
// A sphere-only scene of LIGHTS (1 or 2) point lights with its shadow masks, shadows on, integer Phong exponents below 128 — all of them
// inside the bits of ANY (device_math.h pow_int_sparse; 0x7F: any of them) — and at most 16 spheres.
template <int LIGHTS, unsigned ANY = SKR_POW_FULL7>
struct PointLightShape {
	static constexpr int lights = LIGHTS;
	static constexpr bool point_lights = true, shadows = true, masks = true, pow7 = true, gi_narrow = true;
	static constexpr unsigned pow_any = ANY;
};
namespace {

// One aligned 16-byte row of a table that no kernel writes, at a wave-uniform index, through the constant address space: that is what
// makes the compiler take the scalar path (s_load_dwordx4 into SGPRs) — through a plain pointer it cannot prove that no store of the
// kernel aliases the row and issues a vector load with a uniform address.
SKR_DEV float4 load_const4(const float4 *base, int i)
{
	const skr_v4f __attribute__((address_space(4))) *q = (const skr_v4f __attribute__((address_space(4))) *) (unsigned long long) base;
	const skr_v4f v = q[i];
	return make_float4(v.x, v.y, v.z, v.w);
}

// ---- where a sphere is during a sample (include/skr.h skr_scene_set_sphere_velocities) ----
// The centre policy of the sphere searches: `row(g, i)` is the row {centre, r^2} of sphere i as a search tests it, g the row at rest.
// AtRest is the scene as it lies — no code, as NoTriangleShadows and SphereLoopShadows are none — and what every instance without a
// Motion in its pack is compiled with.  MovingCentres is the sample at shutter time tau of the lane: c' = fma(tau, v_i, c_i), one
// correctly rounded fused multiply-add per component (the stated exception to "not contracted"), r^2 unchanged.  The velocity rows
// {v.xyz, 0} are the renderer's own allocation (launch.h Motion), read through the constant address space: at the wave-uniform index of a
// sphere loop one scalar load beside the sphere row's, at a lane's own index (the normal of a hit) a vector load.
struct AtRest {
	static constexpr bool moving = false;
	__device__ __forceinline__ float4 row(float4 g, int) const { return g; }
};
struct MovingCentres {
	static constexpr bool moving = true;
	const float4 *vel;
	float tau;
	static __device__ __forceinline__ float4 centre(float4 g, float4 v, float tau)
	{
		return make_float4(__builtin_fmaf(tau, v.x, g.x), __builtin_fmaf(tau, v.y, g.y), __builtin_fmaf(tau, v.z, g.z), g.w);
	}
	__device__ __forceinline__ float4 row(float4 g, int i) const { return centre(g, load_const4(vel, i), tau); }
};

// The sphere loops of the level pipelines (closest_pair_deferred, occluded_pair<false>): `test(row, index)` for every sphere in order,
// SKR_SPHERE_TRIP spheres per trip, the rows of the next trip asked for a trip ahead with ONE scalar load (s_load_dwordx8 / x16: the rows
// are consecutive).  The rows come through the scalar cache into SGPRs (geom_u), so the spheres in flight cost no vector register for
// their data — and several independent tests per trip are what a SIMD with four waves wants.  Headline leaf kernel, same box, spheres
// per trip 1 / 2 / 3 / 4 / 5 / 6 / 8: 1.240 / 1.205 / 1.207 / 1.19 / 1.240 / 1.224 / 1.282 ms (LDS rows, one per trip: 1.25; LDS rows,
// two per trip: 1.35 — the second sphere's registers spill; scalar rows fetched one by one with a bounds test each: 1.25).  The lanes of
// these kernels are incoherent; the direct kernel's coherent loops keep LDS rows and their wave-wide early exit.
#ifndef SKR_SPHERE_TRIP
#define SKR_SPHERE_TRIP 4
#endif
template <int K, typename F, typename G>
SKR_DEV void table_rows(const float4 *base, int n, F test, G go_on)
{
	auto row = [&](int i) { return load_const4(base, i); }; // (up to 2 K - 1 rows behind the table are asked for and never used: the tables are padded for them, api.cpp)
	float4 nx[K];
#pragma unroll
	for(int k = 0; k < K; k++) nx[k] = row(k);
	int i = 0;
	for(; i + K <= n; i += K)
	{
		float4 g[K];
#pragma unroll
		for(int k = 0; k < K; k++)
		{
			g[k] = nx[k];
			nx[k] = row(i + K + k);
		}
		__builtin_amdgcn_sched_barrier(0); // the next trip's rows are asked for here, a whole trip ahead of their use
#pragma unroll
		for(int k = 0; k < K; k++) test(g[k], i + k);
		if(!go_on()) return;
	}
#pragma unroll
	for(int k = 0; k < K - 1; k++)
		if(i + k < n) test(nx[k], i + k);
}
template <typename F>
SKR_DEV void sphere_rows(const SceneView &sv, F test)
{
	table_rows<SKR_SPHERE_TRIP>(sv.geom_u, sv.ns, test, [] { return true; });
}
// `test(row, index)` for the spheres a lane's candidate mask names, lowest index first (the lanes' rows differ: LDS)
template <typename F>
SKR_DEV void masked_rows(const SceneView &sv, uint32_t cand, F test)
{
	uint32_t rest = cand;
	while(rest)
	{
		const int i = __builtin_ctz(rest);
		test(sv.geom[i], i);
		rest &= rest - 1u;
	}
}

// Row i of the mesh tables (triangles, culling data: HBM, never written by a kernel), i wave-uniform: one s_load_dwordx4 into SGPRs.
// Through the plain pointer the compiler issues a VECTOR load with a uniform address (it cannot prove that no store of the kernel
// aliases the table): 26 M vector-memory instructions per dragon frame, found in the round-3 counters (SQ_INSTS_VMEM against
// SQ_INSTS_SMEM = 0.5 M) under a comment that said "scalar loads".  Through the constant address space: dragon.scn 1080p 1.306 ->
// 1.18 ms, with --shade-triangles 2.99 -> 2.10 ms; test.scn 640x360 --gillum 4 (a dozen triangles, incoherent lanes) 1.10 -> 1.16 ms.
#ifndef SKR_MESH_SMEM
#define SKR_MESH_SMEM 1
#endif
SKR_DEV float4 mesh_row(const float4 *base, int i)
{
#if SKR_MESH_SMEM
	return load_const4(base, i);
#else
	return base[i];
#endif
}

// What a triangle walk executed, counted per wave on the scalar unit (population counts of lane masks the walk forms anyway) and added
// to one of SKR_TRI_WORK_SHARDS words by one lane when the walk ends: bench.py's FP32-VALU figure for mesh scenes is built from
// these counts, not from the 10 002 tests per ray the reference's loop runs (raytrace.h:171-186).
#define SKR_TRI_WORK_SHARDS 256u
SKR_DEV void tri_work_add(const SceneView &sv, uint32_t n_cull, uint32_t n_tri)
{
	if(sv.tri_work && (n_cull | n_tri))
	{
		const unsigned long long m = __ballot(true);
		if(__builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u)) == 0)
		{
			unsigned long long *w = sv.tri_work + 2u * ((blockIdx.x * 4u + (threadIdx.x >> 6)) & (SKR_TRI_WORK_SHARDS - 1u));
			atomicAdd(&w[0], (unsigned long long) n_cull);
			atomicAdd(&w[1], (unsigned long long) n_tri);
		}
	}
}

struct Counters {
	uint32_t rays, hits, shadow_rays;
	uint32_t shadow_tests; // ray-sphere tests of utils.h:42-58 as the reference runs them: up to and including the first occluder
};

struct RayConst { // per-ray invariants of utils.h:113-121
	f3 o, d;
	float two_a, four_a;
};

SKR_DEV RayConst make_ray(f3 o, f3 d)
{
	const float a = dot3(d, d);
	return RayConst{o, d, 2 * a, 4 * a};
}

// raytrace.h:152-165: closest accepted sphere (strict <, first index wins ties),
// evaluated exactly as written: the binary64 root for every sphere with D >= 0.
template <typename M = AtRest>
SKR_DEV int closest_sphere_exact(const SceneView &sv, const RayConst &r, float &tmin, const M &m = M())
{
	int best = -1;
	tmin = __builtin_inff();
	float4 g_next = sv.geom[0];
	for(int i = 0; i < sv.ns; i++)
	{
		const float4 g = m.row(g_next, i);
		g_next = sv.geom[i + 1]; // software prefetch; geom[] carries one pad entry
		const float t = sphere_distance(r.o, r.d, r.two_a, r.four_a, g);
		if(accept_distance(t) && t < tmin)
		{
			tmin = t;
			best = i;
		}
	}
	return best;
}

// Same result through the binary32 brackets of device_math.h: the winner is
// known as soon as its bracket lies strictly below every other accepted
// sphere's; its exact t2 is then formed once.  Overlapping brackets (two
// surfaces within ~1e-6 relative of each other along the ray) fall back to the
// exact loop for that lane.  The rows of `table`, K per trip; `bracket(row, f, lo, hi, b, D)` is the test of one row.  M: where the
// spheres are (AtRest, MovingCentres; sphere rows only).
template <int K, typename B, typename M = AtRest>
SKR_DEV int closest_of_rows(const SceneView &sv, const float4 *table, const RayConst &r, float &tmin, B bracket, const M &m = M())
{
	const RayFilt f = make_filt(r.d);
	int best = -1;
	float best_lo = __builtin_inff(), best_hi = __builtin_inff(), others_lo = __builtin_inff();
	float best_b = 0.0f, best_D = 0.0f;
	table_rows<K>(table, sv.ns, [&](const float4 row, int i)
	{
		float lo, hi, b, D;
		if(bracket(m.row(row, i), f, lo, hi, b, D)) best_update(best_hi, others_lo, best_lo, best, best_b, best_D, i, lo, hi, b, D);
	}, [] { return true; });
	tmin = __builtin_inff();
	if(best >= 0)
	{
		if(others_lo > best_hi) tmin = bracket_t(f.two_a, best_lo, best_hi, best_b, best_D);
		else best = closest_sphere_exact(sv, r, tmin, m);
	}
	return best;
}
template <typename M = AtRest>
SKR_DEV int closest_sphere(const SceneView &sv, const RayConst &r, float &tmin, const M &m = M())
{
	return closest_of_rows<SKR_SPHERE_TRIP>(sv, sv.geom_u, r, tmin, // (the rows of sphere_rows)
		[&](const float4 g, const RayFilt &f, float &lo, float &hi, float &b, float &D) { return sphere_bracket(r.o, r.d, f, g, lo, hi, b, D); }, m);
}

// closest_sphere() for rays that all start at ONE point (the camera: main.cpp:140-182), with e = o - C and c = e.e - r^2 of utils.h:115-118
// formed once per sphere and renderer (ec[i] = {e.xyz, c}: the same subtractions, products and sums in the same order, on the device, so the
// same floats: skr_camec_kernel, render_wave.hip) instead of once per ray: 9 of the ~17 instructions a sphere costs a ray.  The rows are
// read like the sphere rows of the level pipelines: scalar loads, several per trip (table_rows).
SKR_DEV float4 camec_row(float4 g, f3 o)
{ // row i of the ec table of rays that start at o (skr_camec_kernel; the debug ops of render_kernel.hip)
	const f3 e = o - ld3(g);
	return make_float4(e.x, e.y, e.z, dot3(e, e) - g.w);
}
#ifndef SKR_CAMERA_TRIP
#define SKR_CAMERA_TRIP 4 // spheres per trip of closest_sphere_from: config 2 (15 spheres) 1.312 / 1.284 / 1.19 ms at 1 / 2 / 4 (with the shadow loop at the same count), bear.scn (31) 0.518 / 0.500 / 0.451
#endif
SKR_DEV int closest_sphere_from(const SceneView &sv, const float4 *ec, const RayConst &r, float &tmin)
{
	return closest_of_rows<SKR_CAMERA_TRIP>(sv, ec, r, tmin,
		[&](const float4 q, const RayFilt &f, float &lo, float &hi, float &b, float &D) { return bracket_from_ec(ld3(q), q.w, r.d, f, lo, hi, b, D); });
}

// closest_pair_deferred's end for one slot: where the brackets overlap the exact loop names the winner, and its b, D are formed again
// (b, D and not t: classify_child, render_nodes.hip, forms t only on mesh scenes).
SKR_DEV void best_resolve(const SceneView &sv, f3 o, f3 d, float four_a, BestState &s)
{
	if(s.best >= 0 && !(s.others_lo > s.hi))
	{
		DIAG_WAVE(8, 1);
		float tmin;
		const RayConst r = make_ray(o, d);
		s.best = closest_sphere_exact(sv, r, tmin);
		const f3 e = o - ld3(sv.geom[s.best]);
		s.b = 2 * dot3(d, e);
		const float c = dot3(e, e) - sv.geom[s.best].w;
		s.D = s.b * s.b - four_a * c;
	}
}

// The line part of the culling tests (scene_trees.cpp build_triangle_chunks), for an entry A = {centre, R^2}, B = {axis / kappa,
// R_tight^2}: e = C - o, |e x d|^2 and R^2 |d|^2.  A ray that is not grazing for the entry's (nearly coplanar) triangles,
// (d . axis / kappa)^2 >= d . d, is held to the tight radius.
struct LinePart {
	f3 e;
	float cr2, lim;
};
template <bool CONES>
SKR_DEV LinePart line_part(const RayConst &r, float dd, float4 A, float4 B)
{
	const f3 e = ld3(A) - r.o;
	const f3 cr = cross3(e, r.d);
	float R2 = A.w;
	if constexpr(CONES)
	{
		const float gb = dot3(r.d, ld3(B));
		R2 = (gb * gb >= dd) ? B.w : A.w;
	}
	return LinePart{e, dot3(cr, cr), R2 * dd};
}

// The conservative line-sphere test of the culling data: false only where no triangle below the entry can accept this lane's line,
// |e x d|^2 > R^2 |d|^2.  NaN anywhere => true.
template <bool CONES>
SKR_DEV bool line_touches(const RayConst &r, float dd, float4 A, float4 B)
{
	const LinePart p = line_part<CONES>(r, dd, A, B);
	return !(p.cr2 > p.lim);
}

// lanes x rays of a mask of up to two rays per lane (wave-uniform: scalar registers)
SKR_DEV uint32_t lanes_of(uint32_t mask) { return (uint32_t) __popcll(__ballot((mask & 1u) != 0u)) + (uint32_t) __popcll(__ballot((mask & 2u) != 0u)); }

// The instance of a mesh walk a scene view asks for: f(cones, count) with the types of two compile-time flags — the entries' tight
// radii are tested (sv.cones), the walk counts its work (counting costs the dragon walk 19 %: the counting instances run only while
// sv.tri_work is set — skr_renderer_count_triangle_work).
template <bool V>
struct Flag {
	static constexpr bool value = V;
};
template <typename F>
SKR_DEV void mesh_instance(const SceneView &sv, F f)
{
	if(__builtin_expect(sv.tri_work != nullptr, 0))
	{
		if(sv.cones) f(Flag<true>{}, Flag<true>{});
		else f(Flag<false>{}, Flag<true>{});
	}
	else if(sv.cones) f(Flag<true>{}, Flag<false>{});
	else f(Flag<false>{}, Flag<false>{});
}

// The walk over the triangle tree `sv.chunks` (sv.nchunks > 0 nodes).  A line that misses a conservative sphere cannot pass the test
// for any triangle below it, so a node or chunk that no lane wants is skipped whole.  The levels above the chunks are stored
// depth-first with skip links: one wave-uniform index, no stack, rows through the scalar cache (mesh_row); both successors of a node
// are fetched while its sphere is tested.  The chunk entries of a height-1 node are contiguous: a tight loop, entries and triangles
// loaded where they are used (asked for one ahead, the walks of any_triangle_closer and shadow_triangles were the slower ones: dragon
// 0.915 against 0.860 ms, the shadowed dragon 14.4 against 13.1 ms; 20 scalar registers less).  `live()` = the rays of the lane (a bit
// each, or a bool) that still want tests; `touch(A, B)` = those of them that want this entry: an entry is entered when any lane wants
// it, and `tri(v0, e1, e2, slot, mine)` sees every triangle of a chunk some lane wants, as its three rows, with the bits of its own
// lane.  The wave leaves after a height-1 node once no lane is live.  Counted: an entry per live ray that it is tested for, a
// triangle per ray that is live and wants its chunk.
// Reads past the end: only the successors of the last node, which are the pad node behind the nodes of every set of both trees
// (scene_trees.cpp build_triangle_chunk_level), at every bound on |d|.
template <bool COUNT, typename V, typename T, typename S>
SKR_DEV void mesh_walk(const SceneView &sv, V live, T touch, S tri)
{
	int i = 0;
	uint32_t n_cull = 0, n_tri = 0; // (wave-uniform: scalar registers)
	const float4 *chunk_ent = sv.chunks + 3 * (sv.nchunks + 1); // behind the nodes and their pad
	float4 A = mesh_row(sv.chunks, 0), B = mesh_row(sv.chunks, 1), lk = mesh_row(sv.chunks, 2);
	while(i < sv.nchunks)
	{
		const int i_out = __float_as_int(lk.x);
		// first child (or the next node after a height-1 node) and next sibling (padded past the end)
		const float4 A_in = mesh_row(sv.chunks, 3 * i + 3), B_in = mesh_row(sv.chunks, 3 * i + 4), lk_in = mesh_row(sv.chunks, 3 * i + 5);
		const float4 A_out = mesh_row(sv.chunks, 3 * i_out), B_out = mesh_row(sv.chunks, 3 * i_out + 1), lk_out = mesh_row(sv.chunks, 3 * i_out + 2);
		if(COUNT) n_cull += lanes_of(live());
		const bool enter = __any(touch(A, B) != 0);
		const int count = __float_as_int(lk.z);
		if(enter && count > 0)
		{ // height 1: its chunk entries are contiguous
			const int c0 = __float_as_int(lk.y), c1 = c0 + count;
			for(int c = c0; c < c1; c++)
			{
				const float4 cA = mesh_row(chunk_ent, 2 * c), cB = mesh_row(chunk_ent, 2 * c + 1);
				if(COUNT) n_cull += lanes_of(live());
				const auto mine = touch(cA, cB);
				if(__any(mine != 0))
				{
					const int i0 = c * sv.chunk, i1 = (i0 + sv.chunk < sv.nt) ? i0 + sv.chunk : sv.nt;
					// (one triangle per scalar-cache round trip; a whole 4-triangle chunk asked for at once was measured
					// slower: dragon 1.19 -> 1.27 ms, 48 more SGPRs live)
					for(int k = i0; k < i1; k++)
					{
						const float4 v0 = mesh_row(sv.tris, 3 * k), e1 = mesh_row(sv.tris, 3 * k + 1), e2 = mesh_row(sv.tris, 3 * k + 2);
						if(COUNT) n_tri += lanes_of(mine & live());
						tri(v0, e1, e2, k, mine);
					}
				}
			}
			if(!__any(live() != 0)) break;
		}
		i = enter ? i + 1 : i_out;
		A = enter ? A_in : A_out;
		B = enter ? B_in : B_out;
		lk = enter ? lk_in : lk_out;
	}
	if(COUNT) tri_work_add(sv, n_cull, n_tri);
}

// mesh_walk() where the wave has no tree (sv.nchunks == 0: SKR_NO_CULL, directions longer than the bounds were built for, a query ray
// that starts outside the tree's ball): `tri` sees every triangle with the lane's live rays.  Triangle k + 1 is fetched while k is
// tested (tris[] carries one pad triangle so the prefetch needs no bounds test); the wave looks every eighth triangle whether a lane
// is still live.  The tests are counted while sv.tri_work is set.
template <typename V, typename S>
SKR_DEV void mesh_all(const SceneView &sv, V live, S tri)
{
	uint32_t n_tri = 0;
	float4 n0 = mesh_row(sv.tris, 0), n1 = mesh_row(sv.tris, 1), n2 = mesh_row(sv.tris, 2);
	for(int k = 0; k < sv.nt; k++)
	{
		const float4 v0 = n0, e1 = n1, e2 = n2;
		n0 = mesh_row(sv.tris, 3 * k + 3);
		n1 = mesh_row(sv.tris, 3 * k + 4);
		n2 = mesh_row(sv.tris, 3 * k + 5);
		if(sv.tri_work) n_tri += lanes_of(live());
		tri(v0, e1, e2, k, live());
		if((k & 7) == 7 && !__any(live() != 0)) break;
	}
	tri_work_add(sv, 0u, n_tri);
}

// raytrace.h:171-186.  The outcome is binary: once a triangle passes with
// t < min_distance the sample is black (:221-224) whatever comes later, so a
// lane stops testing at its first accepted triangle and the wave leaves the
// walk when every active lane has.  (No t > 0 test: the reference has none.)
SKR_DEV bool any_triangle_closer(const SceneView &sv, const RayConst &r, float tmin)
{
	bool hit = false;
	const float dd = r.two_a * 0.5f; // dot(d, d)
	auto live = [&] { return !hit; };
	auto tri = [&](const float4 v0, const float4 e1, const float4 e2, int, bool mine)
	{
		float t;
		if(mine && !hit && triangle_hit(r.o, r.d, ld3(v0), ld3(e1), ld3(e2), t) && t < tmin) hit = true;
	};
	if(sv.nchunks > 0)
		mesh_instance(sv, [&](auto cones, auto count)
		{
			constexpr bool CONES = decltype(cones)::value;
			mesh_walk<decltype(count)::value>(sv, live, [&](const float4 A, const float4 B) { return !hit && line_touches<CONES>(r, dd, A, B); }, tri);
		});
	else mesh_all(sv, live, tri);
	return hit;
}

// The cell (face, i, j) of direction v in a cube map of N x N cells per face (shadow_cells.h addressing), in bounds whatever v holds
// (NaN -> 0).
struct CubeCell {
	int face, i, j;
};
SKR_DEV CubeCell cube_cell_n(f3 v, int N)
{
	const float ax = __builtin_fabsf(v.x), ay = __builtin_fabsf(v.y), az = __builtin_fabsf(v.z);
	const bool fx = (ax >= ay) && (ax >= az), fy = !fx && (ay >= az);
	const float m = fx ? ax : (fy ? ay : az), lead = fx ? v.x : (fy ? v.y : v.z);
	const float a = fx ? v.y : v.x, b = fy || fx ? v.z : v.y;
	const int face = (fx ? 0 : (fy ? 2 : 4)) + (lead < 0.0f ? 1 : 0);
	const float inv = __builtin_amdgcn_rcpf(m), h = 0.5f * (float) N, top = (float) (N - 1);
	const int i = (int) __builtin_fminf(__builtin_fmaxf((a * inv) * h + h, 0.0f), top); // (NaN -> 0)
	const int j = (int) __builtin_fminf(__builtin_fmaxf((b * inv) * h + h, 0.0f), top);
	return CubeCell{face, i, j};
}
template <int N>
SKR_DEV CubeCell cube_cell(f3 v)
{
	return cube_cell_n(v, N);
}

// The spheres that may stop the shadow ray of point light l from P (v = Lp - P, the subtraction light_term makes): the cell of v's
// direction in the light's table (shadow_cells.h; DESIGN.md "Shadow masks").  A lane whose P lies beyond the reach the table was built
// for, or whose v is not a vector of normal length (zero, NaN, inf), gets every sphere.  The index is in bounds whatever v holds.
SKR_DEV uint32_t shadow_mask_of(const SceneView &sv, int l, f3 v)
{
	const float vv = sqr3(v);
	const bool ok = (vv <= sv.smask_reach2) && (vv >= 0x1p-98f);
	const CubeCell c = cube_cell<SKR_SHADOW_CELLS>(v);
	const uint32_t mask = sv.smask[(l * 6 + c.face) * (SKR_SHADOW_CELLS * SKR_SHADOW_CELLS) + c.i * SKR_SHADOW_CELLS + c.j];
	return ok ? mask : sv.smask_all;
}

// ---- GI masks (shadow_cells.h; DESIGN.md "GI masks"): the spheres a GI child ray may have as candidates ----
// The row of masks of origin o: its cell in the fine grid, else in the coarse one; -1 = none (outside both, or not finite).  Only a lane
// inside a grid reads its index word.
SKR_DEV int gi_grid_cell(const int32_t *index, const SkrGiGrid &g, f3 o)
{
	const float fx = (o.x - g.lo[0]) * g.inv, fy = (o.y - g.lo[1]) * g.inv, fz = (o.z - g.lo[2]) * g.inv;
	const bool in = (fx >= 0.0f) && (fx < g.n_f[0]) && (fy >= 0.0f) && (fy < g.n_f[1]) && (fz >= 0.0f) && (fz < g.n_f[2]); // (NaN: out)
	int row = -1;
	if(in) row = index[g.base + ((int) fz * g.n[1] + (int) fy) * g.n[0] + (int) fx];
	return row;
}
SKR_DEV int gi_origin_row(const RenderParams &p, f3 o)
{
	int row = gi_grid_cell(p.gi_index, p.gi_grid[0], o);
	if(row < 0) row = gi_grid_cell(p.gi_index, p.gi_grid[1], o); // (the coarse grid only where the fine one has no row)
	return row;
}
// The row of masks of GI origin o, a hit point of sphere s (DESIGN.md "GI surface patches"): the patch of e = o - C_s on sphere s,
// where fl(|e|^2) - r_s^2 is within the sphere's radial slack and the patch is stored; else the grids' row (gi_origin_row).  s
// outside [0, ns) (the sphere is not known) or no patches (SKR_GI_SURFACE=0): the grids' row.  The index is in bounds whatever o holds.
SKR_DEV int gi_surface_row(const RenderParams &p, const SceneView &sv, int s, f3 o)
{
	int row = -1;
	if(p.gi_surface != nullptr && (uint32_t) s < (uint32_t) sv.ns)
	{
		const uint32_t *h = p.gi_surface + SKR_GI_SURFACE_HEAD * s;
		const uint32_t at = h[0], n = h[1];
		const float4 g = sv.geom[s];
		const f3 e = o - ld3(g);
		const float c = dot3(e, e) - g.w;
		if(__builtin_fabsf(c) <= __uint_as_float(h[2])) // (NaN: no; a sphere without patches has a negative slack)
		{
			const CubeCell cc = cube_cell_n(e, (int) n);
			row = (int) p.gi_surface[at + ((uint32_t) cc.face * n + (uint32_t) cc.i) * n + (uint32_t) cc.j];
		}
	}
	if(row < 0) row = gi_origin_row(p, o);
	return row;
}
// The union of the masks of children d0 and (second) d1 from origin row `row`; every sphere where the row is -1 or a direction is not a
// vector of moderate length (zero, tiny, huge, NaN, inf: the margins are derived for |d|^2 in [2^-40, 2^40]).
template <typename SH = RunTimeShape>
SKR_DEV uint32_t gi_cands(const RenderParams &p, int row, f3 d0, f3 d1, bool second)
{
	const float a0 = sqr3(d0), a1 = sqr3(d1);
	const bool ok = (row >= 0) && (a0 >= 0x1p-40f) && (a0 <= 0x1p40f) && (!second || ((a1 >= 0x1p-40f) && (a1 <= 0x1p40f)));
	const uint32_t base = ok ? (uint32_t) row * SKR_GI_ROW_ENTRIES : 0u;
	const CubeCell c0 = cube_cell<SKR_GI_DIR_CELLS>(d0), c1 = cube_cell<SKR_GI_DIR_CELLS>(d1);
	const uint32_t e0 = base + (uint32_t) ((c0.face * SKR_GI_DIR_CELLS + c0.i) * SKR_GI_DIR_CELLS + c0.j);
	const uint32_t e1 = base + (uint32_t) ((c1.face * SKR_GI_DIR_CELLS + c1.i) * SKR_GI_DIR_CELLS + c1.j);
	const uint16_t *m16 = reinterpret_cast<const uint16_t *>(p.gi_masks);
	const bool wide = !SH::gi_narrow && p.gi_wide;
	uint32_t m = wide ? p.gi_masks[e0] : (uint32_t) m16[e0];
	if(second) m |= wide ? p.gi_masks[e1] : (uint32_t) m16[e1]; // (no second child: no second load)
	return ok ? m : p.gi_all;
}

// utils.h:42-58: any sphere with 1 < t < inf along the (unbounded) shadow ray; two lights at a
// time, because both shadow rays start at the same point and share e and c per sphere.
// COHERENT: the lanes of the wave are neighbouring pixels (the direct kernel's 8x8 tiles), where a whole wave in one shadow is common
// and the loop is left once every lane's rays are occluded.  The level pipelines' lanes are hits from all over the scene: the wave-wide
// test never fires there and costs a branch and half a dozen instructions per sphere (headline leaf kernel 1.282 -> 1.247 ms without
// it; two spheres per trip written out by hand, on top: 1.287 ms — eight more live registers, 47 spilled instead of 24).
#ifndef SKR_COHERENT_TRIP
#define SKR_COHERENT_TRIP 4 // spheres per trip of the coherent shadow loop (the wave-wide exit is looked at once per trip)
#endif
// With shadow masks (the level pipelines, !COHERENT): `cand` = the union of the lane's two masks (shadow_mask_of).  A sphere outside a
// ray's mask provably fails pair_any_step's candidate test (its D < 0), so each lane walks only its own candidates, lowest index first: the first
// occluder it finds is the one the loop over every sphere finds, and every decision and count is the same.
// M: where the spheres are (AtRest, MovingCentres).
template <bool COHERENT, typename SH = RunTimeShape, typename M = AtRest>
SKR_DEV void occluded_pair(const SceneView &sv, f3 P, f3 L0, f3 L1, bool second, bool &occ0, bool &occ1, uint32_t &tests, uint32_t cand = 0u, const M &m = M())
{
	const f3 o = add_scalar(P, 0.000001f);
	const RayPair rp = make_pair(L0, L1);
	const PairAny pa = make_pair_any(rp);
	occ0 = false;
	occ1 = !second;
	auto test = [&](const float4 g, int i) { pair_any_step(rp, pa, o, m.row(g, i), i, occ0, occ1, tests); };
	if(COHERENT) table_rows<SKR_COHERENT_TRIP>(sv.geom_u, sv.ns, test, [&] { return !__all(occ0 && occ1); }); // (the wave-wide exit, once per trip)
	else if(SH::masks || sv.smask)
	{
		diag_mask_gate(19, cand, sv.ns);
		masked_rows(sv, cand, test);
	}
	else sphere_rows(sv, test);
	if(!occ0) tests += (uint32_t) sv.ns;
	if(second && !occ1) tests += (uint32_t) sv.ns;
	if(!second) occ1 = false;
}

// The union of the shadow masks of lights i and (second) i + 1 at P, for occluded_pair; 0 where it walks every sphere.  (The masks
// exist only for scenes whose lights are all point lights.)  `sph`: the sphere P was hit on, or -1 (not known, not a sphere).  Where
// the launch has the surface patches (DESIGN.md "Shadow surface patches"), sph is in range and fl(|e|^2) - r^2 of e = P - C_sph is
// within the sphere's radial slack, the mask is the one word of e's patch in the pair's table: one cell, one gather, and the spheres
// behind P or under it are not named.  Everywhere else (NaN, a point off its sphere, no patches) the two direction masks, unchanged.
// The index is in bounds whatever P holds.
template <bool COHERENT, typename SH = RunTimeShape>
SKR_DEV uint32_t shadow_cands(const SceneView &sv, const RenderParams &p, int i, bool second, f3 P, int sph = -1)
{
	if(COHERENT || !(SH::masks || sv.smask) || !(SH::shadows || p.use_shadows)) return 0u;
	if(p.shadow_surface_word != 0u && (uint32_t) sph < (uint32_t) sv.ns)
	{
		const float4 g = sv.geom[sph];
		const uint32_t head = __float_as_uint(sv.kd[sph].w), n = head >> 24; // (base | G << 24: shadow_cells.h)
		const f3 e = P - ld3(g);
		const float c = dot3(e, e) - g.w;
		if(n != 0u && __builtin_fabsf(c) <= g.w * SKR_SURFACE_SLACK) // (NaN: no)
		{
			const CubeCell cc = cube_cell_n(e, (int) n);
			return sv.smask[p.shadow_surface_word + (uint32_t) (i >> 1) * p.shadow_surface_stride + (head & 0xffffffu) + ((uint32_t) cc.face * n + (uint32_t) cc.i) * n + (uint32_t) cc.j];
		}
	}
	const uint32_t m0 = shadow_mask_of(sv, i, ld3(sv.lights[2 * i]) - P);
	return second ? m0 | shadow_mask_of(sv, i + 1, ld3(sv.lights[2 * i + 2]) - P) : m0;
}
// (the facts of a shape that fixes them; else what the launch says)
template <typename SH>
SKR_DEV int shape_lights(const SceneView &sv)
{
	if constexpr(SH::lights > 0) return SH::lights;
	else return sv.nl;
}

// ---- the sphere tree (include/skr.h skr_scene_set_sphere_tree; scene_trees.cpp skr_build_sphere_tree) ----
// The conservative line test of an entry {C, R^2} with its slack factor kappa: false only where no sphere below the entry can be a
// candidate (binary32 D >= 0) of this lane's line.  The slack of D grows with the distance of the ray's origin, so it is a factor of
// |C - o|^2 and not a part of the radius.  NaN anywhere => true.
SKR_DEV bool sphere_entry_touched(f3 o, f3 d, float dd, float4 A, float kappa)
{
	const f3 e = ld3(A) - o;
	const f3 cr = cross3(e, d);
	return !(dot3(cr, cr) > (A.w + kappa * dot3(e, e)) * dd);
}

SKR_DEV void sphere_work_add(const SphereTree &st, uint32_t n_cull, uint32_t n_sph)
{
	if(st.work && (n_cull | n_sph))
	{
		const unsigned long long m = __ballot(true);
		if(__builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u)) == 0)
		{
			unsigned long long *w = st.work + 2u * ((blockIdx.x * 4u + (threadIdx.x >> 6)) & (SKR_TRI_WORK_SHARDS - 1u));
			atomicAdd(&w[0], (unsigned long long) n_cull);
			atomicAdd(&w[1], (unsigned long long) n_sph);
		}
	}
}

// The walk of mesh_walk() over the sphere tree: one wave-uniform index over the depth-first nodes, no stack, rows through the scalar
// cache; both successors of a node are fetched while its culling sphere is tested.  `live()` = the rays of the lane (a bit each) that
// still want tests; `touch(A, kappa, smallest file index below)` = those of them that want this entry: an entry is entered when any
// lane wants it, and `sphere(row, file index, mine)` sees every sphere of a chunk some lane wants, with the bits of its own lane.
// The always-tested chunks at the front come first, without a culling test.
template <bool COUNT, typename V, typename T, typename S>
SKR_DEV void stree_walk(const SphereTree &st, V live, T touch, S sphere)
{
	uint32_t n_cull = 0, n_sph = 0;
	auto chunk_spheres = [&](int c, float4 cL, uint32_t mine)
	{
		const int i0 = __float_as_int(cL.z), cnt = __float_as_int(cL.w);
		const float4 fi = mesh_row(st.chunks, 3 * c + 2);
		const int file[4] = {__float_as_int(fi.x), __float_as_int(fi.y), __float_as_int(fi.z), __float_as_int(fi.w)};
		float4 g[4];
#pragma unroll
		for(int k = 0; k < 4; k++) g[k] = mesh_row(st.rows, i0 + k); // (the rows behind the last sphere are the blob's: readable)
#pragma unroll
		for(int k = 0; k < 4; k++)
			if(k < cnt)
			{
				if(COUNT) n_sph += lanes_of(mine);
				sphere(g[k], file[k], mine);
			}
	};
	for(int c = 0; c < st.n_always; c++) chunk_spheres(c, mesh_row(st.chunks, 3 * c + 1), live());
	int i = 0;
	float4 A = mesh_row(st.nodes, 0), L = mesh_row(st.nodes, 1);
	while(i < st.n_nodes)
	{
		const int i_out = __float_as_int(L.y);
		const float4 A_in = mesh_row(st.nodes, 2 * i + 2), L_in = mesh_row(st.nodes, 2 * i + 3);
		const float4 A_out = mesh_row(st.nodes, 2 * i_out), L_out = mesh_row(st.nodes, 2 * i_out + 1);
		if(COUNT) n_cull += lanes_of(live());
		const bool enter = __any(touch(A, L.x, __float_as_int(L.w)) != 0u);
		const int c0 = __float_as_int(L.z);
		if(enter && c0 >= 0)
		{ // height 1: its chunk entries are contiguous
			const int c1 = c0 + 8 < st.n_chunks ? c0 + 8 : st.n_chunks;
			float4 cA_next = mesh_row(st.chunks, 3 * c0), cL_next = mesh_row(st.chunks, 3 * c0 + 1);
			for(int c = c0; c < c1; c++)
			{
				const float4 cA = cA_next, cL = cL_next;
				cA_next = mesh_row(st.chunks, 3 * c + 3);
				cL_next = mesh_row(st.chunks, 3 * c + 4);
				if(COUNT) n_cull += lanes_of(live());
				const uint32_t mine = touch(cA, cL.x, __float_as_int(cL.y));
				if(__any(mine != 0u)) chunk_spheres(c, cL, mine);
			}
		}
		i = enter ? i + 1 : i_out;
		A = enter ? A_in : A_out;
		L = enter ? L_in : L_out;
	}
	if(COUNT) sphere_work_add(st, n_cull, n_sph);
}

// does a wave whose lanes are all here walk the tree: every lane's origin in the ball, every direction of a length the bounds hold for
SKR_DEV bool stree_lane_fits(const SphereTree &st, f3 o, float dd)
{
	const f3 e = o - mk3(st.ball.x, st.ball.y, st.ball.z);
	return (dot3(e, e) <= st.ball.w * st.ball.w) && (dd >= 0x1p-44f) && (dd <= 0x1p44f); // (NaN: no)
}

// closest_sphere() on the tree (raytrace.h:152-165): the smallest t2 wins, equal t2 goes to the lower file index; the index returned is
// the file's.  The brackets of the candidates the walk meets are selected as closest_of_rows selects them — the outcome does not
// depend on the order where the winner's bracket lies strictly below every other's —; where brackets overlap a second walk evaluates the
// exact form of every candidate of the lanes concerned (every accepted sphere is a candidate: t2 > 1 needs D >= 0 and b < 0).
template <bool COUNT>
SKR_DEV int stree_closest_walk(const SphereTree &st, const RayConst &r, float &tmin)
{
	const RayFilt f = make_filt(r.d);
	const float dd = r.two_a * 0.5f; // dot(d, d)
	int best = -1;
	float best_lo = __builtin_inff(), best_hi = __builtin_inff(), others_lo = __builtin_inff();
	float best_b = 0.0f, best_D = 0.0f;
	stree_walk<COUNT>(st, [] { return 1u; },
		[&](const float4 A, float kappa, int) { return sphere_entry_touched(r.o, r.d, dd, A, kappa) ? 1u : 0u; },
		[&](const float4 g, int file, uint32_t mine)
		{
			float lo, hi, b, D;
			if(mine && sphere_bracket(r.o, r.d, f, g, lo, hi, b, D)) best_update(best_hi, others_lo, best_lo, best, best_b, best_D, file, lo, hi, b, D);
		});
	tmin = __builtin_inff();
	const bool unsure = best >= 0 && !(others_lo > best_hi);
	if(best >= 0 && !unsure) tmin = bracket_t(f.two_a, best_lo, best_hi, best_b, best_D);
	if(__any(unsure))
	{
		int eb = -1;
		float et = __builtin_inff();
		stree_walk<COUNT>(st, [&] { return unsure ? 1u : 0u; },
			[&](const float4 A, float kappa, int) { return (unsure && sphere_entry_touched(r.o, r.d, dd, A, kappa)) ? 1u : 0u; },
			[&](const float4 g, int file, uint32_t mine)
			{
				if(!mine) return;
				const float t = sphere_distance(r.o, r.d, r.two_a, r.four_a, g);
				if(accept_distance(t) && (t < et || (t == et && file < eb)))
				{
					et = t;
					eb = file;
				}
			});
		if(unsure)
		{
			best = eb;
			tmin = et;
		}
	}
	return best;
}
// (every lane of the wave that traces a ray arrives here: the choice between the walk and the loop is wave-wide)
SKR_DEV int stree_closest(const SphereTree &st, const SceneView &sv, const RayConst &r, float &tmin)
{
	if(!st.cull || !__all(stree_lane_fits(st, r.o, r.two_a * 0.5f))) return closest_sphere(sv, r, tmin); // every row in file order, from HBM
	if(__builtin_expect(st.work != nullptr, 0)) return stree_closest_walk<true>(st, r, tmin);
	return stree_closest_walk<false>(st, r, tmin);
}

// occluded_pair() on the tree (utils.h:42-58).  The reference's loop stops at its first occluder in file order and `tests` counts the
// spheres up to it, so the walk looks for the LOWEST file index among each ray's occluders: it cannot stop at the first one it meets,
// but a ray wants neither a sphere nor an entry whose smallest file index is not below the best it has.
template <bool COUNT>
SKR_DEV void stree_occluded_walk(const SphereTree &st, f3 o, const RayPair &rp, f3 L0, f3 L1, bool second, int &idx0, int &idx1)
{
	const PairAny pa = make_pair_any(rp);
	const float dd0 = rp.two_a.x * 0.5f, dd1 = rp.two_a.y * 0.5f;
	constexpr int none = 0x7fffffff;
	idx0 = none;
	idx1 = second ? none : -1;
	stree_walk<COUNT>(st, [&] { return (idx0 > 0 ? 1u : 0u) | (idx1 > 0 ? 2u : 0u); },
		[&](const float4 A, float kappa, int low)
		{
			const uint32_t m0 = (low < idx0 && sphere_entry_touched(o, L0, dd0, A, kappa)) ? 1u : 0u;
			const uint32_t m1 = (low < idx1 && sphere_entry_touched(o, L1, dd1, A, kappa)) ? 2u : 0u;
			return m0 | m1;
		},
		[&](const float4 g, int file, uint32_t mine)
		{
			const bool w0 = (mine & 1u) && file < idx0, w1 = (mine & 2u) && file < idx1;
			if(!(w0 || w1)) return;
			const f3 e = o - ld3(g);
			const float c = dot3(e, e) - g.w;
			f2 b, D;
			pair_bD(rp, e, c, b, D);
			const bool cand0 = w0 && (D.x >= 0.0f) && (b.x < 0.0f), cand1 = w1 && (D.y >= 0.0f) && (b.y < 0.0f);
			if(cand0 || cand1)
			{
				f2 m, al, rl;
				pair_any_m(pa, b, m, al, rl);
				if(cand0 && any_decide(pa.sane0, pa.two_a.x, pa.quarter.x, b.x, D.x, m.x, al.x, rl.x)) idx0 = file;
				if(cand1 && any_decide(pa.sane1, pa.two_a.y, pa.quarter.y, b.y, D.y, m.y, al.y, rl.y)) idx1 = file;
			}
		});
}

// the sphere test of direct_light_of on the tree (SphereLoopShadows' counterpart); a wave with a lane the tree does not hold for runs
// occluded_pair's loop over every row in file order, from HBM (the instances with the tree have no shadow masks)
struct SphereTreeShadows {
	const SphereTree &st;
	static constexpr bool loops = false;
	__device__ __forceinline__ void pair(const SceneView &sv, f3 P, f3 L0, f3 L1, bool second, bool &occ0, bool &occ1, uint32_t &tests) const
	{
		const f3 o = add_scalar(P, 0.000001f);
		const RayPair rp = make_pair(L0, L1);
		const bool fits = stree_lane_fits(st, o, rp.two_a.x * 0.5f) && (!second || stree_lane_fits(st, o, rp.two_a.y * 0.5f));
		if(!st.cull || !__all(fits))
		{
			occluded_pair<false>(sv, P, L0, L1, second, occ0, occ1, tests, 0u);
			return;
		}
		int idx0, idx1;
		if(__builtin_expect(st.work != nullptr, 0)) stree_occluded_walk<true>(st, o, rp, L0, L1, second, idx0, idx1);
		else stree_occluded_walk<false>(st, o, rp, L0, L1, second, idx0, idx1);
		occ0 = idx0 != 0x7fffffff;
		occ1 = second && idx1 != 0x7fffffff;
		tests += occ0 ? (uint32_t) idx0 + 1u : (uint32_t) sv.ns;
		if(second) tests += occ1 ? (uint32_t) idx1 + 1u : (uint32_t) sv.ns;
	}
};

struct LightTerm { // the per-light quantities of blinn_phong.h:67-72 / :100-117
	f3 L, lc;
	float intensity; // 1 / powf(|Lp - P|, 2) (== 1 / (d * d): SURVEY.md 8c); exactly 1 for a directional light
};

template <typename SH = RunTimeShape>
SKR_DEV LightTerm light_term(const SceneView &sv, int i, f3 P)
{
	LightTerm t;
	const float4 lp4 = sv.lights[2 * i];
	t.lc = ld3(sv.lights[2 * i + 1]);
	if(!SH::point_lights && lp4.w != 0.0f)
	{ // a directional light (--strict-scn only; blinn_phong.h:81-82,126-128): L = normalize(direction) and no 1/d^2 — the intensity
	  // factor of the point-light expression is exactly 1, and x * 1 == x
		t.L = normalize3(ld3(lp4));
		t.intensity = 1.0f;
		return t;
	}
	const f3 to_l = ld3(lp4) - P;
	const LenTerms lt = len_terms<true>(sqr3(to_l));
	t.L = to_l * lt.inv;
	t.intensity = lt.inv2;
	return t;
}

// what direct_light_of does about triangles in the way of a light where triangle shadows are not in force: nothing, and no code
struct NoTriangleShadows {
	static constexpr bool on = false;
};

// How direct_light_of tests the spheres against the shadow rays of a pair of lights: the loops over the sphere table (occluded_pair, with
// the shadow masks where the launch has them), or the sphere tree's pair walk (SphereTreeShadows below).  Chosen at compile time, so
// that the instances on the loops keep their code.
struct SphereLoopShadows {
	static constexpr bool loops = true;
};

// raytrace.h:36-44 = bp::ambient (blinn_phong.h:13) + diffuse (:47) + specular (:90).
// The reference casts the same shadow ray in diffuse and again in specular; one cast serves both.
// (kd, ks, ambp = {La * ka, power}: the material rows of the surface hit)
// sph: the sphere the point was hit on where the caller has it (shadow_cands), -1 elsewhere.
// TS: triangle shadows (include/skr.h skr_scene_set_triangle_shadows) — `tri_shadows(P, i, second, L0, L1, occ0, occ1)` darkens the lights of a
// pair that the spheres left lit and a triangle occludes (render_generic.hip TriangleShadows); chosen at compile time, so that the
// instances without it keep their code.
// SH: the facts of the launch that are compiled in (RunTimeShape: none).
template <bool COHERENT, typename TS = NoTriangleShadows, typename SS = SphereLoopShadows, typename SH = RunTimeShape>
SKR_DEV f3 direct_light_of(const SceneView &sv, const RenderParams &p, f3 kd, f3 ks, float4 ambp, f3 P, f3 N, Counters &cn, const TS &tri_shadows = TS(),
						   const SS &sphere_shadows = SS(), int sph = -1)
{
	f3 diffuse = mk3(0, 0, 0), specular = mk3(0, 0, 0);
	const f3 view = normalize3(p.cam_pos - P); // always the camera (blinn_phong.h:93)
	const int nl = shape_lights<SH>(sv);
	for(int i = 0; i < nl; i += 2)
	{
		const bool second = i + 1 < nl;
		const uint32_t cand = SS::loops ? shadow_cands<COHERENT, SH>(sv, p, i, second, P, sph) : 0u; // (asked for ahead of the light terms)
		const LightTerm t0 = light_term<SH>(sv, i, P), t1 = light_term<SH>(sv, second ? i + 1 : i, P);
		bool occ0 = false, occ1 = false;
		if(SH::shadows || p.use_shadows)
		{
			cn.shadow_rays += second ? 2u : 1u;
			if constexpr(SS::loops) occluded_pair<COHERENT, SH>(sv, P, t0.L, t1.L, second, occ0, occ1, cn.shadow_tests, cand);
			else sphere_shadows.pair(sv, P, t0.L, t1.L, second, occ0, occ1, cn.shadow_tests);
			if constexpr(TS::on) tri_shadows(P, i, second, t0.L, t1.L, occ0, occ1);
		}
		auto add_light = [&](const LightTerm &t, bool lit)
		{
			if(lit)
			{
				diffuse = diffuse + ((kd * t.lc) * t.intensity) * max0(dot3(N, t.L));
				const f3 vl = view + t.L;
				const f3 H = vl / length3(vl);
				specular = specular + ((ks * t.lc) * t.intensity) * powf_spec<SH::pow7, SH::pow_any>(max0(dot3(N, H)), ambp.w, p.pow_steps);
			}
		};
		add_light(t0, !occ0);
		add_light(t1, second && !occ1);
	}
	f3 total = mk3(0, 0, 0);
	total = total + ld3(ambp);
	total = total + diffuse;
	total = total + specular;
	return total;
}

// raytrace.h:36-44's closing sum, ambient + diffuse + specular from (0,0,0).  direct_light_cone's; direct_light_of and direct_light_fog keep
// their own copies of it and of the Blinn-Phong terms, as does direct_light_cone of the latter.
SKR_DEV f3 light_sum(float4 ambp, f3 diffuse, f3 specular)
{
	f3 total = mk3(0, 0, 0);
	total = total + ld3(ambp);
	total = total + diffuse;
	total = total + specular;
	return total;
}

// ---- spot lights (include/skr.h SKR_SCN_SPOT; general level pipeline only) ----
// The cone decision and factor of one light at one shading point: a, c1, c2 as the host derived them (render_params.h SpotLights), L the
// unit vector from the point to the light (light_term).  One correctly rounded binary32 operation per step; NaN: outside.
struct SpotCone {
	float f;      // what the light's colour is multiplied by; 0 where outside
	bool outside; // the light adds nothing and casts no shadow ray
};
SKR_DEV SpotCone spot_cone(f3 a, float c1, float c2, f3 L)
{
	const float c = -dot3(a, L);
	if(c >= c1) return SpotCone{1.0f, false};
	if(!(c > c2)) return SpotCone{0.0f, true};
	const float u = sk_divf(c - c2, c1 - c2);
	return SpotCone{(u * u) * (3.0f - 2.0f * u), false};
}

// ---- lights with a radius (include/skr.h skr_scene_set_light_radii; general level pipeline only) ----
// The sample position of the light l at Lp with radius R for the shading node (pixel, aa, node): one Philox call, then binary32 with one
// correctly rounded operation per step.  R == 0 (and NaN): no draw, Lp itself.  phi <= (float) 2 pi: inside the range sincos_spec is
// exhaustively checked on.
SKR_DEV f3 soft_sample(uint32_t pixel, uint32_t aa, uint32_t node, uint32_t l, uint32_t k0, uint32_t k1, f3 Lp, float R)
{
	if(!(R > 0.0f)) return Lp;
	uint32_t rnd[4];
	philox4x32(pixel, aa, node, soft_ctr3(l), k0, k1, rnd);
	const float u1 = u31_to_unit(rnd[0]), u2 = u31_to_unit(rnd[1]);
	const float z = 1.0f - 2.0f * u1;
	const float s = sk_sqrtf(max0(1.0f - z * z));
	float sn, cs;
	sincos_spec(0x1.921fb6p+2f * u2, sn, cs); // (float) 2 pi times u2, in binary32
	return mk3(Lp.x + R * (s * cs), Lp.y + R * z, Lp.z + R * (s * sn));
}

// One float of a table that no kernel writes, at a wave-uniform index, through the constant address space (load_const4's reason).
SKR_DEV float load_const1(const float *base, int i)
{
	const float __attribute__((address_space(4))) *q = (const float __attribute__((address_space(4))) *) (unsigned long long) base;
	return q[i];
}

// direct_light_of<false>() for a scene with spot lights: the pair loop with the cone decision ahead of the shadow walk.  A pair whose
// lights are both inside (or no spot lights) is walked as direct_light_of walks it, with the union of both shadow masks; where one
// light is outside at P the other is walked as a single, with its own mask; where both are, the lane casts nothing.  An outside light
// counts no shadow ray and no sphere test and meets no triangle.
// SOFT: some light of the scene has a radius — the sample ahead of the cone decision.  A light with R > 0 is, for this node, the point
// light at its sample: L, 1 / d^2, the cone decision, the shadow ray and the far end of the triangle walk all come from the sample.  A
// pair in which either light has R > 0 walks every sphere (the shadow masks are built for rays toward Lp); a pair of two R == 0 lights
// is walked as without SOFT.  (pixel, node): the node's counter words.  Nothing of a sample stays live across the shadow walk but its
// LightTerm: the triangle walk's far end draws the sample again.
// M: where the spheres are for the shadow rays (AtRest, MovingCentres; a caller with MovingCentres hands in a view without shadow masks).
template <bool SOFT, typename TS, typename M = AtRest>
SKR_DEV f3 direct_light_cone(const SceneView &sv, const RenderParams &p, const SpotLights &sp, const SoftLights &so, f3 kd, f3 ks, float4 ambp, f3 P, f3 N,
							 uint32_t pixel, uint32_t node, Counters &cn, const TS &tri_shadows, const M &m = M())
{
	f3 diffuse = mk3(0, 0, 0), specular = mk3(0, 0, 0);
	const f3 view = normalize3(p.cam_pos - P);
	for(int i = 0; i < sv.nl; i += 2)
	{
		const bool second = i + 1 < sv.nl;
		// (l is wave-uniform: the radius and the cone rows come through the scalar cache, and the branches on them are the wave's)
		auto radius = [&](int l) { return l < so.n ? load_const1(so.radii, l) : 0.0f; };
		const float R0 = SOFT ? radius(i) : 0.0f, R1 = SOFT && second ? radius(i + 1) : 0.0f;
		auto to_light = [&](int l, float R) { return soft_sample(pixel, p.aa_index, node, (uint32_t) l, p.seed_lo, p.seed_hi, ld3(sv.lights[2 * l]), R) - P; };
		auto term = [&](int l, float R)
		{
			if(!(R > 0.0f)) return light_term(sv, l, P);
			LightTerm t; // light_term's point light, at the sample
			t.lc = ld3(sv.lights[2 * l + 1]);
			const f3 to_l = to_light(l, R);
			const LenTerms lt = len_terms<true>(sqr3(to_l));
			t.L = to_l * lt.inv;
			t.intensity = lt.inv2;
			return t;
		};
		// (SOFT is a constant, one arm of each ?: is compiled; without it the second term is light_term at the index `second` selects, as in direct_light_of)
		LightTerm t0 = SOFT ? term(i, R0) : light_term(sv, i, P), t1 = SOFT ? (second ? term(i + 1, R1) : t0) : light_term(sv, second ? i + 1 : i, P);
		bool in0 = true, in1 = second;
		auto cone = [&](int l, LightTerm &t, bool &in)
		{
			if((uint32_t) (l - sp.first) < (uint32_t) sp.n)
			{
				const float4 A = load_const4(sp.cones, 2 * (l - sp.first)), B = load_const4(sp.cones, 2 * (l - sp.first) + 1);
				const SpotCone c = spot_cone(ld3(A), A.w, B.x, t.L);
				in = !c.outside;
				t.lc = t.lc * c.f; // (per component, before anything else; x * 1 == x)
			}
		};
		cone(i, t0, in0);
		if(second) cone(i + 1, t1, in1);
		bool occ0 = !in0, occ1 = !in1; // (dark: occluded, or outside its cone)
		if(p.use_shadows && (in0 || in1))
		{ // the rays of the lane: (a, b) = the pair, or a = the one light that is inside
			const bool both = in0 && in1;
			const int la = in0 ? i : i + 1;
			const f3 La = in0 ? t0.L : t1.L;
			cn.shadow_rays += both ? 2u : 1u;
			SceneView every; // SOFT: the scene without its shadow masks, for a pair with a sample (every sphere)
			if constexpr(SOFT)
			{
				every = sv;
				if(R0 > 0.0f || R1 > 0.0f) every.smask = nullptr;
			}
			const SceneView &w = SOFT ? every : sv; // (two lvalues of one type: a reference to one of them, no copy; without SOFT `every` is never touched)
			uint32_t cand = 0u;
			if(w.smask)
			{
				cand = shadow_mask_of(sv, la, ld3(sv.lights[2 * la]) - P);
				if(both) cand |= shadow_mask_of(sv, i + 1, ld3(sv.lights[2 * i + 2]) - P);
			}
			bool oa, ob;
			occluded_pair<false, RunTimeShape, M>(w, P, La, t1.L, both, oa, ob, cn.shadow_tests, cand, m);
			if constexpr(TS::on && SOFT)
			{ // blinn_phong.h's `distance`, of the sample where the light has one
				auto far = [&](int l, float R) { return R > 0.0f ? length3(to_light(l, R)) : tri_shadows.reach(l, P); };
				const float fa = far(la, in0 ? R0 : R1), fb = both ? far(i + 1, R1) : fa;
				tri_shadows.ends(P, both, La, t1.L, fa, fb, oa, ob);
			}
			else if constexpr(TS::on) tri_shadows.lights(P, la, i + 1, both, La, t1.L, oa, ob);
			occ0 = in0 ? oa : true;
			occ1 = both ? ob : (in1 ? oa : true);
		}
		auto add_light = [&](const LightTerm &t, bool lit)
		{
			if(lit)
			{
				diffuse = diffuse + ((kd * t.lc) * t.intensity) * max0(dot3(N, t.L));
				const f3 vl = view + t.L;
				const f3 H = vl / length3(vl);
				specular = specular + ((ks * t.lc) * t.intensity) * powf_spec(max0(dot3(N, H)), ambp.w, p.pow_steps);
			}
		};
		add_light(t0, !occ0);
		add_light(t1, !occ1);
	}
	return light_sum(ambp, diffuse, specular);
}

template <bool COHERENT, typename SH = RunTimeShape>
SKR_DEV f3 direct_light(const SceneView &sv, const RenderParams &p, int sph, f3 P, f3 N, Counters &cn)
{
	return direct_light_of<COHERENT, NoTriangleShadows, SphereLoopShadows, SH>(sv, p, ld3(sv.kd[sph]), ld3(sv.ks[sph]), sv.amb[sph], P, N, cn, NoTriangleShadows(), SphereLoopShadows(), sph);
}

// ---- --scn-fog (DESIGN.md "Spherical fog"; general level pipeline only): blinn_phong.h:19-43 as written, rand() replaced ----
// One fog term (blinn_phong.h:19-43 with utils.h:216-225 inlined) for the lit point light t at `lpos` and a hit on the sphere at `centre`;
// the fog's rows a = [radius absorption scattering -], alb = [albedo -] (RenderParams::fog).  ctr: the counter of its one Philox call.
SKR_DEV f3 fog_term(float4 a, float4 alb, const LightTerm &t, f3 centre, f3 lpos, f3 kd, f3 N, const uint32_t ctr[4], uint32_t k0, uint32_t k1,
					float *no_interaction_out = nullptr)
{
	float distance = length3(centre - lpos); // :22 (the sphere's centre, not the hit point)
	if(distance > 2 * a.x) distance = 2 * a.x;
	const float no_interaction = (float) exp_spec((double) ((-1.0f * distance) * (a.y + a.z))); // :27, binary64 exp
	if(no_interaction_out) *no_interaction_out = no_interaction;
	uint32_t rnd[4];
	philox4x32(ctr[0], ctr[1], ctr[2], ctr[3], k0, k1, rnd);
	if(u31_to_unit(rnd[0]) > no_interaction) return ((kd * t.lc) * t.intensity) * max0(dot3(N, t.L)); // :30-38, the plain diffuse term
	// :41-42 + utils.h:219-224: the direction is not re-normalised, no intensity factor
	const f3 nd = mk3(t.L.x + u31_to_pm1(rnd[1]) * a.z, t.L.y + u31_to_pm1(rnd[2]) * a.z, t.L.z + u31_to_pm1(rnd[3]) * a.z);
	return (ld3(alb) * t.lc) * max0(dot3(N, nd));
}

// direct_light_of() for a sphere hit of a scene with fog (blinn_phong.h:47-134): every lit point light adds the fog term of every fog
// volume, in file order, INSTEAD of its diffuse term, and again instead of its specular term; directional lights and the ambient term
// are unchanged.  (pixel, node): the node's counter words (DESIGN.md "Counter RNG").
template <typename SS = SphereLoopShadows>
SKR_DEV f3 direct_light_fog(const SceneView &sv, const RenderParams &p, f3 kd, f3 ks, float4 ambp, f3 P, f3 N, f3 centre, uint32_t pixel,
							uint32_t node, Counters &cn, const SS &sphere_shadows = SS())
{
	f3 diffuse = mk3(0, 0, 0), specular = mk3(0, 0, 0);
	const f3 view = normalize3(p.cam_pos - P);
	for(int i = 0; i < sv.nl; i += 2)
	{
		const bool second = i + 1 < sv.nl;
		const uint32_t cand = SS::loops ? shadow_cands<false>(sv, p, i, second, P) : 0u;
		const LightTerm t0 = light_term(sv, i, P), t1 = light_term(sv, second ? i + 1 : i, P);
		bool occ0 = false, occ1 = false;
		if(p.use_shadows)
		{
			cn.shadow_rays += second ? 2u : 1u;
			if constexpr(SS::loops) occluded_pair<false>(sv, P, t0.L, t1.L, second, occ0, occ1, cn.shadow_tests, cand);
			else sphere_shadows.pair(sv, P, t0.L, t1.L, second, occ0, occ1, cn.shadow_tests);
		}
		auto add_light = [&](const LightTerm &t, int l, bool lit)
		{
			if(!lit) return;
			const float4 lp4 = sv.lights[2 * l];
			if(lp4.w == 0.0f)
			{ // a point light: blinn_phong.h:62-64, :106-108
				for(uint32_t pass = 0; pass < 2; pass++)
					for(int j = 0; j < p.n_fog; j++)
					{
						const uint32_t ctr[4] = {pixel, p.aa_index, node, fog_ctr3((uint32_t) l, (uint32_t) j, pass)};
						const f3 f = fog_term(load_const4(p.sph_geom + p.fog_row, 2 * j), load_const4(p.sph_geom + p.fog_row, 2 * j + 1), t, centre, ld3(lp4), kd, N, ctr, p.seed_lo, p.seed_hi);
						if(pass == 0) diffuse = diffuse + f;
						else specular = specular + f;
					}
				return;
			}
			diffuse = diffuse + ((kd * t.lc) * t.intensity) * max0(dot3(N, t.L));
			const f3 vl = view + t.L;
			const f3 H = vl / length3(vl);
			specular = specular + ((ks * t.lc) * t.intensity) * powf_spec(max0(dot3(N, H)), ambp.w, p.pow_steps);
		};
		add_light(t0, i, !occ0);
		add_light(t1, i + 1, second && !occ1);
	}
	f3 total = mk3(0, 0, 0);
	total = total + ld3(ambp);
	total = total + diffuse;
	total = total + specular;
	return total;
}

// raytrace.h:22-30 + :117-125: hemisphere sample and the reference's basis mix
// (perp_to_both.y/.z where perp_to_normal.y/.z belongs — kept), for the two sibling rays of a pair at once in packed binary32
// (every component is the one-ray expression: v_pk_* round each half like the scalar instruction).
#ifndef SKR_GI_INLINE
#define SKR_GI_INLINE 0 // 1: inline gi_direction_pair into its callers (A/B builds)
#endif
struct DirPair { f3 d0, d1; }; // (returned by value: in registers, where reference parameters of an out-of-line function go through scratch)
#if SKR_GI_INLINE
SKR_DEV
#else
static __device__ __attribute__((noinline))
#endif
DirPair gi_direction_pair(float r1a, float r2a, float r1b, float r2b, f3 N, f3 nt, f3 nb)
{
	const f2 r1 = f2{r1a, r1b};
	const f2 om = 1.0f - r1 * r1;
	const f2 s_theta = f2{sk_sqrtf(om.x), sk_sqrtf(om.y)};
	// (2.0f*M_PI)*r2 in double, narrowed (raytrace.h:25: `float phi = 2 * M_PI * r2`)
	const f2 phi = f2{(float) ((2.0 * 3.14159265358979323846) * (double) r2a), (float) ((2.0 * 3.14159265358979323846) * (double) r2b)};
	f2 sn, cs;
	sincos_spec2(phi, sn, cs);
	const f2 sx = s_theta * cs, sy = r1, sz = s_theta * sn;
	const f2 x = (sx * nb.x + sy * N.x) + sz * nt.x;
	const f2 y = (sx * nb.y + sy * N.y) + sz * nb.y;
	const f2 z = (sx * nb.z + sy * N.z) + sz * nb.z;
	return DirPair{mk3(x.x, y.x, z.x), mk3(x.y, y.y, z.y)};
}

SKR_DEV f3 gi_direction(float r1, float r2, f3 N, f3 nt, f3 nb)
{
	return gi_direction_pair(r1, r2, r1, r2, N, nt, nb).d0;
}

// ---- --shade-triangles (the rules: include/skr.h skr_options.shade_triangles): the closest accepted triangle ----
struct TriBest {
	float t;  // smallest accepted distance so far (starts at the closest sphere's)
	int file; // index of that triangle in the scene file, -1 = the sphere still wins
	int slot; // its position in tris[]
};

SKR_DEV void tri_consider(const RayConst &r, bool mine, f3 v0, float4 n1, float4 n2, int slot, int from_tri, TriBest &b)
{
	float t;
	if(mine && triangle_hit(r.o, r.d, v0, ld3(n1), ld3(n2), t) && t > 0.0f)
	{
		const int file = __float_as_int(n1.w);
		if(file != from_tri && (t < b.t || (t == b.t && b.file >= 0 && file < b.file)))
		{
			b.t = t;
			b.file = file;
			b.slot = slot;
		}
	}
}

// line_touches() for the closest-hit walk: false also where every hit under the entry would lie BEHIND the running best.  A hit point
// o + t d of an accepted triangle lies inside the entry's sphere (that is what the sphere bounds), so t |d| >= d^ . (C - o) - R:
// with lhs = d . (C - o) - t_best (d . d) the entry cannot hold a nearer hit once lhs > R |d|.  The radii carry 16x the rounding slack
// of the test's own u, v; the float t of a near-degenerate triangle can be off by as much again, so the entry is only skipped
// at lhs > 1.125 R |d| (two slacks to spare).  An equal t must still be visited (the lower file index wins a tie): strict test.
template <bool CONES>
SKR_DEV bool entry_may_hold_nearer(const RayConst &r, float dd, float4 A, float4 B, float t_best)
{
	const LinePart p = line_part<CONES>(r, dd, A, B);
	if(p.cr2 > p.lim) return false; // the line misses the sphere (NaN: falls through, "enter")
	const float lhs = dot3(r.d, p.e) - t_best * dd;
	return !(lhs > 0.0f && lhs * lhs > p.lim * 1.27f);
}

// The closest-hit walk: every chunk whose conservative sphere this lane's line touches in front of its running best is tested to the
// end (the spheres bound the accept test itself, whatever t comes out).  mesh_walk() written out by hand: as its visitor the ray
// queries' 2^22 random rays on dragon.scn took 21.11 against 21.02 ms (spreads 0.02 and 0.04; with entries and triangles asked for
// one ahead 24.3 ms), the frame and the camera rays what they take here.
template <bool CONES>
SKR_DEV void tree_walk_closest(const SceneView &sv, const RayConst &r, int from_tri, TriBest &b)
{
	const float dd = r.two_a * 0.5f; // dot(d, d)
	int i = 0;
	uint32_t n_cull = 0, n_tri = 0;
	const float4 *chunk_ent = sv.chunks + 3 * (sv.nchunks + 1);
	float4 A = mesh_row(sv.chunks, 0), B = mesh_row(sv.chunks, 1), lk = mesh_row(sv.chunks, 2);
	while(i < sv.nchunks)
	{
		const int i_out = __float_as_int(lk.x);
		const float4 A_in = mesh_row(sv.chunks, 3 * i + 3), B_in = mesh_row(sv.chunks, 3 * i + 4), lk_in = mesh_row(sv.chunks, 3 * i + 5);
		const float4 A_out = mesh_row(sv.chunks, 3 * i_out), B_out = mesh_row(sv.chunks, 3 * i_out + 1), lk_out = mesh_row(sv.chunks, 3 * i_out + 2);
		if(sv.tri_work) n_cull += (uint32_t) __popcll(__ballot(true));
		const bool enter = __any(entry_may_hold_nearer<CONES>(r, dd, A, B, b.t));
		const int count = __float_as_int(lk.z);
		if(enter && count > 0)
		{
			const int c0 = __float_as_int(lk.y), c1 = c0 + count;
			for(int c = c0; c < c1; c++)
			{
				if(sv.tri_work) n_cull += (uint32_t) __popcll(__ballot(true));
				const bool mine = entry_may_hold_nearer<CONES>(r, dd, mesh_row(chunk_ent, 2 * c), mesh_row(chunk_ent, 2 * c + 1), b.t);
				if(__any(mine))
				{
					const int i0 = c * sv.chunk, i1 = (i0 + sv.chunk < sv.nt) ? i0 + sv.chunk : sv.nt;
					if(sv.tri_work) n_tri += (uint32_t) __popcll(__ballot(mine)) * (uint32_t) (i1 - i0);
					for(int k = i0; k < i1; k++) tri_consider(r, mine, ld3(mesh_row(sv.tris, 3 * k)), mesh_row(sv.tris, 3 * k + 1), mesh_row(sv.tris, 3 * k + 2), k, from_tri, b);
				}
			}
		}
		i = enter ? i + 1 : i_out;
		A = enter ? A_in : A_out;
		B = enter ? B_in : B_out;
		lk = enter ? lk_in : lk_out;
	}
	if(sv.tri_work) tri_work_add(sv, n_cull, n_tri);
}

SKR_DEV void closest_triangle(const SceneView &sv, const RayConst &r, int from_tri, TriBest &b)
{
	if(sv.nchunks > 0)
	{
		if(sv.cones) tree_walk_closest<true>(sv, r, from_tri, b);
		else tree_walk_closest<false>(sv, r, from_tri, b);
		return;
	}
	for(int k = 0; k < sv.nt; k++) tri_consider(r, true, ld3(mesh_row(sv.tris, 3 * k)), mesh_row(sv.tris, 3 * k + 1), mesh_row(sv.tris, 3 * k + 2), k, from_tri, b);
}

// ---- triangle shadows (include/skr.h skr_scene_set_triangle_shadows): does a triangle stand between a hit and a light ----
// The NR shadow rays of one lane (the lights of a pair): they start at the same o = P + 1e-6, the origin the sphere test used.
template <int NR>
struct ShadowRays {
	f3 o;
	f3 d[NR];       // L, the bits the sphere test used
	float tmax[NR]; // |Lp - P| for a point light, +inf for a directional one
	bool live[NR];  // the light is not yet known to be dark: the ray is still tested (false on return: a triangle occludes it, or it was dark before)
	int own;        // file index of the triangle being shaded (it casts no shadow on itself), -1 at a sphere hit
};

// the rule for one (ray, triangle): utils.h:181-213 accepts, 0 < t < tmax, not the lane's own triangle (NaN t: no occluder)
SKR_DEV bool shadow_triangle_hit(f3 o, f3 d, f3 v0, f3 e1, f3 e2, int file, int own, float tmax)
{
	float t;
	return triangle_hit(o, d, v0, e1, e2, t) && t > 0.0f && t < tmax && file != own;
}

// The shadow visitor of mesh_walk() for a lane's NR rays: every entry that is loaded is tested against all of them (the walk is bound
// by its scalar loads, which the rays of a pair share).  A ray leaves at its first occluder, the wave when no ray of any lane is live.
// The line test only: the tree proves nothing about the segment between o and the light.  Without a tree (SKR_NO_CULL, a ray that
// starts outside the tree's ball) every triangle is tested; both give the same answers.
template <int NR>
SKR_DEV void shadow_triangles(const SceneView &sv, ShadowRays<NR> &s)
{
	static_assert(NR <= 2, "a ray is a bit of the masks lanes_of() counts: two per lane");
	auto live = [&]
	{
		uint32_t m = 0;
#pragma unroll
		for(int k = 0; k < NR; k++) m |= s.live[k] ? 1u << k : 0u;
		return m;
	};
	auto tri = [&](const float4 n0, const float4 n1, const float4 n2, int, uint32_t mine)
	{
		const f3 v0 = ld3(n0), e1 = ld3(n1), e2 = ld3(n2);
		const int file = __float_as_int(n1.w);
#pragma unroll
		for(int k = 0; k < NR; k++)
			if((mine >> k & 1u) && s.live[k] && shadow_triangle_hit(s.o, s.d[k], v0, e1, e2, file, s.own, s.tmax[k])) s.live[k] = false;
	};
	if(sv.nchunks > 0)
		mesh_instance(sv, [&](auto cones, auto count)
		{
			constexpr bool CONES = decltype(cones)::value;
			RayConst r[NR];
			float dd[NR];
#pragma unroll
			for(int k = 0; k < NR; k++)
			{
				r[k] = make_ray(s.o, s.d[k]);
				dd[k] = dot3(s.d[k], s.d[k]);
			}
			mesh_walk<decltype(count)::value>(sv, live, [&](const float4 A, const float4 B)
			{
				uint32_t m = 0;
#pragma unroll
				for(int k = 0; k < NR; k++) m |= (s.live[k] && line_touches<CONES>(r[k], dd[k], A, B)) ? 1u << k : 0u;
				return m;
			}, tri);
		});
	else mesh_all(sv, live, tri);
}

// ---- --legacy-reflect: the leaf functions of raytrace.h:45-103 ----
// blinn_phong.h:156-184 (its unqualified sqrt is ::sqrt(double); powf(x, 2.0f) == x * x; utils.h:132-146 clamp)
SKR_DEV float legacy_fresnel(f3 dir, f3 N, float mat_ior)
{
	float cos_internal = dot3(dir, N);
	cos_internal = cos_internal < -1.0f ? -1.0f : (cos_internal > 1.0f ? 1.0f : cos_internal);
	float et = 1.0f, ior = mat_ior;
	if(cos_internal > 0)
	{
		const float t = et;
		et = ior;
		ior = t;
	}
	const float sint = (float) ((double) sk_divf(et, ior) * sqrt((double) max0(1.0f - cos_internal * cos_internal)));
	if(sint >= 1.0f) return 1.0f;
	const float cos_theta = (float) sqrt((double) max0(1 - sint * sint));
	cos_internal = __builtin_fabsf(cos_internal);
	const float Rs = sk_divf((ior * cos_internal) - (et * cos_theta), (ior * cos_internal) + (et * cos_theta));
	const float Rp = sk_divf((et * cos_internal) - (ior * cos_theta), (ior * cos_internal) + (et * cos_theta));
	return sk_divf(Rs * Rs + Rp * Rp, 2.0f);
}

// blinn_phong.h:143-153 refraction(): (0,0,0) on total internal reflection
SKR_DEV f3 legacy_refraction_dir(f3 d, f3 N, float mat_ior)
{
	const float dn = dot3(d, N);
	const float k = 1.0f - (mat_ior * mat_ior) * (1.0f - dn * dn);
	return (k < 0.0f) ? mk3(0, 0, 0) : (d * mat_ior - N * (mat_ior * dn + sk_sqrtf(k)));
}
// blinn_phong.h:137-140 reflect_direction(): the LIGHT direction mirrored at the normal
SKR_DEV f3 legacy_reflect_dir(f3 L, f3 N) { return normalize3(L - N * (2.0f * dot3(L, N))); }

SKR_DEV uint32_t wave_sum(uint32_t v)
{
#pragma unroll
	for(int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}


} // namespace
