// The ray queries (include/skr.h skr_trace_rays, skr_camera_rays; DESIGN.md "Ray queries"): caller-supplied rays traced against the
// scene a renderer holds, by the renderer's own closest-hit rule — the sphere search of closest_sphere() (binary32 brackets, the
// binary64 root only where they cannot decide) and the closest-hit walk of --shade-triangles (closest_triangle()).  One lane per ray,
// 256-thread workgroups, a ray read as two float4 and a result written as two.  No LDS: the sphere rows come through the scalar
// cache (sphere_rows), the mesh rows likewise (mesh_row).
//
// Culling.  The renderer's chunk tree holds for rays that start at the camera or on a sphere.  Query rays start anywhere, so the
// scene carries a second tree built for rays that start anywhere in a ball around the scene (scene_trees.cpp trace_chunks), one set
// per bound on |d| like the renderer's.  A wave whose live rays all start at the scene camera bit for bit walks the renderer's set
// of the smallest bound above every lane's |d| (as a shading query's camera wave does); one whose live rays all start
// inside the ball walks the trace tree's; any other wave tests every triangle.  Either way every lane gets the exact answer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "wave_common.h"

namespace {

// The scene view of one wave: the tree pick_query_tree chooses for it (wave-uniform decision) — the renderer's where every live lane
// starts at the scene camera, else the trace tree where every live lane starts in its ball — or no tree.
template <bool TRI>
SKR_DEV SceneView trace_view(const TraceScene &s, bool live, f3 o, f3 d)
{
	SceneView sv{};
	sv.geom = s.geom; // (closest_sphere_exact's rows: HBM here)
	sv.geom_u = s.geom;
	sv.ns = s.ns;
	sv.tris = s.tris;
	sv.nt = TRI ? s.nt : 0;
	sv.chunks = s.trees.tree;
	sv.nchunks = 0;
	sv.chunk = s.chunk;
	sv.cones = s.trees.trace_cones;
	sv.tri_work = nullptr; // a query counts nothing
	if(TRI) pick_query_tree(sv, s.trees, s.cam, false, live, o, d);
	return sv;
}

// Any accepted sphere with t < tmax.  A bracket wholly below tmax decides the lane at once; one that straddles tmax is settled by
// the exact root (the bracket holds it: lo <= t <= hi).  A lane stops testing once it is decided, the wave once every lane is.
SKR_DEV bool any_sphere_before(const SceneView &sv, const RayConst &r, float tmax)
{
	const RayFilt f = make_filt(r.d);
	bool occ = false;
	table_rows<SKR_SPHERE_TRIP>(sv.geom_u, sv.ns, [&](const float4 g, int)
	{
		float lo, hi, b, D;
		if(!occ && sphere_bracket(r.o, r.d, f, g, lo, hi, b, D))
		{
			if(hi < tmax) occ = true;
			else if(lo < tmax) occ = bracket_t(f.two_a, lo, hi, b, D) < tmax;
		}
	}, [&] { return !__all(occ); });
	return occ;
}

SKR_DEV float4 sphere_ball_of(const SphereTree &st) { return st.ball; }

// any_sphere_before() on the sphere tree: every sphere the lane's line may touch, in the tree's order — the answer is a
// disjunction of per-sphere decisions, each of them exact, so the order does not matter.  A lane stops wanting entries once it is decided.
// A wave with a lane the tree does not hold for (outside the ball, a direction that is not finite) runs the loop over every sphere.
SKR_DEV bool any_sphere_before_tree(const SphereTree &st, const SceneView &sv, const RayConst &r, float tmax)
{
	const float dd = r.two_a * 0.5f;
	if(!st.cull || !__all(stree_lane_fits(st, r.o, dd))) return any_sphere_before(sv, r, tmax);
	const RayFilt f = make_filt(r.d);
	bool occ = false;
	stree_walk<false>(st, [&] { return occ ? 0u : 1u; },
		[&](const float4 A, float kappa, int) { return (!occ && sphere_entry_touched(r.o, r.d, dd, A, kappa)) ? 1u : 0u; },
		[&](const float4 g, int, uint32_t mine)
		{
			float lo, hi, b, D;
			if(mine && !occ && sphere_bracket(r.o, r.d, f, g, lo, hi, b, D))
			{
				if(hi < tmax) occ = true;
				else if(lo < tmax) occ = bracket_t(f.two_a, lo, hi, b, D) < tmax;
			}
		});
	return occ;
}

// triangle `slot` accepted with 0 < t < tmax, not the ray's own
SKR_DEV bool tri_before(const RayConst &r, const SceneView &sv, int slot, float tmax, int ignore)
{
	const float4 n1 = mesh_row(sv.tris, 3 * slot + 1);
	float t;
	return triangle_hit(r.o, r.d, ld3(mesh_row(sv.tris, 3 * slot)), ld3(n1), ld3(mesh_row(sv.tris, 3 * slot + 2)), t) && t > 0.0f && t < tmax &&
		   __float_as_int(n1.w) != ignore;
}

// Any accepted triangle with t < tmax: the walk of tree_walk_closest() with the running best fixed at tmax (an entry that can only
// hold hits behind tmax is skipped), a lane done at its first hit, the wave at the first chunk after which every lane is.
// shade_common.h mesh_walk() written out by hand: as its visitor the any-hit queries on dragon.scn took 2.85 against 2.39 ms for
// camera rays and 34.4 against 25.8 ms for 2^22 random rays (with entries and triangles asked for one ahead 2.60 and 31.2 ms).
template <bool CONES>
SKR_DEV bool tree_walk_any(const SceneView &sv, const RayConst &r, float tmax, int ignore, bool hit)
{
	const float dd = r.two_a * 0.5f;
	int i = 0;
	const float4 *chunk_ent = sv.chunks + 3 * (sv.nchunks + 1);
	float4 A = mesh_row(sv.chunks, 0), B = mesh_row(sv.chunks, 1), lk = mesh_row(sv.chunks, 2);
	while(i < sv.nchunks)
	{
		const int i_out = __float_as_int(lk.x);
		const float4 A_in = mesh_row(sv.chunks, 3 * i + 3), B_in = mesh_row(sv.chunks, 3 * i + 4), lk_in = mesh_row(sv.chunks, 3 * i + 5);
		const float4 A_out = mesh_row(sv.chunks, 3 * i_out), B_out = mesh_row(sv.chunks, 3 * i_out + 1), lk_out = mesh_row(sv.chunks, 3 * i_out + 2);
		const bool enter = __any(!hit && entry_may_hold_nearer<CONES>(r, dd, A, B, tmax));
		const int count = __float_as_int(lk.z);
		if(enter && count > 0)
		{
			const int c0 = __float_as_int(lk.y), c1 = c0 + count;
			for(int c = c0; c < c1; c++)
			{
				const bool mine = !hit && entry_may_hold_nearer<CONES>(r, dd, mesh_row(chunk_ent, 2 * c), mesh_row(chunk_ent, 2 * c + 1), tmax);
				if(__any(mine))
				{
					const int k0 = c * sv.chunk, k1 = (k0 + sv.chunk < sv.nt) ? k0 + sv.chunk : sv.nt;
					for(int k = k0; k < k1; k++)
						if(mine && !hit && tri_before(r, sv, k, tmax, ignore)) hit = true;
				}
			}
			if(__all(hit)) break;
		}
		i = enter ? i + 1 : i_out;
		A = enter ? A_in : A_out;
		B = enter ? B_in : B_out;
		lk = enter ? lk_in : lk_out;
	}
	return hit;
}

// (any_triangle_closer() is not this: it keeps the reference's missing t > 0 test and has no ray of its own to ignore)
SKR_DEV bool any_triangle_before(const SceneView &sv, const RayConst &r, float tmax, int ignore, bool hit)
{
	if(__all(hit)) return hit;
	if(sv.nchunks > 0) return sv.cones ? tree_walk_any<true>(sv, r, tmax, ignore, hit) : tree_walk_any<false>(sv, r, tmax, ignore, hit);
	for(int k = 0; k < sv.nt; k++)
	{
		if(!hit && tri_before(r, sv, k, tmax, ignore)) hit = true;
		if((k & 7) == 7 && __all(hit)) break;
	}
	return hit;
}

} // namespace

// SPH / TRI: the scene has spheres / triangles (the other search is compiled out, as skr_direct_kernel's sphere-free instance);
// ANY: SKR_TRACE_ANY_HIT.  Lanes past n trace a ray that can hit nothing (tmax = -inf) so that the wave-wide walks stay whole.
// ST: an empty pack — the sphere searches are the loops over every sphere — or one SphereTree: they are the tree's walks (the renderer's
// scene has the sphere tree switched on, include/skr.h skr_scene_set_sphere_tree).  The body of both kernels below.
template <bool SPH, bool TRI, bool ANY, typename... ST>
SKR_DEV void ray_query(const TraceScene &s, const float4 *rays, uint32_t n, void *out, const ST &...st)
{
	constexpr bool STREE = sizeof...(ST) > 0;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	const bool valid = i < n;
	float4 ra = make_float4(s.trees.ball.x, s.trees.ball.y, s.trees.ball.z, -__builtin_inff()), rb = make_float4(0.0f, 0.0f, 1.0f, __int_as_float(-1));
	if constexpr(STREE)
	{ // (a lane past n starts inside the sphere ball, so it never sends its wave to the loop; pick_query_tree ignores lanes that are not live,
	  // so it need not lie in the trace ball — and a scene without a mesh has none)
		const float4 sb = sphere_ball_of(st...);
		ra = make_float4(sb.x, sb.y, sb.z, -__builtin_inff());
	}
	if(valid)
	{
		ra = rays[2 * (size_t) i];
		rb = rays[2 * (size_t) i + 1];
	}
	const f3 o = mk3(ra.x, ra.y, ra.z), d = mk3(rb.x, rb.y, rb.z);
	const float tmax = ra.w;
	const int ignore = __float_as_int(rb.w);
	const RayConst r = make_ray(o, d);
	const SceneView sv = trace_view<TRI>(s, valid, o, d);
	if constexpr(ANY)
	{
		bool occ = false;
		if constexpr(STREE) occ = any_sphere_before_tree(st..., sv, r, tmax);
		else if(SPH) occ = any_sphere_before(sv, r, tmax);
		if(TRI) occ = any_triangle_before(sv, r, tmax, ignore, occ);
		if(valid) reinterpret_cast<int32_t *>(out)[i] = occ ? 1 : 0;
	}
	else
	{
		float ts = __builtin_inff();
		int sph = -1;
		if constexpr(STREE) sph = stree_closest(st..., sv, r, ts);
		else if(SPH) sph = closest_sphere(sv, r, ts);         // raytrace.h:152-165
		TriBest tb{__builtin_fminf(ts, tmax), -1, -1}; // the walk is cut at the sphere (it wins a tie) or at tmax, whichever is nearer
		if(TRI) closest_triangle(sv, r, ignore, tb);
		int kind = 0, index = -1;
		float t = __builtin_inff();
		f3 N = mk3(0.0f, 0.0f, 0.0f);
		if(TRI && tb.slot >= 0 && tb.t < tmax)
		{ // render_generic.hip skr_gactivate_kernel: the geometric normal turned against the ray
			kind = 2;
			index = tb.file;
			t = tb.t;
			N = normalize3(cross3(ld3(sv.tris[3 * tb.slot + 1]), ld3(sv.tris[3 * tb.slot + 2])));
			if(dot3(N, d) > 0.0f) N = mk3(-N.x, -N.y, -N.z);
		}
		else if(SPH && sph >= 0 && ts < tmax)
		{ // raytrace.h:204-205 as the level pipelines form it
			kind = 1;
			index = sph;
			t = ts;
			const f3 P = o + d * ts;
			N = normalize3(P - ld3(sv.geom[sph]));
		}
		if(valid)
		{
			float4 *h = reinterpret_cast<float4 *>(out) + 2 * (size_t) i;
			h[0] = make_float4(t, __int_as_float(kind), __int_as_float(index), N.x);
			h[1] = make_float4(N.y, N.z, 0.0f, 0.0f);
		}
	}
}

template <bool SPH, bool TRI, bool ANY>
__global__ __launch_bounds__(256) void skr_ray_query_kernel(const TraceScene s, const float4 *rays, uint32_t n, void *out)
{
	ray_query<SPH, TRI, ANY>(s, rays, n, out);
}
// the instances with the sphere tree's walks (a scene with the switch on has spheres)
template <bool TRI, bool ANY>
__global__ __launch_bounds__(256) void skr_ray_query_tree_kernel(const TraceScene s, const float4 *rays, uint32_t n, void *out, const SphereTree st)
{
	ray_query<true, TRI, ANY>(s, rays, n, out, st);
}

// The primary rays of one AA sample of a frame (include/skr.h skr_camera_rays): one lane per pixel, the direction of primary_ray().
__global__ __launch_bounds__(256) void skr_camera_ray_kernel(const RenderParams p, float4 *rays)
{
	const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	const uint32_t w = (uint32_t) p.width;
	if(i >= (uint64_t) w * (uint32_t) p.height) return;
	const uint32_t y = (uint32_t) (i / w), x = (uint32_t) (i - (uint64_t) y * w);
	f3 dir;
	primary_ray(p, (int) x, y, y * w + x, p.aa_index, dir);
	rays[2 * i] = make_float4(p.cam_pos.x, p.cam_pos.y, p.cam_pos.z, __builtin_inff());
	rays[2 * i + 1] = make_float4(dir.x, dir.y, dir.z, __int_as_float(-1));
}

// The same under a lens (include/skr.h skr_scene_set_lens): (o', d') of wave_common.h lens_ray.  A kernel of its own: the pinhole's keeps its code.
__global__ __launch_bounds__(256) void skr_camera_ray_lens_kernel(const RenderParams p, float4 *rays, const Lens lens)
{
	const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	const uint32_t w = (uint32_t) p.width;
	if(i >= (uint64_t) w * (uint32_t) p.height) return;
	const uint32_t y = (uint32_t) (i / w), x = (uint32_t) (i - (uint64_t) y * w);
	f3 dir, o;
	primary_ray(p, (int) x, y, y * w + x, p.aa_index, dir);
	lens_ray(p, lens, y * w + x, p.aa_index, dir, o, dir);
	rays[2 * i] = make_float4(o.x, o.y, o.z, __builtin_inff());
	rays[2 * i + 1] = make_float4(dir.x, dir.y, dir.z, __int_as_float(-1));
}

hipError_t skr_launch_trace(const TraceScene &s, const float4 *rays, uint32_t n, bool any_hit, void *out, hipStream_t stream, const SphereTree *st)
{
	const dim3 grid((unsigned) (((uint64_t) n + 255) / 256)), block(256);
	const bool sph = s.ns > 0, tri = s.nt > 0;
	if(st && sph)
	{
		if(tri && any_hit) hipLaunchKernelGGL((skr_ray_query_tree_kernel<true, true>), grid, block, 0, stream, s, rays, n, out, *st);
		else if(tri) hipLaunchKernelGGL((skr_ray_query_tree_kernel<true, false>), grid, block, 0, stream, s, rays, n, out, *st);
		else if(any_hit) hipLaunchKernelGGL((skr_ray_query_tree_kernel<false, true>), grid, block, 0, stream, s, rays, n, out, *st);
		else hipLaunchKernelGGL((skr_ray_query_tree_kernel<false, false>), grid, block, 0, stream, s, rays, n, out, *st);
		return hipGetLastError();
	}
#define SKR_TRACE_LAUNCH(S, T)                                                                                                  \
	do                                                                                                                          \
	{                                                                                                                           \
		if(any_hit) hipLaunchKernelGGL((skr_ray_query_kernel<S, T, true>), grid, block, 0, stream, s, rays, n, out);                \
		else hipLaunchKernelGGL((skr_ray_query_kernel<S, T, false>), grid, block, 0, stream, s, rays, n, out);                      \
	} while(0)
	if(sph && tri) SKR_TRACE_LAUNCH(true, true);
	else if(sph) SKR_TRACE_LAUNCH(true, false);
	else if(tri) SKR_TRACE_LAUNCH(false, true);
	else SKR_TRACE_LAUNCH(false, false);
#undef SKR_TRACE_LAUNCH
	return hipGetLastError();
}

hipError_t skr_launch_camera_rays(const RenderParams &p, float4 *rays, hipStream_t stream, const Lens *lens)
{
	const uint64_t n = (uint64_t) (uint32_t) p.width * (uint32_t) p.height;
	if(lens) hipLaunchKernelGGL(skr_camera_ray_lens_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, p, rays, *lens);
	else hipLaunchKernelGGL(skr_camera_ray_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, p, rays);
	return hipGetLastError();
}
