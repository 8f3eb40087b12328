// The general level pipeline: shade() (src/raytrace.h:139-227) with every kind of child ray it can spawn, cut at every level of the
// tree, for any --depth (main.cpp:318-329 accepts any positive depth).  One lane per RAY — not per sibling pair, no state carried
// between kernels but the tables — so that the modes the pair kernels of render_nodes.hip do not know fit in:
//
//   * triangle meshes under --gillum (HEAD semantics: an accepted triangle nearer than the closest sphere blackens the sample,
//     raytrace.h:171-186, :221-224) — one wave-level walk of the culling tree per 64 rays;
//   * --shade-triangles: a triangle is a surface; its hit is a node like a sphere's, its --gillum children do not
//     test the triangle they start on;
//   * --legacy-reflect: every shaded sphere hit has, besides its N --gillum children, two children per light —
//     the refraction and the reflection ray of raytrace.h:54-99 — from the hit point itself;
//   * --gillum beyond 256 children per node;
//   * scenes with fog volumes (--scn-fog, DESIGN.md "Spherical fog"): the fog term of every lit point light at a sphere hit.
//
// Levels.  Level 0 is the camera: one root per pixel of the band with ONE child, the primary ray (main.cpp:140-182).  A hit of level k
// (k >= 1) is a node of level k; it is shaded when its record is activated and, while k < --depth, its A = N + 2 L children are
// the rays of level k + 1 (child c < N: the c-th --gillum ray; child N + 2 l: the refraction ray of light l; N + 2 l + 1: its
// reflection ray — the numbering of the counter RNG's node ids, DESIGN.md "Counter RNG").  Kernels, in launch order, per level:
//
//   skr_gtrace_kernel     one lane per child ray of the level above: the ray, the closest sphere, the triangles; per wave (64 rays) a
//                         32-byte header — first record, ballot of the rays that hit a surface, ballot of the rays a triangle
//                         blackened — and per hit a 32-byte record {parent, surface, child, t, d} appended to one of 64 regions
//   skr_gactivate_kernel  one lane per record: the hit is shaded (raytrace.h:194-207) and becomes a node (80 bytes); a hit of the
//                         last level, whose children are shade(depth 0) == 0, is finished here
//   skr_gfinalize_kernel  deepest level first, one lane per node: its children's values in the reference's order —
//                         refraction_colour = fr * shade() (an assignment: the last light's stays), reflection_colour += (1 - fr) *
//                         specular * shade() (:70-76), total += r1 * shade() / pdf (:130), (direct / pi + 2 indirect) * kd (:213) —;
//                         level 0: the pixel
//
// Every float operation and every order of summation is the reference's; the image is bit-identical to the oracle's
// (tests/test_gpu_parity.py, test_shade_triangles.py, test_legacy_reflect.py run every mode through it).
//
// Shading queries (include/skr.h skr_shade_rays).  The ray source of level 1 and the sink of level 0 are a compile-time
// parameter of the three kernels: without a ShadeRays in the pack `Q...` the camera and the image (frames), with one the caller's rays
// and their float[n][3] values.  Every level below level 1 works on any ray unchanged.
//
// Instances.  What a launch switches on (launch.h GenericFeatures) reaches the kernels as the pack `Q...` of arguments behind
// RenderParams, each feature a type of its own, in the one order with_pack (below) writes down; a kernel asks the pack for a type
// (pack_has, pick).  A feature that is off is not in the pack, which leaves that instance's argument block, and so its code, as it was.
//
// A lens (include/skr.h skr_scene_set_lens).  With a Lens in the pack the camera rays of level 1 are (o', d') of
// wave_common.h lens_ray: the trace kernel forms them and picks the tree of each wave as for query rays (the rays do not start at the
// scene camera), the activate kernel forms o' again for the hit point.  Every level below works on any ray unchanged.
//
// Motion (include/skr.h skr_scene_set_sphere_velocities).  With a Motion in the pack every lane forms the shutter time of
// its sample from the pixel word of its tree's root (wave_common.h shutter_time) and searches the spheres where they are at that time
// (shade_common.h MovingCentres): the closest-hit search of the trace kernel, the normal and the shadow rays of the activate kernel.
// Such an instance consults no table built from the centres at rest — its view of the scene has no shadow masks, and this pipeline reads
// neither GI masks nor the camera's (e, c) rows — and, where its rays start on displaced surfaces (below level 1), picks the tree of
// each wave as for query rays.
//
// The environment (include/skr.h skr_scene_set_environment).  Only the finalize kernel decides a miss, and its tables
// carry nothing for one: with an EnvMap in the pack it forms the missed ray's direction again, by the function that formed it for the
// trace kernel — child_of on its own node below level 0, primary_ray (then lens_ray: a Lens rides behind the EnvMap) or the caller's d at
// level 0 — and returns wave_common.h env_lookup of it.  Trace and activate instances, records and nodes are as they were.
//
// Textures (include/skr.h skr_scene_add_texture).  With a Textures in the pack — the last argument, behind everything —
// the two places that take a node's material rows, the activate kernel and node_value, hand them to textured_material with the node's
// shading normal: at a sphere with a texture kd and the ambient row are multiplied by wave_common.h env_lookup of N on that texture.
// The finalize kernel finds N in the node's rows with the bits the activate kernel had.  Trace instances, records and nodes are as they
// were.
//
// Emission (include/skr.h skr_scene_set_sphere_emission).  With an Emission in the pack — behind the Textures such a
// launch always carries — node_value adds the sphere's row to the value it returns: the activate kernel's last-level arm and the
// finalize kernel, nothing else.  Trace instances, records and nodes are as they were.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "launch.h"
#include "wave_common.h"

namespace {

constexpr uint32_t SURF_TRI = 0x80000000u; // surface code: a sphere index, or SURF_TRI | the triangle's slot in tris[]
constexpr int GNODE_ROWS = 5;              // float4 per node: [P.xyz N.x] [N.yz d.x d.y] [d.z surface pixel node-id] [direct.xyz fr] [own record, file index of a triangle (-1), -, -]
constexpr int GREC_ROWS = 2;               // float4 per record: [parent surface child t] [d.xyz -]
constexpr int GHDR_ROWS = 2;               // uint4 per trace wave: [first record, -, -, -] [hit ballot lo hi, black ballot lo hi]

struct GChild { // one child ray of a node, as the trace kernel forms it and the finalize kernel weighs it
	bool exists;
	f3 o, d;
	int from_tri; // --shade-triangles: the file index of the triangle the ray starts on (-1: none)
};

struct GNode {
	f3 P, N, d, direct;
	float fr;
	uint32_t surf, pixel, node_id, rec;
	int file;
};

SKR_DEV GNode load_node(const float4 *rows)
{
	const float4 a = rows[0], b = rows[1], c = rows[2], e = rows[3], f = rows[4];
	GNode n;
	n.P = mk3(a.x, a.y, a.z);
	n.N = mk3(a.w, b.x, b.y);
	n.d = mk3(b.z, b.w, c.x);
	n.surf = __float_as_uint(c.y);
	n.pixel = __float_as_uint(c.z);
	n.node_id = __float_as_uint(c.w);
	n.direct = mk3(e.x, e.y, e.z);
	n.fr = e.w;
	n.rec = __float_as_uint(f.x);
	n.file = (int) __float_as_uint(f.y);
	return n;
}

// the material rows of a surface: {La * ka, power}, kd, {ks, ior}
SKR_DEV void surface_material(const SceneView &sv, const RenderParams &p, uint32_t surf, float4 &ambp, f3 &kd, float4 &ks4)
{
	if(surf & SURF_TRI)
	{
		const uint32_t slot = surf & ~SURF_TRI;
		ambp = p.tri_mats[3 * slot];
		kd = ld3(p.tri_mats[3 * slot + 1]);
		ks4 = p.tri_mats[3 * slot + 2];
	}
	else
	{
		ambp = sv.amb[surf];
		kd = ld3(sv.kd[surf]);
		ks4 = sv.ks[surf];
	}
}

// tex_k(N) of include/skr.h skr_scene_add_texture on the texture whose texels start at row `first` and whose edge is E >= 1: the
// environment's lookup of N — env_taps and the four clamped gathers — with (1, 1, 1) where its first step fails
SKR_DEV f3 texture_colour(const Textures &tx, uint32_t first, uint32_t E, f3 N)
{
	return env_lookup(EnvMap{tx.texels + first, (int32_t) E}, N, mk3(1, 1, 1));
}

// The one statement of the texture rule: the material rows of a node on sphere `surf` with the shading normal N.  kd' = kd c and
// ambp' = {ambp.xyz c, ambp.w}, one multiply per component; a triangle, and a sphere without a texture, keep their rows.
SKR_DEV void textured_material(const Textures &tx, uint32_t surf, f3 N, float4 &ambp, f3 &kd)
{
	if(surf & SURF_TRI) return;
	const uint2 row = tx.rows[surf];
	if(row.y == 0u) return;
	const f3 c = texture_colour(tx, row.x, row.y, N);
	kd = kd * c;
	ambp = make_float4(ambp.x * c.x, ambp.y * c.y, ambp.z * c.z, ambp.w);
}
// what node_value is handed where the launch has no textures: nothing, and no code
struct NoTextures {
	static constexpr bool on = false;
};
struct WithTextures {
	static constexpr bool on = true;
	const Textures &tx;
};

// The one statement of the emission rule: what shade() returns at surface `surf`, v the value it had.  v + e_i at sphere i, one add per
// component; a triangle has no emission.
SKR_DEV f3 emitted(const Emission &em, uint32_t surf, f3 v)
{
	if(surf & SURF_TRI) return v;
	const float4 e = em.rows[surf];
	return mk3(v.x + e.x, v.y + e.y, v.z + e.z);
}
// what node_value is handed where the launch has no emission: nothing, and no code
struct NoEmission {
	static constexpr bool on = false;
};
struct WithEmission {
	static constexpr bool on = true;
	const Emission &em;
};

// does the node spawn the legacy children (raytrace.h:52: a specular colour other than (0,0,0); only a sphere hit has these terms)
SKR_DEV bool legacy_children(const RenderParams &p, const SceneView &sv, uint32_t surf)
{
	if(!p.legacy_reflect || (surf & SURF_TRI)) return false;
	const float4 ks = sv.ks[surf];
	return ks.x != 0.0f || ks.y != 0.0f || ks.z != 0.0f;
}

// child c of node n (raytrace.h:117-131 for c < N; :54-99 for the two rays of light (c - N) / 2)
SKR_DEV GChild child_of(const SceneView &sv, const RenderParams &p, const GNode &n, uint32_t c)
{
	GChild ch;
	ch.from_tri = -1;
	ch.o = n.P;
	ch.d = mk3(0, 0, 1);
	const uint32_t N = (uint32_t) (p.monte_carlo ? p.num_path_traces : 0);
	if(c < N)
	{
		ch.exists = true;
		f3 nt, nb;
		tangent_basis(n.N, nt, nb);
		uint32_t rnd[4];
		philox4x32(n.pixel, p.aa_index, n.node_id, c >> 1, p.seed_lo, p.seed_hi, rnd);
		const float r1 = u31_to_unit(rnd[2 * (c & 1u)]), r2 = u31_to_unit(rnd[2 * (c & 1u) + 1]);
		ch.d = gi_direction(r1, r2, n.N, nt, nb);
		ch.o = add_scalar(n.P, 0.00001f);
		ch.from_tri = n.file;
		return ch;
	}
	const uint32_t l = (c - N) >> 1;
	const bool reflection = (c - N) & 1u;
	ch.exists = legacy_children(p, sv, n.surf) && (reflection || n.fr < 1);
	if(ch.exists)
	{
		if(reflection) ch.d = legacy_reflect_dir(light_term(sv, (int) l, n.P).L, n.N);
		else ch.d = legacy_refraction_dir(n.d, n.N, sv.ks[n.surf].w);
	}
	return ch;
}

// the argument of type T in a kernel's pack, itself; T{} where the pack has none (such an instance never reads it)
template <typename T>
SKR_DEV T pick() { return T{}; }
template <typename T, typename U, typename... R>
SKR_DEV decltype(auto) pick(const U &u, const R &...rest)
{
	if constexpr(std::is_same<T, U>::value) return (u);
	else return pick<T>(rest...);
}
template <typename T, typename... Q>
constexpr bool pack_has = (std::is_same<T, Q>::value || ...);

// The scene of an instance with the sphere tree: the lights staged into LDS, the sphere rows and materials where they lie in HBM, in
// file order (surface codes are file indices) — surface_material, child_of and the fog term read them by per-lane index, and the
// loops over every sphere (a wave the tree does not hold for) by wave-uniform index.  No LDS need depends on the sphere count.
SKR_DEV SceneView stage_lights(const RenderParams &p, float4 *lds4, bool tris)
{
	for(int i = threadIdx.x; i < 2 * p.n_lights; i += 256) lds4[i] = p.lights[i];
	__syncthreads();
	return SceneView{p.sph_geom, p.sph_amb, p.sph_kd, p.sph_ks, lds4, p.tris, p.n_spheres, tris ? p.n_tris : 0, p.n_lights, p.tri_chunks, p.n_tri_chunks, p.tri_chunk_size,
					 p.tri_cones, p.tri_work, p.sph_geom, nullptr, 0.0f, 0u};
}
template <bool STREE>
SKR_DEV SceneView stage_for(const RenderParams &p, float4 *lds4)
{
	if constexpr(STREE) return stage_lights(p, lds4, true);
	else return stage_scene(p, lds4, true);
}

// The tree a wave of query rays walks (wave_common.h pick_query_tree): at level 1 the renderer's tree where every lane
// starts at the scene camera, else the trace tree where every lane starts in its ball; at a level below (origins on surfaces) the
// renderer's tree.
SKR_DEV void query_tree(SceneView &sv, const RenderParams &p, const ShadeRays &q, bool live, f3 o, f3 d)
{
	pick_query_tree(sv, q.trees, p.cam_pos, p.g_level != 1, live, o, d);
}

// Triangle shadows (include/skr.h skr_scene_set_triangle_shadows), what direct_light_of calls behind the sphere test of a
// pair of lights: a light the spheres left lit is dark if a triangle other than the lane's own accepts the shadow ray (the sphere test's
// o = P + 1e-6 and L) at 0 < t, for a point light also t < |Lp - P|.  The tree is the trace tree — shadow rays start on spheres AND
// on triangles, an origin class the renderer's tree is not built for — where every lane that still has a ray to test starts inside its
// ball (pick_query_tree's rule (b); |L| = 1: the first set); otherwise every triangle.
#ifndef SKR_SHADOW_PAIR_WALK
#define SKR_SHADOW_PAIR_WALK 1 // 1: one walk tests both rays of a pair of lights against every entry it loads; 0: one walk per light (DESIGN.md 8.9 has both times)
#endif
// ON = false means what shade_common.h NoTriangleShadows means, for an instance without the walk: nothing of it is called.  It exists beside
// NoTriangleShadows only so that the activate kernel can build either from the same three arguments without a constructor or a function in
// between — each of those moved instructions in instances that had none to move.
template <bool ON>
struct TriangleShadows {
	static constexpr bool on = ON;
	const SceneView &sv;
	const QueryTrees &trees;
	int own; // file index of the triangle being shaded, -1 at a sphere hit

	__device__ __forceinline__ float reach(int l, f3 P) const
	{ // blinn_phong.h's `distance` = length(Lp - P); a directional light has no far end
		const float4 lp4 = sv.lights[2 * l];
		return lp4.w != 0.0f ? __builtin_inff() : length3(ld3(lp4) - P);
	}
	template <int NR>
	__device__ __forceinline__ void walk(ShadowRays<NR> &s) const
	{ // (every lane of the wave that shades a hit arrives here: the choice of the tree and the walk are wave-wide)
		bool live = false, fits = true;
		constexpr float lim = (float) (4.0 * 4.0 * 0.998); // pick_query_tree's first bound
#pragma unroll
		for(int k = 0; k < NR; k++)
		{
			live = live || s.live[k];
			fits = fits && dot3(s.d[k], s.d[k]) < lim; // (NaN: no tree)
		}
		if(!__any(live)) return;
		const f3 e = s.o - mk3(trees.ball.x, trees.ball.y, trees.ball.z);
		SceneView w = sv;
		w.nchunks = 0;
		if(trees.trace && trees.nchunks > 0 && __all(!live || (fits && dot3(e, e) <= trees.ball.w * trees.ball.w)))
		{
			w.chunks = trees.trace;
			w.cones = trees.trace_cones;
			w.nchunks = trees.nchunks;
		}
		shadow_triangles<NR>(w, s);
	}
	__device__ __forceinline__ void operator()(f3 P, int i, bool second, f3 L0, f3 L1, bool &occ0, bool &occ1) const { lights(P, i, second ? i + 1 : i, second, L0, L1, occ0, occ1); }
	// the lights l0 and (second) l1, any two of the table (direct_light_cone walks a pair's one light inside its cone as a single)
	__device__ __forceinline__ void lights(f3 P, int l0, int l1, bool second, f3 L0, f3 L1, bool &occ0, bool &occ1) const { ends(P, second, L0, L1, reach(l0, P), reach(l1, P), occ0, occ1); }
	// two rays with the far ends the caller has (direct_light_cone<true>: the distance to a light's sample)
	__device__ __forceinline__ void ends(f3 P, bool second, f3 L0, f3 L1, float far0, float far1, bool &occ0, bool &occ1) const
	{
		const f3 o = add_scalar(P, 0.000001f);
#if SKR_SHADOW_PAIR_WALK
		ShadowRays<2> s{o, {L0, L1}, {far0, far1}, {!occ0, second && !occ1}, own};
		walk(s);
		occ0 = !s.live[0];
		if(second) occ1 = !s.live[1];
#else
		ShadowRays<1> s0{o, {L0}, {far0}, {!occ0}, own}, s1{o, {L1}, {far1}, {second && !occ1}, own};
		walk(s0);
		walk(s1);
		occ0 = !s0.live[0];
		if(second) occ1 = !s1.live[0];
#endif
	}
};

// shade_common.h SphereLoopShadows, built from what SphereTreeShadows is built from: likewise a duplicate kept for the instances' code alone
struct SphereLoops {
	static constexpr bool loops = true;
	const SphereTree &st; // (never read)
};

} // namespace

// =====================================================================================================================
// trace: one lane per child ray of the level above (level 1: the primary rays)
// =====================================================================================================================
template <typename... Q>
__global__ __launch_bounds__(256) void skr_gtrace_kernel(const RenderParams p, const Q... qs)
{
	constexpr bool RAYS = pack_has<ShadeRays, Q...>, STREE = pack_has<SphereTree, Q...>, LENS = pack_has<Lens, Q...>, MOTION = pack_has<Motion, Q...>;
	const ShadeRays q = pick<ShadeRays>(qs...);
	extern __shared__ __align__(16) unsigned char lds_raw[];
	float4 *lds4 = reinterpret_cast<float4 *>(lds_raw);
	const uint32_t A = p.g_arity; // children per node of the level above (1 at the camera level)
	const uint64_t n_rays = (uint64_t) *p.nd_count * A;
	if((uint64_t) blockIdx.x * 256u >= n_rays) return; // (uniform per workgroup)
	const SceneView sv = stage_for<STREE>(p, lds4);
	const int tid = threadIdx.x, lane = tid & 63;
	Counters cn{0, 0, 0};
	for(uint32_t blk = blockIdx.x; (uint64_t) blk * 256u < n_rays; blk += gridDim.x)
	{
		const uint32_t chunk = blk * 4u + (uint32_t) (tid >> 6);
		const uint64_t ri = (uint64_t) chunk * 64u + (uint32_t) lane;
		const bool valid = ri < n_rays;
		const uint32_t node = valid ? (uint32_t) (ri / A) : 0u, c = valid ? (uint32_t) (ri - (uint64_t) node * A) : 0u;
		GChild ch;
		ch.exists = false;
		ch.o = ch.d = mk3(0, 0, 1);
		ch.from_tri = -1;
		float tmax = __builtin_inff();
		uint32_t root = 0u; // MOTION: the pixel word of the ray's tree, what its shutter time is drawn from
		if(valid)
		{
			if(p.g_level == 1)
			{
				if constexpr(RAYS)
				{ // the caller's ray {o, tmax} {d, ignore_triangle} (include/skr.h skr_ray); ignore_triangle only where a ray can carry one
					if constexpr(MOTION) root = q.keys ? q.keys[q.ray0 + node] : q.ray0 + node; // (the activate kernel's n.pixel)
					const float4 ra = q.rays[2 * (size_t) (q.ray0 + node)], rb = q.rays[2 * (size_t) (q.ray0 + node) + 1];
					ch.exists = true;
					ch.o = mk3(ra.x, ra.y, ra.z);
					ch.d = mk3(rb.x, rb.y, rb.z);
					ch.from_tri = p.shade_triangles ? __float_as_int(rb.w) : -1;
					tmax = ra.w;
				}
				else
				{ // the camera: root `node` is pixel (x, row) of the band, its one child the primary ray (main.cpp:140-182)
					const uint32_t bw = (uint32_t) p.width, row = p.band_row0 + node / bw, x = node - (node / bw) * bw;
					const uint32_t y = image_row(p, row);
					ch.exists = y < (uint32_t) p.height;
					if(ch.exists)
					{
						ch.o = p.cam_pos;
						primary_ray(p, (int) x, y, y * bw + x, p.aa_index, ch.d);
						if constexpr(MOTION) root = y * bw + x;
						if constexpr(LENS) lens_ray(p, pick<Lens>(qs...), y * bw + x, p.aa_index, ch.d, ch.o, ch.d); // (o', d') of include/skr.h skr_scene_set_lens
					}
				}
			}
			else
			{
				const GNode pn = load_node(p.g_nodes_src + (size_t) node * GNODE_ROWS);
				ch = child_of(sv, p, pn, c);
				if constexpr(MOTION) root = pn.pixel;
			}
		}
		SceneView svw = sv;
		if constexpr(RAYS && MOTION) pick_query_tree(svw, q.trees, p.cam_pos, false, ch.exists, ch.o, ch.d); // (below level 1 too: origins on displaced surfaces)
		else if constexpr(RAYS) query_tree(svw, p, q, ch.exists, ch.o, ch.d);
		else if constexpr(MOTION) // level 1 starts at the scene camera and keeps the renderer's tree; below it the origins lie on displaced surfaces, which that tree is not built for
			if(p.g_level != 1) pick_query_tree(svw, pick<Motion>(qs...).trees, p.cam_pos, false, ch.exists, ch.o, ch.d);
		if constexpr(LENS) // level 1 starts on the lens, not at the scene camera: the tree of query rays; the levels below keep the renderer's
			if(p.g_level == 1) pick_query_tree(svw, pick<Lens>(qs...).trees, p.cam_pos, false, ch.exists, ch.o, ch.d);
		bool hit = false, black = false;
		uint32_t surf = 0;
		float t = 0.0f;
		if(ch.exists)
		{
			cn.rays++;
			const RayConst r = make_ray(ch.o, ch.d);
			float tmin;
			int sph; // raytrace.h:152-165
			if constexpr(STREE) sph = stree_closest(pick<SphereTree>(qs...), sv, r, tmin);
			else if constexpr(MOTION)
			{ // the spheres where they are at the sample's shutter time
				const Motion &mo = pick<Motion>(qs...);
				sph = closest_sphere(sv, r, tmin, MovingCentres{mo.vel, shutter_time(p, root, p.aa_index, mo.S)});
			}
			else sph = closest_sphere(sv, r, tmin);
			float tcut = tmin;
			if constexpr(RAYS)
			{ // include/skr.h skr_shade_rays `tmax`: the winner is cut where it lies at or beyond tmax (a triangle only wins below the cut)
				tcut = tmin < tmax ? tmin : tmax;
				if(!(tmin < tmax)) sph = -1;
			}
			if(p.shade_triangles)
			{
				TriBest b{tcut, -1, -1};
				if(svw.nt > 0) closest_triangle(svw, r, ch.from_tri, b);
				hit = sph >= 0 || b.slot >= 0;
				surf = b.slot >= 0 ? (SURF_TRI | (uint32_t) b.slot) : (uint32_t) sph;
				t = b.t;
			}
			else
			{
				black = svw.nt > 0 && any_triangle_closer(svw, r, tcut); // raytrace.h:171-186, :221-224
				hit = !black && sph >= 0;
				surf = (uint32_t) sph;
				t = tmin;
			}
		}
		// append the wave's hits to its region: rank by ballot, one atomic per wave
		const unsigned long long mh = __ballot(hit), mb = __ballot(black);
		const uint32_t region = chunk & (SKR_P1_REGIONS - 1u);
		const uint32_t nh = (uint32_t) __popcll(mh);
		uint32_t base = 0;
		if(nh != 0u)
		{
			if(lane == 0) base = atomicAdd(lc_count(p.rc_ctr, region), nh);
			base = (uint32_t) __builtin_amdgcn_readfirstlane((int) base);
		}
		const uint32_t rec_base = region * p.rc_cap + base;
		if(hit)
		{
			float4 *rec = p.rc + (size_t) (rec_base + (uint32_t) lanes_below(mh)) * GREC_ROWS;
			rec[0] = make_float4(__uint_as_float(node), __uint_as_float(surf), __uint_as_float(c), t);
			rec[1] = make_float4(ch.d.x, ch.d.y, ch.d.z, 0.0f);
		}
		if(lane == 0)
		{
			p.ixh[GHDR_ROWS * (size_t) chunk] = make_uint4(rec_base, 0u, 0u, 0u);
			p.ixh[GHDR_ROWS * (size_t) chunk + 1] = make_uint4((uint32_t) mh, (uint32_t) (mh >> 32), (uint32_t) mb, (uint32_t) (mb >> 32));
		}
	}
	add_counters(p, cn, (uint32_t) blockIdx.x * 4u + (uint32_t) (tid >> 6), lane);
}

// =====================================================================================================================
// activate: record -> node (raytrace.h:194-207); the last level's hits are finished here
// =====================================================================================================================
namespace {

// the value of a node whose children's values are known — or all (0,0,0): shade(depth 0), raytrace.h:142-145.  `value_of(c)`: child c.
// TX: the launch's textures (WithTextures), or none.  EM: its emission (WithEmission), or none: both returns go through emitted(), behind
// the multiply by kd (nothing here is contracted).  EM travels by value: an empty NoEmission is then no argument at all, and the
// instances without emission keep their instructions (by reference four activate instances had two loads change places)
template <typename F, typename TX = NoTextures, typename EM = NoEmission>
SKR_DEV f3 node_value(const SceneView &sv, const RenderParams &p, const GNode &n, F value_of, const TX &tex = TX(), EM emi = EM())
{
	float4 ambp, ks4;
	f3 kd;
	surface_material(sv, p, n.surf, ambp, kd, ks4);
	if constexpr(TX::on) textured_material(tex.tx, n.surf, n.N, ambp, kd);
	const uint32_t N = (uint32_t) (p.monte_carlo ? p.num_path_traces : 0);
	f3 direct = n.direct;
	if(p.legacy_reflect && !(n.surf & SURF_TRI))
	{ // raytrace.h:45-102
		f3 refraction_colour = mk3(0, 0, 0), reflection_colour = mk3(0, 0, 0);
		if(legacy_children(p, sv, n.surf))
		{
			const f3 ks = ld3(ks4);
			for(int l = 0; l < sv.nl; l++)
			{
				if(n.fr < 1) refraction_colour = value_of(N + 2u * (uint32_t) l) * n.fr;                                // :70 (=, not +=)
				reflection_colour = reflection_colour + (ks * (1 - n.fr)) * value_of(N + 2u * (uint32_t) l + 1u);       // :76
			}
		}
		direct = (direct + refraction_colour) + reflection_colour; // :102
	}
	if(!p.monte_carlo)
	{ // :218
		if constexpr(EM::on) return emitted(emi.em, n.surf, direct);
		else return direct;
	}
	f3 total = mk3(0, 0, 0);
	uint32_t rnd[4] = {0, 0, 0, 0};
	for(uint32_t c = 0; c < N; c++)
	{ // :117-131: total += r1 * shade() / pdf, in child order
		if((c & 1u) == 0u) philox4x32(n.pixel, p.aa_index, n.node_id, c >> 1, p.seed_lo, p.seed_hi, rnd);
		const float r1 = u31_to_unit(rnd[2 * (c & 1u)]);
		total = total + div3_const(value_of(c) * r1, SKR_DIV_PDF);
	}
	total = total / (float) p.num_path_traces;                              // :133 (N == 0: 0/0, as in the reference)
	if constexpr(EM::on) return emitted(emi.em, n.surf, (div3_const(direct, SKR_DIV_PI) + total * 2.0f) * kd);
	else return (div3_const(direct, SKR_DIV_PI) + total * 2.0f) * kd; // :213
}

} // namespace

// FOG: the scene has fog volumes (a separate instance: the fog term's registers would cost every other frame a wave per SIMD)
// Q: TriShadows — the shadow walk behind the sphere test; SphereTree — the sphere test is the tree's pair walk; SpotLights — the pair loop with
//    the cone decision; SpotLights SoftLights — and the light sample ahead of it; Lens — a level-1 hit's ray starts on the lens; Motion —
//    the normal and the shadow rays meet the spheres where they are at the sample's shutter time; Textures — the material rows of a
//    sphere with a texture are multiplied by its colour at the normal; Emission — a last-level sphere hit's value takes the sphere's
//    emission (which packs exist: with_pack)
template <bool FOG, typename... Q>
__global__ __launch_bounds__(256) void skr_gactivate_kernel(const RenderParams p, const Q... qs)
{ // a workgroup covers 256 consecutive positions of one region; positions past the region's count exit
	constexpr bool RAYS = pack_has<ShadeRays, Q...>, TSHADOW = pack_has<TriShadows, Q...>, STREE = pack_has<SphereTree, Q...>, SPOT = pack_has<SpotLights, Q...>,
				   SOFT = pack_has<SoftLights, Q...>, LENS = pack_has<Lens, Q...>, MOTION = pack_has<Motion, Q...>, TEX = pack_has<Textures, Q...>, EMIT = pack_has<Emission, Q...>;
	static_assert(!MOTION || (SPOT && SOFT && !FOG && !STREE && !LENS), "a launch with motion carries SpotLights and SoftLights (with_pack)");
	static_assert(!TEX || (SPOT && SOFT && !FOG && !STREE), "a launch with textures carries SpotLights and SoftLights (with_pack)");
	static_assert(!EMIT || TEX, "a launch with emission carries Textures (with_pack)");
	const ShadeRays q = pick<ShadeRays>(qs...);
	extern __shared__ __align__(16) unsigned char lds_raw[];
	float4 *lds4 = reinterpret_cast<float4 *>(lds_raw);
	const uint32_t per_region = (p.rc_cap + 255u) / 256u;
	const uint32_t region = (uint32_t) blockIdx.x / per_region, pos0 = ((uint32_t) blockIdx.x % per_region) * 256u;
	const uint32_t cnt = *lc_count(p.rc_ctr, region);
	if(pos0 >= cnt && blockIdx.x != 0) return;
	__shared__ uint32_t s_pre[SKR_PREFIX_WORDS];
	region_prefix(p, s_pre, blockIdx.x == 0); // (workgroup 0 leaves the level's record count for the kernels that follow)
	if(pos0 >= cnt) return;
	const SceneView sv = stage_for<STREE>(p, lds4);
	const uint32_t pos = pos0 + threadIdx.x;
	const bool act = pos < cnt;
	const uint32_t rec = region * p.rc_cap + pos;
	Counters cn{0, 0, 0};
	if(act)
	{
		const float4 r0 = p.rc[(size_t) rec * GREC_ROWS], r1 = p.rc[(size_t) rec * GREC_ROWS + 1];
		const uint32_t parent = __float_as_uint(r0.x), surf = __float_as_uint(r0.y), c = __float_as_uint(r0.z);
		const float t = r0.w;
		GNode n;
		n.d = mk3(r1.x, r1.y, r1.z);
		n.surf = surf;
		n.rec = rec;
		n.file = -1;
		f3 o;
		if(p.g_level == 1)
		{
			if constexpr(RAYS)
			{ // the counter RNG's pixel word: the ray's key
				const uint32_t ray = q.ray0 + parent;
				const float4 ra = q.rays[2 * (size_t) ray];
				n.pixel = q.keys ? q.keys[ray] : ray;
				n.node_id = 0u;
				o = mk3(ra.x, ra.y, ra.z);
			}
			else
			{
				const uint32_t bw = (uint32_t) p.width, row = p.band_row0 + parent / bw, x = parent - (parent / bw) * bw;
				const uint32_t y = image_row(p, row);
				n.pixel = y * bw + x;
				n.node_id = 0u;
				o = p.cam_pos;
				if constexpr(LENS)
				{ // the origin the trace kernel gave the ray: the same draw, the same o' (d' is the record's)
					f3 d2;
					lens_ray(p, pick<Lens>(qs...), n.pixel, p.aa_index, n.d, o, d2);
				}
			}
		}
		else
		{
			const GNode pn = load_node(p.g_nodes_src + (size_t) parent * GNODE_ROWS);
			n.pixel = pn.pixel;
			n.node_id = pn.node_id * p.g_arity + c + 1u; // DESIGN.md "Counter RNG": child c of node n
			const uint32_t N = (uint32_t) (p.monte_carlo ? p.num_path_traces : 0);
			o = c < N ? add_scalar(pn.P, 0.00001f) : pn.P; // raytrace.h:128 / :66, :73
		}
		n.P = o + n.d * t; // raytrace.h:204 (t of the winner == the loop's minimum)
		MovingCentres at{nullptr, 0.0f}; // MOTION: where the spheres are at the shutter time of the node's sample (the draw the trace kernel made for the ray)
		if constexpr(MOTION) at = MovingCentres{pick<Motion>(qs...).vel, shutter_time(p, n.pixel, p.aa_index, pick<Motion>(qs...).S)};
		float4 ambp, ks4;
		f3 kd;
		surface_material(sv, p, surf, ambp, kd, ks4);
		if(surf & SURF_TRI)
		{ // include/skr.h skr_options.shade_triangles: the geometric normal, turned against the ray
			const uint32_t slot = surf & ~SURF_TRI;
			n.N = normalize3(cross3(ld3(sv.tris[3 * slot + 1]), ld3(sv.tris[3 * slot + 2])));
			if(dot3(n.N, n.d) > 0.0f) n.N = mk3(-n.N.x, -n.N.y, -n.N.z);
			n.file = __float_as_int(sv.tris[3 * slot + 1].w);
		}
		else if constexpr(MOTION) n.N = normalize3(n.P - ld3(at.row(sv.geom[surf], (int) surf))); // :205, the centre the trace kernel's search met
		else n.N = normalize3(n.P - ld3(sv.geom[surf])); // :205
		if constexpr(TEX) textured_material(pick<Textures>(qs...), surf, n.N, ambp, kd); // (ahead of the light loop: the taps are dead when it starts)
		cn.hits++;
		{ // raytrace.h:36-44: the direct light, each arm with what this instance's pack switches on
			using Shadows = TriangleShadows<TSHADOW>; // what a pair loop calls behind its sphere test
			using Spheres = std::conditional_t<STREE, SphereTreeShadows, SphereLoops>;  // the sphere test of every pair of lights: the tree's pair walk, or the loops
			const TriShadows &ts = pick<TriShadows>(qs...);
			const SphereTree &st = pick<SphereTree>(qs...);
			const Shadows shadows{sv, ts.trees, n.file};
			const Spheres spheres{st};
			if constexpr(MOTION)
			{ // the same pair loop on the spheres of the sample; the shadow masks are built from the centres at rest: a view without them (the precedent: direct_light_cone's `every`)
				SceneView moved = sv;
				moved.smask = nullptr;
				n.direct = direct_light_cone<SOFT>(moved, p, pick<SpotLights>(qs...), pick<SoftLights>(qs...), kd, ld3(ks4), ambp, n.P, n.N, n.pixel, n.node_id, cn, shadows, at);
			}
			else if constexpr(SPOT) // the pair loop with the cone decision ahead of the shadow walk (SOFT: and the light sample ahead of that)
				n.direct = direct_light_cone<SOFT>(sv, p, pick<SpotLights>(qs...), pick<SoftLights>(qs...), kd, ld3(ks4), ambp, n.P, n.N, n.pixel, n.node_id, cn, shadows);
			else if(FOG && !(surf & SURF_TRI)) n.direct = direct_light_fog(sv, p, kd, ld3(ks4), ambp, n.P, n.N, ld3(sv.geom[surf]), n.pixel, n.node_id, cn, spheres);
			else n.direct = direct_light_of<false>(sv, p, kd, ld3(ks4), ambp, n.P, n.N, cn, shadows, spheres);
		}
		n.fr = (p.legacy_reflect && !(surf & SURF_TRI)) ? legacy_fresnel(n.d, n.N, ks4.w) : 0.0f; // :46
		if(p.g_last)
		{ // its children are shade(depth 0) == (0,0,0): the node is finished
			if constexpr(TEX && !EMIT) store3(p.res_out + (size_t) rec * 3, node_value(sv, p, n, [](uint32_t) { return mk3(0, 0, 0); }, WithTextures{pick<Textures>(qs...)}));
			else if constexpr(!TEX) store3(p.res_out + (size_t) rec * 3, node_value(sv, p, n, [](uint32_t) { return mk3(0, 0, 0); }));
			else // (the new arm last: the closure types of the two above keep the numbers they had in the instances without emission)
				store3(p.res_out + (size_t) rec * 3, node_value(sv, p, n, [](uint32_t) { return mk3(0, 0, 0); }, WithTextures{pick<Textures>(qs...)}, WithEmission{pick<Emission>(qs...)}));
		}
		else
		{
			float4 *rows = p.g_nodes_dst + (size_t) (s_pre[region] + pos) * GNODE_ROWS;
			rows[0] = make_float4(n.P.x, n.P.y, n.P.z, n.N.x);
			rows[1] = make_float4(n.N.y, n.N.z, n.d.x, n.d.y);
			rows[2] = make_float4(n.d.z, __uint_as_float(n.surf), __uint_as_float(n.pixel), __uint_as_float(n.node_id));
			rows[3] = make_float4(n.direct.x, n.direct.y, n.direct.z, n.fr);
			rows[4] = make_float4(__uint_as_float(n.rec), __uint_as_float((uint32_t) n.file), 0.0f, 0.0f);
		}
	}
	add_counters(p, cn, blockIdx.x * 4u + (threadIdx.x >> 6), threadIdx.x & 63);
}

// =====================================================================================================================
// finalize: one lane per node of a level (level 0: per pixel of the band)
// =====================================================================================================================
template <typename... Q>
__global__ __launch_bounds__(256) void skr_gfinalize_kernel(const RenderParams p, const Q... qs)
{
	constexpr bool RAYS = pack_has<ShadeRays, Q...>, STREE = pack_has<SphereTree, Q...>, ENV = pack_has<EnvMap, Q...>, LENS = pack_has<Lens, Q...>, TEX = pack_has<Textures, Q...>,
				   EMIT = pack_has<Emission, Q...>;
	static_assert(!TEX || !STREE, "textures exclude the sphere tree (skr_features_conflict)");
	static_assert(!EMIT || TEX, "a launch with emission carries Textures (with_pack)");
	static_assert(!ENV || !STREE, "the environment excludes the sphere tree (skr_features_conflict)");
	static_assert(!LENS || (ENV && !RAYS), "the finalize kernel takes a Lens only behind an EnvMap, and only for frames (with_pack)");
	const ShadeRays q = pick<ShadeRays>(qs...);
	extern __shared__ __align__(16) unsigned char lds_raw[];
	float4 *lds4 = reinterpret_cast<float4 *>(lds_raw);
	const uint32_t n_nodes = *p.nd_count;
	if((uint32_t) blockIdx.x * 256u >= n_nodes) return;
	const SceneView sv = stage_for<STREE>(p, lds4);
	const uint32_t node = (uint32_t) blockIdx.x * 256u + threadIdx.x;
	if(node >= n_nodes) return;
	const uint32_t A = p.g_arity;
	const GNode *own = nullptr; // ENV: the lane's node below level 0, whose child rays value_of may have to form again
	// the direction of child c as the trace kernel formed it (ENV: what a miss looks up)
	auto direction_of = [&](uint32_t c) -> f3 {
		if(p.g_level != 0) return child_of(sv, p, *own, c).d;
		if constexpr(RAYS)
		{
			const float4 rb = q.rays[2 * (size_t) (q.ray0 + node) + 1];
			return mk3(rb.x, rb.y, rb.z);
		}
		else
		{
			const uint32_t bw = (uint32_t) p.width, row = p.band_row0 + node / bw, x = node - (node / bw) * bw;
			const uint32_t y = image_row(p, row);
			f3 d;
			primary_ray(p, (int) x, y, y * bw + x, p.aa_index, d);
			if constexpr(LENS)
			{
				f3 o2;
				lens_ray(p, pick<Lens>(qs...), y * bw + x, p.aa_index, d, o2, d);
			}
			return d;
		}
	};
	// the value of child c: its record's (a hit), (0,0,0) (a triangle took it: raytrace.h:221-224) or the background (:189-192; ENV:
	// the environment in the ray's direction)
	auto value_of = [&](uint32_t c) -> f3 {
		const uint64_t ri = (uint64_t) node * A + c;
		const uint4 *h = p.ixh + GHDR_ROWS * (size_t) (ri >> 6);
		const uint4 h0 = h[0], h1 = h[1];
		const unsigned long long mh = (unsigned long long) h1.y << 32 | h1.x, mb = (unsigned long long) h1.w << 32 | h1.z;
		const uint32_t bit = (uint32_t) ri & 63u;
		if((mh >> bit) & 1ull)
		{
			const float *r = p.res_in + (size_t) (h0.x + (uint32_t) __popcll(mh & ((1ull << bit) - 1ull))) * 3;
			return mk3(r[0], r[1], r[2]);
		}
		if constexpr(ENV)
		{
			if((mb >> bit) & 1ull) return mk3(0, 0, 0);
			return env_lookup(pick<EnvMap>(qs...), direction_of(c), p.background);
		}
		else return ((mb >> bit) & 1ull) ? mk3(0, 0, 0) : p.background;
	};
	if(p.g_level == 0)
	{
		if constexpr(RAYS)
		{ // the caller's ray: its value, unquantised
			store3(q.out + (size_t) (q.ray0 + node) * 3, value_of(0u));
			return;
		}
		// the camera level: the pixel is its primary ray's value (rows outside the image have no ray and no pixel)
		const uint32_t bw = (uint32_t) p.width, row = p.band_row0 + node / bw, x = node - (node / bw) * bw;
		if(image_row(p, row) < (uint32_t) p.height) emit_sample(p, row * bw + x, value_of(0u));
		return;
	}
	const GNode n = load_node(p.g_nodes_src + (size_t) node * GNODE_ROWS);
	GNode m = n;
	if constexpr(ENV) own = &m;
	// a child that does not exist (no legacy terms for this surface; fr >= 1) is never asked for by node_value()
	if constexpr(EMIT) store3(p.res_out + (size_t) n.rec * 3, node_value(sv, p, m, value_of, WithTextures{pick<Textures>(qs...)}, WithEmission{pick<Emission>(qs...)}));
	else if constexpr(TEX) store3(p.res_out + (size_t) n.rec * 3, node_value(sv, p, m, value_of, WithTextures{pick<Textures>(qs...)}));
	else store3(p.res_out + (size_t) n.rec * 3, node_value(sv, p, m, value_of));
}

// =====================================================================================================================
// host side
// =====================================================================================================================
static bool gplan_for(const RenderParams &p, uint32_t rows, GPlan &pl)
{
	const uint64_t A = skr_tree_arity(p);
	pl.levels = (A == 0) ? 1 : p.max_depth;
	if(pl.levels < 1 || pl.levels > SKR_GLEVELS_MAX) return false;
	pl.band_rows = rows;
	pl.nodes_max[0] = (uint64_t) rows * (uint64_t) p.width;
	ScratchLayout s;
	pl.ctr_bytes = (SKR_PULL_STRIDE + LVL_CTR_WORDS * (size_t) (pl.levels + 1)) * sizeof(uint32_t);
	pl.off_ctr = s.take(pl.ctr_bytes);
	for(int L = 1; L <= pl.levels; L++)
	{ // a region receives at most 64 hits from each of its trace waves (64 rays): `cap` record slots per region; the level cannot hold
	  // more hits than it has rays, which bounds the next level's rays (a band of one row would otherwise be sized for 64 x 64 nodes)
		const uint64_t rays = pl.nodes_max[L - 1] * (L == 1 ? 1 : A);
		const uint64_t chunks = (rays + 63) / 64;
		const uint64_t cap = (chunks + SKR_P1_REGIONS - 1) / SKR_P1_REGIONS * 64;
		if(cap * SKR_P1_REGIONS >= (1ull << 31)) return false;
		const uint64_t slots = cap * SKR_P1_REGIONS;
		pl.cap[L] = (uint32_t) cap;
		pl.nodes_max[L] = slots < rays ? slots : rays;
		pl.off_hdr[L] = s.take((chunks + 4) * GHDR_ROWS * 16);
		pl.off_recs[L] = s.take((size_t) slots * GREC_ROWS * 16);
		pl.off_res[L] = s.take((size_t) slots * 12 + 16);
		if(L < pl.levels) pl.off_nodes[L] = s.take((size_t) pl.nodes_max[L] * GNODE_ROWS * 16);
		if(s.off > ((size_t) 1 << 40)) return false;
	}
	pl.total = s.off;
	return true;
}

static uint64_t g_budget(const RenderParams &p) { return p.sw.budget_mb ? (uint64_t) p.sw.budget_mb << 20 : 6ull << 30; }

// the largest band of output rows whose worst-case tables fit the budget (< 65536 spheres, < 2^30 triangles); false: not even one row
bool skr_generic_plan(const RenderParams &p, GPlan &pl, bool sphere_tree)
{ // (with the sphere tree the surface code's 31 bits bound the sphere count: an int32_t holds no more)
	if((p.n_spheres >= 65536 && !sphere_tree) || p.n_tris >= (1 << 30)) return false;
	const uint64_t budget = g_budget(p);
	const uint32_t rows = skr_largest_band(p.out_rows, [&](uint32_t r) { return gplan_for(p, r, pl) && pl.total <= budget; });
	return rows > 0 && gplan_for(p, rows, pl);
}

// Calls `launch` with the pack of an instance: [ShadeRays] [TriShadows] [SphereTree | SpotLights [SoftLights]] [Lens | Motion], the one
// place the order is written down.  K: whose pack — the activate kernel's is the whole of it; the trace kernel takes only [ShadeRays]
// [SphereTree] [Lens | Motion], the finalize kernel [ShadeRays] [SphereTree] [EnvMap [Lens]].  The combinations skr_features_conflict refuses (the sphere
// tree with spot lights, a radius, a lens or motion; a lens with motion) are no instance, nor is a lens with a shading query (its rays are
// the caller's).  A launch with motion always carries SpotLights SoftLights (their tables have n = 0 where the scene has none), so motion
// adds two trace and four activate instances.  The environment excludes the sphere tree too and adds three finalize instances:
// <EnvMap>, <ShadeRays, EnvMap>, <EnvMap, Lens>.  Textures come last, in the activate and the finalize kernel's pack: [...] Textures.
// They exclude the sphere tree, and a launch with them always carries SpotLights SoftLights as one with motion does, so they add ten
// activate instances — [ShadeRays] [TriShadows] SpotLights SoftLights [Lens | Motion] Textures, a Lens never behind ShadeRays — and five
// finalize instances: <Textures>, <EnvMap, Textures>, <EnvMap, Lens, Textures>, <ShadeRays, Textures>, <ShadeRays, EnvMap, Textures>.
// No trace instance takes them.  Emission comes behind Textures, the last of the pack, in the same two kernels: [...] Textures Emission.
// A launch with emission always carries Textures (every row's edge 0 where the scene has none) and with them SpotLights SoftLights, so
// emission mirrors the Textures instances one for one: ten activate and five finalize instances more, and no trace instance.
enum PackOf { PACK_FINALIZE, PACK_TRACE, PACK_ACTIVATE };
template <PackOf K, typename F>
static void with_pack(const GenericFeatures &f, const ShadeRays *q, F launch)
{
	constexpr bool ACT = K == PACK_ACTIVATE;
	auto last = [&](auto... all) { // (the activate kernel's Textures only behind SoftLights: no other pack of it is ever asked for them)
		if constexpr(K == PACK_FINALIZE || (ACT && pack_has<SoftLights, decltype(all)...>))
		{
			if(f.emit) return launch(all..., f.textures, f.emission);
			if(f.tex) return launch(all..., f.textures);
		}
		launch(all...);
	};
	auto lens = [&](auto... all) {
		if constexpr(K != PACK_FINALIZE && !pack_has<ShadeRays, decltype(all)...>)
			if(f.lens) return last(all..., f.thin_lens);
		last(all...);
	};
	auto tail = [&](auto... head) {
		if(f.sphere_tree) return launch(head..., f.stree);
		if constexpr(ACT)
		{
			if(f.motion) return last(head..., f.spots, f.softs, f.mot);
			if(f.soft || f.tex || f.emit) return lens(head..., f.spots, f.softs);
			if(f.spot) return lens(head..., f.spots);
		}
		else if constexpr(K == PACK_TRACE)
		{
			if(f.motion) return launch(head..., f.mot);
		}
		else if(f.env)
		{ // the finalize kernel: the lookup, and under a lens the draw that made the primary ray (a frame's only)
			if constexpr(!pack_has<ShadeRays, decltype(head)...>)
				if(f.lens) return last(head..., f.envmap, f.thin_lens);
			return last(head..., f.envmap);
		}
		lens(head...);
	};
	auto shadows = [&](auto... head) {
		if constexpr(ACT)
			if(f.tri_shadows) return tail(head..., f.shadows);
		tail(head...);
	};
	if(q) shadows(*q);
	else shadows();
}

hipError_t skr_launch_generic(const RenderParams &p_in, const GPlan &pl, hipStream_t stream, const SkrTimingHook *hook, const GenericFeatures &f, const ShadeRays *q_in)
{
	if(skr_features_conflict(f, p_in.legacy_reflect != 0, p_in.shade_triangles != 0, p_in.n_fog > 0)) return hipErrorInvalidValue; // (refused with a text: api.cpp launch_params)
	RenderParams p = p_in;
	char *base = reinterpret_cast<char *>(p.node_scratch);
	uint32_t *ctr0 = reinterpret_cast<uint32_t *>(base + pl.off_ctr);
	auto lvl_ctr = [&](int L) { return ctr0 + SKR_PULL_STRIDE + LVL_CTR_WORDS * (size_t) L; };
	const int nsamp = (p.grid_size > 0 && !q_in) ? p.grid_size * p.grid_size : 1; // (a query: the one sample p.aa_index)
	ShadeRays q = q_in ? *q_in : ShadeRays{};
	const ShadeRays *qp = q_in ? &q : nullptr; // (q.ray0: the band's)
	const size_t lds = (f.sphere_tree ? skr_lights_lds_bytes(p) : skr_scene_lds_bytes(p)) + 32;
	const uint32_t A = skr_tree_arity(p);
	const int D = pl.levels;
	hipError_t e = hipSuccess;
	for(int s = 0; s < nsamp; s++)
	{
		if(!q_in) p.aa_index = (uint32_t) s;
		for(uint32_t row0 = 0; row0 < p.out_rows; row0 += pl.band_rows)
		{ // every band is a complete pass
			const uint32_t rows = p.out_rows - row0 < pl.band_rows ? p.out_rows - row0 : pl.band_rows;
			const bool timed = hook && s == nsamp - 1 && row0 == 0; // (the first band of the last sample: a full-size band)
			p.band_row0 = row0;
			p.band_rows = rows;
			uint32_t roots = rows * (uint32_t) p.width;
			if(q_in)
			{ // a query's band: its rays [ray0, ray0 + roots), the last row partial
				q.ray0 = row0 * (uint32_t) p.width;
				roots = q.n - q.ray0 < roots ? q.n - q.ray0 : roots;
			}
			e = hipMemsetAsync(ctr0, 0, pl.ctr_bytes, stream);
			if(e != hipSuccess) return e;
			e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctr0), (int) roots, 1, stream); // [0]: the band's roots
			if(e != hipSuccess) return e;
			if(timed) skr_hook_start(hook, stream);
			for(int L = 1; L <= D; L++)
			{
				p.g_level = (uint32_t) L;
				p.g_arity = L == 1 ? 1u : A;
				p.g_last = L == D ? 1u : 0u;
				p.nd_count = L == 1 ? ctr0 : lc_prefix_host(lvl_ctr(L - 1));
				p.g_nodes_src = L == 1 ? nullptr : reinterpret_cast<const float4 *>(base + pl.off_nodes[L - 1]);
				p.rc = reinterpret_cast<float4 *>(base + pl.off_recs[L]);
				p.rc_cap = pl.cap[L];
				p.rc_ctr = lvl_ctr(L);
				p.ixh = reinterpret_cast<uint4 *>(base + pl.off_hdr[L]);
				const uint64_t wg_t = (pl.nodes_max[L - 1] * (uint64_t) p.g_arity + 255) / 256;
				const unsigned grid_t = (unsigned) (wg_t < 49152u ? wg_t : 49152u);
				with_pack<PACK_TRACE>(f, qp, [&](auto... a) { hipLaunchKernelGGL((skr_gtrace_kernel<decltype(a)...>), dim3(grid_t), dim3(256), lds, stream, p, a...); });
				p.g_arity = A; // (node ids of this level's hits: parent id * A + child + 1)
				p.g_nodes_dst = L < D ? reinterpret_cast<float4 *>(base + pl.off_nodes[L]) : nullptr;
				p.res_out = reinterpret_cast<float *>(base + pl.off_res[L]);
				const unsigned grid_a = SKR_P1_REGIONS * ((pl.cap[L] + 255u) / 256u);
				with_pack<PACK_ACTIVATE>(f, qp, [&](auto... a) { // FOG: a separate instance, and only of the packs without triangle shadows, spot lights and a lens
					if constexpr(!pack_has<TriShadows, decltype(a)...> && !pack_has<SpotLights, decltype(a)...> && !pack_has<Lens, decltype(a)...>)
						if(p.n_fog > 0)
						{
							hipLaunchKernelGGL((skr_gactivate_kernel<true, decltype(a)...>), dim3(grid_a), dim3(256), lds, stream, p, a...);
							return;
						}
					hipLaunchKernelGGL((skr_gactivate_kernel<false, decltype(a)...>), dim3(grid_a), dim3(256), lds, stream, p, a...);
				});
			}
			for(int L = D - 1; L >= 0; L--)
			{ // sums, deepest level first; level 0 writes the pixels
				p.g_level = (uint32_t) L;
				p.g_arity = L == 0 ? 1u : A;
				p.nd_count = L == 0 ? ctr0 : lc_prefix_host(lvl_ctr(L));
				p.g_nodes_src = L == 0 ? nullptr : reinterpret_cast<const float4 *>(base + pl.off_nodes[L]);
				p.ixh = reinterpret_cast<uint4 *>(base + pl.off_hdr[L + 1]);
				p.res_in = reinterpret_cast<const float *>(base + pl.off_res[L + 1]);
				p.res_out = L == 0 ? nullptr : reinterpret_cast<float *>(base + pl.off_res[L]);
				const dim3 grid_f((unsigned) ((pl.nodes_max[L] + 255) / 256));
				with_pack<PACK_FINALIZE>(f, qp, [&](auto... a) { hipLaunchKernelGGL((skr_gfinalize_kernel<decltype(a)...>), grid_f, dim3(256), lds, stream, p, a...); });
			}
			if(timed) skr_hook_stop(hook, stream);
			e = hipGetLastError();
			if(e != hipSuccess) return e;
		}
	}
	if(p.grid_size > 0 && !q_in) return skr_launch_resolve(p, stream);
	return hipSuccess;
}

// =====================================================================================================================
// skr_debug_eval op 26 (include/skr.h): the texture colour of a normal, through texture_colour as textured_material calls it
// =====================================================================================================================
namespace {
constexpr uint32_t DEBUG_TEX_EDGES[4] = {1u, 2u, 3u, 64u};
}
__global__ void skr_debug_texture_kernel(const uint32_t *in, uint32_t *out, uint32_t n, const Textures tx)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const uint32_t *r = in + 4 * i;
	f3 c = mk3(1, 1, 1);
	if(r[3] < 4u)
	{ // (the op's rows are per texture, not per sphere)
		const uint2 row = tx.rows[r[3]];
		c = texture_colour(tx, row.x, row.y, mk3(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2])));
	}
	uint32_t *w = out + 3 * i;
	w[0] = __float_as_uint(c.x); w[1] = __float_as_uint(c.y); w[2] = __float_as_uint(c.z);
}

hipError_t skr_launch_debug_texture(const void *d_in, void *d_out, uint32_t n, hipStream_t stream)
{ // the op's own textures: edges (1, 2, 3, 64), texel (row j, column i) = (i + 1, j + 1, 0.5 (i + j) + 0.25); two rows of pairs, then the texels
	const size_t rows = 2;
	size_t total = rows;
	for(uint32_t E : DEBUG_TEX_EDGES) total += (size_t) E * E;
	float4 *host = (float4 *) calloc(total, sizeof(float4));
	if(!host) return hipErrorOutOfMemory;
	uint32_t *pairs = reinterpret_cast<uint32_t *>(host);
	size_t at = rows;
	for(int k = 0; k < 4; k++)
	{
		const uint32_t E = DEBUG_TEX_EDGES[k];
		pairs[2 * k] = (uint32_t) (at - rows);
		pairs[2 * k + 1] = E;
		for(uint32_t j = 0; j < E; j++)
			for(uint32_t i = 0; i < E; i++) host[at++] = make_float4((float) (i + 1u), (float) (j + 1u), 0.5f * (float) (i + j) + 0.25f, 0.0f);
	}
	float4 *dev = nullptr;
	hipError_t e = hipMalloc((void **) &dev, total * sizeof(float4));
	if(e == hipSuccess) e = hipMemcpy(dev, host, total * sizeof(float4), hipMemcpyHostToDevice);
	free(host);
	if(e == hipSuccess)
	{
		hipLaunchKernelGGL(skr_debug_texture_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const uint32_t *) d_in, (uint32_t *) d_out, n,
						   Textures{dev + rows, reinterpret_cast<const uint2 *>(dev)});
		e = hipGetLastError();
		if(e == hipSuccess) e = hipStreamSynchronize(stream); // (the textures are freed below)
	}
	if(dev) (void) hipFree(dev);
	return e;
}
