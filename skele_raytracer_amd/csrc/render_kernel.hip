// Which kernels render a launch (gfx950 / CDNA4), and the device-side evaluation of the arithmetic spec for the unit tests.
//
// The per-pixel loop of the reference (src/main.cpp:129-182) and the shade() tree under it (src/raytrace.h:139-227) run as
//   * skr_direct_kernel (render_wave.hip) where shade() does not recurse: no --gillum, no spheres, --depth 1;
//   * the node pipeline (render_nodes.hip: sibling-pair kernels, persistent leaf kernel) for --gillum trees over sphere scenes
//     (and scenes with a handful of triangles) — the headline path;
//   * the general level pipeline (render_generic.hip: one lane per ray) for meshes under --gillum, --shade-triangles,
//     --legacy-reflect, fog volumes (--scn-fog) and more than 256 children per node.
// Rounds 1-2 also had a lane-per-pixel kernel with the recursion depth as a template parameter (--depth <= 6) here; the level
// pipelines take any depth.
//
// skr_plan_launch picks the path once per launch and sizes its scratch and LDS (launch.h LaunchPlan); render_pass (api.cpp) allocates
// and checks from that plan, and skr_launch_render and the pipelines' launchers follow it without planning again.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "launch.h"
#include "shade_common.h"
#include "wave_common.h"

// The direct kernel's workgroup: the scene + 4 x 192 bytes of tile — and, for a scene that is all mesh (every lane's time is the triangle
// walk, whose scalar loads go through a 16 KB cache that more waves only thrash), padding up to a third of the CU's LDS: dragon.scn
// runs 1.18 / 1.24 / 1.26 ms at 3 / 4 / 5 waves per SIMD.  A mesh among spheres wants the fourth wave to hide the shading's latencies:
// test.scn (1800 triangles, 4 spheres) 0.556 / 0.485 ms at 3 / 4.
#ifndef SKR_MESH_LDS_PAD
#define SKR_MESH_LDS_PAD 53248 // 3 x 53 248 B are co-resident on a CU (1280-byte granules), 4 are not
#endif
static size_t direct_lds_bytes(const RenderParams &p)
{
	const size_t need = skr_scene_lds_bytes(p) + 4 * 192; // scene | tile bytes
	return (p.n_tris > 0 && p.n_spheres == 0 && need < SKR_MESH_LDS_PAD) ? SKR_MESH_LDS_PAD : need;
}

// Which kernels render this launch, and what they need.  In this order:
//   * the general level pipeline takes the two modes only it knows (--shade-triangles, --legacy-reflect), fog volumes, spot lights, lights with a radius, a lens, motion, the environment, textures, emission, and every tree
//     (shade() recurses: max_depth > 1; api.cpp folds --depth to 1 where it cannot, raytrace.h:208-218) the node pipeline does not;
//   * the node pipeline takes the trees it selects (render_nodes.hip skr_nodes_plan), if a band of it fits the budget and its kernels
//     fit the device's LDS;
//   * the direct kernel takes the rest, unless the scene leaves it no room for its tile: then the general pipeline does.
// A launch is refused (api.cpp render_pass: lp.lds_bytes > the device's LDS) only where no path fits.
// SKR_PIPELINE=generic forces the general pipeline for every launch, SKR_PIPELINE=nodes keeps triangle meshes on the node pipeline
// (tests, A/B runs).
bool skr_plan_launch(const RenderParams &p, size_t lds_limit, LaunchPlan &lp, const GenericFeatures &f)
{
	lp = LaunchPlan();
	lp.features = f;
	const bool generic_only = f.sphere_tree || p.sw.pipeline == SKR_PIPE_GENERIC || p.shade_triangles || p.legacy_reflect || p.n_fog > 0 || f.spot || f.soft || f.lens || f.motion || f.env || f.tex || f.emit;
	if(!generic_only && skr_nodes_plan(p, lds_limit, lp.nodes))
	{
		lp.path = SKR_PATH_NODES;
		lp.variant = lp.nodes.flat ? "node_levels_v5_flat" : "node_levels_v5";
		lp.scratch_bytes = lp.nodes.total;
		lp.lds_bytes = lp.nodes.lds;
		lp.off_ctr = lp.nodes.off_ctr;
		lp.levels = lp.nodes.levels;
	}
	else if(generic_only || p.max_depth > 1 || direct_lds_bytes(p) > lds_limit)
	{ // (a frame without a tree whose scene leaves the direct kernel no room for its tile: the general pipeline renders it as well;
	  // the sphere tree, DESIGN.md 8.10: every frame, on the instances with the sphere walks, which stage only the lights)
		lp.path = SKR_PATH_GENERIC;
		lp.variant = skr_generic_variant(false, f);
		if(!skr_generic_plan(p, lp.generic, f.sphere_tree)) return false;
		lp.scratch_bytes = lp.generic.total;
		lp.lds_bytes = f.sphere_tree ? skr_lights_kernels_lds(p) : skr_scene_kernels_lds(p);
	}
	else
	{
		lp.lds_bytes = direct_lds_bytes(p);
		return true;
	}
	if(p.grid_size > 0) lp.acc_bytes = (size_t) p.width * p.out_rows * 12; // AA under --gillum: one pass per sample, summed here
	return true;
}

const char *skr_features_conflict(const GenericFeatures &f, bool legacy_reflect, bool shade_triangles, bool fog)
{
	if(fog && (legacy_reflect || shade_triangles || f.tri_shadows)) return "fog volumes (--scn-fog) cannot be combined with --legacy-reflect or --shade-triangles";
	const int with = legacy_reflect ? 0 : fog ? 1 : f.sphere_tree ? 2 : -1;
	static const char *const spot[3] = {"spot lights (--scn-spot) cannot be combined with --legacy-reflect", "spot lights (--scn-spot) cannot be combined with fog volumes (--scn-fog)",
										"spot lights (--scn-spot) cannot be combined with the sphere tree (--sphere-tree)"};
	static const char *const soft[3] = {"light radii (--light-radius) cannot be combined with --legacy-reflect", "light radii (--light-radius) cannot be combined with fog volumes (--scn-fog)",
										"light radii (--light-radius) cannot be combined with the sphere tree (--sphere-tree)"};
	static const char *const lens[3] = {"a lens (--aperture) cannot be combined with --legacy-reflect", "a lens (--aperture) cannot be combined with fog volumes (--scn-fog)",
										"a lens (--aperture) cannot be combined with the sphere tree (--sphere-tree)"};
	static const char *const motion[3] = {"motion blur (sphere velocities under --shutter) cannot be combined with --legacy-reflect", "motion blur (sphere velocities under --shutter) cannot be combined with fog volumes (--scn-fog)",
										  "motion blur (sphere velocities under --shutter) cannot be combined with the sphere tree (--sphere-tree)"};
	static const char *const env[3] = {"an environment map (--envmap) cannot be combined with --legacy-reflect", "an environment map (--envmap) cannot be combined with fog volumes (--scn-fog)",
									   "an environment map (--envmap) cannot be combined with the sphere tree (--sphere-tree)"};
	static const char *const tex[3] = {"sphere textures (--scn-texture) cannot be combined with --legacy-reflect", "sphere textures (--scn-texture) cannot be combined with fog volumes (--scn-fog)",
									   "sphere textures (--scn-texture) cannot be combined with the sphere tree (--sphere-tree)"};
	static const char *const emit[3] = {"sphere emission (--scn-emission) cannot be combined with --legacy-reflect", "sphere emission (--scn-emission) cannot be combined with fog volumes (--scn-fog)",
										"sphere emission (--scn-emission) cannot be combined with the sphere tree (--sphere-tree)"};
	if(f.motion && f.lens) return "motion blur (sphere velocities under --shutter) cannot be combined with a lens (--aperture)";
	return with < 0 ? nullptr : f.spot ? spot[with] : f.soft ? soft[with] : f.lens ? lens[with] : f.motion ? motion[with] : f.env ? env[with] : f.tex ? tex[with] : f.emit ? emit[with] : nullptr;
}

const char *skr_generic_variant(bool query, const GenericFeatures &f)
{ // (fog has no name of its own; a lens is a frame's: no shading query and no sphere-tree instance has one; motion excludes both; the
  // environment's part comes last but for the textures' "_tex" and, behind that, the emission's "_emit")
#define SKR_VARIANT_TEX(name) {{name, name "_emit"}, {name "_tex", name "_tex_emit"}}
#define SKR_VARIANT_ENV(name) {SKR_VARIANT_TEX(name), SKR_VARIANT_TEX(name "_env")}
#define SKR_VARIANT_NAMES(base) {{SKR_VARIANT_ENV(base), SKR_VARIANT_ENV(base "_tshadow")}, {SKR_VARIANT_ENV(base "_lens"), SKR_VARIANT_ENV(base "_lens_tshadow")}, {SKR_VARIANT_ENV(base "_motion"), SKR_VARIANT_ENV(base "_motion_tshadow")}}
	static const char *const name[2][4][3][2][2][2][2] = {
		{SKR_VARIANT_NAMES("level_pipeline_g1"), SKR_VARIANT_NAMES("level_pipeline_g1_stree"), SKR_VARIANT_NAMES("level_pipeline_g1_spot"), SKR_VARIANT_NAMES("level_pipeline_g1_soft")},
		{SKR_VARIANT_NAMES("shade_rays_g1"), SKR_VARIANT_NAMES("shade_rays_g1_stree"), SKR_VARIANT_NAMES("shade_rays_g1_spot"), SKR_VARIANT_NAMES("shade_rays_g1_soft")}};
#undef SKR_VARIANT_NAMES
#undef SKR_VARIANT_ENV
#undef SKR_VARIANT_TEX
	return name[query][f.sphere_tree ? 1 : f.soft ? 3 : f.spot ? 2 : 0][f.motion ? 2 : !query && f.lens][f.tri_shadows][f.env][f.tex][f.emit];
}

hipError_t skr_launch_render(const RenderParams &p, const LaunchPlan &lp, hipStream_t stream, const SkrTimingHook *hook)
{
	if(lp.path == SKR_PATH_GENERIC) return p.node_scratch ? skr_launch_generic(p, lp.generic, stream, hook, lp.features) : hipErrorInvalidValue;
	if(lp.path == SKR_PATH_NODES) return p.node_scratch ? skr_launch_nodes(p, lp.nodes, stream, hook) : hipErrorInvalidValue;
	if(p.n_spheres >= 65536) return hipErrorInvalidValue; // (one launch, no tree: any scene the LDS holds)
	skr_hook_start(hook, stream);
	const hipError_t e = skr_launch_wave(p, lp.lds_bytes, stream);
	skr_hook_stop(hook, stream);
	return e;
}

// ------------------------------------------------------------ debug eval ----
// Device-side evaluation of the arithmetic spec, one record per thread
// (skr_debug_eval in include/skr.h).
// Op 19: the hit root from binary32 pairs.  Op 18: the sample of a light with a radius.  Op 17: the spot-light cone.  Ops 12..16 (include/skr.h): the filtered predicates of device_math.h and the selection code on top of them, through the functions the
// render kernels call.  `i` = the lane's record, `live` = it may write.
#define SKR_DEBUG_TABLE_ROWS 80u // ops 15, 16: rows of the sphere table in the input (<= 64 spheres, the pad row, the rows table_rows asks for behind it)
#define SKR_DEBUG_EC_PAD 8u      // ops 15, 16: rows behind the ns rows of a record's ec table
SKR_DEV void skr_debug_predicates(int op, const uint32_t *in, uint32_t *out, uint32_t n, uint32_t i, bool live)
{
	auto F = [](uint32_t u) { return __uint_as_float(u); };
	auto U = [](float f) { return __float_as_uint(f); };
	auto v3 = [&](const uint32_t *r) { return mk3(F(r[0]), F(r[1]), F(r[2])); };
	auto v4 = [&](const uint32_t *r) { return make_float4(F(r[0]), F(r[1]), F(r[2]), F(r[3])); };
	const float nan = __builtin_nanf("");
	switch(op)
	{
		case 12: { // one ray, one sphere: sphere_bracket, and bracket_from_ec on the row skr_camec_kernel forms
			const uint32_t *r = in + 10 * i;
			const f3 o = v3(r), d = v3(r + 3);
			const float4 g = v4(r + 6);
			const RayFilt f = make_filt(d);
			float lo = nan, hi = nan, b = nan, D = nan;
			const bool acc = sphere_bracket(o, d, f, g, lo, hi, b, D);
			const float4 q = camec_row(g, o);
			float lo2 = nan, hi2 = nan, b2 = nan, D2 = nan;
			const bool acc2 = bracket_from_ec(ld3(q), q.w, d, f, lo2, hi2, b2, D2);
			if(live)
			{
				uint32_t *w = out + 10 * i;
				w[0] = acc; w[1] = U(lo); w[2] = U(hi); w[3] = U(b); w[4] = U(D);
				w[5] = acc2; w[6] = U(lo2); w[7] = U(hi2); w[8] = U(b2); w[9] = U(D2);
			}
			break;
		}
		case 13: { // two rays with one origin, one sphere: pair_closest_step, the test of closest_pair_deferred (wave_common.h), both slots
			const uint32_t *r = in + 13 * i;
			const f3 o = v3(r), d0 = v3(r + 3), d1 = v3(r + 6);
			BestState s0 = best_none(), s1 = s0;
			const PairHit h = pair_closest_step(make_pair(d0, d1), o, true, v4(r + 9), 0, s0, s1);
			if(live)
			{
				uint32_t *w = out + 12 * i;
				w[0] = h.cand0; w[1] = h.acc0; w[2] = U(h.lo0); w[3] = U(h.hi0); w[4] = U(h.b.x); w[5] = U(h.D.x);
				w[6] = h.cand1; w[7] = h.acc1; w[8] = U(h.lo1); w[9] = U(h.hi1); w[10] = U(h.b.y); w[11] = U(h.D.y);
			}
			break;
		}
		case 14: { // two shadow rays from one point P, one sphere: pair_any_step, the test of occluded_pair (shade_common.h), both slots
			const uint32_t *r = in + 13 * i;
			const f3 o = add_scalar(v3(r), 0.000001f), L0 = v3(r + 3), L1 = v3(r + 6);
			const RayPair rp = make_pair(L0, L1);
			bool occ0 = false, occ1 = false;
			uint32_t tests = 0;
			const PairCand h = pair_any_step(rp, make_pair_any(rp), o, v4(r + 9), 0, occ0, occ1, tests);
			if(live)
			{
				uint32_t *w = out + 4 * i;
				w[0] = h.cand0; w[1] = occ0; w[2] = h.cand1; w[3] = occ1;
			}
			break;
		}
		case 15: { // the ec table (skr_camec_kernel's rows) of each record's origin over the scene at the head of the input
			const uint32_t ns = in[0] <= 64u ? in[0] : 64u;
			const float4 *table = (const float4 *) (in + 4);
			const uint32_t *r = in + 4u + 4u * SKR_DEBUG_TABLE_ROWS + 9u * i;
			const f3 o = v3(r);
			if(live)
				for(uint32_t k = 0; k < ns; k++)
				{
					const float4 q = camec_row(table[k], o);
					uint32_t *w = out + ((size_t) i * (ns + SKR_DEBUG_EC_PAD) + k) * 4u;
					w[0] = U(q.x); w[1] = U(q.y); w[2] = U(q.z); w[3] = U(q.w);
				}
			break;
		}
		case 16: { // the selection code over that scene: every closest-hit and any-hit form, both rays of the record
			const uint32_t ns = in[0] <= 64u ? in[0] : 64u;
			const uint32_t rec0 = 4u + 4u * SKR_DEBUG_TABLE_ROWS;
			const uint32_t *r = in + rec0 + 9u * i;
			// (each lane has its own ec table, so closest_sphere_from's rows come by vector loads with per-lane addresses here, not the
			// scalar loads of the primary kernels' one table; the scalar path of table_rows runs on geom_u below.  Same arithmetic.)
			const float4 *ec = (const float4 *) (in + rec0 + ((9u * n + 3u) & ~3u)) + (size_t) i * (ns + SKR_DEBUG_EC_PAD);
			const f3 o = v3(r), d0 = v3(r + 3), d1 = v3(r + 6);
			SceneView sv{}; // as trace_view (trace_rays.hip) builds one: every table in HBM, no mesh, no masks
			sv.geom = (const float4 *) (in + 4);
			sv.geom_u = sv.geom;
			sv.ns = (int) ns;
			sv.smask = nullptr;
			const RayConst r0 = make_ray(o, d0), r1 = make_ray(o, d1);
			int idx[8];
			float t[8];
			idx[0] = closest_sphere(sv, r0, t[0]);
			idx[1] = closest_sphere(sv, r1, t[1]);
			idx[2] = closest_sphere_from(sv, ec, r0, t[2]);
			idx[3] = closest_sphere_from(sv, ec, r1, t[3]);
			const RayPair rp = make_pair(d0, d1);
			BestState s0, s1;
			closest_pair_deferred<false>(sv, o, d0, d1, true, rp, s0, s1, 0u, 0u);
			idx[4] = s0.best;
			t[4] = s0.best >= 0 ? near_root_exact(rp.two_a.x, s0.b, s0.D) : __builtin_inff();
			idx[5] = s1.best;
			t[5] = s1.best >= 0 ? near_root_exact(rp.two_a.y, s1.b, s1.D) : __builtin_inff();
			idx[6] = closest_sphere_exact(sv, r0, t[6]);
			idx[7] = closest_sphere_exact(sv, r1, t[7]);
			bool a0, a1, c0, c1;
			uint32_t ta = 0, tc = 0;
			occluded_pair<false>(sv, o, d0, d1, true, a0, a1, ta); // (its origin is o + 1e-6, utils.h:45)
			occluded_pair<true>(sv, o, d0, d1, true, c0, c1, tc);
			if(live)
			{
				uint32_t *w = out + 22 * i;
				for(int k = 0; k < 8; k++)
				{
					w[2 * k] = (uint32_t) idx[k];
					w[2 * k + 1] = U(t[k]);
				}
				w[16] = a0; w[17] = a1; w[18] = ta;
				w[19] = c0; w[20] = c1; w[21] = tc;
			}
			break;
		}
		case 17: { // the cone decision and factor of one spot light at one shading point: spot_cone, the function direct_light_cone calls
			const uint32_t *r = in + 8 * i;
			const SpotCone c = spot_cone(v3(r), F(r[3]), F(r[4]), v3(r + 5));
			if(live)
			{
				out[2 * i] = U(c.f);
				out[2 * i + 1] = c.outside ? 1u : 0u;
			}
			break;
		}
		case 18: { // the sample of one light with a radius for one shading node: soft_sample, the function direct_light_cone<true> calls
			const uint32_t *r = in + 10 * i;
			const f3 s = soft_sample(r[0], r[1], r[2], r[3], r[4], r[5], v3(r + 6), F(r[9]));
			if(live)
			{
				out[3 * i] = U(s.x);
				out[3 * i + 1] = U(s.y);
				out[3 * i + 2] = U(s.z);
			}
			break;
		}
		case 19: { // the root from binary32 pairs against the binary64 form: near_root, near_root_exact and the interval near_root decides on
			const uint32_t *r = in + 3 * i;
			const float two_a = F(r[0]), b = F(r[1]), D = F(r[2]);
			RootPair q{};
			const bool short_form = SKR_FAST_EXACT && SKR_ROOT_PAIRS && near_root_pair(two_a, b, D, q) && q.lo == q.hi;
			if(live)
			{
				uint32_t *w = out + 7 * i;
				w[0] = U(near_root(two_a, b, D)); w[1] = U(near_root_exact(two_a, b, D)); w[2] = short_form ? 0u : 1u;
				w[3] = U(q.lo); w[4] = U(q.hi); w[5] = U(q.q_h); w[6] = U(q.q_l);
			}
			break;
		}
		default: break;
	}
}

__global__ void skr_debug_kernel(int op, const uint32_t *in, uint32_t *out, uint32_t n)
{
	uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	auto F = [](uint32_t u) { return __uint_as_float(u); };
	auto U = [](float f) { return __float_as_uint(f); };
	if(op >= 12 && op <= 19)
	{ // the predicate ops run whole waves (occluded_pair<true> and table_rows vote wave-wide): a lane past the end evaluates the last record and writes nothing
		const bool live = i < n;
		if(!live) i = n - 1u;
		skr_debug_predicates(op, in, out, n, i, live);
		return;
	}
	if(i >= n) return;
	switch(op)
	{
		case 0: {
			uint32_t o[4];
			const uint32_t *c = in + 6 * i;
			philox4x32(c[0], c[1], c[2], c[3], c[4], c[5], o);
			for(int k = 0; k < 4; k++) out[4 * i + k] = o[k];
			break;
		}
		case 9: { // EXHAUSTIVE check of the short exact forms (device_math.h) against the compiler's correctly rounded expansions: record i
		          // covers the 65536 bit patterns in[i] << 16 ...; out = mismatches of {sk_sqrtf, sk_rcpf, div_const pi, div_const pdf}
			uint32_t bad[4] = {0, 0, 0, 0};
			auto same = [](float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); };
			for(uint32_t k = 0; k < 65536u; k++)
			{
				const float x = F((in[i] << 16) | k);
				bad[0] += !same(sk_sqrtf(x), __builtin_sqrtf(x));
				bad[1] += !same(sk_rcpf(x), 1.0f / x);
				bad[2] += !same(div_const(x, SKR_DIV_PI), x / (float) 3.14159265358979323846);
				bad[3] += !same(div_const(x, SKR_DIV_PDF), x / (float) (1 / 3.14159265358979323846));
			}
			for(int k = 0; k < 4; k++) out[4 * i + k] = bad[k];
			break;
		}
		case 8: { // the round function at Random123's default count (known-answer vectors exist for 7 and for 10 rounds)
			uint32_t o[4];
			const uint32_t *c = in + 6 * i;
			philox4x32_r<10>(c[0], c[1], c[2], c[3], c[4], c[5], o);
			for(int k = 0; k < 4; k++) out[4 * i + k] = o[k];
			break;
		}
		case 1: {
			float s, c;
			sincos_spec(F(in[i]), s, c);
			out[2 * i] = U(s);
			out[2 * i + 1] = U(c);
			break;
		}
		case 2: out[i] = U(powf_spec(F(in[2 * i]), F(in[2 * i + 1]), 11)); break;
		case 3: {
			const float a = F(in[3 * i]), b = F(in[3 * i + 1]), c = F(in[3 * i + 2]);
			const float D = b * b - (4 * a) * c;
			out[i] = U((D < 0) ? __builtin_inff() : near_root_exact(2 * a, b, D));
			break;
		}
		case 4: {
			const uint32_t *r = in + 15 * i;
			const f3 o = mk3(F(r[0]), F(r[1]), F(r[2])), d = mk3(F(r[3]), F(r[4]), F(r[5]));
			const f3 v0 = mk3(F(r[6]), F(r[7]), F(r[8])), v1 = mk3(F(r[9]), F(r[10]), F(r[11])), v2 = mk3(F(r[12]), F(r[13]), F(r[14]));
			float t = 0.0f;
			const bool h = triangle_hit(o, d, v0, v1 - v0, v2 - v0, t);
			out[2 * i] = h ? 1u : 0u;
			out[2 * i + 1] = h ? U(t) : 0u;
			break;
		}
		case 5: out[i] = quantise(F(in[i])); break;
		case 6: {
			f3 nt, nb;
			tangent_basis(mk3(F(in[3 * i]), F(in[3 * i + 1]), F(in[3 * i + 2])), nt, nb);
			out[6 * i] = U(nt.x); out[6 * i + 1] = U(nt.y); out[6 * i + 2] = U(nt.z);
			out[6 * i + 3] = U(nb.x); out[6 * i + 4] = U(nb.y); out[6 * i + 5] = U(nb.z);
			break;
		}
		case 7: { // binary32 sqrt and divide must be the correctly rounded forms
			out[2 * i] = U(sk_sqrtf(F(in[2 * i])));
			out[2 * i + 1] = U(sk_divf(F(in[2 * i]), F(in[2 * i + 1])));
			break;
		}
		case 10: { // exp_spec (binary64 in, binary64 out: lo, hi words)
			const double x = __hiloint2double((int) in[2 * i + 1], (int) in[2 * i]);
			const double y = exp_spec(x);
			out[2 * i] = (uint32_t) __double2loint(y);
			out[2 * i + 1] = (uint32_t) __double2hiint(y);
			break;
		}
		case 11: { // fog_term: 40 words in (include/skr.h), {colour, no-interaction probability} out
			const uint32_t *r = in + 40 * i;
			auto v3 = [&](int k) { return mk3(F(r[k]), F(r[k + 1]), F(r[k + 2])); };
			const float4 a = make_float4(F(r[0]), F(r[1]), F(r[2]), 0.0f), alb = make_float4(F(r[4]), F(r[5]), F(r[6]), 0.0f);
			LightTerm t;
			t.L = v3(8);
			t.intensity = F(r[11]);
			t.lc = v3(12);
			const uint32_t ctr[4] = {r[27], r[32], r[31], fog_ctr3(r[23], r[19], r[15])};
			float pni = 0.0f;
			const f3 c = fog_term(a, alb, t, v3(16), v3(20), v3(24), v3(28), ctr, r[33], r[34], &pni);
			out[4 * i] = U(c.x); out[4 * i + 1] = U(c.y); out[4 * i + 2] = U(c.z); out[4 * i + 3] = U(pni);
			break;
		}
		case 20: { // powf_spec as the render kernels call it: (x, p, steps) -> {the instance that reads steps, the LE7 instance of the shaped leaf kernels}
			const float x = F(in[3 * i]), p = F(in[3 * i + 1]);
			const int steps = (int) in[3 * i + 2];
			out[2 * i] = U(powf_spec<false>(x, p, steps));
			out[2 * i + 1] = U(powf_spec<true>(x, p, steps));
			break;
		}
		case 21: { // EXHAUSTIVE check of len_terms (device_math.h) against the correctly rounded expansions, in the shape of op 9: record i
		           // covers the 65536 bit patterns in[i] << 16 ...; out = mismatches of {len_terms<true>.len, .inv, .inv2, len_terms<false>.inv}
			uint32_t bad[4] = {0, 0, 0, 0};
			auto same = [](float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); };
			for(uint32_t k = 0; k < 65536u; k++)
			{
				const float ss = F((in[i] << 16) | k);
				const LenTerms t = len_terms<true>(ss), u = len_terms<false>(ss);
				const float len = __builtin_sqrtf(ss);
				bad[0] += !same(t.len, len);
				bad[1] += !same(t.inv, 1.0f / len);
				bad[2] += !same(t.inv2, 1.0f / (len * len));
				bad[3] += !same(u.inv, 1.0f / len);
			}
			for(int k = 0; k < 4; k++) out[4 * i + k] = bad[k];
			break;
		}
		default: break;
	}
}

// Op 22: the lens sample and ray of one record: lens_ray, the function the camera kernels call under a lens (a kernel of its own: the
// ops above keep their code)
__global__ void skr_debug_lens_kernel(const uint32_t *in, uint32_t *out, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	auto F = [](uint32_t u) { return __uint_as_float(u); };
	auto U = [](float f) { return __float_as_uint(f); };
	const uint32_t *r = in + 18 * i;
	RenderParams p{};
	p.seed_lo = r[2];
	p.seed_hi = r[3];
	p.cam_pos = mk3(F(r[6]), F(r[7]), F(r[8]));
	p.cam_right = mk3(F(r[9]), F(r[10]), F(r[11]));
	p.cam_up = mk3(F(r[12]), F(r[13]), F(r[14]));
	Lens lens{};
	lens.A = F(r[4]);
	lens.k = F(r[5]);
	f3 o2, d2;
	float s[2];
	lens_ray(p, lens, r[0], r[1], mk3(F(r[15]), F(r[16]), F(r[17])), o2, d2, s);
	uint32_t *w = out + 8 * i;
	w[0] = U(s[0]); w[1] = U(s[1]);
	w[2] = U(o2.x); w[3] = U(o2.y); w[4] = U(o2.z);
	w[5] = U(d2.x); w[6] = U(d2.y); w[7] = U(d2.z);
}

// Op 23: powf_spec as the shaped leaf instance of an exponent mask calls it (launch.h SKR_LEAF_POW_MASKS): (x, p, mask) -> one word; a
// mask that is not listed gives 0xFFFFFFFF (a kernel of its own: the ops above keep their code)
__global__ void skr_debug_pow_kernel(const uint32_t *in, uint32_t *out, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const float x = __uint_as_float(in[3 * i]), p = __uint_as_float(in[3 * i + 1]);
	uint32_t r = 0xFFFFFFFFu;
	switch(in[3 * i + 2])
	{
#define X(m) \
	case m: r = __float_as_uint(powf_spec<true, m>(x, p, 7)); break;
		SKR_LEAF_POW_MASKS(X)
#undef X
	default: break;
	}
	out[i] = r;
}

// Op 24: the shutter time and the displaced centre of one record: (pixel, aa, seed_lo, seed_hi, S, c(3), v(3)) -> (tau, c'(3)), through
// shutter_time and MovingCentres::centre, the functions the kernels of a launch with motion call (a kernel of its own: the ops above
// keep their code)
__global__ void skr_debug_motion_kernel(const uint32_t *in, uint32_t *out, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	auto F = [](uint32_t u) { return __uint_as_float(u); };
	auto U = [](float f) { return __float_as_uint(f); };
	const uint32_t *r = in + 11 * i;
	RenderParams p{};
	p.seed_lo = r[2];
	p.seed_hi = r[3];
	const float tau = shutter_time(p, r[0], r[1], F(r[4]));
	const float4 c = MovingCentres::centre(make_float4(F(r[5]), F(r[6]), F(r[7]), 0.0f), make_float4(F(r[8]), F(r[9]), F(r[10]), 0.0f), tau);
	uint32_t *w = out + 4 * i;
	w[0] = U(tau); w[1] = U(c.x); w[2] = U(c.y); w[3] = U(c.z);
}

// Op 25: the taps of the environment lookup of one record: (d(3), E) -> (flag, i0, i1, j0, j1, fx, fy), through env_taps, the index
// code env_lookup runs (a kernel of its own: the ops above keep their code)
__global__ void skr_debug_env_kernel(const uint32_t *in, uint32_t *out, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const uint32_t *r = in + 4 * i;
	EnvTaps t{0, 0, 0, 0, 0.0f, 0.0f};
	const bool ok = env_taps(mk3(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2])), (int32_t) r[3], t);
	uint32_t *w = out + 7 * i;
	w[0] = ok ? 0u : 1u;
	w[1] = ok ? (uint32_t) t.i0 : 0u; w[2] = ok ? (uint32_t) t.i1 : 0u; w[3] = ok ? (uint32_t) t.j0 : 0u; w[4] = ok ? (uint32_t) t.j1 : 0u;
	w[5] = ok ? __float_as_uint(t.fx) : 0u; w[6] = ok ? __float_as_uint(t.fy) : 0u;
}

// Op 26: the texture colour of a normal on the op's own four textures (include/skr.h skr_debug_eval), through render_generic.hip
// texture_colour: its launcher lives beside that function
hipError_t skr_launch_debug_texture(const void *d_in, void *d_out, uint32_t n, hipStream_t stream);

hipError_t skr_launch_debug(int op, const void *d_in, void *d_out, uint32_t n, hipStream_t stream)
{
	if(op == 26) return skr_launch_debug_texture(d_in, d_out, n, stream);
	if(op == 25)
	{
		hipLaunchKernelGGL(skr_debug_env_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const uint32_t *) d_in, (uint32_t *) d_out, n);
		return hipGetLastError();
	}
	if(op == 24)
	{
		hipLaunchKernelGGL(skr_debug_motion_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const uint32_t *) d_in, (uint32_t *) d_out, n);
		return hipGetLastError();
	}
	if(op == 23)
	{
		hipLaunchKernelGGL(skr_debug_pow_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const uint32_t *) d_in, (uint32_t *) d_out, n);
		return hipGetLastError();
	}
	if(op == 22)
	{
		hipLaunchKernelGGL(skr_debug_lens_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const uint32_t *) d_in, (uint32_t *) d_out, n);
		return hipGetLastError();
	}
	hipLaunchKernelGGL(skr_debug_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, op, (const uint32_t *) d_in, (uint32_t *) d_out, n);
	return hipGetLastError();
}
