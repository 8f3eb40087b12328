// Wave-level helpers shared by the streaming kernels (render_wave.hip) and the node pipeline (render_nodes.hip).
#pragma once

#include "launch.h"
#include "shade_common.h"

namespace {

// Diagnostic build only (-DSKR_STAMPS=1): per-phase cycle shares, summed over waves into
// counters[4*SKR_COUNTER_SHARDS + phase].  Compiles to nothing otherwise.
#if defined(SKR_STAMPS) && SKR_STAMPS
#define STAMP_DECL unsigned long long st_t0 = __builtin_readcyclecounter(); unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define STAMP_ARG , unsigned long long &st_t0, unsigned long long (&st_acc)[8]
#define STAMP_PASS , st_t0, st_acc
#define STAMP(phase) do { const unsigned long long st_now = __builtin_readcyclecounter(); st_acc[phase] += st_now - st_t0; st_t0 = st_now; } while(0)
#else
#define STAMP_DECL
#define STAMP_ARG
#define STAMP_PASS
#define STAMP(phase)
#endif

SKR_DEV void wave_lds_fence()
{ // producer and consumer lanes are in the same wave: ordering only, no instruction
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}


SKR_DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
SKR_DEV f3 shfl3(f3 v, int src) { return mk3(__shfl(v.x, src, 64), __shfl(v.y, src, 64), __shfl(v.z, src, 64)); }
SKR_DEV int lanes_below(unsigned long long m)
{
	return (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u));
}


// ---- two sibling rays per lane ------------------------------------------------
// Children 2j and 2j+1 of a node share their origin (raytrace.h:128), one Philox call
// (DESIGN.md "RNG") and, per sphere, e = o - C and c = e.e - r^2; the per-ray part runs in
// packed binary32 (device_math.h RayPair).  Same values as child_round(), half the issue slots.
// (The selection state and its update: device_math.h BestState; the end of a slot: shade_common.h best_resolve.)

// With GI masks (`masked`, wave-uniform): `cand` = the union of the lane's two masks (shade_common.h gi_cands).  A sphere outside a
// ray's mask provably fails pair_closest_step's candidate test (its D < 0 or b >= 0), so each lane walks only its own candidates, lowest index
// first, rows from LDS: best_update sees the same candidates in the same order, and every decision is the one of the loop over every
// sphere.  A wave with a lane that names every sphere (no mask for it) takes that loop.  GIM = false: the loop over every sphere only,
// compiled without any of the masked walk (kernels that run without masks keep their code).
template <bool GIM>
SKR_DEV void closest_pair_deferred(const SceneView &sv, f3 o, f3 d0, f3 d1, bool second, const RayPair &rp, BestState &s0, BestState &s1,
								   uint32_t cand, uint32_t all)
{
	s0 = s1 = best_none();
	auto test = [&](const float4 g, int i) { pair_closest_step(rp, o, second, g, i, s0, s1); };
	bool masked = GIM;
	if constexpr(GIM)
	{
		diag_mask_gate(25, cand, sv.ns);
		DIAG_WAVE(31, __any(cand == all) ? 1u : 0u);
		masked = !__any(cand == all);
	}
	if(GIM && masked) masked_rows(sv, cand, test);
	else sphere_rows(sv, test);
	best_resolve(sv, o, d0, rp.four_a.x, s0);
	if(second) best_resolve(sv, o, d1, rp.four_a.y, s1);
}


// GIM: the kernel runs with GI masks (p.gi_index set; the launcher picks it); `row` = the lane's origin row (shade_common.h
// gi_origin_row), -1 = none; SH: the facts of the launch that are compiled in (shade_common.h RunTimeShape: none)
template <bool GIM, typename SH = RunTimeShape>
SKR_DEV void closest_pair(const SceneView &sv, const RenderParams &p, int row, f3 o, f3 d0, f3 d1, bool second, const RayPair &rp, BestState &s0, BestState &s1)
{
	const uint32_t cand = GIM ? gi_cands<SH>(p, row, d0, d1, second) : 0u;
	closest_pair_deferred<GIM>(sv, o, d0, d1, second, rp, s0, s1, cand, p.gi_all);
}

// the image row of row `orow` of the compact output (include/skr.h skr_render_tiles / skr_render_tile_list); >= height: no such row
SKR_DEV uint32_t image_row(const RenderParams &p, uint32_t orow)
{
	const uint32_t k = orow / p.tile_rows;
	const uint32_t t = p.tile_table ? p.tile_table[k] : p.first_tile + k * p.tile_stride;
	if(t == 0xFFFFFFFFu) return 0xFFFFFFFFu;
	return t * p.tile_rows + (orow - k * p.tile_rows);
}

SKR_DEV void primary_ray(const RenderParams &p, int x, uint32_t y, uint32_t pixel, uint32_t aa, f3 &dir)
{ // main.cpp:140-182
	float u, v;
	if(p.grid_size > 0)
	{
		uint32_t rnd[4];
		philox4x32(pixel, aa, 0u, 0xFFFFFFFFu, p.seed_lo, p.seed_hi, rnd);
		const float r = u31_to_unit(rnd[0]);
		u = ((2 * (((float) x + r) * p.inv_width) - 1) * p.angle) * p.aspect;
		v = (1 - 2 * (((float) (int) y + r) * p.inv_height)) * p.angle;
	}
	else
	{
		u = (float) (((2 * (((double) x + 0.5) * (double) p.inv_width) - 1) * (double) p.angle) * (double) p.aspect);
		v = (float) ((1 - 2 * (((double) (int) y + 0.5) * (double) p.inv_height)) * (double) p.angle);
	}
	dir = (p.cam_dir + p.cam_right * u) + p.cam_up * v;
}

// The lens sample of (pixel, aa) and the ray (o2, d2) it makes of the pinhole direction d (include/skr.h skr_scene_set_lens, DESIGN.md
// 8.15): one Philox call at node 0 with the counter word SKR_LENS_CTR3, then binary32 with one correctly rounded operation per step.
// phi <= (float) 2 pi: inside the range sincos_spec is exhaustively checked on.  Every kernel that forms a camera ray under a lens calls
// this — the level pipeline's trace kernel, its activate kernel for the origin alone (the same draw, the same o2), the camera-ray kernels.
SKR_DEV void lens_ray(const RenderParams &p, const Lens &lens, uint32_t pixel, uint32_t aa, f3 d, f3 &o2, f3 &d2, float *sample = nullptr)
{
	uint32_t rnd[4];
	philox4x32(pixel, aa, 0u, lens_ctr3(), p.seed_lo, p.seed_hi, rnd);
	const float u1 = u31_to_unit(rnd[0]), u2 = u31_to_unit(rnd[1]);
	const float r = sk_sqrtf(u1);
	float sn, cs;
	sincos_spec(0x1.921fb6p+2f * u2, sn, cs); // (float) 2 pi times u2, in binary32
	const float lx = r * cs, ly = r * sn;
	o2 = (p.cam_pos + p.cam_right * (lens.A * lx)) + p.cam_up * (lens.A * ly);
	d2 = (d - p.cam_right * (lens.k * lx)) - p.cam_up * (lens.k * ly);
	if(sample)
	{
		sample[0] = lx;
		sample[1] = ly;
	}
}

// The shutter time of sample (pixel, aa) of a scene in motion (include/skr.h skr_scene_set_sphere_velocities): one Philox
// call at node 0 with the counter word SKR_SHUTTER_CTR3, tau = S * u in one binary32 multiply.  The one copy of the draw: every lane that
// searches the spheres of a sample or forms a normal on one calls this with the pixel word of its tree's root — a trace lane with
// y * width + x, the query ray's key or its parent node's pixel word, an activate lane with its node's — so nothing of the draw is
// carried in a record or a node (as direct_light_cone draws a light's sample again).
SKR_DEV float shutter_time(const RenderParams &p, uint32_t pixel, uint32_t aa, float S)
{
	uint32_t rnd[4];
	philox4x32(pixel, aa, 0u, shutter_ctr3(), p.seed_lo, p.seed_hi, rnd);
	return S * u31_to_unit(rnd[0]);
}

// The environment lookup (include/skr.h skr_scene_set_environment): the one copy of the rule.  env_taps is its steps 1-5
// — the octahedral fold of d and the four bilinear taps — in binary32 with one correctly rounded operation per step (the unit is
// compiled without contraction); false: the background arm (!(s > 0) or s not finite).  Behind a finite s > 0 every |component| <= s,
// so px, pz lie in [-1, 1], u, v in [0, 1] and x, y in [-0.5, E - 0.5]: the int conversions are exact and small, and the indices are
// clamped to [0, E - 1] before any address is formed.
struct EnvTaps {
	int32_t i0, i1, j0, j1;
	float fx, fy;
};
SKR_DEV bool env_taps(f3 d, int32_t E, EnvTaps &t)
{
	const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
	const float s = (ax + ay) + az;
	if(!(s > 0.0f) || !(s < __builtin_inff())) return false;
	const float px = d.x / s, pz = d.z / s;
	float qx = px, qz = pz;
	if(d.y < 0.0f)
	{
		qx = (1.0f - __builtin_fabsf(pz)) * (px < 0.0f ? -1.0f : 1.0f);
		qz = (1.0f - __builtin_fabsf(px)) * (pz < 0.0f ? -1.0f : 1.0f);
	}
	const float u = qx * 0.5f + 0.5f, v = qz * 0.5f + 0.5f;
	const float fe = (float) E;
	const float x = u * fe - 0.5f, y = v * fe - 0.5f;
	const float x0 = __builtin_floorf(x), y0 = __builtin_floorf(y);
	t.fx = x - x0;
	t.fy = y - y0;
	auto clamp = [E](int32_t i) { return i < 0 ? 0 : i > E - 1 ? E - 1 : i; };
	const int32_t ix = (int32_t) x0, iy = (int32_t) y0;
	t.i0 = clamp(ix);
	t.i1 = clamp(ix + 1);
	t.j0 = clamp(iy);
	t.j1 = clamp(iy + 1);
	return true;
}
// env(d): four clamped float4 gathers {r, g, b, 0}, then step 6 per channel.  A lane's taps are its own (divergent directions): vector
// loads, two neighbouring texels of a row side by side.
SKR_DEV f3 env_lookup(const EnvMap &e, f3 d, f3 background)
{
	EnvTaps t;
	if(!env_taps(d, e.edge, t)) return background;
	const float4 *r0 = e.texels + (size_t) t.j0 * (size_t) e.edge, *r1 = e.texels + (size_t) t.j1 * (size_t) e.edge;
	const float4 a = r0[t.i0], b = r0[t.i1], c = r1[t.i0], g = r1[t.i1];
	const f3 a3 = mk3(a.x, a.y, a.z), c3 = mk3(c.x, c.y, c.z);
	const f3 top = a3 + (mk3(b.x, b.y, b.z) - a3) * t.fx;
	const f3 bot = c3 + (mk3(g.x, g.y, g.z) - c3) * t.fx;
	return top + (bot - top) * t.fy;
}

SKR_DEV void emit_sample(const RenderParams &p, uint32_t out_pix, f3 c)
{ // one sample of one pixel is final: store it (1 spp) or add it to the running sum (AA, sample order = launch order)
	if(p.grid_size > 0)
	{
		float *a = p.acc + (size_t) out_pix * 3;
		if(p.aa_index == 0) { a[0] = c.x; a[1] = c.y; a[2] = c.z; }
		else { a[0] = a[0] + c.x; a[1] = a[1] + c.y; a[2] = a[2] + c.z; }
	}
	else
	{
		if(p.rgbf)
		{
			float *o = p.rgbf + (size_t) out_pix * 3;
			o[0] = c.x; o[1] = c.y; o[2] = c.z;
		}
		if(p.rgb)
		{
			unsigned char *o = p.rgb + (size_t) out_pix * 3;
			o[0] = (unsigned char) quantise(c.x);
			o[1] = (unsigned char) quantise(c.y);
			o[2] = (unsigned char) quantise(c.z);
		}
	}
}

// ---- tables of the level pipelines (render_nodes.hip, render_generic.hip) ----
// Hit records of a level are appended to SKR_P1_REGIONS regions (region = trace wave index mod 64: a region only receives hits of its
// own waves); the level's counter block: [STRIDE r] records in region r, [STRIDE (64 + r)] units handed out, [STRIDE 128] the
// exhausted-regions mask, [STRIDE 129 ..] prefix sums.
SKR_DEV uint32_t *lc_count(uint32_t *ctr, uint32_t region) { return ctr + SKR_PULL_STRIDE * region; }
SKR_DEV uint32_t *lc_taken(uint32_t *ctr, uint32_t region) { return ctr + SKR_PULL_STRIDE * (SKR_P1_REGIONS + region); }
SKR_DEV unsigned long long *lc_dead(uint32_t *ctr) { return reinterpret_cast<unsigned long long *>(ctr + SKR_PULL_STRIDE * (2u * SKR_P1_REGIONS)); }
SKR_DEV uint32_t *lc_prefix(uint32_t *ctr) { return ctr + SKR_PULL_STRIDE * (2u * SKR_P1_REGIONS + 1u); } // 65 words: records before region r; [64] = all
constexpr size_t LVL_CTR_WORDS = (size_t) SKR_PULL_STRIDE * (2u * SKR_P1_REGIONS + 2u); // the whole block: counts, taken, mask, prefix
static inline uint32_t *lc_prefix_host(uint32_t *ctr) { return ctr + SKR_PULL_STRIDE * (2u * SKR_P1_REGIONS + 1u) + 64; } // (host) lc_prefix [64]: the level's record count, for a kernel argument

// the kernel's view of the scene SoA that stage_scene() staged at lds4 (a kernel may form it again from its launch constants: render_nodes.hip)
SKR_DEV SceneView scene_view(const RenderParams &p, float4 *lds4, bool tris)
{
	const int ns = p.n_spheres, nl = p.n_lights;
	float4 *s_geom = lds4, *s_amb = lds4 + ns + 1, *s_kd = s_amb + ns, *s_ks = s_kd + ns, *s_lights = s_ks + ns;
	return SceneView{s_geom, s_amb, s_kd, s_ks, s_lights, p.tris, ns, tris ? p.n_tris : 0, nl, p.tri_chunks, p.n_tri_chunks, p.tri_chunk_size, p.tri_cones, p.tri_work, p.sph_geom,
					 p.shadow_masks, p.shadow_reach2, p.shadow_all};
}

// the scene SoA staged into the workgroup's LDS (one __syncthreads); returns the kernel's view of it
SKR_DEV SceneView stage_scene(const RenderParams &p, float4 *lds4, bool tris)
{
	const int ns = p.n_spheres, nl = p.n_lights;
	float4 *s_geom = lds4, *s_amb = lds4 + ns + 1, *s_kd = s_amb + ns, *s_ks = s_kd + ns, *s_lights = s_ks + ns;
	const int tid = threadIdx.x;
	for(int i = tid; i < ns; i += 256)
	{
		s_geom[i] = p.sph_geom[i];
		s_amb[i] = p.sph_amb[i];
		s_kd[i] = p.sph_kd[i];
		s_ks[i] = p.sph_ks[i];
	}
	for(int i = tid; i < 2 * nl; i += 256) s_lights[i] = p.lights[i];
	if(tid == 0) s_geom[ns] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	__syncthreads();
	return scene_view(p, lds4, tris);
}

SKR_DEV void add_counters(const RenderParams &p, const Counters &cn, uint32_t shard, int lane)
{
	if(!p.counters) return;
	const uint32_t a = wave_sum(cn.rays), b = wave_sum(cn.hits), c = wave_sum(cn.shadow_rays), d4 = wave_sum(cn.shadow_tests);
	if(lane == 0)
	{ // sharded: thousands of waves adding to one word serialise
		unsigned long long *c4 = p.counters + 4u * (shard & (SKR_COUNTER_SHARDS - 1u));
		if(a) atomicAdd(&c4[0], (unsigned long long) a);
		if(b) atomicAdd(&c4[1], (unsigned long long) b);
		if(c) atomicAdd(&c4[2], (unsigned long long) c);
		if(d4) atomicAdd(&c4[3], (unsigned long long) d4);
	}
}

struct F3p { float x, y, z; } __attribute__((packed, aligned(4)));
SKR_DEV void store3(float *g, f3 v) { *reinterpret_cast<F3p *>(g) = F3p{v.x, v.y, v.z}; }

// Prefix sums of a level's 64 region counts (the dense numbering of its records), formed by the first wave of a workgroup
// into 65 words of LDS: s_pre[r] = records before region r, s_pre[64] = all.  `publish`: also written behind the level's
// counters, where the kernels launched later read the level's record count (lc_prefix_host).  Ends in a workgroup barrier.
SKR_DEV void region_prefix(const RenderParams &p, uint32_t *s_pre, bool publish)
{
	if(threadIdx.x < 64)
	{
		const int lane = threadIdx.x;
		const uint32_t v = *lc_count(p.rc_ctr, (uint32_t) lane);
		uint32_t incl = v;
#pragma unroll
		for(int off = 1; off < 64; off <<= 1)
		{
			const uint32_t o = (uint32_t) __shfl_up((int) incl, off, 64);
			if(lane >= off) incl += o;
		}
		s_pre[lane] = incl - v;
		if(lane == 63) s_pre[64] = incl;
		if(publish)
		{
			uint32_t *pre = lc_prefix(p.rc_ctr);
			pre[lane] = incl - v;
			if(lane == 63) pre[64] = incl;
		}
	}
	__syncthreads();
}

// The tree a wave of query rays walks (launch.h QueryTrees), into sv.chunks / cones / nchunks (nchunks = 0: every
// triangle).  The bound is the smallest of SKR_CULL_DMAX_LIST above every live lane's |d| (0.2 % short of it: room for the rounding of
// d.d; NaN and inf: none).  Then (a) every live lane at the scene camera `cam` bit for bit, or `surface` (the rays start on surfaces):
// the renderer's tree, which holds for such origins; (b) every live lane inside the trace ball: the trace tree; (c) otherwise no tree.
// All three give the same answers.  (q by value: read through a reference into the kernel argument, the shading query's trace kernel
// spills one SGPR fewer and its instructions change.)
SKR_DEV void pick_query_tree(SceneView &sv, const QueryTrees q, f3 cam, bool surface, bool live, f3 o, f3 d)
{
	sv.nchunks = 0;
	if(sv.nt == 0 || q.nchunks == 0) return;
	constexpr float lim[SKR_CULL_LEVELS] = {(float) (4.0 * 4.0 * 0.998), (float) (32.0 * 32.0 * 0.998), (float) (256.0 * 256.0 * 0.998)};
	const float dd = dot3(d, d);
	int level = 0;
	while(level < SKR_CULL_LEVELS && !__all(!live || dd < lim[level])) level++;
	if(level == SKR_CULL_LEVELS) return;
	const bool at_cam = __float_as_uint(o.x) == __float_as_uint(cam.x) && __float_as_uint(o.y) == __float_as_uint(cam.y) &&
						__float_as_uint(o.z) == __float_as_uint(cam.z);
	const f3 e = o - mk3(q.ball.x, q.ball.y, q.ball.z);
	if(surface || __all(!live || at_cam))
	{
		sv.chunks = q.tree + (size_t) level * q.stride;
		sv.cones = q.cones;
		sv.nchunks = q.nchunks;
	}
	else if(q.trace && __all(!live || dot3(e, e) <= q.ball.w * q.ball.w))
	{
		sv.chunks = q.trace + (size_t) level * q.stride;
		sv.cones = q.trace_cones;
		sv.nchunks = q.nchunks;
	}
}

} // namespace
