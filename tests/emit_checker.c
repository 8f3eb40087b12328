/* The CPU checker of emissive spheres (include/skr.h skr_scene_set_sphere_emission).  It reuses the checker chain by
 * inclusion: tests/tex_checker.c whole, and through it the environment, motion, lens, soft-light and spot checkers and
 * oracle/skr_oracle.c — the light loop on the primed rows (tex_direct), the miss return (env_miss) and the oracle's geometry are called,
 * not copied.  What is restated here is the shade function and its GI loop (emit_shade, emit_gi: tex_shade and tex_gi statement for
 * statement) with the one add at a sphere hit, and nothing else:
 *   v' = v + e_i          one binary32 add per component behind the final `* kd` (or behind `direct` where the launch is no Monte-Carlo one).
 * It counts the adds whose e_i has a component > 0, and reports the surface every ray's first segment ends on.  With emission NULL, or
 * all zero, a frame must reproduce tex_shade_rays bit for bit, counts included (tests/test_emit_cpu.py checks that first: only then is
 * this file evidence).  Test infrastructure; the product never loads it.  Built by tests/emit_check.py with the oracle's flags
 * (-ffp-contract=off). */
#include "tex_checker.c"

typedef struct {
	tex_ctx xx;
	const float *emission; /* [n_spheres][3]; NULL: no sphere glows */
	uint64_t adds;         /* sphere hits whose e_i has a component > 0 */
	int32_t winner;        /* the surface the level-0 ray ends on: a sphere index, -1 a miss, -2 - i triangle i */
} emit_ctx;

static v3 emit_shade(emit_ctx *ee, v3 o, v3 d, int depth, uint32_t node, int from_triangle, int level);

/* tex_gi() whose children are emit_shade's */
static v3 emit_gi(emit_ctx *ee, v3 P, v3 N, int depth, uint32_t node, int from_triangle, int level)
{
	ctx_t *cx = &ee->xx.ex.tx.cx;
	const int n_rays = cx->op->num_path_traces;
	v3 total = V(0, 0, 0);
	v3 nt, nb;
	basis(N, &nt, &nb);
	float pdf = (float) (1 / M_PI);
	for(int i = 0; i < n_rays; i++)
	{
		float r1 = 0.0f, r2 = 0.0f;
		v3 child = V(0, 0, 0);
		if(depth - 1 > 0)
		{
			sko_counter_draws(cx->op->seed, cx->pixel, cx->aa, node, (uint32_t) i, &r1, &r2);
			v3 s = sample_hemi(cx, r1, r2);
			v3 w = V(s.x * nb.x + s.y * N.x + s.z * nt.x, s.x * nb.y + s.y * N.y + s.z * nb.y, s.x * nb.z + s.y * N.z + s.z * nb.z);
			child = emit_shade(ee, vadds(P, 0.00001f), w, depth - 1, node * node_arity(cx) + (uint32_t) i + 1u, from_triangle, level + 1);
		}
		total = vadd(total, vdivs(vscale(child, r1), pdf));
	}
	total = vdivs(total, (float) n_rays);
	return total;
}

/* tex_shade() with the add at a sphere hit */
static v3 emit_shade(emit_ctx *ee, v3 o, v3 d, int depth, uint32_t node, int from_triangle, int level)
{
	tex_ctx *xx = &ee->xx;
	env_ctx *ex = &xx->ex;
	sl_ctx *tx = &ex->tx;
	ctx_t *cx = &tx->cx;
	const sko_scene *sc = cx->sc;
	if(depth <= 0) return V(0, 0, 0);
	cx->n_rays++;
	float min_distance = INFINITY;
	int hit_sphere = -1;
	int hit_a_sphere = 0, hit_a_triangle = 0;
	for(int i = 0; i < sc->n_spheres; i++)
	{
		cx->n_sph_tests++;
		float distance = collision_distance(o, d, &sc->spheres[i]);
		if(intersection_occurs(distance))
		{
			hit_a_sphere = 1;
			if(distance < min_distance)
			{
				min_distance = distance;
				hit_sphere = i;
			}
		}
	}
	int hit_triangle = -1;
	for(int i = 0; i < sc->n_triangles; i++)
	{
		float t;
		cx->n_tri_tests++;
		if(triangle_test(o, d, &sc->triangles[i], &t))
		{
			if(cx->op->shade_triangles && (!(t > 0.0f) || i == from_triangle)) continue;
			if(t < min_distance)
			{
				min_distance = t;
				hit_a_sphere = 0;
				hit_a_triangle = 1;
				hit_triangle = i;
			}
		}
	}
	if(level == 0) ee->winner = hit_a_triangle ? -2 - hit_triangle : hit_a_sphere ? hit_sphere : -1;
	if(!hit_a_sphere && !hit_a_triangle) return env_miss(ex, d, level);
	if(hit_a_triangle && cx->op->shade_triangles)
	{ /* triangles have no texture and no emission */
		const sko_triangle *tr = &sc->triangles[hit_triangle];
		const sko_sphere *mt = &sc->triangle_materials[hit_triangle];
		v3 P = vadd(o, vscale(d, min_distance));
		v3 N = vnormalize(vcross(vsub(tr->v1, tr->v0), vsub(tr->v2, tr->v0)));
		if(vdot(N, d) > 0.0f) N = V(-N.x, -N.y, -N.z);
		cx->n_hits++;
		v3 direct = sl_direct(tx, mt, P, N, hit_triangle, node);
		if(cx->op->monte_carlo)
		{
			v3 indirect = emit_gi(ee, P, N, depth, node, hit_triangle, level);
			return vmul(vadd(vdivs(direct, (float) M_PI), vscale(indirect, 2.0f)), mt->diffuse);
		}
		return direct;
	}
	if(hit_a_sphere)
	{
		const sko_sphere *sp = &sc->spheres[hit_sphere];
		float t = collision_distance(o, d, sp);
		v3 P = vadd(o, vscale(d, t));
		v3 N = vnormalize(vsub(P, sp->center));
		cx->n_hits++;
		v3 kd;
		v3 v = tex_direct(xx, sp, hit_sphere, P, N, node, &kd);
		if(cx->op->monte_carlo)
		{
			v3 indirect = emit_gi(ee, P, N, depth, node, -1, level);
			v = vmul(vadd(vdivs(v, (float) M_PI), vscale(indirect, 2.0f)), kd);
		}
		if(ee->emission)
		{ /* the rule: v + e_i */
			const float *e = ee->emission + 3 * hit_sphere;
			if(e[0] > 0.0f || e[1] > 0.0f || e[2] > 0.0f) ee->adds++;
			v = vadd(v, V(e[0], e[1], e[2]));
		}
		return v;
	}
	return V(0, 0, 0);
}

/* tex_shade_rays with the emission (NULL: none).  stats[9] are added to: tex_shade_rays' eight, then the adds at emitters.  winner (if
 * not NULL) receives per ray the surface its first segment ends on (a sphere index, -1 a miss or a winner beyond tmax, -2 - i triangle i). */
int emit_shade_rays(const sko_scene *scene, const sko_options *opt, int tri_shadows, int n_spot, const float *spot_rows, const float *spot_cones, const float *radii,
					const float *velocities, float S, int in_force, const float *env_texels, int32_t env_edge, const float *tex_texels, const int64_t *tex_first,
					const int32_t *tex_edges, const int32_t *sphere_tex, const float *emission, const float *rays, int64_t n, uint32_t sample, const uint32_t *keys, float *out,
					int32_t *winner, uint64_t *stats)
{
	if(!sl_options_ok(opt, n_spot) || n_spot < 0 || opt->legacy_reflect || (env_texels && env_edge < 1)) return 1;
	const int ns = scene->n_spheres;
	uint64_t tot[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma omp parallel reduction(+ : tot[:9])
	{
		sko_sphere *moved = (sko_sphere *) malloc(sizeof(sko_sphere) * (size_t) (ns > 0 ? ns : 1));
		sko_scene sc = *scene;
		if(in_force) sc.spheres = moved;
#pragma omp for schedule(dynamic, 16)
		for(int64_t i = 0; i < n; i++)
		{
			const float *ray = rays + 8 * i;
			const uint32_t key = keys ? keys[i] : (uint32_t) i;
			if(in_force)
			{
				const float tau = motion_tau(key, sample, (uint32_t) opt->seed, (uint32_t) (opt->seed >> 32), S);
				for(int s = 0; s < ns; s++)
				{
					moved[s] = scene->spheres[s];
					moved[s].center.x = fmaf(tau, velocities[3 * s], scene->spheres[s].center.x);
					moved[s].center.y = fmaf(tau, velocities[3 * s + 1], scene->spheres[s].center.y);
					moved[s].center.z = fmaf(tau, velocities[3 * s + 2], scene->spheres[s].center.z);
				}
			}
			int32_t ignore;
			memcpy(&ignore, ray + 7, 4);
			const v3 o = V(ray[0], ray[1], ray[2]), d = V(ray[4], ray[5], ray[6]);
			const int from_triangle = opt->shade_triangles ? ignore : -1;
			emit_ctx ee = {{{{{&sc, opt, key, sample, 0, 0, 0, 0, 0}, tri_shadows, n_spot, spot_rows, spot_cones, radii}, env_texels, env_edge, 0, 0},
							tex_texels, tex_first, tex_edges, sphere_tex, 0},
						   emission, 0, -1};
			v3 c;
			if(sl_first_segment_t(&sc, opt, o, d, from_triangle) < ray[3]) c = emit_shade(&ee, o, d, opt->max_depth, 0, from_triangle, 0);
			else
			{ /* the winner lies at or beyond tmax: a miss, which has tested every sphere and triangle */
				ee.xx.ex.tx.cx.n_rays++;
				ee.xx.ex.tx.cx.n_sph_tests += (uint64_t) sc.n_spheres;
				ee.xx.ex.tx.cx.n_tri_tests += (uint64_t) sc.n_triangles;
				c = env_miss(&ee.xx.ex, d, 0);
			}
			out[3 * i] = c.x;
			out[3 * i + 1] = c.y;
			out[3 * i + 2] = c.z;
			if(winner) winner[i] = ee.winner;
			tot[0] += ee.xx.ex.tx.cx.n_rays;
			tot[1] += ee.xx.ex.tx.cx.n_hits;
			tot[2] += ee.xx.ex.tx.cx.n_shadow;
			tot[3] += ee.xx.ex.tx.cx.n_sph_tests;
			tot[4] += ee.xx.ex.tx.cx.n_tri_tests;
			tot[5] += ee.xx.ex.look0;
			tot[6] += ee.xx.ex.look1;
			tot[7] += ee.xx.looks;
			tot[8] += ee.adds;
		}
		free(moved);
	}
	for(int k = 0; k < 9; k++) stats[k] += tot[k];
	return 0;
}
