/* The CPU checker of sphere textures (include/skr.h skr_scene_add_texture).  It reuses the checker chain by inclusion:
 * tests/env_checker.c whole, and through it the motion, lens, soft-light and spot checkers and oracle/skr_oracle.c — the lookup
 * (env_lookup: the texture rule is the environment's steps 1-6 on the normal), the miss return (env_miss), the light loop (sl_direct)
 * and the oracle's geometry are called, not copied.  What is restated here is the shade function and its GI loop (tex_shade, tex_gi:
 * env_shade and env_gi statement for statement) with the two primed rows at a sphere that has a texture, and nothing else:
 *   kd'   = kd * c                      the sphere handed to sl_direct and the final `* diffuse` carry it;
 *   ambp' = (La * ka) * c               sl_direct forms vmul(scene ambient, sphere ambient): it is handed a scene whose ambient is the
 *                                       product La * ka already rounded (the row the device holds) and a sphere whose ambient is c, so
 *                                       its one multiply is the rule's.
 * It counts the texture lookups.  With every index -1, or with a texture of ones, a composed frame must reproduce env_shade_rays bit
 * for bit, counts included (tests/test_tex_cpu.py checks that first: only then is this file evidence).  Test infrastructure; the
 * product never loads it.  Built by tests/tex_check.py with the oracle's flags (-ffp-contract=off). */
#include "env_checker.c"

typedef struct {
	env_ctx ex;
	const float *texels;     /* every texture's float[E][E][3], one after the other */
	const int64_t *first;    /* [n_tex] where texture k starts in texels, in floats */
	const int32_t *edges;    /* [n_tex] */
	const int32_t *sphere_tex; /* [n_spheres] -1 = none; NULL: no sphere has a texture */
	uint64_t looks;
} tex_ctx;

/* tex_k(N): the environment's lookup with (1, 1, 1) where its first step fails.  Returns 1 where that arm was taken. */
int tex_colour(const float *texels, int32_t E, const float N[3], float out[3])
{
	const float one[3] = {1.0f, 1.0f, 1.0f};
	return env_lookup(texels, E, N, one, out);
}

/* the light loop at a sphere hit: sl_direct, on the primed rows where the sphere has a texture; *kd receives the row the final product takes */
static v3 tex_direct(tex_ctx *xx, const sko_sphere *sp, int sphere, v3 P, v3 N, uint32_t node, v3 *kd)
{
	sl_ctx *tx = &xx->ex.tx;
	*kd = sp->diffuse;
	const int32_t k = xx->sphere_tex ? xx->sphere_tex[sphere] : -1;
	if(k < 0) return sl_direct(tx, sp, P, N, -1, node);
	const float n[3] = {N.x, N.y, N.z};
	float c[3];
	tex_colour(xx->texels + xx->first[k], xx->edges[k], n, c);
	xx->looks++;
	const sko_scene *sc = tx->cx.sc;
	sko_scene lit = *sc;
	sko_sphere m = *sp;
	lit.ambient = vmul(sc->ambient, sp->ambient); /* ambp */
	m.ambient = V(c[0], c[1], c[2]);              /* ambp' = ambp * c */
	m.diffuse = vmul(sp->diffuse, V(c[0], c[1], c[2])); /* kd' = kd * c */
	*kd = m.diffuse;
	tx->cx.sc = &lit;
	const v3 direct = sl_direct(tx, &m, P, N, -1, node);
	tx->cx.sc = sc;
	return direct;
}

static v3 tex_shade(tex_ctx *xx, v3 o, v3 d, int depth, uint32_t node, int from_triangle, int level);

/* env_gi() whose children are tex_shade's */
static v3 tex_gi(tex_ctx *xx, v3 P, v3 N, int depth, uint32_t node, int from_triangle, int level)
{
	ctx_t *cx = &xx->ex.tx.cx;
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
			child = tex_shade(xx, vadds(P, 0.00001f), w, depth - 1, node * node_arity(cx) + (uint32_t) i + 1u, from_triangle, level + 1);
		}
		total = vadd(total, vdivs(vscale(child, r1), pdf));
	}
	total = vdivs(total, (float) n_rays);
	return total;
}

/* env_shade() with the primed rows at a sphere that has a texture */
static v3 tex_shade(tex_ctx *xx, v3 o, v3 d, int depth, uint32_t node, int from_triangle, int level)
{
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
	if(!hit_a_sphere && !hit_a_triangle) return env_miss(ex, d, level);
	if(hit_a_triangle && cx->op->shade_triangles)
	{ /* triangles have no texture */
		const sko_triangle *tr = &sc->triangles[hit_triangle];
		const sko_sphere *mt = &sc->triangle_materials[hit_triangle];
		v3 P = vadd(o, vscale(d, min_distance));
		v3 N = vnormalize(vcross(vsub(tr->v1, tr->v0), vsub(tr->v2, tr->v0)));
		if(vdot(N, d) > 0.0f) N = V(-N.x, -N.y, -N.z);
		cx->n_hits++;
		v3 direct = sl_direct(tx, mt, P, N, hit_triangle, node);
		if(cx->op->monte_carlo)
		{
			v3 indirect = tex_gi(xx, P, N, depth, node, hit_triangle, level);
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
		v3 direct = tex_direct(xx, sp, hit_sphere, P, N, node, &kd);
		if(cx->op->monte_carlo)
		{
			v3 indirect = tex_gi(xx, P, N, depth, node, -1, level);
			return vmul(vadd(vdivs(direct, (float) M_PI), vscale(indirect, 2.0f)), kd);
		}
		return direct;
	}
	return V(0, 0, 0);
}

/* env_shade_rays with the textures (sphere_tex NULL: none).  stats[8] are added to: env_shade_rays' seven, then the texture lookups. */
int tex_shade_rays(const sko_scene *scene, const sko_options *opt, int tri_shadows, int n_spot, const float *spot_rows, const float *spot_cones, const float *radii,
				   const float *velocities, float S, int in_force, const float *env_texels, int32_t env_edge, const float *tex_texels, const int64_t *tex_first,
				   const int32_t *tex_edges, const int32_t *sphere_tex, const float *rays, int64_t n, uint32_t sample, const uint32_t *keys, float *out, uint64_t *stats)
{
	if(!sl_options_ok(opt, n_spot) || n_spot < 0 || opt->legacy_reflect || (env_texels && env_edge < 1)) return 1;
	const int ns = scene->n_spheres;
	uint64_t tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma omp parallel reduction(+ : tot[:8])
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
			tex_ctx xx = {{{{&sc, opt, key, sample, 0, 0, 0, 0, 0}, tri_shadows, n_spot, spot_rows, spot_cones, radii}, env_texels, env_edge, 0, 0},
						  tex_texels, tex_first, tex_edges, sphere_tex, 0};
			v3 c;
			if(sl_first_segment_t(&sc, opt, o, d, from_triangle) < ray[3]) c = tex_shade(&xx, o, d, opt->max_depth, 0, from_triangle, 0);
			else
			{ /* the winner lies at or beyond tmax: a miss, which has tested every sphere and triangle */
				xx.ex.tx.cx.n_rays++;
				xx.ex.tx.cx.n_sph_tests += (uint64_t) sc.n_spheres;
				xx.ex.tx.cx.n_tri_tests += (uint64_t) sc.n_triangles;
				c = env_miss(&xx.ex, d, 0);
			}
			out[3 * i] = c.x;
			out[3 * i + 1] = c.y;
			out[3 * i + 2] = c.z;
			tot[0] += xx.ex.tx.cx.n_rays;
			tot[1] += xx.ex.tx.cx.n_hits;
			tot[2] += xx.ex.tx.cx.n_shadow;
			tot[3] += xx.ex.tx.cx.n_sph_tests;
			tot[4] += xx.ex.tx.cx.n_tri_tests;
			tot[5] += xx.ex.look0;
			tot[6] += xx.ex.look1;
			tot[7] += xx.looks;
		}
		free(moved);
	}
	for(int k = 0; k < 8; k++) stats[k] += tot[k];
	return 0;
}
