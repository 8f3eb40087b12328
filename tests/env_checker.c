/* The CPU checker of the environment map (include/skr.h skr_scene_set_environment).  Wherever the miss return is not
 * involved it reuses the checker chain by inclusion: tests/motion_checker.c whole, and through it the lens, soft-light and spot
 * checkers and oracle/skr_oracle.c — the shutter draw and the displaced centres (motion_tau, fmaf), the lens rays (lens_rays), the light
 * loop (sl_direct) and the oracle's geometry are called, not copied.  What is restated here is only what returns a miss: the shade
 * function and its GI loop (env_shade, env_gi: sl_shade and sl_gi statement for statement, without the legacy terms the environment
 * refuses) and the per-ray entry (env_shade_rays: lens_shade_rays with motion_shade_rays' displacement), in which a miss returns env(d),
 * and the lookup itself (env_taps, env_lookup: the rule's steps in binary32, one operation per step).  It counts the lookups at level 0
 * (a primary or query ray) and at levels >= 1 (--gillum children).  With a constant map equal to the scene's background a composed frame
 * must reproduce sko_render, and the motion, lens and soft-light checkers, bit for bit, counts included (tests/test_env_cpu.py checks that
 * first: only then is this file evidence).  Test infrastructure; the product never loads it.  Built by tests/env_check.py with the
 * oracle's flags (-ffp-contract=off). */
#include "motion_checker.c"

typedef struct {
	int32_t i0, i1, j0, j1;
	float fx, fy;
} env_tap;

static int32_t env_clamp(int32_t i, int32_t E) { return i < 0 ? 0 : i > E - 1 ? E - 1 : i; }

/* Steps 1-5 of the rule.  Returns 1 for the background arm (*t untouched), else 0. */
int env_taps(const float d[3], int32_t E, env_tap *t)
{
	const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
	const float axy = ax + ay;
	const float s = axy + az;
	if(!(s > 0.0f) || !isfinite(s)) return 1;
	const float px = d[0] / s, pz = d[2] / s;
	float qx = px, qz = pz;
	if(d[1] < 0.0f)
	{
		const float ox = 1.0f - fabsf(pz), oz = 1.0f - fabsf(px);
		qx = ox * (px < 0.0f ? -1.0f : 1.0f);
		qz = oz * (pz < 0.0f ? -1.0f : 1.0f);
	}
	const float hu = qx * 0.5f, hv = qz * 0.5f;
	const float u = hu + 0.5f, v = hv + 0.5f;
	const float fe = (float) E;
	const float ux = u * fe, vy = v * fe;
	const float x = ux - 0.5f, y = vy - 0.5f;
	const float x0 = floorf(x), y0 = floorf(y);
	t->fx = x - x0;
	t->fy = y - y0;
	t->i0 = env_clamp((int32_t) x0, E);
	t->i1 = env_clamp((int32_t) x0 + 1, E);
	t->j0 = env_clamp((int32_t) y0, E);
	t->j1 = env_clamp((int32_t) y0 + 1, E);
	return 0;
}

/* env(d): texels float[E][E][3], row j first.  Returns 1 where the background arm was taken (out = background). */
int env_lookup(const float *texels, int32_t E, const float d[3], const float background[3], float out[3])
{
	env_tap t;
	if(env_taps(d, E, &t))
	{
		memcpy(out, background, 12);
		return 1;
	}
	for(int c = 0; c < 3; c++)
	{
		const float a = texels[((size_t) t.j0 * E + t.i0) * 3 + c], b = texels[((size_t) t.j0 * E + t.i1) * 3 + c];
		const float e = texels[((size_t) t.j1 * E + t.i0) * 3 + c], f = texels[((size_t) t.j1 * E + t.i1) * 3 + c];
		const float dt = b - a, db = f - e;
		const float mt = t.fx * dt, mb = t.fx * db;
		const float top = a + mt, bot = e + mb;
		const float dv = bot - top;
		const float mv = t.fy * dv;
		out[c] = top + mv;
	}
	return 0;
}

/* One record of skr_debug_eval's op 25: (d(3), E) -> (flag, i0, i1, j0, j1, fx, fy); the six behind a flag of 1 are 0 */
void env_records(const uint32_t *in, int64_t n, uint32_t *out)
{
	for(int64_t i = 0; i < n; i++)
	{
		float d[3];
		memcpy(d, in + 4 * i, 12);
		env_tap t;
		uint32_t *w = out + 7 * i;
		memset(w, 0, 28);
		if(env_taps(d, (int32_t) in[4 * i + 3], &t))
		{
			w[0] = 1u;
			continue;
		}
		w[1] = (uint32_t) t.i0; w[2] = (uint32_t) t.i1; w[3] = (uint32_t) t.j0; w[4] = (uint32_t) t.j1;
		memcpy(w + 5, &t.fx, 4);
		memcpy(w + 6, &t.fy, 4);
	}
}

typedef struct {
	sl_ctx tx;
	const float *texels; /* NULL: no environment, a miss returns the background */
	int32_t edge;
	uint64_t look0, look1; /* lookups at level 0, at levels >= 1 */
} env_ctx;

/* what a miss of a ray with direction d at `level` returns */
static v3 env_miss(env_ctx *ex, v3 d, int level)
{
	const sko_scene *sc = ex->tx.cx.sc;
	if(!ex->texels) return sc->background;
	const float dv[3] = {d.x, d.y, d.z}, bg[3] = {sc->background.x, sc->background.y, sc->background.z};
	float o[3];
	env_lookup(ex->texels, ex->edge, dv, bg, o);
	if(level == 0) ex->look0++;
	else ex->look1++;
	return V(o[0], o[1], o[2]);
}

static v3 env_shade(env_ctx *ex, v3 o, v3 d, int depth, uint32_t node, int from_triangle, int level);

/* sl_gi() whose children are env_shade's */
static v3 env_gi(env_ctx *ex, v3 P, v3 N, int depth, uint32_t node, int from_triangle, int level)
{
	ctx_t *cx = &ex->tx.cx;
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
			child = env_shade(ex, vadds(P, 0.00001f), w, depth - 1, node * node_arity(cx) + (uint32_t) i + 1u, from_triangle, level + 1);
		}
		total = vadd(total, vdivs(vscale(child, r1), pdf));
	}
	total = vdivs(total, (float) n_rays);
	return total;
}

/* sl_shade() in which a miss returns env(d) */
static v3 env_shade(env_ctx *ex, v3 o, v3 d, int depth, uint32_t node, int from_triangle, int level)
{
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
	{
		const sko_triangle *tr = &sc->triangles[hit_triangle];
		const sko_sphere *mt = &sc->triangle_materials[hit_triangle];
		v3 P = vadd(o, vscale(d, min_distance));
		v3 N = vnormalize(vcross(vsub(tr->v1, tr->v0), vsub(tr->v2, tr->v0)));
		if(vdot(N, d) > 0.0f) N = V(-N.x, -N.y, -N.z);
		cx->n_hits++;
		v3 direct = sl_direct(tx, mt, P, N, hit_triangle, node);
		if(cx->op->monte_carlo)
		{
			v3 indirect = env_gi(ex, P, N, depth, node, hit_triangle, level);
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
		v3 direct = sl_direct(tx, sp, P, N, -1, node);
		if(cx->op->monte_carlo)
		{
			v3 indirect = env_gi(ex, P, N, depth, node, -1, level);
			return vmul(vadd(vdivs(direct, (float) M_PI), vscale(indirect, 2.0f)), sp->diffuse);
		}
		return direct;
	}
	return V(0, 0, 0);
}

/* lens_shade_rays with motion_shade_rays' displacement (in_force = 0: the scene as it lies, no draw) and the environment (texels NULL:
 * none).  stats[7] are added to: the five work counts of lens_shade_rays, then the lookups at level 0 and at levels >= 1. */
int env_shade_rays(const sko_scene *scene, const sko_options *opt, int tri_shadows, int n_spot, const float *spot_rows, const float *spot_cones, const float *radii,
				   const float *velocities, float S, int in_force, const float *texels, int32_t edge, const float *rays, int64_t n, uint32_t sample, const uint32_t *keys,
				   float *out, uint64_t *stats)
{
	if(!sl_options_ok(opt, n_spot) || n_spot < 0 || opt->legacy_reflect || (texels && edge < 1)) return 1;
	const int ns = scene->n_spheres;
	uint64_t tot[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma omp parallel reduction(+ : tot[:7])
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
			env_ctx ex = {{{&sc, opt, key, sample, 0, 0, 0, 0, 0}, tri_shadows, n_spot, spot_rows, spot_cones, radii}, texels, edge, 0, 0};
			v3 c;
			if(sl_first_segment_t(&sc, opt, o, d, from_triangle) < ray[3]) c = env_shade(&ex, o, d, opt->max_depth, 0, from_triangle, 0);
			else
			{ /* the winner lies at or beyond tmax: a miss, which has tested every sphere and triangle */
				ex.tx.cx.n_rays++;
				ex.tx.cx.n_sph_tests += (uint64_t) sc.n_spheres;
				ex.tx.cx.n_tri_tests += (uint64_t) sc.n_triangles;
				c = env_miss(&ex, d, 0);
			}
			out[3 * i] = c.x;
			out[3 * i + 1] = c.y;
			out[3 * i + 2] = c.z;
			tot[0] += ex.tx.cx.n_rays;
			tot[1] += ex.tx.cx.n_hits;
			tot[2] += ex.tx.cx.n_shadow;
			tot[3] += ex.tx.cx.n_sph_tests;
			tot[4] += ex.tx.cx.n_tri_tests;
			tot[5] += ex.look0;
			tot[6] += ex.look1;
		}
		free(moved);
	}
	for(int k = 0; k < 7; k++) stats[k] += tot[k];
	return 0;
}
