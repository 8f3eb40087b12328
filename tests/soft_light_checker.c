/* The CPU checker of lights with a radius (include/skr.h skr_scene_set_light_radii): the frozen oracle's integrator
 * (oracle/skr_oracle.c, included whole: its static geometry, sampling and legacy functions are called, not copied) with its shade tree
 * restated so that the sample rule — and the cone rule and the triangle-shadow rule, tests/spot_checker.c — can be added to the light
 * loop.  The restated functions — sl_direct, sl_legacy_terms, sl_gi, sl_shade, sl_render — follow direct_illumination, legacy_terms,
 * global_illumination, shade_from and sko_render statement for statement; with every radius 0 they must reproduce sko_render (no spot
 * light) and tests/spot_checker.c (spot lights) bit for bit (tests/test_soft_lights_cpu.py checks that first: only then is this file
 * evidence).  The spot lights come as arguments, as in tests/spot_checker.c: their rows [n][11] and the cones [n][5] THE LIBRARY
 * derived; the radii [n_point + n_spot] in shading order.  Test infrastructure; the product never loads it.  Built by
 * tests/soft_light_check.py with the oracle's flags (-ffp-contract=off). */
#include "skr_oracle.c"

/* The cone decision and factor (include/skr.h): a, c1, c2 as derived by the host, L the unit vector from the point to the light.
 * Binary32, one operation per step.  Returns 1 where the light is outside (*f = 0). */
static int sp_cone(const float a[3], float c1, float c2, const float L[3], float *f)
{
	const float c = -(a[0] * L[0] + a[1] * L[1] + a[2] * L[2]);
	if(c >= c1)
	{
		*f = 1.0f;
		return 0;
	}
	if(!(c > c2))
	{
		*f = 0.0f;
		return 1;
	}
	const float u = (c - c2) / (c1 - c2);
	*f = (u * u) * (3.0f - 2.0f * u);
	return 0;
}

/* The sample position of the light l at Lp with radius R for the node (pixel, aa, node) (include/skr.h): one Philox call with the
 * counter word 0x80000080 | (l << 8), then binary32, one operation per step.  R == 0: no draw, Lp itself. */
void sl_sample(uint32_t pixel, uint32_t aa, uint32_t node, uint32_t l, uint32_t seed_lo, uint32_t seed_hi, const float Lp[3], float R, float out[3])
{
	out[0] = Lp[0];
	out[1] = Lp[1];
	out[2] = Lp[2];
	if(!(R > 0.0f)) return;
	const uint32_t ctr[4] = {pixel, aa, node, 0x80000080u | (l << 8)}, key[2] = {seed_lo, seed_hi};
	uint32_t o[4];
	sko_philox4x32_spec(ctr, key, o);
	const float u1 = u31(o[0]), u2 = u31(o[1]);
	const float z = 1.0f - 2.0f * u1;
	const float s = sqrtf(max0(1.0f - z * z));
	const float phi = 0x1.921fb6p+2f * u2;
	float sn, cs;
	sko_sincos_shared(phi, &sn, &cs);
	out[0] = Lp[0] + R * (s * cs);
	out[1] = Lp[1] + R * z;
	out[2] = Lp[2] + R * (s * sn);
}

typedef struct {
	ctx_t cx;
	int tri_shadows; /* the scene's switch; in force with op->shade_triangles and op->use_shadows */
	int n_spot;      /* spot lights: shaded behind the point lights, ahead of the directional ones */
	const float *spot_rows, *spot_cones;
	const float *radii; /* [n_point + n_spot], shading order */
} sl_ctx;

static int sl_in_force(const sl_ctx *tx) { return tx->tri_shadows && tx->cx.op->shade_triangles && tx->cx.op->use_shadows && tx->cx.sc->n_triangles > 0; }

/* The rule's step 2: some triangle other than `own` accepts (o, L) with 0 < t < tmax (tmax = +inf: a directional light) */
static int triangle_occludes(const sl_ctx *tx, v3 P, v3 L, int own, float tmax)
{
	const sko_scene *sc = tx->cx.sc;
	const v3 o = vadds(P, 0.000001f);
	for(int i = 0; i < sc->n_triangles; i++)
	{
		float t;
		if(i == own) continue;
		if(triangle_test(o, L, &sc->triangles[i], &t) && t > 0.0f && t < tmax) return 1;
	}
	return 0;
}

/* the position light l at Lp is, for the node being shaded, a point light at */
static v3 sl_position(const sl_ctx *tx, uint32_t node, int l, v3 Lp)
{
	const float p[3] = {Lp.x, Lp.y, Lp.z};
	float o[3];
	sl_sample(tx->cx.pixel, tx->cx.aa, node, (uint32_t) l, (uint32_t) tx->cx.op->seed, (uint32_t) (tx->cx.op->seed >> 32), p, tx->radii[l], o);
	return V(o[0], o[1], o[2]);
}

/* direct_illumination() with the sample rule, the spot lights' loop, and the triangle-shadow rule added behind shadowed(); own: the file index of the triangle being shaded, -1 at a sphere hit */
static v3 sl_direct(sl_ctx *tx, const sko_sphere *sp, v3 P, v3 N, int own, uint32_t node)
{
	ctx_t *cx = &tx->cx;
	const sko_scene *sc = cx->sc;
	v3 ambient = vmul(sc->ambient, sp->ambient);
	v3 diffuse = V(0, 0, 0), specular = V(0, 0, 0);
	v3 view = vnormalize(vsub(sc->cam_pos, P));
	for(int i = 0; i < sc->n_point_lights; i++)
	{
		const sko_point_light *pl = &sc->point_lights[i];
		v3 to_l = vsub(sl_position(tx, node, i, pl->position), P);
		v3 L = vnormalize(to_l);
		if(cx->op->use_shadows && shadowed(cx, P, L)) continue;
		float distance = vlength(to_l);
		if(sl_in_force(tx) && triangle_occludes(tx, P, L, own, distance)) continue;
		float intensity = 1.0f / sq_mode(cx, fabsf(distance));
		diffuse = vadd(diffuse, vscale(vscale(vmul(sp->diffuse, pl->colour), intensity), max0(vdot(N, L))));
		v3 vl = vadd(view, L);
		v3 H = vdivs(vl, vlength(vl));
		specular = vadd(specular, vscale(vscale(vmul(sp->specular, pl->colour), intensity), powf_mode(cx, max0(vdot(N, H)), sp->power)));
	}
	for(int i = 0; i < tx->n_spot; i++)
	{ /* a point light at its position whose colour carries the cone factor; outside its cone it casts no shadow ray */
		const float *row = tx->spot_rows + 11 * i, *cone = tx->spot_cones + 5 * i;
		v3 to_l = vsub(sl_position(tx, node, sc->n_point_lights + i, V(row[3], row[4], row[5])), P);
		v3 L = vnormalize(to_l);
		const float Lf[3] = {L.x, L.y, L.z};
		float f;
		if(sp_cone(cone, cone[3], cone[4], Lf, &f)) continue;
		v3 colour = vscale(V(row[0], row[1], row[2]), f);
		if(cx->op->use_shadows && shadowed(cx, P, L)) continue;
		float distance = vlength(to_l);
		if(sl_in_force(tx) && triangle_occludes(tx, P, L, own, distance)) continue;
		float intensity = 1.0f / sq_mode(cx, fabsf(distance));
		diffuse = vadd(diffuse, vscale(vscale(vmul(sp->diffuse, colour), intensity), max0(vdot(N, L))));
		v3 vl = vadd(view, L);
		v3 H = vdivs(vl, vlength(vl));
		specular = vadd(specular, vscale(vscale(vmul(sp->specular, colour), intensity), powf_mode(cx, max0(vdot(N, H)), sp->power)));
	}
	for(int i = 0; i < sc->n_directional_lights; i++)
	{
		const sko_directional_light *dl = &sc->directional_lights[i];
		v3 L = vnormalize(dl->direction);
		if(cx->op->use_shadows && shadowed(cx, P, L)) continue;
		if(sl_in_force(tx) && triangle_occludes(tx, P, L, own, INFINITY)) continue;
		diffuse = vadd(diffuse, vscale(vmul(sp->diffuse, dl->colour), max0(vdot(N, L))));
		v3 vl = vadd(view, L);
		v3 H = vdivs(vl, vlength(vl));
		specular = vadd(specular, vscale(vmul(sp->specular, dl->colour), powf_mode(cx, max0(vdot(N, H)), sp->power)));
	}
	v3 total = V(0, 0, 0);
	total = vadd(total, ambient);
	total = vadd(total, diffuse);
	total = vadd(total, specular);
	return total;
}

static v3 sl_shade(sl_ctx *tx, v3 o, v3 d, int depth, uint32_t node, int from_triangle);

/* legacy_terms() */
static v3 sl_legacy_terms(sl_ctx *tx, v3 total_colour, v3 ray_dir, const sko_sphere *sp, v3 P, v3 N, int depth, uint32_t node)
{
	ctx_t *cx = &tx->cx;
	const sko_scene *sc = cx->sc;
	float fr = legacy_fresnel(ray_dir, N, sp->ior);
	v3 refraction_colour = V(0, 0, 0), reflection_colour = V(0, 0, 0);
	if((sp->specular.x != 0.0f || sp->specular.y != 0.0f || sp->specular.z != 0.0f) && depth > 0)
	{
		const uint32_t A = node_arity(cx), base = node * A + (uint32_t) cx->op->num_path_traces + 1u;
		const int nl = sc->n_point_lights + sc->n_directional_lights;
		for(int i = 0; i < nl; i++)
		{
			v3 L = i < sc->n_point_lights ? vnormalize(vsub(sc->point_lights[i].position, P)) : vnormalize(sc->directional_lights[i - sc->n_point_lights].direction);
			if(fr < 1)
			{
				v3 rd = legacy_refraction(ray_dir, N, sp->ior);
				refraction_colour = vscale(sl_shade(tx, P, rd, depth - 1, base + 2u * (uint32_t) i, -1), fr);
			}
			v3 md = legacy_reflect_direction(L, N);
			v3 c = sl_shade(tx, P, md, depth - 1, base + 2u * (uint32_t) i + 1u, -1);
			reflection_colour = vadd(reflection_colour, vmul(vscale(sp->specular, 1 - fr), c));
		}
	}
	return vadd(vadd(total_colour, refraction_colour), reflection_colour);
}

/* global_illumination() under the counter RNG (the only RNG this checker runs) */
static v3 sl_gi(sl_ctx *tx, v3 P, v3 N, int depth, uint32_t node, int from_triangle)
{
	ctx_t *cx = &tx->cx;
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
			child = sl_shade(tx, vadds(P, 0.00001f), w, depth - 1, node * node_arity(cx) + (uint32_t) i + 1u, from_triangle);
		}
		total = vadd(total, vdivs(vscale(child, r1), pdf));
	}
	total = vdivs(total, (float) n_rays);
	return total;
}

/* shade_from() */
static v3 sl_shade(sl_ctx *tx, v3 o, v3 d, int depth, uint32_t node, int from_triangle)
{
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
	if(!hit_a_sphere && !hit_a_triangle) return sc->background;
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
			v3 indirect = sl_gi(tx, P, N, depth, node, hit_triangle);
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
		if(cx->op->legacy_reflect) direct = sl_legacy_terms(tx, direct, d, sp, P, N, depth, node);
		if(cx->op->monte_carlo)
		{
			v3 indirect = sl_gi(tx, P, N, depth, node, -1);
			return vmul(vadd(vdivs(direct, (float) M_PI), vscale(indirect, 2.0f)), sp->diffuse);
		}
		return direct;
	}
	return V(0, 0, 0);
}

/* (spot lights and light radii refuse --legacy-reflect, include/skr.h: the checker has no rule for the pair; callers pass n_spot > 0 || some R > 0) */
static int sl_options_ok(const sko_options *opt, int n_spot) { return opt->rng_mode == SKO_RNG_COUNTER && opt->math_mode == SKO_MATH_SHARED && !(n_spot > 0 && opt->legacy_reflect); }

/* sko_render() under the counter RNG and the shared math; stats[5] as sko_render's (rays, hits, shadow rays, sphere tests, the
 * radiance rays' triangle tests) */
int sl_render(const sko_scene *scene, const sko_options *opt, int tri_shadows, int n_spot, const float *spot_rows, const float *spot_cones, const float *radii, uint8_t *rgb, float *rgbf,
			  uint64_t *stats)
{
	const int W = opt->width, H = opt->height;
	if(W <= 0 || H <= 0 || opt->y0 < 0 || opt->y1 > H || opt->y0 > opt->y1 || !sl_options_ok(opt, n_spot) || n_spot < 0) return 1;
	const int threads = opt->threads > 0 ? opt->threads : 1;
	const float inv_width = 1 / (float) W;
	const float inv_height = 1 / (float) H;
	const float aspect_ratio = W / (float) H;
	const float angle = (float) tan(M_PI * 0.5 * opt->fov / 180.);
	uint64_t tot[5] = {0, 0, 0, 0, 0};
	const long n_items = (long) (opt->y1 - opt->y0) * W;
#pragma omp parallel for schedule(dynamic, 32) num_threads(threads) reduction(+ : tot[:5])
	for(long item = 0; item < n_items; item++)
	{
		const int y = opt->y0 + (int) (item / W), x = (int) (item % W);
		sl_ctx tx = {{scene, opt, (uint32_t) y * (uint32_t) W + (uint32_t) x, 0, 0, 0, 0, 0, 0}, tri_shadows, n_spot, spot_rows, spot_cones, radii};
		v3 px = V(0, 0, 0);
		if(opt->grid_size > 0)
		{
			const int g = opt->grid_size;
			for(int s = 0; s < g * g; s++)
			{
				tx.cx.aa = (uint32_t) s;
				float r = sko_counter_jitter(opt->seed, tx.cx.pixel, tx.cx.aa);
				v3 dir = primary_direction(scene, x, y, 1, r, inv_width, inv_height, aspect_ratio, angle);
				px = vadd(px, sl_shade(&tx, scene->cam_pos, dir, opt->max_depth, 0, -1));
			}
			px = vdivs(px, (float) (g * g));
		}
		else
		{
			v3 dir = primary_direction(scene, x, y, 0, 0.0f, inv_width, inv_height, aspect_ratio, angle);
			px = sl_shade(&tx, scene->cam_pos, dir, opt->max_depth, 0, -1);
		}
		size_t o = ((size_t) (y - opt->y0) * W + x) * 3;
		if(rgb) { rgb[o] = sko_quantise(px.x); rgb[o + 1] = sko_quantise(px.y); rgb[o + 2] = sko_quantise(px.z); }
		if(rgbf) { rgbf[o] = px.x; rgbf[o + 1] = px.y; rgbf[o + 2] = px.z; }
		tot[0] += tx.cx.n_rays; tot[1] += tx.cx.n_hits; tot[2] += tx.cx.n_shadow; tot[3] += tx.cx.n_sph_tests; tot[4] += tx.cx.n_tri_tests;
	}
	if(stats) memcpy(stats, tot, sizeof tot);
	return 0;
}

/* The winner's t of a caller's ray (tests/shade_query_checker.c first_segment_t: the frame's rule for the first segment) */
static float sl_first_segment_t(const sko_scene *sc, const sko_options *op, v3 o, v3 d, int from_triangle)
{
	float min_distance = INFINITY;
	for(int i = 0; i < sc->n_spheres; i++)
	{
		const float distance = collision_distance(o, d, &sc->spheres[i]);
		if(intersection_occurs(distance) && distance < min_distance) min_distance = distance;
	}
	for(int i = 0; i < sc->n_triangles; i++)
	{
		float t;
		if(!triangle_test(o, d, &sc->triangles[i], &t)) continue;
		if(op->shade_triangles && (!(t > 0.0f) || i == from_triangle)) continue;
		if(t < min_distance) min_distance = t;
	}
	return min_distance;
}

/* Shading queries (include/skr.h skr_shade_rays): rays[n][8] = o tmax d ignore_triangle (int bits), keys[n] or NULL (= ray index),
 * out[n][3]; stats[3] = {radiance rays, hits shaded, shadow rays} of these rays (added to). */
int sl_shade_rays(const sko_scene *scene, const sko_options *opt, int tri_shadows, int n_spot, const float *spot_rows, const float *spot_cones, const float *radii, const float *rays, int64_t n, uint32_t sample, const uint32_t *keys,
				  float *out, uint64_t *stats)
{
	if(!sl_options_ok(opt, n_spot) || n_spot < 0) return 1;
	uint64_t tot[3] = {0, 0, 0};
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : tot[:3])
	for(int64_t i = 0; i < n; i++)
	{
		const float *ray = rays + 8 * i;
		int32_t ignore;
		memcpy(&ignore, ray + 7, 4);
		const v3 o = V(ray[0], ray[1], ray[2]), d = V(ray[4], ray[5], ray[6]);
		const int from_triangle = opt->shade_triangles ? ignore : -1;
		sl_ctx tx = {{scene, opt, keys ? keys[i] : (uint32_t) i, sample, 0, 0, 0, 0, 0}, tri_shadows, n_spot, spot_rows, spot_cones, radii};
		v3 c;
		if(sl_first_segment_t(scene, opt, o, d, from_triangle) < ray[3]) c = sl_shade(&tx, o, d, opt->max_depth, 0, from_triangle);
		else
		{
			tx.cx.n_rays++;
			c = scene->background;
		}
		out[3 * i] = c.x;
		out[3 * i + 1] = c.y;
		out[3 * i + 2] = c.z;
		tot[0] += tx.cx.n_rays;
		tot[1] += tx.cx.n_hits;
		tot[2] += tx.cx.n_shadow;
	}
	for(int k = 0; k < 3; k++) stats[k] += tot[k];
	return 0;
}
