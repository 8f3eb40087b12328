/* The CPU checker of the shading queries (include/skr.h skr_shade_rays) on scenes with fog volumes: the fog checker's
 * integrator (tests/fog_checker.c, included whole: its static shade and collision_distance) run on caller-supplied rays.  Fog does not
 * combine with --shade-triangles or --legacy-reflect, so a triangle only blackens.  Test infrastructure; the product never loads it. */
#include "fog_checker.c"

/* shade()'s first-segment winner (fog_checker.c shade, raytrace.h:152-186): the closest sphere at 1 < t, or an accepted triangle
 * below the running minimum.  +inf: nothing is hit. */
static float first_segment_t(const sko_scene *sc, v3 o, v3 d)
{
	float min_distance = INFINITY;
	for(int i = 0; i < sc->n_spheres; i++)
	{
		const float distance = collision_distance(o, d, &sc->spheres[i]);
		if(intersection_occurs(distance) && distance < min_distance) min_distance = distance;
	}
	const float of[3] = {o.x, o.y, o.z}, df[3] = {d.x, d.y, d.z};
	for(int i = 0; i < sc->n_triangles; i++)
	{
		const sko_triangle *tr = &sc->triangles[i];
		const float v0[3] = {tr->v0.x, tr->v0.y, tr->v0.z}, v1[3] = {tr->v1.x, tr->v1.y, tr->v1.z}, v2[3] = {tr->v2.x, tr->v2.y, tr->v2.z};
		float t;
		if(sko_triangle_test(of, df, v0, v1, v2, &t) && t < min_distance) min_distance = t;
	}
	return min_distance;
}

/* As shade_query_checker.c shade_rays, with the fog volumes fog[n_fog][9] (include/skr.h skr_scene_get_fog rows).  Returns 0, or
 * skf_render's codes for options it does not cover. */
int shade_rays_fog(const sko_scene *scene, const sko_options *opt, const float *fog, int n_fog, const float *rays, int64_t n, uint32_t sample,
				   const uint32_t *keys, float *out, uint64_t *stats)
{
	if(n_fog < 0 || n_fog > 64) return 1;
	if(opt->rng_mode != SKO_RNG_COUNTER || opt->math_mode != SKO_MATH_SHARED || opt->shade_triangles || opt->legacy_reflect) return 2;
	fog_t fg[64];
	for(int j = 0; j < n_fog; j++)
	{
		const float *f = fog + 9 * j;
		fg[j].radius = f[3];
		fg[j].albedo = V(f[4], f[5], f[6]);
		fg[j].scattering = f[7];
		fg[j].absorption = f[8];
	}
	uint64_t tot[3] = {0, 0, 0};
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : tot[:3])
	for(int64_t i = 0; i < n; i++)
	{
		const float *ray = rays + 8 * i;
		const v3 o = V(ray[0], ray[1], ray[2]), d = V(ray[4], ray[5], ray[6]);
		ctx_t cx = {scene, opt, fg, n_fog, keys ? keys[i] : (uint32_t) i, sample, 0, 0, 0};
		v3 c;
		if(first_segment_t(scene, o, d) < ray[3]) c = shade(&cx, o, d, opt->max_depth, 0);
		else
		{
			cx.n_rays++;
			c = scene->background;
		}
		out[3 * i] = c.x;
		out[3 * i + 1] = c.y;
		out[3 * i + 2] = c.z;
		tot[0] += cx.n_rays;
		tot[1] += cx.n_hits;
		tot[2] += cx.n_shadow;
	}
	for(int k = 0; k < 3; k++) stats[k] += tot[k];
	return 0;
}
