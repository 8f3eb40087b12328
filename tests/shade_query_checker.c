/* The CPU checker of the shading queries (include/skr.h skr_shade_rays), modes without fog: the frozen oracle's own
 * integrator (oracle/skr_oracle.c, included whole: its static shade_from, collision_distance and triangle_test) run on caller-supplied
 * rays.  Test infrastructure; the product never loads it.  Built by tests/shade_query_check.py with the oracle's flags
 * (-ffp-contract=off): every float operation is the oracle's. */
#include "skr_oracle.c"

/* The t of the winner the frame's rule picks for the first segment (shade_from's loops, raytrace.h:152-186): the closest sphere at
 * 1 < t, or a triangle that blackens (any accepted t below the running minimum) or, under --shade-triangles, is shaded (t > 0, not
 * from_triangle).  +inf: nothing is hit. */
static float first_segment_t(const sko_scene *sc, const sko_options *op, v3 o, v3 d, int from_triangle)
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

/* rays[n][8] = o tmax d ignore_triangle (int bits), as include/skr.h skr_ray; keys[n] or NULL (= ray index); out[n][3];
 * stats[3] = {radiance rays, sphere hits shaded, shadow rays} of these rays (added to). */
void shade_rays(const sko_scene *scene, const sko_options *opt, const float *rays, int64_t n, uint32_t sample, const uint32_t *keys, float *out,
				uint64_t *stats)
{
	uint64_t tot[3] = {0, 0, 0};
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : tot[:3])
	for(int64_t i = 0; i < n; i++)
	{
		const float *ray = rays + 8 * i;
		int32_t ignore;
		memcpy(&ignore, ray + 7, 4);
		const v3 o = V(ray[0], ray[1], ray[2]), d = V(ray[4], ray[5], ray[6]);
		const int from_triangle = opt->shade_triangles ? ignore : -1;
		ctx_t cx = {scene, opt, keys ? keys[i] : (uint32_t) i, sample, 0, 0, 0, 0, 0};
		v3 c;
		if(first_segment_t(scene, opt, o, d, from_triangle) < ray[3]) c = shade_from(&cx, o, d, opt->max_depth, 0, from_triangle);
		else
		{ /* the winner lies at or beyond tmax: a miss, traced and counted like one */
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
}
