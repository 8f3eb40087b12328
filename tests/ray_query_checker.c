/* The CPU checker of the ray queries (include/skr.h skr_trace_rays, skr_camera_rays): a brute-force loop over the scene arrays of
 * Scene.arrays() that states the hit rule of skr.h once more, on the oracle's exported primitives only (sko_smallest_root,
 * sko_triangle_test, sko_primary_direction, sko_counter_jitter).  Test infrastructure; the product never loads it.
 * Built with the oracle's flags (-ffp-contract=off): every float operation below is one IEEE binary32 operation, in the order the
 * kernels perform it. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "skr_oracle.h"

static float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static void cross3(const float x[3], const float y[3], float out[3])
{
	out[0] = x[1] * y[2] - y[1] * x[2];
	out[1] = x[2] * y[0] - y[2] * x[0];
	out[2] = x[0] * y[1] - y[0] * x[1];
}
static void normalize3(float v[3])
{
	const float inv = 1.0f / sqrtf(dot3(v, v));
	v[0] = v[0] * inv;
	v[1] = v[1] * inv;
	v[2] = v[2] * inv;
}
static float i2f(int32_t i) { float f; memcpy(&f, &i, 4); return f; }
static int32_t f2i(float f) { int32_t i; memcpy(&i, &f, 4); return i; }

/* utils.h:113-121 with the renderer's accept rule 1 < t < inf (raytrace.h:152-165) */
static float sphere_t(const float *o, const float *d, const float *s)
{
	const float e[3] = {o[0] - s[0], o[1] - s[1], o[2] - s[2]};
	const float a = dot3(d, d), b = 2 * dot3(d, e), c = dot3(e, e) - s[3] * s[3];
	const float t = sko_smallest_root(a, b, c);
	return (t <= 1.0f || t == INFINITY) ? INFINITY : t;
}

/* the triangle in file order, accepted with t > 0 (else +inf) */
static float triangle_t(const float *o, const float *d, const float *tr)
{
	float t;
	if(!sko_triangle_test(o, d, tr, tr + 3, tr + 6, &t) || !(t > 0.0f)) return INFINITY;
	return t;
}

/* rays[n][8] = o tmax d ignore (int bits); spheres[ns][14], triangles[nt][9] as Scene.arrays() returns them.
 * hits[n][8] = t kind index n.xyz 0 0 (int bits where include/skr.h has ints); occluded[n] = the any-hit answer.  Either may be NULL. */
void skq_trace(const float *spheres, int ns, const float *triangles, int nt, const float *rays, int64_t n, float *hits, int32_t *occluded)
{
#pragma omp parallel for schedule(dynamic, 64)
	for(int64_t i = 0; i < n; i++)
	{
		const float *ray = rays + 8 * i;
		const float o[3] = {ray[0], ray[1], ray[2]}, d[3] = {ray[4], ray[5], ray[6]};
		const float tmax = ray[3];
		const int32_t ignore = f2i(ray[7]);
		float ts = INFINITY, tt = INFINITY;
		int sph = -1, tri = -1;
		int occ = 0;
		for(int k = 0; k < ns; k++)
		{
			const float t = sphere_t(o, d, spheres + 14 * k);
			if(t < ts) { ts = t; sph = k; } /* strict: the first index wins a tie */
			if(t < tmax) occ = 1;
		}
		for(int k = 0; k < nt; k++)
		{
			if(k == ignore) continue;
			const float t = triangle_t(o, d, triangles + 9 * k);
			if(t < tt) { tt = t; tri = k; } /* strict, in file order: the lower index wins a tie */
			if(t < tmax) occ = 1;
		}
		if(occluded) occluded[i] = occ;
		if(!hits) continue;
		float *h = hits + 8 * i;
		int32_t kind = 0, index = -1;
		float t = INFINITY, N[3] = {0.0f, 0.0f, 0.0f};
		if(tri >= 0 && tt < ts)
		{ /* a triangle wins against a sphere only with a strictly smaller t */
			kind = 2;
			index = tri;
			t = tt;
			const float *v = triangles + 9 * tri;
			const float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
			cross3(e1, e2, N);
			normalize3(N);
			if(dot3(N, d) > 0.0f) { N[0] = -N[0]; N[1] = -N[1]; N[2] = -N[2]; }
		}
		else if(sph >= 0)
		{
			kind = 1;
			index = sph;
			t = ts;
			const float *s = spheres + 14 * sph;
			const float P[3] = {o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t};
			N[0] = P[0] - s[0];
			N[1] = P[1] - s[1];
			N[2] = P[2] - s[2];
			normalize3(N);
		}
		if(kind != 0 && !(t < tmax))
		{ /* the winner lies at or beyond tmax: a miss */
			kind = 0;
			index = -1;
			t = INFINITY;
			N[0] = N[1] = N[2] = 0.0f;
		}
		h[0] = t;
		h[1] = i2f(kind);
		h[2] = i2f(index);
		h[3] = N[0];
		h[4] = N[1];
		h[5] = N[2];
		h[6] = 0.0f;
		h[7] = 0.0f;
	}
}

/* The primary rays of AA sample `sample` (grid > 0) or the pixel centres (grid == 0): rays[h][w][8] as skr_camera_rays writes them. */
void skq_camera_rays(const sko_scene *scene, int width, int height, float fov, int grid, uint64_t seed, uint32_t sample, float *rays)
{
#pragma omp parallel for schedule(static)
	for(int y = 0; y < height; y++)
		for(int x = 0; x < width; x++)
		{
			const uint32_t pixel = (uint32_t) y * (uint32_t) width + (uint32_t) x;
			const float r = grid > 0 ? sko_counter_jitter(seed, pixel, sample) : 0.0f;
			float *ray = rays + 8 * (size_t) pixel;
			ray[0] = scene->cam_pos.x;
			ray[1] = scene->cam_pos.y;
			ray[2] = scene->cam_pos.z;
			ray[3] = INFINITY;
			sko_primary_direction(scene, width, height, fov, x, y, grid > 0, r, ray + 4);
			ray[7] = i2f(-1);
		}
}
