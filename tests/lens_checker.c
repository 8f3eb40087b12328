/* The CPU checker of the thin-lens camera (include/skr.h skr_scene_set_lens).  It restates the lens draw and the lens
 * ray from the frozen oracle's exported primitives — sko_philox4x32_spec, sko_sincos_shared, sko_primary_direction, sko_counter_jitter —
 * and fills the skr_ray rows of a whole (frame, aa).  A lens frame is then composed in tests/lens_check.py: per aa the rays are shaded
 * with keys y * W + x and sample aa, the samples summed in aa order and divided by (float) (g * g) as sko_render does.  The shading is
 * the existing checker's: tests/soft_light_checker.c is included whole (and with it oracle/skr_oracle.c) and its sl_shade is called, not
 * copied; lens_shade_rays is its sl_shade_rays with all five work counts handed out, since a frame is compared on all of them.  With
 * A = 0 the composed frame must reproduce sko_render bit for bit, counts included (tests/test_lens_cpu.py checks that first: only then is
 * this file evidence).  Test infrastructure; the product never loads it.  Built by tests/lens_check.py with the oracle's flags
 * (-ffp-contract=off). */
#include "soft_light_checker.c"

#define LENS_CTR3 0x800000C0u /* include/skr.h SKR_LENS_CTR3 */

/* The lens sample (lx, ly) of (pixel, aa) under the seed: one Philox call at node 0, then binary32, one operation per step. */
void lens_sample(uint32_t pixel, uint32_t aa, uint32_t seed_lo, uint32_t seed_hi, float out[2])
{
	const uint32_t ctr[4] = {pixel, aa, 0u, LENS_CTR3}, key[2] = {seed_lo, seed_hi};
	uint32_t o[4];
	sko_philox4x32_spec(ctr, key, o);
	const float u1 = u31(o[0]), u2 = u31(o[1]);
	const float r = sqrtf(u1);
	const float phi = 0x1.921fb6p+2f * u2;
	float sn, cs;
	sko_sincos_shared(phi, &sn, &cs);
	out[0] = r * cs;
	out[1] = r * sn;
}

/* The ray (o2, d2) the sample (lx, ly) makes of the pinhole direction d: A the aperture, k = A / F as the host divided. */
void lens_ray(float A, float k, const float cam_pos[3], const float right[3], const float up[3], const float d[3], float lx, float ly, float o2[3], float d2[3])
{
	const float ax = A * lx, ay = A * ly, kx = k * lx, ky = k * ly;
	for(int c = 0; c < 3; c++)
	{
		o2[c] = (cam_pos[c] + right[c] * ax) + up[c] * ay;
		d2[c] = (d[c] - right[c] * kx) - up[c] * ky;
	}
}

/* One record of skr_debug_eval's lens op: (pixel, aa, seed_lo, seed_hi, A, k, cam_pos(3), right(3), up(3), d(3)) -> (lx, ly, o'(3), d'(3)) */
void lens_record(const uint32_t in[18], float out[8])
{
	float f[14];
	memcpy(f, in + 4, sizeof f);
	lens_sample(in[0], in[1], in[2], in[3], out);
	lens_ray(f[0], f[1], f + 2, f + 5, f + 8, f + 11, out[0], out[1], out + 2, out + 5);
}

void lens_records(const uint32_t *in, int64_t n, float *out)
{
	for(int64_t i = 0; i < n; i++) lens_record(in + 18 * i, out + 8 * i);
}

/* The primary rays of AA sample aa of a width x height frame under the lens (A, F), rays[height * width][8] = o tmax d ignore_triangle
 * (include/skr.h skr_ray): the pinhole direction sko_render forms for the pixel and sample (jitter: grid_size > 0), then the lens ray.
 * A == 0: the pinhole ray itself, no draw. */
void lens_rays(const sko_scene *scene, int width, int height, float fov, int jitter, uint64_t seed, uint32_t aa, float A, float F, float *rays)
{
	const float k = A / F;
	const float cam[3] = {scene->cam_pos.x, scene->cam_pos.y, scene->cam_pos.z};
	const float right[3] = {scene->cam_right.x, scene->cam_right.y, scene->cam_right.z};
	const float up[3] = {scene->cam_up.x, scene->cam_up.y, scene->cam_up.z};
	const int32_t none = -1;
	for(int y = 0; y < height; y++)
		for(int x = 0; x < width; x++)
		{
			const uint32_t pixel = (uint32_t) y * (uint32_t) width + (uint32_t) x;
			float *ray = rays + 8 * (size_t) pixel;
			float d[3];
			const float r = jitter ? sko_counter_jitter(seed, pixel, aa) : 0.0f;
			sko_primary_direction(scene, width, height, fov, x, y, jitter, r, d);
			if(A > 0.0f)
			{
				float s[2];
				lens_sample(pixel, aa, (uint32_t) seed, (uint32_t) (seed >> 32), s);
				lens_ray(A, k, cam, right, up, d, s[0], s[1], ray, ray + 4);
			}
			else
			{
				memcpy(ray, cam, sizeof cam);
				memcpy(ray + 4, d, sizeof d);
			}
			ray[3] = INFINITY;
			memcpy(ray + 7, &none, 4);
		}
}

/* sl_shade_rays (tests/soft_light_checker.c) with stats[5] = {radiance rays, hits shaded, shadow rays, sphere tests, the radiance rays'
 * triangle tests} of these rays (added to), as sko_render counts them: a ray cut by its tmax has tested every sphere and triangle. */
int lens_shade_rays(const sko_scene *scene, const sko_options *opt, int tri_shadows, int n_spot, const float *spot_rows, const float *spot_cones, const float *radii,
					const float *rays, int64_t n, uint32_t sample, const uint32_t *keys, float *out, uint64_t *stats)
{
	if(!sl_options_ok(opt, n_spot) || n_spot < 0) return 1;
	uint64_t tot[5] = {0, 0, 0, 0, 0};
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : tot[:5])
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
			tx.cx.n_sph_tests += (uint64_t) scene->n_spheres;
			tx.cx.n_tri_tests += (uint64_t) scene->n_triangles;
			c = scene->background;
		}
		out[3 * i] = c.x;
		out[3 * i + 1] = c.y;
		out[3 * i + 2] = c.z;
		tot[0] += tx.cx.n_rays;
		tot[1] += tx.cx.n_hits;
		tot[2] += tx.cx.n_shadow;
		tot[3] += tx.cx.n_sph_tests;
		tot[4] += tx.cx.n_tri_tests;
	}
	for(int k = 0; k < 5; k++) stats[k] += tot[k];
	return 0;
}
