/* The CPU checker of motion blur (include/skr.h skr_scene_set_sphere_velocities).  A sample at shutter time tau is, by
 * definition, the static scene with displaced centres, shaded by the code the other checkers already pin: this file restates only the
 * shutter draw (sko_philox4x32_spec, one binary32 multiply) and the displacement (fmaf from libm, one per component), copies the sphere
 * array per ray, displaces it and calls lens_shade_rays (tests/lens_checker.c, included whole, and through it the soft-light and spot
 * checkers and oracle/skr_oracle.c) for that one ray with its key.  A frame is composed in tests/motion_check.py per aa in aa order, as
 * lens_check.Checker.render does.  With S = 0 or all velocities 0 the composed frame must reproduce sko_render bit for bit, counts
 * included (tests/test_motion_cpu.py checks that first: only then is this file evidence).  Test infrastructure; the product never loads
 * it.  Built by tests/motion_check.py with the oracle's flags (-ffp-contract=off: the only fused operations are the fmaf calls). */
#include "lens_checker.c"

#define SHUTTER_CTR3 0x800000E0u /* include/skr.h SKR_SHUTTER_CTR3 */

/* The draw's first word for (pixel, aa) under the seed: one Philox call at node 0. */
uint32_t motion_word(uint32_t pixel, uint32_t aa, uint32_t seed_lo, uint32_t seed_hi)
{
	const uint32_t ctr[4] = {pixel, aa, 0u, SHUTTER_CTR3}, key[2] = {seed_lo, seed_hi};
	uint32_t o[4];
	sko_philox4x32_spec(ctr, key, o);
	return o[0];
}

/* tau = S * u, one binary32 multiply */
float motion_tau(uint32_t pixel, uint32_t aa, uint32_t seed_lo, uint32_t seed_hi, float S)
{
	return S * u31(motion_word(pixel, aa, seed_lo, seed_hi));
}

/* c'[n][3] = fmaf(tau, v, c) per component */
void motion_centres(float tau, const float *c, const float *v, int64_t n, float *out)
{
	for(int64_t i = 0; i < 3 * n; i++) out[i] = fmaf(tau, v[i], c[i]);
}

/* One record of skr_debug_eval's motion op: (pixel, aa, seed_lo, seed_hi, S, c(3), v(3)) -> (tau, c'(3)) */
void motion_records(const uint32_t *in, int64_t n, float *out)
{
	for(int64_t i = 0; i < n; i++)
	{
		const uint32_t *r = in + 11 * i;
		float f[7];
		memcpy(f, r + 4, sizeof f);
		out[4 * i] = motion_tau(r[0], r[1], r[2], r[3], f[0]);
		motion_centres(out[4 * i], f + 1, f + 4, 1, out + 4 * i + 1);
	}
}

/* lens_shade_rays on a scene in motion: ray i sees the spheres at the shutter time of (its key, sample).  velocities[n_spheres][3];
 * in_force = 0: the scene as it lies, no draw.  stats[5] are added to. */
int motion_shade_rays(const sko_scene *scene, const sko_options *opt, int tri_shadows, int n_spot, const float *spot_rows, const float *spot_cones, const float *radii,
					  const float *velocities, float S, int in_force, const float *rays, int64_t n, uint32_t sample, const uint32_t *keys, float *out, uint64_t *stats)
{
	if(!in_force) return lens_shade_rays(scene, opt, tri_shadows, n_spot, spot_rows, spot_cones, radii, rays, n, sample, keys, out, stats);
	const int ns = scene->n_spheres;
	uint64_t tot[5] = {0, 0, 0, 0, 0};
	int bad = 0;
#pragma omp parallel reduction(+ : tot[:5]) reduction(| : bad)
	{
		sko_sphere *moved = (sko_sphere *) malloc(sizeof(sko_sphere) * (size_t) (ns > 0 ? ns : 1));
		sko_scene sc = *scene;
		sc.spheres = moved;
#pragma omp for schedule(dynamic, 16)
		for(int64_t i = 0; i < n; i++)
		{
			const uint32_t key = keys ? keys[i] : (uint32_t) i;
			const float tau = motion_tau(key, sample, (uint32_t) opt->seed, (uint32_t) (opt->seed >> 32), S);
			for(int s = 0; s < ns; s++)
			{
				moved[s] = scene->spheres[s];
				moved[s].center.x = fmaf(tau, velocities[3 * s], scene->spheres[s].center.x);
				moved[s].center.y = fmaf(tau, velocities[3 * s + 1], scene->spheres[s].center.y);
				moved[s].center.z = fmaf(tau, velocities[3 * s + 2], scene->spheres[s].center.z);
			}
			uint64_t st[5] = {0, 0, 0, 0, 0};
			bad |= lens_shade_rays(&sc, opt, tri_shadows, n_spot, spot_rows, spot_cones, radii, rays + 8 * i, 1, sample, &key, out + 3 * i, st);
			for(int k = 0; k < 5; k++) tot[k] += st[k];
		}
		free(moved);
	}
	for(int k = 0; k < 5; k++) stats[k] += tot[k];
	return bad;
}
