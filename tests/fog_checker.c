/* tests/fog_checker.c — TEST INFRASTRUCTURE: the CPU checker of the spherical fog (--scn-fog, DESIGN.md "Spherical fog").
 *
 * A restatement of the frozen oracle's integrator (oracle/skr_oracle.c, counter RNG + shared math only) with the fog term of
 * blinn_phong.h:19-43 added, built by tests/fog_check.py with the oracle's flags and linked against liboracle, whose exported
 * primitives it calls wherever they exist.  On scenes without fog it must reproduce sko_render bit for bit (tests/test_fog_cpu.py);
 * only then do its fog frames count as evidence for the GPU's (tests/test_fog_gpu.py).  --legacy-reflect and --shade-triangles are
 * not restated here (fog does not combine with them).
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../oracle/skr_oracle.h"

typedef sko_vec3 v3;

static inline v3 V(float x, float y, float z) { v3 r = {x, y, z}; return r; }
static inline v3 vadd(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline v3 vsub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 vmul(v3 a, v3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline v3 vscale(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
static inline v3 vdivs(v3 a, float s) { return V(a.x / s, a.y / s, a.z / s); }
static inline v3 vadds(v3 a, float s) { return V(a.x + s, a.y + s, a.z + s); }
static inline float vdot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline float vsqr(v3 v) { return v.x * v.x + v.y * v.y + v.z * v.z; }
static inline float vlength(v3 v) { return sqrtf(vsqr(v)); }
static inline v3 vnormalize(v3 v) { return vscale(v, 1.0f / sqrtf(vsqr(v))); }
static inline float max0(float x) { return (0.0f < x) ? x : 0.0f; }

/* ------------------------------------------------------------------ exp: binary64, one IEEE operation per step (device_math.h exp_spec) */
static inline double as_double(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }

double skf_exp_spec(double x)
{
	if(x != x) return x;
	if(x > 710.0) return INFINITY;
	if(x < -746.0) return 0.0;
	const double k = rint(x * 0x1.71547652b82fep+0);
	double r = fma(-k, 0x1.62e42feep-1, x);
	r = fma(-k, 0x1.a39ef35793c76p-33, r);
	static const double c[13] = {0x1.1eed8eff8d898p-29, 0x1.ae64567f544e4p-26, 0x1.27e4fb7789f5cp-22, 0x1.71de3a556c734p-19,
								 0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-13, 0x1.6c16c16c16c17p-10, 0x1.1111111111111p-7,
								 0x1.5555555555555p-5,  0x1.5555555555555p-3,  0.5,                   1.0,                   1.0};
	double q = 0x1.6124613a86d09p-33; /* 1/13!, then 1/12! .. 1/2!, 1, 1 */
	for(int i = 0; i < 13; i++) q = fma(q, r, c[i]);
	const int ki = (int) k, k1 = ki >> 1, k2 = ki - k1;
	return (q * as_double((uint64_t) (k1 + 1023) << 52)) * as_double((uint64_t) (k2 + 1023) << 52);
}

/* ------------------------------------------------------------------ the fog term (blinn_phong.h:19-43, utils.h:216-225) */
/* The counter word of a fog draw: bit 31 set, light << 8, fog << 1, pass (0 diffuse_shading, 1 specular_shading) */
static inline uint32_t fog_ctr3(uint32_t light, uint32_t fog, uint32_t pass) { return 0x80000000u | (light << 8) | (fog << 1) | pass; }
/* float(rand()) / float(RAND_MAX) and -1 + float(rand()) / float(RAND_MAX / (1 + 1)) on a 31-bit draw: float(RAND_MAX) = 2^31,
 * float(RAND_MAX / 2) = 2^30 */
static inline float u31(uint32_t w) { return (float) (w >> 1) / 2147483648.0f; }
static inline float pm1(uint32_t w) { return -1.0f + (float) (w >> 1) / 1073741824.0f; }

typedef struct {
	float radius, absorption, scattering;
	v3 albedo;
} fog_t;

static v3 fog_term(const fog_t *f, v3 L, float intensity, v3 lc, v3 centre, v3 lpos, v3 kd, v3 N, const uint32_t ctr[4], uint64_t seed,
				   float *p_out)
{
	float distance = vlength(vsub(centre, lpos));
	if(distance > 2 * f->radius) distance = 2 * f->radius;
	const float p = (float) skf_exp_spec((double) (-1.0f * distance * (f->absorption + f->scattering)));
	if(p_out) *p_out = p;
	uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, key[2] = {(uint32_t) seed, (uint32_t) (seed >> 32)}, o[4];
	sko_philox4x32_spec(c, key, o);
	if(u31(o[0]) > p) return vscale(vscale(vmul(kd, lc), intensity), max0(vdot(N, L)));
	const v3 nd = V(L.x + pm1(o[1]) * f->scattering, L.y + pm1(o[2]) * f->scattering, L.z + pm1(o[3]) * f->scattering);
	return vscale(vmul(f->albedo, lc), max0(vdot(N, nd)));
}

/* skr_debug_eval op 11's record layout (include/skr.h), evaluated here */
void skf_fog_term_record(const uint32_t in[40], uint32_t out[4])
{
	float x[40];
	memcpy(x, in, sizeof x);
	const fog_t f = {x[0], x[1], x[2], V(x[4], x[5], x[6])};
	const uint32_t ctr[4] = {in[27], in[32], in[31], fog_ctr3(in[23], in[19], in[15])};
	float p = 0;
	const v3 c = fog_term(&f, V(x[8], x[9], x[10]), x[11], V(x[12], x[13], x[14]), V(x[16], x[17], x[18]), V(x[20], x[21], x[22]),
						  V(x[24], x[25], x[26]), V(x[28], x[29], x[30]), ctr, (uint64_t) in[33] | (uint64_t) in[34] << 32, &p);
	const float r[4] = {c.x, c.y, c.z, p};
	memcpy(out, r, sizeof r);
}

/* ------------------------------------------------------------------ integrator (oracle/skr_oracle.c, counter RNG, shared math) */
typedef struct {
	const sko_scene *sc;
	const sko_options *op;
	const fog_t *fog;
	int n_fog;
	uint32_t pixel, aa;
	uint64_t n_rays, n_hits, n_shadow;
} ctx_t;

static inline float collision_distance(v3 o, v3 d, const sko_sphere *sp)
{
	v3 e_c = vsub(o, sp->center);
	float a = vdot(d, d);
	float b = 2 * vdot(d, e_c);
	float c = vdot(e_c, e_c) - sp->radius * sp->radius;
	return sko_smallest_root(a, b, c);
}
static inline int intersection_occurs(float distance) { return !(distance <= 1.0f || distance == INFINITY); }

static int shadowed(ctx_t *cx, v3 P, v3 L)
{
	v3 o = vadds(P, 0.000001f);
	cx->n_shadow++;
	for(int i = 0; i < cx->sc->n_spheres; i++)
		if(intersection_occurs(collision_distance(o, L, &cx->sc->spheres[i]))) return 1;
	return 0;
}

static v3 direct_illumination(ctx_t *cx, const sko_sphere *sp, v3 P, v3 N, uint32_t node)
{
	const sko_scene *sc = cx->sc;
	v3 ambient = vmul(sc->ambient, sp->ambient);
	v3 diffuse = V(0, 0, 0), specular = V(0, 0, 0);
	v3 view = vnormalize(vsub(sc->cam_pos, P));
	for(int i = 0; i < sc->n_point_lights; i++)
	{
		const sko_point_light *pl = &sc->point_lights[i];
		v3 to_l = vsub(pl->position, P);
		v3 L = vnormalize(to_l);
		if(cx->op->use_shadows && shadowed(cx, P, L)) continue;
		float distance = vlength(to_l);
		float intensity = 1.0f / (fabsf(distance) * fabsf(distance));
		if(cx->n_fog > 0)
		{ /* blinn_phong.h:58-64 and :103-109: the fog terms instead of the diffuse and instead of the specular term */
			for(uint32_t pass = 0; pass < 2; pass++)
				for(int j = 0; j < cx->n_fog; j++)
				{
					const uint32_t ctr[4] = {cx->pixel, cx->aa, node, fog_ctr3((uint32_t) i, (uint32_t) j, pass)};
					const v3 f = fog_term(&cx->fog[j], L, intensity, pl->colour, sp->center, pl->position, sp->diffuse, N, ctr, cx->op->seed, NULL);
					if(pass == 0) diffuse = vadd(diffuse, f);
					else specular = vadd(specular, f);
				}
			continue;
		}
		diffuse = vadd(diffuse, vscale(vscale(vmul(sp->diffuse, pl->colour), intensity), max0(vdot(N, L))));
		v3 vl = vadd(view, L);
		v3 H = vdivs(vl, vlength(vl));
		specular = vadd(specular, vscale(vscale(vmul(sp->specular, pl->colour), intensity), sko_powf_shared(max0(vdot(N, H)), sp->power)));
	}
	for(int i = 0; i < sc->n_directional_lights; i++)
	{
		const sko_directional_light *dl = &sc->directional_lights[i];
		v3 L = vnormalize(dl->direction);
		if(cx->op->use_shadows && shadowed(cx, P, L)) continue;
		diffuse = vadd(diffuse, vscale(vmul(sp->diffuse, dl->colour), max0(vdot(N, L))));
		v3 vl = vadd(view, L);
		v3 H = vdivs(vl, vlength(vl));
		specular = vadd(specular, vscale(vmul(sp->specular, dl->colour), sko_powf_shared(max0(vdot(N, H)), sp->power)));
	}
	v3 total = V(0, 0, 0);
	total = vadd(total, ambient);
	total = vadd(total, diffuse);
	total = vadd(total, specular);
	return total;
}

static v3 shade(ctx_t *cx, v3 o, v3 d, int depth, uint32_t node);

static v3 global_illumination(ctx_t *cx, v3 P, v3 N, int depth, uint32_t node)
{
	const int n_rays = cx->op->num_path_traces;
	v3 total = V(0, 0, 0);
	float nn[3] = {N.x, N.y, N.z}, a[3], b[3];
	sko_basis(nn, a, b);
	const v3 nt = V(a[0], a[1], a[2]), nb = V(b[0], b[1], b[2]);
	float pdf = (float) (1 / M_PI);
	for(int i = 0; i < n_rays; i++)
	{
		float r1 = 0.0f, r2 = 0.0f;
		v3 child = V(0, 0, 0);
		if(depth - 1 > 0)
		{
			sko_counter_draws(cx->op->seed, cx->pixel, cx->aa, node, (uint32_t) i, &r1, &r2);
			float s_theta = sqrtf(1 - r1 * r1);
			float phi = (float) (2.0f * M_PI * r2);
			float sn, cs;
			sko_sincos_shared(phi, &sn, &cs);
			v3 s = V(s_theta * cs, r1, s_theta * sn);
			v3 w = V(s.x * nb.x + s.y * N.x + s.z * nt.x, s.x * nb.y + s.y * N.y + s.z * nb.y, s.x * nb.z + s.y * N.z + s.z * nb.z);
			child = shade(cx, vadds(P, 0.00001f), w, depth - 1, node * (uint32_t) n_rays + (uint32_t) i + 1u);
		}
		total = vadd(total, vdivs(vscale(child, r1), pdf));
	}
	return vdivs(total, (float) n_rays);
}

static v3 shade(ctx_t *cx, v3 o, v3 d, int depth, uint32_t node)
{
	const sko_scene *sc = cx->sc;
	if(depth <= 0) return V(0, 0, 0);
	cx->n_rays++;
	float min_distance = INFINITY;
	int hit_sphere = -1, hit_a_sphere = 0, hit_a_triangle = 0;
	for(int i = 0; i < sc->n_spheres; i++)
	{
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
	const float of[3] = {o.x, o.y, o.z}, df[3] = {d.x, d.y, d.z};
	for(int i = 0; i < sc->n_triangles; i++)
	{
		const sko_triangle *tr = &sc->triangles[i];
		const float v0[3] = {tr->v0.x, tr->v0.y, tr->v0.z}, v1[3] = {tr->v1.x, tr->v1.y, tr->v1.z}, v2[3] = {tr->v2.x, tr->v2.y, tr->v2.z};
		float t;
		if(sko_triangle_test(of, df, v0, v1, v2, &t) && t < min_distance)
		{
			min_distance = t;
			hit_a_sphere = 0;
			hit_a_triangle = 1;
		}
	}
	if(!hit_a_sphere && !hit_a_triangle) return sc->background;
	if(hit_a_sphere)
	{
		const sko_sphere *sp = &sc->spheres[hit_sphere];
		float t = collision_distance(o, d, sp);
		v3 P = vadd(o, vscale(d, t));
		v3 N = vnormalize(vsub(P, sp->center));
		cx->n_hits++;
		v3 direct = direct_illumination(cx, sp, P, N, node);
		if(cx->op->monte_carlo)
		{
			v3 indirect = global_illumination(cx, P, N, depth, node);
			return vmul(vadd(vdivs(direct, (float) M_PI), vscale(indirect, 2.0f)), sp->diffuse);
		}
		return direct;
	}
	return V(0, 0, 0);
}

/* fog[n_fog][9] = centre(3) radius albedo(3) scattering absorption (include/skr.h skr_scene_get_fog); stats = {rays, hits, shadow rays} */
int skf_render(const sko_scene *scene, const sko_options *opt, const float *fog, int n_fog, uint8_t *rgb, float *rgbf, uint64_t *stats)
{
	const int W = opt->width, H = opt->height;
	if(W <= 0 || H <= 0 || opt->y0 < 0 || opt->y1 > H || opt->y0 > opt->y1 || n_fog < 0 || n_fog > 64) return 1;
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
	const long n_items = (long) (opt->y1 - opt->y0) * W;
	const int threads = opt->threads > 0 ? opt->threads : 1;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 64) num_threads(threads) reduction(+ : tot[:3])
#endif
	for(long item = 0; item < n_items; item++)
	{
		const int y = opt->y0 + (int) (item / W), x = (int) (item % W);
		ctx_t cx = {scene, opt, fg, n_fog, (uint32_t) y * (uint32_t) W + (uint32_t) x, 0, 0, 0, 0};
		v3 px = V(0, 0, 0);
		float dir[3];
		if(opt->grid_size > 0)
		{
			const int g = opt->grid_size;
			for(int s = 0; s < g * g; s++)
			{
				cx.aa = (uint32_t) s;
				const float r = sko_counter_jitter(opt->seed, cx.pixel, cx.aa);
				sko_primary_direction(scene, W, H, opt->fov, x, y, 1, r, dir);
				px = vadd(px, shade(&cx, scene->cam_pos, V(dir[0], dir[1], dir[2]), opt->max_depth, 0));
			}
			px = vdivs(px, (float) (g * g));
		}
		else
		{
			sko_primary_direction(scene, W, H, opt->fov, x, y, 0, 0.0f, dir);
			px = shade(&cx, scene->cam_pos, V(dir[0], dir[1], dir[2]), opt->max_depth, 0);
		}
		const size_t o = ((size_t) (y - opt->y0) * W + x) * 3;
		if(rgb) { rgb[o] = sko_quantise(px.x); rgb[o + 1] = sko_quantise(px.y); rgb[o + 2] = sko_quantise(px.z); }
		if(rgbf) { rgbf[o] = px.x; rgbf[o + 1] = px.y; rgbf[o + 2] = px.z; }
		tot[0] += cx.n_rays; tot[1] += cx.n_hits; tot[2] += cx.n_shadow;
	}
	if(stats) memcpy(stats, tot, sizeof tot);
	return 0;
}
