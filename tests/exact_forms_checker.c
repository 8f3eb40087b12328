/* The hit root from binary32 pairs (device_math.h near_root_pair / near_root) restated in C, one IEEE binary32 operation per
 * statement, for tests/test_exact_forms_cpu.py.  Test infrastructure; the product never loads it.  Compile with -ffp-contract=off.
 *
 * The device takes sqrt(D) and 1 / 2a from its short exact forms (sk_sqrtf, sk_rcpf: the correctly rounded values on the ranges used
 * here, held exhaustively by tests/test_gpu_units.py), so sqrtf and 1.0f / x stand in for them.  The half reciprocal root h that
 * scales the residual is the hardware's 1-ulp estimate on the device and 0.5f / s here: it enters the low part of the root only,
 * 2^-24 of the root, to 2^-22 of itself either way (DESIGN.md "The root from binary32 pairs"). */
#include <math.h>
#include <stdint.h>
#include <string.h>

static uint32_t bits(float f)
{
	uint32_t u;
	memcpy(&u, &f, 4);
	return u;
}

/* utils.h:87-110 given D: the binary64 form */
static float near_root_exact(float two_a, float b, float D)
{
	const double q = ((double) (-b) - sqrt((double) D)) / (double) two_a;
	const float t2 = (float) q;
	return (t2 >= 0.0f) ? t2 : INFINITY;
}

typedef struct { float lo, hi, q_h, q_l; } root_pair;

static int near_root_pair(float two_a, float b, float D, root_pair *r)
{
	const int in_range = (uint32_t) (bits(two_a) - (87u << 23)) < (80u << 23) && (uint32_t) (bits(D) - (67u << 23)) < (120u << 23);
	const float s = sqrtf(D);
	const float h = 0.5f / s;
	const float s_l = fmaf(-s, s, D) * h;
	const float nb = -b;
	const float n_h = nb - s;
	const float t0 = nb - n_h;
	const float t1 = t0 - s;
	const float n_l = t1 - s_l;
	const float inv = 1.0f / two_a;
	const float q_h = n_h * inv;
	const float r0 = fmaf(-q_h, two_a, n_h);
	const float r1 = r0 + n_l;
	const float q_l = r1 * inv;
	const float k = inv * 0x1p-41f;
	const float m = s + fabsf(n_h);
	const float E = m * k;
	const float wl = q_l - E, wh = q_l + E;
	r->q_h = q_h;
	r->q_l = q_l;
	r->lo = q_h + wl;
	r->hi = q_h + wh;
	return in_range && (nb >= s) && (nb < 0x1p40f);
}

/* n records (2a, b, D) -> 7 words each, the layout of skr_debug_eval op 19 (include/skr.h) */
void skx_near_root(uint32_t n, const float *in, uint32_t *out)
{
	for(uint32_t i = 0; i < n; i++)
	{
		const float two_a = in[3 * i], b = in[3 * i + 1], D = in[3 * i + 2];
		root_pair r;
		const int short_form = near_root_pair(two_a, b, D, &r) && r.lo == r.hi;
		uint32_t *w = out + 7 * (size_t) i;
		w[0] = bits(short_form ? r.lo : near_root_exact(two_a, b, D));
		w[1] = bits(near_root_exact(two_a, b, D));
		w[2] = short_form ? 0u : 1u;
		w[3] = bits(r.lo);
		w[4] = bits(r.hi);
		w[5] = bits(r.q_h);
		w[6] = bits(r.q_l);
	}
}
