/* CPU checker of the denoiser under a per-pixel variance image (include/skr.h skr_denoise_var): the rule restated in
 * plain binary32 C, one pixel at a time, windows and taps in row-major order.  Compiled with -ffp-contract=off
 * (tests/denoise_var_check.py), so every + - * / is one IEEE operation.  Test infrastructure; the product never loads it. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define VAR_SIGMA_L 4.0f /* SKR_DENOISE_VAR_SIGMA_L */
#define SIGMA_Z 0.05f
#define EPS 1e-6f
#define MISS 0xFFFFFFFFu
#define MESH 0xFFFFFFFEu

static float lum(const float *c) { return 0.2126f * c[0] + 0.7152f * c[1] + 0.0722f * c[2]; }
static float max0(float x) { return x > 0.0f ? x : 0.0f; }

static uint32_t quantise(float c)
{ /* device_math.h quantise */
	const float m = (c < 1.0f) ? c : 1.0f;
	const float s = m * 255;
	if(!(s > -2147483648.0f)) return 0;
	return (uint32_t) (int32_t) s & 0xffu;
}

/* the init value of pixel (x, y): the 3x3 pre-filter of the measured variances where var[p] >= 0, else the spatial estimate */
static float init_var(int w, int h, int x, int y, const float *rgbf, const uint32_t *cls, const float *var)
{
	static const float g3[3] = {0.25f, 0.5f, 0.25f}; /* g = g3[dy + 1] * g3[dx + 1]: exact */
	const size_t i = (size_t) y * w + x;
	if(var && var[i] >= 0.0f)
	{
		float sv = 0.0f, sg = 0.0f;
		for(int dy = -1; dy <= 1; dy++)
			for(int dx = -1; dx <= 1; dx++)
			{
				const int yy = y + dy, xx = x + dx;
				if(yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
				const size_t j = (size_t) yy * w + xx;
				if(cls[j] != cls[i] || !(var[j] >= 0.0f)) continue;
				const float g = g3[dy + 1] * g3[dx + 1];
				sv += g * var[j];
				sg += g;
			}
		return sv / sg;
	}
	float s1 = 0.0f, s2 = 0.0f;
	int cnt = 0;
	for(int dy = -1; dy <= 1; dy++)
		for(int dx = -1; dx <= 1; dx++)
		{
			const int yy = y + dy, xx = x + dx;
			if(yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
			const size_t j = (size_t) yy * w + xx;
			if(cls[j] != cls[i]) continue;
			const float l = lum(rgbf + 3 * j);
			s1 += l;
			s2 += l * l;
			cnt++;
		}
	const float m1 = s1 / (float) cnt, m2 = s2 / (float) cnt;
	return max0(m2 - m1 * m1);
}

/* hits: skr_hit[h][w] as 8 words {t, kind, index, n.x, n.y, n.z, 0, 0}; rgbf float[h][w][3]; var float[h][w] or NULL;
 * out_rgbf / out_rgb may be NULL */
void skdv_denoise(int w, int h, const float *rgbf, const void *hits, const float *var, int iterations, float *out_rgbf, uint8_t *out_rgb)
{
	const size_t n = (size_t) w * h;
	const uint32_t *hw = (const uint32_t *) hits;
	const float *hf = (const float *) hits;
	uint32_t *cls = malloc(n * 4);
	float *a = malloc(n * 16), *b = malloc(n * 16);
	for(size_t i = 0; i < n; i++)
	{
		const int32_t kind = (int32_t) hw[8 * i + 1];
		cls[i] = kind == 1 ? hw[8 * i + 2] : kind == 2 ? MESH : MISS;
	}
	for(int y = 0; y < h; y++)
		for(int x = 0; x < w; x++)
		{
			const size_t i = (size_t) y * w + x;
			a[4 * i] = rgbf[3 * i];
			a[4 * i + 1] = rgbf[3 * i + 1];
			a[4 * i + 2] = rgbf[3 * i + 2];
			a[4 * i + 3] = init_var(w, h, x, y, rgbf, cls, var);
		}
	static const float k[5] = {1.0f / 16, 0.25f, 0.375f, 0.25f, 1.0f / 16};
	for(int it = 0; it < iterations; it++)
	{
		const int s = 1 << it;
		for(int y = 0; y < h; y++)
			for(int x = 0; x < w; x++)
			{
				const size_t i = (size_t) y * w + x;
				const float *cp = a + 4 * i, *np = hf + 8 * i + 3;
				const float tp = hf[8 * i];
				const int miss = cls[i] == MISS;
				const float lp = lum(cp);
				const float V = VAR_SIGMA_L * VAR_SIGMA_L * cp[3] + EPS;
				float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
				for(int dy = -2; dy <= 2; dy++)
					for(int dx = -2; dx <= 2; dx++)
					{
						const int yy = y + s * dy, xx = x + s * dx;
						if(yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
						const size_t j = (size_t) yy * w + xx;
						if(cls[j] != cls[i]) continue;
						const float *cq = a + 4 * j, *nq = hf + 8 * j + 3;
						float wn = 1.0f, wz = 1.0f;
						if(!miss)
						{
							wn = max0(np[0] * nq[0] + np[1] * nq[1] + np[2] * nq[2]);
							for(int q = 0; q < 7; q++) wn = wn * wn;
							if(dx != 0 || dy != 0)
							{
								const int m = abs(dx) > abs(dy) ? abs(dx) : abs(dy);
								const float D = SIGMA_Z * tp * (float) (s * m);
								wz = D / (D + fabsf(tp - hf[8 * j]));
							}
						}
						const float dl = lp - lum(cq);
						const float wl = V / (V + dl * dl);
						const float wt = k[dx + 2] * k[dy + 2] * wn * wz * wl;
						sw += wt;
						sr += wt * cq[0];
						sg += wt * cq[1];
						sb += wt * cq[2];
						sv += wt * wt * cq[3];
					}
				float *o = b + 4 * i;
				if(sw > 0.0f)
				{
					o[0] = sr / sw;
					o[1] = sg / sw;
					o[2] = sb / sw;
					o[3] = sv / (sw * sw);
				}
				else memcpy(o, cp, 16);
			}
		float *t = a;
		a = b;
		b = t;
	}
	for(size_t i = 0; i < n; i++)
		for(int c = 0; c < 3; c++)
		{
			const float v = iterations ? a[4 * i + c] : rgbf[3 * i + c];
			if(out_rgbf) memcpy(out_rgbf + 3 * i + c, &v, 4);
			if(out_rgb) out_rgb[3 * i + c] = (uint8_t) quantise(v);
		}
	free(cls);
	free(a);
	free(b);
}
