// The denoiser (include/skr.h skr_denoise): a spatial a-trous wavelet filter with edge-stopping weights (Dammertz et al.
// 2010) and the luminance-variance guidance of SVGF (Schied et al. 2017) without its temporal part, guided by the first hits of the
// pixel-centre camera rays (skr_hit).  Every weight is binary32 `+ - * / max` in a fixed order (contraction off, divide correctly
// rounded), the taps are summed in row-major order, so tests/denoise_checker.c restates the filter bit for bit.
//
// Kernels, all one lane per pixel in 16x16 workgroups (a wave is a 16x4 block, so the taps of its lanes share cache lines):
//   skr_dn_pack_kernel   guides once: {n, t} as one float4 and the pixel's class as one word; the colour as {r, g, b, l}
//   skr_dn_init_kernel   var = max(0, m2 - m1^2) over the same-class 3x3 window; writes {r, g, b, var}
//   skr_dn_init_var_kernel  skr_denoise_var: var = the caller's per-pixel variance, 3x3 pre-filtered, where it is measured
//   skr_dn_iter_kernel   one a-trous step of size s = 2^i over 5x5 taps; the last one writes the float frame and its bytes
// A tap reads 36 bytes: the {r, g, b, var} float4, the {n, t} float4 and the class.  No atomics, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"
#include "launch.h"
#include "skr.h"

namespace {

constexpr uint32_t DN_MISS = 0xFFFFFFFFu, DN_MESH = 0xFFFFFFFEu; // the classes that are not a sphere index
constexpr int DN_TILE = 16;
constexpr float DN_SIGMA_L2 = SKR_DENOISE_SIGMA_L * SKR_DENOISE_SIGMA_L; // (16: exact)
static_assert(SKR_DENOISE_VAR_SIGMA_L == SKR_DENOISE_SIGMA_L, "skr_denoise_var runs skr_dn_iter_kernel: another sigma needs an instance that takes sigma^2");

// l = 0.2126 r + 0.7152 g + 0.0722 b, left to right
SKR_DEV float dn_max0(float x) { return x > 0.0f ? x : 0.0f; }
// h = k[dx + 2] * k[dy + 2] with k = {1/16, 1/4, 3/8, 1/4, 1/16}: every product is exact, so it folds to a constant
constexpr float dn_k(int i) { return i == 0 || i == 4 ? 1.0f / 16 : i == 1 || i == 3 ? 0.25f : 0.375f; }

SKR_DEV bool dn_pixel(uint32_t w, uint32_t h, uint32_t &x, uint32_t &y)
{
	x = blockIdx.x * DN_TILE + threadIdx.x;
	y = blockIdx.y * DN_TILE + threadIdx.y;
	return x < w && y < h;
}

} // namespace

// the guides and the colour with its luminance
__global__ __launch_bounds__(256) void skr_dn_pack_kernel(const float *__restrict__ rgbf, const float4 *__restrict__ hits, uint32_t w, uint32_t h,
														  float4 *__restrict__ col, float4 *__restrict__ guide, uint32_t *__restrict__ cls)
{
	uint32_t x, y;
	if(!dn_pixel(w, h, x, y)) return;
	const size_t i = (size_t) y * w + x;
	const float4 h0 = hits[2 * i], h1 = hits[2 * i + 1]; // {t, kind, index, n.x} {n.y, n.z, 0, 0}
	const int kind = __float_as_int(h0.y);
	cls[i] = kind == 1 ? (uint32_t) __float_as_int(h0.z) : kind == 2 ? DN_MESH : DN_MISS;
	guide[i] = make_float4(h0.w, h1.x, h1.y, h0.x);
	const float r = rgbf[3 * i], g = rgbf[3 * i + 1], b = rgbf[3 * i + 2];
	col[i] = make_float4(r, g, b, sk_lum(r, g, b));
}

// var_p = max(0, m2 - m1 * m1), m1 and m2 the means of l and l * l over the same-class in-image pixels of the 3x3 window (row-major)
SKR_DEV float dn_window_var(const float4 *col, const uint32_t *cls, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t cp)
{
	float s1 = 0.0f, s2 = 0.0f;
	int n = 0;
#pragma unroll
	for(int dy = -1; dy <= 1; dy++)
	{
		const int yy = (int) y + dy;
#pragma unroll
		for(int dx = -1; dx <= 1; dx++)
		{
			const int xx = (int) x + dx;
			if(yy < 0 || yy >= (int) h || xx < 0 || xx >= (int) w) continue;
			const size_t j = (size_t) yy * w + xx;
			if(cls[j] != cp) continue;
			const float l = col[j].w;
			s1 += l;
			s2 += l * l;
			n++;
		}
	}
	const float m1 = s1 / (float) n, m2 = s2 / (float) n; // (n >= 1: the pixel itself)
	return dn_max0(m2 - m1 * m1);
}

__global__ __launch_bounds__(256) void skr_dn_init_kernel(const float4 *__restrict__ col, const uint32_t *__restrict__ cls, uint32_t w, uint32_t h,
														  float4 *__restrict__ out)
{
	uint32_t x, y;
	if(!dn_pixel(w, h, x, y)) return;
	const size_t i = (size_t) y * w + x;
	const float v = dn_window_var(col, cls, w, h, x, y, cls[i]);
	const float4 c = col[i];
	out[i] = make_float4(c.x, c.y, c.z, v);
}

// skr_denoise_var's init.  A pixel whose var[p] >= 0 (measured: false for NaN and negatives) takes (sum g var[q]) / (sum g) over the
// in-image same-class measured q of the 3x3 window, row-major, g = {1, 2, 1; 2, 4, 2; 1, 2, 1} / 16 (SVGF's variance pre-filter, once);
// any other pixel takes skr_dn_init_kernel's value.
__global__ __launch_bounds__(256) void skr_dn_init_var_kernel(const float4 *__restrict__ col, const uint32_t *__restrict__ cls, const float *__restrict__ var,
															  uint32_t w, uint32_t h, float4 *__restrict__ out)
{
	uint32_t x, y;
	if(!dn_pixel(w, h, x, y)) return;
	const size_t i = (size_t) y * w + x;
	const uint32_t cp = cls[i];
	float v;
	if(var[i] >= 0.0f)
	{
		float sv = 0.0f, sg = 0.0f;
#pragma unroll
		for(int dy = -1; dy <= 1; dy++)
		{
			const int yy = (int) y + dy;
#pragma unroll
			for(int dx = -1; dx <= 1; dx++)
			{
				const int xx = (int) x + dx;
				if(yy < 0 || yy >= (int) h || xx < 0 || xx >= (int) w) continue;
				const size_t j = (size_t) yy * w + xx;
				if(cls[j] != cp) continue;
				const float vq = var[j];
				if(!(vq >= 0.0f)) continue;
				const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f); // (exact: it folds to a constant)
				sv += g * vq;
				sg += g;
			}
		}
		v = sv / sg; // (sg >= 1/4: the pixel itself)
	}
	else v = dn_window_var(col, cls, w, h, x, y, cp);
	const float4 c = col[i];
	out[i] = make_float4(c.x, c.y, c.z, v);
}

// One a-trous step of size s.  LAST: the float frame and its bytes (either may be null) instead of the next {r, g, b, var} image.
template <bool LAST>
__global__ __launch_bounds__(256) void skr_dn_iter_kernel(const float4 *__restrict__ in, const float4 *__restrict__ guide, const uint32_t *__restrict__ cls,
														  uint32_t w, uint32_t h, int s, float4 *__restrict__ out, float *__restrict__ out_rgbf,
														  uint8_t *__restrict__ out_rgb)
{
	uint32_t x, y;
	if(!dn_pixel(w, h, x, y)) return;
	const size_t i = (size_t) y * w + x;
	const uint32_t cp = cls[i];
	const float4 gp = guide[i], cpx = in[i];
	const bool miss = cp == DN_MISS;
	const float lp = sk_lum(cpx.x, cpx.y, cpx.z);
	const float V = DN_SIGMA_L2 * cpx.w + SKR_DENOISE_EPS;
	const float zt = SKR_DENOISE_SIGMA_Z * gp.w;
	const float D1 = zt * (float) s, D2 = zt * (float) (2 * s); // D = sigma_z * t_p * (s * max(|dx|, |dy|))
	float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
	for(int dy = -2; dy <= 2; dy++)
	{
		const int yy = (int) y + s * dy;
		const bool row_in = yy >= 0 && yy < (int) h;
#pragma unroll
		for(int dx = -2; dx <= 2; dx++)
		{
			const int xx = (int) x + s * dx;
			if(!row_in || xx < 0 || xx >= (int) w) continue;
			const size_t j = (size_t) yy * w + xx;
			if(cls[j] != cp) continue;
			const float4 q = in[j];
			float wn = 1.0f, wz = 1.0f;
			if(!miss)
			{
				const float4 gq = guide[j];
				wn = dn_max0(gp.x * gq.x + gp.y * gq.y + gp.z * gq.z);
#pragma unroll
				for(int k = 0; k < 7; k++) wn = wn * wn; // ^128
				if(dx != 0 || dy != 0)
				{
					const float D = (dx == 2 || dx == -2 || dy == 2 || dy == -2) ? D2 : D1;
					wz = D / (D + fabsf(gp.w - gq.w));
				}
			}
			const float dl = lp - sk_lum(q.x, q.y, q.z);
			const float wl = V / (V + dl * dl);
			const float hk = dn_k(dx + 2) * dn_k(dy + 2);
			const float wt = hk * wn * wz * wl;
			sw += wt;
			sr += wt * q.x;
			sg += wt * q.y;
			sb += wt * q.z;
			sv += wt * wt * q.w;
		}
	}
	float4 o = cpx; // (no weight: a non-finite guide or colour; the pixel stays)
	if(sw > 0.0f) o = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
	if constexpr(LAST)
	{
		if(out_rgbf)
		{
			out_rgbf[3 * i] = o.x;
			out_rgbf[3 * i + 1] = o.y;
			out_rgbf[3 * i + 2] = o.z;
		}
		if(out_rgb)
		{
			out_rgb[3 * i] = (uint8_t) quantise(o.x);
			out_rgb[3 * i + 1] = (uint8_t) quantise(o.y);
			out_rgb[3 * i + 2] = (uint8_t) quantise(o.z);
		}
	}
	else out[i] = o;
}

// iterations = 0: the input itself, and its bytes
__global__ __launch_bounds__(256) void skr_dn_copy_kernel(const float *__restrict__ rgbf, uint32_t w, uint32_t h, float *__restrict__ out_rgbf, uint8_t *__restrict__ out_rgb)
{
	uint32_t x, y;
	if(!dn_pixel(w, h, x, y)) return;
	const size_t i = (size_t) y * w + x;
	for(int c = 0; c < 3; c++)
	{
		const float v = rgbf[3 * i + c];
		if(out_rgbf) reinterpret_cast<uint32_t *>(out_rgbf)[3 * i + c] = __float_as_uint(v);
		if(out_rgb) out_rgb[3 * i + c] = (uint8_t) quantise(v);
	}
}

hipError_t skr_launch_denoise(const DenoiseScratch &b, uint32_t w, uint32_t h, const float *rgbf, const float4 *hits, const float *var, int iterations,
							  float *out_rgbf, uint8_t *out_rgb, hipStream_t stream)
{
	const dim3 grid((w + DN_TILE - 1) / DN_TILE, (h + DN_TILE - 1) / DN_TILE), block(DN_TILE, DN_TILE);
	if(iterations == 0)
	{
		hipLaunchKernelGGL(skr_dn_copy_kernel, grid, block, 0, stream, rgbf, w, h, out_rgbf, out_rgb);
		return hipGetLastError();
	}
	hipLaunchKernelGGL(skr_dn_pack_kernel, grid, block, 0, stream, rgbf, hits, w, h, b.img[1], b.guide, b.cls);
	if(var) hipLaunchKernelGGL(skr_dn_init_var_kernel, grid, block, 0, stream, b.img[1], b.cls, var, w, h, b.img[0]);
	else hipLaunchKernelGGL(skr_dn_init_kernel, grid, block, 0, stream, b.img[1], b.cls, w, h, b.img[0]);
	for(int it = 0; it < iterations; it++)
	{
		const float4 *src = b.img[it & 1];
		float4 *dst = b.img[(it + 1) & 1];
		if(it + 1 < iterations) hipLaunchKernelGGL(skr_dn_iter_kernel<false>, grid, block, 0, stream, src, b.guide, b.cls, w, h, 1 << it, dst, nullptr, nullptr);
		else hipLaunchKernelGGL(skr_dn_iter_kernel<true>, grid, block, 0, stream, src, b.guide, b.cls, w, h, 1 << it, nullptr, out_rgbf, out_rgb);
	}
	return hipGetLastError();
}
